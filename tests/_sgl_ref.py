"""Test-only yardsticks for gathered values (tests/test_sgl_host.py, tests/test_gpu_sgl.py).

gathered_crcs: the oracle (oracle/liboracle_crc.so) on the concatenated bytes,
built with numpy on the host -- never a product function.

shift / combine_value: a pure-Python restatement of the CRC's zero-byte
shift for part lengths too large to materialise, built from the oracle's
table alone: the 32 columns of the one-zero-byte step, squared 47 times,
one matrix per set bit of the distance, values in Horner form.
"""
from __future__ import annotations

import json
import os

import numpy as np

import _oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))

_mats = None


def _apply(cols, c: int) -> int:
    r = 0
    i = 0
    while c:
        if c & 1:
            r ^= cols[i]
        c >>= 1
        i += 1
    return r


def mats():
    """mats()[b] = the 32 columns of Z_(2^b), b < 48."""
    global _mats
    if _mats is None:
        t = [int(x) for x in O.table()]
        one = [t[(1 << i) & 0xFF] ^ ((1 << i) >> 8) for i in range(32)]
        m = [one]
        for _ in range(47):
            prev = m[-1]
            m.append([_apply(prev, col) for col in prev])
        _mats = m
    return _mats


def shift(c: int, d: int) -> int:
    """state c advanced over d zero bytes (d < 2^48)"""
    assert 0 <= d < 1 << 48
    m = mats()
    b = 0
    while d:
        if d & 1:
            c = _apply(m[b], c)
        d >>= 1
        b += 1
    return c


def combine_value(parts) -> int:
    """CRC of the concatenation from (crc, length) per part: acc = shift(acc, len_j) ^ crc_j"""
    acc = 0
    for crc, ln in parts:
        acc = shift(acc, int(ln)) ^ int(crc)
    return acc


def pack(values):
    """lists of (offset, length) per value -> (offsets u64, lengths u32, first u64[n + 1]); the tests' own packer"""
    offs = np.array([o for v in values for o, _ in v], dtype=np.uint64)
    lens = np.array([n for v in values for _, n in v], dtype=np.uint32)
    first = np.zeros(len(values) + 1, dtype=np.uint64)
    if values:
        first[1:] = np.cumsum([len(v) for v in values])
    return offs, lens, first


def gathered_crcs_arrays(region: np.ndarray, offs, lens, first) -> np.ndarray:
    """oracle CRC of each value's concatenated bytes (the gather is numpy's, on the host)"""
    region = np.ascontiguousarray(region).view(np.uint8).reshape(-1)
    offs = np.asarray(offs, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    first = np.asarray(first, dtype=np.int64)
    assert np.all(np.diff(first) >= 0) and first[0] >= 0 and first[-1] <= offs.size
    assert offs.size == 0 or (offs.min() >= 0 and int((offs + lens).max()) <= region.size)
    start = np.zeros(offs.size + 1, dtype=np.int64)  # where each part starts in the gathered buffer
    np.cumsum(lens, out=start[1:])
    total = int(start[-1])
    idx = np.arange(total, dtype=np.int64) + np.repeat(offs - start[:-1], lens)
    buf = region[idx] if total else np.zeros(1, dtype=np.uint8)
    # parts outside [first[0], first[n]) are gathered too but belong to no value
    voff = start[first[:-1]]
    vlen = start[first[1:]] - voff
    assert vlen.size == 0 or int(vlen.max()) < 2**32
    return O.crc32_ranges(buf, voff.astype(np.uint64), vlen.astype(np.uint32))


def gathered_crcs(region: np.ndarray, values) -> np.ndarray:
    """oracle CRC of each value's concatenated bytes; values: lists of (offset, length)"""
    return gathered_crcs_arrays(region, *pack(values))


def sgl_golden() -> dict:
    with open(os.path.join(HERE, "golden", "sgl_golden.json")) as f:
        return json.load(f)
