#!/usr/bin/env python3
"""Generate tests/golden/sgl_golden.json from the REFERENCE itself.

A gathered value is the concatenation of (offset, length) segments of a
region (a priskv_sgl[] of a GET or SET, client/priskv.h:74-78).  Each case is
a splitmix64 region (seed, size), one value's segment list and the
reference's priskv_crc32 (server/crc.c:90-109, compiled unmodified into
oracle/_ref by oracle/Makefile) of the concatenated bytes, cross-checked
against zlib's identity before it is written.  Regions are stored as
generator specs, so the fixture stays small.

Run where the reference build exists:
    make -C oracle && python tests/golden/gen_sgl_golden.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _oracle as O  # noqa: E402

LENGTHS = [0, 1, 3, 15, 16, 17, 4095, 4096, 4097, 65541]
REGIONS = [(0x5EED5EED, 1 << 17), (0xC0FFEE, (1 << 17) + 13), (0x1234567, 70000), (0xABCDEF01, 1 << 18)]
PART_COUNTS = [0, 1, 1, 2, 3, 7, 8, 9, 17, 40]


def ref(data: bytes) -> int:
    v = O.ref_crc32(data, "O2")
    z = O.zlib_identity(data)
    if v != z:
        raise SystemExit(f"reference/zlib disagree on len={len(data)}: {v:#x} vs {z:#x}")
    return v


def main() -> None:
    if O.ref_lib("O2") is None:
        raise SystemExit("oracle/_ref/libpriskv_ref_crc_O2.so missing: run `make -C oracle`")
    rng = np.random.default_rng(20261019)
    cases = []
    for seed, size in REGIONS:
        region = O.fill_splitmix(size, seed, 0)
        for k, count in enumerate(PART_COUNTS):
            parts = []
            for j in range(count):
                ln = int(rng.choice(LENGTHS))
                if (k % 3 == 0 and j in (0, count - 1)) or k == 2:
                    ln = 0  # zero-length parts first and last, and as a value's only part
                ln = min(ln, size)
                off = int(rng.integers(0, size - ln + 1))
                parts.append([off, ln])
            if count >= 7:
                parts[3] = list(parts[1])  # a repeated segment
                parts[4] = [parts[1][0] + parts[1][1] // 2, min(parts[1][1], size - parts[1][0] - parts[1][1] // 2)]
            data = b"".join(region[o:o + n].tobytes() for o, n in parts)
            cases.append({"seed": seed, "region_bytes": size, "parts": parts, "crc": f"{ref(data):08x}"})
    g = {
        "about": "gathered values: priskv_crc32 (server/crc.c:90-109) of the concatenation of (offset, length) "
                 "segments of a splitmix64 region, produced by the reference compiled unmodified (oracle/_ref, "
                 "-O2) and cross-checked against zlib.crc32(b, 0xFFFFFFFF) ^ 0xFFFFFFFF",
        "generator": "tests/golden/gen_sgl_golden.py",
        "pattern_spec": "64-bit LE word i of a region = mix64(seed + (i + 1) * 0x9E3779B97F4A7C15), "
                        "mix64 = splitmix64 finaliser",
        "cases": cases,
    }
    out = os.path.join(HERE, "sgl_golden.json")
    with open(out, "w") as f:
        json.dump(g, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {out}: {len(cases)} cases")


if __name__ == "__main__":
    main()
