"""Gathered values, host side: pack_sgl, the tests' own yardsticks, and the
committed fixture tests/golden/sgl_golden.json against the oracle.  No GPU.
"""
import numpy as np
import pytest

import _oracle as O
import _sgl_ref as R

LENGTHS = [0, 1, 3, 15, 16, 17, 4095, 4096, 4097, 65541]


def test_pack_sgl_round_trip():
    from priskv_amd import pack_sgl
    values = [[(5, 10), (0, 0), (2**40, 2**32 - 1)], [], [(7, 1)], [(0, 0)]]
    offs, lens, first = pack_sgl(values)
    assert offs.dtype == np.uint64 and lens.dtype == np.uint32 and first.dtype == np.uint64
    assert first.tolist() == [0, 3, 3, 4, 5]
    back = [[(int(offs[j]), int(lens[j])) for j in range(int(first[v]), int(first[v + 1]))]
            for v in range(len(values))]
    assert back == values
    offs, lens, first = pack_sgl([])
    assert offs.size == 0 and lens.size == 0 and first.tolist() == [0]
    assert offs.dtype == np.uint64 and lens.dtype == np.uint32 and first.dtype == np.uint64
    offs, lens, first = pack_sgl([[], []])
    assert offs.size == 0 and first.tolist() == [0, 0, 0]


@pytest.mark.parametrize("bad", [[[(-1, 4)]], [[(0, 2**32)]], [[(3, 4)], [(0, -1)]], [[(2**64, 1)]]])
def test_pack_sgl_errors(bad):
    from priskv_amd import pack_sgl
    with pytest.raises(ValueError):
        pack_sgl(bad)


def test_pack_sgl_exported():
    import priskv_amd
    assert "pack_sgl" in priskv_amd.__all__ and priskv_amd.pack_sgl is priskv_amd.crc.pack_sgl


def test_restatement_against_oracle_and_zlib():
    """The Python shift / Horner restatement is exact against _oracle.crc32
    and zlib's identity on random gathers of 0 to 200 parts."""
    seed = 0x51A7E
    rng = np.random.default_rng(seed)
    region = O.fill_splitmix(1 << 17, seed, 0)
    for it in range(120):
        count = int(rng.integers(0, 201)) if it % 4 == 0 else int(rng.integers(0, 12))
        parts = []
        for _ in range(count):
            ln = int(rng.choice(LENGTHS))
            parts.append((int(rng.integers(0, region.size - ln + 1)), ln))
        data = b"".join(region[o:o + n].tobytes() for o, n in parts)
        want = O.crc32(np.frombuffer(data, dtype=np.uint8))
        assert want == O.zlib_identity(data), f"seed {seed:#x} iteration {it}"
        got = R.combine_value([(O.crc32(region[o:o + n]), n) for o, n in parts])
        assert got == want, f"seed {seed:#x} iteration {it}: {got:#x} != {want:#x}"
        assert int(R.gathered_crcs(region, [parts])[0]) == want, f"seed {seed:#x} iteration {it}"


def test_restatement_zero_bytes_and_composition():
    c = O.crc32(b"123456789")
    assert R.shift(c, 1000) == O.crc32(b"123456789" + b"\0" * 1000) == O.zlib_identity(b"123456789" + b"\0" * 1000)
    assert R.shift(c, 0) == c and R.shift(0, 12345) == 0
    big = 0xFFFFFFFF
    assert R.shift(R.shift(c, big), big) == R.shift(c, 2 * big)
    assert R.shift(R.shift(c, (1 << 47) - 5), 6) == R.shift(c, (1 << 47) + 1)


def test_restatement_against_product_host_helpers():
    """priskv_crc32_shift / _combine (the host helpers the device table is
    built from) agree with the restatement, 2^47 + 1 included."""
    from priskv_amd import crc32_combine, crc32_shift
    for c, d in ((0x80000000, 1), (0xDEADBEEF, 0xFFFFFFFF), (0x12345678, (1 << 47) + 1), (1, 3 * 0xFFFFFFFF)):
        assert crc32_shift(c, d) == R.shift(c, d), (hex(c), d)
    assert crc32_combine(0xCAFEF00D, 0x0BADF00D, 4097) == R.combine_value([(0xCAFEF00D, 5), (0x0BADF00D, 4097)])


def test_golden_fixture_against_oracle():
    g = R.sgl_golden()
    cases = g["cases"]
    assert 30 <= len(cases) <= 60
    regions = {}
    counts = set()
    for i, c in enumerate(cases):
        key = (c["seed"], c["region_bytes"])
        if key not in regions:
            regions[key] = O.fill_splitmix(c["region_bytes"], c["seed"], 0)
        region = regions[key]
        data = b"".join(region[o:o + n].tobytes() for o, n in c["parts"])
        assert f"{O.crc32(np.frombuffer(data, dtype=np.uint8)):08x}" == c["crc"], f"case {i}"
        assert f"{O.zlib_identity(data):08x}" == c["crc"], f"case {i}"
        counts.add(len(c["parts"]))
        if O.ref_lib("O2") is not None:
            assert f"{O.ref_crc32(data):08x}" == c["crc"], f"case {i}"
    assert {0, 1, 2, 7, 8, 9} <= counts
