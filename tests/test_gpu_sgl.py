"""Gathered values on the GPU: combine_dev, sgl_dev, sgl_verify_dev.

The expected CRC of a gathered value is the oracle's on the concatenated
bytes, gathered with numpy on the host (_sgl_ref.gathered_crcs*); for part
lengths too large to materialise it is _sgl_ref's pure-Python restatement
(checked against the oracle and zlib in tests/test_sgl_host.py).  Every
output is sentinel-filled with one extra entry past n that must stay
untouched.  Seeds are fixed and named in every assert message.
"""
import errno
import threading

import numpy as np
import pytest

import _oracle as O
import _sgl_ref as R

pytestmark = pytest.mark.gpu

MIB = 1 << 20
LENGTHS = [0, 1, 3, 15, 16, 17, 4095, 4096, 4097, 65541]
SMALL_LENGTHS = [0, 1, 3, 15, 16, 17]
COUNTS = [0, 1, 2, 7, 8, 9, 63, 64, 65, 200]
SENT = 0x5A5A5A5A
REGION_SEED = 0x56_17_0001
REGION_BYTES = 4 * MIB
FULL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    from priskv_amd import CrcContext
    c = CrcContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def region(torch_cuda, ctx):
    """(device tensor, host copy) of one 4 MiB splitmix region shared by the tests; never written"""
    torch = torch_cuda
    t = torch.empty(REGION_BYTES, dtype=torch.uint8, device="cuda")
    ctx.fill_splitmix(t, REGION_SEED, 0)
    torch.cuda.synchronize()
    host = t.cpu().numpy()
    assert np.array_equal(host, O.fill_splitmix(REGION_BYTES, REGION_SEED, 0))
    return t, host


def _dev(torch, offs, lens, first):
    return (torch.from_numpy(np.ascontiguousarray(offs, dtype=np.uint64).view(np.int64)).cuda(),
            torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint32).view(np.int32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(first, dtype=np.uint64).view(np.int64)).cuda())


def _sentinel(torch, n):
    return torch.full((n + 1,), SENT, dtype=torch.int32, device="cuda")


def _result(out, n, what):
    from priskv_amd import as_u32
    got = as_u32(out)
    assert got[n] == SENT, f"{what}: the entry past n was written"
    return got[:n]


def _sgl(torch, ctx, t, offs, lens, first, what, **kw):
    d_o, d_l, d_f = _dev(torch, offs, lens, first)
    n = len(first) - 1
    out = _sentinel(torch, n)
    ctx.sgl_dev(t, d_o, d_l, d_f, out=out, **kw)
    torch.cuda.synchronize()
    return _result(out, n, what)


def _check_sgl(torch, ctx, region, offs, lens, first, what, **kw):
    t, host = region
    got = _sgl(torch, ctx, t, offs, lens, first, what, **kw)
    want = R.gathered_crcs_arrays(host, offs, lens, first)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {want.size} values differ, first {bad[0]}: "
                           f"{got[bad[0]]:#010x} != {want[bad[0]]:#010x}")
    return got


def _parts(rng, nparts, lengths, size, k0=0):
    """nparts random parts; offset k has alignment (k0 + k) mod 16, so every alignment occurs"""
    lens = rng.choice(np.array(lengths, dtype=np.int64), size=nparts)
    slots = (size - lens - 16) // 16
    offs = (rng.integers(0, 1 << 62, size=nparts) % slots) * 16 + (k0 + np.arange(nparts)) % 16
    return offs.astype(np.uint64), lens.astype(np.uint32)


def _first(counts):
    first = np.zeros(len(counts) + 1, dtype=np.uint64)
    first[1:] = np.cumsum(counts)
    return first


def _lanes_per_value(nparts, n):
    """the G the library picks: the power of two at or above the mean part count, at most 64"""
    mean = -(-nparts // n)
    g = 1
    while g < mean and g < 64:
        g *= 2
    return g


def _grid_stride(torch, nparts, n):
    """values one pass of crc_combine_parts_kernel's whole grid takes: kCombWgPerCu (4)
    workgroups per CU x kCombThreads (256) / G values per workgroup"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * 4 * 256 // _lanes_per_value(nparts, n)


# ---------------------------------------------------------------- part counts
def test_part_counts_mixed(torch_cuda, ctx, region):
    seed = 0xA001
    rng = np.random.default_rng(seed)
    counts = np.array(COUNTS * 3)
    rng.shuffle(counts)
    offs, lens = _parts(rng, int(counts.sum()), LENGTHS, REGION_BYTES)
    _check_sgl(torch_cuda, ctx, region, offs, lens, _first(counts), f"mixed part counts, seed {seed:#x}")


def test_long_values_among_short(torch_cuda, ctx, region):
    """values far above the mean part count (the whole-wave path) beside values of 0-9 parts"""
    seed = 0xA002
    rng = np.random.default_rng(seed)
    counts = np.array([1] * 300 + [0] * 20 + [200, 65, 64, 63, 33, 32, 9, 200, 200, 130])
    rng.shuffle(counts)
    counts[:3] = (200, 1, 65)  # two long values in the first wave
    assert _lanes_per_value(int(counts.sum()), counts.size) == 8  # more than 64 parts: the whole wave
    offs, lens = _parts(rng, int(counts.sum()), LENGTHS, REGION_BYTES)
    _check_sgl(torch_cuda, ctx, region, offs, lens, _first(counts), f"long among short, seed {seed:#x}")


@pytest.mark.parametrize("count", COUNTS)
def test_part_count_alone(torch_cuda, ctx, region, count):
    """each part count alone, n = 1, 3, a workgroup's worth, and PAST_STRIDE = one grid
    stride of the combine kernel plus one (so some workgroup takes a second pass)"""
    torch = torch_cuda
    seed = 0xB000 + count
    rng = np.random.default_rng(seed)
    past_stride = _grid_stride(torch, count, 1) + 1
    for n in (1, 3, 257, past_stride):
        lengths = LENGTHS if n * count <= 2000 else SMALL_LENGTHS
        offs, lens = _parts(rng, n * count, lengths, REGION_BYTES)
        got = _check_sgl(torch, ctx, region, offs, lens, _first([count] * n),
                         f"{count} parts x {n} values (PAST_STRIDE {past_stride}), seed {seed:#x}")
        if count == 0:
            assert not got.any()


# ---------------------------------------------------------------- segment lengths
def test_lengths_at_every_alignment(torch_cuda, ctx, region):
    seed = 0xC001
    rng = np.random.default_rng(seed)
    offs, lens, counts = [], [], []
    for ln in LENGTHS:
        for al in range(16):
            # this length at this alignment as the first, a middle and the last part of a value
            for pos in range(3):
                o, l = _parts(rng, 3, LENGTHS, REGION_BYTES, k0=int(rng.integers(0, 16)))
                l[pos] = ln
                o[pos] = (int(rng.integers(0, (REGION_BYTES - 70000) // 16)) * 16) + al
                offs.append(o)
                lens.append(l)
                counts.append(3)
            offs.append(np.array([int(rng.integers(0, 1000)) * 16 + al], dtype=np.uint64))
            lens.append(np.array([ln], dtype=np.uint32))
            counts.append(1)
    offs, lens = np.concatenate(offs), np.concatenate(lens)
    _check_sgl(torch_cuda, ctx, region, offs, lens, _first(counts), f"lengths x alignments, seed {seed:#x}")


def test_zero_length_parts(torch_cuda, ctx, region):
    values = [[(5, 0)], [(5, 0), (100, 17)], [(100, 17), (7, 0)], [(100, 17), (9, 0), (4000, 4097)],
              [(1, 0), (2, 0), (3, 0)], [], [(0, 0), (33, 1), (0, 0), (34, 1), (0, 0)], [(REGION_BYTES, 0)]]
    offs, lens, first = R.pack(values)
    got = _check_sgl(torch_cuda, ctx, region, offs, lens, first, "zero-length parts")
    assert got[0] == 0 and got[4] == 0 and got[5] == 0 and got[7] == 0


# ---------------------------------------------------------------- dispatch
def test_one_value_of_one_part(torch_cuda, ctx, region):
    torch = torch_cuda
    from priskv_amd import as_u32
    t, host = region
    offs, lens, first = R.pack([[(12345, 65541)]])
    got = _check_sgl(torch, ctx, region, offs, lens, first, "one value of one part")
    d_o, d_l, _ = _dev(torch, offs, lens, first)
    r = as_u32(ctx.ranges_dev(t, d_o, d_l))
    assert got[0] == r[0] == O.crc32(host[12345:12345 + 65541])


def test_max_seg_len_is_a_hint(torch_cuda, ctx, region):
    seed = 0xD001
    for n, lengths in ((5, LENGTHS), (3000, SMALL_LENGTHS + [4097])):
        rng = np.random.default_rng(seed)
        counts = rng.integers(0, 9, size=n)
        offs, lens = _parts(rng, int(counts.sum()), lengths, REGION_BYTES)
        first = _first(counts)
        what = f"max_seg_len, n {n}, seed {seed:#x}"
        a = _check_sgl(torch_cuda, ctx, region, offs, lens, first, what + " absent")
        b = _check_sgl(torch_cuda, ctx, region, offs, lens, first, what + " tight", max_seg_len=int(lens.max()))
        c = _check_sgl(torch_cuda, ctx, region, offs, lens, first, what + " too small", max_seg_len=16)
        d = _check_sgl(torch_cuda, ctx, region, offs, lens, first, what + " huge", max_seg_len=1 << 40)
        assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d)


def test_few_large_segments(torch_cuda, ctx):
    """4 values x 3 segments x 3 MiB + 5 B: the segments take the few-extents (fused) path.
    The one case with a larger region (16 MiB)."""
    torch = torch_cuda
    seed = 0xD002
    rng = np.random.default_rng(seed)
    size, ln = 16 * MIB, 3 * MIB + 5
    t = torch.empty(size, dtype=torch.uint8, device="cuda")
    ctx.fill_splitmix(t, seed, 0)
    host = O.fill_splitmix(size, seed, 0)
    values = [[(int(rng.integers(0, size - ln)), ln) for _ in range(3)] for _ in range(4)]
    offs, lens, first = R.pack(values)
    got = _sgl(torch, ctx, t, offs, lens, first, "few large segments")
    buf = np.concatenate([host[o:o + n] for v in values for o, n in v])
    want = O.crc32_ranges(buf, np.arange(4, dtype=np.uint64) * (3 * ln), np.full(4, 3 * ln, dtype=np.uint32))
    assert np.array_equal(got, want), f"few large segments, seed {seed:#x}: {got} != {want}"
    assert np.array_equal(_sgl(torch, ctx, t, offs, lens, first, "few large, bounded", max_seg_len=ln), want)


def test_many_small_segments(torch_cuda, ctx, region):
    """70 000 segments of 64 to 300 B in values of 7: the many-extents path"""
    seed = 0xD003
    rng = np.random.default_rng(seed)
    nseg = 70000
    lens = rng.integers(64, 301, size=nseg).astype(np.uint32)
    offs = rng.integers(0, REGION_BYTES - 300, size=nseg).astype(np.uint64)
    _check_sgl(torch_cuda, ctx, region, offs, lens, _first([7] * (nseg // 7)), f"many small segments, seed {seed:#x}")


# ---------------------------------------------------------------- sharing and allocations
def test_shared_repeated_overlapping_segments(torch_cuda, ctx, region):
    a, b, c = (1000, 4097), (70001, 65541), (3000, 4096)  # c overlaps a
    values = [[a, b], [b, a], [a, a], [a, c, a], [c, (3001, 4095), (2999, 4097)], [b, b, b], [a]]
    offs, lens, first = R.pack(values)
    got = _check_sgl(torch_cuda, ctx, region, offs, lens, first, "shared / repeated / overlapping")
    assert got[0] != got[1]


def test_segments_in_two_allocations(torch_cuda, ctx):
    """segments in two separate torch allocations, addressed from the lower one's base"""
    torch = torch_cuda
    seed = 0xE001
    x = torch.empty(3 * MIB, dtype=torch.uint8, device="cuda")
    y = torch.empty(3 * MIB, dtype=torch.uint8, device="cuda")
    ctx.fill_splitmix(x, seed, 0)
    ctx.fill_splitmix(y, seed + 1, 0)
    torch.cuda.synchronize()
    lo, hi = (x, y) if x.data_ptr() < y.data_ptr() else (y, x)
    delta = hi.data_ptr() - lo.data_ptr()
    assert delta >= lo.numel()
    hl, hh = lo.cpu().numpy(), hi.cpu().numpy()
    # (allocation, offset in it, length)
    values = [[(0, 17, 4097), (1, 33, 4095)], [(1, 0, 65541), (0, 3 * MIB - 16, 16), (1, 3 * MIB - 1, 1)],
              [(1, 5, 3)], [(0, 5, 3)]]
    offs, lens, first = R.pack([[(o + (delta if w else 0), n) for w, o, n in v] for v in values])
    got = _sgl(torch, ctx, lo, offs, lens, first, "two allocations")
    want = [O.crc32(np.concatenate([(hh if w else hl)[o:o + n] for w, o, n in v])) for v in values]
    assert got.tolist() == want, f"two allocations (delta {delta}), seed {seed:#x}"


def test_bad_value_first_is_clamped(torch_cuda, ctx, region):
    """A table that runs backwards or past nparts gives wrong CRCs for those values only:
    every output is written, good values stay exact, reads stay inside the part arrays."""
    seed = 0xE002
    rng = np.random.default_rng(seed)
    offs, lens = _parts(rng, 12, LENGTHS, REGION_BYTES)
    t, host = region
    first = np.array([0, 5, 3, 3, 1 << 62, 12, 12], dtype=np.uint64)
    got = _sgl(torch_cuda, ctx, t, offs, lens, first, "bad value_first")
    assert got[0] == R.gathered_crcs_arrays(host, offs, lens, [0, 5])[0]
    assert got[1] == 0 and got[2] == 0 and got[4] == 0 and got[5] == 0  # backwards / past the end: empty
    assert got[3] == R.gathered_crcs_arrays(host, offs, lens, [3, 12])[0]  # 3 .. min(2^62, nparts)


# ---------------------------------------------------------------- combine_dev alone
def _combine(torch, ctx, crcs, lens, first, what):
    d_c = torch.from_numpy(np.ascontiguousarray(crcs, dtype=np.uint32).view(np.int32)).cuda()
    _, d_l, d_f = _dev(torch, np.zeros(0), lens, first)
    n = len(first) - 1
    out = _sentinel(torch, n)
    ctx.combine_dev(d_c, d_l, d_f, out=out)
    torch.cuda.synchronize()
    return _result(out, n, what)


def test_combine_page_lists(torch_cuda, ctx, region):
    """one CRC per 4 KiB page (blocks_dev, once), then value CRCs of page lists without the bytes"""
    torch = torch_cuda
    from priskv_amd import as_u32
    seed = 0xF001
    t, host = region
    page = 4096
    npages = REGION_BYTES // page
    page_crcs = as_u32(ctx.blocks_dev(t, page))
    rng = np.random.default_rng(seed)
    lists = [rng.integers(0, npages, size=int(c)) for c in rng.choice(COUNTS, size=40)]
    perm = rng.permutation(npages)[:8]
    lists += [perm, perm[::-1], np.roll(perm, 1), perm[:1], np.arange(npages)]
    idx = np.concatenate(lists).astype(np.int64)
    first = _first([len(x) for x in lists])
    lens = np.full(idx.size, page, dtype=np.uint32)
    got = _combine(torch, ctx, page_crcs[idx], lens, first, "page lists")
    want = R.gathered_crcs_arrays(host, idx * page, lens, first)
    assert np.array_equal(got, want), f"page lists, seed {seed:#x}: values {np.nonzero(got != want)[0][:8]} differ"
    assert len({int(got[40]), int(got[41]), int(got[42])}) == 3, "permutations of the same pages must differ"
    assert got[-1] == O.crc32(host)


def test_combine_huge_lengths(torch_cuda, ctx):
    """lengths that cannot be materialised, against the Python restatement"""
    torch = torch_cuda
    a, b, c, m = 0xDEADBEEF, 0x12345678, 0x0BADF00D, 0xCAFEF00D
    # value 0: three parts of 0xFFFFFFFF bytes.  value 1: 2^47 + 1 bytes as 32768 parts of
    # 0xFFFFFFFF and a remainder of 32769 (CRC 0 where not named: the sums are what is
    # tested); values 2..: one part each, so that the mean is small and value 1 goes to
    # its whole wave.  Second call: value 1 alone (64 lanes per value).
    k = 32768
    crcs1 = np.zeros(k + 1, dtype=np.uint32)
    crcs1[0], crcs1[12345], crcs1[k] = a, m, c
    lens1 = np.full(k + 1, FULL, dtype=np.uint32)
    lens1[k] = 32769
    assert int(lens1.astype(np.uint64).sum()) == (1 << 47) + 1
    want1 = R.combine_value([(a, FULL), (0, 12344 * FULL), (m, FULL), (0, (k - 12346) * FULL), (c, 32769)])
    want0 = R.combine_value([(a, FULL), (b, FULL), (c, FULL)])
    nsmall = 40000
    crcs = np.concatenate([[a, b, c], crcs1, np.arange(1, nsmall + 1)]).astype(np.uint32)
    lens = np.concatenate([[FULL] * 3, lens1, np.full(nsmall, 5)]).astype(np.uint32)
    first = _first([3, k + 1] + [1] * nsmall)
    assert _lanes_per_value(crcs.size, first.size - 1) == 2
    got = _combine(torch, ctx, crcs, lens, first, "huge lengths")
    assert got[0] == want0, f"3 x 0xFFFFFFFF: {got[0]:#x} != {want0:#x}"
    assert got[1] == want1, f"2^47 + 1 bytes (whole-wave path): {got[1]:#x} != {want1:#x}"
    assert np.array_equal(got[2:], np.arange(1, nsmall + 1, dtype=np.uint32))
    alone = _combine(torch, ctx, crcs1, lens1, _first([k + 1]), "2^47 + 1 alone")
    assert alone[0] == want1, f"2^47 + 1 bytes alone: {alone[0]:#x} != {want1:#x}"


# ---------------------------------------------------------------- verify
def _status(torch, ctx, t, offs, lens, first, expected, **kw):
    d_o, d_l, d_f = _dev(torch, offs, lens, first)
    d_e = torch.from_numpy(np.ascontiguousarray(expected, dtype=np.uint32).view(np.int32)).cuda()
    status = torch.full((3,), 0x77, dtype=torch.int64, device="cuda")
    ctx.sgl_verify_dev(t, d_o, d_l, d_f, d_e, status=status, **kw)
    torch.cuda.synchronize()
    s = status.cpu().numpy()
    assert s[2] == 0x77, "the entry past the status was written"
    return [int(s[0]), int(s[1])]


def test_verify(torch_cuda, ctx, region):
    torch = torch_cuda
    seed = 0x7E51
    rng = np.random.default_rng(seed)
    _, host = region
    t = torch.from_numpy(host).cuda()  # a private copy: this test flips bytes
    n = 3000
    counts = rng.integers(0, 9, size=n)
    counts[77] = 0  # an empty value
    counts[100], counts[2500] = 3, 4
    offs, lens = _parts(rng, int(counts.sum()), [1, 3, 15, 16, 17, 4095, 4097], REGION_BYTES)
    first = _first(counts)
    good = R.gathered_crcs_arrays(host, offs, lens, first)
    what = f"verify, seed {seed:#x}"
    for kw in ({}, {"max_seg_len": 4097}):
        assert _status(torch, ctx, t, offs, lens, first, good, **kw) == [0, -1], what
    # one byte flipped in the first segment of value a and in the last segment of value b > a
    va, vb = 100, 2500
    pa = int(offs[int(first[va])])
    jb = int(first[vb + 1]) - 1
    pb = int(offs[jb]) + int(lens[jb]) - 1
    flipped = host.copy()
    flipped[pa] ^= 0x10
    flipped[pb] ^= 0x01
    now = R.gathered_crcs_arrays(flipped, offs, lens, first)
    nbad = int((now != good).sum())  # segments are random: a flipped byte may lie in other values too
    assert now[va] != good[va] and now[vb] != good[vb]
    t[pa] ^= 0x10
    t[pb] ^= 0x01
    want = [nbad, int(np.nonzero(now != good)[0][0])]
    assert _status(torch, ctx, t, offs, lens, first, good) == want, what
    assert _status(torch, ctx, t, offs, lens, first, now) == [0, -1], what
    # exactly {2, a}: expected right everywhere but at a and b
    e = now.copy()
    e[va] = good[va]
    e[vb] = good[vb]
    assert _status(torch, ctx, t, offs, lens, first, e) == [2, va], what
    # wrong only for an empty value
    e = now.copy()
    assert e[77] == 0
    e[77] = 1
    assert _status(torch, ctx, t, offs, lens, first, e) == [1, 77], what
    # n == 0 still writes the status
    assert _status(torch, ctx, t, offs[:0], lens[:0], [0], np.zeros(0, dtype=np.uint32)) == [0, -1]
    # every value empty
    assert _status(torch, ctx, t, offs[:0], lens[:0], [0, 0, 0], np.array([0, 5])) == [1, 1]


# ---------------------------------------------------------------- the rest
def test_golden_fixture(torch_cuda, ctx):
    torch = torch_cuda
    cases = R.sgl_golden()["cases"]
    groups = {}
    for c in cases:
        groups.setdefault((c["seed"], c["region_bytes"]), []).append(c)
    for (seed, size), cs in groups.items():
        t = torch.empty(size, dtype=torch.uint8, device="cuda")
        ctx.fill_splitmix(t, seed, 0)
        offs, lens, first = R.pack([[tuple(p) for p in c["parts"]] for c in cs])
        got = _sgl(torch, ctx, t, offs, lens, first, f"golden, region seed {seed:#x}")
        assert [f"{int(x):08x}" for x in got] == [c["crc"] for c in cs], f"golden, region seed {seed:#x}"


def test_null_arguments(torch_cuda, ctx, region):
    torch = torch_cuda
    from priskv_amd import lib
    L = lib()
    t, _ = region
    offs, lens, first = _dev(torch, *R.pack([[(0, 16)], [(16, 16)]]))
    out = _sentinel(torch, 2)
    exp = torch.zeros(2, dtype=torch.int32, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    h, b, o, l, f = ctx.handle, t.data_ptr(), offs.data_ptr(), lens.data_ptr(), first.data_ptr()
    E = -errno.EINVAL
    comb, sgl, ver = L.priskv_crc32_combine_dev, L.priskv_crc32_sgl_dev, L.priskv_crc32_sgl_verify_dev
    assert comb(None, l, l, 2, f, 2, out.data_ptr(), None) == E
    assert comb(h, None, l, 2, f, 2, out.data_ptr(), None) == E
    assert comb(h, l, None, 2, f, 2, out.data_ptr(), None) == E
    assert comb(h, l, l, 2, None, 2, out.data_ptr(), None) == E
    assert comb(h, l, l, 2, f, 2, None, None) == E
    assert comb(h, None, None, 2, None, 0, None, None) == 0  # n == 0: nothing to do
    assert sgl(None, b, o, l, 2, f, 2, 0, out.data_ptr(), None) == E
    assert sgl(h, None, o, l, 2, f, 2, 0, out.data_ptr(), None) == E
    assert sgl(h, b, None, l, 2, f, 2, 0, out.data_ptr(), None) == E
    assert sgl(h, b, o, None, 2, f, 2, 0, out.data_ptr(), None) == E
    assert sgl(h, b, o, l, 2, None, 2, 0, out.data_ptr(), None) == E
    assert sgl(h, b, o, l, 2, f, 2, 0, None, None) == E
    assert sgl(h, None, None, None, 2, None, 0, 0, None, None) == 0
    assert ver(None, b, o, l, 2, f, 2, 0, exp.data_ptr(), st.data_ptr(), None) == E
    assert ver(h, None, o, l, 2, f, 2, 0, exp.data_ptr(), st.data_ptr(), None) == E
    assert ver(h, b, None, l, 2, f, 2, 0, exp.data_ptr(), st.data_ptr(), None) == E
    assert ver(h, b, o, None, 2, f, 2, 0, exp.data_ptr(), st.data_ptr(), None) == E
    assert ver(h, b, o, l, 2, None, 2, 0, exp.data_ptr(), st.data_ptr(), None) == E
    assert ver(h, b, o, l, 2, f, 2, 0, None, st.data_ptr(), None) == E
    assert ver(h, b, o, l, 2, f, 2, 0, exp.data_ptr(), None, None) == E
    assert ver(h, None, None, None, 0, None, 0, 0, None, None, None) == E  # n == 0 still needs the status
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all(), "a refused call wrote its output"
    # the part arrays may be NULL when there are no parts
    assert comb(h, None, None, 0, f, 2, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert _result(out, 2, "no parts").tolist() == [0, 0]
    out.fill_(SENT)
    assert sgl(h, None, None, None, 0, f, 2, 0, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert _result(out, 2, "no segments").tolist() == [0, 0]
    # python-side checks
    with pytest.raises(ValueError):
        ctx.sgl_dev(t, offs, lens, first.to(torch.int32))
    with pytest.raises(ValueError):
        ctx.sgl_dev(t, offs, lens[:1], first)
    with pytest.raises(ValueError):
        ctx.sgl_verify_dev(t, offs, lens, first, exp[:1])
    with pytest.raises(ValueError):
        ctx.combine_dev(lens, lens, first.cpu())


def test_graph_capture(torch_cuda, ctx):
    """sgl_dev + sgl_verify_dev captured once, replayed three times back to back with the data changed"""
    torch = torch_cuda
    seed = 0x6A01
    rng = np.random.default_rng(seed)
    size = MIB
    t = torch.empty(size, dtype=torch.uint8, device="cuda")
    ctx.fill_splitmix(t, seed, 0)
    counts = np.array([0, 1, 2, 7, 8, 9, 63, 64, 65, 200] + [3] * 500)
    offs, lens = _parts(rng, int(counts.sum()), [0, 1, 17, 300, 4095, 4097], size)
    first = _first(counts)
    n = counts.size
    d_o, d_l, d_f = _dev(torch, offs, lens, first)
    out = _sentinel(torch, n)
    exp = torch.zeros(n, dtype=torch.int32, device="cuda")
    status = torch.full((3,), 0x77, dtype=torch.int64, device="cuda")

    def calls(s):
        ctx.sgl_dev(t, d_o, d_l, d_f, out=out, stream=s)
        ctx.sgl_verify_dev(t, d_o, d_l, d_f, exp, status=status, stream=s, max_seg_len=4097)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        calls(s)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        calls(torch.cuda.current_stream())
    for k, flip in ((1, None), (2, 5), (3, None)):
        ctx.fill_splitmix(t, seed + k, 0)
        want = R.gathered_crcs_arrays(O.fill_splitmix(size, seed + k, 0), offs, lens, first)
        e = want.copy()
        if flip is not None:
            e[flip] ^= 1
        exp.copy_(torch.from_numpy(e.view(np.int32)))
        out.fill_(SENT)
        g.replay()
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_result(out, n, "graph replay"), want), f"graph replay {k}, seed {seed:#x}"
        st = status.cpu().numpy().tolist()
        assert st == ([0, -1, 0x77] if flip is None else [1, flip, 0x77]), f"graph replay {k}: status {st}"


def test_two_threads_one_context(torch_cuda, ctx, region):
    """two host threads, each on its own stream, 200 sgl_dev calls each on one context
    (every call holds two pool slots: the part CRCs, and the extents path's own)"""
    torch = torch_cuda
    t, host = region
    jobs = []
    for i in range(2):
        seed = 0x7100 + i
        rng = np.random.default_rng(seed)
        counts = rng.integers(0, 9, size=4000)  # enough segments for the byte-balanced extents split
        offs, lens = _parts(rng, int(counts.sum()), [0, 1, 17, 300, 4097], REGION_BYTES)
        first = _first(counts)
        jobs.append((seed, _dev(torch, offs, lens, first), R.gathered_crcs_arrays(host, offs, lens, first)))
    errors = []

    def worker(i):
        try:
            seed, (d_o, d_l, d_f), want = jobs[i]
            n = want.size
            s = torch.cuda.Stream()
            outs = [_sentinel(torch, n) for _ in range(4)]
            for it in range(200):
                ctx.sgl_dev(t, d_o, d_l, d_f, out=outs[it % 4], stream=s)
                if it % 50 == 49:
                    s.synchronize()
                    for o in outs:
                        if not np.array_equal(_result(o, n, f"thread {i}"), want):
                            errors.append(f"thread {i} call {it}, seed {seed:#x}: wrong CRCs")
            ctx.stream_release(s)
        except Exception as e:  # noqa: BLE001
            errors.append(f"thread {i}: {e!r}")

    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
