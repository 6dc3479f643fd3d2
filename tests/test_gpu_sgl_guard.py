"""Coarse GPU time guard for the gathered-value path (style of test_gpu_perf_guard.py).

sgl_dev hashes the segments as ranges_dev does and then combines the parts'
CRCs per value: 8 bytes read and a few 32-step multiplies per 4 KiB hashed.
A combine that serialises (one thread per value walking its parts, a
multiply per bit instead of per set bit, ...) would not show in any parity
test.  The yardstick is the existing path on the same segments as separate
values, timed in the same process with the same events; the factor is
deliberately coarse.
"""
import numpy as np
import pytest

import _sgl_ref as R

pytestmark = pytest.mark.gpu

MIB = 1 << 20


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


def _median_us(torch, fn, stream, n=30):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in evs:
        e0.record(stream)
        fn()
        e1.record(stream)
    torch.cuda.synchronize()
    return float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]))


def test_sgl_not_slower_than_its_segments(torch_cuda, ctx):
    """8192 values x 8 segments x 4 KiB (256 MiB), segments shuffled over the region"""
    torch = torch_cuda
    from priskv_amd import as_u32
    seed = 0x6A4D
    nval, per, page = 8192, 8, 4096
    nseg = nval * per
    t = torch.empty(nseg * page, dtype=torch.uint8, device="cuda")
    ctx.fill_splitmix(t, seed, 0)
    rng = np.random.default_rng(seed)
    pages = rng.permutation(nseg).astype(np.int64)
    d_o = torch.from_numpy(pages * page).cuda()
    d_l = torch.full((nseg,), page, dtype=torch.int32, device="cuda")
    d_f = torch.arange(0, nseg + 1, per, dtype=torch.int64, device="cuda")
    out_r = torch.full((nseg,), -1, dtype=torch.int32, device="cuda")
    out_s = torch.full((nval,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    us_r = _median_us(torch, lambda: ctx.ranges_dev(t, d_o, d_l, out=out_r, stream=s), s)
    us_s = _median_us(torch, lambda: ctx.sgl_dev(t, d_o, d_l, d_f, out=out_s, stream=s), s)
    print(f"8192 x 8 x 4 KiB: ranges_dev {us_r:.1f} us, sgl_dev {us_s:.1f} us per call ({us_s / us_r:.3f}x)")
    # exact: the page CRCs combined by the tests' restatement (page CRCs are ranges_dev's,
    # checked against the oracle throughout test_gpu_parity.py), and the first values
    # against the oracle on the gathered bytes
    part = as_u32(out_r)
    got = as_u32(out_s)
    for v in (0, 1, nval // 2, nval - 1):
        assert got[v] == R.combine_value([(int(c), page) for c in part[v * per:(v + 1) * per]]), f"value {v}"
    k = 64
    host_pages = torch.stack([t[int(p) * page:(int(p) + 1) * page] for p in pages[:k * per]]).cpu().numpy()
    want = R.gathered_crcs_arrays(host_pages.reshape(-1), np.arange(k * per) * page, np.full(k * per, page),
                                  np.arange(0, k * per + 1, per))
    assert np.array_equal(got[:k], want), f"seed {seed:#x}"
    assert us_s < 2.0 * us_r, (f"sgl_dev {us_s:.1f} us vs ranges_dev {us_r:.1f} us on the same 65 536 segments "
                               f"({us_s / us_r:.2f}x, bound 2.0x): the combine serialises?")
