#!/usr/bin/env python3
"""Gathered values (sgl_dev / combine_dev) beside ranges_dev on the same segments (tools only).

  python tools/sgl_bench.py [--rounds=R] [--calls=K] [--out=PATH] [--quick]

Every figure is the median over R rounds of a per-round median over K
event-timed calls on one stream, all variants of a shape in the same
process with their order alternating from round to round, as the other
tools/*_ab.py do.
One JSON line per (shape, variant) goes to PATH (default
profiles/sgl/sgl_bench.jsonl).  --quick: the shapes at 1/64 of their size
(a rehearsal; its numbers measure overheads).

Shapes:
  large  64 Ki values x 8 x 4 KiB (2 GiB), segments shuffled: ranges_dev on
         the 512 Ki segments, sgl_dev, and the combine alone on their CRCs
  odd    64 Ki values x 3 segments of 4095, 4097 and 100 B
  small  1 / 8 / 64 values x 8 x 4 KiB, with and without the length bound
  comb   combine_dev alone: 1 Mi values x 8 parts, lengths 4 KiB each /
         random below 1 MiB (the cost per set bit of the shift amounts)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from priskv_amd import CrcContext, as_u32  # noqa: E402


def _opt(name, default):
    return next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith(f"--{name}=")), default)


ROUNDS = int(_opt("rounds", "5"))
CALLS = int(_opt("calls", "20"))
OUT = _opt("out", os.path.join(ROOT, "profiles", "sgl", "sgl_bench.jsonl"))
QUICK = "--quick" in sys.argv
SCALE = 64 if QUICK else 1

ctx = CrcContext(0)
stream = torch.cuda.Stream()
rows = []


def median_us(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for e0, e1 in evs:
        e0.record(stream)
        fn()
        e1.record(stream)
    torch.cuda.synchronize()
    return float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]))


def ab(shape, variants, meta, calls=CALLS):
    """variants: {name: fn}; alternating order over the rounds"""
    names = list(variants)
    per = {k: [] for k in names}
    for r in range(ROUNDS):
        k = r % len(names)
        for name in (names[k:] + names[:k]) if r % 2 == 0 else (names[k:] + names[:k])[::-1]:
            per[name].append(median_us(variants[name], calls))
    base = float(np.median(per[names[0]]))
    for name in names:
        us = float(np.median(per[name]))
        row = dict(shape=shape, variant=name, us=round(us, 2), rounds=[round(x, 2) for x in per[name]],
                   vs_first=round(us / base, 4), **meta)
        rows.append(row)
        print(json.dumps(row), flush=True)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).cuda()


def paged(nval, per, lens_of_value, region, rng):
    """nval values of per segments; segment k of a value has length lens_of_value[k]; each
    segment starts at its own 8 KiB slot of the region, the slots shuffled"""
    nseg = nval * per
    slots = rng.permutation(region.numel() // 8192)[:nseg].astype(np.int64) * 8192
    lens = np.tile(np.array(lens_of_value, dtype=np.int64), nval)
    return dev(slots, np.int64), dev(lens, np.int32), torch.arange(0, nseg + 1, per, dtype=torch.int64,
                                                                     device="cuda")


def run_pages(shape, nval, per, lens_of_value, region, rng, bound=None, calls=CALLS):
    d_o, d_l, d_f = paged(nval, per, lens_of_value, region, rng)
    nseg = nval * per
    out_r = torch.empty(nseg, dtype=torch.int32, device="cuda")
    out_s = torch.empty(nval, dtype=torch.int32, device="cuda")
    out_c = torch.empty(nval, dtype=torch.int32, device="cuda")
    v = {"ranges_dev": lambda: ctx.ranges_dev(region, d_o, d_l, out=out_r, stream=stream),
         "sgl_dev": lambda: ctx.sgl_dev(region, d_o, d_l, d_f, out=out_s, stream=stream),
         "combine_dev": lambda: ctx.combine_dev(out_r, d_l, d_f, out=out_c, stream=stream)}
    if bound:
        v["ranges_dev_bounded"] = lambda: ctx.ranges_dev(region, d_o, d_l, out=out_r, stream=stream, max_len=bound)
        v["sgl_dev_bounded"] = lambda: ctx.sgl_dev(region, d_o, d_l, d_f, out=out_s, stream=stream,
                                                   max_seg_len=bound)
    ab(shape, v, dict(values=nval, parts=nseg, bytes=int(sum(lens_of_value)) * nval), calls)
    torch.cuda.synchronize()
    assert np.array_equal(as_u32(out_s), as_u32(out_c)), shape  # sgl_dev == combine of ranges_dev's CRCs


def main():
    rng = np.random.default_rng(0x561)
    nval = (64 << 10) // SCALE
    region = torch.empty(nval * 8 * 8192, dtype=torch.uint8, device="cuda")  # 4 GiB: one 8 KiB slot per segment
    ctx.fill_splitmix(region, 0x561, 0)
    run_pages("large 64Ki x 8 x 4KiB", nval, 8, [4096] * 8, region, rng)
    run_pages("odd 64Ki x (4095, 4097, 100)", nval, 3, [4095, 4097, 100], region, rng)
    for n in (1, 8, 64):
        run_pages(f"small {n} x 8 x 4KiB", n, 8, [4096] * 8, region, rng, bound=4096, calls=max(CALLS, 100))
    del region
    # combine alone
    nv = (1 << 20) // SCALE
    crcs = torch.randint(-2**31, 2**31 - 1, (nv * 8,), dtype=torch.int32, device="cuda")
    first = torch.arange(0, nv * 8 + 1, 8, dtype=torch.int64, device="cuda")
    out = torch.empty(nv, dtype=torch.int32, device="cuda")
    l_eq = torch.full((nv * 8,), 4096, dtype=torch.int32, device="cuda")
    l_rnd = torch.randint(0, 1 << 20, (nv * 8,), dtype=torch.int32, device="cuda")
    # mean and largest popcount of the shift amounts over a wave's 64 lanes decide the cost
    suf = l_rnd.view(nv, 8).to(torch.int64).flip(1).cumsum(1).flip(1) - l_rnd.view(nv, 8)
    pop = sum(((suf >> b) & 1) for b in range(24)).view(-1, 64)
    meta = dict(values=nv, parts=nv * 8)
    ab("comb 1Mi x 8", {"equal 4KiB": lambda: ctx.combine_dev(crcs, l_eq, first, out=out, stream=stream),
                        "random < 1MiB": lambda: ctx.combine_dev(crcs, l_rnd, first, out=out, stream=stream)},
       dict(meta, random_mean_popcount=round(float(pop.float().mean()), 2),
            random_mean_wave_max_popcount=round(float(pop.max(1).values.float().mean()), 2),
            equal_wave_max_popcount=3))
    for row in rows:
        if row["shape"].startswith("comb"):
            row["parts_per_s"] = round(row["parts"] / (row["us"] * 1e-6), 0)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    print(f"wrote {OUT}: {len(rows)} rows")


if __name__ == "__main__":
    main()
