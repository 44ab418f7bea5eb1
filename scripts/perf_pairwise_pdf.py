"""Timing of the pairwise-velocity histograms (device.pairwise_velocity_pdf: prep + cell grid + pair kernel), device-
resident float64 inputs, both kinds, on the catalogues of scripts/perf_pairwise.py.  Prints ms per call, seen pairs/s
(the pairs inside the reach: counted + outside), the histogram path taken and the per-kernel split (HIP events);
device.pairwise_tv on the same catalogues and reach as the yardstick of the pair finder; and the sweep that the LDS
budget rests on: the same histogram counted in LDS and in global memory (ASTRILD_PVPDF_LDS=0), at sizes from 6 to 145
KiB of counters, which with the j stage is all of a CU's 160 KiB.
usage: python scripts/perf_pairwise_pdf.py [--reps R] > profiles/pairwise_pdf_perf.txt"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from astrild_amd import _lib, device as dev
from tests import pairwise_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
torch.cuda.set_device(0)
VSIG = 300.0                                      # km/s per component: v12 has sigma 424


def compact(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 25.0, (n, 3)) + np.array([-12.5, -12.5, 1000.0])     # diagonal 43 < reach 50


def timed(fn):
    out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.reps * 1e3
    dev.profile_enable(True)
    fn()
    split = dev.profile_report()
    dev.profile_enable(False)
    return out, ms, split


def case(label, p, v, kind, r, dist_bin, vel_bin, env=None, moments=False):
    """One timed configuration; the velocity axis spans +-1000 km/s, the distance axis the reach."""
    env = env or {}
    os.environ.update(env)
    try:
        par = dict(r=r, dist_bin=dist_bin, vel_bin=vel_bin, kind=kind, dist_width=r / dist_bin,
                   vel_width=2000.0 / vel_bin, moments=moments)
        res, ms, split = timed(lambda: dev.pairwise_velocity_pdf(p, v, **par))
    finally:
        for k in env:
            os.environ.pop(k, None)
    seen = int(res[0].sum().item()) + int(res[1].item())
    path = "lds" if "pairwise_pdf_pairs_lds" in split else "global"
    print(f"{label:44s} {kind:6s} {dist_bin:4d} x {vel_bin:4d} {path:6s} {ms:9.3f} ms  {seen / ms * 1e3:9.3e} seen/s"
          f"  ({seen:.3e} seen, {int(res[1].item()) / max(seen, 1):.3f} outside)  "
          + "  ".join(f"{k.replace('pairwise_pdf_', '')} {t[1]:.3f}" for k, t in split.items()), flush=True)
    return ms


def yardstick(label, p, v, r):
    binwidth = r / 40
    res, ms, split = timed(lambda: dev.pairwise_tv(p, v, 40, binwidth))
    acc = int(res[2].sum().item())
    print(f"{label:44s} pairwise_tv, 40 bins        {ms:9.3f} ms  {acc / ms * 1e3:9.3e} accepted/s  ({acc:.3e} accepted)",
          flush=True)


ONE_CELL = {"ASTRILD_PVPDF_CELLS": "0"}
GLOBAL = {"ASTRILD_PVPDF_LDS": "0"}
lib = _lib.lib()
edge = lib.ast_pairwise_pdf_lds_bins(100, 0) // 100
print(f"device: {torch.cuda.get_device_name(0)}   reps {args.reps}   LDS path up to "
      f"{lib.ast_pairwise_pdf_lds_bins(100, 0)} counters at 100 distance bins (no moments)")
rng = np.random.default_rng(1)
cats = []
pos = compact(50_000, 2)
cats.append(("N=5e4 compact", pos, 50.0))
lc, _ = orc.light_cone(1_000_000, seed=4)
cats.append(("N=1e6 light cone r=50", lc, 50.0))
cats.append(("N=1e6 light cone r=150", lc, 150.0))
dev_arrays = {}
for name, pos, r in cats:
    if id(pos) not in dev_arrays:
        vel = np.random.default_rng(1).normal(0.0, VSIG, pos.shape)
        dev_arrays[id(pos)] = (dev.as_device(pos, torch.float64), dev.as_device(vel, torch.float64))

print("--- histogram sizes: 40 x 40 (LDS), just below and above the LDS budget, 100 x 4096 (global); grid and one cell")
for name, pos, r in cats:
    p, v = dev_arrays[id(pos)]
    yardstick(name, p, v[:, :2].contiguous(), r)
    for kind in ("z_sign", "radial"):
        for dist_bin, vel_bin in ((40, 40), (100, edge), (100, edge + 1), (100, 4096)):
            case(name + ", grid", p, v, kind, r, dist_bin, vel_bin)
        for dist_bin, vel_bin in ((40, 40), (100, 4096)):
            case(name + ", one cell", p, v, kind, r, dist_bin, vel_bin, env=ONE_CELL)
    case(name + ", grid, with moments", p, v, "radial", r, 40, 40, moments=True)

print("--- the LDS budget: one histogram counted in LDS and in global memory")
for name, pos, r in cats[:2]:
    p, v = dev_arrays[id(pos)]
    for vel_bin in (16, 64, 100, 130, 200, 260, 370):          # x 100 x 4 B: 6, 25, 39, 51, 78, 102, 145 KiB of counters
        a = case(name + ", LDS", p, v, "radial", r, 100, vel_bin)
        b = case(name + ", global", p, v, "radial", r, 100, vel_bin, env=GLOBAL)
        print(f"{'':44s} {100 * vel_bin * 4 / 1024:6.1f} KiB of counters: LDS / global = {a / b:.3f}", flush=True)
