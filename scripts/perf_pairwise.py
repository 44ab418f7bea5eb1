"""Timing of the transverse-velocity pairwise estimator (device.pairwise_tv: prep + cell grid + pair kernel + fixed-order
sum), device-resident float64 inputs, 40 bins.  Prints ms per call, pair tests/s counted as the reference's loop counts
them (all N (N - 1) / 2 pairs, whatever the grid skips), accepted pairs/s (the pairs inside the reach), the per-kernel
split (HIP events), and the numpy oracle's single-core time at N = 50 000 (timed on every 50th row, scaled by the
pairs of all rows).  usage: python scripts/perf_pairwise.py [--reps R]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from astrild_amd import device as dev
from tests import pairwise_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
torch.cuda.set_device(0)


def compact(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 25.0, (n, 3)) + np.array([-12.5, -12.5, 1000.0])     # diagonal 43 < reach 51.3


def case(label, pos, binwidth, single=False):
    vel = np.random.default_rng(1).normal(0.0, 300.0, (len(pos), 2))
    p, v = dev.as_device(pos, torch.float64), dev.as_device(vel, torch.float64)
    if single:
        os.environ["ASTRILD_PV_CELLS"] = "0"
    try:
        cnt = dev.pairwise_tv(p, v, 40, binwidth)[2]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            dev.pairwise_tv(p, v, 40, binwidth)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.reps * 1e3
        dev.profile_enable(True)
        dev.pairwise_tv(p, v, 40, binwidth)
        split = dev.profile_report()
        dev.profile_enable(False)
    finally:
        os.environ.pop("ASTRILD_PV_CELLS", None)
    n = len(pos)
    tests = n * (n - 1) / 2
    acc = int(dev.to_numpy(cnt).sum())
    print(f"{label:52s} {ms:9.3f} ms  {tests / ms * 1e3:9.3e} pair tests/s  {acc / ms * 1e3:9.3e} accepted/s"
          f"  ({acc:.3e} accepted)  " + "  ".join(f"{k} {v[1]:.3f}" for k, v in split.items()), flush=True)
    return ms


def oracle_single_core(label, pos, binwidth):
    vel = np.random.default_rng(1).normal(0.0, 300.0, (len(pos), 2))
    n = len(pos)
    rows = range(0, n - 1, 50)
    u, t = orc.angles_and_velocities(pos, vel)
    t0 = time.perf_counter()
    orc.pair_sums(pos, u, t, 40, binwidth, rows=rows)
    dt = time.perf_counter() - t0
    scale = (n * (n - 1) / 2) / sum(n - 1 - i for i in rows)
    print(f"{label:52s} {dt * scale * 1e3:9.1f} ms  (numpy oracle, one core, {len(rows)} rows timed x {scale:.1f})",
          flush=True)


print(f"device: {torch.cuda.get_device_name(0)}   reps {args.reps}   40 bins")
bw50 = 50.0 / 39                                  # the reference's bins = linspace(0, 50, 40): reach 51.28
c50 = compact(50_000, 2)
lc50, _ = orc.light_cone(50_000, seed=3)
case("N=5e4 compact (all pairs in reach), grid", c50, bw50)
case("N=5e4 compact, single cell", c50, bw50, single=True)
case("N=5e4 light cone z 500-3000, grid", lc50, bw50)
case("N=5e4 light cone, single cell", lc50, bw50, single=True)
lc1m, _ = orc.light_cone(1_000_000, seed=4)
case("N=1e6 light cone, rmax 50, grid", lc1m, 1.25)
case("N=1e6 light cone, rmax 150, grid", lc1m, 3.75)
case("N=1e6 light cone, rmax 50, single cell", lc1m, 1.25, single=True)
oracle_single_core("N=5e4 compact", c50, bw50)
oracle_single_core("N=5e4 light cone", lc50, bw50)
