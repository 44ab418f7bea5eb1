"""Timing of the periodic two-point correlation function's pair counts (device.tpcf_pair_counts: prep + bounds read-back
+ cell grid + pair kernel + fixed-order sum), device-resident float64 positions in a box of L = 1000 Mpc/h.  Prints ms
per call, the accepted pairs (inside the top s edge and a mu bin) per second, the per-stage split (AST_PROF, HIP events)
and, labelled as such, a CPU baseline: scipy's periodic cKDTree count_neighbors on one core at N = 10^5.
usage: python scripts/perf_tpcf.py [--reps R] [--out FILE]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from astrild_amd import device as dev
from tests import tpcf_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
torch.cuda.set_device(0)
L = 1000.0
MU = np.linspace(0.0, 1.0, 40)
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def case(label, pos, smax, single=False):
    s = np.linspace(0.0, smax, 40)
    p = dev.as_device(pos, torch.float64)
    if single:
        os.environ["ASTRILD_TPCF_CELLS"] = "0"
    try:
        cnt = dev.tpcf_pair_counts(p, L, s, MU)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            dev.tpcf_pair_counts(p, L, s, MU)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.reps * 1e3
        dev.profile_enable(True)
        dev.tpcf_pair_counts(p, L, s, MU)
        split = dev.profile_report()
        dev.profile_enable(False)
    finally:
        os.environ.pop("ASTRILD_TPCF_CELLS", None)
    acc = int(dev.to_numpy(cnt).sum())
    emit(f"{label:56s} {ms:10.3f} ms  {acc / ms * 1e3:9.3e} accepted/s  ({acc:.3e} accepted)  "
         + "  ".join(f"{k} {v[1]:.3f}" for k, v in split.items()))
    return ms, dev.to_numpy(cnt)


def cpu_baseline(label, pos, smax):
    from scipy.spatial import cKDTree
    r = np.linspace(0.0, smax, 40)
    t0 = time.perf_counter()
    tree = cKDTree(pos, boxsize=L)
    tree.count_neighbors(tree, r)
    emit(f"{label:56s} {(time.perf_counter() - t0) * 1e3:10.1f} ms  (CPU baseline: scipy cKDTree(boxsize=L)"
         f".count_neighbors, one core, s only)")


emit(f"device: {torch.cuda.get_device_name(0)}   reps {args.reps}   L {L}   40 s edges x 40 mu edges (39 x 39 bins)")
u1m = orc.uniform(1_000_000, L, 1)
ms_g150, c_g = case("N=1e6 uniform, s <= 150, grid", u1m, 150.0)
ms_s150, c_s = case("N=1e6 uniform, s <= 150, single cell", u1m, 150.0, single=True)
assert np.array_equal(c_g, c_s), "grid and single cell differ"
case("N=1e6 clustered (2000 blobs, sigma 10), s <= 150, grid", orc.clustered(1_000_000, L, 2, blobs=2000, sigma=10.0),
     150.0)
ms_g50, c_g = case("N=1e6 uniform, s <= 50, grid", u1m, 50.0)
ms_s50, c_s = case("N=1e6 uniform, s <= 50, single cell", u1m, 50.0, single=True)
assert np.array_equal(c_g, c_s), "grid and single cell differ"
emit(f"grid speed-up over one cell: s <= 150 {ms_s150 / ms_g150:.1f}x, s <= 50 {ms_s50 / ms_g50:.1f}x")
cpu_baseline("N=1e5 uniform, s <= 150", u1m[:100_000], 150.0)
cpu_baseline("N=1e5 uniform, s <= 50", u1m[:100_000], 50.0)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
