"""Timing of the pairwise-velocity moments in a box (device.pair_velocity_moments) next to the two-point correlation
function's pair counts on the same sets and edges (device.tpcf_cross_counts, the yardstick: it tests the same candidate
pairs and does one integer add per pair): the catalogue of scripts/perf_tpcf_cross.py, a uniform set of 10^6
device-resident float64 positions in L = 500 Mpc/h with N(0, 300) velocities, 40 edges up to 50.  "radial" as the auto
term and as the cross term of the set with itself, "los" with pi_max = 40 (reach 64: seven cells per axis), and "los" with
the largest reach the checks allow (rp, pi_max just below L / 3: one cell, every pair of the box - at --n-one-cell
objects).  Prints ms per call (one warm-up, then the median of --reps calls, each synchronised) and the per-stage split
(AST_PROF, HIP events).
usage: python scripts/perf_pair_velocity.py [--reps R] [--n N] [--n-one-cell M] [--out FILE]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from astrild_amd import device as dev
from tests import tpcf_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--n-one-cell", type=int, default=100_000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
torch.cuda.set_device(0)
L = 500.0
S = np.linspace(0.0, 50.0, 40)
PI = 40.0
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def case(label, call):
    out = call()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    dev.profile_enable(True)
    call()
    split = dev.profile_report()
    dev.profile_enable(False)
    ms = float(np.median(times))
    emit(f"{label:44s} {ms:10.3f} ms (min {min(times):.3f}, max {max(times):.3f})  "
         + "  ".join(f"{k} {v[1]:.3f}" for k, v in split.items()))
    first = out[0] if isinstance(out, tuple) else out
    return ms, dev.to_numpy(first)


emit(f"device: {torch.cuda.get_device_name(0)}   reps {args.reps}   N {args.n}   L {L}   39 bins, r <= 50")
p = dev.as_device(orc.uniform(args.n, L, 1), torch.float64)
v = dev.as_device(np.random.default_rng(2).normal(0.0, 300.0, (args.n, 3)), torch.float64)
ms_ta, c_ta = case("tpcf_cross_counts(A), auto, periodic", lambda: dev.tpcf_cross_counts(p, None, S, boxsize=L))
ms_tx, c_tx = case("tpcf_cross_counts(A, A), periodic", lambda: dev.tpcf_cross_counts(p, p, S, boxsize=L))
ms_ra, c_ra = case("radial, auto, periodic", lambda: dev.pair_velocity_moments(p, v, S, boxsize=L))
ms_rx, c_rx = case("radial, cross(A, A), periodic", lambda: dev.pair_velocity_moments(p, v, S, p, v, boxsize=L))
ms_ro, c_ro = case("radial, auto, open boundaries", lambda: dev.pair_velocity_moments(p, v, S))
ms_la, c_la = case("los, pi_max 40, auto, periodic",
                   lambda: dev.pair_velocity_moments(p, v, S, boxsize=L, kind="los", pi_max=PI))
ms_lx, c_lx = case("los, pi_max 40, cross(A, A), periodic",
                   lambda: dev.pair_velocity_moments(p, v, S, p, v, boxsize=L, kind="los", pi_max=PI))
assert np.array_equal(c_ra, c_ta), "the radial auto counts are not the TPCF's"
assert np.array_equal(c_rx, c_tx) and np.array_equal(c_rx, 2 * c_ra), "the radial cross counts are not the TPCF's"
assert np.all(c_ro <= c_ra), "an open bin above its periodic bin"
assert np.array_equal(c_lx, 2 * c_la), "los: cross(A, A) is not twice the auto counts"
emit(f"radial / tpcf: auto {ms_ra / ms_ta:.2f}x   cross {ms_rx / ms_tx:.2f}x      "
     f"los / tpcf: auto {ms_la / ms_ta:.2f}x   cross {ms_lx / ms_tx:.2f}x")
m = args.n_one_cell
top = 0.333 * L
S1 = np.linspace(0.0, top, 40)
ms_1, c_1 = case(f"los, rp, pi_max <= {top:.1f}: one cell, N {m}",
                 lambda: dev.pair_velocity_moments(p[:m], v[:m], S1, boxsize=L, kind="los", pi_max=top))
ms_g, c_g = case(f"los, pi_max 40, auto, periodic, N {m}",
                 lambda: dev.pair_velocity_moments(p[:m], v[:m], S, boxsize=L, kind="los", pi_max=PI))
emit(f"one cell: {m * (m - 1) / 2 / ms_1 * 1e-6:.1f} G candidate pairs / s, {ms_1 / ms_g:.1f}x the 7-cell grid's time at "
     f"the same N")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
