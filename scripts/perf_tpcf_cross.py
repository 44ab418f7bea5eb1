"""Timing of the two-sample pair counts of the two-point correlation function (device.tpcf_cross_counts) next to the
one-sample kernel (device.tpcf_pair_counts): a uniform set of 10^6 device-resident float64 positions in L = 500 Mpc/h,
40 s edges up to 50 and 40 mu edges.  Three counts of the same set: the cross count with itself in the periodic box
(27 neighbour cells, every ordered pair), the one-sample periodic count (14 half-shell cells, i < j) and the open-boundary
auto count.  Prints ms per call (one warm-up, then the median of --reps calls, each synchronised) and the per-stage split
(AST_PROF, HIP events).
usage: python scripts/perf_tpcf_cross.py [--reps R] [--out FILE]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from astrild_amd import device as dev
from tests import tpcf_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
torch.cuda.set_device(0)
L = 500.0
S = np.linspace(0.0, 50.0, 40)
MU = np.sort(1.0 - np.geomspace(0.001, 1.0, 40))
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def case(label, call):
    cnt = call()
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
    return ms, dev.to_numpy(cnt)


emit(f"device: {torch.cuda.get_device_name(0)}   reps {args.reps}   N {args.n}   L {L}   39 x 39 bins, s <= 50")
p = dev.as_device(orc.uniform(args.n, L, 1), torch.float64)
ms_x, c_x = case("cross(A, A), periodic", lambda: dev.tpcf_cross_counts(p, p, S, MU, boxsize=L))
ms_a, c_a = case("tpcf_pair_counts(A), periodic", lambda: dev.tpcf_pair_counts(p, L, S, MU))
ms_o, c_o = case("auto(A), open boundaries", lambda: dev.tpcf_cross_counts(p, None, S, MU))
ms_p, c_p = case("auto(A), periodic, two-set kernel", lambda: dev.tpcf_cross_counts(p, None, S, MU, boxsize=L))
assert np.array_equal(c_x, 2 * c_a), "cross(A, A) is not twice the one-sample counts"
assert np.array_equal(c_p, c_a), "the periodic auto counts of the two kernels differ"
assert np.all(c_o <= c_a), "an open bin above its periodic bin"
emit(f"cross / one-sample {ms_x / ms_a:.2f}x   open auto / one-sample {ms_o / ms_a:.2f}x   "
     f"two-set periodic auto / one-sample {ms_p / ms_a:.2f}x")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
