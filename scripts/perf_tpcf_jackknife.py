"""Timing of the jackknife pair counts of the two-point correlation function (device.tpcf_jackknife_counts) next to the
plain pair counts of the same input (device.tpcf_cross_counts): 10^6 uniform device-resident float64 positions in
L = 1000 Mpc/h, 20 logarithmic bins up to 50, 5 x 5 x 5 regions, auto pairs.  Three calls on the same set, alternated
within every repetition: the plain counts, the jackknife with its table in LDS, and the jackknife with
ASTRILD_TPCF_JK_LDS=0 (64-bit global atomics).  Then, once each way round, the table that only fits global memory:
125 regions x 40 x 40 (s, mu) bins.  Prints ms per call (one warm-up each, then the median of --reps synchronised calls)
and the per-stage split (AST_PROF, HIP events).
usage: python scripts/perf_tpcf_jackknife.py [--reps R] [--n N] [--out FILE]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from astrild_amd import device as dev
from tests import tpcf_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
torch.cuda.set_device(0)
L = 1000.0
S = np.geomspace(0.1, 50.0, 21)
NSUB = (5, 5, 5)
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def with_lds(value, call):
    def run():
        os.environ["ASTRILD_TPCF_JK_LDS"] = value
        try:
            return call()
        finally:
            del os.environ["ASTRILD_TPCF_JK_LDS"]
    return run


def compare(cases, reps):
    """{label: call} -> {label: (median ms, result)}: a warm-up of each, then ``reps`` rounds over all of them in turn."""
    out, times = {}, {k: [] for k in cases}
    for k, call in cases.items():
        out[k] = call()
        torch.cuda.synchronize()
    for _ in range(reps):
        for k, call in cases.items():
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    res = {}
    for k, call in cases.items():
        dev.profile_enable(True)
        call()
        split = dev.profile_report()
        dev.profile_enable(False)
        ms = float(np.median(times[k]))
        emit(f"{k:44s} {ms:10.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})  "
             + "  ".join(f"{name} {v[1]:.3f}" for name, v in split.items()))
        res[k] = (ms, out[k])
    return res


emit(f"device: {torch.cuda.get_device_name(0)}   reps {args.reps}   N {args.n}   L {L}   20 log bins, 0.1 .. 50, "
     f"{NSUB[0]} x {NSUB[1]} x {NSUB[2]} regions, auto pairs, periodic")
p = dev.as_device(orc.uniform(args.n, L, 1), torch.float64)
jk = lambda: dev.tpcf_jackknife_counts(p, NSUB, S, boxsize=L)
r = compare({"tpcf_cross_counts(A), auto": lambda: dev.tpcf_cross_counts(p, None, S, boxsize=L),
             "tpcf_jackknife_counts(A), table in LDS": with_lds("1", jk),
             "tpcf_jackknife_counts(A), global atomics": with_lds("0", jk)}, args.reps)
(ms_c, c), (ms_l, (cl, el)), (ms_g, (cg, eg)) = r.values()
assert torch.equal(c, cl) and torch.equal(c, cg) and torch.equal(el, eg), "the three calls disagree"
assert torch.equal(el.sum(0), 2 * c), "the endpoint table does not sum to twice the counts"
emit(f"pairs counted {int(c.sum())}   jackknife (LDS) / plain {ms_l / ms_c:.2f}x   global / LDS at 125 x 20 {ms_g / ms_l:.2f}x")

MU = np.linspace(0.0, 1.0, 41)
S40 = np.linspace(0.0, 50.0, 41)
jk2 = lambda: dev.tpcf_jackknife_counts(p, NSUB, S40, MU, boxsize=L)
r = compare({"tpcf_cross_counts(A), 40 x 40 (s, mu)": lambda: dev.tpcf_cross_counts(p, None, S40, MU, boxsize=L),
             "tpcf_jackknife_counts(A), 125 x 40 x 40": jk2}, max(3, args.reps // 3))
(ms_c2, c2), (ms_j2, (cj2, ej2)) = r.values()
assert torch.equal(c2, cj2) and torch.equal(ej2.sum(0), 2 * c2)
emit(f"125 x 40 x 40 counters (global atomics only) / plain {ms_j2 / ms_c2:.2f}x")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
