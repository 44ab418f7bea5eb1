"""Timing of the (r_p, pi) pair counts (device.rp_pi_pair_counts) under both planners - cells of r_p,max across and
pi_max along the line of sight, and with ASTRILD_RPPI_ANISO=0 the isotropic cells of sqrt(r_p,max^2 + pi_max^2) - and,
for context, of device.tpcf_pair_counts with one s bin up to that isotropic reach (the same candidate pairs as the
isotropic plan).  A uniform set of --n device-resident float64 positions in L = 500, r_p edges geomspace(0.1, 30, 21),
pi edges linspace(0, 60, 61).  --warmup runs of every variant, then --reps timed ones, the variants alternating; per
run the per-stage kernel times (AST_PROF, HIP events) and the synchronised wall time; medians, with min and max.
usage: python scripts/perf_rppi.py [--reps R] [--warmup W] [--n N] [--out FILE.json]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from astrild_amd import device as dev

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
torch.cuda.set_device(0)
L = 500.0
RP = np.geomspace(0.1, 30.0, 21)
PI = np.linspace(0.0, 60.0, 61)
S = np.array([0.0, float(np.sqrt(RP[-1] ** 2 + PI[-1] ** 2))])
pos = dev.as_device(np.random.default_rng(2024).uniform(0.0, L, (args.n, 3)))


def rppi(aniso):
    os.environ["ASTRILD_RPPI_ANISO"] = "1" if aniso else "0"
    return dev.rp_pi_pair_counts(pos, L, RP, PI)


variants = {"aniso": (lambda: rppi(True), "rppi"), "iso": (lambda: rppi(False), "rppi"),
            "tpcf_1bin": (lambda: dev.tpcf_pair_counts(pos, L, S), "tpcf")}
stage = {k: {"grid": [], "pairs": [], "reduce": []} for k in variants}
wall = {k: [] for k in variants}
counts = {}
for it in range(args.warmup + args.reps):
    for name, (call, scope) in variants.items():
        dev.profile_enable(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rep = dev.profile_report()
        dev.profile_enable(False)
        counts.setdefault(name, dev.to_numpy(out))
        if it >= args.warmup:
            for part in stage[name]:
                stage[name][part].append(rep[f"{scope}_{part}"][1])
            wall[name].append((t1 - t0) * 1e3)
assert np.array_equal(counts["aniso"], counts["iso"]), "the two planners disagree"
summary = {"device": torch.cuda.get_device_name(0), "n": args.n, "L": L, "reps": args.reps, "warmup": args.warmup,
           "rppi_pairs_counted": int(counts["aniso"].sum()), "tpcf_pairs_counted": int(counts["tpcf_1bin"].sum())}
for name in variants:
    summary[name] = {part: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
                     for part, v in stage[name].items()}
    summary[name]["wall_ms_median"] = float(np.median(wall[name]))
summary["iso_over_aniso_pairs"] = summary["iso"]["pairs"]["median_ms"] / summary["aniso"]["pairs"]["median_ms"]
print(json.dumps(summary, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(summary, f, indent=1)
