"""Timing of the friends-of-friends group finder (particles/hutils/fof.py: fof_groups) by stage.  The catalogue is the
clustered recipe of tests/fof_oracle.py repeated K = n // 6000 times in a box of side 100 K^(1/3), so that the mean
separation and the local structure stay those of the test: K blobs of 500 points (sigma 0.6), K of 700 (sigma 0.15),
10 K of 150 (sigma 0.5), centres uniform in the box, the rest a uniform background; wrapped, shuffled, float64, on the
device.  Sphere linking, b = 0.2 mean separations, periodic, nmin = 20.
Per run: HIP events (torch.cuda.Event) around find_roots (prepare + sort + link + compress, with their host reads)
and around number_groups, the library's own per-launch events (AST_PROF) inside the first, and the synchronised wall
time of the whole.  --warmup runs, then --reps timed ones; medians, with min and max.  --single-n M > 0: the same at M
particles with the cell grid and with ASTRILD_FOF_CELLS=0 (one cell, all pairs), alternating.  --cell-objects A,B,..:
the run at --n once per value of AST_FOF_CELL_OBJECTS (objects per planned cell), alternating, beside the default.
usage: python scripts/perf_fof.py [--reps R] [--warmup W] [--n N] [--single-n M] [--cell-objects A,B] [--out FILE.json]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from astrild_amd import device as dev
from astrild_amd.particles.hutils import fof

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--n", type=int, default=2_000_000)
ap.add_argument("--single-n", type=int, default=0)
ap.add_argument("--cell-objects", default="")
ap.add_argument("--out", default=None)
args = ap.parse_args()
torch.cuda.set_device(0)
NMIN = 20
STAGES = {"prepare_sort": ("fof_prep", "fof_grid"), "link": ("fof_link",), "compress": ("fof_jump", "fof_sizes"),
          "relabel": ("fof_relabel",)}


def catalogue(n, seed=2024):
    k = max(n // 6000, 1)
    box = 100.0 * k ** (1.0 / 3.0)
    rng = np.random.default_rng(seed)
    parts = []
    for count, sigma, blobs in ((500, 0.6, k), (700, 0.15, k), (150, 0.5, 10 * k)):
        centres = rng.uniform(0.0, box, (blobs, 3))
        parts.append((centres[:, None, :] + sigma * rng.standard_normal((blobs, count, 3))).reshape(-1, 3))
    parts.append(rng.uniform(0.0, box, (n - 2700 * k, 3)))
    pos = np.mod(np.concatenate(parts), box)
    return pos[rng.permutation(n)], box


def run(p, box, b):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    dev.profile_enable(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev[0].record()
    root, size, links, passes = fof.find_roots(p, box, b)
    ev[1].record()
    out = fof.number_groups(root, size, NMIN)
    ev[2].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    rep = dev.profile_report()
    dev.profile_enable(False)
    t = {"find_roots_events": ev[0].elapsed_time(ev[1]), "numbering_events": ev[1].elapsed_time(ev[2]), "wall": wall}
    for stage, scopes in STAGES.items():
        t[stage] = sum(rep[s][1] for s in scopes if s in rep)
    t["passes"] = float(passes)                    # the forest's depth depends on the order of the unions: it may vary
    return t, {"links": int(links.item()), "groups": int(out["first"].numel()),
               "largest": int(out["length"][0].item()) if out["first"].numel() else 0,
               "labels_sum": int(out["labels"].sum(dtype=torch.int64).item())}


def measure(n, variants):
    pos, box = catalogue(n)
    b = 0.2 * (box ** 3 / n) ** (1.0 / 3.0)
    p = dev.as_device(pos)
    times, facts = {v: [] for v in variants}, {}
    for it in range(args.warmup + args.reps):
        for v in variants:
            os.environ["ASTRILD_FOF_CELLS"] = "0" if v == "one_cell" else "1"
            os.environ.pop("AST_FOF_CELL_OBJECTS", None)
            if v.startswith("per_"):
                os.environ["AST_FOF_CELL_OBJECTS"] = v[4:]
            t, f = run(p, box, b)
            assert facts.setdefault("result", f) == f, f"the runs disagree: {facts['result']} and {f}"
            if it >= args.warmup:
                times[v].append(t)
    os.environ.pop("ASTRILD_FOF_CELLS", None)
    os.environ.pop("AST_FOF_CELL_OBJECTS", None)
    out = {"n": n, "boxsize": box, "linking_length": b, "nmin": NMIN, **facts["result"]}
    for v in variants:
        out[v] = {k: {"median_ms": float(np.median([t[k] for t in times[v]])),
                      "min_ms": float(np.min([t[k] for t in times[v]])),
                      "max_ms": float(np.max([t[k] for t in times[v]]))} for k in times[v][0] if k != "passes"}
        out[v]["passes"] = sorted({int(t["passes"]) for t in times[v]})
    return out


summary = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
           "cells": measure(args.n, ["cells"] + ["per_" + v for v in args.cell_objects.split(",") if v])}
if args.single_n > 0:
    summary["cells_and_one_cell"] = measure(args.single_n, ["cells", "one_cell"])
print(json.dumps(summary, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(summary, f, indent=1)
