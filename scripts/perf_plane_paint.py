"""Plane paint (plane_paint.plane_paint_sums / plane_paint_finish, csrc/plane_paint.hip): 512^3 float32 particles of
device.synth_lattice_particles with float32 masses into 8 planes of 4096^2 - box and light cone, NGP / CIC / TSC, once in
lattice order (the line of sight is the fastest index: 64 consecutive particles of a column meet in one pixel of one
plane) and once with shuffle=True (every thread somewhere else).  Per case the MEDIAN of REPS calls, each timed with its own
pair of device events after WARM warm-up calls, of (a) the accumulate kernel alone and (b) the whole paint: zero the sums,
accumulate, finish to float32.  From (a): particles per second and the rate of ATOMIC bytes, 8 bytes x W^2 per particle
that deposits (64-bit integer atomics: the guides give a chip-wide rate for float atomics only, 1.3 TB/s of added bytes).
From (b): the share of 8 TB/s that the ALGORITHMIC bytes - np (3 + 1) sizeof(Pt) + P npix^2 (8 + 8 + sizeof(T)):
particles in, sums zeroed and read once, planes out - would take in that time.  Beside them device.paint's direct CIC
paint (float atomics) of the same particles into 512^3, the yardstick.  No pass or fail number is attached: the record
decides whether a grouped or LDS-tiled variant is worth having.
Writes profiles/plane_paint_perf.txt.  --small: 128^3 particles into 8 planes of 1024^2, nothing written (a rehearsal)."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from astrild_amd import _lib, device as dev, plane_paint as pp  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "plane_paint_perf.txt")
WARM, REPS = 2, 10
PEAK = 8e12
BOX = 1000.0
SUPPORT = {"ngp": 1, "cic": 2, "tsc": 3}
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def median_ms(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return statistics.median(times), min(times), max(times)


def main():
    small = "--small" in sys.argv
    side, npix, P = (128, 1024, 8) if small else (512, 4096, 8)
    torch.cuda.set_device(0)
    npart = side ** 3
    emit(f"device: {torch.cuda.get_device_name(0)}   {side}^3 float32 particles and masses, {P} planes of {npix}^2, box {BOX:g}, "
         f"line of sight 2   warm-up {WARM}, median of {REPS} calls (min .. max), one pair of device events per call   "
         f"library {os.path.basename(_lib.LIB_PATH)}")
    emit("accumulate: the kernel alone; atomic bytes = 8 W^2 per depositing particle.  paint: zero + accumulate + finish (float32); "
         "share = algorithmic bytes / time / 8 TB/s, algorithmic bytes = np (3 + 1) 4 + P npix^2 (8 + 8 + 4)")
    alg = npart * 4 * 4 + P * npix * npix * 20
    mass = torch.ones(npart, dtype=torch.float32, device=dev.device())
    sums = torch.zeros((P, npix, npix), dtype=torch.int64, device=dev.device())
    counters = torch.zeros(3, dtype=torch.int64, device=dev.device())
    out = torch.empty((P, npix, npix), dtype=torch.float32, device=dev.device())
    mul, add = pp.upload_doubles(np.full(P, 2.0 ** -20), np.full(P, -1.0))
    # cone: the observer one box length in front of the box's near face, on its axis; 8 shells through the box
    angle, edges = 25.0, np.linspace(BOX, 2 * BOX, P + 1)
    cone = pp.check_plane_paint_args("cone", (npart, 3), np.float32, None, P, npix, opening_angle_deg=angle, chi_edges=edges)
    e2, = pp.upload_doubles(cone["e2"])
    geometries = {"box": dict(boxsize=BOX), "cone": dict(opening_angle_deg=angle, chi_edges=edges, e2=e2,
                                                          origin=(0.5 * BOX, 0.5 * BOX, -BOX))}
    rows = {}
    for order, shuffle in (("lattice order", False), ("shuffled", True)):
        pos = dev.synth_lattice_particles(side, side, BOX, shuffle=shuffle)
        for geometry, kw in geometries.items():
            c1 = cone["c1"] if geometry == "cone" else 0.0
            for window in ("ngp", "cic", "tsc"):
                acc = lambda: pp.plane_paint_sums(pos, mass, geometry, P, npix, window, sums=sums, counters=counters,
                                                  np_total=npart * (WARM + REPS + 1), vmax=1.0, **kw)

                def paint():
                    sums.zero_()
                    acc()
                    pp.plane_paint_finish(sums, mul, add, geometry, c1, out=out)
                sums.zero_()
                counters.zero_()
                med, lo, hi = median_ms(acc)
                outside, clipped, refused = (int(v) // (WARM + REPS) for v in counters.tolist())
                inside = npart - outside - refused
                atomic = 8 * SUPPORT[window] ** 2 * inside
                full, flo, fhi = median_ms(paint)
                name = f"{geometry} {window.upper()}"
                rows[(name, order)] = med
                emit(f"{order:<14} {name:<9} accumulate {med:9.3f} ms  ({lo:.3f} .. {hi:.3f})  {npart / med * 1e-6:7.2f} G particles/s  "
                     f"{inside / npart * 100:5.1f} % deposit ({clipped} clipped)  {atomic / (med * 1e-3) / 1e12:6.3f} TB/s atomic   "
                     f"paint {full:9.3f} ms  ({flo:.3f} .. {fhi:.3f})  {alg / 1e9:5.2f} GB algorithmic  "
                     f"{alg / (full * 1e-3) / PEAK * 100:5.1f} % of 8 TB/s")
        # the yardstick: float atomics into a 3D grid of side `side`
        grid = torch.zeros((side,) * 3, dtype=torch.float32, device=dev.device())
        med, lo, hi = median_ms(lambda: dev.paint(pos, mass, side, BOX, "cic", out=grid, method="direct", accumulate=True))
        emit(f"{order:<14} device.paint direct CIC into {side}^3 (float atomics, 4 bytes x 8 per particle): {med:9.3f} ms  "
             f"({lo:.3f} .. {hi:.3f})  {npart / med * 1e-6:7.2f} G particles/s  {32 * npart / (med * 1e-3) / 1e12:6.3f} TB/s atomic")
        del pos, grid
        torch.cuda.empty_cache()
    med, lo, hi = median_ms(lambda: pp.plane_paint_finish(sums, mul, add, "box", 0.0, out=out))
    cmed, clo, chi = median_ms(lambda: pp.plane_paint_finish(sums, mul, add, "cone", cone["c1"], out=out))
    fin = P * npix * npix * 12
    emit(f"finish alone (reads 8, writes 4 bytes per pixel, {fin / 1e9:.2f} GB): box {med:.3f} ms ({lo:.3f} .. {hi:.3f}) "
         f"{fin / (med * 1e-3) / PEAK * 100:.1f} % of 8 TB/s; cone {cmed:.3f} ms ({clo:.3f} .. {chi:.3f}) "
         f"{fin / (cmed * 1e-3) / PEAK * 100:.1f} % of 8 TB/s")
    emit("shuffled / lattice order, accumulate, same case:")
    for name in sorted({k[0] for k in rows}):
        emit(f"  {name:<9} {rows[(name, 'shuffled')] / rows[(name, 'lattice order')]:6.2f} x")
    if not small:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
