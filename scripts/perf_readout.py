"""Mesh readout (hutils.readout / ast_readout): 512^3 positions of device.synth_lattice_particles (float32) read from a
512^3 field - float32 and float64, CIC and TSC, 1 and 3 components - once in lattice order (neighbouring threads read
neighbouring cells) and once with shuffle=True (every thread somewhere else: the element-granular gather that leans on
L2 and the Infinity Cache).  Per case: the MEDIAN of REPS calls, each timed with its own pair of device events after WARM
warm-up calls, and the share of 8 TB/s that the ALGORITHMIC bytes - np (3 sizeof(pos) + C sizeof(R)) + n^3 C sizeof(R):
positions in, values out, the field once - would take in that time.  A gather moves more than that (a TSC stencil is
27 cells per particle); the share is the yardstick the grouped variant will be judged by, not a claim about traffic.
Writes profiles/readout_perf.txt.  --small: 128^3 / 128^3, nothing written (a rehearsal of the script itself)."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from astrild_amd import _lib, device as dev  # noqa: E402
from astrild_amd.particles.hutils import readout  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "readout_perf.txt")
WARM, REPS = 2, 10
PEAK = 8e12
BOX = 1000.0
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
    side = 128 if small else 512
    torch.cuda.set_device(0)
    emit(f"device: {torch.cuda.get_device_name(0)}   {side}^3 float32 positions, {side}^3 field, box {BOX:g}   warm-up {WARM}, "
         f"median of {REPS} calls (min .. max), one pair of device events per call   library {os.path.basename(_lib.LIB_PATH)}")
    emit("share = algorithmic bytes / time / 8 TB/s; algorithmic bytes = np (3 sizeof(pos) + C sizeof(R)) + n^3 C sizeof(R)")
    npart = side ** 3
    rows = {}
    for order, shuffle in (("lattice order", False), ("shuffled", True)):
        pos = dev.synth_lattice_particles(side, side, BOX, shuffle=shuffle)
        for dtype in (torch.float32, torch.float64):
            for ncomp in (1, 3):
                gen = torch.Generator(device=dev.device()).manual_seed(side + ncomp)
                shape = (side,) * 3 if ncomp == 1 else (side,) * 3 + (ncomp,)
                field = torch.randn(shape, dtype=dtype, device=dev.device(), generator=gen)
                out = torch.empty((npart,) if ncomp == 1 else (npart, ncomp), dtype=dtype, device=dev.device())
                esz = field.element_size()
                alg = npart * (3 * pos.element_size() + ncomp * esz) + side ** 3 * ncomp * esz
                for window in ("cic", "tsc"):
                    med, lo, hi = median_ms(lambda: readout(field, pos, BOX, window, out=out))
                    name = f"{window.upper()} {str(dtype)[6:]} C={ncomp}"
                    rows[(name, order)] = med
                    emit(f"{order:<14} {name:<18} {med:9.3f} ms  ({lo:.3f} .. {hi:.3f})  {alg / 1e9:6.2f} GB algorithmic  "
                         f"{alg / (med * 1e-3) / PEAK * 100:5.1f} % of 8 TB/s  {npart / med * 1e-6:7.2f} G positions/s")
                del field, out
                torch.cuda.empty_cache()
        del pos
        torch.cuda.empty_cache()
    emit("shuffled / lattice order, same case:")
    for name in sorted({k[0] for k in rows}):
        emit(f"  {name:<18} {rows[(name, 'shuffled')] / rows[(name, 'lattice order')]:6.2f} x")
    if not small:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
