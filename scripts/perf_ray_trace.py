"""Multi-plane ray tracing (ray_trace.bench_ray_trace, csrc/ray_trace.hip): one trace of 8 sources through 64 float32
planes of 4096^2 - per plane the potential (pad, R2C, Green's function, C2R) and the ray step, each between its own pair of
device events, medians over the planes behind the first; the step's share of 8 TB/s on its algorithmic bytes, 2 x 96 B of
state and 8 B of psi per ray.  Full and Born mode, pad 1 and 2; the noise is scaled so that the rays end up to half a pixel from where they started.  No pass or fail number is attached.
Writes profiles/ray_trace_perf.txt.  --small: 8 planes of 512^2, nothing written (a rehearsal)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from astrild_amd import _lib, ray_trace as rt  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "ray_trace_perf.txt")
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def main():
    small = "--small" in sys.argv
    P, npix, S = (8, 512, 4) if small else (64, 4096, 8)
    torch.cuda.set_device(0)
    emit(f"device: {torch.cuda.get_device_name(0)}   one trace of {S} sources through {P} float32 planes of {npix}^2, 5 degrees a "
         f"side   per plane one pair of device events around the potential and one around the step; median over planes "
         f"2 .. {P} (min .. max)   library {os.path.basename(_lib.LIB_PATH)}")
    emit("step bytes = (2 x 96 + 8) npix^2: the state read and written, psi read once; share = step bytes / step time / 8 TB/s")
    # plans and code objects; and the noise level at which the rays end up to half a pixel from where they started
    # (the displacement is linear in the planes to first order)
    rms = 0.5 / rt.bench_ray_trace(P, npix, 1)["max_shift_px"]
    emit(f"planes: Gaussian noise of standard deviation {rms:.4g} Mpc/h")
    for pad in (1, 2):
        for born in (False, True):
            r = rt.bench_ray_trace(P, npix, S, pad=pad, born=born, rms=rms)
            assert r["finite"]
            emit(f"pad {pad}  {'born' if born else 'full'}   potential {r['potential_ms']:8.3f} ms / plane  "
                 f"({r['potential_ms_range'][0]:.3f} .. {r['potential_ms_range'][1]:.3f})   step {r['step_ms']:8.3f} ms / plane  "
                 f"({r['step_ms_range'][0]:.3f} .. {r['step_ms_range'][1]:.3f})  {r['step_bytes'] / 1e9:5.2f} GB  "
                 f"{r['step_hbm_share'] * 100:5.1f} % of 8 TB/s   emit {r['emit_ms']:7.3f} ms / source   "
                 f"largest displacement {r['max_shift_px']:.3f} px")
    if not small:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
