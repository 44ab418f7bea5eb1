"""Timing of the Gaussian-random-field generator: the fill kernel (ast_grf_spectrum into a spectrum allocated beforehand)
and the whole call (lensing.gaussian_random_map: table upload, allocation, fill, batched C2R) at 4096^2 and 8192^2 maps,
1 and 8 realisations, with two tables: one that reaches past the corner of the half plane, so that every pixel is drawn,
and a CMB-like one of 10^4 entries, beyond which a pixel is zero and draws nothing (at 20 degrees a side that is most
of them).  HIP events on the stream, one warm-up, then the median of --reps calls.  Beside them two yardsticks: ast_stream_copy writing the fill kernel's 16 B per pixel in the same run
(write only, and the copy rate), and the numpy oracle of the tests at 2048^2 on the host (reported, nothing depends on it).
usage: python scripts/perf_grf.py [--reps R] [--out FILE] [--oracle-npix N]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from astrild_amd import _lib, device as dev, lensing
from tests import grf_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--oracle-npix", type=int, default=2048)
args = ap.parse_args()
torch.cuda.set_device(0)
ANGLE_DEG = 20.0


def table_of(entries):
    return 1e-9 / (np.arange(entries, dtype=np.float64) + 50.0) ** 2

lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def event_ms(call):
    """One warm-up, then the median (and min, max) of args.reps calls between device events."""
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), min(times), max(times)


emit(f"device: {torch.cuda.get_device_name(0)}   reps {args.reps}   side {ANGLE_DEG} deg   no lmax")
L = _lib.lib()
for npix, entries in ((4096, None), (8192, None), (4096, 10000), (8192, 10000)):
    l = orc.pixel_l(npix, np.deg2rad(ANGLE_DEG))
    CL = table_of(int(l.max()) + 2 if entries is None else entries)
    drawn = float((l <= len(CL) - 1).mean())
    del l
    table = dev.as_device(CL)
    emit(f"--- {npix}^2, table of {len(CL)} entries: {100 * drawn:.1f} % of the pixels drawn")
    for nreal in (1, 8):
        nh = npix // 2 + 1
        pixels = nreal * npix * nh
        nbytes = 16 * pixels
        spec = torch.empty((nreal, npix, nh), dtype=torch.complex128, device="cuda")
        src = torch.empty((nreal, npix, nh), dtype=torch.complex128, device="cuda")
        fill = event_ms(lambda: _lib.check(L.ast_grf_spectrum(dev.ptr(spec), npix, float(np.deg2rad(ANGLE_DEG)), dev.ptr(table),
                                                              len(CL), float("inf"), 34077, 0, nreal, dev.stream())))
        write = event_ms(lambda: _lib.check(L.ast_stream_copy(dev.ptr(spec), dev.ptr(src), nbytes, 2, dev.stream())))
        copy = event_ms(lambda: _lib.check(L.ast_stream_copy(dev.ptr(spec), dev.ptr(src), nbytes, 0, dev.stream())))
        del src
        out = torch.empty((npix, npix) if nreal == 1 else (nreal, npix, npix), dtype=torch.float64, device="cuda")
        whole = event_ms(lambda: lensing.gaussian_random_map(npix, ANGLE_DEG, CL, 34077, nreal=nreal, out=out))
        emit(f"{npix}^2 x {nreal}: fill {fill[0]:8.3f} ms (min {fill[1]:.3f}, max {fill[2]:.3f})  {pixels / fill[0] / 1e6:7.2f} Gpixel/s  "
             f"{nbytes / fill[0] / 1e9:6.3f} TB/s stored = {write[0] / fill[0]:.3f} of write-only ({write[0]:.3f} ms, "
             f"{nbytes / write[0] / 1e9:.2f} TB/s), {copy[0] / 2 / fill[0]:.3f} of the copy rate ({2 * nbytes / copy[0] / 1e9:.2f} TB/s)   "
             f"whole call {whole[0]:8.3f} ms (min {whole[1]:.3f}, max {whole[2]:.3f})")
        del spec, out
        torch.cuda.empty_cache()

n = args.oracle_npix
CL = table_of(int(orc.pixel_l(n, np.deg2rad(ANGLE_DEG)).max()) + 2)
t0 = time.perf_counter()
orc.spectrum(n, np.deg2rad(ANGLE_DEG), CL, 34077)
t_or = time.perf_counter() - t0
emit(f"host: numpy oracle spectrum at {n}^2, every pixel drawn: {t_or * 1e3:.0f} ms = {n * (n // 2 + 1) / t_or / 1e6:.2f} Mpixel/s (one core, reported only)")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
