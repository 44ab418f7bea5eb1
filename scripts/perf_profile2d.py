"""Radial profiles on a 4096^2 float64 map (device.annulus_profiles / ast_profile2d): 10^4 objects with rad_pix uniform
in [5, 50], extend 3, 20 bins, alone and with one rad_pix = 600 object; bands against ASTRILD_PROFILE_BANDS=0 (one work
item per object).  Per call: wall ms (host thresholds + uploads + kernels), the two kernels' ms (HIP events), pixels
read per second, and the host threshold time on its own.  CPU baselines: the tests' vectorised numpy oracle on the full
catalogue, and a per-pixel Python restatement of the reference's loop on 100 objects, scaled up (an extrapolation).
Writes profiles/profile2d_perf.txt."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from astrild_amd import device as dev  # noqa: E402
from astrild_amd.profiles import profile_2d as p2d  # noqa: E402
from tests import profile2d_oracle as orc  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "profile2d_perf.txt")
N, EXT, NB, REPS = 4096, 3.0, 20, 5
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def catalogue(big):
    rs = np.random.RandomState(7)
    r = rs.randint(5, 51, 10000)
    x = rs.randint(160, N - 160, 10000)
    y = rs.randint(160, N - 160, 10000)
    if big:
        r, x, y = np.append(r, 600), np.append(x, 2048), np.append(y, 2048)
    return x, y, r


def case(label, t, x, y, r, bands):
    os.environ["ASTRILD_PROFILE_BANDS"] = "1" if bands else "0"
    s, c = dev.annulus_profiles(t, x, y, r, EXT, NB)          # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        s, c = dev.annulus_profiles(t, x, y, r, EXT, NB)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / REPS * 1e3
    dev.profile_enable(True)
    dev.annulus_profiles(t, x, y, r, EXT, NB)
    torch.cuda.synchronize()
    split = dev.profile_report()
    dev.profile_enable(False)
    px = int(dev.to_numpy(c).sum())
    kern = sum(v[1] for k, v in split.items() if k.startswith("profile2d"))
    emit(f"{label:<44} {ms:9.3f} ms/call  {px / (ms * 1e-3):.3e} px/s  ({px:.4e} px read)  kernels {kern:.3f} ms "
         f"({px / (kern * 1e-3):.3e} px/s)  " + "  ".join(f"{k} {v[1]:.3f}" for k, v in sorted(split.items())))
    return dev.to_numpy(s), dev.to_numpy(c), px


def host_thresholds(label, x, y, r):
    t0 = time.perf_counter()
    for _ in range(REPS):
        p2d.annulus_geometry((N, N), x, y, r, EXT, NB)
    emit(f"{label:<44} {(time.perf_counter() - t0) / REPS * 1e3:9.3f} ms  (host thresholds + bounds, in the call above)")


def per_pixel_python(skymap, x, y, r):
    """The reference's loop restated: one Python iteration per pixel of the (2R)^2 square."""
    de = EXT / NB
    for xi, yi, ri in zip(x, y, r):
        R = int(np.ceil(ri * EXT))
        acc = np.zeros(NB)
        for a in range(-R, R):
            for b in range(-R, R):
                e = int(np.sqrt(a * a + b * b) / ri / de)
                if e < NB:
                    acc[e] += skymap[yi + a, xi + b]


def main():
    torch.cuda.set_device(0)
    emit(f"device: {torch.cuda.get_device_name(0)}   reps {REPS}   map {N}^2 float64   extend {EXT}   {NB} bins")
    skymap = np.random.RandomState(1).standard_normal((N, N))
    t = dev.as_device(skymap)
    res = {}
    for big in (False, True):
        x, y, r = catalogue(big)
        name = "1e4 objects r 5-50" + (" + one r=600" if big else "")
        res[(big, 1)] = case(name + ", bands", t, x, y, r, True)
        res[(big, 0)] = case(name + ", one item/object", t, x, y, r, False)
        host_thresholds(name + ", host part", x, y, r)
        assert np.array_equal(res[(big, 1)][1], res[(big, 0)][1])
    for big in (False, True):
        b, o = res[(big, 1)], res[(big, 0)]
        emit(f"bands vs one item per object{' (+ r=600)' if big else ''}: counts equal, max |sum diff| "
             f"{np.max(np.abs(b[0] - o[0])):.3e}")
    os.environ["ASTRILD_PROFILE_BANDS"] = "1"
    x, y, r = catalogue(False)
    t0 = time.perf_counter()
    _, os_, oc, _ = orc.from_map(x, y, r, skymap, EXT, NB)
    cpu = time.perf_counter() - t0
    emit(f"{'CPU: numpy oracle (tests), full 1e4 catalogue':<44} {cpu * 1e3:9.1f} ms  (one process)")
    assert np.array_equal(oc, res[(False, 1)][1])
    sub = slice(0, 100)
    px_sub = int(oc[sub].sum())
    sq_sub = int(np.sum((2 * np.ceil(r[sub] * EXT)) ** 2))
    sq_all = int(np.sum((2 * np.ceil(r * EXT)) ** 2))
    t0 = time.perf_counter()
    per_pixel_python(skymap, x[sub], y[sub], r[sub])
    py = time.perf_counter() - t0
    emit(f"{'CPU: per-pixel Python loop, 100 objects':<44} {py * 1e3:9.1f} ms  ({py / sq_sub * 1e6:.3f} us per square "
         f"pixel, {px_sub} px read)")
    emit(f"{'CPU: per-pixel Python loop, extrapolated':<44} {py / sq_sub * sq_all:9.1f} s    (EXTRAPOLATION to the "
         f"1e4 catalogue: {sq_all:.3e} square pixels)")
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
