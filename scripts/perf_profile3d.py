"""Spherical profiles of 10^7 particles around 10^5 centres (device.sphere_profiles / ast_profile3d_*): a clustered
float32 catalogue in a periodic box of 1000, radii lognormal around 1, 20 log bins 0.05 .. 3, with velocities (four
moments) and without.  Per call: wall ms (host work list + uploads + kernels) and the kernels' ms by launch site (HIP
events).  Rows: the cell grid at three cell caps against ASTRILD_PROFILE3D_CELLS=0 (one cell: every centre reads every
particle; measured on 100 centres, the full catalogue is an extrapolation), the split into runs of z layers against
ASTRILD_PROFILE3D_LAYERS=0 on a catalogue with one very large centre (R = 50), the membership mode, and the tests' numpy
oracle on one core (5 centres, the full catalogue is an extrapolation).  Writes profiles/profile3d_perf.txt."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from astrild_amd import device as dev  # noqa: E402
from tests import profile3d_oracle as orc  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "profile3d_perf.txt")
NP, NC, L, REPS = 10 ** 7, 10 ** 5, 1000.0, 3
EDGES = np.logspace(np.log10(0.05), np.log10(3.0), 21)
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def catalogue():
    rng = np.random.default_rng(5)
    nblob = 20000
    blobs = rng.uniform(0.0, L, (nblob, 3)).astype(np.float32)
    n_cl = NP * 7 // 10
    pos = np.concatenate([blobs[rng.integers(0, nblob, n_cl)] + rng.normal(0.0, 1.0, (n_cl, 3)).astype(np.float32),
                          rng.uniform(0.0, L, (NP - n_cl, 3)).astype(np.float32)])
    pos = np.mod(pos, np.float32(L)).astype(np.float32)
    pos = np.minimum(pos, np.float32(L))
    vel = rng.normal(0.0, 300.0, (NP, 3)).astype(np.float32)
    centres = np.concatenate([blobs.astype(np.float64)[: NC // 5], pos[rng.choice(NP, NC * 3 // 10, replace=False)],
                              rng.uniform(0.0, L, (NC - NC // 5 - NC * 3 // 10, 3))]).astype(np.float64)
    radii = rng.lognormal(0.0, 0.4, NC)
    return pos[rng.permutation(NP)], vel, centres, radii


def case(label, pos, centres, radii, env=None, **kw):
    for k in ("ASTRILD_PROFILE3D_CELLS", "ASTRILD_PROFILE3D_LAYERS"):
        os.environ[k] = (env or {}).get(k, "1")
    c, m = dev.sphere_profiles(pos, centres, radii, EDGES, **kw)              # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        c, m = dev.sphere_profiles(pos, centres, radii, EDGES, **kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / REPS * 1e3
    dev.profile_enable(True)
    dev.sphere_profiles(pos, centres, radii, EDGES, **kw)
    torch.cuda.synchronize()
    split = {k: v for k, v in dev.profile_report().items() if k.startswith("profile3d")}
    dev.profile_enable(False)
    kern = sum(v[1] for v in split.values())
    binned = int(c.sum().item())
    emit(f"{label:<58} {ms:10.3f} ms/call  kernels {kern:10.3f} ms  ({binned:.4e} binned)  "
         + "  ".join(f"{k[10:]} {v[1]:.3f}" for k, v in sorted(split.items())))
    for k in ("ASTRILD_PROFILE3D_CELLS", "ASTRILD_PROFILE3D_LAYERS"):
        os.environ[k] = "1"
    return dev.to_numpy(c), dev.to_numpy(m), kern


def main():
    torch.cuda.set_device(0)
    emit(f"device: {torch.cuda.get_device_name(0)}   reps {REPS}   Np {NP:.0e} float32   Nc {NC:.0e}   box {L}   "
         f"20 bins 0.05..3   occupancy target {dev.PROFILE3D_OCCUPANCY}   layers/item "
         f"{dev._lib.lib().ast_profile3d_layers()}")
    pos_h, vel_h, centres, radii = catalogue()
    pos, vel = dev.as_device(pos_h), dev.as_device(vel_h)
    base = {}
    for cap in (1 << 18, 1 << 21, 1 << 24):
        d = dev.profile3d_dims(NP, cap)
        base[cap] = case(f"grid {d}^3 (cap 2^{cap.bit_length() - 1}), counts + sum w", pos, centres, radii, boxsize=L,
                         cell_cap=cap)
        case(f"grid {d}^3 (cap 2^{cap.bit_length() - 1}), four moments", pos, centres, radii, boxsize=L, vel=vel,
             cell_cap=cap)
    for cap in (1 << 18, 1 << 24):
        assert np.array_equal(base[cap][0], base[1 << 21][0])
    one = case("one cell (CELLS=0), 100 centres, counts + sum w", pos, centres[:100], radii[:100],
               env={"ASTRILD_PROFILE3D_CELLS": "0"}, boxsize=L)
    assert np.array_equal(one[0], base[1 << 21][0][:100])
    emit(f"{'one cell (CELLS=0), EXTRAPOLATED to 1e5 centres':<58} {one[2] * NC / 100 / 1e3:10.1f} s   (EXTRAPOLATION: "
         f"1000 x the 100-centre kernels)")
    big_c, big_r = centres.copy(), radii.copy()
    big_c[NC // 2], big_r[NC // 2] = (500.0, 500.0, 500.0), 50.0
    split = case("+ one centre R = 50, layers split, four moments", pos, big_c, big_r, boxsize=L, vel=vel)
    whole = case("+ one centre R = 50, one item per centre (LAYERS=0)", pos, big_c, big_r,
                 env={"ASTRILD_PROFILE3D_LAYERS": "0"}, boxsize=L, vel=vel)
    assert np.array_equal(split[0], whole[0])
    emit(f"layers split vs one item per centre: counts equal ({int(split[0][NC // 2].sum())} in the large centre), max "
         f"|moment diff| / max |moment| = {np.max(np.abs(split[1] - whole[1])) / np.max(np.abs(whole[1])):.3e}")
    # membership mode: the particles sorted by nearest blob would be a halo finder's job; here contiguous segments
    n_mem = np.full(NC, NP // NC, dtype=np.int64)
    seg = np.stack([np.arange(NC, dtype=np.int64) * (NP // NC), n_mem], axis=1)
    case("membership mode, 100 members each, open, four moments", pos, centres, radii, vel=vel, segments=seg)
    sub = 5
    t0 = time.perf_counter()
    oc, _, _ = orc.profiles(pos_h, centres[:sub], radii[:sub], EDGES, boxsize=L)
    cpu = time.perf_counter() - t0
    assert np.array_equal(oc, base[1 << 21][0][:sub])
    emit(f"{'CPU: numpy oracle (tests), 5 centres, one core':<58} {cpu * 1e3:10.1f} ms  ({cpu / sub * 1e3:.1f} ms per "
         f"centre)")
    emit(f"{'CPU: numpy oracle, EXTRAPOLATED to 1e5 centres':<58} {cpu / sub * NC:10.1f} s   (EXTRAPOLATION)")
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
