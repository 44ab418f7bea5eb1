"""What the y split of the fused power pipeline moves between its three FFT passes, at side n (default 1024): per-site
times of `fft_tile.rows_r2c` (z pass), `fft_tile.c2c` (k_y pass) and `fft_tile.c2c_power` (last pass + binning) with the
route on and off (AST_FFT_YSPLIT unset / 0 at side 1024; 1 / unset below), on a random grid and on a grid painted with
defer_fold=True (the pipeline's z pass: halo fold and low-k z sums).  HIP events, best of `reps` after a warm-up.

The z pass's epilogue mapping and the k_y pass's tile width are compile-time choices of fft_tile.hip: one process per
build (scripts/build_variants.sh c64 fft_tile.hip -DYSPLIT_C=64, ... pairs fft_tile.hip -DYSPLIT_EPI_PAIRS=1, ... pairs64
fft_tile.hip -DYSPLIT_EPI_PAIRS=1 -DYSPLIT_C=64; run with ASTRILD_HIP_LIB=astrild_amd/libastrild_hip_<tag>.so)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from astrild_amd import device as dev
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
SITES = ("fft_tile.rows_r2c", "fft_tile.c2c", "fft_tile.c2c_power")
ON = {} if n == 1024 else {"AST_FFT_YSPLIT": "1"}
OFF = {"AST_FFT_YSPLIT": "0"}
def sites(env, grid, halo):
    os.environ.pop("AST_FFT_YSPLIT", None)
    os.environ.update(env)
    dev.power_sums_fused(grid, 1000.0, halo=halo); torch.cuda.synchronize()
    best = {s: float("inf") for s in SITES}
    for _ in range(reps):
        dev.profile_enable(True)             # (re-arming clears the sites)
        dev.power_sums_fused(grid, 1000.0, halo=halo)
        torch.cuda.synchronize()
        rep = dev.profile_report()
        for s in SITES:
            calls, ms = rep[s]
            best[s] = min(best[s], ms / calls)
    dev.profile_enable(False)
    os.environ.pop("AST_FFT_YSPLIT", None)
    return best
print(f"lib={os.environ.get('ASTRILD_HIP_LIB', 'default')} n={n} best of {reps}, ms", flush=True)
g = torch.Generator(device="cuda").manual_seed(1)
grid = torch.randn((n, n, n), dtype=torch.float32, device="cuda", generator=g)
for name, env in (("random grid, split off", OFF), ("random grid, split on", ON), ("random grid, split off", OFF), ("random grid, split on", ON)):
    t = sites(env, grid, None)
    print(f"  {name:28s} " + "  ".join(f"{s.split('.')[1]} {t[s]:.4f}" for s in SITES) + f"  sum {sum(t.values()):.4f}", flush=True)
del grid
pos = dev.synth_lattice_particles(n, n, 1000.0, seed=11, dtype=torch.float32)
grid, halo = dev.paint(pos, None, n, 1000.0, "cic", method=dev.auto_paint_method(pos.shape[0], n, n, "cic"), defer_fold=True, offset="mean")
del pos
for name, env in (("deferred fold, split off", OFF), ("deferred fold, split on", ON), ("deferred fold, split off", OFF), ("deferred fold, split on", ON)):
    t = sites(env, grid, halo)
    print(f"  {name:28s} " + "  ".join(f"{s.split('.')[1]} {t[s]:.4f}" for s in SITES) + f"  sum {sum(t.values()):.4f}", flush=True)
