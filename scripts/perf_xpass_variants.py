"""What the two strided passes of the fused power pipeline pay for work the result does not need, at side n (default
1024): per-site times of `fft_tile.c2c` (k_y pass), `fft_tile.c2c_power` (last pass + binning) and `fft_tile.shell_reduce`
with each change switched back - the Nyquist column (AST_FFT_NYQ_COLUMN=1: the k_y pass's 17th tile), the epilogue
steps beyond the sphere (AST_FFT_NO_EPI_SKIP=1), one shell table instead of one per column lane
(AST_FFT_SHELL_ATOMICS=1) - and with all three, which is the pass as it was.  HIP events, best of `reps` after a warm-up.

The cost of the epilogue's LDS atomics is the difference to two builds of fft_tile.hip, one process per build
(scripts/build_variants.sh noatom fft_tile.hip -DXPASS_ATOMICS=0, ... uniq fft_tile.hip -DXPASS_ATOMICS=2; run with
ASTRILD_HIP_LIB=astrild_amd/libastrild_hip_<tag>.so): no atomics at all, and every lane of a wave at its own address
(read their "one shell table" rows: the ablations sit in the one-table epilogue).
Their shell sums are wrong on purpose; only the times count."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from astrild_amd import device as dev
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
SITES = ("fft_tile.c2c", "fft_tile.c2c_power", "fft_tile.shell_reduce")
g = torch.Generator(device="cuda").manual_seed(1)
grid = torch.randn((n, n, n), dtype=torch.float32, device="cuda", generator=g)
def sites(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        dev.power_sums_fused(grid, 1000.0); torch.cuda.synchronize()
        best = {s: float("inf") for s in SITES}
        for _ in range(reps):
            dev.profile_enable(True)             # (re-arming clears the sites)
            dev.power_sums_fused(grid, 1000.0)
            torch.cuda.synchronize()
            rep = dev.profile_report()
            for s in SITES:
                calls, ms = rep[s]
                best[s] = min(best[s], ms / calls)
        dev.profile_enable(False)
        return best
    finally:
        for k, v in old.items():
            if v is None: del os.environ[k]
            else: os.environ[k] = v
A, B, D = {"AST_FFT_NYQ_COLUMN": "1"}, {"AST_FFT_NO_EPI_SKIP": "1"}, {"AST_FFT_SHELL_ATOMICS": "1"}
cases = [("default", {}), ("Nyquist column kept", A), ("epilogue skip off", B), ("one shell table", D),
         ("one table, skip off", {**B, **D}), ("none (the passes as they were)", {**A, **B, **D}), ("default again", {})]
print(f"lib={os.environ.get('ASTRILD_HIP_LIB', 'default')} n={n} best of {reps}, ms", flush=True)
for name, env in cases:
    t = sites(env)
    print(f"  {name:32s} " + "  ".join(f"{s.split('.')[1]} {t[s]:.4f}" for s in SITES), flush=True)
