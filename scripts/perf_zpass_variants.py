"""What the z pass of the fused power pipeline pays for its two side jobs, at side n (default 1024), on a grid painted with
defer_fold=True: the plain row pass, the pass with the low-k z sums, the pipeline's z pass with the halo fold only
(AST_LOWK_SEPARATE=1) and with fold and z sums (the default).  HIP events, best of `reps` after a warm-up."""
import ctypes as ct, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from astrild_amd import device as dev, _lib
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
L = _lib.lib()
pos = dev.synth_lattice_particles(n, n, 1000.0, seed=11, dtype=torch.float32)
grid, halo = dev.paint(pos, None, n, 1000.0, "cic", method=dev.auto_paint_method(pos.shape[0], n, n, "cic"), defer_fold=True, offset="mean")
del pos
pitch = n // 2 + 1
spec = torch.empty((n * n, pitch), dtype=torch.complex64, device="cuda")
lowz = torch.empty(n * n * 7, dtype=torch.complex128, device="cuda")
def best(fn):
    fn(); torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return min(a.elapsed_time(b) for a, b in ev)
def plain():
    _lib.check(L.ast_fft_tile_rows_r2c(dev.ptr(grid), dev.ptr(spec), _lib.F32, n, n * n, n, pitch, 1.0, dev.stream()), "rows_r2c")
def sums():
    _lib.check(L.ast_fft_tile_rows_r2c_lowz(dev.ptr(grid), dev.ptr(spec), _lib.F32, n, n * n, n, pitch, 1.0, dev.ptr(lowz), dev.stream()), "rows_r2c_lowz")
def site(name="fft_tile.rows_r2c"):          # best of `reps` pipeline calls at one profile site
    dev.power_sums_fused(grid, 1000.0, halo=halo); torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        dev.profile_enable(True)             # (re-arming clears the sites)
        dev.power_sums_fused(grid, 1000.0, halo=halo)
        torch.cuda.synchronize()
        calls, ms = dev.profile_report()[name]
        t.append(ms / calls)
    dev.profile_enable(False)
    return min(t)
res = {"plain": best(plain), "z sums": best(sums)}
del spec, lowz
os.environ["AST_LOWK_SEPARATE"] = "1"
res["fold"] = site()
del os.environ["AST_LOWK_SEPARATE"]
res["fold + z sums"] = site()
gb = (n ** 3 * 4 + n * n * pitch * 8) / 1e9
for k, v in res.items():
    print(f"n={n} z pass, {k:14s}: {v:.3f} ms  (+{v - res['plain']:.3f} over plain; {gb / v:.2f} TB/s of the grid and spectrum bytes)", flush=True)
