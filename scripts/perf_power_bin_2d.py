"""Timing of the (k, mu) / multipole binning pass (ast_power_bin_2d, Nmu = 5, poles (0, 2, 4)) against the 1-D shell
binning pass (ast_power_bin_1d) on the same random half spectrum in the same run: HIP events around the kernels (the
library's profile hooks), warm-up, median of the repeats.  Both passes read once the modes FFTPower keeps (1 <= |m| <
n/2, about half of the half spectrum: the shell is decided before the load) - "GB needed" counts those elements only;
the 2-D pass issues 1 + npoles LDS atomics per mode where the 1-D pass issues one.  Also the global-atomic variant
(ASTRILD_PK2D_LDS=0).
usage: python scripts/perf_power_bin_2d.py [--n 512] [--reps 11] > profiles/power_bin_2d_perf.txt"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from astrild_amd import _lib, device as dev

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
torch.cuda.set_device(0)
n, L, Nmu, poles = args.n, 1000.0, 5, (0, 2, 4)


def kernel_ms(fn, site, warmup=None, reps=None):
    """Median (and min, max) over the repeats of the HIP-event time of launch site ``site`` in one call of fn."""
    for _ in range(args.warmup if warmup is None else warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps if reps is None else reps):
        dev.profile_enable(True)
        fn()
        rep = dev.profile_report()
        dev.profile_enable(False)
        assert rep[site][0] == 1, rep
        times.append(rep[site][1])
    return statistics.median(times), min(times), max(times)


print(f"device: {torch.cuda.get_device_name(0)}   n {n}   Nmu {Nmu}   poles {poles}   warm-up {args.warmup}   reps {args.reps}"
      f"   LDS table fits: {_lib.lib().ast_power_bin_2d_lds_fits(n, Nmu, len(poles))}")
f = torch.arange(n, device="cuda")
f = torch.where(f > n // 2, f - n, f)
m2 = f[:, None, None] ** 2 + f[None, :, None] ** 2 + torch.arange(n // 2 + 1, device="cuda")[None, None, :] ** 2
kept = int(((m2 >= 1) & (m2 < (n // 2) ** 2)).sum())          # the integer rule; the float64 rule moves a few edge vectors
del m2
print(f"elements of the half spectrum: {n * n * (n // 2 + 1)}, of which kept (1 <= |m| < n/2): {kept}")
gen = torch.Generator(device="cuda").manual_seed(1)
for dtype in (torch.complex128, torch.complex64):
    real = torch.float64 if dtype == torch.complex128 else torch.float32
    spec = torch.view_as_complex(torch.randn((n, n, n // 2 + 1, 2), dtype=real, device="cuda", generator=gen))
    gb = kept * spec.element_size() / 1e9                       # what the passes have to read
    dev.shell_geometry(n, L)
    psum1 = torch.zeros(n // 2 - 1, dtype=torch.float64, device="cuda")
    base = kernel_ms(lambda: dev.power_bin_1d(spec, None, n, L, psum=psum1), "power_bin")
    print(f"{str(dtype):18s} {gb:5.2f} GB needed  power_bin_1d data pass            {base[0]:8.4f} ms  (min {base[1]:.4f}, max {base[2]:.4f})"
          f"  {gb / base[0]:6.2f} TB/s", flush=True)
    for los in (2, 0):
        dev.shell_geometry_2d(n, L, Nmu, los)
        psum = torch.zeros((n // 2 - 1, Nmu), dtype=torch.float64, device="cuda")
        polesum = torch.zeros((len(poles), n // 2 - 1), dtype=torch.float64, device="cuda")
        call = lambda: dev.power_bin_2d(spec, None, n, L, Nmu, los, poles, psum=psum, polesum=polesum)
        for label, env, site in (("LDS tables", None, "power_bin_2d"), ("global atomics", "0", "power_bin_2d_global")):
            if env is not None:
                if los != 2 or dtype != torch.complex128:     # every mode adds to one of ~2000 addresses: slow, once is enough
                    continue
                os.environ["ASTRILD_PK2D_LDS"] = env
            try:
                t = kernel_ms(call, site) if env is None else kernel_ms(call, site, warmup=1, reps=3)
            finally:
                os.environ.pop("ASTRILD_PK2D_LDS", None)
            print(f"{str(dtype):18s} {gb:5.2f} GB needed  power_bin_2d los {los} {label:15s}   {t[0]:8.4f} ms  (min {t[1]:.4f}, max {t[2]:.4f})"
                  f"  {gb / t[0]:6.2f} TB/s   2d / 1d = {t[0] / base[0]:.2f}", flush=True)
    del spec
