"""Finite-difference divergence of a velocity grid (device.divergence / ast_grid_divergence): 512^3 and 1024^3 float32,
512^3 float64; the streaming kernel against the one-work-item-per-cell kernel (ASTRILD_DIVERGENCE_TILED=1 / 0), numpy's
edges against periodic=True.  Per case: ms per call from device events around REPS calls after WARM warm-up calls, the
kernel's own ms from ast_profile_report in a separate profiled call, and the effective rate = algorithmic bytes
(4 sizeof(T) cells: three components in, one value out) / time.  Yardsticks, in the same run: ast_stream_copy moving
the same number of bytes (2 sizeof(T) cells copied = as many read plus as many written); the same divergence composed
from torch slicing on the device (torch.gradient, torch.roll); np.gradient on the host at 256^3.
Writes profiles/grid_divergence_perf.txt.  --kernels-only: the stencil cases alone, nothing written."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from astrild_amd import _lib, device as dev  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "grid_divergence_perf.txt")
WARM, REPS = 3, 10
H = 1 / 500
CASES = ((512, torch.float32), (1024, torch.float32), (512, torch.float64))
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def event_ms(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPS):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / REPS


def kernel_ms(fn, prefix):
    dev.profile_enable(True)
    fn()
    torch.cuda.synchronize()
    split = dev.profile_report()
    dev.profile_enable(False)
    return {k: v[1] / v[0] for k, v in split.items() if k.startswith(prefix)}


def torch_divergence(v, h, periodic):
    if periodic:
        d = [(torch.roll(v[..., a], -1, a) - torch.roll(v[..., a], 1, a)) / (2.0 * h) for a in range(3)]
    else:
        d = [torch.gradient(v[..., a], spacing=h, dim=a, edge_order=2)[0] for a in range(3)]
    return (d[0] + d[1]) + d[2]


def stencil_cases(n, dtype, v, out, copy_ms=None):
    esz = v.element_size()
    alg = 4 * esz * n ** 3
    name = f"{n}^3 {str(dtype)[6:]}"
    res = {}
    for periodic in (False, True):
        for flag, kernel in (("1", "streaming"), ("0", "cell")):
            os.environ["ASTRILD_DIVERGENCE_TILED"] = flag
            fn = lambda: dev.divergence(v, H, periodic=periodic, out=out)      # noqa: E731
            ms = event_ms(fn)
            kern = kernel_ms(fn, "grid_divergence")
            res[(periodic, flag)] = ms
            frac = f"  {copy_ms / ms:5.2f} of the copy's rate" if copy_ms else ""
            emit(f"{name + ', ' + kernel + (', periodic' if periodic else ', edges'):<44} {ms:9.3f} ms/call  "
                 f"{alg / ms * 1e-9:7.3f} TB/s effective{frac}  " + "  ".join(f"{k} {t:.3f} ms" for k, t in sorted(kern.items())))
    os.environ["ASTRILD_DIVERGENCE_TILED"] = "1"
    return res


def main():
    kernels_only = "--kernels-only" in sys.argv
    torch.cuda.set_device(0)
    emit(f"device: {torch.cuda.get_device_name(0)}   warm-up {WARM}   reps {REPS}   spacing 1/500   times from device "
         f"events, kernel times from ast_profile_report   library {os.path.basename(_lib.LIB_PATH)}")
    L = _lib.lib()
    verdict = []
    for n, dtype in CASES:
        gen = torch.Generator(device=dev.device()).manual_seed(n)
        v = torch.randn((n, n, n, 3), dtype=dtype, device=dev.device(), generator=gen)
        out = torch.empty((n, n, n), dtype=dtype, device=v.device)
        esz = v.element_size()
        alg = 4 * esz * n ** 3
        name = f"{n}^3 {str(dtype)[6:]}"
        copy_ms = None
        if not kernels_only:
            half = alg // 2                               # bytes copied: read once, written once = alg bytes moved
            src, dst = v.view(-1), torch.empty(half // esz, dtype=dtype, device=v.device)
            copy_ms = event_ms(lambda: dev.check(L.ast_stream_copy(dev.ptr(dst), dev.ptr(src), half, 0, dev.stream())))
            emit(f"{name + ', ast_stream_copy of ' + f'{half / 1e9:.2f} GB':<44} {copy_ms:9.3f} ms/call  "
                 f"{alg / copy_ms * 1e-9:7.3f} TB/s  ({alg / 1e9:.2f} GB moved = the stencil's algorithmic bytes)")
            del dst
        res = stencil_cases(n, dtype, v, out, copy_ms)
        if kernels_only:
            continue
        for periodic in (False, True):
            os.environ["ASTRILD_DIVERGENCE_TILED"] = "1"
            ours = dev.divergence(v, H, periodic=periodic)
            theirs = torch_divergence(v, H, periodic)
            same = torch.equal(ours, theirs)
            worst = float((ours - theirs).abs().max())
            del ours, theirs
            ms = event_ms(lambda: torch_divergence(v, H, periodic))
            emit(f"{name + ', torch composition' + (', periodic' if periodic else ', edges'):<44} {ms:9.3f} ms/call  "
                 f"{alg / ms * 1e-9:7.3f} TB/s effective  streaming kernel {ms / res[(periodic, '1')]:.2f}x faster  "
                 f"(results {'bit equal' if same else f'differ by at most {worst:.3e}'})")
            verdict.append((name, periodic, res[(periodic, "1")], res[(periodic, "0")], ms))
        del v, out
        torch.cuda.empty_cache()
    if kernels_only:
        return
    for name, periodic, tiled, cell, composed in verdict:
        emit(f"{name + (', periodic' if periodic else ', edges'):<44} streaming {'faster' if tiled < cell else 'SLOWER'} than "
             f"cell ({cell / tiled:.2f}x), {'faster' if tiled < composed else 'SLOWER'} than the torch composition "
             f"({composed / tiled:.2f}x)")
    n = 256
    host = np.random.default_rng(1).standard_normal((n, n, n, 3)).astype(np.float32)
    t0 = time.perf_counter()
    ref = (np.gradient(host[..., 0], H, axis=0, edge_order=2) + np.gradient(host[..., 1], H, axis=1, edge_order=2)
           + np.gradient(host[..., 2], H, axis=2, edge_order=2))
    cpu = time.perf_counter() - t0
    assert np.array_equal(dev.to_numpy(dev.divergence(host, H)), ref)
    emit(f"{'CPU: np.gradient x 3, 256^3 float32 (host)':<44} {cpu * 1e3:9.1f} ms  (one process; the device result at 256^3 "
         f"is bit equal)")
    emit(f"{'CPU: np.gradient x 3, scaled to 1024^3':<44} {cpu * 64:9.1f} s    (EXTRAPOLATION: 64 x the cells of 256^3)")
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
