"""The tunnels void finder (device.tunnels_voids / ast_tunnels_find): uniform random tracers, 10^4 on a 4096^2 map, 10^5
on 8192^2 and 10^6 on 16384^2, the peaks of a smoothed 1024^2 Gaussian field, and a clustered set (3000 tracers in one
64^2 corner of a 2048^2 map plus 30 spread over the rest).  Per input: the median wall ms of a call with device tensors
in and out and with numpy arrays in and out (argument checks, uploads, kernels, the sort of the records, the copy back),
the kernels' ms (HIP events of the library's timers, one extra call), voids per second of the device call, and beside it
the tests' oracle (scipy's Qhull Delaunay triangulation merged by circle, one core) on the same host, once, with the
triangulation alone.  The records of the two are compared.  Writes profiles/tunnels_perf.txt."""
import os
import sys
import time

import numpy as np
import torch
from scipy.spatial import Delaunay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from astrild_amd import device as dev  # noqa: E402
from tests import tunnels_oracle as orc  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tunnels_perf.txt")
REPS = 5
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def distinct(rs, n, npix):
    if npix * npix < 4 * n:
        p = rs.permutation(npix * npix)[:n]
    else:
        p = np.unique(rs.randint(0, npix * npix, n + n // 4 + 16))
        rs.shuffle(p)
        p = p[:n]
        assert len(p) == n
    return np.stack([p % npix, p // npix], axis=1)


def inputs():
    rs = np.random.RandomState(1)
    yield "uniform 1e4 on 4096^2", distinct(rs, 10 ** 4, 4096), 4096
    yield "uniform 1e5 on 8192^2", distinct(rs, 10 ** 5, 8192), 8192
    yield "uniform 1e6 on 16384^2", distinct(rs, 10 ** 6, 16384), 16384
    from scipy.ndimage import gaussian_filter
    x, y = orc.strict_maxima(gaussian_filter(np.random.RandomState(3).standard_normal((1024, 1024)), 2.0, mode="wrap"))
    yield "peaks of a smoothed 1024^2 field", np.stack([x, y], axis=1), 1024
    far = distinct(rs, 60, 2048)
    far = far[(far[:, 0] >= 64) | (far[:, 1] >= 64)][:30]
    yield "clustered: 3000 in 64^2 + 30 on 2048^2", np.concatenate([distinct(rs, 3000, 64), far]), 2048


def median_ms(f):
    f()                                                         # warm-up
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def case(label, P, npix, oracle=True):
    x, y = np.ascontiguousarray(P[:, 0]), np.ascontiguousarray(P[:, 1])
    xd, yd = dev.as_device(x, torch.int32), dev.as_device(y, torch.int32)
    ms_dev = median_ms(lambda: dev.tunnels_voids(xd, yd, npix))
    ms_np = median_ms(lambda: dev.tunnels_voids(x, y, npix))
    dev.profile_enable(True)
    rec = dev.tunnels_voids(xd, yd, npix)
    torch.cuda.synchronize()
    split = {k: v for k, v in dev.profile_report().items() if k.startswith("tunnels")}
    dev.profile_enable(False)
    kern = sum(v[1] for v in split.values())
    rec = dev.to_numpy(rec)
    head = (f"{label:<40} N {len(P):>8}  voids {len(rec):>8}  device in/out {ms_dev:9.3f} ms/call  numpy in/out "
            f"{ms_np:9.3f} ms/call  kernels {kern:9.3f} ms ("
            + ", ".join(f"{k} {v[1]:.3f}" for k, v in sorted(split.items()))
            + f")  {len(rec) / (ms_dev * 1e-3):.3e} voids/s")
    if not oracle:
        emit(head)
        return rec
    t0 = time.perf_counter()
    Delaunay(P.astype(np.float64))
    qhull = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    want = orc.circles(P, npix)
    cpu = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(rec, want), label
    emit(head + f"  |  CPU oracle {cpu:9.1f} ms (Qhull alone {qhull:.1f} ms)  "
         f"oracle / device call {cpu / ms_dev:.2f}x  Qhull / device call {qhull / ms_dev:.2f}x")
    return rec


def main():
    torch.cuda.set_device(0)
    emit(f"device: {torch.cuda.get_device_name(0)}   median of {REPS} calls after a warm-up   records equal to the oracle")
    Delaunay(np.random.RandomState(0).rand(100, 2))             # Qhull's first call
    for label, P, npix in inputs():
        rec = case(label, P, npix)
        if len(P) == 10 ** 4:
            os.environ["ASTRILD_TUNNELS_CELLS"] = "0"
            one = case(label + ", one cell", P, npix, oracle=False)
            os.environ.pop("ASTRILD_TUNNELS_CELLS")
            assert np.array_equal(one, rec)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
