"""Inputs that the ray tracer's tests share (tests/test_gpu_ray_trace.py on the device, tests/test_ray_step_host.py for the
host build of csrc/ray_step.h, tests/test_ray_trace_reference.py for the extended-precision reference): states whose rays
land where the index arithmetic can go wrong.  numpy only; nothing here imports the product."""
import numpy as np

H = 2.0 ** -10                                # a power of two: k * H and (k * H) / H are exact
CHI = (733.1, 1711.3, 2950.7, 3333.3)         # two planes behind one another and a source; no powers of two
RAY_BX, RAY_BY = 64, 4                        # the step kernel's workgroup: 4 rows of 64 rays (csrc/ray_trace.hip)
GEOMETRY_SHAPES = [(64, 64), (65, 65), (130, 130), (67, 134), (128, 256)]            # (npix, m)
TINY_SHAPES = [(npix, m) for m in range(1, 5) for npix in range(1, m + 1)]


def preset_state(npix, m, h, seed):
    """A random state whose first rows are set so that, after the advance from chi 512 to 1024 (d <- (d + s) / 2,
    exact), rays land exactly on nodes, at negative positions and beyond the seam of the m-grid."""
    rng = np.random.default_rng(seed)
    st = np.empty((12, npix, npix))
    st[:4] = rng.normal(0.0, 1.5 * h, size=(4, npix, npix))
    st[4:] = rng.normal(0.0, 0.2, size=(8, npix, npix))
    st[2:4, :4] = 0.0
    st[0, 0], st[1, 0] = 2 * -2.5 * h, 2 * 1.25 * h                     # p1 = 0 - 2.5: node -3, wraps to m - 3
    st[0, 1], st[1, 1] = 2 * 2.0 * h, 2 * -3.0 * h                      # whole pixels: f = 0 on both axes
    st[0, 2], st[1, 2] = 2 * (m - 2 + 0.75) * h, 2 * (m + 0.5) * h      # p1 = 2 + m - 1.25, p2 = j + m + 0.5: past the seam
    st[0, 3], st[1, 3] = 0.0, 2 * -(npix - 0.0) * h                     # p2 = j - npix: negative whole pixels
    return st


def landing(st, h, chi_prev, chi_k):
    """Where the rays of ``st`` meet the plane at chi_k, in nodes, with the roundings of the contract."""
    d1 = (chi_prev * st[0] + (chi_k - chi_prev) * st[2]) / chi_k
    d2 = (chi_prev * st[1] + (chi_k - chi_prev) * st[3]) / chi_k
    n = st.shape[1]
    return np.arange(n)[:, None] + d1 / h, np.arange(n)[None, :] + d2 / h


def wild_state(h):
    """``preset_state(16, 16, h, 12)`` with displacements no index survives unclamped - 1e300, 2^31 and 2^40 pixels, Inf,
    NaN - and the edges of the clamp and of the number format: -0.0, the smallest subnormal, +-(2^30 +- 1) pixels (s = 0
    and d doubled there, so that the advance from 512 to 1024 lands them exactly).  Returns the state and the mask of the
    rays whose input is finite, i.e. where the oracle is defined."""
    st = preset_state(16, 16, h, 12)
    st[0, 5, :4] = [1e300, -1e300, 2.0 ** 31 * h, -2.0 ** 40 * h]
    st[1, 6, :4] = [np.inf, -np.inf, np.nan, 1e300]
    edge = [-0.0, 5e-324, 2 * (2.0 ** 30 + 1) * h, 2 * (2.0 ** 30 - 1) * h, -2 * (2.0 ** 30 + 1) * h, -2 * (2.0 ** 30 - 1) * h]
    st[2:4, 7:9] = 0.0
    st[0, 7, :6] = edge
    st[1, 8, 10:] = edge
    return st, np.isfinite(st).all(axis=0)


def solve_d(target, s, chi_prev, chi_k):
    """d with ``(chi_prev d + (chi_k - chi_prev) s) / chi_k == target`` in the contract's roundings, searched among the
    neighbours of the real-number solution; where none of them hits, the nearest is returned (the callers assert on
    :func:`landing`, not on this)."""
    dchi = chi_k - chi_prev
    d = (target * chi_k - dchi * s) / chi_prev
    best = d.copy()
    hit = np.zeros(d.shape, dtype=bool)
    for k in range(-32, 33):
        c = d.copy()
        for _ in range(abs(k)):
            c = np.nextafter(c, np.inf if k > 0 else -np.inf)
        ok = ((chi_prev * c + dchi * s) / chi_k == target) & ~hit
        best[ok] = c[ok]
        hit |= ok
    return best


def geometry_state(npix, m, h, chi_prev, chi_k, seed):
    """A state for launches of many workgroups: ray (i, j) belongs to class (i + j) % 4, so that every run of four rows
    and every run of four columns - every workgroup row and every workgroup column, a tail of one row or column included -
    holds all of them: 0 lands between nodes a few pixels off, 1 exactly on nodes, 2 below 0 and 3 at or beyond m, the
    last two by up to m + 2 pixels and on whole, half and quarter pixels."""
    rng = np.random.default_rng(seed)
    st = np.empty((12, npix, npix))
    st[:4] = rng.normal(0.0, 4.0 * h, size=(4, npix, npix))
    st[4:] = rng.normal(0.0, 0.2, size=(8, npix, npix))
    i, j = np.indices((npix, npix))
    cls = (i + j) % 4
    frac = rng.choice([0.0, 0.0, 0.5, 0.25, 0.75], size=(2, npix, npix))
    far = rng.integers(0, m + 3, size=(2, npix, npix)).astype(np.float64)
    near = rng.integers(-3, 4, size=(2, npix, npix)).astype(np.float64)
    for axis, own in enumerate((i, j)):
        p = np.where(cls == 1, own + near[axis], np.where(cls == 2, -1.0 - far[axis] + frac[axis], m + far[axis] + frac[axis]))
        target = (p - own) * h
        s = np.where(rng.random((npix, npix)) < 0.5, st[2 + axis], 0.0)         # half of them with s = 0: d alone lands them
        d = solve_d(target, s, chi_prev, chi_k)
        st[axis] = np.where(cls == 0, st[axis], d)
        st[2 + axis] = np.where(cls == 0, st[2 + axis], s)
    return st


def landing_classes(p1, p2, m):
    """For each workgroup column and each workgroup row of the step's launch, whether it holds a ray that lands between
    nodes, one on a node, one below 0 and one at or beyond m - on both axes.  Returns the list of what is missing."""
    npix = p1.shape[0]
    whole1, whole2 = p1 == np.floor(p1), p2 == np.floor(p2)
    kinds = {"between nodes": ~whole1 & ~whole2, "on a node": whole1 & whole2, "axis 1 below 0": p1 < 0,
             "axis 2 below 0": p2 < 0, "axis 1 at or beyond m": p1 >= m, "axis 2 at or beyond m": p2 >= m,
             "on node 0 or m exactly": (whole1 & ((p1 == 0) | (p1 == m))) | (whole2 & ((p2 == 0) | (p2 == m)))}
    missing = []
    for name, mask in kinds.items():
        once = name.startswith("on node 0")
        if once and not mask.any():
            missing.append(name)
        if once:
            continue
        for bx in range((npix + RAY_BX - 1) // RAY_BX):
            if not mask[:, bx * RAY_BX:(bx + 1) * RAY_BX].any():
                missing.append(f"workgroup column {bx}: {name}")
        for by in range((npix + RAY_BY - 1) // RAY_BY):
            if not mask[by * RAY_BY:(by + 1) * RAY_BY].any():
                missing.append(f"workgroup row {by}: {name}")
    return missing


def random_psi(m, h, seed):
    return np.random.default_rng(seed).normal(0.0, 3.0 * h * h, size=(m, m))


def reference_state(npix, m, h, seed):
    """d, s ~ N(0, 4 h), A, B ~ N(0, 0.2); row 1 is 3 m pixels further along axis 1, row 2 (or the last) 2 m pixels back
    along axis 2."""
    rng = np.random.default_rng(seed)
    st = np.empty((12, npix, npix))
    st[:4] = rng.normal(0.0, 4.0 * h, size=(4, npix, npix))
    st[4:] = rng.normal(0.0, 0.2, size=(8, npix, npix))
    st[0, min(1, npix - 1)] += 3 * m * h
    st[1, min(2, npix - 1)] -= 2 * m * h
    return st


def tiny_state(npix, m, h, seed):
    """For the grids on which the 4 x 4 stencil wraps onto itself: displacements of several m pixels in both directions,
    ray (0, 0) exactly 2 m pixels forward on axis 1 and 3 m pixels back on axis 2 (after an advance from 512 to 1024)."""
    rng = np.random.default_rng(seed)
    st = np.empty((12, npix, npix))
    st[:4] = rng.normal(0.0, 3.0 * m * h, size=(4, npix, npix))
    st[4:] = rng.normal(0.0, 0.2, size=(8, npix, npix))
    st[:4, 0, 0] = [2 * 2 * m * h, 2 * -3 * m * h, 0.0, 0.0]
    return st
