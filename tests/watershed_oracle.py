"""The watershed void finder's definition in plain numpy and Python, written independently of
astrild_amd.device: what tests/test_watershed_oracle.py checks on hand-built maps and tests/test_gpu_watershed.py
compares the GPU against.

1. pixels are totally ordered by (f[p], p), p = y * npix + x, values compared in the map's dtype (-0.0 == +0.0);
2. link[p] = the smallest of p and its up-to-8 neighbours inside the map;
3. a minimum has link[p] == p; a basin is the set of pixels whose links end at the same minimum; basins are numbered
   in ascending flat index of their minimum;
4. per basin: area, sum of x, sum of y, pixels on the outermost rows / columns, sum of f (here exactly rounded:
   math.fsum), f_min and the minimum's index;
5. the pass between two basins = min over their 8-adjacent pixel pairs of max(f[p], f[q]) (+ 0: a zero pass is +0.0);
6. merge at height h: edges in ascending (s, a, b); roots ra != rb merge iff s - max(m_ra, m_rb) < h (float64), m the
   lowest minimum of a set; the merged set's root is the one with the smaller (m, id);
7. every final set is a void, numbered in ascending id of its root basin.
"""
import math

import numpy as np

NEIGHBOURS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]      # (dy, dx)


def links(f):
    """link[p] as a flat int64 array."""
    f = np.asarray(f)
    npix = f.shape[0]
    flat = np.arange(npix * npix, dtype=np.int64).reshape(npix, npix)
    best_v, best_p = f.copy(), flat.copy()
    for dy, dx in NEIGHBOURS:
        ys = slice(max(0, -dy), npix - max(0, dy))          # pixels that have this neighbour
        xs = slice(max(0, -dx), npix - max(0, dx))
        yn = slice(max(0, dy), npix - max(0, -dy))
        xn = slice(max(0, dx), npix - max(0, -dx))
        v, p = f[yn, xn], flat[yn, xn]
        bv, bp = best_v[ys, xs], best_p[ys, xs]
        less = (v < bv) | ((v == bv) & (p < bp))
        bv[less] = v[less]
        bp[less] = p[less]
    return best_p.reshape(-1)


def longest_path(link):
    """The largest number of links between a pixel and its minimum."""
    link = np.asarray(link)
    steps = np.zeros(len(link), dtype=np.int64)
    cur = np.arange(len(link))
    while True:
        nxt = link[cur]
        moving = nxt != cur
        if not moving.any():
            return int(steps.max())
        steps += moving
        cur = nxt


def basins(f):
    """The dict of device.watershed_basins, from the definition."""
    f = np.asarray(f)
    npix = f.shape[0]
    assert f.ndim == 2 and f.shape[1] == npix and np.isfinite(f).all()
    link = links(f)
    root = link.copy()
    while True:                                             # one link at a time: no pointer jumping here
        nxt = link[root]
        if np.array_equal(nxt, root):
            break
        root = nxt
    minima = np.flatnonzero(link == np.arange(npix * npix))
    ident = np.full(npix * npix, -1, dtype=np.int64)
    ident[minima] = np.arange(len(minima))
    labels = ident[root].reshape(npix, npix)
    m = len(minima)
    yy, xx = np.divmod(np.arange(npix * npix), npix)
    lab = labels.reshape(-1)
    border = (xx == 0) | (yy == 0) | (xx == npix - 1) | (yy == npix - 1)
    order = np.argsort(lab, kind="stable")
    cuts = np.searchsorted(lab[order], np.arange(m + 1))
    f64 = f.reshape(-1).astype(np.float64)
    sum_f = np.array([math.fsum(f64[order[cuts[b]:cuts[b + 1]]]) for b in range(m)])
    sum_abs = np.array([math.fsum(np.abs(f64[order[cuts[b]:cuts[b + 1]]])) for b in range(m)])
    passes = {}
    for dy, dx in [(0, 1), (1, -1), (1, 0), (1, 1)]:
        ys, xs = slice(0, npix - dy), slice(max(0, -dx), npix - max(0, dx))
        yn, xn = slice(dy, npix), slice(max(0, dx), npix - max(0, -dx))
        la, lb = labels[ys, xs].reshape(-1), labels[yn, xn].reshape(-1)
        top = np.maximum(f[ys, xs], f[yn, xn]).reshape(-1) + f.dtype.type(0)
        for i in np.flatnonzero(la != lb):
            key = (min(la[i], lb[i]), max(la[i], lb[i]))
            if key not in passes or top[i] < passes[key]:
                passes[key] = top[i]
    keys = sorted(passes)
    return {"labels": labels.astype(np.int32), "minima": minima.astype(np.int64), "f_min": f.reshape(-1)[minima],
            "area": np.bincount(lab, minlength=m).astype(np.int64),
            "sum_x": np.bincount(lab, weights=xx, minlength=m).astype(np.int64),
            "sum_y": np.bincount(lab, weights=yy, minlength=m).astype(np.int64),
            "edge_pix": np.bincount(lab, weights=border, minlength=m).astype(np.int64),
            "sum_f": sum_f, "sum_abs_f": sum_abs,
            "edges": np.array(keys, dtype=np.int32).reshape(-1, 2),
            "saddle": np.array([passes[k] for k in keys], dtype=f.dtype)}


def merge(b, h):
    """void_of_basin (M,) for the merge at height h: sets kept as member lists, one owner array."""
    m = len(b["f_min"])
    owner = list(range(m))                                  # the root of every basin's set, always up to date
    members = {i: [i] for i in range(m)}
    lowest = {i: float(b["f_min"][i]) for i in range(m)}
    todo = sorted((float(s), int(a), int(c)) for (a, c), s in zip(b["edges"], b["saddle"]))
    for s, a, c in todo:
        ra, rc = owner[a], owner[c]
        if ra == rc:
            continue
        if s - max(lowest[ra], lowest[rc]) < h:
            win, lose = (ra, rc) if (lowest[ra], ra) < (lowest[rc], rc) else (rc, ra)
            for i in members.pop(lose):
                owner[i] = win
                members[win].append(i)
            del lowest[lose]
    roots = sorted(members)
    number = {r: i for i, r in enumerate(roots)}
    return np.array([number[owner[i]] for i in range(m)], dtype=np.int32), np.array(roots, dtype=np.int64)


def voids(b, void_of_basin, roots):
    """Per-void sums and derived quantities."""
    nv = len(roots)
    out = {k: np.array([int(b[k][void_of_basin == v].sum()) for v in range(nv)], dtype=np.int64)
           for k in ("area", "sum_x", "sum_y", "edge_pix")}
    out["sum_f"] = np.array([math.fsum(b["sum_f"][void_of_basin == v]) for v in range(nv)])
    out["kappa_min"] = b["f_min"][roots]
    out["min_index"] = b["minima"][roots]
    out["x"] = out["sum_x"] / out["area"]
    out["y"] = out["sum_y"] / out["area"]
    out["rad"] = np.sqrt(out["area"] / np.pi)
    out["kappa_mean"] = out["sum_f"] / out["area"]
    return out


def void_map(b, void_of_basin):
    return np.asarray(void_of_basin, dtype=np.int32)[b["labels"]]


# ---------------------------------------------------------------- maps
def smoothed_noise(npix, sigma=2.0, seed=3, dtype=np.float64):
    from scipy.ndimage import gaussian_filter
    return gaussian_filter(np.random.RandomState(seed).standard_normal((npix, npix)), sigma, mode="wrap").astype(dtype)


def snake(npix, dtype=np.float64):
    """Corridors on the even rows, walls (1e6) on the odd rows, each wall with a one-pixel gap at alternating ends;
    values rise by 1 along the path from pixel 0: one basin whose link paths are as long as the map allows."""
    assert npix % 2 == 1
    f = np.full((npix, npix), 1e6, dtype=dtype)
    v = 0
    for r in range(0, npix, 2):
        cols = range(npix) if (r // 2) % 2 == 0 else range(npix - 1, -1, -1)
        for c in cols:
            f[r, c] = v
            v += 1
        if r + 1 < npix:
            f[r + 1, npix - 1 if (r // 2) % 2 == 0 else 0] = v
            v += 1
    return f


def blocks(npix=40, side=8, seed=5, dtype=np.float64):
    """Constant blocks of side x side pixels with random levels (some equal)."""
    rs = np.random.RandomState(seed)
    k = (npix + side - 1) // side
    levels = rs.randint(0, 6, size=(k, k)).astype(dtype)
    return np.kron(levels, np.ones((side, side), dtype=dtype))[:npix, :npix].copy()


def float32_ties(npix=48, seed=9):
    """A float64 map whose values are all distinct and fall onto a few levels, in large plateaus, once rounded to
    float32: levels 0.1 apart round 1, plus a different multiple of 1e-15 per pixel (at most 2.3e-12: far below
    float32's spacing of 1.2e-7 there, four times float64's)."""
    rs = np.random.RandomState(seed)
    levels = np.round(smoothed_noise(npix, 1.5, seed), 1) + 1.0
    return levels + 1e-15 * rs.permutation(npix * npix).reshape(npix, npix)
