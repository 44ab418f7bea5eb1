"""CPU oracle of the friends-of-friends group finder (astrild_amd/particles/hutils/fof.py, astrild_amd/csrc/fof.hip):
plain numpy, brute force over all pairs in chunks, fp64 and op by op in the operand order the kernels document:

  a = |x_i - x_j| per axis, periodic a = min(a, L - a)
  sphere:    d^2 = (a_x^2 + a_y^2) + a_z^2, friends when d^2 <= b b
  cylinder:  rp^2 = a_a a_a + a_b a_b over the axes a < b other than los, pi = a_los,
             friends when rp^2 <= b_perp b_perp and pi <= b_para

Components by min-label propagation over the friend pairs, the numbering rule (groups of >= nmin members by descending
size, ties by ascending smallest index), and the group features as exactly rounded rational sums.  A helper module: no
test functions.
"""
from fractions import Fraction

import numpy as np


def friend_pairs(pos, b, boxsize=None, b_para=None, los=2, chunk=512):
    """``(i, j)`` int64 arrays of all unordered friend pairs, i < j, and, for the tests' margin checks, the smallest
    relative distance |x / limit - 1| of any pair quantity (d^2 or rp^2 against b^2; pi against b_para) to its limit."""
    p = np.asarray(pos).astype(np.float64)
    n = len(p)
    bb = np.float64(b) * np.float64(b)
    a_ax, b_ax = [c for c in range(3) if c != los]
    out_i, out_j, margin = [], [], np.inf
    for i0 in range(0, n, chunk):
        pi = p[i0:i0 + chunk]
        a = [np.abs(pi[:, None, c] - p[None, :, c]) for c in range(3)]
        if boxsize is not None:
            a = [np.minimum(x, np.float64(boxsize) - x) for x in a]
        if b_para is None:
            q = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
            ok = q <= bb
            margin = min(margin, float(np.abs(q / bb - 1.0).min()))
        else:
            q = a[a_ax] * a[a_ax] + a[b_ax] * a[b_ax]
            ok = (q <= bb) & (a[los] <= np.float64(b_para))
            margin = min(margin, float(np.abs(q / bb - 1.0).min()), float(np.abs(a[los] / b_para - 1.0).min()))
        ii, jj = np.nonzero(ok)
        ii = ii + i0
        keep = ii < jj
        out_i.append(ii[keep])
        out_j.append(jj[keep])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return cat(out_i).astype(np.int64), cat(out_j).astype(np.int64), margin


def components(n, i, j):
    """root[k] = the smallest index of k's connected component: min-label propagation along the pairs, with a pointer
    jump per sweep, until nothing changes."""
    root = np.arange(n, dtype=np.int64)
    while True:
        low = np.minimum(root[i], root[j])
        new = root.copy()
        np.minimum.at(new, i, low)
        np.minimum.at(new, j, low)
        new = new[new]
        if np.array_equal(new, root):
            return root
        root = new


def number_groups(root, nmin=1):
    """``labels`` int32, ``length`` int64, ``first`` int64, ``members`` int32, ``offsets`` int64 by the numbering rule."""
    n = len(root)
    firsts, sizes = np.unique(root, return_counts=True)
    keep = sizes >= nmin
    firsts, sizes = firsts[keep], sizes[keep]
    order = np.lexsort((firsts, -sizes))                        # by -size, ties by first
    first, length = firsts[order].astype(np.int64), sizes[order].astype(np.int64)
    table = np.zeros(n, dtype=np.int32)
    table[first] = np.arange(1, len(first) + 1, dtype=np.int32)
    labels = table[root] if n else np.zeros(0, dtype=np.int32)
    idx = np.nonzero(labels > 0)[0]
    members = idx[np.argsort(labels[idx], kind="stable")].astype(np.int32)
    offsets = np.zeros(len(first) + 1, dtype=np.int64)
    np.cumsum(length, out=offsets[1:])
    return {"labels": labels, "length": length, "first": first, "members": members, "offsets": offsets}


def groups(pos, b, boxsize=None, nmin=1, b_para=None, los=2):
    """The result of ``fof_groups`` as numpy arrays, with ``links``, ``ncomponents`` and ``margin``."""
    n = len(pos)
    i, j, margin = friend_pairs(pos, b, boxsize, b_para, los) if n else (np.zeros(0, np.int64),) * 2 + (np.inf,)
    root = components(n, i, j)
    out = number_groups(root, nmin)
    out["links"] = int(len(i))
    out["ncomponents"] = int(len(np.unique(root)))
    out["margin"] = margin
    return out


def _frac(x):
    return Fraction(float(x))


def features(pos, grp, boxsize=None, vel=None, weights=None):
    """``cm_position``, ``cm_velocity`` (with ``vel``), ``weight``: s_i = pos_i - p_ref in fp64 with its one wrap, as
    the kernel forms it; everything after that - the products w s, their sums, the division, the sum with p_ref and the
    one wrap into [0, L) - in rational arithmetic, rounded once at the end.  ``scale`` (G, 3): sum |w s| / W + |p_ref|
    + L, and ``vscale`` (G, 3): sum |w v| / W, the magnitudes the test's error bounds are relative to."""
    p = np.asarray(pos).astype(np.float64)
    v = None if vel is None else np.asarray(vel).astype(np.float64)
    w_all = None if weights is None else np.asarray(weights).astype(np.float64)
    g = len(grp["first"])
    L = 0.0 if boxsize is None else float(boxsize)
    cm, cmv, weight, scale, vscale = np.zeros((g, 3)), np.zeros((g, 3)), np.zeros(g), np.zeros((g, 3)), np.zeros((g, 3))
    for k in range(g):
        idx = grp["members"][grp["offsets"][k]:grp["offsets"][k + 1]].astype(np.int64)
        ref = p[grp["first"][k]]
        w = np.ones(len(idx)) if w_all is None else w_all[idx]
        s = p[idx] - ref
        if boxsize is not None:
            s = np.where(s > 0.5 * L, s - L, np.where(s < -0.5 * L, s + L, s))
        W = sum(_frac(x) for x in w)
        weight[k] = float(W)
        for a in range(3):
            c = _frac(ref[a]) + sum(_frac(x) * _frac(y) for x, y in zip(w, s[:, a])) / W
            if boxsize is not None:
                c = c + _frac(L) if c < 0 else (c - _frac(L) if c >= _frac(L) else c)
            cm[k, a] = float(c)
            scale[k, a] = float(sum(abs(_frac(x) * _frac(y)) for x, y in zip(w, s[:, a])) / W) + abs(ref[a]) + L
            if v is not None:
                cmv[k, a] = float(sum(_frac(x) * _frac(y) for x, y in zip(w, v[idx, a])) / W)
                vscale[k, a] = float(sum(abs(_frac(x) * _frac(y)) for x, y in zip(w, v[idx, a])) / W)
    out = {"cm_position": cm, "weight": weight, "scale": scale}
    if v is not None:
        out["cm_velocity"], out["vscale"] = cmv, vscale
    return out


def clustered(L=100.0, n=6000, seed=11):
    """The clustered catalogue of the GPU tests: 12 Gaussian blobs - 500 points of sigma 0.6 at (0.3, 99.8, 50), across
    two periodic faces; 700 of sigma 0.15 at (52.5, 52.5, 52.5); ten of 150 points and sigma 0.5 at centres uniform in
    [10, 90]^3 - and a uniform background, wrapped into [0, L) and shuffled.  float64 (n, 3)."""
    rng = np.random.default_rng(seed)
    parts = [rng.normal((0.3, 99.8, 50.0), 0.6, (500, 3)), rng.normal((52.5, 52.5, 52.5), 0.15, (700, 3))]
    centres = rng.uniform(10.0, 90.0, (10, 3))
    parts += [rng.normal(c, 0.5, (150, 3)) for c in centres]
    parts.append(rng.uniform(0.0, L, (n - 2700, 3)))
    pos = np.mod(np.concatenate(parts), L)
    return pos[rng.permutation(n)]
