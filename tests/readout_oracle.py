"""A numpy restatement of the readout contract (include/astrild_hip.h: ast_readout), term by term and in
the contract's order, so that the GPU result can be asked for the same BITS.  A helper module: no test functions.

Per axis ``s = x * (n / L) + shift`` in float64.  The kernel forms s with one fused multiply-add; the two agree
whenever the product or the sum is exact: shift = 0 (every case but one), or dyadic inputs (the shift = 0.5 case).
``fl = floor(s)`` for CIC, ``floor(s + 0.5)`` for NGP and TSC; ``frac = s - fl``; base = ``np.mod(fl, n)``.  The weights
are evaluated with arrays and scalars of the FIELD's dtype, with exactly the expressions of ``Window<W>::weights``
(astrild_amd/csrc/paint_window.h), and are not renormalised.  Stencil index a of an axis is ``(base - LO + a) mod n``.
Then, everything widened to float64, ``acc += ((wx[a] * wy[b]) * wz[c]) * f`` from 0.0 in the order a, b, c, and one cast
to the field's dtype.  A coordinate whose ``frac`` is not finite (NaN, +-Inf, or an overflow of the product) gives NaN.
"""
import numpy as np

SUPPORT = {"ngp": 1, "cic": 2, "tsc": 3}
LO = {"ngp": 0, "cic": 0, "tsc": 1}


def axis_stencil(x, n, boxsize, window, shift, rdtype):
    """One axis: ``(idx, w, finite)`` - wrapped stencil indices (W, N) int64, weights (W, N) widened to float64 from
    ``rdtype``, and whether ``frac`` is finite (N,).  Particles that are not finite get base cell 0."""
    R = np.dtype(rdtype).type
    inv_dx = float(n) / float(boxsize)
    with np.errstate(all="ignore"):
        s = np.asarray(x).astype(np.float64) * np.float64(inv_dx) + np.float64(shift)
        fl = np.floor(s if window == "cic" else s + np.float64(0.5))
        frac = s - fl
        finite = np.isfinite(frac)
        base = np.where(finite, np.mod(np.where(finite, fl, 0.0), float(n)), 0.0).astype(np.int64)
        f = frac.astype(R)
        if window == "ngp":
            w = [np.ones_like(f)]
        elif window == "cic":
            w = [R(1) - f, f]
        else:
            hm, hp = R(0.5) - f, R(0.5) + f
            w = [R(0.5) * (hm * hm), R(0.75) - f * f, R(0.5) * (hp * hp)]
    assert all(a.dtype == np.dtype(rdtype) for a in w)
    idx = np.stack([np.mod(base - LO[window] + a, n) for a in range(SUPPORT[window])])
    return idx, np.stack(w).astype(np.float64), finite


def stencil(pos, n, boxsize, window, shift, rdtype):
    pos = np.asarray(pos)
    assert pos.ndim == 2 and pos.shape[1] == 3
    axes = [axis_stencil(pos[:, d], n, boxsize, window, shift, rdtype) for d in range(3)]
    finite = axes[0][2] & axes[1][2] & axes[2][2]
    return [a[0] for a in axes], [a[1] for a in axes], finite


def _sum(lookup, idx, w, finite, npart, ncomp, rdtype):
    W = idx[0].shape[0]
    acc, bound = np.zeros((npart, ncomp)), np.zeros((npart, ncomp))
    with np.errstate(all="ignore"):
        for a in range(W):
            for b in range(W):
                wab = w[0][a] * w[1][b]
                for c in range(W):
                    wabc = wab * w[2][c]
                    v = lookup(idx[0][a], idx[1][b], idx[2][c])                 # (N, C) float64
                    acc += wabc[:, None] * v
                    bound += np.abs(wabc)[:, None] * np.abs(v)
        out = acc.astype(rdtype)
    out[~finite] = np.nan
    return out, bound


def readout(field, pos, boxsize, window="cic", shift=0.0):
    """``(out, A)``: the contract's result - (N,) for a 3-D field, (N, C) for a 4-D one, in the field's dtype - and
    ``A[p, c] = sum |w| |f|`` over the stencil in float64, same shape, the scale of every rounding-error bound."""
    field = np.asarray(field)
    n = field.shape[0]
    f4 = field.reshape(n, n, n, -1)
    idx, w, finite = stencil(pos, n, boxsize, window, shift, field.dtype)
    out, bound = _sum(lambda i, j, k: f4[i, j, k].astype(np.float64), idx, w, finite, len(pos), f4.shape[3], field.dtype)
    if field.ndim == 3:
        return out[:, 0], bound[:, 0]
    return out, bound


def readout_sparse(cells, n, ncomp, rdtype, pos, boxsize, window="cic", shift=0.0):
    """The same weights, indices and order applied to a sparse table ``{(ix, iy, iz): C values}`` of a field of side n
    that is zero elsewhere: ``(out, A, touched)`` with out (N, C) of ``rdtype`` and ``touched`` the set of cells read."""
    idx, w, finite = stencil(pos, n, boxsize, window, shift, rdtype)
    touched = set()
    zero = np.zeros(ncomp)

    def lookup(i, j, k):
        keys = list(zip(i.tolist(), j.tolist(), k.tolist()))
        touched.update(keys)
        return np.array([np.asarray(cells.get(key, zero), dtype=rdtype).astype(np.float64) for key in keys]).reshape(-1, ncomp)
    out, bound = _sum(lookup, idx, w, finite, len(pos), ncomp, rdtype)
    return out, bound, touched


def edge_values(n, boxsize):
    """Coordinates where a window changes cell or a weight vanishes: 0, L, -L, every cell edge and half-cell point of the
    box with their float64 neighbours on both sides, and one far outside (37 L + 3)."""
    L = float(boxsize)
    marks = [0.0, L, -L] + [k * L / n for k in range(n + 1)] + [(k + 0.5) * L / n for k in range(n)]
    vals = []
    for m in marks:
        vals += [m, np.nextafter(m, -np.inf), np.nextafter(m, np.inf)]
    return np.array(vals + [37.0 * L + 3.0])


def edge_positions(n, boxsize):
    """(M, 3): every edge value on all three axes at once, and mixed with two others."""
    v = edge_values(n, boxsize)
    return np.concatenate([np.stack([v, v, v], axis=1), np.stack([v, np.roll(v, 1), np.roll(v, 5)], axis=1)])


def positions(n, boxsize, count, seed, dtype=np.float64):
    """``count`` uniform positions in [-2.5 L, 3.5 L) followed by the edge positions, cast to ``dtype``."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-2.5 * boxsize, 3.5 * boxsize, size=(count, 3))
    return np.concatenate([pos, edge_positions(n, boxsize)]).astype(dtype)


def field(n, ncomp, dtype, seed):
    """A random field with both signs: (n, n, n) for ncomp = 0, else (n, n, n, ncomp)."""
    shape = (n, n, n) if ncomp == 0 else (n, n, n, ncomp)
    return np.random.default_rng(seed).standard_normal(shape).astype(dtype)
