"""An extended-precision reference of the ray step and the emit, built another way than
tests/ray_trace_oracle.py and the kernels: not ray by ray on a 4 x 4 stencil, but field by field.  The five derivative
fields are formed on the whole m x m grid with ``np.roll``, the state is advanced, and each field is interpolated at the
rays' positions, along axis 0 first and then along axis 1.  Everything is ``np.longdouble``; with its 64-bit mantissa the
reference's own rounding is 2^-11 of a float64 rounding, so the distance of the float64 oracle from it is the oracle's.

``step`` also returns, for the planes that the deflection changes (s1, s2, B11 .. B22), a per-ray magnitude M: the same
expression with the absolute value of every term, a bound on the terms whose roundings make up the oracle's error."""
import numpy as np

LD = np.longdouble


def fields(psi, h):
    """(G1, G2, H11, H22, H12) on the nodes and the same five with |.| of every term: central differences, second
    differences and the 4-point cross difference of the periodic psi."""
    psi = np.asarray(psi, dtype=LD)
    h = LD(h)
    up, down = np.roll(psi, -1, 0), np.roll(psi, 1, 0)               # psi[a + 1, b], psi[a - 1, b]
    right, left = np.roll(psi, -1, 1), np.roll(psi, 1, 1)            # psi[a, b + 1], psi[a, b - 1]
    corners = [np.roll(up, -1, 1), np.roll(up, 1, 1), np.roll(down, -1, 1), np.roll(down, 1, 1)]
    value = ((up - down) / (2 * h), (right - left) / (2 * h), (up - 2 * psi + down) / (h * h),
             (right - 2 * psi + left) / (h * h), (corners[0] - corners[1] - corners[2] + corners[3]) / (4 * h * h))
    a = np.abs
    size = ((a(up) + a(down)) / (2 * h), (a(right) + a(left)) / (2 * h), (a(up) + 2 * a(psi) + a(down)) / (h * h),
            (a(right) + 2 * a(psi) + a(left)) / (h * h), sum(a(c) for c in corners) / (4 * h * h))
    return value, size


def cell(p1, p2, m):
    """Node (a, b) under each position, the node after it on either axis, and the offsets inside the cell."""
    f1, f2 = np.floor(p1), np.floor(p2)
    a, b = np.mod(f1, m).astype(np.int64), np.mod(f2, m).astype(np.int64)
    return a, b, (a + 1) % m, (b + 1) % m, p1 - f1, p2 - f2


def interp(field, at):
    """``field`` at the positions ``at`` (from :func:`cell`): linear along axis 0 on both sides of the cell, then along
    axis 1."""
    a, b, a1, b1, fx, fy = at
    lo = field[a, b] + fx * (field[a1, b] - field[a, b])
    hi = field[a, b1] + fx * (field[a1, b1] - field[a, b1])
    return lo + fy * (hi - lo)


def jump(field, at):
    """The largest difference of ``field`` between the four nodes of each ray's cell."""
    a, b, a1, b1, _, _ = at
    four = np.stack([field[a, b], field[a1, b], field[a, b1], field[a1, b1]])
    return four.max(axis=0) - four.min(axis=0)


def step(psi, st, h, chi_prev, chi_k, born=False):
    """One plane in longdouble: ``(state (12, npix, npix), M)`` with M a dict {plane index: (npix, npix) magnitude} for
    the planes 2, 3 (s) and 8 .. 11 (B)."""
    st = np.asarray(st, dtype=LD)
    m, npix = np.asarray(psi).shape[0], st.shape[1]
    h, chi_prev, chi_k = LD(h), LD(chi_prev), LD(chi_k)
    (G1, G2, H11, H22, H12), (MG1, MG2, MH11, MH22, MH12) = fields(psi, h)
    out = st.copy()
    out[0:2] = (chi_prev * st[0:2] + (chi_k - chi_prev) * st[2:4]) / chi_k
    out[4:8] = (chi_prev * st[4:8] + (chi_k - chi_prev) * st[8:12]) / chi_k
    i, j = (x.astype(LD) for x in np.indices((npix, npix)))
    p1, p2 = (i, j) if born else (i + out[0] / h, j + out[1] / h)
    at = cell(p1, p2, m)
    out[2] = st[2] - interp(G1, at)
    out[3] = st[3] - interp(G2, at)
    U = np.empty((2, 2, npix, npix), dtype=LD)
    U[0, 0], U[1, 1] = interp(H11, at), interp(H22, at)
    U[0, 1] = U[1, 0] = interp(H12, at)
    A = out[4:8].reshape(2, 2, npix, npix)
    one_plus_A = A + np.eye(2, dtype=LD)[:, :, None, None]
    out[8:12] = st[8:12] - (U if born else np.einsum("ikxy,kjxy->ijxy", U, one_plus_A)).reshape(4, npix, npix)
    # the magnitudes: every term's absolute value, plus what a rounding of p (relative to 1 + |p1| + |p2|) moves the sample by
    moved = 1 + np.abs(p1) + np.abs(p2)
    M = {2: np.abs(st[2]) + interp(MG1, at) + moved * jump(G1, at), 3: np.abs(st[3]) + interp(MG2, at) + moved * jump(G2, at)}
    gain = 2 * (1 + np.abs(A).max(axis=(0, 1)))
    MH = {(0, 0): (MH11, H11), (1, 1): (MH22, H22), (0, 1): (MH12, H12), (1, 0): (MH12, H12)}
    for r in range(2):
        for c in range(2):
            used = [(r, c)] if born else [(r, 0), (r, 1)]                   # B[r][c] -= sum_k U[r][k] (I + A)[k][c]
            M[8 + 2 * r + c] = np.abs(st[8 + 2 * r + c]) + gain * sum(interp(MH[u][0], at) + moved * jump(MH[u][1], at) for u in used)
    return out, M


def emit(st, chi_k, chi_s):
    """(6, npix, npix) in longdouble: the matrix A and the displacement at the source, then its trace, its symmetric and
    its antisymmetric part."""
    st = np.asarray(st, dtype=LD)
    chi_k, chi_s = LD(chi_k), LD(chi_s)
    d = (chi_k * st[0:2] + (chi_s - chi_k) * st[2:4]) / chi_s
    A = ((chi_k * st[4:8] + (chi_s - chi_k) * st[8:12]) / chi_s).reshape(2, 2, *st.shape[1:])
    sym, anti = (A + A.swapaxes(0, 1)) / 2, (A - A.swapaxes(0, 1)) / 2
    return np.stack([-(sym[0, 0] + sym[1, 1]) / 2, -(sym[0, 0] - sym[1, 1]) / 2, -sym[0, 1], anti[1, 0], -d[0], -d[1]])


def green(m, scale):
    """The multiplier of ``ast_lens_green_multiply`` in longdouble (mode (0, 0): 0)."""
    pi = LD("3.14159265358979323846264338327950288")
    sa = np.sin(pi * np.arange(m, dtype=LD) / m)[:, None]
    sb = np.sin(pi * np.arange(m // 2 + 1, dtype=LD) / m)[None, :]
    den = 4 * (sa * sa + sb * sb)
    den[0, 0] = 1
    g = -2 * LD(scale) / den
    g[0, 0] = 0
    return g
