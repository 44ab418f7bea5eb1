"""numpy restatement of the multi-plane ray tracer (csrc/ray_trace.hip, astrild_amd/ray_trace.py): the
potential of a plane, the ray step and the emit, operation for operation in float64.  numpy rounds every elementwise
operation once and fuses nothing, as the library does when built with -ffp-contract=off, so ``step`` and ``emit`` give
the device's bits (the GPU tests compare ``tobytes()``); ``potential`` goes through numpy's FFT and agrees with the
device's to rounding only.  Independent of the product: nothing here imports astrild_amd."""
import numpy as np

D_HUBBLE = 2997.92458
STATE = ("d1", "d2", "s1", "s2", "A11", "A12", "A21", "A22", "B11", "B12", "B21", "B22")
QUANTITIES = ("kappa", "gamma1", "gamma2", "omega", "alpha1", "alpha2")
INDEX_CLAMP = 2.0 ** 30


def green(m, scale):
    """The multiplier of mode (a, b) of the (m, m/2 + 1) half spectrum: -2 scale / (4 (sin^2(pi a / m) + sin^2(pi b / m))),
    0 at (0, 0)."""
    sa = np.sin(np.pi * (np.arange(m, dtype=np.float64) / m))[:, None]
    sb = np.sin(np.pi * (np.arange(m // 2 + 1, dtype=np.float64) / m))[None, :]
    den = 4.0 * (sa * sa + sb * sb)
    den[0, 0] = 1.0
    g = (-2.0 * scale) / den
    g[0, 0] = 0.0
    return g


def potential(sigma, h, pad, scale):
    """psi (m, m), m = pad npix: sigma in the corner of a zero grid, R2C, times green(m, scale h^2 / m^2), unnormalised
    C2R.  Its 5-point Laplacian is 2 scale (grid - mean of the grid)."""
    sigma = np.asarray(sigma)
    npix = sigma.shape[0]
    m = pad * npix
    grid = np.zeros((m, m), dtype=np.float64)
    grid[:npix, :npix] = sigma
    spec = np.fft.rfft2(grid) * green(m, scale * (h * h) / (float(m) * float(m)))
    return np.fft.irfft2(spec, s=(m, m)) * float(m * m), grid


def laplacian(psi, h):
    """The periodic 5-point Laplacian of psi on nodes h apart."""
    return (np.roll(psi, -1, 0) + np.roll(psi, 1, 0) + np.roll(psi, -1, 1) + np.roll(psi, 1, 1) - 4.0 * psi) / (h * h)


def state(npix):
    return np.zeros((len(STATE), npix, npix), dtype=np.float64)


def _node(fl, m):
    """floor(p) -> node index in [0, m): clamped to +-2^30, then reduced modulo m."""
    return np.mod(np.clip(fl, -INDEX_CLAMP, INDEX_CLAMP).astype(np.int64), m)


def _bilinear(w, q):
    """((w00 q00 + w10 q10) + w01 q01) + w11 q11; q[x][y] belongs to node (a + x, b + y)."""
    return ((w[0][0] * q[0][0] + w[1][0] * q[1][0]) + w[0][1] * q[0][1]) + w[1][1] * q[1][1]


def step(psi, st, h, chi_prev, chi_k, born=False):
    """One plane, on a copy of ``st`` (12, npix, npix): advance from chi_prev to chi_k, deflect by psi (m, m)."""
    psi = np.asarray(psi, dtype=np.float64)
    m, npix = psi.shape[0], st.shape[1]
    v = [np.array(p, dtype=np.float64) for p in st]
    dchi = chi_k - chi_prev
    d1, d2 = (chi_prev * v[0] + dchi * v[2]) / chi_k, (chi_prev * v[1] + dchi * v[3]) / chi_k
    A11, A12 = (chi_prev * v[4] + dchi * v[8]) / chi_k, (chi_prev * v[5] + dchi * v[9]) / chi_k
    A21, A22 = (chi_prev * v[6] + dchi * v[10]) / chi_k, (chi_prev * v[7] + dchi * v[11]) / chi_k
    i = np.arange(npix, dtype=np.float64)[:, None] + np.zeros((npix, npix))
    j = np.arange(npix, dtype=np.float64)[None, :] + np.zeros((npix, npix))
    p1, p2 = (i, j) if born else (i + d1 / h, j + d2 / h)
    f1, f2 = np.floor(p1), np.floor(p2)
    fx, fy = p1 - f1, p2 - f2
    a, b = _node(f1, m), _node(f2, m)

    def at(da, db):
        return psi[np.mod(a + da, m), np.mod(b + db, m)]
    h2, hh = 2.0 * h, h * h
    hh4 = 4.0 * hh
    a1, a2, u11, u22, u12 = ([[None, None], [None, None]] for _ in range(5))
    for x in range(2):
        for y in range(2):
            a1[x][y] = (at(x + 1, y) - at(x - 1, y)) / h2
            a2[x][y] = (at(x, y + 1) - at(x, y - 1)) / h2
            u11[x][y] = ((at(x + 1, y) - 2.0 * at(x, y)) + at(x - 1, y)) / hh
            u22[x][y] = ((at(x, y + 1) - 2.0 * at(x, y)) + at(x, y - 1)) / hh
            u12[x][y] = (((at(x + 1, y + 1) - at(x + 1, y - 1)) - at(x - 1, y + 1)) + at(x - 1, y - 1)) / hh4
    w = [[(1.0 - fx) * (1.0 - fy), (1.0 - fx) * fy], [fx * (1.0 - fy), fx * fy]]
    al1, al2 = _bilinear(w, a1), _bilinear(w, a2)
    U11, U22, U12 = _bilinear(w, u11), _bilinear(w, u22), _bilinear(w, u12)
    out = np.empty_like(st, dtype=np.float64)
    out[0], out[1], out[2], out[3] = d1, d2, v[2] - al1, v[3] - al2
    out[4], out[5], out[6], out[7] = A11, A12, A21, A22
    if born:
        out[8], out[9], out[10], out[11] = v[8] - U11, v[9] - U12, v[10] - U12, v[11] - U22
    else:
        out[8] = v[8] - (U11 * (1.0 + A11) + U12 * A21)
        out[9] = v[9] - (U11 * A12 + U12 * (1.0 + A22))
        out[10] = v[10] - (U12 * (1.0 + A11) + U22 * A21)
        out[11] = v[11] - (U12 * A12 + U22 * (1.0 + A22))
    return out


def emit(st, chi_k, chi_s):
    """(6, npix, npix): kappa, gamma1, gamma2, omega, alpha1, alpha2 of a source at chi_s > chi_k."""
    dchi = chi_s - chi_k
    d1, d2 = (chi_k * st[0] + dchi * st[2]) / chi_s, (chi_k * st[1] + dchi * st[3]) / chi_s
    A11, A12 = (chi_k * st[4] + dchi * st[8]) / chi_s, (chi_k * st[5] + dchi * st[9]) / chi_s
    A21, A22 = (chi_k * st[6] + dchi * st[10]) / chi_s, (chi_k * st[7] + dchi * st[11]) / chi_s
    return np.stack([-0.5 * (A11 + A22), -0.5 * (A11 - A22), -0.5 * (A12 + A21), 0.5 * (A21 - A12), -d1, -d2])


def plane_weights(a, omega_m):
    """3/2 Omega_m D_H^-2 / a_k: sigma_k = chi_k plane_weights_k D_k."""
    return 1.5 * float(omega_m) * (1.0 / D_HUBBLE) ** 2 / np.asarray(a, dtype=np.float64)


def trace(psis, npix, chi, h, chi_src, born=False):
    """The maps (6, S, npix, npix) of the sources at ``chi_src`` (any order) from the potentials ``psis`` of the planes at
    the ascending distances ``chi``; zeros for a source at or in front of the first plane."""
    chi = np.asarray(chi, dtype=np.float64)
    src = np.asarray(chi_src, dtype=np.float64).reshape(-1)
    out = np.zeros((len(QUANTITIES), src.size, npix, npix), dtype=np.float64)
    last = [int(np.sum(chi < c)) - 1 for c in src]
    st = state(npix)
    for k in range(max(last, default=-1) + 1):
        st = step(psis[k], st, h, 0.0 if k == 0 else float(chi[k - 1]), float(chi[k]), born)
        for s in range(src.size):
            if last[s] == k:
                out[:, s] = emit(st, float(chi[k]), float(src[s]))
    return out
