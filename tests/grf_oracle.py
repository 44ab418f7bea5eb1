"""numpy restatement of the Gaussian-random-field generator of astrild_amd/csrc/grf.hip (ast_grf_spectrum in
include/astrild_hip.h states the contract): Philox4x32-10 in uint64 arithmetic, the canonical pixel of the
self-conjugate columns, the linear C(l) interpolation with its cut, Box-Muller in fp64 in the kernel's order of
operations, and the ring-binned |ft|^2 of lenstools' flat-sky power spectrum (bins edges[k] < l <= edges[k+1], every
half-plane pixel counted once, as astrild_amd/csrc/flatsky.hip bins it)."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)          # Philox4x32 multipliers
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)          # Weyl key increments
_MASK, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds (Salmon et al. 2011; Random123): four 32-bit counter words (arrays or scalars) and
    two key words in, four output words out, all as uint64 holding 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _MASK for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & _MASK, np.uint64(k1) & _MASK
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                                # 32 x 32 -> 64 bit: no overflow in uint64
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ k0) & _MASK, p1 & _MASK, ((p0 >> _S32) ^ c3 ^ k1) & _MASK, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def pixel_l(n, theta):
    """|l| of every pixel (i, j) of the n x (n/2 + 1) half plane of a map of side theta [rad]."""
    i = np.arange(n, dtype=np.int64)[:, None]
    j = np.arange(n // 2 + 1, dtype=np.int64)[None, :]
    m = np.minimum(i, n - i)
    return (2.0 * np.pi / theta) * np.sqrt((m * m + j * j).astype(np.float64))


def cl_at(l, cl, lmax=np.inf):
    """C(l): the table at integer l = 0 .. len(cl) - 1, linear in between, 0 where l > min(lmax, len(cl) - 1)."""
    cl = np.asarray(cl, dtype=np.float64)
    ncl = len(cl)
    top = min(float(lmax), ncl - 1.0)
    k = np.minimum(np.floor(l).astype(np.int64), ncl - 1)
    t = l - k
    c = cl[k] + t * (cl[np.minimum(k + 1, ncl - 1)] - cl[k])
    return np.where(l <= top, c, 0.0)


def amplitude(n, theta, cl, lmax=np.inf):
    """A = sqrt(C(l)) (n n / theta) on the half plane."""
    return np.sqrt(cl_at(pixel_l(n, theta), cl, lmax)) * (float(n) * float(n) / theta)


def deviates(n, seed, realisation=0):
    """(a, b, real, conj) on the half plane: the two standard normal deviates of every pixel's canonical counter, which
    pixels are their own conjugates, and which take the conjugate of their partner's value."""
    nh = n // 2 + 1
    i = np.repeat(np.arange(n, dtype=np.int64)[:, None], nh, axis=1)
    j = np.repeat(np.arange(nh, dtype=np.int64)[None, :], n, axis=0)
    selfc = (j == 0) | ((n % 2 == 0) & (j == n // 2))
    ip = (n - i) % n
    ic = np.where(selfc, np.minimum(i, ip), i)
    c = (ic * nh + j).astype(np.uint64)
    seed, realisation = np.uint64(seed), np.uint64(realisation)
    w = philox4x32_10(c & _MASK, c >> _S32, realisation & _MASK, realisation >> _S32, seed & _MASK, seed >> _S32)
    x = (w[0] >> np.uint64(5)) * np.uint64(1 << 26) + (w[1] >> np.uint64(6))
    y = (w[2] >> np.uint64(5)) * np.uint64(1 << 26) + (w[3] >> np.uint64(6))
    u1 = (x.astype(np.float64) + 1.0) * 2.0 ** -53                 # (0, 1], exact
    u2 = y.astype(np.float64) * 2.0 ** -53                         # [0, 1), exact
    r = np.sqrt(-2.0 * np.log(u1))
    phi = (2.0 * np.pi) * u2
    return r * np.cos(phi), r * np.sin(phi), selfc & (i == ip), selfc & (i > ip)


def spectrum(n, theta, cl, seed, realisation=0, lmax=np.inf):
    """(ft, A): the complex128 half-plane spectrum of ast_grf_spectrum and its amplitude."""
    a, b, real, conj = deviates(n, seed, realisation)
    A = amplitude(n, theta, cl, lmax)
    re = np.where(real, A * a, A * a / np.sqrt(2.0))
    im = np.where(real, 0.0, A * b / np.sqrt(2.0))
    im = np.where(conj, -im, im)
    zero = A == 0.0
    return np.where(zero, 0.0, re) + 1j * np.where(zero, 0.0, im), A


def full_plane(ft, n):
    """The n x n spectrum of a real map from its half plane: column j > n/2 is the conjugate of column n - j, rows
    mirrored."""
    full = np.zeros((n, n), dtype=np.complex128)
    nh = n // 2 + 1
    full[:, :nh] = ft
    rows = (n - np.arange(n)) % n
    for j in range(nh, n):
        full[:, j] = np.conj(ft[rows, n - j])
    return full


def binned(values, l, edges):
    """(sum of values, pixel count) per bin edges[k] < l <= edges[k+1] of the half plane."""
    edges = np.asarray(edges, dtype=np.float64)
    k = np.searchsorted(edges, l.ravel(), side="left") - 1
    ok = (k >= 0) & (k < len(edges) - 1)
    hits = np.bincount(k[ok], minlength=len(edges) - 1)
    return np.bincount(k[ok], weights=np.asarray(values).ravel()[ok], minlength=len(edges) - 1), hits


def bin_z(ft2, A, l, edges):
    """(z, hits) per bin: z = (sum |ft|^2 / sum A^2 - 1) sqrt(hits), of order one for a field drawn with amplitude A."""
    s, hits = binned(ft2, l, edges)
    e, _ = binned(A * A, l, edges)
    return (s / e - 1.0) * np.sqrt(hits), hits


# the statistical cases that the CPU and the GPU tests share
STAT_N, STAT_THETA = 256, np.deg2rad(10.0)
STAT_CL = 1e-9 / (np.arange(8000, dtype=np.float64) + 50.0) ** 2
STAT_EDGES = (2.0 * np.pi / STAT_THETA) * (1.5 + 4.0 * np.arange(32))
STAT_SEEDS = (34077, 7, 20240601)
