"""Edge cases for the flat-sky window filters of astrild_amd/csrc/filters.hip: named, seeded inputs per entry point, the
scipy / numpy reference of each operation, an op-by-op numpy model of each kernel's arithmetic (the index formulas in
the kernels' comments), an ELEMENTWISE error bound derived from the operations, and the wrong kernels ("mutations")
that tests/test_filter_edges_cpu.py shows every case would catch.  No GPU, no torch.

u = 2^-53 is the unit roundoff.  No bound is relative to max|ref|: derivative filters cancel, and a max-norm tolerance
hides every pixel whose value is far below the largest one - the map border of a Gaussian window above all.

Bounds, per output pixel, between the kernel and the reference (each is the sum of both sides' errors):

convolve2d      2 K u (|img| conv |w|),  K = kh kw: a K-term sum in any order is within (K - 1) u of the exact one,
                relative to the sum of its absolute terms, plus u per product; twice, for the two summations.  Kernel and
                ndimage.convolve add the same products in the same row-major order, so the difference is in fact zero.
gaussian_filter 2 (K0 + K1) u A + tap term.  K = 2 radius + 1 per axis; A = |img| correlated with scipy's absolute taps
                along axis 0, then axis 1, in the same boundary mode (the first pass's error goes through the second
                pass's absolute taps).  Tap term: the library computes the taps on the host with its own exp and pow.
                tau(sigma, order) = max|w_scipy - w_exact| / max|w_exact|, w_exact from a longdouble restatement of
                _gaussian_kernel1d, is measured for every case (table below); the host side is allowed 4 tau (another
                libm, at most 1 ulp per call), so each tap differs by at most 5 tau max|w| and the output by
                5 tau0 max|w0| (box sum of |img| along axis 0, then |w1|) + 5 tau1 max|w1| (|w0|, then box sum).
dgd_filter      e0 = (5 |a| + 5) u relative error of gaussian_field = exp(a) / (2 pi s^2), a = -d^2 / (2 s^2), per side:
                d = sqrt(x^2 + y^2) of exact half-integers: u;  d d: 2 u + u;  s s: u;  2 (s s): exact;  the quotient: u -
                the argument is within 5 u |a| of exact, which exp turns into a relative error of 5 |a| u;  exp itself 1 ulp
                = 2 u;  2 pi (s s): pi is the same double on both sides, the product u on top of s s, the last division u:
                2 + 3 = 5 more.  The DGD3 sum adds 2 roundings: E0 = sum_i |G_i| e0_i + 2 u sum_i |G_i|.  Each np.gradient
                pass maps E <- S|E| + 4 u S(|W| + E), S the stencil with absolute coefficients ((1, 1) / 2h inside,
                (1.5, 2, 0.5) / h at the two ends) and W the window before the pass: inside, one subtraction and one
                division, 2 u S|W|; at an end, a rounded coefficient, a product and two additions, at most 4 u S|W|.  The
                product with the image adds u |out|.  Both sides: twice all that.  4 subnormal steps are added wherever
                a rounding is, for windows that underflow.  Measured, the sides differ by exp's last bit alone.
aperture        2 N_ring u mean|img[ring]| + u |img|.
hann            8 u |img|.
zoom            8 u (sum of the four |w x| terms).

Measured tau(sigma, order) in units of 1e-16 (scipy 1.15.3; radius = int(4 sigma + 0.5)); a float64 restatement of the
library's host code (host_taps) stays within 4 tau of the exact taps in every case (at most 1.1e-15):
    sigma radius  order 0     1     2     3     4     5     6     7     8
    0.1   0             0     0     0.31  0     1.4   0     1.6   0     2.8
    0.124 0             0     0     1.2   0     2.2   0     3.8   0     4.4
    0.126 1             1.8   11    2.3   11    1.9   10    2.5   8.5   1.4
    0.3   1             1.2   4.1   2.6   2.2   4.1   2.5   4.9   22    5.8
    1.3   5             0.37  1.3   1.2   2.9   3.7   2.5   4.2   5.7   5.7
    5     20            1.2   2.8   1.9   2.3   3.9   3.5   6.3   6.4   6.7
(0: taps that are exactly [1.] or [0.]; an odd order has no tap at radius 0)

Worst err / bound on the MI355X per entry point (tests/test_gpu_filter_edges.py prints them):
    ast_convolve2d              0      bit for bit in every case
    ast_gaussian_filter_order   0.11   random images (npix 17); 0.0099 on the constant image
    ast_dgd_filter              0.060  (npix 17)
    ast_aperture_photometry     0.16   (9, 5), four pixels; 4.2e-5 at (513, 100): the bound is the worst case of a sum of
                                       N_ring = 31408 terms and grows with N, a tree's and numpy's pairwise error with log N
    ast_hann_apodize            0.32   (npix 17)
    ast_zoom_linear             0.13   (3 -> 2); 0 elsewhere
    ast_deflection_to_shear     0      bit for bit
"""
import math

import numpy as np
from scipy import ndimage
from scipy.ndimage import _filters as _ndfilters

U = 2.0 ** -53
TINY = 5e-324                               # one subnormal step
MODES = {0: "reflect", 1: "nearest"}        # the mode codes of ast_gaussian_filter_order


def extend_idx(i, n, mode):
    """extend_idx of filters.hip: 0 = "reflect" (d c b a | a b c d | d c b a), 1 = "nearest"; any number of laps."""
    i = np.asarray(i)
    if mode == 1:
        return np.clip(i, 0, n - 1)
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def border_distance(npix):
    """(npix, npix) int: pixels between each pixel and the nearest map edge, per axis: (rows, columns)."""
    k = np.arange(npix)
    d = np.minimum(k, npix - 1 - k)
    return np.broadcast_to(d[:, None], (npix, npix)), np.broadcast_to(d[None, :], (npix, npix))


def exceeds(a, b, bound):
    """Pixels where a and b differ by more than the bound; NaN against a number, or NaN against NaN the other way
    round, counts as exceeding only if one side alone is NaN."""
    a, b = np.asarray(a), np.asarray(b)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a) | np.isnan(b), np.isnan(a) != np.isnan(b), np.abs(a - b) > bound)


def worst_ratio(got, ref, bound):
    """max err / bound over the pixels (0 / 0 = 0; anything over a zero bound = inf)."""
    err = np.abs(np.asarray(got) - np.asarray(ref))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ ast_convolve2d
def convolve_reference(img, w, mode="reflect"):
    return ndimage.convolve(img, w, mode=mode)


def convolve_bound(img, w):
    return 2.0 * w.size * U * ndimage.convolve(np.abs(img), np.abs(w))


def convolve_model(img, w, shift=True, flip=True):
    """convolve2d_kernel op by op: out[i, j] = sum_{a, b} img[i + a - ca, j + b - cb] * w[kh-1-a, kw-1-b], reflected,
    ca = kh / 2 - (kh even), taps added row-major onto 0.0.  shift=False, flip=False: the wrong kernels."""
    n = img.shape[0]
    kh, kw = w.shape
    ca = kh // 2 - (1 if shift and kh % 2 == 0 else 0)
    cb = kw // 2 - (1 if shift and kw % 2 == 0 else 0)
    cols = [extend_idx(np.arange(n) + b - cb, n, 0) for b in range(kw)]
    acc = np.zeros((n, n))
    for a in range(kh):
        rows = img[extend_idx(np.arange(n) + a - ca, n, 0)]
        for b in range(kw):
            acc += rows[:, cols[b]] * (w[kh - 1 - a, kw - 1 - b] if flip else w[a, b])
    return acc


CONVOLVE_MUTATIONS = {
    "no_origin_shift": lambda img, w: convolve_model(img, w, shift=False),
    "no_flip": lambda img, w: convolve_model(img, w, flip=False),
    "mirror": lambda img, w: convolve_reference(img, w, mode="mirror"),
}


def integer_window(kh, kw, seed):
    """kh x kw distinct integers 1 .. kh kw in a seeded order."""
    return np.random.default_rng(seed).permutation(kh * kw).reshape(kh, kw).astype(np.float64) + 1.0


def convolve_impulse_cases():
    """(name, img, w): one 1.0 on a zero map at a corner or around the 16-pixel tile boundary; windows of distinct
    integers.  Every product is by 1 or 0 and every sum is of small integers: the output is exact."""
    out = []
    for n in (15, 16, 17, 33):
        spots = [p for p in ((0, 0), (n - 1, n - 1), (15, 15), (15, 16), (16, 15), (16, 16)) if max(p) < n]
        for kh, kw in ((3, 4), (4, 3), (6, 5), (8, 8)):
            w = integer_window(kh, kw, 100 * kh + kw)
            for p in dict.fromkeys(spots):
                img = np.zeros((n, n))
                img[p] = 1.0
                out.append((f"impulse_n{n}_w{kh}x{kw}_at{p[0]}_{p[1]}", img, w))
    return out


LDS_LIMIT_BYTES = 65536
LDS_WINDOWS = ((49, 113, True), (113, 49, True), (50, 113, False), (49, 114, False))     # (kh, kw, staged in LDS)


def convolve_lds_cases():
    """(name, img, w, staged): random image and window on either side of (15 + kh) (15 + kw) 8 <= 65536."""
    out = []
    for n in (20, 33):
        for kh, kw, staged in LDS_WINDOWS:
            rng = np.random.default_rng(1000 * n + kh + kw)
            out.append((f"lds_n{n}_w{kh}x{kw}", rng.standard_normal((n, n)), rng.standard_normal((kh, kw)), staged))
    return out


def convolve_lap_cases():
    """(name, img, w): windows that reach over the map more than once (several laps of the reflection)."""
    out = []
    for n in (1, 2, 5, 7):
        for kh, kw in ((3, 3), (5, 4), (13, 2), (1, 16), (12, 13)):
            rng = np.random.default_rng(10 * n + kh * kw)
            out.append((f"lap_n{n}_w{kh}x{kw}", rng.standard_normal((n, n)), rng.standard_normal((kh, kw))))
    return out


def convolve_discriminators(img, w):
    """The mutations that can differ for this case: none on a one-pixel map (every extension of it is that pixel);
    the origin shift only for an even extent."""
    if img.shape[0] == 1:
        return ()
    kh, kw = w.shape
    return (("no_origin_shift",) if kh % 2 == 0 or kw % 2 == 0 else ()) + ("no_flip", "mirror")


# ------------------------------------------------------------------------------------- ast_gaussian_filter_order
GAUSS_NPIX = (1, 2, 3, 5, 17)
GAUSS_SIGMAS = (0.1, 0.124, 0.126, 0.3, 1.3, 5.0)       # radius 0, 0, 1, 1, 5, 20
GAUSS_ORDERS = tuple((o, 0) for o in range(9)) + tuple((0, o) for o in range(1, 9)) + ((8, 7), (5, 4), (3, 3), (1, 2))


def gauss_radius(sigma):
    return int(4.0 * sigma + 0.5)


def gauss_work_doubles(npix, sigma):
    return npix * npix + 2 * (2 * gauss_radius(sigma) + 1)


def gauss_image(npix, seed=0):
    return np.random.default_rng(7000 + 10 * npix + seed).standard_normal((npix, npix))


def scipy_taps(sigma, order, radius):
    """The taps ndimage.gaussian_filter1d hands to correlate1d."""
    return _ndfilters._gaussian_kernel1d(sigma, order, radius)[::-1]


def host_taps(sigma, order, radius):
    """gaussian_kernel1d of filters.hip in float64, op by op (math.exp and math.pow are the C library's)."""
    sigma2 = sigma * sigma
    phi = [math.exp(-0.5 / sigma2 * float(k * k)) for k in range(-radius, radius + 1)]
    total = 0.0
    for v in phi:
        total += v
    phi = [v / total for v in phi]
    if order == 0:
        return np.array(phi)
    q = [1.0] + [0.0] * order
    for _ in range(order):
        t = []
        for r in range(order + 1):
            v = 0.0
            if r + 1 <= order:
                v += float(r + 1) * q[r + 1]
            if r >= 1:
                v += (1.0 / -sigma2) * q[r - 1]
            t.append(v)
        q = t
    w = []
    for k in range(-radius, radius + 1):
        v = 0.0
        for e in range(order + 1):
            v += math.pow(float(k), float(e)) * q[e]
        w.append(v * phi[k + radius])
    return np.array(w[::-1])


def exact_taps(sigma, order, radius):
    """_gaussian_kernel1d(sigma, order, radius)[::-1] in np.longdouble."""
    L = np.longdouble
    sigma2 = L(sigma) * L(sigma)
    x = np.arange(-radius, radius + 1).astype(L)
    phi = np.exp(L(-0.5) / sigma2 * x ** 2)
    phi = phi / phi.sum()
    if order == 0:
        return phi[::-1]
    q = np.zeros(order + 1, dtype=L)
    q[0] = 1
    Q = np.diag(np.arange(1, order + 1).astype(L), 1) + np.diag(np.ones(order, dtype=L) / -sigma2, -1)
    for _ in range(order):
        q = Q.dot(q)
    return ((x[:, None] ** np.arange(order + 1)).dot(q) * phi)[::-1]


_tau = {}


def tap_tau(sigma, order):
    """max|w_scipy - w_exact| / max|w_exact| (0 for taps that are all zero)."""
    key = (sigma, order)
    if key not in _tau:
        r = gauss_radius(sigma)
        exact = exact_taps(sigma, order, r)
        top = np.abs(exact).max()
        _tau[key] = float(np.abs(scipy_taps(sigma, order, r).astype(np.longdouble) - exact).max() / top) if top else 0.0
    return _tau[key]


def gaussian_reference(img, sigma, order0, order1, mode):
    """mode: a code of MODES or one of ndimage's names (the mutations)."""
    return ndimage.gaussian_filter(img, sigma, order=(order0, order1), mode=MODES.get(mode, mode))


def gaussian_bound(img, sigma, order0, order1, mode):
    r, m = gauss_radius(sigma), MODES[mode]
    k = 2 * r + 1
    w0, w1 = np.abs(scipy_taps(sigma, order0, r)), np.abs(scipy_taps(sigma, order1, r))
    box, a = np.ones(k), np.abs(img)
    c = lambda x, w, axis: ndimage.correlate1d(x, w, axis=axis, mode=m)
    first = c(a, w0, 0)
    taps = 5.0 * tap_tau(sigma, order0) * w0.max() * c(c(a, box, 0), w1, 1) \
        + 5.0 * tap_tau(sigma, order1) * w1.max() * c(first, box, 1)
    return 2.0 * (k + k) * U * c(first, w1, 1) + taps


def correlate1d_model(a, axis, w, radius, sym, mode):
    """correlate1d_kernel op by op: the centre tap, then pairs from the outermost inwards."""
    n = a.shape[0]
    c = np.arange(n)

    def at(k):
        idx = extend_idx(c + k, n, mode)
        return a[idx, :] if axis == 0 else a[:, idx]
    acc = at(0) * w[radius]
    for k in range(-radius, 0):
        acc = acc + ((at(k) + at(-k)) if sym > 0 else (at(k) - at(-k))) * w[k + radius]
    return acc


def gaussian_model(img, sigma, order0, order1, mode):
    """ast_gaussian_filter_order: host taps, symmetric path for an even order, antisymmetric for an odd one."""
    r = gauss_radius(sigma)
    tmp = correlate1d_model(img, 0, host_taps(sigma, order0, r), r, -1 if order0 & 1 else 1, mode)
    return correlate1d_model(tmp, 1, host_taps(sigma, order1, r), r, -1 if order1 & 1 else 1, mode)


def gaussian_mutation(npix, sigma, mode):
    """The wrong boundary of a case, or None where no boundary can matter (one pixel; a single tap).  "mirror" for
    "reflect"; "reflect" for "nearest" - but with radius 1 those two read the same pixels (index -1 is pixel 0 under
    both), and the remaining wrong boundary, "mirror", stands in."""
    r = gauss_radius(sigma)
    if npix == 1 or r == 0:
        return None
    if mode == 0:
        return "mirror"
    return "reflect" if r > 1 else "mirror"


# ------------------------------------------------------------------------------------------------ ast_dgd_filter
DGD_NPIX = (3, 4, 5, 16, 17, 64)


def dgd_params(npix):
    """(sigma_pix, h, axis, order) of a map size."""
    return [(float(s), h, axis, order) for s in (1, 2, npix, 4 * npix) for h in (1.0, 2.0 / npix) for axis in (0, 1)
            for order in (1, 3)]


def dgd_image(npix):
    return np.random.default_rng(9000 + npix).standard_normal((npix, npix))


def _dgd_terms(npix, sigma, order):
    """The Gaussians of the window and their exp arguments, op by op as dgd_base_kernel and numpy both compute them."""
    x1 = np.linspace(1, npix, npix) - npix / 2 - 0.5
    x, y = np.meshgrid(x1, x1)
    dist = np.sqrt(x * x + y * y)
    sig = (sigma * 0.5, sigma, sigma * 2.0) if order == 3 else (sigma * 0.5,)
    args = [-(dist * dist) / (2.0 * (s * s)) for s in sig]
    return [np.exp(a) / (2.0 * np.pi * (s * s)) for a, s in zip(args, sig)], args


def dgd_window(npix, sigma, order):
    g, _ = _dgd_terms(npix, sigma, order)
    return (g[0] - g[1]) + g[2] if order == 3 else g[0]


def dgd_reference(img, sigma, h, axis, order, edge_order=2):
    """Filters.gaussian_third_derivative / gaussian_first_derivative with the window width and pixel size given
    directly.  edge_order=1: the wrong border stencil."""
    w = dgd_window(img.shape[0], sigma, order)
    for _ in range(order):
        w = np.gradient(w, h, axis=axis, edge_order=edge_order)
    return np.multiply(w, img)


def _stencil(f, axis, h, absolute):
    """gradient_kernel op by op (absolute=False), or the same stencil with absolute coefficients."""
    f = np.moveaxis(f, axis, 0)
    out = np.empty_like(f)
    if absolute:
        out[1:-1] = (f[2:] + f[:-2]) / (2.0 * h)
        out[0] = (1.5 / h) * f[0] + (2.0 / h) * f[1] + (0.5 / h) * f[2]
        out[-1] = (0.5 / h) * f[-3] + (2.0 / h) * f[-2] + (1.5 / h) * f[-1]
    else:
        out[1:-1] = (f[2:] - f[:-2]) / (2.0 * h)
        out[0] = (-1.5 / h) * f[0] + (2.0 / h) * f[1] + (-0.5 / h) * f[2]
        out[-1] = (0.5 / h) * f[-3] + (-2.0 / h) * f[-2] + (1.5 / h) * f[-1]
    return np.moveaxis(out, 0, axis)


def dgd_model(img, sigma, h, axis, order):
    w = dgd_window(img.shape[0], sigma, order)
    for _ in range(order):
        w = _stencil(w, axis, h, False)
    return w * img


def dgd_bound(img, sigma, h, axis, order):
    g, args = _dgd_terms(img.shape[0], sigma, order)
    mag = sum(np.abs(t) for t in g)
    err = sum(np.abs(t) * (5.0 * np.abs(a) + 5.0) * U for t, a in zip(g, args)) + 2.0 * U * mag + 4.0 * TINY
    w = dgd_window(img.shape[0], sigma, order)
    for _ in range(order):
        err = _stencil(err, axis, h, True) + 4.0 * U * _stencil(np.abs(w) + err, axis, h, True) + 4.0 * TINY
        w = np.gradient(w, h, axis=axis, edge_order=2)
    return 2.0 * (np.abs(img) * err + U * np.abs(w * img) + TINY)


def dgd_window_border_is_zero(npix, sigma, order):
    """The three outermost rows and columns of the window underflow to 0.0: every border stencil, of either edge
    order, reads zeros alone (64 pixels, sigma_pix 1, order 1)."""
    w = dgd_window(npix, sigma, order)
    return npix >= 6 and not (w[:3].any() or w[-3:].any() or w[:, :3].any() or w[:, -3:].any())


# --------------------------------------------------------------------------------------- ast_aperture_photometry
# (npix, alpha_pix): (pixels of the strict ring, of the ring closed on both sides)
RING_COUNTS = {
    (31, 5): (68, 92),              # 12 pixels exactly at d = 5, 12 exactly at d = 5 sqrt 2
    (11, 5): (36, 52),              # ring cut by the border
    (9, 5): (4, 12),                # the corners only
    (301, 61): (11672, 11696),
    (2, 1): (0, 0),                 # empty
    (3, 0): (0, 1),                 # strict ring empty
    (1, 0): (0, 1),                 # strict ring empty
    (513, 100): None,               # filled in below: more pixels than the 262144 threads of the partial kernel
    (16, 40): (0, 0),               # ring wholly off the map
}
RING_THREADS = 1024 * 256


def ring_mask(npix, alpha, inner_closed=False, outer_closed=False):
    """in_ring of filters.hip: alpha < d < alpha sqrt(2), d the distance to the map centre; *_closed: the wrong rings."""
    x1 = np.arange(1, npix + 1, dtype=np.float64) - npix / 2.0 - 0.5
    x, y = np.meshgrid(x1, x1)
    d = np.sqrt(x * x + y * y)
    lo = alpha <= d if inner_closed else alpha < d
    hi = d <= alpha * np.sqrt(2.0) if outer_closed else d < alpha * np.sqrt(2.0)
    return np.logical_and(lo, hi)


RING_COUNTS[(513, 100)] = (int(ring_mask(513, 100.0).sum()), int(ring_mask(513, 100.0, True, True).sum()))


def aperture_image(npix):
    return np.random.default_rng(5000 + npix).standard_normal((npix, npix)) + 3.0


def aperture_reference(img, alpha, inner_closed=False, outer_closed=False):
    """Filters.aperture_photometry: NaN everywhere for an empty ring, like np.mean of nothing."""
    ring = ring_mask(img.shape[0], float(alpha), inner_closed, outer_closed)
    if not ring.any():
        return np.full_like(img, np.nan)
    return img - np.mean(img[ring])


def aperture_bound(img, alpha):
    ring = ring_mask(img.shape[0], float(alpha))
    n = int(ring.sum())
    mean_abs = float(np.abs(img[ring]).mean()) if n else 0.0
    return 2.0 * n * U * mean_abs + U * np.abs(img)


def _tree256(v):
    """The LDS tree of the ring kernels over the last axis (256 wide)."""
    v = v.copy()
    k = 128
    while k > 0:
        v[..., :k] = v[..., :k] + v[..., k:2 * k]
        k >>= 1
    return v[..., 0]


def aperture_model(img, alpha):
    """ring_partial_kernel, ring_final_kernel and subtract_scalar_kernel op by op: thread t of block b adds pixels
    b 256 + t + m 262144 in order of m; a 256-wide tree per block; thread t adds blocks t, t + 256, ...; a tree; s / c."""
    flat = img.ravel()
    ring = ring_mask(img.shape[0], float(alpha)).ravel()
    laps = -(-flat.size // RING_THREADS)
    vals = np.zeros(laps * RING_THREADS)
    cnts = np.zeros(laps * RING_THREADS)
    vals[:flat.size] = np.where(ring, flat, 0.0)
    cnts[:flat.size] = ring
    s, c = np.zeros(RING_THREADS), np.zeros(RING_THREADS)
    for m in range(laps):                       # (adding 0.0 for a pixel outside the ring changes no sum)
        s = s + vals[m * RING_THREADS:(m + 1) * RING_THREADS]
        c = c + cnts[m * RING_THREADS:(m + 1) * RING_THREADS]
    psum, pcnt = _tree256(s.reshape(1024, 256)), _tree256(c.reshape(1024, 256))
    s2, c2 = np.zeros(256), np.zeros(256)
    for b in range(4):
        s2 = s2 + psum[b * 256:(b + 1) * 256]
        c2 = c2 + pcnt[b * 256:(b + 1) * 256]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = _tree256(s2) / _tree256(c2)
    return img - mean


# ----------------------------------------------------------------------------------------------- ast_hann_apodize
HANN_NPIX = (1, 2, 3, 16, 17)


def hann_image(npix):
    return np.random.default_rng(3000 + npix).standard_normal((npix, npix))


def hann_reference(img):
    """Filters.apodization: img * outer(hann(n), hann(n)) with scipy's symmetric window; hann(1) = [1.]."""
    from scipy.signal.windows import hann
    h = hann(img.shape[0])
    return img * np.outer(h, h)


def hann_bound(img):
    return 8.0 * U * np.abs(img)


def hann_model(img):
    n = img.shape[0]
    if n == 1:
        return img * (1.0 * 1.0)
    f = 2.0 * np.pi / float(n - 1)
    w = 0.5 - 0.5 * np.cos(f * np.arange(n, dtype=np.float64))
    return img * (w[:, None] * w[None, :])


# ------------------------------------------------------------------------------------------------ ast_zoom_linear
ZOOM_SHAPES = ((1, 1), (2, 1), (3, 2), (5, 1), (7, 3), (16, 8), (15, 5), (4, 4), (17, 17))


def zoom_image(nin, nout):
    """Integer-valued for (16, 8), where the 2 x 2 block means are then exact."""
    rng = np.random.default_rng(100 * nin + nout)
    if (nin, nout) == (16, 8):
        return rng.integers(-1000, 1000, (nin, nin)).astype(np.float64)
    return rng.standard_normal((nin, nin))


def zoom_reference(img, nout, grid_mode=True):
    """grid_mode=False: the wrong kernel that samples at pixel corners."""
    nin = img.shape[0]
    return ndimage.zoom(img, (nout / nin, nout / nin), order=1, mode="mirror", cval=0.0, grid_mode=grid_mode)


def _zoom_terms(img, nout):
    nin = img.shape[0]
    zoom = float(nin) / float(nout)
    c = (np.arange(nout, dtype=np.float64) + 0.5) * zoom - 0.5
    i0 = np.floor(c).astype(np.int64)
    t = c - i0.astype(np.float64)
    i1 = np.minimum(i0 + 1, nin - 1)
    wa, wb = 1.0 - t, t
    r0, r1, c0, c1 = i0[:, None], i1[:, None], i0[None, :], i1[None, :]
    return (img[r0, c0] * (wa[:, None] * wa[None, :]), img[r0, c1] * (wa[:, None] * wb[None, :]),
            img[r1, c0] * (wb[:, None] * wa[None, :]), img[r1, c1] * (wb[:, None] * wb[None, :]))


def zoom_model(img, nout):
    """zoom_linear_kernel op by op: rows outer, columns inner."""
    a, b, c, d = _zoom_terms(img, nout)
    return ((a + b) + c) + d


def zoom_bound(img, nout):
    return 8.0 * U * sum(np.abs(t) for t in _zoom_terms(img, nout))


def zoom_exact(img, nout):
    """The exact answer where there is one, else None: the input itself for nout == nin (every sample is a pixel
    centre, weight 1); the mean of each 2 x 2 block of an integer-valued image for (16, 8) (all four weights 1/4);
    the centre pixel of each 3 x 3 block for (15, 5) (the samples are pixel centres)."""
    nin = img.shape[0]
    if nout == nin:
        return img.copy()
    if (nin, nout) == (16, 8):
        return img.reshape(8, 2, 8, 2).sum(axis=(1, 3)) / 4.0
    if (nin, nout) == (15, 5):
        return img[1::3, 1::3].copy()
    return None
