"""A numpy restatement of the plane-paint contract (include/astrild_hip.h: ast_plane_paint_accumulate /
ast_plane_paint_finish) and of ``LensPlanes``' factors and weights, so that the GPU results can be asked for the same
BITS.  numpy only; a helper module: no test functions.

All arithmetic is float64, one rounding per written operation, in the contract's order.  The integer sums are formed
with ``np.add.at`` on int64: integer addition is associative, so no order needs restating.
"""
import math

import numpy as np

SUPPORT = {"ngp": 1, "cic": 2, "tsc": 3}
LO = {"ngp": 0, "cic": 0, "tsc": 1}
D_HUBBLE = 2997.92458


def exponent(np_total):
    return min(50, 62 - int(np_total).bit_length())


def box_coefficients(nplanes, npix, boxsize, shift=-0.5):
    """(cl, c1, c0) of the box."""
    return float(nplanes) / float(boxsize), float(npix) / float(boxsize), float(shift)


def cone_coefficients(npix, opening_angle_deg, shift=-0.5):
    """(c1, c0) of the cone: pixels per unit tangent, and the pixel coordinate of the line of sight."""
    return float(npix) / (2.0 * math.tan(0.5 * math.radians(float(opening_angle_deg)))), 0.5 * float(npix) + float(shift)


def _weights(frac, window):
    if window == "ngp":
        return [np.ones_like(frac)]
    if window == "cic":
        return [1.0 - frac, frac]
    hm, hp = 0.5 - frac, 0.5 + frac
    return [0.5 * (hm * hm), 0.75 - frac * frac, 0.5 * (hp * hp)]


def _locate(s, n, window):
    """ast::locate<W> followed by the clamp to [0, n - 1]: base pixel (int64) and offset."""
    fl = np.floor(s if window == "cic" else s + 0.5)
    frac = s - fl
    dn = float(n)
    inv_dn = 1.0 / dn
    r = fl - np.floor(fl * inv_dn) * dn
    r = np.where(r >= dn, r - dn, r)
    r = np.where(r < 0.0, r + dn, r)
    return np.clip(r, 0.0, dn - 1.0).astype(np.int64), frac


def _wrap1(i, n):
    i = np.where(i < 0, i + n, i)
    return np.where(i >= n, i - n, i)


def _axes(los):
    return [c for c in range(3) if c != los]


def accumulate(sums, counters, pos, mass, geometry, window, los, np_total, vmax, scale=1.0, boxsize=None, shift=-0.5,
               opening_angle_deg=None, chi_edges=None, origin=(0.0, 0.0, 0.0), unrounded=None):
    """``sums`` (P, npix, npix) int64 and ``counters`` (3,) int64 are added to in place; returns invq = 2^k / vmax, the
    reciprocal of the quantum, as the kernel multiplies by it.
    ``unrounded``: ``(T, K)``, longdouble and int64 arrays shaped like ``sums`` that receive, per pixel, the sum of the
    float64 products ``t * invq`` - the terms in quanta, before their one rounding to an integer - and the number of terms."""
    P, npix = sums.shape[0], sums.shape[1]
    window = window.lower()
    W, lo = SUPPORT[window], LO[window]
    a, b = _axes(los)
    x = np.asarray(pos).astype(np.float64)
    vmax = float(vmax)
    invq = 2.0 ** exponent(np_total) / vmax
    with np.errstate(all="ignore"):
        ms = (np.ones(len(x)) if mass is None else np.asarray(mass).astype(np.float64)) * float(scale)
        accepted = np.abs(ms) <= vmax
        counters[2] += int(np.count_nonzero(~accepted))
        if geometry == "box":
            cl, c1, c0 = box_coefficients(P, npix, boxsize, shift)
            sl = x[:, los] * cl
            sa = x[:, a] * c1 + c0
            sb = x[:, b] * c1 + c0
            inside = np.isfinite(sl) & np.isfinite(sa) & np.isfinite(sb)
            use = accepted & inside
            counters[0] += int(np.count_nonzero(accepted & ~inside))
            sl, sa, sb, ms = sl[use], sa[use], sb[use], ms[use]
            plane, _ = _locate(sl, P, "cic")
            ba, fa = _locate(sa, npix, window)
            bb, fb = _locate(sb, npix, window)
        else:
            c1, c0 = cone_coefficients(npix, opening_angle_deg, shift)
            e = np.asarray(chi_edges, dtype=np.float64)
            e2 = e * e
            d = x - np.asarray(origin, dtype=np.float64)[None, :]
            r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            inside = np.isfinite(d).all(axis=1) & (d[:, los] > 0.0) & (r2 >= e2[0]) & (r2 < e2[P])
            use = accepted & inside
            outside = accepted & ~inside
            d, r2, ms = d[use], r2[use], ms[use]
            plane = np.searchsorted(e2, r2, side="right").astype(np.int64) - 1
            base, frac = [], []
            for c in (a, b):
                s = (d[:, c] / d[:, los]) * c1 + c0
                fl = np.floor(s if window == "cic" else s + 0.5)
                frac.append(s - fl)
                base.append(np.clip(fl, -2.0, float(npix) + 1.0).astype(np.int64))
            (ba, bb), (fa, fb) = base, frac
        wa, wb = _weights(fa, window), _weights(fb, window)
        kept = np.zeros(len(ms), dtype=np.int64)
        for i in range(W):
            ia = ba - lo + i
            for j in range(W):
                ib = bb - lo + j
                t = ((ms * wa[i]) * wb[j]) * invq
                r = np.rint(t)
                if geometry == "box":
                    ok = np.ones(len(ms), dtype=bool)
                    where = (plane, _wrap1(ia, npix), _wrap1(ib, npix))
                else:
                    ok = (ia >= 0) & (ia < npix) & (ib >= 0) & (ib < npix)
                    where = (plane[ok], ia[ok], ib[ok])
                    kept += ok
                np.add.at(sums, where, r[ok].astype(np.int64))
                if unrounded is not None:
                    np.add.at(unrounded[0], where, t[ok].astype(np.longdouble))
                    np.add.at(unrounded[1], where, 1)
        if geometry == "cone":
            counters[0] += int(np.count_nonzero(outside)) + int(np.count_nonzero(kept == 0))
            counters[1] += int(np.count_nonzero((kept > 0) & (kept < W * W)))
    return invq


def paint(pos, mass, geometry, nplanes, npix, window, los=2, np_total=None, vmax=None, **kw):
    """Fresh ``(sums, counters, invq)``; ``np_total`` defaults to len(pos), ``vmax`` to max |mass| |scale| (1 without masses)."""
    sums = np.zeros((nplanes, npix, npix), dtype=np.int64)
    counters = np.zeros(3, dtype=np.int64)
    if np_total is None:
        np_total = len(pos)
    if vmax is None:
        vmax = (1.0 if mass is None else float(np.abs(np.asarray(mass).astype(np.float64)).max())) * (abs(kw.get("scale", 1.0)) or 1.0)
    invq = accumulate(sums, counters, pos, mass, geometry, window, los, np_total, vmax, **kw)
    return sums, counters, invq


def cone_factor(npix, c1):
    """(npix, npix) float64: w sqrt(w), w = (1 + ta ta) + tb tb at the pixel centres - the finish kernel's cos^-3."""
    t = ((np.arange(npix, dtype=np.float64) + 0.5) - 0.5 * float(npix)) / float(c1)
    w = (1.0 + (t * t)[:, None]) + (t * t)[None, :]
    return w * np.sqrt(w)


def finish(sums, mul, add, geometry, dtype, c1=None):
    """out = dtype((double)sums * mul[p] (* cone_factor) + add[p])."""
    mul, add = np.asarray(mul, dtype=np.float64), np.asarray(add, dtype=np.float64)
    v = sums.astype(np.float64) * mul[:, None, None]
    if geometry == "cone":
        v = v * cone_factor(sums.shape[1], c1)[None, :, :]
    return (v + add[:, None, None]).astype(dtype)


# ------------------------------------------------------------------ LensPlanes in plain float64
def plane_factors(geometry, npix, chi_edges, mean_density, np_total, vmax, boxsize=None, opening_angle_deg=None):
    """(mul, add): D_p = dchi_p (M_pix / Mbar_p - 1) as an affine map of the integer sums."""
    e = np.asarray(chi_edges, dtype=np.float64)
    lo, hi = e[:-1], e[1:]
    dchi = hi - lo
    q = float(vmax) / 2.0 ** exponent(np_total)
    rho = float(mean_density)
    if geometry == "box":
        side = float(boxsize) / float(npix)
        mul = np.full(dchi.shape, q / (rho * (side * side)))
    else:
        side = 2.0 * math.tan(0.5 * math.radians(float(opening_angle_deg))) / float(npix)
        mul = q * dchi / (rho * (side * side) * ((hi * hi * hi - lo * lo * lo) / 3.0))
    return mul, -dchi


def comoving(z, omega_m, points=64, parts=8):
    """chi(z) in Mpc/h of a scalar z: ``points``-point Gauss-Legendre quadrature on each of ``parts`` equal pieces of
    [y, 1], y = (1 + z)^-1/2, of 2 D_H / sqrt(Omega_m + (1 - Omega_m) t^6) - another rule than the product's.  The
    integrand is analytic on [0, 1]; one piece of 128 points gives the same value within 2e-11 Mpc/h for Omega_m >= 0.1."""
    x, w = np.polynomial.legendre.leggauss(points)
    edges = np.linspace(1.0 / math.sqrt(1.0 + float(z)), 1.0, parts + 1)
    total = 0.0
    for lo, hi in zip(edges[:-1], edges[1:]):
        t = 0.5 * (lo + hi) + 0.5 * (hi - lo) * x
        total += 0.5 * (hi - lo) * float(np.sum(w / np.sqrt(omega_m + (1.0 - omega_m) * t ** 6)))
    return 2.0 * D_HUBBLE * total


def eds_comoving(z):
    return 2.0 * D_HUBBLE * (1.0 - 1.0 / np.sqrt(1.0 + np.asarray(z, dtype=np.float64)))


def source_weights(chi, a, chi_s, omega_m):
    """(wnum, wden): W_p = wnum_p / wden_p = 1.5 Omega_m D_H^-2 g(chi_p, chi_s) / a_p, 0 from chi_p >= chi_s on."""
    chi = np.asarray(chi, dtype=np.float64)
    pref = 1.5 * float(omega_m) * (1.0 / D_HUBBLE) ** 2
    g = np.where(chi < chi_s, (chi_s - chi) * chi / chi_s, 0.0)
    return pref * g, np.asarray(a, dtype=np.float64)


def stack(planes, wnum, wden):
    """``lensing.kappa_stack``'s rule (tests/test_gpu_kappa.py): per plane the term T(float64(plane) * wnum / wden), T the
    planes' dtype, summed in plane order in T, the first term copied."""
    total = None
    for p in range(len(planes)):
        term = (planes[p].astype(np.float64) * wnum[p] / wden[p]).astype(planes.dtype)
        total = term.copy() if total is None else total + term
    return total


# ------------------------------------------------------------------ inputs
def lattice(ns, boxsize):
    g = (np.arange(ns) + 0.5) * (float(boxsize) / ns)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def particles(count, boxsize, seed, dtype=np.float64, masses=True):
    """``count`` positions uniform in [-L, 2 L)^3 and masses in [0.5, 2): random, non-dyadic."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-boxsize, 2.0 * boxsize, size=(count, 3)).astype(dtype)
    mass = rng.uniform(0.5, 2.0, size=count).astype(dtype) if masses else None
    return pos, mass
