"""Lens planes from particles, and Born-approximation convergence maps over them.

The reference reads its lens planes from Ray-Ramses output and has no code that makes them (hard part 6).
``LensPlanes`` paints particles - a periodic box seen plane-parallel, or a light cone seen through a gnomonic
(tangent-plane) map - into P planes that stay on the device, in the units the stack wants, and sums them with the lensing
kernel for any number of source redshifts (``lensing.kappa_stack``).

Conventions.  Lengths are comoving Mpc/h, D_H = c / H_0 = 2997.92458 Mpc/h.  ``planes[p, ia, ib]``: (a, b) are the two
axes other than ``los`` in increasing order; pixel i covers [i, i + 1) and its centre sits at i + 1/2.  Box: pixel
coordinate ``x npix / L``, plane p spans ``chi0 + [p, p + 1) L / P`` along ``los``.  Cone: the observer looks along
+``los``; pixel coordinate ``npix / 2 + (d_a / d_los) npix / (2 tan(theta / 2))``, the map spans ``theta`` between its
edges through the centre; plane p is the radial shell ``chi_edges[p] <= |d| < chi_edges[p + 1]``.  Every plane holds
``D_p = dchi_p (M_pix / Mbar_p - 1)``, the density contrast integrated through the plane, with Mbar_p the mass a pixel
of that plane holds at the mean density: ``rho (L / npix)^2 dchi_p`` (box), ``rho (2 tan(theta / 2) / npix)^2
(chi_hi^3 - chi_lo^3) / 3`` per unit cos^-3 (cone: gnomonic pixels shrink in solid angle as cos^3 off axis, and the
finish kernel divides that out).  Then ``kappa = sum_p W_p D_p``, ``W_p = 3/2 Omega_m D_H^-2 g(chi_p, chi_s) / a_p`` with
g = (chi_s - chi) chi / chi_s at the plane's mid-point and 0 from chi_p >= chi_s on: the Born approximation, no
lens-lens coupling.  ``ray_trace`` goes beyond it: multi-plane ray tracing over the same planes gives convergence, shear,
rotation and deflection with lens-lens coupling (``astrild_amd.ray_trace``)."""
import math

import numpy as np
import torch

from .. import device as dev, lensing, plane_paint as pp, ray_trace as rt

D_HUBBLE = 2997.92458              # c / (100 km/s/Mpc) in Mpc/h
SIMPSON_STEPS = 512


def _unit_integral(y, omega_m):
    """int_y^1 dt / sqrt(Omega_m + (1 - Omega_m) t^6), composite Simpson with SIMPSON_STEPS intervals per element."""
    y = np.asarray(y, dtype=np.float64)
    om = float(omega_m)
    k = np.arange(SIMPSON_STEPS + 1, dtype=np.float64)
    w = np.where(k % 2 == 1, 4.0, 2.0)
    w[0] = w[-1] = 1.0
    h = (1.0 - y) / SIMPSON_STEPS
    t = y[..., None] + h[..., None] * k
    f = 1.0 / np.sqrt(om + (1.0 - om) * t ** 6)
    return np.sum(f * w, axis=-1) * (h / 3.0)


def _check_omega(omega_m):
    om = float(omega_m)
    if not 0.0 < om <= 1.0:
        raise ValueError(f"omega_m must lie in (0, 1] (flat LCDM), got {omega_m!r}")
    return om


def flat_lcdm_comoving(z, omega_m):
    """Comoving distance in Mpc/h of redshift ``z`` (scalar or array, >= 0) in flat LCDM:
    ``chi = D_H int_0^z dz' / E(z')``, ``E^2 = Omega_m (1 + z)^3 + 1 - Omega_m``.  With y = (1 + z)^-1/2 this is
    ``2 D_H int_y^1 dt / sqrt(Omega_m + (1 - Omega_m) t^6)``: a bounded, smooth integrand at every redshift, constant
    for Einstein-de Sitter.  Composite Simpson rule with 512 intervals, numpy on the host.  Error: for Omega_m = 1 the
    integrand is the constant 1, the weighted sum is the integer 1536 in any order and 1536 fl(h / 3) = 512 h exactly, so
    the result equals the closed form 2 D_H (1 - 1 / sqrt(1 + z)) bit for bit.  For Omega_m = 0.1, 0.3, 0.7 the largest
    error over z = 0 .. 1100, measured against 8 x 64-point Gauss-Legendre quadrature (itself good to 2e-11), is 9.1e-9,
    7.5e-9 and 3.2e-9 Mpc/h, reached at z = 1100 (z <= 10: 3.6e-9 at most); 256 intervals would give 16 times that.  The
    analytic remainder (1 - y)^5 max |f''''| / (180 x 512^4) with |f''''| < 1600 on [0, 1] for Omega_m >= 0.1 bounds it
    by 7.8e-7 Mpc/h."""
    om = _check_omega(omega_m)
    zz = np.asarray(z, dtype=np.float64)
    if not (np.isfinite(zz).all() and (zz >= 0).all()):
        raise ValueError(f"z must be finite and >= 0, got {z!r}")
    chi = 2.0 * D_HUBBLE * _unit_integral(1.0 / np.sqrt(1.0 + zz), om)
    return float(chi) if np.ndim(z) == 0 else chi


def flat_lcdm_redshift(chi, omega_m):
    """The inverse of :func:`flat_lcdm_comoving`: the redshift of comoving distance ``chi`` (Mpc/h, scalar or array,
    0 <= chi below the horizon).  Newton's method on y = (1 + z)^-1/2 from the Einstein-de Sitter value, a fixed 40
    steps of the same quadrature (``d chi / d y = -2 D_H / sqrt(Omega_m + (1 - Omega_m) y^6)`` is known in closed form
    and never vanishes).  Round trip z -> chi -> z, measured for Omega_m = 0.1, 0.3, 1 and z = 0 .. 1100: off by at most
    2.2 x 2^-53 (1 + z)^(3/2).  The power 3/2: the quadrature's rounding leaves y off by a few 2^-53, and
    z = y^-2 - 1 multiplies an error of y by 2 (1 + z)^(3/2)."""
    om = _check_omega(omega_m)
    c = np.asarray(chi, dtype=np.float64)
    horizon = 2.0 * D_HUBBLE * float(_unit_integral(0.0, om))
    if not (np.isfinite(c).all() and (c >= 0).all() and (c < horizon).all()):
        raise ValueError(f"chi must lie in [0, {horizon:.6g}) Mpc/h (the horizon for omega_m = {om}), got {chi!r}")
    target = c / (2.0 * D_HUBBLE)
    y = np.clip(1.0 - target, 1e-8, 1.0)
    for _ in range(40):
        y = np.clip(y + (_unit_integral(y, om) - target) * np.sqrt(om + (1.0 - om) * y ** 6), 1e-8, 1.0)
    z = 1.0 / (y * y) - 1.0
    return float(z) if np.ndim(chi) == 0 else z


class LensPlanes:
    """P lens planes of npix x npix on the device (module docstring).  Made by :meth:`from_box` (complete on return) or
    :meth:`lightcone` (then :meth:`add` any number of times and :meth:`finish`).

    ``planes``: ``(P, npix, npix)`` device tensor of ``dtype`` holding D_p in Mpc/h (None until finished);
    ``chi``: shell mid-points, ``a``: their scale factors, ``chi_edges``; ``sums`` (int64) and ``counters`` (3 int64:
    outside, clipped, refused) on the device, as ``plane_paint.plane_paint_sums`` leaves them."""

    def __init__(self, geometry, npix, chi_edges, omega_m, mean_density, np_total, vmax, window="cic",
                 dtype=torch.float32, boxsize=None, opening_angle_deg=None, los=2):
        self.geometry, self.window, self.dtype, self.los = geometry, window, dtype, int(los)
        self.npix, self.omega_m = int(npix), float(omega_m)
        self.boxsize, self.opening_angle_deg = boxsize, opening_angle_deg
        self.chi_edges = np.array(chi_edges, dtype=np.float64).reshape(-1)
        self.nplanes = self.chi_edges.size - 1
        self.mean_density = float(mean_density)
        if not (math.isfinite(self.mean_density) and self.mean_density > 0.0):
            raise ValueError(f"mean_density must be positive and finite, got {mean_density!r}")
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"dtype must be torch.float32 or torch.float64, got {dtype!r}")
        # (validates everything else, for an empty particle set)
        self._args = pp.check_plane_paint_args(geometry, (0, 3), np.float64, None, self.nplanes, npix, window, los, np_total,
                                               vmax, 1.0, -0.5, boxsize, opening_angle_deg, self.chi_edges)
        self.np_total, self.vmax = self._args["np_total"], self._args["vmax"]
        self.chi = 0.5 * (self.chi_edges[:-1] + self.chi_edges[1:])
        self.a = 1.0 / (1.0 + flat_lcdm_redshift(self.chi, self.omega_m))
        self.mul, self.add_term = plane_factors(geometry, self.npix, self.chi_edges, self.mean_density, self.np_total,
                                                self.vmax, boxsize, opening_angle_deg)
        self.sums = torch.zeros((self.nplanes, self.npix, self.npix), dtype=torch.int64, device=dev.device())
        self.counters = torch.zeros(3, dtype=torch.int64, device=dev.device())
        self._e2 = pp.upload_doubles(self._args["e2"])[0] if geometry == "cone" else None
        self.planes = None

    @classmethod
    def from_box(cls, pos, mass, boxsize, nplanes, npix, omega_m, chi0=0.0, los=2, window="cic", dtype=torch.float32,
                 mean_density=None):
        """The planes of a periodic box of side ``boxsize`` seen along ``los``: plane p spans
        ``chi0 + [p, p + 1) boxsize / nplanes``.  ``pos`` (N, 3), ``mass`` (N,) or None: device tensors or numpy arrays.
        ``mean_density``: default ``sum(mass) / boxsize^3``.  A NaN or Inf mass raises ValueError."""
        p = dev.dense(dev.as_device(pos))
        m = None if mass is None else dev.dense(dev.as_device(mass, dtype=p.dtype))
        npart = int(p.shape[0])
        box = float(boxsize)
        vmax = dev._mass_bound(m, npart)
        if mean_density is None:
            mean_density = dev.total_mass(m, npart) / (box * box * box)
        edges = float(chi0) + np.arange(int(nplanes) + 1, dtype=np.float64) * (box / int(nplanes))
        self = cls("box", npix, edges, omega_m, mean_density, max(npart, 1), vmax, window, dtype, boxsize=box, los=los)
        pp.plane_paint_sums(p, m, "box", self.nplanes, self.npix, window, los, self.sums, self.counters, self.np_total,
                            self.vmax, boxsize=box)
        return self.finish()

    @classmethod
    def lightcone(cls, npix, opening_angle_deg, chi_edges, omega_m, mean_density, np_total, vmax, window="cic",
                  dtype=torch.float32):
        """Empty planes of a light cone: a gnomonic map of ``opening_angle_deg`` a side, shells between ``chi_edges``
        (P + 1 ascending comoving radii).  ``np_total``: a bound on all particles that will be added; ``vmax``: a bound
        on their masses (heavier ones are refused and counted); ``mean_density``: mass per (Mpc/h)^3."""
        return cls("cone", npix, chi_edges, omega_m, mean_density, np_total, vmax, window, dtype,
                   opening_angle_deg=opening_angle_deg)

    def add(self, pos, mass, observer, offset=(0.0, 0.0, 0.0), los=2):
        """Add particles - a box replica, a file chunk - as seen from ``observer`` looking along +``los``, the positions
        displaced by ``offset`` (a replica's shift): d = pos + offset - observer.  Returns self."""
        if self.geometry != "cone":
            raise ValueError("add() belongs to a light cone; a box is complete after from_box")
        origin = tuple(float(o) - float(s) for o, s in zip(observer, offset))
        pp.plane_paint_sums(pos, mass, "cone", self.nplanes, self.npix, self.window, los, self.sums, self.counters,
                            self.np_total, self.vmax, opening_angle_deg=self.opening_angle_deg, chi_edges=self.chi_edges,
                            e2=self._e2, origin=origin)
        self.planes = None
        return self

    def finish(self):
        """sums -> ``planes`` (every element written; may be called again after further ``add`` calls).  Returns self."""
        self.planes = pp.plane_paint_finish(self.sums, self.mul, self.add_term, self.geometry, self._args["c1"], self.dtype,
                                            out=self.planes)
        return self

    def source_weights(self, z_src):
        """``(wnum, wden)`` of one source redshift for ``lensing.kappa_stack`` (:func:`born_weights`)."""
        return born_weights(self.chi, self.a, flat_lcdm_comoving(float(z_src), self.omega_m), self.omega_m)

    def convergence(self, z_src):
        """Born convergence for the source redshift(s) ``z_src``: ``(npix, npix)`` for a scalar, ``(S, npix, npix)`` for a
        sequence, on the device in the planes' dtype; one ``lensing.kappa_stack`` per source over the resident planes."""
        if self.planes is None:
            raise ValueError("the planes are not finished: call finish() after the last add()")
        if np.ndim(z_src) == 0:
            return lensing.kappa_stack(self.planes, *self.source_weights(z_src))
        zs = [float(z) for z in z_src]
        out = torch.empty((len(zs), self.npix, self.npix), dtype=self.dtype, device=self.planes.device)
        for s, z in enumerate(zs):
            lensing.kappa_stack(self.planes, *self.source_weights(z), out=out[s])
        return out

    def ray_trace(self, z_src, born=False, pad=None, opening_angle=None):
        """Multi-plane ray tracing through the resident planes (``ray_trace.trace``): a dict of float64
        device tensors "kappa", "gamma1", "gamma2", "omega", "alpha1", "alpha2" (deflection in radians, component 1
        along array axis 0; the lens equation is beta = theta - alpha), ``(npix, npix)`` for a scalar ``z_src`` and
        ``(S, npix, npix)`` for a sequence, in the caller's order.  Plane k deflects with the potential of
        ``sigma_k = chi_k 3/2 Omega_m D_H^-2 D_k / a_k`` minus its mean, solved on a periodic grid of ``pad`` times npix
        a side with the map in one corner: ``pad`` 1 for a box (it is periodic), 2 for a cone by default.  Pixels are
        ``opening_angle`` / npix apart (degrees: the cone's own by default; a box has none, the caller gives it).
        ``born``: deflections and distortions are sampled along the undeflected rays and do not couple.  A source at or
        in front of the first plane gets zeros."""
        if self.planes is None:
            raise ValueError("the planes are not finished: call finish() after the last add()")
        if pad is None:
            pad = 1 if self.geometry == "box" else 2
        pad = rt.check_pad(pad)
        if opening_angle is None:
            if self.geometry != "cone":
                raise ValueError("a box has no opening angle: pass opening_angle (degrees)")
            opening_angle = self.opening_angle_deg
        angle = float(opening_angle)
        if not (math.isfinite(angle) and angle > 0.0):
            raise ValueError(f"opening_angle must be positive and finite (degrees), got {opening_angle!r}")
        scalar = np.ndim(z_src) == 0
        chi_src = [flat_lcdm_comoving(float(z), self.omega_m) for z in ([z_src] if scalar else z_src)]
        weights = 1.5 * self.omega_m * (1.0 / D_HUBBLE) ** 2 / self.a
        maps = rt.trace(self.planes, self.chi, weights, math.radians(angle) / self.npix, chi_src, born=born, pad=pad)
        return {name: maps[q, 0] if scalar else maps[q] for q, name in enumerate(rt.QUANTITIES)}

    def sky_array(self, z_src, opening_angle=None):
        """The convergence map of ONE source redshift as a ``SkyArray`` of quantity "kappa_2"; the map stays on the
        device in its ``MapStore``.  ``opening_angle`` in degrees: the cone's own by default; a box has none, the caller
        gives it."""
        from .skys.sky_array import SkyArray
        if opening_angle is None:
            if self.geometry != "cone":
                raise ValueError("a box has no opening angle: pass opening_angle (degrees)")
            opening_angle = self.opening_angle_deg
        if np.ndim(z_src) != 0:
            raise ValueError(f"sky_array takes one source redshift, got {z_src!r}")
        return SkyArray.from_array(self.convergence(z_src), float(opening_angle), "kappa_2", None)


def born_weights(chi, a, chi_s, omega_m):
    """``(wnum, wden)`` with W_p = wnum_p / wden_p = 3/2 Omega_m D_H^-2 g(chi_p, chi_s) / a_p, the Born weight of the
    contrast integrated through plane p (Mpc/h) for a source at comoving distance ``chi_s``: wnum_p = 3/2 Omega_m
    D_H^-2 g, 0 where chi_p >= chi_s; wden_p = a_p."""
    chi = np.asarray(chi, dtype=np.float64)
    pref = 1.5 * float(omega_m) * (1.0 / D_HUBBLE) ** 2
    g = np.where(chi < chi_s, lensing.kernel_function(chi, chi_s), 0.0) if chi_s > 0 else np.zeros_like(chi)
    return pref * g, np.array(a, dtype=np.float64)


def plane_factors(geometry, npix, chi_edges, mean_density, np_total, vmax, boxsize=None, opening_angle_deg=None):
    """``(mul, add)``, P float64 each: ``D_p = sums mul_p (cos^-3) + add_p`` with the quantum q = vmax / 2^k.
    Box: ``mul = q / (rho (L / npix)^2)`` (the plane's thickness cancels), cone: ``mul = q dchi / Mbar``,
    ``Mbar = rho (2 tan(theta / 2) / npix)^2 (chi_hi^3 - chi_lo^3) / 3``; ``add = -dchi`` in both."""
    edges = np.asarray(chi_edges, dtype=np.float64)
    lo, hi = edges[:-1], edges[1:]
    dchi = hi - lo
    q = float(vmax) / 2.0 ** pp.plane_exponent(np_total)
    rho = float(mean_density)
    if geometry == "box":
        side = float(boxsize) / float(npix)
        mul = np.full(dchi.shape, q / (rho * (side * side)))
    else:
        side = 2.0 * math.tan(0.5 * math.radians(float(opening_angle_deg))) / float(npix)
        mbar = rho * (side * side) * ((hi * hi * hi - lo * lo * lo) / 3.0)
        mul = q * dchi / mbar
    return mul, -dchi
