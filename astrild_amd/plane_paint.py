"""Particles -> lens planes on the GPU (``ast_plane_paint_accumulate`` / ``ast_plane_paint_finish``, csrc/plane_paint.hip,
DESIGN.md 6n): P planes of npix x npix from a periodic box (plane-parallel) or a light cone (gnomonic map, radial shells),
NGP / CIC / TSC on the two transverse axes.  ``rays.LensPlanes`` is the interface in physical units; these are the
one-call-per-C-entry wrappers under it.

* ``sums``: ``(P, npix, npix)`` int64 on the device, indexed ``[plane, ia, ib]`` with (a, b) the two axes other than
  ``los`` in increasing order.  It is ADDED to: one allocation with ``torch.zeros`` (made here when none is given), then
  any number of calls for chunks and box replicas.  Every deposit is rounded once to a multiple of
  ``q = vmax / 2^k`` and added as an integer, so the sums hold the same bits for every particle order, chunking and
  launch geometry (tests/plane_paint_oracle.py restates them in numpy).
* ``counters``: 3 int64 on the device, added to: particles outside (non-finite, behind the observer, outside the
  shells, or with the whole stencil off the map), clipped (part of the stencil off the map: cone only), refused
  (``!(|mass * scale| <= vmax)``).  Reading them is the caller's synchronisation.
* Everything is queued on the caller's current stream.  With ``vmax`` given and edges on the device no call waits for
  the device; the default ``vmax`` costs one 16-byte fetch (``device._mass_bound``, which raises on a NaN or Inf mass).
"""
import ctypes as ct
import math

import numpy as np
import torch

from . import _lib, device as dev
from ._lib import check
from .device import as_device, dense, ptr, real_code, stream

_FLOATS = ("float32", "float64")
NP_TOTAL_MAX = (1 << 60) - 1


def _dtype_name(dt):
    if isinstance(dt, torch.dtype):
        return str(dt).replace("torch.", "")
    try:
        return np.dtype(dt).name
    except TypeError:
        return repr(dt)


def _real(value, name, positive=False):
    try:
        v = float("nan") if isinstance(value, (str, bytes, bool)) or value is None else float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if not math.isfinite(v) or (positive and not v > 0.0):
        raise ValueError(f"{name} must be a {'positive, ' if positive else ''}finite real number, got {value!r}")
    return v


def _count(value, name, least=1):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < least:
        raise ValueError(f"{name} must be an integer >= {least}, got {value!r}")
    return int(value)


def plane_exponent(np_total):
    """k = min(50, 62 - bit_length(np_total)): with every |term| <= vmax, np_total (2^k + 1) < 2^63."""
    return min(50, 62 - int(np_total).bit_length())


def check_plane_paint_args(geometry, pos_shape, pos_dtype, mass_shape, nplanes, npix, window="cic", los=2, np_total=None,
                           vmax=1.0, scale=1.0, shift=-0.5, boxsize=None, opening_angle_deg=None, chi_edges=None,
                           origin=(0.0, 0.0, 0.0)):
    """The argument checks of ``plane_paint_sums``, on the host and before any GPU work.  Returns a dict with the values
    the C entry takes - ``geometry``, ``window`` (codes), ``npart``, ``np_total``, ``los``, ``nplanes``, ``npix``, ``cl``,
    ``c1``, ``c0``, ``origin`` (3 floats), ``e2`` (float64 array of the squared edges, cone only), ``scale``, ``vmax``,
    ``k`` - or raises ValueError / TypeError naming the offending value: a geometry other than "box" / "cone"; ``pos``
    that is not (N, 3); a mass that is not (N,); a dtype that is not float32 or float64 (TypeError); ``nplanes`` or
    ``npix`` below 1, or planes beyond what one allocation addresses; a ``window`` that is no key of ``_lib.WIN``; ``los``
    outside 0 .. 2; ``np_total`` below N or above 2^60 - 1; ``vmax`` not positive and finite; ``scale`` or ``shift`` not
    finite; box: ``boxsize`` not positive and finite; cone: ``opening_angle_deg`` outside (0, 180), ``chi_edges`` that
    are not nplanes + 1 finite, non-negative, strictly ascending numbers, an ``origin`` that is not 3 finite numbers."""
    if not isinstance(geometry, str) or geometry.lower() not in _lib.PLANE_GEOMETRY:
        raise ValueError(f"geometry must be one of {sorted(_lib.PLANE_GEOMETRY)}, got {geometry!r}")
    geometry = geometry.lower()
    ps = tuple(int(s) for s in pos_shape)
    if len(ps) != 2 or ps[1] != 3:
        raise ValueError(f"pos must be (N, 3), got shape {ps}")
    if mass_shape is not None and tuple(int(s) for s in mass_shape) != (ps[0],):
        raise ValueError(f"mass must be ({ps[0]},) like pos, got shape {tuple(int(s) for s in mass_shape)}")
    if _dtype_name(pos_dtype) not in _FLOATS:
        raise TypeError(f"pos must be float32 or float64, got {_dtype_name(pos_dtype)}")
    P, n = _count(nplanes, "nplanes"), _count(npix, "npix")
    if n > 1 << 30 or P * n * n > (1 << 60):
        raise ValueError(f"{P} planes of {n} x {n} pixels are more than one allocation addresses")
    if not isinstance(window, str) or window.lower() not in _lib.WIN:
        raise ValueError(f"window must be one of {sorted(_lib.WIN)}, got {window!r}")
    if isinstance(los, bool) or not isinstance(los, (int, np.integer)) or not 0 <= int(los) <= 2:
        raise ValueError(f"los must be 0, 1 or 2, got {los!r}")
    total = ps[0] if np_total is None else _count(np_total, "np_total", 0)
    if total < ps[0] or total > NP_TOTAL_MAX:
        raise ValueError(f"np_total must be the declared bound on all particles added to these sums: at least the {ps[0]} "
                         f"of this call and at most 2^60 - 1, got {np_total!r}")
    out = dict(geometry=_lib.PLANE_GEOMETRY[geometry], window=_lib.WIN[window.lower()], npart=ps[0], np_total=total,
               los=int(los), nplanes=P, npix=n, vmax=_real(vmax, "vmax", positive=True), scale=_real(scale, "scale"),
               k=plane_exponent(total), e2=None, origin=(0.0, 0.0, 0.0), cl=0.0)
    sh = _real(shift, "shift")
    if geometry == "box":
        box = _real(boxsize, "boxsize", positive=True)
        out.update(cl=float(P) / box, c1=float(n) / box, c0=sh)
    else:
        angle = _real(opening_angle_deg, "opening_angle_deg", positive=True)
        if not angle < 180.0:
            raise ValueError(f"opening_angle_deg must lie in (0, 180): a tangent-plane map, got {opening_angle_deg!r}")
        try:
            edges = np.array(chi_edges, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"chi_edges must be {P + 1} numbers, got {chi_edges!r}") from None
        if chi_edges is None or edges.size != P + 1 or not np.isfinite(edges).all() or edges[0] < 0 or not (np.diff(edges) > 0).all():
            raise ValueError(f"chi_edges must be nplanes + 1 = {P + 1} finite, non-negative, strictly ascending numbers, "
                             f"got {chi_edges!r}")
        try:
            o = tuple(float(v) for v in origin)
        except (TypeError, ValueError):
            o = ()
        if len(o) != 3 or not all(math.isfinite(v) for v in o):
            raise ValueError(f"origin must be 3 finite numbers, got {origin!r}")
        out.update(c1=float(n) / (2.0 * math.tan(0.5 * math.radians(angle))), c0=0.5 * float(n) + sh, e2=edges * edges,
                   origin=o)
    return out


def upload_doubles(*arrays):
    """Host float64 arrays -> device tensors, views into ONE allocation filled by one non-blocking copy from pinned
    memory (a pageable host-to-device copy would block the host behind everything queued on the stream)."""
    arrays = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in arrays]
    sizes = [a.size for a in arrays]
    host = torch.empty(sum(sizes), dtype=torch.float64, pin_memory=True)
    at = 0
    for a, size in zip(arrays, sizes):
        host[at:at + size] = torch.from_numpy(a)
        at += size
    table = host.to(dev.device(), non_blocking=True)
    return list(torch.split(table, sizes))


def plane_paint_sums(pos, mass, geometry, nplanes, npix, window="cic", los=2, sums=None, counters=None, np_total=None,
                     vmax=None, scale=1.0, shift=-0.5, boxsize=None, opening_angle_deg=None, chi_edges=None, e2=None,
                     origin=(0.0, 0.0, 0.0)):
    """Add the deposits of ``pos`` (N, 3), ``mass`` (N,) or None - device tensors or numpy arrays, float32 or float64, in
    any layout - to ``sums`` (module docstring); returns ``(sums, counters)``, both on the device.  ``geometry`` "box":
    ``boxsize``; "cone": ``opening_angle_deg``, ``chi_edges`` (nplanes + 1 comoving radii) and ``origin`` (observer
    minus replication offset); ``e2``: the squared edges on the device already (float64, what
    ``check_plane_paint_args`` returns, uploaded by the caller), so that repeated calls upload nothing.
    ``shift``: added to the pixel coordinate; -0.5 puts pixel centres at i + 1/2.  ``np_total``: the declared bound on all
    particles ever added to these sums (default: this call's N) - it fixes the quantum and must be the same for every
    call on the same sums.  ``vmax``: the bound on ``|mass * scale|`` (default ``max |mass| * |scale|``, one reduction
    and a 16-byte fetch; ValueError on a NaN or Inf mass); particles above it are refused and counted."""
    pos = pos if isinstance(pos, torch.Tensor) else np.asarray(pos)
    if mass is not None and not isinstance(mass, torch.Tensor):
        mass = np.asarray(mass)
    a = check_plane_paint_args(geometry, pos.shape, pos.dtype, None if mass is None else mass.shape, nplanes, npix, window,
                               los, np_total, 1.0 if vmax is None else vmax, scale, shift, boxsize, opening_angle_deg,
                               chi_edges, origin)
    p = dense(as_device(pos))
    m = None if mass is None else dense(as_device(mass, dtype=p.dtype))
    P, n = a["nplanes"], a["npix"]
    if sums is None:
        sums = torch.zeros((P, n, n), dtype=torch.int64, device=p.device)
    if counters is None:
        counters = torch.zeros(3, dtype=torch.int64, device=p.device)
    assert sums.is_cuda and sums.is_contiguous() and sums.dtype == torch.int64 and tuple(sums.shape) == (P, n, n)
    assert counters.is_cuda and counters.is_contiguous() and counters.dtype == torch.int64 and counters.numel() == 3
    if not a["npart"]:
        return sums, counters
    if vmax is None:
        a["vmax"] = dev._mass_bound(m, a["npart"]) * (abs(a["scale"]) or 1.0)
    if a["e2"] is not None and e2 is None:
        e2, = upload_doubles(a["e2"])
    e2 = dense(e2)
    assert e2 is None or (e2.is_cuda and e2.dtype == torch.float64 and e2.numel() == P + 1)
    origin_c = (ct.c_double * 3)(*a["origin"])
    check(_lib.lib().ast_plane_paint_accumulate(a["geometry"], a["window"], real_code(p), ptr(p), ptr(m), a["npart"],
                                                a["np_total"], a["los"], P, n, a["cl"], a["c1"], a["c0"], origin_c, ptr(e2),
                                                a["scale"], a["vmax"], ptr(sums), ptr(counters), stream()),
          "ast_plane_paint_accumulate")
    return sums, counters


def plane_paint_finish(sums, mul, add, geometry="box", c1=0.0, dtype=torch.float32, out=None):
    """``out[p] = dtype(sums[p] * mul[p] + add[p])`` in float64 with one rounding per operation, in the cone times the
    cos^-3 of the pixel centre between the two (``c1``: pixels per unit tangent, as ``check_plane_paint_args`` returns
    it).  ``mul``, ``add``: P numbers each (host), or float64 device tensors.  Every element of ``out`` - ``(P, npix,
    npix)`` of ``dtype``, allocated here when not given - is written."""
    if not isinstance(geometry, str) or geometry.lower() not in _lib.PLANE_GEOMETRY:
        raise ValueError(f"geometry must be one of {sorted(_lib.PLANE_GEOMETRY)}, got {geometry!r}")
    assert sums.is_cuda and sums.is_contiguous() and sums.dtype == torch.int64 and sums.dim() == 3 and sums.shape[1] == sums.shape[2]
    P, n = int(sums.shape[0]), int(sums.shape[1])
    if not (isinstance(mul, torch.Tensor) and isinstance(add, torch.Tensor)):
        mul, add = upload_doubles(mul, add)
    for t in (mul, add):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float64 and t.numel() == P
    if out is None:
        out = torch.empty((P, n, n), dtype=dtype, device=sums.device)
    assert out.is_cuda and out.is_contiguous() and tuple(out.shape) == (P, n, n)
    check(_lib.lib().ast_plane_paint_finish(_lib.PLANE_GEOMETRY[geometry.lower()], real_code(out), ptr(sums), ptr(mul),
                                            ptr(add), P, n, float(c1), ptr(out), stream()), "ast_plane_paint_finish")
    return out
