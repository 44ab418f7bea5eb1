"""Friends-of-friends groups on the GPU (``ast_fof_*``, csrc/fof.hip): particles -> objects, so that
particles -> groups -> profiles runs without a catalogue file.  ``FOF`` has nbodykit's argument meaning, ``FoFGroups``
halotools'; neither library is used here, and the definitions below are this module's own, restated by
tests/fof_oracle.py.

* **Input**: ``pos`` (N, 3) float32 or float64, numpy array or device tensor, widened to fp64 on load; N < 2^31.
* **Box**: with ``boxsize = L`` periodic, every coordinate in [0, L] (checked from the device bounds, as the pair
  counters do); without, open, every coordinate finite.
* **Sphere linking**: per axis ``a = |x_i - x_j|``, periodic ``a = min(a, L - a)``; ``d^2 = (a_x^2 + a_y^2) + a_z^2``
  in fp64 in this operand order, no FMA; i and j are friends when ``d^2 <= b b`` (a pair at distance 0 is a pair of
  friends).
* **Cylinder linking** (``b_para`` given, line of sight ``los``): ``rp^2 = a_a a_a + a_b a_b`` over the two other axes
  a < b and ``pi = a_los``; friends when ``rp^2 <= b_perp b_perp and pi <= b_para``.
* **Groups** are the connected components of the friendship graph; ``first(g)`` is the smallest original index among
  the members of g.  Groups of at least ``nmin`` members are numbered 1 .. G by descending size, ties by ascending
  ``first``; every other particle has label 0.
* **links**: the number of unordered friend pairs.
* **members** / **offsets**: the indices of the labelled particles ordered by (label, index), and G + 1 offsets into
  them: ``pos[members]`` with ``segments = (offsets[:-1], length)`` is what ``device.sphere_profiles`` takes.
* **Features** per group: ``p_ref = pos[first]``, ``s_i = pos_i - p_ref``, periodic wrapped once per axis
  (``s > L/2 -> s - L``, else ``s < -L/2 -> s + L``); ``CM = p_ref + sum(w s) / sum(w)``, periodic wrapped once into
  [0, L); ``CMV = sum(w v) / sum(w)``; w = 1 without weights.  A group wider than L/2 still gets this value, which then
  means little: its members do not all lie within half a box of the reference particle, so the wrap no longer picks
  one image of the group.

``ASTRILD_FOF_CELLS=0`` forces one cell (all pairs) instead of the cell grid; ``AST_FOF_CELL_OBJECTS=k`` plans the grid
with one cell per k objects instead of 64.  Neither changes a result.
"""
import ctypes as ct
import os

import numpy as np
import torch

from ... import _lib
from ...device import as_device, check, ptr, real_code, stream, to_numpy


def _length(name, v):
    try:
        x = float("nan") if v is None or isinstance(v, (str, bytes)) else float(v)
    except (TypeError, ValueError):
        x = float("nan")
    if not (np.isfinite(x) and x > 0):
        raise ValueError(f"{name} must be a positive, finite real number, got {v!r}")
    return x


def _check_real(name, a, shape_rule, ok):
    """Shape and dtype of a numpy array or tensor argument (anything else goes through numpy first)."""
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
    shape = tuple(int(s) for s in a.shape)
    if not ok(shape):
        raise ValueError(f"{name} must be {shape_rule}, got {shape}")
    floats = (torch.float32, torch.float64) if isinstance(a, torch.Tensor) else (np.float32, np.float64)
    if a.dtype not in floats:
        raise ValueError(f"{name} must be float32 or float64, got {a.dtype}")
    return a


def check_fof_args(pos, linking_length, boxsize=None, nmin=1, b_para=None, los=2):
    """The argument checks of ``fof_groups``, on the host and before any GPU work: ``(pos, b_perp, b_para, box)`` with
    ``b_para`` None for the sphere and ``box`` 0.0 for open boundaries, or ValueError: ``pos`` not (N, 3) float32 /
    float64 or N >= 2^31; a linking length that is not positive and finite; a periodic sphere with b >= L / 3 or a
    periodic cylinder with max(b_perp, b_para) >= L / 3 (the pair counters' rule: below it the periodic grid has at
    least 3 cells per axis); ``nmin`` < 1; ``los`` outside {0, 1, 2}."""
    pos = _check_real("pos", pos, "(N, 3)", lambda s: len(s) == 2 and s[1] == 3)
    if pos.shape[0] >= 1 << 31:
        raise ValueError(f"{pos.shape[0]} particles: fewer than 2^31 are supported")
    b_perp = _length("linking_length", linking_length)
    b_par = None if b_para is None else _length("b_para", b_para)
    box = 0.0
    if boxsize is not None:
        box = _length("boxsize", boxsize)
        reach = b_perp if b_par is None else max(b_perp, b_par)
        if not reach < box / 3.0:
            raise ValueError(f"the linking length ({reach}) must be below boxsize / 3 ({box / 3.0})")
    if isinstance(nmin, bool) or not isinstance(nmin, (int, np.integer)) or nmin < 1:
        raise ValueError(f"nmin must be an integer >= 1, got {nmin!r}")
    if isinstance(los, bool) or not isinstance(los, (int, np.integer)) or los not in (0, 1, 2):
        raise ValueError(f"los must be 0, 1 or 2, got {los!r}")
    return pos, b_perp, b_par, box


def find_roots(p, box, b_perp, b_par=None, los=2):
    """The library stages of ``fof_groups`` for n >= 2 positions on the device (``ast_fof_prepare``, the check of the
    device bounds, ``ast_fof_link``, ``ast_fof_compress``): ``(root, size, links, passes)`` - root[i] the smallest index
    of i's group, size[r] the members of the group whose smallest index is r (0 elsewhere), both int32; the link count
    as a one-element int64 device tensor; the pointer-jumping passes taken."""
    lib = _lib.lib()
    n, dev = int(p.shape[0]), p.device
    single = os.environ.get("ASTRILD_FOF_CELLS", "1") == "0"
    st = stream()
    ws_bytes = lib.ast_fof_workspace_bytes(n)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    bounds = torch.empty(6, dtype=torch.float64, device=dev)
    check(lib.ast_fof_prepare(ptr(p), real_code(p), n, ptr(work), ws_bytes, ptr(bounds), st), "ast_fof_prepare")
    b = to_numpy(bounds)
    if box > 0.0 and not (np.all(b[:3] >= 0.0) and np.all(b[3:] <= box)):
        raise ValueError(f"positions must lie in [0, {box}]: min {b[:3].tolist()}, max {b[3:].tolist()}")
    if box == 0.0 and not np.all(np.isfinite(b)):
        raise ValueError(f"positions must be finite: min {b[:3].tolist()}, max {b[3:].tolist()}")
    links = torch.empty(1, dtype=torch.int64, device=dev)
    check(lib.ast_fof_link(ptr(work), ws_bytes, n, box, int(b_par is not None), b_perp, b_par or 0.0, int(los),
                           int(single), ptr(links), st), "ast_fof_link")
    pending = torch.empty(lib.ast_fof_max_passes(n), dtype=torch.int32, device=dev)
    root = torch.empty(n, dtype=torch.int32, device=dev)
    size = torch.empty(n, dtype=torch.int32, device=dev)        # counts below 2^31, read as int32
    passes = ct.c_int(0)
    check(lib.ast_fof_compress(ptr(work), ws_bytes, n, ptr(pending), ct.byref(passes), ptr(root), ptr(size), st),
          "ast_fof_compress")
    return root, size, links, passes.value


def number_groups(root, size, nmin):
    """The numbering of ``fof_groups`` from ``find_roots``' result: ``labels``, ``length``, ``first``, ``members``,
    ``offsets``.  Groups of >= nmin members by (-size, first), members by (label, index): torch indexing and stable
    sorts on the caller's stream (plumbing, as in ``device.watershed_basins``) around ``ast_fof_relabel``."""
    n, dev = int(root.numel()), root.device
    roots = torch.nonzero(size >= nmin).reshape(-1)             # ascending: a root is its group's smallest index
    length, order = torch.sort(size[roots].to(torch.int64), descending=True, stable=True)
    first = roots[order]
    table = torch.zeros(n, dtype=torch.int32, device=dev)
    table[first] = torch.arange(1, first.numel() + 1, dtype=torch.int32, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    check(_lib.lib().ast_fof_relabel(ptr(root), ptr(table), n, ptr(labels), stream()), "ast_fof_relabel")
    idx = torch.nonzero(labels > 0).reshape(-1)                 # ascending index; a stable sort by label keeps it
    members = idx[torch.sort(labels[idx], stable=True)[1]].to(torch.int32)
    offsets = torch.zeros(first.numel() + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(length, 0)
    return {"labels": labels, "length": length, "first": first, "members": members, "offsets": offsets}


def fof_groups(pos, linking_length, boxsize=None, nmin=1, b_para=None, los=2, return_passes=False):
    """Friends-of-friends groups (module docstring for the definitions).  ``linking_length``: b of the sphere, or
    b_perp of the cylinder when ``b_para`` is given (line of sight ``los``).  Returns a dict of device tensors
    ``labels`` (N,) int32, ``length`` (G,) int64, ``first`` (G,) int64, ``members`` int32, ``offsets`` (G + 1,) int64,
    and ``links``, a Python int.  ``return_passes``: ``(dict, pointer-jumping passes taken)``.  ValueError before any
    GPU work by ``check_fof_args``, and from the device bounds for periodic positions outside [0, boxsize] or open
    positions that are not finite.  N < 2 returns without a call into the library."""
    pos, b_perp, b_par, box = check_fof_args(pos, linking_length, boxsize, nmin, b_para, los)
    _lib.lib()
    p = as_device(pos)
    n, dev = int(p.shape[0]), p.device
    if n < 2:
        g = 1 if n == 1 and nmin <= 1 else 0
        out = {"labels": torch.full((n,), g, dtype=torch.int32, device=dev),
               "length": torch.ones(g, dtype=torch.int64, device=dev),
               "first": torch.zeros(g, dtype=torch.int64, device=dev),
               "members": torch.zeros(g, dtype=torch.int32, device=dev),
               "offsets": torch.arange(g + 1, dtype=torch.int64, device=dev), "links": 0}
        return (out, 0) if return_passes else out
    root, size, links, passes = find_roots(p, box, b_perp, b_par, int(los))
    out = number_groups(root, size, int(nmin))
    out["links"] = int(links.item())
    return (out, passes) if return_passes else out


def check_fof_feature_args(pos, boxsize=None, vel=None, weights=None):
    """The argument checks of ``fof_features`` on the host: ``(pos, vel, weights, box)`` or ValueError for shapes,
    dtypes or a ``boxsize`` that is not positive and finite."""
    pos = _check_real("pos", pos, "(N, 3)", lambda s: len(s) == 2 and s[1] == 3)
    n = int(pos.shape[0])
    if vel is not None:
        vel = _check_real("vel", vel, f"(N, 3) = ({n}, 3) like pos", lambda s: s == (n, 3))
    if weights is not None:
        weights = _check_real("weights", weights, f"(N,) = ({n},)", lambda s: s == (n,))
    return pos, vel, weights, 0.0 if boxsize is None else _length("boxsize", boxsize)


def fof_features(pos, groups, boxsize=None, vel=None, weights=None):
    """Centre of mass, mean velocity and weight of every group of ``groups`` (a ``fof_groups`` result for the same
    ``pos``): a dict of fp64 device tensors ``cm_position`` (G, 3), ``cm_velocity`` (G, 3) when ``vel`` is given, and
    ``weight`` (G,), by the rule of the module docstring.  The order of the additions is fixed (ast_fof_features):
    two calls give the same bits.  ``boxsize`` should be the one the groups were found with."""
    pos, vel, weights, box = check_fof_feature_args(pos, boxsize, vel, weights)
    lib = _lib.lib()
    p = as_device(pos)
    v = None if vel is None else as_device(vel)
    w = None if weights is None else as_device(weights)
    n, g, dev = int(p.shape[0]), int(groups["first"].numel()), p.device
    if int(groups["labels"].numel()) != n:
        raise ValueError(f"groups were found for {int(groups['labels'].numel())} particles, pos has {n}")
    cm = torch.empty((g, 3), dtype=torch.float64, device=dev)
    cmv = None if v is None else torch.empty((g, 3), dtype=torch.float64, device=dev)
    weight = torch.empty(g, dtype=torch.float64, device=dev)
    if g:
        code = lambda t: real_code(t) if t is not None else _lib.F64
        members, offsets, first = (groups[k].contiguous() for k in ("members", "offsets", "first"))
        check(lib.ast_fof_features(ptr(p), code(p), ptr(v), code(v), ptr(w), code(w), n, ptr(members), ptr(offsets),
                                   ptr(first), g, box, ptr(cm), ptr(cmv), ptr(weight), stream()), "ast_fof_features")
    out = {"cm_position": cm, "weight": weight}
    if cmv is not None:
        out["cm_velocity"] = cmv
    return out


def mean_separation(boxsize, n):
    """(L^3 / N)^(1/3), the unit of relative linking lengths."""
    return (float(boxsize) ** 3 / float(max(int(n), 1))) ** (1.0 / 3.0)


class FOF:
    """nbodykit's ``FOF(source, linking_length, nmin, absolute=False, periodic=True)`` on positions: with
    ``absolute=False`` the linking length is in units of the mean separation (L^3 / N)^(1/3), which needs ``boxsize``
    (ValueError without); ``periodic=True`` needs it as well.  ``labels`` (numpy int32, 0 for particles in no group of
    ``nmin`` members) and ``max_label`` = G; ``links`` and the device tensors of ``fof_groups`` in ``groups``."""

    def __init__(self, pos, linking_length, nmin, absolute=False, periodic=True, boxsize=None):
        if boxsize is None and (periodic or not absolute):
            raise ValueError("boxsize is needed for periodic=True and for a relative linking length (absolute=False)")
        self.pos, self.boxsize, self.periodic = pos, boxsize, bool(periodic)
        b = _length("linking_length", linking_length)
        if not absolute:
            b *= mean_separation(_length("boxsize", boxsize), np.shape(pos)[0] if np.ndim(pos) else 0)
        self.linking_length = b
        self._box = boxsize if periodic else None
        self.groups = fof_groups(pos, b, boxsize=self._box, nmin=nmin)
        self.labels = to_numpy(self.groups["labels"])
        self.max_label = int(self.groups["first"].numel())
        self.links = self.groups["links"]

    def find_features(self, vel=None, weights=None):
        """``CMPosition`` (G, 3), ``CMVelocity`` (G, 3; None without ``vel``) and ``Length`` (G,) of groups 1 .. G
        (nbodykit's columns; it keeps a row for label 0, which is left out here), as numpy arrays."""
        f = fof_features(self.pos, self.groups, boxsize=self._box, vel=vel, weights=weights)
        return {"CMPosition": to_numpy(f["cm_position"]),
                "CMVelocity": to_numpy(f["cm_velocity"]) if vel is not None else None,
                "Length": to_numpy(self.groups["length"])}

    def segments(self):
        """``(members, segments)`` for ``device.sphere_profiles(pos[members], centres, radii, edges,
        segments=segments)``: the labelled particles ordered by (label, index) and, per group, its (offset, count)
        in them - numpy int32 (M,) and int64 (G, 2)."""
        offsets = to_numpy(self.groups["offsets"])
        return to_numpy(self.groups["members"]), np.stack([offsets[:-1], np.diff(offsets)], axis=1)


class FoFGroups:
    """halotools' ``FoFGroups(positions, b_perp, b_para, period=None, Lbox=None)``: cylinders along z, both lengths in
    units of the mean separation (L^3 / N)^(1/3) with L = ``period`` (periodic) or ``Lbox`` (open boundaries;
    ValueError when both are None or ``period`` is not one length for all axes).  Every object gets a group
    (nmin = 1): ``group_ids`` (numpy int32) are 1 .. ``n_groups``, by descending size and then by first member."""

    def __init__(self, positions, b_perp, b_para, period=None, Lbox=None):
        side = period if period is not None else Lbox
        if side is None:
            raise ValueError("period (a periodic box) or Lbox (open boundaries) is needed for the mean separation")
        side = np.unique(np.asarray(side, dtype=np.float64).reshape(-1))
        if len(side) != 1:
            raise ValueError(f"a cubic box is expected, got sides {side.tolist()}")
        L = _length("period" if period is not None else "Lbox", side[0])
        unit = mean_separation(L, np.shape(positions)[0] if np.ndim(positions) else 0)
        self.b_perp, self.b_para = _length("b_perp", b_perp) * unit, _length("b_para", b_para) * unit
        self.groups = fof_groups(positions, self.b_perp, boxsize=L if period is not None else None, nmin=1,
                                 b_para=self.b_para, los=2)
        self.group_ids = to_numpy(self.groups["labels"])
        self.n_groups = int(self.groups["first"].numel())
        self.links = self.groups["links"]
