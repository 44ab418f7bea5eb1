"""Cell-by-cell accuracy of the mass-assignment paint: an exact reference, the quantum of the fixed-point column walk, two
derived error bounds per cell and a numpy emulator of the walk.  GPU-free (numpy only); a helper module: no test functions.
tests/test_paint_accuracy_cpu.py checks the emulator and its mutants against the bounds, tests/test_gpu_paint_accuracy.py
and tests/test_gpu_paint_paths.py the kernels.  Line numbers: astrild_amd/csrc/mesh_paint_tiled.hip unless another file
is named.

Reference (:class:`Reference`; :class:`OracleReference`: the same from float64 bincount sweeps, for millions of particles)
    ``oracle.mesh.window_1d`` in float64 gives the cells and the (renormalised) weights (``shift`` = 0: the kernels form
    ``x * n / L + shift`` in one fma, the oracle in two roundings, and the bounds below do not cover that difference); the terms
    ``m * scale * wx * wy * wz`` and the per-cell sums are formed in ``np.longdouble``:
    S = sum of terms, A = sum of |terms|, K = number of terms, D = sum of |m scale| (wy wz + wx wz + wx wy) (what an
    absolute error of one weight is multiplied by), Q = sum over the terms of HALF the quantum of the term's own
    tile column (:func:`column_quanta`).  The reference's own error, (K + 8) * ulp_longdouble / 2 * A, is part of every bound.

Quantum (:func:`tile_capacity` 1933-1938, :func:`quantum` = paint_inv_quantum 1245-1251, cmax 1345-1350)
    q = 1 / (2^min(50, SUM_BITS - bits) / vmax), vmax = mass_bound * |scale| (1.0 when that is 0), SUM_BITS 47 (fp32 grids) or
    62 (fp64), bits = 33 - clz(min(cmax, 2^30 - 1)); cmax = 5 * tile_capacity(np, ntiles) on the single-pass and scattered
    lists (one q for the whole grid), the largest tile count of the column on the two-pass lists (one q per column).  A
    particle belongs to the tile of its base cell (floor(s) CIC, floor(s + 0.5) TSC; buffer plane (base - x_start) mod n).
    A cell's deposits from a neighbouring column arrive through that column's halo record, quantised with THAT column's
    q: Q sums q / 2 term by term, and :func:`column_quanta` also returns the q of each cell's own column.

Column-walk bound (an overwrite paint that left nothing on the overflow / late list), per cell, ``base`` = |offset|:
    |g - (S - offset)| <= Q + u |S - offset| + c_d u64 (A + base) + c_h u (A + base) + (K + 8) u_ld A
  * Q: every term is rounded to its quantum once - the fma with 1.5 * 2^52 at line 1530 - then summed exactly in int64
    (1533; seams and the periodic z wrap add exact integers, 1683 and 1717); for Q = K q / 2 with one q.
  * u |S - offset|: the one rounding to the grid dtype T (1593 / 1595 / 1273 / 1276).
  * c_d, double roundings between the reference's term and the kernel's, each relative to the term (or to the cell):
      weights: the kernel's are not renormalised (paint_window.h 31-45), the oracle's are.  CIC: sigma = fl(fl(1 - f) + f) is
        within 2 u64 of 1 and the division rounds once: 3 per axis.  TSC: w1 may be one fma (contraction) instead of two
        roundings: 3; sigma is within 5 u64 of 1 (w0, w2 carry 3 roundings each and add up to <= 1/2, w1 >= 1/2 carries an
        absolute u64, two additions) and the division rounds once: 6 more; 9 per axis.                      3 * 3 | 3 * 9
      m * scale_invq (1508), scale * invq (1468), mwa (1524), mab (1527), q = 1 / invq (1352), sum * q (1593 / 1595):   6
      (double)(long long)raw above 2^53 (fp64 grids, 1595):                                                             1
      the subtraction of the offset in double (1593 / 1595), relative to |sum| + |offset|:                              1
      second-order terms ((1 + u64)^36 - 1 - 36 u64 < 1e-14 u64) and the double rounding before the cast to T:          1
    c_d = 18 (CIC), 36 (TSC).  (errors in vmax and invq themselves only move q, which :func:`quantum` forms the same way.)
  * c_h: column_fold_kernel (1787-1790) adds up to three neighbour halo lines, each rounded to T on its own (1593), in
    T: ``sum = h0 (+ h1) (+ h2); cell = cell + sum``.  With n_h lines the roundings that are not the last one are: the
    cell's own (<= u (A_own + base)), n_h line roundings (<= u A_halo in all) and n_h - 1 partial sums (<= u A_halo each):
    c_h = n_h = 0, 1 or 3, from the cell's place in its 8 x 8 tile footprint (:func:`halo_lines`): CIC x or y index
    0 mod 8, TSC 0 or 7 mod 8; both: 3.  A bound with c_h u A alone would miss that the cell's own rounding happens after the offset is
    subtracted, hence A + base.

Any-path bound (overflow list 1041-1076, late list 906-928 and 1134-1221, direct paint mesh_paint.hip 21-62, accumulating
tile flush 1134-1221): the bound above plus
    (2 K + c_a) u (A + base) + 3 u D
  * weights in T (paint_window.h: ``(R)frac``): an ABSOLUTE error of at most u per weight (CIC: the cast of f <= 1 and
    1 - f; TSC: d <= 1/2 cast, times the slope |dw/dd| <= 1), which is multiplied by m scale and the other two weights:
    3 axes -> u D.  Relative to a tiny deposit this is unbounded: a particle that touches a cell with weight 1e-9
    leaves an error of u * m there.  D is what the max-scaled tolerance of the older tests stood in for.  The factor 3:
    one u for the cast, up to 2 u relative roundings inside the weight formula that are bounded by the weight <= 1.
  * c_a = 13: relative roundings of one T term: 3 per axis inside the weight formulas (9), the cast of m * scale (1) and
    three products (3).
  * 2 K u (A + base): additions in T in arbitrary order, each rounding a partial sum of at most A + base (``base`` = the
    largest |prefilled value| for a paint that accumulates into ``out``).  The list kernels add term by term: K global
    atomics.  The tile kernel (1134-1221: accumulating paint, long late lists) adds a tile's terms in an LDS double
    (u64 <= u each), casts the tile's sum to T (1211) and adds it atomically (1218): with P <= K tile parts per cell, P
    casts, P atomics and K - P LDS additions, at most 2 K roundings.  A bound with (K + c_a) u A counts the
    list kernels only.

Total mass: |sum(g) - sum(S - offset)| <= sum of the per-cell bounds (the sum itself is taken in longdouble).
"""
import numpy as np

from oracle import mesh as omesh

TILE = (8, 8, 32)                              # paint_tile_geom.h
SUM_BITS = {np.float32: 47, np.float64: 62}
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
U64 = 2.0 ** -53
ULD = float(np.finfo(np.longdouble).eps) / 2
C_D = {"cic": 18, "tsc": 36}
C_A = 13
LD = np.longdouble


def tile_capacity(npart, ntiles):
    """Slots per tile of the single pass (1933-1938)."""
    mean = (npart + ntiles - 1) // ntiles
    cap = max(2 * mean, mean + 512)
    cap = (cap + 63) // 64 * 64
    return min(cap, 0x7fffffff)


def quantum_exponent(cmax, dtype):
    """k of ``invq = 2^k / vmax`` (1247-1250)."""
    c = min(int(cmax), 0x3fffffff)
    bits = 33 - (32 - c.bit_length())          # __clz of a 32-bit word
    return min(50, SUM_BITS[np.dtype(dtype).type] - bits)


def quantum(cmax, mass_bound, scale, dtype, coarser=0):
    """(q, scale_invq) in float64, formed as the kernel forms them (1249-1250, 1352, 1468).  ``coarser``: bits taken off
    the exponent (mutants only)."""
    vmax = float(mass_bound) * abs(float(scale))
    vmax = vmax if vmax > 0.0 else 1.0
    invq = 2.0 ** (quantum_exponent(cmax, dtype) - coarser) / vmax
    return 1.0 / invq, float(scale) * invq


def mass_bound_of(mass):
    """device._mass_bound: max |mass|, 1.0 for None or all zeros."""
    if mass is None or len(mass) == 0:
        return 1.0
    return float(np.abs(np.asarray(mass, dtype=np.float64)).max()) or 1.0


class Terms:
    """Every deposit of a paint, one entry per (particle, stencil point): ``cell`` (flat index into the (nx, n, n) buffer,
    -1 outside it), ``part`` (particle), the oracle's weights ``w`` (3, nterms) and kernel-style un-normalised weights
    ``wk``; per particle ``col`` (tile column tx * nty + ty of its base cell, buffer coordinates) and ``tile``."""

    def __init__(self, pos, nmesh, boxsize, window, shift=0.0, x_start=0, nx_alloc=None):
        pos = np.asarray(pos)
        n = self.n = int(nmesh)
        nx = self.nx = n if nx_alloc is None else int(nx_alloc)
        self.window, self.npart = window, pos.shape[0]
        sup = {"cic": 2, "tsc": 3}[window]
        s = pos.astype(np.float64) * (n / float(boxsize)) + shift
        i0, w, wk = [], [], []
        for d in range(3):
            a, b = omesh.window_1d(s[:, d], window)
            i0.append(a)
            w.append(b)
            if window == "cic":
                f = s[:, d] - np.floor(s[:, d])
                wk.append(np.stack([1.0 - f, f]))
            else:
                dd = s[:, d] - np.floor(s[:, d] + 0.5)
                hm, hp = 0.5 - dd, 0.5 + dd
                wk.append(np.stack([0.5 * (hm * hm), 0.75 - dd * dd, 0.5 * (hp * hp)]))
        lo = 0 if window == "cic" else 1
        base = [np.mod(i0[d] + lo, n) for d in range(3)]
        bx = np.mod(base[0] - int(x_start), n)                      # buffer plane of the base cell
        ntx, nty, ntz = (nx + TILE[0] - 1) // TILE[0], n // TILE[1], n // TILE[2]
        self.ntiles, self.ncols, self.ntz, self.nty, self.ntx = ntx * nty * ntz, ntx * nty, ntz, nty, ntx
        in_buf = bx < nx
        self.col = np.where(in_buf, (bx // TILE[0]) * nty + base[1] // TILE[1], -1)
        self.tile = np.where(in_buf, self.col * ntz + base[2] // TILE[2], -1)
        A, B, C = np.meshgrid(np.arange(sup), np.arange(sup), np.arange(sup), indexing="ij")
        A, B, C = A.ravel()[:, None], B.ravel()[:, None], C.ravel()[:, None]       # (sup^3, 1)
        px = np.mod(i0[0][None, :] + A - int(x_start), n)
        cell = (px * n + np.mod(i0[1][None, :] + B, n)) * n + np.mod(i0[2][None, :] + C, n)
        cell = np.where((px < nx) & in_buf[None, :], cell, -1)
        part = np.broadcast_to(np.arange(self.npart)[None, :], cell.shape)
        take = lambda ww: np.stack([ww[0][A[:, 0]], ww[1][B[:, 0]], ww[2][C[:, 0]]])       # (3, sup^3, npart)
        self.cell, self.part = cell.ravel(), part.ravel()
        self.w, self.wk = take(w).reshape(3, -1), take(wk).reshape(3, -1)
        self.centre = ((A == lo) & (B == lo) & (C == lo) & np.ones((1, self.npart), bool)).ravel()
        # the halo a term travels through: tile-column step from the particle's column to the cell's, (dx, dy) in -1 .. 1
        cpx, cy = self.cell // (n * n), (self.cell // n) % n
        ptx, pty = (self.col // nty)[self.part], (self.col % nty)[self.part]
        dx, dy = cpx // TILE[0] - ptx, cy // TILE[1] - pty
        dx = np.where(dx > 1, dx - ntx, np.where(dx < -1, dx + ntx, dx))           # (periodic buffers; a slab's steps are in range)
        dy = np.where(dy > 1, dy - nty, np.where(dy < -1, dy + nty, dy))
        self.route = np.where(self.cell >= 0, (dx + 1) * 3 + (dy + 1), -1)        # 4: the particle's own column
        self.inside = self.cell >= 0
        self._order = None

    @property
    def ncell(self):
        return self.nx * self.n * self.n

    def cell_sum(self, values, dtype=LD):
        """Per-cell sums of ``values`` (one per term) in ``dtype``: sorted by cell once, then one reduceat."""
        if self._order is None:
            order = np.argsort(np.where(self.inside, self.cell, self.ncell), kind="stable")
            order = order[: int(self.inside.sum())]
            sc = self.cell[order]
            starts = np.flatnonzero(np.r_[True, sc[1:] != sc[:-1]]) if len(sc) else np.zeros(0, np.int64)
            self._order, self._starts, self._cells = order, starts, sc[starts] if len(sc) else sc
        out = np.zeros(self.ncell, dtype=dtype)
        if len(self._order):
            out[self._cells] = np.add.reduceat(np.asarray(values, dtype=dtype)[self._order], self._starts)
        return out.reshape(self.nx, self.n, self.n)


def column_quanta(terms, mass, scale, dtype, lists, coarser=0):
    """Per tile column (q, scale_invq) as float64 arrays of length ncols.  ``lists``: "single" (single-pass and scattered
    lists: cmax = 5 * tile_capacity, 1349) or "two-pass" (cmax = the column's largest tile count, at least 1: 1345-1347)."""
    mb = mass_bound_of(mass)
    if lists == "single":
        cmax = np.full(terms.ncols, min(5 * tile_capacity(terms.npart, terms.ntiles), 0x3fffffff), dtype=np.int64)
    elif lists == "two-pass":
        counts = np.bincount(terms.tile[terms.tile >= 0], minlength=terms.ntiles).reshape(terms.ncols, terms.ntz)
        cmax = np.maximum(1, counts.max(axis=1))
    else:
        raise ValueError(lists)
    qs = np.array([quantum(c, mb, scale, dtype, coarser) for c in cmax])
    return qs[:, 0], qs[:, 1]


def cell_column(terms):
    """The tile column of every buffer cell, shape (nx, n, n)."""
    cx = (np.arange(terms.nx) // TILE[0])[:, None, None]
    cy = (np.arange(terms.n) // TILE[1])[None, :, None]
    return np.broadcast_to(cx * terms.nty + cy, (terms.nx, terms.n, terms.n))


def halo_lines(terms):
    """c_h per cell: how many neighbour halo lines column_fold_kernel adds into it (0, 1 or 3; a slab buffer's first and
    last tile rows have fewer: an upper bound there)."""
    edge = (lambda i: i % 8 == 0) if terms.window == "cic" else (lambda i: (i % 8 == 0) | (i % 8 == 7))
    ex, ey = edge(np.arange(terms.nx))[:, None, None], edge(np.arange(terms.n))[None, :, None]
    return np.broadcast_to(np.where(ex & ey, 3, np.where(ex | ey, 1, 0)), (terms.nx, terms.n, terms.n))


class Reference:
    """S, A, D (longdouble), K (int64) and, per list format, Q and the own-column q of every cell."""

    ref_unit = ULD                                # unit roundoff of the arithmetic that formed S, A and D

    def __init__(self, pos, mass, nmesh, boxsize, window, scale=1.0, shift=0.0, x_start=0, nx_alloc=None, keep_terms=False):
        self.terms = t = Terms(pos, nmesh, boxsize, window, shift, x_start, nx_alloc)
        self.mass, self.scale = mass, float(scale)
        m = np.ones(t.npart, dtype=LD) if mass is None else np.asarray(mass).astype(LD)
        ms = (m * LD(scale))[t.part]
        w = t.w.astype(LD)
        val = ms * w[0] * w[1] * w[2]
        self.S, self.A = t.cell_sum(val), t.cell_sum(np.abs(val))
        self.D = t.cell_sum(np.abs(ms) * (w[1] * w[2] + w[0] * w[2] + w[0] * w[1]))
        self.K = t.cell_sum(np.ones(len(val), dtype=np.int64), np.int64)
        self._q = {}
        self.window, self.halo_lines = window, np.array(halo_lines(t))
        for dtype in (np.float32, np.float64):
            for lists in ("single", "two-pass"):
                self.quanta(dtype, lists)
        if not keep_terms:
            self.terms = None                     # (a few hundred MB per input: the grids above are all a bound needs)

    def quanta(self, dtype, lists):
        """(Q, q of the cell's own column), float64 grids."""
        key = (np.dtype(dtype).type, lists)
        if key not in self._q:
            t = self.terms
            q, _ = column_quanta(t, self.mass, self.scale, dtype, lists)
            qt = q[np.maximum(t.col, 0)][t.part]
            self._q[key] = (t.cell_sum(0.5 * qt, np.float64), q[cell_column(t)])
        return self._q[key]

    def walk_bound(self, dtype, lists, offset=0.0):
        """The column-walk bound per cell (float64; Q stands for K q / 2 and A + |offset| for A where the offset enters before a rounding)."""
        u = U[np.dtype(dtype).type]
        Q, _ = self.quanta(dtype, lists)
        A, base = self.A.astype(np.float64), abs(float(offset))
        S = np.abs((self.S - LD(offset)).astype(np.float64))
        return Q + u * S + C_D[self.window] * U64 * (A + base) + self.halo_lines * u * (A + base) + (self.K + 8) * self.ref_unit * A

    def any_bound(self, dtype, lists=None, offset=0.0, base=None):
        """The any-path bound per cell.  ``lists`` None: no column walk at all (direct paint, accumulating paint): Q and the
        walk's roundings drop out, the one rounding of the result stays.  ``base``: the largest |prefilled value|."""
        u = U[np.dtype(dtype).type]
        A = self.A.astype(np.float64)
        base = abs(float(offset)) if base is None else float(base)
        atom = (2 * self.K + C_A) * u * (A + base) + 3 * u * self.D.astype(np.float64)
        if lists is None:
            return atom + u * np.abs((self.S - LD(offset)).astype(np.float64)) + (self.K + 8) * self.ref_unit * A
        return self.walk_bound(dtype, lists, offset) + atom


class OracleReference(Reference):
    """The same quantities for inputs of millions of particles, on the whole periodic grid: float64 bincount sweeps over
    the stencil, as ``oracle.mesh.paint`` (whose grid, times ``scale``, is ``S``), instead of term arrays in longdouble; the
    reference's own error is then (K + 8) u64 A.  ``share``: another instance for the same positions and window, whose
    mass-independent sums (K, the two-pass quanta in units of vmax) are reused."""
    ref_unit = U64

    def __init__(self, pos, mass, nmesh, boxsize, window, S, scale=1.0, share=None):
        n = self.n = int(nmesh)
        self.window, self.scale, self.mass, self.terms = window, float(scale), mass, None
        pos = np.asarray(pos, dtype=np.float64)
        npart = pos.shape[0]
        ax = [omesh.window_1d(pos[:, d] * (n / float(boxsize)), window) for d in range(3)]
        sup, lo = ax[0][1].shape[0], 0 if window == "cic" else 1
        idx = [[np.mod(ax[d][0] + a, n) for a in range(sup)] for d in range(3)]
        w = [ax[d][1] for d in range(3)]

        def sweep(per_particle, kind):
            out = np.zeros(n ** 3)
            for a in range(sup):
                for b in range(sup):
                    for c in range(sup):
                        flat = (idx[0][a] * n + idx[1][b]) * n + idx[2][c]
                        if kind == "count":
                            wt = per_particle
                        elif kind == "term":
                            wt = per_particle * w[0][a] * w[1][b] * w[2][c]
                        else:
                            wt = per_particle * (w[1][b] * w[2][c] + w[0][a] * w[2][c] + w[0][a] * w[1][b])
                        out += np.bincount(flat, weights=wt, minlength=n ** 3)
            return out.reshape(n, n, n)

        ms = np.full(npart, abs(float(scale))) if mass is None else np.abs(np.asarray(mass, dtype=np.float64) * float(scale))
        self.S = np.asarray(S, dtype=np.float64)
        positive = mass is None or (np.asarray(mass) >= 0).all()
        self.A = np.abs(self.S) if positive and scale > 0 else sweep(ms, "term")
        self.D = sweep(ms, "other-two")
        nty, ntz = n // TILE[1], n // TILE[2]
        self.halo_lines = np.where(*(lambda e: (e[:, None, None] & e[None, :, None], 3, np.where(e[:, None, None] | e[None, :, None], 1, 0)))(
            (np.arange(n) % 8 == 0) | ((np.arange(n) % 8 == 7) & (window == "tsc")))) * np.ones((1, 1, n), dtype=np.int64)
        if share is None:
            self.K = np.rint(sweep(np.ones(npart), "count")).astype(np.int64)
            col = (idx[0][lo] // TILE[0]) * nty + idx[1][lo] // TILE[1]
            counts = np.bincount(col * ntz + idx[2][lo] // TILE[2], minlength=(n // TILE[0]) * nty * ntz).reshape(-1, ntz)
            cmax = np.maximum(1, counts.max(axis=1))
            self._two = {}
            for T in (np.float32, np.float64):
                unit = np.array([2.0 ** -quantum_exponent(c, T) for c in cmax])          # q / vmax per column
                self._two[T] = (sweep(0.5 * unit[col], "count"), unit[cell_column(self)])
            self.ntiles, self.npart = counts.size, npart
        else:
            self.K, self._two, self.ntiles, self.npart = share.K, share._two, share.ntiles, share.npart

    nx = property(lambda self: self.n)
    nty = property(lambda self: self.n // TILE[1])

    def quanta(self, dtype, lists):
        T = np.dtype(dtype).type
        vmax = mass_bound_of(self.mass) * abs(self.scale)
        vmax = (vmax if vmax > 0.0 else 1.0) * (1.0 + 4 * U64)        # q = fl(1 / fl(2^k / vmax)) <= vmax 2^-k (1 + 2 u64 + ...)
        if lists == "single":
            unit = 2.0 ** -quantum_exponent(min(5 * tile_capacity(self.npart, self.ntiles), 0x3fffffff), T)
            return 0.5 * unit * vmax * self.K, np.full(self.S.shape, unit * vmax)
        Qk, qk = self._two[T]
        return Qk * vmax, qk * vmax


def measure(got, ref, bound, offset=0.0, add=None):
    """(largest error / bound, largest error / A, cells over the bound) of a painted grid ``got`` against ``ref.S - offset``
    (+ ``add``: what the grid held before an accumulating paint).  Cells with a zero bound must be exact."""
    want = ref.S - LD(offset)
    if add is not None:
        want = want + np.asarray(add).astype(LD)
    err = np.abs(np.asarray(got).astype(LD) - want).astype(np.float64)
    A = ref.A.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        rel = np.where(A > 0, err / A, 0.0)
    return float(ratio.max()), float(rel.max()), int((err > bound).sum())


def total_mass_error(got, ref, offset=0.0, add=None):
    """|sum(got) - sum(S - offset)| in longdouble."""
    want = (ref.S - LD(offset)).sum()
    if add is not None:
        want = want + np.asarray(add).astype(LD).sum()
    return float(abs(np.asarray(got).astype(LD).sum() - want))


def old_criterion(got, ref_S, dtype):
    """What tests/test_gpu_paint_paths.py::_check_grid held a grid to before the per-cell bounds: a tolerance scaled by the
    LARGEST cell of the grid."""
    ref = np.asarray(ref_S, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    if np.dtype(dtype).type is np.float64:
        return bool((np.abs(got - ref) <= 1e-11 * ref.max() + 1e-11 * np.abs(ref)).all())
    return bool((np.abs(got - ref) <= 3e-6 * ref.max()).all())


def emulate(pos, mass, nmesh, boxsize, window, dtype, lists="single", scale=1.0, offset=0.0, x_start=0, nx_alloc=None,
            terms=None, drop_term=None, truncate=False, coarser=0, fp32_particles=None):
    """The column walk + halo fold in numpy, float64 arithmetic as the kernel's: per term ``np.rint(m * scale_invq * wx * wy * wz)``
    (un-normalised weights, the products in the kernel's order), int64 sums per (cell, source column), ``T(sum * q - offset)``
    for the cell's own column (fp32 grids: through the biased 48-bit form of 1301-1304) and ``T(sum * q)`` per halo line, the
    lines added in T in column_fold_kernel's order.  Returns the (nx, n, n) grid in ``dtype``.
    Mutants: ``drop_term`` (index of a term that is left out), ``truncate`` (np.trunc for np.rint), ``coarser`` (bits taken
    off the quantum's exponent), ``fp32_particles`` (boolean per particle: weights and products formed in float32)."""
    T = np.dtype(dtype).type
    t = terms if terms is not None else Terms(pos, nmesh, boxsize, window, 0.0, x_start, nx_alloc)
    q, scale_invq = column_quanta(t, mass, scale, T, lists, coarser)
    pcol = np.maximum(t.col, 0)
    m = np.ones(t.npart) if mass is None else np.asarray(mass).astype(np.float64)
    md = m * scale_invq[pcol]                                                      # 1508 (unit masses: the constant itself)
    x = ((md[t.part] * t.wk[0]) * t.wk[1]) * t.wk[2]                              # 1524, 1527, and the exact product of 1530
    if fp32_particles is not None:
        sel = np.asarray(fp32_particles)[t.part]
        w32 = t.wk[:, sel].astype(np.float32)
        x32 = ((md[t.part][sel].astype(np.float32) * w32[0]) * w32[1]) * w32[2]
        x = x.copy()
        x[sel] = x32.astype(np.float64)
    v = (np.trunc(x) if truncate else np.rint(x)).astype(np.int64)
    keep = t.inside.copy()
    if drop_term is not None:
        keep[drop_term] = False
    v = np.where(keep, v, 0)
    qcell = None
    own = np.zeros(t.ncell, dtype=np.int64)
    halo = {}
    flat_col = cell_column(t).reshape(-1)
    for route in range(9):
        sel = keep & (t.route == route)
        if not sel.any():
            continue
        sums = np.zeros(t.ncell, dtype=np.int64)
        np.add.at(sums, t.cell[sel], v[sel])
        if route == 4:
            own = sums
        else:
            # the source column of this route, per cell: the cell's column minus the step
            dx, dy = route // 3 - 1, route % 3 - 1
            stx = np.mod(flat_col // t.nty - dx, t.ntx)
            sty = np.mod(flat_col % t.nty - dy, t.nty)
            halo[route] = (sums.astype(np.float64) * q[stx * t.nty + sty]).astype(T)           # the record line, rounded to T
    qcell = q[flat_col]
    if T is np.float32:
        low = (own + (1 << 47)) & ((1 << 48) - 1)                                  # the low 48 bits of BIAS + sum
        own_d = low.astype(np.float64) - float(1 << 47)
    else:
        own_d = own.astype(np.float64)
    grid = (own_d * qcell - float(offset)).astype(T)
    if halo:
        hsum = np.zeros(t.ncell, dtype=T)
        for route in sorted(halo, reverse=True):          # the fold's loops run over the NEIGHBOUR's step, minus the term's
            hsum = (hsum + halo[route]).astype(T)
        grid = (grid + hsum).astype(T)
    return grid.reshape(t.nx, t.n, t.n)


# ------------------------------------------------------------------ the inputs of tests/test_gpu_paint_accuracy.py
N, L, NP = 64, 250.0, 1 << 17
SCALE = (N / L) ** 3                           # 1 / dx^3
BLOB_TILE = (3, 4, 1)                          # the crowded inputs' blob sits at the centre of this tile (tx, ty, tz)
WIDE_EXP = {np.float32: 12, np.float64: 30}   # masses m0 * 2^e, integer e uniform in [-E, E]
M0 = 1.25


def sort_by_tile(pos, nmesh, boxsize, x_start=0):
    """Indices that put the particles in tile order (tile of the CIC base cell in buffer coordinates): order in memory, what
    the single pass's grouping kernel turns into group records."""
    s = np.asarray(pos, dtype=np.float64) * (nmesh / float(boxsize))
    c = np.mod(np.floor(s).astype(np.int64), nmesh)
    bx = np.mod(c[:, 0] - x_start, nmesh)
    key = ((bx // TILE[0]) * nmesh + c[:, 1] // TILE[1]) * nmesh + c[:, 2] // TILE[2]
    return np.argsort(key, kind="stable")


def _uniform(rng, count):
    """Uniform positions reaching past both box faces, as float32 values (one reference serves both dtypes), in tile order."""
    pos = rng.uniform(-0.3 * L, 1.3 * L, size=(count, 3)).astype(np.float32)
    return pos[sort_by_tile(pos, N, L)]


def _lattice(nz):
    """32 x 32 x nz particles, z fastest, off the cell faces."""
    g = lambda k: (np.arange(k) + 0.37) * (L / k)
    return np.stack(np.meshgrid(g(32), g(32), g(nz), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


def _crowded(rng, nz):
    lat = _lattice(nz)
    nblob = NP - len(lat)
    centre = (np.array(BLOB_TILE) + 0.5) * np.array(TILE) * (L / N)
    blob = (centre + 0.5 * (L / N) * rng.standard_normal((nblob, 3))).astype(np.float32)
    pos = np.concatenate([blob, lat])
    mass = np.concatenate([np.full(nblob, 2.0 ** 10), np.full(len(lat), 2.0 ** -10)]).astype(np.float32)
    return pos, mass


def make_input(name):
    """(positions, masses) of one named input, float32-representable values in float64 arrays (cast to the grid dtype by the
    caller, exactly).  ``wide-f32`` / ``wide-f64`` share their positions."""
    rng = np.random.default_rng(20261021)
    if name in ("wide-f32", "wide-f64"):
        pos = _uniform(rng, NP)
        E = WIDE_EXP[np.float32 if name == "wide-f32" else np.float64]
        mass = M0 * 2.0 ** np.random.default_rng(5).integers(-E, E + 1, size=NP)
    elif name == "crowded":                    # 60 % in one tile: blob 78848 particles of mass 2^10, lattice 32 x 32 x 51 of 2^-10
        pos, mass = _crowded(rng, 51)
    elif name == "crowded-late":               # 10 %: what the scatter path's late list still holds at either dtype
        pos, mass = _crowded(rng, 115)
    elif name == "signed":
        # planes 32 .. 40 are left to the coincident pairs +m, -m: cells there are touched by nothing else
        npair = 4096
        pos = _uniform(rng, NP - 2 * npair)
        x = pos[:, 0].astype(np.float64) % L
        pos[:, 0] = np.where((x >= 31.0 * L / N) & (x < 42.0 * L / N), x + 0.25 * L, pos[:, 0]).astype(np.float32)
        pair = rng.uniform(0.0, L, size=(npair, 3))
        pair[:, 0] = rng.uniform(33.5, 38.5, size=npair) * (L / N)
        pair = pair.astype(np.float32)
        m = rng.uniform(0.5, 2.0, size=len(pos)) * rng.choice([-1.0, 1.0], size=len(pos))
        pm = rng.uniform(0.5, 2.0, size=npair)
        pos = np.concatenate([pos, np.repeat(pair, 2, axis=0)])
        mass = np.concatenate([m, np.stack([pm, -pm], axis=1).ravel()])
        order = sort_by_tile(pos, N, L)
        pos, mass = pos[order], mass[order]
    elif name == "some-zero":
        pos = _uniform(rng, NP)
        mass = rng.uniform(0.5, 2.0, size=NP) * (rng.uniform(size=NP) >= 0.3)
    elif name == "all-zero":
        pos, mass = _uniform(rng, NP), np.zeros(NP)
    else:
        raise ValueError(name)
    return np.ascontiguousarray(pos, dtype=np.float64), np.asarray(mass, dtype=np.float32).astype(np.float64)


INPUTS = ("wide-f32", "wide-f64", "crowded", "crowded-late", "signed", "some-zero", "all-zero")


def pair_only_cells(pos, mass, window):
    """Cells of the ``signed`` input that only coincident pairs touch (with non-zero weight): exactly 0 on the column walk,
    where rint(x) + rint(-x) = 0 and the sums are integers."""
    p64 = np.asarray(pos, dtype=np.float64)
    _, first, counts = np.unique(p64, axis=0, return_index=True, return_counts=True)
    single = np.zeros(len(p64), bool)
    single[first[counts == 1]] = True
    touched = omesh.paint(p64, None, N, L, window) > 0
    return touched & (omesh.paint(p64[single], None, N, L, window) == 0)
