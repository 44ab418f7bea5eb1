"""Plane-wave and spike probes for the 3D power-spectrum paths.  Test infrastructure: host only at import (numpy and the
oracle); torch is imported inside the functions that build a grid on a device.

A probe is ``(m, A, phi)``: the field ``A cos(2 pi m.x / n + phi)`` with an integer wave vector m in the box convention
(every component in (-n/2, n/2]), stored with m_z >= 0 (cos is even: +-m are the same field).  Its whole power sits in the
two modes +-m, so the shell sums of a sum of probes are known in closed form (:func:`expected_psum`) and ONE mode that is
dropped, counted twice, weighted wrongly or binned one shell off changes a shell sum by a fraction of order one.

Which vectors (:func:`probe_set`, verified by :func:`check_categories` from the vectors alone):

1. Hermitian plane m_z = 0 (both +-m are stored, weight 1 each), m_x m_y of both signs.
2. m_z = 1, and m_z = n/2 - 1 or n/2 - 2 with |m| < n/2.
3. Negative frequencies -1 and -(n/2 - 1) (indices n - 1 and n/2 + 1) on axes 0 and 1.
4. The pruning boundary: |m|^2 = (n/2)^2 - 2 and (n/2)^2 - 3 ((n/2)^2 - 1 = 7 mod 8 is no sum of three squares for the
   sides in use), and the three self-conjugate Nyquist vectors of norm exactly n/2.
5. Tile seams: components t - 1, t, t + 1 for t = 16, 32, 64, and n/4.
6. The low-k patch boundary: all |m_i| <= 6 in shells 3, 4, 5, norm exactly 4, 5, 6 and 7; norm 16 and 17 (the boundary of
   the sixteen double-precision shells of the big fp32 passes).
7. On-edge vectors with three non-zero components, (2,3,6) j, (1,4,8) j, (4,4,7) j, (2,6,9) j, (6,6,7) j: every distinct
   permutation, two sign patterns, multipliers :func:`edge_multipliers`.

Crowding: a shell that holds no on-edge probe has at most CAP = 4 probes.  A shell with on-edge probes has to take whole
permutation families (six vectors of one norm; at side 32 the families of norm 9 and of norm 11 are nine vectors each),
so it may hold CAP_EDGE = 9; the amplitudes of one shell stay within 7 % of a common value instead, and EVERY probe of
every shell carries at least MIN_SHARE = 5 % of its shell's sum under the integer rule.
"""
import itertools
import math

import numpy as np

from oracle import fftpower as offt

CAP, CAP_EDGE, MIN_SHARE = 4, 9, 0.05
EDGE_BASES = ((2, 3, 6), (1, 4, 8), (4, 4, 7), (2, 6, 9), (6, 6, 7))
SEAM_TILES = (16, 32, 64)


# ---------------------------------------------------------------- lattice helpers
def _box(c, n):
    c %= n
    return c - n if c > n // 2 else c


def canonical(m, n):
    """The representative of +-m with components in (-n/2, n/2] and m_z >= 0 (m_z = 0: m_y >= 0, then m_x >= 0)."""
    a = tuple(_box(int(c), n) for c in m)
    b = tuple(_box(-int(c), n) for c in m)
    return max(a, b, key=lambda v: (v[2], v[1], v[0]))


def is_self_conjugate(m, n):
    return all((2 * int(c)) % n == 0 for c in m)


def norm2(m):
    return sum(int(c) * int(c) for c in m)


def integer_shell(m, n):
    """Shell of m under the integer rule, None when it is dropped (DC, |m| >= n/2)."""
    r = math.isqrt(norm2(m))
    return r - 1 if 1 <= r < n // 2 else None


def on_edge(m):
    m2 = norm2(m)
    return m2 > 0 and math.isqrt(m2) ** 2 == m2


def three_squares(v):
    """(a >= b >= c >= 0) with a^2 + b^2 + c^2 = v, preferring c > 0; None if there is none."""
    best = None
    for a in range(math.isqrt(v), 0, -1):
        for b in range(min(a, math.isqrt(v - a * a)), -1, -1):
            c2 = v - a * a - b * b
            c = math.isqrt(c2)
            if c * c == c2 and c <= b:
                if c > 0:
                    return a, b, c
                best = best or (a, b, c)
    return best


def edge_multipliers(n, base):
    """The j for which ``base * j`` is probed: every j with |base| j < n/2 when there are at most four, else 1, 2, 3, the
    first j with |base| j > n/4 and the largest one (a power-of-two j repeats the rounding pattern of j = 1 exactly;
    the others need not)."""
    r = math.isqrt(norm2(base))
    js = [j for j in range(1, n) if r * j < n // 2]
    if len(js) <= 4:
        return js
    return sorted({1, 2, 3, next(j for j in js if r * j > n // 4), js[-1]})


def _family(m):
    """(base, j, permutation pattern) if m is a multiple of a permutation of an EDGE_BASES vector, else None."""
    a = [abs(int(c)) for c in m]
    for base in EDGE_BASES:
        j, rem = divmod(max(a), max(base))
        if j >= 1 and rem == 0 and sorted(a) == [j * c for c in sorted(base)]:
            return base, j, tuple(c // j for c in a)
    return None


# ---------------------------------------------------------------- the probe set
class _Builder:
    def __init__(self, n):
        self.n, self.vecs, self.count, self.edge_shells = n, [], {}, set()

    def add(self, m):
        n = self.n
        m = canonical(m, n)
        if m in self.vecs:
            return True
        s = integer_shell(m, n)
        if s is None:
            if not (is_self_conjugate(m, n) and norm2(m) == (n // 2) ** 2):
                return False                              # outside the binned range and no Nyquist vector: nothing to probe
        else:
            if on_edge(m):
                self.edge_shells.add(s)
            if self.count.get(s, 0) >= (CAP_EDGE if s in self.edge_shells else CAP):
                return False
            self.count[s] = self.count.get(s, 0) + 1
        self.vecs.append(m)
        return True


def _vectors(n, seed):
    R = n // 2
    b = _Builder(n)
    signs = [(-1, 1), (1, -1), (1, 1), (-1, -1)]
    signs = signs[seed % 4:] + signs[:seed % 4]
    # --- on-edge vectors first: they decide which shells may be crowded
    for base in EDGE_BASES:                                                      # 7
        perms = sorted(set(itertools.permutations(base)))
        js = edge_multipliers(n, base)
        for i in range(max(len(perms), len(js))):
            p, j, (sx, sy) = perms[i % len(perms)], js[i % len(js)], signs[i % 2]
            b.add((sx * p[0] * j, sy * p[1] * j, p[2] * j))
        if base == EDGE_BASES[0]:                                                # second round: the other sign pattern, the next j
            for i, p in enumerate(perms):
                j, (sx, sy) = js[(i + 1) % len(js)], signs[(i + 1) % 2]
                b.add((sx * p[0] * j, sy * p[1] * j, p[2] * j))
    for m in [(6, 0, 0), (0, 6, 0), (0, 0, 6), (4, 4, 2), (2, 4, 4), (-4, 2, 4), (4, -4, 2),         # 6: norm 6
              (7, 0, 0), (2, 3, 6), (3, 6, 2), (6, 2, 3),                                             # norm 7
              (4, 0, 0), (3, 0, 4), (-4, 3, 0),                                                       # norm 4, 5
              (16, 0, 0), (0, 16, 0), (0, 0, 16),                                                     # norm 16 (side 32: the Nyquist vectors)
              (12, 12, 1), (8, 9, 12), (0, 8, 15), (-12, 1, 12), (9, -12, 8), (15, 0, 8)]:            # norm 17
        b.add(m)
    # --- the rest
    for m in [(5, 9, 0), (-7, 11, 0), (13, -4, 0), (-3, -8, 0)]:                 # 1 (canonical() turns (-3,-8,0) into (3,8,0))
        b.add(m)
    for m in [(2, -3, 1), (-4, 1, 1), (3, 2, R - 2), (-1, 2, R - 2)]:            # 2
        b.add(m)
    for m in [(-1, 2, 3), (4, -1, 2), (-(R - 1), 1, 2), (2, -(R - 1), 1)]:       # 3
        b.add(m)
    for v, axis in ((R * R - 2, 2), (R * R - 3, 0), (R * R - 1, 1)):             # 4
        t = three_squares(v)
        if t is not None:                         # the largest component on `axis`, one of the others negative
            m = [t[1], -t[2]]
            m.insert(axis, t[0])
            b.add(tuple(m))
    for m in [(R, 0, 0), (0, R, 0), (0, 0, R)]:
        b.add(m)
    for t in SEAM_TILES:                                                         # 5
        vals = [v for v in (t - 1, t, t + 1) if v < R]
        if len(vals) == 3 and norm2(vals) < R * R:
            for m in [(t - 1, -t, t + 1), (-(t + 1), t - 1, t), (t, t + 1, t - 1)]:
                b.add(m)
        else:
            for v in vals:
                if v < R - 1:                          # (v = R - 1 is there already: category 3)
                    for m in [(-v, 2, 1), (1, v, 2), (2, -1, v)]:
                        b.add(m)
    q = n // 4
    for m in [(q, 1, -2), (2, -q, 1), (-1, 2, q)]:
        b.add(m)
    for m in [(2, -3, 2), (4, 1, 1), (3, 4, 1), (-5, 1, 2), (3, -4, 4), (1, 5, 3)]:      # 6: shells 3, 4, 5 inside the box
        b.add(m)
    # --- fillers: every shell of a small side, at least 28 non-empty shells of a large one
    rng = np.random.default_rng([n, seed, 1])
    want = min(28, R - 1)
    for s in range(R - 1):
        if len(b.count) >= want or len(b.vecs) >= 92:
            break
        if s in b.count:
            continue
        for _ in range(200):
            u = rng.standard_normal(3)
            m = tuple(int(c) for c in np.rint(u / np.linalg.norm(u) * (s + 1.5)))
            if integer_shell(m, n) == s and not on_edge(m) and b.add(m):
                break
    return b.vecs


def probe_set(n, seed=0):
    """Deterministic list of ``(m, A, phi)`` for side n (module docstring); ``seed`` moves amplitudes, phases, the sign
    patterns and the fillers.  48 ... 96 probes, A in [0.5, 1.5]; the categories are asserted."""
    assert n % 2 == 0 and n >= 32
    vecs = _vectors(n, seed)
    rng = np.random.default_rng([n, seed])
    level = rng.uniform(0.6, 1.35, size=n // 2)               # one amplitude level per shell (last entry: the Nyquist vectors)
    probes = []
    for m in vecs:
        s = integer_shell(m, n)
        A = float(level[n // 2 - 1 if s is None else s] * rng.uniform(0.93, 1.07))
        # a self-conjugate mode holds (A cos phi)^2: keep cos phi away from zero
        phi = float(rng.uniform(-1.0, 1.0)) if is_self_conjugate(m, n) else float(rng.uniform(0.0, 2.0 * np.pi))
        probes.append((m, A, phi))
    check_categories(n, probes)
    return probes


def check_categories(n, probes):
    """Assert, from the vectors alone, that every category of the module docstring is present and the crowding rule holds."""
    R = n // 2
    ms = [tuple(m) for m, _, _ in probes]
    assert 48 <= len(probes) <= 96, len(probes)
    assert len(set(ms)) == len(ms) and all(canonical(m, n) == m for m in ms), "probes must be distinct canonical modes"
    assert all(0.5 <= A <= 1.5 for _, A, _ in probes)
    inside = [m for m in ms if integer_shell(m, n) is not None]
    # crowding
    share, edge_shells = {}, {integer_shell(m, n) for m in inside if on_edge(m)}
    for m, A, _ in probes:
        s = integer_shell(m, n)
        if s is not None:
            share.setdefault(s, []).append(A * A)
    for s, a2 in share.items():
        assert len(a2) <= (CAP_EDGE if s in edge_shells else CAP), (s, len(a2))
        assert min(a2) / sum(a2) >= MIN_SHARE, (s, min(a2) / sum(a2))
    # 1
    plane = [m for m in inside if m[2] == 0 and m[0] * m[1] != 0]
    assert any(m[0] * m[1] > 0 for m in plane) and any(m[0] * m[1] < 0 for m in plane), "category 1"
    # 2
    assert any(m[2] == 1 for m in inside) and any(m[2] in (R - 1, R - 2) for m in inside), "category 2"
    # 3 (m_z > 0: the sign of a component means something only then)
    for axis in (0, 1):
        for v in (-1, -(R - 1)):
            assert any(m[axis] == v and m[2] > 0 for m in inside), ("category 3", axis, v)
    # 4
    axes = set()
    for v in (R * R - 1, R * R - 2, R * R - 3):
        if three_squares(v) is not None:
            hit = [m for m in inside if norm2(m) == v]
            assert hit, ("category 4", v)
            axes.update(int(np.argmax(np.abs(m))) for m in hit)
    assert len(axes) >= 2, "category 4: spread over the axes"
    for m in [(R, 0, 0), (0, R, 0), (0, 0, R)]:
        assert m in ms, ("category 4: Nyquist", m)
    # 5
    seam_axes = set()
    for v in sorted({v for t in SEAM_TILES for v in (t - 1, t, t + 1) if v < R} | {n // 4}):
        hit = [m for m in inside if v in (abs(m[0]), abs(m[1]), abs(m[2]))]
        assert hit, ("category 5", v)
        seam_axes.update(ax for m in hit for ax in range(3) if abs(m[ax]) == v)
    assert seam_axes == {0, 1, 2}, "category 5: every axis"
    # 6
    for s in (3, 4, 5):
        assert any(integer_shell(m, n) == s and max(map(abs, m)) <= 6 and not on_edge(m) for m in inside), ("category 6", s)
    want = [(6, 0, 0), (4, 4, 2), (2, 4, 4), (2, 3, 6), (3, 6, 2), (6, 2, 3), (7, 0, 0)]
    want += [(12, 12, 1), (8, 9, 12), (0, 8, 15)] if R > 17 else []
    for w in want:
        assert any(tuple(map(abs, m)) == w for m in inside), ("category 6", w)
    assert sum(norm2(m) == 36 for m in inside) >= 5, "category 6: variants of norm 6"
    if R > 16:
        assert any(norm2(m) == 256 for m in inside), "category 6: norm 16"
    # 7
    fams = {}
    for m in inside:
        f = _family(m)
        if f is not None:
            fams.setdefault(f[0], []).append((f[1], f[2], m))
    far = False
    for base in EDGE_BASES:
        got = fams.get(base, [])
        assert {p for _, p, _ in got} == set(itertools.permutations(base)), ("category 7: permutations", base)
        assert {j for j, _, _ in got} == set(edge_multipliers(n, base)), ("category 7: multipliers", base)
        assert len({(m[0] > 0, m[1] > 0) for _, _, m in got if m[2] > 0}) >= 2, ("category 7: sign patterns", base)
        far = far or any(4 * norm2(m) > R * R for _, _, m in got)
    assert far, "category 7: |m| > n/4"


# ---------------------------------------------------------------- what the probes must give
def probe_shell(m, n, boxsize, binning):
    """Shell of the mode m under the rule ``binning`` (oracle.fftpower.shell_index on the m_z >= 0 representative), -1: dropped."""
    m = canonical(m, n)
    one = lambda c: np.array([c], dtype=np.int64)
    s = int(offt.shell_index(one(m[0]), one(m[1]), one(m[2]), np.array([[[norm2(m)]]], dtype=np.int64), n, boxsize,
                             binning).ravel()[0])
    return s if 0 <= s < n // 2 - 1 else -1


def expected_psum(n, boxsize, probes, binning):
    """Analytic shell sums of the probe field: L^3 A^2 / 2 per probe (both of +-m: weight 2 once or weight 1 twice),
    L^3 (A cos phi)^2 for a self-conjugate one (stored once, weight 1); nothing from a probe outside the shells."""
    out = np.zeros(n // 2 - 1)
    for m, A, phi in probes:
        s = probe_shell(m, n, boxsize, binning)
        if s >= 0:
            out[s] += float(boxsize) ** 3 * ((A * math.cos(phi)) ** 2 if is_self_conjugate(m, n) else 0.5 * A * A)
    return out


# ---------------------------------------------------------------- grids
def _slab_planes(n):
    return max(1, min(n, (1 << 25) // (n * n)))          # 2^25 cells: complex128 product + float64 real part + cast < 1.5 GB


def probe_field(n, probes, mean=0.0, dtype=np.float64, device="cpu"):
    """``mean + sum_p A_p cos(2 pi m_p.x / n + phi_p)`` on the (n, n, n) grid, worked out in float64 and cast once.
    The phases are exact: exp(2 pi i (m_i x_i mod n) / n) comes from ONE table of the n-th roots of unity, and a slab of x
    planes is the real part of one complex128 product  [(x, y), p] @ [p, z].  device "cpu": numpy array of numpy dtype;
    otherwise a torch tensor of the torch dtype on that device."""
    ms = np.array([m for m, _, _ in probes], dtype=np.int64)
    amp = np.array([A * np.exp(1j * phi) for _, A, phi in probes])
    roots = np.exp(2j * np.pi * np.arange(n) / n)
    idx = np.arange(n, dtype=np.int64)
    ex, ey, ez = (roots[(idx[:, None] * ms[None, :, a]) % n] for a in range(3))          # (n, P) each
    ex = ex * amp[None, :]
    step = _slab_planes(n)
    if device == "cpu":
        out = np.empty((n, n, n), dtype=dtype)
        for x0 in range(0, n, step):
            exy = (ex[x0:x0 + step, None, :] * ey[None, :, :]).reshape(-1, len(probes))
            out[x0:x0 + step] = ((exy @ ez.T).real + mean).reshape(-1, n, n)
        return out
    import torch
    tex, tey, tez = (torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (ex, ey, ez.T))
    out = torch.empty((n, n, n), dtype=dtype, device=device)
    for x0 in range(0, n, step):
        exy = (tex[x0:x0 + step, None, :] * tey[None, :, :]).reshape(-1, len(probes))
        out[x0:x0 + step] = ((exy @ tez).real + mean).reshape(-1, n, n)
    return out


def spike_field(n, cells, values, dtype=np.float64, device="cpu"):
    """Zero (n, n, n) grid with ``values[i]`` at ``cells[i]``."""
    if device == "cpu":
        out = np.zeros((n, n, n), dtype=dtype)
    else:
        import torch
        out = torch.zeros((n, n, n), dtype=dtype, device=device)
    for c, v in zip(cells, values):
        out[tuple(c)] = v
    return out
