"""Edge-case catalogues of the friends-of-friends group finder (astrild_amd/csrc/fof.hip, particles/hutils/fof.py), each
seeded and with its known answer or a call into tests/fof_oracle.py; numpy restatements, op by op in float64, of the
planners the finder uses (fof_plan_cap of fof.hip, grid_periodic_plan and grid_cyl_plan of cell_grid.h; the open sphere
plan is pair_geometry.plan with fof's cap); a numpy model of what the cell walk sees; hand-made parent forests for
ast_fof_compress.  A helper module: no test functions, no GPU, no torch.  tests/test_fof_cases_cpu.py shows that each
catalogue does what it claims; tests/test_gpu_fof_edges.py runs them on the GPU."""
import functools

import numpy as np

from tests import fof_oracle as orc
from tests import pair_geometry as pg

CELL_OBJECTS = 64                           # FOF_CELL_OBJECTS of fof.hip


def frozen(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------ the planners, restated
def plan_cap(n, per=CELL_OBJECTS):
    """fof_plan_cap of fof.hip: one cell per ``per`` objects (AST_FOF_CELL_OBJECTS; below 1 counts as 1), at least 27,
    at most the layout's grid_cells_cap(n, 27) = max(27, min(n, GRID_MAX_CELLS))."""
    layout = 27 if n < 27 else min(n, pg.MAX_CELLS)
    return min(max(n // max(int(per), 1), 27), layout)


def _cells(pos, lo, inv_cs, dims):
    """grid_box_cell: (cells (N, 3), cell_id (N,))."""
    v = (np.asarray(pos, dtype=np.float64) - lo) * inv_cs
    v = np.where(v >= 0.0, v, 0.0)
    v = np.minimum(v, (dims - 1).astype(np.float64))
    cells = v.astype(np.int64)
    return cells, (cells[:, 2] * dims[1] + cells[:, 1]) * dims[0] + cells[:, 0]


def plan_sphere(pos, b, boxsize=None, cap=None, single=False):
    """grid_plan as ast_fof_link calls it for the sphere.  Open: pair_geometry.plan (grid_box_plan) with ``cap``.
    Periodic: grid_periodic_plan - floor(L / (b (1 + 1e-6))) cells per axis, at most 1024, lowered while the cube
    exceeds ``cap``, one cell below 3.  ``cap`` None: plan_cap(n)."""
    pos = np.asarray(pos, dtype=np.float64)
    cap = plan_cap(len(pos)) if cap is None else cap
    if boxsize is None:
        return pg.plan(pos, b, single=single, cap=cap)
    box = np.float64(boxsize)
    d = 1
    m = np.floor(box / (np.float64(b) * (1.0 + 1e-6)))
    if not single and m >= 3.0:
        d = 1024 if m > 1024.0 else int(m)
        while d * d * d > cap:
            d -= 1
    dims = np.full(3, d, dtype=np.int64)
    inv_cs = np.full(3, float(d) / box if d > 1 else 0.0)
    cells, cell_id = _cells(pos, np.zeros(3), inv_cs, dims)
    return pg.Plan(lo=np.zeros(3), inv_cs=inv_cs, dims=dims, steps=0, cells=cells, cell_id=cell_id)


def plan_cyl(pos, b_perp, b_para, los, boxsize=None, cap=None, single=False, growth=1.25, margins=True):
    """grid_cyl_plan of cell_grid.h: the reach of axis c is b_para on ``los`` and b_perp elsewhere, times (1 + 1e-6).
    Periodic: floor(L / reach_c) cells on axis c, at most 1024, exactly 1 below 3.  Open: over the bounding box, with
    amax 1e-12 added to every reach, at least 1 cell and at most GRID_MAX_CELLS per axis.  While the grid exceeds
    ``cap`` every reach grows by 1.25.  ``growth`` and ``margins=False`` are the wrong planners of the sensitivity
    tests."""
    pos = np.asarray(pos, dtype=np.float64)
    cap = plan_cap(len(pos)) if cap is None else cap
    periodic = boxsize is not None
    reach = np.array([(b_para if a == los else b_perp) for a in range(3)], dtype=np.float64)
    if margins:
        reach = reach * (1.0 + 1e-6)
    if periodic:
        lo, ext = np.zeros(3), np.full(3, np.float64(boxsize))
    else:
        lo, hi = pos.min(axis=0), pos.max(axis=0)
        ext = hi - lo
        amax = np.float64(0.0)
        for a in range(3):
            amax = max(amax, max(abs(lo[a]), abs(hi[a])))
        if margins:
            reach = reach + amax * 1e-12
    dims = np.ones(3, dtype=np.int64)
    steps = 0
    if not single and (reach > 0.0).all():
        while True:
            prod = 1.0
            for a in range(3):
                m = np.floor(ext[a] / reach[a])
                if periodic:
                    m = (1024.0 if m > 1024.0 else m) if m >= 3.0 else 1.0
                else:
                    m = 1.0 if not m >= 1.0 else (float(pg.MAX_CELLS) if m > float(pg.MAX_CELLS) else m)
                dims[a] = int(m)
                prod *= m
            if prod <= float(cap):
                break
            reach = reach * growth
            steps += 1
    inv_cs = np.zeros(3)
    for a in range(3):
        inv_cs[a] = float(dims[a]) / ext[a] if dims[a] > 1 else 0.0
    cells, cell_id = _cells(pos, lo, inv_cs, dims)
    return pg.Plan(lo=lo, inv_cs=inv_cs, dims=dims, steps=steps, cells=cells, cell_id=cell_id)


def walk_pairs(plan, i, j, periodic, wrap=True):
    """Of the pairs (i, j), those the walk of cell_grid.h visits under ``plan``: the two cells differ by -1, 0 or +1 on
    every axis - periodic, on an axis of 3 or more cells, modulo its cells (an axis of one cell has offset 0 only).
    ``wrap=False`` is the wrong walk of the sensitivity test: no neighbour through a periodic face."""
    d = plan.cells[j] - plan.cells[i]
    ok = np.ones(len(i), dtype=bool)
    for a in range(3):
        n = int(plan.dims[a])
        if periodic and wrap and n >= 3:
            r = np.mod(d[:, a], n)
            ok &= (r == 0) | (r == 1) | (r == n - 1)
        else:
            ok &= np.abs(d[:, a]) <= 1
    return i[ok], j[ok]


def groups_from_pairs(n, i, j, nmin=1):
    out = orc.number_groups(orc.components(n, i, j), nmin)
    out["links"] = int(len(i))
    return out


def friend_pairs_strict_pi(pos, b_perp, b_para, los, boxsize=None):
    """The wrong cylinder of the sensitivity test: pi < b_para instead of pi <= b_para."""
    p = np.asarray(pos, dtype=np.float64)
    a = [np.abs(p[:, None, c] - p[None, :, c]) for c in range(3)]
    if boxsize is not None:
        a = [np.minimum(x, np.float64(boxsize) - x) for x in a]
    a_ax, b_ax = [c for c in range(3) if c != los]
    q = a[a_ax] * a[a_ax] + a[b_ax] * a[b_ax]
    ii, jj = np.nonzero((q <= np.float64(b_perp) * np.float64(b_perp)) & (a[los] < np.float64(b_para)))
    keep = ii < jj
    return ii[keep].astype(np.int64), jj[keep].astype(np.int64)


def known(root, links):
    """The result of fof_groups (nmin = 1) for a known root per particle and link count."""
    out = orc.number_groups(np.asarray(root, dtype=np.int64), 1)
    out["links"] = int(links)
    return out


def min_index_roots(group_of):
    """root[i] = the smallest index with i's value of ``group_of``."""
    group_of = np.asarray(group_of)
    _, inv = np.unique(group_of, return_inverse=True)
    smallest = np.full(inv.max() + 1, len(group_of), dtype=np.int64)
    np.minimum.at(smallest, inv, np.arange(len(group_of)))
    return smallest[inv]


# ------------------------------------------------------------------ 1. the slabbed lattice
LATTICE_B = 1.5


@functools.lru_cache(maxsize=None)
def lattice(m=24, slabbed=False, seed=31):
    """An integer lattice of m^3 points, spacing 1, for a periodic box of L = m and b = 1.5: the 18 neighbours at d^2 =
    1 and 2 are friends (the next, d^2 = 3, against b^2 = 2.25).  ``slabbed``: without the planes x = 0 and x = m / 2,
    which leaves two slabs.  Indices shuffled.  ``(pos, root, links)``: root[i] the smallest index of i's slab (or of
    all), links in closed form: m^2 points per plane; 4 of the 9 half-shell friend offsets stay in a plane x (kept
    planes: m or m - 2), 5 go from x to x + 1 (both kept: m or m - 4, the two gaps breaking two steps each)."""
    ijk = np.stack(np.meshgrid(*(np.arange(float(m)),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    if slabbed:
        ijk = ijk[(ijk[:, 0] != 0.0) & (ijk[:, 0] != float(m // 2))]
    pos = ijk[np.random.default_rng(seed).permutation(len(ijk))]
    root = min_index_roots(pos[:, 0] > m // 2) if slabbed else np.zeros(len(pos), dtype=np.int64)
    planes, steps = (m - 2, m - 4) if slabbed else (m, m)
    return frozen(pos), frozen(root), m * m * (4 * planes + 5 * steps)


# ------------------------------------------------------------------ 2. the serpentine
SERPENTINE_B = 0.05


@functools.lru_cache(maxsize=None)
def serpentine(cut=False, seed=32):
    """One path through hundreds of cells: 32 rows of 128 points 0.045 apart along x, the rows 0.5 apart in y, and
    between consecutive rows, at alternating ends, 11 connector points that divide the 0.5 evenly (0.0417 apart; at
    0.045 the last one would sit 0.005 from the next row and make a diagonal friend of that row's second point).
    4437 points in the plane z = 0, b = 0.05: every point is a friend of its path neighbours only, one group, 4436
    links.  ``cut``: without point 64 of row 16, two groups, 4434 links.  Indices shuffled.  ``(pos, path)``: path[i]
    the position of particle i along the path (for ``cut``, of the uncut path)."""
    pts = []
    for r in range(32):
        xs = np.arange(128) * 0.045
        if r % 2:
            xs = xs[::-1]
        pts += [(x, 0.5 * r, 0.0) for x in xs]
        if r < 31:
            pts += [(xs[-1], 0.5 * r + k * (0.5 / 12.0), 0.0) for k in range(1, 12)]
    pos, path = np.array(pts), np.arange(len(pts))
    if cut:
        keep = path != 16 * 139 + 64
        pos, path = pos[keep], path[keep]
    perm = np.random.default_rng(seed).permutation(len(pos))
    return frozen(pos[perm]), frozen(path[perm])


# ------------------------------------------------------------------ 3. hand-made forests for ast_fof_compress
def forest(kind, n, seed=33):
    """parent (n,) int32.  chain: parent[i] = i - 1, a path of n - 1 links; star: all under 0; heap: (i - 1) // 2;
    random: parent[i] uniform in [0, i]; identity; two_cycle: the identity with parent[1] = 2, parent[2] = 1 - not a
    forest, every entry inside [0, n)."""
    i = np.arange(n, dtype=np.int64)
    if kind == "chain":
        p = np.maximum(i - 1, 0)
    elif kind == "star":
        p = np.zeros(n, dtype=np.int64)
    elif kind == "heap":
        p = np.maximum((i - 1) // 2, 0)
    elif kind == "random":
        p = np.random.default_rng(seed).integers(0, i + 1)
    elif kind == "identity":
        p = i.copy()
    elif kind == "two_cycle":
        p = i.copy()
        p[1], p[2] = 2, 1
    else:
        raise ValueError(kind)
    return p.astype(np.int32)


def chase(parent):
    """root[i] by following parent to its fixed point, at most n steps (ValueError for a cycle), and the longest
    path's links."""
    parent = np.asarray(parent).astype(np.int64)
    r, depth = np.arange(len(parent), dtype=np.int64), 0
    while True:
        nxt = parent[r]
        if np.array_equal(nxt, r):
            return r, depth
        r, depth = nxt, depth + 1
        if depth > len(parent):
            raise ValueError("the parent array is not a forest")


def jump_passes(parent):
    """The passes ast_fof_compress takes when each is applied as a whole (no thread sees another's store of the same
    pass): p <- parent[parent[parent[p]]] unless parent[p] is a root, pending when the grandparent was not one."""
    parent = np.asarray(parent).astype(np.int64).copy()
    passes = 0
    while True:
        g0 = parent
        g1 = g0[g0]
        g2 = g0[g1]
        act = g1 != g0
        passes += 1
        parent = np.where(act, g2, g0)
        if not (act & (g2 != g1)).any():
            return passes


def max_passes(n):
    """ast_fof_max_passes: ceil(log2 n) + 1."""
    bits = 0
    while (1 << bits) < n:
        bits += 1
    return bits + 1


# ------------------------------------------------------------------ 4. open-boundary geometry
# A second linking length per catalogue of pair_geometry.CATALOGUES, beside its reach: one for which the oracle finds at
# least two groups and one of two or more members (all_coincident is one group at any b).  tests/test_fof_cases_cpu.py
# holds every (catalogue, b) that is not exact on purpose (edge_pairs at its reach of 49) to a margin above 6e-6.
SECOND_B = dict(plane=3.0, line=2.0, coincident=2.5, all_coincident=1.0, cap=5.5, corners=4.0, crowded_neighbours=0.25,
                offset_1e6=1.5, offset_f32=1.5, edge_pairs=24.5)
for _n in pg.ONE_CELL_SIZES:
    SECOND_B[f"one_cell_{_n}"] = 4.0 if _n < 4 else 0.9
EXACT = {("edge_pairs", "reach")}            # pairs at exactly d = 49 = b, on purpose
# The reach is given, not chosen, and among the 4.5 million pairs of these two one comes closer to it than 6e-6 (margins
# 4.3e-7 and 7.2e-7).  They stay in: the kernel's fp64 operations are the oracle's, one for one, so a margin matters
# only against a difference of a few ulp (1e-16); the CPU test holds these two to 1e-7 instead.
NEAR = {("offset_1e6", "reach"), ("offset_f32", "reach")}
MARGIN, NEAR_MARGIN = 6e-6, 1e-7


@functools.lru_cache(maxsize=None)
def geometry(name):
    """(pos float64, reach, cond) of a catalogue of pair_geometry; offset_f32's values are float32 values."""
    pos, par, cond = pg.CATALOGUES[name]()
    return frozen(np.ascontiguousarray(pos, dtype=np.float64)), par["binnr"] * par["binwidth"], cond


def geometry_cases():
    return [(name, which) for name in pg.CATALOGUES for which in ("reach", "second")]


def geometry_b(name, which):
    return geometry(name)[1] if which == "reach" else SECOND_B[name]


@functools.lru_cache(maxsize=None)
def geometry_groups(name, which):
    return orc.groups(geometry(name)[0], geometry_b(name, which))


# ------------------------------------------------------------------ 5. the cylinder
CL, CN = 100.0, 6000                        # the clustered catalogue of tests/test_gpu_fof.py
MEAN_SEP = (CL ** 3 / CN) ** (1.0 / 3.0)
CB, CB_PERP, CB_PARA = 0.2 * MEAN_SEP, 0.14 * MEAN_SEP, 0.75 * MEAN_SEP


@functools.lru_cache(maxsize=None)
def clustered(dtype="float64"):
    return frozen(orc.clustered(CL, CN, 11).astype(dtype))


@functools.lru_cache(maxsize=None)
def clustered_cylinder_open(los, nmin=1):
    return orc.groups(clustered(), CB_PERP, None, nmin, CB_PARA, los)


@functools.lru_cache(maxsize=None)
def clustered_sphere(periodic=True, nmin=1, dtype="float64"):
    return orc.groups(clustered(dtype), CB, CL if periodic else None, nmin)


COLLAPSED = dict(L=100.0, b_perp=1.0, b_para=30.0, n=200)


@functools.lru_cache(maxsize=None)
def collapsed(los, seed=38):
    """200 points in a periodic box of L = 100 for a cylinder of b_perp = 1, b_para = 30 along ``los``: under the floor
    of 27 cells the plan gives 5 x 5 cells across and ONE along the line of sight.  Six clumps of 20 (0.3 wide across,
    20 long along the line of sight), of which one sits across the periodic face of the line of sight (its members
    near 0 and near L along it), one across the face of the first perpendicular axis and one across a cell face of
    the 5 x 5 grid at 40; 80 background points.  The seed is the first of those tried for which no pair of any ``los``
    comes within 6e-5 of a limit."""
    rng = np.random.default_rng(seed)
    a_ax, b_ax = [c for c in range(3) if c != los]
    centres = {a_ax: [20.0, 99.95, 40.0, 70.0, 55.0, 85.0], b_ax: [30.0, 50.0, 70.0, 10.0, 90.0, 61.0],
               los: [99.0, 50.0, 30.0, 75.0, 10.0, 52.0]}
    parts = []
    for k in range(6):
        c = np.zeros((20, 3))
        c[:, a_ax] = centres[a_ax][k] + rng.uniform(-0.15, 0.15, 20)
        c[:, b_ax] = centres[b_ax][k] + rng.uniform(-0.15, 0.15, 20)
        c[:, los] = centres[los][k] + rng.uniform(-10.0, 10.0, 20)
        parts.append(c)
    parts.append(rng.uniform(0.0, 100.0, (80, 3)))
    pos = np.mod(np.concatenate(parts), 100.0)
    return frozen(pos[rng.permutation(len(pos))])


@functools.lru_cache(maxsize=None)
def collapsed_groups(los):
    return orc.groups(collapsed(los), 1.0, 100.0, 1, 30.0, los)


def lattice8():
    return np.stack(np.meshgrid(*(np.arange(8.0),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)


BELOW_ONE = float(np.nextafter(1.0, 0.0))
# (b_perp, b_para) -> periodic (links, group sizes), open (links, group sizes) of the 8^3 lattice (box L = 8), any los.
# Both 1: the 4 in-plane neighbours at rp = 1, each also one step along the line of sight, and the 2 along it alone: 14
# friends, 7 N links; open, per half-shell offset (da, db, dl) the (8 - |da|)(8 - |db|)(8 - |dl|) pairs inside:
# 3 * 448 + 4 * 392 = 2912.  b_para just below 1: the in-plane links only, 8 planes of 64.  b_perp just below 1: the
# links along the line of sight only, 64 lines of 8.
LATTICE8 = {
    (1.0, 1.0): ((7 * 512, [512]), (3 * 448 + 4 * 392, [512])),
    (1.0, BELOW_ONE): ((2 * 512, [64] * 8), (2 * 448, [64] * 8)),
    (BELOW_ONE, 1.0): ((512, [8] * 64), (448, [8] * 64)),
}


# ------------------------------------------------------------------ 6. boundaries, tiny N, features
FACE_L, FACE_B = 100.0, 2.0
FACE_SETS = ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2))    # 3 faces, 3 edges, the corner


@functools.lru_cache(maxsize=None)
def on_the_boundary(axes, seed=36):
    """1000 background points in [0, 100)^3 and, as particles 0 .. 4, a clump at the face, edge or corner where the
    coordinates ``axes`` are 0 = L (the others 37.25): 0 at exactly 100.0 on those axes; 1 at exactly 0.0 (distance 0
    from 0 in the periodic box); 2 and 3 a distance 0.9 b inside on either side (0.9 b / sqrt(len(axes)) per axis, from
    0.0 and from 100.0); 4 another 1.3 b per axis beyond 2, a friend of none of them.  Background points within 3 b of
    the clump are moved away.  Periodic: 0 - 3 are one group; open: 0 and 3, 1 and 2."""
    rng = np.random.default_rng(seed + sum(1 << a for a in axes))
    step = 0.9 * FACE_B / np.sqrt(float(len(axes)))
    clump = np.full((5, 3), 37.25)
    for a in axes:
        clump[:, a] = [100.0, 0.0, step, 100.0 - step, step + 1.3 * FACE_B]
    back = rng.uniform(0.0, 100.0, (1000, 3))
    d = np.abs(back[:, None, :] - clump[None, :, :])
    d = np.minimum(d, 100.0 - d)
    near = (np.sqrt((d * d).sum(axis=2)) < 3.0 * FACE_B).any(axis=1)
    back[near] = np.mod(back[near] + 50.0, 100.0)
    return frozen(np.concatenate([clump, back]))


TINY_N = (2, 3, 26, 27, 28)
TINY_L, TINY_B = 100.0, 2.0


@functools.lru_cache(maxsize=None)
def tiny(n, friends):
    """n points on a line along (1, 1/2, 1/4) from (97, 50, 50), wrapped into a box of L = 100: 0.8 b apart (friends:
    one group in the periodic box, two in open space once the line has crossed x = 100) or 1.3 b apart (no friends)."""
    step = (0.8 if friends else 1.3) * TINY_B / np.sqrt(1.0 + 0.25 + 0.0625)
    k = np.arange(n, dtype=np.float64)[:, None]
    pos = np.mod(np.array([97.0, 50.0, 50.0]) + k * step * np.array([1.0, 0.5, 0.25]), TINY_L)
    return frozen(pos[np.random.default_rng(37 + n).permutation(n)])


SIZES = (1, 63, 64, 65, 128, 129)           # the edges of fof_features_kernel's chunks of 64 lanes
SIZES_L, SIZES_B = 100.0, 0.6


@functools.lru_cache(maxsize=None)
def sized_groups(seed=38):
    """Clumps of exactly 1, 63, 64, 65, 128 and 129 points, each uniform in a cube 0.3 wide (every pair within it is
    closer than b = 0.6), the cubes tens of units apart in a box of L = 100; the clump of 65 lies across the face x = 0
    = L (wrapped), and one of its points is at exactly x = 100.0.  Shuffled."""
    rng = np.random.default_rng(seed)
    corners = [(10.0, 10.0, 10.0), (50.0, 20.0, 80.0), (80.0, 70.0, 30.0), (99.85, 45.0, 60.0), (30.0, 85.0, 40.0),
               (65.0, 50.0, 5.0)]
    parts = [np.array(c) + rng.uniform(0.0, 0.3, (s, 3)) for s, c in zip(SIZES, corners)]
    parts[3][0, 0] = 100.0
    pos = np.concatenate(parts)
    pos[:, 0] = np.where(pos[:, 0] > 100.0, pos[:, 0] - 100.0, pos[:, 0])
    return frozen(pos[rng.permutation(len(pos))])


def feature_inputs(n, seed=39):
    """(vel (n, 3), weights (n,)) float64."""
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 300.0, (n, 3)), rng.uniform(0.5, 2.0, n)


def feature_ratios(got, ref, length, u=2.0 ** -53):
    """|error| / bound per group of fof_features against fof_oracle.features, with the bound that
    tests/test_gpu_fof.py::test_features derives: (2 N + 4) u scale for the centre, (2 N + 1) u vscale for the velocity,
    N u W for the weight.  {key: ratios}; a key the oracle has but ``got`` lacks is left out."""
    n_g = np.asarray(length, dtype=np.float64)
    out = {"cm_position": np.abs(got["cm_position"] - ref["cm_position"]) / ((2 * n_g[:, None] + 4) * u * ref["scale"]),
           "weight": np.abs(got["weight"] - ref["weight"]) / (n_g * u * ref["weight"])}
    if "cm_velocity" in ref:
        err = np.abs(got["cm_velocity"] - ref["cm_velocity"])
        out["cm_velocity"] = err / ((2 * n_g[:, None] + 1) * u * ref["vscale"])
    return out
