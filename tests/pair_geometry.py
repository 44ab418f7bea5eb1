"""Degenerate catalogue geometry for the pair finders that walk the bounding-box cell grid of
astrild_amd/csrc/cell_grid.h (pairwise.hip, pairwise_pdf.hip): named, seeded catalogues, a numpy float64 restatement
of the planner (grid_box_plan, grid_box_cell) and a numpy model of the half-shell pair walk.  No GPU, no torch.

Every catalogue returns ``(pos, par, cond)``: positions (N, 3) float64; ``par = dict(binnr, binwidth)``, the reach being
``binnr * binwidth`` (every reach here is a float32 value, so the histogram kernel's float32(r) is the same number);
``cond``: what tests/test_pair_geometry_cpu.py asserts of it - the planned ``dims``, the least number of widening
``steps``, and ``sparse`` where not every bin can hold pairs.  All objects are far from the origin (z ~ 1000 and more),
so that u = r / |r| is finite."""
import numpy as np

# grid_offsets of cell_grid.h, copied as data: the cell itself and its 13 half-shell neighbours.
HALF_SHELL = (
    (0, 0, 0),
    (1, 0, 0),
    (-1, 1, 0), (0, 1, 0), (1, 1, 0),
    (-1, -1, 1), (0, -1, 1), (1, -1, 1),
    (-1, 0, 1), (0, 0, 1), (1, 0, 1),
    (-1, 1, 1), (0, 1, 1), (1, 1, 1),
)
MAX_CELLS = 1 << 20                         # GRID_MAX_CELLS
TILE = 256                                  # PV_BLOCK, PD_BLOCK: objects per tile of a cell


class Plan(dict):
    """lo, inv_cs (3,) float64; dims (3,) int; steps: how often the cell width was widened by 1.25; cells (N, 3) int:
    each object's cell; cell_id (N,): (z dims_y + y) dims_x + x, as grid_box_cell returns it."""
    __getattr__ = dict.__getitem__


def plan_box(lo, hi, n, reach, single=False, margins=True, rounding=np.floor, cap=None):
    """grid_box_plan for the bounding box [lo, hi] of n objects, op by op in float64: (dims, inv_cs, steps).
    ``cap``: the most cells the grid may have; None: the pair finders' min(n, MAX_CELLS) (a finder with a cap of its
    own, such as fof.hip's fof_plan_cap, passes it).  ``margins=False`` and ``rounding=np.ceil`` are the wrong planners
    of the sensitivity tests."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    ext = hi - lo
    amax = np.float64(0.0)
    for a in range(3):
        amax = max(amax, max(abs(lo[a]), abs(hi[a])))
    cap = float(1 if n < 1 else min(n, MAX_CELLS)) if cap is None else float(cap)
    dims = np.ones(3, dtype=np.int64)
    steps = 0
    if not single:
        s = np.float64(reach) * (1.0 + 1e-6) + amax * 1e-12 if margins else np.float64(reach)
        while True:
            prod = 1.0
            for a in range(3):
                m = rounding(ext[a] / s)
                if not m >= 1.0:
                    m = 1.0
                if m > float(MAX_CELLS):
                    m = float(MAX_CELLS)
                dims[a] = int(m)
                prod *= m
            if prod <= cap:
                break
            s = s * 1.25
            steps += 1
    inv_cs = np.zeros(3)
    for a in range(3):
        inv_cs[a] = float(dims[a]) / ext[a] if dims[a] > 1 else 0.0
    return dims, inv_cs, steps


def plan(pos, reach, single=False, cap=None, **variant):
    """grid_box_plan and grid_box_cell of cell_grid.h for a catalogue, op by op in float64; ``cap`` as in plan_box."""
    pos = np.asarray(pos, dtype=np.float64)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    dims, inv_cs, steps = plan_box(lo, hi, len(pos), reach, single, cap=cap, **variant)
    v = (pos - lo) * inv_cs
    v = np.where(v >= 0.0, v, 0.0)
    v = np.minimum(v, (dims - 1).astype(np.float64))
    cells = v.astype(np.int64)
    cell_id = (cells[:, 2] * dims[1] + cells[:, 1]) * dims[0] + cells[:, 0]
    return Plan(lo=lo, inv_cs=inv_cs, dims=dims, steps=steps, cells=cells, cell_id=cell_id)


def plan_periodic(pos, boxsize, reach, single=False):
    """grid_periodic_plan and grid_box_cell of cell_grid.h for a catalogue in the cube [0, boxsize]^3, op by op in
    float64: floor(L / (reach (1 + 1e-6))) cells per axis, at most 1024, lowered until the cube fits the cap
    max(27, min(N, MAX_CELLS)), at least 3 or else one cell; lo = 0, inv_cs = d / L (0 for one cell)."""
    pos = np.asarray(pos, dtype=np.float64)
    boxsize = np.float64(boxsize)
    cap = max(27, min(len(pos), MAX_CELLS))
    d = 1
    m = np.floor(boxsize / (np.float64(reach) * (1.0 + 1e-6)))
    if not single and m >= 3.0:
        d = 1024 if m > 1024.0 else int(m)
        while d * d * d > cap:
            d -= 1
    dims = np.full(3, d, dtype=np.int64)
    inv_cs = np.full(3, float(d) / boxsize if d > 1 else 0.0)
    v = (pos - 0.0) * inv_cs
    v = np.where(v >= 0.0, v, 0.0)
    v = np.minimum(v, (dims - 1).astype(np.float64))
    cells = v.astype(np.int64)
    cell_id = (cells[:, 2] * dims[1] + cells[:, 1]) * dims[0] + cells[:, 0]
    return Plan(lo=np.zeros(3), inv_cs=inv_cs, dims=dims, steps=0, cells=cells, cell_id=cell_id)


# (top s edge, objects, single_cell) -> cells per axis, in a box of L = 100: too wide a reach for 3 cells; exactly 3;
# 10 lowered to the cap of 300 cells; lowered to the least cap, max(27, N); one forced cell.
PERIODIC_L = 100.0
PERIODIC_CASES = {
    "two_fit": (40.0, 300, False, 1),
    "three_fit": (33.0, 300, False, 3),
    "cap_300": (9.99, 300, False, 6),
    "cap_30": (9.99, 30, False, 3),
    "single": (9.99, 300, True, 1),
}


def parse_grid_params(head):
    """``struct GridBoxParams`` of astrild_amd/csrc/cell_grid.h from the first 128 bytes (uint8) of a pair finder's
    workspace, where GridLayout puts it: GridBounds box: unsigned long long kmin[3], kmax[3] (bytes 0-47);
    double lo[3] (48), inv_cs[3] (72); int dims[3] (96); unsigned ncells (108), ntiles (112)."""
    head = np.ascontiguousarray(head, dtype=np.uint8)
    return dict(lo=head[48:72].view(np.float64), inv_cs=head[72:96].view(np.float64),
                dims=head[96:108].view(np.int32), ncells=int(head[108:112].view(np.uint32)[0]),
                ntiles=int(head[112:116].view(np.uint32)[0]))


def tiles(p):
    """prm->ntiles for a plan: sum over the cells of ceil(objects / TILE)."""
    return int(((np.bincount(p.cell_id) + TILE - 1) // TILE).sum())


def grid_pair_counts(pos, reach, binnr, binwidth, offsets=HALF_SHELL, planner=plan, dmax=None):
    """Pair counts per bin as the kernels' walk finds them: for every cell and every row of ``offsets`` the pairs of
    (cell, cell + offset), no wrap - an all-zero row is the cell itself, j > i only - binned by int(d / binwidth) when
    that is below binnr - and, with ``dmax``, when d <= dmax: binnr + 1 bins and dmax = reach give the pairs that the
    histogram kernel sees, those exactly at the reach in the last bin.  d = ((dx^2 + dy^2) + dz^2)^(1/2), as in the
    kernels and the oracles."""
    pos = np.asarray(pos, dtype=np.float64)
    p = planner(pos, reach)
    top = np.inf if dmax is None else dmax / binwidth
    dims = p.dims
    order = np.argsort(p.cell_id, kind="stable")
    ids, start = np.unique(p.cell_id[order], return_index=True)
    members = dict(zip(ids.tolist(), np.split(order, start[1:])))
    cnt = np.zeros(binnr, dtype=np.int64)
    for a, ia in members.items():
        ax, ay, az = a % dims[0], (a // dims[0]) % dims[1], a // (dims[0] * dims[1])
        for off in offsets:
            bx, by, bz = ax + off[0], ay + off[1], az + off[2]
            if not (0 <= bx < dims[0] and 0 <= by < dims[1] and 0 <= bz < dims[2]):
                continue
            ib = members.get(int((bz * dims[1] + by) * dims[0] + bx))
            if ib is None:
                continue
            d = pos[ia][:, None, :] - pos[ib][None, :, :]
            bf = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / binwidth
            if not any(off):
                bf = bf[np.triu_indices(len(ia), 1)]
            bf = bf[(bf < binnr) & (bf <= top)]
            cnt += np.bincount(bf.astype(np.int64).reshape(-1), minlength=binnr)
    return cnt


def brute_pair_counts(pos, binnr, binwidth, dmax=None):
    """Pair counts per bin over all pairs i < j: int(d / binwidth) when that is below binnr (and d <= dmax)."""
    pos = np.asarray(pos, dtype=np.float64)
    cnt = np.zeros(binnr, dtype=np.int64)
    for i in range(len(pos) - 1):
        d = pos[i] - pos[i + 1:]
        nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        bf = nrm / binwidth
        ok = bf < binnr if dmax is None else (bf < binnr) & (nrm <= dmax)
        cnt += np.bincount(bf[ok].astype(np.int64), minlength=binnr)
    return cnt


def pairs_per_offset(pos, reach):
    """{offset: number of pairs with d <= reach whose planned cells differ by it}, the difference taken so that it is a
    row of HALF_SHELL; a pair two or more cells apart counts under its own (out of table) difference."""
    pos = np.asarray(pos, dtype=np.float64)
    cells = plan(pos, reach).cells
    out = {}
    for i in range(len(pos) - 1):
        d = pos[i] - pos[i + 1:]
        near = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= reach
        for off in (cells[i + 1:][near] - cells[i]).tolist():
            if tuple(off[::-1]) < (0, 0, 0):               # the half shell: z, then y, then x positive first
                off = [-c for c in off]
            out[tuple(off)] = out.get(tuple(off), 0) + 1
    return out


def velocities(pos, seed, sigma=6.0, infall=0.05):
    """Cartesian (N, 3) velocities: normal scatter plus a coherent infall towards the catalogue's centre, so that the
    per-bin sums are not pure cancellation."""
    pos = np.asarray(pos, dtype=np.float64)
    rng = np.random.default_rng(seed)
    return -infall * (pos - pos.mean(axis=0)) + rng.normal(0.0, sigma, pos.shape)


# ------------------------------------------------------------------ the catalogues
FAR = np.array([0.0, 0.0, 1000.0])
REACH10 = dict(binnr=8, binwidth=1.25)


def plane():
    """2000 objects in the plane z = 1000: zero extent on one axis beside two wide ones."""
    rng = np.random.default_rng(101)
    pos = np.zeros((2000, 3))
    pos[:, :2] = rng.uniform(0.0, 200.0, (2000, 2))
    pos[0, :2], pos[1, :2] = (0.0, 0.0), (200.0, 200.0)
    return pos + FAR, dict(REACH10), dict(dims=(19, 19, 1))


def line():
    """1500 objects on a line along x: zero extent on two axes."""
    rng = np.random.default_rng(102)
    pos = np.zeros((1500, 3))
    pos[:, 0] = rng.uniform(0.0, 3000.0, 1500)
    pos[0, 0], pos[1, 0] = 0.0, 3000.0
    pos[:, 1] = 5.0
    return pos + FAR, dict(REACH10), dict(dims=(299, 1, 1))


def coincident():
    """300 copies of one point, where the eight cells of a 2 x 2 x 2 grid meet, and 300 objects scattered around it:
    44 850 pairs with d = 0 in bin 0, whose p = 0 / 0 turns the sums of that bin into NaN."""
    rng = np.random.default_rng(103)
    centre = np.array([40.0, -30.0, 1000.0])
    scatter = rng.uniform(-10.5, 10.5, (300, 3))
    scatter[0], scatter[1] = -10.5, 10.5
    pos = np.concatenate([np.tile(centre, (300, 1)), centre + scatter])
    return pos[rng.permutation(600)], dict(REACH10), dict(dims=(2, 2, 2))


def all_coincident():
    """64 copies of one point: all three extents are 0."""
    return np.tile(np.array([3.0, -4.0, 1000.0]), (64, 1)), dict(REACH10), dict(dims=(1, 1, 1), sparse=True)


def cap():
    """56 objects over a 1000-wide cube at reach 10: 100^3 cells of the least width are more than the 56 allowed, so
    the planner widens (15 steps, to 3 x 3 x 3).  The eight corners of the cube fix the grid; 24 close pairs then
    sit astride faces, edges and corners of the grid that the planner returns for that box."""
    lo, hi, n = FAR, FAR + 1000.0, 56
    dims, inv_cs, _ = plan_box(lo, hi, n, 10.0)
    corners = np.array([[x, y, z] for z in (0.0, 1000.0) for y in (0.0, 1000.0) for x in (0.0, 1000.0)]) + FAR
    rng = np.random.default_rng(104)
    pts = []
    for k in range(24):
        normal = np.array(HALF_SHELL[1 + k % 13], dtype=np.float64)
        unit = normal / np.sqrt((normal * normal).sum())
        # a point on the face / edge / corner between cell (1, 1, 1) (or, every other pair, (0, 0, 0) + ...) and its
        # neighbour along `normal`: the shared planes where normal != 0, inside the cell elsewhere
        width = (hi - lo) / dims
        base = np.where(normal > 0, 2.0, 1.0) * width
        mid = np.where(normal != 0, base, width * rng.uniform(1.2, 1.8, 3))
        sep = (k % 8 + 0.5) * 1.25
        pts += [lo + mid - 0.5 * sep * unit, lo + mid + 0.5 * sep * unit]
    return np.concatenate([corners, np.array(pts)]), dict(REACH10), dict(dims=(3, 3, 3), steps=1, sparse=True)


def corners():
    """A 3 x 3 x 3 grid (cells 11 wide at reach 10) with one pair for each of the 13 half-shell offsets, 1.5 on either
    side of the face, edge or corner that a cell, drawn at random, shares with its neighbour at that offset.  The
    seed is the one of 2000 tried that leaves the fewest pairs on the busiest offset: 1 to 5 on each, 13 inside
    cells, 28 objects in all - one lost or doubled offset changes a count."""
    rng = np.random.default_rng(206)
    pts = [np.zeros(3), np.full(3, 33.0)]
    for off in HALF_SHELL[1:]:
        o = np.array(off, dtype=np.float64)
        base = np.array([rng.integers(0, 2) if c > 0 else rng.integers(1, 3) if c < 0 else rng.integers(0, 3)
                         for c in off])
        shared = 11.0 * (base + (o > 0))
        mid = np.where(o != 0, shared, 11.0 * base + rng.uniform(2.0, 9.0, 3))
        pts += [mid - 1.5 * o, mid + 1.5 * o]
    return np.array(pts) + FAR, dict(REACH10), dict(dims=(3, 3, 3), sparse=True)


def crowded_neighbours():
    """Two cells of 700 objects each (2 x 256 + 188: three i tiles, three j stages, ragged tails) on either side of a
    shared face, within reach of each other; two far objects stretch the box to 5 x 2 x 2 cells."""
    rng = np.random.default_rng(106)
    left = rng.uniform([27.2, 1.0, 1.0], [31.1, 9.0, 9.0], (700, 3))
    right = rng.uniform([31.3, 1.0, 1.0], [35.2, 9.0, 9.0], (700, 3))
    pos = np.concatenate([[[0.0, 0.0, 0.0]], left, right, [[52.0, 21.0, 21.0]]])
    return pos[rng.permutation(len(pos))] + FAR, dict(REACH10), dict(dims=(5, 2, 2))


def offset_1e6():
    """3000 objects in a 40-wide cube a million away from the origin on every axis, fp64.  Reach 12: three cells of
    13.3 per axis, where a planner that rounds up would make four of 10."""
    rng = np.random.default_rng(107)
    pos = rng.uniform(0.0, 40.0, (3000, 3))
    pos[0], pos[1] = 0.0, 40.0
    return pos + 1.0e6, dict(binnr=8, binwidth=1.5), dict(dims=(3, 3, 3))


def offset_f32():
    """The same cube 4096 away, rounded to float32 (ulp 4.9e-4) and widened again: what a float32 catalogue holds."""
    pos = offset_1e6()[0] - 1.0e6 + 4096.0
    return pos.astype(np.float32).astype(np.float64), dict(binnr=8, binwidth=1.5), dict(dims=(3, 3, 3))


def edge_pairs():
    """Integer coordinates, reach 49 = 7 x 7: pairs exactly 7 k apart (on bin edges; 49 is the reach itself), along x
    and along k (2, 3, 6), across cell faces and cell corners of the 5 x 2 x 2 grid over a 294 x 120 x 120 box.
    The pair (196, 245) is for a planner without its margins: that one makes six cells 49 wide along x, with
    inv_cs = fl(6 / 294), and 196 inv_cs = 3.99.., 245 inv_cs = 5: a pair at the reach, two cells apart."""
    pts = [(0, 0, 0), (294, 120, 120)]
    for y, z in ((10, 10), (100, 30), (30, 100), (70, 110)):
        pts += [(196, y, z), (245, y, z)]
    for face in (58, 117, 176, 235):                        # the faces at 58.8 k, along x
        for k in range(1, 8):
            pts += [(face - 3 * k, 20 + k, 90), (face + 4 * k, 20 + k, 90)]
    for face in (117, 176):                                 # the corners (58.8 k, 60, 60), along (+-2, 3, 6) k
        for k, sx in ((1, 1), (1, -1), (3, 1), (7, 1), (7, -1)):
            a = np.array([face + (1 - sx) * k, 60 - k, 60 - 3 * k - 1])
            pts += [tuple(a), tuple(a + k * np.array([2 * sx, 3, 6]))]
    pos = np.array(sorted(set(tuple(int(c) for c in p) for p in pts)), dtype=np.float64)
    return pos + FAR, dict(binnr=7, binwidth=7.0), dict(dims=(5, 2, 2), sparse=True)


def one_cell(n):
    """n objects in a cube 8 wide, narrower than the reach: one cell, the j > i triangle over ceil(n / 256) tiles."""
    rng = np.random.default_rng(200 + n)
    return rng.uniform(0.0, 8.0, (n, 3)) + np.array([12.0, -7.0, 1000.0]), dict(REACH10), dict(dims=(1, 1, 1),
                                                                                               sparse=n < 255)


ONE_CELL_SIZES = (2, 3, 255, 256, 257, 512, 513)
CATALOGUES = dict(plane=plane, line=line, coincident=coincident, all_coincident=all_coincident, cap=cap,
                  corners=corners, crowded_neighbours=crowded_neighbours, offset_1e6=offset_1e6, offset_f32=offset_f32,
                  edge_pairs=edge_pairs)
for _n in ONE_CELL_SIZES:
    CATALOGUES[f"one_cell_{_n}"] = (lambda n: lambda: one_cell(n))(_n)
