"""CPU: the catalogues of tests/pair_geometry.py do what they claim, the numpy model of the cell-grid pair walk equals
brute force on every one of them and stops doing so under each single mutation of the offset table or the planner, and
the numpy oracle of the transverse-velocity estimator, run in two orders, stays inside the tolerance that
tests/test_gpu_pair_geometry.py grants the kernels."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

from tests import pair_geometry as pg
from tests import pairwise_oracle as orc

NAMES = list(pg.CATALOGUES)


@functools.lru_cache(maxsize=None)
def catalogue(name):
    pos, par, cond = pg.CATALOGUES[name]()
    pos.setflags(write=False)
    return pos, par, cond


@functools.lru_cache(maxsize=None)
def brute(name, at_reach=0):
    """Brute-force counts; at_reach = 1: one bin more, for the pairs exactly at the reach (d <= reach is kept)."""
    pos, par, _ = catalogue(name)
    return pg.brute_pair_counts(pos, par["binnr"] + at_reach, par["binwidth"], reach_of(par) if at_reach else None)


def reach_of(par):
    return par["binnr"] * par["binwidth"]


def test_the_module_needs_no_gpu():
    import sys
    assert "torch" not in vars(pg) and not any(getattr(v, "__name__", "") == "torch" for v in vars(pg).values())
    assert "tests.pair_geometry" in sys.modules


# ------------------------------------------------------------------ catalogue conditions
@pytest.mark.parametrize("name", NAMES)
def test_catalogue_conditions(name):
    pos, par, cond = catalogue(name)
    reach = reach_of(par)
    assert np.float64(np.float32(reach)) == reach           # both kernels plan for the same reach
    assert pos.dtype == np.float64 and pos.shape[1] == 3 and np.all(np.abs(pos[:, 2]) >= 900.0)
    p = pg.plan(pos, reach)
    assert tuple(p.dims) == cond["dims"]
    assert p.steps >= cond.get("steps", 0)
    if "steps" not in cond:
        assert p.steps == 0
    ext = pos.max(axis=0) - pos.min(axis=0)
    for a in range(3):                                      # dims of 1 <-> inv_cs of 0; zero extent only where claimed
        assert (p.inv_cs[a] == 0.0) == (p.dims[a] == 1)
        assert np.isfinite(p.inv_cs[a])
    assert np.all((p.cells >= 0) & (p.cells < p.dims))
    one = pg.plan(pos, reach, single=True)
    assert tuple(one.dims) == (1, 1, 1) and not one.cell_id.any() and pg.tiles(one) == -(-len(pos) // pg.TILE)
    cnt = brute(name)
    assert cnt.sum() > 0
    if not cond.get("sparse"):
        assert np.all(cnt > 0), cnt                         # every bin below the reach holds pairs
    if name == "plane":
        assert ext[2] == 0.0 and len(pos) == 2000
    if name == "line":
        assert ext[1] == 0.0 and ext[2] == 0.0 and len(pos) == 1500
    if name == "coincident":
        assert np.all(ext > 0.0) and cnt[0] >= 300 * 299 // 2
        assert np.sum(np.all(pos == pos[np.argmax(np.all(pos == np.array([40.0, -30.0, 1000.0]), axis=1))], axis=1)) == 300
    if name == "all_coincident":
        assert np.all(ext == 0.0) and cnt.tolist() == [64 * 63 // 2] + [0] * 7
    if name.startswith("one_cell"):
        assert np.all(ext < reach) and len(pos) == int(name.rsplit("_", 1)[1])


def test_cap_catalogue_is_cap_limited():
    pos, par, _ = catalogue("cap")
    p = pg.plan(pos, 10.0)
    assert len(pos) == 56 and p.steps == 15 and int(np.prod(p.dims)) <= len(pos)
    # without the cap the grid would be 99^3 cells; one widening step fewer would still be more cells than objects
    unlimited, _, steps = pg.plan_box(pos.min(axis=0), pos.max(axis=0), pg.MAX_CELLS, 10.0)
    assert tuple(unlimited) == (99, 99, 99) and steps == 0
    per = pg.pairs_per_offset(pos, 10.0)
    assert set(per) == set(pg.HALF_SHELL)                   # close pairs astride every kind of face of the planned grid
    assert sum(per.values()) - per[(0, 0, 0)] >= 24 and brute("cap").sum() == sum(per.values())
    assert np.all(brute("cap") > 0)


def test_corners_put_a_few_pairs_on_each_offset():
    pos, par, _ = catalogue("corners")
    per = pg.pairs_per_offset(pos, 10.0)
    assert set(per) == set(pg.HALF_SHELL)
    for off in pg.HALF_SHELL[1:]:
        assert 1 <= per[off] <= 10, (off, per[off])
    assert per[(0, 0, 0)] <= 20 and len(pos) < 64


def test_crowded_neighbours_are_crowded():
    pos, par, _ = catalogue("crowded_neighbours")
    p = pg.plan(pos, 10.0)
    per_cell = np.bincount(p.cell_id, minlength=20)
    a, b = np.argsort(per_cell)[-2:]
    assert abs(int(a) - int(b)) == 1 and min(a, b) % 5 != 4             # neighbours along x, in one row of cells
    assert per_cell[a] >= 513 and per_cell[b] >= 513 and per_cell[a] % 256 and per_cell[b] % 256
    assert pg.tiles(p) == 3 + 3 + 1 + 1
    d = pos[p.cell_id == a][:, None, :] - pos[p.cell_id == b][None, :, :]
    assert np.sum(np.sqrt((d * d).sum(axis=-1)) < 10.0) >= 10_000


def test_edge_pairs_sit_on_edges():
    pos, par, _ = catalogue("edge_pairs")
    bw, reach = par["binwidth"], reach_of(par)
    p = pg.plan(pos, reach)
    assert np.all(pos == np.round(pos))
    i, j = np.triu_indices(len(pos), 1)
    d = pos[i] - pos[j]
    nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    off = np.abs(p.cells[i] - p.cells[j])
    face, corner = (off.sum(axis=1) == 1), np.all(off == 1, axis=1)
    on_edge = (nrm / bw == np.round(nrm / bw)) & (nrm < reach)
    for where in (face, corner):
        assert np.sum(on_edge & where) >= 1 and np.sum((nrm == reach) & where) >= 1
    assert np.all(np.isin(np.arange(1, par["binnr"]), (nrm[on_edge] / bw).astype(int)))      # every inner edge is hit
    assert brute("edge_pairs", 1)[-1] == np.sum(nrm == reach) >= 4     # the bin past the last: exactly the reach


@pytest.mark.parametrize("name", ["offset_1e6", "offset_f32"])
def test_offset_catalogues_have_coarse_coordinates(name):
    pos, par, _ = catalogue(name)
    if name == "offset_1e6":
        assert np.all(pos >= 1.0e6) and np.spacing(pos.min()) > 1e-10
    else:
        assert np.array_equal(pos, pos.astype(np.float32).astype(np.float64)) and np.spacing(np.float32(4096.0)) > 4e-4
        assert not np.array_equal(pos, pg.offset_1e6()[0] - 1.0e6 + 4096.0)


# ------------------------------------------------------------------ the model against brute force
@pytest.mark.parametrize("name", NAMES)
def test_model_equals_brute_force(name):
    pos, par, _ = catalogue(name)
    npt.assert_array_equal(pg.grid_pair_counts(pos, reach_of(par), par["binnr"], par["binwidth"]), brute(name))
    # one bin more than the reach covers: the pairs exactly at the reach, which the histogram kernel sees (d <= r)
    reach = reach_of(par)
    npt.assert_array_equal(pg.grid_pair_counts(pos, reach, par["binnr"] + 1, par["binwidth"], dmax=reach), brute(name, 1))


# ------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("k", range(1, 14))
def test_a_lost_offset_loses_pairs_on_corners(k):
    pos, par, _ = catalogue("corners")
    table = pg.HALF_SHELL[:k] + pg.HALF_SHELL[k + 1:]
    got = pg.grid_pair_counts(pos, 10.0, par["binnr"], par["binwidth"], offsets=table)
    per = pg.pairs_per_offset(pos, 10.0)[pg.HALF_SHELL[k]]
    lost = brute("corners") - got
    assert np.all(lost >= 0) and 1 <= lost.sum() <= per           # `per` counts d <= 10, the bins d < 10


@pytest.mark.parametrize("k", range(14))
def test_a_doubled_offset_doubles_pairs_on_corners(k):
    pos, par, _ = catalogue("corners")
    got = pg.grid_pair_counts(pos, 10.0, par["binnr"], par["binwidth"], offsets=pg.HALF_SHELL + (pg.HALF_SHELL[k],))
    extra = got - brute("corners")
    assert np.all(extra >= 0) and 1 <= extra.sum() <= pg.pairs_per_offset(pos, 10.0)[pg.HALF_SHELL[k]]


def test_the_opposite_offset_is_not_the_same_table():
    """A row with its sign flipped still visits every unordered pair of cells once: the model cannot tell, and neither
    can a count.  Stated so that nobody expects this suite to notice."""
    pos, par, _ = catalogue("corners")
    table = tuple(tuple(-c for c in off) for off in pg.HALF_SHELL)
    npt.assert_array_equal(pg.grid_pair_counts(pos, 10.0, par["binnr"], par["binwidth"], offsets=table), brute("corners"))


def variant(**kw):
    return lambda pos, reach: pg.plan(pos, reach, **kw)


def test_a_planner_without_margins_loses_a_pair_at_the_reach():
    """Cells exactly as wide as the reach: fl(6 / 294) 196 < 4 and fl(6 / 294) 245 = 5, so the pair (196, 245), 49
    apart, is two cells apart.  Only a pair exactly at the reach can be lost this way (in exact arithmetic objects two
    cells apart are more than a cell width apart), so the bin past the last one is what shows it: the pairs the
    histogram kernel sees with d == r.  No other catalogue can bite: their pairs are not at the reach to the last bit."""
    pos, par, _ = catalogue("edge_pairs")
    reach = reach_of(par)
    wrong = pg.plan(pos, reach, margins=False)
    assert tuple(wrong.dims) == (6, 2, 2) and wrong.steps == 0
    x = pos[:, 0]
    assert set(wrong.cells[x == 196.0, 0]) == {3} and set(wrong.cells[x == 245.0, 0]) == {5}
    got = pg.grid_pair_counts(pos, reach, par["binnr"] + 1, par["binwidth"], planner=variant(margins=False), dmax=reach)
    lost = brute("edge_pairs", 1) - got
    assert lost[:-1].sum() == 0 and 4 <= lost[-1] <= brute("edge_pairs", 1)[-1]     # the four (196, 245) pairs among them
    right = pg.plan(pos, reach)
    assert set(right.cells[x == 196.0, 0]) == {3} and set(right.cells[x == 245.0, 0]) == {4}


@pytest.mark.parametrize("name", ["offset_1e6", "offset_f32", "edge_pairs"])
def test_a_planner_that_rounds_up_loses_pairs(name):
    """ceil(ext / s) cells are narrower than the reach unless ext is a multiple of it, as in `plane` (200 / 10) and
    `crowded_neighbours`, whose pairs all lie within 8 of one face: those two cannot bite.  In `edge_pairs` the cells
    along y and z shrink from 60 to 40, which the pairs along 7 (2, 3, 6), 42 apart in z, straddle."""
    pos, par, _ = catalogue(name)
    reach = reach_of(par)
    extra = 1 if name == "edge_pairs" else 0
    wrong = pg.plan(pos, reach, rounding=np.ceil)
    assert np.any(wrong.dims > pg.plan(pos, reach).dims)
    got = pg.grid_pair_counts(pos, reach, par["binnr"] + extra, par["binwidth"], planner=variant(rounding=np.ceil),
                              dmax=reach if extra else None)
    lost = brute(name, extra) - got
    assert np.all(lost >= 0) and lost.sum() >= 1 and lost[-1] >= 1     # the widest bin goes first


@pytest.mark.parametrize("case", list(pg.PERIODIC_CASES))
def test_the_periodic_plan_gives_the_stated_cells(case):
    """The restatement of grid_periodic_plan alone: the cells per axis of the five cases, d / L bit for bit, every
    object in a cell of the cube, and cells at least as wide as the reach."""
    top, n, single, d = pg.PERIODIC_CASES[case]
    pos = np.random.default_rng(11).uniform(0.0, pg.PERIODIC_L, (n, 3))
    p = pg.plan_periodic(pos, pg.PERIODIC_L, top, single)
    assert p.dims.tolist() == [d, d, d]
    npt.assert_array_equal(p.lo, np.zeros(3))
    npt.assert_array_equal(p.inv_cs, np.full(3, d / pg.PERIODIC_L if d > 1 else 0.0))
    assert p.cell_id.min() >= 0 and p.cell_id.max() < d ** 3
    assert d ** 3 <= max(27, n) and (d == 1 or (d >= 3 and pg.PERIODIC_L / d >= top))
    # one cell: two tiles of its 300 objects; else fewer than a tile of objects in every cell
    assert pg.tiles(p) == (-(-n // pg.TILE) if d == 1 else len(np.unique(p.cell_id)))


# ------------------------------------------------------------------ the reference inside its own tolerance
def sums_bound(cnt, sum_abs):
    """|a - b| of two orders of an fp64 sum of `cnt` terms: cnt 2^-52 sum|term|; at least 8 terms' worth, since the
    terms themselves differ by a few ulp when i and j swap ((2p - u_i d_i) - u_j d_j is not symmetric to the bit)."""
    return np.maximum(cnt, 8) * 2.0 ** -52 * sum_abs


@functools.lru_cache(maxsize=None)
def oracle(name, permuted=False):
    pos, par, _ = catalogue(name)
    vel = pg.velocities(pos, 7)
    if permuted:
        order = np.random.default_rng(8).permutation(len(pos))
        pos, vel = pos[order], vel[order]
    u, _ = orc.angles_and_velocities(pos, np.zeros((len(pos), 2)))
    return orc.pair_sums(pos, u, vel, par["binnr"], par["binwidth"], with_abs=True)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_in_two_orders_stays_inside_the_bound(name):
    a, b = oracle(name), oracle(name, True)
    npt.assert_array_equal(a[2], b[2])
    npt.assert_array_equal(a[2], brute(name))
    nan = np.isnan(a[0])
    npt.assert_array_equal(nan, np.isnan(b[0]))
    npt.assert_array_equal(nan, np.isnan(a[1]))
    npt.assert_array_equal(nan, np.isnan(b[1]))
    if name in ("coincident", "all_coincident"):
        assert nan.tolist() == [True] + [False] * 7
    else:
        assert not nan.any()
    ok = ~nan
    worst = 0.0
    for x, y, scale in ((a[0], b[0], a[3]), (a[1], b[1], a[1])):
        err, bound = np.abs(x - y)[ok], sums_bound(a[2], scale)[ok]
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300), initial=0.0)))
        assert np.all(err <= bound), (name, err, bound)
    print(f"{name}: oracle order error / bound {worst:.3g}")
    assert np.all(a[3][ok] >= np.abs(a[0][ok]))
