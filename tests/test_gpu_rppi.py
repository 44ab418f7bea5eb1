"""GPU: the (r_p, pi) pair counts (ast_rppi_pair_counts / ast_rppi_cross_counts / ast_rppi_jk_counts through
device.rp_pi_pair_counts / rp_pi_cross_counts / rp_pi_jackknife_counts) and rp_pi_tpcf / wp and their jackknife variants
on top of them.  Every count is an int64 compared exactly with the numpy oracle (tests/rppi_oracle.py): a lattice with
known answers, random catalogues periodic and open under both planners with the planned grid read back, an axis with
one cell, a crowded cell, the faces of the periodic box, degenerate sets, ties to the pairwise-velocity and (s, mu)
kernels, the jackknife's endpoint table, the estimators, and dirty scratch memory."""
import functools
import itertools

import numpy as np
import numpy.testing as npt
import pytest

from tests import pair_geometry as pg
from tests import rppi_oracle as orc
from tests import tpcf_cross_oracle as xorc
from tests import tpcf_jackknife_oracle as jorc
from tests import tpcf_oracle as sorc
from tests.dirty_memory import ZERO_BYTES, dirty_alloc             # noqa: F401  (dirty_alloc: a fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

L = 100.0
RP = np.geomspace(0.5, 8.0, 9)
PI = np.linspace(0.0, 30.0, 16)
PLANNERS = {"aniso": {}, "iso": {"ASTRILD_RPPI_ANISO": "0"}, "one_cell": {"ASTRILD_TPCF_CELLS": "0"}}


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


def use(monkeypatch, planner):
    for key, value in PLANNERS[planner].items():
        monkeypatch.setenv(key, value)


def gpu_cross(a, b, rp=RP, pi=PI, boxsize=None, vel1=None, vel2=None, los=2):
    from astrild_amd import device as dev
    out = dev.rp_pi_cross_counts(a, b, rp, pi, boxsize=boxsize, vel1=vel1, vel2=vel2, los=los)
    assert out.dtype == torch.int64 and tuple(out.shape) == (len(rp) - 1, len(pi) - 1)
    return dev.to_numpy(out)


def gpu_auto(pos, boxsize, rp=RP, pi=PI, vel=None, los=2):
    from astrild_amd import device as dev
    out = dev.rp_pi_pair_counts(pos, boxsize, rp, pi, vel=vel, los=los)
    assert out.dtype == torch.int64 and tuple(out.shape) == (len(rp) - 1, len(pi) - 1)
    return dev.to_numpy(out)


@functools.lru_cache(maxsize=None)
def sets():
    return sorc.uniform(3000, L, 71), sorc.uniform(2000, L, 72)         # shared: the tests copy before they write


@functools.lru_cache(maxsize=None)
def ref(kind, los=2, periodic=True):
    """The oracle's counts for the two random sets: "ab", "ba" (cross) or "a" (auto); computed once, read-only."""
    a, b = sets()
    box = L if periodic else None
    out = orc.rppi_auto_brute(a, RP, PI, los, box) if kind == "a" else \
        orc.rppi_cross_brute(*((a, b) if kind == "ab" else (b, a)), RP, PI, los, box)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------- 1. lattice
@pytest.mark.parametrize("planner", list(PLANNERS))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("los", [0, 1, 2])
def test_lattice(los, dtype, planner, monkeypatch):
    # integer edges 0..3: every pair sits on an r_p edge or on r_p^2 in {2, 5, 8}, and on a pi edge.  m = 12 is the
    # smallest even lattice whose box admits the top edge 3 (< 12 / 3): 3 x 3 x 3 cells of width 4, with lattice
    # planes on the cell faces.
    use(monkeypatch, planner)
    edges = np.arange(4.0)
    lat = sorc.lattice(12).astype(dtype)
    exp = orc.lattice_expected(12, edges, edges, los)
    assert exp.sum() > 0
    npt.assert_array_equal(gpu_auto(lat, 12.0, edges, edges, los=los), exp)
    npt.assert_array_equal(gpu_cross(lat, lat, edges, edges, boxsize=12.0, los=los), 2 * exp)


@pytest.mark.parametrize("plan, single", [(0, 0), (1, 0), (0, 1)], ids=list(PLANNERS))
@pytest.mark.parametrize("los", [0, 1, 2])
def test_lattice_of_8_through_the_c_abi(los, plan, single):
    # m = 8 with the same edges: the top edge 3 is above 8 / 3, which check_rp_pi_edges refuses, so this goes to the
    # library itself, which plans one cell per axis (floor(8 / 3) = 2) and leaves the pairs to the minimum image
    edges = np.arange(4.0)
    lat = sorc.lattice(8)
    exp = orc.lattice_expected(8, edges, edges, los)
    assert exp.sum() > 0
    counts, prm = c_abi_cross(lat, lat, edges, edges, 8.0, los, plan, single)
    npt.assert_array_equal(counts, 2 * exp)
    assert prm["dims"].tolist() == [1, 1, 1]


# ---------------------------------------------------------------- 2. random catalogues, and the planned grid
@pytest.mark.parametrize("planner", list(PLANNERS))
@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
def test_random_catalogues(periodic, planner, monkeypatch):
    use(monkeypatch, planner)
    a, b = sets()
    box = L if periodic else None
    assert ref("ab", 2, periodic).sum() > 50_000 and (ref("ab", 2, periodic) > 0).all()
    npt.assert_array_equal(gpu_cross(a, b, boxsize=box), ref("ab", 2, periodic))
    npt.assert_array_equal(gpu_cross(b, a, boxsize=box), ref("ba", 2, periodic))          # swapped sets
    npt.assert_array_equal(ref("ba", 2, periodic), ref("ab", 2, periodic))
    npt.assert_array_equal(gpu_cross(a, None, boxsize=box), ref("a", 2, periodic))
    if periodic:
        npt.assert_array_equal(gpu_auto(a, L), ref("a", 2, True))
        assert (ref("ab", 2, True) - ref("ab", 2, False)).sum() > 1000                    # pairs across the faces


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
@pytest.mark.parametrize("los", [0, 1])
def test_each_line_of_sight(los, periodic):
    a, b = sets()
    box = L if periodic else None
    npt.assert_array_equal(gpu_cross(a, b, boxsize=box, los=los), ref("ab", los, periodic))
    npt.assert_array_equal(gpu_cross(a, None, boxsize=box, los=los), ref("a", los, periodic))
    assert not np.array_equal(ref("ab", los, periodic), ref("ab", 2, periodic))


def test_mixed_dtypes_and_device_tensors():
    from astrild_amd import device as dev
    a, b = sets()
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    exp = orc.rppi_cross_brute(a32, b, RP, PI, 2, L)
    npt.assert_array_equal(gpu_cross(a32, b, boxsize=L), exp)
    npt.assert_array_equal(gpu_cross(b, a32, boxsize=L), exp)
    npt.assert_array_equal(gpu_cross(a, b32), orc.rppi_cross_brute(a, b32, RP, PI, 2, None))
    npt.assert_array_equal(gpu_cross(dev.as_device(a), dev.as_device(b), boxsize=L), ref("ab"))
    npt.assert_array_equal(gpu_cross(dev.as_device(a32), dev.as_device(b), boxsize=L), exp)
    npt.assert_array_equal(gpu_auto(dev.as_device(a), L), ref("a"))


@pytest.mark.parametrize("los", [0, 2])
def test_velocities_shift_each_set_in_its_own_dtypes(los):
    a, b = sets()
    rng = np.random.default_rng(73)
    va, vb = rng.normal(0.0, 400.0, a.shape), rng.normal(0.0, 400.0, b.shape).astype(np.float32)
    a32 = a.astype(np.float32)
    sa, sb = sorc.shift_and_wrap(a32, va, L, los), sorc.shift_and_wrap(b, vb, L, los)
    exp = orc.rppi_cross_brute(sa, sb, RP, PI, los, L)
    assert not np.array_equal(exp, ref("ab", los))
    npt.assert_array_equal(gpu_cross(a32, b, boxsize=L, vel1=va, vel2=vb, los=los), exp)
    npt.assert_array_equal(gpu_auto(a32, L, vel=va, los=los), orc.rppi_auto_brute(sa, RP, PI, los, L))
    # open boundaries: the shift without the wrap; only set 2 moves
    ob = b.copy()
    ob[:, los] += vb[:, los] / np.float32(100.0)
    npt.assert_array_equal(gpu_cross(a, b, vel2=vb, los=los), orc.rppi_cross_brute(a, ob, RP, PI, los, None))


def c_abi_cross(a, b, rp, pi, box, los, plan, single=0):
    """ast_tpcf_cross_prepare / ast_rppi_cross_counts on a workspace of the test's own: (counts, GridBoxParams)."""
    from astrild_amd import _lib, device as dev
    lib = _lib.lib()
    p1, p2 = dev.as_device(np.asarray(a, dtype=np.float64)), dev.as_device(np.asarray(b, dtype=np.float64))
    n1, n2, nrp, npi = len(a), len(b), len(rp) - 1, len(pi) - 1
    ws_bytes = lib.ast_tpcf_cross_workspace_bytes(n1, n2, nrp, npi)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    bounds = torch.empty(12, dtype=torch.float64, device="cuda")
    counts = torch.full((nrp, npi), -1, dtype=torch.int64, device="cuda")
    rp_d, pi_d = dev.as_device(np.asarray(rp, dtype=np.float64)), dev.as_device(np.asarray(pi, dtype=np.float64))
    st = dev.stream()
    _lib.check(lib.ast_tpcf_cross_prepare(dev.ptr(p1), _lib.F64, None, _lib.F64, n1, dev.ptr(p2), _lib.F64, None,
                                          _lib.F64, n2, los, box, dev.ptr(work), ws_bytes, dev.ptr(bounds), st),
               "ast_tpcf_cross_prepare")
    _lib.check(lib.ast_rppi_cross_counts(dev.ptr(work), ws_bytes, n1, n2, 0, box, los, dev.ptr(rp_d), nrp, dev.ptr(pi_d),
                                         npi, single, plan, dev.ptr(counts), st), "ast_rppi_cross_counts")
    torch.cuda.synchronize()
    return counts.cpu().numpy(), pg.parse_grid_params(work[:128].cpu().numpy())


def permuted(across, along, los):
    dims = [across, across, across]
    dims[los] = along
    return dims


@pytest.mark.parametrize("los", [0, 1, 2])
def test_planned_grid_of_the_random_catalogues(los):
    a, b = sets()
    counts, prm = c_abi_cross(a, b, RP, PI, L, los, plan=0)
    npt.assert_array_equal(counts, ref("ab", los))
    assert prm["dims"].tolist() == permuted(12, 3, los) and prm["ncells"] == 432
    npt.assert_array_equal(prm["inv_cs"], np.array(permuted(12, 3, los)) / L)
    counts, prm = c_abi_cross(a, b, RP, PI, L, los, plan=1)
    npt.assert_array_equal(counts, ref("ab", los))
    assert prm["dims"].tolist() == [3, 3, 3]
    counts, prm = c_abi_cross(a, b, RP, PI, L, los, plan=0, single=1)
    npt.assert_array_equal(counts, ref("ab", los))
    assert prm["dims"].tolist() == [1, 1, 1]
    # open boundaries: the extent of 3000 + 2000 uniform points is just below L on every axis
    counts, prm = c_abi_cross(a, b, RP, PI, 0.0, los, plan=0)
    npt.assert_array_equal(counts, ref("ab", los, False))
    assert prm["dims"].tolist() == permuted(12, 3, los)
    counts, prm = c_abi_cross(a, b, RP, PI, 0.0, los, plan=1)
    npt.assert_array_equal(counts, ref("ab", los, False))
    assert prm["dims"].tolist() == [3, 3, 3]


def test_plan_argument_is_checked():
    from astrild_amd import _lib
    a, b = sets()
    with pytest.raises(_lib.AstrildHipError):
        c_abi_cross(a[:10], b[:10], RP, PI, L, 2, plan=2)


# ---------------------------------------------------------------- 3. an axis with one cell
@pytest.mark.parametrize("los", [0, 1, 2])
def test_an_axis_with_one_cell(los):
    a, b = sets()
    a, b = a[:1500], b[:1000]
    # floor(L / pi_max) = 2 along the line of sight: one cell there, the minimum image finds the pairs
    pi = np.array([0.0, 5.0, 20.0, 33.33333])
    exp = orc.rppi_cross_brute(a, b, RP, pi, los, L)
    counts, prm = c_abi_cross(a, b, RP, pi, L, los, plan=0)
    assert prm["dims"].tolist() == permuted(12, 1, los)
    npt.assert_array_equal(counts, exp)
    npt.assert_array_equal(gpu_cross(a, b, RP, pi, boxsize=L, los=los), exp)
    npt.assert_array_equal(gpu_auto(a, L, RP, pi, los=los), orc.rppi_auto_brute(a, RP, pi, los, L))
    # r_p,max just below L / 3 with a small pi_max: one cell on both axes across
    rp, pi = np.array([0.0, 10.0, 25.0, 33.33333]), np.array([0.0, 1.0, 2.5, 4.0])
    exp = orc.rppi_cross_brute(a, b, rp, pi, los, L)
    counts, prm = c_abi_cross(a, b, rp, pi, L, los, plan=0)
    assert prm["dims"].tolist() == permuted(1, 24, los)
    npt.assert_array_equal(counts, exp)
    npt.assert_array_equal(gpu_auto(a, L, rp, pi, los=los), orc.rppi_auto_brute(a, rp, pi, los, L))


# ---------------------------------------------------------------- 4. crowded cell
CROWD_RP = np.array([0.0, 1.0, 3.0, 7.0, 15.0])
CROWD_PI = np.array([0.0, 2.0, 5.0, 10.0, 20.0, 33.0])


@pytest.fixture(scope="module")
def crowded():
    # 2 x (256 + 256 + 188) objects within one cell's width: several i tiles against several j stages, ragged tails
    rng = np.random.default_rng(21)
    a = np.concatenate([rng.uniform(45.0, 55.0, (600, 3)), rng.uniform(0.0, 100.0, (300, 3))])
    b = np.concatenate([rng.uniform(45.0, 55.0, (700, 3)), rng.uniform(0.0, 100.0, (200, 3))])
    return a, b


@pytest.mark.parametrize("flush", [None, "1000"])
@pytest.mark.parametrize("planner", list(PLANNERS))
def test_tiles_and_stages_in_a_crowded_cell(crowded, planner, flush, monkeypatch):
    use(monkeypatch, planner)
    if flush is not None:
        monkeypatch.setenv("AST_TPCF_FLUSH_AT", flush)
    a, b = crowded
    exp = orc.rppi_cross_brute(a, b, CROWD_RP, CROWD_PI, 2, L)
    assert exp.sum() > 300_000
    npt.assert_array_equal(gpu_cross(a, b, CROWD_RP, CROWD_PI, boxsize=L), exp)
    npt.assert_array_equal(gpu_cross(a, b, CROWD_RP, CROWD_PI), orc.rppi_cross_brute(a, b, CROWD_RP, CROWD_PI, 2, None))
    npt.assert_array_equal(gpu_auto(b, L, CROWD_RP, CROWD_PI, los=0), orc.rppi_auto_brute(b, CROWD_RP, CROWD_PI, 0, L))


@pytest.mark.parametrize("flush", [None, "1000"])
def test_one_lds_copy_with_100_x_100_bins(crowded, flush, monkeypatch):
    if flush is not None:
        monkeypatch.setenv("AST_TPCF_FLUSH_AT", flush)
    a, b = crowded
    rp, pi = np.linspace(0.0, 33.0, 101), np.linspace(0.0, 33.0, 101)
    npt.assert_array_equal(gpu_cross(a, b, rp, pi, boxsize=L), orc.rppi_cross_brute(a, b, rp, pi, 2, L))
    npt.assert_array_equal(gpu_cross(a, b, rp, pi, los=0), orc.rppi_cross_brute(a, b, rp, pi, 0, None))
    npt.assert_array_equal(gpu_cross(a, None, rp, pi), orc.rppi_auto_brute(a, rp, pi, 2, None))


# ---------------------------------------------------------------- 5. faces, edges and corners of the periodic box
FACE_BOX = 10.0
FACE_RP = np.array([0.0, 0.5, 1.0, 1.5])
FACE_PI = np.array([0.0, 1.0, 2.0, 3.0])


@pytest.fixture(scope="module")
def near_faces():
    """Both sets within one reach of the faces of a box of 10, on a coordinate grid of 1 / 64: image shifts and
    separations are exact, so the periodic count is the open count of set 1 against the 27 images of set 2."""
    rng = np.random.default_rng(31)

    def draw(n):
        p = rng.integers(0, 641, (8 * n, 3)) / 64.0
        return p[np.any((p < 3.0) | (p > FACE_BOX - 3.0), axis=1)][:n]

    a, b = draw(400), draw(500)
    a[0], b[0] = [0.0, FACE_BOX, FACE_BOX], [FACE_BOX, 0.0, 0.0]      # on the faces themselves
    assert len(a) == 400 and len(b) == 500
    images = np.concatenate([b + FACE_BOX * np.array(o) for o in itertools.product((-1.0, 0.0, 1.0), repeat=3)])
    exp = [orc.rppi_cross_brute(a, images, FACE_RP, FACE_PI, los) for los in (0, 1, 2)]
    return a, b, images, exp


@pytest.mark.parametrize("planner", list(PLANNERS))
def test_faces_edges_and_corners(near_faces, planner, monkeypatch):
    use(monkeypatch, planner)
    a, b, images, exp = near_faces
    for los in (0, 1, 2):
        got = gpu_cross(a, b, FACE_RP, FACE_PI, boxsize=FACE_BOX, los=los)
        npt.assert_array_equal(got, exp[los])
        npt.assert_array_equal(gpu_cross(a, images, FACE_RP, FACE_PI, los=los), exp[los])
        opn = gpu_cross(a, b, FACE_RP, FACE_PI, los=los)
        npt.assert_array_equal(opn, orc.rppi_cross_brute(a, b, FACE_RP, FACE_PI, los))
        assert (got - opn).sum() > 500                                # pairs across the faces are there


def test_faces_grid_is_anisotropic(near_faces):
    a, b, _, exp = near_faces
    for los in (0, 1, 2):
        counts, prm = c_abi_cross(a, b, FACE_RP, FACE_PI, FACE_BOX, los, plan=0)
        assert prm["dims"].tolist() == permuted(6, 3, los)
        npt.assert_array_equal(counts, exp[los])


# ---------------------------------------------------------------- 6. degenerate sets
@pytest.mark.parametrize("planner", list(PLANNERS))
def test_degenerate_sets(planner, monkeypatch):
    use(monkeypatch, planner)
    a, b = sets()
    a, b = a[:800], b[:600]
    none = np.zeros((0, 3))
    for box in (L, None):
        for n in (0, 1):
            assert not gpu_cross(a[:n], None, boxsize=box).any()
            assert not gpu_cross(none, a[:n], boxsize=box).any()
        assert not gpu_cross(a, none, boxsize=box).any()
        npt.assert_array_equal(gpu_cross(a[:1], b, boxsize=box), orc.rppi_cross_brute(a[:1], b, RP, PI, 2, box))
    assert not gpu_auto(a[:1], L).any() and not gpu_auto(none, L).any()
    for los in (0, 1, 2):
        plane_a, plane_b = a.copy(), b.copy()
        plane_a[:, los] = plane_b[:, los] = 37.5                      # every pi = 0: in no bin, the lowest edge is 0
        line_a, line_b = a.copy(), b.copy()
        for ax in set(range(3)) - {los}:
            line_a[:, ax] = line_b[:, ax] = 12.25                     # every r_p = 0, and RP starts above 0 anyway
        rp0 = np.concatenate([[0.0], RP])
        for box in (L, None):
            assert not gpu_cross(plane_a, plane_b, boxsize=box, los=los).any()
            assert not gpu_cross(plane_a, None, boxsize=box, los=los).any()
            assert not gpu_cross(line_a, line_b, rp0, PI, boxsize=box, los=los).any()
            assert not gpu_cross(line_a, None, rp0, PI, boxsize=box, los=los).any()
            # thin, not flat, along the line of sight: the pairs are back, in the lowest pi bin
            thin = plane_a + np.where(np.arange(3) == los, 1.0, 0.0) * np.linspace(0.0, 2.0, len(a))[:, None]
            npt.assert_array_equal(gpu_cross(thin, None, boxsize=box, los=los),
                                   orc.rppi_auto_brute(thin, RP, PI, los, box))
    far_a, far_b = a + 1.0e6, b + 1.0e6                               # open coordinates offset by 10^6
    exp = orc.rppi_cross_brute(far_a, far_b, RP, PI, 2, None)
    assert exp.sum() > 4000
    npt.assert_array_equal(gpu_cross(far_a, far_b), exp)
    npt.assert_array_equal(gpu_cross(far_a, None, los=1), orc.rppi_auto_brute(far_a, RP, PI, 1, None))


def test_coincident_points_never_count():
    a, _ = sets()
    a = a[:500]
    rp0, pi0 = np.array([0.0, 2.0, 8.0]), np.array([0.0, 10.0, 30.0])
    exp = orc.rppi_auto_brute(a, rp0, pi0, 2, L)
    npt.assert_array_equal(gpu_cross(a, a, rp0, pi0, boxsize=L), 2 * exp)       # the 500 self pairs are in no bin
    twice = np.concatenate([a, a])
    npt.assert_array_equal(gpu_auto(twice, L, rp0, pi0), 4 * exp)               # nor are the 500 coincident pairs


# ---------------------------------------------------------------- 7. ties to independent kernels
def test_against_the_pairwise_velocity_kernel_and_the_s_counts():
    from astrild_amd import device as dev
    a, b = sets()
    vel = np.zeros_like(a)
    for pi_max, box in ((30.0, L), (12.5, L), (30.0, None)):
        moments = dev.pair_velocity_moments(a, vel, RP, boxsize=box, kind="los", pi_max=pi_max)
        got = gpu_cross(a, None, RP, np.array([0.0, pi_max]), boxsize=box)
        assert got.sum() > 10_000
        npt.assert_array_equal(got.sum(axis=1), dev.to_numpy(moments[0]))
    moments = dev.pair_velocity_moments(a, vel, RP, pos2=b, vel2=np.zeros_like(b), boxsize=L, kind="los", pi_max=30.0,
                                        los=0)
    npt.assert_array_equal(gpu_cross(a, b, RP, np.array([0.0, 30.0]), boxsize=L, los=0).sum(axis=1),
                           dev.to_numpy(moments[0]))
    # the sphere s <= R lies inside the cylinder r_p <= R, pi <= R
    R = 20.0
    edges = np.linspace(0.0, R, 6)
    sphere = dev.to_numpy(dev.tpcf_pair_counts(a, L, np.array([0.0, R]))).sum()
    cylinder = gpu_auto(a, L, edges, edges).sum()
    assert cylinder >= sphere > 10_000
    # and holds 3 / 2 of its volume: the counts of a uniform set follow within a few per cent
    assert abs(cylinder / sphere - 1.5) < 0.05


# ---------------------------------------------------------------- 8. jackknife
JK_RP = np.geomspace(0.5, 8.0, 5)
JK_PI = np.linspace(0.0, 30.0, 7)


@pytest.mark.parametrize("lds", ["1", "0"], ids=["lds", "global"])
@pytest.mark.parametrize("nsub", [(2, 2, 2), (3, 1, 2)])
@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
def test_jackknife_counts(periodic, nsub, lds, monkeypatch):
    from astrild_amd import device as dev
    monkeypatch.setenv("ASTRILD_TPCF_JK_LDS", lds)
    a, b = sets()
    a, b = a[:1200], b[:900]
    box = L if periodic else None
    ntot = int(np.prod(nsub))
    for pos2, los in ((b, 2), (None, 0)):
        # the regions: over the periodic box, else over the bounding box of the samples given (the default extents)
        given = [a] if pos2 is None else [a, b]
        lo, hi = (np.zeros(3), np.full(3, L)) if periodic else (np.min([p.min(0) for p in given], axis=0),
                                                                np.max([p.max(0) for p in given], axis=0))
        counts, ends = dev.rp_pi_jackknife_counts(a, nsub, JK_RP, JK_PI, pos2=pos2, boxsize=box, los=los)
        assert counts.dtype == torch.int64 and ends.dtype == torch.int64
        counts, ends = dev.to_numpy(counts), dev.to_numpy(ends)
        assert counts.shape == (4, 6) and ends.shape == (ntot, 4, 6)
        ta = jorc.region_tags(a, nsub, lo, hi)
        tb = None if pos2 is None else jorc.region_tags(b, nsub, lo, hi)
        exp, w2 = orc.jackknife_brute(a, ta, pos2, tb, ntot, JK_RP, JK_PI, los, box)
        assert exp.sum() > 5000
        npt.assert_array_equal(counts, exp)
        npt.assert_array_equal(ends.sum(axis=0), 2 * counts)
        npt.assert_array_equal(2 * counts[None] - ends, w2)
        npt.assert_array_equal(counts, gpu_cross(a, pos2, JK_RP, JK_PI, boxsize=box, los=los))


def test_jackknife_with_explicit_tags_and_the_isotropic_plan(monkeypatch):
    from astrild_amd import device as dev
    monkeypatch.setenv("ASTRILD_RPPI_ANISO", "0")
    a, b = sets()
    a, b = a[:700], b[:500]
    rng = np.random.default_rng(75)
    ta, tb = rng.integers(0, 5, len(a)), rng.integers(0, 5, len(b))
    counts, ends = (dev.to_numpy(x) for x in dev.rp_pi_jackknife_counts(a, 5, JK_RP, JK_PI, pos2=b, boxsize=L, tags1=ta,
                                                                        tags2=tb))
    exp, w2 = orc.jackknife_brute(a, ta, b, tb, 5, JK_RP, JK_PI, 2, L)
    npt.assert_array_equal(counts, exp)
    npt.assert_array_equal(2 * counts[None] - ends, w2)


# ---------------------------------------------------------------- 9. estimators and the API
EST_RP = np.array([1.0, 4.0, 8.0, 12.0])
EST_PI = np.array([0.0, 10.0, 20.0, 30.0])


@functools.lru_cache(maxsize=None)
def est_sets():
    d1, d2 = sorc.clustered(1500, L, 81, blobs=20, sigma=4.0), sorc.clustered(1200, L, 82, blobs=20, sigma=4.0)
    return d1, d2, sorc.uniform(3000, L, 83)


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
@pytest.mark.parametrize("name", xorc.ESTIMATORS)
def test_estimators_with_user_randoms(name, periodic):
    from astrild_amd.particles.hutils import rp_pi_tpcf, wp
    d1, d2, r = est_sets()
    period = L if periodic else None
    (x11, x12, x22), c = rp_pi_tpcf(d1, EST_RP, EST_PI, sample2=d2, randoms=r, period=period, estimator=name,
                                    return_counts=True)
    f = lambda key: None if key not in c else c[key].astype(np.float64)
    two = lambda key: None if key not in c else 2.0 * c[key].astype(np.float64)
    assert all(v.dtype == np.int64 and v.shape == (3, 3) for v in c.values())
    npt.assert_array_equal(c["D1D2"], orc.rppi_cross_brute(d1, d2, EST_RP, EST_PI, 2, period))
    n1, n2, nr = len(d1), len(d2), len(r)
    npt.assert_allclose(x11, xorc.estimator(name, two("D1D1"), f("D1R"), two("RR"), n1, n1, nr), rtol=1e-12)
    npt.assert_allclose(x12, xorc.estimator(name, f("D1D2"), f("D1R"), two("RR"), n1, n2, nr), rtol=1e-12)
    npt.assert_allclose(x22, xorc.estimator(name, two("D2D2"), f("D2R"), two("RR"), n2, n2, nr), rtol=1e-12)
    assert np.isfinite(x11).all() and x11.max() > 0.5               # a clustered sample against uniform randoms
    w = wp(d1, EST_RP, 30.0, sample2=d2, randoms=r, period=period, estimator=name, pi_bins=EST_PI)
    for got, xi in zip(w, (x11, x12, x22)):
        npt.assert_allclose(got, orc.wp_from_xi(xi, EST_PI), rtol=1e-12)


def test_analytic_randoms_and_the_return_shapes():
    from astrild_amd.particles.hutils import rp_pi_tpcf, wp, wp_from_xi
    d1, d2, _ = est_sets()
    n1, n2 = len(d1), len(d2)
    xi, dd = rp_pi_tpcf(d1, EST_RP, EST_PI, period=L, return_counts=True)
    npt.assert_array_equal(dd["D1D1"], orc.rppi_auto_brute(d1, EST_RP, EST_PI, 2, L))
    npt.assert_allclose(xi, orc.analytic_xi(2.0 * dd["D1D1"], n1, n1, L, EST_RP, EST_PI), rtol=1e-12)
    for name in xorc.ESTIMATORS:                                    # every name reduces to DD / RR - 1
        npt.assert_array_equal(rp_pi_tpcf(d1, EST_RP, EST_PI, period=L, estimator=name), xi)
    (x11, x12, x22), c = rp_pi_tpcf(d1, EST_RP, EST_PI, sample2=d2, period=L, return_counts=True)
    assert sorted(c) == ["D1D1", "D1D2", "D2D2"]
    npt.assert_array_equal(x11, xi)
    npt.assert_allclose(x12, orc.analytic_xi(c["D1D2"], n1, n2, L, EST_RP, EST_PI), rtol=1e-12)
    npt.assert_allclose(x22, orc.analytic_xi(2.0 * c["D2D2"], n2, n2, L, EST_RP, EST_PI), rtol=1e-12)
    only_cross = rp_pi_tpcf(d1, EST_RP, EST_PI, sample2=d2, period=L, do_auto=False)
    npt.assert_array_equal(only_cross, x12)
    only_auto = rp_pi_tpcf(d1, EST_RP, EST_PI, sample2=d2, period=L, do_cross=False)
    assert isinstance(only_auto, tuple) and len(only_auto) == 2
    npt.assert_array_equal(only_auto[0], x11)
    npt.assert_array_equal(only_auto[1], x22)
    for los in (0, 1):
        got = rp_pi_tpcf(d1, EST_RP, EST_PI, period=L, los=los)
        npt.assert_allclose(got, orc.analytic_xi(2.0 * orc.rppi_auto_brute(d1, EST_RP, EST_PI, los, L), n1, n1, L, EST_RP,
                                                 EST_PI), rtol=1e-12)
    # wp: halotools' single bin by default, and the sum over finer bins
    single = rp_pi_tpcf(d1, EST_RP, [0.0, 30.0], period=L)
    assert single.shape == (3, 1)
    npt.assert_array_equal(wp(d1, EST_RP, 30.0, period=L), wp_from_xi(single, [0.0, 30.0]))
    npt.assert_array_equal(wp(d1, EST_RP, 30.0, period=L, pi_bins=EST_PI), wp_from_xi(xi, EST_PI))
    w3 = wp(d1, EST_RP, 30.0, sample2=d2, period=L, pi_bins=EST_PI)
    assert isinstance(w3, tuple) and len(w3) == 3 and all(w.shape == (3,) for w in w3)
    npt.assert_array_equal(w3[1], wp_from_xi(x12, EST_PI))
    w, c = wp(d1, EST_RP, 30.0, period=L, return_counts=True, num_threads=4)
    assert w.shape == (3,) and c["D1D1"].shape == (3, 1)


@pytest.mark.parametrize("name", ["Natural", "Landy-Szalay"])
def test_jackknife_api(name):
    from astrild_amd.particles.hutils import rp_pi_tpcf, rp_pi_tpcf_jackknife, wp, wp_jackknife
    d1, d2, r = est_sets()
    nsub = [2, 2, 2]
    out = rp_pi_tpcf_jackknife(d1, r, EST_RP, EST_PI, Nsub=nsub, sample2=d2, period=L, estimator=name,
                               return_counts=True, num_threads=2, seed=1)
    x11, x12, x22, c11, c12, c22, c = out
    full = rp_pi_tpcf(d1, EST_RP, EST_PI, sample2=d2, randoms=r, period=L, estimator=name)
    for got, exp in zip((x11, x12, x22), full):
        assert got.shape == (3, 3)
        npt.assert_array_equal(got, exp)
    # the covariance from the oracle's weighted counts
    lo, hi = np.zeros(3), np.full(3, L)
    tags = {k: jorc.region_tags(p, nsub, lo, hi) for k, p in (("1", d1), ("2", d2), ("R", r))}
    pos = {"1": d1, "2": d2, "R": r}
    w2, counts = {}, {}
    for key, (p, q) in (("D1D1", ("1", None)), ("D1D2", ("1", "2")), ("D2D2", ("2", None)), ("D1R", ("1", "R")),
                        ("D2R", ("2", "R")), ("RR", ("R", None))):
        if key not in c:
            continue
        counts[key], w2[key] = orc.jackknife_brute(pos[p], tags[p], None if q is None else pos[q],
                                                   None if q is None else tags[q], 8, EST_RP, EST_PI, 2, L)
        npt.assert_array_equal(c[key][0], counts[key])
    sizes = {k: len(p) for k, p in pos.items()}
    occupancy = {k: np.bincount(t, minlength=8) for k, t in tags.items()}
    for (p, q), xi, cov in ((("1", "1"), x11, c11), (("1", "2"), x12, c12), (("2", "2"), x22, c22)):
        exp_xi, exp_cov, _ = jorc.xi_and_cov(name, w2, counts, sizes, occupancy, p, q)
        npt.assert_allclose(xi, exp_xi, rtol=1e-12)
        assert cov.shape == (9, 9) and np.isfinite(exp_cov).all()
        # both sum the same 8 fp64 products per element in another order (np.cov against d.T @ d): a few ulps of the
        # largest element per term, 20 x 8 x 2^-52 of max|cov| in all
        assert np.abs(cov - exp_cov).max() <= 160 * 2.0 ** -52 * np.abs(exp_cov).max()
    # w_p: the full-sample value, and the covariance A cov_xi A^T
    w11, w12, w22, v11, v12, v22 = wp_jackknife(d1, r, EST_RP, 30.0, Nsub=nsub, sample2=d2, period=L, estimator=name,
                                                pi_bins=EST_PI)
    for got, exp in zip((w11, w12, w22), wp(d1, EST_RP, 30.0, sample2=d2, randoms=r, period=L, estimator=name,
                                            pi_bins=EST_PI)):
        npt.assert_array_equal(got, exp)
    A = orc.wp_matrix(3, EST_PI)
    for got, cov in ((v11, c11), (v12, c12), (v22, c22)):
        assert got.shape == (3, 3)
        npt.assert_allclose(got, A @ cov @ A.T, rtol=1e-10)
    # one sample, the default single pi bin
    w, v = wp_jackknife(d1, r, EST_RP, 30.0, Nsub=nsub, period=L, estimator=name)
    xi1, cov1 = rp_pi_tpcf_jackknife(d1, r, EST_RP, [0.0, 30.0], Nsub=nsub, period=L, estimator=name)
    npt.assert_allclose(w, 60.0 * xi1[:, 0], rtol=1e-15)
    npt.assert_allclose(v, 3600.0 * cov1, rtol=1e-10)


def test_value_errors_before_any_pair_work(monkeypatch):
    from astrild_amd import _lib
    from astrild_amd import device as dev
    from astrild_amd.particles.hutils import rp_pi_tpcf, wp
    lib = _lib.lib()
    a, b = sets()
    a, b = a[:50].copy(), b[:40].copy()

    class Spy:
        """The library without its pair counts: a check that lets one through fails the test."""
        def __getattr__(self, name):
            if name.endswith("_counts"):
                raise AssertionError(f"{name} was called")
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    outside, nan = a.copy(), a.copy()
    outside[7, 1], nan[3, 2] = L + 0.5, np.nan
    for call in (lambda: dev.rp_pi_cross_counts(outside, b, RP, PI, boxsize=L),
                 lambda: dev.rp_pi_cross_counts(b, outside, RP, PI, boxsize=L),
                 lambda: dev.rp_pi_pair_counts(outside, L, RP, PI),
                 lambda: dev.rp_pi_cross_counts(nan, b, RP, PI),
                 lambda: dev.rp_pi_jackknife_counts(nan, 2, RP, PI, pos2=b, boxsize=L),
                 lambda: dev.rp_pi_jackknife_counts(a, 2, RP, PI, boxsize=L, tags1=np.full(len(a), 2)),
                 lambda: dev.rp_pi_pair_counts(a, L, RP, PI, los=3),
                 lambda: dev.rp_pi_cross_counts(a, b, RP, PI, boxsize=L, los=-1),
                 lambda: dev.rp_pi_cross_counts(a, None, RP, PI, boxsize=L, vel2=np.zeros_like(a)),
                 lambda: dev.rp_pi_pair_counts(a[:, :2], L, RP, PI),
                 lambda: dev.rp_pi_pair_counts(a, L, RP, PI, vel=np.zeros((len(a), 2))),
                 lambda: dev.rp_pi_pair_counts(a, L, RP, [0.0, 34.0]),
                 lambda: dev.rp_pi_pair_counts(a, L, RP[::-1], PI),
                 lambda: dev.rp_pi_jackknife_counts(a, (2, 2), RP, PI, boxsize=L),
                 lambda: rp_pi_tpcf(a, RP, PI, period=None),
                 lambda: rp_pi_tpcf(outside, RP, PI, period=L),
                 lambda: wp(a, RP, 30.0, period=L, pi_bins=[0.0, 29.0]),
                 lambda: wp(a, RP, 30.0, period=L, estimator="Peebles")):
        with pytest.raises(ValueError):
            call()
    # a velocity shift that one wrap does not bring back into the box
    vel = np.zeros_like(a)
    vel[0, 2] = 3.0e4
    with pytest.raises(ValueError):
        dev.rp_pi_pair_counts(a, L, RP, PI, vel=vel)


# ---------------------------------------------------------------- 10. dirty workspace and call order
def test_dirty_scratch_memory(dirty_alloc):
    from astrild_amd import device as dev
    a, b = sets()
    a, b = a[:1200], b[:900]
    exp_x, exp_a = orc.rppi_cross_brute(a, b, RP, PI, 2, L), orc.rppi_auto_brute(a, RP, PI, 2, L)
    ta, tb = jorc.region_tags(a, (2, 2, 2), np.zeros(3), np.full(3, L)), jorc.region_tags(b, (2, 2, 2), np.zeros(3),
                                                                                          np.full(3, L))
    exp_j, w2 = orc.jackknife_brute(a, ta, b, tb, 8, JK_RP, JK_PI, 2, L)

    def run():
        mark = dirty_alloc.mark()
        auto = dev.to_numpy(dev.rp_pi_pair_counts(a, L, RP, PI))
        cross = dev.to_numpy(dev.rp_pi_cross_counts(a, b, RP, PI, boxsize=L))
        opn = dev.to_numpy(dev.rp_pi_cross_counts(a, b, RP, PI))
        counts, ends = (dev.to_numpy(x) for x in dev.rp_pi_jackknife_counts(a, (2, 2, 2), JK_RP, JK_PI, pos2=b,
                                                                           boxsize=L))
        assert dirty_alloc.since(mark) >= 12                        # workspaces, bounds and outputs were poisoned
        return auto, cross, opn, counts, ends

    auto, cross, opn, counts, ends = run()
    npt.assert_array_equal(auto, exp_a)
    npt.assert_array_equal(cross, exp_x)
    npt.assert_array_equal(opn, orc.rppi_cross_brute(a, b, RP, PI, 2, None))
    npt.assert_array_equal(counts, exp_j)
    npt.assert_array_equal(2 * counts[None] - ends, w2)
    with dirty_alloc.using(ZERO_BYTES):
        for got, dirty in zip(run(), (auto, cross, opn, counts, ends)):
            npt.assert_array_equal(got, dirty)


def test_call_order_after_an_s_mu_count_of_the_same_size(dirty_alloc):
    from astrild_amd import device as dev
    a, b = sets()
    a, b = a[:1200], b[:900]
    s, mu = np.linspace(0.0, 30.0, len(RP)), np.linspace(0.0, 1.0, len(PI))     # (8, 15) bins: the same workspace size
    exp = orc.rppi_cross_brute(a, b, RP, PI, 2, L)
    exp_smu = xorc.cross_counts_brute(a, b, s, mu, boxsize=L)
    smu = lambda: dev.to_numpy(dev.tpcf_cross_counts(a, b, s, mu_edges=mu, boxsize=L))
    rppi = lambda: dev.to_numpy(dev.rp_pi_cross_counts(a, b, RP, PI, boxsize=L))
    for order in ((smu, rppi, smu, rppi), (rppi, rppi, smu, smu)):
        for call in order:
            npt.assert_array_equal(call(), exp if call is rppi else exp_smu)
    jk_smu = lambda: dev.tpcf_jackknife_counts(a, (2, 2, 2), s, mu, pos2=b, boxsize=L)
    jk_rppi = lambda: dev.rp_pi_jackknife_counts(a, (2, 2, 2), RP, PI, pos2=b, boxsize=L)
    first = [dev.to_numpy(x) for x in jk_rppi()]
    jk_smu()
    npt.assert_array_equal(dev.to_numpy(dev.tpcf_pair_counts(a, L, s, mu_edges=mu)),
                           sorc.pair_counts_brute(a, L, s, mu))
    npt.assert_array_equal(dev.to_numpy(dev.rp_pi_pair_counts(a, L, RP, PI)), orc.rppi_auto_brute(a, RP, PI, 2, L))
    for got, exp_k in zip(jk_rppi(), first):
        npt.assert_array_equal(dev.to_numpy(got), exp_k)
    npt.assert_array_equal(first[0], exp)
