"""GPU: the two-sample pair counts of the two-point correlation function (ast_tpcf_cross_prepare /
ast_tpcf_cross_counts through device.tpcf_cross_counts) and what tpcf_r / s_mu_tpcf / TPCF build on them: a
parity-split lattice with known answers, int64 counts exactly equal to the numpy oracle (tests/tpcf_cross_oracle.py)
in a periodic cube and with open boundaries, ties to the one-sample kernel, pairs across faces, edges and corners, the
edge cases of the open grid, the redshift-space shift per sample, the five estimators with user randoms term by term,
the argument checks, dirty scratch memory and the order of calls."""
import itertools

import numpy as np
import numpy.testing as npt
import pytest

from tests import tpcf_cross_oracle as xorc
from tests import tpcf_oracle as orc
from tests.dirty_memory import dirty_alloc                        # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LAT_S = [0.5, 1.2, 1.6, 1.9, 2.1, 2.5]
LAT_MU = [0.0, 0.25, 0.6, 0.8, 1.0]
L = 500.0
S50 = np.linspace(0.0, 50.0, 40)
MU40 = np.sort(1.0 - np.geomspace(0.001, 1.0, 40))
CROWD_S = [0, 1, 3, 7, 15, 33]


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


def gpu_cross(a, b, s_edges, mu_edges=None, boxsize=None, vel1=None, vel2=None, los=2):
    from astrild_amd import device as dev
    return dev.to_numpy(dev.tpcf_cross_counts(a, b, s_edges, mu_edges=mu_edges, boxsize=boxsize, vel1=vel1, vel2=vel2,
                                              los=los))


def gpu_auto(pos, boxsize, s_edges, mu_edges=None, vel=None, los=2):
    """The one-sample kernel of the parent (device.tpcf_pair_counts)."""
    from astrild_amd import device as dev
    return dev.to_numpy(dev.tpcf_pair_counts(pos, boxsize, s_edges, mu_edges=mu_edges, vel=vel, los=los))


@pytest.fixture(scope="module")
def catalogues():
    a = orc.clustered(5000, L, 11, blobs=60, sigma=6.0)
    b = orc.clustered(7000, L, 12, blobs=60, sigma=6.0)
    ref = {"periodic": xorc.cross_counts(a, b, S50, MU40, boxsize=L), "open": xorc.cross_counts(a, b, S50, MU40)}
    assert ref["periodic"].sum() == 150_719 and ref["open"].sum() == 139_353
    for r in ref.values():
        r.setflags(write=False)
    return a, b, ref


@pytest.fixture(scope="module")
def crowded():
    rng = np.random.default_rng(21)
    a = np.concatenate([rng.uniform(45.0, 55.0, (600, 3)), rng.uniform(0.0, 100.0, (300, 3))])
    b = np.concatenate([rng.uniform(45.0, 55.0, (700, 3)), rng.uniform(0.0, 100.0, (200, 3))])
    return a, b


# ---------------------------------------------------------------- known answers and the oracle
@pytest.mark.parametrize("cells", ["1", "0"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("los", [0, 1, 2])
def test_parity_lattice(los, dtype, cells, monkeypatch):
    monkeypatch.setenv("ASTRILD_TPCF_CELLS", cells)
    even, odd = xorc.parity_lattice(8)
    exp = xorc.parity_lattice_expected(8, LAT_S, LAT_MU, los)
    got = gpu_cross(even.astype(dtype), odd.astype(dtype), LAT_S, LAT_MU, boxsize=8.0, los=los)
    npt.assert_array_equal(got, exp)
    assert got[[0, 2, 4]].tolist() == [[0, 0, 0, 512], [0, 2048, 0, 0], [0, 2048, 0, 2048]] and not got[[1, 3]].any()


@pytest.mark.parametrize("mode", ["periodic", "open"])
def test_catalogues_equal_the_oracle(catalogues, mode):
    a, b, ref = catalogues
    box = L if mode == "periodic" else None
    got = gpu_cross(a, b, S50, MU40, boxsize=box)
    npt.assert_array_equal(got, ref[mode])
    assert got.dtype == np.int64 and got.shape == (39, 39)
    if mode == "periodic":
        assert np.all(got >= ref["open"])
    real = gpu_cross(a, b, S50, boxsize=box)
    assert real.shape == (39,)
    npt.assert_array_equal(real, xorc.cross_counts(a, b, S50, boxsize=box))


@pytest.mark.parametrize("mode", ["periodic", "open"])
def test_mixed_dtypes_and_swapped_sets(catalogues, mode):
    a, b, ref = catalogues
    box = L if mode == "periodic" else None
    a32 = a.astype(np.float32)
    exp = xorc.cross_counts(a32.astype(np.float64), b, S50, MU40, boxsize=box)
    npt.assert_array_equal(gpu_cross(a32, b, S50, MU40, boxsize=box), exp)
    npt.assert_array_equal(gpu_cross(b, a32, S50, MU40, boxsize=box), exp)
    npt.assert_array_equal(gpu_cross(b, a, S50, MU40, boxsize=box), ref[mode])
    npt.assert_array_equal(gpu_cross(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), S50, MU40, boxsize=box),
                           ref[mode])


@pytest.mark.parametrize("flush", [None, "1000"])
@pytest.mark.parametrize("cells", ["1", "0"])
def test_tiles_and_stages_in_a_crowded_cell(crowded, cells, flush, monkeypatch):
    # 600 + and 700 + objects in the middle cell of the 3-cell grid: three i tiles against three j stages, the last of
    # each partly filled
    monkeypatch.setenv("ASTRILD_TPCF_CELLS", cells)
    if flush is not None:
        monkeypatch.setenv("AST_TPCF_FLUSH_AT", flush)
    a, b = crowded
    got = gpu_cross(a, b, CROWD_S, boxsize=100.0)
    assert got.tolist() == [1537, 31336, 198712, 194352, 55184]
    npt.assert_array_equal(got, xorc.cross_counts_brute(a, b, CROWD_S, boxsize=100.0))
    npt.assert_array_equal(gpu_cross(a, b, CROWD_S), xorc.cross_counts_brute(a, b, CROWD_S))
    npt.assert_array_equal(gpu_cross(a, None, CROWD_S), xorc.auto_counts_open_brute(a, CROWD_S))
    npt.assert_array_equal(gpu_cross(b, None, CROWD_S, MU40, boxsize=100.0),
                           orc.pair_counts_brute(b, 100.0, CROWD_S, MU40))


@pytest.mark.parametrize("flush", [None, "1000"])
def test_one_lds_copy_with_100_x_100_bins(crowded, flush, monkeypatch):
    if flush is not None:
        monkeypatch.setenv("AST_TPCF_FLUSH_AT", flush)
    a, b = crowded
    s, mu = np.linspace(0.0, 33.0, 101), np.linspace(0.0, 1.0, 101)
    npt.assert_array_equal(gpu_cross(a, b, s, mu, boxsize=100.0), xorc.cross_counts_brute(a, b, s, mu, boxsize=100.0))
    npt.assert_array_equal(gpu_cross(a, b, s, mu, los=0), xorc.cross_counts_brute(a, b, s, mu, los=0))
    npt.assert_array_equal(gpu_cross(a, None, s, mu), xorc.auto_counts_open_brute(a, s, mu))


# ---------------------------------------------------------------- ties to the one-sample kernel
def test_cross_with_itself_is_twice_the_pair_counts(catalogues):
    a, _, _ = catalogues
    auto = gpu_auto(a, L, S50, MU40)
    npt.assert_array_equal(gpu_cross(a, a, S50, MU40, boxsize=L), 2 * auto)
    npt.assert_array_equal(gpu_cross(a, None, S50, MU40, boxsize=L), auto)
    assert auto.sum() > 10_000


def test_open_auto_of_an_inner_set_equals_its_periodic_counts(catalogues):
    _, b, _ = catalogues
    inner = b[np.all((b > 50.0) & (b < L - 50.0), axis=1)]           # further than smax from every face
    assert len(inner) > 3000
    for los in (0, 2):
        npt.assert_array_equal(gpu_cross(inner, None, S50, MU40, los=los), gpu_auto(inner, L, S50, MU40, los=los))
    npt.assert_array_equal(gpu_cross(inner, None, S50), gpu_auto(inner, L, S50))


FACE_BOX = 10.0
FACE_S = np.array([0.0, 0.5, 1.0, 2.0, 3.0])
FACE_MU = np.array([0.0, 0.3, 0.7, 1.0])


@pytest.fixture(scope="module")
def near_faces():
    """Both sets within smax of the faces of a box of 10, on a coordinate grid of 1 / 64: image shifts and separations
    are exact, so the periodic count is the open count of set 1 against the 27 images of set 2 (the oracle's, per los)."""
    rng = np.random.default_rng(31)

    def draw(n):
        p = rng.integers(0, 641, (8 * n, 3)) / 64.0
        return p[np.any((p < 3.0) | (p > FACE_BOX - 3.0), axis=1)][:n]

    a, b = draw(400), draw(500)
    a[0], b[0] = [0.0, FACE_BOX, FACE_BOX], [FACE_BOX, 0.0, 0.0]      # on the faces themselves
    assert len(a) == 400 and len(b) == 500
    images = np.concatenate([b + FACE_BOX * np.array(o) for o in itertools.product((-1.0, 0.0, 1.0), repeat=3)])
    exp = [xorc.cross_counts_brute(a, images, FACE_S, FACE_MU, los=los) for los in (0, 1, 2)]
    return a, b, images, exp


@pytest.mark.parametrize("cells", ["1", "0"])
def test_faces_edges_and_corners(near_faces, cells, monkeypatch):
    monkeypatch.setenv("ASTRILD_TPCF_CELLS", cells)
    a, b, images, exp = near_faces
    for los in (0, 1, 2):
        got = gpu_cross(a, b, FACE_S, FACE_MU, boxsize=FACE_BOX, los=los)
        npt.assert_array_equal(got, exp[los])
        npt.assert_array_equal(gpu_cross(a, images, FACE_S, FACE_MU, los=los), exp[los])
        opn = gpu_cross(a, b, FACE_S, FACE_MU, los=los)
        npt.assert_array_equal(opn, xorc.cross_counts_brute(a, b, FACE_S, FACE_MU, los=los))
        assert (got - opn).sum() > 1000                               # pairs across the faces are there


# ---------------------------------------------------------------- the open grid
def test_open_sets_in_one_plane():
    rng = np.random.default_rng(32)
    for axis in (0, 1, 2):
        a, b = rng.uniform(0.0, 150.0, (1000, 3)), rng.uniform(0.0, 150.0, (1200, 3))
        a[:, axis] = b[:, axis] = 17.25
        s = np.linspace(0.0, 20.0, 11)
        for los in (axis, (axis + 1) % 3):
            npt.assert_array_equal(gpu_cross(a, b, s, LAT_MU, los=los), xorc.cross_counts_brute(a, b, s, LAT_MU, los=los))
        npt.assert_array_equal(gpu_cross(a, b, s), xorc.cross_counts_brute(a, b, s))
        npt.assert_array_equal(gpu_cross(a, None, s), xorc.auto_counts_open_brute(a, s))


def test_open_disjoint_bounding_boxes():
    rng = np.random.default_rng(33)
    s = np.linspace(0.0, 10.0, 6)
    a = rng.uniform(0.0, 30.0, (1200, 3))
    far = rng.uniform(0.0, 30.0, (1300, 3)) + np.array([40.5, 0.0, 0.0])      # gap 10.5 > smax
    got = gpu_cross(a, far, s, LAT_MU)
    assert not got.any()
    close = far - np.array([6.0, 0.0, 0.0])                                   # gap 4.5 < smax
    got = gpu_cross(a, close, s, LAT_MU, los=0)
    npt.assert_array_equal(got, xorc.cross_counts_brute(a, close, s, LAT_MU, los=0))
    assert got.sum() > 1000


def test_open_coordinates_offset_by_a_million():
    rng = np.random.default_rng(34)
    off = np.array([1.0e6, -1.0e6, 1.0e6])
    a, b = rng.uniform(0.0, 100.0, (2000, 3)) + off, rng.uniform(0.0, 100.0, (2500, 3)) + off
    s = np.linspace(0.0, 12.0, 13)
    got = gpu_cross(a, b, s, LAT_MU)
    npt.assert_array_equal(got, xorc.cross_counts_brute(a, b, s, LAT_MU))
    assert got.sum() > 10_000
    npt.assert_array_equal(gpu_cross(a, None, s, LAT_MU), xorc.auto_counts_open_brute(a, s, LAT_MU))


@pytest.mark.parametrize("box", [None, L])
@pytest.mark.parametrize("n1,n2", [(0, 0), (0, 1), (1, 0), (1, 1), (0, 500), (500, 0), (1, 500), (500, 1)])
def test_empty_and_single_object_sets(n1, n2, box):
    a, b = orc.uniform(500, L, 35)[:n1], (orc.uniform(500, L, 36) if n2 > 1 else np.array([[250.0, 244.0, 242.0]]))[:n2]
    if n1 == 1:
        a = np.array([[250.0, 250.0, 250.0]])
    got = gpu_cross(a, b, S50, MU40, boxsize=box, vel1=np.zeros_like(a))
    assert got.shape == (39, 39)
    npt.assert_array_equal(got, xorc.cross_counts_brute(a, b, S50, MU40, boxsize=box))
    if (n1, n2) == (1, 1):
        assert got.sum() == 1                                         # d = 10, mu = 0.8
    if not (n1 and n2):
        assert not got.any()
    auto = gpu_cross(a, None, S50, boxsize=box)
    assert auto.shape == (39,)
    if n1 < 2:
        assert not auto.any()
    torch.cuda.synchronize()


@pytest.mark.parametrize("box", [None, 20.0])
@pytest.mark.parametrize("shift", [0.0, 7.0])
def test_pairs_exactly_on_an_s_edge_and_a_mu_edge(shift, box):
    a = np.array([[0.0, 0.0, 0.0]]) + shift
    b = np.array([[0.0, 0.0, 2.0],       # d^2 = 4 = s_1^2: bin 0; mu = 1, the top mu edge: bin 1
                  [3.0, 0.0, 4.0],       # d^2 = 25 = s_2^2: bin 1; mu = 4 / 5 = the edge 0.8: bin 0
                  [2.0, 0.0, 0.0],       # mu = 0, the lowest mu edge: in no bin
                  [0.0, 0.0, 0.0],       # coincident with the point of set 1: never counts
                  [0.0, 6.0, 0.0]]) + shift                               # d = 6 = the top s edge, mu = 0: real-space only
    s, mu = [0.0, 2.0, 5.0, 6.0], [0.0, 0.8, 1.0]
    exp = [[0, 1], [1, 0], [0, 0]]
    for dtype in (np.float32, np.float64):
        assert gpu_cross(a.astype(dtype), b.astype(dtype), s, mu, boxsize=box).tolist() == exp
        assert gpu_cross(b.astype(dtype), a.astype(dtype), s, mu, boxsize=box).tolist() == exp
        assert gpu_cross(a.astype(dtype), b.astype(dtype), s, boxsize=box).tolist() == [2, 1, 1]
    npt.assert_array_equal(gpu_cross(a, b, s, mu, boxsize=box), xorc.cross_counts_brute(a, b, s, mu, boxsize=box))
    both = np.concatenate([a, b[:3]])
    npt.assert_array_equal(gpu_cross(both, None, s, mu, boxsize=box),
                           xorc.auto_counts_open_brute(both, s, mu))      # nothing within reach across a face of 20


# ---------------------------------------------------------------- redshift space
@pytest.mark.parametrize("pdt,vdt", list(itertools.product([np.float32, np.float64], repeat=2)))
def test_velocities_shift_each_set_in_its_own_dtypes(pdt, vdt):
    rng = np.random.default_rng(41)
    a = orc.uniform(3000, L, 42).astype(pdt)
    b = orc.uniform(3500, L, 43).astype(vdt)                          # set 2: the dtypes swapped
    va = rng.normal(0.0, 3000.0, a.shape).astype(vdt)                 # shifts of up to ~100 Mpc/h cross the faces
    vb = rng.normal(0.0, 3000.0, b.shape).astype(pdt)
    for los in (0, 2):
        sa, sb = orc.shift_and_wrap(a, va, L, los), orc.shift_and_wrap(b, vb, L, los)
        raw = a[:, los].astype(np.float64) + va[:, los] / 100.0
        assert np.sum((raw > L) | (raw < 0)) > 50                     # the wrap is exercised
        npt.assert_array_equal(gpu_cross(a, b, S50, MU40, boxsize=L, vel1=va, vel2=vb, los=los),
                               xorc.cross_counts(sa, sb, S50, MU40, los=los, boxsize=L))
        npt.assert_array_equal(gpu_cross(a, b, S50, MU40, boxsize=L, vel1=va, los=los),
                               xorc.cross_counts(sa, b.astype(np.float64), S50, MU40, los=los, boxsize=L))
        # open: the shift without the wrap (a box of 0 wraps nothing in the oracle either)
        oa, ob = orc.shift_and_wrap(a, va, 0.0, los), orc.shift_and_wrap(b, vb, 0.0, los)
        assert oa[:, los].max() > L and oa[:, los].min() < 0.0
        npt.assert_array_equal(gpu_cross(a, b, S50, MU40, vel1=va, vel2=vb, los=los),
                               xorc.cross_counts(oa, ob, S50, MU40, los=los))


def test_tpcf_class_shifts_both_samples_and_not_the_randoms():
    from astrild_amd.particles.hutils import TPCF
    rng = np.random.default_rng(44)
    a, b, r = orc.uniform(3000, L, 45).astype(np.float32), orc.uniform(3500, L, 46), orc.uniform(6000, L, 47)
    va, vb = rng.normal(0.0, 2000.0, a.shape), rng.normal(0.0, 2000.0, b.shape).astype(np.float32)
    s_e = np.linspace(0.1, 50.0, 40)
    for los in (None, 0):
        ax = 2 if los is None else los
        cen, mu, xi, c = TPCF.compute(a, va, L, "redshift", (0.1, 50.0), (0.001, 1.0), los=los, return_counts=True,
                                      pos2=b, vel2=vb, randoms=r)
        npt.assert_array_equal(cen, (s_e[1:] + s_e[:-1]) / 2.0)
        npt.assert_array_equal(mu, MU40)
        sa, sb = orc.shift_and_wrap(a, va, L, ax), orc.shift_and_wrap(b, vb, L, ax)
        assert sorted(c) == ["D1D1", "D1D2", "D1R", "D2D2", "D2R", "RR"] and len(xi) == 3
        npt.assert_array_equal(c["D1D2"], xorc.cross_counts(sa, sb, s_e, MU40, los=ax, boxsize=L))
        npt.assert_array_equal(c["D1R"], xorc.cross_counts(sa, r, s_e, MU40, los=ax, boxsize=L))
        npt.assert_array_equal(c["D2R"], xorc.cross_counts(sb, r, s_e, MU40, los=ax, boxsize=L))
        npt.assert_array_equal(c["D2D2"], orc.pair_counts(sb, L, s_e, MU40, los=ax))
        npt.assert_array_equal(c["RR"], orc.pair_counts(r, L, s_e, MU40, los=ax))
        ref = xorc.estimator("Landy-Szalay", c["D1D2"], c["D1R"], 2 * c["RR"], len(a), len(b), len(r))
        _close(xi[1], ref, xorc.estimator_terms("Landy-Szalay", c["D1D2"], c["D1R"], 2 * c["RR"], len(a), len(b), len(r)))
    x12 = TPCF.tpcf_s(a, va, s_e, MU40, 2, L, pos2=b, vel2=vb, do_auto=False, estimator="Natural")
    sa, sb = orc.shift_and_wrap(a, va, L, 2), orc.shift_and_wrap(b, vb, L, 2)
    ref = xorc.analytic_cross_xi(xorc.cross_counts(sa, sb, s_e, MU40, boxsize=L), len(a), len(b), L, s_e, MU40)
    _close(x12, ref, [ref + 1.0, np.ones_like(ref)])


# ---------------------------------------------------------------- estimators end to end
def _close(got, ref, terms):
    """Equal within 8 ulp of the largest term of the bin; where a term is not finite, the same inf / nan."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float64
    big = np.max(np.abs(np.stack([np.broadcast_to(t, ref.shape) for t in terms])), axis=0)
    ok = np.isfinite(big)
    npt.assert_array_equal(got[~ok], ref[~ok])
    assert np.all(np.abs(got[ok] - ref[ok]) <= 8.0 * np.finfo(np.float64).eps * big[ok])


EST_S = np.linspace(0.0, 30.0, 16)
EST_MU = np.linspace(0.0, 1.0, 6)
EST_L = 300.0


@pytest.fixture(scope="module")
def samples():
    """Sizes 4000 / 5000 / 12000 and the oracle's counts of every term, per geometry and per binning."""
    d1 = orc.clustered(4000, EST_L, 51, blobs=40, sigma=6.0)
    d2 = orc.clustered(5000, EST_L, 52, blobs=40, sigma=6.0)
    rnd = orc.uniform(12000, EST_L, 53)
    ref = {}
    for box, mu in itertools.product((EST_L, None), (None, EST_MU)):
        auto = (lambda p: orc.pair_counts(p, box, EST_S, mu)) if box else (lambda p: xorc.auto_counts(p, EST_S, mu))
        ref[box, mu is not None] = {
            "D1D1": auto(d1), "D2D2": auto(d2), "RR": auto(rnd),
            "D1D2": xorc.cross_counts(d1, d2, EST_S, mu, boxsize=box), "D1R": xorc.cross_counts(d1, rnd, EST_S, mu, boxsize=box),
            "D2R": xorc.cross_counts(d2, rnd, EST_S, mu, boxsize=box)}
    return d1, d2, rnd, ref


def _reference_terms(name, c, n1, n2, nr):
    """{11 / 12 / 22: (xi, terms)} from the oracle's counts with the oracle's formulas."""
    f = lambda k: c[k].astype(np.float64)
    args = {11: (2.0 * f("D1D1"), f("D1R"), 2.0 * f("RR"), n1, n1, nr), 12: (f("D1D2"), f("D1R"), 2.0 * f("RR"), n1, n2, nr),
            22: (2.0 * f("D2D2"), f("D2R"), 2.0 * f("RR"), n2, n2, nr)}
    return {k: (xorc.estimator(name, *a), xorc.estimator_terms(name, *a)) for k, a in args.items()}


NEEDS = {"Natural": {"RR"}, "Davis-Peebles": {"DR"}, "Hewett": {"DR", "RR"}, "Hamilton": {"DR", "RR"},
         "Landy-Szalay": {"DR", "RR"}}


@pytest.mark.parametrize("box", [EST_L, None], ids=["periodic", "open"])
@pytest.mark.parametrize("name", xorc.ESTIMATORS)
def test_estimators_with_randoms(samples, name, box):
    from astrild_amd.particles.hutils import s_mu_tpcf, tpcf_r
    d1, d2, rnd, ref = samples
    n1, n2, nr = len(d1), len(d2), len(rnd)
    for with_mu in (False, True):
        c_ref = ref[box, with_mu]
        exp = _reference_terms(name, c_ref, n1, n2, nr)
        if with_mu:
            call = lambda **kw: s_mu_tpcf(d1, EST_S, EST_MU, randoms=rnd, period=box, estimator=name, **kw)
            shape = (15, 5)
        else:
            call = lambda **kw: tpcf_r(d1, EST_S, box, estimator=name, randoms=rnd, **kw)
            shape = (15,)
        for do_auto, do_cross in ((True, True), (False, True), (True, False)):
            out, c = call(sample2=d2, do_auto=do_auto, do_cross=do_cross, return_counts=True)
            keys = [k for k, on in ((11, do_auto), (12, do_cross), (22, do_auto)) if on]
            if keys == [12]:
                assert isinstance(out, np.ndarray)
                out = (out,)
            assert isinstance(out, tuple) and len(out) == len(keys)
            for k, xi in zip(keys, out):
                assert xi.shape == shape
                _close(xi, *exp[k])
            want = {"D1D1", "D2D2"} if do_auto else set()
            want |= {"D1D2"} if do_cross else set()
            want |= {"RR"} if "RR" in NEEDS[name] else set()
            want |= ({"D1R"} | ({"D2R"} if do_auto else set())) if "DR" in NEEDS[name] else set()
            assert set(c) == want
            for k in c:
                assert c[k].dtype == np.int64
                npt.assert_array_equal(c[k], c_ref[k], err_msg=k)
        # one sample with randoms: xi_11 alone
        xi, c = call(return_counts=True)
        assert isinstance(xi, np.ndarray) and "D1D2" not in c and "D2D2" not in c
        _close(xi, *exp[11])


def test_symmetric_landy_szalay_from_the_counts(samples):
    from astrild_amd.particles.hutils import s_mu_tpcf
    d1, d2, rnd, ref = samples
    _, c = s_mu_tpcf(d1, EST_S, EST_MU, sample2=d2, randoms=rnd, estimator="Landy-Szalay", return_counts=True)
    for k in c:
        npt.assert_array_equal(c[k], ref[None, True][k])
    n1, n2, nr = float(len(d1)), float(len(d2)), float(len(rnd))
    with np.errstate(divide="ignore", invalid="ignore"):
        rr = 2.0 * c["RR"] / (nr * nr)
        xi = (c["D1D2"] / (n1 * n2) - c["D1R"] / (n1 * nr) - c["D2R"] / (n2 * nr) + rr) / rr
    assert np.isfinite(xi[c["RR"] > 0]).all() and np.count_nonzero(c["RR"]) > 60


def test_analytic_randoms_with_two_samples(samples):
    from astrild_amd.particles.hutils import s_mu_tpcf, tpcf_r
    d1, d2, _, ref = samples
    n1, n2 = len(d1), len(d2)
    c_ref = ref[EST_L, True]
    x12 = xorc.analytic_cross_xi(c_ref["D1D2"], n1, n2, EST_L, EST_S, EST_MU)
    first = None
    for name in xorc.ESTIMATORS:
        (a11, a12, a22), c = s_mu_tpcf(d1, EST_S, EST_MU, sample2=d2, period=EST_L, estimator=name, return_counts=True)
        assert sorted(c) == ["D1D1", "D1D2", "D2D2"]
        npt.assert_array_equal(c["D1D2"], c_ref["D1D2"])
        _close(a12, x12, [x12 + 1.0, np.ones_like(x12)])
        first = a12 if first is None else first
        npt.assert_array_equal(a12, first)                             # the same for every estimator name
        # the auto terms are the one-sample path, bit for bit
        npt.assert_array_equal(a11, orc.xi(gpu_auto(d1, EST_L, EST_S, EST_MU), n1, EST_L, EST_S, EST_MU))
        npt.assert_array_equal(a22, orc.xi(gpu_auto(d2, EST_L, EST_S, EST_MU), n2, EST_L, EST_S, EST_MU))
    r12 = tpcf_r(d1, EST_S, EST_L, sample2=d2, do_auto=False)
    rx = xorc.analytic_cross_xi(ref[EST_L, False]["D1D2"], n1, n2, EST_L, EST_S)
    _close(r12, rx, [rx + 1.0, np.ones_like(rx)])
    r11, r22 = tpcf_r(d1, EST_S, EST_L, "Hamilton", False, d2, do_cross=False)
    npt.assert_array_equal(r11, tpcf_r(d1, EST_S, EST_L))
    npt.assert_array_equal(r22, tpcf_r(d2, EST_S, EST_L))


def test_one_sample_calls_are_what_they_were(samples):
    from astrild_amd.particles.hutils import TPCF, tpcf_r
    d1 = samples[0]
    vel = np.random.default_rng(54).normal(0.0, 400.0, d1.shape)
    s_e = np.linspace(0.1, 60.0, 40)
    dd = gpu_auto(d1, EST_L, s_e, MU40, vel=vel)
    xi_then = orc.xi(dd, len(d1), EST_L, s_e, MU40)                   # 2 DD / RR - 1, the operations of _xi
    cen, mu, xi, counts = TPCF.compute(d1, vel, EST_L, "redshift", (0.1, 60.0), (0.001, 1.0), return_counts=True)
    assert isinstance(counts, np.ndarray)
    npt.assert_array_equal(counts, dd)
    npt.assert_array_equal(xi, xi_then)
    npt.assert_array_equal(TPCF.tpcf_s(d1, vel, s_e, MU40, 2, EST_L), xi_then)
    npt.assert_array_equal(TPCF.compute(d1, vel, EST_L, "redshift", (0.1, 60.0), (0.001, 1.0))[2], xi_then)
    xr, ddr = tpcf_r(d1, EST_S, EST_L, "Landy-Szalay", True)
    npt.assert_array_equal(ddr, gpu_auto(d1, EST_L, EST_S))
    npt.assert_array_equal(xr, orc.xi(ddr, len(d1), EST_L, EST_S))


# ---------------------------------------------------------------- argument checks
def test_value_errors_before_any_pair_work(monkeypatch):
    from astrild_amd import _lib
    from astrild_amd import device as dev
    from astrild_amd.particles.hutils import s_mu_tpcf, tpcf_r
    lib = _lib.lib()
    calls = []

    class Spy:
        """The library, with the pair-count entries recorded."""
        def __getattr__(self, name):
            if name in ("ast_tpcf_cross_counts", "ast_tpcf_pair_counts"):
                calls.append(name)
            return getattr(lib, name)

    a, b, r = orc.uniform(800, L, 61), orc.uniform(900, L, 62), orc.uniform(1000, L, 63)

    def bad(p, row, col, value):
        q = p.copy()
        q[row, col] = value
        return q

    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    for kw in (dict(pos1=bad(a, 17, 1, L + 0.5)), dict(pos2=bad(b, 3, 0, -1e-9)), dict(pos1=bad(a, 5, 2, np.nan)),
               dict(pos2=bad(b, 0, 0, np.inf))):
        args = dict(pos1=a, pos2=b)
        args.update(kw)
        with pytest.raises(ValueError, match="must lie in"):
            dev.tpcf_cross_counts(args["pos1"], args["pos2"], S50, MU40, boxsize=L)
    vel = np.zeros_like(b)
    vel[9, 2] = 200.0 * L                                             # shifted by 2 L: one wrap is not enough
    with pytest.raises(ValueError, match="must lie in"):
        dev.tpcf_cross_counts(a, b, S50, MU40, boxsize=L, vel2=vel)
    for p1, p2 in ((bad(a, 1, 1, np.nan), b), (a, bad(b, 2, 0, np.nan)), (bad(a, 4, 2, -np.inf), b), (bad(a, 7, 0, np.nan), None)):
        with pytest.raises(ValueError, match="must be finite"):
            dev.tpcf_cross_counts(p1, p2, S50, MU40)
    with pytest.raises(ValueError, match="boxsize / 3"):
        dev.tpcf_cross_counts(a, b, np.linspace(0.0, L / 3.0, 10), boxsize=L)
    for args in ((a[:, :2], b), (a, b.reshape(-1)), (a, b[:, :2])):
        with pytest.raises(ValueError, match=r"\(N, 3\)"):
            dev.tpcf_cross_counts(*args, S50)
    with pytest.raises(ValueError, match="los"):
        dev.tpcf_cross_counts(a, b, S50, los=3)
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        dev.tpcf_cross_counts(a, b, S50, vel1=np.zeros((5, 3)))
    assert calls == []
    # the randoms of the Python API: outside the box when periodic, not finite when open
    with pytest.raises(ValueError, match="must lie in"):
        tpcf_r(a, S50, L, "Davis-Peebles", sample2=b, randoms=bad(r, 11, 1, L + 1.0), do_auto=False)
    with pytest.raises(ValueError, match="must be finite"):
        s_mu_tpcf(a, S50, MU40, sample2=b, randoms=bad(r, 11, 1, np.nan), estimator="Davis-Peebles", do_auto=False)
    # on the faces is inside, as for the one-sample call; open boundaries have no limit on the top edge
    edge = bad(bad(a, 0, 0, 0.0), 1, 2, L)
    npt.assert_array_equal(gpu_cross(edge, b, S50, MU40, boxsize=L), xorc.cross_counts(edge, b, S50, MU40, boxsize=L))
    wide = np.linspace(0.0, 400.0, 5)
    npt.assert_array_equal(gpu_cross(a, b, wide), xorc.cross_counts_brute(a, b, wide))


# ---------------------------------------------------------------- scratch memory and call order
@pytest.mark.parametrize("mode", ["periodic", "open", "open-auto"])
def test_dirty_scratch(catalogues, dirty_alloc, mode):
    a, b, ref = catalogues
    mark = dirty_alloc.mark()
    if mode == "open-auto":
        sub = a[:1500]
        got = gpu_cross(sub, None, S50, MU40)
        exp = xorc.auto_counts_open_brute(sub, S50, MU40)
    else:
        got = gpu_cross(a, b, S50, MU40, boxsize=L if mode == "periodic" else None)
        exp = ref[mode]
    assert dirty_alloc.since(mark) >= 3                               # workspace, bounds, counts
    npt.assert_array_equal(got, exp)


def test_dirty_scratch_early_returns(dirty_alloc):
    a = orc.uniform(300, L, 71)
    none = np.zeros((0, 3))
    for box in (None, L):
        assert not gpu_cross(a, none, S50, MU40, boxsize=box).any()
        assert not gpu_cross(none, a, S50, boxsize=box).any()
        assert not gpu_cross(a[:1], None, S50, MU40, boxsize=box).any()


def test_call_order(catalogues, crowded):
    a, b, ref = catalogues
    ca, cb = crowded
    first = lambda: gpu_cross(a, b, S50, MU40, boxsize=L)
    second = lambda: gpu_cross(ca, cb, CROWD_S)
    third = lambda: gpu_cross(b, None, S50, MU40)
    x1, x2, x3 = first(), second(), third()
    y3, y2, y1 = third(), second(), first()
    npt.assert_array_equal(x1, y1)
    npt.assert_array_equal(x2, y2)
    npt.assert_array_equal(x3, y3)
    npt.assert_array_equal(x1, ref["periodic"])
    npt.assert_array_equal(x2, xorc.cross_counts_brute(ca, cb, CROWD_S))
