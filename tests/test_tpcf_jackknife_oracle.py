"""CPU: the jackknife of the two-point correlation function without a GPU.  The endpoint identity the kernel rests on,
against the brute-force WEIGHTED count of tests/tpcf_jackknife_oracle.py; jackknife_from_counts (the package's host
arithmetic) against a covariance the oracle forms on its own; the region tags; the argument checks and the four return
shapes of tpcf_jackknife with the device counts replaced by the oracle's."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import tpcf_cross_oracle as xorc
from tests import tpcf_jackknife_oracle as jorc
from tests import tpcf_oracle as orc

BOX = 100.0
EDGES = [0, 2, 5, 10, 18, 30]
NSUB = (3, 2, 2)
NTOT = 12
TERMS = {"D1D1": ("1", None), "D1R": ("1", "R"), "RR": ("R", None)}


@pytest.fixture(scope="module")
def sample():
    """The input of the issue: 400 clustered points, 1200 randoms, five bins, 3 x 2 x 2 regions of a box of 100; per
    term the oracle's (counts, w2, ends)."""
    pos = {"1": orc.clustered(400, BOX, 5, blobs=12, sigma=6), "R": orc.uniform(1200, BOX, 6)}
    tags = {k: jorc.region_tags(p, NSUB, [0.0] * 3, [BOX] * 3) for k, p in pos.items()}
    ints = {}
    for term, (a, b) in TERMS.items():
        ints[term] = jorc.jackknife_counts_brute(pos[a], tags[a], None if b is None else pos[b],
                                                 None if b is None else tags[b], NTOT, EDGES, boxsize=BOX)
        for x in ints[term]:
            x.setflags(write=False)
    return pos, tags, ints


def test_endpoint_identity_against_the_weighted_count(sample):
    """2 W_k == 2 counts - E_k and sum_k E_k == 2 counts, for DD, DR and RR; every leave-one-out bin is populated, so
    no estimator divides by zero on this input."""
    _, tags, ints = sample
    assert all(len(np.unique(t)) == NTOT for t in tags.values())
    for term, (counts, w2, ends) in ints.items():
        assert counts.shape == (5,) and w2.shape == ends.shape == (NTOT, 5)
        npt.assert_array_equal(w2, 2 * counts[None] - ends, err_msg=term)
        npt.assert_array_equal(ends.sum(axis=0), 2 * counts, err_msg=term)
        assert w2.min() > 0, term
        assert np.any(ends != ends[0]), term                     # the regions differ: the table is not counts / n


@pytest.mark.parametrize("name", xorc.ESTIMATORS)
def test_xi_and_covariance_against_the_oracles_loop(sample, name):
    """jackknife_from_counts, fed (counts, ends), against the oracle's loop over the regions fed the weighted counts,
    with np.cov.  Both sum the same fp64 numbers in another order; largest deviation of a covariance element measured
    on the CPU over the five estimators: 1.5e-16 of max|cov| (1.451e-16, Davis-Peebles; 0.2e-16 to 0.5e-16 for the
    others), so the bound is 10 x that, 1.5e-15 max|cov|.  xi itself is the same operations on the same numbers:
    equal."""
    from astrild_amd.particles.hutils.tpcf import jackknife_from_counts
    pos, tags, ints = sample
    sizes = {k: len(p) for k, p in pos.items()}
    occ = {k: np.bincount(t, minlength=NTOT) for k, t in tags.items()}
    xi, cov = jackknife_from_counts({t: (v[0], v[2]) for t, v in ints.items()}, sizes["1"], occ["1"], sizes["R"], occ["R"],
                                    estimator=name)
    ref_xi, ref_cov, xik = jorc.xi_and_cov(name, {t: v[1] for t, v in ints.items()}, {t: v[0] for t, v in ints.items()},
                                           sizes, occ, "1", "1")
    assert np.isfinite(xik).all() and np.isfinite(ref_cov).all() and np.isfinite(cov).all()
    assert xi.shape == (5,) and cov.shape == (5, 5)
    npt.assert_array_equal(xi, ref_xi)
    scale = np.abs(ref_cov).max()
    dev = np.abs(cov - ref_cov).max() / scale
    print(f"{name}: max |cov - ref| / max|cov| = {dev:.3e}, max|cov| = {scale:.3e}")
    assert dev <= 1.5e-15
    npt.assert_array_equal(cov, cov.T)
    assert np.all(np.diag(cov) > 0)


# ---------------------------------------------------------------- tags
def test_tags_on_faces_and_at_the_top_of_the_box():
    from astrild_amd.particles.hutils.tpcf import jackknife_tags
    L = 12.0
    pts = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [8.0, 6.0, 6.0], [L, L, L], [np.nextafter(4.0, 0.0), 6.0, 0.0],
                    [11.9, 5.9, 11.9], [-1.0, 13.0, 3.0], [np.nan, 1.0, 7.0]])
    exp = [0, 4, 11, 11, 2, 9, 2, 1]                              # (ix * 2 + iy) * 2 + iz over 3 x 2 x 2
    got = jackknife_tags(pts, (3, 2, 2), [0.0] * 3, [L] * 3)
    assert got.dtype == np.int32 and got.tolist() == exp
    npt.assert_array_equal(jorc.region_tags(pts, (3, 2, 2), [0.0] * 3, [L] * 3), exp)


def test_tags_of_float32_points_and_a_non_cubic_grid():
    from astrild_amd.particles.hutils.tpcf import jackknife_tags
    rng = np.random.default_rng(3)
    for dtype in (np.float32, np.float64):
        pts = rng.uniform(0.0, BOX, (5000, 3)).astype(dtype)
        pts[:50] = np.round(pts[:50] / 12.5) * 12.5               # on the faces of 8, 4 and 2 regions per axis
        for nsub, lo, hi in (((8, 4, 2), [0.0] * 3, [BOX] * 3), ((2, 3, 5), [-7.0, 0.5, 10.0], [93.0, 99.25, 60.0]),
                             ((1, 1, 7), [0.0] * 3, [BOX] * 3)):
            got = jackknife_tags(pts, nsub, lo, hi)
            npt.assert_array_equal(got, jorc.region_tags(pts, nsub, lo, hi))
            assert got.min() == 0 and got.max() == nsub[0] * nsub[1] * nsub[2] - 1
    one = np.array([[10.0, 60.0, 30.0]], dtype=np.float32)        # axis order: x slowest, z fastest
    assert jackknife_tags(one, (8, 4, 2), [0.0] * 3, [BOX] * 3).tolist() == [(0 * 4 + 2) * 2 + 0]
    assert jackknife_tags(one, (2, 4, 8), [0.0] * 3, [BOX] * 3).tolist() == [(0 * 4 + 2) * 8 + 2]
    assert jackknife_tags(np.zeros((0, 3)), (2, 2, 2), [0.0] * 3, [1.0] * 3).shape == (0,)


def test_a_single_region_leaves_nothing(sample):
    pos, _, ints = sample
    tags = np.zeros(len(pos["1"]), dtype=np.int64)
    npt.assert_array_equal(jorc.region_tags(pos["1"], (1, 1, 1), [0.0] * 3, [BOX] * 3), tags)
    counts, w2, ends = jorc.jackknife_counts_brute(pos["1"], tags, None, None, 1, EDGES, boxsize=BOX)
    npt.assert_array_equal(counts, ints["D1D1"][0])
    assert not w2.any()
    npt.assert_array_equal(ends, 2 * counts[None])


# ---------------------------------------------------------------- arguments and return shapes
def test_check_jackknife_args():
    from astrild_amd import _lib
    from astrild_amd.device import check_jackknife_args as check
    nsub3, ntot, lo, hi = check(5, (10, 3), boxsize=50.0)
    assert nsub3 == (5, 5, 5) and ntot == 125 and lo.tolist() == [0.0] * 3 and hi.tolist() == [50.0] * 3
    nsub3, ntot, lo, hi = check(np.array([3, 2, 2]), (10, 3), (4, 3))
    assert nsub3 == (3, 2, 2) and ntot == 12 and lo is None and hi is None
    nsub3, ntot, lo, hi = check([2, 1, 4], (10, 3), extent=(-1.0, [1.0, 2.0, 3.0]), boxsize=50.0)
    assert nsub3 == (2, 1, 4) and lo.tolist() == [-1.0] * 3 and hi.tolist() == [1.0, 2.0, 3.0]
    nsub3, ntot, lo, hi = check(np.int64(7), (10, 3), (4, 3), (10,), (4,))
    assert nsub3 == (7, 1, 1) and ntot == 7
    for bad in (0, -1, 2.5, True, "3", None, [2, 2], [2, 2, 0], [2, 2, 2.0], [2, 2, 2, 2]):
        with pytest.raises(ValueError, match="nsub"):
            check(bad, (10, 3))
    for shape in ((10,), (10, 2), (3, 10, 3)):
        with pytest.raises(ValueError, match=r"\(N, 3\)"):
            check(2, shape)
        with pytest.raises(ValueError, match=r"\(N, 3\)"):
            check(2, (10, 3), shape)
    with pytest.raises(ValueError, match="tags2 given without pos2"):
        check(2, (10, 3), None, (10,), (10,))
    with pytest.raises(ValueError, match="both samples or for neither"):
        check(2, (10, 3), (4, 3), (10,))
    with pytest.raises(ValueError, match="both samples or for neither"):
        check(2, (10, 3), (4, 3), None, (4,))
    with pytest.raises(ValueError, match="a single int"):
        check([2, 2, 2], (10, 3), tags1_shape=(10,))
    with pytest.raises(ValueError, match="one region per object"):
        check(2, (10, 3), tags1_shape=(9,))
    with pytest.raises(ValueError, match="one region per object"):
        check(2, (10, 3), (4, 3), (10,), (4, 1))
    with pytest.raises(ValueError, match="extent has no meaning"):
        check(2, (10, 3), tags1_shape=(10,), extent=(0.0, 1.0))
    for extent in ((0.0, 0.0), (1.0, 0.0), (0.0, np.inf), (np.nan, 1.0), ([0.0, 0.0], 1.0), (0.0,), 3.0):
        with pytest.raises(ValueError, match="extent"):
            check(2, (10, 3), extent=extent)
    limit = _lib.TPCF_JK_MAX_TABLE
    assert check(4, (10, 3), nbins=limit // 64)[1] == 64
    with pytest.raises(ValueError, match="counters"):
        check(4, (10, 3), nbins=limit // 64 + 1)


def _stub_counts(calls):
    """device.tpcf_jackknife_counts on the host: the oracle's integers as CPU tensors (explicit tags only)."""
    torch = pytest.importorskip("torch")

    def counts(pos1, nsub, s_edges, mu_edges=None, pos2=None, boxsize=None, vel1=None, vel2=None, los=2, tags1=None,
               tags2=None, extent=None):
        assert tags1 is not None and (pos2 is None) == (tags2 is None) and extent is None and vel1 is None
        calls.append((len(pos1), None if pos2 is None else len(pos2)))
        c, _, e = jorc.jackknife_counts_brute(pos1, tags1, pos2, tags2, nsub, s_edges, mu_edges, los, boxsize)
        return torch.from_numpy(c.copy()), torch.from_numpy(e.copy())
    return counts


@pytest.mark.parametrize("period", [BOX, None], ids=["periodic", "open"])
def test_return_shapes_and_argument_checks_with_stubbed_counts(sample, period, monkeypatch):
    from astrild_amd import device as dev
    from astrild_amd.particles.hutils import tpcf_jackknife
    from astrild_amd.particles.hutils.tpcf import jackknife_from_counts, jackknife_tags
    pos, _, ints = sample
    d1, d2, rnd = pos["1"][:150], pos["1"][150:330].astype(np.float32), pos["R"][:500]
    calls = []
    monkeypatch.setattr(dev, "tpcf_jackknife_counts", _stub_counts(calls))
    mu = [0.0, 0.5, 1.0]
    # one sample
    xi, cov, c = tpcf_jackknife(d1, rnd, EDGES, Nsub=NSUB, period=period, estimator="Landy-Szalay", return_counts=True,
                                num_threads=4, seed=1)
    assert xi.shape == (5,) and cov.shape == (5, 5) and sorted(c) == ["D1D1", "D1R", "RR"]
    assert calls == [(150, None), (150, 500), (500, None)]
    lo, hi = (np.zeros(3), np.full(3, BOX)) if period else (np.minimum(d1.min(0), rnd.min(0)), np.maximum(d1.max(0), rnd.max(0)))
    t1, tr = jackknife_tags(d1, NSUB, lo, hi), jackknife_tags(rnd, NSUB, lo, hi)
    exp = jorc.jackknife_counts_brute(d1, t1, rnd, tr, NTOT, EDGES, boxsize=period)
    npt.assert_array_equal(c["D1R"][0], exp[0])
    npt.assert_array_equal(c["D1R"][1], exp[2])
    ref = jackknife_from_counts(c, 150, np.bincount(t1, minlength=NTOT), 500, np.bincount(tr, minlength=NTOT),
                                estimator="Landy-Szalay")
    npt.assert_array_equal(xi, ref[0])
    npt.assert_array_equal(cov, ref[1])
    out = tpcf_jackknife(d1, rnd, EDGES, Nsub=NSUB, period=period)                       # Natural: no DR
    assert len(out) == 2 and calls[3:] == [(150, None), (500, None)]
    # two samples: all three terms, cross only, auto only; with mu bins the covariance is over the flattened bins
    del calls[:]
    out = tpcf_jackknife(d1, rnd, EDGES, Nsub=[2, 2, 1], sample2=d2, period=period, estimator="Hamilton", mu_bins=mu,
                         return_counts=True)
    assert len(out) == 7 and sorted(out[6]) == ["D1D1", "D1D2", "D1R", "D2D2", "D2R", "RR"]
    assert all(x.shape == (5, 2) for x in out[:3]) and all(x.shape == (10, 10) for x in out[3:6])
    assert out[6]["D1D2"][0].shape == (5, 2) and out[6]["D1D2"][1].shape == (4, 5, 2)
    assert calls == [(150, None), (150, 180), (180, None), (150, 500), (180, 500), (500, None)]
    x12, c12 = tpcf_jackknife(d1, rnd, EDGES, Nsub=[2, 2, 1], sample2=d2, period=period, estimator="Hamilton", mu_bins=mu,
                              do_auto=False)
    npt.assert_array_equal(x12, out[1])
    npt.assert_array_equal(c12, out[4])
    a = tpcf_jackknife(d1, rnd, EDGES, Nsub=[2, 2, 1], sample2=d2, period=period, estimator="Hamilton", mu_bins=mu,
                       do_cross=False)
    assert len(a) == 4
    for got, want in zip(a, (out[0], out[2], out[3], out[5])):
        npt.assert_array_equal(got, want)
    # ValueErrors before any count
    del calls[:]
    for kw, match in ((dict(estimator="Peebles"), "estimator"), (dict(do_auto=False, do_cross=False), "both False"),
                      (dict(Nsub=0), "nsub"), (dict(Nsub=[2, 2]), "nsub"), (dict(rbins=[3.0, 2.0]), "s edges"),
                      (dict(mu_bins=[0.0, 2.0]), "mu edges")):
        args = dict(sample1=d1, randoms=rnd, rbins=EDGES, Nsub=NSUB, period=period)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            tpcf_jackknife(**args)
    with pytest.raises(ValueError, match="randoms"):
        tpcf_jackknife(d1, None, EDGES, period=period)
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        tpcf_jackknife(d1[:, :2], rnd, EDGES, period=period)
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        tpcf_jackknife(d1, rnd, EDGES, sample2=d2.reshape(-1), period=period)
    if period:
        with pytest.raises(ValueError, match="boxsize / 3"):
            tpcf_jackknife(d1, rnd, [0.0, 40.0], period=period)
    assert calls == []
