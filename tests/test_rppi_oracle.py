"""CPU-only: the (r_p, pi) oracle (tests/rppi_oracle.py) against known answers and direct counts, and the host-only
parts of the package's (r_p, pi) API - device.check_rp_pi_edges and wp_from_xi - which need no GPU."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import rppi_oracle as orc
from tests.tpcf_oracle import lattice, uniform


@pytest.mark.parametrize("los", [0, 1, 2])
@pytest.mark.parametrize("m, top", [(8, 3), (12, 5)])
def test_brute_force_equals_the_lattice_count(m, top, los):
    # integer edges: every pair sits exactly on an r_p edge or between two, and on a pi edge; m = 12 reaches the
    # offsets (3, 4) across the line of sight, r_p = 5 exactly on the top edge
    rp, pi = np.arange(top + 1.0), np.arange(top + 1.0)
    lat = lattice(m)
    exp = orc.lattice_expected(m, rp, pi, los)
    assert exp.sum() > 0 and exp[0].sum() == m ** 3 // 2 * 4 * 2 * top      # r_p = 1: 4 vectors across, 2 top along
    npt.assert_array_equal(orc.rppi_auto_brute(lat, rp, pi, los, boxsize=float(m)), exp)
    cross = orc.rppi_cross_brute(lat, lat, rp, pi, los, boxsize=float(m))
    npt.assert_array_equal(cross, 2 * exp)                                  # ordered; the self pairs are in no bin


def test_pairs_on_the_lowest_edges_are_in_no_bin():
    rp, pi = np.array([0.0, 1.0, 2.0]), np.array([0.0, 1.0, 2.0])
    a = np.array([[5.0, 5.0, 5.0]])
    for b, hit in (([5.0, 5.0, 5.0], None), ([6.0, 5.0, 5.0], None), ([5.0, 5.0, 6.0], None), ([6.0, 5.0, 6.0], (0, 0)),
                   ([5.0, 7.0, 7.0], (1, 1)), ([5.0, 7.0, 7.5], None)):
        got = orc.rppi_cross_brute(a, np.array([b]), rp, pi, los=2)
        assert got.sum() == (0 if hit is None else 1), b
        if hit is not None:
            assert got[hit] == 1


@pytest.mark.parametrize("los", [0, 1, 2])
@pytest.mark.parametrize("boxsize", [None, 60.0])
def test_sum_over_pi_is_the_rp_count(los, boxsize):
    a, b = uniform(400, 60.0, 31), uniform(300, 60.0, 32)
    rp = np.geomspace(0.5, 15.0, 7)
    big = 1000.0
    # pi = 0 would be in no (r_p, pi) bin: none of these continuous coordinates coincide
    assert all((np.abs(a[:, None, ax] - b[None, :, ax]) > 0).all() for ax in range(3))
    got = orc.rppi_cross_brute(a, b, rp, [0.0, big], los, boxsize)
    assert got.shape == (6, 1) and got.sum() > 1000
    npt.assert_array_equal(got.sum(axis=1), orc.rp_counts_brute(a, b, rp, los, boxsize))
    split = orc.rppi_cross_brute(a, b, rp, [0.0, 3.0, 7.5, 20.0, big], los, boxsize)
    npt.assert_array_equal(split.sum(axis=1), got[:, 0])
    auto = orc.rppi_auto_brute(a, rp, [0.0, big], los, boxsize)
    npt.assert_array_equal(2 * auto, orc.rppi_cross_brute(a, a, rp, [0.0, big], los, boxsize))


def test_weighted_leave_one_out_counts():
    a, b = uniform(150, 30.0, 41), uniform(120, 30.0, 42)
    rp, pi = np.array([0.0, 2.0, 5.0]), np.array([0.0, 4.0, 9.0])
    ta, tb = (a[:, 0] > 15.0).astype(np.int64), (b[:, 0] > 15.0).astype(np.int64)
    counts, w2 = orc.jackknife_brute(a, ta, b, tb, 2, rp, pi, boxsize=30.0)
    npt.assert_array_equal(counts, orc.rppi_cross_brute(a, b, rp, pi, boxsize=30.0))
    for k in (0, 1):
        # region k left out: the pairs of the other region's objects weigh 1, those across 1/2
        both_out = orc.rppi_cross_brute(a[ta != k], b[tb != k], rp, pi, boxsize=30.0)
        mixed = orc.rppi_cross_brute(a[ta == k], b[tb != k], rp, pi, boxsize=30.0) + \
            orc.rppi_cross_brute(a[ta != k], b[tb == k], rp, pi, boxsize=30.0)
        npt.assert_array_equal(w2[k], 2 * both_out + mixed)
    counts, w2 = orc.jackknife_brute(a, ta, None, None, 2, rp, pi, boxsize=30.0)
    npt.assert_array_equal(counts, orc.rppi_auto_brute(a, rp, pi, boxsize=30.0))
    npt.assert_array_equal(w2.sum(axis=0), 2 * counts)          # two regions: every pair end is in one of them


def test_wp_of_a_constant_xi():
    pi = np.array([0.0, 1.0, 2.5, 7.0, 40.0])
    xi = np.full((6, 4), 0.375)
    npt.assert_allclose(orc.wp_from_xi(xi, pi), np.full(6, 2.0 * 0.375 * 40.0), rtol=1e-15)
    npt.assert_allclose(orc.wp_matrix(6, pi) @ xi.ravel(), orc.wp_from_xi(xi, pi), rtol=1e-15)
    vol = orc.bin_volume([0.0, 1.0, 3.0], pi)
    npt.assert_allclose(vol.sum(), np.pi * 9.0 * 2.0 * 40.0, rtol=1e-15)    # the whole cylinder, both sides


# ---------------------------------------------------------------- the package's host-only parts
def test_package_wp_from_xi():
    from astrild_amd.particles.hutils import wp_from_xi
    rng = np.random.default_rng(5)
    pi = np.array([0.0, 0.5, 2.0, 2.25, 30.0])
    xi = rng.normal(0.0, 1.0, (7, 4))
    got = wp_from_xi(xi, pi)
    assert got.shape == (7,) and got.dtype == np.float64
    npt.assert_allclose(got, orc.wp_from_xi(xi, pi), rtol=1e-13)
    npt.assert_allclose(got, orc.wp_matrix(7, pi) @ xi.ravel(), rtol=1e-13)
    npt.assert_array_equal(wp_from_xi(np.full((3, 1), 1.5), [0.0, 40.0]), np.full(3, 2.0 * 1.5 * 40.0))
    assert wp_from_xi(xi[0], pi).shape == ()
    assert wp_from_xi(np.stack([xi, xi]), pi).shape == (2, 7)
    with pytest.raises(ValueError):
        wp_from_xi(xi, pi[:-1])


def test_check_rp_pi_edges():
    from astrild_amd import device as dev
    rp, pi = dev.check_rp_pi_edges([0, 1, 2.5], np.array([0, 10, 33], dtype=np.float32), 100.0)
    assert rp.dtype == np.float64 and pi.dtype == np.float64
    npt.assert_array_equal(rp, [0.0, 1.0, 2.5])
    npt.assert_array_equal(pi, [0.0, 10.0, 33.0])
    bad = [
        ([0.0, 1.0, 1.0], [0.0, 5.0]),                  # r_p not strictly increasing
        ([1.0, 0.5], [0.0, 5.0]),
        ([-1.0, 1.0], [0.0, 5.0]),
        ([0.0, np.nan], [0.0, 5.0]),
        ([0.0, np.inf], [0.0, 5.0]),
        ([1.0], [0.0, 5.0]),
        ([0.0, 1.0], [5.0]),                            # pi: at least two values
        ([0.0, 1.0], None),
        ([0.0, 1.0], [0.0, 5.0, 5.0]),
        ([0.0, 1.0], [-0.5, 5.0]),
        ([0.0, 1.0], [0.0, np.nan]),
        ([0.0, 1.0], [0.0, np.inf]),
        ([0.0, 100.0 / 3.0], [0.0, 5.0]),               # periodic: both top edges below boxsize / 3
        ([0.0, 1.0], [0.0, 100.0 / 3.0]),
        (np.linspace(0.0, 10.0, 1002), [0.0, 5.0]),     # fewer than 1001 edges per axis
        ([0.0, 1.0], np.linspace(0.0, 10.0, 1002)),
        (np.linspace(0.0, 10.0, 102), np.linspace(0.0, 10.0, 101)),     # 101 x 100 bins
    ]
    for rp_e, pi_e in bad:
        with pytest.raises(ValueError):
            dev.check_rp_pi_edges(rp_e, pi_e, 100.0)
    for box in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            dev.check_rp_pi_edges([0.0, 1.0], [0.0, 5.0], box)
    # open boundaries: no box, free top edges, the other rules unchanged
    rp, pi = dev.check_rp_pi_edges([0.0, 500.0], [0.0, 1e6], None, periodic=False)
    assert rp[-1] == 500.0 and pi[-1] == 1e6
    with pytest.raises(ValueError):
        dev.check_rp_pi_edges([0.0, 500.0], [1e6], None, periodic=False)
    dev.check_rp_pi_edges(np.linspace(0.0, 10.0, 101), np.linspace(0.0, 10.0, 101), 100.0)      # 100 x 100: the limit


def test_api_value_errors_need_no_gpu():
    from astrild_amd.particles.hutils import rp_pi_tpcf, rp_pi_tpcf_jackknife, wp, wp_jackknife
    a = uniform(10, 100.0, 1)
    with pytest.raises(ValueError):
        rp_pi_tpcf(a, [0.0, 1.0], [0.0, 5.0])                               # neither period nor randoms
    with pytest.raises(ValueError):
        rp_pi_tpcf(a, [0.0, 1.0], [0.0, 5.0], period=100.0, estimator="Peebles")
    with pytest.raises(ValueError):
        rp_pi_tpcf(a, [0.0, 1.0], [0.0, 5.0], period=100.0, do_auto=False, do_cross=False)
    with pytest.raises(ValueError):
        rp_pi_tpcf(a, [0.0, 1.0], [0.0, 40.0], period=100.0)
    with pytest.raises(ValueError):
        wp(a, [0.0, 1.0], 20.0, period=100.0, pi_bins=[0.0, 10.0, 19.0])   # pi_bins must end at pi_max
    with pytest.raises(ValueError):
        wp(a, [0.0, 1.0], 40.0, period=100.0)
    with pytest.raises(ValueError):
        rp_pi_tpcf_jackknife(a, None, [0.0, 1.0], [0.0, 5.0], period=100.0)
    with pytest.raises(ValueError):
        wp_jackknife(a, None, [0.0, 1.0], 5.0, period=100.0)
    with pytest.raises(ValueError):
        wp_jackknife(a, a, [0.0, 1.0], 5.0, period=100.0, pi_bins=[0.0, 4.0])
