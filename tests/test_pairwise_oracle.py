"""CPU: the numpy restatement of the pairwise-velocity estimator against the reference's known answers
(tests/golden/pairwise_known_answers.json), its edge semantics, and the product module's GPU-free helpers."""
import json
import os

import numpy as np
import numpy.testing as npt

from tests import pairwise_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairwise_known_answers.json")


def spec():
    with open(GOLDEN) as f:
        return json.load(f)


def test_product_module_imports_without_a_gpu():
    from astrild_amd.particles.hutils import mean_pairwise_velocity as mpv
    from astrild_amd.particles.hutils import make_rsep, make_rsep_uneven_bins, mean_pv_from_tv  # noqa: F401
    assert callable(mpv.mean_pv_from_tv)


def test_make_rsep_known_answers():
    from astrild_amd.particles.hutils.mean_pairwise_velocity import make_rsep
    s = spec()["make_rsep"]
    bins = np.linspace(*spec()["catalogue"]["bins_linspace"])
    binnr, binwidth = len(bins), np.diff(bins)[0]
    assert (binnr, binwidth) == (s["binnr"], s["binwidth"])
    rsep = make_rsep(binnr, binwidth)
    assert len(rsep) == s["len"]
    npt.assert_almost_equal(np.diff(rsep), s["step"], decimal=s["decimal"])
    npt.assert_almost_equal(rsep[0], s["first"], decimal=s["decimal"])
    npt.assert_almost_equal(rsep[-1], s["last"], decimal=s["decimal"])
    npt.assert_array_equal(rsep, orc.mean_pv_from_tv(np.zeros((0, 3)), np.zeros((0, 2)), bins)[0])


def test_make_rsep_uneven_bins():
    from astrild_amd.particles.hutils.mean_pairwise_velocity import make_rsep_uneven_bins
    edges = np.array([0.0, 1.0, 3.0, 7.0, 15.0])
    npt.assert_array_equal(make_rsep_uneven_bins(edges), [0.5, 2.0, 5.0, 11.0])
    assert len(make_rsep_uneven_bins(edges)) == len(edges) - 1


def test_oracle_reproduces_known_answers():
    s = spec()
    pos, vel, bins = orc.known_answer_catalogue(s)
    rsep, pest, nom, den, cnt = orc.mean_pv_from_tv(pos, vel, bins)
    k = s["mean_pv_from_tv"]
    assert len(pest) == k["len"]
    npt.assert_almost_equal(pest[0], k["first"], decimal=k["decimal"])
    npt.assert_almost_equal(pest[-1], k["last"], decimal=k["decimal"])


def test_binnr_is_len_bins_and_one_width():
    # two objects 10.5 apart: bins [0, 1, 2, 3] have len 4, so the reach is 4 * 1 and the pair is out;
    # the same edges extended by one uneven far edge still use width 1 (reach 5 * 1): still out.  Width 3: bin 3 of 4.
    pos = np.array([[0.0, 0.0, 1000.0], [10.5, 0.0, 1000.0], [0.0, 2.5, 1000.0]])
    vel = np.array([[10.0, -20.0], [30.0, 5.0], [-7.0, 1.0]])
    _, _, _, _, cnt = orc.mean_pv_from_tv(pos, vel, np.array([0.0, 1.0, 2.0, 3.0]))
    assert len(cnt) == 4 and cnt.tolist() == [0, 0, 1, 0]          # only the 2.5 pair, in bin int(2.5) = 2
    _, _, _, _, cnt = orc.mean_pv_from_tv(pos, vel, np.array([0.0, 1.0, 2.0, 3.0, 100.0]))
    assert len(cnt) == 5 and cnt.tolist() == [0, 0, 1, 0, 0]
    _, _, _, _, cnt = orc.mean_pv_from_tv(pos, vel, np.array([0.0, 3.0, 6.0, 9.0]))
    assert cnt.tolist() == [1, 0, 0, 2] and len(cnt) == 4          # 10.5 / 3, 10.8 / 3 -> bin 3 = binnr - 1: in reach


def test_empty_bins_are_dropped():
    pos = np.array([[0.0, 0.0, 1000.0], [0.5, 0.0, 1000.0], [0.0, 3.2, 1000.0]])
    vel = np.array([[10.0, -20.0], [30.0, 5.0], [-7.0, 1.0]])
    rsep, pest, nom, den, cnt = orc.mean_pv_from_tv(pos, vel, np.arange(0.0, 10.0, 1.0))
    assert len(rsep) == 10 and cnt.tolist() == [1, 0, 0, 2, 0, 0, 0, 0, 0, 0]
    assert len(pest) == 2
    npt.assert_array_equal(pest, nom[[0, 3]] / den[[0, 3]])


def test_coincident_pair_drops_bin_zero():
    pos = np.array([[1.0, 2.0, 800.0], [1.0, 2.0, 800.0], [1.0, 4.5, 800.0]])
    vel = np.array([[10.0, -20.0], [30.0, 5.0], [-7.0, 1.0]])
    rsep, pest, nom, den, cnt = orc.mean_pv_from_tv(pos, vel, np.arange(0.0, 5.0, 1.0))
    assert cnt.tolist() == [1, 0, 2, 0, 0]
    assert np.isnan(nom[0]) and np.isnan(den[0])
    assert len(pest) == 1 and np.isfinite(pest[0])
