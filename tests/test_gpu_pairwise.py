"""GPU: the transverse-velocity pairwise estimator (ast_pairwise_tv_prepare / ast_pairwise_tv, through
device.pairwise_tv and astrild_amd.particles.hutils.mean_pv_from_tv) against the reference's known answers and the
numpy oracle (tests/pairwise_oracle.py): per-bin pair counts exactly, the sums to rtol 1e-10."""
import json
import os

import numpy as np
import numpy.testing as npt
import pytest

from tests import pairwise_oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairwise_known_answers.json")
RTOL = 1e-10


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


def coherent_velocities(pos, seed, noise=50.0):
    """RA / DEC velocities with a pairwise signal (infall towards the catalogue's centre) under noise, so that the
    per-bin sums do not cancel to rounding level."""
    rng = np.random.default_rng(seed)
    return -0.5 * (pos[:, :2] - pos[:, :2].mean(axis=0)) + rng.normal(0.0, noise, (len(pos), 2))


def gpu_sums(pos, vel, binnr, binwidth, theta1=None, theta2=None):
    from astrild_amd import device as dev
    nom, den, cnt = dev.pairwise_tv(pos, vel, binnr, binwidth, theta1=theta1, theta2=theta2)
    return dev.to_numpy(nom), dev.to_numpy(den), dev.to_numpy(cnt)


def oracle_sums(pos, vel, binnr, binwidth, theta1=None, theta2=None):
    u, t = orc.angles_and_velocities(pos, vel, theta1, theta2)
    return orc.pair_sums(pos, u, t, binnr, binwidth)


def assert_same(got, ref, rtol=RTOL):
    npt.assert_array_equal(got[2], ref[2])
    npt.assert_allclose(got[0], ref[0], rtol=rtol, atol=0)
    npt.assert_allclose(got[1], ref[1], rtol=rtol, atol=0)


def test_known_answers():
    from astrild_amd.particles.hutils import mean_pv_from_tv
    with open(GOLDEN) as f:
        spec = json.load(f)
    pos, vel, bins = orc.known_answer_catalogue(spec)
    rsep, vij = mean_pv_from_tv(pos_cart=pos, vel_ang=vel, bins=bins, multithreading=False)
    k = spec["mean_pv_from_tv"]
    assert len(vij) == k["len"] == 40 and len(rsep) == 40
    npt.assert_almost_equal(vij[0], k["first"], decimal=k["decimal"])
    npt.assert_almost_equal(vij[-1], k["last"], decimal=k["decimal"])
    _, _, cnt = mean_pv_from_tv(pos, vel, bins, return_counts=True)
    npt.assert_array_equal(cnt, oracle_sums(pos, vel, len(bins), np.diff(bins)[0])[2])


@pytest.mark.parametrize("shape", ["compact", "light_cone"])
def test_random_catalogues_against_oracle(shape):
    rng = np.random.default_rng(11)
    if shape == "compact":
        pos = rng.uniform(-20.0, 20.0, (3000, 3)) + np.array([30.0, -10.0, 1200.0])
        bins = np.linspace(0.0, 30.0, 16)                # reach 32: nearly every pair
    else:
        pos, _ = orc.light_cone(6000, seed=5, clusters=300, sigma=8.0)
        bins = np.linspace(0.0, 50.0, 40)                # the reference's bins, reach 51.28
    vel = coherent_velocities(pos, 3)
    binnr, bw = len(bins), float(np.diff(bins)[0])
    assert_same(gpu_sums(pos, vel, binnr, bw), oracle_sums(pos, vel, binnr, bw))
    # given angles, radians and degrees (max > 2 pi)
    th1 = np.arctan2(pos[:, 0], pos[:, 2]) + 0.3
    th2 = np.arctan2(pos[:, 1], np.hypot(pos[:, 0], pos[:, 2])) + 0.2
    assert_same(gpu_sums(pos, vel, binnr, bw, th1, th2), oracle_sums(pos, vel, binnr, bw, th1, th2))
    d1, d2 = np.rad2deg(th1) + 360.0, np.rad2deg(th2)
    assert np.max(d1) > 2 * np.pi
    assert_same(gpu_sums(pos, vel, binnr, bw, d1, d2), oracle_sums(pos, vel, binnr, bw, d1, d2))


def test_lattice_bin_edges_exact():
    # integer lattice, binwidth 2: separations 2, 4, 6 ... sit exactly on bin edges
    g = np.arange(12.0)
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + np.array([-6.0, 4.0, 1000.0])
    vel = coherent_velocities(pos, 4)
    got, ref = gpu_sums(pos, vel, 8, 2.0), oracle_sums(pos, vel, 8, 2.0)
    assert_same(got, ref)
    assert ref[2][1] > 0 and ref[2][7] > 0


@pytest.mark.parametrize("cells", ["1", "0"])
def test_reach_edge_at_large_radius(cells, monkeypatch):
    # binwidth 4, 10 bins: reach 40.  At |r| ~ 3000, a pair 1e-9 inside the reach is counted (bin 9), one 1e-9
    # outside is not; two such groups 600 apart so that the grid has several cells.
    monkeypatch.setenv("ASTRILD_PV_CELLS", cells)
    eps, rmax = 1e-9, 40.0
    pos = []
    for x0 in (0.0, 600.0):
        pos += [[x0, 0.0, 3000.0], [x0, 0.0, 3000.0 + rmax - eps], [x0, 0.0, 3000.0 - rmax - eps]]
    pos = np.array(pos)
    vel = coherent_velocities(pos, 6)
    got, ref = gpu_sums(pos, vel, 10, 4.0), oracle_sums(pos, vel, 10, 4.0)
    assert ref[2].tolist() == [0] * 9 + [2]
    assert_same(got, ref)


def test_grid_equals_single_cell_above_the_reference_cap(monkeypatch):
    pos, _ = orc.light_cone(200_000, seed=21, clusters=2000, sigma=4.0)
    vel = coherent_velocities(pos, 8)
    bins = np.linspace(0.0, 50.0, 40)
    binnr, bw = len(bins), float(np.diff(bins)[0])
    grid = gpu_sums(pos, vel, binnr, bw)
    monkeypatch.setenv("ASTRILD_PV_CELLS", "0")
    single = gpu_sums(pos, vel, binnr, bw)
    assert_same(grid, single)
    assert grid[2].sum() > 5_000_000
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return                                              # the grid-vs-single-cell check above stands alone
    # cumulative counts: pairs with int(d / bw) <= b, i.e. d < (b + 1) bw (no pair sits on an edge here)
    sample = pos[:50_000]
    tree = cKDTree(sample)
    ordered = tree.count_neighbors(tree, bw * np.arange(1, binnr + 1))
    sub = gpu_sums(sample, vel[:50_000], binnr, bw)[2]
    npt.assert_array_equal(np.cumsum(sub), (ordered - len(sample)) // 2)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_tensor_inputs(dtype):
    pos, _ = orc.light_cone(4000, seed=9, clusters=200, sigma=6.0)
    pos = pos.astype(dtype)
    vel = coherent_velocities(pos.astype(np.float64), 2).astype(dtype)
    host = gpu_sums(pos, vel, 40, 50.0 / 39)
    dev_in = gpu_sums(torch.from_numpy(pos).cuda(), torch.from_numpy(vel).cuda(), 40, 50.0 / 39)
    assert_same(dev_in, host, rtol=1e-14)
    assert_same(host, oracle_sums(pos.astype(np.float64), vel.astype(np.float64), 40, 50.0 / 39))


@pytest.mark.parametrize("n", [0, 1])
def test_fewer_than_two_objects(n):
    from astrild_amd.particles.hutils import mean_pv_from_tv
    pos = np.full((n, 3), 1000.0)
    vel = np.ones((n, 2))
    nom, den, cnt = gpu_sums(pos, vel, 40, 1.25)
    assert not nom.any() and not den.any() and not cnt.any() and len(cnt) == 40
    rsep, pest = mean_pv_from_tv(pos, vel, np.linspace(0.0, 50.0, 40))
    assert len(rsep) == 40 and len(pest) == 0
    torch.cuda.synchronize()


def test_repeat_stability():
    pos, _ = orc.light_cone(20_000, seed=13, clusters=500, sigma=5.0)
    vel = coherent_velocities(pos, 1)
    a, b = gpu_sums(pos, vel, 40, 50.0 / 39), gpu_sums(pos, vel, 40, 50.0 / 39)
    assert_same(a, b, rtol=1e-14)
