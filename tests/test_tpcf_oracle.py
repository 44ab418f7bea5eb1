"""CPU: the numpy restatement of the periodic two-point correlation function (tests/tpcf_oracle.py) against scipy's
periodic cKDTree and the analytic RR, the host-side tpcf_multipole, and the argument handling of
astrild_amd.particles.hutils.tpcf, all without a GPU."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import tpcf_oracle as orc

P2 = lambda x: (3.0 * x * x - 1.0) / 2.0            # noqa: E731


def test_product_module_imports_without_a_gpu():
    from astrild_amd.particles.hutils import tpcf as mod
    from astrild_amd.particles.hutils import TPCF, tpcf_multipole, tpcf_r  # noqa: F401
    assert callable(mod.TPCF.compute) and callable(mod.TPCF.tpcf_s)


@pytest.mark.parametrize("seed,kind", [(1, "uniform"), (2, "clustered"), (3, "uniform")])
def test_oracle_cumulative_counts_equal_ckdtree(seed, kind):
    from scipy.spatial import cKDTree
    L = 100.0
    pos = orc.uniform(3000, L, seed) if kind == "uniform" else orc.clustered(3000, L, seed, blobs=20, sigma=3.0)
    r = np.linspace(0.0, 30.0, 13)
    cnt = orc.pair_counts_brute(pos, L, r)
    tree = cKDTree(pos, boxsize=L)
    cum = tree.count_neighbors(tree, r)                 # ordered pairs with d <= r, self pairs included
    npt.assert_array_equal(np.cumsum(cnt), (cum[1:] - len(pos)) // 2)


def test_tree_prefiltered_oracle_equals_brute_force():
    L = 60.0
    pos = orc.clustered(2500, L, 4, blobs=10, sigma=2.0)
    s = np.array([0.0, 0.7, 1.5, 4.0, 9.0, 19.9])
    mu = np.sort(1.0 - np.geomspace(0.01, 1.0, 12))
    for los in (0, 2):
        npt.assert_array_equal(orc.pair_counts(pos, L, s, mu, los=los), orc.pair_counts_brute(pos, L, s, mu, los=los))
    npt.assert_array_equal(orc.pair_counts(pos, L, s), orc.pair_counts_brute(pos, L, s))


def test_oracle_lattice_known_answer():
    s = [0.5, 1.2, 1.6, 1.9, 2.1, 2.5]
    mu = [0.0, 0.25, 0.6, 0.8, 1.0]
    for los in (0, 2):
        exp = orc.lattice_expected(8, s, mu, los, 2.5)
        npt.assert_array_equal(orc.pair_counts_brute(orc.lattice(8), 8.0, s, mu, los=los), exp)
    # |m|^2 = 5: 8 vectors with mu = 2 / sqrt 5 in (0.8, 1], 8 with 1 / sqrt 5 in (0.25, 0.6], 8 with mu = 0 dropped
    per_object = orc.lattice_expected(8, s, mu, 2, 2.5) * 2 // 8 ** 3
    assert per_object.tolist() == [[0, 0, 0, 2], [0, 0, 8, 0], [0, 8, 0, 0], [0, 0, 0, 2], [0, 24, 0, 16]]


def test_rr_sums_to_the_sphere():
    n, L, rmax = 12345, 250.0, 40.0
    s = np.array([0.0, 1.0, 2.5, 7.0, 20.0, rmax])
    mu = np.append(np.sort(1.0 - np.geomspace(0.001, 1.0, 40)), 1.0)      # 0 ... 0.999, 1
    assert mu[0] == 0.0
    total = orc.rr(n, L, s, mu).sum()
    npt.assert_allclose(total, n * n * (4.0 * np.pi / 3.0) * rmax ** 3 / L ** 3, rtol=1e-12)


def test_shift_and_wrap_in_the_input_dtype():
    L = 100.0
    pos = np.array([[1.0, 2.0, 99.9], [1.0, 2.0, 0.05], [3.0, 4.0, 50.0]], dtype=np.float32)
    vel = np.array([[0.0, 0.0, 30.0], [0.0, 0.0, -20.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    out = orc.shift_and_wrap(pos, vel, L)
    z = np.float32(99.9) + np.float32(30.0) / np.float32(100.0) - np.float32(L)
    assert out[0, 2] == np.float64(np.float32(z))
    assert out[1, 2] == np.float64((np.float32(0.05) - np.float32(0.2)) + np.float32(L))
    assert out[2, 2] == np.float64(np.float32(50.01))
    assert out.dtype == np.float64 and np.all(out[:, :2] == pos[:, :2])


def test_multipole_of_constant_and_of_p2():
    from astrild_amd.particles.hutils import tpcf_multipole
    mu = np.linspace(0.0, 1.0, 41)
    c = (mu[:-1] + mu[1:]) / 2.0
    xi = np.full((3, 40), 2.5)
    npt.assert_allclose(tpcf_multipole(xi, mu, 0), 2.5, rtol=1e-14)
    # midpoint rule: the quadrupole of a constant is 5 c sum P2(mu_c) dmu = -c dmu^2 / 4 away from 0
    npt.assert_allclose(tpcf_multipole(xi, mu, 2), 0.0, atol=2.5 * (1 / 40) ** 2)
    xi2 = np.tile(P2(c), (2, 1))
    npt.assert_allclose(tpcf_multipole(xi2, mu, 2), 1.0, atol=5e-3)
    npt.assert_allclose(tpcf_multipole(xi2, mu, 0), 0.0, atol=5e-3)
    for order in (0, 2, 4):
        npt.assert_allclose(tpcf_multipole(xi2, mu, order), orc.multipole(xi2, mu, order), rtol=1e-13, atol=1e-15)


def _capture(monkeypatch):
    """Replace the GPU pair count by a recorder returning zeros, so the host path runs without a GPU."""
    import torch
    from astrild_amd import device as dev
    seen = {}

    def fake(pos, boxsize, s_edges, mu_edges=None, vel=None, los=2):
        seen.update(s=np.asarray(s_edges), mu=None if mu_edges is None else np.asarray(mu_edges), los=los)
        shape = (len(s_edges) - 1, len(mu_edges) - 1) if mu_edges is not None else (len(s_edges) - 1,)
        return torch.zeros(shape, dtype=torch.int64)

    monkeypatch.setattr(dev, "tpcf_pair_counts", fake)
    return seen


def test_compute_tuple_defaults(monkeypatch):
    from astrild_amd.particles.hutils import TPCF
    seen = _capture(monkeypatch)
    pos = orc.uniform(10, 300.0, 1)
    s, mu, xi = TPCF.compute(pos, np.zeros_like(pos), 300.0, "redshift", (0.5, 60.0), (0.001, 1.0))
    npt.assert_array_equal(seen["s"], np.linspace(0.5, 60.0, 40))
    npt.assert_array_equal(seen["mu"], np.sort(1.0 - np.geomspace(0.001, 1.0, 40)))
    assert seen["los"] == 2
    assert len(s) == 39 and xi.shape == (39, 39) and len(mu) == 40
    npt.assert_array_equal(s, (seen["s"][1:] + seen["s"][:-1]) / 2.0)
    npt.assert_array_equal(xi, -1.0)
    TPCF.compute(pos, np.zeros_like(pos), 300.0, "real", (0.5, 60.0), (0.001, 1.0), los=0)
    assert seen["los"] == 0
    _, _, _, dd = TPCF.compute(pos, pos, 300.0, "redshift", np.array([1.0, 2.0]), np.array([0.0, 1.0]),
                               return_counts=True)
    assert dd.dtype == np.int64 and dd.shape == (1, 1)


@pytest.mark.parametrize("kwargs", [
    dict(s=np.array([0.0, 10.0, 100.0])),                       # rmax >= L / 3 (L = 300)
    dict(s=np.array([0.0, 10.0, 99.99999]), L=299.9999),
    dict(mu=np.array([0.0, 0.5, 1.2])),                         # mu outside [0, 1]
    dict(mu=np.array([-0.1, 0.5, 1.0])),
    dict(s=np.array([0.0, 20.0, 10.0])),                        # unsorted
    dict(mu=np.array([0.0, 0.6, 0.5, 1.0])),
    dict(s=np.array([-1.0, 10.0])),                             # negative s
    dict(s=np.array([0.0, 10.0, 10.0])),                        # repeated edge
    dict(los=3),
])
def test_value_errors_before_any_gpu_call(kwargs):
    from astrild_amd.particles.hutils import TPCF
    L = kwargs.get("L", 300.0)
    s = kwargs.get("s", np.linspace(0.0, 50.0, 11))
    mu = kwargs.get("mu", np.linspace(0.0, 1.0, 5))
    pos = orc.uniform(10, 299.0, 1)
    with pytest.raises(ValueError):
        TPCF.compute(pos, np.zeros_like(pos), L, "redshift", s, mu, los=kwargs.get("los"))
    with pytest.raises(ValueError):
        TPCF.tpcf_s(pos, np.zeros_like(pos), s, mu, kwargs.get("los", 2), L)


def test_tpcf_r_estimators(monkeypatch):
    from astrild_amd.particles.hutils import tpcf_r
    pos = orc.uniform(10, 300.0, 1)
    with pytest.raises(ValueError):
        tpcf_r(pos, np.linspace(1.0, 50.0, 10), 300.0, estimator="Peebles-Hauser")
    with pytest.raises(ValueError):
        tpcf_r(pos, np.linspace(1.0, 150.0, 10), 300.0)
    seen = _capture(monkeypatch)
    for est in ("Natural", "Davis-Peebles", "Hewett", "Hamilton", "Landy-Szalay"):
        xi = tpcf_r(pos, np.linspace(1.0, 50.0, 10), 300.0, estimator=est)
        assert xi.shape == (9,) and seen["mu"] is None
