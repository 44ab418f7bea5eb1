"""CPU-only: the rules of the (k, mu) / multipole binning as tests/fftpower2d_oracle.py restates them - half lattice
with Hermitian weights against brute-force counts on the full lattice, the line of sight's symmetry, the sum over mu
against the 1-D oracle, constant and mu^2 spectra - and device.check_fftpower_2d_args."""
import numpy as np
import pytest

from oracle import fftpower as offt
from tests import fftpower2d_oracle as o2

L = 100.0


@pytest.fixture(scope="module")
def full_counts():
    cache = {}

    def get(n, Nmu, los):
        if (n, Nmu, los) not in cache:
            cache[n, Nmu, los] = o2.full_lattice_counts(n, Nmu, los)
        return cache[n, Nmu, los]
    return get


@pytest.mark.parametrize("n", [8, 16, 32])
@pytest.mark.parametrize("Nmu", [1, 4, 5, 7, 50])
def test_half_lattice_with_weights_equals_full_lattice_counts(full_counts, n, Nmu):
    for los in (0, 1, 2):
        got = o2.project_2d(None, n, L, Nmu, los, binning="integer")["modes"]
        np.testing.assert_array_equal(got, full_counts(n, Nmu, los))


@pytest.mark.parametrize("n,Nmu", [(8, 5), (16, 7), (32, 5), (32, 50)])
def test_counts_do_not_depend_on_the_axis(full_counts, n, Nmu):
    np.testing.assert_array_equal(full_counts(n, Nmu, 0), full_counts(n, Nmu, 2))
    half = [o2.project_2d(None, n, L, Nmu, los, binning="integer")["modes"] for los in (0, 1, 2)]
    np.testing.assert_array_equal(half[0], half[2])
    np.testing.assert_array_equal(half[1], half[2])


@pytest.mark.parametrize("binning", ["integer", "float64"])
@pytest.mark.parametrize("n,Nmu,los", [(16, 5, 2), (32, 7, 0), (32, 5, 1)])
def test_sum_over_mu_is_the_1d_projection(binning, n, Nmu, los):
    rng = np.random.default_rng(11)
    p = rng.standard_normal((n, n, n // 2 + 1))
    s = o2.project_2d(p, n, L, Nmu, los, binning=binning)
    ksum, psum, modes = offt.project_1d(p, n, L, binning)
    np.testing.assert_array_equal(s["modes"].sum(axis=1), modes)
    np.testing.assert_allclose(s["psum"].sum(axis=1), psum.real, rtol=0, atol=1e-12 * s["abs_psum"].sum(axis=1).max())
    np.testing.assert_allclose(s["ksum"].sum(axis=1), ksum, rtol=1e-13)
    np.testing.assert_allclose(s["polesum"][0], psum.real, rtol=0, atol=1e-12 * s["abs_psum"].sum(axis=1).max())


def test_on_edge_vectors_exist_at_nmu_5_and_not_at_4():
    """3-4-5 triples put mu = 3/5 and 4/5 exactly on the edges of 5 bins: 48 kept vectors at n = 32."""
    for los in (0, 1, 2):
        count, rows = o2.on_edge_modes(32, 5, los)
        assert count == 48 and set(rows[:, 3]) == {3, 4}
        assert o2.on_edge_modes(32, 4, los)[0] == 0
        m2 = (rows[:, :3] ** 2).sum(axis=1)
        np.testing.assert_array_equal(o2.mu_bin_index(m2, np.abs(rows[:, los]), 5), rows[:, 3])


@pytest.mark.parametrize("los", [0, 1, 2])
def test_constant_spectrum_gives_constant_wedges_and_monopole(los):
    n, Nmu, A = 16, 5, 3.25
    r = o2.finish(o2.project_2d(np.full((n, n, n // 2 + 1), A), n, L, Nmu, los, poles=(0, 2), binning="integer"), (0, 2))
    filled = r["modes"] > 0
    np.testing.assert_allclose(r["power"][filled], A, rtol=1e-14)
    assert np.all(np.isnan(r["power"][~filled]))
    np.testing.assert_allclose(r["poles"]["power_0"], A, rtol=1e-14)


@pytest.mark.parametrize("n", [16, 32])
def test_mu_squared_spectrum_has_monopole_one_third(n):
    """P = mu^2 = m_los^2 / |m|^2: summed over a whole shell of the cubic lattice, each axis carries a third."""
    f = offt._freq_int(n).astype(np.float64)
    mz = np.arange(n // 2 + 1, dtype=np.float64)
    m2 = f[:, None, None] ** 2 + f[None, :, None] ** 2 + mz[None, None, :] ** 2
    m2[0, 0, 0] = 1.0
    worst = 0.0
    for los in (0, 1, 2):
        a2 = np.broadcast_to((f[:, None, None] ** 2, f[None, :, None] ** 2, mz[None, None, :] ** 2)[los], m2.shape)
        r = o2.finish(o2.project_2d(a2 / m2, n, L, 5, los, poles=(0,), binning="integer"), (0,))
        worst = max(worst, np.abs(r["poles"]["power_0"] - 1.0 / 3.0).max())
    print("max |P0 - 1/3| at n = %d: %.3g" % (n, worst))
    assert worst <= 1e-14


def test_check_fftpower_2d_args():
    from astrild_amd.device import check_fftpower_2d_args as chk
    assert chk(5, 2, (0, 2, 4)) == (5, 2, (0, 2, 4))
    assert chk(1, 0, [0, 2, 4, 6, 8]) == (1, 0, (0, 2, 4, 6, 8))
    assert chk(np.int64(1024), np.int32(1), ()) == (1024, 1, ())
    for bad in (dict(poles=(1,)), dict(los=3), dict(Nmu=0), dict(Nmu=1025), dict(los=-1), dict(poles=(0, 0)),
                dict(poles=(10,)), dict(Nmu=2.5), dict(poles=(0, 3))):
        args = dict(Nmu=5, los=2, poles=(0, 2, 4))
        args.update(bad)
        with pytest.raises(ValueError):
            chk(**args)
