"""CPU-only: the numpy restatement of the Gaussian-random-field generator (tests/grf_oracle.py) on its own - the Philox
known answers, the Hermitian rule of the half plane, the statistics of what it draws, the l cut - and the parts of the
Python interface that need no GPU.  tests/test_gpu_grf.py holds the kernel against this oracle element by element."""
import itertools

import numpy as np
import pytest

from tests import grf_oracle as orc

CL4000 = 1e-9 / (np.arange(4000, dtype=np.float64) + 50.0) ** 2
PAIRS = [(34077, 0), (34077, 1), (7, 0), (7, 1), (20240601, 0)]


@pytest.mark.parametrize("counter, key, words", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, words):
    """The three Philox4x32-10 vectors of Random123's kat_vectors."""
    got = orc.philox4x32_10(*counter, *key)
    assert " ".join(f"{int(w):08x}" for w in got) == words


def test_philox_is_elementwise():
    """An array of counters gives what the counters give one by one."""
    c = np.array([0, 1, 0xffffffff, 12345], dtype=np.uint64)
    many = orc.philox4x32_10(c, c[::-1], 7, c, 34077, 1 << 20)
    for e in range(len(c)):
        one = orc.philox4x32_10(c[e], c[::-1][e], 7, c[e], 34077, 1 << 20)
        assert [int(w[e]) for w in many] == [int(w) for w in one]


@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 9, 64])
def test_half_plane_is_hermitian(n):
    """rfft2(irfft2(ft)) == ft: the half plane is the spectrum of a real map as it stands, and irfft2(ft) is the real part of
    the inverse transform of the full plane built from ft and its conjugates, whose imaginary part is rounding."""
    theta = np.deg2rad(5.0)
    ft, _ = orc.spectrum(n, theta, CL4000, 34077)
    scale = np.abs(ft).max()
    m = np.fft.irfft2(ft, s=(n, n))
    back = np.abs(np.fft.rfft2(m) - ft).max() / scale
    mf = np.fft.ifft2(orc.full_plane(ft, n))
    imag = np.abs(mf.imag).max() / np.abs(mf.real).max()
    diff = np.abs(mf.real - m).max() / np.abs(m).max()
    print(f"n {n}: round trip {back:.3g}, imaginary part {imag:.3g}, half against full plane {diff:.3g} (bound 1e-14)")
    assert back <= 1e-14 and imag <= 1e-14 and diff <= 1e-14
    # the structure itself, exactly
    a, b, real, conj = orc.deviates(n, 34077)
    for j in [0] + ([n // 2] if n % 2 == 0 else []):
        for i in range(n):
            assert ft[i, j] == np.conj(ft[(n - i) % n, j])
    assert (ft.imag[real] == 0.0).all() and real.sum() == (4 if n % 2 == 0 else 1)


def test_binned_power_follows_the_table():
    """z = (sum |ft|^2 / sum A^2 - 1) sqrt(hits) per bin stays within 4 for three seeds and two realisations each; the
    smallest bin holds at least 48 pixels."""
    l = orc.pixel_l(orc.STAT_N, orc.STAT_THETA)
    worst = 0.0
    for seed, real in itertools.product(orc.STAT_SEEDS, (0, 1)):
        ft, A = orc.spectrum(orc.STAT_N, orc.STAT_THETA, orc.STAT_CL, seed, real)
        z, hits = orc.bin_z(np.abs(ft) ** 2, A, l, orc.STAT_EDGES)
        assert hits.min() >= 48
        worst = max(worst, float(np.abs(z).max()))
    print(f"binned power of the oracle: max |z| = {worst:.3g} (bound 4)")
    assert worst <= 4.0


def _whitened(seed, real):
    """The 65 024 deviates behind the columns 1 .. n/2 - 1 (no self-conjugate pixel), recovered from the spectrum."""
    n = orc.STAT_N
    ft, A = orc.spectrum(n, orc.STAT_THETA, orc.STAT_CL, seed, real)
    cols = slice(1, n // 2)
    g = ft[:, cols] * np.sqrt(2.0) / A[:, cols]
    return np.concatenate([g.real.ravel(), g.imag.ravel()])


def test_deviates_are_standard_normal():
    g = {p: _whitened(*p) for p in PAIRS}
    N = 65024
    for p, v in g.items():
        assert v.size == N
        stats = (v.mean() * np.sqrt(N), (v.var() - 1.0) * np.sqrt(N / 2.0), ((v ** 4).mean() - 3.0) * np.sqrt(N / 96.0))
        print(f"seed {p[0]} realisation {p[1]}: mean, variance, fourth moment in sigma: "
              + ", ".join(f"{s:.3g}" for s in stats) + " (bound 4)")
        assert all(abs(s) <= 4.0 for s in stats)
    worst = 0.0
    for p, q in itertools.combinations(PAIRS, 2):
        worst = max(worst, abs(float(np.corrcoef(g[p], g[q])[0, 1])) * np.sqrt(N))
    print(f"correlation between realisations: max |rho| sqrt(N) = {worst:.3g} (bound 4)")
    assert worst <= 4.0


def test_lmax_and_the_end_of_the_table():
    n, theta = 64, np.deg2rad(5.0)
    cl = 1e-9 / (np.arange(2000, dtype=np.float64) + 50.0) ** 2
    l = orc.pixel_l(n, theta)
    ft, A = orc.spectrum(n, theta, cl, 34077, lmax=1500.0)
    assert (l > 1500.0).any() and (l <= 1500.0).any()
    assert (ft[l > 1500.0] == 0.0).all() and (A[l > 1500.0] == 0.0).all()
    assert (ft[l <= 1500.0] != 0.0).all()
    # without lmax the table's last entry is the end: nothing above l = 1999, and no read past the table
    ft, A = orc.spectrum(n, theta, cl, 34077)
    assert (l > 1999.0).any() and (ft[l > 1999.0] == 0.0).all() and (ft[l <= 1999.0] != 0.0).all()
    assert orc.cl_at(np.array([1999.0]), cl)[0] == cl[1999] and orc.cl_at(np.array([0.5]), cl)[0] == cl[0] + 0.5 * (cl[1] - cl[0])


def test_add_cmb_is_refused_off_an_isw_map():
    from astrild_amd.rays.skys.sky_array import SkyArray, SkyArrayWarning
    with pytest.raises(SkyArrayWarning):
        SkyArray.from_array(np.zeros((8, 8)), 10.0, "kappa_2", "").add_cmb("x.npy")


@pytest.mark.parametrize("kw", [
    dict(cl=[1.0, -1.0]), dict(cl=[1.0, float("nan")]), dict(cl=[1.0, float("inf")]), dict(cl=[]), dict(cl=[[1.0, 2.0]]),
    dict(seed=-1), dict(seed=1 << 64), dict(realisation=-1), dict(realisation=1 << 64),
    dict(realisation=(1 << 64) - 2, nreal=3), dict(npix=1), dict(nreal=0), dict(lmax=float("nan")),
])
def test_python_validation_needs_no_gpu(kw):
    """The ValueErrors of lensing.gaussian_random_spectrum are raised before anything touches the device."""
    from astrild_amd import lensing
    args = dict(npix=8, angle_deg=5.0, cl=[1.0, 1.0], seed=1)
    args.update(kw)
    with pytest.raises(ValueError):
        lensing.gaussian_random_spectrum(**args)


def test_cl_table_from_file(tmp_path):
    """Row 1 as it is when row 0 counts 0, 1, 2, ...; otherwise resampled onto integer l, zero outside the range."""
    from astrild_amd.rays.skys.sky_array import SkyArray
    cl = 1.0 / (np.arange(6.0) + 1.0)
    np.save(tmp_path / "a.npy", np.stack([np.arange(6.0), cl]))
    assert np.array_equal(SkyArray._load_cl_table(str(tmp_path / "a.npy")), cl)
    ell = np.array([2.0, 3.5, 6.0])
    np.save(tmp_path / "b.npy", np.stack([ell, [4.0, 1.0, 2.0]]))
    got = SkyArray._load_cl_table(str(tmp_path / "b.npy"))
    assert np.array_equal(got, np.interp(np.arange(7.0), ell, [4.0, 1.0, 2.0], left=0.0, right=0.0))
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] == 4.0 and got[6] == 2.0 and len(got) == 7
