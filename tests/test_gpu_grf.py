"""GPU: the Gaussian-random-field generator (astrild_amd/csrc/grf.hip) against its numpy restatement
(tests/grf_oracle.py) element by element through the C ABI, the maps of lensing.gaussian_random_map against numpy's
inverse transform of the GPU's own spectrum, the measured flat-sky power spectrum of such a map, determinism, batching,
memory discipline, refusals, and SkyArray.create_cmb / add_cmb.  Every comparison prints its worst err / bound."""
import itertools

import numpy as np
import pytest

from tests import grf_oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
NAN = float("nan")
THETA5 = np.deg2rad(5.0)
CL4000 = 1e-9 / (np.arange(4000, dtype=np.float64) + 50.0) ** 2
# (seed, first realisation): small words, and values whose high key and counter words are not zero
STREAMS = [(34077, 0), ((1 << 40) + 3, (1 << 33) + 1)]
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


def _abi():
    from astrild_amd import _lib
    from astrild_amd.device import as_device, ptr, stream
    return _lib, as_device, ptr, stream


def _report(what, ratio):
    print(f"{what}: max err / bound = {ratio:.3g}")
    return ratio


def _spectrum(n, theta, cl, seed, first, nreal, lmax=np.inf, pad=64):
    """(rc, spectra (nreal, n, nh), the pads) of ast_grf_spectrum writing `pad` complex slots inside a NaN-filled
    allocation."""
    _lib, as_device, ptr, stream = _abi()
    nh = n // 2 + 1
    count = nreal * n * nh
    buf = torch.full((count + 2 * pad,), complex(NAN, NAN), dtype=torch.complex128, device="cuda")
    out = buf[pad:pad + count]
    table = as_device(np.ascontiguousarray(cl, dtype=np.float64))
    rc = _lib.lib().ast_grf_spectrum(ptr(out), n, float(theta), ptr(table), len(cl), float(lmax), seed, first, nreal, stream())
    host = buf.cpu().numpy()
    return rc, host[pad:pad + count].reshape(nreal, n, nh), np.concatenate([host[:pad], host[pad + count:]])


# ------------------------------------------------------------------------------- the spectrum against the oracle
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 9, 64, 65])
def test_spectrum_matches_the_oracle(n):
    """Per component |delta| <= 1e-13 A(l), exactly 0 where A = 0.  u1, u2, phi and the interpolation are the same IEEE
    operations on both sides; log, cos and sin differ by at most 2 ulp (device library) + 1 ulp (numpy), so
    |delta a| <~ r 1e-15 <= 9e-15 with r <= sqrt(106 ln 2) = 8.6; 1e-13 leaves a tenfold margin.  With and without a
    cut at lmax = 1500, which n = 64 and 65 reach at 5 degrees (l up to 3258)."""
    _lib = _abi()[0]
    worst = 0.0
    for (seed, first), lmax in itertools.product(STREAMS, (np.inf, 1500.0)):
        rc, got, pads = _spectrum(n, THETA5, CL4000, seed, first, 3, lmax)
        _lib.check(rc, "ast_grf_spectrum")
        assert np.isnan(pads.real).all() and np.isnan(pads.imag).all() and pads.size == 128
        for r in range(3):
            ref, A = orc.spectrum(n, THETA5, CL4000, seed, first + r, lmax)
            zero = A == 0.0
            assert (got[r][zero] == 0.0).all(), (n, seed, r, lmax)
            assert np.isfinite(got[r].real).all() and np.isfinite(got[r].imag).all()
            if (~zero).any():
                err = np.maximum(np.abs(got[r].real - ref.real), np.abs(got[r].imag - ref.imag))[~zero] / (1e-13 * A[~zero])
                worst = max(worst, float(err.max()))
    _report(f"ast_grf_spectrum[n {n}]", worst)
    assert worst <= 1.0


# -------------------------------------------------------------- the map against numpy's inverse of the same spectrum
@pytest.mark.parametrize("n", [2, 3, 8, 9, 64, 65, 256])
def test_map_is_the_inverse_transform_of_the_spectrum(n):
    """Elementwise |delta| <= 4 eps log2(n^2) ||map||_2: the FFT's error bound in the 2-norm, which bounds each element.
    Two realisations in one batched transform, and a single one."""
    from astrild_amd import lensing
    worst = 0.0
    for nreal in (2, 1):
        spec = lensing.gaussian_random_spectrum(n, 5.0, CL4000, 34077, realisation=4, nreal=nreal).cpu().numpy()
        maps = lensing.gaussian_random_map(n, 5.0, CL4000, 34077, realisation=4, nreal=nreal)
        assert tuple(maps.shape) == ((n, n) if nreal == 1 else (nreal, n, n)) and maps.dtype == torch.float64
        maps = maps.cpu().numpy().reshape(nreal, n, n)
        for r in range(nreal):
            ref = np.fft.irfft2(spec[r], s=(n, n))
            bound = 4.0 * EPS * np.log2(float(n) ** 2) * np.linalg.norm(ref)
            assert bound > 0.0
            worst = max(worst, float(np.abs(maps[r] - ref).max() / bound))
    _report(f"gaussian_random_map[n {n}]", worst)
    assert worst <= 1.0


def test_map_into_a_given_tensor():
    from astrild_amd import lensing
    out = torch.full((2, 8, 8), NAN, dtype=torch.float64, device="cuda")
    got = lensing.gaussian_random_map(8, 5.0, CL4000, 3, nreal=2, out=out)
    assert got is out and torch.equal(out, lensing.gaussian_random_map(8, 5.0, CL4000, 3, nreal=2))
    with pytest.raises(ValueError):
        lensing.gaussian_random_map(8, 5.0, CL4000, 3, nreal=2, out=out[0])


# ---------------------------------------------------------------------------------- consistency with the measuring side
def test_measured_power_spectrum_of_the_map():
    """flat_power_spectrum(map) equals the oracle's binned sum |ft|^2 / hits (theta / n^2)^2 to 1e-12 relative - a half
    plane left inconsistent in its self-conjugate columns does not come back from the C2R / R2C round trip - and the
    measured spectrum follows the table: |z| <= 4 in every bin."""
    from astrild_amd import lensing
    n, theta = orc.STAT_N, orc.STAT_THETA
    l = orc.pixel_l(n, theta)
    worst, worst_z = 0.0, 0.0
    for seed, real in ((34077, 0), (7, 1)):
        ft, A = orc.spectrum(n, theta, orc.STAT_CL, seed, real)
        s, hits = orc.binned(np.abs(ft) ** 2, l, orc.STAT_EDGES)
        ref = s / hits * (theta / float(n) ** 2) ** 2
        m = lensing.gaussian_random_map(n, 10.0, orc.STAT_CL, seed, realisation=real)
        centres, power = lensing.flat_power_spectrum(m, 10.0, orc.STAT_EDGES)
        assert np.array_equal(centres, 0.5 * (orc.STAT_EDGES[:-1] + orc.STAT_EDGES[1:]))
        worst = max(worst, float((np.abs(power - ref) / (1e-12 * ref)).max()))
        e, _ = orc.binned(A * A, l, orc.STAT_EDGES)
        z = (power * hits * (float(n) ** 2 / theta) ** 2 / e - 1.0) * np.sqrt(hits)
        worst_z = max(worst_z, float(np.abs(z).max()))
    _report("flat_power_spectrum(gaussian_random_map)[256]", worst)
    print(f"measured spectrum against the table: max |z| = {worst_z:.3g} (bound 4)")
    assert worst <= 1.0 and worst_z <= 4.0


# ------------------------------------------------------------------------------------------ determinism and batching
def test_determinism_and_batching():
    from astrild_amd import lensing
    first = (1 << 33) + 1
    for n in (9, 64):
        a = lensing.gaussian_random_spectrum(n, 5.0, CL4000, 34077, realisation=first, nreal=3)
        b = lensing.gaussian_random_spectrum(n, 5.0, CL4000, 34077, realisation=first, nreal=3)
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))
        ma = lensing.gaussian_random_map(n, 5.0, CL4000, 34077, realisation=first, nreal=3)
        assert torch.equal(ma, lensing.gaussian_random_map(n, 5.0, CL4000, 34077, realisation=first, nreal=3))
        for r in range(3):
            one = lensing.gaussian_random_spectrum(n, 5.0, CL4000, 34077, realisation=first + r)
            assert tuple(one.shape) == (1, n, n // 2 + 1)
            assert torch.equal(torch.view_as_real(one[0]), torch.view_as_real(a[r])), (n, r)
            assert torch.equal(lensing.gaussian_random_map(n, 5.0, CL4000, 34077, realisation=first + r), ma[r]), (n, r)
        assert not torch.equal(ma[0], ma[1])
        other = lensing.gaussian_random_map(n, 5.0, CL4000, 34078, realisation=first, nreal=3)
        assert not torch.equal(other, ma)
    # a launch with more than one block and a tail: the batch is the single calls, whatever the grid
    a = lensing.gaussian_random_spectrum(65, 5.0, CL4000, 7, nreal=3)
    for r in range(3):
        assert torch.equal(torch.view_as_real(lensing.gaussian_random_spectrum(65, 5.0, CL4000, 7, realisation=r)[0]),
                           torch.view_as_real(a[r]))


# ------------------------------------------------------------------------------------------------ memory discipline
def test_every_slot_is_written_and_nothing_else():
    _lib = _abi()[0]
    for n, nreal in ((2, 1), (3, 2), (64, 3), (65, 1)):
        rc, got, pads = _spectrum(n, THETA5, CL4000, 11, 0, nreal, pad=96)
        _lib.check(rc, "ast_grf_spectrum")
        assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
        assert pads.size == 192 and np.isnan(pads.real).all() and np.isnan(pads.imag).all()


def test_zero_table_gives_a_zero_map():
    from astrild_amd import lensing
    _lib = _abi()[0]
    rc, got, _ = _spectrum(9, THETA5, np.zeros(4000), 11, 0, 2)
    _lib.check(rc, "ast_grf_spectrum")
    assert (got == 0.0).all()
    for n in (8, 9):
        m = lensing.gaussian_random_map(n, 5.0, np.zeros(4000), 11, nreal=2)
        assert (m == 0.0).all().item()
    # a one-entry table is C(0) alone: only the mean of the map is drawn
    m = lensing.gaussian_random_map(8, 5.0, [1e-9], 11).cpu().numpy()
    assert m[0, 0] != 0.0 and np.abs(m - m[0, 0]).max() <= 1e-14 * abs(m[0, 0])


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    """Every bad argument set is refused on the host with "bad argument", the output untouched, and a valid call follows."""
    _lib, as_device, ptr, stream = _abi()
    lib = _lib.lib()
    table = as_device(CL4000)
    n = 8
    out = torch.full((n * (n // 2 + 1),), complex(NAN, NAN), dtype=torch.complex128, device="cuda")
    good = dict(spec=ptr(out), npix=n, angle=float(THETA5), cl=ptr(table), ncl=4000, lmax=float("inf"), seed=1, first=0, nreal=1)
    bad = [dict(npix=1), dict(npix=0), dict(npix=-4), dict(angle=0.0), dict(angle=float("inf")), dict(angle=-1.0),
           dict(angle=NAN), dict(ncl=0), dict(nreal=0), dict(nreal=-1), dict(spec=None), dict(cl=None), dict(lmax=NAN)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.ast_grf_spectrum(a["spec"], a["npix"], a["angle"], a["cl"], a["ncl"], a["lmax"], a["seed"], a["first"],
                                  a["nreal"], stream())
        assert rc != 0, change
        assert b"bad argument" in lib.ast_last_error(), change
        torch.cuda.synchronize()
        assert torch.isnan(torch.view_as_real(out)).all().item(), change
        rc, got, _ = _spectrum(n, THETA5, CL4000, 1, 0, 1)
        _lib.check(rc, "ast_grf_spectrum")
        assert np.array_equal(got[0], _spectrum(n, THETA5, CL4000, 1, 0, 1)[1][0])
    from astrild_amd import lensing
    for cl in ([1.0, -1e-30], [1.0, NAN], [float("inf")], [], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            lensing.gaussian_random_map(8, 5.0, cl, 1)
    assert lensing.gaussian_random_map(8, 5.0, [1.0, 2.0], (1 << 64) - 1, realisation=(1 << 64) - 2, nreal=2).shape == (2, 8, 8)


# --------------------------------------------------------------------------------------------------------------- API
def test_create_cmb_and_add_cmb(tmp_path):
    from astrild_amd import lensing
    from astrild_amd.rays.skys.sky_array import SkyArray
    n, angle = 64, 2.0                                                # l up to 8146: both cuts below bite
    cl = 1e-9 / (np.arange(6000, dtype=np.float64) + 50.0) ** 2
    path = str(tmp_path / "cl.npy")
    np.save(path, np.stack([np.arange(6000.0), cl]))
    orig = np.random.default_rng(3).standard_normal((n, n)) * 1e-6
    sky = SkyArray.from_array(orig.copy(), angle, "isw_rs", "")
    assert sky.create_cmb(path) is None
    assert sky.data.resident("cmb") and 0 <= sky.cmb_seed < 1 << 64
    ref = lensing.gaussian_random_map(n, angle, cl, sky.cmb_seed, lmax=3e3).cpu().numpy()
    assert (ref != 0.0).any()
    sky.add_cmb(overwrite=False)
    assert sky.data.resident("orig_cmb")
    assert np.array_equal(sky.data["cmb"], ref)
    assert np.array_equal(sky.data["orig_cmb"], orig + ref) and np.array_equal(sky.data["orig"], orig)
    # the default lmax = 3000 cuts: the uncut field differs
    assert not np.array_equal(lensing.gaussian_random_map(n, angle, cl, sky.cmb_seed).cpu().numpy(), ref)
    # a seed of the caller's, handed back as an array
    got = sky.create_cmb(path, lmax=2000, rnd_seed=5, rtn=True)
    assert sky.cmb_seed == 5 and isinstance(got, np.ndarray)
    assert np.array_equal(got, lensing.gaussian_random_map(n, angle, cl, 5, lmax=2000).cpu().numpy())
    assert np.array_equal(sky.data["cmb"], ref)                       # rtn=True stores nothing
    # a table that starts at l = 2 with uneven steps: resampled onto integer l, zero outside
    ell = np.concatenate([[2.0, 3.5], np.arange(5.0, 3000.0, 2.0)])
    path2 = str(tmp_path / "cl2.npy")
    np.save(path2, np.stack([ell, 1e-9 / (ell + 50.0) ** 2]))
    table = np.interp(np.arange(int(ell[-1]) + 1, dtype=np.float64), ell, 1e-9 / (ell + 50.0) ** 2, left=0.0, right=0.0)
    assert table[0] == 0.0 and table[1] == 0.0 and table[2] > 0.0
    sky2 = SkyArray.from_array(orig.copy(), angle, "isw_rs", "")
    sky2.add_cmb(filepath_cl=path2, rnd_seed=9)                       # lmax None: no cut; overwrites "orig"
    cmb2 = lensing.gaussian_random_map(n, angle, table, 9).cpu().numpy()
    assert sky2.cmb_seed == 9 and np.array_equal(sky2.data["cmb"], cmb2) and np.array_equal(sky2.data["orig"], orig + cmb2)
    # only a stored CMB map
    path3 = str(tmp_path / "cmb.npy")
    np.save(path3, ref)
    sky3 = SkyArray.from_array(orig.copy(), angle, "isw_rs_x", "")
    got = sky3.add_cmb(filepath_cmb=path3, rtn=True)
    assert np.array_equal(got, orig + ref) and np.array_equal(sky3.data["orig"], orig) and "orig_cmb" not in sky3.data
