"""GPU: P(k, mu) wedges and multipoles of the 3D spectrum (ast_power_bin_2d, device.fftpower_2d / catalog_power_2d,
PowerSpectrum3D mode "2d") and the redshift-space shift (ast_rsd_shift) against tests/fftpower2d_oracle.py.

Tolerance of a sum of w P over a bin (``check_sums``): 1e-11 x the bin's sum of w |P| - at most 5e4 modes per bin at
n = 128 times the 1.1e-16 of a double add, plus a few ulp of the Legendre recurrence; a multipole P_l carries the factor
2l + 1 on both sides."""
import importlib.util
import os
import subprocess
import sys
import types

import numpy as np
import numpy.testing as npt
import pandas as pd
import pytest

from oracle import fftpower as offt
from tests import fftpower2d_oracle as o2

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 100.0
POLES5 = (0, 2, 4, 6, 8)
CHILD_SEED = 77


@pytest.fixture(scope="module")
def dev(hip):
    from astrild_amd import device
    torch.cuda.set_device(0)
    return device


def random_spectrum(n, seed, dtype=np.complex128):
    """A random half spectrum built on the host; complex64 values are what both the device and the oracle see."""
    rng = np.random.default_rng(seed)
    shape = (n, n, n // 2 + 1)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


_spectra = {}


def spectra(n, dtype):
    if (n, dtype) not in _spectra:
        _spectra[n, dtype] = (random_spectrum(n, 100 + n, dtype), random_spectrum(n, 200 + n, dtype))
    return _spectra[n, dtype]


def check_sums(got, ref, npoles):
    """got: device.power_bin_2d's tuple; ref: project_2d's sums for POLES5 (a prefix of them was asked of the device)."""
    ksum, musum, psum, nmodes, polesum = (t.cpu().numpy() for t in got)
    npt.assert_array_equal(nmodes, ref["modes"])
    npt.assert_allclose(ksum, ref["ksum"], rtol=1e-12)
    npt.assert_allclose(musum, ref["musum"], rtol=1e-12, atol=0)
    err = np.abs(psum - ref["psum"])
    tol = 1e-11 * ref["abs_psum"]
    assert np.all(err <= tol), ("wedges", (err - tol).max())
    err = np.abs(polesum - ref["polesum"][:npoles])
    tol = 1e-11 * ref["abs_psum"].sum(axis=1)[None, :]          # (2l + 1) on both sides of P_l's tolerance
    assert np.all(err <= tol), ("poles", (err - tol).max())


# ------------------------------------------------------------------ 1, 2: geometry
@pytest.mark.parametrize("n", [8, 16, 32])
def test_geometry_counts_are_the_full_lattice_counts(dev, n):
    for Nmu in (1, 5, 7):
        for los in (0, 1, 2):
            ksum, musum, nmodes = (t.cpu().numpy() for t in dev.shell_geometry_2d(n, L, Nmu, los, binning="integer"))
            assert nmodes.dtype == np.int64 and nmodes.shape == (n // 2 - 1, Nmu)
            npt.assert_array_equal(nmodes, o2.full_lattice_counts(n, Nmu, los))
            ref = o2.project_2d(None, n, L, Nmu, los, binning="integer")
            with np.errstate(invalid="ignore", divide="ignore"):
                k, mu = ksum / nmodes, musum / nmodes
                kr, mur = ref["ksum"] / ref["modes"], ref["musum"] / ref["modes"]
            npt.assert_array_equal(np.isnan(k), np.isnan(kr))
            npt.assert_array_equal(np.isnan(mu), np.isnan(mur))
            npt.assert_allclose(k, kr, rtol=1e-12)
            npt.assert_allclose(mu, mur, rtol=1e-12)
    if n == 8:                       # 3 shells, a 5-element half axis: most (shell, mu) bins are empty
        nm = dev.shell_geometry_2d(8, L, 7, 2, binning="integer")[2].cpu().numpy()
        assert (nm == 0).sum() > 0


@pytest.mark.parametrize("los", [0, 1, 2])
def test_on_edge_vectors_open_the_bin_they_sit_on(dev, los):
    """n = 32, Nmu = 5: the 48 kept vectors with mu = 3/5 or 4/5 exactly.  A spectrum that is 1 on them and 0 elsewhere
    (box side 1: the sums are small integers, exact) must put them into bins 3 and 4 of their shells."""
    n, Nmu = 32, 5
    count, rows = o2.on_edge_modes(n, Nmu, los)
    assert count == 48
    spec = np.zeros((n, n, n // 2 + 1), dtype=np.complex128)
    expect = np.zeros((n // 2 - 1, Nmu))
    for m0, m1, m2, j in rows:
        if m2 < 0:
            m0, m1, m2 = -m0, -m1, -m2
        spec[m0 % n, m1 % n, m2] = 1.0
        expect[int(offt.isqrt_array(np.array([m0 * m0 + m1 * m1 + m2 * m2]))[0]) - 1, j] += 1.0
    assert expect.sum() == 48
    _, _, psum, nmodes, polesum = dev.power_bin_2d(dev.as_device(spec), None, n, 1.0, Nmu, los, (0,), binning="integer")
    npt.assert_array_equal(psum.cpu().numpy(), expect)
    npt.assert_array_equal(polesum.cpu().numpy()[0], expect.sum(axis=1))
    npt.assert_array_equal(nmodes.cpu().numpy(), o2.full_lattice_counts(n, Nmu, los))


# ------------------------------------------------------------------ 3: the data pass
@pytest.mark.parametrize("los", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("n", [16, 64, 128])
def test_data_pass_against_the_oracle(dev, n, dtype, los):
    """n = 16: half axis 9 < 64 lanes; n = 128: half axis 65, lane 0 takes a second element.  Auto and cross, both
    sets of poles, both binning rules."""
    h1, h2 = spectra(n, dtype)
    d1, d2 = dev.as_device(h1), dev.as_device(h2)
    Nmu = 5
    for binning in ("integer", "float64"):
        for cross in (False, True):
            ref = o2.project_2d(o2.p3d(h1, h2 if cross else None, L), n, L, Nmu, los, POLES5, binning)
            for poles in ((0, 2, 4), POLES5):
                got = dev.power_bin_2d(d1, d2 if cross else None, n, L, Nmu, los, poles, binning=binning)
                check_sums(got, ref, len(poles))


# ------------------------------------------------------------------ 4: ties to the 1-D kernel
@pytest.mark.parametrize("binning", ["integer", "float64"])
def test_sum_over_mu_is_the_1d_kernel(dev, binning):
    """Auto spectrum: the wedge sums added over mu are power_bin_1d's psum and P_0 is its power, both at rtol 1e-12 and
    nothing else (sums of positive terms: at most 6e3 adds of 1.1e-16 per shell at n = 64).  The cross spectrum is an
    extra case: its shell sums cancel, and the round-off of a double sum scales with the sum of |terms|, not with the
    result - so there, and only there, an absolute term per shell of 1e-11 x that shell's own sum of w |P| (the
    oracle's, the tolerance of the data-pass test) stands beside the rtol."""
    n, Nmu = 64, 5
    h1, h2 = spectra(n, np.complex128)
    d1, d2 = dev.as_device(h1), dev.as_device(h2)
    for second in (None, d2):
        t1 = dev.power_bin_1d(d1, second, n, L, binning=binning)
        psum1, nmodes1 = t1[1].cpu().numpy(), t1[2].cpu().numpy()
        r1 = dev.finish_power(*t1)
        sums = dev.power_bin_2d(d1, second, n, L, Nmu, 1, (0, 2), binning=binning)
        r2 = dev.finish_power_2d(*sums, poles=(0, 2))
        atol = 0.0
        if second is not None:
            ref = o2.project_2d(o2.p3d(h1, h2, L), n, L, Nmu, 1, (0,), binning)
            atol = 1e-11 * ref["abs_psum"].sum(axis=1)
        got = sums[2].cpu().numpy().sum(axis=1)
        assert np.all(np.abs(got - psum1) <= 1e-12 * np.abs(psum1) + atol), np.abs(got / psum1 - 1).max()
        p0 = r2["poles"]["power_0"]
        assert np.all(np.abs(p0 - r1["power"]) <= 1e-12 * np.abs(r1["power"]) + atol / nmodes1), np.abs(p0 / r1["power"] - 1).max()
        npt.assert_array_equal(r2["poles"]["modes"], r1["modes"])
        npt.assert_allclose(r2["poles"]["k"], r1["k"], rtol=1e-12)
    one = dev.shell_geometry_2d(n, L, 1, 0, binning=binning)[2].cpu().numpy()
    npt.assert_array_equal(one[:, 0], dev.shell_geometry(n, L, binning=binning)[1].cpu().numpy())


# ------------------------------------------------------------------ 5: plane wave, r2c + binning
@pytest.mark.parametrize("los,mu,mubin", [(0, 0.6, 3), (1, 0.8, 4), (2, 0.0, 0)])
def test_plane_wave_lands_in_one_cell(dev, los, mu, mubin):
    """cos(2 pi (3 x + 4 y) / n): delta_k = 1/2 at +-(3, 4, 0), |m| = 5 (shell 4 by the integer rule), mu = 3/5, 4/5, 0."""
    n, Nmu = 32, 5
    x = np.arange(n)
    grid = np.cos(2 * np.pi * (3 * x[:, None, None] + 4 * x[None, :, None] + 0 * x[None, None, :]) / n)
    r = dev.fftpower_2d(dev.as_device(grid), L, Nmu=Nmu, los=los, poles=(0, 2), binning="integer")
    psum = np.where(r["modes"] > 0, r["power"] * r["modes"], 0.0)
    total = 2 * 0.25 * L ** 3
    npt.assert_allclose(psum[4, mubin], total, rtol=1e-12)
    rest = psum.copy()
    rest[4, mubin] = 0.0
    assert np.abs(rest).max() <= 1e-12 * total
    npt.assert_allclose(r["power"][4, mubin], total / r["modes"][4, mubin], rtol=1e-12)
    if mubin == 0:
        assert r["mu"][4, 0] < 0.2
    assert r["modes"][4, mubin] == o2.full_lattice_counts(n, Nmu, los)[4, mubin]
    p0 = np.zeros(n // 2 - 1)
    p0[4] = total / r["poles"]["modes"][4]
    npt.assert_allclose(r["poles"]["power_0"], p0, rtol=1e-12, atol=1e-12 * p0[4])
    p2 = 5 * 0.5 * (3 * mu * mu - 1) * p0[4]
    npt.assert_allclose(r["poles"]["power_2"][4], p2, rtol=1e-12)


# ------------------------------------------------------------------ 6: blocks add
def test_blocks_accumulate_into_the_whole(dev):
    n, Nmu, los = 32, 5, 0
    h1, h2 = random_spectrum(n, 61), random_spectrum(n, 62)
    ref = o2.project_2d(o2.p3d(h1, h2, L), n, L, Nmu, los, POLES5, "float64")
    psum = polesum = None
    geo = [np.zeros((n // 2 - 1, Nmu)), np.zeros((n // 2 - 1, Nmu)), np.zeros((n // 2 - 1, Nmu), dtype=np.int64)]
    for lo, cnt in ((0, 13), (13, 19)):
        b1, b2 = (dev.as_device(np.ascontiguousarray(h[lo:lo + cnt])) for h in (h1, h2))
        ksum, musum, psum, nmodes, polesum = dev.power_bin_2d(b1, b2, n, L, Nmu, los, POLES5, i0=(lo, cnt), i1=(0, n),
                                                              psum=psum, polesum=polesum, binning="float64")
        part = o2.project_2d(None, n, L, Nmu, los, binning="float64", i0=(lo, cnt), i1=(0, n))
        npt.assert_array_equal(nmodes.cpu().numpy(), part["modes"])
        for acc, t in zip(geo, (ksum, musum, nmodes)):
            acc += t.cpu().numpy()
    ksum, musum, nmodes = (torch.from_numpy(g) for g in geo)
    check_sums((ksum, musum, psum, nmodes, polesum), ref, 5)
    whole = dev.power_bin_2d(dev.as_device(h1), dev.as_device(h2), n, L, Nmu, los, POLES5, binning="float64")
    npt.assert_array_equal(geo[2], whole[3].cpu().numpy())
    for mine, theirs, scale in ((psum, whole[2], ref["abs_psum"]), (polesum, whole[4], ref["abs_psum"].sum(axis=1)[None, :])):
        assert np.all(np.abs(mine.cpu().numpy() - theirs.cpu().numpy()) <= 1e-11 * scale)


# ------------------------------------------------------------------ 7: both table paths
def test_tables_beyond_the_lds_budget_take_the_global_path(dev, hip):
    n, Nmu, los = 128, 400, 2
    assert hip.ast_power_bin_2d_lds_fits(n, Nmu, 3) == 0
    assert hip.ast_power_bin_2d_lds_fits(n, 5, 3) == 1 and hip.ast_power_bin_2d_lds_fits(64, 5, 3) == 1
    assert hip.ast_power_bin_2d_lds_fits(n, 0, 3) == 0 and hip.ast_power_bin_2d_lds_fits(n, 5, 6) == 0
    h1, _ = spectra(n, np.complex128)
    ref = o2.project_2d(o2.p3d(h1, None, L), n, L, Nmu, los, (0, 2, 4), "float64")
    dev.profile_enable(True)
    try:
        got = dev.power_bin_2d(dev.as_device(h1), None, n, L, Nmu, los, (0, 2, 4), binning="float64")
        sites = dev.profile_report()
    finally:
        dev.profile_enable(False)
    assert sites["power_bin_2d_global"][0] == 1 and "power_bin_2d" not in sites         # the launch sites name the variant
    assert "wedge_geometry" not in sites
    check_sums(got, ref, 3)


CHILD = """
import sys
import numpy as np
import torch
sys.path.insert(0, {root!r})
from astrild_amd import device as dev
from tests.test_gpu_fftpower2d import random_spectrum, CHILD_SEED
torch.cuda.set_device(0)
h1 = random_spectrum(64, CHILD_SEED)
h2 = random_spectrum(64, CHILD_SEED + 1, np.complex64)
out = {{}}
dev.profile_enable(True)
for name, h in (("f64", h1), ("f32", h2)):
    sums = dev.power_bin_2d(dev.as_device(h), None, 64, {L!r}, 5, 0, (0, 2, 4), binning="float64")
    for key, t in zip(("ksum", "musum", "psum", "modes", "polesum"), sums):
        out[name + "_" + key] = t.cpu().numpy()
out["sites"] = np.array(sorted(name + ":%d" % calls for name, (calls, ms) in dev.profile_report().items()))
np.savez({out!r}, **out)
"""


def test_forced_global_path_agrees_with_the_lds_path(dev, tmp_path):
    """ASTRILD_PK2D_LDS=0 in a fresh process: same counts, sums within the tolerance of the data pass."""
    out = str(tmp_path / "global.npz")
    env = dict(os.environ, ASTRILD_PK2D_LDS="0")
    subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, L=L, out=out)], check=True, env=env, cwd=ROOT, timeout=300)
    child = np.load(out)
    # the launch sites the child went through name the variant: both data passes and the one geometry pass in global memory
    assert list(child["sites"]) == ["power_bin_2d_global:2", "wedge_geometry_global:1"]
    dev.profile_enable(True)
    dev.power_bin_2d(dev.as_device(random_spectrum(64, CHILD_SEED)), None, 64, L, 5, 0, (0, 2, 4), binning="float64")
    here_sites = dev.profile_report()
    dev.profile_enable(False)
    assert "power_bin_2d" in here_sites and "power_bin_2d_global" not in here_sites
    for name, h in (("f64", random_spectrum(64, CHILD_SEED)), ("f32", random_spectrum(64, CHILD_SEED + 1, np.complex64))):
        ref = o2.project_2d(o2.p3d(h, None, L), 64, L, 5, 0, POLES5, "float64")
        here = dev.power_bin_2d(dev.as_device(h), None, 64, L, 5, 0, (0, 2, 4), binning="float64")
        there = tuple(torch.from_numpy(child[name + "_" + key]) for key in ("ksum", "musum", "psum", "modes", "polesum"))
        check_sums(here, ref, 3)
        check_sums(there, ref, 3)
        npt.assert_array_equal(here[3].cpu().numpy(), there[3].numpy())


# ------------------------------------------------------------------ 8: rsd_shift
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rsd_shift(dev, hip, dtype):
    """One wrap into [0, L), never L itself; like TPCF a shift that one wrap does not bring back is a ValueError."""
    rng = np.random.default_rng(5)
    t = dtype
    box = 100.0
    npart = 1000                                  # not a multiple of the 256-thread block
    pos = rng.uniform(0, box, size=(npart, 3)).astype(t)
    vel = rng.uniform(-3000, 3000, size=(npart, 3)).astype(t)
    tiny = 1e-7 if t == np.float32 else 1e-15     # 0.01 * tiny is far below half an ulp of L
    for los in (0, 1, 2):
        pos[0, los], vel[0, los] = np.nextafter(t(box), t(0)), 50.0          # L - tiny, pushed out
        pos[1, los], vel[1, los] = 0.0, -tiny                                # 0 + (-tiny) + L rounds to L
        pos[2, los], vel[2, los] = 0.0, -1.0
        pos[3, los], vel[3, los] = np.nextafter(t(box), t(0)), 0.0
    ulp = float(np.spacing(t(box)))
    for los in (0, 1, 2):
        got = dev.rsd_shift(dev.as_device(pos), dev.as_device(vel), box, los=los).cpu().numpy()
        assert got.dtype == t
        s = pos[:, los].astype(np.float64) + 0.01 * vel[:, los].astype(np.float64)
        ref = np.where(s >= box, s - box, np.where(s < 0, s + box, s))
        col = got[:, los].astype(np.float64)
        assert np.all(col >= 0.0) and np.all(col < box) and not np.any(got[:, los] == t(box))
        d = np.abs(col - ref)
        assert np.all(np.minimum(d, box - d) <= 2 * ulp), np.minimum(d, box - d).max()
        assert got[1, los] == 0.0
        for other in {0, 1, 2} - {los}:
            npt.assert_array_equal(got[:, other], pos[:, other])
        alias = dev.as_device(pos)
        assert dev.rsd_shift(alias, dev.as_device(vel), box, los=los, out=alias) is alias
        npt.assert_array_equal(alias.cpu().numpy(), got)
        alias, v = dev.as_device(pos), dev.as_device(vel)                    # the kernel itself with out_d = pos_d
        assert hip.ast_rsd_shift(dev.ptr(alias), dev.ptr(v), dev.real_code(alias), npart, los, 0.01, box, dev.ptr(alias),
                                 dev.stream()) == 0
        npt.assert_array_equal(alias.cpu().numpy(), got)
    one = dev.rsd_shift(dev.as_device(pos[:1]), dev.as_device(vel[:1]), box, los=2).cpu().numpy()
    npt.assert_array_equal(one, dev.rsd_shift(dev.as_device(pos), dev.as_device(vel), box, los=2).cpu().numpy()[:1])
    far = vel.copy()
    far[7, 1] = 100.0 * (2.5 * box)               # a shift of 2.5 box lengths
    with pytest.raises(ValueError):
        dev.rsd_shift(dev.as_device(pos), dev.as_device(far), box, los=1)
    far[7, 1] = -100.0 * (2.5 * box)
    with pytest.raises(ValueError):
        dev.rsd_shift(dev.as_device(pos), dev.as_device(far), box, los=1)
    alias = dev.as_device(pos)                    # a rejected in-place call leaves the positions as they were
    with pytest.raises(ValueError):
        dev.rsd_shift(alias, dev.as_device(far), box, los=1, out=alias)
    npt.assert_array_equal(alias.cpu().numpy(), pos)
    with pytest.raises(ValueError):
        dev.rsd_shift(dev.as_device(pos), dev.as_device(vel), box, los=3)


# ------------------------------------------------------------------ 9: end to end in redshift space
@pytest.mark.parametrize("los", [0, 2])
def test_catalog_power_2d_in_redshift_space(dev, los):
    rng = np.random.default_rng(9)
    n, box, npart = 32, 100.0, 4096
    pos = rng.uniform(0, box, size=(npart, 3))
    vel = rng.uniform(-2000, 2000, size=(npart, 3))        # shifts of +-20: a tenth of the particles wrap
    s = pos.copy()
    s[:, los] += 0.01 * vel[:, los]
    wrapped = (s[:, los] >= box) | (s[:, los] < 0)
    assert 0.07 * npart < wrapped.sum() < 0.13 * npart
    s[:, los] = np.where(s[:, los] >= box, s[:, los] - box, np.where(s[:, los] < 0, s[:, los] + box, s[:, los]))
    c, sn = offt.catalog_mesh_complex(s, None, n, box, "tsc", True, True)
    ref = o2.finish(o2.project_2d(o2.p3d(c, None, box), n, box, 5, los, (0, 2, 4)), (0, 2, 4), sn)
    got = dev.catalog_power_2d(dev.as_device(pos), None, n, box, "tsc", True, True, vel1=dev.as_device(vel), los=los)
    npt.assert_array_equal(got["modes"], ref["modes"])
    npt.assert_allclose(got["shotnoise"], ref["shotnoise"], rtol=1e-12)
    top = np.nanmax(np.abs(ref["power"]))
    npt.assert_allclose(got["power"], ref["power"], rtol=1e-9, atol=1e-9 * top)
    npt.assert_allclose(got["k"], ref["k"], rtol=1e-12)
    npt.assert_allclose(got["mu"], ref["mu"], rtol=1e-12)
    for l in (0, 2, 4):
        npt.assert_allclose(got["poles"]["power_%d" % l], ref["poles"]["power_%d" % l], rtol=1e-9,
                            atol=1e-9 * (2 * l + 1) * top)
    # without velocities the catalogue stays in real space: the monopole is catalog_power_1d's spectrum
    plain = dev.catalog_power_2d(dev.as_device(pos), None, n, box, los=los)
    one = dev.catalog_power_1d(dev.as_device(pos), None, n, box)
    npt.assert_allclose(plain["poles"]["power_0"], one["power"], rtol=1e-10)


# ------------------------------------------------------------------ 10: the API
def test_power_spectrum_3d_mode_2d(dev, tmp_path, monkeypatch):
    """compute(mode="2d") on a tiny fake simulation, returned and saved; the default call is unchanged.  PyTables is
    not assumed: without it DataFrame.to_hdf is replaced by a pickle per (file, key), read back below - the frames and
    the sequence of (file, key, mode) calls are checked, the HDF layout itself only where PyTables is installed."""
    from astrild_amd.power_spectra import PowerSpectrum3D
    rng = np.random.default_rng(12)
    n, box = 16, 250.0
    grids = {3: rng.standard_normal((n, n, n)) + 2.0, 7: rng.standard_normal((n, n, n))}
    files = {}
    for nr, g in grids.items():
        files[nr] = str(tmp_path / f"grid_{nr:03d}.npy")
        np.save(files[nr], g)
    sim = types.SimpleNamespace(boxsize=box, domain_level=n, npar=n, dirs={"out": str(tmp_path) + "/"}, dir_nrs=sorted(files),
                                get_file_nrs=lambda dsc, path, which: sorted(files),
                                get_file_paths=lambda dsc, path, which: [files[k] for k in sorted(files)])
    ps = PowerSpectrum3D("particles", sim)
    dsc = lambda: [{"path": "x", "root": "grid", "extension": "npy"}]
    res = ps.compute(["rho"], dsc(), save=False, mode="2d", Nmu=4, los=1, poles=(0, 2))
    assert sorted(res) == ["snap_3", "snap_7"]
    for nr, g in grids.items():
        c = offt.r2c(g)
        ref = o2.finish(o2.project_2d(o2.p3d(c, None, box), n, box, 4, 1, (0, 2)), (0, 2))
        got = res["snap_%d" % nr]
        npt.assert_array_equal(got["modes"], ref["modes"])
        npt.assert_allclose(got["power"], ref["power"], rtol=1e-9)
        for key in ("k", "power_0", "power_2"):
            npt.assert_allclose(got["poles"][key], ref["poles"][key], rtol=1e-9, atol=1e-9 * np.abs(ref["poles"]["power_0"]).max())
    written, calls = {}, []
    filename = str(tmp_path / "pkmu_rho_v.h5")
    have_tables = importlib.util.find_spec("tables") is not None       # with PyTables the real file is written and read

    def to_pickle_instead(self, path, key="df", mode="a", **kw):
        self.to_pickle(path + "." + key + ".pkl")
    real_to_hdf = pd.DataFrame.to_hdf if have_tables else to_pickle_instead

    def recording_to_hdf(self, path, key="df", mode="a", **kw):
        calls.append((path, key, mode))
        written[key] = path + "." + key + ".pkl"
        real_to_hdf(self, path, key=key, mode=mode, **kw)
    monkeypatch.setattr(pd.DataFrame, "to_hdf", recording_to_hdf)
    read_back = (lambda key: pd.read_hdf(filename, key=key)) if have_tables else (lambda key: pd.read_pickle(written[key]))
    saved, inner = [], ps._power_spectrum_2d           # what the saving call computes (float atomics: last bits vary per run)
    monkeypatch.setattr(ps, "_power_spectrum_2d", lambda *a, **kw: saved.append(inner(*a, **kw)) or saved[-1])
    assert ps.compute(["rho", "v"], dsc(), save=True, mode="2d", Nmu=4, los=1, poles=(0, 2)) is None
    # one file, the first key opens it ("w"), the others are appended
    assert calls == [(filename, "snap_3_pkmu", "w"), (filename, "snap_3_poles", "a"), (filename, "snap_7_pkmu", "a"),
                     (filename, "snap_7_poles", "a")]
    for i, nr in enumerate(sorted(grids)):
        got = saved[i]
        npt.assert_allclose(got["power"], res["snap_%d" % nr]["power"], rtol=1e-12)
        wedges = read_back("snap_%d_pkmu" % nr)
        poles = read_back("snap_%d_poles" % nr)
        npt.assert_array_equal(wedges.values, got["power"])
        npt.assert_array_equal(wedges.columns.values, [0.125, 0.375, 0.625, 0.875])
        npt.assert_array_equal(wedges.index.values, got["poles"]["k"])
        assert list(poles.columns) == ["P0", "P2", "modes"]
        npt.assert_array_equal(poles["P0"].values, got["poles"]["power_0"])
        npt.assert_array_equal(poles["P2"].values, got["poles"]["power_2"])
        npt.assert_array_equal(poles["modes"].values, got["poles"]["modes"])
    monkeypatch.undo()
    pk = ps.compute(["rho"], dsc(), save=False)
    for nr, g in grids.items():
        k, p = ps._power_spectrum_3d(g)
        npt.assert_allclose(pk["k"]["snap_%d" % nr], k, rtol=1e-13)
        npt.assert_allclose(pk["P"]["snap_%d" % nr], p, rtol=1e-12)
    with pytest.raises(ValueError):
        ps.compute(["rho"], dsc(), save=False, mode="2d", poles=(1,))
    with pytest.raises(ValueError):
        ps.compute(["rho"], dsc(), save=False, mode="3d")
