"""GPU parity: HIP mass assignment + rocFFT + shell binning vs the oracle.

Tolerances: indices / mode counts / NGP assignment bit-exact; fp64 floats
1e-12 (sum order only); fp32 floats 1e-6 relative (north_star tolerance).
"""
import numpy as np
import pytest

from oracle import mesh as omesh, fftpower as offt

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev(hip):
    from astrild_amd import device
    torch.cuda.set_device(0)
    return device


def _tt(dtype):
    return torch.float32 if dtype == np.float32 else torch.float64


@pytest.mark.parametrize("method", ["direct", "tiled", "tiled2"])
@pytest.mark.parametrize("window", ["ngp", "cic", "tsc"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_paint_random_particles_with_mass(dev, method, window, dtype):
    if method in ("tiled", "tiled2") and window == "ngp":
        pytest.skip("tiled path is CIC/TSC only")
    rng = np.random.default_rng(11)
    n, L, npart = 64, 250.0, 70000
    pos = rng.uniform(-0.3 * L, 1.3 * L, size=(npart, 3)).astype(dtype)   # wraps on both sides
    mass = rng.uniform(0.5, 2.0, size=npart).astype(dtype)
    got = dev.paint(dev.as_device(pos), dev.as_device(mass), n, L, window, method=method).cpu().numpy()
    ref = omesh.paint(pos, mass, n, L, window)
    tol = 1e-12 if dtype == np.float64 else 2e-6
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * ref.max())
    assert got.sum(dtype=np.float64) == pytest.approx(mass.sum(dtype=np.float64), rel=1e-6)


@pytest.mark.parametrize("method", ["direct", "tiled", "tiled2"])
@pytest.mark.parametrize("window", ["cic", "tsc"])
def test_paint_lattice_particles_natural_and_shuffled(dev, method, window):
    n, L = 64, 1000.0
    for shuffle in (False, True):
        pos = omesh.lattice_particles(n, n, L, seed=20240601, shuffle=shuffle, dtype=np.float32)
        got = dev.paint(dev.as_device(pos), None, n, L, window, method=method).cpu().numpy()
        ref = omesh.paint(pos, None, n, L, window)
        np.testing.assert_allclose(got, ref, rtol=2e-6, atol=2e-6)


def test_paint_scale_folds_cell_volume(dev):
    rng = np.random.default_rng(3)
    n, L = 32, 500.0
    pos = rng.uniform(0, L, size=(5000, 3))
    dx = L / n
    got = dev.paint(dev.as_device(pos), None, n, L, "tsc", scale=1.0 / dx**3, method="direct").cpu().numpy()
    ref = omesh.paint(pos, None, n, L, "tsc") / dx**3          # stats_subfind.py:131-132
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * ref.max())


@pytest.mark.parametrize("method", ["direct", "tiled", "tiled2"])
@pytest.mark.parametrize("window", ["cic", "tsc"])
def test_paint_slab_buffer_with_ghost_planes(dev, method, window):
    # rank owning planes [16, 32) of a 64-grid, one ghost plane each side
    rng = np.random.default_rng(5)
    n, L = 64, 64.0
    pos = rng.uniform(0, L, size=(40000, 3))
    s = pos[:, 0] * (n / L)
    base = np.floor(s) if window == "cic" else np.floor(s + 0.5)
    own = (base >= 16) & (base < 32)
    mine = np.ascontiguousarray(pos[own])
    x_start, nx_alloc = 15, 18
    got = dev.paint(dev.as_device(mine), None, n, L, window, method=method,
                    x_start=x_start, nx_alloc=nx_alloc).cpu().numpy()
    ref = omesh.paint(mine, None, n, L, window)[x_start:x_start + nx_alloc]
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
    # a particle outside the buffer must be reported, not silently lost
    with pytest.raises(Exception):
        dev.paint(dev.as_device(pos), None, n, L, window, method=method, x_start=x_start, nx_alloc=nx_alloc)


@pytest.mark.parametrize("method", ["direct", "tiled", "tiled2"])
def test_paint_accumulate_and_overwrite_modes(dev, method):
    rng = np.random.default_rng(17)
    n, L = 64, 100.0
    pos = dev.as_device(rng.uniform(0, L, size=(80000, 3)))
    ref = omesh.paint(pos.cpu().numpy(), None, n, L, "cic")
    out = torch.full((n, n, n), 7.0, dtype=torch.float64, device="cuda")
    dev.paint(pos, None, n, L, "cic", out=out, method=method)                      # out given -> accumulate
    np.testing.assert_allclose(out.cpu().numpy(), ref + 7.0, rtol=1e-12)
    dev.paint(pos, None, n, L, "cic", out=out, method=method, accumulate=False)    # overwrite: garbage in `out` is fine
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-12, atol=1e-13)
    dev.paint(pos, None, n, L, "cic", out=out, method=method, accumulate=True)
    np.testing.assert_allclose(out.cpu().numpy(), 2 * ref, rtol=1e-12, atol=1e-13)
    # sparse input: most tiles are empty and must still be cleared in overwrite mode
    few = dev.as_device(rng.uniform(0, L, size=(70000, 3)) * np.array([0.05, 1.0, 1.0]))
    out.fill_(3.0)
    dev.paint(few, None, n, L, "tsc", out=out, method=method, accumulate=False)
    np.testing.assert_allclose(out.cpu().numpy(), omesh.paint(few.cpu().numpy(), None, n, L, "tsc"), rtol=1e-12, atol=1e-13)


def test_paint_empty_and_single_particle(dev):
    n, L = 32, 32.0
    empty = torch.empty((0, 3), dtype=torch.float64, device="cuda")
    assert float(dev.paint(empty, None, n, L, "cic", method="direct").abs().sum()) == 0.0
    one = np.array([[31.25, 0.5, 3.0]])
    got = dev.paint(dev.as_device(one), None, n, L, "cic", method="tiled").cpu().numpy()
    np.testing.assert_array_equal(got, omesh.paint(one, None, n, L, "cic"))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ngp_assign_bit_exact_last_write_wins(dev, dtype):
    rng = np.random.default_rng(9)
    npar, npart = 32, 120000                       # ~3.7 particles per cell: many duplicates
    x, y, z = (rng.uniform(0, 1, npart).astype(dtype) for _ in range(3))
    x[x >= 1] = 0
    y[y >= 1] = 0
    z[z >= 1] = 0
    v = rng.standard_normal(npart).astype(dtype)
    got = dev.ngp_assign(x, y, z, v, npar, dtype=_tt(dtype)).cpu().numpy()
    ref = omesh.ngp_assign(x, y, z, v, npar)
    np.testing.assert_array_equal(got.astype(np.float64), ref)
    with pytest.raises(IndexError):
        dev.ngp_assign(np.array([1.5]), np.array([0.1]), np.array([0.1]), np.array([1.0]), 8)


@pytest.mark.parametrize("n", [16, 32, 64])
def test_mode_counts_and_k_bit_exact(dev, n):
    """Both shell-membership rules, several box sizes (the float64 rule's edge decisions depend on L): mode counts
    identical to the oracle's, the integer rule's also to a brute-force count over the full lattice."""
    f = torch.zeros((n, n, n), dtype=torch.float64, device="cuda")
    res = dev.fftpower_1d(f, 123.0, binning="integer")
    ref = offt.fftpower_1d(np.zeros((n, n, n)), 123.0, binning="integer")
    np.testing.assert_array_equal(res["modes"], ref["modes"])
    np.testing.assert_array_equal(res["modes"], offt.brute_force_mode_counts(n))
    np.testing.assert_allclose(res["k"], ref["k"], rtol=1e-12)
    differs = 0
    for L in (123.0, 1000.0, 500.0, 100.0, 2 * np.pi):
        res = dev.fftpower_1d(f, L)                                       # default: nbodykit's float64 comparison
        ref = offt.fftpower_1d(np.zeros((n, n, n)), L)
        np.testing.assert_array_equal(res["modes"], ref["modes"])
        np.testing.assert_allclose(res["k"], ref["k"], rtol=1e-12)
        differs += int((res["modes"] != offt.brute_force_mode_counts(n)).sum())
    assert differs > 0                                                    # the two rules are not the same thing


@pytest.mark.parametrize("n", [256])
def test_fused_path_follows_the_binning_rule(dev, n):
    """The fused fp32 path (shell lookup in the x pass epilogue, low-k channel) under both rules against the unfused
    fp64 binning of the same grid: mode-for-mode the same membership."""
    rng = np.random.default_rng(2)
    f = (1.0 + 0.3 * rng.standard_normal((n, n, n))).astype(np.float32)
    t = dev.as_device(f)
    for L in (1000.0, 100.0):
        for binning in ("integer", "float64"):
            fused = dev.fftpower_1d(t, L, binning=binning)
            plain = dev.fftpower_1d(t.double(), L, binning=binning)
            np.testing.assert_array_equal(fused["modes"], plain["modes"])
            np.testing.assert_allclose(fused["power"], plain["power"], rtol=1e-6)
    a = dev.fftpower_1d(t, 1000.0, binning="integer")["power"]
    b = dev.fftpower_1d(t, 1000.0, binning="float64")["power"]
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-12), (np.float32, 1e-6)])
def test_fftpower_white_noise_field(dev, dtype, tol):
    rng = np.random.default_rng(21)
    n, L = 64, 200.0
    f = (1.0 + 0.3 * rng.standard_normal((n, n, n))).astype(dtype)
    res = dev.fftpower_1d(dev.as_device(f), L)
    ref = offt.fftpower_1d(f, L)
    np.testing.assert_array_equal(res["modes"], ref["modes"])
    np.testing.assert_allclose(res["k"], ref["k"], rtol=1e-12)
    np.testing.assert_allclose(res["power"], ref["power"].real, rtol=tol)


def test_fftpower_cross_spectrum(dev):
    rng = np.random.default_rng(22)
    n, L = 32, 50.0
    f1 = rng.standard_normal((n, n, n))
    f2 = 0.5 * f1 + rng.standard_normal((n, n, n))
    res = dev.fftpower_1d(dev.as_device(f1), L, dev.as_device(f2))
    ref = offt.fftpower_1d(f1, L, f2)
    np.testing.assert_allclose(res["power"], ref["power"].real, rtol=1e-11, atol=1e-12 * abs(ref["power"]).max())


def test_plane_wave_known_answer(dev):
    n, L, A = 32, 100.0, 0.3
    x = np.arange(n) / n
    m = (2, -3, 4)
    f = 5.0 + A * np.cos(2 * np.pi * (m[0] * x[:, None, None] + m[1] * x[None, :, None] + m[2] * x[None, None, :]))
    res = dev.fftpower_1d(dev.as_device(f), L)
    shell = int(np.floor(np.sqrt(29))) - 1
    exp = np.zeros(n // 2 - 1)
    exp[shell] = 2 * (A * A / 4) * L**3 / res["modes"][shell]
    np.testing.assert_allclose(res["power"], exp, atol=1e-9 * L**3)


@pytest.mark.parametrize("method", ["direct", "tiled", "tiled2"])
def test_pipeline_cic_pk_lattice_fp32_vs_oracle(dev, method):
    # configs[0]-shaped: 64^3 here to keep the oracle in seconds; same code path as 128^3
    n, L = 64, 1000.0
    pos = omesh.lattice_particles(n, n, L, dtype=np.float32)
    grid = dev.paint(dev.as_device(pos), None, n, L, "cic", method=method)
    res = dev.fftpower_1d(grid, L)
    ref = offt.fftpower_1d(omesh.paint(pos, None, n, L, "cic"), L)
    np.testing.assert_array_equal(res["modes"], ref["modes"])
    # fp32 grid + fp32 FFT: measured deviation is reported in DESIGN.md; cold-lattice low-k
    # shells carry ~1e-5 of the Nyquist power, so compare against the spectrum's peak
    np.testing.assert_allclose(res["power"], ref["power"].real, rtol=1e-4, atol=1e-6 * ref["power"].real.max())


def test_pipeline_cic_pk_fp64_tight(dev):
    n, L = 64, 1000.0
    pos = omesh.lattice_particles(n, n, L, seed=7)
    grid = dev.paint(dev.as_device(pos), None, n, L, "cic", method="tiled")
    res = dev.fftpower_1d(grid, L)
    ref = offt.fftpower_1d(omesh.paint(pos, None, n, L, "cic"), L)
    np.testing.assert_array_equal(res["modes"], ref["modes"])
    np.testing.assert_allclose(res["power"], ref["power"].real, rtol=1e-9)


def test_synthetic_generator_statistics(dev):
    n, L = 64, 1000.0
    pos = dev.synth_lattice_particles(n, n, L, seed=1, dtype=torch.float64).cpu().numpy()
    g = (np.arange(n) + 0.5) * (L / n)
    q = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    d = pos - q
    d -= L * np.round(d / L)
    sigma = 0.5 * L / n
    assert abs(d.mean()) < 4 * sigma / np.sqrt(d.size)
    assert d.std() == pytest.approx(sigma, rel=5e-3)
    assert pos.min() >= 0 and pos.max() < L
    sh = dev.synth_lattice_particles(n, n, L, seed=1, shuffle=True, dtype=torch.float64).cpu().numpy()
    # same multiset of particles, different order
    np.testing.assert_allclose(np.sort(sh[:, 0]), np.sort(pos[:, 0]), rtol=0, atol=0)
    assert not np.array_equal(sh, pos)
    # the pseudo-random order (Feistel network keyed by seed + 1) is a PERMUTATION of any range - also of one whose length
    # is no power of two - and a different one per seed; the stride order of rounds 1-4 stays available
    first, count = 1000, 29791
    sub = dev.synth_lattice_particles(n, n, L, seed=1, dtype=torch.float64, first=first, count=count).cpu().numpy()
    for kind in (True, "stride"):
        shs = dev.synth_lattice_particles(n, n, L, seed=1, shuffle=kind, dtype=torch.float64, first=first, count=count).cpu().numpy()
        assert np.array_equal(shs[np.lexsort(shs.T)], sub[np.lexsort(sub.T)]) and not np.array_equal(shs, sub)
    other = dev.synth_lattice_particles(n, n, L, seed=2, shuffle=True, dtype=torch.float64, first=first, count=count).cpu().numpy()
    assert not np.array_equal(other[:, 0], shs[:, 0])
    # random, not low-discrepancy: consecutive particles of the shuffled array are far apart in the lattice
    idx = {tuple(r): i for i, r in enumerate(np.round(pos, 9).tolist())}
    where = np.array([idx[tuple(r)] for r in np.round(sh[:4096], 9).tolist()])
    assert len(set(np.diff(where).tolist())) > 4000          # (the stride order has ONE difference modulo the count)


def test_single_pass_overflow_path_on_clustered_input(dev):
    # 90 % of the particles in one corner blob: most of them overflow their tile's fixed
    # segment and take the global-atomic path; the result must not change
    rng = np.random.default_rng(23)
    n, L, npart = 64, 100.0, 200000
    blob = rng.normal(10.0, 1.5, size=(int(0.9 * npart), 3))
    rest = rng.uniform(0, L, size=(npart - len(blob), 3))
    pos = np.concatenate([blob, rest])
    rng.shuffle(pos)
    mass = rng.uniform(0.5, 1.5, npart)
    from tests import paint_accuracy as pa
    for dtype in (np.float64, np.float32):
        # (float32: the reference is that of the rounded coordinates and masses)
        pos, mass = pos.astype(dtype), mass.astype(dtype)
        ref = omesh.paint(pos, mass, n, L, "cic")
        acc = pa.Reference(pos, mass, n, L, "cic")
        # (check_dropped=False: nothing repaints, the single pass stands with its overflow list)
        for method, kw in (("tiled", {}), ("tiled2", {}), ("tiled", dict(check_dropped=False))):
            st = {}
            got = dev.paint(dev.as_device(pos), dev.as_device(mass), n, L, "cic", method=method, stats=st, **kw).cpu().numpy()
            assert not kw or (st["path"], st["attempts"], st["overflow"] > npart // 2) == ("single-pass", 1, True), st
            if dtype == np.float64 or st["path"] == "two-pass":
                # (float32 atomics in arrival order, a hundred thousand per blob cell, are held to the per-cell bound alone)
                tol = 1e-11 if dtype == np.float64 else 2e-6
                np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * ref.max())
            # cell by cell: the any-path bound of tests/paint_accuracy.py
            bound = acc.any_bound(dtype, "two-pass" if st["path"] == "two-pass" else "single")
            ratio, rel, over = pa.measure(got, acc, bound)
            print(f"[{np.dtype(dtype).name} {method}] path {st['path']} attempts {st['attempts']}: error / bound {ratio:.3g}, error / A {rel:.3g}")
            assert over == 0, (dtype, method, st, ratio)


@pytest.mark.parametrize("window", ["cic", "tsc"])
def test_overwrite_paint_is_bit_reproducible_and_order_independent(dev, window):
    # fixed-point LDS tiles + plain-store flush + fixed-order halo fold: the painted grid does not
    # depend on atomic arrival order, nor on the order of the particles in memory
    n, L = 128, 1000.0
    nat = dev.synth_lattice_particles(n, n, L, seed=9, dtype=torch.float32)
    shf = dev.synth_lattice_particles(n, n, L, seed=9, dtype=torch.float32, shuffle=True)
    a = dev.paint(nat, None, n, L, window, method="tiled")
    b = dev.paint(nat, None, n, L, window, method="tiled")
    c = dev.paint(shf, None, n, L, window, method="tiled")
    assert torch.equal(a, b)
    assert torch.equal(a, c)
    mass = torch.rand(nat.shape[0], dtype=torch.float32, device="cuda") + 0.5
    d = dev.paint(nat, mass, n, L, window, method="tiled")
    e = dev.paint(nat, mass, n, L, window, method="tiled")
    assert torch.equal(d, e)


@pytest.mark.parametrize("window", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_tiled_paint_far_outside_the_box_and_on_its_edges(dev, window, dtype):
    """Positions several box lengths away, exactly on 0 / L / -L and just below 0: the general cell
    reduction of both tiled kernels (column flags, careful deposit variant) against the oracle."""
    rng = np.random.default_rng(5)
    n, L = 64, 100.0
    far = rng.uniform(-7.5 * L, 9.25 * L, size=(40000, 3))
    inside = rng.uniform(0, L, size=(40000, 3))
    edges = np.array([[0.0, 0.0, 0.0], [L, L, L], [-L, 2 * L, 0.0], [-1e-6, L - 1e-6, 0.5 * L], [3 * L, -4 * L, L],
                      [L * (1 - 2.0 ** -24), 0.0, L * (1 - 2.0 ** -24)]])
    pos = np.concatenate([inside, far, edges]).astype(dtype)
    for method in ("tiled", "tiled2"):
        got = dev.paint(dev.as_device(pos), None, n, L, window, method=method).cpu().numpy()
        ref = omesh.paint(pos, None, n, L, window)
        tol = 1e-11 if dtype == np.float64 else 2e-6
        np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * ref.max())
        assert got.sum(dtype=np.float64) == pytest.approx(len(pos), rel=1e-6)


@pytest.mark.parametrize("window", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_paint_offset_stores_the_density_contrast(dev, window, dtype):
    """offset="mean": owned cells hold rho - mean, subtracted in double before the one rounding to the
    grid dtype, so an fp32 cell is accurate to 6e-8 of |delta| (not of the O(1) mean); with masses and
    a cell-volume scale; both the folded grid and the deferred-fold pair (grid + halo records)."""
    rng = np.random.default_rng(31)
    n, L = 64, 320.0
    pos = omesh.lattice_particles(n, n, L, seed=3, dtype=dtype)
    mass = rng.uniform(0.5, 2.0, size=len(pos)).astype(dtype)
    scale = (n / L) ** 3
    ref = omesh.paint(pos, mass, n, L, window) * scale
    mean = mass.astype(np.float64).sum() * scale / n ** 3
    delta = ref - mean
    got = dev.paint(dev.as_device(pos), dev.as_device(mass), n, L, window, scale=scale, method="tiled",
                    offset="mean").cpu().numpy()
    err = np.abs(got - delta)
    if dtype == np.float64:
        assert err.max() <= 1e-12 * np.abs(ref).max()
    else:
        # cells no halo record is folded into (interior of the 8 x 8 tile footprint): ONE rounding of the exact
        # fixed-point sum minus the mean -> half an fp32 ulp of |delta|
        ix = np.arange(n) % 8
        inner = ((ix > 1) & (ix < 6))[:, None, None] & ((ix > 1) & (ix < 6))[None, :, None] & np.ones(n, bool)[None, None, :]
        # (plus the fixed-point quantum of the LDS tiles, 2^-31 of the largest deposit, once per term)
        quantum = float(mass.max()) * scale / 2.0 ** 31
        assert (err[inner] <= 6.0e-8 * np.abs(delta[inner]) + 32 * quantum).all()
        # border cells add up to three fp32 records in fp32
        assert err.max() <= 2.5e-7 * np.abs(ref).max()
    assert abs(got.sum(dtype=np.float64)) < 1e-3 * np.abs(delta).sum()
    assert dev.total_mass(dev.as_device(mass), len(mass)) == pytest.approx(mass.astype(np.float64).sum(), rel=1e-14)


@pytest.mark.parametrize("window", ["cic", "tsc"])
def test_slab_buffer_with_a_partial_last_tile_reports_lost_deposits(dev, window):
    """nx_alloc % 8 != 0: a particle whose base plane is the buffer's last plane deposits its +1 (+2)
    planes onto owned cells of a plane the buffer does not hold.  Every paint variant must count
    them (they used to vanish silently in the overwrite column walk)."""
    from astrild_amd._lib import AstrildHipError
    n, L = 64, 64.0
    rng = np.random.default_rng(8)
    x_start, nx_alloc = 10, 18                           # planes 10..27; 18 % 8 = 2
    inside = rng.uniform(0, L, size=(70000, 3))
    inside[:, 0] = rng.uniform(x_start + 1.0, x_start + nx_alloc - 2.0, size=len(inside))
    for method in ("direct", "tiled", "tiled2"):
        for accumulate in (None, False):
            ok = dev.paint(dev.as_device(inside), None, n, L, window, method=method, x_start=x_start, nx_alloc=nx_alloc,
                           accumulate=accumulate).cpu().numpy()
            ref = omesh.paint(inside, None, n, L, window)[x_start:x_start + nx_alloc]
            np.testing.assert_allclose(ok, ref, rtol=1e-12, atol=1e-12)
            bad = inside.copy()
            bad[0] = [x_start + nx_alloc - 1 + 0.4, 20.3, 30.6]       # base plane = last buffer plane (CIC); +1 is outside
            with pytest.raises(AstrildHipError, match="outside the grid buffer"):
                dev.paint(dev.as_device(bad), None, n, L, window, method=method, x_start=x_start, nx_alloc=nx_alloc,
                          accumulate=accumulate)


def test_config_a_128_cic_power_vs_oracle(dev):
    """BASELINE.json configs[0] at its stated size: 128^3 synthetic particles -> CIC -> P(k).
    fp64 (the reference's dtype) against the oracle to 1e-9 on every shell, mode counts and k exact;
    fp32 through the fused pipeline (paint stores rho - mean) against the same oracle."""
    n, L = 128, 1000.0
    pos = omesh.lattice_particles(n, n, L, seed=20240601)
    ref = offt.fftpower_1d(omesh.paint(pos, None, n, L, "cic"), L)
    res = dev.fftpower_1d(dev.paint(dev.as_device(pos), None, n, L, "cic", method="tiled"), L)
    np.testing.assert_array_equal(res["modes"], ref["modes"])
    np.testing.assert_allclose(res["k"], ref["k"], rtol=1e-12)
    np.testing.assert_allclose(res["power"], ref["power"].real, rtol=1e-9)
    pos32 = pos.astype(np.float32)
    ref32 = offt.fftpower_1d(omesh.paint(pos32, None, n, L, "cic"), L)       # same fp32 positions, fp64 arithmetic
    for window in ("cic",):
        got = dev.paint_power_1d(dev.as_device(pos32), None, n, L, window)
        np.testing.assert_array_equal(got["modes"], ref32["modes"])
        rel = np.abs(got["power"] / ref32["power"].real - 1.0)
        # fp32 grid (rho - mean, rounded once) + fp32 FFT, the five lowest shells from the double-precision
        # low-k channel: 1e-6 on every shell (north_star tolerance)
        assert rel.max() < 1e-6


@pytest.mark.parametrize("window", ["cic", "tsc"])
@pytest.mark.parametrize("interlaced,compensated", [(True, True), (False, True), (True, False)])
def test_catalogue_mesh_interlacing_and_compensation_vs_oracle(dev, window, interlaced, compensated):
    """the half-cell shifted paint (shift in grid units, one fma), the interlaced combination and the
    window compensation against the oracle's restatement of nbodykit's CatalogMesh - spectra to 1e-10, power to 1e-9."""
    rng = np.random.default_rng(17)
    n, L, npart = 32, 250.0, 90000
    pos = rng.uniform(0, L, size=(npart, 3))
    mass = rng.uniform(0.5, 2.0, size=npart)
    shifted = dev.paint(dev.as_device(pos), dev.as_device(mass), n, L, window, shift=0.5, method="tiled").cpu().numpy()
    np.testing.assert_allclose(shifted, omesh.paint(pos, mass, n, L, window, shift=0.5), rtol=1e-11, atol=1e-11)
    direct = dev.paint(dev.as_device(pos), dev.as_device(mass), n, L, window, shift=0.5, method="direct").cpu().numpy()
    np.testing.assert_allclose(direct, shifted, rtol=1e-11, atol=1e-11)
    c, sn = dev.catalog_mesh_complex(dev.as_device(pos), dev.as_device(mass), n, L, window, interlaced, compensated)
    rc, rsn = offt.catalog_mesh_complex(pos, mass, n, L, window, interlaced, compensated)
    assert sn == pytest.approx(rsn, rel=1e-13)
    np.testing.assert_allclose(c.cpu().numpy(), rc, rtol=0, atol=1e-10 * np.abs(rc).max())
    pos2 = rng.uniform(0, L, size=(npart // 2, 3))
    got = dev.catalog_power_1d(dev.as_device(pos), dev.as_device(mass), n, L, window, interlaced, compensated,
                               pos2=dev.as_device(pos2))
    ref = offt.catalog_power_1d(pos, mass, n, L, window, interlaced, compensated, pos2=pos2)
    np.testing.assert_array_equal(got["modes"], ref["modes"])
    np.testing.assert_allclose(got["power"], ref["power"].real, rtol=1e-9, atol=1e-9 * np.abs(ref["power"]).max())


def test_power_spectrum_3d_catalogue_branch(dev, tmp_path):
    """PowerSpectrum3D._power_spectrum_3d_catalog: the reference's cross branch parameters (compensated, interlaced,
    TSC; power_spectrum_3d.py:197-212) applied to particle catalogues; fp32 catalogue path against the fp64 oracle."""
    import types
    from astrild_amd.power_spectra import PowerSpectrum3D
    rng = np.random.default_rng(4)
    n, L = 64, 400.0
    pos1 = rng.uniform(0, L, size=(300000, 3))
    pos2 = np.mod(pos1[:150000] + rng.normal(0, 2.0, size=(150000, 3)), L)
    sim = types.SimpleNamespace(boxsize=L, domain_level=n, npar=n, dirs={"out": str(tmp_path) + "/"}, dir_nrs=[0])
    ps = PowerSpectrum3D("particles", sim)
    k, pk = ps._power_spectrum_3d_catalog(pos1, None, pos2, None)
    ref = offt.catalog_power_1d(pos1, None, n, L, "tsc", True, True, pos2=pos2)
    np.testing.assert_allclose(k, ref["k"], rtol=1e-12)
    np.testing.assert_allclose(pk, ref["power"].real, rtol=1e-9, atol=1e-9 * np.abs(ref["power"]).max())
    k, pk = ps._power_spectrum_3d_catalog(pos1, None)
    ref = offt.catalog_power_1d(pos1, None, n, L, "tsc", True, True)
    np.testing.assert_allclose(pk, ref["power"].real - ref["shotnoise"], rtol=1e-9, atol=1e-9 * np.abs(ref["power"]).max())


@pytest.mark.parametrize("window,dtype", [("cic", np.float32), ("tsc", np.float64)])
def test_scattered_path_two_level_bucket_scatter(dev, window, dtype, monkeypatch):
    """AST_PAINT_SCATTERED (hint="scattered"): count, scan, particle -> bucket staging, bucket -> tile stray segments,
    column walk over stray copies only.  Unordered uniform input with masses against the oracle; a clustered blob
    on top exercises the late list (tile segments full) and, through the API's retry, the exact two-pass variant."""
    rng = np.random.default_rng(41)
    n, L, npart = 64, 200.0, 150000
    pos = rng.uniform(-0.4 * L, 1.4 * L, size=(npart, 3)).astype(dtype)
    mass = rng.uniform(0.5, 2.0, size=npart).astype(dtype)
    st = {}
    got = dev.paint(dev.as_device(pos), dev.as_device(mass), n, L, window, method="tiled", accumulate=False,
                    hint="scattered", stats=st).cpu().numpy()
    assert st["scattered"] and st["groups"] == 0 and st["strays"] == npart and st["overflow"] == 0
    ref = omesh.paint(pos, mass, n, L, window)
    tol = 1e-11 if dtype == np.float64 else 2e-6
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * ref.max())
    blob = np.concatenate([rng.normal(0.3 * L, 0.01 * L, size=(npart // 50, 3)), pos[: npart - npart // 50]]).astype(dtype)
    rng.shuffle(blob)
    st = {}
    got = dev.paint(dev.as_device(blob), None, n, L, window, method="tiled", accumulate=False, hint="scattered",
                    check_dropped=False, stats=st).cpu().numpy()
    assert 0 < st["overflow"] < npart // 64                       # a few thousand records take the late list
    ref = omesh.paint(blob, None, n, L, window)
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * ref.max())
    # a LONG late list is deposited through LDS tiles (counted per tile, scanned, filled, one workgroup per tile) instead of
    # global atomics record by record: forced here for the short one, with and without masses
    monkeypatch.setenv("AST_PAINT_LATE_LDS_MIN", "1")
    st = {}
    got = dev.paint(dev.as_device(blob), None, n, L, window, method="tiled", accumulate=False, hint="scattered",
                    check_dropped=False, stats=st).cpu().numpy()
    assert 0 < st["overflow"] < npart // 64
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * ref.max())
    bmass = rng.uniform(0.5, 2.0, size=npart).astype(dtype)
    got = dev.paint(dev.as_device(blob), dev.as_device(bmass), n, L, window, method="tiled", accumulate=False, hint="scattered",
                    check_dropped=False).cpu().numpy()
    refm = omesh.paint(blob, bmass, n, L, window)
    np.testing.assert_allclose(got, refm, rtol=tol, atol=tol * refm.max())
    monkeypatch.delenv("AST_PAINT_LATE_LDS_MIN")
    heavy = np.concatenate([rng.normal(0.3 * L, 0.01 * L, size=(npart // 2, 3)), pos[: npart // 2]]).astype(dtype)
    rng.shuffle(heavy)
    got = dev.paint(dev.as_device(heavy), None, n, L, window, method="tiled", accumulate=False).cpu().numpy()   # retries
    ref = omesh.paint(heavy, None, n, L, window)
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * ref.max())


def test_paint_without_hint_samples_the_order_first(hip):
    """hint=None on >= 2^20 particles: device.paint looks at 256 runs of 32 consecutive particles before it picks the path.
    Lattice order (also halo-like order: compact clumps, unordered inside) goes to the grouping kernel, shuffled input to
    the two-level scatter IN THE FIRST ATTEMPT (no grouping launch at all) - and both give the grid of the explicit hint."""
    from astrild_amd import device as dev
    torch.cuda.set_device(0)
    n, L = 128, 500.0
    nat = dev.synth_lattice_particles(n, n, L, seed=5, dtype=torch.float32)
    shuf = nat[torch.randperm(nat.shape[0], device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))].contiguous()
    assert not dev.sample_is_unordered(nat, n, L) and dev.sample_is_unordered(shuf, n, L)
    # clumps of 64 neighbours in lattice order, shuffled INSIDE each clump: still groupable
    clumps = nat.view(-1, 64, 3)[:, torch.randperm(64, device="cuda"), :].reshape(-1, 3).contiguous()
    assert not dev.sample_is_unordered(clumps, n, L)
    for pos in (nat, shuf, clumps, nat.double(), nat[:1000003].contiguous()):      # the kernel against the same arithmetic in torch
        assert dev.sample_is_unordered(pos, n, L, 0.5, fraction=True) == dev.sample_is_unordered(pos.cpu(), n, L, 0.5, fraction=True)
    for pos, want_scattered in ((nat, False), (shuf, True)):
        st = {}
        dev.profile_enable(True)
        got = dev.paint(pos, None, n, L, "cic", method="tiled", accumulate=False, stats=st)
        torch.cuda.synchronize()
        sites = set(dev.profile_report())
        dev.profile_enable(False)
        assert st["scattered"] == want_scattered and st["overflow"] == 0
        assert ("paint_tiled.level_a" in sites) == want_scattered and ("paint_tiled.fill" in sites) == (not want_scattered), sites
        ref = dev.paint(pos, None, n, L, "cic", method="tiled", accumulate=False, hint="scattered" if want_scattered else None,
                        check_dropped=False)
        assert torch.equal(got, ref)


def test_repeated_fused_pipeline_calls_are_bit_identical(hip):
    """paint -> FFT -> shells with the low-k channel on its side stream: 30 back-to-back calls (no host sync in between
    except the result fetch) give bit-identical spectra - the event ordering between the two streams holds and every
    reduction has a fixed order."""
    from astrild_amd import device as dev
    torch.cuda.set_device(0)
    n = 256
    pos = dev.synth_lattice_particles(n, n, 1000.0, seed=11, dtype=torch.float32)
    ref = None
    for _ in range(30):
        p = np.asarray(dev.paint_power_1d(pos, None, n, 1000.0, "cic")["power"])
        if ref is None:
            ref = p.copy()
        assert np.array_equal(ref, p)


# ------------------------------------------------------------------ z-segmented walk and the x-sorted chunk pipeline
def _env(monkeypatch, **kv):
    for k, v in kv.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


@pytest.mark.parametrize("window", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_z_segmented_walk_is_bit_identical(dev, monkeypatch, window, dtype):
    """A column cut into z-segments (more, shorter workgroups; the seams written from exact sums by z_seam_kernel) gives
    the grid of the unsegmented walk bit for bit - also with masses, an offset, and a slab buffer with a partial tile."""
    n, L = 128, 1000.0
    rng = np.random.default_rng(5)
    pos = dev.as_device(omesh.lattice_particles(n, n, L, seed=3, dtype=dtype))
    mass = dev.as_device(rng.uniform(0.5, 2.0, size=n ** 3).astype(dtype))
    cases = [dict(), dict(x_start=120, nx_alloc=20, check_dropped=False)]
    for kw in cases:
        _env(monkeypatch, AST_PAINT_ZSEG=1)
        ref = dev.paint(pos, mass, n, L, window, method="tiled", accumulate=False, offset=0.25, **kw)
        for nseg in (2, 4):
            _env(monkeypatch, AST_PAINT_ZSEG=nseg)
            got = dev.paint(pos, mass, n, L, window, method="tiled", accumulate=False, offset=0.25, **kw)
            assert torch.equal(got, ref), (window, dtype, kw, nseg)
    _env(monkeypatch, AST_PAINT_ZSEG=None)


@pytest.mark.parametrize("window", ["cic", "tsc"])
@pytest.mark.parametrize("streams", [1, 2])
def test_xsorted_pipeline_matches_plain_paint(dev, monkeypatch, window, streams):
    """AST_PAINT_XSORTED on lattice-ordered particles: chunked grouping + row-by-row walks give the plain paint's grid bit
    for bit (nothing arrives late: overflow 0); on SHUFFLED particles the hint is wrong, the late arrivals go through the
    overflow list and the grid still matches the oracle."""
    n, L = 256, 1000.0
    _env(monkeypatch, AST_PAINT_XCHUNK_MB=4, AST_PAINT_XSTREAMS=streams)
    pos = dev.synth_lattice_particles(n, n, L, dtype=torch.float32)
    ref = dev.paint(pos, None, n, L, window, method="tiled", accumulate=False, offset="mean")
    st = {}
    got = dev.paint(pos, None, n, L, window, method="tiled", accumulate=False, offset="mean", hint="xsorted", stats=st)
    assert st["overflow"] == 0
    assert torch.equal(got, ref)
    # float64 particles with masses (group records + 4-word stray copies)
    rng = np.random.default_rng(3)
    pos64 = pos.double()
    mass64 = dev.as_device(rng.uniform(0.5, 2.0, size=pos.shape[0]))
    ref = dev.paint(pos64, mass64, n, L, window, method="tiled", accumulate=False)
    got = dev.paint(pos64, mass64, n, L, window, method="tiled", accumulate=False, hint="xsorted")
    assert torch.equal(got, ref)
    del pos64, mass64
    # a slab buffer (not periodic in x): rows are walked in order, row 0 is not held back
    kw = dict(x_start=64, nx_alloc=72, check_dropped=False)
    sel = pos[(pos[:, 0] >= 66 * L / n) & (pos[:, 0] < 134 * L / n)].contiguous()
    ref = dev.paint(sel, None, n, L, window, method="tiled", accumulate=False, **kw)
    got = dev.paint(sel, None, n, L, window, method="tiled", accumulate=False, hint="xsorted", **kw)
    assert torch.equal(got, ref)
    if streams == 1:
        n2 = 128
        shuf = omesh.lattice_particles(n2, n2, L, seed=9, shuffle=True, dtype=np.float32)
        st = {}
        got = dev.paint(dev.as_device(shuf), None, n2, L, window, method="tiled", accumulate=False, hint="xsorted",
                        stats=st, check_dropped=False).cpu().numpy()
        assert st["overflow"] > 0
        np.testing.assert_allclose(got, omesh.paint(shuf, None, n2, L, window), rtol=2e-6, atol=2e-6)
    _env(monkeypatch, AST_PAINT_XCHUNK_MB=None, AST_PAINT_XSTREAMS=None)


def test_scattered_paint_with_full_staging_segments(dev):
    """The unordered paint has no counting pass: a (bucket, label) segment of its staging array holds twice the mean.  A
    blob that overfills some segments sends the surplus through the late list (global atomics) - no retry, nothing lost."""
    n, L = 128, 1000.0
    rng = np.random.default_rng(17)
    uniform = rng.uniform(0, L, size=(3_400_000, 3))
    blob = 0.5 * L + rng.uniform(-0.06, 0.06, size=(600_000, 3)) * L
    pos = np.concatenate([uniform, blob]).astype(np.float32)
    rng.shuffle(pos)
    st = {}
    got = dev.paint(dev.as_device(pos), None, n, L, "cic", method="tiled", accumulate=False, hint="scattered",
                    check_dropped=False, stats=st).cpu().numpy()
    assert st["scattered"] and 0 < st["overflow"] < pos.shape[0] // 4
    ref = omesh.paint(pos, None, n, L, "cic")
    np.testing.assert_allclose(got, ref, rtol=2e-6, atol=2e-6 * ref.max())
    assert got.sum(dtype=np.float64) == pytest.approx(pos.shape[0], rel=1e-6)


@pytest.mark.parametrize("window", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_staged_paint_row_by_row_is_bit_identical(dev, window, dtype):
    """ast_paint_tiled_stage: GROUP once, then WALK / FOLD tile row by tile row - in pipeline order (a row is folded as
    soon as the rows its window reaches have been walked) and in a scrambled order - leaves the grid of the one-call
    paint bit for bit: whole periodic grid, slab buffers (whole tiles, a partial last tile), masses, offset on the owned
    planes only, natural and unordered (scattered) input."""
    n, L = 128, 1000.0
    rng = np.random.default_rng(8)
    pos = dev.as_device(omesh.lattice_particles(n, n, L, seed=3, dtype=dtype))
    mass = dev.as_device(rng.uniform(0.5, 2.0, size=n ** 3).astype(dtype))
    shuf = dev.as_device(omesh.lattice_particles(n, n, L, seed=3, shuffle=True, dtype=dtype))
    cases = [(pos, mass, dict(), None), (pos, None, dict(x_start=120, nx_alloc=24), (4, 16)),
             (pos, mass, dict(x_start=40, nx_alloc=20), (2, 16)), (shuf, None, dict(x_start=8, nx_alloc=40), (4, 32))]
    for p, m, kw, owned in cases:
        hint = "scattered" if p is shuf else None
        ref = dev.paint(p, m, n, L, window, method="tiled", accumulate=False, offset=0.25, offset_planes=owned,
                        check_dropped=False, hint=hint, **kw)
        nx = kw.get("nx_alloc", n)
        for order in ("pipeline", "scrambled"):
            out = torch.full((nx, n, n), float("nan"), dtype=p.dtype, device="cuda")
            sp = dev.StagedPaint(p, m, n, L, window, out, offset=0.25, offset_planes=owned, hint=hint, **kw)
            assert sp.nrows_total == (nx + sp.row_planes - 1) // sp.row_planes
            sp.group()
            rows = list(range(sp.nrows_total))
            if order == "pipeline":
                walked, folded = set(), set()
                for r in rows:
                    sp.walk(r, 1)
                    walked.add(r)
                    for f in rows:
                        if f not in folded and set(sp.fold_needs(f)) <= walked:
                            sp.fold(f, 1)
                            folded.add(f)
                assert folded == set(rows)
            else:
                perm = [int(v) for v in rng.permutation(sp.nrows_total)]
                for r in perm:
                    sp.walk(r, 1)
                half = sp.nrows_total // 2
                sp.fold(half, sp.nrows_total - half)            # several rows per call
                if half:
                    sp.fold(0, half)
            assert torch.equal(out, ref), (window, dtype, kw, order)
            if "x_start" in kw:
                assert int(sp.dropped.item()) > 0               # lattice particles beyond the buffer were counted
                with pytest.raises(Exception, match="outside the grid buffer"):
                    sp.check()


def test_staged_paint_overflow_list_is_deposited_with_its_rows(dev):
    """Clustered input overfills tile segments: the overflow list (global atomics) is deposited by the FOLD stage of the
    rows that hold the cells; row by row the grid matches the oracle and nothing is added twice or lost."""
    n, L = 64, 1000.0
    rng = np.random.default_rng(23)
    blob = 0.5 * L + rng.normal(0, 0.01, size=(300_000, 3)) * L
    pos = np.concatenate([rng.uniform(0, L, size=(400_000, 3)), blob])          # float64: the global atomics add in double
    out = torch.empty((n, n, n), dtype=torch.float64, device="cuda")
    sp = dev.StagedPaint(dev.as_device(pos), None, n, L, "cic", out)
    sp.group()
    for r in range(sp.nrows_total):
        sp.walk(r, 1)
    for r in reversed(range(sp.nrows_total)):
        sp.fold(r, 1)
    sp.check()
    ref = omesh.paint(pos, None, n, L, "cic")
    got = out.cpu().numpy()
    assert int(sp.dropped.item()) == 0
    np.testing.assert_allclose(got, ref, rtol=1e-11, atol=1e-11 * ref.max())
    assert got.sum(dtype=np.float64) == pytest.approx(pos.shape[0], rel=1e-12)


@pytest.mark.parametrize("window", ["cic", "tsc"])
def test_staged_paint_grouped_in_parts(dev, window):
    """ast_paint_tiled_stage GROUP_PART: x-ordered particles of a slab buffer grouped in four parts - the last part first
    (it completes the top rows), rows walked as soon as every part that can hold their particles is in, closed rows handed
    to the later parts - give the grid of the one-call paint bit for bit and nothing is counted as dropped; on SHUFFLED
    particles the promise is broken: particles turn up for rows already walked and are counted (check() raises)."""
    n, L = 256, 1000.0
    nx, x_start, gl, ghost = 72, 60, 4, 3                        # owned planes 64 .. 127 of the box, ghost zone 4
    pos = dev.synth_lattice_particles(n, n, L, dtype=torch.float32)
    idx = torch.arange(n ** 3, device="cuda") // (n * n)
    mine = pos[(idx >= x_start + gl) & (idx < x_start + nx - gl)].contiguous()           # lattice planes 64 .. 127: x-ordered, jitter < ghost
    ref = dev.paint(mine, None, n, L, window, method="tiled", accumulate=False, x_start=x_start, nx_alloc=nx, offset=0.5,
                    offset_planes=(gl, nx - 2 * gl), check_dropped=True)
    PR = 8
    nloc = nx - 2 * gl
    shuffled = mine[torch.randperm(mine.shape[0], device="cuda")].contiguous()
    # equal parts one by one, and stages of unequal size: several consecutive parts of 8 in one launch
    plans = ((4, [(3, 1), (0, 1), (1, 1), (2, 1)]), (8, [(7, 1), (0, 4), (4, 2), (6, 1)]))

    for (K, launches), (particles, expect_loss) in [(pl, case) for pl in plans for case in ((mine, False), (shuffled, True))]:
        def key_rows(k):
            return range((gl - ghost + k * nloc // K) // PR, (gl + ghost + (k + 1) * nloc // K - 1) // PR + 1)

        out = torch.full((nx, n, n), float("nan"), dtype=torch.float32, device="cuda")
        sp = dev.StagedPaint(particles, None, n, L, window, out, x_start=x_start, nx_alloc=nx, offset=0.5, offset_planes=(gl, nloc))
        R = sp.nrows_total
        sp.reset()
        grouped, walked = set(), []
        for k, span in launches:
            high = [r for r in walked if all(q in walked for q in range(r, R))]
            sp.group_part(k, K, min(high) if high else 0, len(walked), span)
            grouped.update(range(k, k + span))
            ready = [r for r in range(R) if r not in walked and all(j in grouped for j in range(K) if r in key_rows(j))]
            top = sorted(r for r in ready if all(q in ready or q in walked for q in range(r, R)))
            bottom = sorted(r for r in ready if r not in top)
            for r in top + bottom:
                sp.walk(r, 1)
                walked.append(r)
        assert sorted(walked) == list(range(R))
        sp.fold(0, R)
        if expect_loss:
            assert int(sp.dropped.item()) > 0
            with pytest.raises(Exception, match="walked already"):
                sp.check()
        else:
            sp.check()
            assert torch.equal(out, ref)


@pytest.mark.parametrize("shuffle", [False, True])
def test_clustered_input_goes_to_the_two_pass_path_in_one_attempt(dev, shuffle):
    """What the reference's paint calls really see (evolved snapshots, stats_subfind.py:125-131): a heavy tail of tile
    occupancies.  256^3 particles collapsing onto 64 attractors: the probe reads the overflow from a sample BEFORE anything
    is painted, the exact two-pass variant runs at once (also with check_dropped=False), and grid and spectrum match the
    oracle on the same particles."""
    n, L = 256, 1000.0
    pos = dev.synth_clustered_particles(n, n, L, seed=11, nattractors=64, shuffle=shuffle, dtype=torch.float32)
    probe = dev.probe_input(pos, n, L)
    assert probe["overflow"] > pos.shape[0] // 64 and probe["max_tile"] > 20 * probe["mean_tile"]
    assert (probe["groupable"] < 0.25) == shuffle
    st = {}
    grid = dev.paint(pos, None, n, L, "cic", method="tiled", check_dropped=False, stats=st)
    # file order: the exact two-pass lists; no order in memory: the bucket scatter (its late list reserved per workgroup)
    # (the late list holds a quarter of the particles at float32: beyond four fifths of that estimated - this set, a third -
    # also two-pass)
    limit = dev.scatter_overflow_limit(pos.dtype, pos.shape[0])
    assert limit <= pos.shape[0] // 5 < dev.scatter_late_capacity(pos.dtype, pos.shape[0])
    want = "scattered" if shuffle and probe["overflow"] <= limit else "two-pass"
    assert st["path"] == want and st["attempts"] == 1
    host = pos.cpu().numpy().astype(np.float64)
    ref = omesh.paint(host, None, n, L, "cic")
    got = grid.cpu().numpy().astype(np.float64)
    assert abs(got.sum() - ref.sum()) < 1e-6 * ref.sum()
    np.testing.assert_allclose(got, ref, rtol=0, atol=3e-6 * ref.max())
    if shuffle:
        # a milder set (16 attractors: a few per cent beyond capacity) in pseudo-random order takes the bucket scatter with
        # its late list (reserved once per workgroup and chunk) - complete and equal to the oracle
        mild = pm = None
        for na in (16, 8, 24, 4, 32, 2):
            mild = dev.synth_clustered_particles(n, n, L, seed=12, nattractors=na, shuffle=True, dtype=torch.float32)
            pm = dev.probe_input(mild, n, L)
            if mild.shape[0] // 64 < pm["overflow"] <= limit:
                break
        assert mild.shape[0] // 64 < pm["overflow"] <= limit and pm["groupable"] < 0.25, pm
        stm = {}
        gm = dev.paint(mild, None, n, L, "cic", method="tiled", stats=stm)          # (check_dropped: nothing may be lost)
        assert stm["path"] == "scattered" and stm["attempts"] == 1 and stm["overflow"] > 0
        refm = omesh.paint(mild.cpu().numpy().astype(np.float64), None, n, L, "cic")
        np.testing.assert_allclose(gm.cpu().numpy().astype(np.float64), refm, rtol=0, atol=3e-6 * refm.max())
        del mild, gm, refm
    # the uniform lattice reads no overflow and stays on the single pass (scattered when it has no order in memory)
    lat = dev.synth_lattice_particles(n, n, L, seed=11, dtype=torch.float32, shuffle=shuffle)
    p2 = dev.probe_input(lat, n, L)
    assert p2["overflow"] < lat.shape[0] // 1000
    st2 = {}
    dev.paint(lat, None, n, L, "cic", method="tiled", check_dropped=False, stats=st2)
    assert st2["path"] == ("scattered" if shuffle else "single-pass") and st2["attempts"] == 1
    # the whole pipeline on the clustered set: fp32 (deferred fold + rho - mean, two-pass lists) against the oracle's spectrum
    res = dev.paint_power_1d(pos, None, n, L, "cic")
    want = offt.fftpower_1d(ref, L)
    assert np.array_equal(res["modes"], want["modes"])
    np.testing.assert_allclose(res["power"], want["power"].real, rtol=2e-6)


@pytest.mark.parametrize("window,dtype", [("cic", torch.float32), ("tsc", torch.float64)])
def test_paint_in_chunks_for_more_particles_than_32_bit_indices(dev, window, dtype, monkeypatch):
    """More than 2^32 - 65 particles (2048^3) do not fit the tile lists' 32-bit indices: device.paint paints them in chunks
    onto the same grid (first chunk as asked for - overwrite, rho - mean -, the rest accumulated).  Forced at 256^3 with
    ASTRILD_PAINT_CHUNK; against the one-call paint."""
    n, L = 256, 1000.0
    pos = dev.synth_lattice_particles(n, n, L, seed=4, dtype=dtype)
    whole = dev.paint(pos, None, n, L, window, method="tiled", offset="mean")
    monkeypatch.setenv("ASTRILD_PAINT_CHUNK", str(5_000_000))
    parts = dev.paint(pos, None, n, L, window, method="tiled", offset="mean")
    monkeypatch.delenv("ASTRILD_PAINT_CHUNK")
    tol = 2e-6 if dtype == torch.float32 else 1e-12
    assert float((parts - whole).abs().max()) <= tol * max(1.0, float(whole.abs().max()))
    assert abs(float(parts.double().sum())) < 1e-3 * n ** 3 * (1e-3 if dtype == torch.float64 else 1.0)     # rho - mean sums to ~0
