"""GPU: the seam between the paint and the FFT - the z pass's low-k z sums and its halo fold on load, at the
register shapes and branches that the pipeline tests do not reach below full size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def dev(hip):
    from astrild_amd import device
    torch.cuda.set_device(0)
    return device


def _rows_with_z_sums(dev, hip, t, n, lowz):
    from astrild_amd import _lib
    nrows = t.numel() // n
    out = torch.zeros((nrows, n // 2 + 1), dtype=torch.complex64, device="cuda")
    _lib.check(hip.ast_fft_tile_rows_r2c_lowz(dev.ptr(t), dev.ptr(out), 0, n, nrows, n, n // 2 + 1, 1.0, dev.ptr(lowz),
                                              dev.stream()), "ast_fft_tile_rows_r2c_lowz")
    return out


@pytest.mark.parametrize("n", [256, 512, 1024])
def test_z_sums_of_every_register_shape_meet_the_summation_bound(dev, hip, n):
    """Sides 256, 512, 1024 are the (8, 16), (16, 16) and (16, 32) register shapes; 40 rows are two and a half
    workgroups.  Every z sum k_z <= 6 lies within 2 N 2^-53 sum_z |x_z| of numpy's float64 transform of the same fp32
    samples, in its real and its imaginary part - the a-priori bound of a double summation of N terms in any order
    (about 1e-10 here; a wrong twiddle or index errs by O(|x|)) - and the spectrum the call writes is the plain
    pass's, bit for bit."""
    from astrild_amd import _lib
    nrows = 40
    rng = np.random.default_rng(n)
    x = (2.5 + rng.standard_normal((nrows, n))).astype(np.float32)       # nonzero mean
    x[5, 17] = 3.0e4                                                     # one large spike
    x[7] = 0.0                                                           # one empty row
    t = dev.as_device(x)
    lowz = torch.full((nrows, 7), float("nan"), dtype=torch.complex128, device="cuda")
    spec = _rows_with_z_sums(dev, hip, t, n, lowz)
    plain = torch.zeros_like(spec)
    _lib.check(hip.ast_fft_tile_rows_r2c(dev.ptr(t), dev.ptr(plain), 0, n, nrows, n, n // 2 + 1, 1.0, dev.stream()),
               "ast_fft_tile_rows_r2c")
    assert torch.equal(torch.view_as_real(spec), torch.view_as_real(plain))
    x64 = x.astype(np.float64)
    ref = np.fft.rfft(x64, axis=1)[:, :7]
    bound = 2.0 * n * EPS * np.abs(x64).sum(axis=1)[:, None]
    got = lowz.cpu().numpy()
    err_re, err_im = np.abs(got.real - ref.real), np.abs(got.imag - ref.imag)
    print(f"n={n}: worst error / bound {np.max(np.maximum(err_re, err_im)[bound[:, 0] > 0] / bound[bound[:, 0] > 0]):.3g}")
    assert np.all(err_re <= bound) and np.all(err_im <= bound)           # (the empty row: exactly zero)


def test_fused_z_sums_give_the_modes_of_the_separate_kernel(dev, hip):
    """The low-k modes from the z pass's own z sums (ast_lowk_modes_from_z) against those of ast_lowk_modes, which
    reads the planes a second time, on a 256^3 random grid.  A row's z sum is off by at most b = 2 N 2^-53 sum_z |x_z|
    (the test above); a mode adds the N^2 rows with factors of modulus one, so the two results may differ by N^2
    times the largest b."""
    from astrild_amd import _lib
    n = 256
    g = torch.Generator(device="cuda").manual_seed(5)
    grid = torch.randn((n, n, n), generator=g, device="cuda", dtype=torch.float32) + 0.5
    ref = dev.lowk_modes(grid, n)
    work = torch.zeros(int(hip.ast_lowk_work_bytes(n, n)) // 16, dtype=torch.complex128, device="cuda")
    _rows_with_z_sums(dev, hip, grid, n, work)
    got = torch.empty_like(ref)
    _lib.check(hip.ast_lowk_modes_from_z(n, 0, n, 0, dev.ptr(got), dev.ptr(work), work.numel() * 16, dev.stream()),
               "ast_lowk_modes_from_z")
    tol = float(n) ** 2 * 2.0 * n * EPS * grid.double().abs().sum(dim=2).max().item()
    diff = torch.view_as_real(got - ref).abs().max().item()
    print(f"largest difference {diff:.3g}, tolerance {tol:.3g}, largest mode {ref.abs().max().item():.3g}")
    assert ref.abs().max().item() > 1e3                                  # (the modes are there: sqrt(N^3) = 4096)
    assert diff <= tol


@pytest.fixture(scope="module")
def edge_particles():
    """2^20 particles of a 1024^3 box of unit cells that sit in the cells x, y = 0 and 7 mod 8 - the edges and corners
    of the paint's 8 x 8 tile columns, whose deposits go through the halo records - 4096 of them in the box's four
    corner columns (cells 0 and 1023 in x and y) and 4096 in the first and last z plane, so that records and windows
    wrap around every axis.  The particles are in random order."""
    n, npart = 1024, 1 << 20
    rng = np.random.default_rng(77)
    cell = np.empty((npart, 3), dtype=np.int64)
    cell[:, :2] = 8 * rng.integers(0, n // 8, size=(npart, 2)) + 7 * rng.integers(0, 2, size=(npart, 2))
    cell[:, 2] = rng.integers(0, n, size=npart)
    cell[:4096, :2] = (n - 1) * rng.integers(0, 2, size=(4096, 2))          # the box's corner columns, any z
    cell[4096:8192, 2] = (n - 1) * rng.integers(0, 2, size=4096)            # the first and the last z plane
    pos = (cell + rng.uniform(0.05, 0.95, size=(npart, 3))).astype(np.float32)
    assert pos.min() >= 0.0 and pos.max() < n
    return pos


@pytest.mark.parametrize("window", ["cic", "tsc"])
def test_fold_on_load_at_side_1024_with_particles_on_tile_edges(dev, edge_particles, window):
    """paint(defer_fold=True) + power_sums_fused(halo=) against the paint that folds its records itself, at side 1024
    with every particle on a tile edge or corner: rows that take one, two and three record lines in the (16, 32)
    instantiation, the periodic wrap included.  All shell sums are the same bits.  The paint takes its exact
    two-pass lists ("tiled2"), which hold every particle: on the single pass a set in random order goes through the
    bucket scatter, whose late list is deposited onto the grid after the paint's own fold but before the z pass's -
    the same terms in another order, and how many records the list gets differs from run to run."""
    n, L = 1024, 1024.0
    pos = dev.as_device(edge_particles)
    mean = pos.shape[0] / float(n) ** 3
    grid = dev.paint(pos, None, n, L, window, method="tiled2")
    _, ref, _ = dev.power_sums_fused(grid, L, mean=mean)
    ref = ref.clone()
    grid2, halo = dev.paint(pos, None, n, L, window, method="tiled2", defer_fold=True)
    assert not torch.equal(grid2, grid)                                  # the deferred grid alone is incomplete
    del grid
    _, got, _ = dev.power_sums_fused(grid2, L, mean=mean, halo=halo)
    assert torch.isfinite(ref).all() and ref.abs().max().item() > 0.0
    assert torch.equal(got, ref)
