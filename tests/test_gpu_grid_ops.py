"""GPU: the vector-grid kernels of csrc/grid_ops.hip through device.py and MapTransform.  The oracle of the stencil is
numpy itself: device.divergence must equal np.gradient(..., edge_order=2) summed over the axes bit for bit, at both
dtypes and through both kernels (ASTRILD_DIVERGENCE_TILED=0 / 1); the periodic form is restated here with np.roll."""

import numpy as np
import pytest
import torch

from astrild_amd import device as dev
from astrild_amd import formats
from astrild_amd.particles.hutils import MapTransform
from oracle import fftpower as offt

pytestmark = pytest.mark.gpu

SPACINGS = (1 / 500, 1 / 137.3, 0.78125)
# every cell an edge cell; odd, unaligned rows; sides below, equal to and just above the streaming kernel's tile of
# 4 x 64 (float32) or 8 x 64 (float64) cells in (y, z) and its march chunks of at least 8 planes along axis 0; a
# partial tile on every axis; one more than whole tiles on each axis with a chunk boundary on axis 0
SHAPES = ((3, 3, 3), (4, 5, 7), (33, 8, 65), (64, 64, 64), (130, 34, 67), (19, 17, 129))
DTYPES = (np.float32, np.float64)


def np_divergence(v, h):
    return (np.gradient(v[:, :, :, 0], h, axis=0, edge_order=2) + np.gradient(v[:, :, :, 1], h, axis=1, edge_order=2)
            + np.gradient(v[:, :, :, 2], h, axis=2, edge_order=2))


def np_divergence_periodic(v, h):
    two_h = v.dtype.type(2.0 * h)
    d = [(np.roll(v[:, :, :, a], -1, axis=a) - np.roll(v[:, :, :, a], 1, axis=a)) / two_h for a in range(3)]
    return (d[0] + d[1]) + d[2]


def random_grid(shape, dtype, seed=0):
    return np.random.default_rng(seed).standard_normal(tuple(shape) + (3,)).astype(dtype)


@pytest.fixture(params=("0", "1"), ids=("cell", "tiled"))
def variant(request, monkeypatch):
    monkeypatch.setenv("ASTRILD_DIVERGENCE_TILED", request.param)
    return request.param


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_divergence_equals_np_gradient_bit_for_bit(hip, variant, shape, dtype):
    v = random_grid(shape, dtype, seed=sum(shape))
    vd = dev.as_device(v)
    for h in SPACINGS:
        got = dev.to_numpy(dev.divergence(vd, h))
        ref = np_divergence(v, h)
        assert got.dtype == ref.dtype == dtype and got.shape == tuple(shape)
        np.testing.assert_array_equal(got, ref, err_msg=f"h={h}")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_periodic_divergence_equals_the_roll_restatement(hip, variant, shape, dtype):
    v = random_grid(shape, dtype, seed=1 + sum(shape))
    vd = dev.as_device(v)
    for h in SPACINGS:
        got = dev.to_numpy(dev.divergence(vd, h, periodic=True))
        np.testing.assert_array_equal(got, np_divergence_periodic(v, h), err_msg=f"h={h}")


def test_periodic_divergence_of_plane_waves(hip, variant):
    n, L, m = 16, 100.0, (1, 3, 5)
    h = L / n
    x = np.stack(np.meshgrid(*(np.arange(n),) * 3, indexing="ij"), axis=-1).astype(np.float64)
    v = np.sin(2 * np.pi * np.array(m) * x / n)
    exact = sum(np.sin(2 * np.pi * m[a] / n) / h * np.cos(2 * np.pi * m[a] * x[..., a] / n) for a in range(3))
    got = dev.to_numpy(dev.divergence(v, h, periodic=True))
    print("largest error", abs(got - exact).max(), "numpy restatement", abs(np_divergence_periodic(v, h) - exact).max())
    np.testing.assert_allclose(got, exact, rtol=0, atol=1e-14)


@pytest.mark.parametrize("periodic", (False, True), ids=("edges", "periodic"))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_both_kernels_give_the_same_bits(hip, monkeypatch, dtype, periodic):
    vd = dev.as_device(random_grid((96, 40, 72), dtype, seed=5))
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("ASTRILD_DIVERGENCE_TILED", flag)
        outs.append(dev.divergence(vd, 0.37, periodic=periodic))
    assert torch.equal(outs[0], outs[1])
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0


def test_divergence_arguments(hip):
    v = dev.as_device(random_grid((4, 4, 4), np.float64))
    out = torch.empty((4, 4, 4), dtype=torch.float64, device=v.device)
    assert dev.divergence(v, 0.5, out=out) is out
    np.testing.assert_array_equal(dev.to_numpy(out), np_divergence(dev.to_numpy(v), 0.5))
    with pytest.raises(ValueError):
        dev.divergence(v[:2], 0.5)
    with pytest.raises(ValueError):
        dev.divergence(v, 0.0)
    # the C entry refuses what the Python checks would have caught
    from astrild_amd import _lib
    assert hip.ast_grid_divergence(dev.ptr(v), dev.ptr(out), _lib.F64, 2, 4, 4, 0.5, 0, 1, dev.stream()) != 0
    assert hip.ast_grid_divergence(dev.ptr(v), dev.ptr(out), _lib.F64, 4, 4, 4, 0.5, 0, 2, dev.stream()) != 0


def test_vector_magnitude(hip):
    v = np.random.default_rng(11).standard_normal((5, 6, 7, 3))
    ref = np.sqrt(np.sum(np.square(v), axis=3))
    got = dev.to_numpy(dev.vector_magnitude(v))
    assert got.shape == (5, 6, 7)
    np.testing.assert_array_equal(got, ref)
    v32 = v.astype(np.float32)
    ref32 = np.sqrt(np.sum(np.square(v32), axis=3))
    got32 = dev.to_numpy(dev.vector_magnitude(v32))
    assert got32.dtype == np.float32
    assert np.all(np.abs(got32 - ref32) <= np.spacing(ref32))
    with pytest.raises(ValueError):
        dev.vector_magnitude(v[..., :2])


def np_modes(n):
    m = np.fft.fftfreq(n, 1.0 / n)
    m[n // 2] = 0.0
    mz = np.arange(n // 2 + 1, dtype=np.float64)
    mz[n // 2] = 0.0
    return m[:, None, None], m[None, :, None], mz[None, None, :]


def np_spectral_divergence(cx, cy, cz, n, L):
    k0, k1, k2 = (2 * np.pi / L * m for m in np_modes(n))
    return 1j * ((k0 * cx + k1 * cy) + k2 * cz)


@pytest.mark.parametrize("cdtype", (np.complex128, np.complex64), ids=("c128", "c64"))
@pytest.mark.parametrize("n", (8, 32))
def test_spectral_divergence(hip, n, cdtype):
    L = 100.0
    rng = np.random.default_rng(n)
    shape = (n, n, n // 2 + 1)
    c = [(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdtype) for _ in range(3)]
    cd = [dev.as_device(a) for a in c]
    got = dev.to_numpy(dev.spectral_divergence(*cd, n, L))
    assert got.dtype == cdtype
    wide = [a.astype(np.complex128) for a in c]
    ref = np_spectral_divergence(*wide, n, L)
    k = [abs(2 * np.pi / L * m) for m in np_modes(n)]
    eps = np.finfo(np.float32 if cdtype == np.complex64 else np.float64).eps
    tol = 8 * eps * sum(ka * abs(a) for ka, a in zip(k, wide))
    err = abs(got.astype(np.complex128) - ref)
    print("largest error / tolerance", (err[tol > 0] / tol[tol > 0]).max())
    assert np.all(err <= tol)
    # the Nyquist plane of an axis carries nothing of that axis's component: m = 0 there
    h = n // 2
    ks = [2 * np.pi / L * m for m in np_modes(n)]
    for axis, others in ((0, (1, 2)), (1, (0, 2)), (2, (0, 1))):
        plane = (slice(None),) * axis + (h,)
        expect = 1j * (ks[others[0]] * wide[others[0]] + ks[others[1]] * wide[others[1]])
        assert np.all(abs(got[plane] - expect[plane]) <= tol[plane])
        changed = [a.copy() for a in c]
        changed[axis][plane] = 7.0 - 3.0j
        again = dev.to_numpy(dev.spectral_divergence(*(dev.as_device(a) for a in changed), n, L))
        np.testing.assert_array_equal(again[plane], got[plane])
    # in place on the first spectrum
    aliased = dev.spectral_divergence(cd[0], cd[1], cd[2], n, L, out=cd[0])
    assert aliased is cd[0]
    np.testing.assert_array_equal(dev.to_numpy(aliased), got)


def band_limited_velocity(n, seed):
    """(n, n, n, 3) float64, no power above a quarter of the sampling frequency on any axis."""
    rng = np.random.default_rng(seed)
    m0, m1, m2 = np_modes(n)
    keep = (abs(m0) <= n // 4) & (abs(m1) <= n // 4) & (abs(m2) <= n // 4)
    keep[n // 2], keep[:, n // 2], keep[:, :, n // 2] = False, False, False
    comps = [np.fft.irfftn(np.fft.rfftn(rng.standard_normal((n, n, n))) * keep, s=(n, n, n), axes=(0, 1, 2)) for _ in range(3)]
    return np.ascontiguousarray(np.stack(comps, axis=-1))


def assert_same_power(res, ref):
    assert np.array_equal(res["modes"], ref["modes"])
    np.testing.assert_allclose(res["k"], ref["k"], rtol=1e-12)
    power = ref["power"].real
    np.testing.assert_allclose(res["power"], power, rtol=1e-9, atol=1e-9 * np.nanmax(power))


@pytest.mark.parametrize("n", (32, 64))
def test_velocity_divergence_power(hip, n):
    L = 100.0
    v = band_limited_velocity(n, seed=n)
    spectra = [np.fft.rfftn(v[..., a]) for a in range(3)]
    theta = np.fft.irfftn(np_spectral_divergence(*spectra, n, L), s=(n, n, n), axes=(0, 1, 2))
    res = dev.velocity_divergence_power(v, L)
    assert res["shotnoise"] == 0.0
    assert_same_power(res, offt.fftpower_1d(theta, L))
    # a float32 grid is widened: the same spectrum to fp32 input rounding
    res32 = dev.velocity_divergence_power(v.astype(np.float32), L)
    np.testing.assert_allclose(res32["power"], res["power"], rtol=1e-4, atol=1e-6 * np.nanmax(res["power"]))
    # the finite-difference theta through the ordinary spectrum
    fd = dev.divergence(v, L / n, periodic=True)
    assert_same_power(dev.fftpower_1d(fd, L), offt.fftpower_1d(np_divergence_periodic(v, L / n), L))


class _Sim:
    boxsize = 500.0
    npar = 16

    def __init__(self, directory, names):
        self.dirs = {"sim": str(directory)}
        self.dir_nrs = [1, 2, 3]
        self._names = list(names)

    def get_file_nrs(self, file_dsc, directory, uniques):
        return self.dir_nrs[:len(self._names)]

    def get_file_paths(self, file_dsc, directory, uniques):
        return [str(directory) + "/" + name for name in self._names]


def test_map_transform_end_to_end(hip, tmp_path):
    v = random_grid((16, 16, 16), np.float64, seed=3)
    v32 = random_grid((16, 16, 16), np.float32, seed=4)
    np.save(tmp_path / "dtfe_001.npy", v)
    formats.write_density_grid(str(tmp_path / "dtfe_002.a_vel"), v32, 500.0, file_type=11)
    sim = _Sim(tmp_path, ["dtfe_001.npy", "dtfe_002.a_vel"])
    mt = MapTransform("particles", sim)
    assert mt.divergence() is None
    h = 1 / sim.boxsize
    np.testing.assert_array_equal(np.load(tmp_path / "div_dtfe_001.npy"), np_divergence(v, h))
    saved32 = np.load(tmp_path / "div_dtfe_002.a_vel.npy")
    assert saved32.dtype == np.float32
    np.testing.assert_array_equal(saved32, np_divergence(v32, h))
    # save=False: the first snapshot's array; spacing= and periodic= reach the kernel
    first = mt.divergence(save=False, spacing=0.25, periodic=True)
    assert isinstance(first, np.ndarray)
    np.testing.assert_array_equal(first, np_divergence_periodic(v, 0.25))
    # a device tensor stays on the device
    vd = dev.as_device(v)
    on_device = mt._compute_divergence(vd)
    assert isinstance(on_device, torch.Tensor) and on_device.is_cuda
    np.testing.assert_array_equal(dev.to_numpy(on_device), np_divergence(v, h))
    assert isinstance(mt._compute_divergence(v), np.ndarray)


def restate_cells(values, h, T):
    """The stencil of ast_grid_divergence (non-periodic) from gathered values: values[a] is (cells, 3), the line values
    (f[i-1], f[i+1], unused) of an interior cell of axis a, (f[0], f[1], f[2]) of a first and (f[n-3], f[n-2], f[n-1])
    of a last cell, with the kind in values[a + 3] (0 interior, 1 first, 2 last)."""
    d = []
    for a in range(3):
        f, kind = values[a], values[a + 3]
        central = (f[:, 1] - f[:, 0]) / T(2.0 * h)
        first = (T(-1.5 / h) * f[:, 0] + T(2.0 / h) * f[:, 1]) + T(-0.5 / h) * f[:, 2]
        last = (T(0.5 / h) * f[:, 0] + T(-2.0 / h) * f[:, 1]) + T(1.5 / h) * f[:, 2]
        d.append(np.where(kind == 0, central, np.where(kind == 1, first, last)))
    return (d[0] + d[1]) + d[2]


def test_restate_cells_is_np_gradient():
    """The sampled restatement used at the large size below, against numpy on a whole small grid (no GPU work)."""
    shape, h = (4, 5, 7), 1 / 137.3
    v = random_grid(shape, np.float32, seed=2)
    cells = np.stack(np.unravel_index(np.arange(np.prod(shape)), shape), axis=1)
    idx, kinds = stencil_indices(cells, shape)
    values = [v.reshape(-1)[idx[a]] for a in range(3)] + kinds
    np.testing.assert_array_equal(restate_cells(values, h, np.float32).reshape(shape), np_divergence(v, h))


def stencil_indices(cells, shape):
    """Flat element indices (cells, 3) per axis of the values restate_cells wants, and the cell kinds per axis."""
    shape = np.asarray(shape, dtype=np.int64)
    idx, kinds = [], []
    for a in range(3):
        i, n = cells[:, a], shape[a]
        kind = np.where(i == 0, 1, np.where(i == n - 1, 2, 0))
        line = np.where(kind[:, None] == 0, np.stack([i - 1, i + 1, i], axis=1),
                        np.where(kind[:, None] == 1, np.array([0, 1, 2]), np.array([n - 3, n - 2, n - 1])))
        at = np.repeat(cells[:, None, :], 3, axis=1)
        at[:, :, a] = line
        idx.append(((at[:, :, 0] * shape[1] + at[:, :, 1]) * shape[2] + at[:, :, 2]) * 3 + a)
        kinds.append(kind)
    return idx, kinds


def test_divergence_past_2_to_the_32_elements(hip, monkeypatch):
    """(4, 4, 89 478 486) float32: 17.2 GB in, 5.7 GB out, the input's flat element index passes 2^32.  4096 sampled
    cells - the eight corners, the cells about element offsets 2^31 and 2^32, random ones - against the restatement,
    through both kernels."""
    shape = (4, 4, 89_478_486)
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < 32 * 2 ** 30:
        pytest.skip(f"torch.cuda.mem_get_info() reports {free / 2 ** 30:.1f} GB free, fewer than 32 GB")
    assert 3 * np.prod(shape, dtype=np.int64) > 2 ** 32
    h = 1 / 137.3
    rng = np.random.default_rng(9)
    cells = [[x, y, z] for x in (0, 3) for y in (0, 3) for z in (0, shape[2] - 1)]
    for offset in (2 ** 31, 2 ** 32):
        for cell in range(offset // 3 - 4, offset // 3 + 5):
            cells.append(list(np.unravel_index(cell, shape)))
            for axis in (0, 1):                                 # and their neighbours across the slow axes
                near = list(np.unravel_index(cell, shape))
                near[axis] = (near[axis] + 1) % 4
                cells.append(near)
    cells = np.array(cells, dtype=np.int64)
    more = np.stack([rng.integers(0, s, 4096 - len(cells)) for s in shape], axis=1)
    cells = np.concatenate([cells, more])
    assert len(cells) == 4096
    idx, kinds = stencil_indices(cells, shape)
    assert max(int(i.max()) for i in idx) > 2 ** 32
    gen = torch.Generator(device=dev.device()).manual_seed(17)
    v = torch.randn(shape + (3,), dtype=torch.float32, device=dev.device(), generator=gen)
    flat = v.reshape(-1)
    values = [flat[dev.as_device(i.reshape(-1))].cpu().numpy().reshape(-1, 3) for i in idx] + kinds
    ref = restate_cells(values, h, np.float32)
    assert np.isfinite(ref).all() and np.count_nonzero(ref) > 4000
    at = dev.as_device((cells[:, 0] * shape[1] + cells[:, 1]) * shape[2] + cells[:, 2])
    out = torch.empty(shape, dtype=torch.float32, device=v.device)
    for flag in ("1", "0"):
        monkeypatch.setenv("ASTRILD_DIVERGENCE_TILED", flag)
        out.zero_()
        dev.divergence(v, h, out=out)
        np.testing.assert_array_equal(out.reshape(-1)[at].cpu().numpy(), ref, err_msg=f"ASTRILD_DIVERGENCE_TILED={flag}")
    del v, out, flat
    torch.cuda.empty_cache()
