"""GPU: every wrapper that allocates scratch or output memory with ``torch.empty`` / ``empty_like`` / ``new_empty``,
run on DIRTY memory (tests/dirty_memory.py): every byte of every such buffer is 0xFF (NaN, -1, UINT_MAX) or 0x7F (huge
finite floats, huge positive integers) when the kernel sees it.  The C ABI's contract for these buffers is "contents
undefined on entry" (include/astrild_hip.h); a kernel that relies on a missing memset, or leaves one slot unwritten,
differs from its oracle here while it passes on the fresh or recycled blocks of the ordinary suite.

Each case compares with the oracle of the kernel's own test module at that module's tolerance; integer outputs exactly.
Results the project documents as order independent are also bit-identical to the same call on all-zero memory.  Every
case asserts that the call under test drew at least one poisoned allocation, so none passes vacuously.

Not reached: memory the library takes with hipMalloc itself (plan internals, twiddle / lane tables, side-stream
scratch) - see tests/test_gpu_call_order.py.  c2r_tile, c2r_tile_batch and the triangle-sum kernels are poisoned in
tests/test_gpu_bispectrum_kernels.py already.
"""
import functools

import numpy as np
import numpy.testing as npt
import pytest

from oracle import fftpower as offt, kappa as ok, mesh as omesh
from tests import dirty_memory as dm
from tests import pairwise_oracle as tv_orc
from tests import pairwise_pdf_oracle as pdf_orc
from tests import tpcf_oracle as tpcf_orc
from tests import tunnels_oracle as tun_orc
from tests.dirty_memory import dirty_alloc                         # noqa: F401  (the fixture: one run per pattern)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def dev(hip):
    from astrild_amd import device
    return device


@pytest.fixture(scope="module")
def lens(hip):
    from astrild_amd import lensing
    return lensing


# ------------------------------------------------------------------ helpers
def _host(v):
    """Outputs as numpy, whatever the wrapper returns (tensors, arrays, numbers, tuples / lists / dicts of them)."""
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    if isinstance(v, dict):
        return {k: _host(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return tuple(_host(x) for x in v)
    return v


def _leaves(v):
    if isinstance(v, dict):
        for k in sorted(v):
            yield from _leaves(v[k])
    elif isinstance(v, (tuple, list)):
        for x in v:
            yield from _leaves(x)
    else:
        yield np.asarray(v)


def dirty_call(alloc, fn):
    """fn() on dirty memory, as numpy; the call must have drawn at least one poisoned allocation."""
    mark, nbytes = alloc.mark(), alloc.bytes
    out = _host(fn())
    torch.cuda.synchronize()
    assert alloc.since(mark) > 0 and alloc.bytes > nbytes, "the call under test drew no poisoned allocation"
    return out


def zero_call(alloc, fn):
    """The same call with every such buffer all zero: the control of a bit-identity case."""
    with alloc.using(dm.ZERO_BYTES):
        return _host(fn())


def assert_same_bits(got, want):
    a, b = list(_leaves(got)), list(_leaves(want))
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()


def assert_finite_where(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.isfinite(got[np.isfinite(ref)]).all()


def close(got, ref, rtol, atol=0.0):
    assert_finite_where(got, ref)
    npt.assert_allclose(got, ref, rtol=rtol, atol=atol)


def buffers(alloc):
    """What arrived dirty, for the record (pytest -s)."""
    seen = {}
    for dtype, shape in alloc.log:
        seen[(str(dtype).replace("torch.", ""), shape)] = seen.get((str(dtype).replace("torch.", ""), shape), 0) + 1
    return ", ".join(f"{d}{list(s)}" + (f" x{c}" if c > 1 else "") for (d, s), c in seen.items())


@pytest.fixture(autouse=True)
def _report(request):
    yield
    alloc = request.node.funcargs.get("dirty_alloc")
    if alloc is not None:
        print(f"\nDIRTY {request.node.name}: {alloc.allocations} buffers, {alloc.bytes} bytes: {buffers(alloc)}")


# ------------------------------------------------------------------ the helper itself, and the positive control
CUDA_DTYPES = [torch.float32, torch.float64, torch.complex64, torch.complex128, torch.int32, torch.int64, torch.uint8]


def test_helper_patched_empty_holds_the_pattern_in_every_byte(dirty_alloc):
    p = dirty_alloc.pattern
    for dtype in CUDA_DTYPES:
        src = torch.ones((5, 3), dtype=dtype, device="cuda")
        for t in (torch.empty((7, 9), dtype=dtype, device="cuda"), torch.empty_like(src), src.new_empty((4, 2, 3))):
            assert t.is_cuda and t.dtype == dtype and dm.all_bytes_are(t, p)
            assert np.all(t.cpu().numpy().view(np.uint8) == p)
    assert dirty_alloc.allocations == 3 * len(CUDA_DTYPES)
    # pinned-host and meta tensors, empty tensors and torch.zeros pass through
    host = torch.empty(64, dtype=torch.int64, pin_memory=True)
    host.zero_()
    assert torch.empty(8, device="meta").device.type == "meta" and torch.empty(0, device="cuda").numel() == 0
    assert bool((torch.zeros(16, dtype=torch.float64, device="cuda") == 0).all())
    assert dirty_alloc.allocations == 3 * len(CUDA_DTYPES)
    f64 = torch.empty(4, dtype=torch.float64, device="cuda")
    i64 = torch.empty(4, dtype=torch.int64, device="cuda")
    if p == dm.NAN_BYTES:
        assert bool(torch.isnan(f64).all()) and bool((i64 == -1).all())
    else:
        assert bool(torch.isfinite(f64).all()) and float(f64[0]) > 1.3e306 and bool((i64 == 0x7F7F7F7F7F7F7F7F).all())


def test_control_power_bin_1d_adds_onto_a_poisoned_psum(dev, dirty_alloc):
    """The poison is visible to kernels: ``psum`` of power_bin_1d is documented as ``+=``, so a caller-supplied psum from
    the patched torch.empty stays NaN under 0xFF and huge under 0x7F - and the same call with the wrapper's own
    torch.zeros psum matches the oracle."""
    n, L = 32, 100.0
    field = np.random.default_rng(2).standard_normal((n, n, n))
    spec = dev.r2c(dev.as_device(field))
    mark = dirty_alloc.mark()
    psum = torch.empty(n // 2 - 1, dtype=torch.float64, device="cuda")
    assert dirty_alloc.since(mark) == 1
    _, got, _ = dev.power_bin_1d(spec, None, n, L, psum=psum)
    got = got.cpu().numpy()
    if dirty_alloc.pattern == dm.NAN_BYTES:
        assert not np.isfinite(got).any()
    else:
        assert np.isfinite(got).all() and (got > 1.3e306).all()
    res = dev.finish_power(*dev.power_bin_1d(spec, None, n, L))
    ref = offt.fftpower_1d(field, L)
    assert np.array_equal(res["modes"], ref["modes"])
    close(res["power"], ref["power"].real, rtol=1e-12)


# ================================================================== pair finders
from tests import test_gpu_pairwise as t_tv                        # noqa: E402
from tests import test_gpu_pairwise_pdf as t_pdf                   # noqa: E402
from tests import test_gpu_tpcf as t_tpcf                          # noqa: E402


@functools.lru_cache(maxsize=None)
def _tv_case(ncomp):
    pos, _ = tv_orc.light_cone(4000, seed=9, clusters=200, sigma=6.0)
    vel = t_tv.coherent_velocities(pos, 2)
    if ncomp == 3:
        vel = np.concatenate([vel, np.random.default_rng(4).normal(0.0, 50.0, (len(pos), 1))], axis=1)
        u = pos / np.sqrt((pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1]) + pos[:, 2] * pos[:, 2])[:, None]
        ref = tv_orc.pair_sums(pos, u, vel, 40, 50.0 / 39)
    else:
        ref = t_tv.oracle_sums(pos, vel, 40, 50.0 / 39)
    assert ref[2].sum() > 10_000 and ref[2][-1] > 0
    return pos, vel, ref


@pytest.mark.parametrize("ncomp", [2, 3], ids=["ra_dec", "cartesian"])
@pytest.mark.parametrize("cells", ["1", "0"], ids=["grid", "one_cell"])
def test_pairwise_tv(dev, dirty_alloc, monkeypatch, cells, ncomp):
    monkeypatch.setenv("ASTRILD_PV_CELLS", cells)
    pos, vel, ref = _tv_case(ncomp)
    got = dirty_call(dirty_alloc, lambda: dev.pairwise_tv(pos, vel, 40, 50.0 / 39))
    assert got[2].dtype == np.int64
    for g, r in zip(got[:2], ref[:2]):
        assert_finite_where(g, r)
    t_tv.assert_same(got, ref)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_pairwise_tv_early_returns(dev, dirty_alloc, n):
    pos = np.array([[10.0, -4.0, 1000.0], [12.0, -3.0, 1003.0]])[:n]
    vel = np.array([[30.0, -20.0], [-10.0, 45.0]])[:n]
    got = dirty_call(dirty_alloc, lambda: dev.pairwise_tv(pos, vel, 40, 1.25))
    if n < 2:
        assert not got[0].any() and not got[1].any() and not got[2].any() and len(got[2]) == 40
    else:
        ref = t_tv.oracle_sums(pos, vel, 40, 1.25)
        assert ref[2].sum() == 1
        t_tv.assert_same(got, ref)


PDF_CASES = {
    # name: (catalogue, extra parameters, environment)
    "lds": ("compact", {}, {}),
    "global_forced": ("compact", {}, {"ASTRILD_PVPDF_LDS": "0"}),
    "one_cell": ("compact", {}, {"ASTRILD_PVPDF_CELLS": "0"}),
    "grid": ("light_cone", {}, {}),
    "rows": ("compact", {"ffirst": 700, "ssecond": 3000}, {}),
}


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "hist_only"])
@pytest.mark.parametrize("kind", t_pdf.KINDS)
@pytest.mark.parametrize("case", list(PDF_CASES))
def test_pairwise_velocity_pdf(dev, dirty_alloc, monkeypatch, case, kind, moments):
    name, extra, env = PDF_CASES[case]
    pos, vel, par = t_pdf.catalogue(name)
    ref = t_pdf.oracle(name, kind, tuple(sorted(extra.items())))
    assert ref["hist"].sum() > 0 and ref["outside"] > 0
    assert par["dist_bin"] * par["vel_bin"] <= t_pdf.lds_bins(par["dist_bin"], moments)       # a histogram that fits LDS
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mark = dirty_alloc.mark()
    got = t_pdf.gpu(pos, vel, kind, moments=moments, **{**par, **extra})
    assert dirty_alloc.since(mark) >= (6 if moments else 3)          # work, hist, outside (+ count, s1, s2)
    if moments:
        assert np.isfinite(got["s1"]).all() and np.isfinite(got["s2"]).all()
    t_pdf.assert_same(got, ref)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_pairwise_velocity_pdf_early_returns(dev, dirty_alloc, n):
    pos = np.array([[1.0, 2.0, 3.0], [1.5, 2.0, 5.0]])[:n]
    vel = np.array([[0.0, 0.0, 1.0], [0.5, 0.0, 4.0]])[:n]
    for kind in t_pdf.KINDS:
        mark = dirty_alloc.mark()
        got = t_pdf.gpu(pos, vel, kind, r=4.0, dist_bin=5, vel_bin=10)
        assert dirty_alloc.since(mark) >= 5
        if n < 2:
            assert not got["hist"].any() and got["outside"] == 0
            assert not got["count"].any() and not got["s1"].any() and not got["s2"].any()
        else:
            ref = pdf_orc.pair_pdf(pos, vel, 4.0, 5, 10, kind)
            assert ref["hist"].sum() + ref["outside"] == 1
            t_pdf.assert_same(got, ref)


@functools.lru_cache(maxsize=None)
def _tpcf_case(with_mu, with_vel):
    pos = tpcf_orc.clustered(5000, t_tpcf.L, 2, blobs=30, sigma=6.0)
    vel = np.random.default_rng(8).normal(0.0, 400.0, pos.shape) if with_vel else None
    mu = t_tpcf.MU40 if with_mu else None
    ref = t_tpcf.oracle_counts(pos, t_tpcf.L, t_tpcf.S50, mu, vel=vel)
    assert ref.sum() > 10_000
    return pos, vel, mu, ref


@pytest.mark.parametrize("flush", [None, "0"], ids=["flush_default", "flush_at_0"])
@pytest.mark.parametrize("cells", ["1", "0"], ids=["grid", "one_cell"])
@pytest.mark.parametrize("with_vel", [False, True], ids=["real", "redshift"])
@pytest.mark.parametrize("with_mu", [False, True], ids=["s", "s_mu"])
def test_tpcf_pair_counts(dev, dirty_alloc, monkeypatch, with_mu, with_vel, cells, flush):
    monkeypatch.setenv("ASTRILD_TPCF_CELLS", cells)
    if flush is not None:
        monkeypatch.setenv("AST_TPCF_FLUSH_AT", flush)
    pos, vel, mu, ref = _tpcf_case(with_mu, with_vel)
    call = lambda: dev.tpcf_pair_counts(pos, t_tpcf.L, t_tpcf.S50, mu_edges=mu, vel=vel)
    got = dirty_call(dirty_alloc, call)
    assert got.dtype == np.int64
    npt.assert_array_equal(got, ref)
    assert_same_bits(got, zero_call(dirty_alloc, call))


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tpcf_pair_counts_early_returns(dev, dirty_alloc, n):
    pos = np.array([[1.0, 2.0, 3.0], [2.0, 2.5, 4.0]])[:n]
    s, mu = np.array([0.0, 0.5, 1.0, 2.0]), np.array([0.0, 0.5, 1.0])
    for mu_edges in (None, mu):
        got = dirty_call(dirty_alloc, lambda: dev.tpcf_pair_counts(pos, 50.0, s, mu_edges=mu_edges))
        if n < 2:
            assert not got.any() and got.shape == ((3, 2) if mu_edges is not None else (3,))
        else:
            ref = tpcf_orc.pair_counts(pos, 50.0, s, mu_edges)
            assert ref.sum() == 1
            npt.assert_array_equal(got, ref)


# ================================================================== sky-map objects
from tests import test_gpu_profile2d as t_prof                     # noqa: E402
from tests import test_gpu_tunnels as t_tun                        # noqa: E402


@pytest.mark.parametrize("bands", ["1", "0"], ids=["bands", "one_item"])
@pytest.mark.parametrize("nbins", [1, 10])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_annulus_profiles(dev, dirty_alloc, monkeypatch, dtype, nbins, bands):
    monkeypatch.setenv("ASTRILD_PROFILE_BANDS", bands)
    extend = 3.0
    skymap = t_prof.random_map(64, 64, dtype, seed=3)
    x, y, r = t_prof.mixed_catalogue(20, 64, 64, 8, extend, seed=8)
    assert (x < 0).any() and (y < 0).any() and (x >= 0).any()          # some objects wrap through negative indices
    call = lambda: dev.annulus_profiles(skymap, x, y, r, extend, nbins)
    s, c = dirty_call(dirty_alloc, call)
    os_, oc = t_prof.oracle(skymap, x, y, r, extend, nbins)
    assert c.dtype == np.int64 and oc.sum() > 0
    npt.assert_array_equal(c, oc)
    assert np.isfinite(s).all()
    assert np.all(np.abs(s - os_) <= 1e-12 * t_prof.abs_sums(skymap, x, y, r, extend, nbins))
    assert_same_bits((s, c), zero_call(dirty_alloc, call))               # (test_bit_identical_on_repeat: a fixed order)


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "tensors"])
@pytest.mark.parametrize("cells", ["1", "0"], ids=["grid", "one_cell"])
def test_tunnels_voids(dev, dirty_alloc, monkeypatch, cells, on_device):
    monkeypatch.setenv("ASTRILD_TUNNELS_CELLS", cells)
    P = t_tun.distinct(np.random.RandomState(17), 200, 256)
    want = tun_orc.circles(P, 256)
    assert len(want) > 200
    x, y = P[:, 0].astype(np.int32), P[:, 1].astype(np.int32)
    if on_device:
        x, y = dev.as_device(x), dev.as_device(y)

    def call():
        rec, violations = dev.tunnels_voids(x, y, 256, return_violations=True)
        assert violations == 0 and isinstance(rec, torch.Tensor) == on_device
        return rec
    got = dirty_call(dirty_alloc, call)
    assert got.dtype == np.int64
    npt.assert_array_equal(got, want)
    assert_same_bits(got, zero_call(dirty_alloc, call))


# ================================================================== grid operations
from tests import test_gpu_grid_ops as t_grid                      # noqa: E402

GRID_SHAPES = ((3, 3, 3), (33, 8, 65), (19, 17, 129))


@pytest.mark.parametrize("periodic", [False, True], ids=["edges", "periodic"])
@pytest.mark.parametrize("tiled", ["0", "1"], ids=["cell", "tiled"])
@pytest.mark.parametrize("dtype", t_grid.DTYPES, ids=["f32", "f64"])
def test_divergence(dev, dirty_alloc, monkeypatch, dtype, tiled, periodic):
    monkeypatch.setenv("ASTRILD_DIVERGENCE_TILED", tiled)
    for shape in GRID_SHAPES:
        v = t_grid.random_grid(shape, dtype, seed=sum(shape))
        vd = dev.as_device(v)
        h = t_grid.SPACINGS[1]
        call = lambda: dev.divergence(vd, h, periodic=periodic)
        got = dirty_call(dirty_alloc, call)
        ref = t_grid.np_divergence_periodic(v, h) if periodic else t_grid.np_divergence(v, h)
        assert got.dtype == dtype
        npt.assert_array_equal(got, ref)
        assert_same_bits(got, zero_call(dirty_alloc, call))


def test_vector_magnitude(dev, dirty_alloc):
    v = np.random.default_rng(11).standard_normal((5, 6, 7, 3))
    call = lambda: dev.vector_magnitude(v)
    got = dirty_call(dirty_alloc, call)
    npt.assert_array_equal(got, np.sqrt(np.sum(np.square(v), axis=3)))
    assert_same_bits(got, zero_call(dirty_alloc, call))
    v32 = v.astype(np.float32)
    ref32 = np.sqrt(np.sum(np.square(v32), axis=3))
    got32 = dirty_call(dirty_alloc, lambda: dev.vector_magnitude(v32))
    assert got32.dtype == np.float32 and np.all(np.abs(got32 - ref32) <= np.spacing(ref32))


@pytest.mark.parametrize("cdtype", (np.complex128, np.complex64), ids=("c128", "c64"))
@pytest.mark.parametrize("n", (8, 32))
def test_spectral_divergence(dev, dirty_alloc, n, cdtype):
    L = 100.0
    rng = np.random.default_rng(n)
    shape = (n, n, n // 2 + 1)
    c = [(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdtype) for _ in range(3)]
    cd = [dev.as_device(a) for a in c]
    call = lambda: dev.spectral_divergence(*cd, n, L)
    got = dirty_call(dirty_alloc, call)
    wide = [a.astype(np.complex128) for a in c]
    ref = t_grid.np_spectral_divergence(*wide, n, L)
    k = [abs(2 * np.pi / L * m) for m in t_grid.np_modes(n)]
    eps = np.finfo(np.float32 if cdtype == np.complex64 else np.float64).eps
    tol = 8 * eps * sum(ka * abs(a) for ka, a in zip(k, wide))
    assert got.dtype == cdtype and np.isfinite(got.view(got.real.dtype)).all()
    assert np.all(abs(got.astype(np.complex128) - ref) <= tol)
    assert_same_bits(got, zero_call(dirty_alloc, call))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("in_place", [False, True], ids=["fresh", "in_place"])
def test_rsd_shift(dev, dirty_alloc, dtype, in_place):
    rng = np.random.default_rng(6)
    L, npart = 500.0, 5001
    pos = rng.uniform(0, L, (npart, 3)).astype(dtype)
    vel = rng.normal(0.0, 3000.0, (npart, 3)).astype(dtype)
    s = pos[:, 2].astype(np.float64) + 0.01 * vel[:, 2].astype(np.float64)          # (the restatement of test_gpu_fftpower2d.py)
    ref = np.where(s >= L, s - L, np.where(s < 0, s + L, s))
    assert np.sum(s >= L) > 50 and np.sum(s < 0) > 50                                # the wrap is exercised

    def call():
        p = dev.as_device(pos.copy())
        return dev.rsd_shift(p, dev.as_device(vel), L, los=2, out=p if in_place else None)
    got = dirty_call(dirty_alloc, call)
    assert got.dtype == dtype and np.isfinite(got).all()
    npt.assert_array_equal(got[:, :2], pos[:, :2])
    col = got[:, 2].astype(np.float64)
    d = np.abs(col - ref)
    assert np.all(col >= 0.0) and np.all(col < L) and np.all(np.minimum(d, L - d) <= 2 * float(np.spacing(dtype(L))))
    assert_same_bits(got, zero_call(dirty_alloc, call))


# ================================================================== paint
PAINT_TOL = {np.float64: 1e-12, np.float32: 2e-6}                  # test_paint_random_particles_with_mass
SCATTER_TOL = {np.float64: 1e-11, np.float32: 2e-6}                # test_scattered_path_two_level_bucket_scatter


@functools.lru_cache(maxsize=None)
def _paint_case(window, dtype):
    """test_paint_random_particles_with_mass's set: 70 000 particles in [-0.3 L, 1.3 L) with masses on a 64^3 grid."""
    rng = np.random.default_rng(11)
    n, L, npart = 64, 250.0, 70000
    pos = rng.uniform(-0.3 * L, 1.3 * L, size=(npart, 3)).astype(dtype)
    mass = rng.uniform(0.5, 2.0, size=npart).astype(dtype)
    ref = omesh.paint(pos, mass, n, L, window)
    ref.setflags(write=False)
    return n, L, pos, mass, ref


@functools.lru_cache(maxsize=None)
def _lattice_case(window, dtype):
    """64^3 particles in lattice order with masses: input the grouping kernel of the single pass turns into group records."""
    n, L = 64, 1000.0
    pos = omesh.lattice_particles(n, n, L, seed=20240601, dtype=dtype)
    mass = np.random.default_rng(31).uniform(0.5, 2.0, size=len(pos)).astype(dtype)
    ref = omesh.paint(pos, mass, n, L, window)
    ref.setflags(write=False)
    return n, L, pos, mass, ref


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("window", ["cic", "tsc"])
def test_paint_single_pass_on_ordered_input(dev, dirty_alloc, window, dtype):
    n, L, pos, mass, ref = _lattice_case(window, dtype)
    pd, md = dev.as_device(pos), dev.as_device(mass)
    stats = {}

    def call():
        stats.clear()
        return dev.paint(pd, md, n, L, window, method="tiled", accumulate=False, stats=stats)
    got = dirty_call(dirty_alloc, call)
    assert (stats["path"], stats["attempts"]) == ("single-pass", 1) and stats["groups"] > 0, stats
    tol = PAINT_TOL[dtype]
    close(got, ref, rtol=tol, atol=tol * ref.max())
    if stats["overflow"] == 0:
        assert_same_bits(got, zero_call(dirty_alloc, call))


@pytest.mark.parametrize("path", ["tiled", "tiled2", "scattered"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("window", ["cic", "tsc"])
def test_paint(dev, dirty_alloc, window, dtype, path):
    """out=None, accumulate=False: the grid itself comes from torch.empty, with the workspace (tile lists, halo records)
    and the list statistics."""
    n, L, pos, mass, ref = _paint_case(window, dtype)
    pd, md = dev.as_device(pos), dev.as_device(mass)
    kw = dict(method="tiled", hint="scattered") if path == "scattered" else dict(method=path)
    # (method="tiled" on particles without order in memory: the single pass, then - its overflow list too long - the
    # bucket scatter: both attempts run on dirty memory)
    want = {"tiled": ("single-pass", "scattered"), "tiled2": ("two-pass",), "scattered": ("scattered",)}[path]
    stats = {}

    def call():
        stats.clear()
        return dev.paint(pd, md, n, L, window, accumulate=False, stats=stats, **kw)
    got = dirty_call(dirty_alloc, call)
    print("paint", path, stats)
    assert stats["path"] in want and stats["attempts"] == (1 if stats["path"] == want[0] else 2), stats
    assert got.dtype == dtype and got.shape == (n, n, n)
    tol = (SCATTER_TOL if path == "scattered" else PAINT_TOL)[dtype]
    close(got, ref, rtol=tol, atol=tol * ref.max())
    assert got.sum(dtype=np.float64) == pytest.approx(mass.sum(dtype=np.float64), rel=1e-6)
    if stats.get("overflow", 0) == 0:                               # no list of float atomics: a fixed order of additions
        assert_same_bits(got, zero_call(dirty_alloc, call))


@pytest.mark.parametrize("method", ["tiled", "tiled2"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("window", ["cic", "tsc"])
def test_paint_slab_buffer_with_a_partial_last_tile_row(dev, dirty_alloc, window, dtype, method):
    """test_paint_slab_buffer_with_ghost_planes: planes [15, 33) of a 64-grid, 18 planes - two whole tile rows and one of
    two planes."""
    rng = np.random.default_rng(5)
    n, L = 64, 64.0
    pos = rng.uniform(0, L, size=(70000, 3))
    s = pos[:, 0] * (n / L)
    base = np.floor(s) if window == "cic" else np.floor(s + 0.5)
    mine = np.ascontiguousarray(pos[(base >= 16) & (base < 32)]).astype(dtype)
    x_start, nx_alloc = 15, 18
    pd = dev.as_device(mine)
    call = lambda: dev.paint(pd, None, n, L, window, method=method, x_start=x_start, nx_alloc=nx_alloc, accumulate=False)
    got = dirty_call(dirty_alloc, call)
    ref = omesh.paint(mine, None, n, L, window)[x_start:x_start + nx_alloc]
    tol = 1e-12 if dtype == np.float64 else 2e-6
    close(got, ref, rtol=tol, atol=tol)
    assert_same_bits(got, zero_call(dirty_alloc, call))


def test_paint_clustered_input_on_the_probed_two_pass_path(dev, dirty_alloc):
    """test_clustered_input_goes_to_the_two_pass_path_in_one_attempt at the smallest size the probe looks at (2^21
    particles; below 2^20 there is no probe): probe kernel, exact two-pass lists, grid from torch.empty."""
    n, L = 128, 1000.0
    pos = dev.synth_clustered_particles(n, n, L, seed=11, nattractors=64, dtype=torch.float32)
    st = {}

    def call():
        st.clear()
        return dev.paint(pos, None, n, L, "cic", method="tiled", check_dropped=False, stats=st)
    got = dirty_call(dirty_alloc, call)
    print("probe", st.get("probe"), "path", st["path"], "attempts", st["attempts"])
    assert st["probe"]["overflow"] > pos.shape[0] // 64 and st["probe"]["groupable"] >= 0.25
    assert (st["path"], st["attempts"]) == ("two-pass", 1)
    ref = omesh.paint(pos.cpu().numpy().astype(np.float64), None, n, L, "cic")
    got = got.astype(np.float64)
    assert abs(got.sum() - ref.sum()) < 1e-6 * ref.sum()
    close(got, ref, rtol=0, atol=3e-6 * ref.max())
    assert_same_bits(got.astype(np.float32), zero_call(dirty_alloc, call))


def test_paint_deferred_fold_into_the_double_z_pass(dev, dirty_alloc):
    """paint(defer_fold=True) + power_sums_fused64(halo=): grid, workspace with the halo records and the power scratch
    all dirty; against the oracle's spectrum of the oracle's grid at test_pipeline_cic_pk_fp64_tight's 1e-9."""
    n, L = 128, 1000.0
    pos = np.random.default_rng(19).uniform(0, L, size=(400_000, 3))
    pd = dev.as_device(pos)

    def call():
        grid, halo = dev.paint(pd, None, n, L, "cic", method="tiled", accumulate=False, defer_fold=True)
        return dev.finish_power(*dev.power_sums_fused64(grid, L, halo=halo))
    res = dirty_call(dirty_alloc, call)
    ref = offt.fftpower_1d(omesh.paint(pos, None, n, L, "cic"), L)
    assert np.array_equal(res["modes"], ref["modes"])
    close(res["k"], ref["k"], rtol=1e-12)
    close(res["power"], ref["power"].real, rtol=1e-9)


def _staged_rows(sp):
    """Tile row by tile row in pipeline order: a row is folded once the rows its window reaches have been walked."""
    sp.group()
    rows, walked, folded = list(range(sp.nrows_total)), set(), set()
    for r in rows:
        sp.walk(r, 1)
        walked.add(r)
        for f in rows:
            if f not in folded and set(sp.fold_needs(f)) <= walked:
                sp.fold(f, 1)
                folded.add(f)
    assert folded == set(rows)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("window", ["cic", "tsc"])
def test_staged_paint_row_by_row(dev, dirty_alloc, window, dtype):
    n, L, pos, mass, ref = _paint_case(window, dtype)
    pd, md = dev.as_device(pos), dev.as_device(mass)

    def call():
        out = torch.empty((n, n, n), dtype=pd.dtype, device="cuda")
        sp = dev.StagedPaint(pd, md, n, L, window, out, hint="scattered")       # (the particles have no order in memory)
        _staged_rows(sp)
        sp.check()
        return out
    got = dirty_call(dirty_alloc, call)
    tol = SCATTER_TOL[dtype]
    close(got, ref, rtol=tol, atol=tol * ref.max())
    st = {}
    one_call = zero_call(dirty_alloc, lambda: dev.paint(pd, md, n, L, window, method="tiled", accumulate=False,
                                                        hint="scattered", stats=st))
    assert st["path"] == "scattered"
    if st["overflow"] == 0:                                          # (test_staged_paint_row_by_row_is_bit_identical)
        assert_same_bits(got, one_call)


# ================================================================== assignment and transforms
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_ngp_assign(dev, dirty_alloc, dtype):
    rng = np.random.default_rng(9)
    npar, npart = 32, 120000
    x, y, z = (rng.uniform(0, 1, npart).astype(dtype) for _ in range(3))
    for a in (x, y, z):
        a[a >= 1] = 0
    v = rng.standard_normal(npart).astype(dtype)
    tt = torch.float32 if dtype == np.float32 else torch.float64
    call = lambda: dev.ngp_assign(x, y, z, v, npar, dtype=tt)
    got = dirty_call(dirty_alloc, call)
    # (cells no particle falls into: numpy's zeros there - 3.7 particles per cell leave a few per cent empty)
    npt.assert_array_equal(got.astype(np.float64), omesh.ngp_assign(x, y, z, v, npar))
    assert_same_bits(got, zero_call(dirty_alloc, call))


@pytest.mark.parametrize("n,prec,engine", [(64, "f32", "rocfft"), (64, "f64", "rocfft"), (128, "f64", "tile"),
                                           (256, "f32", "tile")])
def test_r2c(dev, dirty_alloc, n, prec, engine):
    """Relative L2 error against numpy's float64 transform: 1e-6 at float32 (test_r2c_3d_tile_vs_rocfft_and_numpy), 1e-12 at
    float64 (tests/test_gpu_mesh.py)."""
    f = (1.0 + np.random.default_rng(n).standard_normal((n, n, n))).astype(np.float32 if prec == "f32" else np.float64)
    t = dev.as_device(f)
    got = dirty_call(dirty_alloc, lambda: dev.r2c(t, engine=engine)).astype(np.complex128)
    ref = np.fft.rfftn(f.astype(np.float64)) / f.size
    assert np.isfinite(got.view(np.float64)).all()
    err = np.sqrt(np.sum(np.abs(got - ref) ** 2)) / np.sqrt(np.sum(np.abs(ref) ** 2))
    print(f"r2c {n} {prec} {engine}: relative L2 error {err:.3e}")
    assert err < (1e-6 if prec == "f32" else 1e-12)


@pytest.mark.parametrize("cdtype", [np.complex64, np.complex128], ids=["c64", "c128"])
def test_shell_filter_and_c2r(dev, dirty_alloc, cdtype):
    n, nz = 32, 17
    rng = np.random.default_rng(3)
    field = rng.standard_normal((n, n, n))
    spec_h = (np.fft.rfftn(field) / field.size).astype(cdtype)
    spec = dev.as_device(spec_h)
    m = np.fft.fftfreq(n, 1.0 / n)
    m2 = m[:, None, None] ** 2 + m[None, :, None] ** 2 + np.arange(nz)[None, None, :] ** 2
    for lo, hi in ((1, 3), (3, 8), (8, 16)):
        inside = (m2 >= lo * lo) & (m2 < hi * hi)
        call = lambda: dev.shell_filter(spec, n, lo, hi)
        masked = dirty_call(dirty_alloc, call)
        assert np.array_equal(masked, spec_h * inside)                       # (test_shell_filter_on_sub_blocks: bit for bit)
        assert_same_bits(masked, zero_call(dirty_alloc, call))
        ind = dirty_call(dirty_alloc, lambda: dev.shell_filter(None, n, lo, hi, dtype=spec.dtype))
        assert np.array_equal(ind, inside.astype(cdtype))
        real = dirty_call(dirty_alloc, lambda: dev.c2r(dev.as_device(masked), (n, n, n)))
        ref = np.fft.irfftn(masked.astype(np.complex128), s=(n, n, n), axes=(0, 1, 2)) * float(n) ** 3
        tol = 1e-12 if cdtype == np.complex128 else 1e-6
        close(real, ref, rtol=0, atol=tol * np.abs(ref).max())


@pytest.mark.parametrize("window", ["cic", "tsc"])
@pytest.mark.parametrize("interlaced,compensated", [(True, True), (False, True), (True, False)])
def test_catalog_mesh_complex_and_interlace_compensate(dev, dirty_alloc, window, interlaced, compensated):
    """test_catalogue_mesh_interlacing_and_compensation_vs_oracle: two paints (the shifted one too), two transforms, the
    in-place combination."""
    rng = np.random.default_rng(17)
    n, L, npart = 32, 250.0, 90000
    pos = rng.uniform(0, L, size=(npart, 3))
    mass = rng.uniform(0.5, 2.0, size=npart)
    pd, md = dev.as_device(pos), dev.as_device(mass)
    sn = []

    def call():
        c, s = dev.catalog_mesh_complex(pd, md, n, L, window, interlaced, compensated)
        sn.append(s)
        return c
    c = dirty_call(dirty_alloc, call)
    rc, rsn = offt.catalog_mesh_complex(pos, mass, n, L, window, interlaced, compensated)
    assert sn[0] == pytest.approx(rsn, rel=1e-13)
    assert np.isfinite(c.view(np.float64)).all()
    npt.assert_allclose(c, rc, rtol=0, atol=1e-10 * np.abs(rc).max())


# ================================================================== fused power
from tests import test_gpu_power_probes as t_probe                 # noqa: E402


@pytest.fixture(scope="module")
def probe_fields(hip):
    f = t_probe._Fields()
    yield f
    f.grids.clear()
    torch.cuda.empty_cache()


POWER_BOX = 700.0            # (the box at which the float64 rule moves every vector of norm 6 into the low-k channel's last shell)


@pytest.mark.parametrize("rule", t_probe.RULES)
@pytest.mark.parametrize("lowk", [True, False], ids=["lowk", "no_lowk"])
def test_power_sums_fused_f32_256(dev, dirty_alloc, probe_fields, lowk, rule):
    """ast_fft_tile_power_3d on a dirty scratch (shell partials, low-k area): the plane-wave probes, shell by shell."""
    n = 256
    g = probe_fields.grid(n, "f32")
    call = lambda: dev.power_sums_fused(g, POWER_BOX, mean=t_probe.MEAN, lowk=lowk, binning=rule)[1]
    mark = dirty_alloc.mark()
    psum = call()
    assert dirty_alloc.since(mark) == 1                              # the scratch; psum comes from torch.zeros
    t_probe._check("dirty fused f32", probe_fields, n, POWER_BOX, rule, psum, "f32")
    again = call()                                                   # the cached, now used, scratch
    t_probe._check("dirty fused f32 again", probe_fields, n, POWER_BOX, rule, again, "f32")
    # Bit identity on a field whose modes are all of one magnitude (test_forward_pruning_to_the_nyquist_disc_changes_no_bit:
    # "bit for bit in fp32").  Not on the probes: a workgroup adds its modes with LDS atomics in arrival order, which is
    # exact - and so order independent - only while the float32-valued terms of a shell span less than 2^29; a probe's
    # mode beside the transform's round-off in the same shell spans more, and the last bit moves from call to call.
    noise = torch.randn((n, n, n), dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(n + 5))
    flat = lambda: dev.power_sums_fused(noise, POWER_BOX, lowk=lowk, binning=rule)[1]
    dev._power_scratch.clear()
    first = dirty_call(dirty_alloc, flat)
    assert np.isfinite(first).all() and first[-1] > 0.0
    assert_same_bits(first, _host(flat()))
    assert_same_bits(first, zero_call(dirty_alloc, lambda: (dev._power_scratch.clear(), flat())[1]))


@pytest.mark.parametrize("rule", t_probe.RULES)
@pytest.mark.parametrize("n,prec,mean", [(128, "f64", None), (128, "f32", None), (256, "f32", t_probe.MEAN)],
                         ids=["f64_128", "f32_widened_128", "big32_256"])
def test_power_sums_fused64(dev, dirty_alloc, probe_fields, hip, n, prec, mean, rule):
    """The double passes at side 128 (float64 grid; float32 grid widened on load) and the big single-precision passes at
    side 256 (their sixteen lowest shells from double sums over the grid, inside the call)."""
    if mean is not None:
        assert hip.ast_fft32_big_supported(n)
    g = probe_fields.grid(n, prec)
    mark = dirty_alloc.mark()
    psum = dev.power_sums_fused64(g, POWER_BOX, binning=rule, mean=mean)[1]
    assert dirty_alloc.since(mark) == 1
    t_probe._check("dirty fused64", probe_fields, n, POWER_BOX, rule, psum, prec)


@pytest.mark.parametrize("rule", t_probe.RULES)
def test_lowk_modes_and_shell_sums(dev, dirty_alloc, probe_fields, hip, rule):
    """The low-k channel alone at side 256: double-precision sums of the modes |m_i| <= 6 (work area and result dirty),
    in one piece and plane range by plane range, then the lowest shells' psum entries against the probes' closed form at
    the float32 routes' tolerance (the grid's cells are float32)."""
    n = 256
    g = probe_fields.grid(n, "f32")
    whole = dirty_call(dirty_alloc, lambda: dev.lowk_modes(g, n))
    assert whole.dtype == np.complex128 and len(whole) == hip.ast_lowk_mode_count()
    assert np.isfinite(whole.view(np.float64)).all()

    def in_parts():
        acc = None
        for x0, nx in ((0, 100), (100, 27), (127, 129)):
            acc = dev.lowk_modes(g[x0:x0 + nx], n, x0, out=acc)
        return acc
    parts = dirty_call(dirty_alloc, in_parts)
    # two double summations of the same N^3 terms in different orders: each within N^3 2^-53 max|x| of the exact sum in
    # its real and its imaginary part (the a-priori bound of tests/test_gpu_zpass_seam.py, rows added up)
    bound = 2.0 * float(n) ** 3 * 2.0 ** -53 * float(g.abs().max())
    assert np.abs(whole).max() > 1e3
    assert np.abs((parts - whole).view(np.float64)).max() <= bound
    sums = dirty_call(dirty_alloc, lambda: dev.lowk_shell_sums(dev.as_device(whole), n, POWER_BOX, binning=rule))
    ns = int(hip.ast_lowk_shell_count())
    assert sums.shape == (ns,) and np.isfinite(sums).all()
    want = probe_fields.expected(n, POWER_BOX, rule)[:ns]
    rtol, eps = t_probe.TOL["f32"]
    signal = want > 0
    assert signal.any()
    assert np.abs(sums[signal] / want[signal] - 1).max() <= rtol
    if (~signal).any():
        assert np.abs(sums[~signal]).max() <= eps * eps * probe_fields.expected(n, POWER_BOX, rule).sum()


@functools.lru_cache(maxsize=None)
def _pipeline_case(window):
    """2^20 particles in random order on a 256^3 grid (128 per tile: the probed single-pass / scattered paint) and their
    oracle grid."""
    n, L = 256, 1000.0
    pos = np.random.default_rng(23).uniform(0, L, size=(1 << 20, 3)).astype(np.float32)
    grid = omesh.paint(pos.astype(np.float64), None, n, L, window)
    return n, L, pos, {rule: offt.fftpower_1d(grid, L, binning=rule) for rule in (None, "integer")}


@pytest.mark.parametrize("rule", [None, "integer"], ids=["default_binning", "integer_binning"])
@pytest.mark.parametrize("window", ["cic", "tsc"])
def test_paint_power_1d_f32_256(dev, dirty_alloc, window, rule):
    """The flagship pipeline: probe, paint with the deferred fold (grid, lists, halo records dirty), fused transform with
    the low-k channel (scratch dirty).  fp32 against the float64 oracle: 1e-6 on every shell, as in
    test_config_a_128_cic_power_vs_oracle / test_fused_fft_power_matches_unfused_and_oracle."""
    n, L, pos, refs = _pipeline_case(window)
    ref = refs[rule]
    pd = dev.as_device(pos)
    call = lambda: dev.paint_power_1d(pd, None, n, L, window, binning=rule)
    res = dirty_call(dirty_alloc, call)
    assert np.array_equal(res["modes"], ref["modes"])
    close(res["k"], ref["k"], rtol=1e-12)
    close(res["power"], ref["power"].real, rtol=1e-6)


# ================================================================== lensing
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_kappa_stack(dev, lens, dirty_alloc, dtype, weighted):
    rng = np.random.default_rng(2)
    P = 5
    planes = [(rng.standard_normal((32, 32)) * 10.0 ** rng.integers(-2, 2)).astype(dtype) for _ in range(P)]
    x_near = np.arange(P) * 150.0
    x_far, x_src, x_shift = x_near + 150.0, 1100.0, 500.0              # planes beyond 500 get the x_far clamp
    w = lens.translate_redshift_weights(x_near, x_far, x_src, x_shift) if weighted else (None, None)
    pd = [dev.as_device(p) for p in planes]
    call = lambda: lens.kappa_stack(pd, *w)
    got = dirty_call(dirty_alloc, call)
    assert got.dtype == dtype
    if dtype == np.float64:
        ref = ok.kappa_stack(planes, x_near, x_far, x_src, x_shift) if weighted else ok.kappa_stack(planes)
        assert np.array_equal(got, ref)                                # (test_stack_*_bit_exact)
    elif not weighted:
        ref = planes[0].copy()
        for p in planes[1:]:
            ref = ref + p
        assert np.array_equal(got, ref)                                # (test_stack_fp32_and_single_plane)
    else:
        # float32 planes with float64 weights: P terms rounded to float32 and added in float32, each step within half
        # an ulp of the running magnitude: |error| <= 2 P 2^-24 sum_p |plane_p w_p|
        wide = [p.astype(np.float64) for p in planes]
        ref = ok.kappa_stack(wide, x_near, x_far, x_src, x_shift)
        mag = sum(np.abs(p * a / b) for p, a, b in zip(wide, *w))
        assert np.isfinite(got).all() and np.all(np.abs(got - ref) <= 2 * P * 2.0 ** -24 * mag)
    assert_same_bits(got, zero_call(dirty_alloc, call))


@pytest.mark.parametrize("nc", [128, 100], ids=["hand_written_128", "embedded_100"])
def test_lens_plan_alphas_and_phi(dev, lens, dirty_alloc, nc):
    rng = np.random.default_rng(nc)
    kappa = rng.standard_normal((nc, nc)) * 0.01
    bsz = np.deg2rad(3.0)
    kd = dev.as_device(kappa)
    plan = lens.LensPlan(nc, bsz)
    a1, a2 = dirty_call(dirty_alloc, lambda: plan.alphas(kd))
    phi = dirty_call(dirty_alloc, lambda: plan.phi(kd))
    r1, r2 = ok.kappa0_to_alphas(kappa, nc, bsz)
    rp = ok.kappa0_to_phi(kappa, nc, bsz)
    close(a1, r1, rtol=0, atol=1e-10 * abs(r1).max())                   # (test_lens_plan_device_variants_vs_oracle)
    close(a2, r2, rtol=0, atol=1e-10 * abs(r2).max())
    close(phi, rp, rtol=0, atol=1e-10 * abs(rp).max())


def test_resize_antialiased(lens, dirty_alloc):
    nin, npix = 96, 24
    rng = np.random.default_rng(nin * 1000 + npix)
    img = rng.standard_normal((nin, nin)) * 0.02 + np.linspace(0.0, 1.0, nin)[None, :]
    call = lambda: lens.resize_antialiased(img, npix)
    got = dirty_call(dirty_alloc, call)
    want = ok.resize_antialiased(img, npix)
    assert got.shape == (npix, npix)
    close(got, want, rtol=0, atol=1e-13 * np.abs(want).max())          # (test_resize_antialiased_against_scipy_restatement)
    assert_same_bits(got, zero_call(dirty_alloc, call))


@pytest.mark.parametrize("npix", [2, 37])
def test_deflection_to_shear(lens, dirty_alloc, npix):
    rng = np.random.default_rng(npix)
    a1, a2 = rng.standard_normal((npix, npix)) * 1e-3, rng.standard_normal((npix, npix)) * 1e-3
    h = np.deg2rad(10.0) / npix
    call = lambda: lens.deflection_to_shear(a1, a2, h)
    g1, g2 = dirty_call(dirty_alloc, call)
    w1, w2 = ok.deflection_to_shear(a1, a2, h)
    assert np.array_equal(g1, w1) and np.array_equal(g2, w2)           # (test_deflection_to_shear_bit_exact)
    assert_same_bits((g1, g2), zero_call(dirty_alloc, call))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_minmax_histogram_order_statistics_percentile(dev, lens, dirty_alloc, dtype):
    rng = np.random.default_rng(5)
    img = (rng.standard_normal((300, 300)) * 0.02).astype(dtype)
    wide = img.astype(np.float64)
    t = dev.as_device(img)
    lo, hi = dirty_call(dirty_alloc, lambda: lens.minmax(t))
    assert lo == img.min() and hi == img.max()
    # range=None: min / max and counts in one call (its buffer is torch.zeros; the pinned copy passes through)
    for nbins in (1, 100):
        counts, edges = lens.histogram(t, nbins)
        rc, re = np.histogram(wide, bins=nbins)
        assert np.array_equal(counts, rc)
        npt.assert_allclose(edges, re, rtol=1e-15, atol=0)
    c2, _ = lens.histogram(t, 10, range=(-0.01, 0.03))
    assert np.array_equal(c2, np.histogram(wide, bins=10, range=(-0.01, 0.03))[0])
    n = img.size
    ks = [0, 1, n // 3, n - 1]
    got = dirty_call(dirty_alloc, lambda: lens.order_statistics(t, ks))
    assert list(got) == np.sort(img.ravel())[ks].astype(np.float64).tolist()
    qs = [0, 5, 33.3, 50, 95, 100]
    got = dirty_call(dirty_alloc, lambda: lens.percentile(t, qs))
    assert list(got) == [np.percentile(wide, q) for q in qs]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_peak_find_with_more_peaks_than_the_first_buffer_holds(dev, lens, dirty_alloc, hip, monkeypatch, dtype):
    """test_more_peaks_than_the_first_buffer_holds at its smaller size: both calls write into dirty value / index buffers."""
    npix, npeaks, cap = 129, 4096, 2080
    rng = np.random.default_rng(npix)
    img = np.zeros((npix, npix), dtype=dtype)
    img[1::2, 1::2] = (1.0 + rng.permutation(npeaks)).reshape(npix // 2, npix // 2)
    calls = []
    real = hip.ast_peak_find
    monkeypatch.setattr(hip, "ast_peak_find", lambda *a: (calls.append(int(a[5])), real(*a))[1])
    t = dev.as_device(img)
    vals, idx = dirty_call(dirty_alloc, lambda: lens.peak_find(t))
    assert calls == [cap, npeaks]
    rv, rp = ok.locate_peaks(img, np.array([-np.inf, np.inf]))
    assert idx.dtype == np.int64 and np.array_equal(idx, rp[:, 0] * npix + rp[:, 1])
    assert vals.dtype == dtype and np.array_equal(vals.astype(np.float64), rv)
    del calls[:]
    lo, hi = np.percentile(rv, 30), np.percentile(rv, 70)
    vals, idx = dirty_call(dirty_alloc, lambda: lens.peak_find(t, lo, hi))
    rv, rp = ok.locate_peaks(img, np.array([lo, hi]))
    assert calls == [cap] and 0 < len(idx) < cap
    assert np.array_equal(idx, rp[:, 0] * npix + rp[:, 1]) and np.array_equal(vals.astype(np.float64), rv)


from tests import test_gpu_map_statistics as t_stat               # noqa: E402


def test_flat_power_spectrum_and_bispectrum(lens, dirty_alloc):
    """test_flat_power_and_bispectrum_on_odd_and_even_maps at 32^2: the transform's output, the ring spectrum and the
    field of the bispectrum are dirty."""
    npix = 32
    img = t_stat._sky(npix)
    edges = t_stat._issue_edges(npix)
    l, p = dirty_call(dirty_alloc, lambda: lens.flat_power_spectrum(img, t_stat.THETA, edges))
    rl, rp = ok.flat_power_spectrum(img, t_stat.THETA, edges)
    assert np.array_equal(l, rl)
    close(p, rp, rtol=1e-12, atol=1e-14 * np.abs(rp).max())
    l, b, ntri = dirty_call(dirty_alloc, lambda: lens.flat_bispectrum_equilateral(img, t_stat.THETA, edges))
    rl, rb, rn = ok.flat_bispectrum_equilateral_brute(img, t_stat.THETA, edges)
    assert ntri.dtype == np.int64 and np.array_equal(ntri, rn) and np.array_equal(l, rl)
    close(b, rb, rtol=1e-9, atol=1e-12 * np.abs(rb).max())


from tests import test_gpu_nfw as t_nfw                           # noqa: E402


def test_nfw_paint_add_patch_and_add(dev, lens, dirty_alloc):
    """The halo map of SkyArray.from_halo_dataframe by hand: nfw_paint (out=None: torch.zeros, its contract is +=),
    add_patch onto it (+= as well) and add of a noise map, whose output is the chain's dirty buffer."""
    rng = np.random.default_rng(0)
    nh, npix = 12, 128
    cat = {"r200_deg": rng.uniform(0.02, 0.08, nh), "r200_pix": rng.integers(4, 12, nh).astype(float),
           "m200": 10 ** rng.uniform(13, 14.5, nh), "c_NFW": rng.uniform(2, 8, nh), "Dc": rng.uniform(500, 2000, nh),
           "theta1_pix": rng.integers(-5, npix + 5, nh), "theta2_pix": rng.integers(-5, npix + 5, nh),
           "theta1_tv": rng.normal(0, 300, nh), "theta2_tv": rng.normal(0, 300, nh)}
    small = rng.standard_normal((21, 21))
    noise = rng.standard_normal((npix, npix)) * 1e-9
    ref = ok.analytic_halo_signal_map(cat, 3, [0, 1], True, 2, npix, "dT")
    stages = {}

    def call():
        m = lens.nfw_paint(cat, 3, [0, 1], True, 2, npix, "dT")
        stages["nfw"] = m.cpu().numpy()
        lens.add_patch(m, dev.as_device(small), (3, 120))
        stages["patched"] = m.cpu().numpy()
        return lens.add(m, dev.as_device(noise))
    got = dirty_call(dirty_alloc, call)
    close(stages["nfw"], ref, rtol=0, atol=1e-9 * abs(ref).max())       # (tests/test_gpu_nfw.py)
    patched = ok.add_patch_to_map(stages["nfw"].copy(), small, (3, 120))
    assert np.array_equal(stages["patched"], patched)                    # (test_add_patch_to_map_clipping)
    assert np.array_equal(got, patched + noise)                          # (test_add_galaxy_shape_noise)


# ================================================================== filters
from tests import test_gpu_filters as t_filt                      # noqa: E402


@pytest.fixture(scope="module")
def map64():
    return np.random.default_rng(64).standard_normal((64, 64))


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("direction", [0, 1])
def test_filters_dgd(dirty_alloc, map64, order, direction):
    from astrild_amd.rays.utils import Filters
    fct = Filters.gaussian_third_derivative if order == 3 else Filters.gaussian_first_derivative
    call = lambda: fct(map64, 2.0, 0.13, direction)
    got = dirty_call(dirty_alloc, call)
    ref = ok.dgd_filter(map64, 2.0, 0.13, direction, order)
    close(got, ref, rtol=t_filt.RTOL, atol=t_filt.RTOL * np.abs(ref).max())
    assert_same_bits(got, zero_call(dirty_alloc, call))


@pytest.mark.parametrize("direction", [1, [0, 1], [1, 0]], ids=["both", "axis1", "axis0"])
def test_filters_gaussian_third_derivative_convolution(dirty_alloc, map64, direction):
    from astrild_amd.rays.utils import Filters
    d = direction if isinstance(direction, int) else np.asarray(direction)
    call = lambda: Filters.gaussian_third_derivative_convolution(map64, 1.0, 0.03, d)
    got = dirty_call(dirty_alloc, call)
    ref = ok.dgd3_convolution(map64, 1.0, 0.03, d)
    close(got, ref, rtol=1e-11, atol=1e-11 * np.abs(ref).max())        # (test_dgd3_convolution_matches_scipy)
    assert_same_bits(got, zero_call(dirty_alloc, call))


def test_filters_gaussian_compensated(dirty_alloc, map64):
    from astrild_amd.rays.utils import Filters
    call = lambda: Filters.gaussian_compensated(map64, 1.0, 0.11 / 3, 0.11)
    got = dirty_call(dirty_alloc, call)
    ref = ok.gaussian_compensated(map64, 1.0, 0.11 / 3, 0.11)
    close(got, ref, rtol=t_filt.RTOL, atol=t_filt.RTOL * np.abs(ref).max())
    assert_same_bits(got, zero_call(dirty_alloc, call))


def test_filters_apodization(dirty_alloc, map64):
    from astrild_amd.rays.utils import Filters
    call = lambda: Filters.apodization(map64, 1.0)
    got = dirty_call(dirty_alloc, call)
    ref = ok.apodization(map64)
    close(got, ref, rtol=1e-13, atol=1e-13 * np.abs(ref).max())        # (test_apodization_matches_oracle)
    assert_same_bits(got, zero_call(dirty_alloc, call))


def test_filters_aperture_photometry(dirty_alloc, map64):
    from astrild_amd.rays.utils import Filters
    img = map64 + 3.0
    ref = ok.aperture_photometry(img, 1.0, 0.2)
    got = dirty_call(dirty_alloc, lambda: Filters.aperture_photometry(img.copy(), 1.0, 0.2))
    close(got, ref, rtol=t_filt.RTOL, atol=t_filt.RTOL * np.abs(ref).max())


# ================================================================== slab pieces on one GPU
@pytest.mark.parametrize("window,dtype", [("cic", torch.float32), ("tsc", torch.float64)])
def test_slab_route_scatter(dev, dirty_alloc, window, dtype):
    """test_route_kernels_group_particles_by_destination_slab: every particle in its slab's range exactly once."""
    from astrild_amd import slab
    from tests.slab_doubles import NumpySlabOps
    rng = np.random.default_rng(21)
    n, L, parts, npart = 64, 100.0, 8, 50001
    pos = rng.uniform(-1.5 * L, 2.5 * L, size=(npart, 3))
    pos[:5, 0] = [0.0, L, -L, L * (1 - 2.0 ** -30), 0.5 * L / n]
    pos = pos.astype(np.float32 if dtype == torch.float32 else np.float64)
    mass = rng.uniform(1, 2, size=npart).astype(pos.dtype)
    ops = slab.HipSlabOps(dtype)
    tp, tm = dev.as_device(pos), dev.as_device(mass)
    counts = ops.route_count(tp, n, L, window, parts)
    ref = NumpySlabOps()
    want = ref.route_count(torch.from_numpy(pos.astype(np.float64)), n, L, window, parts)
    dest = ref._dest(torch.from_numpy(pos.astype(np.float64)), n, L, window, parts)
    assert np.array_equal(counts.cpu().numpy(), want.numpy())
    spos, smass = dirty_call(dirty_alloc, lambda: ops.route_scatter(tp, tm, n, L, window, parts, counts))
    bounds = np.concatenate([[0], np.cumsum(want.numpy())])
    for p in range(parts):
        seg = slice(bounds[p], bounds[p + 1])
        got = np.concatenate([spos[seg], smass[seg, None]], axis=1)
        exp = np.concatenate([pos[dest == p], mass[dest == p, None]], axis=1)
        assert np.array_equal(got[np.lexsort(got.T)], exp[np.lexsort(exp.T)])


def test_slab_y_pass_with_fused_pack(dev, dirty_alloc):
    """HipSlabOps.fft2d_planes_packed on dirty spectrum, send and own-piece buffers (pitched rows: the padding columns
    are never written and stay dirty) against fft2d_planes + pack, bit for bit (test_y_pass_with_fused_pack_equals_
    y_pass_then_pack), and against numpy's transform at 2e-6 of the rms (tests/test_gpu_fft_tile.py)."""
    from astrild_amd import slab
    n, nplanes, parts, me = 256, 3, 4, 3
    nz = n // 2 + 1
    ops = slab.HipSlabOps(torch.float32)
    pitch = ops.spectrum_pitch(n, parts)
    assert pitch % 16 == 0 and pitch > nz
    x = np.random.default_rng(n + parts).standard_normal((nplanes, n, n)).astype(np.float32)
    planes = dev.as_device(x)
    assert ops.packed_supported(planes, parts)

    def call():
        spec = ops.empty((nplanes, n, pitch), ops.cdtype)
        packed = ops.empty((parts, nplanes, n // parts, pitch), ops.cdtype)
        mine = ops.empty((nplanes, n // parts, pitch), ops.cdtype)
        ops.fft2d_planes_packed(planes, spec, packed, parts, me, mine)
        return [mine[..., :nz] if s == me else packed[s][..., :nz] for s in range(parts)], packed[me], mine[..., nz:]
    pieces, own_slot, padding = dirty_call(dirty_alloc, call)
    pat = np.uint8(dirty_alloc.pattern)
    assert np.all(own_slot.view(np.uint8) == pat) and np.all(np.ascontiguousarray(padding).view(np.uint8) == pat)
    spec2d = ops.fft2d_planes(planes, ops.empty((nplanes, n, nz), ops.cdtype))
    ref_packed = _host(ops.pack(spec2d, ops.empty((parts, nplanes, n // parts, nz), ops.cdtype), parts))
    ref = np.fft.fft2(x.astype(np.float64))[:, :, :nz].reshape(nplanes, parts, n // parts, nz).transpose(1, 0, 2, 3)
    rms = np.sqrt(np.mean(np.abs(ref) ** 2))
    for s in range(parts):
        assert np.ascontiguousarray(pieces[s]).tobytes() == ref_packed[s].tobytes()
        close(np.ascontiguousarray(pieces[s]).view(np.float32), np.ascontiguousarray(ref[s].astype(np.complex64)).view(np.float32),
              rtol=0, atol=2e-6 * rms)


def test_slab_block_power_scratch(dev, dirty_alloc, probe_fields):
    """test_slab_blocks through HipSlabOps: the last pass over each rank's block fused with its shell binning, on a
    dirty scratch (allocated once, reused by the next blocks) and dirty spectrum buffers."""
    from astrild_amd import slab
    n, P = 256, 4
    nloc, nz = n // P, n // 2 + 1
    ops = slab.HipSlabOps(torch.float32)
    mark = dirty_alloc.mark()
    spec = ops.fft2d_planes(probe_fields.grid(n, "f32"), ops.empty((n, n, nz), ops.cdtype))
    total = torch.zeros(n // 2 - 1, dtype=torch.float64, device="cuda")
    for r in range(P):
        block = spec[:, r * nloc:(r + 1) * nloc, :].contiguous()
        psum = ops.fft1d_axis0_power(block, 1.0 / float(n) ** 3, n, POWER_BOX, r * nloc, ops.empty((n // 2 - 1,), torch.float64), 0)
        total += psum
    assert dirty_alloc.since(mark) == 2 + P                          # the spectrum, the scratch (once), P psum buffers
    t_probe._check("dirty slab blocks", probe_fields, n, POWER_BOX, dev.DEFAULT_BINNING, total, "f32")


def test_slab_disc_power_scratch(dev, dirty_alloc, probe_fields):
    """test_disc_blocks through HipSlabOps: z rows, the k_y pass storing in the disc layout (own part into its own
    buffer), the last pass over every part's block with its shell binning - every buffer and the scratch dirty."""
    from astrild_amd import slab
    n, parts, me = 256, 4, 0
    ops = slab.HipSlabOps(torch.float32)
    lay = ops.disc_layout(n, parts)
    assert lay is not None and lay["parts"] == parts
    pitch = (n // 2 + 1 + 15) // 16 * 16
    grid = probe_fields.grid(n, "f32")
    mark = dirty_alloc.mark()
    spec = ops.empty((n, n, pitch), ops.cdtype)
    packed = ops.empty((n * lay["total"],), ops.cdtype)
    mine = ops.empty((n * lay["S"][me],), ops.cdtype)
    ops.fft2d_planes_disc(grid, spec, packed, lay, me, mine)
    total = torch.zeros(n // 2 - 1, dtype=torch.float64, device="cuda")
    for q in range(parts):
        block = mine if q == me else packed[n * lay["cumS"][q]: n * (lay["cumS"][q] + lay["S"][q])].clone()
        total += ops.axis0_power_disc(block, 1.0 / float(n) ** 3, n, POWER_BOX, lay, q, ops.empty((n // 2 - 1,), torch.float64), 0)
    assert dirty_alloc.since(mark) == 4 + parts
    t_probe._check("dirty disc blocks", probe_fields, n, POWER_BOX, dev.DEFAULT_BINNING, total, "f32")
