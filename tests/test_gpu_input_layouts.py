"""GPU: the result does not depend on how the caller's tensor lies in memory (Input layouts).  Every entry
family of tests/stream_order.py runs on every re-layout of every input (tests/input_layouts.py: ``run_layouts``) - one
element into a buffer, as a strided view, as a transposed view; padded with NaN, under a dirty allocator - and is held to
its own comparison rule; only the (input, variant) pairs of the registry's ``refuses`` may be refused, and only before
any library call; all inputs and paddings stay bit-unchanged.  Then the narrow (element-wise) branches of the kernels
that switch on the pointer's alignment, the routes the wrappers take around the C entries that demand one, and those
entries' own refusals.  A failure here is a wrong value or an exception, never a fault: no misaligned pointer reaches a
wide access (the table in DESIGN.md).
"""
import ctypes as ct

import numpy as np
import pytest

from tests import input_layouts as il
from tests import stream_order as so
from tests import watershed_oracle as ws_orc

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


def offset(t):
    """``t`` one element into a NaN-padded buffer: contiguous, ``data_ptr() % 16 == itemsize``."""
    v = next(v for v in il.device_variants(t) if v.name == "offset")
    assert v.view.is_contiguous() and v.view.data_ptr() % 16 == t.element_size() and torch.equal(v.view, t)
    return v.view


def bits(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().tobytes()


# ------------------------------------------------------------------ controls: the checker's own power, on device tensors
def _ctrl_case(op, **kw):
    def make():
        x = np.arange(1.0, 2049.0 * 3 + 1).reshape(2049, 3)
        w = np.arange(1, 2050, dtype=np.int32)
        return [x, w], [x[::-1].copy(), w[::-1].copy()]
    return so.Case(name="control", covers=(), make=make, call=lambda dev, lens, x, w: op(x, w), **kw)


def _correct(x, w):
    return (x * 3.0).sum(dim=1) * w, x.clone()


def test_control_a_correct_op_passes(dev, lens):
    outcomes = il.run_layouts(_ctrl_case(_correct), dev, lens)
    assert [o for _, o in outcomes] == ["same"] * 7                      # 3 + 2 single inputs; all inputs: offset, strided
    assert "input 0: transposed" in dict(outcomes) and "all inputs: strided" in dict(outcomes)


def test_control_flat_walk_of_a_strided_input(dev, lens):
    def op(x, w):
        flat = torch.as_strided(x, (x.numel(),), (1,), x.storage_offset()).reshape(x.shape)
        return (flat * 3.0).sum(dim=1) * w, flat.clone()
    with pytest.raises(il.LayoutMismatch) as e:
        il.run_layouts(_ctrl_case(op), dev, lens)
    text = str(e.value)
    assert "input 0: strided: the result differs" in text and "input 0: transposed: the result differs" in text
    assert "offset" not in text and "input 1" not in text


def test_control_dropped_storage_offset(dev, lens):
    def op(x, w):
        base = torch.as_strided(x, x.shape, x.stride(), 0)
        return (base * 3.0).sum(dim=1) * w, base.clone()
    with pytest.raises(il.LayoutMismatch) as e:
        il.run_layouts(_ctrl_case(op), dev, lens)
    text = str(e.value)
    assert "input 0: offset: the result differs" in text and "strided" not in text and "transposed" not in text


def test_control_written_input(dev, lens):
    def op(x, w):
        out = _correct(x, w)
        w.add_(1)
        return out
    with pytest.raises(il.LayoutMismatch) as e:
        il.run_layouts(_ctrl_case(op), dev, lens)
    assert "plain: input 1 was written" in str(e.value) and "input 1 (strided) or its padding was written" in str(e.value)


# ------------------------------------------------------------------ one case per entry family
@pytest.mark.parametrize("c", so.CASES, ids=[c.name for c in so.CASES])
def test_entry_family_on_every_layout(dev, lens, c):
    il.run_layouts(c, dev, lens)


# ------------------------------------------------------------------ functions that take host arrays
def _host_calls(dev, lens):
    r = np.random.default_rng(5)
    pos = r.uniform(0.0, so.L_PAIR, (600, 3))
    img = r.standard_normal((65, 65))
    grid = r.standard_normal((8, 9, 10, 3))
    flat = next(c for c in so.CASES if c.name == "flat_power_spectrum_64").compare      # (atomic sums: that case's tolerance)
    return {
        "tpcf_pair_counts": (pos, lambda a: dev.tpcf_pair_counts(a, so.L_PAIR, so._S_EDGES, so._MU_EDGES), "equal"),
        "watershed_basins": (img, lambda a: {k: v for k, v in dev.watershed_basins(a).items() if k != "sum_f"}, "equal"),
        "divergence": (grid, lambda a: dev.divergence(a, 0.5), "equal"),
        "vector_magnitude": (grid, lambda a: dev.vector_magnitude(a), "equal"),
        "flat_power_spectrum": (img[:64, :64].copy(), lambda a: lens.flat_power_spectrum(a, 3.0, so._L_EDGES), flat),
        "resize_antialiased": (img[:64, :64].copy(), lambda a: lens.resize_antialiased(a, 16), "equal"),
        "ngp_assign": (r.uniform(0.0, 1.0, 501), lambda a: dev.ngp_assign(a, a[::-1].copy(), a, a, 8), "equal"),
    }


@pytest.mark.parametrize("name", ["tpcf_pair_counts", "watershed_basins", "divergence", "vector_magnitude",
                                  "flat_power_spectrum", "resize_antialiased", "ngp_assign"])
def test_host_arrays_in_any_layout(dev, lens, name):
    """Fortran order, negative strides and read-only arrays give the plain array's result - bit for bit, or within the
    registry's tolerance where the function sums with atomics - (these functions copy the array to the device, where the
    kernel sees one layout); another byte order does too or is refused with TypeError / ValueError before any library
    call."""
    a, fn, rule = _host_calls(dev, lens)[name]
    same = so.same_bits if rule == "equal" else (lambda got, want: so.close(got, want, *rule))
    host = lambda v: so.tree_map(lambda t: t.detach().cpu().numpy(), v)
    want = host(fn(a))
    seen = []
    for v in il.variants(a, on_device=False):
        before = il.raw_bytes(v.buffer)
        with il.LibraryGuard() as guard:
            try:
                got = host(fn(v.view))
            except (TypeError, ValueError):
                assert v.name in il.MAY_REFUSE_ON_HOST and guard.calls == 0, (v.name, guard.names)
                got = None
        assert il.raw_bytes(v.buffer) == before, f"{v.name}: the array was written"
        assert got is None or same(got, want), v.name
        seen.append((v.name, "refused" if got is None else "same"))
    print(f"\nINPUT_LAYOUTS host {name}: {seen}")
    assert {n for n, _ in seen} == set(il.HOST_VARIANTS) - ({"fortran"} if a.ndim == 1 else set())


# ------------------------------------------------------------------ the narrow branches, at the smallest shapes that reach them
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_kappa_stack_narrow_path(lens, dtype, weighted):
    """kappa.hip: ast_kappa_stack takes element loads and stores (``wide`` false) when a plane or the output is off 16
    bytes; the sum runs plane by plane in either branch, so it is numpy's sequence bit for bit."""
    r = np.random.default_rng(3)
    planes = [(r.standard_normal((64, 64)) * 0.01).astype(dtype) for _ in range(3)]
    wn, wd = (np.array([0.5, 1.25, 2.0]), np.array([2.0, 1.5, 0.75])) if weighted else (None, None)
    want = np.zeros((64, 64), dtype=dtype)
    for p, a in enumerate(planes):
        term = (a.astype(np.float64) * wn[p] / wd[p]).astype(dtype) if weighted else a
        want = term.copy() if p == 0 else want + term
    dplanes = [torch.from_numpy(a).cuda() for a in planes]
    aligned = lens.kappa_stack(dplanes, wn, wd)
    assert bits(aligned) == want.tobytes()
    one_off = [dplanes[0], offset(dplanes[1]), dplanes[2]]
    assert bits(lens.kappa_stack(one_off, wn, wd)) == want.tobytes()
    buf = il.pad(torch.empty(64 * 64 + 1, dtype=dplanes[0].dtype, device="cuda"))
    out = buf[1:].view(64, 64)
    assert out.data_ptr() % 16 == out.element_size()
    assert lens.kappa_stack(dplanes, wn, wd, out=out) is out
    assert bits(out) == want.tobytes() and bool(torch.isnan(buf[0]))           # (the element in front: untouched)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_watershed_from_an_offset_map(dev, dtype):
    """watershed.hip: ws_sums_kernel loads its runs of 16 pixels element by element when the map is off 16 bytes (the
    labels are the wrapper's own allocation, so the map alone decides ``wide``)."""
    from tests import test_gpu_watershed as own
    f = ws_orc.smoothed_noise(65, dtype=dtype)
    want = ws_orc.basins(f)
    t = offset(torch.from_numpy(f).cuda())
    got = dev.watershed_basins(t)
    own.compare({k: v.cpu().numpy() for k, v in got.items()}, f, want)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("periodic", [False, True], ids=["edges", "periodic"])
def test_divergence_from_an_offset_grid(dev, dtype, periodic, monkeypatch):
    """grid_ops.hip: gd_launch_tiled declines an input off 16 bytes and the cell kernel takes it; both are np.gradient's
    arithmetic in its order, so the two runs are bit-equal."""
    monkeypatch.setenv("ASTRILD_DIVERGENCE_TILED", "1")
    g = torch.Generator(device="cuda").manual_seed(4)
    v = torch.randn((16, 17, 66, 3), generator=g, device="cuda", dtype=dtype)       # (66 cells in z: two tiles, one ragged)
    assert v.data_ptr() % 16 == 0
    aligned = dev.divergence(v, 0.5, periodic=periodic)
    assert bits(dev.divergence(offset(v), 0.5, periodic=periodic)) == bits(aligned)
    monkeypatch.setenv("ASTRILD_DIVERGENCE_TILED", "0")
    assert bits(dev.divergence(v, 0.5, periodic=periodic)) == bits(aligned)


@pytest.mark.parametrize("n,dtype,engine", [(128, torch.float64, "auto"), (256, torch.float32, "auto"),
                                            (256, torch.float32, "tile"), (64, torch.float32, "rocfft")],
                         ids=["fft64_128", "tile_256", "tile_256_asked", "rocfft_64"])
def test_r2c_from_an_offset_cube(dev, n, dtype, engine):
    """ast_fft64_r2c_3d demands 16 bytes and ast_fft_tile_r2c_3d 8: ``r2c`` transforms an aligned copy (device.dense), so
    the spectrum is the aligned run's bit for bit."""
    field = torch.from_numpy(so._cube(n, np.float64 if dtype == torch.float64 else np.float32, 1)).cuda()
    want = bits(dev.r2c(field, engine=engine))
    t = offset(field)
    before = il.raw_bytes(t)
    assert bits(dev.r2c(t, engine=engine)) == want
    assert il.raw_bytes(t) == before


def test_smooth_plan_in_place_on_an_offset_map(dev, lens):
    """SmoothPlan.gaussian writes its argument: a map off 16 bytes is smoothed in an aligned copy and copied back."""
    img = torch.from_numpy(so._kappa(64)(1)[0]).cuda()
    for sigma, kind in ((1.0, "gaussianFFT"), (3.0, "gaussianFFT"), (1.2, "gaussian")):
        want = bits(lens.SmoothPlan(64).gaussian(img.clone(), sigma, kind))
        t = offset(img)
        assert lens.SmoothPlan(64).gaussian(t, sigma, kind) is t
        assert bits(t) == want, (sigma, kind)


def test_dense_leaves_aligned_contiguous_tensors_alone(dev):
    """The aligned, contiguous path does no new work: ``dense`` returns the very tensor, and allocates nothing."""
    t = torch.zeros((64, 64, 64), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    assert dev.dense(t) is t and dev.dense(t, 16) is t and dev.dense(None, 16) is None
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    o = offset(t)
    d = dev.dense(o, 16)
    assert d is not o and d.data_ptr() % 16 == 0 and torch.equal(d, o) and dev.dense(o) is o
    s = t[..., :63]
    assert dev.dense(s).is_contiguous() and torch.equal(dev.dense(s), s)


# ------------------------------------------------------------------ the C entries' own refusals
def test_c_entries_refuse_misaligned_pointers_before_any_launch(dev, hip):
    """The guards of DESIGN.md's table: an entry whose kernel reads or writes wider than the element refuses a pointer
    off that width with an error code, and touches nothing."""
    n = 256
    grid = torch.zeros(n * n * n + 4, dtype=torch.float32, device="cuda")
    spec = torch.full((n * n * (n // 2 + 1) + 1,), 7.0, dtype=torch.complex64, device="cuda")
    at = lambda t, nbytes: ct.c_void_p(t.data_ptr() + nbytes)
    s = dev.stream()
    assert grid.data_ptr() % 16 == 0 and spec.data_ptr() % 16 == 0
    # the z rows are read as float2
    assert hip.ast_fft_tile_rows_r2c(at(grid, 4), dev.ptr(spec), 0, n, n * n, n, n // 2 + 1, 1.0, s) != 0
    assert b"& 7" in hip.ast_last_error()
    assert hip.ast_fft_tile_r2c_3d(at(grid, 4), dev.ptr(spec), 0, n, 1.0, s) != 0
    scratch = torch.empty(int(hip.ast_fft_tile_power_scratch_bytes(n)), dtype=torch.uint8, device="cuda")
    psum = torch.zeros(n // 2 - 1, dtype=torch.float64, device="cuda")
    for lowk in (0, 1):
        assert hip.ast_fft_tile_power_3d(at(grid, 4), dev.ptr(scratch), scratch.numel(), 0, n, 1000.0, 0.0, lowk, 1,
                                         dev.ptr(psum), s) != 0
    # the real rows of the inverse transform are stored 16 bytes at a time
    work = torch.empty_like(spec[1:])
    assert hip.ast_fft_tile_c2r_3d(dev.ptr(spec), dev.ptr(work), at(grid, 8), 0, n, 0, 0, 1.0, s) != 0
    # the tiled paint's fold walks the grid's lines 16 bytes at a time
    pos = torch.rand((1000, 3), dtype=torch.float32, device="cuda") * 100.0
    flags = dev.paint_flags("single-pass", False)
    ws_bytes = int(hip.ast_paint_tiled_workspace_bytes(1, 0, 1000, n, n, flags))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    dropped = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert hip.ast_paint_tiled(1, 0, dev.ptr(pos), None, 1000, n, 100.0, 1.0, 0, n, at(grid, 8), dev.ptr(ws), ws_bytes,
                               dev.ptr(dropped), flags, 1.0, 0.0, 0, -1, 0.0, s) != 0
    torch.cuda.synchronize()
    assert not bool(grid.any()) and bool((spec == 7.0).all()) and not bool(psum.any()) and int(dropped) == 0
