"""GPU: the mesh readout (astrild_amd/particles/hutils/readout.py, astrild_amd/csrc/mesh_readout.hip) against the numpy
restatement of its contract (tests/readout_oracle.py).  The contract fixes every operation and its order, so the
comparison is ``tobytes()``; the tolerances below are for properties (known fields, the adjoint of the paint) and are
worked out from the number formats.  Every oracle result is computed once and shared."""
import functools
import importlib

import numpy as np
import pytest

from tests import dirty_memory as dm
from tests import input_layouts as il
from tests import readout_oracle as orc
from tests import stream_order as so

torch = pytest.importorskip("torch")
# (the package exports the function ``readout`` under the module's own name: the module itself comes from importlib)
readout_module = importlib.import_module("astrild_amd.particles.hutils.readout")

pytestmark = pytest.mark.gpu

L = 100.0
WINDOWS = ("ngp", "cic", "tsc")
DTYPES = {"f32": np.float32, "f64": np.float64}
SHAPES = {"scalar": 0, "vec3": 3, "vec4": 4}                      # (n, n, n), (n, n, n, 3), (n, n, n, 4)


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def dev(hip):
    from astrild_amd import device
    return device


@pytest.fixture(scope="module")
def ro(hip):
    return readout_module


def same_bits(got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


@functools.lru_cache(maxsize=None)
def case(n, window, fdt, pdt, ncomp, count=1000, boxsize=L):
    """(field, pos, oracle result, A) - host arrays, made once."""
    field = orc.field(n, ncomp, DTYPES[fdt], seed=100 * n + ncomp)
    pos = orc.positions(n, boxsize, count, seed=n + 17, dtype=DTYPES[pdt])
    want, A = orc.readout(field, pos, boxsize, window)
    for a in (field, pos, want, A):
        a.setflags(write=False)
    return field, pos, want, A


# ------------------------------------------------------------------ 1. bit equality
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pdt", DTYPES)
@pytest.mark.parametrize("fdt", DTYPES)
@pytest.mark.parametrize("window", WINDOWS)
def test_bit_equal_to_the_oracle(dev, ro, window, fdt, pdt, shape):
    for n in (1, 2, 5, 8):
        field, pos, want, _ = case(n, window, fdt, pdt, SHAPES[shape])
        got = ro.readout(dev.as_device(field), dev.as_device(pos), L, window)
        assert isinstance(got, torch.Tensor) and got.is_cuda
        assert same_bits(got, want), (n, "device tensors")
        got = ro.readout(field, pos, L, window.upper())
        assert isinstance(got, np.ndarray)
        assert same_bits(got, want), (n, "numpy arrays")


@pytest.mark.parametrize("fdt", DTYPES)
@pytest.mark.parametrize("window", WINDOWS)
def test_bit_equal_with_a_half_cell_shift(dev, ro, window, fdt):
    """L and n powers of two, positions multiples of L / (8 n): x n / L and the sum with 0.5 are exact, so the kernel's
    fused multiply-add and numpy's two operations give the same s."""
    box, n = 64.0, 8
    rng = np.random.default_rng(5)
    step = box / (8 * n)
    field = orc.field(n, 3, DTYPES[fdt], seed=9)
    for pdt in DTYPES.values():
        pos = (rng.integers(-20 * n, 28 * n, size=(1000, 3)) * step).astype(pdt)
        want, _ = orc.readout(field, pos, box, window, shift=0.5)
        assert not same_bits(orc.readout(field, pos, box, window)[0], want)             # the shift is not a no-op
        assert same_bits(ro.readout(dev.as_device(field), dev.as_device(pos), box, window, shift=0.5), want)


# ------------------------------------------------------------------ 2. non-finite coordinates
@pytest.mark.parametrize("shape", ["scalar", "vec3"])
@pytest.mark.parametrize("fdt", DTYPES)
@pytest.mark.parametrize("window", WINDOWS)
def test_non_finite_coordinates(dev, ro, window, fdt, shape):
    n, ncomp, guard = 8, SHAPES[shape], 64
    field = orc.field(n, ncomp, DTYPES[fdt], seed=2)
    pos = np.random.default_rng(3).uniform(-L, 2 * L, size=(64, 3))
    pos[5, 0], pos[17, 1], pos[40, 2] = np.nan, np.inf, -np.inf
    pos[50] = 1e300                                               # finite, far out: a value, not NaN
    want, _ = orc.readout(field, pos, L, window)
    assert np.isnan(want[[5, 17, 40]]).all() and np.isfinite(np.delete(want, [5, 17, 40], axis=0)).all()
    shape_out = want.shape
    buf = il.pad(torch.empty(want.size + 2 * guard, dtype=getattr(torch, field.dtype.name), device="cuda"))
    before = il.raw_bytes(buf)
    out = buf[guard:guard + want.size].view(shape_out)
    got = ro.readout(dev.as_device(field), dev.as_device(pos), L, window, out=out)
    assert got is out
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert np.isnan(got[[5, 17, 40]]).all()
    finite = np.delete(np.arange(64), [5, 17, 40, 50])
    assert got[finite].tobytes() == want[finite].tobytes()
    assert np.isfinite(got[50]).all()
    after = il.raw_bytes(buf)
    item = buf.element_size()
    assert after[:guard * item] == before[:guard * item] and after[-guard * item:] == before[-guard * item:]


# ------------------------------------------------------------------ 3. known fields
@pytest.mark.parametrize("fdt", DTYPES)
@pytest.mark.parametrize("window", WINDOWS)
def test_constant_field(dev, ro, window, fdt):
    """NGP: the constant itself.  CIC, TSC: within 4 eps_R |c| (the weights of an axis sum to 1 within 2 ulp)."""
    n, R = 8, DTYPES[fdt]
    c = R(1.7)
    field = np.full((n, n, n), c, dtype=R)
    pos = orc.positions(n, L, 1000, seed=23)
    got = ro.readout(field, pos, L, window)
    err = np.abs(got.astype(np.float64) - float(c)).max()
    print(f"READOUT constant {window} {fdt}: max error {err / (np.finfo(R).eps * float(c)):.2f} eps |c|")
    if window == "ngp":
        assert np.all(got == c)
    else:
        assert err <= 4 * np.finfo(R).eps * abs(float(c))


@pytest.mark.parametrize("fdt", DTYPES)
@pytest.mark.parametrize("window", ["cic", "tsc"])
def test_linear_field(dev, ro, window, fdt):
    """f = x of the grid point: CIC and TSC reproduce a linear function, so away from the wrap (2 cells) the value is the
    particle's own x, within 16 eps_R A."""
    n, R = 16, DTYPES[fdt]
    dx = L / n
    field = np.broadcast_to((np.arange(n) * dx).astype(R)[:, None, None], (n, n, n)).copy()
    rng = np.random.default_rng(31)
    pos = rng.uniform(0.0, L, size=(1000, 3))
    pos[:, 0] = rng.uniform(2 * dx, L - 2 * dx, size=1000)
    _, A = orc.readout(field, pos, L, window)
    got = ro.readout(field, pos, L, window).astype(np.float64)
    ratio = np.abs(got - pos[:, 0]) / (np.finfo(R).eps * A)
    print(f"READOUT linear {window} {fdt}: max |value - x| / (eps A) = {ratio.max():.2f}")
    assert np.all(np.abs(got - pos[:, 0]) <= 16 * np.finfo(R).eps * A)


# ------------------------------------------------------------------ 4. adjoint of the device paint
@pytest.mark.parametrize("fdt", DTYPES)
@pytest.mark.parametrize("window", WINDOWS)
def test_adjoint_of_the_device_paint(dev, ro, window, fdt):
    """sum paint(m, pos) f = sum m readout(f, pos) within (k_max + 16) eps_R sum_p |m_p| A_p (tests/test_readout_oracle.py,
    (b)), both sides summed in float64 on the host."""
    n, R = 8, DTYPES[fdt]
    rng = np.random.default_rng(41)
    pos = rng.uniform(0.0, L, size=(64, 3)).astype(R)
    mass = rng.uniform(0.5, 2.0, size=64).astype(R)
    field = orc.field(n, 0, R, seed=43)
    grid = dev.paint(dev.as_device(pos), dev.as_device(mass), n, L, window, method="direct")
    val = ro.readout(field, pos, L, window)
    _, A = orc.readout(field, pos, L, window)
    idx, _, _ = orc.stencil(pos, n, L, window, 0.0, R)
    W = idx[0].shape[0]
    flat = np.concatenate([((idx[0][a] * n + idx[1][b]) * n + idx[2][c]) for a in range(W) for b in range(W) for c in range(W)])
    k_max = int(np.bincount(flat, minlength=n ** 3).max())
    lhs = float(np.sum(grid.cpu().numpy().astype(np.float64) * field.astype(np.float64)))
    rhs = float(np.sum(mass.astype(np.float64) * val.astype(np.float64)))
    bound = (k_max + 16) * np.finfo(R).eps * float(np.sum(np.abs(mass.astype(np.float64)) * A))
    print(f"READOUT adjoint {window} {fdt}: k_max={k_max} |lhs - rhs| / bound = {abs(lhs - rhs) / bound:.3f}")
    assert abs(lhs - rhs) <= bound


# ------------------------------------------------------------------ 5. element indices past 2^31 and 2^32
def test_large_index(dev, ro):
    """(1030, 1030, 1030, 4) float32: 17.5 GB, element indices up to 4.37e9.  Particles around the cells (0, 0, 0) -
    indices below 2^31, and, wrapped, above 2^32 -, (515, 515, 515) - between 2^31 and 2^32 - and (1029, 1029, 1029) -
    above 2^32, wrapping to 0; their stencil cells hold small integers, everything else is zero."""
    n, C, box = 1030, 4, 1030.0
    free, _ = torch.cuda.mem_get_info()
    if free < 20e9:
        pytest.skip(f"{free / 1e9:.1f} GB of device memory free, the 17.5 GB field needs 20")
    rng = np.random.default_rng(51)
    pos = np.concatenate([c + rng.uniform(-1.4, 1.4, size=(67, 3)) for c in (0.0, 515.0, 1029.0)])
    cells = {}
    for window in ("cic", "tsc"):
        idx, _, finite = orc.stencil(pos, n, box, window, 0.0, np.float32)
        assert finite.all()
        W = idx[0].shape[0]
        for a in range(W):
            for b in range(W):
                for c in range(W):
                    for key in zip(idx[0][a].tolist(), idx[1][b].tolist(), idx[2][c].tolist()):
                        cells[key] = np.array([(7 * key[0] + 3 * key[1] + key[2] + 5 * comp) % 13 - 6 for comp in range(C)],
                                              dtype=np.float32)
    keys = np.array(sorted(cells), dtype=np.int64)
    flat = ((keys[:, 0] * n + keys[:, 1]) * n + keys[:, 2]) * C
    assert (flat < 2 ** 31).any() and ((flat > 2 ** 31) & (flat < 2 ** 32)).any() and (flat > 2 ** 32).any()
    field = torch.zeros((n, n, n, C), dtype=torch.float32, device="cuda")
    try:
        kd = torch.from_numpy(keys).cuda()
        values = torch.from_numpy(np.stack([cells[tuple(k)] for k in keys.tolist()])).cuda()
        field[kd[:, 0], kd[:, 1], kd[:, 2]] = values
        assert torch.equal(field[kd[:, 0], kd[:, 1], kd[:, 2]], values) and int(torch.count_nonzero(field[0, 0, :4])) > 0
        pd = dev.as_device(pos)
        for window in ("tsc", "cic"):
            want, _, touched = orc.readout_sparse(cells, n, C, np.float32, pos, box, window)
            assert touched <= set(cells) and np.abs(want).max() > 0
            assert same_bits(ro.readout(field, pd, box, window), want), window
    finally:
        del field
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 6. launch geometry
@pytest.mark.parametrize("window, fdt, shape", [("tsc", "f32", "vec3"), ("cic", "f64", "scalar"), ("ngp", "f32", "vec4")])
def test_launch_geometry(dev, ro, window, fdt, shape):
    """One thread, one short of a block, a block, one more, and three more than the capped grid covers in one sweep."""
    n, most = 8, 2048 * 256 + 3
    field, pos, want, _ = case(n, window, fdt, "f32", SHAPES[shape], count=most)
    fd, pd = dev.as_device(field), dev.as_device(pos)
    for count in (1, 255, 256, 257, most):
        got = ro.readout(fd, pd[:count], L, window)
        again = ro.readout(fd, pd[:count], L, window)
        assert same_bits(got, want[:count]), count
        assert same_bits(again, want[:count]), count


def test_no_particles_no_library_call(dev, ro):
    field = dev.as_device(orc.field(4, 3, np.float32, seed=1))
    with il.LibraryGuard() as guard:
        got = ro.readout(field, torch.empty((0, 3), dtype=torch.float64, device="cuda"), L)
        got1 = ro.readout(field[..., 0], np.empty((0, 3), dtype=np.float32), L, "tsc")
        host = ro.readout(np.zeros((4, 4, 4)), np.empty((0, 3)), L)
    assert guard.calls == 0
    assert tuple(got.shape) == (0, 3) and got.dtype == torch.float32 and got.is_cuda
    assert tuple(got1.shape) == (0,) and got1.dtype == torch.float32
    assert isinstance(host, np.ndarray) and host.shape == (0,) and host.dtype == np.float64


# ------------------------------------------------------------------ 7. streams, layouts, dirty memory
def _stream_case(ro):
    def make():
        real = [orc.field(8, 3, np.float32, seed=61), orc.positions(8, L, 4000, seed=62)]
        decoy = [orc.field(8, 3, np.float32, seed=63), orc.positions(8, L, 4000, seed=64)]
        return real, decoy
    # built directly: stream_order.case() would append to the registry the other test modules walk
    return so.Case(name="readout_tsc_vec3", covers=(), make=make, compare="equal",
                   call=lambda dev, lens, f, p: ro.readout(f, p, L, "tsc"))


def test_streams_layouts_dirty_memory(dev, ro):
    from astrild_amd import lensing
    c = _stream_case(ro)
    ins, dec = c.make()
    want, _ = orc.readout(ins[0], ins[1], L, "tsc")
    be = so.cuda_backend()
    fn = lambda *a: c.call(dev, lensing, *a)
    with dm.dirty(dm.HUGE_BYTES):
        ref = fn(*[be.upload(a) for a in ins])                    # the default stream
        assert same_bits(ref, want)
        assert not same_bits(fn(*[be.upload(a) for a in dec]), want), "the decoy gives the real answer"
        with torch.cuda.stream(be.stream(0)):                     # under S, nothing late
            plain = fn(*[be.upload(a) for a in ins])
        torch.cuda.synchronize()
        assert same_bits(plain, want)
        so.late_call(fn, ins, dec)                                # (first launches of the probe's own kernels under S)
        got, armed = so.late_call(fn, ins, dec)
    torch.cuda.synchronize()
    assert armed, "readout waited for the device: it must only queue work on the caller's stream"
    assert same_bits(got, want), "behind the late producer"
    outcomes = il.run_layouts(c, dev, lensing)                    # field, pos, and both together; bit equal to plain
    assert {o for _, o in outcomes} == {"same"}, outcomes
    assert {label.split(":")[0] for label, _ in outcomes} == {"input 0", "input 1", "all inputs"}
    with dm.dirty(dm.NAN_BYTES):
        assert same_bits(fn(*[be.upload(a) for a in ins]), want)


# ------------------------------------------------------------------ 8. density_at
@pytest.mark.parametrize("window, fdt, masses", [("ngp", "f32", False), ("cic", "f32", True), ("tsc", "f64", True),
                                                 ("cic", "f64", False)])
def test_density_at(dev, ro, window, fdt, masses):
    """Tracers on multiples of dx / 8 with small integer masses: every deposit is a dyadic number and every cell's sum is
    exact in the grid's dtype, so the paint's atomic additions give the same grid in any order and two paints can be
    compared for equality."""
    n, box, R = 16, 64.0, DTYPES[fdt]
    rng = np.random.default_rng(71)
    tracers = (rng.integers(0, 8 * n, size=(4096, 3)) * (box / (8 * n))).astype(R)
    mass = rng.integers(1, 4, size=4096).astype(R) if masses else None
    query = rng.uniform(-box, 2 * box, size=(100, 3))
    t, q = dev.as_device(tracers), dev.as_device(query)
    m = None if mass is None else dev.as_device(mass)
    mean = dev.total_mass(m, 4096) / float(n) ** 3
    assert mean == (float(mass.sum()) if masses else 4096.0) / n ** 3
    want = ro.readout(dev.paint(t, m, n, box, window), q, box, window)
    got = ro.density_at(t, q, n, box, window, mass=m)
    assert got.shape == (100,) and got.dtype == t.dtype
    assert torch.equal(got, want / mean - 1.0)
    assert torch.equal(ro.density_at(t, q, n, box, window, mass=m, contrast=False), want)
    host = ro.density_at(tracers, query, n, box, window, mass=mass)
    assert isinstance(host, np.ndarray) and same_bits(got, host)


def test_density_at_uniform_lattice_is_zero(dev, ro):
    n, box = 16, 64.0
    g = (np.arange(n) + 0.25) * (box / n)
    tracers = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    assert len(tracers) == 4096
    query = np.random.default_rng(73).uniform(0.0, box, size=(100, 3))
    delta = ro.density_at(tracers, query, n, box, "ngp")
    assert delta.shape == (100,) and np.all(delta == 0.0)
