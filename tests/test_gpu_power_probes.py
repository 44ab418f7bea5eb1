"""GPU: every route that produces the shell sums psum[s] of the 3D power spectrum, mode by mode.

The field is a sum of plane waves (tests/power_probes.py: Hermitian plane, negative frequencies, the pruning boundary, tile
seams, the low-k patch boundary, on-edge vectors in every axis order) on a mean of 2; its shell sums are known in closed form
(checked against the oracle on the host in test_power_probes_cpu.py).  One mode that a route drops, counts twice, weights
wrongly or bins one shell off moves a shell by at least 5 %; the tolerances are those of tests/test_gpu_mesh.py:

* signal shells: 1e-6 relative on float32 routes, 1e-12 on float64 routes;
* empty shells: psum <= eps^2 sum(expected), eps = 1e-6 (the relative L2 bound test_r2c_3d_tile_vs_rocfft_and_numpy asserts
  of the fp32 transform) or 1e-12.

Every route runs under both shell rules and the box sizes 1000, 100, 1000, 700 in this order: the fused routes' table of edge
falls is cached per (side, box) - built, replaced, reused; at L = 100 and L = 1000 the float64 rule moves probes whose three
components differ (the expression it restates is not symmetric in the axes), at L = 700 it moves every vector of norm 6 from
shell 5 into shell 4, the last one of the fp32 route's double-precision low-k channel.

Side 2048 is left to test_gpu_fullsize.py (its grid alone is 32 ... 64 GB).
"""
import os

import numpy as np
import pytest

from oracle import fftpower as offt
from tests import power_probes as pp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MEAN = 2.0
BOXES = (1000.0, 100.0, 1000.0, 700.0)
RULES = ("integer", "float64")
TOL = {"f32": (1e-6, 1e-6), "f64": (1e-12, 1e-12)}          # (rtol of the signal shells, eps of the empty ones)


class _Fields:
    """Probe sets, their grids on the device (one per (side, dtype)) and their expected shell sums, built once."""

    def __init__(self):
        self.sets, self.grids, self.want = {}, {}, {}

    def probes(self, n):
        if n not in self.sets:
            self.sets[n] = pp.probe_set(n)
        return self.sets[n]

    def grid(self, n, prec):
        if (n, prec) not in self.grids:
            dtype = torch.float32 if prec == "f32" else torch.float64
            self.grids[n, prec] = pp.probe_field(n, self.probes(n), MEAN, dtype, "cuda")
        return self.grids[n, prec]

    def expected(self, n, boxsize, rule):
        key = (n, boxsize, rule)
        if key not in self.want:
            self.want[key] = pp.expected_psum(n, boxsize, self.probes(n), rule)
        return self.want[key]


@pytest.fixture(scope="module")
def fields(hip):
    torch.cuda.set_device(0)
    f = _Fields()
    yield f
    f.grids.clear()                      # the 1024^3 grids: 12 GB
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def dev(hip):
    from astrild_amd import device
    torch.cuda.set_device(0)
    return device


def _check(label, fields, n, boxsize, rule, psum, prec):
    want = fields.expected(n, boxsize, rule)
    got = psum.cpu().numpy()
    rtol, eps = TOL[prec]
    signal = want > 0
    rel = np.abs(got[signal] / want[signal] - 1).max()
    leak = np.abs(got[~signal]).max() / want.sum() if (~signal).any() else 0.0
    print(f"PROBE {label} n={n} L={boxsize:g} {rule}: signal shells {rel:.2e} (at shell {np.nonzero(signal)[0][np.argmax(np.abs(got[signal] / want[signal] - 1))]}), "
          f"empty shells / total {leak:.2e}")
    assert rel <= rtol, (label, n, boxsize, rule)
    assert leak <= eps * eps, (label, n, boxsize, rule)


def _run(label, fields, n, prec, shell_sums):
    """shell_sums(boxsize, rule) -> psum tensor, under every (box, rule) in order."""
    probes = fields.probes(n)
    # the run at L = 100 says something about the float64 rule only if that rule moves probes there
    assert not np.array_equal(fields.expected(n, 100.0, "float64"), fields.expected(n, 100.0, "integer"))
    assert len(probes) >= 48
    # at least 24 shells carry a probe (side 32 has 15 shells: all of them); the float64 rule may empty one by moving its probes
    assert (fields.expected(n, BOXES[0], "integer") > 0).sum() >= min(24, n // 2 - 1)
    for boxsize in BOXES:
        for rule in RULES:
            _check(label, fields, n, boxsize, rule, shell_sums(boxsize, rule), prec)


class _env:
    """Set environment variables for a block and restore them (the library reads them per call)."""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# ---------------------------------------------------------------- the plain route: transform to HBM, ast_power_bin_1d
@pytest.mark.parametrize("n", [32, 64])
def test_plain_float64(dev, fields, n):
    spec = dev.r2c(fields.grid(n, "f64"))
    _run("plain f64", fields, n, "f64", lambda L, rule: dev.power_bin_1d(spec, None, n, L, binning=rule)[1])


@pytest.mark.parametrize("n,engine", [(64, "rocfft"), (256, "tile")])
def test_plain_complex64(dev, fields, n, engine):
    spec = dev.r2c(fields.grid(n, "f32"), engine=engine)
    assert spec.dtype == torch.complex64
    _run("plain c64 " + engine, fields, n, "f32", lambda L, rule: dev.power_bin_1d(spec, None, n, L, binning=rule)[1])


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_plain_four_sub_blocks(dev, fields, prec):
    """The block form (i0 = / i1 =, the slab ranks' call): four quarters of the half spectrum added into one psum."""
    n = 64
    h = n // 2
    spec = dev.r2c(fields.grid(n, prec), engine="rocfft")

    def sums(L, rule):
        psum = torch.zeros(n // 2 - 1, dtype=torch.float64, device="cuda")
        for a in (0, h):
            for b in (0, h):
                dev.power_bin_1d(spec[a:a + h, b:b + h].contiguous(), None, n, L, i0=(a, h), i1=(b, h), psum=psum, binning=rule)
        return psum
    _run("plain blocks " + prec, fields, n, prec, sums)


# ---------------------------------------------------------------- fused fp32 passes (ast_fft_tile_power_3d)
@pytest.mark.parametrize("lowk", [True, False])
@pytest.mark.parametrize("n", [256, 512, 1024])
def test_fused_float32(dev, fields, n, lowk):
    g = fields.grid(n, "f32")
    _run(f"fused f32 lowk={int(lowk)}", fields, n, "f32",
         lambda L, rule: dev.power_sums_fused(g, L, mean=MEAN, lowk=lowk, binning=rule)[1])


@pytest.mark.parametrize("n,var,value", [(256, "AST_FFT_NO_PRUNE", "1"), (256, "AST_FFT_DISC", "1"), (256, "AST_FFT_DISC", "2"),
                                         (256, "AST_LOWK_SEPARATE", "1"), (512, "AST_FFT_DISC", "1")])
def test_fused_float32_variants(dev, fields, n, var, value):
    """Unpruned passes, the disc layout between the last two passes, the low-k sums as kernels of their own."""
    g = fields.grid(n, "f32")

    def sums(L, rule):
        with _env(**{var: value}):
            return dev.power_sums_fused(g, L, mean=MEAN, binning=rule)[1]
    _run(f"fused f32 {var}={value}", fields, n, "f32", sums)


# ---------------------------------------------------------------- double-precision passes and the big fp32 passes (cube_fft.hip)
@pytest.mark.parametrize("n", [128, 256, 512, 1024])
def test_fused_float64(dev, fields, n):
    g = fields.grid(n, "f64")
    _run("fused f64", fields, n, "f64", lambda L, rule: dev.power_sums_fused64(g, L, binning=rule)[1])


def test_float32_grid_through_the_double_passes(dev, fields):
    n = 128
    g = fields.grid(n, "f32")
    _run("f32 via f64 passes", fields, n, "f32", lambda L, rule: dev.power_sums_fused64(g, L, binning=rule, mean=None)[1])


def test_big_float32_passes(dev, fields, hip):
    n = 256
    assert hip.ast_fft32_big_supported(n)            # (otherwise the call below would take the double passes)
    g = fields.grid(n, "f32")
    _run("big f32", fields, n, "f32", lambda L, rule: dev.power_sums_fused64(g, L, binning=rule, mean=MEAN)[1])


# ---------------------------------------------------------------- slab ranks on one GPU: the last pass over blocks
def test_slab_blocks(dev, fields, hip):
    """All ranks on one GPU (test_gpu_slab.py): z rows and k_y columns of every plane, then each rank's (n, n / P, n/2+1) block
    through ast_fft_tile_block_power with its k_y offset."""
    from astrild_amd import _lib, slab
    n, P = 256, 4
    nloc, nz = n // P, n // 2 + 1
    ops = slab.HipSlabOps(torch.float32)
    spec = ops.fft2d_planes(fields.grid(n, "f32"), ops.empty((n, n, nz), ops.cdtype))
    scratch = torch.empty(int(hip.ast_fft_tile_block_power_scratch_bytes(n, nloc)), dtype=torch.uint8, device="cuda")

    def sums(L, rule):
        total = torch.zeros(n // 2 - 1, dtype=torch.float64, device="cuda")
        for r in range(P):
            block = spec[:, r * nloc:(r + 1) * nloc, :].contiguous()            # (the call leaves the block undefined)
            psum = torch.zeros_like(total)
            _lib.check(hip.ast_fft_tile_block_power(dev.ptr(block), dev.ptr(scratch), scratch.numel(), 0, n, nloc, r * nloc, nz,
                                                    1.0 / float(n) ** 3, L, 0, _lib.BIN[rule], dev.ptr(psum), dev.stream()))
            total += psum
        return total
    _run("slab blocks", fields, n, "f32", sums)


def test_disc_blocks(dev, fields, hip):
    """The same with the disc layout as the wire format (test_last_pass_over_disc_blocks_adds_up_to_the_single_gpu_sums)."""
    from astrild_amd import _lib, slab
    n, parts = 256, 4
    lay = slab.disc_layout(n, parts, 16, 16)
    nz, pitch = n // 2 + 1, (n // 2 + 1 + 15) // 16 * 16
    grid = fields.grid(n, "f32")
    spec = torch.empty((n, n, pitch), dtype=torch.complex64, device="cuda")
    _lib.check(hip.ast_fft_tile_rows_r2c(dev.ptr(grid), dev.ptr(spec), 0, n, n * n, n, pitch, 1.0, dev.stream()))
    packed = torch.empty((n * lay["total"],), dtype=torch.complex64, device="cuda")
    _lib.check(hip.ast_fft_tile_c2c_disc(dev.ptr(spec), dev.ptr(packed), 0, n, pitch, n, parts, -1, None, 1.0, dev.stream()))
    scratch = torch.empty(int(hip.ast_fft_tile_disc_power_scratch_bytes(n, parts)), dtype=torch.uint8, device="cuda")

    def sums(L, rule):
        total = torch.zeros(n // 2 - 1, dtype=torch.float64, device="cuda")
        for q in range(parts):
            block = packed[n * lay["cumS"][q]: n * (lay["cumS"][q] + lay["S"][q])].clone()
            psum = torch.zeros_like(total)
            _lib.check(hip.ast_fft_tile_disc_block_power(dev.ptr(block), dev.ptr(scratch), scratch.numel(), 0, n, parts, q,
                                                         1.0 / float(n) ** 3, L, 0, _lib.BIN[rule], dev.ptr(psum), dev.stream()))
            total += psum
        return total
    _run("disc blocks", fields, n, "f32", sums)


# ---------------------------------------------------------------- spikes: every mode of every shell at once
# One cell of value 1000: |delta_k|^2 = 1e6 / N^6 for EVERY mode, so psum[s] N^6 / (L^3 1e6 nmodes[s]) = 1 on every shell and a
# mode that is missing or counted twice shows as 1 / nmodes[s].  float64: 1e-12.  float32: four times the worst deviation
# of the plain fp32 route (power_bin_1d(r2c(grid, engine="rocfft"))) on the same grid, measured on an MI355X (SPIKE_PLAIN_F32;
# the fused routes themselves: 2.5e-7 at side 256, 3.0e-7 at side 512) - two correct fp32 transforms differ by a small
# factor.  Where the allowance is not below 1 / (2 nmodes[s]) the shell is left out - the assertion could not see one mode
# there: side 256 keeps every shell (1.13e-6 < 2.44e-6), side 512 the shells below |m| ~ 204 (9.5e-7 against 6.1e-7 at the
# fullest shell) - and the 32 lowest shells must all stay in.
SPIKE_PLAIN_F32 = {256: 2.82e-7, 512: 2.38e-7}
SPIKE_F32_ALLOW = {n: 4 * v for n, v in SPIKE_PLAIN_F32.items()}
SPIKE_CELL = lambda n: (1, n - 1, n // 2 - 1)


def _spike_ratio(n, boxsize, psum, nmodes):
    return psum.cpu().numpy() * float(n) ** 6 / (boxsize ** 3 * 1e6 * nmodes.cpu().numpy())


@pytest.mark.parametrize("route,n", [("fused f32", 256), ("fused f32", 512), ("big f32", 256), ("fused f64", 128), ("fused f64", 256)])
def test_single_spike_fills_every_shell_evenly(dev, route, n):
    L = 1000.0
    dtype = torch.float64 if route == "fused f64" else torch.float32
    t = pp.spike_field(n, [SPIKE_CELL(n)], [1000.0], dtype, "cuda")
    for rule in RULES:
        if route == "fused f32":
            _, psum, nmodes = dev.power_sums_fused(t, L, binning=rule)
        elif route == "big f32":
            _, psum, nmodes = dev.power_sums_fused64(t, L, binning=rule, mean=0.0)
        else:
            _, psum, nmodes = dev.power_sums_fused64(t, L, binning=rule)
        dev_ = np.abs(_spike_ratio(n, L, psum, nmodes) - 1)
        if dtype == torch.float32:                     # the plain fp32 route on the same grid, for the record
            _, p0, _ = dev.power_bin_1d(dev.r2c(t, engine="rocfft"), None, n, L, binning=rule)
            print(f"SPIKE plain c64 rocfft n={n} {rule}: worst deviation {np.abs(_spike_ratio(n, L, p0, nmodes) - 1).max():.3e}")
        print(f"SPIKE {route} n={n} {rule}: worst deviation {dev_.max():.3e} at shell {dev_.argmax()}, "
              f"1 / (2 max nmodes) = {0.5 / float(nmodes.max()):.3e}")
        if dtype == torch.float64:
            assert dev_.max() <= 1e-12
            continue
        allow = SPIKE_F32_ALLOW[n]
        seen = allow < 0.5 / nmodes.cpu().numpy()
        assert seen[:32].all()
        assert dev_[seen].max() <= allow, (route, n, rule, int(seen.sum()))


@pytest.mark.parametrize("route,n,rtol", [("fused f32", 256, 1e-6), ("fused f64", 128, 1e-12)])
def test_spike_pair_against_the_oracle(dev, route, n, rtol):
    """Two cells, 700 at the origin and -300 at (17, n - 16, 33): P(k) depends on WHERE the second one is read from - the
    real-space addressing, which one spike cannot show."""
    L = 1000.0
    cells, values = [(0, 0, 0), (17, n - 16, 33)], [700.0, -300.0]
    ref = offt.fftpower_1d(pp.spike_field(n, cells, values), L)
    dtype = torch.float32 if route == "fused f32" else torch.float64
    t = pp.spike_field(n, cells, values, dtype, "cuda")
    fn = dev.power_sums_fused if route == "fused f32" else dev.power_sums_fused64
    res = dev.finish_power(*fn(t, L))
    assert np.array_equal(res["modes"], ref["modes"])
    err = np.abs(res["power"] / ref["power"].real - 1)
    print(f"SPIKE PAIR {route} n={n}: worst deviation {err.max():.3e} at shell {err.argmax()}")
    np.testing.assert_allclose(res["power"], ref["power"].real, rtol=rtol)
