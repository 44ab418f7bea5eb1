"""GPU: the y-split route of the fused fp32 power passes - the z pass takes its 16 rows n/16 apart in y and
does the first radix-16 stage of the y transform, the k_y pass the remaining n/16 points, and the last pass reads k_y off
the permuted row index.  Default at side 1024; AST_FFT_YSPLIT=1 takes it at sides 256 and 512 (remaining transform 16 and
32 points), AST_FFT_YSPLIT=0 gives the passes as they were.  tests/test_fft_ysplit_cpu.py restates the factorisation.

Tolerances: the plane-wave probes carry those of tests/test_gpu_power_probes.py (1e-6 on a probed shell, 1e-12 of the
total in an empty one).  Route against route: each route is within the project's 1e-6 of the float64 passes, so two
routes agree within 2e-6; the low-k patched shells come from per-row z sums whose arithmetic does not change - same bits.
"""
import os

import numpy as np
import pytest

from tests import power_probes as pp
from tests.test_gpu_power_probes import BOXES, MEAN, RULES, TOL
from tests.test_gpu_fft_power_unused_work import _check_reordered, _poison_scratch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LOWK_SHELLS = 5                      # shells 0 .. 4 are patched from the double-precision channel


@pytest.fixture(scope="module")
def dev(hip):
    from astrild_amd import device
    torch.cuda.set_device(0)
    return device


class _env:
    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _route(n):
    """The environment that takes the new route at side n."""
    return {"AST_FFT_YSPLIT": None if n == 1024 else "1"}


def _psum(dev, g, L=1000.0, env=None, **kw):
    with _env(**(env or {})):
        return dev.power_sums_fused(g, L, **kw)[1].clone()


def _random_grid(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((n, n, n), dtype=torch.float32, device="cuda", generator=g)


# ---------------------------------------------------------------- a. plane-wave probes
def extra_probes(n, have):
    """Probes at the k_y where the split's index arithmetic turns over - around one block of 16, around n/16 rows,
    around the Nyquist row, the last rows - each at the k_z of the tile seams, and vectors just inside, on and just
    outside norm n/2 with the large component on y.  Vectors outside the shells stay in: they must add nothing."""
    R = n // 2
    kys = [1, 15, 16, 17, n // 16 - 1, n // 16, R - 1, R, R + 1, n - 16, n - 1]
    kzs = [0, 15, 16, 31, 32, R - 1]
    ms = []
    for i, ky in enumerate(kys):
        for j, kz in enumerate(kzs):
            kx = (1 + (i + 2 * j) % 3) * (-1 if (i + j) % 2 else 1)
            ms.append((kx, ky, kz))
    for v, sgn in ((R * R - 2, 1), (R * R - 3, -1), (R * R + 1, 1), (R * R + 2, -1)):      # just inside, just outside
        t = pp.three_squares(v)
        if t is not None:
            ms.append((t[2], sgn * t[0], t[1]))
    ms += [(0, R, 0), (1, R, 0), (0, R, 1)]                                                 # on the edge and one step out
    seen = {m for m, _, _ in have}
    rng = np.random.default_rng([n, 42])
    out = []
    for m in ms:
        m = pp.canonical(m, n)
        if m in seen:
            continue
        seen.add(m)
        phi = float(rng.uniform(-1.0, 1.0)) if pp.is_self_conjugate(m, n) else float(rng.uniform(0.0, 2.0 * np.pi))
        out.append((m, float(rng.uniform(0.6, 1.35)), phi))
    inside = [m for m, _, _ in out if pp.integer_shell(m, n) is not None]
    assert len(inside) >= 40 and len(out) - len(inside) >= 4                               # both kinds are there
    for ky in kys:                                                                          # every k_y index is hit
        assert any((m[1] % n) in (ky, (n - ky) % n) for m in inside + [m for m, _, _ in have]), ky
    return out


@pytest.mark.parametrize("lowk", [True, False])
@pytest.mark.parametrize("n", [256, 512])
def test_plane_wave_probes(dev, n, lowk):
    probes = pp.probe_set(n)
    probes = probes + extra_probes(n, probes)
    g = pp.probe_field(n, probes, MEAN, torch.float32, "cuda")
    rtol, eps = TOL["f32"]
    for L in BOXES:
        for rule in RULES:
            want = pp.expected_psum(n, L, probes, rule)
            got = _psum(dev, g, L, _route(n), mean=MEAN, lowk=lowk, binning=rule).cpu().numpy()
            signal = want > 0
            rel = np.abs(got[signal] / want[signal] - 1).max()
            leak = np.abs(got[~signal]).max() / want.sum() if (~signal).any() else 0.0
            print(f"YSPLIT PROBE n={n} lowk={int(lowk)} L={L:g} {rule}: signal shells {rel:.2e}, empty shells / total {leak:.2e}")
            assert rel <= rtol, (n, L, rule)
            assert leak <= eps * eps, (n, L, rule)


def test_low_k_sums_as_kernels_of_their_own(dev):
    """AST_LOWK_SEPARATE=1 on the new route: the treatment of test_fused_float32_variants."""
    n = 256
    probes = pp.probe_set(n)
    g = pp.probe_field(n, probes, MEAN, torch.float32, "cuda")
    rtol, eps = TOL["f32"]
    for L in BOXES:
        for rule in RULES:
            want = pp.expected_psum(n, L, probes, rule)
            got = _psum(dev, g, L, {**_route(n), "AST_LOWK_SEPARATE": "1"}, mean=MEAN, binning=rule).cpu().numpy()
            signal = want > 0
            assert np.abs(got[signal] / want[signal] - 1).max() <= rtol, (L, rule)
            assert np.abs(got[~signal]).max() / want.sum() <= eps * eps, (L, rule)


# ---------------------------------------------------------------- b. route against route
@pytest.mark.parametrize("lowk", [True, False])
@pytest.mark.parametrize("n", [256, 512, 1024])
def test_route_against_route(dev, n, lowk):
    t = _random_grid(n, 100 + n)
    new = _psum(dev, t, env=_route(n), lowk=lowk)
    old = _psum(dev, t, env={"AST_FFT_YSPLIT": None if n != 1024 else "0"}, lowk=lowk)
    assert torch.isfinite(new).all() and float(new.min()) > 0.0
    rel = ((new - old).abs() / old).max().item()
    print(f"YSPLIT ROUTES n={n} lowk={int(lowk)}: largest relative difference {rel:.2e}, shells that differ {(new != old).sum().item()}")
    assert rel <= 2e-6
    assert (new != old).any(), "the two routes are different arithmetic: the switch did nothing"
    if lowk:
        assert torch.equal(new[:LOWK_SHELLS], old[:LOWK_SHELLS])
    del t
    if n == 1024:
        dev._power_scratch.clear()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- c, f. poisoned scratch, repeats
@pytest.mark.parametrize("n", [256, 1024])
def test_poisoned_scratch_and_three_calls_in_a_row(dev, n):
    t = _random_grid(n, 7 + n)
    base = _psum(dev, t, env=_route(n))
    assert torch.isfinite(base).all()
    for _ in range(2):
        assert torch.equal(_psum(dev, t, env=_route(n)), base), "three calls in a row"
    _poison_scratch(dev, n)
    got = _psum(dev, t, env=_route(n))
    assert torch.isfinite(got).all()
    assert torch.equal(got, base), "scratch full of NaN before the call"
    del t
    if n == 1024:
        dev._power_scratch.clear()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- d. the switches on the new route
def test_switches_keep_their_meaning(dev):
    n = 256
    t = _random_grid(n, 19)
    t -= t.mean()
    for L, rule in ((1000.0, "integer"), (1000.0, "float64")):
        with _env(**_route(n)):
            base = dev.power_sums_fused(t, L, binning=rule)[1].clone()
            assert torch.isfinite(base).all() and float(base[-1]) > 0.0
            for var in ("AST_FFT_NO_PRUNE", "AST_FFT_NYQ_COLUMN", "AST_FFT_NO_EPI_SKIP"):
                with _env(**{var: "1"}):
                    assert torch.equal(dev.power_sums_fused(t, L, binning=rule)[1], base), (var, rule)
            _check_reordered(dev, t, L, rule, base, n)                  # AST_FFT_SHELL_ATOMICS=1 within its bound


# ---------------------------------------------------------------- e. the deferred fold
@pytest.fixture(scope="module")
def edge_particles():
    """2^17 particles of a 256^3 box of unit cells in the cells x, y = 0 and 7 mod 8 - the faces, edges and corners of the
    paint's tile columns, whose deposits go through the halo records - 2048 of them in the box's four corner columns and
    2048 in the first and last z plane, so that records and windows wrap around every axis.  Random order."""
    n, npart = 256, 1 << 17
    rng = np.random.default_rng(78)
    cell = np.empty((npart, 3), dtype=np.int64)
    cell[:, :2] = 8 * rng.integers(0, n // 8, size=(npart, 2)) + 7 * rng.integers(0, 2, size=(npart, 2))
    cell[:, 2] = rng.integers(0, n, size=npart)
    cell[:2048, :2] = (n - 1) * rng.integers(0, 2, size=(2048, 2))
    cell[2048:4096, 2] = (n - 1) * rng.integers(0, 2, size=2048)
    pos = (cell + rng.uniform(0.05, 0.95, size=(npart, 3))).astype(np.float32)
    assert pos.min() >= 0.0 and pos.max() < n
    return pos


@pytest.mark.parametrize("window", ["cic", "tsc"])
def test_fold_on_load_through_the_new_route(dev, edge_particles, window):
    """paint(defer_fold=True) + power_sums_fused(halo=) against the paint that folds its records itself, both through the
    new route, with every particle on a tile edge or corner (rows of one, two and three record lines, the periodic wrap
    included; the exact two-pass lists, as in tests/test_gpu_zpass_seam.py): the same bits in every shell."""
    n, L = 256, 256.0
    pos = dev.as_device(edge_particles)
    mean = pos.shape[0] / float(n) ** 3
    with _env(**_route(n)):
        grid = dev.paint(pos, None, n, L, window, method="tiled2")
        ref = dev.power_sums_fused(grid, L, mean=mean)[1].clone()
        grid2, halo = dev.paint(pos, None, n, L, window, method="tiled2", defer_fold=True)
        assert not torch.equal(grid2, grid)                              # the deferred grid alone is incomplete
        got = dev.power_sums_fused(grid2, L, mean=mean, halo=halo)[1]
        assert torch.isfinite(ref).all() and ref.abs().max().item() > 0.0
        assert torch.equal(got, ref)
    with _env(AST_FFT_YSPLIT="0"):                                       # and the switch did take another route
        assert not torch.equal(dev.power_sums_fused(grid, L, mean=mean)[1], ref)
