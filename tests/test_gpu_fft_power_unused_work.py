"""GPU: the work the fused fp32 power passes (ast_fft_tile_power_3d) leave out changes nothing FFTPower bins.

Left out, each with a switch that restores the pass as it was (tests/test_power_skip_cpu.py restates the geometry):
A. the column k_z = N/2: the k_y pass takes N/2 columns, the last pass prunes the tile that starts there
   (AST_FFT_NYQ_COLUMN=1 keeps the column in both);
B. the epilogue steps of waves whose rows lie beyond the Nyquist sphere (AST_FFT_NO_EPI_SKIP=1 does them);
(C of the proposal, no zero rows in `partial`, measured no gain and is not in the code: profiles/EXPERIMENTS.md.)
And D: the last pass adds into one shell table per column lane and sums the tables in lane order (AST_FFT_SHELL_ATOMICS=1:
one table for all lanes, as before) - another order of the same double-precision adds.

Sides: 256 (16 x 16 points, unsplit exchange), 512 (16 x 32); 1024 (split exchange, 32-column k_y tiles) in one test.
Plane-wave probes (tests/power_probes.py) have their whole power in one shell: 1e-6 relative on a probed shell - the
project's fp32 tolerance - and every unprobed shell below 1e-6 of the smallest probe's power.
"""
import math
import os

import numpy as np
import pytest

from tests import power_probes as pp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

R1 = {256: 16, 512: 16, 1024: 32}                     # rows k_x index = sub + R1 * k2 in the binning pass
SWITCH = {"A": "AST_FFT_NYQ_COLUMN", "B": "AST_FFT_NO_EPI_SKIP", "D": "AST_FFT_SHELL_ATOMICS"}
BOXES = ((1000.0, "integer"), (1000.0, "float64"), (700.0, "float64"))


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
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _psum(dev, g, L, rule, off=()):
    with _env(**{SWITCH[s]: "1" for s in off}):
        return dev.power_sums_fused(g, L, binning=rule)[1].clone()


def _check_reordered(dev, t, L, rule, base, n):
    """D against off: the same M_s non-negative doubles of a shell added in another order differ by at most
    2 M_s 2^-53 sum_s (each of the M_s - 1 adds of either order rounds by at most 2^-53 of a partial sum <= sum_s)."""
    old = _psum(dev, t, L, rule, ("D",))
    modes = torch.as_tensor(dev.power_sums_fused(t, L, binning=rule)[2]).to(base.device, torch.float64)
    bound = 2.0 * modes * 2.0 ** -53 * torch.maximum(base, old)
    worst = ((base - old).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"TABLES n={n} L={L:g} {rule}: largest |tables - one table| / bound {worst:.3g}, shells that differ {(base != old).sum().item()}")
    assert ((base - old).abs() <= bound).all()
    return old


def _poison_scratch(dev, n):
    """NaN in every byte pattern of the cached scratch: spectrum, partial rows, reducer rows, low-k area."""
    for key, scratch in dev._power_scratch.items():
        if key[1] == n:
            scratch.fill_(0xFF)
            return
    raise AssertionError("no scratch cached: call the pipeline once first")


def edge_pairs(n):
    """[(inside, outside)]: k_x = +-floor(sqrt((N/2)^2 - k_y^2 - k_z^2)) and the same with one added to |k_x|, for (k_y, k_z)
    that put the two rows on either side of a boundary of the skip's row blocks: +k_x = R1 - 1 mod R1 (rows k_x, k_x + 1),
    -k_x with |k_x| = 0 mod R1 (rows N - |k_x|, N - |k_x| - 1).  k_z in tile 0, tile 1 and the tile at N/4; k_y of both signs."""
    R, r1 = n // 2, R1[n]
    out = []
    for sign, want in ((1, r1 - 1), (-1, 0)):
        for i, kz in enumerate((3, 21, n // 4 + 2)):
            for ky in range(2 + i, R):
                rem = R * R - ky * ky - kz * kz
                kx = math.isqrt(max(rem, 0))
                if rem > 0 and kx * kx != rem and kx % r1 == want and 1 <= kx < R - 1:
                    sy = -1 if (i + (sign > 0)) % 2 else 1
                    out.append(((sign * kx, sy * ky, kz), (sign * (kx + 1), sy * ky, kz)))
                    break
    assert len(out) == 6, out
    for a, b in out:
        assert pp.norm2(a) < R * R < pp.norm2(b) and pp.integer_shell(a, n) == R - 2 and pp.integer_shell(b, n) is None
    return out


def probe_list(n):
    R = n // 2
    ms = [(0, 0, R),                                   # the one mode of the Nyquist column with |m| <= N/2: dropped by both rules
          (0, 1, R - 1), (R - 1, 0, 1),                # last full tile / last rows, last shell
          (5, -7, 3), (-9, 4, n // 4 + 1),             # tile 0; the tile at k_z0 = N/4 (256 at side 1024)
          (-(R - 3), 2, 1), (3, -(R - 2), 17)]         # negative frequencies near the edge on both strided axes
    for a, b in edge_pairs(n):
        ms += [a, b]
    probes = []
    for i, m in enumerate(ms):
        m = pp.canonical(m, n)
        probes.append((m, 0.8 + 0.03 * i, 0.3 if pp.is_self_conjugate(m, n) else 0.37 * (i + 1)))
    assert len({m for m, _, _ in probes}) == len(probes)
    return probes


def _check_probes(dev, n, g, probes, off=()):
    R = n // 2
    for L, rule in BOXES:
        want = pp.expected_psum(n, L, probes, rule)
        assert pp.probe_shell((0, 0, R), n, L, rule) == -1           # (tests/test_power_skip_cpu.py: at every box size)
        got = _psum(dev, g, L, rule, off).cpu().numpy()
        signal = want > 0
        assert signal.sum() >= 4 and signal[R - 2]
        rel = np.abs(got[signal] / want[signal] - 1).max()
        smallest = min(L ** 3 * 0.5 * A * A for _, A, _ in probes)
        leak = np.abs(got[~signal]).max() / smallest
        print(f"PROBES n={n} L={L:g} {rule} off={''.join(off) or '-'}: probed shells {rel:.2e}, unprobed / smallest probe {leak:.2e}")
        assert rel <= 1e-6, (n, L, rule)
        assert leak <= 1e-6, (n, L, rule)
        # the last shell holds the six inside modes of the pairs and two more; one outside mode counted, or one inside
        # mode lost, moves it by more than 5 %
        share = min(0.5 * A * A for m, A, _ in probes if pp.integer_shell(m, n) == R - 2) * L ** 3 / want[R - 2]
        assert share > 0.05


def _random_grid(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randn((n, n, n), dtype=torch.float32, device="cuda", generator=g)
    t -= t.mean()
    return t


@pytest.mark.parametrize("n", [256, 512])
def test_plane_wave_probes(dev, n):
    probes = probe_list(n)
    g = pp.probe_field(n, probes, 0.0, torch.float32, "cuda")
    _check_probes(dev, n, g, probes)
    _check_probes(dev, n, g, probes, off=("A", "B", "D"))


@pytest.mark.parametrize("n", [256, 512])
def test_switches_dirty_memory_and_repeats_change_no_bit(dev, n):
    """B removes adds of nothing: bit-identical.  A removes the column k_z = N/2, whose only mode
    with |m| <= N/2 neither rule bins: every shell but the last is bit-identical because no workgroup that feeds it
    changes, and the last shell's bound - the rounding of that one mode's term, 1e-6 of it - is zero because the term is
    absent on both sides; so A is held to bit equality in every shell as well."""
    t = _random_grid(n, n + 11)
    for L, rule in BOXES[:2]:
        base = _psum(dev, t, L, rule)
        assert torch.isfinite(base).all() and float(base[-1]) > 0.0
        for off in (("B",), ("A",), ("A", "B")):
            assert torch.equal(_psum(dev, t, L, rule, off), base), (L, rule, off)
        old = _check_reordered(dev, t, L, rule, base, n)
        assert torch.equal(_psum(dev, t, L, rule, ("A", "B", "D")), old), "all three off against the tables alone off"
        assert torch.equal(_psum(dev, t, L, rule), base), "two calls in a row"
        _poison_scratch(dev, n)
        assert torch.equal(_psum(dev, t, L, rule), base), "scratch full of NaN before the call"
        _poison_scratch(dev, n)
        assert torch.equal(_psum(dev, t, L, rule, ("D",)), old), "scratch full of NaN, one shell table"


def test_side_1024(dev):
    """The split exchange and the k_y pass's 32-column tiles exist at this side only: probes, switches, dirty memory, repeat."""
    n = 1024
    probes = probe_list(n)
    g = pp.probe_field(n, probes, 0.0, torch.float32, "cuda")
    _check_probes(dev, n, g, probes)
    del g
    t = _random_grid(n, 5)
    L, rule = 1000.0, "float64"
    base = _psum(dev, t, L, rule)
    assert torch.isfinite(base).all() and float(base[-1]) > 0.0
    for off in (("B",), ("A",)):
        assert torch.equal(_psum(dev, t, L, rule, off), base), off
    _check_reordered(dev, t, L, rule, base, n)
    _poison_scratch(dev, n)
    assert torch.equal(_psum(dev, t, L, rule), base), "scratch full of NaN before the call"
    assert torch.equal(_psum(dev, t, L, rule), base), "two calls in a row"
    del t
    dev._power_scratch.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n", [256, 1024])
def test_k_y_pass_over_half_the_columns_never_touches_column_nyquist(dev, hip, n):
    """The k_y pass as power_3d_impl calls it with the column left out (N/2 columns, the row pitch of N/2 + 1 rounded up to
    16): column N/2 and the padding hold NaN before and the same bits after, and the N/2 columns are the transform."""
    from astrild_amd import _lib
    nzp, planes = (n // 2 + 1 + 15) // 16 * 16, 8
    g = torch.Generator(device="cuda").manual_seed(n)
    buf = torch.full((planes, n, nzp), float("nan"), dtype=torch.complex64, device="cuda")
    src = torch.randn((planes, n, n // 2, 2), dtype=torch.float32, device="cuda", generator=g)
    buf[:, :, :n // 2] = torch.view_as_complex(src)
    ref = torch.fft.fft(buf[:, :, :n // 2].to(torch.complex128), dim=1)
    tail = torch.view_as_real(buf[:, :, n // 2:]).view(torch.int32).clone()
    _lib.check(hip.ast_fft_tile_c2c(dev.ptr(buf), _lib.F32, n, nzp, n // 2, planes, n * nzp, 1.0, dev.stream()), "ast_fft_tile_c2c")
    assert torch.equal(torch.view_as_real(buf[:, :, n // 2:]).view(torch.int32), tail)
    err = (buf[:, :, :n // 2].to(torch.complex128) - ref).abs().max().item() / ref.abs().max().item()
    print(f"k_y pass over {n // 2} columns at side {n}: max error / max value {err:.2e}")
    assert err <= 1e-6           # fp32 transform of 256 ... 1024 points: a few 1e-7 of the largest value
