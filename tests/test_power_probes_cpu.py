"""The probe helper against the oracle on the host: the closed-form shell sums of tests/power_probes.py equal the oracle's
binning of the transformed probe field, mode for mode, under both shell rules - so that the GPU tests
(test_gpu_power_probes.py) may compare device results with the closed form alone."""
import numpy as np
import pytest

from oracle import fftpower as offt
from tests import power_probes as pp

BOXES = (1000.0, 100.0, 2.0 * np.pi)


@pytest.fixture(scope="module", params=[32, 64])
def case(request):
    n = request.param
    probes = pp.probe_set(n)
    f64 = pp.probe_field(n, probes, mean=2.0)
    spec = {}
    for name, f in (("f64", f64), ("f32", f64.astype(np.float32))):
        c = offt.r2c(f)
        p3d = (c * np.conj(c)).real
        p3d[0, 0, 0] = 0.0
        spec[name] = p3d
    return n, probes, spec


@pytest.mark.parametrize("binning", ["integer", "float64"])
@pytest.mark.parametrize("boxsize", BOXES)
def test_closed_form_equals_the_oracle(case, boxsize, binning):
    n, probes, spec = case
    want = pp.expected_psum(n, boxsize, probes, binning)
    _, got, _ = offt.project_1d(spec["f64"] * boxsize ** 3, n, boxsize, binning)
    err = np.abs(got.real - want).max() / want.max()
    print(f"n={n} L={boxsize:g} {binning}: float64 field, worst |oracle - closed form| / peak = {err:.2e}")
    assert err <= 1e-13


@pytest.mark.parametrize("binning", ["integer", "float64"])
@pytest.mark.parametrize("boxsize", BOXES)
def test_float32_rounding_of_the_field_is_far_below_the_gpu_tolerances(case, boxsize, binning):
    n, probes, spec = case
    want = pp.expected_psum(n, boxsize, probes, binning)
    _, got, _ = offt.project_1d(spec["f32"] * boxsize ** 3, n, boxsize, binning)
    got, signal = got.real, want > 0
    rel = np.abs(got[signal] / want[signal] - 1).max()
    leak = got[~signal].max() / want.max() if (~signal).any() else 0.0
    print(f"n={n} L={boxsize:g} {binning}: float32 field, signal shells {rel:.2e}, empty shells / peak {leak:.2e}")
    assert rel <= 1e-8
    assert leak <= 1e-14


@pytest.mark.parametrize("n", [32, 64, 128, 256, 512, 1024])
def test_probe_set_holds_every_category(n):
    probes = pp.probe_set(n)
    pp.check_categories(n, probes)                         # (probe_set asserts it too)
    assert probes == pp.probe_set(n)                       # deterministic
    assert [m for m, _, _ in pp.probe_set(n, seed=1)] != [m for m, _, _ in probes]
    for m, _, _ in probes:
        assert all(-n // 2 < c <= n // 2 for c in m) and m[2] >= 0


def test_a_probe_that_is_lost_or_moved_shows_in_the_closed_form():
    """What the GPU assertions rest on: every probe carries at least 5 % of its shell, and the float64 rule at L = 100 moves
    probes that the integer rule keeps (otherwise a run under it would say nothing about the rule)."""
    for n in (64, 256):
        probes = pp.probe_set(n)
        full = pp.expected_psum(n, 1000.0, probes, "integer")
        for i in range(len(probes)):
            less = pp.expected_psum(n, 1000.0, probes[:i] + probes[i + 1:], "integer")
            s = np.nonzero(full != less)[0]
            if pp.integer_shell(probes[i][0], n) is None:
                assert len(s) == 0
            else:
                assert len(s) == 1 and 1 - less[s[0]] / full[s[0]] >= pp.MIN_SHARE
        assert not np.array_equal(pp.expected_psum(n, 100.0, probes, "float64"), pp.expected_psum(n, 100.0, probes, "integer"))


def test_spike_field_and_its_spectrum():
    n, L = 32, 100.0
    f = pp.spike_field(n, [(1, n - 1, n // 2 - 1)], [1000.0])
    assert f.sum() == 1000.0 and f[1, n - 1, n // 2 - 1] == 1000.0
    r = offt.fftpower_1d(f, L)
    np.testing.assert_allclose(r["power"].real * float(n) ** 6 / (L ** 3 * 1e6), 1.0, rtol=1e-12)
