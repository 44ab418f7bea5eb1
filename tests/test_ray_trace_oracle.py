"""Without a GPU: tests/ray_trace_oracle.py against what the multi-plane algorithm must give - the 2 x 2 matrix
recursion on quadratic sheets, the Born sum of ``LensPlanes.convergence`` less the mean term, and the Laplacian of the
potential - so that the GPU tests, which compare the device with that oracle byte for byte, compare it with the physics."""
import numpy as np
import pytest

from tests import ray_trace_oracle as orc

OMEGA_M = 0.3
CASES = [(8, 1), (12, 2), (32, 2)]                 # (npix, pad)


def quadratic_sheet(m, h, a, b, c):
    """psi = (a beta1^2 + b beta2^2) / 2 + c beta1 beta2 on the nodes, beta = (node - m / 2) h: central differences and
    the bilinear rule are exact on it, grad psi = (a beta1 + c beta2, c beta1 + b beta2), grad grad psi constant."""
    b1 = ((np.arange(m, dtype=np.float64) - m // 2) * h)[:, None]
    b2 = ((np.arange(m, dtype=np.float64) - m // 2) * h)[None, :]
    return 0.5 * (a * b1 * b1 + b * b2 * b2) + c * b1 * b2


def matrix_recursion(U, chi, chi_s, born):
    """A' = d beta / d theta - I at the source, by the recursion of the issue on 2 x 2 matrices."""
    A, B, prev = np.zeros((2, 2)), np.zeros((2, 2)), 0.0
    for Uk, ck in zip(U, chi):
        A = (prev * A + (ck - prev) * B) / ck
        B = B - (Uk if born else Uk @ (np.eye(2) + A))
        prev = ck
    return (prev * A + (chi_s - prev) * B) / chi_s


@pytest.mark.parametrize("born", [False, True])
def test_quadratic_sheets_follow_the_matrix_recursion(born):
    npix, h = 64, 2.0 ** -12
    chi, chi_s = np.array([300.0, 750.0, 1300.0]), 2100.0
    coeff = [(0.11, -0.07, 0.05), (-0.06, 0.09, 0.03), (0.08, 0.04, -0.05)]
    psis = [quadratic_sheet(npix, h, *abc) for abc in coeff]
    U = [np.array([[a, c], [c, b]]) for a, b, c in coeff]
    st, prev = orc.state(npix), 0.0
    inner = slice(16, 48)
    for psi, ck in zip(psis, chi):
        st = orc.step(psi, st, h, prev, float(ck), born)
        prev = float(ck)
        # the stencils of the rays compared below stay 8 nodes and more from the seam, where the sheet is not periodic
        assert np.abs(st[:2, inner, inner]).max() / h < 7.0
    if not born:
        assert np.abs(st[:2, inner, inner]).max() / h > 1.0          # ... and the rays do leave their pixels
    maps = orc.emit(st, prev, chi_s)
    want = matrix_recursion(U, chi, chi_s, born)
    got = np.array([[-maps[0] - maps[1], -maps[2] - maps[3]], [-maps[2] + maps[3], -maps[0] + maps[1]]])[:, :, inner, inner]
    err = np.abs(got - want[:, :, None, None]).max(axis=(2, 3)) / np.abs(want)
    print("A' against the matrix recursion, largest relative error per entry:", err)
    assert np.all(err <= 1e-12)
    if born:
        assert np.all(maps[3] == 0.0)
    else:
        assert abs(want[1, 0] - want[0, 1]) > 1e-4                   # lens-lens coupling rotates: omega is not 0
    # the deflection: alpha = -d_s, and d_s = A' theta for sheets centred on theta = 0
    theta = (np.arange(npix, dtype=np.float64) - npix // 2) * h
    d1 = want[0, 0] * theta[:, None] + want[0, 1] * theta[None, :]
    d2 = want[1, 0] * theta[:, None] + want[1, 1] * theta[None, :]
    scale = np.abs(d1[inner, inner]).max()
    assert np.abs(-maps[4] - d1)[inner, inner].max() <= 1e-12 * scale and np.abs(-maps[5] - d2)[inner, inner].max() <= 1e-12 * scale


def test_a_single_sheet_gives_the_born_weight():
    """One plane of uniform Sigma: psi = chi_k Sigma (beta1^2 + beta2^2) / 2, kappa = g(chi_k, chi_s) Sigma, no shear."""
    npix, h, chi_k, chi_s, Sigma = 64, 2.0 ** -12, 800.0, 1900.0, 3.1e-5
    psi = quadratic_sheet(npix, h, chi_k * Sigma, chi_k * Sigma, 0.0)
    maps = orc.emit(orc.step(psi, orc.state(npix), h, 0.0, chi_k), chi_k, chi_s)
    inner = slice(16, 48)
    g = (chi_s - chi_k) * chi_k / chi_s
    np.testing.assert_allclose(maps[0][inner, inner], g * Sigma, rtol=1e-12, atol=0)
    assert np.abs(maps[1:4, inner, inner]).max() <= 1e-12 * g * Sigma


def random_planes(npix, pad, seed):
    rng = np.random.default_rng(seed)
    P = 3
    planes = rng.normal(0.0, 40.0, size=(P, npix, npix))
    chi = np.array([250.0, 610.0, 1400.0])
    a = 1.0 / (1.0 + np.array([0.09, 0.22, 0.55]))
    return planes, chi, a, np.radians(3.0) / npix


@pytest.mark.parametrize("npix,pad", CASES)
def test_born_mode_is_the_born_sum_less_the_mean_term(npix, pad):
    planes, chi, a, h = random_planes(npix, pad, 100 + npix)
    w = orc.plane_weights(a, OMEGA_M)
    psis = [orc.potential(planes[k], h, pad, chi[k] * w[k])[0] for k in range(len(chi))]
    src = [2300.0, 900.0]
    maps = orc.trace(psis, npix, chi, h, src, born=True)
    for s, chi_s in enumerate(src):
        g = np.where(chi < chi_s, (chi_s - chi) * chi / chi_s, 0.0)
        want = sum(w[k] * g[k] * (planes[k] - planes[k].sum() / (pad * npix) ** 2) for k in range(len(chi)))
        err = np.abs(maps[0, s] - want).max() / np.abs(want).max()
        print(f"npix {npix} pad {pad} chi_s {chi_s}: born identity off by {err:.2e} of max |kappa|")
        assert err <= 1e-12
        assert np.all(maps[3, s] == 0.0)
    assert np.abs(maps[0, 1] - maps[0, 0]).max() > 0


@pytest.mark.parametrize("npix,pad", CASES)
def test_the_potential_has_the_laplacian_it_was_solved_for(npix, pad):
    planes, chi, a, h = random_planes(npix, pad, 100 + npix)
    for sigma in planes:
        psi, grid = orc.potential(sigma, h, pad, 1.0)
        err = np.abs(orc.laplacian(psi, h) - 2.0 * (grid - grid.mean())).max() / np.abs(sigma).max()
        print(f"npix {npix} pad {pad}: laplacian identity off by {err:.2e} of max |sigma|")
        assert err <= 1e-12
        assert abs(psi.mean()) <= 1e-12 * np.abs(psi).max()


def test_sources_between_planes_in_any_order():
    planes, chi, a, h = random_planes(8, 1, 7)
    w = orc.plane_weights(a, OMEGA_M)
    psis = [orc.potential(planes[k], h, 1, chi[k] * w[k])[0] for k in range(3)]
    src = [1500.0, 100.0, 611.0, 610.0, 250.0]
    maps = orc.trace(psis, 8, chi, h, src)
    assert np.all(maps[:, 1] == 0.0) and np.all(maps[:, 4] == 0.0)              # at or in front of the first plane
    assert maps[:, 2].tobytes() == orc.trace(psis[:2], 8, chi[:2], h, [611.0])[:, 0].tobytes()
    assert maps[:, 3].tobytes() == orc.trace(psis[:1], 8, chi[:1], h, [610.0])[:, 0].tobytes()   # a plane AT the source: not in front
    assert maps[:, 0].tobytes() == orc.trace(psis, 8, chi, h, [1500.0])[:, 0].tobytes()


def test_product_helpers_without_a_device():
    """The host-side rules of astrild_amd.ray_trace: the pad, and which plane serves a source."""
    pytest.importorskip("torch")
    from astrild_amd import ray_trace as rt
    assert rt.STATE == orc.STATE and rt.QUANTITIES == orc.QUANTITIES
    assert rt.check_pad(1) == 1 and rt.check_pad(np.int64(2)) == 2
    for bad in (0, 3, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="pad"):
            rt.check_pad(bad)
    chi = [250.0, 610.0, 1400.0]
    assert [rt.emitting_plane(chi, c) for c in (0.0, 250.0, 250.1, 610.0, 1400.0, 1e4)] == [-1, -1, 0, 0, 1, 2]


def test_the_largest_npix_is_the_one_the_step_entry_takes():
    """``ast_ray_step`` refuses ``(npix + RAY_BY - 1) / RAY_BY > 65535`` rows of workgroups; ``NPIX_MAX`` is the largest
    npix that passes, read from the source, and ``ray_state`` refuses the next one before it allocates (no device here)."""
    import os
    import re
    pytest.importorskip("torch")
    from astrild_amd import ray_trace as rt
    src = open(os.path.join(os.path.dirname(os.path.abspath(rt.__file__)), "csrc", "ray_trace.hip")).read()
    rows = int(re.search(r"constexpr int RAY_BX = \d+, RAY_BY = (\d+);", src).group(1))
    most = int(re.search(r"AST_CHECK_ARG\(\(npix \+ RAY_BY - 1\) / RAY_BY <= (\d+)\);", src).group(1))
    assert (rows, most) == (4, 65535)
    assert (rt.NPIX_MAX + rows - 1) // rows <= most < (rt.NPIX_MAX + 1 + rows - 1) // rows
    assert rt.NPIX_MAX == 4 * 65535 == 262140
    for bad in (rt.NPIX_MAX + 1, 1 << 18, 0, -1):
        with pytest.raises(ValueError, match="npix must lie in 1 .. 262140"):
            rt.ray_state(bad)
