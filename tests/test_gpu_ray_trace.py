"""GPU: the multi-plane ray tracer (csrc/ray_trace.hip, astrild_amd/ray_trace.py, ``rays.LensPlanes.ray_trace``) against
tests/ray_trace_oracle.py.  Step and emit are compared ``tobytes()``; the potential, which goes through another FFT than
numpy's, by the Laplacian it was solved for, to the tolerance tests/test_ray_trace_oracle.py holds numpy's to; the whole
trace byte for byte against the oracle's step and emit fed with the device's own potentials."""
import math

import numpy as np
import pytest

from tests import dirty_memory as dm
from tests import plane_paint_oracle as porc, ray_trace_cases as cases, ray_trace_oracle as orc
from tests import stream_order as so

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

OMEGA_M = 0.3


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def rt(hip):
    from astrild_amd import ray_trace
    return ray_trace


@pytest.fixture(scope="module")
def lp(hip):
    from astrild_amd.rays import lens_planes
    return lens_planes


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same_bits(got, want):
    got = host(got) if isinstance(got, torch.Tensor) else got
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


# ------------------------------------------------------------------ (1) step and emit, byte for byte
preset_state, landing = cases.preset_state, cases.landing          # shared with the host build's test


@pytest.mark.parametrize("born", [False, True], ids=["full", "born"])
@pytest.mark.parametrize("npix,m", [(16, 16), (8, 16)])
def test_step_and_emit_on_preset_states_equal_the_oracle(rt, npix, m, born):
    h = 2.0 ** -10
    rng = np.random.default_rng(5 + npix)
    psi = rng.normal(0.0, 3.0 * h * h, size=(m, m))
    st = preset_state(npix, m, h, 11)
    p1, p2 = landing(st, h, 512.0, 1024.0)
    assert (p1 < 0).any() and (p2 < 0).any() and (p1 >= m).any() and (p2 >= m).any()
    assert ((p1 == np.floor(p1)) & (p2 == np.floor(p2))).any() and ((p1 != np.floor(p1)) & (p2 != np.floor(p2))).any()
    want = orc.step(psi, st, h, 512.0, 1024.0, born)
    assert np.isfinite(want).all() and np.abs(want[2:4, :4]).min() > 0              # (those rows had s = 0: deflected)
    state = up(st)
    assert rt.ray_step(up(psi), state, h, 512.0, 1024.0, born) is state
    assert same_bits(state, want)
    if born:                                                              # the position is the pixel's own, whatever d says
        assert np.array_equal(want[8:], orc.step(psi, np.concatenate([0 * st[:4], st[4:]]), h, 512.0, 1024.0, True)[8:])
    # a second plane from the result, distances that are no powers of two
    psi2 = rng.normal(0.0, 3.0 * h * h, size=(m, m))
    want2 = orc.step(psi2, want, h, 1024.0, 1711.3, born)
    rt.ray_step(up(psi2), state, h, 1024.0, 1711.3, born)
    assert same_bits(state, want2)
    maps = rt.ray_emit(state, 1711.3, 2950.7)
    assert same_bits(maps, orc.emit(want2, 1711.3, 2950.7))
    wide = torch.full((6, 3, npix, npix), 7.0, dtype=torch.float64, device="cuda")
    rt.ray_emit(state, 1711.3, 1711.4, out=wide[:, 1])
    assert same_bits(wide[:, 1].contiguous(), orc.emit(want2, 1711.3, 1711.4)) and bool((wide[:, [0, 2]] == 7.0).all())


@pytest.mark.parametrize("born", [False, True], ids=["full", "born"])
@pytest.mark.parametrize("npix,m", [(16, 16), (8, 16)])
def test_three_planes_from_the_observer_with_displacements_of_three_pixels(rt, npix, m, born):
    """chi_prev = 0 at the first plane; psi is scaled so that the rays are up to 3 pixels off when they meet plane 2."""
    h = math.radians(2.0) / 16
    chi = [410.0, 905.5, 1633.0]
    rng = np.random.default_rng(21 + npix)
    psis = [rng.normal(size=(m, m)) for _ in chi]
    first = orc.step(psis[0], orc.state(npix), h, 0.0, chi[0], born)
    psis[0] *= 3.0 * h / (np.abs(first[2:4]).max() * (chi[1] - chi[0]) / chi[1])
    psis[1] *= np.abs(psis[0]).max() / np.abs(psis[1]).max()
    psis[2] *= np.abs(psis[0]).max() / np.abs(psis[2]).max()
    state, st, prev = rt.ray_state(npix), orc.state(npix), 0.0
    assert tuple(state.shape) == (12, npix, npix) and state.dtype == torch.float64 and not bool(state.any())
    for k, ck in enumerate(chi):
        st = orc.step(psis[k], st, h, prev, ck, born)
        rt.ray_step(up(psis[k]), state, h, prev, ck, born)
        assert same_bits(state, st), k
        if k == 1:
            assert 2.9 < np.abs(st[:2]).max() / h < 3.1
        prev = ck
    assert same_bits(rt.ray_emit(state, chi[-1], 2200.0), orc.emit(st, chi[-1], 2200.0))
    if born:
        assert bool((rt.ray_emit(state, chi[-1], 2200.0)[3] == 0.0).all())


def test_no_state_reads_outside_the_potential(rt):
    """Displacements of 1e300, Inf and NaN pixels: every index is reduced into the grid (the source clamps floor(p) to
    +-2^30 before the conversion), the huge rays still equal the oracle and their neighbours are untouched."""
    npix = m = 16
    h = 2.0 ** -10
    rng = np.random.default_rng(3)
    psi = rng.normal(0.0, 3.0 * h * h, size=(m, m))
    st = preset_state(npix, m, h, 12)
    st[0, 5, :4] = [1e300, -1e300, 2.0 ** 31 * h, -2.0 ** 40 * h]
    st[1, 6, :4] = [np.inf, -np.inf, np.nan, 1e300]
    want = orc.step(psi, np.where(np.isfinite(st), st, 0.0), h, 512.0, 1024.0)
    state = up(st)
    rt.ray_step(up(psi), state, h, 512.0, 1024.0)
    got = host(state)
    keep = np.ones((npix, npix), dtype=bool)
    keep[6, :3] = False
    assert got[:, keep].tobytes() == want[:, keep].tobytes()
    assert np.isnan(got[3, 6, :3]).all()


def test_entries_refuse_bad_arguments(rt, hip):
    from astrild_amd import _lib
    psi, state = torch.zeros((16, 16), dtype=torch.float64, device="cuda"), rt.ray_state(8)
    with pytest.raises(ValueError, match="fit"):
        rt.ray_step(psi[:4, :4].contiguous(), state, 1e-3, 0.0, 100.0)
    with pytest.raises(ValueError, match="chi_prev"):
        rt.ray_step(psi, state, 1e-3, 100.0, 100.0)
    with pytest.raises(ValueError, match="behind"):
        rt.ray_emit(state, 100.0, 100.0)
    with pytest.raises(TypeError):
        rt.ray_step(psi.float(), state, 1e-3, 0.0, 100.0)
    s = torch.cuda.current_stream().cuda_stream
    assert hip.ast_ray_step(None, 16, state.data_ptr(), 8, 1e-3, 0.0, 100.0, 0, s) != 0
    assert b"ast_ray_step" in hip.ast_last_error()
    assert hip.ast_ray_step(psi.data_ptr(), 16, state.data_ptr(), 17, 1e-3, 0.0, 100.0, 0, s) != 0
    assert hip.ast_ray_step(psi.data_ptr(), 16, state.data_ptr(), 8, 1e-3, 100.0, 50.0, 0, s) != 0
    assert hip.ast_ray_step(psi.data_ptr(), 16, state.data_ptr(), 8, 0.0, 0.0, 100.0, 0, s) != 0
    assert hip.ast_ray_step(psi.data_ptr(), 16, state.data_ptr(), 8, 1e-3, 0.0, 100.0, 2, s) != 0
    assert hip.ast_ray_emit(state.data_ptr(), 8, 100.0, 200.0, psi.data_ptr(), 63, s) != 0
    assert hip.ast_ray_emit(state.data_ptr(), 8, 100.0, 100.0, psi.data_ptr(), 64, s) != 0
    assert hip.ast_lens_green_multiply(None, 16, 1.0, s) != 0
    assert hip.ast_lens_green_multiply(psi.data_ptr(), 0, 1.0, s) != 0
    assert hip.ast_lens_green_multiply(psi.data_ptr(), 4, float("nan"), s) != 0
    with pytest.raises(_lib.AstrildHipError, match="ast_ray_emit"):
        _lib.check(hip.ast_ray_emit(None, 8, 100.0, 200.0, psi.data_ptr(), 64, s), "ast_ray_emit")
    assert not bool(state.any()) and not bool(psi.any())


# ------------------------------------------------------------------ (2) the potential
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("npix,pad", [(16, 1), (8, 2), (24, 1), (12, 2)])
def test_the_device_potential_has_the_laplacian_it_was_solved_for(rt, npix, pad, dtype):
    rng = np.random.default_rng(40 + npix)
    sigma = rng.normal(0.0, 40.0, size=(npix, npix)).astype(dtype)
    h = math.radians(3.0) / npix
    m = pad * npix
    psi = rt.lens_potential(up(sigma), h, pad, 1.0)
    assert tuple(psi.shape) == (m, m) and psi.dtype == torch.float64
    ref, grid = orc.potential(sigma, h, pad, 1.0)
    err = np.abs(orc.laplacian(host(psi), h) - 2.0 * (grid - grid.mean())).max() / np.abs(sigma).max()
    print(f"npix {npix} pad {pad} {np.dtype(dtype).name}: laplacian identity off by {err:.2e} of max |sigma|")
    assert err <= 1e-12
    # two solutions of one Laplacian with mean 0 are the same function; both FFTs err by a few ulp of the largest value
    assert np.abs(host(psi) - ref).max() <= 1e-12 * np.abs(ref).max()
    # a workspace that has served another plane, an output of the caller's, a scale: the same function times the scale
    work = rt.potential_work(npix, pad)
    rt.lens_potential(up(rng.normal(size=(npix, npix))), h, pad, 3.0, work=work)
    out = torch.full((m, m), np.nan, dtype=torch.float64, device="cuda")
    assert rt.lens_potential(up(sigma), h, pad, 1.0, work=work, out=out) is out
    assert same_bits(out, host(psi))
    half = rt.lens_potential(up(sigma), h, pad, 0.5, work=work)
    assert np.abs(host(half) - 0.5 * host(psi)).max() <= 1e-14 * np.abs(ref).max()


# ------------------------------------------------------------------ (3) - (6) LensPlanes.ray_trace
def box_lens(lp, P, npix, dtype, seed=41):
    box = 100.0
    pos, mass = porc.particles(1000, box, seed, np.float32)
    return lp.LensPlanes.from_box(pos, mass, box, P, npix, OMEGA_M, chi0=500.0, dtype=dtype)


def cone_lens(lp, P, npix, dtype, seed=42):
    box = 100.0
    pos, mass = porc.particles(1000, box, seed, np.float64)
    edges = np.array([280.0, 345.5, 410.1, 520.0, 600.0]) if P == 4 else np.array([280.0, 600.0])
    lens = lp.LensPlanes.lightcone(npix, 30.0, edges, OMEGA_M, 1000 * 1.25 / (3 * box) ** 3, 2000, 2.0, dtype=dtype)
    for offset in ((0.0, 0.0, 0.0), (0.0, 0.0, 3 * box)):
        lens.add(pos, mass, (47.0, 52.5, -300.0), offset)
    return lens.finish()


def oracle_maps(rt, lp, lens, angle_deg, pad, zs, born):
    """The oracle's step and emit over the DEVICE's potentials, with the scale restated from the lens's distances."""
    h = math.radians(angle_deg) / lens.npix
    w = orc.plane_weights(lens.a, OMEGA_M)
    psis = [host(rt.lens_potential(lens.planes[k], h, pad, float(lens.chi[k] * w[k]))) for k in range(lens.nplanes)]
    src = [lp.flat_lcdm_comoving(z, OMEGA_M) for z in zs]
    return orc.trace(psis, lens.npix, lens.chi, h, src, born)


@pytest.mark.parametrize("born", [False, True], ids=["full", "born"])
@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("geometry,npix", [("box", 8), ("box", 11), ("cone", 12), ("cone", 9)])
def test_ray_trace_equals_the_oracle_over_the_device_potentials(rt, lp, geometry, npix, P, dt, born):
    dtype = getattr(torch, dt)
    if geometry == "box":
        lens, angle, pad, kw = box_lens(lp, P, npix, dtype), 4.0, 1, dict(opening_angle=4.0)
        zs = [1.0, 0.2]                                     # chi(0.2) = 571.7: between the last two of four planes
    else:
        lens, angle, pad, kw = cone_lens(lp, P, npix, dtype), 30.0, 2, {}
        zs = [0.14, 1.5]                                    # chi(0.14) = 407: behind two of four planes
    assert float(lens.planes.double().abs().max()) > 0
    res = lens.ray_trace(zs, born=born, **kw)
    want = oracle_maps(rt, lp, lens, angle, pad, zs, born)
    assert sorted(res) == sorted(orc.QUANTITIES)
    for q, name in enumerate(orc.QUANTITIES):
        assert res[name].is_cuda and same_bits(res[name], want[q]), name
    assert np.abs(want[0]).max() > 0 and np.abs(want[4]).max() > 0
    if P == 4:
        assert not np.array_equal(want[0, 0], want[0, 1])
    if geometry == "cone":                                   # the other pad is another (periodic) potential
        other = lens.ray_trace(zs, born=born, pad=1)
        assert same_bits(other["gamma1"], oracle_maps(rt, lp, lens, angle, 1, zs, born)[1])
        assert not same_bits(other["gamma1"], want[1])


@pytest.mark.parametrize("geometry", ["box", "cone"])
def test_born_mode_on_the_device_is_convergence_less_the_mean_term(lp, geometry):
    if geometry == "box":
        lens, pad, kw = box_lens(lp, 4, 12, torch.float64), 1, dict(opening_angle=4.0)
    else:
        lens, pad, kw = cone_lens(lp, 4, 12, torch.float64), 2, {}
    for z in (0.2, 1.0):
        res = lens.ray_trace(z, born=True, **kw)
        wnum, wden = lens.source_weights(z)
        means = host(lens.planes).sum(axis=(1, 2)) / (pad * lens.npix) ** 2
        want = host(lens.convergence(z)) - float(np.sum(wnum / wden * means))
        err = np.abs(host(res["kappa"]) - want).max() / np.abs(want).max()
        print(f"{geometry} z {z}: born identity on the device off by {err:.2e} of max |kappa|")
        assert err <= 1e-12
        assert bool((res["omega"] == 0.0).all())
        full = lens.ray_trace(z, **kw)
        assert not same_bits(full["kappa"], host(res["kappa"]))                          # post-Born terms: small, not 0
        print(f"   beyond Born: {np.abs(host(full['kappa']) - want).max() / np.abs(want).max():.2e} of max |kappa|, "
              f"max |omega| {float(full['omega'].abs().max()):.2e}")


def test_sources(rt, lp):
    lens = box_lens(lp, 4, 10, torch.float32)                # planes at chi = 512.5, 537.5, 562.5, 587.5
    zs = [1.0, 0.0, 0.2, 0.19]
    seq = lens.ray_trace(zs, opening_angle=4.0)
    for name in orc.QUANTITIES:
        assert tuple(seq[name].shape) == (4, 10, 10) and seq[name].dtype == torch.float64
        for s, z in enumerate(zs):
            one = lens.ray_trace(z, opening_angle=4.0)[name]
            assert tuple(one.shape) == (10, 10) and same_bits(seq[name][s].contiguous(), host(one)), (name, z)
        assert bool((seq[name][1] == 0.0).all())             # z = 0: in front of every plane
    back = lens.ray_trace(zs[::-1], opening_angle=4.0)
    assert same_bits(back["gamma2"], host(seq["gamma2"])[::-1].copy())
    # chi(0.2) = 571.7 lies between planes 2 and 3: the last plane does not matter
    chi_s = lp.flat_lcdm_comoving(0.2, OMEGA_M)
    assert lens.chi[2] < chi_s < lens.chi[3]
    h = math.radians(4.0) / 10
    w = orc.plane_weights(lens.a, OMEGA_M)
    three = rt.trace(lens.planes[:3], lens.chi[:3], w[:3], h, [chi_s])
    assert same_bits(three[0, 0], host(seq["kappa"][2])) and same_bits(three[4, 0], host(seq["alpha1"][2]))
    changed = lens.planes.clone()
    changed[3] += 5.0
    assert same_bits(rt.trace(changed, lens.chi, w, h, [chi_s]), host(three))
    assert same_bits(rt.trace(lens.planes, lens.chi, w, h, [10.0, lens.chi[0]]), np.zeros((6, 2, 10, 10)))


def test_errors(lp):
    lens = box_lens(lp, 2, 8, torch.float32)
    with pytest.raises(ValueError, match="opening angle"):
        lens.ray_trace(1.0)
    with pytest.raises(ValueError, match="pad"):
        lens.ray_trace(1.0, pad=3, opening_angle=4.0)
    with pytest.raises(ValueError, match="opening_angle"):
        lens.ray_trace(1.0, opening_angle=0.0)
    cone = lp.LensPlanes.lightcone(8, 3.5, [100.0, 200.0], OMEGA_M, 1.0, 10, 1.0)
    with pytest.raises(ValueError, match="finish"):
        cone.ray_trace(1.0)
    cone.add(np.array([[0.0, 0.0, 150.0]]), None, (0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="finish"):
        cone.ray_trace(1.0)
    assert tuple(cone.finish().ray_trace(1.0)["kappa"].shape) == (8, 8)


# ------------------------------------------------------------------ dirty memory, a side stream, a late producer
def test_trace_on_dirty_memory_and_behind_a_late_producer(rt):
    """``trace`` writes every byte it reads (state and result are zeroed, psi and the spectrum are filled by the
    transforms), queues everything on the caller's stream and never waits for the device."""
    rng = np.random.default_rng(9)
    planes, decoy = rng.normal(0.0, 40.0, size=(3, 12, 12)), rng.normal(0.0, 40.0, size=(3, 12, 12))
    chi, h, src = np.array([250.0, 610.0, 1400.0]), math.radians(3.0) / 12, [2300.0, 900.0]
    w = orc.plane_weights(1.0 / (1.0 + np.array([0.09, 0.22, 0.55])), OMEGA_M)
    fn = lambda p: rt.trace(p, chi, w, h, src, pad=2)
    want = host(fn(up(planes)))
    assert np.abs(want).max() > 0
    for pattern in dm.PATTERNS:
        with dm.dirty(pattern):
            assert same_bits(fn(up(planes)), want), dm.PATTERN_IDS[pattern]
    assert not same_bits(fn(up(decoy)), want)
    so.late_call(fn, [planes], [decoy])                          # (first launches of the probe's own kernels under S)
    got, armed = so.late_call(fn, [planes], [decoy])
    torch.cuda.synchronize()
    assert armed, "the trace waited for the device: it must only queue work on the caller's stream"
    assert same_bits(got, want), "behind the late producer"


# ------------------------------------------------------------------ many workgroups, second trips, the smallest grids
SENTINEL = -7.0e77                                          # finite, so that == compares it; no result comes near it


def guarded(shape, front=1, behind=4096):
    """A dense float64 view of ``shape`` inside a flat buffer of SENTINEL, ``front`` elements in: with the default front
    it starts 8 bytes off a 16-byte boundary.  Returns the view and the two guards."""
    n = int(np.prod(shape))
    flat = torch.full((front + n + behind,), SENTINEL, dtype=torch.float64, device="cuda")
    view = flat[front:front + n].view(*shape)
    assert view.is_contiguous() and view.data_ptr() == flat.data_ptr() + 8 * front
    return view, (flat[:front], flat[front + n:])


def intact(guards):
    return all(bool((g == SENTINEL).all()) for g in guards)


@pytest.mark.parametrize("born", [False, True], ids=["full", "born"])
@pytest.mark.parametrize("npix,m", cases.GEOMETRY_SHAPES)
def test_every_workgroup_of_the_step_equals_the_oracle(rt, npix, m, born):
    """More than one workgroup along x, partial wavefronts at the x tail, up to 33 rows of workgroups: in every workgroup
    column and row rays land between nodes, on nodes, below 0 and at or beyond m (asserted on the landing positions)."""
    h, chi = cases.H, cases.CHI
    st = cases.geometry_state(npix, m, h, chi[0], chi[1], 200 + npix)
    assert cases.landing_classes(*landing(st, h, chi[0], chi[1]), m) == []
    psi1, psi2 = cases.random_psi(m, h, 300 + m), cases.random_psi(m, h, 301 + m)
    want1 = orc.step(psi1, st, h, chi[0], chi[1], born)
    want2 = orc.step(psi2, want1, h, chi[1], chi[2], born)
    assert np.isfinite(want2).all()
    state = up(st)
    rt.ray_step(up(psi1), state, h, chi[0], chi[1], born)
    assert same_bits(state, want1)
    rt.ray_step(up(psi2), state, h, chi[1], chi[2], born)
    assert same_bits(state, want2)
    assert same_bits(rt.ray_emit(state, chi[2], chi[3]), orc.emit(want2, chi[2], chi[3]))


@pytest.mark.parametrize("born", [False, True], ids=["full", "born"])
@pytest.mark.parametrize("npix,m", [(65, 65), (67, 134)])
def test_step_and_emit_write_nothing_but_their_results(rt, npix, m, born):
    """The state 8 bytes off a 16-byte boundary with a guard element in front and 4096 behind, the maps in the middle
    column of a guarded (6, 3, npix, npix) tensor: the guards and the other columns keep the sentinel's bytes."""
    h, chi = cases.H, cases.CHI
    st = cases.geometry_state(npix, m, h, chi[0], chi[1], 200 + npix)
    psi = cases.random_psi(m, h, 300 + m)
    want = orc.step(psi, st, h, chi[0], chi[1], born)
    state, guards = guarded((12, npix, npix))
    assert state.data_ptr() % 16 == 8
    state.copy_(up(st))
    rt.ray_step(up(psi), state, h, chi[0], chi[1], born)
    assert same_bits(state, want) and intact(guards)
    wide, wide_guards = guarded((6, 3, npix, npix))
    rt.ray_emit(state, chi[1], chi[2], out=wide[:, 1])
    assert same_bits(wide[:, 1].contiguous(), orc.emit(want, chi[1], chi[2]))
    assert bool((wide[:, [0, 2]] == SENTINEL).all()) and intact(wide_guards) and intact(guards)
    assert same_bits(state, want)


def test_the_grid_stride_loops_take_a_second_trip(rt):
    """npix = 768: 589 824 rays, more than the 2048 x 256 work items of one trip of the emit's loop; the step's 12 x 192
    workgroups beside it."""
    npix = m = 768
    h, chi = cases.H, cases.CHI
    assert npix * npix > 2048 * 256
    st = cases.reference_state(npix, m, h, 17)
    psi = cases.random_psi(m, h, 18)
    want = orc.step(psi, st, h, chi[0], chi[1])
    state = up(st)
    rt.ray_step(up(psi), state, h, chi[0], chi[1])
    assert same_bits(state, want)
    maps = orc.emit(want, chi[1], chi[2])
    assert same_bits(rt.ray_emit(state, chi[1], chi[2]), maps)
    wide, guards = guarded((6, 2, npix, npix), front=2)
    rt.ray_emit(state, chi[1], chi[2], out=wide[:, 1])
    assert same_bits(wide[:, 1].contiguous(), maps) and bool((wide[:, 0] == SENTINEL).all()) and intact(guards)


@pytest.mark.parametrize("m", [1100, 1101])
def test_green_multiply_mode_by_mode_beyond_one_trip(rt, hip, m):
    """m (m/2 + 1) > 2048 x 256, so the loop of the multiply goes round again.  A spectrum of 1 - 2i everywhere comes
    back as g (1 - 2i): mode 0 exactly 0, every other mode within max(4 r0, 16 eps) of ``orc.green`` RELATIVELY (the
    high-k modes are 10^6 times smaller than the low ones), r0 being the oracle's own worst relative distance from a
    longdouble evaluation.  Measured: r0 = 1.52e-13 (m = 1100) and 1.28e-13 (1101), at the modes (m - 1, 0), where a / m
    is rounded next to 1 and the sine is pi (1 - a / m); the device, which rounds a / m the same way, is 1.03e-13 and
    9.8e-14 off the oracle (1.09e-13 and 3.0e-14 off the longdouble value); the bounds are 6.1e-13 and 5.1e-13."""
    from tests import ray_trace_reference as ref
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    nh, scale = m // 2 + 1, 0.37
    assert m * nh > 2048 * 256
    want, exact = orc.green(m, scale), ref.green(m, scale)
    nonzero = np.ones((m, nh), dtype=bool)
    nonzero[0, 0] = False
    r0 = float((np.abs(want - exact)[nonzero] / np.abs(exact)[nonzero]).max())
    bound = max(4 * r0, 16 * np.finfo(np.float64).eps)
    flat = torch.full((m * nh + 4096,), SENTINEL, dtype=torch.complex128, device="cuda")
    spec = flat[:m * nh].view(m, nh)
    spec.fill_(complex(1.0, -2.0))
    assert hip.ast_lens_green_multiply(spec.data_ptr(), m, scale, torch.cuda.current_stream().cuda_stream) == 0
    got = host(spec)
    assert got[0, 0] == 0 and bool((flat[m * nh:] == complex(SENTINEL, 0.0)).all())
    assert np.array_equal(got.imag, -2.0 * got.real)
    dev = float((np.abs(got.real - want)[nonzero] / np.abs(want)[nonzero]).max())
    true = float((np.abs(got.real - exact)[nonzero] / np.abs(exact)[nonzero]).max())
    print(f"m {m}: orc.green is {r0:.2e} off longdouble (worst mode, relative); the device {dev:.2e} off orc.green and "
          f"{true:.2e} off longdouble; bound {bound:.2e}")
    assert dev <= bound


@pytest.mark.parametrize("npix,pad", [(1024, 1), (520, 2)])
def test_the_potential_beyond_one_trip_of_the_multiply(rt, npix, pad):
    """``lens_potential`` at m = 1024 and 1040, where ``ast_lens_green_multiply`` loops: the two assertions of
    test_the_device_potential_has_the_laplacian_it_was_solved_for, with its tolerances."""
    rng = np.random.default_rng(40 + npix)
    sigma = rng.normal(0.0, 40.0, size=(npix, npix))
    h = math.radians(3.0) / npix
    m = pad * npix
    assert m * (m // 2 + 1) > 2048 * 256
    psi = host(rt.lens_potential(up(sigma), h, pad, 1.0))
    ref, grid = orc.potential(sigma, h, pad, 1.0)
    err = np.abs(orc.laplacian(psi, h) - 2.0 * (grid - grid.mean())).max() / np.abs(sigma).max()
    print(f"npix {npix} pad {pad}: laplacian identity off by {err:.2e} of max |sigma|")
    assert err <= 1e-12
    assert np.abs(psi - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("born", [False, True], ids=["full", "born"])
def test_the_smallest_grids_equal_the_oracle(rt, born):
    """Every 1 <= npix <= m <= 4, where the 4 x 4 stencil wraps onto itself, with displacements of several m."""
    h = cases.H
    for npix, m in cases.TINY_SHAPES:
        psi, st = cases.random_psi(m, h, 70 + m), cases.tiny_state(npix, m, h, 80 + 4 * m + npix)
        p1, p2 = landing(st, h, 512.0, 1024.0)
        assert p1[0, 0] == 2 * m and p2[0, 0] == -3 * m
        want = orc.step(psi, st, h, 512.0, 1024.0, born)
        state = up(st)
        rt.ray_step(up(psi), state, h, 512.0, 1024.0, born)
        assert same_bits(state, want), (npix, m)
        psi2 = cases.random_psi(m, h, 90 + m)
        want2 = orc.step(psi2, want, h, 1024.0, 1711.3, born)
        rt.ray_step(up(psi2), state, h, 1024.0, 1711.3, born)
        assert same_bits(state, want2), (npix, m)
        assert same_bits(rt.ray_emit(state, 1711.3, 2950.7), orc.emit(want2, 1711.3, 2950.7)), (npix, m)


@pytest.mark.parametrize("npix,pad", [(1, 1), (2, 1), (3, 1), (2, 2), (4, 1), (3, 2)])
def test_the_potential_of_the_smallest_grids(rt, npix, pad):
    """m = 1, 2, 3, 4, 6.  ``ast_fft_plan_create`` takes any length >= 1 and the transforms of one element run: one
    periodic pixel less its mean is 0 everywhere, and so is its potential."""
    rng = np.random.default_rng(60 + npix)
    sigma = rng.normal(0.0, 40.0, size=(npix, npix))
    h, m = math.radians(3.0) / 4, pad * npix
    psi = host(rt.lens_potential(up(sigma), h, pad, 1.0))
    ref, grid = orc.potential(sigma, h, pad, 1.0)
    assert psi.shape == (m, m)
    if m == 1:
        assert ref[0, 0] == 0.0 and psi[0, 0] == 0.0
        return
    assert np.abs(ref).max() > 0
    assert np.abs(orc.laplacian(psi, h) - 2.0 * (grid - grid.mean())).max() <= 1e-12 * np.abs(sigma).max()
    assert np.abs(psi - ref).max() <= 1e-12 * np.abs(ref).max()


def test_layouts_of_the_potential_and_the_planes(rt):
    """psi as a transposed view and 8 bytes into a larger buffer, planes out of a strided stack: the dense call's bytes."""
    npix, m, h, chi = 24, 48, cases.H, cases.CHI
    psi, st = cases.random_psi(m, h, 31), cases.reference_state(npix, m, h, 32)
    want = orc.step(psi, st, h, chi[0], chi[1])
    turned = up(psi.T).t()
    assert not turned.is_contiguous() and same_bits(turned.contiguous(), psi)
    shifted, guards = guarded((m, m))
    shifted.copy_(up(psi))
    assert shifted.data_ptr() % 16 == 8
    for view in (turned, shifted):
        state = up(st)
        rt.ray_step(view, state, h, chi[0], chi[1])
        assert same_bits(state, want)
    assert intact(guards) and same_bits(shifted, psi)
    rng = np.random.default_rng(33)
    stack = up(rng.normal(0.0, 40.0, size=(3, 2 * npix, 2 * npix)))
    planes = stack[:, ::2, ::2]
    assert not planes.is_contiguous() and not planes[1].is_contiguous()
    dist, w = np.array([250.0, 610.0, 1400.0]), orc.plane_weights(1.0 / (1.0 + np.array([0.09, 0.22, 0.55])), OMEGA_M)
    for pad in (1, 2):
        dense = rt.trace(planes.contiguous(), dist, w, h, [2300.0, 900.0], pad=pad)
        assert float(dense.abs().max()) > 0
        assert same_bits(rt.trace(planes, dist, w, h, [2300.0, 900.0], pad=pad), host(dense))


def test_refusals_launch_nothing_and_leave_the_entries_usable(rt, hip):
    """npix = 262141 .. 262144 would need more than 65535 rows of workgroups; h = 1e-170 has h h = 0.  Both are refused by
    the argument checks, which come before any access (the pointers are those of a 16-ray state), and the next valid
    call is the oracle's."""
    from astrild_amd import _lib
    npix, m, h = 4, 8, cases.H
    psi_h, st = cases.random_psi(m, h, 51), cases.tiny_state(npix, m, h, 52)
    want = orc.step(psi_h, st, h, 512.0, 1024.0)
    psi, state = up(psi_h), up(st)
    s = torch.cuda.current_stream().cuda_stream

    def valid_call_still_works():
        again = up(st)
        rt.ray_step(psi, again, h, 512.0, 1024.0)
        assert same_bits(again, want) and same_bits(state, st) and same_bits(psi, psi_h)
    assert rt.NPIX_MAX == 262140
    for big in (262141, 262142, 262143, 262144):
        assert hip.ast_ray_step(psi.data_ptr(), 262144, state.data_ptr(), big, h, 512.0, 1024.0, 0, s) != 0
        assert b"RAY_BY <= 65535" in hip.ast_last_error()
        valid_call_still_works()
    with pytest.raises(ValueError, match="262140"):
        rt.ray_state(262141)
    assert hip.ast_ray_step(psi.data_ptr(), m, state.data_ptr(), npix, 1e-170, 512.0, 1024.0, 0, s) != 0
    assert b"h * h > 0.0" in hip.ast_last_error()
    valid_call_still_works()
    with pytest.raises(_lib.AstrildHipError, match="ast_ray_step"):
        rt.ray_step(psi, state, 1e-170, 512.0, 1024.0)
    valid_call_still_works()
