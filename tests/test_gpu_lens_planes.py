"""GPU: ``rays.LensPlanes`` - lens planes in physical units from a box and from a light cone, Born convergence over the
resident planes, the hand-over to ``SkyArray`` - against tests/plane_paint_oracle.py.  The planes are compared
``tobytes()``; the convergence by the rule tests/test_gpu_kappa.py holds ``kappa_stack`` to (``np.array_equal`` with the
plane-order sum in the planes' dtype), with weights restated in the oracle from the product's distances, which
tests/test_plane_paint_oracle.py checks on their own."""
import math

import numpy as np
import pytest

from tests import plane_paint_oracle as orc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

OMEGA_M = 0.3
DTYPES = {"f32": np.float32, "f64": np.float64}


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def lp(hip):
    from astrild_amd.rays import lens_planes
    return lens_planes


def same_bits(got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def oracle_kappa(lp, planes, lens, z):
    wnum, wden = orc.source_weights(lens.chi, lens.a, lp.flat_lcdm_comoving(z, OMEGA_M), OMEGA_M)
    return orc.stack(planes, wnum, wden), wnum


def test_exported():
    from astrild_amd.rays import LensPlanes
    from astrild_amd.rays.lens_planes import LensPlanes as same
    assert LensPlanes is same


@pytest.mark.parametrize("window", ["ngp", "cic", "tsc"])
def test_lattice_box_has_no_contrast_and_no_convergence(lp, window):
    """16^3 unit masses on cell centres of a box of 64 Mpc/h, 4 planes of 8^2, the default mean density (sum m / L^3):
    every operation is exact, planes and kappa are 0.0."""
    box = 64.0
    pos = orc.lattice(16, box).astype(np.float32)
    for mass in (None, np.full(len(pos), 0.25, dtype=np.float32)):
        lens = lp.LensPlanes.from_box(pos, mass, box, 4, 8, OMEGA_M, chi0=512.0, window=window)
        assert tuple(lens.planes.shape) == (4, 8, 8) and lens.planes.dtype == torch.float32 and lens.planes.is_cuda
        assert lens.counters.tolist() == [0, 0, 0] and int(lens.sums.min()) == int(lens.sums.max()) > 0
        assert bool(torch.all(lens.planes == 0.0))
        kappa = lens.convergence([0.3, 1.0])
        assert tuple(kappa.shape) == (2, 8, 8) and bool(torch.all(kappa == 0.0))
        assert lens.chi.tolist() == [520.0, 536.0, 552.0, 568.0] and np.all((0 < lens.a) & (lens.a < 1)) and np.all(np.diff(lens.a) < 0)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("window", ["ngp", "cic", "tsc"])
def test_box_planes_and_convergence_equal_the_oracle(lp, window, dt):
    box, P, npix, chi0 = 100.0, 3, 5, 500.0
    pos, mass = orc.particles(1000, box, 41, np.float32)
    rho = float(mass.astype(np.float64).sum()) / box ** 3
    vmax = float(mass.max())
    for los in (0, 2):
        lens = lp.LensPlanes.from_box(pos, mass, box, P, npix, OMEGA_M, chi0=chi0, los=los, window=window,
                                      dtype=getattr(torch, DTYPES[dt].__name__), mean_density=rho)
        sums, counters, _ = orc.paint(pos, mass, "box", P, npix, window, los, vmax=vmax, boxsize=box)
        edges = chi0 + np.arange(P + 1) * (box / P)
        mul, add = orc.plane_factors("box", npix, edges, rho, len(pos), vmax, boxsize=box)
        want = orc.finish(sums, mul, add, "box", DTYPES[dt])
        assert same_bits(lens.sums, sums) and same_bits(lens.counters, counters)
        assert same_bits(lens.planes, want), los
        assert abs(float(want.astype(np.float64).mean())) < 1e-4                       # (all the mass is in: mean contrast 0)
        assert np.array_equal(lens.chi, 0.5 * (edges[:-1] + edges[1:]))
        # z = 0.2 lies inside the plane range (chi = 571.7): the last plane weighs 0
        zs = (0.2, 1.0, 2.0)
        kappas = lens.convergence(zs)
        for s, z in enumerate(zs):
            ref, wnum = oracle_kappa(lp, want, lens, z)
            assert (wnum[-1] == 0.0) == (z == 0.2) and np.all(wnum[:-1] > 0)
            assert np.array_equal(kappas[s].cpu().numpy(), ref), (los, z)
            assert np.array_equal(lens.convergence(z).cpu().numpy(), ref), (los, z, "scalar")
        assert lens.convergence(0.0).abs().max() == 0.0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("window", ["ngp", "cic", "tsc"])
def test_lightcone_planes_and_convergence_equal_the_oracle(lp, window, dt):
    """1000 particles of a box of 100 Mpc/h, seen from 300 Mpc/h in front of it and replicated once behind itself, added
    in two chunks per replica."""
    box, npix, angle = 100.0, 8, 30.0
    pos, mass = orc.particles(1000, box, 42, np.float64)
    edges = np.array([280.0, 345.5, 410.1, 520.0])
    observer = (47.0, 52.5, -300.0)
    rho, vmax, np_total = 1000 * 1.25 / (3 * box) ** 3, 2.0, 2000
    lens = lp.LensPlanes.lightcone(npix, angle, edges, OMEGA_M, rho, np_total, vmax, window=window,
                                   dtype=getattr(torch, DTYPES[dt].__name__))
    sums, counters = np.zeros((3, npix, npix), dtype=np.int64), np.zeros(3, dtype=np.int64)
    for offset in ((0.0, 0.0, 0.0), (0.0, 0.0, 3 * box)):
        origin = tuple(o - s for o, s in zip(observer, offset))
        for part in (slice(0, 400), slice(400, 1000)):
            assert lens.add(pos[part], mass[part], observer, offset) is lens
            orc.accumulate(sums, counters, pos[part], mass[part], "cone", window, 2, np_total, vmax, opening_angle_deg=angle,
                           chi_edges=edges, origin=origin)
    with pytest.raises(ValueError, match="finish"):
        lens.convergence(1.0)
    assert lens.finish() is lens
    mul, add = orc.plane_factors("cone", npix, edges, rho, np_total, vmax, opening_angle_deg=angle)
    c1, _ = orc.cone_coefficients(npix, angle)
    want = orc.finish(sums, mul, add, "cone", DTYPES[dt], c1)
    assert np.count_nonzero(sums) > 20 and counters[0] > 0
    assert same_bits(lens.sums, sums) and same_bits(lens.counters, counters)
    assert same_bits(lens.planes, want)
    zs = [0.14, 0.5, 1.5]                                           # chi(0.14) = 407: inside, the last plane weighs 0
    kappas = lens.convergence(zs)
    for s, z in enumerate(zs):
        ref, wnum = oracle_kappa(lp, want, lens, z)
        assert (wnum[-1] == 0.0) == (z == 0.14) and wnum[0] > 0
        assert np.array_equal(kappas[s].cpu().numpy(), ref), z


def test_sky_array_holds_a_device_map(lp):
    box, npix = 100.0, 64
    pos, mass = orc.particles(20000, box, 43, np.float32)
    lens = lp.LensPlanes.from_box(pos, mass, box, 2, npix, OMEGA_M, chi0=400.0)
    with pytest.raises(ValueError, match="opening angle"):
        lens.sky_array(1.0)
    sky = lens.sky_array(1.0, opening_angle=5.0)
    assert sky.quantity == "kappa_2" and sky.npix == npix and sky.opening_angle == 5.0
    assert sky.data.resident("orig")
    kappa = lens.convergence(1.0)
    pdf = sky.pdf(20)
    assert len(pdf["values"]) == 20 and np.isfinite(pdf["values"]).all()
    assert math.isclose(pdf["bins"][0], float(kappa.min()), rel_tol=1e-12) and math.isclose(pdf["bins"][-1], float(kappa.max()), rel_tol=1e-12)
    sky.filter({"gaussian": {"theta_i": 10.0, "abbrev": "gauss"}}, on="orig")
    assert sky.data.resident("orig_gauss") and sky.data.resident("orig")
    smooth = sky.data["orig_gauss"]
    assert smooth.shape == (npix, npix) and np.isfinite(smooth).all() and smooth.std() < float(kappa.std())
    assert np.array_equal(sky.data["orig"], kappa.cpu().numpy())
    cone = lp.LensPlanes.lightcone(8, 3.5, [100.0, 200.0], OMEGA_M, 1.0, 10, 1.0).finish()
    assert cone.sky_array(0.5).opening_angle == 3.5


@pytest.mark.parametrize("window", ["ngp", "cic"])
def test_one_particle_cone_stamps_the_predicted_pixel(lp, window):
    """One particle 2.1 degrees off axis along a and -1.3 degrees along b at 300 Mpc/h: the only pixel above the floor
    -W dchi is the one its tangents fall into (NGP), or the four around it (CIC), the heaviest the predicted one."""
    npix, angle, chi = 16, 8.0, 300.0
    ta, tb = math.tan(math.radians(2.1)), math.tan(math.radians(-1.3))
    dl = chi / math.sqrt(1.0 + ta * ta + tb * tb)
    observer = (10.0, -20.0, 5.0)
    for los in (0, 1, 2):
        a, b = [c for c in range(3) if c != los]
        pos = np.zeros((1, 3))
        pos[0, a], pos[0, b], pos[0, los] = observer[a] + ta * dl, observer[b] + tb * dl, observer[los] + dl
        lens = lp.LensPlanes.lightcone(npix, angle, [250.0, 350.0], OMEGA_M, 1e-6, 1, 1.0, window=window, dtype=torch.float64)
        lens.add(pos, None, observer, los=los).finish()
        kappa = lens.convergence(1.0).cpu().numpy()
        c1 = npix / (2.0 * math.tan(math.radians(angle / 2)))
        ia, ib = int(math.floor(npix / 2 + ta * c1)), int(math.floor(npix / 2 + tb * c1))
        assert (ia, ib) == (12, 5)
        assert np.unravel_index(np.argmax(kappa), kappa.shape) == (ia, ib), los
        wnum, wden = orc.source_weights(lens.chi, lens.a, lp.flat_lcdm_comoving(1.0, OMEGA_M), OMEGA_M)
        floor = -100.0 * wnum[0] / wden[0]
        above = np.argwhere(kappa > 0.5 * floor)
        assert kappa[ia, ib] > 0 and len(above) == (1 if window == "ngp" else 4)
        assert np.all(np.abs(above - np.array([ia, ib])).max(axis=1) <= 1)
        assert np.allclose(np.delete(kappa.reshape(-1), [r * npix + c for r, c in above]), floor, rtol=1e-12, atol=0)
        assert lens.counters.tolist() == [0, 0, 0]
