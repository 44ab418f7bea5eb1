"""CPU: the plane-paint contract restated in numpy (tests/plane_paint_oracle.py) has the properties the design rests on,
the host-only parts of the product agree with it (exponent, factors, weights, argument checks), and the cosmology
helpers meet the errors their docstrings state."""
import math

import numpy as np
import pytest

from tests import plane_paint_oracle as orc

WINDOWS = ("ngp", "cic", "tsc")
L = 64.0
CONE = dict(opening_angle_deg=60.0, chi_edges=(10.0, 60.0, 110.0, 170.0), origin=(31.0, 33.5, -70.0))


def _paint(pos, mass, geometry, P, npix, window, los=2, **kw):
    if geometry == "box":
        return orc.paint(pos, mass, "box", P, npix, window, los, boxsize=L, **kw)
    return orc.paint(pos, mass, "cone", P, npix, window, los, **CONE, **kw)


# ------------------------------------------------------------------ the contract
@pytest.mark.parametrize("window", WINDOWS)
def test_lattice_gives_exactly_zero(window):
    """16^3 unit masses on cell centres into 4 planes of 8^2: every pixel holds the mean, the contrast is 0.0 exactly
    (box side, counts and weights are dyadic, so no operation rounds)."""
    pos = orc.lattice(16, L)
    sums, counters, q = _paint(pos, None, "box", 4, 8, window)
    assert not counters.any() and len(set(sums.reshape(-1).tolist())) == 1
    edges = np.arange(5) * (L / 4)
    mul, add = orc.plane_factors("box", 8, edges, len(pos) / L ** 3, len(pos), 1.0, boxsize=L)
    for dtype in (np.float32, np.float64):
        planes = orc.finish(sums, mul, add, "box", dtype)
        assert planes.dtype == dtype and np.all(planes == 0.0)


@pytest.mark.parametrize("geometry", ["box", "cone"])
@pytest.mark.parametrize("window", WINDOWS)
def test_any_order_and_chunking_give_identical_sums(window, geometry):
    pos, mass = orc.particles(3000, L, seed=1, dtype=np.float32)
    vmax = float(mass.max())
    whole, c0, _ = _paint(pos, mass, geometry, 3, 5, window, vmax=vmax)
    assert whole.any()
    perm = np.random.default_rng(2).permutation(len(pos))
    shuffled, c1, _ = _paint(pos[perm], mass[perm], geometry, 3, 5, window, vmax=vmax)
    assert np.array_equal(whole, shuffled) and np.array_equal(c0, c1)
    sums, counters = np.zeros_like(whole), np.zeros(3, dtype=np.int64)
    kw = dict(boxsize=L) if geometry == "box" else CONE
    for part in np.array_split(np.arange(len(pos)), [7, 1500]):
        orc.accumulate(sums, counters, pos[part], mass[part], geometry, window, 2, len(pos), vmax, **kw)
    assert np.array_equal(whole, sums) and np.array_equal(c0, counters)


@pytest.mark.parametrize("geometry", ["box", "cone"])
@pytest.mark.parametrize("window", WINDOWS)
def test_every_pixel_is_within_half_a_quantum_per_term(window, geometry):
    """One rounding to the quantum per term: |sums - sum of the terms in quanta| <= K / 2 in every pixel (K terms).  The
    term in quanta is the float64 product t * invq, itself within 2^-53 |t invq| <= 2^(k - 53) of the real number.  So the
    planes hold the painted mass to K q (1 / 2 + 2^(k - 53)); in the box, where nothing is dropped and the weights of a
    particle sum to 1 within 4 ulp (and each term carries two more roundings), their total is sum(m) to within that
    and 8 eps sum(m)."""
    pos, mass = orc.particles(2000, L, seed=3)
    sums = np.zeros((3, 5, 5), dtype=np.int64)
    T, K = np.zeros(sums.shape, dtype=np.longdouble), np.zeros(sums.shape, dtype=np.int64)
    kw = dict(boxsize=L) if geometry == "box" else CONE
    invq = orc.accumulate(sums, np.zeros(3, dtype=np.int64), pos, mass, geometry, window, 2, len(pos), float(mass.max()),
                          unrounded=(T, K), **kw)
    assert invq == 2.0 ** 50 / float(mass.max())
    err = np.abs(sums.astype(np.longdouble) - T)
    slack = K * np.finfo(np.longdouble).eps * np.abs(T)                    # (the longdouble sum of K terms)
    print(f"plane paint {geometry} {window}: {K.sum()} terms, max |sums - T| / (K / 2) = {float((err[K > 0] / (K[K > 0] / 2)).max()):.3f}")
    assert K.sum() > 100 and np.all(err <= K / np.longdouble(2) + slack)
    if geometry == "box":
        assert K.sum() == len(pos) * orc.SUPPORT[window] ** 2
        q = np.longdouble(1) / np.longdouble(invq)
        total = float(np.sum(sums.astype(np.longdouble)) * q)
        assert abs(total - mass.sum()) <= K.sum() * float(q) * (0.5 + 2.0 ** (50 - 53)) + 8 * np.finfo(np.float64).eps * mass.sum()


def test_refused_and_outside_particles_are_counted_not_deposited():
    pos, mass = orc.particles(200, L, seed=4)
    base, c, _ = _paint(pos, mass, "box", 2, 5, "cic", vmax=2.0, np_total=300)
    bad_pos = np.concatenate([pos, pos[:6]])
    bad_mass = np.concatenate([mass, [np.nan, np.inf, -np.inf, 2.5, 1.0, 1.0]])
    bad_pos[-2, 0], bad_pos[-1, 2] = np.nan, np.inf
    got, c2, _ = _paint(bad_pos, bad_mass, "box", 2, 5, "cic", vmax=2.0, np_total=300)
    assert np.array_equal(got, base) and c.tolist() == [0, 0, 0] and c2.tolist() == [2, 0, 4]


# ------------------------------------------------------------------ the exponent
ABI_COUNTS = (32, 33, 64, 65, 1000, 1 << 20, (1 << 20) + 1, (1 << 20) + 7, 3 * 2 ** 20 + 5, 1 << 21, 1 << 24, (1 << 30) - 1,
              1 << 30, (1 << 30) + 31, 1 << 31, (1 << 32) - 67, (1 << 32) - 66)


def test_exponent_never_overflows_and_the_library_agrees():
    """Every |term| <= vmax rounds to at most 2^k + 1 quanta, so np_total particles on one pixel stay below 2^63: for the
    particle counts of tests/test_abi.py, their geometric and random fill-ins, and the smallest counts."""
    from astrild_amd import _lib, plane_paint as pp
    lib = _lib.lib()
    counts = set(ABI_COUNTS) | {1, 2, 3, 255, 4095, 4096, 4097}
    counts |= {int(v) for v in np.geomspace(1 << 20, (1 << 32) - 66, 97)}
    counts |= {int(v) for v in np.random.default_rng(5).integers(1 << 20, (1 << 32) - 65, 200)}
    for n in sorted(counts):
        k = orc.exponent(n)
        assert 1 <= k <= 50 and n * (2 ** k + 1) < 2 ** 63, n
        assert k == 50 or 2 * n * (2 ** (k + 1) + 1) >= 2 ** 63, n      # (and not needlessly coarse)
        assert k == pp.plane_exponent(n) == int(lib.ast_plane_paint_exponent(n)), n
    assert int(lib.ast_plane_paint_exponent(0)) == 50
    assert int(lib.ast_plane_paint_exponent(1 << 60)) == -1 and int(lib.ast_plane_paint_exponent((1 << 60) - 1)) == 2


# ------------------------------------------------------------------ the host side of the product
def test_product_factors_and_weights_equal_the_oracle():
    from astrild_amd.rays import lens_planes as lp
    edges = np.array([12.5, 40.0, 77.7, 130.1])
    for geometry, kw in (("box", dict(boxsize=117.6)), ("cone", dict(opening_angle_deg=7.3))):
        got = lp.plane_factors(geometry, 37, edges, 0.37, 1000, 1.9, **kw)
        want = orc.plane_factors(geometry, 37, edges, 0.37, 1000, 1.9, **kw)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    assert lp.D_HUBBLE == orc.D_HUBBLE


def _ok_args(**over):
    kw = dict(geometry="box", pos_shape=(10, 3), pos_dtype=np.float32, mass_shape=(10,), nplanes=3, npix=5, window="cic",
              los=2, np_total=10, vmax=1.0, scale=1.0, shift=-0.5, boxsize=L)
    kw.update(over)
    return kw


def test_check_plane_paint_args_returns_what_the_entry_takes():
    from astrild_amd import plane_paint as pp
    a = pp.check_plane_paint_args(**_ok_args())
    assert (a["cl"], a["c1"], a["c0"]) == orc.box_coefficients(3, 5, L) and a["k"] == 50 and a["e2"] is None
    a = pp.check_plane_paint_args(**_ok_args(geometry="Cone", opening_angle_deg=20.0, chi_edges=[1.0, 2.0, 3.0, 4.5],
                                             origin=(1, 2, 3), window="TSC", np_total=1 << 20))
    assert (a["c1"], a["c0"]) == orc.cone_coefficients(5, 20.0) and a["origin"] == (1.0, 2.0, 3.0) and a["k"] == 41
    assert a["e2"].tolist() == [1.0, 4.0, 9.0, 20.25] and a["window"] == 2 and a["geometry"] == 1


@pytest.mark.parametrize("over, word", [
    (dict(geometry="sphere"), "sphere"), (dict(pos_shape=(10, 2)), "(10, 2)"), (dict(mass_shape=(9,)), "(9,)"),
    (dict(nplanes=0), "nplanes"), (dict(npix=-3), "-3"), (dict(npix=2.5), "2.5"), (dict(npix=(1 << 30) + 1), "allocation"),
    (dict(window="pcs"), "pcs"), (dict(los=3), "los"), (dict(np_total=9), "np_total"), (dict(np_total=1 << 60), "np_total"),
    (dict(vmax=0.0), "vmax"), (dict(vmax=float("nan")), "nan"), (dict(vmax=float("inf")), "inf"),
    (dict(scale=float("inf")), "scale"), (dict(shift=float("nan")), "shift"), (dict(boxsize=0.0), "boxsize"),
    (dict(boxsize=None), "boxsize"), (dict(boxsize="64"), "boxsize"),
    (dict(geometry="cone", opening_angle_deg=180.0, chi_edges=[1, 2, 3, 4]), "180"),
    (dict(geometry="cone", opening_angle_deg=None, chi_edges=[1, 2, 3, 4]), "opening_angle_deg"),
    (dict(geometry="cone", opening_angle_deg=20.0, chi_edges=[1, 2, 3]), "chi_edges"),
    (dict(geometry="cone", opening_angle_deg=20.0, chi_edges=[1, 2, 2, 4]), "ascending"),
    (dict(geometry="cone", opening_angle_deg=20.0, chi_edges=[-1, 2, 3, 4]), "non-negative"),
    (dict(geometry="cone", opening_angle_deg=20.0, chi_edges=[1, 2, 3, float("inf")]), "finite"),
    (dict(geometry="cone", opening_angle_deg=20.0, chi_edges=None), "chi_edges"),
    (dict(geometry="cone", opening_angle_deg=20.0, chi_edges=[1, 2, 3, 4], origin=(0, 0)), "origin"),
    (dict(geometry="cone", opening_angle_deg=20.0, chi_edges=[1, 2, 3, 4], origin=(0, float("nan"), 0)), "origin"),
])
def test_check_plane_paint_args_refuses_with_the_offending_value(over, word):
    from astrild_amd import plane_paint as pp
    with pytest.raises(ValueError) as e:
        pp.check_plane_paint_args(**_ok_args(**over))
    assert word in str(e.value)


def test_check_plane_paint_args_refuses_other_dtypes():
    from astrild_amd import plane_paint as pp
    for dt in (np.float16, np.int32, "complex64"):
        with pytest.raises(TypeError, match="float32 or float64"):
            pp.check_plane_paint_args(**_ok_args(pos_dtype=dt))


# ------------------------------------------------------------------ cosmology
U = 2.0 ** -53
REDSHIFTS = np.array([0.0, 1e-3, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 1100.0])


def test_comoving_distance_einstein_de_sitter_closed_form():
    """flat_lcdm_comoving's docstring: for Omega_m = 1 the rule reproduces the closed form bit for bit (the weighted sum
    of a constant integrand is an integer in any order, and 1536 fl(h / 3) = 512 h exactly)."""
    from astrild_amd.rays import lens_planes as lp
    got = lp.flat_lcdm_comoving(REDSHIFTS, 1.0)
    want = orc.eds_comoving(REDSHIFTS)
    print("chi EdS: max |error| / u chi =", float((np.abs(got - want)[1:] / want[1:]).max() / U))
    assert got[0] == 0.0 and np.array_equal(got, want)
    assert isinstance(lp.flat_lcdm_comoving(1.0, 1.0), float)
    assert lp.flat_lcdm_comoving(1.0, 1.0) == got[4]


#: the largest error over REDSHIFTS that flat_lcdm_comoving's docstring states for 512 intervals, Mpc/h
STATED_CHI_ERROR = {0.1: 9.1e-9, 0.3: 7.5e-9, 0.7: 3.2e-9}


@pytest.mark.parametrize("omega_m", sorted(STATED_CHI_ERROR))
def test_comoving_distance_lcdm_against_another_quadrature(omega_m):
    """The error the docstring states for 512 Simpson intervals, with a margin of 10 and no more, against Gauss-Legendre
    quadrature good to 2e-11 Mpc/h.  256 intervals miss it (16 times the error), and so does a wrong Simpson weight."""
    from astrild_amd.rays import lens_planes as lp
    got = lp.flat_lcdm_comoving(REDSHIFTS, omega_m)
    want = np.array([orc.comoving(z, omega_m) for z in REDSHIFTS])
    one_piece = np.array([orc.comoving(z, omega_m, points=128, parts=1) for z in REDSHIFTS])
    assert np.abs(want - one_piece).max() <= 2e-11
    err = np.abs(got - want).max()
    print(f"chi Omega_m={omega_m}: max |error| = {err:.3g} Mpc/h, stated {STATED_CHI_ERROR[omega_m]:.3g}")
    assert err <= 10 * STATED_CHI_ERROR[omega_m]
    assert lp.SIMPSON_STEPS == 512 and np.all(np.diff(got) > 0)
    half = np.abs(_with_steps(lp, 256, REDSHIFTS, omega_m) - want).max()
    assert half > 10 * STATED_CHI_ERROR[omega_m], "the bound does not tell 512 intervals from 256"


def _with_steps(lp, steps, z, omega_m):
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(lp, "SIMPSON_STEPS", steps)
        return lp.flat_lcdm_comoving(z, omega_m)
    finally:
        mp.undo()


@pytest.mark.parametrize("omega_m", [0.1, 0.3, 1.0])
def test_redshift_round_trip(omega_m):
    """flat_lcdm_redshift's docstring: |z' - z| measured at 2.2 u (1 + z)^(3/2) at most; asserted with a margin of 10."""
    from astrild_amd.rays import lens_planes as lp
    chi = lp.flat_lcdm_comoving(REDSHIFTS, omega_m)
    back = lp.flat_lcdm_redshift(chi, omega_m)
    ratio = np.abs(back - REDSHIFTS) / (U * (1.0 + REDSHIFTS) ** 1.5)
    print(f"z round trip Omega_m={omega_m}: max |dz| / (u (1 + z)^1.5) = {ratio.max():.2f}")
    assert np.all(ratio <= 22.0)
    assert lp.flat_lcdm_redshift(0.0, omega_m) == 0.0
    for bad in (-1.0, 1e9, float("nan")):
        with pytest.raises(ValueError):
            lp.flat_lcdm_redshift(bad, omega_m)
    with pytest.raises(ValueError):
        lp.flat_lcdm_comoving(-0.5, omega_m)
    with pytest.raises(ValueError):
        lp.flat_lcdm_comoving(1.0, 0.0)


# ------------------------------------------------------------------ the units, against physics and not against a copy
def test_mean_pixel_mass_of_the_cone_against_density_times_volume():
    """A pixel of plane p reads D = 0 when it holds q dchi / (mul_p F) of mass, F the finish kernel's factor at its
    centre.  That must be the mean density times the pixel's volume, rho Omega_pix (chi_hi^3 - chi_lo^3) / 3, with the
    solid angle Omega_pix from 16 x 16 Gauss-Legendre points over the pixel; the centre value stands for the pixel mean
    within h^2 / 4 (+ h^4), h the pixel's side in tangent units (test_cone_factor_...).  The box: rho L^3 / (npix^2 P)."""
    from astrild_amd.rays import lens_planes as lp
    npix, angle, rho, np_total, vmax = 24, 17.0, 0.37, 5000, 1.9
    edges = np.array([12.5, 40.0, 77.7, 130.1])
    mul, add = lp.plane_factors("cone", npix, edges, rho, np_total, vmax, opening_angle_deg=angle)
    q = vmax / 2.0 ** orc.exponent(np_total)
    c1, _ = orc.cone_coefficients(npix, angle)
    h = 1.0 / c1
    x, wq = np.polynomial.legendre.leggauss(16)
    t = (((np.arange(npix) + 0.5) - 0.5 * npix) / c1)[:, None] + 0.5 * h * x[None, :]
    w = 1.0 + (t * t)[:, None, :, None] + (t * t)[None, :, None, :]
    omega = np.einsum("abij,i,j->ab", w ** -1.5, wq, wq) * (0.5 * h) ** 2
    assert abs(h * npix - 2 * math.tan(math.radians(angle / 2))) < 1e-15
    assert np.array_equal(add, -(edges[1:] - edges[:-1]))
    for p in range(3):
        implied = q * (edges[p + 1] - edges[p]) / (mul[p] * orc.cone_factor(npix, c1))
        exact = rho * omega * (edges[p + 1] ** 3 - edges[p] ** 3) / 3.0
        assert np.all(np.abs(implied / exact - 1.0) <= h * h / 4 + h ** 4), p
    box, P = 117.6, 3
    mul, add = lp.plane_factors("box", npix, edges, rho, np_total, vmax, boxsize=box)
    dchi = edges[1:] - edges[:-1]
    # (the planes of a box are equally thick: box / P each; the contrast is mass over rho area, minus the thickness)
    assert np.allclose(q / mul, rho * (box / npix) ** 2, rtol=4 * U, atol=0) and np.array_equal(add, -dchi)


def test_uniform_particles_through_a_cone_have_no_mean_contrast():
    """200000 particles uniform in a cuboid around a cone of 20 degrees, NGP (no clipping at the map's edges): the mean of
    D_p / dchi_p over a plane is the Poisson fluctuation of its count N_p, within 5 / sqrt(N_p) - against the density
    the particles were drawn with, through accumulate, the cos^-3 factor and the product's factors."""
    from astrild_amd.rays import lens_planes as lp
    rng = np.random.default_rng(7)
    n, npix, angle = 200000, 16, 20.0
    edges = np.array([60.0, 100.0, 150.0])
    half = 150.0 * math.tan(math.radians(angle / 2)) * 1.5
    pos = np.stack([rng.uniform(-half, half, n), rng.uniform(-half, half, n), rng.uniform(0.0, 150.0, n)], axis=1)
    rho = n / (4 * half * half * 150.0)
    sums, counters, _ = orc.paint(pos, None, "cone", 2, npix, "ngp", 2, opening_angle_deg=angle, chi_edges=edges)
    mul, add = lp.plane_factors("cone", npix, edges, rho, n, 1.0, opening_angle_deg=angle)
    planes = orc.finish(sums, mul, add, "cone", np.float64, orc.cone_coefficients(npix, angle)[0])
    for p in range(2):
        count = int(sums[p].sum() >> orc.exponent(n))
        mean = float(planes[p].mean() / (edges[p + 1] - edges[p]))
        print(f"uniform cone plane {p}: {count} particles, mean contrast {mean:+.4f}, 1 / sqrt(N) = {count ** -0.5:.4f}")
        assert count > 2000 and abs(mean) <= 5.0 / math.sqrt(count)


def test_born_weights_against_the_constants_and_a_uniform_slab():
    """W_p = 3/2 Omega_m (H_0 / c)^2 g / a with H_0 = 100 h km/s/Mpc and c = 299792.458 km/s; 0 from chi_p >= chi_s on.
    And the sum: kappa of a uniform contrast delta = 1 out to the source is int W dchi, in Einstein-de Sitter with
    a = (1 - chi / 2 D_H)^2 an integrand f known in closed form.  400 planes are the midpoint rule on it: off by at
    most chi_s h^2 / 24 max |f''| from the 64-point Gauss-Legendre value."""
    from astrild_amd.rays import lens_planes as lp
    chi = np.array([100.0, 800.0, 1500.0, 2000.0])
    a = np.array([0.9, 0.6, 0.5, 0.4])
    wnum, wden = lp.born_weights(chi, a, 1500.0, 0.31)
    want = 1.5 * 0.31 * (100.0 / 299792.458) ** 2 * (1500.0 - chi) * chi / 1500.0 / a
    assert np.allclose((wnum / wden)[:2], want[:2], rtol=8 * U, atol=0) and wnum[2] == 0.0 and wnum[3] == 0.0
    assert np.array_equal(wden, a)
    chi_s, P = lp.flat_lcdm_comoving(1.0, 1.0), 400
    edges = np.linspace(0.0, chi_s, P + 1)
    mid = 0.5 * (edges[:-1] + edges[1:])
    scale = lambda c: (1.0 - c / (2.0 * lp.D_HUBBLE)) ** 2
    wnum, wden = lp.born_weights(mid, scale(mid), chi_s, 1.0)
    kappa = float(np.sum(wnum / wden * np.diff(edges)))
    f = lambda c: 1.5 * (1.0 / lp.D_HUBBLE) ** 2 * (chi_s - c) * c / chi_s / scale(c)
    x, wq = np.polynomial.legendre.leggauss(64)
    exact = 0.5 * chi_s * float(np.sum(wq * f(0.5 * chi_s * (1.0 + x))))
    dense = np.linspace(0.0, chi_s, 20001)
    f2 = np.abs(np.gradient(np.gradient(f(dense), dense), dense))[2:-2].max()
    bound = chi_s * (chi_s / P) ** 2 / 24 * f2 * 1.01
    print(f"uniform slab to z = 1: kappa = {kappa:.6f}, exact {exact:.6f}, |difference| / bound = {abs(kappa - exact) / bound:.3f}")
    assert 0.05 < exact < 0.5 and abs(kappa - exact) <= bound and bound < 1e-4 * exact


# ------------------------------------------------------------------ the cone's cos^-3
def test_cone_factor_against_the_exact_solid_angle_of_a_pixel():
    """A gnomonic pixel of side h in the tangent plane subtends int dta dtb (1 + ta^2 + tb^2)^-3/2; the finish kernel
    multiplies by w^3/2 at the pixel centre.  Midpoint rule on g = w^-3/2: the relative error is (h^2 / 24) |g_aa + g_bb|
    / g + O(h^4) with (g_aa + g_bb) / g = (9 - 15 / w) / w in [-6, 9/4], so at most h^2 / 4 (+ h^4).  The exact value: 16 x 16
    Gauss-Legendre points per pixel."""
    npix, angle = 64, 20.0
    c1, _ = orc.cone_coefficients(npix, angle)
    h = 1.0 / c1
    factor = orc.cone_factor(npix, c1)
    x, wq = np.polynomial.legendre.leggauss(16)
    centres = ((np.arange(npix) + 0.5) - 0.5 * npix) / c1
    t = centres[:, None] + 0.5 * h * x[None, :]                              # (npix, 16)
    w = 1.0 + (t * t)[:, None, :, None] + (t * t)[None, :, None, :]          # (npix, npix, 16, 16)
    omega = np.einsum("abij,i,j->ab", w ** -1.5, wq, wq) * (0.5 * h) ** 2
    ratio = factor * omega / (h * h)
    print(f"cone factor: max |factor x solid angle / area - 1| = {np.abs(ratio - 1).max():.3g}, h^2 / 4 = {h * h / 4:.3g}")
    assert np.all(np.abs(ratio - 1.0) <= h * h / 4 + h ** 4)
    # (the whole map: a square pyramid of apex angle theta subtends 4 asin(sin^2(theta / 2)))
    assert abs(omega.sum() - 4 * math.asin(math.sin(math.radians(angle) / 2) ** 2)) <= 1e-12
    # without the factor a uniform cone reads 4.5 % low 10 degrees off axis
    edge = orc.cone_factor(npix, c1)[npix // 2, -1]
    assert abs(1.0 / edge - math.cos(math.radians(10.0 - 10.0 / npix)) ** 3) < 2e-3 and 0.04 < 1.0 - 1.0 / edge < 0.05
