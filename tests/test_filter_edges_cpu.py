"""No GPU: every case of tests/filter_edges.py, on the CPU.  The unmutated reference stays within the case's own bound
of the op-by-op numpy model of the kernel, and at least one wrong kernel ("mutation") leaves the bound at some pixel -
at a border pixel where the mutation is one of the border.  A case that no mutation can tell apart says why, and the
test asserts that too."""
import numpy as np
import pytest

from tests import filter_edges as fe


def _within(model, ref, bound):
    bad = fe.exceeds(model, ref, bound)
    assert not bad.any(), (int(bad.sum()), fe.worst_ratio(model, ref, bound))


# ------------------------------------------------------------------------------------------------ ast_convolve2d
def _convolve_case(img, w, exact=False):
    ref = fe.convolve_reference(img, w)
    model = fe.convolve_model(img, w)
    if exact:
        assert np.array_equal(model, ref)
    _within(model, ref, fe.convolve_bound(img, w))
    # the index formulas of the kernel's comment add scipy's products in scipy's order
    assert np.array_equal(model, ref)
    bound = fe.convolve_bound(img, w)
    told = [m for m in fe.CONVOLVE_MUTATIONS if fe.exceeds(fe.CONVOLVE_MUTATIONS[m](img, w), ref, bound).any()]
    return ref, told


def test_convolve_impulses_are_exact_and_discriminate():
    cases = fe.convolve_impulse_cases()
    # 15, 16: the two corners ((15, 15) is the last pixel of 16); 17: five, (16, 16) being its last pixel; 33: all six
    assert len(cases) == 4 * (2 + 2 + 5 + 6)
    for name, img, w in cases:
        ref, told = _convolve_case(img, w, exact=True)
        i, j = np.argwhere(img)[0]
        if min(i, j, img.shape[0] - 1 - i, img.shape[0] - 1 - j) >= 8:
            assert ref.sum() == w.sum(), name           # away from the border the whole window lands on the map
        assert np.array_equal(ref, np.round(ref)), name
        # an impulse shows the flip always, the shift for an even extent; "mirror" only next to the border
        assert "no_flip" in told and "no_origin_shift" in told, (name, told)


def test_convolve_lds_limit_cases():
    for kh, kw, staged in fe.LDS_WINDOWS:
        assert ((15 + kh) * (15 + kw) * 8 <= fe.LDS_LIMIT_BYTES) == staged
    assert (15 + 49) * (15 + 113) * 8 == fe.LDS_LIMIT_BYTES
    for name, img, w, staged in fe.convolve_lds_cases():
        _, told = _convolve_case(img, w)
        assert set(told) == set(fe.convolve_discriminators(img, w)), (name, told)
        assert ("no_origin_shift" in told) == (name.endswith(("50x113", "49x114"))), name


def test_convolve_multi_lap_cases():
    for name, img, w in fe.convolve_lap_cases():
        ref, told = _convolve_case(img, w)
        assert set(told) == set(fe.convolve_discriminators(img, w)), (name, told)
        if img.shape[0] == 1:                           # one pixel: img[0, 0] * sum(w) under every extension
            assert not told
            for mutate in fe.CONVOLVE_MUTATIONS.values():
                assert abs(mutate(img, w)[0, 0] - ref[0, 0]) <= fe.convolve_bound(img, w)[0, 0]
        else:
            assert told, name
    # really more than one lap: windows wider than twice the map, at every map size
    assert all(any(max(w.shape) > 2 * img.shape[0] for _, img, w in fe.convolve_lap_cases() if img.shape[0] == n)
               for n in (1, 2, 5, 7))


# ------------------------------------------------------------------------------------- ast_gaussian_filter_order
def test_host_taps_have_the_parity_of_their_order_exactly():
    """The general path of NI_Correlate1D is unreachable: the library's taps are symmetric for an even order and
    antisymmetric for an odd one to the last bit, over the case list and over sigma 0.126 .. 30."""
    sigmas = list(fe.GAUSS_SIGMAS) + [0.126 * (30.0 / 0.126) ** (i / 60.0) for i in range(61)]
    for sigma in sigmas:
        r = fe.gauss_radius(sigma)
        for order in range(9):
            w = fe.host_taps(sigma, order, r)
            assert np.all(np.isfinite(w))
            assert np.array_equal(w[::-1], -w if order & 1 else w), (sigma, order)
            if order & 1:
                assert w[r] == 0.0


def test_host_taps_agree_with_scipy_within_the_measured_tau():
    worst_tau, worst_host = 0.0, 0.0
    for sigma in fe.GAUSS_SIGMAS:
        r = fe.gauss_radius(sigma)
        for order in range(9):
            tau = fe.tap_tau(sigma, order)
            exact = fe.exact_taps(sigma, order, r)
            top = float(np.abs(exact).max())
            host = fe.host_taps(sigma, order, r)
            if top == 0.0:
                assert tau == 0.0 and not host.any()
                continue
            off = float(np.abs(host.astype(np.longdouble) - exact).max() / top)
            assert off <= 4.0 * tau, (sigma, order, off, tau)          # the allowance of gaussian_bound
            worst_tau, worst_host = max(worst_tau, tau), max(worst_host, off)
    assert worst_tau < 4e-15 and worst_host < 4e-15     # (sanity: a few ulp of the largest tap)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("npix", fe.GAUSS_NPIX)
def test_gaussian_cases(npix, mode):
    img = fe.gauss_image(npix)
    for sigma in fe.GAUSS_SIGMAS:
        r = fe.gauss_radius(sigma)
        for o0, o1 in fe.GAUSS_ORDERS:
            ref = fe.gaussian_reference(img, sigma, o0, o1, mode)
            bound = fe.gaussian_bound(img, sigma, o0, o1, mode)
            _within(fe.gaussian_model(img, sigma, o0, o1, mode), ref, bound)
            wrong = fe.gaussian_mutation(npix, sigma, mode)
            if wrong is None:
                for other in ("reflect", "nearest", "mirror"):      # one pixel or one tap: no boundary is read
                    _within(fe.gaussian_reference(img, sigma, o0, o1, other), ref, bound)
                continue
            bad = fe.exceeds(fe.gaussian_reference(img, sigma, o0, o1, wrong), ref, bound)
            assert bad.any(), (npix, sigma, o0, o1, mode, wrong)
            di, dj = fe.border_distance(npix)
            # (order 0 along an axis still filters along it: both axes read across the border)
            assert np.all((np.minimum(di, dj) < r)[bad]), (npix, sigma, o0, o1)


@pytest.mark.parametrize("npix", fe.GAUSS_NPIX)
def test_gaussian_constant_image_nearest(npix):
    """A constant image in mode "nearest": an odd order along either axis gives exactly zero (the antisymmetric path
    subtracts equal pixels); an even derivative order gives c sum(w0) sum(w1), which is NOT rounding - the taps of an even
    derivative of a Gaussian cut at 4 sigma do not sum to zero (order 2, sigma 1.3: -1.8e-4 against taps of 0.18) - and
    is within the bound of scipy's value."""
    img = np.full((npix, npix), 2.75)
    for sigma in fe.GAUSS_SIGMAS:
        for o0, o1 in fe.GAUSS_ORDERS:
            got = fe.gaussian_model(img, sigma, o0, o1, 1)
            bound = fe.gaussian_bound(img, sigma, o0, o1, 1)
            if (o0 | o1) & 1:
                assert not got.any()
                assert np.all(np.abs(fe.gaussian_reference(img, sigma, o0, o1, 1)) <= bound)
            else:
                _within(got, fe.gaussian_reference(img, sigma, o0, o1, 1), bound)
    r = fe.gauss_radius(1.3)
    assert abs(fe.host_taps(1.3, 2, r).sum()) > 1e-4


def test_gaussian_work_doubles():
    assert fe.gauss_work_doubles(17, 5.0) == 289 + 2 * 41 and fe.gauss_work_doubles(1, 0.1) == 3
    assert [fe.gauss_radius(s) for s in fe.GAUSS_SIGMAS] == [0, 0, 1, 1, 5, 20]


# ------------------------------------------------------------------------------------------------ ast_dgd_filter
@pytest.mark.parametrize("npix", fe.DGD_NPIX)
def test_dgd_cases(npix):
    ones, rand = np.ones((npix, npix)), fe.dgd_image(npix)
    di, dj = fe.border_distance(npix)
    zero_border = 0
    for sigma, h, axis, order in fe.dgd_params(npix):
        for img in (ones, rand):
            ref = fe.dgd_reference(img, sigma, h, axis, order)
            bound = fe.dgd_bound(img, sigma, h, axis, order)
            assert np.all(np.isfinite(ref))
            _within(fe.dgd_model(img, sigma, h, axis, order), ref, bound)
            bad = fe.exceeds(fe.dgd_reference(img, sigma, h, axis, order, edge_order=1), ref, bound)
            if fe.dgd_window_border_is_zero(npix, sigma, order):
                zero_border += 1
                assert not bad.any()
                edge = (di if axis == 0 else dj) == 0
                assert not ref[edge].any()              # exactly zero, not NaN
                continue
            if npix == 3 and order == 3:
                # three points: either end stencil makes the first derivative linear in the index and the second one
                # constant, so the third is zero but for rounding under both - nothing to tell apart, and nothing but
                # rounding to compare
                assert not bad.any() and np.all(np.abs(ref) <= bound)
                continue
            assert bad.any(), (npix, sigma, h, axis, order)
            # a wrong end stencil is wrong in the first and last `order` rows (columns) along the axis, nowhere else
            assert np.all(((di if axis == 0 else dj) < order)[bad])
            assert bad[(di if axis == 0 else dj) == 0].any()
    assert zero_border == (8 if npix == 64 else 0)      # sigma_pix 1, order 1: 2 h x 2 axes x 2 images


def test_dgd_smallest_map_reads_all_three_points():
    """npix = 3: both one-sided stencils read the whole line, and idx + step in place of idx + 2 step is told apart."""
    img = np.ones((3, 3))
    for sigma, h, axis, order in fe.dgd_params(3):
        w = fe.dgd_window(3, sigma, order)
        f = np.moveaxis(w, axis, 0)
        wrong = np.moveaxis(np.stack([(-1.5 / h) * f[0] + (2.0 / h) * f[1] + (-0.5 / h) * f[1],
                                      (f[2] - f[0]) / (2.0 * h),
                                      (0.5 / h) * f[1] + (-2.0 / h) * f[1] + (1.5 / h) * f[2]]), 0, axis)
        if order == 1:
            assert fe.exceeds(wrong, fe.dgd_reference(img, sigma, h, axis, 1), fe.dgd_bound(img, sigma, h, axis, 1)).any()


# --------------------------------------------------------------------------------------- ast_aperture_photometry
def test_ring_counts():
    assert np.sqrt(50.0) == 5.0 * np.sqrt(2.0)          # the outer-edge pixels of (31, 5) are truly on the edge
    for (npix, alpha), counts in fe.RING_COUNTS.items():
        strict = int(fe.ring_mask(npix, float(alpha)).sum())
        closed = int(fe.ring_mask(npix, float(alpha), True, True).sum())
        assert (strict, closed) == counts, (npix, alpha, strict, closed)
    inner = fe.ring_mask(31, 5.0, True, False).sum() - 68
    outer = fe.ring_mask(31, 5.0, False, True).sum() - 68
    assert (inner, outer) == (12, 12)
    assert fe.RING_COUNTS[(513, 100)][0] < fe.RING_COUNTS[(513, 100)][1] and 513 * 513 > fe.RING_THREADS


@pytest.mark.parametrize("npix,alpha", list(fe.RING_COUNTS))
def test_aperture_cases(npix, alpha):
    img = fe.aperture_image(npix)
    ref = fe.aperture_reference(img, alpha)
    bound = fe.aperture_bound(img, alpha)
    model = fe.aperture_model(img, alpha)
    strict, closed = fe.RING_COUNTS[(npix, alpha)]
    if strict == 0:
        assert np.isnan(ref).all() and np.isnan(model).all()
    else:
        _within(model, ref, bound)
    told = [fe.exceeds(fe.aperture_reference(img, alpha, *m), ref, bound).any()
            for m in ((True, False), (False, True), (True, True))]
    assert any(told) == (closed > strict)               # an empty ring that stays empty when closed tells nothing apart
    if alpha == 0:                                      # d = 0 = alpha = alpha sqrt 2: only closing both sides lets it in
        assert told == [False, False, True]
    if (npix, alpha) in ((31, 5), (301, 61), (513, 100)):
        assert all(told)


# ----------------------------------------------------------------------------------------------- ast_hann_apodize
@pytest.mark.parametrize("npix", fe.HANN_NPIX)
def test_hann_cases(npix):
    img = fe.hann_image(npix)
    ref, model = fe.hann_reference(img), fe.hann_model(img)
    _within(model, ref, fe.hann_bound(img))
    if npix == 1:
        assert np.array_equal(ref, img) and np.array_equal(model, img)
    if npix in (2, 3):
        di, dj = fe.border_distance(npix)
        edge = np.minimum(di, dj) == 0
        assert np.all(np.abs(model[edge]) <= 4.0 * fe.U * np.abs(img[edge]))
        assert np.all(np.abs(ref[edge]) <= 4.0 * fe.U * np.abs(img[edge]))
    if npix == 3:
        assert model[1, 1] == img[1, 1] and ref[1, 1] == img[1, 1]
    if npix > 1:                                        # the periodic window (sym=False) is the wrong one
        from scipy.signal.windows import hann
        h = hann(npix, sym=False)
        assert fe.exceeds(img * np.outer(h, h), ref, fe.hann_bound(img)).any()


# ------------------------------------------------------------------------------------------------ ast_zoom_linear
@pytest.mark.parametrize("nin,nout", fe.ZOOM_SHAPES)
def test_zoom_cases(nin, nout):
    img = fe.zoom_image(nin, nout)
    ref, model = fe.zoom_reference(img, nout), fe.zoom_model(img, nout)
    assert ref.shape == (nout, nout)
    bound = fe.zoom_bound(img, nout)
    _within(model, ref, bound)
    exact = fe.zoom_exact(img, nout)
    if exact is not None:
        assert np.array_equal(model, exact) and np.array_equal(ref, exact)
    corners = fe.zoom_reference(img, nout, grid_mode=False)
    if nout == nin:                                     # zoom factor 1: corners and centres coincide
        assert np.array_equal(corners, ref)
    else:
        assert fe.exceeds(corners, ref, bound).any()
