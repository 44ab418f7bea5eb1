"""GPU: the seven entry points of astrild_amd/csrc/filters.hip at their edges, called through the C ABI directly so that
no Python wrapper filters the shapes, against the references and the elementwise bounds of tests/filter_edges.py.
Every test prints its worst err / bound.  Every refused argument set is refused by a host-side argument check before
any launch, and is followed by a valid call."""
import numpy as np
import pytest

from oracle import kappa as ok
from tests import filter_edges as fe

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


def _abi():
    from astrild_amd import _lib
    from astrild_amd.device import as_device, ptr, stream
    return _lib, as_device, ptr, stream


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float64, device="cuda")


def _refused(rc):
    _lib = _abi()[0]
    assert rc != 0
    assert b"bad argument" in _lib.lib().ast_last_error()


def _report(what, ratio):
    print(f"{what}: max err / bound = {ratio:.3g}")
    return ratio


def _check(got, ref, bound, what=""):
    bad = fe.exceeds(got, ref, bound)
    assert not bad.any(), (what, int(bad.sum()), fe.worst_ratio(got, ref, bound))
    return fe.worst_ratio(got, ref, bound)


# ------------------------------------------------------------------------------------------------ ast_convolve2d
def _convolve(img, w, pad=0):
    """out sits `pad` doubles inside a NaN-filled allocation; returns (out, the pads)."""
    _lib, as_device, ptr, stream = _abi()
    n = img.shape[0]
    t, wd = as_device(img), as_device(w)
    buf = _nan(n * n + 2 * pad)
    out = buf[pad:pad + n * n]
    _lib.check(_lib.lib().ast_convolve2d(ptr(t), ptr(wd), ptr(out), n, w.shape[0], w.shape[1], stream()), "ast_convolve2d")
    host = buf.cpu().numpy()
    return host[pad:pad + n * n].reshape(n, n), np.concatenate([host[:pad], host[pad + n * n:]])


def test_convolve2d_impulses_exact():
    """A single 1.0 at a corner or around the 16-pixel tile boundary, windows of distinct integers with odd and even
    extents: the output is the reflected, flipped placement of the window, exactly."""
    for name, img, w in fe.convolve_impulse_cases():
        got, _ = _convolve(img, w)
        assert np.array_equal(got, fe.convolve_reference(img, w)), name
    _report("ast_convolve2d[impulse]", 0.0)


def test_convolve2d_at_the_lds_limit():
    """49 x 113 and 113 x 49 are staged in LDS (exactly 65536 bytes), 50 x 113 and 49 x 114 read global memory."""
    worst = 0.0
    for name, img, w, _staged in fe.convolve_lds_cases():
        got, _ = _convolve(img, w)
        worst = max(worst, _check(got, fe.convolve_reference(img, w), fe.convolve_bound(img, w), name))
    _report("ast_convolve2d[lds limit]", worst)


def test_convolve2d_multi_lap_reflection_and_pads():
    """Windows that reach over maps of 1, 2, 5 and 7 pixels several times; the output lies inside a larger NaN-filled
    allocation whose bytes on either side stay untouched."""
    worst = 0.0
    for name, img, w in fe.convolve_lap_cases():
        got, pads = _convolve(img, w, pad=64)
        worst = max(worst, _check(got, fe.convolve_reference(img, w), fe.convolve_bound(img, w), name))
        assert pads.size == 128 and np.isnan(pads).all(), name
    _report("ast_convolve2d[multi lap]", worst)


def test_convolve2d_refuses_in_place():
    _lib, as_device, ptr, stream = _abi()
    _, img, w = fe.convolve_lap_cases()[6]
    t, wd = as_device(img), as_device(w)
    _refused(_lib.lib().ast_convolve2d(ptr(t), ptr(wd), ptr(t), img.shape[0], w.shape[0], w.shape[1], stream()))
    assert np.array_equal(t.cpu().numpy(), img)
    got, _ = _convolve(img, w)
    _check(got, fe.convolve_reference(img, w), fe.convolve_bound(img, w))


# ------------------------------------------------------------------------------------- ast_gaussian_filter_order
def _gaussian(t, sigma, o0, o1, mode, work_doubles=None, work=None):
    """rc and the output (NaN-filled before the call, like the work buffer of exactly the documented size)."""
    _lib, _, ptr, stream = _abi()
    n = t.shape[0]
    need = fe.gauss_work_doubles(n, sigma) if sigma > 0 else n * n + 2
    work = _nan(need) if work is None else work
    out = _nan(n, n)
    rc = _lib.lib().ast_gaussian_filter_order(ptr(t), ptr(out), ptr(work), need if work_doubles is None else work_doubles,
                                              n, float(sigma), o0, o1, mode, stream())
    return rc, out


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("npix", fe.GAUSS_NPIX)
def test_gaussian_filter_order_cases(npix, mode):
    """Every order 0 .. 8 along either axis and four mixed pairs, radius 0 (sigma 0.1, 0.124), 1, 5 and 20 (at least two
    map widths on the small maps), both modes, against ndimage.gaussian_filter.  scipy leaves its symmetric summation
    path for sigma 0.3 and 1.3 at orders 7 and 8 (its taps are off by more than its tolerance there) while the library's taps keep
    their parity exactly: the summation order differs, which the bound covers."""
    _lib, as_device, _, _ = _abi()
    img = fe.gauss_image(npix)
    t = as_device(img)
    worst = 0.0
    for sigma in fe.GAUSS_SIGMAS:
        for o0, o1 in fe.GAUSS_ORDERS:
            rc, out = _gaussian(t, sigma, o0, o1, mode)
            _lib.check(rc, "ast_gaussian_filter_order")
            worst = max(worst, _check(out.cpu().numpy(), fe.gaussian_reference(img, sigma, o0, o1, mode),
                                      fe.gaussian_bound(img, sigma, o0, o1, mode), (sigma, o0, o1)))
    _report(f"ast_gaussian_filter_order[{fe.MODES[mode]}, npix {npix}]", worst)


@pytest.mark.parametrize("npix", fe.GAUSS_NPIX)
def test_gaussian_filter_order_constant_image_nearest(npix):
    """A constant image in mode "nearest".  An odd order along either axis: exactly zero - the antisymmetric path
    subtracts equal pixels.  An even derivative order: c sum(w0) sum(w1), within the bound of scipy's value; that is not
    rounding, since the taps of an even derivative of a Gaussian cut at 4 sigma do not sum to zero (order 2, sigma 1.3:
    -1.8e-4 against taps of 0.18; tests/test_filter_edges_cpu.py)."""
    _lib, as_device, _, _ = _abi()
    img = np.full((npix, npix), 2.75)
    t = as_device(img)
    worst = 0.0
    for sigma in fe.GAUSS_SIGMAS:
        for o0, o1 in fe.GAUSS_ORDERS:
            if (o0, o1) == (0, 0):
                continue
            rc, out = _gaussian(t, sigma, o0, o1, 1)
            _lib.check(rc, "ast_gaussian_filter_order")
            got = out.cpu().numpy()
            bound = fe.gaussian_bound(img, sigma, o0, o1, 1)
            if (o0 | o1) & 1:
                assert np.all(np.abs(got) <= bound), (sigma, o0, o1)
                assert not got.any(), (sigma, o0, o1)
            else:
                worst = max(worst, _check(got, fe.gaussian_reference(img, sigma, o0, o1, 1), bound, (sigma, o0, o1)))
    _report(f"ast_gaussian_filter_order[constant, npix {npix}]", worst)


def test_gaussian_filter_order_work_size_and_refusals():
    """work_doubles of exactly npix^2 + 2 (2 radius + 1) passes, one less is refused; order 9, order -1, mode 2 and
    sigma 0 are refused; a valid call right after each succeeds."""
    _lib, as_device, _, _ = _abi()
    img = fe.gauss_image(17)
    t = as_device(img)

    def valid(sigma=1.3):
        rc, out = _gaussian(t, sigma, 2, 1, 0)
        _lib.check(rc, "ast_gaussian_filter_order")
        _check(out.cpu().numpy(), fe.gaussian_reference(img, sigma, 2, 1, 0), fe.gaussian_bound(img, sigma, 2, 1, 0))

    for sigma in (0.1, 1.3, 5.0):
        need = fe.gauss_work_doubles(17, sigma)
        work = _nan(need)
        rc, out = _gaussian(t, sigma, 2, 1, 0, work_doubles=need - 1, work=work)
        _refused(rc)
        assert torch.isnan(out).all() and torch.isnan(work).all()          # nothing ran
        valid(sigma)
    for sigma, o0, o1, mode in ((1.3, 9, 0, 0), (1.3, 0, 9, 0), (1.3, -1, 0, 0), (1.3, 0, -1, 1), (1.3, 1, 1, 2),
                                (0.0, 0, 0, 0)):
        rc, out = _gaussian(t, sigma, o0, o1, mode)
        _refused(rc)
        assert torch.isnan(out).all()
        valid()


# ------------------------------------------------------------------------------------------------ ast_dgd_filter
def _dgd(t, sigma, h, axis, order, npix=None):
    _lib, _, ptr, stream = _abi()
    n = t.shape[0] if npix is None else npix
    work, out = _nan(2 * n * n), _nan(n, n)
    rc = _lib.lib().ast_dgd_filter(ptr(t), ptr(out), ptr(work), n, float(sigma), float(h), axis, order, stream())
    return rc, out


@pytest.mark.parametrize("npix", fe.DGD_NPIX)
def test_dgd_filter_cases(npix):
    """img = ones - the output is the window's derivative, border stencils included, pixel by pixel - and a random image;
    sigma_pix from 1 to four map widths, h = 1 and 2 / npix.  With sigma_pix 1 on 64 pixels the border of the DGD1 window
    underflows to zero and the output there is exactly 0.0, not NaN."""
    _lib, as_device, _, _ = _abi()
    images = [(np.ones((npix, npix)), True), (fe.dgd_image(npix), False)]
    di, dj = fe.border_distance(npix)
    worst, zero_border = 0.0, 0
    for img, is_ones in images:
        t = as_device(img)
        for sigma, h, axis, order in fe.dgd_params(npix):
            rc, out = _dgd(t, sigma, h, axis, order)
            _lib.check(rc, "ast_dgd_filter")
            got = out.cpu().numpy()
            assert np.all(np.isfinite(got)), (sigma, h, axis, order)
            worst = max(worst, _check(got, fe.dgd_reference(img, sigma, h, axis, order),
                                      fe.dgd_bound(img, sigma, h, axis, order), (sigma, h, axis, order)))
            if fe.dgd_window_border_is_zero(npix, sigma, order):
                zero_border += 1
                assert not got[(di if axis == 0 else dj) == 0].any()
                assert not got[np.minimum(di, dj) == 0].any()
    assert zero_border == (8 if npix == 64 else 0)
    _report(f"ast_dgd_filter[npix {npix}]", worst)


def test_dgd_filter_refusals():
    _lib, as_device, _, _ = _abi()
    img = fe.dgd_image(5)
    t = as_device(img)
    for npix, axis, order in ((2, 0, 1), (5, 0, 2), (5, 2, 1)):
        rc, out = _dgd(t, 2.0, 1.0, axis, order, npix=npix)
        _refused(rc)
        assert torch.isnan(out).all()
        rc, out = _dgd(t, 2.0, 1.0, 1, 3)
        _lib.check(rc, "ast_dgd_filter")
        _check(out.cpu().numpy(), fe.dgd_reference(img, 2.0, 1.0, 1, 3), fe.dgd_bound(img, 2.0, 1.0, 1, 3))


# --------------------------------------------------------------------------------------- ast_aperture_photometry
@pytest.mark.parametrize("npix,alpha", list(fe.RING_COUNTS))
def test_aperture_photometry_cases(npix, alpha):
    """Rings with pixels exactly on either edge, cut by the map border, made of the corners alone, empty, wholly off the
    map, and on a map larger than the partial kernel's 262144 threads.  An empty ring gives NaN in every pixel, like
    np.mean of nothing.  Out of place equals in place bit for bit and leaves the image alone; the work buffer starts
    as NaN."""
    _lib, as_device, ptr, stream = _abi()
    img = fe.aperture_image(npix)
    t = as_device(img)
    out = _nan(npix, npix)
    _lib.check(_lib.lib().ast_aperture_photometry(ptr(t), ptr(out), ptr(_nan(2048)), npix, float(alpha), stream()),
               "ast_aperture_photometry")
    got = out.cpu().numpy()
    assert np.array_equal(t.cpu().numpy(), img)
    _lib.check(_lib.lib().ast_aperture_photometry(ptr(t), ptr(t), ptr(_nan(2048)), npix, float(alpha), stream()),
               "ast_aperture_photometry")
    assert np.array_equal(t.cpu().numpy(), got, equal_nan=True)
    if fe.RING_COUNTS[(npix, alpha)][0] == 0:
        assert np.isnan(got).all()
        ratio = 0.0
    else:
        ratio = _check(got, fe.aperture_reference(img, alpha), fe.aperture_bound(img, alpha))
    _report(f"ast_aperture_photometry[{npix}, {alpha}]", ratio)


# ----------------------------------------------------------------------------------------------- ast_hann_apodize
@pytest.mark.parametrize("npix", fe.HANN_NPIX)
def test_hann_apodize_cases(npix):
    """npix = 1 returns the image exactly: scipy.signal.windows.hann(1) = [1.] is the contract (the reference calls
    scipy's window); oracle.kappa.apodization divides by zero there and has no answer.  npix 2 and 3: the border is within
    4 u |img| of zero and the centre pixel of 3 is the image's."""
    _lib, as_device, ptr, stream = _abi()
    img = fe.hann_image(npix)
    t = as_device(img)
    out = _nan(npix, npix)
    _lib.check(_lib.lib().ast_hann_apodize(ptr(t), ptr(out), npix, stream()), "ast_hann_apodize")
    got = out.cpu().numpy()
    ratio = _check(got, fe.hann_reference(img), fe.hann_bound(img))
    if npix == 1:
        assert np.array_equal(got, img)
    if npix in (2, 3):
        di, dj = fe.border_distance(npix)
        edge = np.minimum(di, dj) == 0
        assert np.all(np.abs(got[edge]) <= 4.0 * fe.U * np.abs(img[edge]))
    if npix == 3:
        assert got[1, 1] == img[1, 1]
    _report(f"ast_hann_apodize[{npix}]", ratio)


# ------------------------------------------------------------------------------------------------ ast_zoom_linear
def _zoom(t, nout, out=None, nin=None):
    _lib, _, ptr, stream = _abi()
    out = _nan(max(nout, 1), max(nout, 1)) if out is None else out
    rc = _lib.lib().ast_zoom_linear(ptr(t), t.shape[0] if nin is None else nin, ptr(out), nout, stream())
    return rc, out


@pytest.mark.parametrize("nin,nout", fe.ZOOM_SHAPES)
def test_zoom_linear_cases(nin, nout):
    """On its own, without the Gaussian prefilter: one output pixel, one input pixel, nout == nin (the input bit for
    bit), samples exactly between four pixels ((16, 8): the exact block means of an integer-valued image) and exactly on
    a pixel ((15, 5): the block centres), against ndimage.zoom(order=1, grid_mode=True, mode="mirror")."""
    _lib, as_device, _, _ = _abi()
    img = fe.zoom_image(nin, nout)
    rc, out = _zoom(as_device(img), nout)
    _lib.check(rc, "ast_zoom_linear")
    got = out.cpu().numpy()
    ratio = _check(got, fe.zoom_reference(img, nout), fe.zoom_bound(img, nout))
    exact = fe.zoom_exact(img, nout)
    assert (exact is not None) == (nout == nin or (nin, nout) in ((16, 8), (15, 5)))
    if exact is not None:
        assert np.array_equal(got, exact)
    _report(f"ast_zoom_linear[{nin} -> {nout}]", ratio)


def test_zoom_linear_refusals():
    _lib, as_device, _, _ = _abi()
    img = fe.zoom_image(7, 3)
    t = as_device(img)
    for attempt in ("nout > nin", "nout = 0", "img == out"):
        if attempt == "nout > nin":
            rc, out = _zoom(t, 8, out=_nan(8, 8))
        elif attempt == "nout = 0":
            rc, out = _zoom(t, 0)
        else:
            rc, out = _zoom(t, 3, out=t)
        _refused(rc)
        assert np.array_equal(t.cpu().numpy(), img) and (out is t or torch.isnan(out).all())
        rc, out = _zoom(t, 3)
        _lib.check(rc, "ast_zoom_linear")
        _check(out.cpu().numpy(), fe.zoom_reference(img, 3), fe.zoom_bound(img, 3))


# ---------------------------------------------------------------------------------------- ast_deflection_to_shear
def test_deflection_to_shear_three_pixels_and_aliasing_refusals():
    """npix = 3 - one interior pixel per line between the two one-sided ends - bit for bit like numpy; each of the five
    aliasings the entry point rules out (an output on an input, the outputs on each other) is refused and leaves the
    inputs alone, and a valid call follows."""
    _lib, as_device, ptr, stream = _abi()
    rng = np.random.default_rng(33)
    a1, a2 = rng.standard_normal((3, 3)) * 1e-3, rng.standard_normal((3, 3)) * 1e-3
    h = np.deg2rad(10.0) / 3
    w1, w2 = ok.deflection_to_shear(a1, a2, h)
    t1, t2 = as_device(a1), as_device(a2)

    def call(g1, g2):
        return _lib.lib().ast_deflection_to_shear(ptr(t1), ptr(t2), 3, float(h), ptr(g1), ptr(g2), stream())

    def valid():
        g1, g2 = _nan(3, 3), _nan(3, 3)
        _lib.check(call(g1, g2), "ast_deflection_to_shear")
        assert np.array_equal(g1.cpu().numpy(), w1) and np.array_equal(g2.cpu().numpy(), w2)

    valid()
    for alias in ("g1=a1", "g1=a2", "g2=a1", "g2=a2", "g1=g2"):
        g1, g2 = _nan(3, 3), _nan(3, 3)
        if alias == "g1=g2":
            g2 = g1
        else:
            src = t1 if alias.endswith("a1") else t2
            g1, g2 = (src, g2) if alias.startswith("g1") else (g1, src)
        _refused(call(g1, g2))
        assert np.array_equal(t1.cpu().numpy(), a1) and np.array_equal(t2.cpu().numpy(), a2)
        valid()
