"""Oracle: Ray-Ramses kappa-map stack and the per-map pipeline (numpy, float64).

TEST INFRASTRUCTURE — see oracle/__init__.py.  Paths below are relative to
/root/reference/src/astrild/.

Pinned by the reference's own known-answer tests (values restated as data in
tests/golden/reference_known_answers.json; checked in tests/test_oracle_kappa.py):
  * kappa0_to_alphas      <- tests/unit/rays/skys/test_skyutils.py:113-125
  * NFW dT / alpha maps   <- tests/unit/rays/skys/test_skyutils.py:43-95
  * unit conversion       <- tests/unit/rays/skys/test_skyutils.py:97-111
  * Gaussian smoothing    <- tests/unit/rays/utils/test_filters.py:47-55
The reference C library (rays/skys/lib_so_cgls/*.c) is NOT built here: it needs
fftw3.h / libfftw3, which this image lacks, and stand-ins are not allowed, so it
is "unbuildable"; the numpy restatement below is pinned by the test values
instead.  The plane stack itself has no reference test (parity unpinned); it
is plain sequential IEEE addition and is compared bit for bit.
"""
import numpy as np
from scipy import ndimage

C_LIGHT_KMS = 299792.458      # astropy c.to("km/s").value, rays/skys/sky_utils.py:17
GCM2 = 4.785e-20              # G/c^2 [Mpc/M_sun], rays/skys/sky_utils.py:19


# ----------------------------------------------------------------- a-7 stack
def kernel_function(x, x_s):
    """g = (x_s - x) * x / x_s — rays/rayramses.py:315-326, simcoll.py:432-443."""
    return (x_s - x) * x / x_s


def translate_redshift(quantity, x_near, x_far, x_src, x_src_shift):
    """rays/rayramses.py:269-312 with comoving distances already evaluated
    (the reference calls astropy's cosmology.comoving_distance for them)."""
    x_shift = x_far if x_far > x_src_shift else x_src_shift
    x_mid = 0.5 * (x_far + x_near)
    return quantity * kernel_function(x_mid, x_shift) / kernel_function(x_mid, x_src)


def kappa_stack(planes, x_near=None, x_far=None, x_src=None, x_src_shift=None):
    """Running sum in plane order: first plane copied, then ``sum = sum + plane``
    (rays/rayramses.py:224-232; simcoll.py:322-336), each plane optionally
    re-weighted first."""
    total = None
    for p, plane in enumerate(planes):
        q = np.asarray(plane, dtype=np.float64)
        if x_near is not None:
            q = translate_redshift(q, x_near[p], x_far[p], x_src, x_src_shift)
        total = q.copy() if total is None else total + q
    return total


# --------------------------------------------------------------- a-8 per map
def convert_code_to_phy_units(quantity, values):
    """rays/skys/sky_utils.py:318-339."""
    values = np.asarray(values, dtype=np.float64)
    if quantity in ["shear_x", "shear_y", "deflt_x", "deflt_y", "kappa_2"]:
        return values / C_LIGHT_KMS ** 2
    if quantity in ["isw_rs"]:
        return values / C_LIGHT_KMS ** 3
    return values


def rays_to_map(values):
    """rays/skyio.py:32-48: the sort key is arange, so this is a row-major reshape."""
    npix = int(np.sqrt(len(values)))
    return np.asarray(values, dtype=np.float64)[: npix * npix].reshape(npix, npix).copy()


def gaussian_smooth(img, theta_deg, sigma_arcmin, kind=None):
    """Filters.gaussian (rays/utils/filters.py:181-225) -> lenstools
    ConvergenceMap.smooth: sigma_px = sigma * npix / theta; <500 px real space
    (scipy gaussian_filter: reflect, truncate 4), else FFT (periodic)."""
    img = np.asarray(img, dtype=np.float64)
    npix = img.shape[0]
    sigma_px = (sigma_arcmin / 60.0) * npix / theta_deg
    if kind is None:
        kind = "gaussian" if npix < 500 else "gaussianFFT"
    if kind == "gaussian":
        return ndimage.gaussian_filter(img, sigma=sigma_px)
    lx = np.fft.rfftfreq(npix)
    ly = np.fft.fftfreq(npix)
    l2 = lx[None, :] ** 2 + ly[:, None] ** 2
    return np.fft.irfft2(np.exp(-0.5 * l2 * (2 * np.pi * sigma_px) ** 2) * np.fft.rfft2(img), s=img.shape)


def fwhm_to_sigma(fwhm):
    return fwhm / (2 * np.sqrt(2 * np.log(2)))      # rays/utils/filters.py:256-257


def galaxy_shape_noise(npix, rnd_seed):
    """rays/skys/sky_array.py:665-690: sigma_pix is hard-coded to 0.007."""
    rg = np.random.Generator(np.random.PCG64(rnd_seed))
    return rg.normal(loc=0, scale=0.007, size=[npix, npix])


def pdf(img, nbins):
    """rays/skys/sky_array.py:428-433."""
    return np.histogram(img, bins=nbins, density=True)


def locate_peaks(img, thresholds):
    """lenstools ``ConvergenceMap.locatePeaks(thresholds)`` as called at rays/skys/sky_array.py:465-466
    (lenstools is un-vendored and unpinned; its peak finder restated): interior pixels strictly larger than all
    8 neighbours, height in [thresholds[0], thresholds[-1]); heights and (y, x) in row-major scan order."""
    a = np.asarray(img, dtype=np.float64)
    c = a[1:-1, 1:-1]
    peak = np.ones(c.shape, dtype=bool)
    n0, n1 = a.shape
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if dy == 1 and dx == 1:
                continue
            peak &= c > a[dy:n0 - 2 + dy, dx:n1 - 2 + dx]
    peak &= (c >= thresholds[0]) & (c < thresholds[-1])
    ys, xs = np.nonzero(peak)
    return c[ys, xs], np.stack([ys + 1, xs + 1], axis=1)


def wl_peak_counts(img, nbins, field_conversion="", limits=None):
    """rays/skys/sky_array.py:435-472 (the mean of the map itself where the reference reads ``self.skymap``)."""
    img = np.asarray(img, dtype=np.float64)
    _map = img - np.mean(img) if field_conversion == "normalize" else img
    if limits is None:
        lower_bound, upper_bound = np.percentile(img, 5), np.percentile(img, 95)
    else:
        lower_bound, upper_bound = min(limits), max(limits)
    map_bins = np.arange(lower_bound, upper_bound, (upper_bound - lower_bound) / nbins)
    _kappa, _ = locate_peaks(_map, map_bins)
    _hist, _kappa = np.histogram(_kappa, bins=nbins, density=False)
    return (_kappa[1:] + _kappa[:-1]) / 2, _hist


# ------------------------------------------------ f-3 flat-sky spectra (lenstools)
def _pixel_l(npix, angle_rad):
    i = np.arange(npix)
    lx = np.minimum(i, npix - i) * 2.0 * np.pi / angle_rad
    ly = np.arange(npix // 2 + 1) * 2.0 * np.pi / angle_rad
    return np.sqrt(lx[:, None] ** 2 + ly[None, :] ** 2)


def flat_power_spectrum(img, angle_deg, l_edges, img2=None):
    """lenstools ``ConvergenceMap.powerSpectrum`` as called at power_spectra/angular_power_spectrum.py:48-52
    (un-vendored, unpinned; its rfft2 + azimuthal average restated): bins (l_k, l_k+1], mean of Re(ft1 conj ft2)
    over the half-plane pixels of the bin, times (angle / npix^2)^2."""
    img = np.asarray(img, dtype=np.float64)
    n = img.shape[0]
    angle = np.deg2rad(angle_deg)
    f1 = np.fft.rfft2(img)
    f2 = f1 if img2 is None else np.fft.rfft2(np.asarray(img2, dtype=np.float64))
    l = _pixel_l(n, angle)
    p = (f1 * np.conj(f2)).real
    l_edges = np.asarray(l_edges, dtype=np.float64)
    out = np.zeros(len(l_edges) - 1)
    for k in range(len(out)):
        sel = (l > l_edges[k]) & (l <= l_edges[k + 1])
        if sel.any():
            out[k] = p[sel].mean()
    return 0.5 * (l_edges[:-1] + l_edges[1:]), out * (angle / n ** 2) ** 2


def flat_bispectrum_equilateral_brute(img, angle_deg, l_edges):
    """Equilateral flat-sky bispectrum by direct enumeration of the closed triangles of the FULL Fourier plane
    (tiny maps only): B_k = angle^4 / npix^6 * mean of ft(l1) ft(l2) ft(l3) over l1 + l2 + l3 = 0 with every
    |l_i| in (l_k, l_k+1] - what lenstools' ``bispectrum(configuration="equilateral")`` averages
    (bispectra/bispectrum_2d.py:45-49)."""
    img = np.asarray(img, dtype=np.float64)
    n = img.shape[0]
    angle = np.deg2rad(angle_deg)
    ft = np.fft.fft2(img)
    m = np.arange(n)
    m = np.minimum(m, n - m)
    lmod = np.sqrt(m[:, None] ** 2 + m[None, :] ** 2) * 2.0 * np.pi / angle
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    l_edges = np.asarray(l_edges, dtype=np.float64)
    b, ntri = np.zeros(len(l_edges) - 1), np.zeros(len(l_edges) - 1, dtype=np.int64)
    for k in range(len(b)):
        sel = (lmod > l_edges[k]) & (lmod <= l_edges[k + 1])
        a_i, a_j = ii[sel], jj[sel]
        i3 = (-(a_i[:, None] + a_i[None, :])) % n
        j3 = (-(a_j[:, None] + a_j[None, :])) % n
        ok_ = sel[i3, j3]
        ntri[k] = int(ok_.sum())
        if ntri[k]:
            prod = ft[a_i, a_j][:, None] * ft[a_i, a_j][None, :] * ft[i3, j3]
            b[k] = prod[ok_].real.sum() / ntri[k] * angle ** 4 / float(n) ** 6
    return 0.5 * (l_edges[:-1] + l_edges[1:]), b, ntri


# ----------------------------------------------------- a-9 kappa -> alpha, phi
def _iso_kernel(ncc, dcell, which):
    """kernel_alphas_iso / kernel_phi_iso, rays/skys/lib_so_cgls/lensing_funcs.c:45-83,117-148."""
    h = ncc // 2
    idx = np.arange(ncc)
    folded = np.where(idx <= h, idx, ncc - idx)
    x = (folded * dcell + 0.5 * dcell)[:, None] * np.ones((1, ncc))
    y = (folded * dcell + 0.5 * dcell)[None, :] * np.ones((ncc, 1))
    r = np.sqrt(x * x + y * y)
    inside = ~(r > dcell * ncc / 2.0)
    if which == 0:
        k = np.where(inside, x / (np.pi * r * r), 0.0)
        k = np.where((idx > h)[:, None], -k, k)
    elif which == 1:
        k = np.where(inside, y / (np.pi * r * r), 0.0)
        k = np.where((idx > h)[None, :], -k, k)
    else:
        k = np.where(inside, np.log(r) / np.pi, 0.0)
    return k


def _convolve_corner(kappa0, kernel, nc, dsx):
    """zero_padding + convolve_fft + corner_matrix (lensing_funcs.c:8-43, fft_convolve.c:48-95)."""
    n2 = 2 * nc
    pad = np.zeros((n2, n2))
    pad[:nc, :nc] = kappa0
    full = np.fft.irfft2(np.fft.rfft2(pad) * np.fft.rfft2(kernel), s=(n2, n2)) * (n2 * n2)   # FFTW c2r is unnormalised
    return (full / (n2 * n2) * dsx * dsx)[:nc, :nc]


def kappa0_to_alphas(kappa0, nc, bsz):
    """lensing_funcs.c:86-115.  Returns (alpha1, alpha2) in the C argument order."""
    kappa0 = np.asarray(kappa0, dtype=np.float64).reshape(nc, nc)
    dsx = bsz / nc
    a1 = _convolve_corner(kappa0, _iso_kernel(2 * nc, dsx, 0), nc, dsx)
    a2 = _convolve_corner(kappa0, _iso_kernel(2 * nc, dsx, 1), nc, dsx)
    return a1, a2


def kappa0_to_phi(kappa0, nc, bsz):
    """lensing_funcs.c:151-173."""
    kappa0 = np.asarray(kappa0, dtype=np.float64).reshape(nc, nc)
    dsx = bsz / nc
    return _convolve_corner(kappa0, _iso_kernel(2 * nc, dsx, 2), nc, dsx)


def general_gaussian(m, p, sig):
    """scipy.signal.general_gaussian (removed from scipy.signal's top level):
    exp(-0.5 * |n/sig|^(2p)), n = arange(m) - (m-1)/2.  Input of the reference's
    kappa->alpha test fixture (test_skyutils.py:35-40)."""
    n = np.arange(m) - (m - 1.0) / 2.0
    return np.exp(-0.5 * np.abs(n / sig) ** (2 * p))


# ---------------------------------------------------- f-2 NFW stamps (next row)
def nfw_deflection_angle_map(theta_200c, m_200c, c_200c, angu_diam_dist, npix=100, extent=1,
                             direction=(0,), suppress=False, suppression_r=1):
    """rays/skys/sky_utils.py:214-282 (Baxter et al. 2015, Sec. 3.2)."""
    assert np.sum(direction) <= 1
    r200 = np.tan(theta_200c * np.pi / 180) * angu_diam_dist
    edges = np.linspace(0, 2 * r200 * extent, npix) - r200 * extent
    tx, ty = np.meshgrid(edges, edges)
    rr = np.sqrt(tx ** 2 + ty ** 2)
    amp = m_200c * c_200c ** 2 / (np.log(1 + c_200c) - c_200c / (1 + c_200c)) / 4.0 / np.pi
    const = 16 * np.pi * GCM2 * amp / c_200c / r200
    x = (rr / (r200 / c_200c)).astype(complex)
    with np.errstate(all="ignore"):
        f = np.true_divide(1, x) * (np.log(x / 2) + 2 / np.sqrt(1 - x ** 2)
                                    * np.arctanh(np.sqrt(np.true_divide(1 - x, 1 + x))))
        out = np.zeros((npix, npix), dtype=complex)
        for d in direction:
            out += const * np.true_divide(tx if d == 0 else ty, rr) * f
    out = np.nan_to_num(out, copy=False, nan=0.0, posinf=0.0, neginf=0.0)
    if suppress:
        out *= np.exp(-(rr / (suppression_r * r200)) ** 3)
    out = out.real.copy()
    out[abs(out) > 100] = 0.0
    return out


def nfw_temperature_perturbation_map(theta_200c, m_200c, c_200c, vel, angu_diam_dist, npix=100, extent=1,
                                     direction=(0, 1), suppress=False, suppression_r=1):
    """rays/skys/sky_utils.py:176-211 (moving-lens / Birkinshaw-Gull effect)."""
    dt = np.zeros((npix, npix))
    for d in direction:
        a = nfw_deflection_angle_map(theta_200c, m_200c, c_200c, angu_diam_dist, npix, extent, [d],
                                     suppress, suppression_r)
        dt += -a * vel[d] / C_LIGHT_KMS
    return dt


def add_patch_to_map(limg, simg, cen_pix):
    """rays/skys/sky_utils.py:140-173: add a stamp, clipped at the map boundary.  Stamp pixel (i, j) of an S x S stamp
    lands on map pixel (cen_y - S // 2 + i, cen_x - S // 2 + j).  For an odd stamp that touches the map this is the
    reference's sum, addition for addition.  Two extensions, where the reference raises (IndexError, ValueError): an
    even stamp follows the same rule, and a stamp with no pixel on the map adds nothing."""
    s, n = len(simg), len(limg)
    x0, y0 = cen_pix[0] - s // 2, cen_pix[1] - s // 2
    j_lo, j_hi = max(0, -x0), min(s, n - x0)
    i_lo, i_hi = max(0, -y0), min(s, n - y0)
    if j_hi <= j_lo or i_hi <= i_lo:
        return limg
    limg[y0 + i_lo: y0 + i_hi, x0 + j_lo: x0 + j_hi] += simg[i_lo:i_hi, j_lo:j_hi]
    return limg


def analytic_halo_signal_map(halo_cat, extent, direction, suppress, suppression_r, npix, signal):
    """rays/skys/sky_utils.py:79-137 for a catalogue dict of equal-length arrays."""
    out = np.zeros((npix, npix))
    for i in range(len(halo_cat["m200"])):
        stamp_npix = int(2 * halo_cat["r200_pix"][i] * extent) + 1
        dist = halo_cat["Dc"][i] * 0.6774
        if signal == "dT":
            stamp = nfw_temperature_perturbation_map(
                halo_cat["r200_deg"][i], halo_cat["m200"][i], halo_cat["c_NFW"][i],
                [halo_cat["theta1_tv"][i], halo_cat["theta2_tv"][i]], dist, stamp_npix, extent, direction,
                suppress, suppression_r)
        else:
            stamp = nfw_deflection_angle_map(
                halo_cat["r200_deg"][i], halo_cat["m200"][i], halo_cat["c_NFW"][i], dist, stamp_npix, extent,
                direction, suppress, suppression_r)
        out = add_patch_to_map(out, stamp, (halo_cat["theta1_pix"][i], halo_cat["theta2_pix"][i]))
    return out


# ------------------------------------------------ f-3 dipole windows, apodization
def gaussian_field(theta, sigma):
    """rays/utils/filters.py:403-413."""
    return np.exp(-theta ** 2 / (2 * sigma ** 2)) / (2 * np.pi * sigma ** 2)


def dgd_filter(img, theta_deg, theta_i_deg, direction, order=3):
    """Filters.gaussian_third_derivative (order 3, filters.py:305-355) /
    gaussian_first_derivative (order 1, :358-400): window from repeated np.gradient, times img."""
    img = np.asarray(img, dtype=np.float64)
    npix = len(img)
    x1 = np.linspace(1, npix, npix) - npix / 2 - 0.5
    x, y = np.meshgrid(x1, x1)
    dist = np.sqrt(x ** 2 + y ** 2)
    theta_fov = theta_deg * len(dist) / npix
    s = np.ceil(npix * theta_i_deg / theta_deg).astype("int")
    if order == 3:
        w = gaussian_field(dist, s * 0.5) - gaussian_field(dist, s) + gaussian_field(dist, s * 2.0)
    else:
        w = gaussian_field(dist, s * 0.5)
    for _ in range(order):
        w = np.gradient(w, theta_fov / len(dist), axis=direction, edge_order=2)
    return np.multiply(w, img)


def deflection_to_shear(alpha1, alpha2, h):
    """SkyUtils.convert_deflection_to_shear, rays/skys/sky_utils.py:342-362, with the undefined `coord` read as the
    uniform pixel spacing h (np.gradient's scalar spacing; edge_order 1, numpy's default).  PARITY UNPINNED: the
    reference's body is marked TODO and no reference test holds a value."""
    a1, a2 = np.asarray(alpha1, dtype=np.float64), np.asarray(alpha2, dtype=np.float64)
    al11 = 1 - np.gradient(a1, h, axis=0)
    al12 = -np.gradient(a1, h, axis=1)
    al21 = -np.gradient(a2, h, axis=0)
    al22 = 1 - np.gradient(a2, h, axis=1)
    return 0.5 * (al11 - al22), 0.5 * (al21 + al12)


def resize_antialiased(img, npix):
    """SkyArray.resize (sky_array.py:475-496) = skimage.transform.resize(img, (npix, npix), anti_aliasing=True), restated
    from scikit-image >= 0.19 (transform/_warps.py resize: Gaussian prefilter with sigma = (in / out - 1) / 2 in the
    boundary mode of the resampling, then scipy.ndimage.zoom with grid_mode=True), with scipy doing what it does there.
    resize's default mode="reflect" is numpy.pad's name; _to_ndimage_mode maps it to ndimage's "mirror".
    PARITY UNPINNED: scikit-image is neither importable here nor pinned by the reference's lock file, and no reference
    test holds a value."""
    from scipy import ndimage
    img = np.asarray(img, dtype=np.float64)
    nin = img.shape[0]
    sigma = max(0.0, (nin / npix - 1.0) / 2.0)
    if sigma > 0.0:
        img = ndimage.gaussian_filter(img, (sigma, sigma), cval=0.0, mode="mirror")
    return ndimage.zoom(img, (npix / nin, npix / nin), order=1, mode="mirror", cval=0.0, grid_mode=True)


def apodization(img):
    """rays/utils/filters.py:150-178 with scipy.signal.hann(n) = 0.5 - 0.5 cos(2 pi k / (n-1))."""
    n = len(img)
    h = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / (n - 1))
    return np.asarray(img, dtype=np.float64) * np.outer(h, h)


def dgd3_convolution(img, theta_deg, theta_i_deg, direction=1):
    """Filters.gaussian_third_derivative_convolution, rays/utils/filters.py:260-304."""
    img = np.asarray(img, dtype=np.float64)
    s = np.ceil(img.shape[0] * theta_i_deg / theta_deg).astype("int")
    g = [ndimage.gaussian_filter(img, sigma=s * f, order=3 * direction, output=np.float64, mode="nearest")
         for f in (0.5, 1.0, 2.0)]
    return g[0] - g[1] + g[2]


def gaussian_compensated(img, theta_deg, theta_i_deg, theta_o_deg):
    """Filters.gaussian_compensated, rays/utils/filters.py:415-459."""
    img = np.asarray(img, dtype=np.float64)
    pw = theta_deg / img.shape[0]
    t_i, t_o = theta_i_deg / pw, theta_o_deg / pw
    t_o_int = np.ceil(t_o).astype("int")
    y, x = np.ogrid[-t_o_int:t_o_int, -t_o_int:t_o_int]
    dist = np.sqrt(x ** 2 + y ** 2)
    xx, x_o = dist / t_i, t_o / t_i
    gt = (np.exp(-xx ** 2.0) / (np.pi * t_i ** 2.0)) - ((1.0 - np.exp(-x_o ** 2.0)) / (np.pi * t_o ** 2.0))
    gt[t_o < dist] = 0
    return ndimage.convolve(img, gt)


def aperture_photometry(img, theta_deg, alpha_deg):
    """Filters.aperture_photometry, rays/utils/filters.py:40-73."""
    img = np.array(img, dtype=np.float64)
    npix = len(img)
    x1 = np.linspace(1, npix, npix) - npix / 2 - 0.5
    x, y = np.meshgrid(x1, x1)
    d = np.sqrt(x ** 2 + y ** 2)
    a = np.ceil(alpha_deg * npix / theta_deg).astype("int")
    ring = np.logical_and(a < d, d < a * np.sqrt(2))
    return img - np.mean(img[ring])
