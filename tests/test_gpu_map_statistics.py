"""GPU: the sky-map statistics kernels at their edges - peaks and order statistics (peaks.hip), flat-sky spectra
(flatsky.hip), the periodic Gaussian passes (kappa.hip) around a small map and the histogram's bin limits (util.hip) -
against numpy in float64 and the oracle.

Selections (peaks, order statistics, percentiles, counts) are compared for exact equality; the spectra and the
smoothing at the tolerances of test_gpu_kappa.py, quoted where they are used."""
import numpy as np
import numpy.testing as npt
import pytest

from oracle import kappa as ok

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

INF = np.inf


@pytest.fixture(scope="module")
def lens(hip):
    from astrild_amd import lensing
    torch.cuda.set_device(0)
    return lensing


@pytest.fixture(scope="module")
def dev(hip):
    from astrild_amd import device
    return device


# ====================================================================== peaks
def _check_peaks(lens, dev, img, lo=-INF, hi=INF):
    """peak_find against the oracle on the very array (float32 maps are widened by the oracle, exactly)."""
    npix = img.shape[0]
    vals, idx = lens.peak_find(dev.as_device(np.ascontiguousarray(img)), lo, hi)
    with np.errstate(invalid="ignore"):
        rv, rp = ok.locate_peaks(img, np.array([lo, hi]))
    ri = rp[:, 0] * npix + rp[:, 1]
    assert vals.dtype == img.dtype and idx.dtype == np.int64
    assert np.array_equal(idx, ri), (npix, lo, hi, len(idx), len(ri))
    assert np.array_equal(vals.astype(np.float64), rv)
    if len(idx):
        y, x = idx // npix, idx % npix
        assert y.min() >= 1 and x.min() >= 1 and y.max() <= npix - 2 and x.max() <= npix - 2
    return vals, idx


NPIX = [3, 4, 15, 16, 17, 18, 33, 257]


def _planted(npix, side_y, side_x, high_border, rng):
    """Low noise with peaks of distinct heights on the four interior corners and, per tile seam at 16 k, on the row
    (column) just before (side 0) or just after (side 1) it."""
    img = rng.uniform(0.0, 0.1, (npix, npix))
    seams = np.arange(16, npix, 16)
    inside = lambda v: sorted(set(int(c) for c in v if 1 <= c <= npix - 2))
    rows = inside([1, npix - 2] + list(seams - 1 + side_y))
    cols = inside([1, npix - 2] + list(seams - 1 + side_x))
    h = 1.0
    for y in rows:
        for x in cols:
            img[y, x] = h
            h += 1.0 / 1024
    if high_border:                       # never peaks themselves, but they put out the interior pixels next to them
        for k in range(0, npix, 3):
            img[0, k] = img[k, npix - 1] = 50.0 + k
        for k in range(1, npix, 4):
            img[npix - 1, k] = img[k, 0] = 70.0 + k
    return img, rows, cols


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("npix", NPIX)
def test_peaks_at_corners_and_on_both_sides_of_every_tile_seam(lens, dev, npix, dtype):
    rng = np.random.default_rng(npix)
    for side_y in (0, 1):
        for side_x in (0, 1):
            img, rows, cols = _planted(npix, side_y, side_x, False, rng)
            img = img.astype(dtype)
            vals, idx = _check_peaks(lens, dev, img)
            found = set(idx.tolist())
            # planted pixels with no planted neighbour must all be there
            for y in rows:
                for x in cols:
                    alone = all((yy, xx) == (y, x) or not (abs(yy - y) <= 1 and abs(xx - x) <= 1)
                                for yy in rows for xx in cols)
                    if alone:
                        assert y * npix + x in found, (npix, y, x)
            assert (npix - 2) * npix + npix - 2 in found          # the highest of all
            assert npix < 5 or npix + 1 in found
            bordered, _, _ = _planted(npix, side_y, side_x, True, rng)
            _check_peaks(lens, dev, bordered.astype(dtype))
    # a random map, and one of few levels (ties everywhere)
    _check_peaks(lens, dev, rng.standard_normal((npix, npix)).astype(dtype))
    _check_peaks(lens, dev, rng.integers(0, 4, (npix, npix)).astype(dtype))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_outermost_rows_and_columns_are_never_peaks_but_suppress(lens, dev, dtype):
    for npix in NPIX:
        img = np.zeros((npix, npix), dtype=dtype)
        img[0, :] = img[-1, :] = img[:, 0] = img[:, -1] = 9.0
        img[1:-1, 1:-1] = 1.0 + np.arange((npix - 2) ** 2).reshape(npix - 2, npix - 2) % 7
        vals, idx = _check_peaks(lens, dev, img)
        y, x = idx // npix, idx % npix
        assert not ((y == 1) | (x == 1) | (y == npix - 2) | (x == npix - 2)).any()
        img[0, :] = img[-1, :] = img[:, 0] = img[:, -1] = -9.0          # now the ring next to the border is free
        _check_peaks(lens, dev, img)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_equal_neighbours_are_not_peaks(lens, dev, dtype):
    npix = 49
    img = np.zeros((npix, npix), dtype=dtype)
    pairs = [((8, 4), (8, 5)), ((22, 15), (22, 16)), ((40, 31), (40, 32)),             # side by side: in a tile, across seams
             ((4, 12), (5, 12)), ((15, 26), (16, 26)), ((31, 44), (32, 44)),           # one above the other
             ((4, 4), (5, 5)), ((15, 15), (16, 16)), ((31, 31), (32, 32)),             # diagonal
             ((4, 21), (5, 20)), ((15, 32), (16, 31)), ((31, 16), (32, 15))]           # the other diagonal
    used = np.zeros((npix, npix), dtype=bool)
    for k, (a, b) in enumerate(pairs):
        box = (slice(min(a[0], b[0]) - 1, max(a[0], b[0]) + 2), slice(min(a[1], b[1]) - 1, max(a[1], b[1]) + 2))
        assert not used[box].any()                                # no pair is next to another
        used[box] = True
        img[a] = img[b] = 2.0 + k
    singles = [(45, 3), (3, 45), (45, 45), (22, 2)]
    for s in singles:
        assert not used[s[0] - 1:s[0] + 2, s[1] - 1:s[1] + 2].any()
        img[s] = 1.5
    vals, idx = _check_peaks(lens, dev, img)
    assert sorted(idx.tolist()) == sorted(y * npix + x for y, x in singles)
    for npix in NPIX:
        for level in (0.0, -3.5, INF, -INF):
            vals, idx = _check_peaks(lens, dev, np.full((npix, npix), level, dtype=dtype))
            assert len(idx) == 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_peaks_among_nan_and_infinite_pixels(lens, dev, dtype):
    rng = np.random.default_rng(5)
    for npix in (4, 17, 33, 257):
        img = rng.standard_normal((npix, npix)).astype(dtype)
        ny, nx = rng.integers(0, npix, 12), rng.integers(0, npix, 12)
        img[ny, nx] = np.nan
        if npix > 20:
            img[15, 15] = img[16, 20] = img[0, 16] = np.nan          # at the seam and on the border
        vals, idx = _check_peaks(lens, dev, img)
        assert not np.isnan(vals).any()
        hit = np.zeros((npix, npix), dtype=bool)
        hit.ravel()[idx] = True
        for y, x in zip(ny, nx):                                     # neither a nan pixel nor any of its neighbours
            assert not hit[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].any()
        # -inf background, finite peaks, one isolated +inf
        bg = np.full((npix, npix), -INF, dtype=dtype)
        bg[1, 1] = -1e30
        if npix > 20:
            bg[15, 16] = 3.0
            bg[20, 5] = INF
            bg[25, 25] = bg[25, 26] = 7.0
        vals, idx = _check_peaks(lens, dev, bg)                       # hi = inf: "< hi" drops the +inf pixel
        assert idx.tolist() == ([npix + 1, 15 * npix + 16] if npix > 20 else [npix + 1])
        _check_peaks(lens, dev, bg, lo=-INF, hi=0.0)
        _check_peaks(lens, dev, bg, lo=0.0, hi=INF)


def test_thresholds_on_exact_peak_heights(lens, dev):
    rng = np.random.default_rng(8)
    for npix in (18, 33, 257):
        img = rng.standard_normal((npix, npix))
        heights = np.sort(_check_peaks(lens, dev, img)[0])
        assert len(heights) >= 8
        lo, hi = heights[2], heights[-3]
        vals, _ = _check_peaks(lens, dev, img, lo, hi)
        assert lo in vals and hi not in vals and len(vals) == len(heights) - 2 - 3      # >= lo kept, < hi dropped
        vals, _ = _check_peaks(lens, dev, img, np.nextafter(lo, INF), np.nextafter(hi, INF))
        assert lo not in vals and hi in vals
        for lo2, hi2 in ((hi, lo), (lo, lo), (INF, -INF), (np.nan, INF), (-INF, np.nan)):
            assert len(_check_peaks(lens, dev, img, lo2, hi2)[0]) == 0


def test_float64_thresholds_between_float32_values(lens, dev):
    """The thresholds stay float64: one just above a float32 peak height (not a float32 number) drops that peak."""
    rng = np.random.default_rng(9)
    img = rng.standard_normal((65, 65)).astype(np.float32)
    heights = np.sort(_check_peaks(lens, dev, img)[0])
    h = heights[len(heights) // 2]
    up, down = np.nextafter(np.float64(h), INF), np.nextafter(np.float64(h), -INF)
    assert np.float32(up) == h and np.float32(down) == h and up != np.float64(h)
    n_all = len(heights)
    below = int((heights < h).sum())
    assert len(_check_peaks(lens, dev, img, lo=np.float64(h))[0]) == n_all - below
    assert len(_check_peaks(lens, dev, img, lo=up)[0]) == n_all - below - 1
    assert len(_check_peaks(lens, dev, img, lo=down)[0]) == n_all - below
    assert len(_check_peaks(lens, dev, img, hi=np.float64(h))[0]) == below
    assert len(_check_peaks(lens, dev, img, hi=up)[0]) == below + 1
    assert len(_check_peaks(lens, dev, img, hi=down)[0]) == below


def test_values_that_differ_in_float64_and_tie_in_float32(lens, dev):
    npix = 40
    img = np.zeros((npix, npix))
    spots = [(5, 5), (15, 15), (15, 30), (31, 16), (36, 36)]
    for k, (y, x) in enumerate(spots):
        img[y, x] = 1.0 + k + 1e-10                  # a peak in float64 ...
        img[y + (k % 2), x + 1] = 1.0 + k            # ... beside a neighbour that float32 cannot tell from it
    assert np.array_equal(img.astype(np.float32)[5, 5], img.astype(np.float32)[5, 6])
    v64, i64 = _check_peaks(lens, dev, img)
    v32, i32 = _check_peaks(lens, dev, img.astype(np.float32))
    assert sorted(i64.tolist()) == sorted(y * npix + x for y, x in spots) and len(i32) == 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("npix,npeaks,cap", [(129, 4096, 2080), (257, 16384, 8256)])
def test_more_peaks_than_the_first_buffer_holds(lens, dev, hip, monkeypatch, npix, npeaks, cap, dtype):
    """A peak on every odd (y, x): the count passes the first capacity and peak_find runs again with the count."""
    rng = np.random.default_rng(npix)
    img = np.zeros((npix, npix), dtype=dtype)
    img[1::2, 1::2] = (1.0 + rng.permutation(npeaks)).reshape(npix // 2, npix // 2)
    assert max(1024, npix * npix // 8) == cap < npeaks
    calls = []
    real = hip.ast_peak_find

    def spy(*args):
        calls.append(int(args[5]))
        return real(*args)

    monkeypatch.setattr(hip, "ast_peak_find", spy)
    vals, idx = _check_peaks(lens, dev, img)
    assert len(vals) == npeaks and calls == [cap, npeaks]
    del calls[:]
    lo, hi = np.percentile(vals.astype(np.float64), 30), np.percentile(vals.astype(np.float64), 70)
    vals, idx = _check_peaks(lens, dev, img, lo, hi)
    assert 0 < len(vals) < cap and calls == [cap]


# ============================================================ order statistics
def _check_order(lens, dev, arr, ks):
    ks = [int(k) for k in ks]
    got = np.array(lens.order_statistics(dev.as_device(arr), ks), dtype=np.float64)
    ref = np.sort(arr)[ks].astype(np.float64)
    assert np.array_equal(got, ref), (arr.dtype, len(arr), [(k, g, r) for k, g, r in zip(ks, got, ref) if g != r][:5])
    return got


def _ulp_ladder(dtype, n, rng):
    """n distinct numbers that differ in the lowest mantissa bits only, shuffled."""
    bits = np.int64 if dtype == np.float64 else np.int32
    base = np.array([1.7], dtype=dtype).view(bits)[0]
    return rng.permutation((base + np.arange(n, dtype=bits)).view(dtype))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_order_statistics_every_k_on_small_arrays(lens, dev, dtype):
    rng = np.random.default_rng(21)
    tiny = np.finfo(dtype).smallest_subnormal
    arrays = [rng.standard_normal(n).astype(dtype) for n in (1, 2, 7, 255, 256, 257, 1000)]
    arrays += [np.full(300, 0.25, dtype=dtype),                                     # constant
               rng.integers(-2, 3, 777).astype(dtype),                              # heavy duplicates
               np.array([4.0], dtype=dtype),                                        # count == 1
               np.array([0.0, -0.0, INF, -INF, tiny, -tiny, 1.0, -1.0, 0.0, -0.0, tiny], dtype=dtype),
               (rng.integers(-40, 41, 500) * tiny).astype(dtype),                   # subnormals, both signs, duplicates
               np.concatenate([rng.integers(-40, 41, 300) * tiny, rng.standard_normal(301) * 1e-30]).astype(dtype),
               _ulp_ladder(dtype, 600, rng),                                        # the last radix passes decide
               -_ulp_ladder(dtype, 513, rng),
               np.array([np.finfo(dtype).max, -np.finfo(dtype).max, np.finfo(dtype).tiny, INF, -INF] * 3, dtype=dtype)]
    for arr in arrays:
        n = len(arr)
        _check_order(lens, dev, arr, range(n))
        ks = rng.integers(0, n, 9).tolist()
        _check_order(lens, dev, arr, ks + ks[::-1] + [n - 1, 0, 0, n - 1])           # unsorted and repeated
    sub = (np.arange(1, 6) * tiny).astype(dtype)
    got = _check_order(lens, dev, sub, range(5))
    assert (got > 0).all() and len(set(got.tolist())) == 5                          # subnormals are not flushed


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_order_statistics_spread_of_k_on_large_arrays(lens, dev, dtype):
    rng = np.random.default_rng(22)
    for n in ((1 << 20) + 37, 65537, 300 * 300):
        arr = rng.standard_normal(n).astype(dtype)
        arr[rng.integers(0, n, n // 50)] = arr[0]                                   # a heavy value
        ks = np.unique(np.concatenate([[0, 1, 2, n - 3, n - 2, n - 1], np.linspace(0, n - 1, 17).astype(np.int64)]))
        _check_order(lens, dev, arr, rng.permutation(np.concatenate([ks, ks[:4]])))
    arr = _ulp_ladder(dtype, 100003, rng)
    _check_order(lens, dev, arr, [0, 1, 255, 256, 50001, 100001, 100002])
    from astrild_amd._lib import AstrildHipError
    for bad in ([len(arr)], [0, len(arr) + 5], []):
        with pytest.raises(AstrildHipError):
            lens.order_statistics(dev.as_device(arr), bad)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_percentile_equals_numpy_on_finite_data(lens, dev, dtype):
    rng = np.random.default_rng(23)
    qs = [0, 5, 33.3, 50, 95, 100]
    for n in (1, 2, 3, 11, 101, 1000, 4097, 129 * 129):
        arr = rng.standard_normal(n).astype(dtype)
        if n > 10:
            arr[rng.integers(0, n, n // 5)] = arr[1]                                # duplicates around the quantiles
        on_element = [q for q in (1, 10, 20, 37, 50, 75, 99) if n in (11, 101) and (n - 1) * q % 100 == 0]
        for q in qs + on_element:
            got = lens.percentile(dev.as_device(arr), [q])[0]
            assert got == np.percentile(arr.astype(np.float64), q), (n, q)
        assert lens.percentile(dev.as_device(arr), qs) == [np.percentile(arr.astype(np.float64), q) for q in qs]
    arr = np.arange(101, dtype=dtype)[::-1].copy()
    assert lens.percentile(dev.as_device(arr), [37, 1, 99]) == [37.0, 1.0, 99.0]      # q lands on an element


# ============================================================ flat-sky spectra
THETA = 2.0
LF = 2 * np.pi / np.deg2rad(THETA)


def _sky(npix, seed=0):
    rng = np.random.default_rng(100 + npix + seed)
    g = ok.gaussian_smooth(rng.standard_normal((npix, npix)), THETA, 6.0 * 32 / npix, kind="gaussianFFT")
    g = g / g.std()
    return g + 0.5 * g ** 2 + 0.3                                                   # skewed, with a mean


def _issue_edges(npix):
    return LF * np.array([0.5, 1, 2, 3, 5, 8, 12, 16.5, 21, 0.75 * npix])


def _check_power(lens, img, edges, img2=None, theta=THETA):
    l, p = lens.flat_power_spectrum(img, theta, edges, img2=img2)
    rl, rp = ok.flat_power_spectrum(img, theta, edges, img2=img2)
    assert np.array_equal(l, rl)
    npt.assert_allclose(p, rp, rtol=1e-12, atol=1e-14 * np.abs(rp).max())
    return p, rp


@pytest.mark.parametrize("npix", [31, 32, 33, 63, 64])
def test_flat_power_and_bispectrum_on_odd_and_even_maps(lens, npix):
    img = _sky(npix)
    edges = _issue_edges(npix)
    p, rp = _check_power(lens, img, edges)
    assert (rp > 0).all()
    l, b, ntri = lens.flat_bispectrum_equilateral(img, THETA, edges)
    rl, rb, rn = ok.flat_bispectrum_equilateral_brute(img, THETA, edges)
    assert np.array_equal(l, rl)
    assert ntri.dtype == np.int64 and np.array_equal(ntri, rn)
    assert rn[0] == 0 and b[0] == 0.0 and (rn[1:7] > 0).all()       # (0.5, 1]: four pixels and no closed triangle
    npt.assert_allclose(b, rb, rtol=1e-9, atol=1e-12 * np.abs(rb).max())


@pytest.mark.parametrize("npix", [31, 64])
def test_flat_spectra_in_a_single_bin(lens, npix):
    img = _sky(npix, 1)
    for edges in (LF * np.array([2.0, 9.0]), LF * np.array([0.5, 1.0]), LF * np.array([npix, 2.0 * npix])):
        p, rp = (lens.flat_power_spectrum(img, THETA, edges)[1], ok.flat_power_spectrum(img, THETA, edges)[1])
        assert p.shape == (1,)
        npt.assert_allclose(p, rp, rtol=1e-12, atol=1e-14 * max(np.abs(rp).max(), 1e-300))
        l, b, ntri = lens.flat_bispectrum_equilateral(img, THETA, edges)
        rl, rb, rn = ok.flat_bispectrum_equilateral_brute(img, THETA, edges)
        assert b.shape == (1,) and np.array_equal(ntri, rn) and np.array_equal(l, rl)
        npt.assert_allclose(b, rb, rtol=1e-9, atol=1e-12 * np.abs(rb).max())
    assert lens.flat_power_spectrum(img, THETA, LF * np.array([npix, 2.0 * npix]))[1][0] == 0.0     # past the corner: empty


def test_flat_power_with_1024_bins_and_the_limit(lens):
    npix = 256
    img = _sky(npix, 2)
    edges = LF * np.linspace(0.37, 181.3, 1025)                     # the corner lies at 181.02
    # membership must not hang on the last bit of |l|: no pixel radius within 1e-9 of an edge
    radii = ok._pixel_l(npix, np.deg2rad(THETA)).ravel()
    k = np.clip(np.searchsorted(edges, radii), 1, len(edges) - 1)
    near = np.minimum(np.abs(radii - edges[k]), np.abs(radii - edges[k - 1])).min()
    assert near > 1e-9 * LF
    p, rp = _check_power(lens, img, edges)
    assert np.count_nonzero(rp) > 900 and (rp == 0).any()           # some of the fine bins hold no pixel
    assert np.array_equal(p == 0, rp == 0)
    from astrild_amd._lib import AstrildHipError
    with pytest.raises(AstrildHipError):
        lens.flat_power_spectrum(img, THETA, LF * np.linspace(0.37, 181.3, 1026))
    _check_power(lens, img, LF * np.linspace(0.37, 181.3, 1024))     # 1023 bins


@pytest.mark.parametrize("npix", [33, 64])
def test_flat_cross_power(lens, npix):
    img = _sky(npix, 3)
    edges = _issue_edges(npix)
    auto = lens.flat_power_spectrum(img, THETA, edges)[1]
    # the bin sums are atomic additions in no fixed order: equal to rounding, at P's tolerance, not bit for bit
    npt.assert_allclose(lens.flat_power_spectrum(img, THETA, edges, img2=img.copy())[1], auto, rtol=1e-12,
                        atol=1e-14 * auto.max())
    for shifted in (np.roll(img, 3, axis=0), np.roll(img, (1, -5), axis=(0, 1)), _sky(npix, 4)):
        l, p = lens.flat_power_spectrum(img, THETA, edges, img2=shifted)
        rp = ok.flat_power_spectrum(img, THETA, edges, img2=shifted)[1]
        # a cross power changes sign: the absolute floor is relative to the auto power, as in test_gpu_kappa.py
        npt.assert_allclose(p, rp, rtol=1e-12, atol=1e-14 * auto.max())
        assert not np.allclose(p, auto, rtol=1e-3, atol=0)


@pytest.mark.parametrize("npix", [31, 32])
def test_lowest_edge_at_and_below_zero(lens, npix):
    img = _sky(npix, 5)
    assert abs(img.mean()) > 0.1
    tail = LF * np.array([1.0, 2.5, 6.0])
    p0, _ = _check_power(lens, img, np.concatenate([[0.0], tail]))           # (0, ..]: the DC pixel is left out
    pm, _ = _check_power(lens, img, np.concatenate([[-1.0], tail]))          # (-1, ..]: it is in
    dc = (img.sum() ** 2) * (np.deg2rad(THETA) / npix ** 2) ** 2
    assert np.array_equal(p0[1:], pm[1:]) and pm[0] > 2 * p0[0]
    npt.assert_allclose(4 * pm[0], 3 * p0[0] + dc, rtol=1e-12)               # three half-plane pixels, and the DC one
    only_dc = lens.flat_power_spectrum(img, THETA, np.array([-1.0, 0.5 * LF]))[1]
    npt.assert_allclose(only_dc, [dc], rtol=1e-12)
    for edges in (np.concatenate([[0.0], tail]), np.concatenate([[-1.0], tail])):
        l, b, ntri = lens.flat_bispectrum_equilateral(img, THETA, edges)
        rl, rb, rn = ok.flat_bispectrum_equilateral_brute(img, THETA, edges)
        assert np.array_equal(ntri, rn)
        npt.assert_allclose(b, rb, rtol=1e-9, atol=1e-12 * np.abs(rb).max())


# ====================================== periodic smoothing around a small map
@pytest.mark.parametrize("npix,sigma_px", [(32, 5.0), (16, 2.5), (17, 4.0), (41, 18.8), (40, 18.8)])
def test_periodic_gaussian_passes_lap_a_small_map(lens, dev, monkeypatch, npix, sigma_px):
    """The taps reach 8.5 sigma: up to 160 pixels on a 40-pixel map, four laps.  Against the oracle at 1e-12 of the
    peak and against the FFT route at 2e-13 (both as in test_gpu_kappa.py)."""
    rng = np.random.default_rng(npix)
    img = rng.standard_normal((npix, npix))
    img[npix // 3, npix // 2] += 40.0
    plan = lens.SmoothPlan(npix)
    a = dev.as_device(img.copy())
    plan.gaussian(a, sigma_px, "gaussianFFT")
    monkeypatch.setenv("AST_SMOOTH_FFT", "1")
    b = dev.as_device(img.copy())
    plan.gaussian(b, sigma_px, "gaussianFFT")
    monkeypatch.delenv("AST_SMOOTH_FFT")
    a, b = a.cpu().numpy(), b.cpu().numpy()
    theta = 1.0
    ref = ok.gaussian_smooth(img, theta, sigma_px * 60.0 * theta / npix, kind="gaussianFFT")
    print(f"npix {npix} sigma {sigma_px}: |passes - oracle| / peak = {np.abs(a - ref).max() / np.abs(ref).max():.3e}, "
          f"|fft - oracle| / peak = {np.abs(b - ref).max() / np.abs(ref).max():.3e}, "
          f"|passes - fft| / peak = {np.abs(a - b).max() / np.abs(b).max():.3e}")
    assert not np.array_equal(a, b)                                # two different routes did run
    npt.assert_allclose(b, ref, rtol=0, atol=1e-12 * np.abs(ref).max())
    npt.assert_allclose(a, ref, rtol=0, atol=1e-12 * np.abs(ref).max())
    npt.assert_allclose(a, b, rtol=0, atol=2e-13 * np.abs(b).max())


def test_periodic_gaussian_beyond_the_weight_buffer_takes_the_fft_route(lens, dev, monkeypatch):
    npix, sigma_px = 39, 18.8                                      # 321 taps against room for 8 * 39 + 1 = 313
    rng = np.random.default_rng(npix)
    img = rng.standard_normal((npix, npix))
    plan = lens.SmoothPlan(npix)
    a = dev.as_device(img.copy())
    plan.gaussian(a, sigma_px, "gaussianFFT")
    monkeypatch.setenv("AST_SMOOTH_FFT", "1")
    b = dev.as_device(img.copy())
    plan.gaussian(b, sigma_px, "gaussianFFT")
    monkeypatch.delenv("AST_SMOOTH_FFT")
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(a, b)                                    # the same route both times
    ref = ok.gaussian_smooth(img, 1.0, sigma_px * 60.0 / npix, kind="gaussianFFT")
    npt.assert_allclose(a, ref, rtol=0, atol=1e-12 * np.abs(ref).max())


# ============================================================ histogram limits
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nbins", [1, 4096])
def test_histogram_with_the_fewest_and_the_most_bins(lens, dev, dtype, nbins):
    rng = np.random.default_rng(nbins)
    for n in (1, 1000, 300 * 300 + 3):
        img = (rng.standard_normal(n) * 0.01).astype(dtype)
        t = dev.as_device(img)
        counts, edges = lens.histogram(t, nbins)
        rc, re = np.histogram(img.astype(np.float64), bins=nbins)
        assert np.array_equal(counts, rc) and np.array_equal(edges, re) and counts.sum() == n
        counts, edges = lens.histogram(t, nbins, range=(-0.011, 0.0173))
        rc, re = np.histogram(img.astype(np.float64), bins=nbins, range=(-0.011, 0.0173))
        assert np.array_equal(counts, rc) and np.array_equal(edges, re)
    # values on the edges of 4096 bins
    grid = np.linspace(-1.0, 1.0, 4097).astype(dtype)
    counts, _ = lens.histogram(dev.as_device(grid), nbins, range=(-1.0, 1.0))
    assert np.array_equal(counts, np.histogram(grid.astype(np.float64), bins=nbins, range=(-1.0, 1.0))[0])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_histogram_bin_count_out_of_range_raises(lens, dev, dtype):
    from astrild_amd._lib import AstrildHipError
    t = dev.as_device(np.arange(100, dtype=dtype))
    for nbins in (4097, 0):
        with pytest.raises(AstrildHipError):
            lens.histogram(t, nbins)
        with pytest.raises(AstrildHipError):
            lens.histogram(t, nbins, range=(0.0, 50.0))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_histogram_with_a_range_ignores_nan_and_infinite_pixels(lens, dev, dtype):
    rng = np.random.default_rng(31)
    img = rng.standard_normal(5003).astype(dtype)
    img[rng.integers(0, 5003, 40)] = np.nan
    img[rng.integers(0, 5003, 40)] = INF
    img[rng.integers(0, 5003, 40)] = -INF
    img[:3] = [np.nan, INF, -INF]
    for nbins, rng_ in ((1, (-0.5, 0.5)), (17, (-1.0, 2.0)), (4096, (-4.0, 4.0))):
        counts, _ = lens.histogram(dev.as_device(img), nbins, range=rng_)
        with np.errstate(invalid="ignore"):
            rc = np.histogram(img.astype(np.float64), bins=nbins, range=rng_)[0]
        assert np.array_equal(counts, rc) and counts.sum() <= np.isfinite(img).sum()
