"""CPU: the oracle of the tunnels void finder (tests/tunnels_oracle.py) - scipy's Delaunay triangulation merged by exact
circle against an O(N^4) enumeration with Python integers, degenerate sets included - the host logic of
rays.voids.TunnelsFinder with the device calls replaced by the oracle, and the argument checks of device.tunnels_voids
that need no GPU."""
import types

import numpy as np
import numpy.testing as npt
import pandas as pd
import pytest

from tests import tunnels_oracle as orc


def distinct(rs, n, npix):
    p = rs.permutation(npix * npix)[:n]
    return np.stack([p % npix, p // npix], axis=1)


def lattice_with_holes():
    return np.array([(x, y) for x in range(0, 36, 5) for y in range(0, 36, 5) if (7 * x + 3 * y) % 11 != 0])


def full_lattice():
    return np.array([(x, y) for x in range(6) for y in range(7)])


CASES = {
    "random": (distinct(np.random.RandomState(1), 50, 300), 300),
    "lattice_with_holes": (lattice_with_holes(), 36),
    "full_lattice": (full_lattice(), 7),
    "dense_12": (distinct(np.random.RandomState(2), 50, 12), 12),
    "row_plus_one": (np.array([(x, 3) for x in range(0, 20, 2)] + [(7, 9)]), 20),
    "three": (np.array([(0, 0), (5, 1), (2, 7)]), 8),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_circles_equal_brute_force(name):
    P, npix = CASES[name]
    got = orc.circles(P, npix)
    npt.assert_array_equal(got, orc.brute(P, npix))
    assert got.dtype == np.int64 and got.shape[1] == 7 and len(got) >= 1
    assert np.all(got[:, 3] >= 3) and np.all(got[:, 6] > 0)
    assert np.all(got[:, 0] < got[:, 1]) and np.all(got[:, 0] < got[:, 2])


def test_lattice_with_holes_is_mostly_degenerate():
    """The cocircular path cannot pass by being absent: more than half of the circles carry more than three tracers."""
    rec = orc.circles(lattice_with_holes(), 36)
    assert 2 * int((rec[:, 3] > 3).sum()) > len(rec)
    full = orc.circles(full_lattice(), 7)
    assert len(full) == 5 * 6 and np.all(full[:, 3] == 4)


def test_no_voids_without_a_triangle():
    assert orc.circles(np.array([(x, 2 * x) for x in range(8)]), 16).shape == (0, 7)
    assert orc.circles(np.array([(1, 1), (5, 2)]), 16).shape == (0, 7)
    assert orc.brute(np.array([(x, 2 * x) for x in range(8)]), 16).shape == (0, 7)


def test_centre_outside_the_map_is_dropped():
    """A flat triangle along the lower edge has its centre far below the map; raised to the middle it stays."""
    assert len(orc.circles(np.array([(0, 0), (10, 1), (20, 0)]), 32)) == 0
    rec = orc.circles(np.array([(5, 10), (15, 5), (25, 10)]), 32)
    assert len(rec) == 1
    cx, cy, r = orc.floats(rec, [5, 15, 25], [10, 5, 10])
    assert cx[0] == 15.0 and cy[0] == 17.5 and r[0] == 12.5


def test_host_floats_are_the_oracles():
    """device.tunnels_circles forms centre and radius with the oracle's expressions, bit for bit."""
    from astrild_amd import device as dev
    P, npix = CASES["random"]
    rec = orc.circles(P, npix)
    for a, b in zip(dev.tunnels_circles(rec, P[:, 0], P[:, 1]), orc.floats(rec, P[:, 0], P[:, 1])):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ TunnelsFinder on the host
class HostStore(dict):
    """SkyArray.data without a device: ``device(name)`` hands out the array itself."""
    def device(self, key):
        return self[key]


def host_peak_find(t, lo=-np.inf, hi=np.inf):
    """lensing.peak_find in numpy: heights and flat indices of the strict maxima, row-major order."""
    t = np.asarray(t)
    x, y = orc.strict_maxima(t)
    keep = (t[y, x] >= lo) & (t[y, x] < hi)
    return t[y, x][keep], (y * t.shape[0] + x)[keep]


def smooth_map(npix, seed, sigma=2.0):
    from scipy.ndimage import gaussian_filter
    return gaussian_filter(np.random.RandomState(seed).standard_normal((npix, npix)), sigma, mode="wrap")


@pytest.fixture
def finder(monkeypatch):
    from astrild_amd import device as dev, lensing
    from astrild_amd.rays.voids import TunnelsFinder
    monkeypatch.setattr(lensing, "peak_find", host_peak_find)
    monkeypatch.setattr(dev, "tunnels_voids", lambda x, y, npix: orc.circles(np.stack([x, y], axis=1), npix))
    npix, angle = 128, 3.5
    kappa = smooth_map(npix, 5)
    skymap = types.SimpleNamespace(data=HostStore(orig=kappa), npix=npix, opening_angle=angle, map_file=None,
                                   quantity="kappa_2")
    return TunnelsFinder(skymap), kappa, npix, angle


def test_find_peaks_thresholds_snr_and_edge_buffer(finder):
    f, kappa, npix, angle = finder
    thr = f._get_convergence_thresholds(on="orig", nbins=50)
    step = (kappa.max() - kappa.min()) / 50
    npt.assert_array_equal(thr, np.arange(kappa.min(), kappa.max(), step))
    f.find_peaks("orig", "normalize", {"on": "orig", "nbins": 50})
    norm = kappa - np.mean(kappa)
    heights, index = host_peak_find(norm)
    keep = (heights >= thr[0]) & (heights < thr[-1])
    assert 0 < keep.sum() < len(keep)                       # the top threshold cuts the highest peak
    npt.assert_array_equal(f.peaks["kappa"], heights[keep])
    npt.assert_array_equal(f.peaks["pos"][:, 0], (index[keep] % npix) * (angle / npix))
    npt.assert_array_equal(f.peaks["pos"][:, 1], (index[keep] // npix) * (angle / npix))
    npt.assert_array_equal(f.peaks["snr"], heights[keep] / np.std(norm))
    f.find_peaks("orig", "normalize", {"on": "orig", "nbins": 50}, snr_sigma=0.25)
    npt.assert_array_equal(f.peaks["snr"], heights[keep] / 0.25)
    # raw heights without "normalize"
    f.find_peaks("orig", None, {"on": "orig", "nbins": 50})
    raw, rindex = host_peak_find(kappa)
    rkeep = (raw >= thr[0]) & (raw < thr[-1])
    npt.assert_array_equal(f.peaks["kappa"], raw[rkeep])
    npt.assert_array_equal(f.peaks["snr"], raw[rkeep] / np.std(kappa))
    # a buffer of ceil(10 arcmin / pixel) pixels: pixel = 3.5 deg / 128 = 1.640625 arcmin -> 7 pixels
    f.find_peaks("orig", None, {"on": "orig", "nbins": 50}, smoothing_length=10.0)
    x, y = rindex[rkeep] % npix, rindex[rkeep] // npix
    inside = (x >= 7) & (x <= npix - 1 - 7) & (y >= 7) & (y <= npix - 1 - 7)
    assert 0 < inside.sum() < len(inside)
    npt.assert_array_equal(f.peaks["kappa"], raw[rkeep][inside])


def test_find_voids_frames_records_and_concatenation(finder):
    f, kappa, npix, angle = finder
    f.find_peaks("orig", "normalize", {"on": "orig", "nbins": 50})
    snrs = [0.5, 1.5, 100.0, 2.5]                           # 100: no peak is left
    assert (f.peaks["snr"] > 2.5).sum() >= 3 and (f.peaks["snr"] > 100.0).sum() == 0
    f.find_voids(snrs, dir_temp="/nonexistent")
    voids, peaks = orc.frames(f.peaks, snrs, npix, angle)
    assert list(f.voids_df.columns) == ["x_deg", "x_pix", "y_deg", "y_pix", "rad_deg", "rad_pix", "sigma", "theta1_pix",
                                        "theta2_pix"]
    assert list(f.peaks_df.columns) == ["x_deg", "x_pix", "y_deg", "y_pix", "sigma", "rad_deg", "rad_pix"]
    pd.testing.assert_frame_equal(f.voids_df, voids, check_exact=True)
    pd.testing.assert_frame_equal(f.peaks_df, peaks, check_exact=True)
    for c in ("x_pix", "y_pix", "rad_pix"):
        assert f.voids_df[c].dtype == np.int64 and f.peaks_df[c].dtype == np.int64
    for c in ("x_deg", "y_deg", "rad_deg", "sigma"):
        assert f.voids_df[c].dtype == np.float64 and f.peaks_df[c].dtype == np.float64
    assert sorted(f.voids_df["sigma"].unique()) == [0.5, 1.5, 2.5]
    assert sorted(f.void_records) == sorted(snrs) and f.void_records[100.0].shape == (0, 7)
    assert len(f.void_records[0.5]) == (f.voids_df["sigma"] == 0.5).sum() > (f.voids_df["sigma"] == 2.5).sum() > 0
    assert len(f.peaks_orig_df) == len(f.peaks["snr"])
    p2, v2 = f.find_voids(snrs, rtn=True)
    pd.testing.assert_frame_equal(v2, voids, check_exact=True)
    pd.testing.assert_frame_equal(p2, peaks, check_exact=True)


def test_find_voids_with_no_void_at_all_gives_empty_typed_frames(finder):
    f, kappa, npix, angle = finder
    f.find_peaks("orig", "normalize", {"on": "orig", "nbins": 50})
    f.find_voids([100.0])
    assert len(f.voids_df) == 0 and len(f.peaks_df) == 0
    assert "rad_pix" in f.voids_df.columns and f.voids_df["rad_pix"].dtype == np.int64
    assert "rad_deg" in f.peaks_df.columns and f.peaks_df["rad_deg"].dtype == np.float64


def test_set_peak_radii_is_the_distance_to_the_nearest_void(finder):
    f, kappa, npix, angle = finder
    peaks = pd.DataFrame({"x_deg": [0.0, 1.0, 3.0], "y_deg": [0.0, 1.0, 3.0]})
    voids = pd.DataFrame({"x_deg": [0.0, 3.0], "y_deg": [1.0, 2.5]})
    out = f.set_peak_radii(peaks, voids, npix, angle)
    npt.assert_array_equal(out["rad_deg"].values, [1.0, 1.0, 0.5])
    npt.assert_array_equal(out["rad_pix"].values, np.rint(np.array([1.0, 1.0, 0.5]) * (npix / angle)).astype(int))


# ------------------------------------------------------------------ argument checks that need no GPU
@pytest.mark.parametrize("x,y,npix,match", [
    ([1.0, 2.0, 3.0], [1, 2, 3], 16, "integer"),
    ([1, 2, 3], np.array([1.5, 2, 3]), 16, "integer"),
    ([1, 2, 16], [1, 2, 3], 16, "lie in"),
    ([1, 2, 3], [-1, 2, 3], 16, "lie in"),
    ([1, 2, 1, 7], [5, 2, 5, 7], 16, "duplicate"),
    ([1, 2, 3], [1, 2], 16, "one entry per tracer"),
    ([1, 2, 3], [1, 2, 4], 0, "npix"),
])
def test_errors_before_the_library_is_touched(x, y, npix, match, monkeypatch):
    from astrild_amd import _lib, device as dev

    def no_library():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(ValueError, match=match):
        dev.tunnels_voids(np.asarray(x), np.asarray(y), npix)


def test_npix_above_the_int64_bound_is_refused_without_a_launch(monkeypatch):
    from astrild_amd import _lib, device as dev
    lib = _lib.lib()
    assert lib.ast_tunnels_max_npix() == 16384
    assert lib.ast_tunnels_workspace_bytes(1000, 16385) == 0 and lib.ast_tunnels_workspace_bytes(1000, 16384) > 0

    def no_launch(*a):
        raise AssertionError("ast_tunnels_find must not be called")

    monkeypatch.setattr(lib, "ast_tunnels_find", no_launch)
    with pytest.raises(ValueError, match="16384"):
        dev.tunnels_voids(np.array([0, 5, 9]), np.array([0, 7, 1]), 16385)
