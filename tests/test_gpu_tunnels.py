"""GPU: the tunnels void finder (ast_tunnels_find through device.tunnels_voids and rays.voids.TunnelsFinder): the sorted
integer records exactly equal to the oracle (tests/tunnels_oracle.py: scipy's Delaunay triangulation merged by exact
circle) with no violations, on random, gridded, clustered, border and degenerate tracer sets, the peaks of a smoothed
field, the single-cell switch, repeat stability, device tensors, the int64 bound at npix = 16384, the errors raised
before any launch, and the chain map -> peaks -> voids -> profiles from one SkyArray."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import profile2d_oracle as porc
from tests import tunnels_oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


def distinct(rs, n, npix):
    p = rs.permutation(npix * npix)[:n]
    return np.stack([p % npix, p // npix], axis=1)


def lattice_with_holes():
    return np.array([(x, y) for x in range(0, 36, 5) for y in range(0, 36, 5) if (7 * x + 3 * y) % 11 != 0])


def full_lattice():
    return np.array([(x, y) for x in range(6) for y in range(7)])


def clustered():
    rs = np.random.RandomState(7)
    far = distinct(rs, 60, 2048)
    far = far[(far[:, 0] >= 64) | (far[:, 1] >= 64)][:30]
    return np.concatenate([distinct(rs, 3000, 64), far])


def border(npix=256):
    b = np.arange(0, npix, 3)
    top = npix - 1
    edge = np.concatenate([np.stack([b, 0 * b], 1), np.stack([b, 0 * b + top], 1), np.stack([0 * b, b], 1),
                           np.stack([0 * b + top, b], 1), distinct(np.random.RandomState(8), 100, npix)])
    return np.unique(edge, axis=0)


def smooth_field(npix=1024):
    from scipy.ndimage import gaussian_filter
    return gaussian_filter(np.random.RandomState(3).standard_normal((npix, npix)), 2.0, mode="wrap")


def gpu(P, npix):
    from astrild_amd import device as dev
    P = np.asarray(P)
    rec, violations = dev.tunnels_voids(P[:, 0], P[:, 1], npix, return_violations=True)
    assert violations == 0
    assert rec.dtype == np.int64 and rec.shape[1] == 7
    return rec


def check(P, npix):
    want = orc.circles(P, npix)
    npt.assert_array_equal(gpu(P, npix), want)
    return want


def test_random_tracers():
    want = check(distinct(np.random.RandomState(11), 2000, 512), 512)
    assert len(want) > 3000


def test_peaks_of_a_smoothed_field():
    x, y = orc.strict_maxima(smooth_field())
    assert len(x) == 11424
    want = check(np.stack([x, y], axis=1), 1024)
    assert int((want[:, 3] > 3).sum()) >= 10             # peaks sit on a pixel grid: cocircular sets are not rare


def test_lattices():
    want = check(lattice_with_holes(), 36)
    assert 2 * int((want[:, 3] > 3).sum()) > len(want)
    want = check(full_lattice(), 7)
    assert len(want) == 30 and np.all(want[:, 3] == 4)
    fine = np.array([(x, y) for x in range(0, 128, 2) for y in range(0, 128, 2)])
    assert len(check(fine, 128)) == 63 * 63


def test_clustered_tracers_with_long_hull_walks():
    P = clustered()
    assert len(P) == 3030
    want = check(P, 2048)
    cx, cy, r = orc.floats(want, P[:, 0], P[:, 1])
    assert r.max() > 300 and np.median(r) < 3


def test_tracers_on_the_border():
    P = border()
    assert (P[:, 0] == 0).sum() > 50 and (P[:, 1] == 255).sum() > 50
    check(P, 256)


def test_three_two_and_collinear_tracers():
    want = check(np.array([(0, 0), (5, 1), (2, 7)]), 8)
    assert len(want) == 1 and tuple(want[0, :4]) == (0, 1, 2, 3)
    assert gpu(np.array([(1, 1), (5, 2)]), 16).shape == (0, 7)
    assert gpu(np.array([(x, 2 * x) for x in range(500)]), 1024).shape == (0, 7)
    assert gpu(np.array([(x, 7) for x in range(0, 1000, 3)]), 1024).shape == (0, 7)
    check(np.array([(x, 3) for x in range(0, 200, 2)] + [(70, 90)]), 256)


@pytest.mark.parametrize("which", ["random", "holes", "field"])
def test_single_cell_against_the_grid(which, monkeypatch):
    if which == "random":
        P, npix = distinct(np.random.RandomState(12), 1500, 400), 400
    elif which == "holes":
        P, npix = lattice_with_holes(), 36
    else:
        x, y = orc.strict_maxima(smooth_field(256))
        P, npix = np.stack([x, y], axis=1), 256
    grid = check(P, npix)
    monkeypatch.setenv("ASTRILD_TUNNELS_CELLS", "0")
    npt.assert_array_equal(gpu(P, npix), grid)


def test_bit_identical_on_repeat():
    P = distinct(np.random.RandomState(13), 5000, 1024)
    a, b = gpu(P, 1024), gpu(P, 1024)
    assert a.tobytes() == b.tobytes()


def test_device_tensor_in_and_out():
    from astrild_amd import device as dev
    P = distinct(np.random.RandomState(14), 1000, 300)
    x, y = dev.as_device(P[:, 0].copy()), dev.as_device(P[:, 1].astype(np.int32))
    rec = dev.tunnels_voids(x, y, 300)
    assert isinstance(rec, torch.Tensor) and rec.is_cuda and rec.dtype == torch.int64
    want = orc.circles(P, 300)
    npt.assert_array_equal(rec.cpu().numpy(), want)
    for a, b in zip(dev.tunnels_circles(rec, x, y), orc.floats(want, P[:, 0], P[:, 1])):
        assert a.tobytes() == b.tobytes()


def test_largest_map_with_tracers_in_all_corners():
    """npix = 16384: coordinate differences of 2^14 - 1, the bound that keeps the in-circle determinant in int64."""
    from astrild_amd import _lib
    assert _lib.lib().ast_tunnels_max_npix() == 16384
    top = 16383
    rs = np.random.RandomState(15)
    P = np.concatenate([[(0, 0), (top, 0), (0, top), (top, top), (8000, 8100), (3, 16000), (top, 5)],
                        distinct(rs, 200, 16384)])
    P = np.unique(P, axis=0)
    check(P, 16384)
    want = check(np.array([(0, 0), (top, 0), (0, top), (top, top)]), 16384)
    assert len(want) == 1 and want[0, 3] == 4 and want[0, 6] == 2 * top * top and want[0, 4] > 1 << 41


@pytest.mark.parametrize("x,y,npix", [([1.0, 2.0, 3.0], [1, 2, 3], 16), ([1, 2, 16], [1, 2, 3], 16),
                                      ([1, 2, 3], [-1, 2, 3], 16), ([1, 2, 1, 7], [5, 2, 5, 7], 16),
                                      ([1, 2, 3], [1, 2, 4], 16385)])
def test_errors_before_any_launch(x, y, npix, monkeypatch):
    from astrild_amd import _lib, device as dev
    lib = _lib.lib()

    def no_launch(*a):
        raise AssertionError("ast_tunnels_find must not be called")

    monkeypatch.setattr(lib, "ast_tunnels_find", no_launch)
    with pytest.raises(ValueError):
        dev.tunnels_voids(np.asarray(x), np.asarray(y), npix)
    with pytest.raises(ValueError):
        dev.tunnels_voids(dev.as_device(np.asarray(x)), dev.as_device(np.asarray(y)), npix)


def test_map_to_peaks_to_voids_to_profiles():
    """One SkyArray, no file and no external program: find_peaks, find_voids at three thresholds, Voids.get_profiles."""
    from scipy.spatial import cKDTree
    from astrild_amd.rays.skys.sky_array import SkyArray
    from astrild_amd.rays.void import Voids
    from astrild_amd.rays.voids import TunnelsFinder
    npix, angle, extend, nbins = 1024, 10.0, 2.0, 10
    kappa = 0.02 * smooth_field(npix) / smooth_field(npix).std()
    sky = SkyArray.from_array(kappa.copy(), angle, "kappa_2", "/data")
    finder = TunnelsFinder(sky)
    finder.find_peaks("orig", "normalize", {"on": "orig", "nbins": 100})
    x_all, y_all = orc.strict_maxima(kappa)
    assert 0 < len(x_all) - len(finder.peaks["kappa"]) < 10         # all but the few at and above the top threshold
    snrs = [1.0, 2.0, 3.0]
    finder.find_voids(snrs)
    import pandas as pd
    voids, peaks = orc.frames(finder.peaks, snrs, npix, angle)
    pd.testing.assert_frame_equal(finder.voids_df, voids, check_exact=True)
    pd.testing.assert_frame_equal(finder.peaks_df, peaks, check_exact=True)
    for nu in snrs:
        sel = finder.peaks["snr"] > nu
        assert sel.sum() >= 3
        pos = np.rint(finder.peaks["pos"][sel] * npix / angle)
        rec = finder.void_records[nu]
        cx, cy, r = orc.floats(rec, pos[:, 0].astype(int), pos[:, 1].astype(int))
        tree = cKDTree(pos)
        centres = np.stack([cx, cy], axis=1)
        # fp64 errors of cx, cy, r and of a distance are ~1e-12 px at npix = 1024; a tracer off the circle has
        # |d - r| > 2e-10 px (|d^2 - r^2| >= 1 / |D|, |D| < 2 * 1024^2, r <= 1024): 1e-10 lies between the two
        inside = tree.query_ball_point(centres, r - 1e-10, return_length=True)
        upto = tree.query_ball_point(centres, r + 1e-10, return_length=True)
        assert np.all(inside == 0) and np.all(upto >= 3)
        npt.assert_array_equal(upto, rec[:, 3])
    assert len(finder.void_records[1.0]) > len(finder.void_records[2.0]) > len(finder.void_records[3.0]) > 10

    v = Voids("/data/tunnels.h5", finder.voids_df, {"name": "tunnels", "sigmas": {"name": "sigma", "values": snrs}},
              {"npix": npix})
    v.get_profiles(extend, nbins, skymap=kappa, field_conversion="normalize")
    df = voids
    reach = extend * df["rad_pix"].values
    keep = df[(df["theta1_pix"].values + reach < npix) & (df["theta1_pix"].values - reach > 0)
              & (df["theta2_pix"].values + reach < npix) & (df["theta2_pix"].values - reach > 0)].reset_index()
    keep = keep[extend * keep["rad_pix"] > 10].reset_index()
    assert len(keep) > 100
    npt.assert_array_equal(v.data["x_pix"].values, keep["x_pix"].values)
    npt.assert_array_equal(v.data["sigma"].values, keep["sigma"].values)
    norm = kappa - np.mean(kappa)
    xs, ys, rs = keep["x_pix"].values, keep["y_pix"].values, keep["rad_pix"].values
    values, _, counts, radii = porc.from_map(xs, ys, rs, norm, extend, nbins)
    a = porc.from_map(xs, ys, rs, np.abs(norm), extend, nbins)[1]
    tol = np.array([porc.aligned(ai, ci) for ai, ci in zip(a, counts)]) * 1e-12
    fin = np.isfinite(values)
    npt.assert_array_equal(v.profiles["radii"], radii)
    npt.assert_array_equal(np.isfinite(v.profiles["values"]), fin)
    assert np.all(np.abs(v.profiles["values"][fin] - values[fin]) <= tol[fin])
    res = v.get_profile_stats(cats=["sigma"])
    assert res["mean"].shape == (3, nbins) and np.all(res["nr_of_obj"] > 0)
