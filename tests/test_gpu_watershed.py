"""GPU: the watershed void finder (ast_watershed_* through device.watershed_basins / watershed_void_map and
rays.voids.WatershedFinder) against tests/watershed_oracle.py.  Everything integer - labels, minima, area, sum_x, sum_y,
edge_pix, edges, the void maps of every threshold - equals the oracle exactly; saddle and f_min equal it bit for bit;
sum_f agrees within (A - 1) 2^-53 sum|f| per basin, the worst case of float64 addition in any order (the oracle's sum
is exactly rounded).  Shapes: the snake (one basin, link paths of 144, 544 and 2112 links: more than 2^11), smoothed
noise on one ragged tile, on whole tiles and on several tiles with a ragged edge, plateaus, float32 ties, dirty
scratch memory, device tensors, the errors, and the chain map -> filter -> voids -> profiles."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

from tests import profile2d_oracle as porc
from tests import watershed_oracle as orc
from tests.dirty_memory import HUGE_BYTES, NAN_BYTES, PATTERN_IDS, ZERO_BYTES, dirty

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

INT_KEYS = ("labels", "minima", "area", "sum_x", "sum_y", "edge_pix", "edges")
BIT_KEYS = ("saddle", "f_min")
DTYPES = {"labels": np.int32, "minima": np.int64, "area": np.int64, "sum_x": np.int64, "sum_y": np.int64,
          "edge_pix": np.int64, "edges": np.int32, "sum_f": np.float64}

MAPS = {
    "snake17": lambda: orc.snake(17),
    "snake33": lambda: orc.snake(33),
    "snake65": lambda: orc.snake(65),
    "noise33": lambda: orc.smoothed_noise(33),
    "noise64": lambda: orc.smoothed_noise(64),
    "noise130": lambda: orc.smoothed_noise(130),
    "noise64_f32": lambda: orc.smoothed_noise(64, dtype=np.float32),
    "constant40": lambda: np.full((40, 40), 0.75),
    "blocks40": lambda: orc.blocks(40, 8),
    "ties_f32": lambda: orc.float32_ties().astype(np.float32),
    "ties_f64": lambda: orc.float32_ties(),
}


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


@functools.lru_cache(maxsize=None)
def case(name):
    """(map, the oracle's basins), computed once and read only."""
    f = MAPS[name]()
    return f, orc.basins(f)


def compare(got, f, want):
    assert sorted(got) == sorted(k for k in want if k != "sum_abs_f")
    for k in INT_KEYS:
        assert got[k].dtype == DTYPES[k], k
        npt.assert_array_equal(got[k], want[k], err_msg=k)
    for k in BIT_KEYS:
        assert got[k].dtype == f.dtype, k
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["sum_f"].dtype == np.float64
    tol = (want["area"] - 1) * 2.0 ** -53 * want["sum_abs_f"]
    err = np.abs(got["sum_f"] - want["sum_f"])
    print("sum_f: largest error / bound", float(np.max(err / np.maximum(tol, 1e-300))), "basins", len(tol))
    assert np.all(err <= tol)


@pytest.mark.parametrize("name", sorted(MAPS))
def test_basins_equal_the_oracle(name):
    from astrild_amd import device as dev
    f, want = case(name)
    compare(dev.watershed_basins(f), f, want)


@pytest.mark.parametrize("npix,longest", [(17, 144), (33, 544), (65, 2112)])
def test_snake_is_resolved_within_the_pass_bound(npix, longest, hip):
    from astrild_amd import device as dev
    f, want = case(f"snake{npix}")
    assert orc.longest_path(orc.links(f)) == longest and len(want["minima"]) == 1
    bound = hip.ast_watershed_max_passes(npix)
    assert bound == int(np.ceil(np.log2(npix * npix)))
    got, passes = dev.watershed_basins(f, return_passes=True)
    print("snake", npix, "passes", passes, "bound", bound)
    assert 1 <= passes <= bound
    assert np.all(got["labels"] == 0) and got["area"][0] == npix * npix and got["edges"].shape == (0, 2)


def test_float32_ties_differ_from_their_float64_twin():
    """The float32 map is compared with the oracle run on the float32 values (above); here: the case bites."""
    _, b32 = case("ties_f32")
    _, b64 = case("ties_f64")
    assert len(b32["minima"]) != len(b64["minima"]) or not np.array_equal(b32["labels"], b64["labels"])


def test_thresholds_on_the_64_map():
    from astrild_amd import device as dev
    f, want = case("noise64")
    got = dev.watershed_basins(f)
    counts = []
    for nu in (0, 0.25, 1, np.inf):
        h = nu * f.std() if nu else 0.0
        vob, roots = orc.merge(want, h)
        merged = dev.watershed_merge(got, h)
        npt.assert_array_equal(merged["void_of_basin"], vob)
        assert len(merged["root"]) == len(roots)
        vmap = dev.watershed_void_map(got, merged["void_of_basin"])
        assert vmap.dtype == np.int32 and vmap.shape == f.shape
        npt.assert_array_equal(vmap, orc.void_map(want, vob))
        counts.append(len(roots))
    print("void counts", counts)
    assert counts[0] == len(want["minima"]) and counts[-1] == 1 and counts == sorted(counts, reverse=True)


def test_bit_identical_on_repeat():
    from astrild_amd import device as dev
    f, _ = case("noise130")
    a, b = dev.watershed_basins(f), dev.watershed_basins(f)
    for k in INT_KEYS + BIT_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_device_tensor_in_and_out():
    from astrild_amd import device as dev
    f, want = case("noise130")
    for dtype in (np.float64, np.float32):
        g = np.ascontiguousarray(f, dtype=dtype)
        t = dev.as_device(g)
        got = dev.watershed_basins(t)
        assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got.values())
        assert got["labels"].dtype == torch.int32 and got["saddle"].dtype == t.dtype
        assert t.cpu().numpy().tobytes() == g.tobytes()                  # the caller's map is unchanged
        compare({k: v.cpu().numpy() for k, v in got.items()}, g, want if dtype == np.float64 else orc.basins(g))
        merged = dev.watershed_merge(got, 0.5 * float(g.std()))
        vmap = dev.watershed_void_map(got, merged["void_of_basin"])
        assert isinstance(vmap, torch.Tensor) and vmap.is_cuda and vmap.dtype == torch.int32
        npt.assert_array_equal(vmap.cpu().numpy(), merged["void_of_basin"][got["labels"].cpu().numpy()])


@pytest.mark.parametrize("pattern", [NAN_BYTES, HUGE_BYTES, ZERO_BYTES], ids=lambda p: PATTERN_IDS[p])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_on_dirty_memory(name, pattern):
    from astrild_amd import device as dev
    f, want = case(name)
    with dirty(pattern) as alloc:
        got = dev.watershed_basins(f)
        merged = dev.watershed_merge(got, 0.5 * float(f.std()))
        vmap = dev.watershed_void_map(got, merged["void_of_basin"])
        assert alloc.allocations >= 5
    compare(got, f, want)
    vob, _ = orc.merge(want, 0.5 * float(f.std()))
    npt.assert_array_equal(vmap, orc.void_map(want, vob))


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_non_finite_pixel_is_an_error(value, dtype):
    from astrild_amd import device as dev
    f = orc.smoothed_noise(33).astype(dtype)
    f[17, 32] = value
    with pytest.raises(ValueError):
        dev.watershed_basins(f)
    with pytest.raises(ValueError):
        dev.watershed_basins(dev.as_device(f))


@pytest.mark.parametrize("bad", [np.zeros((2, 2)), np.zeros((4, 5)), np.zeros((6, 6), dtype=np.int32), np.zeros(16),
                                 np.zeros((6, 6), dtype=np.int64)], ids=["npix2", "not_square", "int32", "1d", "int64"])
def test_errors_before_any_launch(bad, monkeypatch):
    from astrild_amd import _lib, device as dev
    lib = _lib.lib()

    def no_launch(*a):
        raise AssertionError("no watershed kernel may be launched")

    for name in ("ast_watershed_link", "ast_watershed_jump", "ast_watershed_relabel", "ast_watershed_sums",
                 "ast_watershed_edges"):
        monkeypatch.setattr(lib, name, no_launch)
    with pytest.raises(ValueError):
        dev.watershed_basins(bad)
    with pytest.raises(ValueError):
        dev.watershed_basins(dev.as_device(bad))


# ---------------------------------------------------------------- the chain
NPIX, ANGLE, HEIGHTS = 256, 10.0, [0, 0.5, 1.0]
MAP_FILE = "/data/test_box/Ray_maps_output12_lc.h5"


@pytest.fixture(scope="module")
def chain():
    """SkyArray -> filter (gaussian, sigma = 2 px) -> WatershedFinder.find_voids, and the oracle on the filtered map."""
    from astrild_amd.rays.skys.sky_array import SkyArray
    from astrild_amd.rays.voids import WatershedFinder
    kappa = 0.02 * np.random.RandomState(21).standard_normal((NPIX, NPIX))
    sky = SkyArray.from_array(kappa.copy(), ANGLE, "kappa_2", "/data", map_file=MAP_FILE)
    sky.filter({"gaussian": {"theta_i": 2.0 * 60.0 * ANGLE / NPIX, "abbrev": "smooth"}}, on="orig")
    finder = WatershedFinder(sky)
    finder.find_voids("orig_smooth", HEIGHTS)
    smooth = np.array(sky.data["orig_smooth"])
    return finder, smooth, orc.basins(smooth)


def test_map_to_filter_to_voids(chain):
    finder, smooth, want = chain
    assert smooth.shape == (NPIX, NPIX) and 0.1 < smooth.std() / 0.02 < 0.2        # it was smoothed
    df = finder.voids_df
    assert list(df.columns[:9]) == ["x_deg", "x_pix", "y_deg", "y_pix", "rad_deg", "rad_pix", "sigma", "theta1_pix",
                                    "theta2_pix"]
    counts = []
    for nu in HEIGHTS:
        vob, roots = orc.merge(want, nu * smooth.std())
        v = orc.voids(want, vob, roots)
        vmap = finder.void_maps[nu]
        npt.assert_array_equal(vmap, orc.void_map(want, vob))
        part = df[df["sigma"] == nu].reset_index(drop=True)
        assert len(part) == len(roots)
        npt.assert_array_equal(part["void_id"].values, np.arange(len(roots)))
        npt.assert_array_equal(part["area_pix"].values, v["area"])
        npt.assert_array_equal(part["edge_pix"].values, v["edge_pix"])
        npt.assert_array_equal(part["theta1_pix"].values, v["x"])
        npt.assert_array_equal(part["theta2_pix"].values, v["y"])
        npt.assert_array_equal(part["x_pix"].values, np.rint(v["x"]).astype(int))
        npt.assert_array_equal(part["y_pix"].values, np.rint(v["y"]).astype(int))
        npt.assert_array_equal(part["rad_pix"].values, np.rint(v["rad"]).astype(int))
        npt.assert_array_equal(part["x_deg"].values, v["x"] * (ANGLE / NPIX))
        npt.assert_array_equal(part["rad_deg"].values, v["rad"] * (ANGLE / NPIX))
        npt.assert_array_equal(part["kappa_min"].values, v["kappa_min"])
        npt.assert_array_equal(part["y_min_pix"].values * NPIX + part["x_min_pix"].values, v["min_index"])
        # sum_f / A: at most A roundings of at most 2^-53 sum|f| each in the sums, and one in the division
        mean_tol = (v["area"] + 1) * 2.0 ** -53 * np.abs(smooth).max()
        assert np.all(np.abs(part["kappa_mean"].values - v["kappa_mean"]) <= mean_tol)
        # every void's lowest pixel lies in it; its centre - the centroid of its pixels - lies in it wherever the
        # oracle's does: always for single basins here, and for all but the few merged voids that bend round another
        assert np.all(vmap[part["y_min_pix"].values, part["x_min_pix"].values] == part["void_id"].values)
        own = vmap[part["y_pix"].values, part["x_pix"].values] == part["void_id"].values
        own_want = orc.void_map(want, vob)[np.rint(v["y"]).astype(int), np.rint(v["x"]).astype(int)] == np.arange(len(roots))
        npt.assert_array_equal(own, own_want)
        print("height", nu, "voids", len(roots), "centres in their own void", int(own.sum()))
        if nu == 0:
            assert own.all()
        assert own.sum() >= 0.99 * len(own)
        counts.append(len(roots))
    assert counts[0] == len(want["minima"]) > counts[1] > counts[2] > 20
    big = finder.find_voids("orig_smooth", [0.5], min_rad_pix=6.0, rtn=True)
    full = df[df["sigma"] == 0.5]
    assert 0 < len(big) == int((np.sqrt(full["area_pix"].values / np.pi) > 6.0).sum()) < len(full)


def test_voids_to_profiles(chain):
    from astrild_amd.rays.void import Voids
    finder, smooth, _ = chain
    extend, nbins = 2.0, 10
    v = Voids("/data/wvf.h5", finder.voids_df.copy(), {"name": "wvf"}, {"npix": NPIX})
    v.get_profiles(extend, nbins, skymap=smooth)
    df = finder.voids_df
    reach = extend * df["rad_pix"].values
    keep = df[(df["theta1_pix"].values + reach < NPIX) & (df["theta1_pix"].values - reach > 0)
              & (df["theta2_pix"].values + reach < NPIX) & (df["theta2_pix"].values - reach > 0)].reset_index()
    keep = keep[extend * keep["rad_pix"] > 10].reset_index()
    assert len(keep) > 100
    npt.assert_array_equal(v.data["void_id"].values, keep["void_id"].values)
    npt.assert_array_equal(v.data["sigma"].values, keep["sigma"].values)
    xs, ys, rs = keep["x_pix"].values, keep["y_pix"].values, keep["rad_pix"].values
    values, _, counts, radii = porc.from_map(xs, ys, rs, smooth, extend, nbins)
    a = porc.from_map(xs, ys, rs, np.abs(smooth), extend, nbins)[1]
    tol = np.array([porc.aligned(ai, ci) for ai, ci in zip(a, counts)]) * 1e-12
    fin = np.isfinite(values)
    npt.assert_array_equal(v.profiles["radii"], radii)
    npt.assert_array_equal(np.isfinite(v.profiles["values"]), fin)
    assert np.all(np.abs(v.profiles["values"][fin] - values[fin]) <= tol[fin])


def test_to_file_and_back(chain, tmp_path):
    pytest.importorskip("tables")
    import pandas as pd
    from astrild_amd.rays.void import Voids
    finder, smooth, _ = chain
    finder.to_file(str(tmp_path))
    path = finder._create_filename("voids", str(tmp_path), "orig_smooth")
    v = Voids.from_file("wvf", {"npix": NPIX}, ffile=path)
    assert v.finder_spec == {"name": "wvf"}
    pd.testing.assert_frame_equal(v.data, finder.voids_df, check_exact=True)
    v.get_profiles(2.0, 10, skymap=smooth)
    assert len(v.data) > 100 and v.profiles["values"].shape == (len(v.data), 10)
