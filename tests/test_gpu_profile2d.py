"""GPU: radial profiles of objects on 2D maps (ast_profile2d through device.annulus_profiles, profile_2d.from_map and
rays.void.Voids): per-annulus counts exactly equal to the numpy oracle (tests/profile2d_oracle.py), sums exactly equal on
integer-valued maps and within 1e-12 of the summed magnitudes on random maps, the reference's recorded outputs, a huge
object among many small ones, bands against one work item per object, repeat stability, device-tensor maps and the
errors raised before any launch."""
import json
import os

import numpy as np
import numpy.testing as npt
import pandas as pd
import pytest

from tests import profile2d_oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(3.0, 20), (2.5, 7), (1.2, 12)]


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


def closed_map(ny, nx, dtype=np.float64):
    i, j = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    return (((i * 7919 + j * 104729) % 1009) / 64).astype(dtype)


def random_map(ny, nx, dtype, seed):
    return np.random.RandomState(seed).standard_normal((ny, nx)).astype(dtype)


def mixed_catalogue(n, ny, nx, rmax, extend, seed):
    """Radii 1..rmax (small ones with empty annuli included); centres anywhere numpy can index, the negative wrap
    included: |offset| <= R keeps y - R >= -ny and y + R - 1 < ny."""
    rs = np.random.RandomState(seed)
    r = rs.randint(1, rmax + 1, n)
    R = np.ceil(r * extend).astype(int)
    y = np.array([rs.randint(-ny + Ri, ny - Ri) for Ri in R])
    x = np.array([rs.randint(-nx + Ri, nx - Ri) for Ri in R])
    return x, y, r


def gpu(skymap, x, y, r, extend, nbins):
    from astrild_amd import device as dev
    s, c = dev.annulus_profiles(skymap, x, y, r, extend, nbins)
    return dev.to_numpy(s), dev.to_numpy(c)


def oracle(skymap, x, y, r, extend, nbins):
    _, s, c, _ = orc.from_map(x, y, r, skymap, extend, nbins)
    return s, c


def abs_sums(skymap, x, y, r, extend, nbins):
    return oracle(np.abs(skymap.astype(np.float64)), x, y, r, extend, nbins)[0]


@pytest.mark.parametrize("extend,nbins", PAIRS)
def test_counts_and_integer_sums_exact(extend, nbins):
    skymap = closed_map(300, 340)
    x, y, r = mixed_catalogue(2000, 300, 340, 24, extend, seed=int(extend * 10) + nbins)
    s, c = gpu(skymap, x, y, r, extend, nbins)
    os_, oc = oracle(skymap, x, y, r, extend, nbins)
    npt.assert_array_equal(c, oc)
    npt.assert_array_equal(s, os_)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_random_map_sums_within_tolerance(dtype):
    extend, nbins = 3.0, 20
    skymap = random_map(256, 320, dtype, seed=3)
    x, y, r = mixed_catalogue(2000, 256, 320, 20, extend, seed=8)
    s, c = gpu(skymap, x, y, r, extend, nbins)
    os_, oc = oracle(skymap, x, y, r, extend, nbins)
    npt.assert_array_equal(c, oc)
    assert np.all(np.abs(s - os_) <= 1e-12 * abs_sums(skymap, x, y, r, extend, nbins))


def test_from_map_values_with_nan_and_inf():
    from astrild_amd.profiles import profile_2d as p2d
    skymap = closed_map(128, 128)
    x, y, r = mixed_catalogue(400, 128, 128, 6, 3.0, seed=5)
    df = pd.DataFrame({"x_pix": x, "y_pix": y, "rad_pix": r})
    out = p2d.from_map(df, skymap, 3.0, 20, return_counts=True)
    values, sums, counts, radii = orc.from_map(x, y, r, skymap, 3.0, 20)
    assert np.isnan(values).any() and np.isinf(values).any()
    npt.assert_array_equal(out["values"], values)
    npt.assert_array_equal(out["radii"], radii)
    npt.assert_array_equal(out["counts"], counts)
    npt.assert_array_equal(out["sums"], sums)


def golden_cases():
    with open(os.path.join(ROOT, "tests", "golden", "profile2d_reference.json")) as f:
        return [c for c in json.load(f)["cases"] if c["kind"] == "from_map"]


def dec(v):
    if isinstance(v, list):
        return np.array([dec(x) for x in v], dtype=np.float64)
    return {"nan": np.nan, "inf": np.inf, "-inf": -np.inf}[v] if isinstance(v, str) else float(v)


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_from_map_matches_the_reference(case):
    from astrild_amd.profiles import profile_2d as p2d
    m = case["map"]
    ny, nx = m["shape"]
    skymap = closed_map(ny, nx, m["dtype"]) if m["kind"] == "closed" else random_map(ny, nx, m["dtype"], m["seed"])
    o = case["objects"]
    out = p2d.from_map(pd.DataFrame(o), skymap, case["extend"], case["nbins"])
    want = dec(case["values"])
    npt.assert_array_equal(out["radii"], dec(case["radii"]))
    npt.assert_array_equal(np.isnan(out["values"]), np.isnan(want))
    fin = np.isfinite(want)
    npt.assert_array_equal(np.where(fin, 0, out["values"]), np.where(fin, 0, want))
    if m["kind"] == "closed":
        npt.assert_array_equal(out["values"], want)
    else:
        a = abs_sums(skymap, o["x_pix"], o["y_pix"], o["rad_pix"], case["extend"], case["nbins"])
        c = oracle(skymap, o["x_pix"], o["y_pix"], o["rad_pix"], case["extend"], case["nbins"])[1]
        tol = np.array([orc.aligned(ai, ci) for ai, ci in zip(a, c)]) * 1e-12
        assert np.all(np.abs(out["values"][fin] - want[fin]) <= tol[fin])


def test_huge_object_among_many_small(monkeypatch):
    extend, nbins = 3.0, 20
    n = 4096
    skymap = random_map(n, n, np.float64, seed=21)
    rs = np.random.RandomState(4)
    r = np.concatenate([[500], rs.randint(5, 51, 10000)])
    x = np.concatenate([[2048], rs.randint(160, n - 160, 10000)])
    y = np.concatenate([[2000], rs.randint(160, n - 160, 10000)])
    s, c = gpu(skymap, x, y, r, extend, nbins)
    pick = np.concatenate([[0], np.arange(1, len(r), 97)])
    os_, oc = oracle(skymap, x[pick], y[pick], r[pick], extend, nbins)
    npt.assert_array_equal(c[pick], oc)
    a = abs_sums(skymap, x[pick], y[pick], r[pick], extend, nbins)
    assert np.all(np.abs(s[pick] - os_) <= 1e-12 * a)
    assert int(np.ceil(500 * extend)) == 1500 and c[0].sum() > 6_000_000
    monkeypatch.setenv("ASTRILD_PROFILE_BANDS", "0")
    s1, c1 = gpu(skymap, x, y, r, extend, nbins)
    npt.assert_array_equal(c1, c)
    a_all = abs_sums(skymap, x[:1], y[:1], r[:1], extend, nbins)
    assert np.all(np.abs(s1[0] - s[0]) <= 1e-12 * a_all[0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bands_against_one_item_per_object(dtype, monkeypatch):
    extend, nbins = 2.5, 7
    skymap = random_map(400, 400, dtype, seed=9)
    x, y, r = mixed_catalogue(1500, 400, 400, 60, extend, seed=10)
    s, c = gpu(skymap, x, y, r, extend, nbins)
    monkeypatch.setenv("ASTRILD_PROFILE_BANDS", "0")
    s0, c0 = gpu(skymap, x, y, r, extend, nbins)
    npt.assert_array_equal(c, c0)
    assert np.all(np.abs(s - s0) <= 2e-12 * abs_sums(skymap, x, y, r, extend, nbins))


def test_bit_identical_on_repeat():
    skymap = random_map(512, 512, np.float64, seed=1)
    x, y, r = mixed_catalogue(3000, 512, 512, 40, 3.0, seed=2)
    s1, c1 = gpu(skymap, x, y, r, 3.0, 20)
    s2, c2 = gpu(skymap, x, y, r, 3.0, 20)
    assert s1.tobytes() == s2.tobytes() and c1.tobytes() == c2.tobytes()


def test_device_tensor_map_of_a_resident_skyarray():
    from astrild_amd.profiles import profile_2d as p2d
    from astrild_amd.rays._resident import MapStore
    from astrild_amd import device as dev
    host = random_map(256, 256, np.float64, seed=12)
    store = MapStore()
    store["orig"] = dev.as_device(host)
    assert store.resident("orig")
    x, y, r = mixed_catalogue(500, 256, 256, 15, 3.0, seed=13)
    df = pd.DataFrame({"x_pix": x, "y_pix": y, "rad_pix": r})
    a = p2d.from_map(df, store.device("orig"), 3.0, 20, return_counts=True)
    b = p2d.from_map(df, host, 3.0, 20, return_counts=True)
    assert store.resident("orig")
    npt.assert_array_equal(a["sums"], b["sums"])
    npt.assert_array_equal(a["counts"], b["counts"])
    f32 = dev.as_device(host.astype(np.float32))
    c = p2d.from_map(df, f32, 3.0, 20, return_counts=True)
    d = p2d.from_map(df, host.astype(np.float32), 3.0, 20, return_counts=True)
    npt.assert_array_equal(c["sums"], d["sums"])


@pytest.mark.parametrize("kw,exc", [({"x": [-70]}, IndexError), ({"y": [63]}, IndexError), ({"x": [62]}, IndexError),
                                    ({"r": [0]}, ValueError), ({"extend": 0.0}, ValueError),
                                    ({"nbins": 0}, ValueError), ({"x": [], "y": [], "r": []}, ValueError)])
def test_errors_before_any_launch(kw, exc, monkeypatch):
    from astrild_amd import _lib, device as dev
    lib = _lib.lib()

    def no_launch(*a):
        raise AssertionError("ast_profile2d must not be called")

    monkeypatch.setattr(lib, "ast_profile2d", no_launch)
    args = {"x": [10], "y": [10], "r": [2], "extend": 3.0, "nbins": 20}
    args.update(kw)
    with pytest.raises(exc):
        dev.annulus_profiles(np.zeros((64, 64)), args["x"], args["y"], args["r"], args["extend"], args["nbins"])


def test_voids_pipeline_against_the_oracle():
    from astrild_amd.rays.void import Voids
    npix, extend, nbins = 512, 2.0, 10
    rs = np.random.RandomState(31)
    n = 300
    x, y = rs.randint(0, npix, n), rs.randint(0, npix, n)
    rad = rs.randint(2, 15, n)
    df = pd.DataFrame({"x_pix": x, "y_pix": y, "theta1_pix": x + 0.5, "theta2_pix": y + 0.5, "rad_pix": rad,
                       "rad_deg": rad * 0.01, "sigma": rs.choice([2.0, 3.0, 4.0], n)})
    skymap = random_map(npix, npix, np.float64, seed=32)
    keep = df[(x + 0.5 + extend * rad < npix) & (x + 0.5 - extend * rad > 0) & (y + 0.5 + extend * rad < npix)
              & (y + 0.5 - extend * rad > 0)].reset_index()
    keep = keep[extend * keep["rad_pix"] > 10].reset_index()
    norm = skymap - np.mean(skymap)
    values, _, _, radii = orc.from_map(keep["x_pix"].values, keep["y_pix"].values, keep["rad_pix"].values, norm,
                                       extend, nbins)
    v = Voids("/data/tunnels.h5", df, {"name": "tunnels"}, {"npix": npix})
    before = skymap.copy()
    v.get_profiles(extend, nbins, skymap=skymap, field_conversion="normalize")
    npt.assert_array_equal(skymap, before)
    npt.assert_array_equal(v.data["x_pix"].values, keep["x_pix"].values)
    a = abs_sums(norm, keep["x_pix"].values, keep["y_pix"].values, keep["rad_pix"].values, extend, nbins)
    c = oracle(norm, keep["x_pix"].values, keep["y_pix"].values, keep["rad_pix"].values, extend, nbins)[1]
    tol = np.array([orc.aligned(ai, ci) for ai, ci in zip(a, c)]) * 1e-12
    fin = np.isfinite(values)
    npt.assert_array_equal(np.isfinite(v.profiles["values"]), fin)
    assert np.all(np.abs(v.profiles["values"][fin] - values[fin]) <= tol[fin])
    np.random.seed(99)
    res = v.get_profile_stats(cats=["sigma"])
    np.random.seed(99)
    gpu_vals = v.profiles["values"]
    for ss, sigma in enumerate(np.unique(keep["sigma"].values)):
        cat = v.data.loc[v.data["sigma"] == sigma]
        mean = orc.mean_and_interpolate(gpu_vals[cat.index.values, :], cat["rad_pix"].values, radii.max(), nbins)
        err = orc.bootstrapping(gpu_vals[cat.index.values, :], cat["x_pix"].values, cat["y_pix"].values,
                                cat["rad_pix"].values, npix, radii.max(), nbins)
        npt.assert_array_equal(res["mean"][ss], mean)
        npt.assert_array_equal(res["lowerr"][ss], err[0])
        omean = orc.mean_and_interpolate(values[cat.index.values, :], cat["rad_pix"].values, radii.max(), nbins)
        npt.assert_allclose(res["mean"][ss], omean, rtol=1e-9, atol=1e-12)
