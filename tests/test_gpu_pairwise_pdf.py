"""GPU: the pairwise-velocity histograms (ast_pairwise_pdf_prepare / ast_pairwise_pdf, through
device.pairwise_velocity_pdf and astrild_amd.particles.hutils.mean_pv_z_sign / mean_pv_radial) against the recorded
results of the reference and the numpy oracle (tests/pairwise_pdf_oracle.py).  The histogram and `outside` are compared
for equality, always.  The moments: counts equal, and per row |s1 - s1_ref| <= count 2^-52 sum|v12| and
|s2 - s2_ref| <= count 2^-52 sum v12^2, the bound on the difference of two orders of an fp64 sum of `count` terms
(each order is within (count - 1) 2^-53 sum|x| of the exact sum), from the oracle's own per-row values."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

from tests import pairwise_oracle as tv_orc
from tests import pairwise_pdf_oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
KINDS = ["z_sign", "radial"]
MODES = {"default": {}, "one_cell": {"ASTRILD_PVPDF_CELLS": "0"}, "global_hist": {"ASTRILD_PVPDF_LDS": "0"}}


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


@functools.lru_cache(maxsize=None)
def catalogue(name):
    if name == "compact":                               # one cell, about 12 tiles, several j stages, the j > i triangle
        pos = orc.compact(3000, seed=11)
        # dist_width 4: the 9 rows span 36 > r = 30, so every seen pair has a row and `outside` holds velocities only;
        # at width 1 nine tenths of the pairs (d >= 9) would go outside (test_compact_at_unit_width runs that too)
        return pos, orc.coherent_velocities(pos, 3), dict(r=30.0, dist_bin=9, vel_bin=40, dist_width=4.0)
    if name == "light_cone":                            # many cells, half-shell neighbours, ragged tiles
        pos, _ = tv_orc.light_cone(6000, seed=5, clusters=300, sigma=8.0)
        return pos, orc.coherent_velocities(pos, 3), dict(r=50.0, dist_bin=51, vel_bin=40)
    if name == "lattice":
        pos, vel = orc.lattice(12)
        return pos, vel, dict(r=8.0, dist_bin=9, vel_bin=40)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle(name, kind, extra=()):
    """The oracle's result for a catalogue, computed once and shared (read-only) by the tests that need it."""
    pos, vel, par = catalogue(name)
    res = orc.pair_pdf(pos, vel, kind=kind, **{**par, **dict(extra)})
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def gpu(pos, vel, kind, moments=True, **par):
    from astrild_amd import device as dev
    res = dev.pairwise_velocity_pdf(pos, vel, kind=kind, moments=moments, **par)
    out = dict(hist=dev.to_numpy(res[0]), outside=int(res[1].item()))
    assert res[0].dtype == torch.int64 and res[1].dtype == torch.int64 and res[1].dim() == 0
    assert tuple(res[0].shape) == (par["dist_bin"], par["vel_bin"])
    if moments:
        out.update(count=dev.to_numpy(res[2][0]), s1=dev.to_numpy(res[2][1]), s2=dev.to_numpy(res[2][2]))
    return out


def assert_same(got, ref):
    npt.assert_array_equal(got["hist"], ref["hist"])
    assert got["outside"] == ref["outside"]
    if "count" in got:
        npt.assert_array_equal(got["count"], ref["count"])
        e1, e2 = np.abs(got["s1"] - ref["s1"]), np.abs(got["s2"] - ref["s2"])
        b1, b2 = ref["count"] * 2.0 ** -52 * ref["sum_abs"], ref["count"] * 2.0 ** -52 * ref["s2"]
        print("moment errors / bounds:", np.max(e1 / np.maximum(b1, 1e-300)), np.max(e2 / np.maximum(b2, 1e-300)))
        assert np.all(e1 <= b1), (e1, b1)
        assert np.all(e2 <= b2), (e2, b2)


def lds_bins(dist_bin, moments):
    from astrild_amd import _lib
    return _lib.lib().ast_pairwise_pdf_lds_bins(dist_bin, int(moments))


def test_known_answers():
    from astrild_amd.particles.hutils import mean_pv_z_sign
    cat, edges = orc.load_golden()
    chunk = dict(cat, **cat["chunk"])
    for case in [cat, chunk] + edges:
        ref = orc.dense(case["entries"], case["dist_bin"], case["vel_bin"])
        counter, outside = mean_pv_z_sign(None, case["pos"], case["vel"], case["ffirst"], case["ssecond"], case["r"],
                                          case["dist_bin"], case["vel_bin"], return_outside=True)
        assert counter.dtype == np.float64 and counter.shape == (case["dist_bin"] * case["vel_bin"],)
        npt.assert_array_equal(counter, ref.reshape(-1), case.get("note", "catalogue"))
        o = orc.pair_pdf(case["pos"], case["vel"], case["r"], case["dist_bin"], case["vel_bin"], "z_sign",
                         ffirst=case["ffirst"], ssecond=case["ssecond"])
        assert outside == o["outside"], case.get("note", "catalogue")
    plain = mean_pv_z_sign(None, cat["pos"], cat["vel"], 0, len(cat["pos"]), cat["r"], cat["dist_bin"], cat["vel_bin"])
    npt.assert_array_equal(plain, orc.dense(cat["entries"], cat["dist_bin"], cat["vel_bin"]).reshape(-1))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["compact", "light_cone"])
def test_random_catalogues_against_oracle(name, kind, mode, monkeypatch):
    pos, vel, par = catalogue(name)
    ref = oracle(name, kind)
    # not vacuous: pairs outside the velocity range, both end columns populated, most pairs inside
    assert ref["outside"] > 0 and ref["hist"][:, 0].sum() > 0 and ref["hist"][:, -1].sum() > 0
    assert ref["hist"].sum() > 20 * ref["outside"]
    assert par["dist_bin"] * par["vel_bin"] <= lds_bins(par["dist_bin"], True)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    assert_same(gpu(pos, vel, kind, **par), ref)


@pytest.mark.parametrize("kind", KINDS)
def test_compact_at_unit_width(kind):
    """The compact catalogue with the reference's own widths: 9 x 40 bins of width 1 at r = 30, so the pairs with
    d >= 9 are seen and go outside."""
    pos, vel, _ = catalogue("compact")
    extra = dict(dist_bin=9, vel_bin=40, dist_width=1.0)
    ref = oracle("compact", kind, tuple(sorted(extra.items())))
    assert ref["outside"] > ref["hist"].sum() > 0 and ref["hist"][:, 0].sum() > 0 and ref["hist"][:, -1].sum() > 0
    assert_same(gpu(pos, vel, kind, r=30.0, **extra), ref)


def test_mean_pv_radial_moments():
    from astrild_amd.particles.hutils import mean_pv_radial
    pos, vel, par = catalogue("compact")
    ref = oracle("compact", "radial")
    counter, outside, mom = mean_pv_radial(None, pos, vel, 0, len(pos), par["r"], par["dist_bin"], par["vel_bin"],
                                           dist_width=par["dist_width"], return_outside=True, return_moments=True)
    npt.assert_array_equal(counter, ref["hist"].reshape(-1))
    assert outside == ref["outside"]
    mean, sigma = orc.mean_and_sigma(ref["count"], ref["s1"], ref["s2"])
    assert ref["count"][-1] == 0 and np.isnan(mom["mean"][-1]) and np.isnan(mom["sigma"][-1])      # d < 30 < 32
    npt.assert_allclose(mom["mean"][:-1], mean[:-1], rtol=1e-10)
    npt.assert_allclose(mom["sigma"][:-1], sigma[:-1], rtol=1e-10)
    assert np.all(mom["mean"][2:-1] < 0)                # the infall term: not pure cancellation


@pytest.mark.parametrize("kind", KINDS)
def test_integer_lattice(kind):
    pos, vel, par = catalogue("lattice")
    ref = oracle("lattice", kind)
    d0 = np.sqrt(((pos[1:] - pos[0]) ** 2).sum(axis=1))
    assert np.sum((d0 == np.round(d0)) & (d0 <= 8.0)) >= 21            # separations exactly on bin edges
    assert ref["hist"][1:].sum(axis=1).all() and ref["outside"] > 0
    if kind == "z_sign":
        assert ref["hist"][:, 20].sum() >= 12 * 12 * 11 * 2           # whole planes of equal z: v12 = 0
    assert_same(gpu(pos, vel, kind, **par), ref)


@pytest.mark.parametrize("kind", KINDS)
def test_histogram_beyond_lds(kind):
    pos, vel, _ = catalogue("compact")
    par = dict(r=30.0, dist_bin=40, vel_bin=4096, vel_width=0.01)
    assert lds_bins(40, True) < 40 * 4096 and lds_bins(40, False) < 40 * 4096      # the global path, by size
    ref = oracle("compact", kind, tuple(sorted(dict(dist_bin=40, vel_bin=4096, vel_width=0.01, dist_width=1.0).items())))
    assert ref["outside"] > 0 and ref["hist"].sum() > 20 * ref["outside"] and np.count_nonzero(ref["hist"]) > 40000
    assert_same(gpu(pos, vel, kind, **par), ref)


@pytest.mark.parametrize("over", [0, 1])
def test_histogram_at_the_lds_edge(over):
    """The largest histogram that is counted in LDS (all of the CU's LDS in one workgroup) and the first one that is
    not, by the library's own report."""
    pos, vel, _ = catalogue("compact")
    vel_bin = lds_bins(40, True) // 40 + over
    assert (40 * vel_bin <= lds_bins(40, True)) == (not over) and vel_bin > 800
    extra = dict(dist_bin=40, vel_bin=vel_bin, vel_width=0.05, dist_width=1.0)
    ref = oracle("compact", "radial", tuple(sorted(extra.items())))
    assert ref["outside"] > 0 and ref["hist"][:, 0].sum() > 0 and ref["hist"][:, -1].sum() > 0
    assert_same(gpu(pos, vel, "radial", r=30.0, **extra), ref)


@pytest.mark.parametrize("kind", KINDS)
def test_widths(kind):
    pos, vel, _ = catalogue("compact")
    extra = dict(dist_bin=9, vel_bin=40, dist_width=2.5, vel_width=0.5)
    ref = oracle("compact", kind, tuple(sorted(extra.items())))
    assert ref["outside"] > ref["hist"].sum() > 0       # reach 30 against 9 x 2.5: rows beyond dist_bin go outside
    assert_same(gpu(pos, vel, kind, r=30.0, **extra), ref)


@pytest.mark.parametrize("mode", ["default", "one_cell"])
def test_flush_at_every_stage(mode, monkeypatch):
    monkeypatch.setenv("AST_PVPDF_FLUSH_AT", "0")
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    name = "compact" if mode == "default" else "light_cone"
    pos, vel, par = catalogue(name)
    assert_same(gpu(pos, vel, "z_sign", **par), oracle(name, "z_sign"))


@pytest.mark.parametrize("kind", KINDS)
def test_row_ranges(kind):
    pos, vel, par = catalogue("compact")
    ref = oracle("compact", kind)
    a = gpu(pos, vel, kind, ffirst=0, ssecond=700, **par)
    b = gpu(pos, vel, kind, ffirst=700, ssecond=3000, **par)
    assert a["hist"].sum() > 0 and b["hist"].sum() > 0
    npt.assert_array_equal(a["hist"] + b["hist"], ref["hist"])
    assert a["outside"] + b["outside"] == ref["outside"]
    npt.assert_array_equal(a["count"] + b["count"], ref["count"])
    part = orc.pair_pdf(pos, vel, kind=kind, ffirst=0, ssecond=700, **par)
    assert_same(a, part)
    for f in (0, 700, 3000):
        z = gpu(pos, vel, kind, ffirst=f, ssecond=f, **par)
        assert not z["hist"].any() and z["outside"] == 0 and not z["count"].any() and not z["s1"].any()


@pytest.mark.parametrize("kind", KINDS)
def test_float32_and_device_tensor_inputs(kind):
    pos, vel, par = catalogue("light_cone")
    p32, v32 = pos[:3000].astype(np.float32), vel[:3000].astype(np.float32)
    ref = orc.pair_pdf(p32.astype(np.float64), v32.astype(np.float64), kind=kind, **par)
    host = gpu(p32, v32, kind, **par)
    assert_same(host, ref)
    dev_in = gpu(torch.from_numpy(p32).cuda(), torch.from_numpy(v32).cuda(), kind, **par)
    assert_same(dev_in, ref)
    npt.assert_array_equal(dev_in["hist"], host["hist"])
    mixed = gpu(torch.from_numpy(p32).cuda(), v32.astype(np.float64), kind, moments=False, **par)
    npt.assert_array_equal(mixed["hist"], host["hist"])


@pytest.mark.parametrize("n", [0, 1])
def test_fewer_than_two_objects(n):
    from astrild_amd.particles.hutils import mean_pv_radial
    pos, vel = np.full((n, 3), 1000.0), np.ones((n, 3))
    for kind in KINDS:
        z = gpu(pos, vel, kind, r=5.0, dist_bin=6, vel_bin=7)
        assert z["hist"].shape == (6, 7) and not z["hist"].any() and z["outside"] == 0
        assert z["count"].shape == (6,) and not z["count"].any() and not z["s1"].any() and not z["s2"].any()
    counter = mean_pv_radial(None, pos, vel, 0, n, 5.0, 6, 7)
    assert counter.shape == (42,) and not counter.any()
    torch.cuda.synchronize()


def test_coincident_pair_in_radial():
    pos = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.0, 2.0, 5.0]])
    vel = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 2.0], [0.0, 0.0, 4.0]])
    ref = orc.pair_pdf(pos, vel, 4.0, 5, 10, "radial")
    got = gpu(pos, vel, "radial", r=4.0, dist_bin=5, vel_bin=10)
    assert ref["outside"] == 1 and got["outside"] == 1
    assert np.all(np.isfinite(got["s1"])) and np.all(np.isfinite(got["s2"]))
    assert_same(got, ref)
    assert_same(gpu(pos, vel, "z_sign", r=4.0, dist_bin=5, vel_bin=10), orc.pair_pdf(pos, vel, 4.0, 5, 10, "z_sign"))


@pytest.mark.parametrize("mode", ["default", "global_hist"])
def test_two_calls_are_bit_identical(mode, monkeypatch):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    pos, vel, par = catalogue("light_cone")
    a, b = gpu(pos, vel, "radial", **par), gpu(pos, vel, "radial", **par)
    npt.assert_array_equal(a["hist"], b["hist"])
    assert a["outside"] == b["outside"]
    npt.assert_array_equal(a["count"], b["count"])
