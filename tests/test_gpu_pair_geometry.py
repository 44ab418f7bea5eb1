"""GPU: the two pairwise-velocity kernels that walk the bounding-box cell grid of cell_grid.h - pairwise.hip
(ast_pairwise_tv_prepare / ast_pairwise_tv) and pairwise_pdf.hip (ast_pairwise_pdf_prepare / ast_pairwise_pdf) - on the
degenerate catalogues of tests/pair_geometry.py: planes, lines, coincident objects, a cap-limited grid, a pair on each
of the 13 half-shell offsets, two crowded neighbour cells, coordinates a million from the origin, float32 coordinates,
separations exactly on bin edges and at the reach, and one-cell catalogues of tile-boundary sizes.  Each runs on the
cell grid and on one forced cell, against the numpy oracles (tests/pairwise_oracle.py, tests/pairwise_pdf_oracle.py).

Pair counts, histograms and `outside` are compared for equality.  The fp64 sums, per bin:
|got - ref| <= max(count, 8) 2^-52 sum|term|, with sum|term| from the oracle: count 2^-52 sum|term| bounds the
difference of two orders of an fp64 sum of `count` terms (each is within (count - 1) 2^-53 sum|x| of the exact sum);
the floor of 8 allows the few ulp by which a term itself differs when the kernel holds the pair as (j, i).  The
transverse-velocity kernel gets cartesian (N, 3) velocities, so its prep calls no libm function and each term is, op
for op, the oracle's.  tests/test_pair_geometry_cpu.py shows that the oracle, run in two orders, stays inside this
bound, and that the catalogues reach what they claim; here the planned grid is read back from the workspace, so that a
catalogue which silently collapsed to one cell would be noticed."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

from tests import pair_geometry as pg
from tests import pairwise_oracle as tv_orc
from tests import pairwise_pdf_oracle as pdf_orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
NAMES = list(pg.CATALOGUES)
KINDS = ["z_sign", "radial"]
CELLS = {"grid": "1", "one_cell": "0"}
VEL_BIN, VEL_WIDTH = 16, 2.0                # velocity differences scatter by 8.5: a few per cent of the pairs outside
F32, F64 = np.float32, np.float64
WORST = {}                                  # kernel -> largest error / bound seen, printed as it grows


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


@functools.lru_cache(maxsize=None)
def catalogue(name, pos_dtype=F64, vel_dtype=F64):
    """(pos, vel, par) in the given dtypes; the velocities are drawn for the float64 positions.  Shared: read only."""
    pos, par, _ = pg.CATALOGUES[name]()
    vel = pg.velocities(pos, 7).astype(vel_dtype)
    return pos.astype(pos_dtype), vel, par


def frozen(arrays):
    for v in arrays:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def tv_oracle(name, pos_dtype=F64, vel_dtype=F64, binnr=None, binwidth=None):
    """(nom, denom, counts, sum|term|) of the oracle on the catalogue's values, widened to float64; computed once."""
    pos, vel, par = catalogue(name, pos_dtype, vel_dtype)
    pos, vel = pos.astype(F64), vel.astype(F64)
    u, _ = tv_orc.angles_and_velocities(pos, np.zeros((len(pos), 2)))
    return frozen(tv_orc.pair_sums(pos, u, vel, binnr or par["binnr"], binwidth or par["binwidth"], with_abs=True))


def pdf_par(par):
    """The histogram kernel's arguments for a catalogue: its reach, and one row more than the reach covers, which
    holds exactly the pairs with d == r."""
    return dict(r=par["binnr"] * par["binwidth"], dist_bin=par["binnr"] + 1, vel_bin=VEL_BIN, dist_width=par["binwidth"],
                vel_width=VEL_WIDTH)


@functools.lru_cache(maxsize=None)
def pdf_oracle(name, kind, pos_dtype=F64, vel_dtype=F64, ffirst=0, ssecond=None):
    pos, vel, par = catalogue(name, pos_dtype, vel_dtype)
    res = pdf_orc.pair_pdf(pos.astype(F64), vel.astype(F64), kind=kind, ffirst=ffirst, ssecond=ssecond, **pdf_par(par))
    frozen(res.values())
    return res


def gpu_tv(pos, vel, binnr, binwidth):
    from astrild_amd import device as dev
    nom, den, cnt = dev.pairwise_tv(pos, vel, binnr, binwidth)
    return dev.to_numpy(nom), dev.to_numpy(den), dev.to_numpy(cnt)


def gpu_pdf(pos, vel, kind, **par):
    from astrild_amd import device as dev
    hist, outside, (count, s1, s2) = dev.pairwise_velocity_pdf(pos, vel, kind=kind, moments=True, **par)
    return dict(hist=dev.to_numpy(hist), outside=int(outside.item()), count=dev.to_numpy(count), s1=dev.to_numpy(s1),
                s2=dev.to_numpy(s2))


def bound(count, scale):
    return np.maximum(count, 8) * 2.0 ** -52 * scale


def within(kernel, what, got, ref, count, scale):
    """|got - ref| <= bound per bin, NaN exactly where the reference has it; prints error / bound."""
    nan = np.isnan(ref)
    npt.assert_array_equal(np.isnan(got), nan, what)
    err, lim = np.abs(got - ref)[~nan], bound(count, scale)[~nan]
    ratio = float(np.max(err / np.maximum(lim, 1e-300), initial=0.0))
    if ratio > WORST.get(kernel, -1.0):
        WORST[kernel] = ratio
        print(f"{kernel}: largest error / bound so far {ratio:.3g} ({what})")
    assert np.all(err <= lim), (what, err, lim)


def assert_tv(got, ref, what):
    npt.assert_array_equal(got[2], ref[2], what)
    within("pairwise_tv", what + " nom", got[0], ref[0], ref[2], ref[3])
    within("pairwise_tv", what + " denom", got[1], ref[1], ref[2], ref[1])


def assert_pdf(got, ref, what):
    npt.assert_array_equal(got["hist"], ref["hist"], what)
    assert got["outside"] == ref["outside"], what
    npt.assert_array_equal(got["count"], ref["count"], what)
    within("pairwise_pdf", what + " s1", got["s1"], ref["s1"], ref["count"], ref["sum_abs"])
    within("pairwise_pdf", what + " s2", got["s2"], ref["s2"], ref["count"], ref["s2"])


# ------------------------------------------------------------------ both kernels, every catalogue, grid and one cell
@pytest.mark.parametrize("cells", list(CELLS))
@pytest.mark.parametrize("name", NAMES)
def test_tv_against_oracle(name, cells, monkeypatch):
    monkeypatch.setenv("ASTRILD_PV_CELLS", CELLS[cells])
    pos, vel, par = catalogue(name)
    ref = tv_oracle(name)
    assert ref[2].sum() > 0
    nan = [True] + [False] * (par["binnr"] - 1) if name in ("coincident", "all_coincident") else [False] * par["binnr"]
    assert np.isnan(ref[0]).tolist() == nan and np.isnan(ref[1]).tolist() == nan
    assert_tv(gpu_tv(pos, vel, par["binnr"], par["binwidth"]), ref, f"{name} {cells}")


@pytest.mark.parametrize("cells", list(CELLS))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_pdf_against_oracle(name, kind, cells, monkeypatch):
    monkeypatch.setenv("ASTRILD_PVPDF_CELLS", CELLS[cells])
    pos, vel, par = catalogue(name)
    ref = pdf_oracle(name, kind)
    assert ref["hist"].sum() + ref["outside"] > 0
    if name == "edge_pairs":
        assert ref["count"][-1] >= 4                        # the pairs exactly at the reach have a row
    if name == "coincident" and kind == "radial":
        assert ref["outside"] >= 300 * 299 // 2             # v12 = 0 / 0
    assert_pdf(gpu_pdf(pos, vel, kind, **pdf_par(par)), ref, f"{name} {kind} {cells}")


# ------------------------------------------------------------------ the planned grid is the intended one
def read_grid_params(work):
    """The head of a pair finder's workspace after a run: ``struct GridBoxParams`` (pair_geometry.parse_grid_params)."""
    torch.cuda.synchronize()
    return pg.parse_grid_params(work[:128].cpu().numpy())


def assert_planned(work, pos, reach, single, what):
    got, want = read_grid_params(work), pg.plan(pos, reach, single=bool(single))
    assert got["dims"].tolist() == want.dims.tolist(), what
    assert got["ncells"] == int(np.prod(want.dims)), what
    assert got["ntiles"] == pg.tiles(want), what
    npt.assert_array_equal(got["lo"], want.lo, what)
    npt.assert_array_equal(got["inv_cs"], want.inv_cs, what)


@pytest.mark.parametrize("name", NAMES)
def test_tv_plans_the_intended_grid(name, hip):
    from astrild_amd import _lib, device as dev
    pos, vel, par = catalogue(name)
    _, _, cond = pg.CATALOGUES[name]()
    n, binnr, bw = len(pos), par["binnr"], par["binwidth"]
    p, v = dev.as_device(pos), dev.as_device(vel)
    ws_bytes = hip.ast_pairwise_workspace_bytes(n, binnr)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    s = dev.stream()
    _lib.check(hip.ast_pairwise_tv_prepare(dev.ptr(p), _lib.F64, dev.ptr(v), _lib.F64, 3, None, None, 0, n, dev.ptr(work),
                                           ws_bytes, s), "ast_pairwise_tv_prepare")
    for single in (0, 1, 0):
        nom = torch.full((binnr,), float("nan"), dtype=torch.float64, device="cuda")
        den = torch.full((binnr,), float("nan"), dtype=torch.float64, device="cuda")
        cnt = torch.full((binnr,), -1, dtype=torch.int64, device="cuda")
        _lib.check(hip.ast_pairwise_tv(dev.ptr(work), ws_bytes, n, binnr, bw, single, dev.ptr(nom), dev.ptr(den),
                                       dev.ptr(cnt), s), "ast_pairwise_tv")
        assert_planned(work, pos, binnr * bw, single, f"{name} single={single}")
        if not single:
            assert read_grid_params(work)["dims"].tolist() == list(cond["dims"])
        assert_tv((nom.cpu().numpy(), den.cpu().numpy(), cnt.cpu().numpy()), tv_oracle(name), f"{name} C single={single}")


@pytest.mark.parametrize("name", NAMES)
def test_pdf_plans_the_intended_grid(name, hip):
    from astrild_amd import _lib, device as dev
    pos, vel, par = catalogue(name)
    _, _, cond = pg.CATALOGUES[name]()
    n, pp = len(pos), pdf_par(par)
    db, vb = pp["dist_bin"], pp["vel_bin"]
    p, v = dev.as_device(pos), dev.as_device(vel)
    ws_bytes = hip.ast_pairwise_pdf_workspace_bytes(n, db, vb, 1)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    st = dev.stream()
    _lib.check(hip.ast_pairwise_pdf_prepare(dev.ptr(p), _lib.F64, dev.ptr(v), _lib.F64, n, dev.ptr(work), ws_bytes, st),
               "ast_pairwise_pdf_prepare")
    for kind, single in (("radial", 0), ("z_sign", 1), ("z_sign", 0)):
        hist = torch.full((db, vb), -1, dtype=torch.int64, device="cuda")
        outside = torch.full((), -1, dtype=torch.int64, device="cuda")
        count = torch.full((db,), -1, dtype=torch.int64, device="cuda")
        s1 = torch.full((db,), float("nan"), dtype=torch.float64, device="cuda")
        s2 = torch.full((db,), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(hip.ast_pairwise_pdf(dev.ptr(work), ws_bytes, n, _lib.PVPDF_KIND[kind], pp["r"], db, vb, pp["dist_width"],
                                        pp["vel_width"], 0, n, single, 0, dev.ptr(hist), dev.ptr(outside), dev.ptr(s1),
                                        dev.ptr(s2), dev.ptr(count), st), "ast_pairwise_pdf")
        assert_planned(work, pos, float(np.float32(pp["r"])), single, f"{name} single={single}")
        if not single:
            assert read_grid_params(work)["dims"].tolist() == list(cond["dims"])
        got = dict(hist=hist.cpu().numpy(), outside=int(outside.item()), count=count.cpu().numpy(), s1=s1.cpu().numpy(),
                   s2=s2.cpu().numpy())
        assert_pdf(got, pdf_oracle(name, kind), f"{name} {kind} C single={single}")


# ------------------------------------------------------------------ dtype pairings
MIXED = [(F32, F64), (F64, F32)]


@pytest.mark.parametrize("cells", list(CELLS))
@pytest.mark.parametrize("dtypes", MIXED, ids=["pos32_vel64", "pos64_vel32"])
@pytest.mark.parametrize("name", ["offset_f32", "crowded_neighbours"])
def test_tv_mixed_dtypes(name, dtypes, cells, monkeypatch):
    monkeypatch.setenv("ASTRILD_PV_CELLS", CELLS[cells])
    pos, vel, par = catalogue(name, *dtypes)
    assert (pos.dtype, vel.dtype) == dtypes
    ref = tv_oracle(name, *dtypes)
    if name == "crowded_neighbours":                        # the rounding of either input is visible to the oracle
        assert not np.array_equal(ref[0], tv_oracle(name)[0])
    assert_tv(gpu_tv(pos, vel, par["binnr"], par["binwidth"]), ref, f"{name} {cells} mixed")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtypes", MIXED, ids=["pos32_vel64", "pos64_vel32"])
@pytest.mark.parametrize("name", ["offset_f32", "crowded_neighbours"])
def test_pdf_mixed_dtypes(name, dtypes, kind):
    pos, vel, par = catalogue(name, *dtypes)
    assert (pos.dtype, vel.dtype) == dtypes
    ref = pdf_oracle(name, kind, *dtypes)
    if name == "crowded_neighbours":
        assert not np.array_equal(ref["s1"], pdf_oracle(name, kind)["s1"])
    assert_pdf(gpu_pdf(pos, vel, kind, **pdf_par(par)), ref, f"{name} {kind} mixed")


# ------------------------------------------------------------------ the bin limits of ast_pairwise_tv
def test_tv_at_the_bin_limit(hip):
    """480 bins fill 64 512 of the 65 536 bytes of LDS: 9 x 256 x 8 for the j stage, 4 x 480 x 24 for the histograms."""
    binnr = hip.ast_pairwise_max_bins()
    assert binnr == 480 and 9 * 256 * 8 + 4 * binnr * 24 == 64512 <= 65536
    pos, vel, _ = catalogue("one_cell_513")
    ref = tv_oracle("one_cell_513", binnr=binnr, binwidth=0.02)
    assert np.count_nonzero(ref[2]) >= 400 and ref[2][-1] > 0 and ref[2].sum() < 513 * 512 // 2
    assert_tv(gpu_tv(pos, vel, binnr, 0.02), ref, "480 bins")


@pytest.mark.parametrize("name", ["one_cell_513", "corners", "crowded_neighbours"])
def test_tv_with_one_bin(name):
    pos, vel, par = catalogue(name)
    reach = par["binnr"] * par["binwidth"]
    ref = tv_oracle(name, binnr=1, binwidth=reach)
    assert ref[2].tolist() == [tv_oracle(name)[2].sum()]
    assert_tv(gpu_tv(pos, vel, 1, reach), ref, f"{name} one bin")


def test_tv_refuses_one_bin_too_many(hip):
    from astrild_amd import _lib, device as dev
    pos, vel, par = catalogue("one_cell_257")
    n, too_many = len(pos), hip.ast_pairwise_max_bins() + 1
    with pytest.raises(ValueError):
        dev.pairwise_tv(pos, vel, too_many, 0.02)
    with pytest.raises(ValueError):
        dev.pairwise_tv(pos, vel, 0, 0.02)
    assert hip.ast_pairwise_workspace_bytes(n, too_many) == 0
    ws_bytes = hip.ast_pairwise_workspace_bytes(n, too_many - 1)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    p, v = dev.as_device(pos), dev.as_device(vel)
    s = dev.stream()
    _lib.check(hip.ast_pairwise_tv_prepare(dev.ptr(p), _lib.F64, dev.ptr(v), _lib.F64, 3, None, None, 0, n, dev.ptr(work),
                                           ws_bytes, s), "ast_pairwise_tv_prepare")

    def run(binnr, bw):
        out = (torch.full((binnr,), float("nan"), dtype=torch.float64, device="cuda"),
               torch.full((binnr,), float("nan"), dtype=torch.float64, device="cuda"),
               torch.full((binnr,), -1, dtype=torch.int64, device="cuda"))
        rc = hip.ast_pairwise_tv(dev.ptr(work), ws_bytes, n, binnr, bw, 0, dev.ptr(out[0]), dev.ptr(out[1]), dev.ptr(out[2]), s)
        return rc, tuple(t.cpu().numpy() for t in out)
    rc, out = run(too_many, 0.02)
    assert rc != 0 and b"binnr" in hip.ast_last_error()
    assert np.isnan(out[0]).all() and np.isnan(out[1]).all() and np.all(out[2] == -1)     # nothing was written
    rc, out = run(par["binnr"], par["binwidth"])
    assert rc == 0
    assert_tv(out, tv_oracle("one_cell_257"), "after the refusal")


# ------------------------------------------------------------------ row ranges on a multi-cell grid
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["plane", "crowded_neighbours"])
def test_pdf_row_ranges_on_a_grid(name, kind):
    """The row of a pair is the smaller of its two original indices, after the sort by cell has moved everything."""
    pos, vel, par = catalogue(name)
    n, pp = len(pos), pdf_par(par)
    assert np.prod(pg.plan(pos, pp["r"]).dims) > 1
    cuts = [0, n // 5, n // 5 + n // 2, n]
    whole = pdf_oracle(name, kind)
    parts = [gpu_pdf(pos, vel, kind, ffirst=a, ssecond=b, **pp) for a, b in zip(cuts[:-1], cuts[1:])]
    assert all(q["hist"].sum() > 0 for q in parts)
    npt.assert_array_equal(sum(q["hist"] for q in parts), whole["hist"])
    assert sum(q["outside"] for q in parts) == whole["outside"]
    npt.assert_array_equal(sum(q["count"] for q in parts), whole["count"])
    assert_pdf(parts[1], pdf_oracle(name, kind, ffirst=cuts[1], ssecond=cuts[2]), f"{name} {kind} rows {cuts[1]}-{cuts[2]}")


# ------------------------------------------------------------------ repeat
def test_two_runs_of_crowded_neighbours_agree():
    pos, vel, par = catalogue("crowded_neighbours")
    ref = tv_oracle("crowded_neighbours")
    a, b = (gpu_tv(pos, vel, par["binnr"], par["binwidth"]) for _ in range(2))
    npt.assert_array_equal(a[2], b[2])
    within("pairwise_tv", "repeat nom", a[0], b[0], ref[2], ref[3])
    within("pairwise_tv", "repeat denom", a[1], b[1], ref[2], ref[1])
    for kind in KINDS:
        ref = pdf_oracle("crowded_neighbours", kind)
        a, b = (gpu_pdf(pos, vel, kind, **pdf_par(par)) for _ in range(2))
        npt.assert_array_equal(a["hist"], b["hist"])
        assert a["outside"] == b["outside"]
        npt.assert_array_equal(a["count"], b["count"])
        within("pairwise_pdf", "repeat s1", a["s1"], b["s1"], ref["count"], ref["sum_abs"])
        within("pairwise_pdf", "repeat s2", a["s2"], b["s2"], ref["count"], ref["s2"])
