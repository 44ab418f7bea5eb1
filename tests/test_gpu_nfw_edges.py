"""GPU: the NFW stamp kernels (nfw.hip) at their edges, against the oracle's numpy restatement: one-pixel, even,
clipped, off-map and very large stamps, single-stamp maps over a sweep of sizes and extents, and a catalogue longer
than one launch holds.

Tolerance as in test_gpu_nfw.py: atol = 1e-9 * max|ref|, rtol = 0.  Each edge case is painted on a map of its own, so
the peak the tolerance is relative to is set by that case alone."""
import numpy as np
import numpy.testing as npt
import pytest

from oracle import kappa as ok

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIGNALS = [("alpha", [0]), ("alpha", [1]), ("dT", [0]), ("dT", [1]), ("dT", [0, 1])]


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


def _cat(r200_pix, cen, r200_deg=0.05, m200=7e13, c=2.0, dc=1050.0, tv=(150.0, -80.0)):
    """A catalogue of len(r200_pix) halos; scalars are repeated."""
    nh = len(r200_pix)
    rep = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (nh,)).copy()
    cen = np.asarray(cen).reshape(nh, 2)
    return {"r200_deg": rep(r200_deg), "r200_pix": np.asarray(r200_pix, dtype=np.float64), "m200": rep(m200),
            "c_NFW": rep(c), "Dc": rep(dc), "theta1_pix": cen[:, 0].copy(), "theta2_pix": cen[:, 1].copy(),
            "theta1_tv": rep(tv[0]), "theta2_tv": rep(tv[1])}


def _paint(cat, extent, direction, npix, signal, suppress=False, suppression_R=1):
    from astrild_amd.rays.skys import SkyUtils
    return SkyUtils.analytic_Halo_signal_to_SkyArray(np.arange(len(cat["m200"])), cat, extent, direction, suppress,
                                                     suppression_R, npix, signal)


def _check(cat, extent, direction, npix, signal, ref_cat=None, **kw):
    got = _paint(cat, extent, direction, npix, signal, **kw)
    ref = ok.analytic_halo_signal_map(cat if ref_cat is None else ref_cat, extent, direction, kw.get("suppress", False),
                                      kw.get("suppression_R", 1), npix, signal)
    assert abs(ref).max() > 0.0                       # the case does paint something
    npt.assert_allclose(got, ref, rtol=0, atol=1e-9 * abs(ref).max())
    return got, ref


# ------------------------------------------------------------------ one pixel
@pytest.mark.parametrize("signal,direction", SIGNALS)
@pytest.mark.parametrize("cen", [(2, 2), (0, 0), (4, 0), (3, 4)])
def test_one_pixel_stamp_alone_on_a_small_map(signal, direction, cen):
    """2 * r200_pix * extent < 1: a stamp of one pixel, sampled at (-r200 extent, -r200 extent) as
    np.linspace(0, stop, 1) = [0] has it - both deflection components are negative there."""
    cat = _cat([0.1], [cen])
    assert int(2 * cat["r200_pix"][0] * 3) + 1 == 1
    got, ref = _check(cat, 3, direction, 5, signal)
    assert np.count_nonzero(ref) == 1 and ref[cen[1], cen[0]] != 0.0
    assert np.sign(got[cen[1], cen[0]]) == np.sign(ref[cen[1], cen[0]])
    if signal == "alpha":
        assert got[cen[1], cen[0]] < 0.0


def test_one_pixel_stamps_with_suppression():
    _check(_cat([0.1], [(1, 3)]), 3, [0, 1], 5, "dT", suppress=True, suppression_R=2)


# ------------------------------------------------- single-stamp maps, any size
FULL_SWEEP_EXTENTS = (7, 0.7, 1.1, 3.3, 5, 2, 1, 0.3, 12.5)


def test_single_stamp_size_is_npix_for_every_odd_npix(monkeypatch):
    """Host side: the stamp size that reaches the kernel equals npix.  Deriving it from an r200_pix of
    (npix - 1) / (2 extent) lost a pixel at e.g. (npix, extent) = (123, 7), (231, 7), (245, 7), (7, 0.7), (59, 1.1)."""
    from astrild_amd import lensing
    from astrild_amd.rays.skys import SkyUtils
    seen = []

    def record(cat, extent, direction, suppress, suppression_R, npix, signal, out=None, **kw):
        size = lensing.nfw_stamp_npix(cat, extent, kw.get("stamp_npix"))
        seen.append((npix, extent, int(size[0]), int(cat["theta1_pix"][0]), int(cat["theta2_pix"][0])))
        return np.zeros((npix, npix))

    monkeypatch.setattr(lensing, "nfw_paint", record)
    monkeypatch.setattr("astrild_amd.rays.skys.sky_utils.to_numpy", lambda a: a)
    for extent in FULL_SWEEP_EXTENTS:
        for npix in range(3, 2000, 2):
            SkyUtils.NFW_deflection_angle_map(0.05, 7e13, 2.0, 700.0, npix=npix, extent=extent, direction=[1])
    SkyUtils.NFW_temperature_perturbation_map(0.05, 7e13, 2.0, [1.0, 2.0], 700.0, npix=123, extent=7)
    assert len(seen) == 999 * len(FULL_SWEEP_EXTENTS) + 1
    wrong = [s for s in seen if s[2] != s[0] or s[3] != s[0] // 2 or s[4] != s[0] // 2]
    assert not wrong, wrong[:10]


def _sweep():
    cases = [(7, n) for n in range(3, 256, 2)]                       # 123, 231, 245 lost a pixel
    for extent in (0.7, 1.1, 3.3):
        cases += [(extent, n) for n in range(3, 130, 2)]             # 0.7: 7, 13, 25, ..; 1.1: 59, 83, ..; 3.3: 15, 29, ..
    cases += [(0.7, 193), (0.7, 253), (1.1, 165), (1.1, 233), (3.3, 217), (3.3, 255), (7, 461)]
    return cases


@pytest.mark.parametrize("extent", [7, 0.7, 1.1, 3.3])
def test_single_stamp_maps_over_sizes_and_extents(extent):
    from astrild_amd.rays.skys import SkyUtils
    sizes = [n for e, n in _sweep() if e == extent]
    assert len(sizes) >= 60
    bad = []
    for k, npix in enumerate(sizes):
        d = [k % 2]
        a = SkyUtils.NFW_deflection_angle_map(0.05, 7e13, 2.0, 711.0, npix=npix, extent=extent, direction=d,
                                              suppress=bool(k % 3 == 0), suppression_R=2)
        ra = ok.nfw_deflection_angle_map(0.05, 7e13, 2.0, 711.0, npix, extent, d, bool(k % 3 == 0), 2)
        t = SkyUtils.NFW_temperature_perturbation_map(0.05, 7e13, 2.0, [150.0, -80.0], 711.0, npix=npix, extent=extent)
        rt = ok.nfw_temperature_perturbation_map(0.05, 7e13, 2.0, [150.0, -80.0], 711.0, npix, extent, [0, 1])
        for name, got, ref in (("alpha", a, ra), ("dT", t, rt)):
            assert got.shape == ref.shape == (npix, npix) and abs(ref).max() > 0
            err = abs(got - ref).max() / abs(ref).max()
            if not err <= 1e-9:
                bad.append((name, npix, err))
    assert not bad, bad


@pytest.mark.parametrize("npix,extent", [(123, 7), (231, 7), (245, 7), (7, 0.7), (59, 1.1), (15, 3.3)])
def test_single_stamp_map_at_sizes_that_lost_a_pixel(npix, extent):
    from astrild_amd.rays.skys import SkyUtils
    a = SkyUtils.NFW_deflection_angle_map(0.05, 7e13, 2.0, 711.0, npix=npix, extent=extent, direction=[0])
    ref = ok.nfw_deflection_angle_map(0.05, 7e13, 2.0, 711.0, npix, extent, [0])
    assert np.count_nonzero(a[-1]) > 0 and np.count_nonzero(a[:, -1]) > 0        # last row and column are painted
    npt.assert_allclose(a, ref, rtol=0, atol=1e-9 * abs(ref).max())


def test_stated_stamp_sizes_override_r200_pix_and_are_validated():
    from astrild_amd import lensing
    cat = _cat([3.0, 4.0], [(10, 12), (20, 5)])
    assert lensing.nfw_stamp_npix(cat, 2).tolist() == [13, 17]
    got = lensing.nfw_paint(cat, 2, [0], False, 1, 32, "alpha", stamp_npix=[5, 8]).cpu().numpy()
    ref = np.zeros((32, 32))
    for h, s in enumerate((5, 8)):
        stamp = ok.nfw_deflection_angle_map(0.05, 7e13, 2.0, 1050.0 * 0.6774, s, 2, [0])
        ref = ok.add_patch_to_map(ref, stamp, (cat["theta1_pix"][h], cat["theta2_pix"][h]))
    npt.assert_allclose(got, ref, rtol=0, atol=1e-9 * abs(ref).max())
    for wrong in ([5], [5, 0], [[5, 8]]):
        with pytest.raises(ValueError):
            lensing.nfw_paint(cat, 2, [0], False, 1, 32, "alpha", stamp_npix=wrong)


# ------------------------------------------------------------------ even stamps
def _even_centres(npix, s):
    lo, hi, mid = 0, npix - 1, npix // 2
    cen = [(mid, mid), (lo, mid), (hi, mid), (mid, lo), (mid, hi), (lo, lo), (lo, hi), (hi, lo), (hi, hi),
           (npix, mid), (mid, npix), (npix, npix),                    # x0 = npix - S/2: S/2 columns / rows still on the map
           (-s // 2 + 1, mid), (mid, -s // 2 + 1), (-s // 2 + 1, -s // 2 + 1)]   # only the stamp's last column / row
    return cen


@pytest.mark.parametrize("signal,direction", [("alpha", [0]), ("alpha", [1]), ("dT", [0, 1])])
@pytest.mark.parametrize("r200_pix,size", [(0.5, 2), (1.5, 4), (12.5, 26), (0.75, 2), (12.99, 26)])
def test_even_stamps_inside_and_clipped_at_every_edge_and_corner(r200_pix, size, signal, direction):
    npix = 40
    assert int(2 * r200_pix * 1) + 1 == size
    for cen in _even_centres(npix, size):
        got, ref = _check(_cat([r200_pix], [cen]), 1, direction, npix, signal)
        # the footprint itself: rows and columns that hold anything
        assert np.array_equal(abs(got).sum(axis=0) > 0, abs(ref).sum(axis=0) > 0), cen
        assert np.array_equal(abs(got).sum(axis=1) > 0, abs(ref).sum(axis=1) > 0), cen


def test_even_stamp_footprint_is_cen_minus_half_size():
    got = _paint(_cat([1.5], [(10, 20)]), 1, [0, 1], 40, "dT")
    ys, xs = np.nonzero(got)
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (8, 11, 18, 21)


@pytest.mark.parametrize("size", [2, 4, 26])
def test_add_patch_to_map_with_an_even_stamp(size):
    from astrild_amd.rays.skys import SkyUtils
    rng = np.random.default_rng(size)
    n = 50
    big = rng.standard_normal((n, n))
    small = rng.standard_normal((size, size))
    h = size // 2
    centres = [(25, 25), (0, 25), (25, 0), (n - 1, 25), (25, n - 1), (0, 0), (n - 1, n - 1), (0, n - 1), (n - 1, 0),
               (n, n), (-h + 1, -h + 1), (n + h - 1, 7), (7, n + h - 1),
               (-h, 25), (25, -h), (n + h, 25), (25, n + h), (-500, 10**6)]              # the last five miss the map
    for cen in centres:
        got = SkyUtils.add_patch_to_map(big.copy(), small, cen)
        ref = ok.add_patch_to_map(big.copy(), small, cen)
        assert np.array_equal(got, ref), cen
    for cen in centres[-5:]:
        assert np.array_equal(SkyUtils.add_patch_to_map(big.copy(), small, cen), big), cen


# --------------------------------------------------------------- off the map
def _visible_and_hidden(npix):
    """(r200_pix, centre, m200) rows at extent 2: S = int(4 r) + 1.  Hidden ones are 100 times as massive."""
    vis = [(3.0, (20, 30)), (2.6, (1, 2)), (4.2, (npix - 2, npix - 3)), (3.5, (-7, 40)), (1.0, (50, npix + 1)),
           (2.0, (-4, 10)), (2.0, (npix + 3, 10))]                    # one column or one row of each of the last four
    hid = [(3.0, (-7, 30)), (3.0, (30, -7)), (3.0, (npix + 6, 30)), (3.0, (30, npix + 6)),       # S = 13
           (3.0, (-7, -7)), (3.0, (npix + 6, npix + 6)), (3.0, (-1000, 30)), (3.0, (30, 100000)),
           (2.0, (-5, 10)), (2.0, (npix + 4, 10)), (2.0, (10, -5)), (2.0, (10, npix + 4)),       # S = 9: just off
           (1.75, (-4, 10)), (1.75, (npix + 4, 10)), (1.75, (10, -4)), (1.75, (10, npix + 4)),   # S = 8, even
           (0.1, (-1, 5)), (0.1, (5, npix))]                                                      # S = 1
    return vis, hid


@pytest.mark.parametrize("signal,direction", [("alpha", [0]), ("alpha", [1]), ("dT", [0, 1])])
def test_stamps_wholly_off_the_map_add_nothing(signal, direction):
    npix = 64
    vis, hid = _visible_and_hidden(npix)
    rows = []
    for k in range(max(len(vis), len(hid))):                          # interleaved
        rows += [v + (7e13,) for v in vis[k:k + 1]] + [h + (7e15,) for h in hid[k:k + 1]]
    cat = _cat([r[0] for r in rows], [r[1] for r in rows], m200=[r[2] for r in rows])
    seen = _cat([v[0] for v in vis], [v[1] for v in vis])
    got, ref = _check(cat, 2, direction, npix, signal, ref_cat=seen)
    assert np.array_equal(ok.analytic_halo_signal_map(cat, 2, direction, False, 1, npix, signal), ref)
    # the hidden ones alone: an untouched map
    only = _cat([h[0] for h in hid], [h[1] for h in hid], m200=7e15)
    assert not _paint(only, 2, direction, npix, signal).any()
    # each halo that shows one column or row, alone
    for v in vis[3:]:
        _check(_cat([v[0]], [v[1]]), 2, direction, npix, signal)


# --------------------------------------------------------------- large stamps
LARGE = [(50.0, (256, 256)), (50.0, (500, 505)), (3.0, (40, 470))]


@pytest.mark.parametrize("signal,direction", [("alpha", [1]), ("dT", [0, 1])])
def test_stamps_with_more_pixels_than_one_pass_of_the_grid(signal, direction):
    """S = 301 centred on 512^2: 90 601 in-bounds pixels against 65 536 threads per halo - the grid-stride loop."""
    npix = 512
    assert int(2 * 50.0 * 3) + 1 == 301
    for r, cen in LARGE:
        _check(_cat([r], [cen]), 3, direction, npix, signal, suppress=True, suppression_R=2)
    cat = _cat([h[0] for h in LARGE], [h[1] for h in LARGE], r200_deg=[0.05, 0.05, 0.003])
    _check(cat, 3, direction, npix, signal, suppress=True, suppression_R=2)
    # and a stamp larger than the map itself: every map pixel, 262 144 of them
    _check(_cat([100.0], [(250, 260)]), 3, direction, npix, signal)


# ------------------------------------------------------- a very long catalogue
def test_catalogue_longer_than_one_launch():
    """66 000 halos with S in {3, 5} on 300^2: lensing.nfw_paint splits at 65 535 halos per launch."""
    rng = np.random.default_rng(11)
    nh, npix = 66000, 300
    r200_pix = np.where(rng.random(nh) < 0.5, rng.uniform(1.0, 1.49, nh), rng.uniform(2.0, 2.49, nh))
    assert set(np.unique((2 * r200_pix * 1).astype(int) + 1)) == {3, 5}
    cen = np.stack([rng.integers(-3, npix + 3, nh), rng.integers(-3, npix + 3, nh)], axis=1)
    cat = _cat(r200_pix, cen, r200_deg=rng.uniform(0.02, 0.08, nh), m200=10 ** rng.uniform(13, 13.5, nh),
               c=rng.uniform(2, 8, nh), dc=rng.uniform(500, 2000, nh))
    # the halos of the second launch carry a tenth of the mass: a tail added twice, dropped or read from the wrong
    # offset moves the map by far more than the tolerance either way
    cat["m200"][65535:] *= 0.1
    got, ref = _check(cat, 1, [0], npix, "alpha")
    head = {k: v[:65535] for k, v in cat.items()}
    tail = {k: v[65535:] for k, v in cat.items()}
    ref_tail = ok.analytic_halo_signal_map(tail, 1, [0], False, 1, npix, "alpha")
    assert abs(ref_tail).max() > 1e-3 * abs(ref).max()
    # a difference of two painted maps, each within 1e-9 of the peak: twice the bound
    npt.assert_allclose(got - _paint(head, 1, [0], npix, "alpha"), ref_tail, rtol=0, atol=2e-9 * abs(ref).max())
