"""CPU: the watershed oracle (tests/watershed_oracle.py) on hand-built maps whose answers can be written down, and
device.watershed_merge (host-only: numpy and a union-find) against the oracle's independent merge on those maps and on
a 64^2 map of smoothed noise."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import watershed_oracle as orc


def valley(g):
    """A square map with the profile g along its middle row and walls rising by 10 per row away from it: every pixel off
    the middle row links towards it, so the minima are those of g, at flat index mid * npix + x."""
    g = np.asarray(g, dtype=np.float64)
    npix = len(g)
    assert npix % 2 == 1
    y = np.abs(np.arange(npix) - npix // 2)
    return g[None, :] + 10.0 * y[:, None], npix // 2


TWO_WELLS = [3, 1, 2, 4, 2.5, 0, 3]                      # A at x = 1 (1), B at x = 5 (0), pass max(4, 2.5) = 4
CHAIN = [2, 0, 4, 3, 3.5, 1, 5, 6, 7]                    # A (0), B (3), C (1); s_AB = 4, s_BC = 3.5
EQUAL_PASSES = [2, 0, 4, 3, 4, 1, 5, 6, 7]               # A (0), B (3), C (1); s_AB = s_BC = 4


def corner_and_border(npix=7):
    y, x = np.mgrid[0:npix, 0:npix].astype(np.float64)
    return np.minimum(np.hypot(y - (npix - 1), x - (npix - 1)), np.hypot(y, x - 3) + 0.5)


def signed_zero():
    f = np.zeros((3, 3))
    f[1, 1] = -0.0
    return f


def hand_maps():
    return {"two_wells": valley(TWO_WELLS)[0], "chain": valley(CHAIN)[0], "equal": valley(EQUAL_PASSES)[0],
            "constant": np.full((5, 5), 2.5), "zero": signed_zero(), "corner": corner_and_border(),
            "snake": orc.snake(9), "blocks": orc.blocks(24, 8)}


def test_two_wells_and_their_pass():
    f, mid = valley(TWO_WELLS)
    b = orc.basins(f)
    npt.assert_array_equal(b["minima"], [mid * 7 + 1, mid * 7 + 5])
    npt.assert_array_equal(b["f_min"], [1.0, 0.0])
    npt.assert_array_equal(b["labels"][mid], [0, 0, 0, 0, 1, 1, 1])
    npt.assert_array_equal(b["edges"], [[0, 1]])
    npt.assert_array_equal(b["saddle"], [4.0])                       # depth 4 - max(1, 0) = 3
    assert b["area"].sum() == 49 and b["edge_pix"].sum() == 24
    assert b["sum_x"].sum() == 7 * 21 and b["sum_y"].sum() == 7 * 21
    for h, count in ((0.0, 2), (2.999, 2), (3.0, 2), (3.001, 1), (np.inf, 1)):
        vob, roots = orc.merge(b, h)
        assert len(roots) == count, h
    vob, roots = orc.merge(b, 3.001)
    npt.assert_array_equal(vob, [0, 0])
    npt.assert_array_equal(roots, [1])                               # B is the deeper well
    v = orc.voids(b, vob, roots)
    assert v["area"][0] == 49 and v["kappa_min"][0] == 0.0 and v["min_index"][0] == mid * 7 + 5
    assert v["x"][0] == 3.0 and v["y"][0] == 3.0 and v["rad"][0] == np.sqrt(49 / np.pi)
    assert v["kappa_mean"][0] == f.sum() / 49


def test_chain_of_three_where_the_ascending_pass_order_decides():
    b = orc.basins(valley(CHAIN)[0])
    npt.assert_array_equal(b["f_min"], [0.0, 3.0, 1.0])
    npt.assert_array_equal(b["edges"], [[0, 1], [1, 2]])
    npt.assert_array_equal(b["saddle"], [4.0, 3.5])
    # B - C first (3.5 - 3 = 0.5 < 2: merged, root C with m = 1), then A - C: 4 - max(0, 1) = 3 >= 2.  Taking A - B
    # first would have merged A and B (4 - 3 = 1 < 2) and left C alone.
    vob, roots = orc.merge(b, 2.0)
    npt.assert_array_equal(vob, [0, 1, 1])
    npt.assert_array_equal(roots, [0, 2])
    npt.assert_array_equal(orc.merge(b, 0.5)[0], [0, 1, 2])
    npt.assert_array_equal(orc.merge(b, 0.5001)[0], [0, 1, 1])
    npt.assert_array_equal(orc.merge(b, 3.0)[0], [0, 1, 1])
    vob, roots = orc.merge(b, 3.0001)
    npt.assert_array_equal(vob, [0, 0, 0])
    npt.assert_array_equal(roots, [0])


def test_two_equal_passes_are_taken_in_the_order_of_the_basin_pair():
    b = orc.basins(valley(EQUAL_PASSES)[0])
    npt.assert_array_equal(b["saddle"], [4.0, 4.0])
    # (4, A, B) before (4, B, C): A and B merge (4 - 3 = 1 < 2, root A), then A - C: 4 - max(0, 1) = 3 >= 2
    vob, roots = orc.merge(b, 2.0)
    npt.assert_array_equal(vob, [0, 0, 1])
    npt.assert_array_equal(roots, [0, 2])


def test_constant_map_is_one_basin_rooted_at_pixel_0():
    b = orc.basins(np.full((5, 5), 2.5))
    npt.assert_array_equal(b["minima"], [0])
    npt.assert_array_equal(b["area"], [25])
    npt.assert_array_equal(b["edge_pix"], [16])
    assert b["edges"].shape == (0, 2) and b["saddle"].shape == (0,)
    assert np.all(b["labels"] == 0) and b["sum_f"][0] == 62.5
    for h in (0.0, 1.0, np.inf):
        vob, roots = orc.merge(b, h)
        npt.assert_array_equal(vob, [0])


def test_negative_zero_ties_with_positive_zero():
    b = orc.basins(signed_zero())
    npt.assert_array_equal(b["minima"], [0])                         # not pixel 4, which holds -0.0
    assert not np.signbit(b["f_min"][0])
    two = np.array([[1.0, 1.0, 1.0, 1.0], [0.0, 1.0, 1.0, -0.0], [1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]])
    b = orc.basins(two)
    npt.assert_array_equal(b["minima"], [4, 7])
    npt.assert_array_equal(b["saddle"], [1.0])
    zero_pass = np.array([[-1.0, -0.0, -2.0], [5.0, 5.0, 5.0], [5.0, 5.0, 5.0]])
    b = orc.basins(zero_pass)
    npt.assert_array_equal(b["minima"], [0, 2])
    assert b["saddle"][0] == 0.0 and not np.signbit(b["saddle"][0])  # max(-1, -0.0) + 0


def test_minima_in_a_corner_and_on_a_border_row():
    b = orc.basins(corner_and_border())
    npt.assert_array_equal(b["minima"], [3, 48])
    npt.assert_array_equal(b["f_min"], [0.5, 0.0])
    assert b["edge_pix"].sum() == 24 and np.all(b["edge_pix"] > 0)
    assert b["labels"][0, 3] == 0 and b["labels"][6, 6] == 1


def test_snake_is_one_basin_with_long_link_paths():
    for npix, longest in ((17, 144), (33, 544), (65, 2112)):
        f = orc.snake(npix)
        assert orc.longest_path(orc.links(f)) == longest
        b = orc.basins(f)
        assert len(b["minima"]) == 1 and b["minima"][0] == 0 and b["area"][0] == npix * npix


def test_smoothed_noise_counts():
    f = orc.smoothed_noise(64)
    b = orc.basins(f)
    assert len(b["minima"]) == 48 and len(b["edges"]) == 121
    lower = np.maximum(b["f_min"][b["edges"][:, 0]], b["f_min"][b["edges"][:, 1]])
    assert np.all(b["saddle"] >= lower)
    counts = [len(orc.merge(b, nu * f.std())[1]) for nu in (0, 0.25, 0.5, 1, 2, np.inf)]
    assert counts == [48, 35, 27, 15, 3, 1]


def merge_cases():
    cases = [(name, f, h) for name, f in hand_maps().items() for h in (0.0, 0.5, 0.5001, 2.0, 3.0, 3.0001, np.inf)]
    noise = orc.smoothed_noise(64)
    cases += [("noise64", noise, nu * noise.std()) for nu in (0, 0.25, 0.5, 1, 2, np.inf)]
    noise32 = orc.smoothed_noise(64, dtype=np.float32)
    cases += [("noise64_f32", noise32, nu * float(noise32.std())) for nu in (0.25, 1)]
    return cases


def test_device_merge_equals_the_oracle():
    from astrild_amd import device as dev
    cache = {}
    for name, f, h in merge_cases():
        b = cache.setdefault(name, orc.basins(f))
        vob, roots = orc.merge(b, h)
        want = orc.voids(b, vob, roots)
        got = dev.watershed_merge(b, h)
        npt.assert_array_equal(got["void_of_basin"], vob, err_msg=f"{name} h={h}")
        assert got["void_of_basin"].dtype == np.int32
        npt.assert_array_equal(got["root"], roots)
        for k in ("area", "sum_x", "sum_y", "edge_pix", "min_index"):
            npt.assert_array_equal(got[k], want[k], err_msg=f"{name} h={h} {k}")
            assert got[k].dtype == np.int64
        assert got["kappa_min"].tobytes() == want["kappa_min"].tobytes()
        # both add the same float64 basin sums, the oracle exactly rounded: at most (basins - 1) roundings apart
        nb = np.bincount(vob, minlength=len(roots))
        tol = (nb - 1) * 2.0 ** -53 * np.bincount(vob, weights=np.abs(b["sum_f"]), minlength=len(roots))
        assert np.all(np.abs(got["sum_f"] - want["sum_f"]) <= tol)


def test_device_merge_rejects_a_negative_height():
    from astrild_amd import device as dev
    b = orc.basins(valley(TWO_WELLS)[0])
    for h in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            dev.watershed_merge(b, h)


def test_pass_bound_of_the_library():
    """ceil(log2(npix^2)) pointer-jumping passes at most; 0 for a map the library does not take.  A host-only call."""
    from astrild_amd import _lib
    lib = _lib.lib()
    assert [lib.ast_watershed_max_passes(n) for n in (2, 3, 4, 5, 65, 4096, 46340, 46341)] == [0, 4, 4, 5, 13, 24, 31, 0]


def test_map_checks_need_no_gpu():
    from astrild_amd import device as dev
    for bad in (np.zeros((2, 2)), np.zeros((4, 5)), np.zeros((4, 4), dtype=np.int32), np.zeros(16), np.zeros((3, 3, 3))):
        with pytest.raises(ValueError):
            dev.check_watershed_map(bad)
    assert dev.check_watershed_map(np.zeros((3, 3), dtype=np.float32)) == (3, False)
