"""CPU-only: the numpy oracle of the pairwise-velocity moments in a box (tests/pair_velocity_oracle.py) against its
enumerated known answers and against the two-point correlation function's oracle, the sensitivity of those known answers
to a wrong wrap, and the host-side parts of the feature (check_pair_velocity_args, finish_pair_velocity,
SubFind.mean_pairwise_velocity's defaults, split and units).  No GPU."""
import types

import numpy as np
import numpy.testing as npt
import pytest

from astrild_amd.particles.hutils import pair_velocity_box          # noqa: F401  (the feature under test)
from tests import pair_velocity_oracle as orc
from tests import tpcf_cross_oracle as xorc
from tests import tpcf_oracle as torc

KINDS = ("radial", "los")


def lattice_moments(kind, axis, **kw):
    p1, v1, p2, v2 = orc.parity_lattice_case(axis)
    if kind == "radial":
        return orc.moments_brute(p1, v1, orc.LATTICE_R_EDGES, p2, v2, boxsize=8.0, **kw)
    return orc.moments_brute(p1, v1, orc.LATTICE_RP_EDGES, p2, v2, boxsize=8.0, kind="los", pi_max=orc.LATTICE_PI_MAX,
                             los=axis, **kw)


def corner_moments(kind, los=2, **kw):
    p1, v1, p2, v2 = orc.corner_case()
    if kind == "radial":
        return orc.moments_brute(p1, v1, orc.CORNER_R_EDGES, p2, v2, boxsize=8.0, **kw)
    return orc.moments_brute(p1, v1, orc.CORNER_RP_EDGES, p2, v2, boxsize=8.0, kind="los", pi_max=orc.CORNER_PI_MAX,
                             los=los, **kw)


# ---------------------------------------------------------------- known answers
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_reproduces_the_parity_lattice(kind, axis):
    count, s1, s2 = lattice_moments(kind, axis)
    ecount, es1, es2 = orc.parity_lattice_expected(kind, axis)
    npt.assert_array_equal(count, ecount)
    # sum v cancels term by term (q against -q, equal magnitudes): what is left is the rounding of a sum of count
    # terms of at most LATTICE_SPEED each
    assert np.all(np.abs(s1 - es1) <= orc.sum_bound(count, orc.LATTICE_SPEED * count))
    npt.assert_allclose(s2, es2, rtol=(count.max() + 16) * 2.0 ** -52)
    if kind == "radial":
        # |q|^2 = 1, (none in (1.44, 2.56]), 3, (none), 5: 6, 0, 8, 0, 24 vectors
        assert count.tolist() == [1536, 0, 2048, 0, 6144]
        npt.assert_allclose(es2, 256 * 9.0 * np.array([2.0, 0.0, 8.0 / 3.0, 0.0, 8.0]), rtol=1e-15)
    else:
        # rp^2 = 1 with q_los in {0, +-2}, rp^2 = 2 with q_los = +-1, rp^2 = 4 with q_los = +-1
        assert count.tolist() == [3072, 2048, 2048]
        assert es2.tolist() == [256 * 9.0 * 8, 256 * 9.0 * 8, 256 * 9.0 * 8]


@pytest.mark.parametrize("los", [0, 1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_reproduces_the_infall_across_a_corner(kind, los):
    count, s1, s2 = corner_moments(kind, los)
    ecount, es1, es2 = orc.corner_expected(kind, los)
    npt.assert_array_equal(count, ecount)
    rtol = (count.max() + 16) * 2.0 ** -52
    npt.assert_allclose(s1, es1, rtol=rtol)
    npt.assert_allclose(s2, es2, rtol=rtol)
    assert np.all(s1 < 0)                                           # infall
    if kind == "radial":
        assert count.tolist() == [4, 13, 21, 40]
    else:
        # 3, 5 and 5 lattice columns in the rp bins, each with five sites within pi_max (|s_los| = 0.25 .. 2.25)
        assert count.tolist() == [15, 25, 25]


def test_oracle_sees_the_boundary_pairs_with_their_sign():
    pa, va, pb, vb, expected = orc.boundary_pairs()
    for p1, v1, p2, v2 in ((pa, va, pb, vb), (pb, vb, pa, va)):
        count, s1, s2 = orc.moments_brute(p1, v1, orc.BOUNDARY_EDGES, p2, v2, boxsize=orc.BOUNDARY_BOX)
        assert count.tolist() == [3, 3, 1]
        assert s1.tolist() == expected.tolist()
    count, s1, _ = orc.moments_brute(np.concatenate([pa, pb]), np.concatenate([va, vb]), orc.BOUNDARY_EDGES,
                                     boxsize=orc.BOUNDARY_BOX)
    assert count.tolist() == [3, 3, 1] and s1.tolist() == expected.tolist()
    for dtype in (np.float32, np.float64):                          # every number is exact in float32
        for x in (pa, pb, vb):
            npt.assert_array_equal(x.astype(dtype).astype(np.float64), x)
    # open boundaries: none of the pairs is within reach
    assert orc.moments_brute(pa, va, orc.BOUNDARY_EDGES, pb, vb)[0].sum() == 0


# ---------------------------------------------------------------- a wrong wrap fails the known answers
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("wrap", ["none", "wrong_way", "mirrored"])
def test_a_wrong_wrap_fails_the_corner(kind, wrap):
    count, s1, s2 = corner_moments(kind, wrap=wrap)
    ecount, es1, es2 = orc.corner_expected(kind)
    if wrap == "mirrored":
        # the right magnitudes, so the same pairs; radial: the pairs across a face get a wrong cosine, and the infall
        # turns into outflow for some; los: sign(s_los) flips for the sites across the z face
        npt.assert_array_equal(count, ecount)
        assert np.any(np.abs(s1 - es1) > 0.1 * np.abs(es1))
    else:
        assert count.sum() < ecount.sum()                           # the pairs across the faces are lost


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("wrap", ["none", "wrong_way"])
def test_a_missing_wrap_fails_the_lattice(kind, wrap):
    # (a wrap with the right magnitude and the wrong sign leaves the lattice's count, its cancelling sum v and its
    # sum v^2 alone: that mistake is the corner's and the boundary pairs' to catch)
    count = lattice_moments(kind, 2, wrap=wrap)[0]
    ecount = orc.parity_lattice_expected(kind, 2)[0]
    assert np.all(count[ecount > 0] < ecount[ecount > 0])


@pytest.mark.parametrize("wrap", ["none", "wrong_way", "mirrored"])
def test_a_wrong_wrap_fails_the_boundary_pairs(wrap):
    pa, va, pb, vb, expected = orc.boundary_pairs()
    count, s1, _ = orc.moments_brute(pa, va, orc.BOUNDARY_EDGES, pb, vb, boxsize=orc.BOUNDARY_BOX, wrap=wrap)
    assert s1.tolist() != expected.tolist()
    if wrap == "mirrored":
        assert count.tolist() == [3, 3, 1] and np.all(s1 < 0)


# ---------------------------------------------------------------- the separation rule and the TPCF's counts
def _edge_points(n, box, seed, dtype):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, box, (n, 3)).astype(dtype)
    pos[:12] = np.array([0.0, box, box / 2.0, 0.0] * 9, dtype=dtype).reshape(12, 3)
    pos[12:15] = [[0.0, 0.0, 0.0], [box, box, box], [box / 2.0, box / 2.0, box / 2.0]]
    return pos.astype(np.float64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_signed_wrap_is_antisymmetric_and_has_the_minimum_image_magnitude(dtype):
    box = 100.0
    a, b = _edge_points(700, box, 5, dtype), _edge_points(900, box, 6, dtype)
    x, y = a[:, None, :], b[None, :, :]
    s, t = orc.signed_sep(x, y, box), orc.signed_sep(y, x, box)
    npt.assert_array_equal(s, -t)
    d = np.abs(x - y)
    npt.assert_array_equal(np.abs(s), np.minimum(d, box - d))
    assert np.all(np.abs(s) <= box / 2.0)
    assert (np.abs(s) == box / 2.0).any() and (s == 0.0).any()
    npt.assert_array_equal(orc.signed_sep(x, y, None), y - x)


@pytest.mark.parametrize("boxsize", [100.0, None])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_radial_counts_are_the_tpcf_cross_counts(dtype, boxsize):
    edges = [0, 1, 3, 7, 15, 33]
    a, b = _edge_points(700, 100.0, 7, dtype), _edge_points(900, 100.0, 8, dtype)
    rng = np.random.default_rng(9)
    va, vb = rng.normal(0.0, 300.0, a.shape), rng.normal(0.0, 300.0, b.shape)
    count = orc.moments_brute(a, va, edges, b, vb, boxsize=boxsize)[0]
    npt.assert_array_equal(count, xorc.cross_counts_brute(a, b, edges, boxsize=boxsize))
    auto = orc.moments_brute(a, va, edges, boxsize=boxsize)[0]
    ref = torc.pair_counts_brute(a, boxsize, edges) if boxsize else xorc.auto_counts_open_brute(a, edges)
    npt.assert_array_equal(auto, ref)
    assert count.min() > 0


@pytest.mark.parametrize("kind", KINDS)
def test_v_is_unchanged_under_swapping_the_pair(kind):
    a, b = _edge_points(300, 100.0, 17, np.float32), _edge_points(200, 100.0, 18, np.float64)
    rng = np.random.default_rng(19)
    va, vb = rng.normal(0.0, 300.0, a.shape), rng.normal(0.0, 300.0, b.shape)
    kw = dict(boxsize=100.0, kind=kind, pi_max=20.0, los=1)
    c1, s1, q1, a1 = orc.moments_brute(a, va, [0, 5, 10, 30], b, vb, with_abs=True, **kw)
    c2, s2, q2, a2 = orc.moments_brute(b, vb, [0, 5, 10, 30], a, va, with_abs=True, **kw)
    npt.assert_array_equal(c1, c2)
    assert np.all(np.abs(s1 - s2) <= orc.sum_bound(c1, a1)) and np.all(np.abs(q1 - q2) <= orc.sum_bound(c1, q1))
    # auto = half of the cross term of a set with itself
    c3, s3, q3 = orc.moments_brute(a, va, [0, 5, 10, 30], **kw)
    c4, s4, q4, a4 = orc.moments_brute(a, va, [0, 5, 10, 30], a, va, with_abs=True, **kw)
    npt.assert_array_equal(2 * c3, c4)
    assert np.all(np.abs(2 * s3 - s4) <= orc.sum_bound(c4, a4)) and np.all(np.abs(2 * q3 - q4) <= orc.sum_bound(c4, q4))


@pytest.mark.parametrize("auto", [False, True])
@pytest.mark.parametrize("boxsize", [100.0, None])
@pytest.mark.parametrize("kind", KINDS)
def test_tree_oracle_equals_brute_force(kind, boxsize, auto):
    pytest.importorskip("scipy")
    a, b = _edge_points(700, 100.0, 27, np.float64), _edge_points(900, 100.0, 28, np.float32)
    rng = np.random.default_rng(29)
    va, vb = rng.normal(0.0, 300.0, a.shape), rng.normal(0.0, 300.0, b.shape)
    args = (a, va, [0, 1, 3, 7, 15, 33]) + (() if auto else (b, vb))
    kw = dict(boxsize=boxsize, kind=kind, pi_max=30.0, los=0)
    c1, s1, q1, a1 = orc.moments_brute(*args, with_abs=True, **kw)
    c2, s2, q2, a2 = orc.moments(*args, with_abs=True, **kw)
    npt.assert_array_equal(c1, c2)
    assert c1.min() > 0
    assert np.all(np.abs(s1 - s2) <= orc.sum_bound(c1, a1)) and np.all(np.abs(q1 - q2) <= orc.sum_bound(c1, q1))
    assert np.all(np.abs(a1 - a2) <= orc.sum_bound(c1, a1))


# ---------------------------------------------------------------- host-side argument checks
GOOD = dict(pos1_shape=(10, 3), vel1_shape=(10, 3), edges=[0.0, 1.0, 2.0])


def check(**kw):
    from astrild_amd import device as dev
    args = dict(GOOD)
    args.update(kw)
    return dev.check_pair_velocity_args(**args)


def test_good_arguments_pass_without_a_library_call(monkeypatch):
    from astrild_amd import _lib

    def no_library():
        raise AssertionError("check_pair_velocity_args called into the library")
    monkeypatch.setattr(_lib, "lib", no_library)
    e, box, pmax, n1, n2 = check()
    assert e.dtype == np.float64 and e.tolist() == [0.0, 1.0, 2.0] and (box, pmax, n1, n2) == (0.0, 0.0, 10, 0)
    e, box, pmax, n1, n2 = check(pos2_shape=(4, 3), vel2_shape=(4, 3), boxsize=9.0, kind="los", pi_max=2.5, los=0)
    assert (box, pmax, n1, n2) == (9.0, 2.5, 10, 4)
    assert check(pos1_shape=(0, 3), vel1_shape=(0, 3))[3] == 0
    assert check(edges=np.linspace(0.0, 1.0, _lib.PAIRVEL_MAX_BINS + 1))[0].size == _lib.PAIRVEL_MAX_BINS + 1
    assert check(boxsize=30.0, edges=[0.0, np.nextafter(10.0, 0.0)])[1] == 30.0
    assert check(kind="los", pi_max=1e9)[2] == 1e9                  # open boundaries: pi_max is free


BAD = {
    "edges not increasing": dict(edges=[0.0, 1.0, 1.0]),
    "edges decreasing": dict(edges=[2.0, 1.0]),
    "edges not finite": dict(edges=[0.0, 1.0, np.inf]),
    "edges nan": dict(edges=[0.0, np.nan, 2.0]),
    "edges negative": dict(edges=[-1.0, 1.0]),
    "one edge": dict(edges=[1.0]),
    "top edge at a third of the box": dict(edges=[0.0, 10.0], boxsize=30.0),
    "pi_max at a third of the box": dict(kind="los", pi_max=10.0, boxsize=30.0),
    "boxsize zero": dict(boxsize=0.0),
    "boxsize not finite": dict(boxsize=np.inf),
    "pi_max missing": dict(kind="los"),
    "pi_max zero": dict(kind="los", pi_max=0.0),
    "pi_max negative": dict(kind="los", pi_max=-1.0),
    "pi_max not finite": dict(kind="los", pi_max=np.inf),
    "pi_max nan": dict(kind="los", pi_max=np.nan),
    "los 3": dict(los=3),
    "los -1": dict(los=-1),
    "los 1.5": dict(los=1.5),
    "los None": dict(los=None),
    "kind z_sign": dict(kind="z_sign"),
    "kind None": dict(kind=None),
    "pos (N, 2)": dict(pos1_shape=(10, 2), vel1_shape=(10, 2)),
    "pos flat": dict(pos1_shape=(30,), vel1_shape=(30,)),
    "vel of another length": dict(vel1_shape=(9, 3)),
    "vel missing": dict(vel1_shape=None),
    "vel2 without pos2": dict(vel2_shape=(4, 3)),
    "pos2 without vel2": dict(pos2_shape=(4, 3)),
    "vel2 of another shape": dict(pos2_shape=(4, 3), vel2_shape=(5, 3)),
    "pos2 (N, 4)": dict(pos2_shape=(4, 4), vel2_shape=(4, 4)),
    "too many bins": dict(edges=np.arange(514.0)),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_raise_before_any_library_call(case, monkeypatch):
    from astrild_amd import _lib

    def no_library():
        raise AssertionError("check_pair_velocity_args called into the library")
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(ValueError):
        check(**BAD[case])


def test_the_bin_limit_is_the_header_s():
    import os
    import re
    from astrild_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "astrild_hip.h")).read()
    assert int(re.search(r"#define\s+AST_PAIRVEL_MAX_BINS\s+(\d+)", header).group(1)) == _lib.PAIRVEL_MAX_BINS
    assert _lib.lib().ast_pairvel_max_bins() == _lib.PAIRVEL_MAX_BINS              # host-only call
    assert _lib.lib().ast_pairvel_workspace_bytes(10, 10, _lib.PAIRVEL_MAX_BINS + 1) == 0
    assert _lib.lib().ast_pairvel_workspace_bytes(10, 10, 0) == 0
    assert _lib.lib().ast_pairvel_workspace_bytes(10, 10, _lib.PAIRVEL_MAX_BINS) > 0
    for kind, code in _lib.PAIRVEL_KIND.items():
        assert int(re.search(rf"#define\s+AST_PAIRVEL_{kind.upper()}\s+(\d+)", header).group(1)) == code


def test_the_wrapper_checks_before_it_touches_the_library(monkeypatch):
    from astrild_amd import _lib, device as dev

    def no_library():
        raise AssertionError("pair_velocity_moments called into the library before its checks")
    monkeypatch.setattr(_lib, "lib", no_library)
    pos, vel = np.zeros((5, 3)), np.zeros((5, 3))
    with pytest.raises(ValueError):
        dev.pair_velocity_moments(pos, vel, [0.0, 1.0], vel2=vel)
    with pytest.raises(ValueError):
        dev.pair_velocity_moments(pos, vel, [0.0, 1.0], pos2=pos)
    with pytest.raises(ValueError):
        dev.pair_velocity_moments(pos, vel[:4], [0.0, 1.0])
    with pytest.raises(ValueError):
        dev.pair_velocity_moments(pos, vel, [0.0, 40.0], boxsize=100.0)


# ---------------------------------------------------------------- finish_pair_velocity
def test_finish_gives_nan_for_empty_bins_and_clamps_sigma():
    from astrild_amd import device as dev
    count = np.array([0, 1, 4, 3], dtype=np.int64)
    v = np.array([0.1, 0.1, 0.1])                                   # three equal velocities: s2 / n - mean^2 rounds below 0
    s1 = np.array([0.0, -7.0, 8.0, v.sum()])
    s2 = np.array([0.0, 49.0, 36.0, (v * v).sum()])
    mean, sigma = dev.finish_pair_velocity(count, s1, s2)
    assert np.isnan(mean[0]) and np.isnan(sigma[0])
    assert mean[1:].tolist() == [-7.0, 2.0, s1[3] / 3.0]
    assert sigma[1] == 0.0 and sigma[2] == np.sqrt(36.0 / 4.0 - 4.0) and sigma[3] == 0.0
    assert s2[3] / 3.0 - (s1[3] / 3.0) ** 2 < 0                     # the clamp was needed
    om, osig = orc.finish(count, s1, s2)
    npt.assert_array_equal(mean, om)
    npt.assert_array_equal(sigma, osig)
    assert mean.dtype == np.float64 and sigma.dtype == np.float64


# ---------------------------------------------------------------- SubFind.mean_pairwise_velocity
def _snapshot(n=400, box_kpc=30000.0, hubble=0.7, seed=31):
    rng = np.random.default_rng(seed)
    cat = {
        "GroupPos": rng.uniform(0.0, 0.999 * box_kpc / hubble, (n, 3)),
        "GroupVel": rng.normal(0.0, 300.0, (n, 3)),
        "Group_M_Crit200": 10.0 ** rng.uniform(12.0, 15.0, n),
    }
    return types.SimpleNamespace(cat=cat, header=types.SimpleNamespace(boxsize=box_kpc, hubble=hubble))


def _patch_moments(monkeypatch, calls):
    """device.pair_velocity_moments -> the oracle, recording what it was given."""
    import torch
    from astrild_amd import device as dev

    def fake(pos1, vel1, edges, pos2=None, vel2=None, boxsize=None, kind="radial", pi_max=None, los=2):
        calls.append(dict(pos1=pos1, vel1=vel1, edges=np.asarray(edges), pos2=pos2, vel2=vel2, boxsize=boxsize,
                          kind=kind))
        return tuple(torch.from_numpy(x) for x in orc.moments_brute(pos1, vel1, edges, pos2, vel2, boxsize=boxsize,
                                                                    kind=kind, pi_max=pi_max, los=los))
    monkeypatch.setattr(dev, "pair_velocity_moments", fake)


def test_subfind_defaults_split_and_units(monkeypatch):
    from astrild_amd.particles.hutils import SubFind
    snap = _snapshot()
    calls = []
    _patch_moments(monkeypatch, calls)
    r_c, v12 = SubFind.mean_pairwise_velocity(snap, seperate={"Group_M_Crit200": 14, "compare": [1, 2]})
    c = calls[-1]
    # boxsize = 30000 / 1e3 = 30, limits = (0.3, 6), nbins = int(2 / 3 * 6) = 4 edges, 3 bins
    edges = np.geomspace(0.3, 30.0 / 5, 4)
    assert c["boxsize"] == 30.0 and c["kind"] == "radial"
    npt.assert_array_equal(c["edges"], edges)
    npt.assert_array_equal(r_c, 0.5 * (edges[1:] + edges[:-1]))
    assert len(r_c) == len(v12) == 3
    m = snap.cat["Group_M_Crit200"]
    low, high = m < 1e14, m > 1e14
    assert 0 < high.sum() < low.sum()
    npt.assert_array_equal(c["pos1"], snap.cat["GroupPos"][low] * 0.7 / 1e3)
    npt.assert_array_equal(c["vel1"], snap.cat["GroupVel"][low])
    npt.assert_array_equal(c["pos2"], snap.cat["GroupPos"][high] * 0.7 / 1e3)
    npt.assert_array_equal(c["vel2"], snap.cat["GroupVel"][high])
    count, s1, s2 = orc.moments_brute(c["pos1"], c["vel1"], edges, c["pos2"], c["vel2"], boxsize=30.0)
    npt.assert_array_equal(v12, orc.finish(count, s1, s2)[0])
    assert count[-1] > 0 and np.isfinite(v12[-1])

    # the compare codes: [2, 1] swaps the groups, [2, 2] takes the heavy ones twice
    SubFind.mean_pairwise_velocity(snap, seperate={"Group_M_Crit200": 14, "compare": [2, 1]})
    assert len(calls[-1]["pos1"]) == high.sum() and len(calls[-1]["pos2"]) == low.sum()
    SubFind.mean_pairwise_velocity(snap, seperate={"Group_M_Crit200": 14, "compare": [2, 2]})
    assert len(calls[-1]["pos1"]) == high.sum() and len(calls[-1]["pos2"]) == high.sum()
    # another threshold; no split: every halo in both groups
    SubFind.mean_pairwise_velocity(snap, seperate={"Group_M_Crit200": 13, "compare": [1, 2]})
    assert len(calls[-1]["pos1"]) == (m < 1e13).sum() and len(calls[-1]["pos2"]) == (m > 1e13).sum()
    SubFind.mean_pairwise_velocity(snap)
    assert len(calls[-1]["pos1"]) == len(calls[-1]["pos2"]) == len(m)
    # explicit arguments win over the defaults
    r_c, v12 = SubFind.mean_pairwise_velocity(snap, limits=(0.5, 4.0), nbins=6, boxsize=40.0)
    npt.assert_array_equal(calls[-1]["edges"], np.geomspace(0.5, 4.0, 6))
    assert calls[-1]["boxsize"] == 40.0 and len(r_c) == len(v12) == 5


def test_public_functions_on_the_oracle(monkeypatch):
    from astrild_amd.particles import hutils
    calls = []
    _patch_moments(monkeypatch, calls)
    a, b = _edge_points(150, 50.0, 41, np.float64), _edge_points(120, 50.0, 42, np.float64)
    rng = np.random.default_rng(43)
    va, vb = rng.normal(0.0, 300.0, a.shape), rng.normal(0.0, 300.0, b.shape)
    bins = [0.0, 4.0, 9.0, 15.0]
    for p2, v2 in ((None, None), (b, vb)):
        for period in (50.0, None):
            ref = orc.moments_brute(a, va, bins, p2, v2, boxsize=period)
            mean, sigma = orc.finish(*ref)
            npt.assert_array_equal(hutils.mean_radial_velocity_vs_r(a, va, bins, p2, v2, period), mean)
            got, mom = hutils.radial_pvd_vs_r(a, va, bins, sample2=p2, velocities2=v2, period=period,
                                              return_moments=True)
            npt.assert_array_equal(got, sigma)
            assert sorted(mom) == ["count", "sum_v", "sum_v2"] and mom["count"].dtype == np.int64
            npt.assert_array_equal(mom["count"], ref[0])
            npt.assert_array_equal(mom["sum_v"], ref[1])
            npt.assert_array_equal(mom["sum_v2"], ref[2])
            ref = orc.moments_brute(a, va, bins, p2, v2, boxsize=period, kind="los", pi_max=12.0, los=1)
            mean, sigma = orc.finish(*ref)
            npt.assert_array_equal(hutils.mean_los_velocity_vs_rp(a, va, bins, 12.0, p2, v2, period, 1), mean)
            npt.assert_array_equal(hutils.los_pvd_vs_rp(a, va, bins, 12.0, sample2=p2, velocities2=v2, period=period,
                                                        los=1), sigma)
            assert len(mean) == len(bins) - 1
    with pytest.raises(TypeError):
        hutils.mean_radial_velocity_vs_r(a, va, rbins_normalized=bins)
