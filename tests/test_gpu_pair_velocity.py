"""GPU: the pairwise-velocity moments of one or two samples in a periodic box or with open boundaries
(device.pair_velocity_moments, astrild_amd/csrc/pair_velocity.hip) and the public functions on top of it, against the
numpy oracle tests/pair_velocity_oracle.py, its enumerated known answers, the two-point correlation function's counts
and the moments of the pairwise-velocity histogram kernel.

Tolerances, from the arithmetic and not from a run: counts are exact.  Every term v is computed op by op as the oracle
computes it, so sum v and sum v^2 differ from the oracle's only by the order of two fp64 sums of the same terms: at
most max(count, 8) 2^-52 sum |term| per bin (pair_velocity_oracle.sum_bound).  Against a known answer that replaces v
by a closed form (v = -2 d, v^2 = 9 q_z^2 / |q|^2) the few roundings of a term (a product, a division, a square root,
a square: under 4 x 2^-53 relative) come on top: rtol (count + 16) 2^-52."""
import functools
import types

import numpy as np
import numpy.testing as npt
import pytest

from tests import pair_geometry as pg
from tests import pair_velocity_oracle as orc
from tests import tpcf_oracle as torc
from tests.dirty_memory import dirty_alloc                        # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from astrild_amd.particles.hutils import pair_velocity_box          # noqa: E402, F401  (the feature under test)

KINDS = ("radial", "los")
L = 500.0
S50 = np.linspace(0.0, 50.0, 40)
PI40 = 40.0
CROWD_S = [0, 1, 3, 7, 15, 33]


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


def gpu(pos1, vel1, edges, pos2=None, vel2=None, **kw):
    from astrild_amd import device as dev
    return tuple(dev.to_numpy(x) for x in dev.pair_velocity_moments(pos1, vel1, edges, pos2=pos2, vel2=vel2, **kw))


def assert_moments(got, ref):
    """got = (count, s1, s2) against ref = (count, s1, s2, sum |v|) of the oracle."""
    count, s1, s2, sa = ref
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64 and got[2].dtype == np.float64
    npt.assert_array_equal(got[0], count)
    b1, b2 = orc.sum_bound(count, sa), orc.sum_bound(count, s2)
    assert np.all(np.abs(got[1] - s1) <= b1), (got[1] - s1, b1)
    assert np.all(np.abs(got[2] - s2) <= b2), (got[2] - s2, b2)
    assert not np.isnan(got[1]).any() and not np.isnan(got[2]).any()


# ---------------------------------------------------------------- the enumerated known answers
@pytest.mark.parametrize("cells", ["1", "0"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,axis", [("radial", 2), ("radial", 0), ("los", 0), ("los", 1), ("los", 2)])
def test_parity_lattice(kind, axis, dtype, cells, monkeypatch):
    monkeypatch.setenv("ASTRILD_PAIRVEL_CELLS", cells)
    p1, v1, p2, v2 = orc.parity_lattice_case(axis, dtype)
    if kind == "radial":
        kw = dict(boxsize=8.0)
        edges = orc.LATTICE_R_EDGES
    else:
        kw = dict(boxsize=8.0, kind="los", pi_max=orc.LATTICE_PI_MAX, los=axis)
        edges = orc.LATTICE_RP_EDGES
    got = gpu(p1, v1, edges, p2, v2, **kw)
    ecount, es1, es2 = orc.parity_lattice_expected(kind, axis)
    npt.assert_array_equal(got[0], ecount)
    # q against -q: what is left of sum v is the rounding of a sum of count terms of at most LATTICE_SPEED each
    assert np.all(np.abs(got[1]) <= orc.sum_bound(ecount, orc.LATTICE_SPEED * ecount))
    npt.assert_allclose(got[2], es2, rtol=(ecount.max() + 16) * 2.0 ** -52)
    assert_moments(got, orc.moments_brute(p1, v1, edges, p2, v2, with_abs=True, **kw))
    if kind == "radial" and axis == 2:
        assert got[0].tolist() == [1536, 0, 2048, 0, 6144]
    # the other way round: the odd sites move, so every dv changes sign and every v stays
    swapped = gpu(p2, v2, edges, p1, v1, **kw)
    npt.assert_array_equal(swapped[0], ecount)
    npt.assert_allclose(swapped[2], es2, rtol=(ecount.max() + 16) * 2.0 ** -52)


@pytest.mark.parametrize("cells", ["1", "0"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,los", [("radial", 2), ("los", 0), ("los", 2)])
def test_infall_across_a_corner(kind, los, dtype, cells, monkeypatch):
    monkeypatch.setenv("ASTRILD_PAIRVEL_CELLS", cells)
    p1, v1, p2, v2 = orc.corner_case(dtype)
    if kind == "radial":
        kw = dict(boxsize=8.0)
        edges = orc.CORNER_R_EDGES
    else:
        kw = dict(boxsize=8.0, kind="los", pi_max=orc.CORNER_PI_MAX, los=los)
        edges = orc.CORNER_RP_EDGES
    ecount, es1, es2 = orc.corner_expected(kind, los)
    rtol = (ecount.max() + 16) * 2.0 ** -52
    for got in (gpu(p1, v1, edges, p2, v2, **kw), gpu(p2, v2, edges, p1, v1, **kw)):
        npt.assert_array_equal(got[0], ecount)
        npt.assert_allclose(got[1], es1, rtol=rtol)
        npt.assert_allclose(got[2], es2, rtol=rtol)
        assert np.all(got[1] < 0)
    if kind == "radial":
        assert got[0].tolist() == [4, 13, 21, 40]


@pytest.mark.parametrize("cells", ["1", "0"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_faces_edges_and_corner_of_the_box(dtype, cells, monkeypatch):
    # the radial velocity of pair p is exactly 2^p: sum v per bin names the pairs that were seen, and their sign
    monkeypatch.setenv("ASTRILD_PAIRVEL_CELLS", cells)
    pa, va, pb, vb, expected = (x.astype(dtype) if x.ndim == 2 else x for x in orc.boundary_pairs())
    sq = np.array([1.0 + 4.0 + 16.0, 64.0 + 256.0 + 1024.0, 4096.0])
    for p1, v1, p2, v2 in ((pa, va, pb, vb), (pb, vb, pa, va), (np.concatenate([pa, pb]), np.concatenate([va, vb]),
                                                                None, None)):
        count, s1, s2 = gpu(p1, v1, orc.BOUNDARY_EDGES, p2, v2, boxsize=orc.BOUNDARY_BOX)
        assert count.tolist() == [3, 3, 1]
        assert s1.tolist() == expected.tolist()
        assert s2.tolist() == sq.tolist()
    # open boundaries: the pairs are a box apart
    assert gpu(pa, va, orc.BOUNDARY_EDGES, pb, vb)[0].sum() == 0


# ---------------------------------------------------------------- clustered catalogues against the oracle
@pytest.fixture(scope="module")
def clustered():
    a = torc.clustered(5000, L, 11, blobs=60, sigma=6.0)
    b = torc.clustered(7000, L, 12, blobs=60, sigma=6.0)
    rng = np.random.default_rng(13)
    va, vb = rng.normal(0.0, 300.0, a.shape), rng.normal(0.0, 300.0, b.shape)

    @functools.lru_cache(maxsize=None)
    def ref(mode, periodic, kind):
        kw = dict(boxsize=L if periodic else None, kind=kind, pi_max=PI40, with_abs=True)
        if mode == "auto":
            out = orc.moments(a, va, S50, **kw)
        elif mode == "swapped":
            out = orc.moments(b, vb, S50, a, va, **kw)
        else:
            out = orc.moments(a, va, S50, b, vb, **kw)
        for x in out:
            x.setflags(write=False)
        return out
    return types.SimpleNamespace(a=a, b=b, va=va, vb=vb, ref=ref)


def _args(c, mode):
    return {"auto": (c.a, c.va, S50), "cross": (c.a, c.va, S50, c.b, c.vb), "swapped": (c.b, c.vb, S50, c.a, c.va)}[mode]


def _kw(periodic, kind):
    return dict(boxsize=L if periodic else None, kind=kind, pi_max=PI40 if kind == "los" else None)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
@pytest.mark.parametrize("mode", ["cross", "auto"])
def test_clustered_against_the_oracle(clustered, mode, periodic, kind):
    from astrild_amd import device as dev
    got = gpu(*_args(clustered, mode), **_kw(periodic, kind))
    ref = clustered.ref(mode, periodic, kind)
    assert ref[0].min() > 0
    assert_moments(got, ref)
    if kind == "radial":
        # the parent's kernel, on the same edges: the same pairs exactly
        tp = dev.to_numpy(dev.tpcf_cross_counts(clustered.a, None if mode == "auto" else clustered.b, S50,
                                                boxsize=L if periodic else None))
        npt.assert_array_equal(got[0], tp)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
def test_swapped_sets_give_the_same_moments(clustered, periodic, kind):
    got = gpu(*_args(clustered, "swapped"), **_kw(periodic, kind))
    assert_moments(got, clustered.ref("cross", periodic, kind))
    assert_moments(got, clustered.ref("swapped", periodic, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("f32", ["pos", "vel"])
def test_mixed_dtypes(clustered, f32, kind):
    c = clustered
    cast = (lambda p, v: (p.astype(np.float32), v)) if f32 == "pos" else (lambda p, v: (p, v.astype(np.float32)))
    (a, va), (b, vb) = cast(c.a, c.va), cast(c.b, c.vb)
    got = gpu(a, va, S50, b, vb, **_kw(True, kind))
    assert_moments(got, orc.moments(a, va, S50, b, vb, boxsize=L, kind=kind, pi_max=PI40, with_abs=True))
    # one set float32 / float64, the other float64 / float32
    got = gpu(a, va, S50, c.b.astype(va.dtype), c.vb.astype(a.dtype), **_kw(True, kind))
    assert_moments(got, orc.moments(a, va, S50, c.b.astype(va.dtype), c.vb.astype(a.dtype), boxsize=L, kind=kind,
                                    pi_max=PI40, with_abs=True))


@pytest.mark.parametrize("mode", ["cross", "auto"])
def test_device_tensor_inputs(clustered, mode):
    from astrild_amd import device as dev
    args = [x if x is S50 else dev.as_device(x) for x in _args(clustered, mode)]
    tensors = [x for x in args if x is not S50]
    before = [x.clone() for x in tensors]
    out = dev.pair_velocity_moments(*args, boxsize=L)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda and x.shape == (len(S50) - 1,) for x in out)
    assert [x.dtype for x in out] == [torch.int64, torch.float64, torch.float64]
    assert_moments(tuple(dev.to_numpy(x) for x in out), clustered.ref(mode, True, "radial"))
    for x, y in zip(tensors, before):
        assert torch.equal(x, y)                                   # the inputs are left alone


def test_repeated_calls(clustered):
    ref = clustered.ref("cross", True, "radial")
    runs = [gpu(*_args(clustered, "cross"), **_kw(True, "radial")) for _ in range(3)]
    for r in runs:
        assert_moments(r, ref)
        npt.assert_array_equal(r[0], runs[0][0])
        assert np.all(np.abs(r[1] - runs[0][1]) <= orc.sum_bound(ref[0], ref[3]))
        assert np.all(np.abs(r[2] - runs[0][2]) <= orc.sum_bound(ref[0], ref[2]))


# ---------------------------------------------------------------- a second, independent kernel
def test_open_auto_radial_equals_the_histogram_kernel_s_moments():
    """device.pairwise_velocity_pdf(kind="radial", moments=True) bins by int(float32(d / w)); this kernel by
    (k w)^2 < d^2 <= ((k + 1) w)^2.  The two agree for every pair that is not on an edge, which the oracle confirms of
    this catalogue first: then count, sum v and sum v^2 are sums of the same terms."""
    from astrild_amd import device as dev
    w, nb = 1.5, 8
    rng = np.random.default_rng(51)
    pos = rng.uniform(0.0, 60.0, (2000, 3))
    vel = rng.normal(0.0, 300.0, pos.shape)
    edges = w * np.arange(nb + 1)
    # every pair within a little more than the reach: its bin by both rules, and none at the reach itself
    from scipy.spatial import cKDTree
    ij = cKDTree(pos).query_pairs(w * nb * 1.001, output_type="ndarray")
    d = pos[ij[:, 1]] - pos[ij[:, 0]]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    dist = np.sqrt(d2)
    theirs = (dist / w).astype(np.float32).astype(np.int64)
    theirs_seen = (dist <= np.float32(w * nb)) & (theirs < nb)
    mine = np.searchsorted(edges ** 2, d2, side="left") - 1
    mine_seen = (d2 > 0) & (d2 <= edges[-1] ** 2)
    npt.assert_array_equal(theirs_seen, mine_seen)
    npt.assert_array_equal(theirs[mine_seen], mine[mine_seen])
    assert mine_seen.sum() > 50_000

    ref = orc.moments(pos, vel, edges, with_abs=True)
    got = gpu(pos, vel, edges)
    assert_moments(got, ref)
    _, _, (count, s1, s2) = dev.pairwise_velocity_pdf(pos, vel, w * nb, nb, 16, "radial", dist_width=w, vel_width=100.0,
                                                      moments=True)
    assert_moments(tuple(dev.to_numpy(x) for x in (count, s1, s2)), ref)
    npt.assert_array_equal(got[0], dev.to_numpy(count))


# ---------------------------------------------------------------- tiles, stages, the bin limit
@pytest.fixture(scope="module")
def crowded():
    """The crowded catalogue of tests/test_gpu_tpcf_cross.py (600 + 300 against 700 + 200 points, box 100): 600 + and
    700 + objects in the middle cell of the 3-cell grid, three i tiles against three j stages with ragged tails."""
    rng = np.random.default_rng(21)
    a = np.concatenate([rng.uniform(45.0, 55.0, (600, 3)), rng.uniform(0.0, 100.0, (300, 3))])
    b = np.concatenate([rng.uniform(45.0, 55.0, (700, 3)), rng.uniform(0.0, 100.0, (200, 3))])
    rng = np.random.default_rng(22)
    return a, rng.normal(0.0, 300.0, a.shape), b, rng.normal(0.0, 300.0, b.shape)


@pytest.mark.parametrize("cells", ["1", "0"])
@pytest.mark.parametrize("kind", KINDS)
def test_tiles_and_stages_in_a_crowded_cell(crowded, kind, cells, monkeypatch):
    monkeypatch.setenv("ASTRILD_PAIRVEL_CELLS", cells)
    a, va, b, vb = crowded
    kw = dict(boxsize=100.0, kind=kind, pi_max=20.0 if kind == "los" else None)
    got = gpu(a, va, CROWD_S, b, vb, **kw)
    if kind == "radial":
        assert got[0].tolist() == [1537, 31336, 198712, 194352, 55184]         # the TPCF's counts of this catalogue
    assert_moments(got, orc.moments_brute(a, va, CROWD_S, b, vb, boxsize=100.0, kind=kind, pi_max=20.0, with_abs=True))
    assert_moments(gpu(a, va, CROWD_S, **kw),
                   orc.moments_brute(a, va, CROWD_S, boxsize=100.0, kind=kind, pi_max=20.0, with_abs=True))
    kw["boxsize"] = None
    assert_moments(gpu(b, vb, CROWD_S, **kw),
                   orc.moments_brute(b, vb, CROWD_S, kind=kind, pi_max=20.0, with_abs=True))


def test_the_bin_limit(crowded):
    from astrild_amd import _lib, device as dev
    a, va, b, vb = crowded
    nb = dev._lib.lib().ast_pairvel_max_bins()
    assert nb == _lib.PAIRVEL_MAX_BINS
    edges = np.linspace(0.0, 33.0, nb + 1)
    got = gpu(a, va, edges, b, vb, boxsize=100.0)
    assert len(got[0]) == nb
    assert_moments(got, orc.moments_brute(a, va, edges, b, vb, boxsize=100.0, with_abs=True))
    with pytest.raises(ValueError):
        gpu(a, va, np.linspace(0.0, 33.0, nb + 2), b, vb, boxsize=100.0)


# ---------------------------------------------------------------- degenerate geometry, open boundaries
GEOMETRY = ["plane", "line", "all_coincident", "coincident", "corners", "edge_pairs"] + \
           [f"one_cell_{n}" for n in (2, 255, 256, 257, 513)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", GEOMETRY)
def test_degenerate_geometry(name, kind):
    pos, par, _ = pg.CATALOGUES[name]()
    vel = pg.velocities(pos, 300 + len(pos))
    edges = par["binwidth"] * np.arange(par["binnr"] + 1)
    reach = float(edges[-1])
    kw = dict(kind=kind, pi_max=reach if kind == "los" else None)
    got = gpu(pos, vel, edges, **kw)
    assert_moments(got, orc.moments_brute(pos, vel, edges, kind=kind, pi_max=reach, with_abs=True))
    if name == "all_coincident":
        assert got[0].sum() == 0 and not got[1].any() and not got[2].any()
    if name == "coincident" and kind == "radial":
        # the 44 850 pairs at d = 0 are in no bin: bin 0 holds the pairs of the scattered objects only
        d = pos[:, None, :] - pos[None, :, :]
        d2 = (d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2
        iu = np.triu_indices(len(pos), 1)
        assert (d2[iu] == 0).sum() == 44_850
        assert got[0][0] == ((d2[iu] > 0) & (d2[iu] <= edges[1] ** 2)).sum()
    if name == "edge_pairs" and kind == "radial":
        # integer coordinates: d^2 is an exact integer, and a pair exactly 7 k apart belongs to bin k - 1, (lo, hi]
        q = np.rint(pos).astype(np.int64)
        npt.assert_array_equal(q, pos)
        iu = np.triu_indices(len(q), 1)
        n2 = ((q[:, None, :] - q[None, :, :]) ** 2).sum(axis=-1)[iu]
        n2 = n2[(n2 > 0) & (n2 <= 49 * 49)]
        k = np.array([min(k for k in range(7) if v <= (7 * (k + 1)) ** 2) for v in n2.tolist()])
        on_edge = np.isin(n2, [(7 * k) ** 2 for k in range(1, 8)])
        assert on_edge.sum() >= 20
        npt.assert_array_equal(got[0], np.bincount(k, minlength=7))
        assert got[0].tolist() != pg.brute_pair_counts(pos, 7, 7.0).tolist()       # the [lo, hi) rule differs


# ---------------------------------------------------------------- empty inputs, refused inputs
def test_empty_inputs(clustered):
    from astrild_amd import device as dev
    none = np.zeros((0, 3))
    a, va = clustered.a[:100], clustered.va[:100]
    for kind in KINDS:
        kw = _kw(True, kind)
        for args in ((a, va, S50, none, none), (none, none, S50, a, va), (none, none, S50, none, none),
                     (a[:1], va[:1], S50), (none, none, S50)):
            count, s1, s2 = gpu(*args, **kw)
            assert count.shape == s1.shape == s2.shape == (39,)
            assert not count.any() and not s1.any() and not s2.any()
            mean, sigma = dev.finish_pair_velocity(count, s1, s2)
            assert np.isnan(mean).all() and np.isnan(sigma).all()
    # one object against one object
    count, s1, s2 = gpu(a[:1], va[:1], [0.0, 100.0], a[1:2], va[1:2], boxsize=L)
    assert_moments((count, s1, s2), orc.moments_brute(a[:1], va[:1], [0.0, 100.0], a[1:2], va[1:2], boxsize=L,
                                                       with_abs=True))


def test_positions_outside_the_box_are_refused(clustered):
    a, va = clustered.a[:100].copy(), clustered.va[:100]
    b, vb = clustered.b[:100].copy(), clustered.vb[:100]
    b[7, 1] = np.nextafter(L, np.inf)
    with pytest.raises(ValueError, match="sample 2"):
        gpu(a, va, S50, b, vb, boxsize=L)
    a[3, 2] = -1e-300
    with pytest.raises(ValueError, match="sample 1"):
        gpu(a, va, S50, boxsize=L)
    gpu(a, va, S50, b, vb)                                           # open boundaries: anything finite
    a[3, 2] = 0.0
    for bad in (np.nan, np.inf, -np.inf):
        b[7, 1] = bad
        with pytest.raises(ValueError, match="sample 2"):
            gpu(a, va, S50, b, vb)
        with pytest.raises(ValueError, match="sample 2"):
            gpu(a, va, S50, b, vb, boxsize=L)
    # the faces themselves belong to the box
    a[3, 2], b[7, 1] = 0.0, L
    gpu(a, va, S50, b, vb, boxsize=L)


# ---------------------------------------------------------------- dirty memory, call order
@pytest.mark.parametrize("mode,periodic,kind", [("cross", True, "radial"), ("cross", True, "los"),
                                                ("auto", False, "radial"), ("auto", True, "los")])
def test_dirty_scratch_and_outputs(clustered, dirty_alloc, mode, periodic, kind):
    mark = dirty_alloc.mark()
    got = gpu(*_args(clustered, mode), **_kw(periodic, kind))
    assert dirty_alloc.since(mark) >= 5                              # workspace, bounds and the three outputs
    assert_moments(got, clustered.ref(mode, periodic, kind))


def test_dirty_empty_sets(dirty_alloc):
    none = np.zeros((0, 3))
    one = np.ones((1, 3))
    for args in ((one, one, S50, none, none), (one, one, S50)):
        for x in gpu(*args, boxsize=L):
            assert not x.any()


def test_call_order(clustered, crowded):
    from astrild_amd import device as dev
    c = clustered
    a, va, b, vb = crowded
    tp = lambda: dev.to_numpy(dev.tpcf_cross_counts(c.a, c.b, S50, boxsize=L))
    pdf = lambda: [dev.to_numpy(x) for x in dev.pairwise_velocity_pdf(a, va, 12.0, 8, 16, "radial", dist_width=1.5,
                                                                      vel_width=100.0, moments=True)[2]]
    mine = lambda: gpu(*_args(c, "cross"), **_kw(True, "radial"))
    mine_los = lambda: gpu(a, va, CROWD_S, b, vb, boxsize=100.0, kind="los", pi_max=20.0)
    tp0, pdf0 = tp(), pdf()
    ref, ref_los = c.ref("cross", True, "radial"), orc.moments_brute(a, va, CROWD_S, b, vb, boxsize=100.0, kind="los",
                                                                     pi_max=20.0, with_abs=True)
    pdf_ref = orc.moments(a, va, 1.5 * np.arange(9), with_abs=True)
    for step in (mine, tp, mine_los, pdf, mine, pdf, mine_los, tp):
        out = step()
        if step is tp:
            npt.assert_array_equal(out, tp0)
        elif step is pdf:
            npt.assert_array_equal(out[0], pdf0[0])
            assert np.all(np.abs(out[1] - pdf0[1]) <= orc.sum_bound(pdf_ref[0], pdf_ref[3]))
            assert np.all(np.abs(out[2] - pdf0[2]) <= orc.sum_bound(pdf_ref[0], pdf_ref[2]))
        else:
            assert_moments(out, ref if step is mine else ref_los)


# ---------------------------------------------------------------- the public functions
def _mean_tol(ref):
    count, s1, s2, sa = ref
    with np.errstate(divide="ignore", invalid="ignore"):
        return orc.sum_bound(count, sa) / count + 4.0 * np.spacing(np.abs(s1 / count))


def _sigma_tol(ref):
    """First-order bound on sigma = sqrt(s2 / n - mean^2): d(var) <= bound(s2) / n + 2 |mean| d(mean) plus the few
    roundings of the expression itself, d(sigma) = d(var) / (2 sigma) plus the rounding of the square root."""
    count, s1, s2, sa = ref
    mean, sigma = orc.finish(count, s1, s2)
    with np.errstate(divide="ignore", invalid="ignore"):
        dvar = orc.sum_bound(count, s2) / count + 2.0 * np.abs(mean) * _mean_tol(ref) + 4.0 * np.spacing(s2 / count)
        return dvar / (2.0 * sigma) + 4.0 * np.spacing(sigma)


def _close(got, ref, tol):
    """NaN (an empty bin) where the reference has NaN, within tol elsewhere."""
    empty = np.isnan(ref)
    return np.array_equal(np.isnan(got), empty) and bool(np.all(np.abs(got[~empty] - ref[~empty]) <= tol[~empty]))


@pytest.mark.parametrize("two", [False, True], ids=["auto", "cross"])
@pytest.mark.parametrize("period", [L, None], ids=["periodic", "open"])
def test_hutils_functions(clustered, period, two):
    from astrild_amd.particles import hutils
    c = clustered
    a, va = c.a[:3000], c.va[:3000]
    b, vb = (c.b[:2000], c.vb[:2000]) if two else (None, None)
    for kind, mean_f, pvd_f, extra in (("radial", hutils.mean_radial_velocity_vs_r, hutils.radial_pvd_vs_r, ()),
                                       ("los", hutils.mean_los_velocity_vs_rp, hutils.los_pvd_vs_rp, (PI40,))):
        ref = orc.moments(a, va, S50, b, vb, boxsize=period, kind=kind, pi_max=PI40, los=2 if kind == "radial" else 1,
                          with_abs=True)
        kw = dict(sample2=b, velocities2=vb, period=period)
        if kind == "los":
            kw["los"] = 1
        mean, mom = mean_f(a, va, S50, *extra, return_moments=True, **kw)
        assert sorted(mom) == ["count", "sum_v", "sum_v2"]
        assert_moments((mom["count"], mom["sum_v"], mom["sum_v2"]), ref)
        emean, esigma = orc.finish(*ref[:3])
        npt.assert_array_equal(mean, orc.finish(mom["count"], mom["sum_v"], mom["sum_v2"])[0])
        assert mean.shape == (len(S50) - 1,) and _close(mean, emean, _mean_tol(ref))
        mean2 = mean_f(a, va, S50, *extra, **kw)
        assert isinstance(mean2, np.ndarray) and _close(mean2, emean, _mean_tol(ref))
        sigma, mom = pvd_f(a, va, S50, *extra, return_moments=True, **kw)
        npt.assert_array_equal(sigma, orc.finish(mom["count"], mom["sum_v"], mom["sum_v2"])[1])
        assert np.nanmedian(sigma) > 100.0                          # two draws of N(0, 300): far from the clamp at 0
        assert sigma.shape == (len(S50) - 1,) and _close(sigma, esigma, _sigma_tol(ref))


@pytest.mark.parametrize("seperate", [None, {"Group_M_Crit200": 14, "compare": [1, 2]}], ids=["all", "split"])
def test_subfind_mean_pairwise_velocity(seperate):
    from astrild_amd.particles.hutils import SubFind
    n, hubble, box_kpc = 3000, 0.6774, 60_000.0
    rng = np.random.default_rng(61)
    cat = {"GroupPos": rng.uniform(0.0, 0.999 * box_kpc / hubble, (n, 3)).astype(np.float32),
           "GroupVel": rng.normal(0.0, 300.0, (n, 3)).astype(np.float32),
           "Group_M_Crit200": 10.0 ** rng.uniform(12.0, 15.0, n)}
    snap = types.SimpleNamespace(cat=cat, header=types.SimpleNamespace(boxsize=box_kpc, hubble=hubble))
    r_c, v12 = SubFind.mean_pairwise_velocity(snap, seperate=seperate)
    # boxsize 60, limits (0.3, 12), nbins = 8 edges
    edges = np.geomspace(0.3, 12.0, 8)
    npt.assert_array_equal(r_c, 0.5 * (edges[1:] + edges[:-1]))
    m = cat["Group_M_Crit200"]
    i1, i2 = (np.ones(n, bool), np.ones(n, bool)) if seperate is None else (m < 1e14, m > 1e14)
    pos1, pos2 = (cat["GroupPos"][i, :] * hubble / 1e3 for i in (i1, i2))
    ref = orc.moments(pos1, cat["GroupVel"][i1], edges, pos2, cat["GroupVel"][i2], boxsize=60.0, with_abs=True)
    assert ref[0][-1] > 100
    emean = orc.finish(*ref[:3])[0]
    assert v12.shape == (7,) and _close(v12, emean, _mean_tol(ref))
