"""GPU: the jackknife pair counts of the two-point correlation function (ast_tpcf_jk_prepare / ast_tpcf_jk_counts
through device.tpcf_jackknife_counts) and tpcf_jackknife on top of them: a lattice with known answers; counts and
endpoint table exactly equal to the brute-force WEIGHTED oracle (tests/tpcf_jackknife_oracle.py: ends must equal
2 counts - 2 W_k) for auto and cross pairs, periodic and open, explicit and computed tags; a crowded cell with several
tiles and stages under every flush / LDS / global combination and a table just over the LDS limit; empty and
one-object samples, empty and all-holding regions, the redshift-space shift across region and box faces; the refusal of
an out-of-range tag; dirty scratch memory and call order; tpcf_jackknife end to end."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import tpcf_jackknife_oracle as jorc
from tests import tpcf_oracle as orc
from tests.dirty_memory import dirty_alloc                        # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LAT_S = [0.5, 1.2, 1.6, 1.9, 2.1, 2.5]
MU4 = [0.0, 0.25, 0.6, 0.8, 1.0]
L = 100.0
S30 = np.linspace(0.0, 30.0, 11)
CROWD_S = [0, 1, 3, 7, 15, 33]
NSUB = (3, 2, 2)


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


def gpu_jk(pos1, nsub, s_edges, mu_edges=None, **kw):
    from astrild_amd import device as dev
    counts, ends = dev.tpcf_jackknife_counts(pos1, nsub, s_edges, mu_edges, **kw)
    assert counts.dtype == ends.dtype == torch.int64 and ends.shape[1:] == counts.shape
    return dev.to_numpy(counts), dev.to_numpy(ends)


def gpu_cross(a, b, s_edges, mu_edges=None, **kw):
    from astrild_amd import device as dev
    return dev.to_numpy(dev.tpcf_cross_counts(a, b, s_edges, mu_edges=mu_edges, **kw))


def oracle(a, ta, b, tb, ntot, s_edges, mu_edges=None, los=2, boxsize=None):
    """(counts, ends) as the kernel must return them, from the WEIGHTED counts: ends[k] = 2 counts - 2 W_k; and the
    oracle's own count of pair ends agrees."""
    counts, w2, ends = jorc.jackknife_counts_brute(a, ta, b, tb, ntot, s_edges, mu_edges, los, boxsize)
    want = 2 * counts[None] - w2
    npt.assert_array_equal(ends, want)
    return counts, want


def bounding_box(*sets):
    sets = [np.asarray(p, dtype=np.float64) for p in sets if p is not None and len(p)]
    return np.min([p.min(0) for p in sets], axis=0), np.max([p.max(0) for p in sets], axis=0)


def check(got, want):
    npt.assert_array_equal(got[0], want[0])
    npt.assert_array_equal(got[1], want[1])
    npt.assert_array_equal(got[1].sum(axis=0), 2 * got[0])


# ---------------------------------------------------------------- known answers and the oracle
@pytest.mark.parametrize("cells", ["1", "0"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lattice(dtype, cells, monkeypatch, hip):
    from astrild_amd import _lib
    assert hip.ast_tpcf_jk_max_table() == _lib.TPCF_JK_MAX_TABLE
    monkeypatch.setenv("ASTRILD_TPCF_CELLS", cells)
    counts, ends = gpu_jk(orc.lattice(8).astype(dtype), 2, LAT_S, boxsize=8.0)
    assert counts.tolist() == [1536, 3072, 2048, 1536, 12288]
    assert ends.shape == (8, 5) and all(row == [384, 768, 512, 384, 3072] for row in ends.tolist())
    counts, ends = gpu_jk(orc.lattice(8).astype(dtype), (2, 2, 2), LAT_S, MU4, boxsize=8.0)
    npt.assert_array_equal(counts, orc.lattice_expected(8, LAT_S, MU4, 2, 2.5))
    npt.assert_array_equal(ends, np.broadcast_to(counts // 4, (8, 5, 4)))


@pytest.fixture(scope="module")
def catalogues():
    rng = np.random.default_rng(7)
    a = orc.clustered(1300, L, 11, blobs=20, sigma=6.0)
    b = orc.clustered(1500, L, 12, blobs=20, sigma=6.0)
    return a, b, rng.integers(0, 7, len(a)).astype(np.int32), rng.integers(0, 7, len(b)).astype(np.int64)


@pytest.mark.parametrize("mode", ["periodic", "open"])
@pytest.mark.parametrize("pairs", ["auto", "cross"])
def test_catalogues_equal_the_oracle(catalogues, pairs, mode):
    a, b, ta, tb = catalogues
    box = L if mode == "periodic" else None
    b, tb = (None, None) if pairs == "auto" else (b, tb)
    # computed tags: [0, L] when periodic, the joint bounding box when open
    lo, hi = (np.zeros(3), np.full(3, L)) if box else bounding_box(a, b)
    ra, rb = jorc.region_tags(a, NSUB, lo, hi), None if b is None else jorc.region_tags(b, NSUB, lo, hi)
    want = oracle(a, ra, b, rb, 12, S30, MU4, boxsize=box)
    got = gpu_jk(a, NSUB, S30, MU4, pos2=b, boxsize=box)
    assert got[0].shape == (10, 4) and got[1].shape == (12, 10, 4) and got[0].sum() > 10_000
    check(got, want)
    npt.assert_array_equal(got[0], gpu_cross(a, b, S30, MU4, boxsize=box))
    # the same regions given as tags, a device tensor among them
    check(gpu_jk(a, 12, S30, MU4, pos2=b, boxsize=box, tags1=torch.from_numpy(ra).cuda(), tags2=rb), want)
    # an extent of the caller's, non-cubic, with objects outside it; real space
    lo, hi = np.array([10.0, -5.0, 20.0]), np.array([90.0, 70.0, 120.0])
    ra, rb = jorc.region_tags(a, (2, 1, 3), lo, hi), None if b is None else jorc.region_tags(b, (2, 1, 3), lo, hi)
    check(gpu_jk(a, (2, 1, 3), S30, pos2=b, boxsize=box, extent=(lo, hi)), oracle(a, ra, b, rb, 6, S30, boxsize=box))
    # regions of the caller's that follow no geometry
    got = gpu_jk(a, 7, S30, MU4, pos2=b, boxsize=box, tags1=ta, tags2=tb, los=0)
    check(got, oracle(a, ta, b, tb, 7, S30, MU4, los=0, boxsize=box))
    npt.assert_array_equal(got[0], gpu_cross(a, b, S30, MU4, boxsize=box, los=0))


def test_float32_positions_and_regions_on_faces():
    rng = np.random.default_rng(8)
    a = (rng.integers(0, 65, (1200, 3)) * (L / 64.0)).astype(np.float32)     # on the faces of 4 x 8 x 2 regions, and at L
    b = rng.uniform(0.0, L, (900, 3))
    ra, rb = jorc.region_tags(a, (4, 8, 2), [0.0] * 3, [L] * 3), jorc.region_tags(b, (4, 8, 2), [0.0] * 3, [L] * 3)
    assert np.any(a == L) and len(np.unique(ra)) == 64
    # 64 x 10 x 4 counters: two LDS copies shared by the four waves (640 below: a copy per wave; one copy: the crowded cell)
    check(gpu_jk(a, (4, 8, 2), S30, MU4, pos2=b, boxsize=L), oracle(a, ra, b, rb, 64, S30, MU4, boxsize=L))
    check(gpu_jk(a, (4, 8, 2), S30, boxsize=L), oracle(a, ra, None, None, 64, S30, boxsize=L))


# ---------------------------------------------------------------- tiles, stages, flushes, LDS and global memory
@pytest.fixture(scope="module")
def crowded(hip):
    """600 + and 700 + objects in the middle cell of the 3-cell grid (three i tiles against three j stages, the last of
    each partly filled), spread over all 2 x 2 x 2 regions; the oracle's integers per case, among them two (s, mu)
    tables of 8 x 5 x nmu counters: the largest that fits the LDS limit and the first that does not."""
    rng = np.random.default_rng(21)
    a = np.concatenate([rng.uniform(45.0, 55.0, (600, 3)), rng.uniform(0.0, 100.0, (300, 3))])
    b = np.concatenate([rng.uniform(45.0, 55.0, (700, 3)), rng.uniform(0.0, 100.0, (200, 3))])
    nmu = 1
    while 40 * nmu <= hip.ast_tpcf_jk_lds_table(5, nmu):
        nmu += 1
    assert 900 < nmu < 1000 and 40 * (nmu - 1) <= hip.ast_tpcf_jk_lds_table(5, nmu - 1)
    fit, over = np.linspace(0.0, 1.0, nmu), np.linspace(0.0, 1.0, nmu + 1)
    ta, tb = jorc.region_tags(a, (2, 2, 2), [0.0] * 3, [L] * 3), jorc.region_tags(b, (2, 2, 2), [0.0] * 3, [L] * 3)
    lo, hi = bounding_box(a, b)
    oa, ob = jorc.region_tags(a, (2, 2, 2), lo, hi), jorc.region_tags(b, (2, 2, 2), lo, hi)
    want = {"cross": oracle(a, ta, b, tb, 8, CROWD_S, boxsize=L), "auto": oracle(b, tb, None, None, 8, CROWD_S, MU4, boxsize=L),
            "open": oracle(a, oa, b, ob, 8, CROWD_S), "fit": oracle(a, ta, b, tb, 8, CROWD_S, fit, boxsize=L),
            "over": oracle(a, ta, b, tb, 8, CROWD_S, over, boxsize=L)}
    assert want["cross"][0].tolist() == [1537, 31336, 198712, 194352, 55184]
    return a, b, fit, over, want


@pytest.mark.parametrize("lds", ["1", "0"])
@pytest.mark.parametrize("flush", [None, "1000"])
@pytest.mark.parametrize("cells", ["1", "0"])
def test_tiles_and_stages_in_a_crowded_cell(crowded, cells, flush, lds, monkeypatch):
    from astrild_amd import device as dev
    monkeypatch.setenv("ASTRILD_TPCF_CELLS", cells)
    monkeypatch.setenv("ASTRILD_TPCF_JK_LDS", lds)
    if flush is not None:
        monkeypatch.setenv("AST_TPCF_FLUSH_AT", flush)
    a, b, fit, over, want = crowded
    dev.profile_enable(True)
    try:
        check(gpu_jk(a, 2, CROWD_S, pos2=b, boxsize=L), want["cross"])
        check(gpu_jk(b, 2, CROWD_S, MU4, boxsize=L), want["auto"])
        check(gpu_jk(a, 2, CROWD_S, pos2=b), want["open"])
        check(gpu_jk(a, 2, CROWD_S, fit, pos2=b, boxsize=L), want["fit"])
        before = dict(dev.profile_report())
        check(gpu_jk(a, 2, CROWD_S, over, pos2=b, boxsize=L), want["over"])
        after = dev.profile_report()
    finally:
        dev.profile_enable(False)
    calls = lambda rep, name: rep.get(name, (0, 0.0))[0]
    # the table just over the limit takes global memory whatever the switch says; the others follow the switch
    assert calls(after, "tpcf_jk_pairs_global") == calls(before, "tpcf_jk_pairs_global") + 1
    assert calls(after, "tpcf_jk_pairs_lds") == calls(before, "tpcf_jk_pairs_lds")
    assert (calls(before, "tpcf_jk_pairs_lds") > 0) == (lds == "1")


# ---------------------------------------------------------------- edge inputs
@pytest.mark.parametrize("box", [None, L])
@pytest.mark.parametrize("n1,n2", [(0, 0), (0, 1), (1, 0), (1, 1), (0, 300), (300, 0), (1, 300), (300, 1)])
def test_empty_and_single_object_sets(n1, n2, box):
    a = orc.uniform(300, L, 35)[:n1]
    b = (orc.uniform(300, L, 36) if n2 > 1 else np.array([[50.0, 44.0, 42.0]]))[:n2]
    if n1 == 1:
        a = np.array([[50.0, 50.0, 50.0]])
    lo, hi = (np.zeros(3), np.full(3, L)) if box or not (n1 or n2) else bounding_box(a, b)
    ta, tb = jorc.region_tags(a, NSUB, lo, hi), jorc.region_tags(b, NSUB, lo, hi)
    got = gpu_jk(a, NSUB, S30, MU4, pos2=b, boxsize=box, vel1=np.zeros_like(a))
    assert got[1].shape == (12, 10, 4)
    check(got, oracle(a, ta, b, tb, 12, S30, MU4, boxsize=box))
    if (n1, n2) == (1, 1):
        assert got[0].sum() == 1 and got[1].sum() == 2                # d = 10, mu = 0.8
    if not (n1 and n2):
        assert not got[0].any() and not got[1].any()
    auto = gpu_jk(a, 3, S30, boxsize=box, tags1=np.full(n1, 2))
    assert auto[1].shape == (3, 10)
    if n1 < 2:
        assert not auto[0].any() and not auto[1].any()
    else:
        assert auto[0].sum() > 0 and not auto[1][:2].any()            # all objects in region 2
        npt.assert_array_equal(auto[1][2], 2 * auto[0])
    torch.cuda.synchronize()


def test_empty_regions_and_one_region_holding_everything():
    a, b = orc.uniform(1000, 40.0, 37) + 5.0, orc.uniform(1100, 40.0, 38) + 5.0     # inside [5, 45] of a box of 100
    ta, tb = jorc.region_tags(a, (4, 4, 4), [0.0] * 3, [L] * 3), jorc.region_tags(b, (4, 4, 4), [0.0] * 3, [L] * 3)
    assert len(np.unique(ta)) == 8
    got = gpu_jk(a, 4, S30[:6], pos2=b, boxsize=L)
    check(got, oracle(a, ta, b, tb, 64, S30[:6], boxsize=L))
    empty = np.setdiff1d(np.arange(64), np.union1d(ta, tb))
    assert len(empty) == 56 and not got[1][empty].any()
    # one region of one: E == 2 counts and nothing is left over
    for nsub in (1, (1, 1, 1)):
        counts, ends = gpu_jk(a, nsub, S30[:6], MU4, pos2=b, boxsize=L)
        npt.assert_array_equal(ends, 2 * counts[None])
        npt.assert_array_equal(counts, gpu_cross(a, b, S30[:6], MU4, boxsize=L))
    # everything in the far corner region of an extent that misses the objects
    counts, ends = gpu_jk(a, (2, 3, 2), S30[:6], extent=([-50.0] * 3, [0.0] * 3))
    npt.assert_array_equal(ends[11], 2 * counts)
    assert counts.sum() > 1000 and not ends[:11].any()


@pytest.mark.parametrize("pdt,vdt", [(np.float32, np.float64), (np.float64, np.float32)])
def test_tags_follow_the_redshift_space_shift(pdt, vdt):
    rng = np.random.default_rng(41)
    a, b = orc.uniform(1500, L, 42).astype(pdt), orc.uniform(1400, L, 43).astype(vdt)
    va = rng.normal(0.0, 1500.0, a.shape).astype(vdt)                 # shifts of ~15: across region faces and the box faces
    vb = rng.normal(0.0, 1500.0, b.shape).astype(pdt)
    for los in (0, 2):
        sa, sb = orc.shift_and_wrap(a, va, L, los), orc.shift_and_wrap(b, vb, L, los)
        ta, tb = jorc.region_tags(sa, NSUB, [0.0] * 3, [L] * 3), jorc.region_tags(sb, NSUB, [0.0] * 3, [L] * 3)
        raw = a[:, los].astype(np.float64) + va[:, los] / 100.0
        assert np.sum((raw > L) | (raw < 0)) > 50                     # wrapped across the box face
        assert np.sum(ta != jorc.region_tags(a, NSUB, [0.0] * 3, [L] * 3)) > 200        # and across region faces
        check(gpu_jk(a, NSUB, S30, MU4, pos2=b, boxsize=L, vel1=va, vel2=vb, los=los),
              oracle(sa, ta, sb, tb, 12, S30, MU4, los=los, boxsize=L))
        # open: the shift without the wrap; the default extent is the box of the GIVEN positions, so shifted outliers
        # belong to the border regions
        oa = orc.shift_and_wrap(a, va, 0.0, los)
        lo, hi = bounding_box(a)
        assert oa[:, los].max() > hi[los] and oa[:, los].min() < lo[los]
        check(gpu_jk(a, NSUB, S30, vel1=va, los=los), oracle(oa, jorc.region_tags(oa, NSUB, lo, hi), None, None, 12, S30))


# ---------------------------------------------------------------- refusals
def test_an_out_of_range_tag_is_refused_before_any_pair_work(catalogues, monkeypatch):
    from astrild_amd import _lib
    from astrild_amd import device as dev
    a, b, ta, tb = catalogues
    lib = _lib.lib()
    calls = []

    class Spy:
        """The library, with the pair-count entry recorded."""
        def __getattr__(self, name):
            if name == "ast_tpcf_jk_counts":
                calls.append(name)
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    for row, value, second in ((17, 7, False), (0, -1, False), (len(b) - 1, 7, True), (3, np.iinfo(np.int32).min, True),
                               (5, np.iinfo(np.int32).max, False)):
        t1, t2 = ta.copy(), tb.copy()
        (t2 if second else t1)[row] = value
        with pytest.raises(ValueError, match=r"tags must lie in \[0, 7\)"):
            dev.tpcf_jackknife_counts(a, 7, S30, pos2=b, boxsize=L, tags1=t1, tags2=t2)
    with pytest.raises(ValueError, match="must lie in"):
        dev.tpcf_jackknife_counts(a + 1.0, NSUB, S30, boxsize=L)
    with pytest.raises(ValueError, match="must be finite"):
        dev.tpcf_jackknife_counts(np.where(np.arange(len(a))[:, None] == 4, np.nan, a), NSUB, S30)
    with pytest.raises(ValueError, match="nsub"):
        dev.tpcf_jackknife_counts(a, [2, 2], S30, boxsize=L)
    with pytest.raises(ValueError, match="counters"):
        dev.tpcf_jackknife_counts(a, 1000, np.linspace(0.0, 30.0, 101), np.linspace(0.0, 1.0, 101), boxsize=L)
    assert calls == []
    monkeypatch.undo()
    check(gpu_jk(a, 7, S30, pos2=b, boxsize=L, tags1=ta, tags2=tb), oracle(a, ta, b, tb, 7, S30, boxsize=L))


# ---------------------------------------------------------------- scratch memory and call order
def test_dirty_scratch_and_call_order(catalogues, dirty_alloc):
    a, b, ta, tb = catalogues
    first = lambda: gpu_jk(a, 7, S30, pos2=b, boxsize=L, tags1=ta, tags2=tb)
    second = lambda: gpu_jk(b[:700], (2, 2, 3), CROWD_S, MU4)
    mark = dirty_alloc.mark()
    x1 = first()
    assert dirty_alloc.since(mark) >= 4                               # workspace, bounds, counts, ends
    x2 = second()
    y2, y1 = second(), first()
    for x, y in ((x1, y1), (x2, y2)):
        npt.assert_array_equal(x[0], y[0])
        npt.assert_array_equal(x[1], y[1])
    check(x1, oracle(a, ta, b, tb, 7, S30, boxsize=L))
    lo, hi = bounding_box(b[:700])
    check(x2, oracle(b[:700], jorc.region_tags(b[:700], (2, 2, 3), lo, hi), None, None, 12, CROWD_S, MU4))
    none = np.zeros((0, 3))
    for box in (None, L):                                             # the early returns write both outputs
        for got in (gpu_jk(a[:300], 2, S30, MU4, pos2=none, boxsize=box), gpu_jk(none, 2, S30, pos2=a[:300], boxsize=box),
                    gpu_jk(a[:1], 2, S30, MU4, boxsize=box)):
            assert got[1].shape[0] == 8 and not got[0].any() and not got[1].any()


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("period", [L, None], ids=["periodic", "open"])
def test_tpcf_jackknife_end_to_end(period):
    """Same host code, same integers: tpcf_jackknife equals jackknife_from_counts fed the oracle's counts, bit for bit."""
    from astrild_amd.particles.hutils import tpcf_jackknife
    from astrild_amd.particles.hutils.tpcf import jackknife_from_counts
    edges = [0, 2, 5, 10, 18, 30]
    pos = {"1": orc.clustered(400, L, 5, blobs=12, sigma=6), "R": orc.uniform(1200, L, 6),
           "2": orc.clustered(300, L, 9, blobs=12, sigma=6).astype(np.float32)}
    lo, hi = (np.zeros(3), np.full(3, L)) if period else bounding_box(*pos.values())
    tags = {k: jorc.region_tags(p, NSUB, lo, hi) for k, p in pos.items()}
    occ = {k: np.bincount(t, minlength=12) for k, t in tags.items()}
    terms = {"D1D1": ("1", None), "D1D2": ("1", "2"), "D2D2": ("2", None), "D1R": ("1", "R"), "D2R": ("2", "R"),
             "RR": ("R", None)}
    c = {}
    for term, (p, q) in terms.items():
        c[term] = oracle(pos[p], tags[p], None if q is None else pos[q], None if q is None else tags[q], 12, edges,
                         boxsize=period)
    out = tpcf_jackknife(pos["1"], pos["R"], edges, Nsub=list(NSUB), sample2=pos["2"], period=period,
                         estimator="Landy-Szalay", return_counts=True)
    assert len(out) == 7 and sorted(out[6]) == sorted(terms)
    for term in terms:
        check(out[6][term], c[term])
    ref = jackknife_from_counts(c, 400, occ["1"], 1200, occ["R"], 300, occ["2"], "Landy-Szalay")
    for got, want in zip(out[:6], ref):
        npt.assert_array_equal(got, want)
        assert np.isfinite(got).all()
    assert all(x.shape == (5,) for x in out[:3]) and all(x.shape == (5, 5) and np.all(np.diag(x) > 0) for x in out[3:6])
    # one sample on a device tensor, the default 5 x 5 x 5 regions
    xi, cov = tpcf_jackknife(torch.from_numpy(pos["1"]).cuda(), pos["R"], edges, period=period)
    t1 = jorc.region_tags(pos["1"], (5, 5, 5), *((np.zeros(3), np.full(3, L)) if period else bounding_box(pos["1"], pos["R"])))
    tr = jorc.region_tags(pos["R"], (5, 5, 5), *((np.zeros(3), np.full(3, L)) if period else bounding_box(pos["1"], pos["R"])))
    c5 = {"D1D1": oracle(pos["1"], t1, None, None, 125, edges, boxsize=period),
          "RR": oracle(pos["R"], tr, None, None, 125, edges, boxsize=period)}
    ref = jackknife_from_counts(c5, 400, np.bincount(t1, minlength=125), 1200, np.bincount(tr, minlength=125))
    npt.assert_array_equal(xi, ref[0])
    npt.assert_array_equal(cov, ref[1])
