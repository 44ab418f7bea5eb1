"""GPU: every path of the paint held to the per-cell bounds of tests/paint_accuracy.py - over a wide mass range, masses
of both signs, zero masses, a cell-volume scale and a crowded tile next to light cells - plus the exact power-of-two,
sign and permutation relations of the fixed-point column walk, and the refusal of NaN / Inf masses.

64^3 grid, box 250, 2^17 particles, scale = 1 / dx^3.  Coordinates and masses are float32 values, so one reference per
input and window serves both dtypes (the wide mass range is chosen per dtype: its own input).  Each case prints
``ACC | case | window | dtype | bound | largest error / bound | largest error / A`` - the tables of DESIGN.md.
(The grid has two z tiles per column: AST_PAINT_ZSEG=4 asks for more segments than there are tiles and runs as 2; 1 is
the unsegmented walk, which this grid does not take by default.)"""
import numpy as np
import pytest

from tests import paint_accuracy as pa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, L, NP, SCALE = pa.N, pa.L, pa.NP, pa.SCALE
NPT = {"f32": np.float32, "f64": np.float64}
TT = {"f32": torch.float32, "f64": torch.float64}
SP, SC, TP = "single-pass", "scattered", "two-pass"
SLAB = dict(x_start=15, nx_alloc=18)            # planes 15 .. 32: one ghost plane each side of 16 .. 31, 18 % 8 = 2
WINDOWS = pytest.mark.parametrize("window", ["cic", "tsc"])
DTYPES = pytest.mark.parametrize("dtype", ["f32", "f64"])


@pytest.fixture(scope="module")
def dev(hip):
    from astrild_amd import device
    torch.cuda.set_device(0)
    return device


def _slab_subset(pos):
    s = (pos[:, 0] * (N / L)) % N
    return (s >= 16.5) & (s < 31.5)


@pytest.fixture(scope="module")
def refs():
    """(positions, masses, Reference) per (input, window, slab), made once and never changed."""
    cache = {}

    def get(name, window, slab=False):
        key = (name, window, slab)
        if key not in cache:
            pos, mass = pa.make_input(name)
            kw = {}
            if slab:
                sel = _slab_subset(pos)
                pos, mass = pos[sel], mass[sel]
                order = pa.sort_by_tile(pos, N, L, SLAB["x_start"])
                pos, mass, kw = pos[order], mass[order], SLAB
            cache[key] = (pos, mass, pa.Reference(pos, mass, N, L, window, scale=SCALE, **kw))
        return cache[key]
    return get


def _dev_arrays(dev, pos, mass, dtype):
    return dev.as_device(pos.astype(NPT[dtype])), dev.as_device(mass.astype(NPT[dtype]))


def _report(case, window, dtype, kind, got, ref, bound, offset=0.0, add=None):
    ratio, rel, over = pa.measure(got, ref, bound, offset, add)
    print(f"\nACC | {case} | {window} | {dtype} | {kind} | {ratio:.3g} | {rel:.3g}")
    return ratio, over


def _check(case, window, dtype, grid, ref, lists, walk, offset=0.0, add=None, base=None):
    """The any-path bound everywhere, the column-walk bound where it applies (``walk``), and the total mass within the
    sum of the per-cell bounds."""
    T = NPT[dtype]
    got = grid.cpu().numpy()
    assert np.isfinite(got).all()
    bound = ref.any_bound(T, lists, offset, base)
    ratio, over = _report(case, window, dtype, "any path", got, ref, bound, offset, add)
    assert over == 0, (case, window, dtype, "any-path bound", ratio)
    if walk:
        bound = ref.walk_bound(T, lists, offset)
        ratio, over = _report(case, window, dtype, "column walk", got, ref, bound, offset, add)
        assert over == 0, (case, window, dtype, "column-walk bound", ratio)
    assert pa.total_mass_error(got, ref, offset, add) <= float(bound.sum())


def _paint(dev, pos, mass, window, method, want=None, **kw):
    """One paint with its statistics; ``want``: (path, attempts, overflow is zero?)."""
    st = {}
    grid = dev.paint(pos, mass, N, L, window, scale=SCALE, method=method, stats=st, **kw)
    if want is not None:
        path, attempts, clean = want
        assert (st["path"], st["attempts"]) == (path, attempts), st
        if path != TP:
            assert (st["overflow"] == 0) == clean, st
    return grid


ORDERED = dict(method="tiled", accumulate=False, hint="ordered", want=(SP, 1, True))
SCATTERED = dict(method="tiled", accumulate=False, hint="scattered", want=(SC, 1, True))
TWO_PASS = dict(method="tiled2", accumulate=False, want=(TP, 1, True))
WALKS = {"ordered": (ORDERED, "single"), "scattered": (SCATTERED, "single"), "tiled2": (TWO_PASS, "two-pass")}


# ------------------------------------------------------------------ wide mass range: every path
@WINDOWS
@DTYPES
def test_wide_masses_direct(dev, refs, window, dtype):
    pos, mass, ref = refs("wide-" + dtype, window)
    p, m = _dev_arrays(dev, pos, mass, dtype)
    st = {}
    grid = dev.paint(p, m, N, L, window, scale=SCALE, method="direct", stats=st)
    assert st == {}                                            # (no tiled paint ran)
    _check("wide direct", window, dtype, grid, ref, None, False)


@WINDOWS
@DTYPES
@pytest.mark.parametrize("path", list(WALKS))
def test_wide_masses_column_walk(dev, refs, window, dtype, path):
    """The three list formats of the overwrite paint on input they hold completely: pure column walks.  The scattered
    path gets the particles in a random order - and must give the ordered paint's grid bit for bit."""
    pos, mass, ref = refs("wide-" + dtype, window)
    kw, lists = WALKS[path]
    if path == "scattered":
        perm = np.random.default_rng(7).permutation(NP)
        pos, mass = pos[perm], mass[perm]
    p, m = _dev_arrays(dev, pos, mass, dtype)
    grid = _paint(dev, p, m, window, **kw)
    _check("wide " + path, window, dtype, grid, ref, lists, True)
    if path == "scattered":
        p, m = _dev_arrays(dev, *refs("wide-" + dtype, window)[:2], dtype)
        assert torch.equal(grid, _paint(dev, p, m, window, **ORDERED))


@WINDOWS
@DTYPES
@pytest.mark.parametrize("method", ["direct", "tiled"])
def test_wide_masses_accumulated_into_a_prefilled_grid(dev, refs, window, dtype, method):
    pos, mass, ref = refs("wide-" + dtype, window)
    p, m = _dev_arrays(dev, pos, mass, dtype)
    top = float(np.abs(ref.S).max())
    pre = (np.random.default_rng(11).uniform(-1.0, 1.0, size=(N, N, N)) * top).astype(NPT[dtype])
    out = dev.as_device(pre.copy())
    st = {}
    grid = dev.paint(p, m, N, L, window, scale=SCALE, method=method, out=out, stats=st)
    assert grid is out
    if method == "tiled":
        assert (st["path"], st["attempts"]) == (SP, 1) and "overflow" not in st, st        # accumulating: no list statistics
    _check(f"wide accumulate {method}", window, dtype, grid, ref, None, False, add=pre, base=float(np.abs(pre).max()))


@WINDOWS
@DTYPES
def test_wide_masses_z_segmented_walk(dev, refs, window, dtype, monkeypatch):
    pos, mass, ref = refs("wide-" + dtype, window)
    p, m = _dev_arrays(dev, pos, mass, dtype)
    plain = _paint(dev, p, m, window, **ORDERED)
    for nseg in (1, 2, 4):
        monkeypatch.setenv("AST_PAINT_ZSEG", str(nseg))
        grid = _paint(dev, p, m, window, **ORDERED)
        monkeypatch.delenv("AST_PAINT_ZSEG")
        _check(f"wide zseg {nseg}", window, dtype, grid, ref, "single", True)
        assert torch.equal(grid, plain)


@WINDOWS
@DTYPES
def test_wide_masses_slab_buffer_with_ghost_planes_and_a_partial_tile(dev, refs, window, dtype):
    pos, mass, ref = refs("wide-" + dtype, window, slab=True)
    assert 20000 < len(pos) < 40000
    p, m = _dev_arrays(dev, pos, mass, dtype)
    grid = _paint(dev, p, m, window, **ORDERED, **SLAB)
    assert tuple(grid.shape) == (SLAB["nx_alloc"], N, N)
    _check("wide slab", window, dtype, grid, ref, "single", True)
    two = _paint(dev, p, m, window, **TWO_PASS, **SLAB)
    _check("wide slab tiled2", window, dtype, two, ref, "two-pass", True)


@WINDOWS
@DTYPES
@pytest.mark.parametrize("name", ["wide", "some-zero"])
def test_offset_mean_keeps_the_bound(dev, refs, window, dtype, name):
    """offset="mean": the mean the paint subtracts is fetched the same way (device.total_mass), so that the bound is about
    the paint and not about that sum."""
    name = name + "-" + dtype if name == "wide" else name
    pos, mass, ref = refs(name, window)
    p, m = _dev_arrays(dev, pos, mass, dtype)
    mean = dev.total_mass(m, NP) * SCALE / float(N) ** 3
    assert mean > 0
    for path, (kw, lists) in WALKS.items():
        if path == "scattered":
            continue                                   # (tile order: the scattered path would fill its buckets unevenly)
        grid = _paint(dev, p, m, window, offset="mean", **kw)
        _check(f"{name} offset {path}", window, dtype, grid, ref, lists, True, offset=mean)
        assert torch.equal(grid, _paint(dev, p, m, window, offset=mean, **kw))


@WINDOWS
@DTYPES
def test_wide_masses_staged_paint_row_by_row(dev, refs, window, dtype):
    pos, mass, ref = refs("wide-" + dtype, window)
    p, m = _dev_arrays(dev, pos, mass, dtype)
    out = torch.full((N, N, N), float("nan"), dtype=TT[dtype], device="cuda")
    sp = dev.StagedPaint(p, m, N, L, window, out, scale=SCALE)
    sp.group()
    for r in range(sp.nrows_total):
        sp.walk(r, 1)
    for r in reversed(range(sp.nrows_total)):
        sp.fold(r, 1)
    sp.check()
    _check("wide staged", window, dtype, out, ref, "single", True)
    assert torch.equal(out, _paint(dev, p, m, window, **ORDERED))


# ------------------------------------------------------------------ crowded: light cells next to a dense tile
@WINDOWS
@DTYPES
def test_crowded_through_the_overflow_list(dev, refs, window, dtype):
    pos, mass, ref = refs("crowded", window)
    p, m = _dev_arrays(dev, pos, mass, dtype)
    grid = _paint(dev, p, m, window, method="tiled", accumulate=False, hint="ordered", check_dropped=False, want=(SP, 1, False))
    _check("crowded overflow list", window, dtype, grid, ref, "single", False)


@WINDOWS
@DTYPES
def test_crowded_through_the_late_list(dev, refs, window, dtype):
    """A tenth of the particles in one tile: the scatter path's late list holds the surplus at either dtype (float32: through
    LDS tiles, float64: global atomics).  Six tenths do not fit: the paint repaints on the exact two-pass lists."""
    pos, mass, ref = refs("crowded-late", window)
    perm = np.random.default_rng(7).permutation(NP)
    p, m = _dev_arrays(dev, pos[perm], mass[perm], dtype)
    grid = _paint(dev, p, m, window, method="tiled", accumulate=False, hint="scattered", check_dropped=False, want=(SC, 1, False))
    _check("crowded late list", window, dtype, grid, ref, "single", False)
    pos, mass, ref = refs("crowded", window)
    p, m = _dev_arrays(dev, pos[perm], mass[perm], dtype)
    grid = _paint(dev, p, m, window, method="tiled", accumulate=False, hint="scattered", check_dropped=False, want=(TP, 2, True))
    _check("crowded late list full", window, dtype, grid, ref, "two-pass", True)


@WINDOWS
@DTYPES
def test_crowded_two_pass_quantum_per_column(dev, refs, window, dtype):
    """The two-pass lists scale the quantum by the column's largest tile: light cells of the blob's own column are
    quantised 2^3 times as coarsely as on the single pass, those of every other column far finer."""
    pos, mass, ref = refs("crowded", window)
    p, m = _dev_arrays(dev, pos, mass, dtype)
    grid = _paint(dev, p, m, window, **TWO_PASS)
    _check("crowded tiled2", window, dtype, grid, ref, "two-pass", True)
    q2, q1 = ref.quanta(NPT[dtype], "two-pass")[1], ref.quanta(NPT[dtype], "single")[1]
    assert q2.max() == 8 * q1.max() and q2.min() < q1.min()


# ------------------------------------------------------------------ signs and zeros
@WINDOWS
@DTYPES
def test_signed_masses_and_cancelling_pairs(dev, refs, window, dtype):
    pos, mass, ref = refs("signed", window)
    only = torch.from_numpy(pa.pair_only_cells(pos, mass, window)).cuda()
    assert int(only.sum()) > 1000
    p, m = _dev_arrays(dev, pos, mass, dtype)
    for path, (kw, lists) in WALKS.items():
        if path == "scattered":
            continue
        grid = _paint(dev, p, m, window, **kw)
        _check("signed " + path, window, dtype, grid, ref, lists, True)
        assert not grid[only].any()                      # +m and -m at one place: exact integers that cancel
        assert torch.equal(_paint(dev, p, -m, window, **kw), -grid)
    _check("signed direct", window, dtype, dev.paint(p, m, N, L, window, scale=SCALE, method="direct"), ref, None, False)


@WINDOWS
@DTYPES
def test_zero_masses(dev, refs, window, dtype):
    pos, mass, ref = refs("all-zero", window)
    p, m = _dev_arrays(dev, pos, mass, dtype)
    for path, (kw, lists) in WALKS.items():
        if path != "scattered":
            grid = _paint(dev, p, m, window, **kw)
            assert not grid.any() and not torch.signbit(grid).any()
    assert not dev.paint(p, m, N, L, window, scale=SCALE, method="direct").any()
    pos, mass, ref = refs("some-zero", window)
    p, m = _dev_arrays(dev, pos, mass, dtype)
    for path, (kw, lists) in WALKS.items():
        if path != "scattered":
            _check("some-zero " + path, window, dtype, _paint(dev, p, m, window, **kw), ref, lists, True)


# ------------------------------------------------------------------ exact relations of the column walk
# One large and one small |k| of each sign.  Every non-zero cell of a column walk is a multiple of the smallest quantum
# q_min of the grid and at most the largest sum of |terms|, so 2^k keeps all of them normal when q_min * 2^k >= the
# smallest normal number and 2 max(A) * 2^k <= the largest; the reference cells the walk can resolve (|S| >= q_min) then
# stay normal too.  The same for the scaled masses, scale and positions themselves.
K_OF = {"f32": (-60, -3, 2, 60), "f64": (-500, -3, 2, 500)}


def _normal(a, T, k=0):
    a = np.abs(np.asarray(a, dtype=np.longdouble))[np.asarray(a) != 0] * np.longdouble(2.0) ** k
    return len(a) == 0 or (a.min() >= np.finfo(T).tiny and a.max() <= np.finfo(T).max / 2)


@WINDOWS
@DTYPES
@pytest.mark.parametrize("path", ["ordered", "tiled2"])
def test_exact_power_of_two_sign_and_permutation_relations(dev, refs, window, dtype, path):
    T = NPT[dtype]
    pos, mass, ref = refs("wide-" + dtype, window)
    kw, lists = WALKS[path]
    qmin = float(ref.quanta(T, lists)[1].min())
    S, A = ref.S, ref.A
    resolved = np.abs(S) >= qmin
    assert resolved.sum() > S.size // 2                 # (the relation is about most of the grid, not a few heavy cells)
    p, m = _dev_arrays(dev, pos, mass, dtype)
    base = _paint(dev, p, m, window, **kw)
    for k in K_OF[dtype]:
        f = 2.0 ** k
        assert _normal(S[resolved], T, k) and _normal([qmin, 2 * float(A.max())], T, k), (k, "reference cells leave the normal range")
        assert _normal(mass, T, k) and _normal(pos, T, k) and _normal([SCALE], np.float64, k) and _normal([SCALE], np.float64, -k)
        scaled = base * f
        assert torch.equal(_paint(dev, p, m * f, window, **kw), scaled), ("masses", k)
        st = {}
        assert torch.equal(dev.paint(p, m, N, L, window, scale=SCALE * f, method=kw["method"], accumulate=False,
                                     hint=kw.get("hint"), stats=st), scaled), ("scale", k)
        assert torch.equal(dev.paint(p, m * f, N, L, window, scale=SCALE / f, method=kw["method"], accumulate=False,
                                     hint=kw.get("hint")), base), ("masses and scale", k)
        assert torch.equal(dev.paint(p * f, m, N, L * f, window, scale=SCALE, method=kw["method"], accumulate=False,
                                     hint=kw.get("hint")), base), ("positions and box", k)
    assert torch.equal(_paint(dev, p, -m, window, **kw), -base)
    if path == "tiled2":                       # (the single pass's permutation: test_wide_masses_column_walk[scattered])
        perm = torch.from_numpy(np.random.default_rng(13).permutation(NP)).cuda()
        assert torch.equal(_paint(dev, p[perm].contiguous(), m[perm].contiguous(), window, **kw), base)


# ------------------------------------------------------------------ NaN and Inf masses are refused
def _guarded(call):
    """(exception or None, names of the library calls that were handed device memory)."""
    from tests.input_layouts import LibraryGuard
    with LibraryGuard() as g:
        try:
            call()
            err = None
        except Exception as e:              # noqa: BLE001 - the test asserts on its type
            err = e
    return err, g.names


@DTYPES
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_masses_are_refused_before_any_paint_kernel(dev, refs, dtype, bad):
    pos, mass, ref = refs("some-zero", "cic")
    p, m = _dev_arrays(dev, pos, mass, dtype)
    clean = {path: _paint(dev, p, m, "cic", **kw) for path, (kw, _) in WALKS.items() if path != "scattered"}
    for where in (0, 1, NP // 2 + 3, NP - 1):                  # first vector, an odd element, the middle, the tail
        mb = m.clone()
        mb[where] = bad
        calls = {
            "tiled": lambda: dev.paint(p, mb, N, L, "cic", scale=SCALE, method="tiled", accumulate=False, hint="ordered"),
            "tiled2": lambda: dev.paint(p, mb, N, L, "cic", scale=SCALE, method="tiled2", accumulate=False),
            "scattered": lambda: dev.paint(p, mb, N, L, "tsc", scale=SCALE, method="tiled", accumulate=False, hint="scattered"),
            "staged": lambda: dev.StagedPaint(p, mb, N, L, "cic", torch.empty((N, N, N), dtype=TT[dtype], device="cuda"), scale=SCALE),
        }
        for name, call in calls.items():
            err, names = _guarded(call)
            assert isinstance(err, ValueError) and "NaN or Inf" in str(err), (name, where, err)
            assert names == ["ast_absmax_finite"], (name, names)
    # the slab pipeline's operations go through the same two entries
    from astrild_amd.slab import HipSlabOps
    # (a buffer that starts at plane 5 and holds all 64: enough particles for the tiled paint, which "auto" then takes)
    ops = HipSlabOps(TT[dtype])
    mb = m.clone()
    mb[NP // 3] = bad
    buf = ops.empty((N, N, N))
    for call in (lambda: ops.paint(p, mb, N, L, "cic", buf, 5, N), lambda: ops.staged_paint(p, mb, N, L, "cic", buf, 5, N)):
        err, names = _guarded(call)
        assert isinstance(err, ValueError) and names == ["ast_absmax_finite"], (err, names)
    good = ops.paint(p, m, N, L, "cic", buf, 5, N, check=True)
    rolled = torch.roll(dev.paint(p, m, N, L, "cic", method="tiled2", accumulate=False), -5, 0)      # (other tiles: not bit for bit)
    assert ((good - rolled).abs() <= 1e-5 * rolled.abs().max()).all()
    # the direct paint has no reduction over the masses (and gets none): float atomics carry the NaN / Inf into the cells the
    # particle touches, by the rules of the arithmetic, and nowhere else
    direct = dev.paint(p, m, N, L, "cic", scale=SCALE, method="direct")
    hit = dev.paint(p, mb, N, L, "cic", scale=SCALE, method="direct")
    touched = torch.from_numpy(pa.Reference(pos[NP // 3: NP // 3 + 1], None, N, L, "cic").K > 0).cuda()
    assert int(touched.sum()) == 8 and not torch.isfinite(hit[touched]).any() and torch.isfinite(hit[~touched]).all()
    assert ((hit[~touched] - direct[~touched]).abs() <= 1e-5 * direct[~touched].abs()).all()
    # after the error a valid paint gives the clean grid, bit for bit
    for path, (kw, _) in WALKS.items():
        if path != "scattered":
            assert torch.equal(_paint(dev, p, m, "cic", **kw), clean[path])


def test_unit_masses_run_no_mass_reduction(dev, refs):
    pos, _, _ = refs("some-zero", "cic")
    p = dev.as_device(pos.astype(np.float32))
    err, names = _guarded(lambda: dev.paint(p, None, N, L, "cic", method="tiled", accumulate=False, hint="ordered"))
    assert err is None and "ast_absmax_finite" not in names and "ast_minmax" not in names and "ast_paint_tiled" in names


@DTYPES
def test_absmax_finite_entry(dev, dtype):
    """ast_absmax_finite: {0 or -1, max |x|} in one pass - aligned and unaligned views, ragged tails, NaN / Inf anywhere;
    ast_minmax keeps skipping NaN."""
    from astrild_amd import _lib, lensing
    rng = np.random.default_rng(3)

    def run(t):
        out = torch.empty(2, dtype=torch.float64, device="cuda")
        dev.check(_lib.lib().ast_absmax_finite(dev.ptr(t), dev.real_code(t), t.numel(), dev.ptr(out), dev.stream()), "ast_absmax_finite")
        return out.tolist()

    for count in (1, 3, 4, 5, 1023, 4096, 70001, 9_000_001):
        v = rng.uniform(-2.0, 1.0, size=count + 1).astype(NPT[dtype])
        t = dev.as_device(v)
        for view, host in ((t[:count], v[:count]), (t[1:], v[1:])):
            assert run(view) == [0.0, float(np.abs(host.astype(np.float64)).max())]
        for bad in (float("nan"), float("inf"), float("-inf")):
            for where in sorted({0, count // 2, count - 1}):
                tb = t[:count].clone()
                tb[where] = bad
                flag, top = run(tb)
                rest = np.delete(v[:count], where).astype(np.float64)
                assert flag == -1.0
                assert top == (float("inf") if np.isinf(bad) else (float(np.abs(rest).max()) if count > 1 else top))
                if np.isnan(bad) and count > 1:
                    lo, hi = lensing.minmax(tb)
                    assert (lo, hi) == (float(rest.min()), float(rest.max()))
    assert run(torch.zeros(77, dtype=TT[dtype], device="cuda")) == [0.0, 0.0]
