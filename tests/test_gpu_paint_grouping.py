"""The grouping kernel of the tiled paint's single pass (``tile_group_kernel``) at the ends of its units: windows of 32
particles, waves of 64, trips of 1024, intervals of 4096, the per-wave slices of its LDS lists, its 256-slot tile
table, the tile segments, closed tiles.

Every paint is ``dev.paint(..., method="tiled", hint="ordered", accumulate=False, stats=st)`` - the single pass at any
particle count - on a 64^3 grid (8 x 8 x 2 tiles of 8 x 8 x 32 cells) unless stated, and is held against the float64
oracle with the tolerances of tests/test_gpu_paint_paths.py.  Each case is painted again, once more on a workspace
full of 0xFF bytes (tests/dirty_memory.py), and the repeats must give the same bits whenever nothing went through the
overflow list (its deposits are float atomics, whose order varies).  Coordinates and masses are rounded to float32
first, so one oracle grid serves both dtypes.

The earlier grouping (per-lane window decisions, lists shared by the waves) is gone from the tree, and a library takes
a minute to compile: no test builds a second one.  ``scripts/group_variant_hashes.py`` paints ``variant_cases()`` below
with whatever library is loaded and prints the grids' hashes, for comparing any two builds by hand - this tree against
a build of another commit loaded through ``ASTRILD_HIP_LIB``, for example (profiles/EXPERIMENTS.md, "Paint
grouping"); the suite itself rests on the oracle and on the record and stray counts.
"""
import hashlib

import numpy as np
import pytest

from oracle import mesh as omesh
from tests import dirty_memory as dm
from tests import paint_grouping_rule as rule
from tests.test_gpu_paint_paths import _check_grid

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, L = 64, 1000.0
TILE = (8, 8, 32)
DT = {"f32": torch.float32, "f64": torch.float64}
SP = "single-pass"


@pytest.fixture(scope="module")
def dev(hip):
    from astrild_amd import device
    torch.cuda.set_device(0)
    return device


# ---------------------------------------------------------------- inputs (host, float32 values)
def lattice(npart, n=N, seed=3, jitter=0.45):
    """The first npart sites of the n^3 cell-centre lattice in z-fastest order, moved by up to `jitter` cells."""
    i = np.arange(npart)
    cell = np.stack([i // (n * n) % n, i // n % n, i % n], axis=1).astype(np.float64)
    u = np.random.default_rng(seed).uniform(-jitter, jitter, size=(npart, 3))
    return ((cell + 0.5 + u) * (L / n)).astype(np.float32)


def masses(npart, seed=11):
    return np.random.default_rng(seed).uniform(0.5, 2.0, size=npart).astype(np.float32)


def tile_ids(pos, n=N):
    """Tile of the CIC base cell, as the kernel numbers them (z fastest)."""
    c = np.floor(pos.astype(np.float64) * (n / L)).astype(np.int64) % n
    nty, ntz = n // TILE[1], n // TILE[2]
    return (c[:, 0] // TILE[0] * nty + c[:, 1] // TILE[1]) * ntz + c[:, 2] // TILE[2]


def in_tiles(tiles, rng, n=N):
    """One position per entry of `tiles`, in a random cell of that tile, a quarter to three quarters into the cell."""
    nty, ntz = n // TILE[1], n // TILE[2]
    t = np.asarray(tiles)
    origin = np.stack([t // (nty * ntz) * TILE[0], t // ntz % nty * TILE[1], t % ntz * TILE[2]], axis=1)
    cell = origin + np.stack([rng.integers(0, TILE[a], size=len(t)) for a in range(3)], axis=1)
    return ((cell + rng.uniform(0.25, 0.75, size=(len(t), 3))) * (L / n)).astype(np.float32)


def window_interval(seed=5):
    """4096 positions: the 128 windows of rule.interval_windows(), every window's labels on tiles drawn afresh."""
    rng = np.random.default_rng(seed)
    ntiles = (N // TILE[0]) * (N // TILE[1]) * (N // TILE[2])
    tiles = []
    for name in rule.interval_windows():
        labels = rule.PATTERNS[name][0]
        uniq = np.unique(labels)
        draw = dict(zip(uniq.tolist(), rng.permutation(ntiles)[:len(uniq)].tolist()))
        tiles += [draw[int(lab)] for lab in labels]
    return in_tiles(tiles, rng), np.array(tiles)


# ---------------------------------------------------------------- one case: paint, oracle, repeats
def _sha(grid):
    return hashlib.sha256(grid.cpu().numpy().tobytes()).hexdigest()


def run_case(dev, pos, mass, dtype, window, n=N, hint="ordered", want=(SP, 1), check_dropped=True, ref=None):
    p = dev.as_device(pos, DT[dtype])
    m = None if mass is None else dev.as_device(mass, DT[dtype])
    kw = dict(method="tiled", hint=hint, accumulate=False, check_dropped=check_dropped)
    st = {}
    grid = dev.paint(p, m, n, L, window, stats=st, **kw)
    print(f"  [{dtype} {window} np={len(pos)} {'mass' if mass is not None else 'unit'}] {st}")
    if want is not None:
        assert (st["path"], st["attempts"]) == want, st
    if ref is None:
        ref = omesh.paint(pos.astype(np.float64), None if mass is None else mass.astype(np.float64), n, L, window)
    total = float(len(pos)) if mass is None else float(mass.astype(np.float64).sum())
    _check_grid(grid, ref, total, dtype)
    again = dev.paint(p, m, n, L, window, **kw)
    with dm.dirty(dm.NAN_BYTES) as alloc:
        dirty = dev.paint(p, m, n, L, window, **kw)
        assert alloc.allocations > 0                       # the grid and the workspace came back poisoned
    exact = st["path"] == SP and st["overflow"] == 0
    for g in (again, dirty):
        if exact:
            assert torch.equal(grid, g)
        else:
            _check_grid(g, ref, total, dtype)
    return st, grid, ref


# ---------------------------------------------------------------- 1. ends of every unit
ENDS = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 17]


@pytest.mark.parametrize("npart", ENDS)
def test_ends_of_every_unit(dev, npart):
    """Lanes past the end re-read the last particle: it must be deposited once (the grid total is the particle count)."""
    pos = lattice(npart)
    st, _, _ = run_case(dev, pos, None, "f32", "cic")
    assert st["overflow"] == 0
    assert (st["groups"], st["strays"]) == rule.count_lists(tile_ids(pos))
    run_case(dev, pos, masses(npart), "f64", "tsc")


# ---------------------------------------------------------------- 2. window composition
def test_window_composition_counts(dev):
    """One interval of hand-made windows: the kernel's record and stray counts are the restated rule's, window by window
    summed - every pattern in the lower and in the upper half of a wave."""
    pos, tiles = window_interval()
    assert np.array_equal(tile_ids(pos), tiles)
    want = [rule.PATTERNS[nm][1] for nm in rule.interval_windows()]
    assert rule.count_lists(tiles) == (sum(w[0] for w in want), sum(w[1] for w in want))
    for dtype in ("f32", "f64"):
        st, _, _ = run_case(dev, pos, None, dtype, "cic")
        assert st["overflow"] == 0
        assert (st["groups"], st["strays"]) == rule.count_lists(tiles), st


@pytest.mark.parametrize("name", list(rule.PATTERNS))
def test_single_window_in_either_half(dev, name):
    """One pattern alone: 32 particles (lower half of the first wave), then behind 32 particles of one far tile (upper)."""
    rng = np.random.default_rng(17)
    labels = rule.PATTERNS[name][0]
    uniq = np.unique(labels)
    draw = dict(zip(uniq.tolist(), rng.permutation(127)[:len(uniq)].tolist()))      # tile 127 is the filler's
    tiles = np.array([draw[int(lab)] for lab in labels])
    lower = in_tiles(tiles, rng)
    st, _, _ = run_case(dev, lower, None, "f32", "cic")
    assert (st["groups"], st["strays"], st["overflow"]) == (*rule.PATTERNS[name][1], 0), st
    upper = np.concatenate([in_tiles(np.full(32, 127), rng), lower])
    st, _, _ = run_case(dev, upper, None, "f32", "cic")
    rec, stray = rule.PATTERNS[name][1]
    assert (st["groups"], st["strays"], st["overflow"]) == (rec + 1, stray, 0), st


# ---------------------------------------------------------------- 3. capacities of the LDS lists
def test_every_particle_a_stray(dev):
    """3 x 4096 uniformly random particles: no window has 8 particles of one tile (128 tiles), every particle is a stray,
    and 1024 strays per wave and interval overflow any LDS list.  What the retry ladder makes of the overflow is its
    own business: the expected path is whatever ``next_paint_path`` says for the first attempt's statistics."""
    npart = 3 * 4096
    pos = np.random.default_rng(23).uniform(0.0, L, size=(npart, 3)).astype(np.float32)
    records, strays = rule.count_lists(tile_ids(pos))
    assert records == 0 and strays == npart
    p = dev.as_device(pos, torch.float32)
    first = {}
    dev.paint(p, None, N, L, "cic", method="tiled", hint="ordered", accumulate=False, stats=first, check_dropped=False)
    assert (first["path"], first["attempts"], first["groups"]) == (SP, 1, 0), first
    assert first["strays"] + first["overflow"] == npart, first
    for dtype, window in (("f32", "cic"), ("f64", "tsc")):
        # what the ladder makes of THIS paint's first attempt (the TSC base cell, hence its tiles, differ from CIC's)
        one = {}
        dev.paint(dev.as_device(pos, DT[dtype]), None, N, L, window, method="tiled", hint="ordered", accumulate=False,
                  stats=one, check_dropped=False)
        assert (one["path"], one["attempts"]) == (SP, 1), one
        again = dev.next_paint_path(SP, False, True, True, npart, one["overflow"])
        # (a second attempt on "scattered" may itself be followed by a third: only the single pass is this test's)
        want = (SP, 1) if again is None else None
        st, _, _ = run_case(dev, pos, None, dtype, window, want=want)
        if again is not None:
            assert st["attempts"] >= 2 and st["path"] != SP, st


# ---------------------------------------------------------------- 4. table collisions
def test_more_tiles_than_table_slots(dev):
    """128^3 grid, 1024 tiles, 2 x 4096 random particles sorted by tile: an interval meets about 512 distinct tiles, the
    table has 256 slots - whatever collides is placed one entry at a time."""
    n, npart = 128, 2 * 4096
    pos = np.random.default_rng(29).uniform(0.0, L, size=(npart, 3)).astype(np.float32)
    pos = pos[np.argsort(tile_ids(pos, n), kind="stable")]
    keys = tile_ids(pos, n)
    assert len(np.unique(keys[:4096])) > 256
    for dtype, window, mass in (("f32", "cic", None), ("f64", "cic", masses(npart)), ("f32", "tsc", masses(npart))):
        st, _, _ = run_case(dev, pos, mass, dtype, window, n=n)
        if window == "cic":
            assert (st["groups"], st["strays"], st["overflow"]) == (*rule.count_lists(keys), 0), st


# ---------------------------------------------------------------- 5. segment overflow
def test_tile_segments_overflow_to_the_late_list(dev):
    """20 000 particles in one cell beside a lattice: that tile's record segment is full long before they are placed, and
    most of them reach the grid through the overflow list.  That list is deposited with float atomics in the grid's
    dtype: 19 000 float32 additions into a cell that grows to 2500 leave about eps * sqrt(count) of it (measured with the
    particles spread over the cell: 3.9e-6 of the cell against the bound of 3e-6; the deposit kernel is not the
    grouping's).  The particles therefore sit at the cell's CENTRE: every weight is a small power of two or a sum of
    two, all sums are exact in float32, and a particle lost or deposited twice shows at any tolerance."""
    centre = (np.array([20.0, 36.0, 40.0]) + 0.5) * (L / N)
    blob = np.tile(centre.astype(np.float32), (20000, 1))
    assert (blob[0].astype(np.float64) == centre).all()                 # (k + 1/2) * 15.625 is exact in float32
    pos = np.concatenate([lattice(4096 + 300), blob, lattice(700, seed=4)])
    for dtype, window in (("f32", "cic"), ("f64", "tsc")):
        st, _, _ = run_case(dev, pos, None, dtype, window, check_dropped=False)
        assert st["overflow"] > 0, st


# ---------------------------------------------------------------- 6. geometry edges
def edge_positions():
    rng = np.random.default_rng(37)
    dx = L / N
    base = lattice(4096 + 77, seed=6)
    faces = base[:1500].copy()                       # exactly on tile faces, at 0 and at L
    k = np.arange(len(faces))
    faces[:, 0] = np.where(k % 3 == 0, (k % 9) * 8 * dx, faces[:, 0])
    faces[:, 1] = np.where(k % 3 == 1, (k % 9) * 8 * dx, faces[:, 1])
    faces[:, 2] = np.where(k % 3 == 2, (k % 3) * 32 * dx, faces[:, 2])
    near = base[1500:3000] + rng.choice([-L, 0.0, L], size=(1500, 3)).astype(np.float32)       # up to a box length outside
    far = base[3000:3300] + (rng.integers(-3, 4, size=(300, 3)) * L).astype(np.float32)        # further
    return np.concatenate([faces, near, far, base[3300:]]).astype(np.float32)


@pytest.mark.parametrize("with_mass", [False, True], ids=["unit", "mass"])
@pytest.mark.parametrize("window", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_geometry_edges(dev, dtype, window, with_mass):
    pos = edge_positions()
    assert pos.min() < -L and pos.max() > 2 * L and (pos == 0.0).any() and (pos == np.float32(L)).any()
    st, _, _ = run_case(dev, pos, masses(len(pos)) if with_mass else None, dtype, window)
    assert st["groups"] + st["strays"] + st["overflow"] >= 1


# ---------------------------------------------------------------- 7. closed tiles
def test_xsorted_late_particles_are_all_deposited(dev):
    """hint="xsorted" on the 64^3 lattice in ascending x with 1 % of the particles moved to the end of the array: when
    their turn comes their tile rows have been walked - closed - and they go through the late list.  All are deposited."""
    npart = N ** 3
    pos = lattice(npart, seed=8)
    late = np.random.default_rng(41).choice(npart * 3 // 4, size=npart // 100, replace=False)
    keep = np.ones(npart, bool)
    keep[late] = False
    pos = np.concatenate([pos[keep], pos[late]])
    ref = omesh.paint(pos.astype(np.float64), None, N, L, "cic")
    st, _, _ = run_case(dev, pos, None, "f32", "cic", hint="xsorted", ref=ref, check_dropped=False)
    assert st["overflow"] > 0, st                       # closed tiles were met: the pipeline ran in chunks
    run_case(dev, pos, None, "f64", "cic", hint="xsorted", ref=ref, check_dropped=False)


def test_staged_slab_paint_counts_a_late_particle_as_dropped(dev):
    """The slab instantiation: a 32-plane buffer of the 64^3 grid painted in stages, particles grouped in two parts.  The
    second part ends with ONE particle for a tile row that has been walked already: it cannot be deposited any more
    and is counted in `dropped`, exactly once; everything else is in the buffer."""
    x_start, nx = 16, 32
    rng = np.random.default_rng(43)
    npart = 2 * 4096
    pos = lattice(npart, seed=9)
    # ascending x inside the buffer: the first part holds tile rows 0 and 1 (planes 16 .. 31), the second rows 2 and 3
    x = np.concatenate([np.sort(rng.uniform(x_start + 0.25, x_start + 15.75, size=npart // 2)),
                        np.sort(rng.uniform(x_start + 16.25, x_start + nx - 1.25, size=npart // 2))])
    pos[:, 0] = (x * (L / N)).astype(np.float32)
    pos[-1, 0] = np.float32((x_start + 3.5) * (L / N))                                # tile row 0, in the last part
    p = dev.as_device(pos, torch.float32)
    buf = torch.empty((nx, N, N), dtype=torch.float32, device=p.device)
    sp = dev.StagedPaint(p, None, N, L, "cic", buf, x_start=x_start, nx_alloc=nx)
    assert sp.nrows_total == 4
    sp.reset()
    sp.group_part(0, 2)
    sp.walk(0, 2)
    sp.group_part(1, 2, closed_row0=0, closed_nrows=2)
    sp.walk(2, 2)
    sp.fold(0, 4)
    assert int(sp.dropped.item()) == 1
    from astrild_amd import _lib
    with pytest.raises(_lib.AstrildHipError):
        sp.check()
    ref = omesh.paint(pos[:-1].astype(np.float64), None, N, L, "cic")[x_start:x_start + nx]
    got = buf.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(got, ref, rtol=0, atol=3e-6 * ref.max())
    assert got.sum() == pytest.approx(npart - 1, rel=1e-6)


# ---------------------------------------------------------------- for scripts/group_variant_hashes.py
def variant_cases():
    """(name, positions, masses, dtype, window, grid side) of cases whose overflow list stays empty: their grids do not
    depend on the order of the lists, so two builds of the grouping must give the same bits."""
    yield "windows", window_interval()[0], None, "f32", "cic", N
    for npart in (33, 1025, 4097, 2 * 4096 + 17):
        yield f"ends-{npart}", lattice(npart), masses(npart), "f32", "tsc", N
    e = edge_positions()
    yield "edges", e, masses(len(e)), "f64", "cic", N
    pos = np.random.default_rng(29).uniform(0.0, L, size=(2 * 4096, 3)).astype(np.float32)
    yield "collisions", pos[np.argsort(tile_ids(pos, 128), kind="stable")], None, "f32", "cic", 128


def variant_hashes(dev):
    out = {}
    for name, pos, mass, dtype, window, n in variant_cases():
        st = {}
        grid = dev.paint(dev.as_device(pos, DT[dtype]), None if mass is None else dev.as_device(mass, DT[dtype]), n, L,
                         window, method="tiled", hint="ordered", accumulate=False, stats=st)
        out[name] = [_sha(grid), st["groups"], st["strays"], st["overflow"]]
    return out
