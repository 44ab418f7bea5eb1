"""CPU-only: the per-cell bounds of tests/paint_accuracy.py against its numpy emulator of the fixed-point column walk.

The emulator meets the column-walk bound on every input of tests/test_gpu_paint_accuracy.py, is exactly covariant under the
power-of-two relations asserted there of the kernels, and four mutants of it - each a way the walk could be subtly wrong
in a low-density cell - break the new bound while the older criterion, a tolerance scaled by the LARGEST cell of the grid,
lets them pass."""
import numpy as np
import pytest

from tests import paint_accuracy as pa

N, L, SCALE = pa.N, pa.L, pa.SCALE
DTYPES = {"f32": np.float32, "f64": np.float64}


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name, window):
        if (name, window) not in cache:
            pos, mass = pa.make_input(name)
            cache[name, window] = (pos, mass, pa.Reference(pos, mass, N, L, window, scale=SCALE, keep_terms=True))
        return cache[name, window]
    return get


def test_quantum_model_matches_the_figures_of_the_kernel_comments():
    # 2^21 particles on 1024 tiles: q = 2^-31 vmax at fp32, 2^-46 vmax at fp64
    cap = pa.tile_capacity(1 << 21, 1024)
    assert cap == 4096
    assert pa.quantum(5 * cap, 3.0, 0.5, np.float32)[0] == 1.5 * 2.0 ** -31
    assert pa.quantum(5 * cap, 3.0, 0.5, np.float64)[0] == 1.5 * 2.0 ** -46
    # a small column of the two-pass lists: the exponent is capped at 50 (every term below 2^50)
    assert pa.quantum(1, 1.0, 1.0, np.float64)[0] == 2.0 ** -50
    assert pa.quantum(1, 1.0, 1.0, np.float32)[0] == 2.0 ** -45
    assert pa.quantum(7, 0.0, 1.0, np.float32)[0] == pa.quantum(7, 1.0, 1.0, np.float32)[0]       # all masses zero: vmax = 1
    assert pa.tile_capacity(100, 128) == 576 and pa.tile_capacity(pa.NP, 128) == 2048


def test_reference_sums_match_the_oracle_paint():
    from oracle import mesh as omesh
    pos, mass = pa.make_input("signed")
    for window in ("cic", "tsc"):
        ref = pa.Reference(pos, mass, N, L, window, scale=SCALE)
        want = omesh.paint(pos, mass, N, L, window) * SCALE
        A = ref.A.astype(np.float64)
        assert (np.abs(ref.S.astype(np.float64) - want) <= 64 * pa.U64 * A).all()
        assert int(ref.K.sum()) == len(pos) * {"cic": 8, "tsc": 27}[window]
        assert (np.abs(ref.S) <= ref.A).all() and (ref.D >= ref.A).all()
    # a slab buffer: the cells of the whole grid's planes x_start .. x_start + nx_alloc - 1
    sel = (np.floor(pos[:, 0] * N / L) % N >= 16) & (np.floor(pos[:, 0] * N / L) % N < 31)
    slab = pa.Reference(pos[sel], mass[sel], N, L, "cic", scale=SCALE, x_start=15, nx_alloc=18)
    want = omesh.paint(pos[sel], mass[sel], N, L, "cic")[15:33] * SCALE
    assert (np.abs(slab.S.astype(np.float64) - want) <= 64 * pa.U64 * slab.A.astype(np.float64)).all()


# (the wide mass range is chosen per dtype)
NAME_DTYPE = [(name, dtype) for name in pa.INPUTS for dtype in ("f32", "f64") if not name.startswith("wide") or name == "wide-" + dtype]


@pytest.mark.parametrize("lists", ["single", "two-pass"])
@pytest.mark.parametrize("window", ["cic", "tsc"])
@pytest.mark.parametrize("name,dtype", NAME_DTYPE)
def test_emulator_meets_the_column_walk_bound(refs, name, window, dtype, lists):
    T = DTYPES[dtype]
    pos, mass, ref = refs(name, window)
    for offset in (0.0, float(ref.S.sum() / N ** 3)):
        got = pa.emulate(pos, mass, N, L, window, T, lists, scale=SCALE, offset=offset, terms=ref.terms)
        ratio, rel, over = pa.measure(got, ref, ref.walk_bound(T, lists, offset), offset)
        print(f"[{name} {window} {dtype} {lists} offset {offset:.3g}] error / bound {ratio:.3f}  error / A {rel:.3g}")
        assert over == 0 and ratio <= 1.0
        bound = ref.walk_bound(T, lists, offset)
        assert pa.total_mass_error(got, ref, offset) <= bound.sum()
    if name == "all-zero":
        assert not got.any() or offset != 0.0
    if name == "signed":
        plain = pa.emulate(pos, mass, N, L, window, T, lists, scale=SCALE, terms=ref.terms)
        only = pa.pair_only_cells(pos, mass, window)
        assert only.sum() > 1000 and not plain[only].any()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("window", ["cic", "tsc"])
def test_emulator_is_exactly_covariant_under_powers_of_two(window, dtype):
    T = DTYPES[dtype]
    pos, mass = pa.make_input("wide-" + dtype)
    pos, mass = pos[:: 8], mass[:: 8]
    rng = np.random.default_rng(3)
    for lists in ("single", "two-pass"):
        run = lambda p=pos, m=mass, s=SCALE, box=L: pa.emulate(p, m, N, box, window, T, lists, scale=s).astype(np.float64)
        base = run()
        for k in (-20, -3, 2, 17):
            f = 2.0 ** k
            assert np.array_equal(run(m=mass * f), base * f)
            assert np.array_equal(run(s=SCALE * f), base * f)
            assert np.array_equal(run(m=mass * f, s=SCALE / f), base)
            assert np.array_equal(run(p=pos * f, box=L * f), base)
        assert np.array_equal(run(m=-mass), -base)
        perm = rng.permutation(len(pos))
        assert np.array_equal(run(p=pos[perm], m=mass[perm]), base)


def _light_cells(ref, mass, terms):
    """Cells that hold light particles only, and have at least one term."""
    heavy = np.asarray(mass)[terms.part] > 1.0
    touched_by_heavy = terms.cell_sum(heavy.astype(np.int64), np.int64) > 0
    return (ref.K > 0) & ~touched_by_heavy


MUTANTS = {
    # name -> (grid dtype of the emulation, what the mutant does)
    "dropped-centre-deposit": "f32",
    "truncation": "f32",
    "quantum-one-bit-coarser": "f32",
    "light-terms-in-fp32": "f64",
}


@pytest.mark.parametrize("window", ["cic", "tsc"])
@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutants_break_the_new_bound_and_pass_the_old_criterion(refs, mutant, window):
    """The crowded input: blob cells hold tens of thousands of particles of mass 2^10, lattice cells about one of 2^-10."""
    T = DTYPES[MUTANTS[mutant]]
    pos, mass, ref = refs("crowded", window)
    t = ref.terms
    light = _light_cells(ref, mass, t)
    assert light.sum() > 10000
    kw = {}
    if mutant == "dropped-centre-deposit":
        # one light particle's deposit into its base cell, a light cell
        cand = np.flatnonzero(t.centre & (np.asarray(mass)[t.part] < 1.0) & light.reshape(-1)[np.maximum(t.cell, 0)] & t.inside)
        kw["drop_term"] = int(cand[len(cand) // 2])
    elif mutant == "truncation":
        kw["truncate"] = True
    elif mutant == "quantum-one-bit-coarser":
        kw["coarser"] = 1
    else:
        kw["fp32_particles"] = np.asarray(mass) < 1.0
    for lists in ("single", "two-pass"):
        good = pa.emulate(pos, mass, N, L, window, T, lists, scale=SCALE, terms=t)
        bad = pa.emulate(pos, mass, N, L, window, T, lists, scale=SCALE, terms=t, **kw)
        bound = ref.walk_bound(T, lists)
        assert pa.measure(good, ref, bound)[2] == 0
        ratio, rel, over = pa.measure(bad, ref, bound)
        err = np.abs(bad.astype(np.float64) - ref.S.astype(np.float64))
        over_light = int(((err > bound) & light).sum())
        print(f"[{mutant} {window} {lists}] cells over the bound {over} (light {over_light}), error / bound {ratio:.3g}, "
              f"error / A {rel:.3g}, error / largest cell {err.max() / float(ref.S.max()):.3g}")
        assert over_light >= 1, "the per-cell bound must see the mutant in a light cell"
        assert pa.old_criterion(bad, ref.S, np.float32), "... which a tolerance scaled by the largest cell lets pass"
        assert pa.old_criterion(bad, ref.S, T)
