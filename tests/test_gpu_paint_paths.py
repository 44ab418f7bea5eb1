"""GPU parity of every path of the tiled overwrite paint, at float32 and float64, against the oracle (float64 numpy).

``device.paint`` looks at an overwrite paint of >= 2^20 particles onto the whole grid first (``device.probe_input``: order
in memory, estimated overflow of the tile segments) and runs the single pass, the two-level bucket scatter with its late
list, or the exact two-pass lists.  Each row below builds an input for one of them on a 128^3 grid: 2^21 particles, 1024
tiles of 8 x 8 x 32 cells, 64 buckets of 16 tiles (a bucket: one tile row x and four tile rows y).  Part of the lattice is
replaced by compact Gaussian blobs (sigma = 0.5 cell), each centred in a tile of its own bucket, so that the blob tiles
overflow their segments by a chosen amount.  Coordinates and masses are rounded to float32 first: one oracle grid serves
both dtypes.  Every row asserts the probe values it relies on, so that it cannot drift onto another path unnoticed.
"""
import numpy as np
import pytest

from oracle import mesh as omesh, fftpower as offt
from tests import paint_accuracy as pa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, L = 128, 1000.0
NP = N ** 3
TILE = (8, 8, 32)                       # cells per tile (x, y, z)
SIGMA = 0.5 * L / N                     # blob width: half a cell
DT = {"f32": torch.float32, "f64": torch.float64}
SC, TP, SP = "scattered", "two-pass", "single-pass"


def _limit(dev, dtype):
    """The probe's estimate up to which device.paint takes the bucket scatter."""
    return dev.scatter_overflow_limit(DT[dtype], NP)


def _late_capacity(dev, dtype):
    return dev.scatter_late_capacity(DT[dtype], NP)


# name -> (blob fraction, blobs, shuffled, {dtype: path}, what the probe must read).  `probe`: (lo, hi] windows of the
# estimated overflow as functions of the two limits, or "limit-f32" / "limit-f64": tuned to just under that dtype's limit.
ROWS = {
    "uniform-ordered": (0.0, 0, False, {"f32": SP, "f64": SP}, "uniform"),
    "uniform-shuffled": (0.0, 0, True, {"f32": SC, "f64": SC}, "uniform"),
    "late-short": (0.05, 8, True, {"f32": SC, "f64": SC}, lambda l32, l64: (NP // 64, l64)),
    "late-f64-limit": (0.095, 4, True, {"f32": SC, "f64": SC}, "limit-f64"),
    "late-f64-over": (0.16, 4, True, {"f32": SC, "f64": TP}, lambda l32, l64: (l64, l32)),
    "late-f32-limit": (0.195, 4, True, {"f32": SC, "f64": TP}, "limit-f32"),
    "clustered-shuffled": (0.36, 4, True, {"f32": TP, "f64": TP}, lambda l32, l64: (l32, NP)),
    "clustered-ordered": (0.16, 4, False, {"f32": TP, "f64": TP}, lambda l32, l64: (NP // 64, NP)),
}


def _blob_centres(k):
    """k tile centres (box units), in k different tile rows x - k different buckets."""
    ntx, nty, ntz = N // TILE[0], N // TILE[1], N // TILE[2]
    c = []
    for j in range(k):
        tx, ty, tz = (j * ntx // k + 1) % ntx, (3 * j + 1) % nty, j % ntz
        c.append(((tx + 0.5) * TILE[0], (ty + 0.5) * TILE[1], (tz + 0.5) * TILE[2]))
    return np.array(c) * (L / N)


def _build(frac, k, shuffled):
    """(positions, masses) as float32 host arrays: the 128^3 lattice with round(frac * NP) particles (chosen at random
    indices) moved into k blobs, in lattice order or in one fixed permutation."""
    rng = np.random.default_rng(20261016)
    pos = omesh.lattice_particles(N, N, L, seed=20240601)
    mass = rng.uniform(0.5, 2.0, size=NP)
    nblob = int(round(frac * NP)) // k * k if k else 0
    if nblob:
        idx = rng.choice(NP, size=nblob, replace=False)
        which = np.repeat(np.arange(k), nblob // k)
        pos[idx] = np.mod(_blob_centres(k)[which] + SIGMA * rng.standard_normal((nblob, 3)), L)
    if shuffled:
        perm = np.random.default_rng(7).permutation(NP)
        pos, mass = pos[perm], mass[perm]
    return np.ascontiguousarray(pos, dtype=np.float32), mass.astype(np.float32)


class _Input:
    def __init__(self, dev, name):
        frac, k, shuffled, self.paths, want = ROWS[name]
        self.dev, self.name, self.k, self.shuffled = dev, name, k, shuffled
        l32, l64 = _limit(dev, "f32"), _limit(dev, "f64")
        if isinstance(want, str) and want.startswith("limit-"):
            # just under the limit: aim at 95 % of it, then correct the fraction by the probe's reading (the estimate
            # grows by one particle per particle moved into a full tile)
            lim = l32 if want == "limit-f32" else l64
            lo, hi = 0.9 * lim, lim
            for _ in range(4):
                self._make(frac)
                if lo < self.probe["overflow"] <= hi:
                    break
                frac += (0.95 * lim - self.probe["overflow"]) / NP
        else:
            self._make(frac)
            lo, hi = (-1, NP // 1000) if want == "uniform" else want(l32, l64)
        self.frac, self.window = frac, (lo, hi)
        p = self.probe
        assert lo < p["overflow"] <= hi, (name, frac, p, (lo, hi))
        assert (p["groupable"] < 0.25) == shuffled, (name, p)
        self._grids = {}

    def _make(self, frac):
        self.pos, self.mass = _build(frac, self.k, self.shuffled)
        self.probe = self.dev.probe_input(self.dev.as_device(self.pos), N, L)

    def device(self, dtype, masses):
        t = DT[dtype]
        return self.dev.as_device(self.pos, t), (self.dev.as_device(self.mass, t) if masses else None)

    def total(self, masses):
        return float(self.mass.astype(np.float64).sum()) if masses else float(NP)

    def oracle(self, window, masses):
        key = (window, masses)
        if key not in self._grids:
            self._grids[key] = omesh.paint(self.pos.astype(np.float64), self.mass.astype(np.float64) if masses else None,
                                           N, L, window)
        return self._grids[key]

    def accuracy(self, window, masses):
        """The per-cell quantities of tests/paint_accuracy.py around the oracle grid (K and the quanta: once per window)."""
        key = ("acc", window, masses)
        if key not in self._grids:
            mass = self.mass.astype(np.float64) if masses else None
            self._grids[key] = pa.OracleReference(self.pos.astype(np.float64), mass, N, L, window, self.oracle(window, masses),
                                                  share=self._grids.get(("acc", window, not masses)))
        return self._grids[key]


@pytest.fixture(scope="module")
def dev(hip):
    from astrild_amd import device
    torch.cuda.set_device(0)
    return device


@pytest.fixture(scope="module")
def inputs(dev):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Input(dev, name)
            print(f"\n[{name}] fraction {cache[name].frac:.5f} probe {cache[name].probe} window {cache[name].window}")
        return cache[name]
    return get


def _check_grid(grid, ref, total, dtype, acc=None, path=None):
    got = grid.cpu().numpy().astype(np.float64)
    if acc is not None:
        # cell by cell, the any-path bound of tests/paint_accuracy.py (path unknown: the looser of the two list formats per cell)
        T = np.float32 if dtype == "f32" else np.float64
        lists = ["two-pass"] if path == TP else ["single"] if path in (SP, SC) else ["single", "two-pass"]
        bound = np.maximum.reduce([acc.any_bound(T, l) for l in lists])
        ratio, rel, over = pa.measure(got, acc, bound)
        print(f"    per cell: error / bound {ratio:.3g}, error / A {rel:.3g}")
        assert over == 0, (ratio, rel, over)
    if dtype == "f64":
        np.testing.assert_allclose(got, ref, rtol=1e-11, atol=1e-11 * ref.max())
        assert got.sum() == pytest.approx(total, rel=1e-12)
    else:
        np.testing.assert_allclose(got, ref, rtol=0, atol=3e-6 * ref.max())
        assert got.sum() == pytest.approx(total, rel=1e-6)


def _paint_and_check(dev, inp, dtype, window, masses, want_path, want_attempts=1, **kw):
    pos, mass = inp.device(dtype, masses)
    st = {}
    grid = dev.paint(pos, mass, N, L, window, method="tiled", accumulate=False, stats=st, **kw)
    print(f"  [{inp.name} {dtype} {window} {'mass' if masses else 'unit'}] path {st['path']} attempts {st['attempts']} "
          f"late/overflow {st.get('overflow')} probe {inp.probe['overflow']}")
    assert (st["path"], st["attempts"]) == (want_path, want_attempts), st
    if st["path"] == SC:
        assert st["overflow"] <= _late_capacity(dev, dtype), st            # the late list held every record
    ref, acc = inp.oracle(window, masses), inp.accuracy(window, masses)
    _check_grid(grid, ref, inp.total(masses), dtype, acc, st["path"])
    # nothing on a whole periodic grid raises, and not checking the drop count loses nothing
    again = dev.paint(pos, mass, N, L, window, method="tiled", accumulate=False, check_dropped=False, **kw)
    if st["path"] == SC and st["overflow"] > 0:
        # (the late list is added with float atomics: the order, hence the last bits, varies from call to call)
        _check_grid(again, ref, inp.total(masses), dtype, acc, st["path"])
    else:
        assert torch.equal(grid, again)
    return st


@pytest.mark.parametrize("masses", [False, True], ids=["unit", "mass"])
@pytest.mark.parametrize("window", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", list(ROWS))
def test_paint_path_table(dev, inputs, name, dtype, window, masses):
    inp = inputs(name)
    st = _paint_and_check(dev, inp, dtype, window, masses, inp.paths[dtype])
    if name == "uniform-shuffled":
        assert st["overflow"] == 0
    elif name.startswith("late-") and st["path"] == SC:
        assert st["overflow"] > 0                                            # the late list was used


@pytest.mark.parametrize("masses", [False, True], ids=["unit", "mass"])
@pytest.mark.parametrize("window", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", ["late-short", "late-f64-limit", "late-f64-over"])
def test_late_list_through_lds_tiles(dev, inputs, name, dtype, window, masses, monkeypatch):
    """AST_PAINT_LATE_LDS_MIN=1: every non-empty late list is deposited through LDS tiles (counted, scanned, one
    workgroup per tile) instead of global atomics - at float64 with masses too."""
    inp = inputs(name)
    monkeypatch.setenv("AST_PAINT_LATE_LDS_MIN", "1")
    _paint_and_check(dev, inp, dtype, window, masses, inp.paths[dtype])


@pytest.mark.parametrize("window", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_scattered_hint_never_loses_a_deposit(dev, inputs, dtype, window):
    """hint="scattered" skips the probe: on this input the float64 late list (NP / 8 records) runs out of room.  On the
    whole periodic grid nothing can fall outside, so a dropped deposit is a capacity loss: the paint repaints through
    the two-pass lists - with check_dropped=False and without stats as well."""
    inp = inputs("late-f64-over")
    assert inp.probe["overflow"] > _late_capacity(dev, "f64")
    pos, mass = inp.device(dtype, True)
    grid = dev.paint(pos, mass, N, L, window, method="tiled", accumulate=False, hint="scattered", check_dropped=False)
    ref = inp.oracle(window, True)
    _check_grid(grid, ref, inp.total(True), dtype, inp.accuracy(window, True), SC if dtype == "f32" else TP)
    st = {}
    dev.paint(pos, mass, N, L, window, method="tiled", accumulate=False, hint="scattered", check_dropped=False, stats=st)
    assert (st["path"], st["attempts"]) == ((SC, 1) if dtype == "f32" else (TP, 2)), st


def test_paint_power_1d_float64_on_a_late_list_input(dev, inputs):
    """The whole float64 pipeline (probe, paint with the deferred fold, double transform) on the input whose late list
    would not fit at float64, against the oracle's spectrum of the oracle's grid."""
    inp = inputs("late-f64-over")
    pos, _ = inp.device("f64", False)
    res = dev.paint_power_1d(pos, None, N, L, "cic")
    want = offt.fftpower_1d(inp.oracle("cic", False), L)
    assert np.array_equal(res["modes"], want["modes"])
    np.testing.assert_allclose(res["power"], want["power"].real, rtol=1e-10)
