"""CPU-only: the workspace layout of the tiled paint is pinned.

ast_paint_tiled_workspace_bytes and ast_paint_tiled_halo only do arithmetic, so they run without a GPU.  The byte count
and the offset of the halo records inside the workspace (what ast_fft_tile_power_3d_halo reads after a DEFER_FOLD paint)
are compared, exactly, with values recorded from the library before the layout code was gathered into one function
(tests/golden/paint_layout_parent.json).  A reordered carve, a forgotten seam area or a changed default of the walk plan
shows up here as a different number."""
import ctypes as ct
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "paint_layout_parent.json")

WINDOWS = (1, 2)                         # AST_WIN_CIC, AST_WIN_TSC
DTYPES = (0, 1)                          # AST_F32, AST_F64
GEOMETRIES = ((64, 64, 150000), (128, 20, 1 << 21), (1024, 1024, 1 << 30), (1024, 136, 1 << 27), (2048, 2048, 1 << 30))   # (nmesh, nx_alloc, np)
FLAGS = (0, 1, 2, 3, 2 | 4, 2 | 8, 2 | 16, 2 | 8 | 16)
NOT_TILED = ((100, 100, 1 << 20), (48, 48, 1 << 20), (1000, 125, 1 << 24))      # nmesh not a multiple of 32: 0 bytes
# the test hooks that change the walk plan, and with it the seam area: (variable, value, flags they act on)
HOOKS = (("AST_PAINT_ZSEG", "4", (2, 2 | 4, 2 | 8, 2 | 16)), ("AST_PAINT_XCHUNK_MB", "4", (2 | 16, 2 | 8 | 16)))
LATE_SIZES = (1 << 20, (1 << 20) + 1, (1 << 20) + 7, 3 * 2 ** 20 + 5, 1 << 21, 1 << 24, (1 << 30) - 1, 1 << 30, 1 << 31,
              (1 << 32) - 67, (1 << 32) - 66)                                   # the explicit sizes of tests/test_abi.py
BASE = 1 << 40                           # a made-up workspace address: nothing is read or written through it


def rows():
    """(hook variable or "", its value, window, dtype, np, nmesh, nx_alloc, flags)"""
    out = []
    for window in WINDOWS:
        for dtype in DTYPES:
            for nmesh, nx_alloc, npart in GEOMETRIES:
                out += [("", "", window, dtype, npart, nmesh, nx_alloc, flags) for flags in FLAGS]
                for name, value, flags_set in HOOKS:
                    out += [(name, value, window, dtype, npart, nmesh, nx_alloc, flags) for flags in flags_set]
            out += [("", "", window, dtype, npart, nmesh, nx_alloc, flags) for nmesh, nx_alloc, npart in NOT_TILED for flags in (0, 2)]
    return out


def key(row):
    return " ".join(str(v) for v in row if v != "")


def measure(lib, row):
    """[workspace bytes, offset of the halo records (None without AST_PAINT_OVERWRITE or where no tiling exists)].
    The hook variables are read by the library at every call, from the process environment."""
    name, value, window, dtype, npart, nmesh, nx_alloc, flags = row
    old = {n: os.environ.pop(n, None) for n, _, _ in HOOKS}
    try:
        if name:
            os.environ[name] = value
        nbytes = int(lib.ast_paint_tiled_workspace_bytes(window, dtype, npart, nmesh, nx_alloc, flags))
        rec_off = None
        if (flags & 2) and nbytes:
            rec = ct.c_void_p(0)
            rc = lib.ast_paint_tiled_halo(ct.c_void_p(BASE), window, dtype, npart, nmesh, nx_alloc, flags, ct.byref(rec))
            assert rc == 0, (row, rc)
            rec_off = int(rec.value) - BASE
    finally:
        for n, v in old.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = v
    return [nbytes, rec_off]


def measure_all(lib):
    from astrild_amd import _lib
    return {"layout": {key(r): measure(lib, r) for r in rows()},
            "late_capacity": {f"{dtype} {npart}": int(lib.ast_paint_scatter_late_capacity(dtype, npart))
                              for dtype in (_lib.F32, _lib.F64) for npart in LATE_SIZES}}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_table_covers_what_it_should():
    table = rows()
    assert len({key(r) for r in table}) == len(table)
    plain = [r for r in table if not r[0]]
    for window in WINDOWS:
        for dtype in DTYPES:
            for nmesh, nx_alloc, npart in GEOMETRIES:
                assert {r[7] for r in plain if r[2:7] == (window, dtype, npart, nmesh, nx_alloc)} == set(FLAGS)
    assert any(r[0] == "AST_PAINT_ZSEG" for r in table) and any(r[0] == "AST_PAINT_XCHUNK_MB" for r in table)
    assert all(r[5] % 32 for r in table if r[5:7] in {(n, a) for n, a, _ in NOT_TILED})


def test_workspace_layout_matches_the_recorded_one(hip, golden):
    got = measure_all(hip)["layout"]
    assert sorted(got) == sorted(golden["layout"])
    wrong = {k: (got[k], golden["layout"][k]) for k in got if got[k] != golden["layout"][k]}
    assert not wrong, f"{len(wrong)} rows differ (got, recorded), e.g. {dict(list(wrong.items())[:5])}"


def test_recorded_layout_is_not_trivial(golden):
    """What the recorded values must show for the comparison to mean something: untileable grids give 0 bytes; the halo
    records lie inside the workspace; the seam area lies behind them and follows the plan (AST_PAINT_ZSEG=4 makes the
    workspace larger at 1024^3, where the default walk is not segmented, and leaves the records where they were)."""
    lay = golden["layout"]
    for r in rows():
        nbytes, rec_off = lay[key(r)]
        if (r[5], r[6]) in {(n, a) for n, a, _ in NOT_TILED}:
            assert nbytes == 0 and rec_off is None
            continue
        assert nbytes > 0 and nbytes % 256 == 0
        assert (rec_off is not None) == bool(r[7] & 2)
        if rec_off is not None:
            assert 0 < rec_off < nbytes and rec_off % 256 == 0
    for window in WINDOWS:
        for dtype in DTYPES:
            plain = lay[key(("", "", window, dtype, 1 << 30, 1024, 1024, 2))]
            seg = lay[key(("AST_PAINT_ZSEG", "4", window, dtype, 1 << 30, 1024, 1024, 2))]
            assert seg[0] > plain[0] and seg[1] == plain[1]


def test_late_capacity_matches_the_recorded_one(hip, golden):
    assert measure_all(hip)["late_capacity"] == golden["late_capacity"]
