"""CPU-only: which path a tiled ``device.paint`` takes first and which follows which after an attempt, case by case.
``first_paint_path``, ``paint_probe_kind``, ``next_paint_path`` and ``paint_flags`` are plain functions of plain values: no
GPU and no shared library.  The tables below are written out by hand from the rules in ``paint``'s docstring; the GPU-side
proof that the paint follows them is tests/test_gpu_paint_paths.py."""
import itertools

import pytest

from astrild_amd import device as dev

NP = 1 << 21
LIMIT32, LIMIT64 = 419430, 209715            # four fifths of NP / 4 and of NP / 8
TWO_PASS, OVERWRITE, DEFER_FOLD, SCATTERED, XSORTED = 1, 2, 4, 8, 16      # include/astrild_hip.h (tests/test_abi.py compares)
SP, SC, TP = "single-pass", "scattered", "two-pass"
HINTS = (None, "scattered", "xsorted", "clustered", "ordered")


def probe(groupable, overflow):
    return {"groupable": groupable, "overflow": overflow, "max_tile": 0, "mean_tile": 1.0, "samples": 65536}


def test_paint_constants_are_importable_without_the_library():
    from astrild_amd import _lib
    assert (_lib.PAINT_TWO_PASS, _lib.PAINT_OVERWRITE, _lib.PAINT_DEFER_FOLD, _lib.PAINT_SCATTERED, _lib.PAINT_XSORTED) == \
        (TWO_PASS, OVERWRITE, DEFER_FOLD, SCATTERED, XSORTED)


# (method, accumulate, hint, whole, check_dropped, npart) -> (probe the caller runs, path without / before the probe)
NO_PROBE = [
    (("tiled2", False, None, True, True, NP), TP),
    (("tiled2", False, "scattered", True, True, NP), TP),
    (("tiled2", True, None, True, True, NP), TP),
    (("tiled", False, "clustered", True, True, NP), TP),
    (("tiled", True, None, True, True, NP), SP),
    (("tiled", True, "scattered", True, True, NP), SP),
    (("tiled", True, "xsorted", True, True, NP), SP),
    (("tiled", True, "ordered", True, True, NP), SP),
    (("tiled", False, "scattered", True, True, NP), SC),
    (("tiled", False, "scattered", False, False, 1000), SC),
    (("tiled", False, "xsorted", True, True, NP), SP),
    (("tiled", False, "ordered", True, True, NP), SP),
    (("tiled", False, None, True, True, (1 << 20) - 1), SP),
    (("tiled", False, None, True, False, (1 << 20) - 1), SP),
    (("tiled", False, None, False, True, (1 << 20) - 1), SP),
    (("tiled", False, None, False, False, NP), SP),
]


@pytest.mark.parametrize("args,path", NO_PROBE)
def test_first_path_without_a_probe(args, path):
    assert dev.paint_probe_kind(*args) is None
    assert dev.first_paint_path(*args) == path
    # whatever a probe might have said does not matter where none runs
    assert dev.first_paint_path(*args, probe(0.0, NP), True, 0) == path
    assert dev.first_paint_path(*args, probe(0.0, 0), True, NP) == path


# (dtype's limit, check_dropped, npart, probe_input's result) -> path
INPUT_PROBE = [
    (LIMIT64, True, NP, None, SP),
    (LIMIT64, False, NP, None, SP),
    (LIMIT64, True, NP, probe(0.1, 209715), SC),
    (LIMIT64, True, NP, probe(0.1, 209716), TP),
    (LIMIT32, True, NP, probe(0.1, 419430), SC),
    (LIMIT32, True, NP, probe(0.1, 419431), TP),
    (LIMIT32, False, NP, probe(0.1, 419430), SC),          # the probe runs and decides without check_dropped too
    (LIMIT32, False, NP, probe(0.1, 419431), TP),
    (LIMIT32, True, NP, probe(0.1, 0), SC),
    (LIMIT32, True, NP, probe(0.9, 32768), SP),
    (LIMIT32, True, NP, probe(0.9, 32769), TP),
    (LIMIT64, False, NP, probe(0.9, 32768), SP),
    (LIMIT64, False, NP, probe(0.9, 32769), TP),
    (LIMIT32, True, NP, probe(0.25, 0), SP),               # a quarter groupable counts as ordered
    (LIMIT32, True, NP, probe(0.25, 32769), TP),
    (LIMIT32, True, 1 << 20, probe(0.1, 16384), SC),       # the smallest probed paint
    (LIMIT32, True, 1 << 20, probe(0.9, 16385), TP),
]


@pytest.mark.parametrize("limit,check_dropped,npart,probed,path", INPUT_PROBE)
def test_first_path_from_the_input_probe(limit, check_dropped, npart, probed, path):
    args = ("tiled", False, None, True, check_dropped, npart)
    assert dev.paint_probe_kind(*args) == "input"
    assert dev.first_paint_path(*args, probed, None, limit if probed is not None else None) == path


@pytest.mark.parametrize("unordered,path", [(True, SC), (False, SP)])
def test_first_path_of_a_slab_buffer_from_the_order_probe(unordered, path):
    args = ("tiled", False, None, False, True, NP)
    assert dev.paint_probe_kind(*args) == "order"
    assert dev.first_paint_path(*args, None, unordered) == path
    # ... and without check_dropped nothing is probed and the order does not matter
    quiet = ("tiled", False, None, False, False, NP)
    assert dev.paint_probe_kind(*quiet) is None
    assert dev.first_paint_path(*quiet, None, unordered) == SP


def test_accumulate_never_scatters():
    for method, hint, whole, check_dropped in itertools.product(("tiled", "tiled2"), HINTS, (True, False), (True, False)):
        args = (method, True, hint, whole, check_dropped, NP)
        assert dev.paint_probe_kind(*args) is None
        path = dev.first_paint_path(*args, probe(0.0, 0), True, NP)
        assert path == (TP if method == "tiled2" or hint == "clustered" else SP)
        flags = dev.paint_flags(path, True, False, hint == "xsorted")
        assert flags == (TWO_PASS if path == TP else 0)
        assert dev.next_paint_path(path, False, whole, check_dropped, NP) is None


# (path, accumulate, defer_fold, xsorted) -> the AST_PAINT_* word
FLAGS = [
    ((SP, False, False, False), 2),
    ((SP, False, True, False), 2 | 4),
    ((SP, False, False, True), 2 | 16),
    ((SP, False, True, True), 2 | 4 | 16),
    ((SC, False, False, False), 2 | 8),
    ((SC, False, True, False), 2 | 4 | 8),
    ((SC, False, False, True), 2 | 8),                     # a climb from the XSORTED single pass has lost bit 16
    ((SC, False, True, True), 2 | 4 | 8),
    ((TP, False, False, False), 1 | 2),
    ((TP, False, True, False), 1 | 2 | 4),
    ((TP, False, False, True), 1 | 2),
    ((TP, False, True, True), 1 | 2 | 4),
    ((SP, True, False, False), 0),
    ((SP, True, False, True), 0),
    ((TP, True, False, False), 1),
    ((TP, True, False, True), 1),
]


@pytest.mark.parametrize("args,word", FLAGS)
def test_flag_word(args, word):
    assert dev.paint_flags(*args) == word


def test_scattered_accumulate_has_no_flag_word():
    with pytest.raises(AssertionError):
        dev.paint_flags(SC, True)
    with pytest.raises(AssertionError):
        dev.paint_flags("direct")


LIM = NP // 64                                             # 32768
# (path, probe gave a result, whole, check_dropped, overflow or None, dropped or None) -> next path
NEXT = [
    # R1: the overflow list, for callers that check
    ((SP, False, True, True, LIM, None), None),
    ((SP, False, True, True, LIM + 1, None), SC),
    ((SP, False, False, True, LIM + 1, None), SC),
    ((SP, True, True, True, LIM, None), None),
    ((SP, True, True, True, LIM + 1, None), SC),           # a probed single pass still climbs ...
    ((SC, True, True, True, LIM + 1, None), None),         # ... but not further: the probe had given a result
    ((SC, True, True, True, LIM + 1, 0), None),
    ((SC, False, True, True, LIM, None), None),
    ((SC, False, True, True, LIM + 1, None), TP),
    ((SC, False, False, True, LIM + 1, None), TP),
    ((SC, False, True, True, LIM + 1, 0), TP),             # R1 does not wait for the drop count
    ((SP, False, True, False, LIM + 1, None), None),       # statistics fetched for stats= only: never climbs by R1
    ((SP, True, True, False, NP, None), None),
    ((SC, False, True, False, LIM + 1, None), None),
    ((SC, False, False, False, NP, None), None),
    ((SP, False, True, True, None, None), None),           # nothing fetched
    ((SC, False, True, True, None, None), None),
    # R2: the late list, on the whole periodic grid, checked or not
    ((SC, False, True, True, 0, 0), None),
    ((SC, False, True, True, 0, 1), TP),
    ((SC, True, True, True, LIM + 1, 1), TP),
    ((SC, True, True, False, None, 0), None),
    ((SC, True, True, False, None, 1), TP),
    ((SC, False, True, False, LIM + 1, 1), TP),
    ((SC, False, False, True, 0, 1), None),                # a slab buffer: a drop there is a particle outside the buffer
    ((SC, False, False, False, None, 1), None),
    ((SP, False, True, True, 0, 1), None),                 # only the bucket scatter has a late list
    ((SP, True, True, False, None, 7), None),
    # the two-pass lists have no capacity: the attempt stands
    ((TP, False, True, True, None, None), None),
    ((TP, True, True, True, NP, NP), None),
    ((TP, False, False, False, NP, 1), None),
]


@pytest.mark.parametrize("args,path", NEXT)
def test_next_path(args, path):
    p, probed, whole, check_dropped, overflow, dropped = args
    assert dev.next_paint_path(p, probed, whole, check_dropped, NP, overflow, dropped) == path


def test_the_ladder_only_climbs_and_ends_after_three_attempts():
    rank = {SP: 0, SC: 1, TP: 2}
    for start, probed, whole, check_dropped in itertools.product((SP, SC, TP), (True, False), (True, False), (True, False)):
        for overflow, dropped in itertools.product((None, 0, LIM, LIM + 1, NP), (None, 0, 1, NP)):
            path, attempts = start, 1
            while True:
                nxt = dev.next_paint_path(path, probed, whole, check_dropped, NP, overflow, dropped)
                if nxt is None:
                    break
                assert rank[nxt] > rank[path]
                path, attempts = nxt, attempts + 1
            assert attempts <= 3 - rank[start]
    # the longest one: unordered and clustered input that nothing announced
    assert dev.next_paint_path(SP, False, True, True, NP, LIM + 1) == SC
    assert dev.next_paint_path(SC, False, True, True, NP, LIM + 1) == TP
    assert dev.next_paint_path(TP, False, True, True, NP) is None
