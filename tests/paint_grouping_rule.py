"""The grouping rule of the tiled paint's single pass (``tile_group_kernel``), restated in numpy, and the hand-made
32-particle windows the GPU test paints.

A window is 32 particles that are consecutive in memory, aligned to 32 in the particle ids.  The tiles of three fixed
lanes - 16, 8, 24, in this order - are its candidates.  A candidate takes the particles of its tile that no earlier
candidate took; with MINPOP takers or more they become one group record, with fewer they stay strays.  Whatever no
candidate took is a stray as well.  (The kernel stops early once fewer than MINPOP particles are pending: no later
candidate could reach MINPOP, so the outcome is the same.)
"""
import numpy as np

MINPOP = 8
CANDIDATES = (16, 8, 24)


def window_rule(keys):
    """keys: the 32 tile ids of a window (negative: no particle).  Returns (records, strays)."""
    keys = np.asarray(keys)
    assert keys.shape == (32,)
    live = keys >= 0
    pending, member, records = live.copy(), np.zeros(32, bool), 0
    for c in CANDIDATES:
        match = pending & (keys == keys[c])
        if match.sum() >= MINPOP:
            records += 1
            member |= match
        pending &= ~match
    return records, int((live & ~member).sum())


def count_lists(keys):
    """keys: tile ids of all particles in memory order.  Returns (records, strays) summed over the windows."""
    keys = np.asarray(keys, dtype=np.int64)
    pad = (-len(keys)) % 32
    k = np.concatenate([keys, np.full(pad, -1)]).reshape(-1, 32)
    got = np.array([window_rule(w) for w in k])
    return int(got[:, 0].sum()), int(got[:, 1].sum())


def _labels(*runs):
    """Label per lane from (label, lanes) runs; a label of -1 gives every lane a tile of its own."""
    out = np.empty(32, dtype=np.int64)
    nxt = 100
    for label, lanes in runs:
        for lane in lanes:
            out[lane] = label if label >= 0 else nxt
            nxt += 1
    return out


R = range
#: name -> (label per lane, (records, strays) by hand).  Equal labels share a tile, different labels never do.
PATTERNS = {
    "32": (_labels((0, R(32))), (1, 0)),
    "24-8": (_labels((0, R(24)), (1, R(24, 32))), (2, 0)),
    "25-7": (_labels((0, R(25)), (1, R(25, 32))), (1, 7)),
    "8-8-8-8": (_labels((0, R(8)), (1, R(8, 16)), (2, R(16, 24)), (3, R(24, 32))), (3, 8)),
    "10-10-10-2": (_labels((0, R(10)), (1, R(10, 20)), (2, R(20, 30)), (3, R(30, 32))), (3, 2)),
    "7-7-7-7-4": (_labels((0, R(7)), (1, R(7, 14)), (2, R(14, 21)), (3, R(21, 28)), (4, R(28, 32))), (0, 32)),
    # eleven takers, none of them a candidate lane: never looked at
    "no-candidate": (_labels((0, list(R(8)) + [9, 10, 11]), (-1, [8] + list(R(12, 32)))), (0, 32)),
    # the three candidates in one tile: the first settles it, the singletons stay strays
    "29-1-1-1": (_labels((1, [0]), (2, [1]), (3, [2]), (0, R(3, 32))), (1, 3)),
    "one-tile": (_labels((0, R(32))), (1, 0)),
    "all-distinct": (_labels((-1, R(32))), (0, 32)),
}
FILLERS = ("one-tile", "all-distinct")


def interval_windows():
    """Names of the 128 windows of one 4096-particle interval: every pattern as the lower and as the upper window of its
    wave, beside either filler (so a half with one tile sits beside a half with 32, both ways round), twice."""
    names = []
    for p in PATTERNS:
        for f in FILLERS:
            names += [p, f, f, p]
    names = names + names
    while len(names) < 128:
        names += list(FILLERS)
    return names[:128]
