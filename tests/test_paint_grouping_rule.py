"""The numpy restatement of the paint's grouping rule (tests/paint_grouping_rule.py) on the hand-made windows, against
the counts worked out by hand.  tests/test_gpu_paint_grouping.py holds the kernel to the same restatement."""
import numpy as np
import pytest

from tests import paint_grouping_rule as rule


@pytest.mark.parametrize("name", list(rule.PATTERNS))
def test_window_rule_on_the_hand_made_windows(name):
    labels, want = rule.PATTERNS[name]
    assert rule.window_rule(labels) == want
    # a record takes its members off the stray list: records * MINPOP <= 32 - strays
    assert want[0] * rule.MINPOP <= 32 - want[1]


def test_dead_lanes_are_neither_members_nor_strays():
    keys = np.full(32, -1)
    assert rule.window_rule(keys) == (0, 0)
    keys[:9] = 5                                   # nine particles of one tile, lane 8 among them
    assert rule.window_rule(keys) == (1, 0)
    keys[8] = -1                                   # the candidate lane is dead: eight strays
    assert rule.window_rule(keys) == (0, 8)


def test_a_candidate_taken_earlier_takes_nothing():
    keys = np.array([1] * 16 + [2] * 16)           # lanes 16 and 24 share a tile, lane 8 has the other
    assert rule.window_rule(keys) == (2, 0)


def test_count_lists_pads_the_last_window():
    keys = np.zeros(40, dtype=np.int64)            # 32 + 8: lane 16 of the second window is past the end
    assert rule.count_lists(keys) == (1, 8)
    assert rule.count_lists(np.zeros(32 + 17, dtype=np.int64)) == (2, 0)


def test_interval_is_one_interval_with_every_pattern_in_both_halves():
    names = rule.interval_windows()
    assert len(names) == 128
    for p in rule.PATTERNS:
        assert {i % 2 for i, nm in enumerate(names) if nm == p} == {0, 1}
