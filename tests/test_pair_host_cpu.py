"""The host checks that the pair finders of astrild_amd.device share (_pair_sample, _check_edges, _positive_real,
_check_device_bounds) and the messages that the public functions raise through them, without a GPU: no library call
but the host-only limit getters (ast_tpcf_max_bins in check_tpcf_edges, ast_pairwise_max_bins in pairwise_tv)."""
import numpy as np
import pytest
import torch

from astrild_amd import device as dev

INF = np.inf


# ---------------------------------------------------------------- edges
@pytest.mark.parametrize("edges", [[1.0], [0.0, 1.0, 1.0], [2.0, 1.0], [0.0, INF], [0.0, np.nan, 2.0], [-1.0, 1.0]])
def test_bad_edges_name_their_noun(edges):
    with pytest.raises(ValueError, match="^s edges must be at least two finite, non-negative, strictly increasing"):
        dev._check_edges(edges, "s edge")
    with pytest.raises(ValueError, match="^s edges must be"):
        dev.check_tpcf_edges(edges, None, 100.0)
    with pytest.raises(ValueError, match="^bin edges must be at least two finite, non-negative, strictly increasing"):
        dev.check_pair_velocity_args((4, 3), (4, 3), edges)


def test_edges_come_back_as_flat_fp64():
    e = dev._check_edges(np.array([[0, 1], [2, 3]], dtype=np.int32), "bin edge")
    assert e.dtype == np.float64 and e.tolist() == [0.0, 1.0, 2.0, 3.0]
    assert dev._check_edges([0.0, 1e9], "s edge").tolist() == [0.0, 1e9]       # no top: open boundaries


def test_top_edge_against_a_third_of_the_box():
    third = 30.0 / 3.0
    assert dev._check_edges([0.0, np.nextafter(third, 0.0)], "s edge", top=third)[-1] < third
    with pytest.raises(ValueError, match=r"^the largest s edge \(10\.0\) must be below boxsize / 3 \(10\.0\)$"):
        dev.check_tpcf_edges([0.0, 10.0], None, 30.0)
    with pytest.raises(ValueError, match=r"^the largest bin edge \(10\.0\) must be below boxsize / 3 \(10\.0\)$"):
        dev.check_pair_velocity_args((4, 3), (4, 3), [0.0, 10.0], boxsize=30.0)
    assert dev.check_tpcf_edges([0.0, 10.0], None, None, periodic=False)[0][-1] == 10.0


def test_bin_limit_comes_before_the_top_edge():
    with pytest.raises(ValueError, match="^4 bins: at most 3$"):
        dev._check_edges(np.arange(5.0), "bin edge", top=1.0, max_bins=3)
    assert len(dev._check_edges(np.arange(4.0), "bin edge", max_bins=3)) == 4


# ---------------------------------------------------------------- positive, finite real numbers
@pytest.mark.parametrize("bad", [0.0, -1, INF, np.nan, None, "1.0", b"1", [1.0, 2.0], 1j])
def test_positive_real_refuses(bad):
    with pytest.raises(ValueError, match="^pi_max must be a positive, finite real number, got ") as err:
        dev._positive_real("pi_max", bad)
    assert str(err.value).endswith(f"got {bad!r}")
    with pytest.raises(ValueError, match="^pi_max must be a positive, finite real number"):
        dev.check_pair_velocity_args((4, 3), (4, 3), [0.0, 1.0], kind="los", pi_max=bad)


def test_positive_real_returns_the_float():
    for good in (2, 2.5, np.float32(0.5), np.int64(3), True):
        x = dev._positive_real("r", good)
        assert type(x) is float and x == float(good)


@pytest.mark.parametrize("name", ["r", "dist_width", "vel_width"])
@pytest.mark.parametrize("bad, shown", [(-1, "-1.0"), ("abc", "nan"), (None, "nan"), (INF, "inf")])
def test_pairwise_pdf_names_the_argument_and_echoes_the_float(name, bad, shown):
    args = dict(r=1.0, dist_width=1.0, vel_width=1.0)
    args[name] = bad
    with pytest.raises(ValueError, match=f"^{name} must be a positive, finite real number, got {shown}$"):
        dev.check_pairwise_pdf_args((4, 3), (4, 3), args["r"], 2, 2, "radial", args["dist_width"], args["vel_width"],
                                    0, None, False)


# ---------------------------------------------------------------- device bounds
L = 100.0
INSIDE = [0.0, 0.0, 0.0, L, L, L]                       # the periodic edge values themselves are allowed
EMPTY = [INF, INF, INF, -INF, -INF, -INF]               # what a prepare call returns for an empty sample


def test_bounds_inside_pass():
    dev._check_device_bounds(np.array(INSIDE), (5,), L)
    dev._check_device_bounds(np.array(INSIDE + INSIDE), (5, 7), L)
    dev._check_device_bounds(np.array(INSIDE), (5,), L, shifted=True)
    dev._check_device_bounds(np.array([-1e300, 0.0, 0.0, 1e300, 0.0, 0.0] * 2), (5, 7), 0.0, periodic=False)


def test_an_empty_sample_is_skipped():
    dev._check_device_bounds(np.array(EMPTY), (0,), L)
    dev._check_device_bounds(np.array(INSIDE + EMPTY), (5, 0), L)
    dev._check_device_bounds(np.array(EMPTY + INSIDE), (0, 5), 0.0, periodic=False)
    out = [-1.0] + INSIDE[1:]
    dev._check_device_bounds(np.array(out + INSIDE), (0, 5), L)        # stale bounds of a sample without objects


@pytest.mark.parametrize("axis", range(3))
def test_just_outside_the_periodic_box_is_refused(axis):
    low, high = list(INSIDE), list(INSIDE)
    low[axis] = np.nextafter(0.0, -1.0)
    high[3 + axis] = np.nextafter(L, INF)
    for b in (low, high):
        with pytest.raises(ValueError, match=r"^positions must lie in \[0, 100\.0\]: min \[.*\], max \[.*\]$"):
            dev._check_device_bounds(np.array(b), (5,), L)
        with pytest.raises(ValueError,
                           match=r"^positions \(after the redshift-space shift\) must lie in \[0, 100\.0\]: min "):
            dev._check_device_bounds(np.array(b), (5,), L, shifted=True)
        with pytest.raises(ValueError, match=r"^positions of sample 1 must lie in \[0, 100\.0\]: min "):
            dev._check_device_bounds(np.array(b + INSIDE), (5, 7), L)
        with pytest.raises(ValueError,
                           match=r"^positions of sample 2 \(after the redshift-space shift\) must lie in \[0, 100\.0\]"):
            dev._check_device_bounds(np.array(INSIDE + b), (5, 7), L, shifted=True)


def test_the_message_quotes_the_bounds():
    b = [-0.5, 1.0, 2.0, 3.0, 4.0, 5.0]
    with pytest.raises(ValueError) as err:
        dev._check_device_bounds(np.array(INSIDE + b), (5, 7), L)
    assert str(err.value) == ("positions of sample 2 must lie in [0, 100.0]: "
                              "min [-0.5, 1.0, 2.0], max [3.0, 4.0, 5.0]")


def test_a_nan_coordinate_is_refused_either_way():
    nan_bounds = [-INF, 0.0, 0.0, INF, 1.0, 1.0]        # a prep kernel counts a NaN as -inf and +inf
    with pytest.raises(ValueError, match="must lie in"):
        dev._check_device_bounds(np.array(nan_bounds), (5,), L)
    with pytest.raises(ValueError, match="^positions of sample 1 must be finite: min "):
        dev._check_device_bounds(np.array(nan_bounds + INSIDE), (5, 7), 0.0, periodic=False)


@pytest.mark.parametrize("slot, value", [(0, -INF), (5, INF)])
def test_open_boundaries_refuse_infinities(slot, value):
    b = list(INSIDE)
    b[slot] = value
    with pytest.raises(ValueError, match=r"^positions of sample 2 \(after the redshift-space shift\) must be finite: "):
        dev._check_device_bounds(np.array(INSIDE + b), (5, 7), 0.0, periodic=False, shifted=True)
    with pytest.raises(ValueError, match="^positions of sample 1 must be finite: min "):
        dev._check_device_bounds(np.array(b + INSIDE), (5, 7), 0.0, periodic=False)


# ---------------------------------------------------------------- los: a recorded difference
class Reached(Exception):
    pass


def test_tpcf_takes_whatever_equals_an_axis(monkeypatch):
    """The TPCF functions test ``los not in (0, 1, 2)``: True, 1.0 and numpy integers pass as the axis they equal."""
    def reached(*a, **k):
        raise Reached
    monkeypatch.setattr(dev, "_pair_sample", reached)
    pos = np.zeros((4, 3))
    for los in (0, 1, 2, True, False, 1.0, np.int64(2)):
        with pytest.raises(Reached):
            dev.tpcf_pair_counts(pos, L, [0.0, 1.0], los=los)
        with pytest.raises(Reached):
            dev.tpcf_cross_counts(pos, pos, [0.0, 1.0], boxsize=L, los=los)
    for los in (3, -1, 1.5, None, "2"):
        with pytest.raises(ValueError, match=f"^los must be 0, 1 or 2, got {los}$"):
            dev.tpcf_pair_counts(pos, L, [0.0, 1.0], los=los)
        with pytest.raises(ValueError, match=f"^los must be 0, 1 or 2, got {los}$"):
            dev.tpcf_cross_counts(pos, None, [0.0, 1.0], los=los)


def test_pair_velocity_refuses_a_bool_axis():
    """check_pair_velocity_args refuses bool, and otherwise takes what equals an axis."""
    for los in (0, 1, 2, 1.0, np.int64(2)):
        dev.check_pair_velocity_args((4, 3), (4, 3), [0.0, 1.0], los=los)
    for los in (True, False, 3, -1, 1.5, None, "2"):
        with pytest.raises(ValueError, match="^los must be 0, 1 or 2, got "):
            dev.check_pair_velocity_args((4, 3), (4, 3), [0.0, 1.0], los=los)


# ---------------------------------------------------------------- one sample
@pytest.fixture
def on_cpu(monkeypatch):
    monkeypatch.setattr(dev, "as_device", lambda a, dtype=None: a if isinstance(a, torch.Tensor) else torch.as_tensor(a))


POS_MSG, VEL_MSG = "pos must be (N, 3), got {p}", "vel must be (N, 3) like pos, got {v}"


def test_sample_dtypes(on_cpu):
    p, v, n = dev._pair_sample(np.arange(12).reshape(4, 3), None, POS_MSG, VEL_MSG)
    assert (p.dtype, v, n) == (torch.float64, None, 4) and p.tolist() == np.arange(12.0).reshape(4, 3).tolist()
    p, v, n = dev._pair_sample(np.zeros((4, 3), np.float32), torch.zeros((4, 3), dtype=torch.float16), POS_MSG, VEL_MSG)
    assert (p.dtype, v.dtype, n) == (torch.float32, torch.float64, 4)
    p, v, n = dev._pair_sample(torch.zeros((0, 3), dtype=torch.float64), np.zeros((0, 3), np.float32), POS_MSG, VEL_MSG)
    assert (p.dtype, v.dtype, n) == (torch.float64, torch.float32, 0)


@pytest.mark.parametrize("pos", [np.zeros(12), np.zeros((4, 2)), np.zeros((4, 3, 1)), np.zeros(())])
def test_sample_refuses_positions(on_cpu, pos):
    with pytest.raises(ValueError, match=r"^pos must be \(N, 3\), got \(") as err:
        dev._pair_sample(pos, None, POS_MSG, VEL_MSG)
    assert str(err.value).endswith(str(tuple(torch.as_tensor(pos).shape)))


@pytest.mark.parametrize("vel", [np.zeros(12), np.zeros((4, 2)), np.zeros((5, 3)), np.zeros((4, 4))])
def test_sample_refuses_velocities(on_cpu, vel):
    with pytest.raises(ValueError, match=r"^vel must be \(N, 3\) like pos, got \("):
        dev._pair_sample(np.zeros((4, 3)), vel, POS_MSG, VEL_MSG)


def test_sample_widths(on_cpu):
    both = "got {p} and {v}"
    for w in (2, 3):
        assert dev._pair_sample(np.zeros((4, 3)), np.zeros((4, w)), both, both, widths=(2, 3))[1].shape == (4, w)
    with pytest.raises(ValueError, match=r"^got \(4, 3\) and \(4, 1\)$"):
        dev._pair_sample(np.zeros((4, 3)), np.zeros((4, 1)), both, both, widths=(2, 3))
    with pytest.raises(ValueError, match=r"^got \(4, 2\) and \(4, 2\)$"):
        dev._pair_sample(np.zeros((4, 2)), np.zeros((4, 2)), both, both, widths=(2, 3))


def test_the_public_functions_word_their_shape_errors(on_cpu):
    good, flat, two = np.zeros((4, 3)), np.zeros(12), np.zeros((4, 2))
    with pytest.raises(ValueError, match=r"^pos must be \(N, 3\), got \(12,\)$"):
        dev.tpcf_pair_counts(flat, L, [0.0, 1.0])
    with pytest.raises(ValueError, match=r"^vel must be \(N, 3\) like pos, got \(4, 2\)$"):
        dev.tpcf_pair_counts(good, L, [0.0, 1.0], vel=two)
    with pytest.raises(ValueError, match=r"^pos1 must be \(N, 3\), got \(4, 2\)$"):
        dev.tpcf_cross_counts(two, good, [0.0, 1.0])
    with pytest.raises(ValueError, match=r"^pos2 must be \(N, 3\), got \(12,\)$"):
        dev.tpcf_cross_counts(good, flat, [0.0, 1.0])
    with pytest.raises(ValueError, match=r"^the velocities of pos2 must be \(N, 3\) like it, got \(4, 2\)$"):
        dev.tpcf_cross_counts(good, good, [0.0, 1.0], vel2=two)
    with pytest.raises(ValueError, match="^vel2 given without pos2$"):
        dev.tpcf_cross_counts(good, None, [0.0, 1.0], vel2=good)
    with pytest.raises(ValueError,
                       match=r"^pos must be \(N, 3\) and velocities \(N, 2\) or \(N, 3\), got \(4, 2\) and \(4, 2\)$"):
        dev.pairwise_tv(two, two, 4, 1.0)
    with pytest.raises(ValueError, match=r"velocities \(N, 2\) or \(N, 3\), got \(4, 3\) and \(4, 4\)$"):
        dev.pairwise_tv(good, np.zeros((4, 4)), 4, 1.0)
    with pytest.raises(ValueError, match=r"^positions and velocities of sample 2 must both be \(N, 3\), got "):
        dev.check_pair_velocity_args((4, 3), (4, 3), [0.0, 1.0], pos2_shape=(4, 2), vel2_shape=(4, 2))
    with pytest.raises(ValueError, match=r"^positions and velocities of sample 1 must both be \(N, 3\), got "):
        dev.check_pair_velocity_args((12,), (12,), [0.0, 1.0])
