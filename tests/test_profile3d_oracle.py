"""CPU: the numpy oracle of the spherical profiles (tests/profile3d_oracle.py) against answers known by hand and
against the reference's literal expression, and the host-side planning and argument checks of
device.sphere_profiles, which need no GPU."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import profile3d_oracle as orc


def test_norm_is_bit_equal_to_the_oracles_expression():
    rng = np.random.default_rng(1)
    d = rng.normal(0.0, 3.0, (20000, 3))
    npt.assert_array_equal(np.linalg.norm(d, axis=1), orc.scaled_distance(d, 1.0))
    assert np.logspace(np.log10(0.05), 0, 21)[-1] == 1.0
    assert np.logspace(np.log10(0.05), np.log10(1), 21, base=10.0)[-1] == 1.0


@pytest.mark.parametrize("case", range(len(orc.LATTICE_CASES)))
def test_lattice_known_answers(case):
    centres, edges, expected = orc.LATTICE_CASES[case]
    pos = orc.unit_lattice(8)
    counts, moments, scale = orc.profiles(pos, centres, np.ones(len(centres)), edges, boxsize=8.0)
    for row in counts:
        assert row.tolist() == expected
    npt.assert_array_equal(moments[..., 0], counts)
    npt.assert_array_equal(scale, moments)


def test_lattice_scales_with_the_radius():
    """Edges are in units of each centre's radius: R = 0.5 with doubled edges counts the same shells."""
    centres, edges, expected = orc.LATTICE_CASES[0]
    counts, _, _ = orc.profiles(orc.unit_lattice(8), centres[:1], [0.5], 2.0 * np.asarray(edges), boxsize=8.0)
    assert counts[0].tolist() == expected


def test_oracle_equals_the_references_expression():
    """Open boundaries, one halo: np.histogram(np.linalg.norm(coords - c, axis=1) / r200, bins) and the reference's
    bin_value = counts * Mpart / bin_volumes."""
    rng = np.random.default_rng(2)
    c, r200 = np.array([10.0, 20.0, 30.0]), 1.7
    coords = c + rng.normal(0.0, 0.8, (5000, 3))
    bins = np.logspace(np.log10(0.05), np.log10(1), 21, base=10.0)
    ref = np.histogram(np.linalg.norm(coords - c, axis=1) / r200, bins=bins)[0]
    counts, moments, _ = orc.profiles(coords, [c], [r200], bins)
    npt.assert_array_equal(counts[0], ref)
    assert ref.sum() > 1000
    from astrild_amd.profiles.profile_3d import Profiles3D, bin_volumes
    radii, value = Profiles3D.from_particle_data(np.linalg.norm(coords - c, axis=1) / r200, 0, 2.5, "mass", 7)
    npt.assert_array_equal(value, ref * 2.5 / (4.0 / 3.0 * np.pi * (bins[1:] ** 3 - bins[:-1] ** 3)))
    npt.assert_array_equal(radii, 0.5 * (bins[1:] + bins[:-1]))
    npt.assert_array_equal(bin_volumes(bins), 4.0 / 3.0 * np.pi * (bins[1:] ** 3 - bins[:-1] ** 3))


def test_moments_by_hand():
    """Two particles on the x axis of a centre moving with (1, 0, 0): v_r, v_r^2 and |u|^2 by hand; a particle at the
    centre has v_r = 0 and counts in a first bin that starts at 0."""
    pos = np.array([[2.0, 0.0, 0.0], [0.0, 0.0, 0.0], [9.0, 0.0, 0.0], [0.0, 3.0, 0.0]])
    vel = np.array([[3.0, 1.0, 0.0], [5.0, 0.0, 0.0], [0.0, 0.0, 2.0], [1.0, -2.0, 0.0]])
    w = np.array([2.0, 1.0, 4.0, 0.5])
    counts, mom, scale = orc.profiles(pos, [[0.0, 0.0, 0.0]], [2.0], [0.0, 1.0, 2.0], boxsize=10.0, weights=w, vel=vel,
                                      centre_vel=[[1.0, 0.0, 0.0]])
    # x = 1 (bin 1), 0 (bin 0), 0.5 through the face (s = -1, bin 0), 1.5 (bin 1)
    assert counts.tolist() == [[2, 2]]
    # bin 0: centre particle u = (4, 0, 0), v_r = 0; wrapped particle u = (-1, 0, 2), s = (-1, 0, 0), v_r = 1
    npt.assert_array_equal(mom[0, 0], [5.0, 4.0, 4.0, 1.0 * 16.0 + 4.0 * 5.0])
    # bin 1: u = (2, 1, 0), s = (2, 0, 0), v_r = 2; u = (0, -2, 0), s = (0, 3, 0), v_r = -2
    npt.assert_array_equal(mom[0, 1], [2.5, 4.0 - 1.0, 8.0 + 2.0, 2.0 * 5.0 + 0.5 * 4.0])
    npt.assert_array_equal(scale[0, 1], [2.5, 5.0, 10.0, 12.0])


def test_segments_restrict_the_particles():
    pos = orc.unit_lattice(4)
    seg = [(0, 0), (5, 40), (60, 4)]
    counts, _, _ = orc.profiles(pos, [[1.0, 1.0, 1.0]] * 3, [1.0] * 3, [0.0, 1.5, 4.0], segments=seg)
    assert counts.sum(axis=1).tolist() == [0, 40, 4]


# ---------------------------------------------------------------- host-side planning of device.sphere_profiles
def test_grid_dims_are_a_pure_function_of_count_and_cap():
    from astrild_amd import device as dev
    assert dev.profile3d_dims(0) == 1 and dev.profile3d_dims(1) == 1 and dev.profile3d_dims(31) == 1
    assert dev.profile3d_dims(32) == 2 and dev.profile3d_dims(4 * 27 - 1) == 2 and dev.profile3d_dims(4 * 27) == 3
    assert dev.profile3d_dims(10 ** 7) == 128 and dev.profile3d_dims(10 ** 7, cell_cap=1 << 24) == 135
    assert [dev.profile3d_dims(20000, cell_cap=c) for c in (26, 27, 63, 64, 125, 10 ** 9)] == [2, 3, 3, 4, 5, 17]
    with pytest.raises(ValueError):
        dev.profile3d_dims(100, cell_cap=0)


def test_axis_range_covers_the_cells_of_every_particle_in_reach():
    """Brute force on one axis: every particle within `reach` of a centre (periodic distance) lies in a cell of the
    centre's range, the range never repeats a cell, and it never exceeds dims."""
    from astrild_amd import device as dev
    rng = np.random.default_rng(4)
    L = 100.0
    x = np.concatenate([rng.uniform(0.0, L, 2000), [0.0, L, np.nextafter(L, 0.0), 50.0]])
    c = np.concatenate([rng.uniform(0.0, L, 40), [0.0, L, 25.0, 75.0]])
    for dims in (1, 2, 3, 4, 5, 17):
        inv = dims / L if dims > 1 else 0.0
        cell = np.clip(np.floor(x * inv), 0, dims - 1).astype(int)
        for reach in (0.0, 1.0, 12.5, 25.0, 49.0):
            first, n = dev._profile3d_axis_range(c, np.full(len(c), reach * (1 + 1e-9) + 1e-12 * L), 0.0, inv, dims, True)
            assert np.all((n >= 1) & (n <= dims) & (first >= 0) & (first < dims))
            for i in range(len(c)):
                d = np.abs(x - c[i])
                near = np.minimum(d, L - d) <= reach
                assert np.all((cell[near] - first[i]) % dims < n[i])
    # open boundaries: clamped, empty when the reach misses the grid
    first, n = dev._profile3d_axis_range(np.array([-50.0, 5.0, 95.0, 200.0]), np.full(4, 10.0), 0.0, 0.04, 4, False)
    assert first.tolist() == [0, 0, 3, 0] and n.tolist() == [0, 1, 1, 0]


def test_argument_checks_need_no_gpu():
    from astrild_amd import device as dev
    ok = dict(pos_shape=(10, 3), centres=np.zeros((2, 3)), radii=[1.0, 2.0], edges=[0.0, 1.0, 2.0], boxsize=10.0)
    c, r, e, cv, seg = dev.check_profile3d_args(**ok)
    assert c.dtype == r.dtype == e.dtype == np.float64 and cv is None and seg is None
    bad = [dict(pos_shape=(10, 2)), dict(pos_shape=(10,)), dict(weights_shape=(9,)), dict(vel_shape=(10, 2)),
           dict(edges=[1.0]), dict(edges=[0.0, 1.0, 1.0]), dict(edges=[-0.1, 1.0]), dict(edges=[0.0, np.inf]),
           dict(edges=np.arange(300.0)), dict(centres=np.zeros((2, 2))), dict(centres=np.full((2, 3), np.nan)),
           dict(radii=[1.0]), dict(radii=[1.0, 0.0]), dict(radii=[1.0, -1.0]), dict(radii=[1.0, np.inf]),
           dict(radii=[1.0, np.nan]), dict(centre_vel=np.zeros((2, 3))), dict(vel_shape=(10, 3), centre_vel=np.zeros((3, 3))),
           dict(boxsize=0.0), dict(boxsize=np.inf), dict(radii=[1.0, 2.5]), dict(centres=np.full((2, 3), 10.5)),
           dict(centres=np.full((2, 3), -0.5)), dict(segments=[(0, 5)]), dict(segments=[(0, 5), (6, 5)]),
           dict(segments=[(0, 5), (-1, 2)]), dict(segments=[(0.0, 5.0), (1.0, 2.0)]), dict(segments=[(0, 5), (11, 0)])]
    for change in bad:
        with pytest.raises(ValueError):
            dev.check_profile3d_args(**{**ok, **change})
    # the reach bound holds only in a periodic box; the largest allowed reach is just below boxsize / 2
    dev.check_profile3d_args(**{**ok, "boxsize": None, "radii": [1.0, 50.0], "centres": np.full((2, 3), -7.0)})
    dev.check_profile3d_args(**{**ok, "radii": [1.0, np.nextafter(2.5, 0.0)]})
    dev.check_profile3d_args(**{**ok, "segments": [(0, 10), (10, 0)], "vel_shape": (10, 3), "centre_vel": np.ones((2, 3))})
