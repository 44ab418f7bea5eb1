"""Without a GPU: the friends-of-friends oracle (tests/fof_oracle.py) on hand-worked cases and against scipy's connected
components, and every ValueError of the definition from the host-only check functions of
astrild_amd/particles/hutils/fof.py."""
import numpy as np
import pytest

from tests import fof_oracle as orc


def test_three_points_in_a_row():
    """0 - 1 are friends, 1 - 2 are friends, 0 - 2 are not: one group through the middle point, two links."""
    pos = np.array([[1.0, 5.0, 5.0], [2.0, 5.0, 5.0], [3.0, 5.0, 5.0], [7.0, 5.0, 5.0]])
    g = orc.groups(pos, 1.5, boxsize=10.0, nmin=1)
    assert g["links"] == 2 and g["ncomponents"] == 2
    assert g["labels"].tolist() == [1, 1, 1, 2] and g["length"].tolist() == [3, 1] and g["first"].tolist() == [0, 3]
    assert g["members"].tolist() == [0, 1, 2, 3] and g["offsets"].tolist() == [0, 3, 4]
    assert g["labels"].dtype == np.int32 and g["members"].dtype == np.int32 and g["offsets"].dtype == np.int64
    assert orc.groups(pos, 1.5, boxsize=10.0, nmin=2)["labels"].tolist() == [1, 1, 1, 0]


def test_a_pair_at_exactly_b_and_at_distance_zero():
    pos = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0], [3.0, 4.0, 0.0]])         # d(0, 1) = 5 exactly, d(1, 2) = 0
    assert orc.groups(pos, 5.0)["links"] == 3 and orc.groups(pos, 5.0)["labels"].tolist() == [1, 1, 1]
    below = orc.groups(pos, np.nextafter(5.0, 0.0))
    assert below["links"] == 1 and below["labels"].tolist() == [2, 1, 1] and below["first"].tolist() == [1, 0]


def test_periodic_minimum_image_and_cylinder():
    pos = np.array([[0.5, 5.0, 5.0], [9.6, 5.0, 5.0], [9.6, 5.0, 7.0]])
    assert orc.groups(pos, 1.0, boxsize=10.0)["labels"].tolist() == [1, 1, 2]     # 0 - 1 across the face: 0.9
    assert orc.groups(pos, 1.0)["labels"].tolist() == [1, 2, 3]
    assert orc.groups(pos, 0.5, boxsize=10.0, b_para=2.0, los=2)["labels"].tolist() == [2, 1, 1]  # 1 - 2: rp 0, pi 2
    assert orc.groups(pos, 0.5, boxsize=10.0, b_para=2.0, los=0)["labels"].tolist() == [1, 1, 2]  # 0 - 1: rp 0, pi .9


def test_a_tie_in_size_goes_to_the_smaller_first_index():
    pos = np.array([[8.0, 0, 0], [1.0, 0, 0], [8.5, 0, 0], [1.5, 0, 0], [4.0, 0, 0], [4.2, 0, 0], [4.4, 0, 0]])
    g = orc.groups(pos, 0.6, nmin=2)
    assert g["length"].tolist() == [3, 2, 2] and g["first"].tolist() == [4, 0, 1]
    assert g["labels"].tolist() == [2, 3, 2, 3, 1, 1, 1]
    assert g["members"].tolist() == [4, 5, 6, 0, 2, 1, 3] and g["offsets"].tolist() == [0, 3, 5, 7]


def test_components_equal_scipy_connected_components():
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    rng = np.random.default_rng(5)
    pos = rng.uniform(0.0, 20.0, (1500, 3))
    for box, b_para in ((20.0, None), (None, None), (20.0, 2.5)):
        i, j, _ = orc.friend_pairs(pos, 1.2, box, b_para, los=1)
        assert len(i) > 500
        root = orc.components(len(pos), i, j)
        adj = sparse.coo_matrix((np.ones(len(i)), (i, j)), shape=(len(pos),) * 2)
        ncomp, lab = connected_components(adj, directed=False)
        assert ncomp == len(np.unique(root)) and 1 < ncomp < len(pos)
        smallest = np.full(ncomp, len(pos))
        np.minimum.at(smallest, lab, np.arange(len(pos)))
        assert np.array_equal(root, smallest[lab])


def test_feature_oracle_on_a_group_across_a_face():
    pos = np.array([[9.5, 1.0, 1.0], [0.5, 1.0, 1.0], [9.0, 1.0, 1.0]])
    g = orc.groups(pos, 1.1, boxsize=10.0)
    f = orc.features(pos, g, boxsize=10.0, vel=pos * 2.0, weights=np.array([1.0, 2.0, 1.0]))
    assert g["length"].tolist() == [3]
    np.testing.assert_allclose(f["cm_position"], [[9.875, 1.0, 1.0]], rtol=0, atol=1e-15)      # 9.5 + (2 - 0.5) / 4
    np.testing.assert_allclose(f["cm_velocity"], [[(19.0 + 2.0 + 18.0) / 4.0, 2.0, 2.0]], rtol=1e-15)
    assert f["weight"].tolist() == [4.0]
    assert orc.features(pos, g, boxsize=10.0)["cm_position"][0, 0] == pytest.approx(29.0 / 3.0, abs=1e-14)


def test_argument_errors_are_raised_on_the_host():
    from astrild_amd.particles.hutils import fof
    pos = np.zeros((10, 3))
    ok = fof.check_fof_args(pos, 1.0, boxsize=10.0, nmin=2, b_para=2.0, los=1)
    assert ok[1:] == (1.0, 2.0, 10.0) and fof.check_fof_args(pos.astype(np.float32), 1.0)[2:] == (None, 0.0)
    bad = [dict(pos=np.zeros((10, 2))), dict(pos=np.zeros(30)), dict(pos=np.zeros((10, 3), dtype=np.int64)),
           dict(pos=np.zeros((10, 3), dtype=np.float16)),
           dict(linking_length=0.0), dict(linking_length=-1.0), dict(linking_length=np.inf), dict(linking_length=np.nan),
           dict(linking_length=None), dict(linking_length="1"),
           dict(b_para=0.0), dict(b_para=np.inf), dict(boxsize=0.0), dict(boxsize=np.nan),
           dict(linking_length=10.0 / 3.0, boxsize=10.0), dict(linking_length=1.0, b_para=10.0 / 3.0, boxsize=10.0),
           dict(linking_length=3.4, b_para=1.0, boxsize=10.0),
           dict(nmin=0), dict(nmin=-3), dict(nmin=1.5), dict(los=3), dict(los=-1), dict(los=None)]
    for kw in bad:
        args = dict(pos=pos, linking_length=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            fof.check_fof_args(**args)
        with pytest.raises(ValueError):                     # fof_groups checks before it touches the library or a GPU
            fof.fof_groups(**args)
    fof.check_fof_args(pos, 3.3, boxsize=10.0)              # just below L / 3; open boundaries: no such rule
    fof.check_fof_args(pos, 50.0)
    for kw in (dict(vel=np.zeros((9, 3))), dict(vel=np.zeros((10, 3), dtype=np.int32)), dict(weights=np.zeros((10, 1))),
               dict(boxsize=-1.0)):
        with pytest.raises(ValueError):
            fof.check_fof_feature_args(pos, **kw)
    with pytest.raises(ValueError):
        fof.FOF(pos, 0.2, 5)                                # a relative length without a box
    with pytest.raises(ValueError):
        fof.FOF(pos, 0.2, 5, absolute=True)                 # periodic without a box
    with pytest.raises(ValueError):
        fof.FoFGroups(pos, 0.14, 0.75)
    with pytest.raises(ValueError):
        fof.FoFGroups(pos, 0.14, 0.75, period=[10.0, 10.0, 20.0])


def test_the_clustered_catalogue_has_the_structure_the_gpu_tests_rely_on():
    """12 groups with a tie in size, a group across two periodic faces that open boundaries split, under the plan of one
    cell per object (AST_FOF_CELL_OBJECTS=1) 18^3 cells of which one holds more than two tiles of 256, and no pair so
    close to the linking length that float32 input could matter."""
    L, n = 100.0, 6000
    pos = orc.clustered(L, n)
    assert pos.shape == (n, 3) and (pos >= 0).all() and (pos < L).all()
    b = 0.2 * (L ** 3 / n) ** (1.0 / 3.0)
    g = orc.groups(pos, b, boxsize=L, nmin=20)
    assert g["length"].tolist() == [700, 499, 151] + [150] * 9 and g["links"] == 345050
    assert int((g["labels"] == 0).sum()) == 3300 and g["ncomponents"] == 3273 and g["margin"] > 6e-6
    dims = int(np.floor(L / (b * (1.0 + 1e-6))))            # grid_periodic_plan: 90 cells per axis for the reach,
    while dims ** 3 > n:                                    # fewer while the cube exceeds the cap of n cells
        dims -= 1
    assert dims == 18
    cells = np.minimum((pos * (dims / L)).astype(np.int64), dims - 1)
    assert np.unique(cells @ np.array([1, dims, dims * dims]), return_counts=True)[1].max() == 701
    open_ = orc.groups(pos, b, nmin=20)
    assert open_["length"].tolist()[:2] == [700, 228] and len(open_["length"]) == 15
