"""Without a GPU: the catalogues, planners and forests of tests/fof_cases.py do what they claim, every known answer
equals the brute-force oracle (tests/fof_oracle.py), and each kind of assertion that tests/test_gpu_fof_edges.py makes
can fail: a walk without the periodic wrap, `pi < b_para`, a cell cap of n, and planners without margin or with another
growth give other results on these catalogues."""
import numpy as np
import pytest

from tests import fof_cases as fc
from tests import fof_oracle as orc
from tests import pair_geometry as pg

KEYS = ("labels", "length", "first", "members", "offsets", "links")


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS)


# ------------------------------------------------------------------ 1. lattice
@pytest.mark.parametrize("slabbed", [False, True])
def test_lattice_closed_form_equals_the_oracle_at_12(slabbed):
    pos, root, links = fc.lattice(12, slabbed)
    g = orc.groups(pos, fc.LATTICE_B, boxsize=12.0)
    assert g["margin"] == pytest.approx(1.0 / 9.0, rel=1e-12)            # d^2 = 2 against b^2 = 2.25
    assert (g["links"], g["length"].tolist()) == ((11520, [720, 720]) if slabbed else (15552, [1728]))
    assert same(fc.known(root, links), g)
    assert not np.array_equal(np.sort(pos, axis=0), pos)                 # shuffled
    assert sorted(set(g["first"].tolist())) == sorted(set(root.tolist()))


def test_lattice_numbers_at_24_and_its_three_plans():
    pos, root, links = fc.lattice(24, False)
    assert len(pos) == 13824 and links == 9 * 13824 == 124416 and (root == 0).all()
    spos, sroot, slinks = fc.lattice(24, True)
    assert len(spos) == 12672 and slinks == 108288
    firsts, sizes = np.unique(sroot, return_counts=True)
    assert sizes.tolist() == [6336, 6336] and firsts[0] == 0 and firsts[1] > 0
    for f in firsts:                                                     # first: the smallest index of its slab
        side = spos[f, 0] > 12
        assert f == np.nonzero((spos[:, 0] > 12) == side)[0].min()
    # links again from the offsets: every half-shell friend offset, counted over the kept points whose partner is kept
    kept = np.ones(24, dtype=bool)
    kept[[0, 12]] = False
    offs = [o for o in ((dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1))
            if 0 < sum(c * c for c in o) <= 2 and o[::-1] > (0, 0, 0)]
    assert len(offs) == 9
    assert sum(576 * int((kept & np.roll(kept, -o[0])).sum()) for o in offs) == slinks
    dims = lambda p, per: fc.plan_sphere(p, fc.LATTICE_B, 24.0, cap=fc.plan_cap(len(p), per)).dims.tolist()
    assert dims(pos, 64) == [6] * 3 and dims(pos, 1) == [15] * 3 and dims(pos, 512) == [3] * 3
    assert dims(spos, 64) == [5] * 3 and dims(spos, 1) == [15] * 3 and dims(spos, 512) == [3] * 3
    cells = fc.plan_sphere(pos, fc.LATTICE_B, 24.0, cap=fc.plan_cap(len(pos), 512))
    assert np.bincount(cells.cell_id).tolist() == [512] * 27            # two tiles of 256 per cell
    assert np.bincount(fc.plan_sphere(pos, fc.LATTICE_B, 24.0).cell_id).tolist() == [64] * 216


# ------------------------------------------------------------------ 2. serpentine
@pytest.mark.parametrize("cut", [False, True])
def test_serpentine_is_one_path(cut):
    pos, path = fc.serpentine(cut)
    g = orc.groups(pos, fc.SERPENTINE_B)
    assert g["margin"] > 0.18
    if cut:
        assert len(pos) == 4436 and g["links"] == 4434 and g["ncomponents"] == 2
        assert sorted(g["length"].tolist()) == sorted([16 * 139 + 64, 4437 - 16 * 139 - 65])
        assert same(fc.known(fc.min_index_roots(path > 16 * 139 + 64), 4434), g)
    else:
        assert len(pos) == 4437 and g["links"] == 4436 and g["length"].tolist() == [4437]
    i, j, _ = orc.friend_pairs(pos, fc.SERPENTINE_B)
    assert (np.abs(path[i] - path[j]) == 1).all()                        # friends are path neighbours, nothing else
    default = fc.plan_sphere(pos, fc.SERPENTINE_B)
    finest = fc.plan_sphere(pos, fc.SERPENTINE_B, cap=fc.plan_cap(len(pos), 1))
    assert default.dims.tolist() == [5, 13, 1] and finest.dims.tolist() == [37, 101, 1]
    assert len(np.unique(finest.cell_id)) > 300                          # the path crosses hundreds of cells


# ------------------------------------------------------------------ 3. forests
def test_forests_and_the_pass_bound():
    for n in (2, 3, 1024, 1025, 4096, 4097):
        chain = fc.forest("chain", n)
        root, depth = fc.chase(chain)
        assert (root == 0).all() and depth == n - 1
        assert 1 <= fc.jump_passes(chain) <= fc.max_passes(n)
    # a pass covers three links: what the GPU took as well
    assert [fc.jump_passes(fc.forest("chain", n)) for n in (2, 3, 1024, 1025, 4096, 4097)] == [1, 1, 7, 7, 8, 8]
    assert [fc.max_passes(n) for n in (1, 2, 3, 1024, 1025, 1500, 4096, 4097)] == [1, 2, 3, 11, 12, 12, 13, 14]
    for kind in ("star", "heap", "random", "identity"):
        p = fc.forest(kind, 5000)
        assert (p <= np.arange(5000)).all() and p.dtype == np.int32
        root, depth = fc.chase(p)
        assert (p[root] == root).all()
        assert fc.jump_passes(p) <= fc.max_passes(5000)
        flat = kind in ("star", "identity")
        assert (fc.jump_passes(p) == 1) == flat and (depth <= 1) == flat
    assert fc.chase(fc.forest("random", 5000))[1] > 10 and len(np.unique(fc.chase(fc.forest("random", 5000))[0])) > 1
    cyc = fc.forest("two_cycle", 100)
    assert ((cyc >= 0) & (cyc < 100)).all()
    with pytest.raises(ValueError):
        fc.chase(cyc)


# ------------------------------------------------------------------ 4. open-boundary geometry
@pytest.mark.parametrize("name,which", fc.geometry_cases())
def test_geometry_cases(name, which):
    pos, reach, cond = fc.geometry(name)
    b, g = fc.geometry_b(name, which), fc.geometry_groups(name, which)
    n = len(pos)
    if (name, which) in fc.EXACT:
        assert g["margin"] == 0.0
    else:
        assert g["margin"] > (fc.NEAR_MARGIN if (name, which) in fc.NEAR else fc.MARGIN), g["margin"]
    finest = pg.plan(pos, b, cap=fc.plan_cap(n, 1))
    assert fc.plan_cap(n, 1) == max(27, n)
    if which == "reach":
        assert finest.dims.tolist() == list(cond["dims"])
    elif name == "all_coincident":
        assert g["ncomponents"] == 1                                     # one group at any b
    elif name == "one_cell_2":
        assert g["length"].tolist() == [1, 1]                            # two points: the other answer there is
    else:
        assert g["ncomponents"] >= 2 and g["length"][0] >= 2
    # the walk over either planned grid sees every friend pair
    i, j, _ = orc.friend_pairs(pos, b)
    for plan in (finest, fc.plan_sphere(pos, b)):
        wi, _ = fc.walk_pairs(plan, i, j, periodic=False)
        assert len(wi) == len(i)


def test_geometry_known_counts():
    pos, _, _ = fc.geometry("edge_pairs")
    g = fc.geometry_groups("edge_pairs", "reach")
    assert g["links"] == int(pg.brute_pair_counts(pos, 8, 7.0, dmax=49.0).sum())
    assert g["links"] > int(pg.brute_pair_counts(pos, 7, 7.0).sum())     # the pairs at exactly 49 are among them
    pos, _, _ = fc.geometry("coincident")
    i, j, _ = orc.friend_pairs(pos, 2.5)
    d = pos[i] - pos[j]
    assert int(((d * d).sum(axis=1) == 0.0).sum()) == 300 * 299 // 2 == 44850
    f32 = fc.geometry("offset_f32")[0]
    assert np.array_equal(f32, f32.astype(np.float32).astype(np.float64))
    assert not np.array_equal(fc.geometry_groups("offset_f32", "second")["labels"],
                              fc.geometry_groups("offset_1e6", "second")["labels"])


# ------------------------------------------------------------------ 5. cylinder
@pytest.mark.parametrize("los", [0, 1, 2])
def test_collapsed_axis(los):
    c = fc.COLLAPSED
    pos, g = fc.collapsed(los), fc.collapsed_groups(los)
    assert pos.shape == (200, 3) and (pos >= 0).all() and (pos < 100).all()
    perp = [a for a in range(3) if a != los]
    plan = fc.plan_cyl(pos, c["b_perp"], c["b_para"], los, c["L"])
    assert plan.dims[los] == 1 and plan.dims[perp].tolist() == [5, 5] and plan.steps == 13
    fine = fc.plan_cyl(pos, c["b_perp"], c["b_para"], los, c["L"], cap=fc.plan_cap(200, 1))
    assert fine.dims[los] == 1 and fine.dims[perp].tolist() == [13, 13]
    assert g["length"][:6].min() >= 20 and g["margin"] > 6e-5
    i, j, _ = orc.friend_pairs(pos, c["b_perp"], c["L"], c["b_para"], los)
    raw = np.abs(pos[i] - pos[j])
    assert (raw[:, los] > 50.0).sum() >= 1                               # friends through the face of the line of sight
    assert (raw[:, perp[0]] > 50.0).sum() >= 1                           # and through a perpendicular face
    for p in (plan, fine):
        wi, wj = fc.walk_pairs(p, i, j, periodic=True)
        assert same(fc.groups_from_pairs(200, wi, wj), g)
        ni, nj = fc.walk_pairs(p, i, j, periodic=True, wrap=False)       # the wrong walk loses the perpendicular face
        assert len(ni) < len(i) and not same(fc.groups_from_pairs(200, ni, nj), g)
    assert not same(orc.groups(pos, c["b_perp"], None, 1, c["b_para"], los), g)


@pytest.mark.parametrize("los", [0, 1, 2])
def test_lattice8_exact_limits(los):
    ijk = fc.lattice8()
    for (b_perp, b_para), (periodic, open_) in fc.LATTICE8.items():
        for box, (links, sizes) in ((8.0, periodic), (None, open_)):
            g = orc.groups(ijk, b_perp, box, 1, b_para, los)
            assert g["links"] == links and g["length"].tolist() == sizes, (b_perp, b_para, box)
    strict = fc.groups_from_pairs(512, *fc.friend_pairs_strict_pi(ijk, 1.0, 1.0, los, 8.0))
    assert strict["links"] == 2 * 512 and not same(strict, orc.groups(ijk, 1.0, 8.0, 1, 1.0, los))


@pytest.mark.parametrize("los", [0, 1, 2])
def test_open_cylinder_plan_is_anisotropic(los):
    pos = fc.clustered()
    perp = [a for a in range(3) if a != los]
    for per, across, along in ((64, 8, 1), (1, 27, 5)):
        p = fc.plan_cyl(pos, fc.CB_PERP, fc.CB_PARA, los, cap=fc.plan_cap(len(pos), per))
        assert p.dims[perp].tolist() == [across, across] and p.dims[los] == along and p.steps > 0
        assert (p.lo == pos.min(axis=0)).all()
        assert fc.plan_cyl(pos, fc.CB_PERP, fc.CB_PARA, los, cap=fc.plan_cap(len(pos), per), growth=1.5).dims.tolist() \
            != p.dims.tolist()
    far = pos + 1.0e9                                                    # the margins: another grid without them
    b = float((far.max(axis=0) - far.min(axis=0)).min()) / 50.0 / (1.0 + 5e-6)
    with_, without = (fc.plan_cyl(far, b, b, los, cap=10 ** 9, margins=m) for m in (True, False))
    assert with_.dims.min() == 49 and without.dims.min() == 50


# ------------------------------------------------------------------ 6. boundaries, tiny N, sizes
@pytest.mark.parametrize("axes", fc.FACE_SETS)
def test_boundary_clumps(axes):
    pos = fc.on_the_boundary(axes)
    assert pos.max() == 100.0 and pos.min() == 0.0 and all(pos[0, a] == 100.0 and pos[1, a] == 0.0 for a in axes)
    per, opn = orc.groups(pos, fc.FACE_B, fc.FACE_L), orc.groups(pos, fc.FACE_B)
    assert per["margin"] > fc.MARGIN and opn["margin"] > fc.MARGIN
    lab = per["labels"]
    assert lab[0] == lab[1] == lab[2] == lab[3] != lab[4] and (lab == lab[0]).sum() == 4 and (lab == lab[4]).sum() == 1
    lab = opn["labels"]
    assert lab[0] == lab[3] != lab[1] == lab[2] and (lab == lab[0]).sum() == 2 and (lab == lab[1]).sum() == 2
    plan = fc.plan_sphere(pos, fc.FACE_B, fc.FACE_L, cap=fc.plan_cap(len(pos), 1))
    assert plan.dims.tolist() == [10] * 3
    assert all(plan.cells[0, a] == 9 and plan.cells[1, a] == 0 for a in axes)     # x = L: the last cell; 0: the first
    i, j, _ = orc.friend_pairs(pos, fc.FACE_B, fc.FACE_L)
    wi, wj = fc.walk_pairs(plan, i, j, periodic=True)
    assert len(wi) == len(i)
    ni, nj = fc.walk_pairs(plan, i, j, periodic=True, wrap=False)
    assert not same(fc.groups_from_pairs(len(pos), ni, nj), per)


@pytest.mark.parametrize("n", fc.TINY_N)
def test_tiny_catalogues(n):
    pos = fc.tiny(n, True)
    assert orc.groups(pos, fc.TINY_B, fc.TINY_L)["length"].tolist() == [n]
    assert orc.groups(pos, fc.TINY_B)["length"].tolist() == ([n] if n < 4 else [n - 3, 3])
    for box in (fc.TINY_L, None):
        g = orc.groups(fc.tiny(n, False), fc.TINY_B, box)
        assert g["links"] == 0 and g["length"].tolist() == [1] * n
    assert fc.plan_cap(n) == 27 and fc.plan_cap(n, 1) == max(27, n)      # the floor: more cells than objects below 27


def test_a_cell_cap_of_n_plans_other_grids():
    """What the read-back of the planned grid tells apart: fof_plan_cap(n) against the pair finders' cap of n."""
    pos, _ = fc.serpentine()
    default = fc.plan_sphere(pos, fc.SERPENTINE_B)
    assert pg.plan(pos, fc.SERPENTINE_B, cap=len(pos)).dims.tolist() != default.dims.tolist()
    differ = 0
    for name, which in fc.geometry_cases():
        p, b = fc.geometry(name)[0], fc.geometry_b(name, which)
        differ += pg.plan(p, b, cap=len(p)).dims.tolist() != fc.plan_sphere(p, b).dims.tolist()
    assert differ >= 10
    two = fc.tiny(26, True)
    assert pg.plan(two, fc.TINY_B, cap=8).dims.tolist() != pg.plan(two, fc.TINY_B, cap=fc.plan_cap(26)).dims.tolist()
    c = fc.COLLAPSED
    assert fc.plan_cyl(fc.collapsed(2), c["b_perp"], c["b_para"], 2, c["L"], cap=200).dims.tolist() != [5, 5, 1]


def test_sized_groups():
    pos = fc.sized_groups()
    assert len(pos) == sum(fc.SIZES) and pos.max() == 100.0 and (pos >= 0).all()
    g = orc.groups(pos, fc.SIZES_B, fc.SIZES_L)
    assert g["length"].tolist() == sorted(fc.SIZES, reverse=True) and g["margin"] > 0.1
    assert g["links"] == sum(s * (s - 1) // 2 for s in fc.SIZES)         # every pair of a clump
    assert len(orc.groups(pos, fc.SIZES_B)["length"]) == 7               # open: the clump across the face splits
    f = orc.features(pos, g, boxsize=fc.SIZES_L)
    across = f["cm_position"][2]                                         # the clump of 65
    assert across[0] < 0.15 or across[0] > 99.85


def test_feature_ratio_is_zero_for_the_oracle_and_bites():
    pos = fc.sized_groups()
    vel, w = fc.feature_inputs(len(pos))
    g = orc.groups(pos, fc.SIZES_B, fc.SIZES_L)
    ref = orc.features(pos, g, boxsize=fc.SIZES_L, vel=vel, weights=w)
    assert all(r.max() == 0.0 for r in fc.feature_ratios(ref, ref, g["length"]).values())
    off = {k: v * (1.0 + 1e-12) for k, v in ref.items()}
    assert all(r.max() > 1.0 for r in fc.feature_ratios(off, ref, g["length"]).values())
