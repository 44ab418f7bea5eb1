"""GPU: the friends-of-friends group finder (astrild_amd/particles/hutils/fof.py, astrild_amd/csrc/fof.hip) against the
numpy oracle of tests/fof_oracle.py.  Labels, sizes, first members, member lists, offsets and the link count are
integers and must equal the oracle exactly; the group features are held to the worst case of fp64 evaluation in any
order (test_features).  Every oracle result is computed once per session and shared."""
import functools

import numpy as np
import pytest

from tests import fof_oracle as orc
from tests.dirty_memory import HUGE_BYTES, dirty, dirty_alloc  # noqa: F401  (dirty_alloc: a fixture)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

L, N, NMIN = 100.0, 6000, 20
MEAN_SEP = (L ** 3 / N) ** (1.0 / 3.0)
B = 0.2 * MEAN_SEP
KEYS = ("labels", "length", "first", "members", "offsets")
DTYPES = {"labels": np.int32, "length": np.int64, "first": np.int64, "members": np.int32, "offsets": np.int64}


@functools.lru_cache(maxsize=None)
def catalogue(dtype="float64", seed=11):
    return orc.clustered(L, N, seed).astype(dtype)


@functools.lru_cache(maxsize=None)
def roots(dtype="float64", periodic=True, cylinder=False, los=2, seed=11):
    """(root of every particle, links) of the clustered catalogue by the oracle; the cylinder with the line of sight
    moved to z by a permutation of the axes that keeps the other two in order."""
    pos = catalogue(dtype, seed)
    box = L if periodic else None
    if cylinder:
        perm = [a for a in range(3) if a != los] + [los]
        i, j, _ = orc.friend_pairs(pos[:, perm], 0.14 * MEAN_SEP, box, 0.75 * MEAN_SEP, los=2)
    else:
        i, j, _ = orc.friend_pairs(pos, B, box)
    return orc.components(len(pos), i, j), len(i)


def reference(nmin=NMIN, **kw):
    root, links = roots(**kw)
    ref = orc.number_groups(root, nmin)
    ref["links"] = links
    return ref


def host(groups):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in groups.items()}


def assert_groups(got, ref):
    got = host(got)
    assert got["links"] == ref["links"] and isinstance(got["links"], int)
    for k in KEYS:
        assert got[k].dtype == DTYPES[k] and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k], ref[k]), k


def fof():
    from astrild_amd.particles.hutils import fof as module
    return module


# ------------------------------------------------------------------ 1. clustered
@pytest.mark.parametrize("cell_objects", [None, "1"], ids=["cells_of_64", "cells_of_1"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_clustered_periodic_and_open(dtype, cell_objects, monkeypatch):
    """12 groups (700, 499, 151 and nine of 150: the tie rule bites), one of them across two periodic faces.  The plan
    of one cell per 64 objects gives 4^3 cells here; AST_FOF_CELL_OBJECTS=1, the pair finders' one cell per object,
    gives 18^3 and one cell of 701 objects (tests/test_fof_oracle.py holds the catalogue to that): three tiles and
    three LDS stages either way.  float32 input: the oracle on the widened values."""
    if cell_objects:
        monkeypatch.setenv("AST_FOF_CELL_OBJECTS", cell_objects)
    pos = catalogue(dtype)
    ref = reference(dtype=dtype)
    assert ref["length"].tolist() == [700, 499, 151] + [150] * 9 and int((ref["labels"] == 0).sum()) == 3300
    got = fof().fof_groups(pos, B, boxsize=L, nmin=NMIN)
    assert all(v.is_cuda for k, v in got.items() if k != "links")
    assert_groups(got, ref)
    open_ref = reference(dtype=dtype, periodic=False)
    assert not np.array_equal(open_ref["labels"], ref["labels"]) and open_ref["links"] < ref["links"]
    assert_groups(fof().fof_groups(pos, B, nmin=NMIN), open_ref)


def test_clustered_in_one_cell(monkeypatch):
    monkeypatch.setenv("ASTRILD_FOF_CELLS", "0")
    assert_groups(fof().fof_groups(catalogue(), B, boxsize=L, nmin=NMIN), reference())
    assert_groups(fof().fof_groups(catalogue(), B, nmin=NMIN), reference(periodic=False))


def test_clustered_from_device_tensors():
    for dtype in ("float64", "float32"):
        t = torch.from_numpy(catalogue(dtype).copy()).cuda()
        before = t.clone()
        assert_groups(fof().fof_groups(t, B, boxsize=L, nmin=NMIN), reference(dtype=dtype))
        assert torch.equal(t, before)


# ------------------------------------------------------------------ 2. lattice
def test_lattice_links_at_exactly_b():
    ijk = np.stack(np.meshgrid(*(np.arange(8.0),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    for box, links in ((8.0, 3 * 512), (None, 3 * 8 * 8 * 7)):
        got = host(fof().fof_groups(ijk, 1.0, boxsize=box))
        assert got["links"] == links and got["length"].tolist() == [512] and got["first"].tolist() == [0]
        assert np.array_equal(got["labels"], np.ones(512, dtype=np.int32))
        assert np.array_equal(got["members"], np.arange(512, dtype=np.int32)) and got["offsets"].tolist() == [0, 512]
        got = host(fof().fof_groups(ijk, np.nextafter(1.0, 0.0), boxsize=box))
        assert got["links"] == 0 and np.array_equal(got["labels"], np.arange(1, 513, dtype=np.int32))
        assert np.array_equal(got["length"], np.ones(512, dtype=np.int64))
        assert np.array_equal(got["first"], np.arange(512)) and np.array_equal(got["offsets"], np.arange(513))


# ------------------------------------------------------------------ 3. chain
def chain(s):
    pos = np.zeros((1500, 3))
    pos[:, 0] = np.mod(97.0 + np.arange(1500) * s * 0.05, 100.0)
    pos[:, 2] = 50.0
    return pos


def test_chain_across_the_box_and_the_pass_bound():
    from astrild_amd import _lib
    bound = _lib.lib().ast_fof_max_passes(1500)
    assert bound == 12 and _lib.lib().ast_fof_max_passes(1 << 31) == 0
    pos = chain(0.9)
    got, passes = fof().fof_groups(pos, 0.05, boxsize=100.0, return_passes=True)
    print(f"chain of 1500, periodic: {passes} passes (bound {bound})")
    assert 1 <= passes <= bound
    assert_groups(got, orc.groups(pos, 0.05, boxsize=100.0))
    assert host(got)["length"].tolist() == [1500] and got["links"] == 1499
    got, passes = fof().fof_groups(pos, 0.05, return_passes=True)
    print(f"chain of 1500, open: {passes} passes (bound {bound})")
    assert 1 <= passes <= bound
    assert_groups(got, orc.groups(pos, 0.05))
    assert host(got)["length"].tolist() == [1433, 67] and got["links"] == 1498
    pos = chain(1.1)
    got = fof().fof_groups(pos, 0.05, boxsize=100.0)
    assert_groups(got, orc.groups(pos, 0.05, boxsize=100.0))
    assert got["links"] == 0 and host(got)["length"].tolist() == [1] * 1500


# ------------------------------------------------------------------ 4. nmin and numbering
def test_nmin_and_numbering():
    all_ = reference(nmin=1)
    assert len(all_["length"]) == 3273 and (all_["labels"] > 0).all()
    got = fof().fof_groups(catalogue(), B, boxsize=L, nmin=1)
    assert_groups(got, all_)
    three = reference(nmin=151)
    assert three["length"].tolist() == [700, 499, 151]
    assert_groups(fof().fof_groups(catalogue(), B, boxsize=L, nmin=151), three)
    assert_groups(fof().fof_groups(catalogue(), B, boxsize=L, nmin=701), reference(nmin=701))     # no group at all


# ------------------------------------------------------------------ 5. cylinder
@pytest.mark.parametrize("los", [0, 1, 2])
def test_cylinder(los):
    ref = reference(cylinder=True, los=los)
    assert len(ref["length"]) == 12 and ref["length"][0] >= 700 and ref["length"][1] == 500
    find = lambda: fof().fof_groups(catalogue(), 0.14 * MEAN_SEP, boxsize=L, nmin=NMIN, b_para=0.75 * MEAN_SEP, los=los)
    assert_groups(find(), ref)
    with pytest.MonkeyPatch.context() as mp:             # the cylinder's own plan, a cell width per axis, at its finest
        mp.setenv("AST_FOF_CELL_OBJECTS", "1")
        assert_groups(find(), ref)
    if los == 2:
        groups = fof().FoFGroups(catalogue(), 0.14, 0.75, period=L)
        assert np.array_equal(groups.group_ids, reference(nmin=1, cylinder=True)["labels"])
        assert groups.n_groups == groups.group_ids.max() and groups.group_ids.min() == 1


# ------------------------------------------------------------------ 6. features
def feature_inputs(seed=11):
    rng = np.random.default_rng(seed + 100)
    return rng.normal(0.0, 300.0, (N, 3)), rng.uniform(0.5, 2.0, N)


@functools.lru_cache(maxsize=None)
def feature_reference(weighted):
    vel, w = feature_inputs()
    return orc.features(catalogue(), reference(), boxsize=L, vel=vel, weights=w if weighted else None)


@pytest.mark.parametrize("weighted", [True, False])
def test_features(weighted):
    """The oracle forms s_i = pos_i - p_ref and its wrap in fp64, as the kernel does (one subtraction, one addition: the
    same roundings), and everything after that exactly, rounded once.  With u = 2^-53 and N the members of the group,
    the kernel's cm = p_ref + sum(w s) / W differs from that, to first order in u and for ANY order of the additions,
    by at most: u per product w s and (N - 1) u for their sum, both relative to sum |w s|; (N - 1) u for W and u for the
    division, relative to |sum(w s) / W| <= sum |w s| / W - together 2 N u sum |w s| / W -; u (|p_ref| + sum |w s| / W)
    for the addition of p_ref; u L for the wrap into [0, L); and u (|p_ref| + sum |w s| / W + L) for the oracle's own
    final rounding.  Hence |error| <= (2 N + 4) u (sum |w s| / W + |p_ref| + L) per axis, `scale` of the oracle.  The
    velocity: the same without p_ref and L, (2 N + 1) u sum |w v| / W (`vscale`); the weight: N u W.  The largest error / bound is
    printed.  A second call must give the same bits; the group across two periodic faces (the second largest) is in."""
    vel, w = feature_inputs()
    pos, grp = catalogue(), reference()
    ref = feature_reference(weighted)
    groups = fof().fof_groups(pos, B, boxsize=L, nmin=NMIN)
    args = dict(boxsize=L, vel=vel, weights=w if weighted else None)
    got = fof().fof_features(pos, groups, **args)
    again = fof().fof_features(pos, groups, **args)
    for k in ("cm_position", "cm_velocity", "weight"):
        assert got[k].dtype == torch.float64 and torch.equal(got[k], again[k]), k
    u, n_g = 2.0 ** -53, grp["length"].astype(np.float64)
    cm, cmv, wt = (got[k].cpu().numpy() for k in ("cm_position", "cm_velocity", "weight"))
    worst = {"cm_position": np.abs(cm - ref["cm_position"]) / ((2 * n_g[:, None] + 4) * u * ref["scale"]),
             "cm_velocity": np.abs(cmv - ref["cm_velocity"]) / ((2 * n_g[:, None] + 1) * u * ref["vscale"]),
             "weight": np.abs(wt - ref["weight"]) / (n_g * u * ref["weight"])}
    for k, ratio in worst.items():
        print(f"fof_features {k} weighted={weighted}: largest error / bound = {ratio.max():.3g}")
    corner = ref["cm_position"][1]
    assert (corner[0] < 1.0 or corner[0] > 99.0) and corner[1] > 99.0     # the group across the faces, wrapped
    assert ((cm >= 0.0) & (cm < L)).all()
    if not weighted:
        assert np.array_equal(wt, n_g)
    for k, ratio in worst.items():
        assert ratio.max() <= 1.0, k


# ------------------------------------------------------------------ 7. dirty workspace and outputs
def test_dirty_workspace_and_outputs(dirty_alloc):
    mark = dirty_alloc.mark()
    groups = fof().fof_groups(catalogue(), B, boxsize=L, nmin=NMIN)
    assert dirty_alloc.since(mark) >= 5                  # workspace, bounds, links, pending, root, size, labels
    assert_groups(groups, reference())
    vel, w = feature_inputs()
    got = fof().fof_features(catalogue(), groups, boxsize=L, vel=vel, weights=w)
    with dirty_alloc.using(0x00):
        clean = fof().fof_features(catalogue(), fof().fof_groups(catalogue(), B, boxsize=L, nmin=NMIN), boxsize=L,
                                   vel=vel, weights=w)
    for k in ("cm_position", "cm_velocity", "weight"):
        assert torch.equal(got[k], clean[k]), k
    monkey = pytest.MonkeyPatch()
    try:
        monkey.setenv("ASTRILD_FOF_CELLS", "0")
        assert_groups(fof().fof_groups(catalogue(), B, nmin=NMIN), reference(periodic=False))
    finally:
        monkey.undo()


# ------------------------------------------------------------------ 8. side stream behind a late producer
def test_side_stream_behind_a_late_producer():
    """tests/stream_order.py's probe on both wrappers, the decoy another catalogue of the same recipe.  fof_groups reads
    the bounds, `pending` and the link count on the host (a host_syncs case: the null-stream sleep and the consumer
    check it); fof_features reads nothing back and must return before the producer has run."""
    from tests import stream_order as so
    module = fof()
    pos, decoy = catalogue(), catalogue(seed=12)
    assert not np.array_equal(pos, decoy)
    vel, w = feature_inputs()
    dvel, dw = feature_inputs(seed=12)
    find = lambda p: module.fof_groups(p, B, boxsize=L, nmin=NMIN)
    plain = find(torch.from_numpy(pos.copy()).cuda())
    assert_groups(plain, reference())
    feats = lambda p, v, ww: module.fof_features(p, plain, boxsize=L, vel=v, weights=ww)
    plain_f = feats(*(torch.from_numpy(a.copy()).cuda() for a in (pos, vel, w)))
    be = so.cuda_backend()
    with be.on(be.stream(0)):                            # once plainly under the side stream: code objects loaded
        find(torch.from_numpy(pos.copy()).cuda())
        feats(*(torch.from_numpy(a.copy()).cuda() for a in (pos, vel, w)))
    torch.cuda.synchronize()
    with dirty(HUGE_BYTES):
        late, _ = so.late_call(find, [pos], [decoy])
        late_f, armed = so.late_call(feats, [pos, vel, w], [decoy, dvel, dw])
    assert so.same_bits(late, plain)
    assert_groups(dict(late), reference())
    assert armed, "fof_features waited for the device"
    assert so.same_bits(late_f, plain_f)


# ------------------------------------------------------------------ 9. chain to profiles
def test_groups_to_sphere_profiles():
    from astrild_amd import device as dev
    pos = catalogue()
    finder = fof().FOF(pos, 0.2, NMIN, boxsize=L)
    assert finder.linking_length == pytest.approx(B, rel=1e-15) and finder.max_label == 12
    assert np.array_equal(finder.labels, reference()["labels"]) and finder.labels.dtype == np.int32
    feat = finder.find_features()
    assert np.array_equal(feat["Length"], reference()["length"]) and feat["CMVelocity"] is None
    members, segments = finder.segments()
    assert np.array_equal(members, reference()["members"]) and segments.shape == (12, 2)
    radii, edges = np.full(12, 2.0), np.linspace(0.0, 2.0, 9)
    counts, _ = dev.sphere_profiles(pos[members], feat["CMPosition"], radii, edges, boxsize=L, segments=segments)
    counts = counts.cpu().numpy()
    assert counts.sum() > 2000
    for g, (offset, count) in enumerate(segments):
        s = pos[members[offset:offset + count]] - feat["CMPosition"][g]
        s = np.where(s > L / 2, s - L, np.where(s < -L / 2, s + L, s))
        x = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]) / radii[g]
        assert np.array_equal(counts[g], np.histogram(x, bins=edges)[0]), g
    open_ = fof().FOF(pos, B, NMIN, absolute=True, periodic=False)
    assert np.array_equal(open_.labels, reference(periodic=False)["labels"])


# ------------------------------------------------------------------ 10. empty inputs
def test_empty_and_single_inputs():
    got = host(fof().fof_groups(np.zeros((0, 3)), 1.0, boxsize=10.0))
    assert got["links"] == 0 and got["offsets"].tolist() == [0]
    assert all(got[k].shape == (0,) and got[k].dtype == DTYPES[k] for k in ("labels", "length", "first", "members"))
    one = np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    got, passes = fof().fof_groups(one, 1.0, return_passes=True)
    got = host(got)
    assert passes == 0 and got["links"] == 0 and got["labels"].tolist() == [1] and got["length"].tolist() == [1]
    assert got["first"].tolist() == [0] and got["members"].tolist() == [0] and got["offsets"].tolist() == [0, 1]
    assert all(got[k].dtype == DTYPES[k] for k in KEYS)
    feat = fof().fof_features(one, fof().fof_groups(one, 1.0), vel=one)
    assert feat["cm_position"].cpu().tolist() == [[1.0, 2.0, 3.0]] and feat["weight"].cpu().tolist() == [1.0]
    assert feat["cm_velocity"].cpu().tolist() == [[1.0, 2.0, 3.0]]
    got = host(fof().fof_groups(one, 1.0, nmin=2))
    assert got["labels"].tolist() == [0] and got["length"].shape == (0,) and got["offsets"].tolist() == [0]
    empty = fof().fof_features(np.zeros((0, 3)), fof().fof_groups(np.zeros((0, 3)), 1.0))
    assert empty["cm_position"].shape == (0, 3) and empty["weight"].shape == (0,)
