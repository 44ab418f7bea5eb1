"""GPU: the friends-of-friends finder (astrild_amd/csrc/fof.hip, particles/hutils/fof.py) at its edges and under
contention, on the catalogues of tests/fof_cases.py (tests/test_fof_cases_cpu.py shows what each of them reaches):

1. one component out of many cells and workgroups - the 24^3 lattice, whole and in two slabs, under four plans, with the
   parent forest read back between ast_fof_link and ast_fof_compress;
2. a long path through hundreds of cells - the serpentine;
3. ast_fof_compress alone on hand-made forests in a dirty workspace, and its AST_ERR_LIMIT return;
4. every open-boundary catalogue of tests/pair_geometry.py at two linking lengths, with the planned grid read back;
5. the cylinder: open boundaries, the line-of-sight axis collapsed to one cell, pairs exactly at both limits;
6. members at exactly 0 and exactly L on faces, edges and the corner; 2 <= N <= 28; fof_features for every dtype
   pairing, open boundaries, single-particle groups and groups of 1, 63, 64, 65, 128 and 129 members.

Every integer result - labels, length, first, members, offsets, links, root, size, the planned grid's dims, ncells and
ntiles - is compared for equality, lo and inv_cs of the grid bit for bit; the features against exactly rounded rational
sums with the bound that tests/test_gpu_fof.py::test_features derives (fof_cases.feature_ratios)."""
import ctypes as ct
import functools

import numpy as np
import pytest

from tests import fof_cases as fc
from tests import fof_oracle as orc
from tests import pair_geometry as pg
from tests.dirty_memory import dirty_alloc  # noqa: F401  (a fixture)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

KEYS = ("labels", "length", "first", "members", "offsets")
DTYPES = {"labels": np.int32, "length": np.int64, "first": np.int64, "members": np.int32, "offsets": np.int64}
PLANS = {"cells_of_64": dict(), "cells_of_1": dict(AST_FOF_CELL_OBJECTS="1"),
         "cells_of_512": dict(AST_FOF_CELL_OBJECTS="512"), "one_cell": dict(ASTRILD_FOF_CELLS="0")}
PER = {"cells_of_64": 64, "cells_of_1": 1, "cells_of_512": 512}
AST_ERR_LIMIT = -5


def fof():
    from astrild_amd.particles.hutils import fof as module
    return module


def host(groups):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in groups.items()}


def assert_groups(got, ref, what=""):
    got = host(got)
    assert got["links"] == ref["links"] and isinstance(got["links"], int), (what, got["links"], ref["links"])
    for k in KEYS:
        assert got[k].dtype == DTYPES[k] and got[k].shape == ref[k].shape, (what, k)
        assert np.array_equal(got[k], ref[k]), (what, k)


def use_plan(monkeypatch, plan):
    monkeypatch.delenv("AST_FOF_CELL_OBJECTS", raising=False)
    monkeypatch.delenv("ASTRILD_FOF_CELLS", raising=False)
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)


def align256(b):
    return (b + 255) & ~255


def parent_area(lib, n):
    """Where `parent` (n int32) lies in the workspace.  fof_layout(n) is a GridLayout whose last area, `part`, holds
    it: total = part + align256(part_bytes) with part_bytes = 4 n, so part = ast_fof_workspace_bytes(n) - align256(4 n).
    (byte offset, workspace bytes), the area inside the workspace."""
    total = int(lib.ast_fof_workspace_bytes(n))
    off = total - align256(4 * n)
    assert 0 < off and off % 256 == 0 and off + 4 * n <= total
    return off, total


def run_abi(pos, b, box=None, b_para=None, los=2, single=False):
    """ast_fof_prepare, ast_fof_link and ast_fof_compress on a workspace of the test's own: `parent` as the link kernel
    left it (numpy), the planned grid read back from the workspace head, root and size (device int32), links, passes."""
    from astrild_amd import _lib
    from astrild_amd.device import as_device, check, ptr, real_code, stream
    lib = _lib.lib()
    p = as_device(pos)
    n = int(p.shape[0])
    off, total = parent_area(lib, n)
    work = torch.empty(total, dtype=torch.uint8, device="cuda")
    bounds = torch.empty(6, dtype=torch.float64, device="cuda")
    links = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    st = stream()
    check(lib.ast_fof_prepare(ptr(p), real_code(p), n, ptr(work), total, ptr(bounds), st), "ast_fof_prepare")
    check(lib.ast_fof_link(ptr(work), total, n, 0.0 if box is None else float(box), int(b_para is not None), float(b),
                           float(b_para or 0.0), int(los), int(single), ptr(links), st), "ast_fof_link")
    torch.cuda.synchronize()
    parent = work[off:off + 4 * n].cpu().numpy().view(np.int32).copy()
    grid = pg.parse_grid_params(work[:128].cpu().numpy())
    bound = lib.ast_fof_max_passes(n)
    pending = torch.empty(bound, dtype=torch.int32, device="cuda")
    root = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    size = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    passes = ct.c_int(0)
    check(lib.ast_fof_compress(ptr(work), total, n, ptr(pending), ct.byref(passes), ptr(root), ptr(size), st),
          "ast_fof_compress")
    torch.cuda.synchronize()
    assert 1 <= passes.value <= bound
    return dict(parent=parent, grid=grid, root=root, size=size, links=int(links.item()), passes=passes.value,
                bound=bound)


def numbered(run, nmin=1):
    out = fof().number_groups(run["root"], run["size"], nmin)
    out["links"] = run["links"]
    return out


def assert_grid(grid, want, what=""):
    assert grid["dims"].tolist() == want.dims.tolist(), (what, grid["dims"], want.dims)
    assert grid["ncells"] == int(np.prod(want.dims)), what
    assert grid["ntiles"] == pg.tiles(want), what
    assert np.array_equal(grid["lo"], want.lo) and np.array_equal(grid["inv_cs"], want.inv_cs), what


def assert_forest(run, root_ref, what=""):
    """The forest as ast_fof_link leaves it: parent[x] <= x; two particles under one root exactly when the known answer
    has them in one group (the root need not be the smallest index yet).  After ast_fof_compress: root = the group's
    smallest index, size = the group's size there and 0 elsewhere."""
    parent, n = run["parent"], len(root_ref)
    assert parent.shape == (n,) and (parent >= 0).all() and (parent <= np.arange(n)).all(), what
    top, depth = fc.chase(parent)
    pairs = np.unique(np.stack([top, root_ref], axis=1), axis=0)
    assert len(pairs) == len(np.unique(top)) == len(np.unique(root_ref)), what
    root, size = run["root"].cpu().numpy(), run["size"].cpu().numpy()
    assert np.array_equal(root, root_ref), what
    assert np.array_equal(size, np.bincount(root_ref, minlength=n)), what
    return depth


# ------------------------------------------------------------------ 1. the slabbed lattice
@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("slabbed", [False, True], ids=["whole", "two_slabs"])
def test_lattice_forest_under_contention(slabbed, plan, monkeypatch):
    """13 824 points in one group (124 416 links), or 12 672 in two slabs of 6336 (108 288 links): every cell and every
    workgroup unites into the same one or two trees.  If an assertion on `parent` fails here, the proof in fof_unite's
    comment is wrong or the code is."""
    use_plan(monkeypatch, plan)
    pos, root_ref, links = fc.lattice(24, slabbed)
    ref = fc.known(root_ref, links)
    assert ref["length"].tolist() == ([6336, 6336] if slabbed else [13824])
    labels = []
    for call in range(2):
        run = run_abi(pos, fc.LATTICE_B, box=24.0, single=plan == "one_cell")
        if plan == "one_cell":
            assert run["grid"]["dims"].tolist() == [1, 1, 1]
        else:
            want = fc.plan_sphere(pos, fc.LATTICE_B, 24.0, cap=fc.plan_cap(len(pos), PER[plan]))
            assert_grid(run["grid"], want, plan)
            if not slabbed:
                assert want.dims[0] == {"cells_of_64": 6, "cells_of_1": 15, "cells_of_512": 3}[plan]
        depth = assert_forest(run, root_ref, plan)
        print(f"lattice {'slabs' if slabbed else 'whole'} {plan} call {call}: depth after link {depth}, "
              f"{run['passes']} passes (bound {run['bound']})")
        got = numbered(run)
        assert_groups(got, ref, plan)
        labels.append(host(got)["labels"])
    assert np.array_equal(labels[0], labels[1])
    assert_groups(fof().fof_groups(pos, fc.LATTICE_B, boxsize=24.0), ref, plan)


# ------------------------------------------------------------------ 2. the serpentine
@functools.lru_cache(maxsize=None)
def serpentine_ref(cut):
    return orc.groups(fc.serpentine(cut)[0], fc.SERPENTINE_B)


@pytest.mark.parametrize("plan", ["cells_of_64", "cells_of_1"])
@pytest.mark.parametrize("cut", [False, True], ids=["whole", "cut"])
def test_serpentine(cut, plan, monkeypatch):
    use_plan(monkeypatch, plan)
    pos, _ = fc.serpentine(cut)
    ref = serpentine_ref(cut)
    assert (ref["links"], len(ref["length"])) == ((4434, 2) if cut else (4436, 1))
    run = run_abi(pos, fc.SERPENTINE_B)
    assert_grid(run["grid"], fc.plan_sphere(pos, fc.SERPENTINE_B, cap=fc.plan_cap(len(pos), PER[plan])), plan)
    depth = assert_forest(run, fc.min_index_roots(ref["labels"]), plan)
    print(f"serpentine {'cut' if cut else 'whole'} {plan}: depth after link {depth}, {run['passes']} passes "
          f"(bound {run['bound']})")
    assert_groups(numbered(run), ref, plan)
    got, passes = fof().fof_groups(pos, fc.SERPENTINE_B, return_passes=True)
    assert 1 <= passes <= run["bound"]
    assert_groups(got, ref, plan)


# ------------------------------------------------------------------ 3. ast_fof_compress on hand-made forests
def compress(parent, work=None, sentinel=-7):
    """ast_fof_compress on `parent` written into a workspace that went through neither prepare nor link:
    (return code, passes, root, size, work); root and size pre-filled with `sentinel`."""
    from astrild_amd import _lib
    from astrild_amd.device import ptr, stream
    lib = _lib.lib()
    n = len(parent)
    off, total = parent_area(lib, n)
    if work is None:
        work = torch.empty(total, dtype=torch.uint8, device="cuda")      # dirty: the fixture poisons it
    work[off:off + 4 * n] = torch.from_numpy(np.ascontiguousarray(parent, dtype=np.int32).view(np.uint8).copy()).cuda()
    pending = torch.empty(lib.ast_fof_max_passes(n), dtype=torch.int32, device="cuda")
    root = torch.full((n,), sentinel, dtype=torch.int32, device="cuda")
    size = torch.full((n,), sentinel, dtype=torch.int32, device="cuda")
    passes = ct.c_int(-1)
    rc = lib.ast_fof_compress(ptr(work), total, n, ptr(pending), ct.byref(passes), ptr(root), ptr(size), stream())
    torch.cuda.synchronize()
    return rc, passes.value, root.cpu().numpy(), size.cpu().numpy(), work


FORESTS = [("chain", n) for n in (2, 3, 1024, 1025, 4096, 4097)] + [("star", 5000), ("heap", 4097), ("heap", 5000),
                                                                    ("random", 5000), ("identity", 5000)]


@pytest.mark.parametrize("kind,n", FORESTS, ids=[f"{k}_{n}" for k, n in FORESTS])
def test_compress_on_a_known_forest(kind, n, dirty_alloc):
    from astrild_amd import _lib
    parent = fc.forest(kind, n)
    want, depth = fc.chase(parent)
    mark = dirty_alloc.mark()
    rc, passes, root, size, _ = compress(parent)
    assert dirty_alloc.since(mark) >= 2                                  # the workspace and `pending`
    bound = _lib.lib().ast_fof_max_passes(n)
    assert bound == fc.max_passes(n)
    log3 = int(np.ceil(np.log(n) / np.log(3.0) - 1e-12)) + 1
    print(f"compress {kind} n={n}: longest path {depth}, {passes} passes; ceil(log3 n) + 1 = {log3}, bound {bound}")
    assert rc == 0 and 1 <= passes <= bound
    if kind in ("star", "identity"):
        assert passes == 1
    assert np.array_equal(root, want)
    assert np.array_equal(size, np.bincount(want, minlength=n))
    if kind == "identity":
        assert (size == 1).all()


def test_compress_refuses_what_is_not_a_forest(dirty_alloc):
    """A two-cycle never resolves: the bounded host loop ends with AST_ERR_LIMIT, the message names the passes, root
    and size are untouched, and the same workspace serves a valid call afterwards.  No index outside [0, n) is
    formed."""
    from astrild_amd import _lib
    n = 1000
    lib = _lib.lib()
    rc, passes, root, size, work = compress(fc.forest("two_cycle", n), sentinel=-12345)
    bound = lib.ast_fof_max_passes(n)
    assert rc == AST_ERR_LIMIT and passes == bound
    msg = lib.ast_last_error().decode()
    assert "passes" in msg and str(bound) in msg, msg
    assert (root == -12345).all() and (size == -12345).all()
    parent = fc.forest("random", n)
    want, _ = fc.chase(parent)
    rc, passes, root, size, _ = compress(parent, work=work)
    assert rc == 0 and 1 <= passes <= bound
    assert np.array_equal(root, want) and np.array_equal(size, np.bincount(want, minlength=n))


# ------------------------------------------------------------------ 4. open-boundary geometry
@pytest.mark.parametrize("name,which", fc.geometry_cases(), ids=[f"{n}-{w}" for n, w in fc.geometry_cases()])
def test_open_geometry(name, which, monkeypatch):
    pos, reach, cond = fc.geometry(name)
    b, ref = fc.geometry_b(name, which), fc.geometry_groups(name, which)
    given = pos.astype(np.float32) if name == "offset_f32" else pos
    assert np.array_equal(given.astype(np.float64), pos)
    n = len(pos)
    for plan in ("cells_of_1", "cells_of_64", "one_cell"):
        use_plan(monkeypatch, plan)
        what = f"{name} b={b} {plan}"
        run = run_abi(given, b, single=plan == "one_cell")
        if plan == "one_cell":
            assert run["grid"]["dims"].tolist() == [1, 1, 1] and run["grid"]["ntiles"] == (n + 255) // 256, what
        else:
            assert fc.plan_cap(n, 1) == max(27, n)
            assert_grid(run["grid"], pg.plan(pos, b, cap=fc.plan_cap(n, PER[plan])), what)
            if plan == "cells_of_1" and which == "reach":
                assert run["grid"]["dims"].tolist() == list(cond["dims"]), what
        assert_forest(run, fc.min_index_roots(ref["labels"]), what)
        assert_groups(numbered(run), ref, what)
        assert_groups(fof().fof_groups(given, b), ref, what)
    if (name, which) == ("edge_pairs", "reach"):                         # the pairs at exactly d = 49 are friends
        assert ref["links"] == int(pg.brute_pair_counts(pos, 8, 7.0, dmax=49.0).sum())
    if name == "coincident":
        assert ref["links"] >= 44850


# ------------------------------------------------------------------ 5. the cylinder
@pytest.mark.parametrize("los", [0, 1, 2])
def test_cylinder_open_boundaries(los, monkeypatch):
    pos, ref = fc.clustered(), fc.clustered_cylinder_open(los)
    perp = [a for a in range(3) if a != los]
    for plan in ("cells_of_64", "cells_of_1"):
        use_plan(monkeypatch, plan)
        run = run_abi(pos, fc.CB_PERP, b_para=fc.CB_PARA, los=los)
        want = fc.plan_cyl(pos, fc.CB_PERP, fc.CB_PARA, los, cap=fc.plan_cap(len(pos), PER[plan]))
        assert_grid(run["grid"], want, plan)
        dims = run["grid"]["dims"]
        assert dims[perp[0]] == dims[perp[1]] > dims[los] and dims[los] == (1 if plan == "cells_of_64" else 5)
        assert_groups(numbered(run), ref, plan)
        assert_groups(fof().fof_groups(pos, fc.CB_PERP, b_para=fc.CB_PARA, los=los), ref, plan)
    if los == 2:
        groups = fof().FoFGroups(pos, 0.14, 0.75, Lbox=fc.CL)
        assert np.array_equal(groups.group_ids, ref["labels"]) and groups.links == ref["links"]
        assert groups.n_groups == len(ref["length"])


@pytest.mark.parametrize("los", [0, 1, 2])
def test_cylinder_with_the_line_of_sight_in_one_cell(los, monkeypatch):
    c = fc.COLLAPSED
    pos, ref = fc.collapsed(los), fc.collapsed_groups(los)
    perp = [a for a in range(3) if a != los]
    for plan, across in (("cells_of_64", 5), ("cells_of_1", 13)):
        use_plan(monkeypatch, plan)
        run = run_abi(pos, c["b_perp"], box=c["L"], b_para=c["b_para"], los=los)
        want = fc.plan_cyl(pos, c["b_perp"], c["b_para"], los, c["L"], cap=fc.plan_cap(200, PER[plan]))
        assert_grid(run["grid"], want, plan)
        dims = run["grid"]["dims"]
        assert dims[los] == 1 and dims[perp].tolist() == [across, across]
        assert_forest(run, fc.min_index_roots(ref["labels"]), plan)
        assert_groups(numbered(run), ref, plan)
        assert_groups(fof().fof_groups(pos, c["b_perp"], boxsize=c["L"], b_para=c["b_para"], los=los), ref, plan)


@pytest.mark.parametrize("los", [0, 1, 2])
def test_cylinder_exactly_at_its_limits(los, monkeypatch):
    """pi <= b_para at pi = b_para and rp^2 <= b_perp^2 at rp = b_perp on the 8^3 lattice; one ulp below either, those
    links are gone.  fof_cases.LATTICE8 has the counts, which the CPU test holds to the oracle."""
    ijk = fc.lattice8()
    for plan in ("cells_of_64", "cells_of_1", "one_cell"):
        use_plan(monkeypatch, plan)
        for (b_perp, b_para), (periodic, open_) in fc.LATTICE8.items():
            for box, (links, sizes) in ((8.0, periodic), (None, open_)):
                got = host(fof().fof_groups(ijk, b_perp, boxsize=box, b_para=b_para, los=los))
                what = (plan, b_perp, b_para, box)
                assert got["links"] == links and got["length"].tolist() == sizes, what
                line = np.delete(ijk, los, axis=1) @ np.array([8, 1])
                group_of = {512: np.zeros(512), 64: ijk[:, los], 8: line}[sizes[0]]
                assert np.array_equal(got["labels"], fc.known(fc.min_index_roots(group_of), links)["labels"]), what


# ------------------------------------------------------------------ 6. boundaries, tiny N, features
@pytest.mark.parametrize("axes", fc.FACE_SETS, ids=["".join("xyz"[a] for a in s) for s in fc.FACE_SETS])
def test_members_at_exactly_zero_and_exactly_L(axes, monkeypatch):
    pos = fc.on_the_boundary(axes)
    assert pos.max() == fc.FACE_L and pos.min() == 0.0
    periodic, open_ = orc.groups(pos, fc.FACE_B, fc.FACE_L), orc.groups(pos, fc.FACE_B)
    assert len(set(periodic["labels"][:4])) == 1 and len(set(open_["labels"][:4])) == 2
    for plan in ("cells_of_1", "one_cell"):
        use_plan(monkeypatch, plan)
        run = run_abi(pos, fc.FACE_B, box=fc.FACE_L, single=plan == "one_cell")
        assert run["grid"]["dims"].tolist() == ([10] * 3 if plan == "cells_of_1" else [1] * 3)
        assert_groups(numbered(run), periodic, plan)
        assert_groups(fof().fof_groups(pos, fc.FACE_B, boxsize=fc.FACE_L), periodic, plan)
        assert_groups(fof().fof_groups(pos, fc.FACE_B), open_, plan)


@pytest.mark.parametrize("friends", [True, False], ids=["friends", "strangers"])
@pytest.mark.parametrize("n", fc.TINY_N)
def test_fewer_objects_than_cells(n, friends, monkeypatch):
    pos = fc.tiny(n, friends)
    for plan in ("cells_of_64", "cells_of_1", "one_cell"):
        use_plan(monkeypatch, plan)
        for box in (fc.TINY_L, None):
            ref = orc.groups(pos, fc.TINY_B, box)
            run = run_abi(pos, fc.TINY_B, box=box, single=plan == "one_cell")
            if plan != "one_cell":
                want = fc.plan_sphere(pos, fc.TINY_B, box, cap=fc.plan_cap(n, PER[plan]))
                assert_grid(run["grid"], want, (plan, box))
            assert_groups(numbered(run), ref, (plan, box))
            assert_groups(fof().fof_groups(pos, fc.TINY_B, boxsize=box), ref, (plan, box))
            assert_groups(fof().fof_groups(pos.astype(np.float32), fc.TINY_B, boxsize=box, nmin=2),
                          orc.groups(pos.astype(np.float32), fc.TINY_B, box, nmin=2), (plan, box))


def assert_features(pos, ref_groups, box, vel, weights, what):
    """fof_features on the GPU's own groups (equal to ref_groups) against the oracle on the widened values, within the
    derived bound; the same bits on a second call.  Returns (got, oracle)."""
    groups = fof().fof_groups(pos, ref_groups["b"], boxsize=box, nmin=ref_groups["nmin"])
    assert_groups(groups, ref_groups, what)
    got_t = fof().fof_features(pos, groups, boxsize=box, vel=vel, weights=weights)
    again = fof().fof_features(pos, groups, boxsize=box, vel=vel, weights=weights)
    assert set(got_t) == {"cm_position", "weight"} | ({"cm_velocity"} if vel is not None else set())
    for k in got_t:
        assert got_t[k].dtype == torch.float64 and torch.equal(got_t[k], again[k]), (what, k)
    got = {k: v.cpu().numpy() for k, v in got_t.items()}
    ref = orc.features(pos, ref_groups, boxsize=box, vel=vel, weights=weights)
    for k, ratio in fc.feature_ratios(got, ref, ref_groups["length"]).items():
        print(f"fof_features {what} {k}: largest error / bound = {ratio.max():.3g}")
        assert ratio.max() <= 1.0, (what, k)
    if box is not None:
        assert ((got["cm_position"] >= 0.0) & (got["cm_position"] < box)).all(), what
    if weights is None:
        assert np.array_equal(got["weight"], ref_groups["length"].astype(np.float64)), what
    return got, ref


def with_call(groups, b, nmin):
    groups = dict(groups)
    groups["b"], groups["nmin"] = b, nmin
    return groups


F32, F64 = "float32", "float64"
FEATURE_DTYPES = [(p, v, w) for p in (F64, F32) for v in (F64, F32) for w in (F64, F32)]
FEATURE_DTYPES += [(F64, None, F32), (F32, None, F64), (F64, F32, None), (F32, F64, None)]


@pytest.mark.parametrize("pdt,vdt,wdt", FEATURE_DTYPES, ids=["-".join(str(d) for d in c) for c in FEATURE_DTYPES])
def test_features_of_chunk_edge_groups_in_every_dtype(pdt, vdt, wdt):
    """Groups of exactly 1, 63, 64, 65, 128 and 129 members, the one of 65 across the face x = 0 = L with a member at
    exactly L, for each of the eight instantiations of fof_features_kernel and for vel or weights left out."""
    pos = fc.sized_groups().astype(pdt)
    vel, w = fc.feature_inputs(len(pos))
    vel = None if vdt is None else vel.astype(vdt)
    w = None if wdt is None else w.astype(wdt)
    ref_groups = with_call(orc.groups(pos, fc.SIZES_B, fc.SIZES_L), fc.SIZES_B, 1)
    assert ref_groups["length"].tolist() == sorted(fc.SIZES, reverse=True)
    got, ref = assert_features(pos, ref_groups, fc.SIZES_L, vel, w, f"sizes {pdt} {vdt} {wdt}")
    single = int(ref_groups["first"][-1])
    assert np.array_equal(got["cm_position"][-1], pos[single].astype(np.float64))
    assert got["weight"][-1] == (1.0 if w is None else float(w[single]))


def test_features_with_open_boundaries():
    pos = fc.clustered()
    vel, w = fc.feature_inputs(len(pos))
    ref_groups = with_call(fc.clustered_sphere(periodic=False, nmin=20), fc.CB, 20)
    assert len(ref_groups["length"]) == 15
    assert_features(pos, ref_groups, None, vel, w, "open clustered")


def test_features_of_thousands_of_groups():
    """nmin = 1 on the clustered catalogue: 3273 groups in one launch, most of them one particle, whose centre must be
    its position and whose weight its own, exactly."""
    pos = fc.clustered()
    vel, w = fc.feature_inputs(len(pos))
    ref_groups = with_call(fc.clustered_sphere(periodic=True, nmin=1), fc.CB, 1)
    assert len(ref_groups["length"]) == 3273
    got, _ = assert_features(pos, ref_groups, fc.CL, vel, w, "clustered nmin=1")
    ones = np.nonzero(ref_groups["length"] == 1)[0]
    assert len(ones) > 3000
    first = ref_groups["first"][ones]
    assert np.array_equal(got["cm_position"][ones], pos[first])
    assert np.array_equal(got["weight"][ones], w[first])
