"""GPU: spherical profiles of particles around centres (ast_profile3d_* through device.sphere_profiles,
profiles.profile_3d.radial_profiles and Profiles3D): lattice cases with answers known by hand, int64 counts exactly equal
to the numpy oracle (tests/profile3d_oracle.py) and moments within a derived bound, a reach as wide as the grid, the
split of a very large centre into work items, the membership mode against the reference's expression, empty and
degenerate inputs, the argument checks, dirty scratch memory, the order of calls and repeated calls.

The moment tolerance 1e-10 * sum|term| is derived, not measured: two summation orders of n <= 2e4 fp64 terms differ by at
most 2 n eps sum|term| ~ 9e-12 sum|term|."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import profile3d_oracle as orc
from tests import tpcf_oracle as torc
from tests.dirty_memory import dirty_alloc                        # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

L = 500.0
NP = 20000
EDGES = np.logspace(np.log10(0.05), np.log10(3.0), 21)
RTOL = 1e-10
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


def gpu(pos, centres, radii, edges, **kw):
    from astrild_amd import device as dev
    counts, moments = dev.sphere_profiles(pos, centres, radii, edges, **kw)
    return dev.to_numpy(counts), dev.to_numpy(moments)


def assert_moments(got, ref, scale, rtol=RTOL):
    err = np.abs(got - ref)
    worst = np.max(err / np.where(scale > 0, scale, 1.0))
    print(f"max |moment - ref| / sum|term| = {worst:.3e}, max |err| where sum|term| == 0: {err[scale == 0].max(initial=0.0):.3e}")
    assert np.all(err <= rtol * scale)


@pytest.fixture(scope="module")
def catalogue():
    """The clustered catalogue, 300 centres (half on particles, half uniform), lognormal radii around 5, weights and
    velocities, and the oracle's answers for each variant of the optional inputs."""
    rng = np.random.default_rng(31)
    pos = torc.clustered(NP, L, 30)
    centres = np.concatenate([pos[rng.choice(NP, 150, replace=False)], rng.uniform(0.0, L, (150, 3))])
    radii = rng.lognormal(np.log(5.0), 0.3, 300)
    cat = {"pos": pos, "centres": centres, "radii": radii, "weights": rng.uniform(0.5, 2.0, NP),
           "vel": rng.normal(0.0, 300.0, (NP, 3)), "centre_vel": rng.normal(0.0, 300.0, (300, 3))}
    assert 3.0 * radii.max() < L / 2
    variants = {"plain": {}, "weights": {"weights": cat["weights"]}, "vel": {"vel": cat["vel"]},
                "all": {"weights": cat["weights"], "vel": cat["vel"], "centre_vel": cat["centre_vel"]},
                "f32": {"weights": cat["weights"], "vel": cat["vel"].astype(np.float32)}}
    cat["kw"] = variants
    cat["ref"] = {}
    for name, kw in variants.items():
        p = pos.astype(np.float32) if name == "f32" else pos
        ref = orc.profiles(p, centres, radii, EDGES, boxsize=L, **kw)
        for a in ref:
            a.setflags(write=False)
        cat["ref"][name] = ref
    assert cat["ref"]["plain"][0].sum() > 20000 and cat["ref"]["plain"][0].max() < 2e4
    return cat


# ---------------------------------------------------------------- known answers and the oracle
@pytest.mark.parametrize("layers", ["1", "0"])
@pytest.mark.parametrize("cells", ["1", "0"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", range(len(orc.LATTICE_CASES)))
def test_lattice(case, dtype, cells, layers, monkeypatch):
    monkeypatch.setenv("ASTRILD_PROFILE3D_CELLS", cells)
    monkeypatch.setenv("ASTRILD_PROFILE3D_LAYERS", layers)
    centres, edges, expected = orc.LATTICE_CASES[case]
    pos = orc.unit_lattice(8).astype(dtype)
    counts, moments = gpu(pos, np.asarray(centres, dtype=dtype), np.ones(len(centres)), edges, boxsize=8.0)
    assert counts.dtype == np.int64 and counts.shape == (len(centres), len(expected))
    for row in counts:
        assert row.tolist() == expected
    npt.assert_array_equal(moments[..., 0], counts)


@pytest.mark.parametrize("variant", ["plain", "weights", "vel", "all", "f32"])
def test_catalogue_equals_the_oracle(catalogue, variant):
    kw = catalogue["kw"][variant]
    pos = catalogue["pos"].astype(np.float32) if variant == "f32" else catalogue["pos"]
    counts, moments = gpu(pos, catalogue["centres"], catalogue["radii"], EDGES, boxsize=L, **kw)
    ref_c, ref_m, scale = catalogue["ref"][variant]
    npt.assert_array_equal(counts, ref_c)
    assert moments.shape == ref_m.shape == (300, 20, 4 if "vel" in kw else 1)
    assert_moments(moments, ref_m, scale)


def test_open_boundaries_equal_the_oracle(catalogue):
    kw = catalogue["kw"]["all"]
    ref_c, ref_m, scale = orc.profiles(catalogue["pos"], catalogue["centres"], catalogue["radii"], EDGES, **kw)
    counts, moments = gpu(catalogue["pos"], catalogue["centres"], catalogue["radii"], EDGES, **kw)
    npt.assert_array_equal(counts, ref_c)
    assert_moments(moments, ref_m, scale)
    assert np.all(ref_c <= catalogue["ref"]["all"][0]) and ref_c.sum() < catalogue["ref"]["all"][0].sum()


@pytest.mark.parametrize("cap,dims", [(27, 3), (64, 4), (125, 5)])
def test_reach_as_wide_as_the_grid(catalogue, cap, dims, monkeypatch):
    """One centre whose reach is 0.49 L: its cell range is clamped to dims cells per axis and no cell is visited twice."""
    from astrild_amd import device as dev
    assert dev.profile3d_dims(NP, cap) == dims
    centre, radius = np.array([[10.0, 250.0, 490.0]]), np.array([10.0])
    edges = np.linspace(0.0, 0.49 * L / 10.0, 9)
    ref_c, ref_m, scale = orc.profiles(catalogue["pos"], centre, radius, edges, boxsize=L, vel=catalogue["vel"])
    counts, moments = gpu(catalogue["pos"], centre, radius, edges, boxsize=L, vel=catalogue["vel"], cell_cap=cap)
    npt.assert_array_equal(counts, ref_c)
    assert_moments(moments, ref_m, scale)
    monkeypatch.setenv("ASTRILD_PROFILE3D_CELLS", "0")
    one_c, one_m = gpu(catalogue["pos"], centre, radius, edges, boxsize=L, vel=catalogue["vel"], cell_cap=cap)
    assert counts[0, -1] == one_c[0, -1] and counts.sum() == one_c.sum() > 1000
    assert_moments(moments, one_m, scale)


def test_load_split(catalogue, monkeypatch):
    """299 small centres and one of 100 times the radius: with and without the split into runs of z layers."""
    radii = np.full(300, 0.8)
    radii[137] = 80.0
    args = (catalogue["pos"], catalogue["centres"], radii, EDGES)
    kw = dict(boxsize=L, **catalogue["kw"]["all"])
    ref_c, ref_m, scale = orc.profiles(*args, **kw)
    monkeypatch.setenv("ASTRILD_PROFILE3D_LAYERS", "1")
    split_c, split_m = gpu(*args, **kw)
    monkeypatch.setenv("ASTRILD_PROFILE3D_LAYERS", "0")
    whole_c, whole_m = gpu(*args, **kw)
    npt.assert_array_equal(split_c, whole_c)
    npt.assert_array_equal(split_c, ref_c)
    assert_moments(split_m, whole_m, scale)
    assert_moments(split_m, ref_m, scale)
    assert ref_c[137].sum() > NP // 10 and ref_c[137].sum() > 20 * np.delete(ref_c.sum(axis=1), 137).max()


# ---------------------------------------------------------------- membership mode
@pytest.fixture(scope="module")
def haloes():
    """Five haloes' members in one coordinate array, with gaps between the segments: an empty halo, one longer than a
    chunk of members, one straddling a face of a box of 100."""
    rng = np.random.default_rng(41)
    n_members = [700, 0, 20000, 1500, 3000]
    halo_pos = np.array([[20.0, 30.0, 40.0], [50.0, 50.0, 50.0], [70.0, 20.0, 60.0], [99.5, 0.3, 50.0], [10.0, 80.0, 5.0]])
    r200 = np.array([1.5, 1.0, 2.5, 1.2, 0.9])
    blocks, offsets, o = [], [], 0
    for k, n in enumerate(n_members):
        gap = rng.uniform(0.0, 100.0, (int(rng.integers(1, 50)), 3))
        blocks += [gap, halo_pos[k] + rng.normal(0.0, 0.5 * r200[k], (n, 3))]
        offsets.append(o + len(gap))
        o += len(gap) + n
    coords = np.concatenate(blocks)
    vel = rng.normal(0.0, 200.0, coords.shape)
    return {"coords": coords, "vel": vel, "halo_pos": halo_pos, "r200": r200, "N": np.array(n_members),
            "cum": np.array(offsets), "halo_vel": rng.normal(0.0, 100.0, (5, 3))}


def test_membership_equals_the_references_histogram(hip, haloes):
    from astrild_amd.profiles import Profiles3D
    from astrild_amd.profiles.profile_3d import bin_volumes, log_bins
    assert haloes["N"].max() > hip.ast_profile3d_chunk() and 0 in haloes["N"]
    prof = Profiles3D(haloes["coords"], haloes["halo_pos"], haloes["r200"], haloes["N"], haloes["cum"], Mpart=3.5)
    bins = log_bins(20)
    radii, values = prof.get_profiles("mass")
    _, counts = prof.get_profiles("count")
    npt.assert_array_equal(radii, 0.5 * (bins[1:] + bins[:-1]))
    assert counts.dtype == np.int64 and counts.shape == values.shape == (5, 20)
    for i in range(5):
        members = haloes["coords"][haloes["cum"][i]:haloes["cum"][i] + haloes["N"][i]]
        x = np.linalg.norm(members - haloes["halo_pos"][i], axis=1) / haloes["r200"][i]
        ref = np.histogram(x, bins=bins)[0]
        npt.assert_array_equal(counts[i], ref)
        npt.assert_array_equal(values[i], ref * 3.5 / bin_volumes(bins))
        one_r, one_v = prof.get_one_profile(i)
        lit_r, lit_v = Profiles3D.from_particle_data(x, 0, 3.5, "mass", 20)
        npt.assert_array_equal(one_v, lit_v)
        npt.assert_array_equal(one_r, lit_r)
    assert counts[1].sum() == 0 and counts[2].sum() > 10000
    r7, v7 = prof.get_one_profile(2, nbins=7)
    assert r7.shape == v7.shape == (7,)
    npt.assert_array_equal(v7, np.histogram(np.linalg.norm(
        haloes["coords"][haloes["cum"][2]:haloes["cum"][2] + 20000] - haloes["halo_pos"][2], axis=1) / 2.5,
        bins=log_bins(7))[0] * 3.5 / bin_volumes(log_bins(7)))


def test_membership_moments_and_the_default_offsets(haloes):
    """Velocity moments in membership mode against the oracle; cum_N_particles=None means contiguous segments."""
    seg = np.stack([haloes["cum"], haloes["N"]], axis=1)
    kw = dict(vel=haloes["vel"], centre_vel=haloes["halo_vel"], segments=seg)
    ref_c, ref_m, scale = orc.profiles(haloes["coords"], haloes["halo_pos"], haloes["r200"], EDGES, **kw)
    counts, moments = gpu(haloes["coords"], haloes["halo_pos"], haloes["r200"], EDGES, **kw)
    npt.assert_array_equal(counts, ref_c)
    assert_moments(moments, ref_m, scale)
    from astrild_amd.profiles import Profiles3D
    from astrild_amd.profiles.profile_3d import log_bins
    n = np.array([100, 0, 900])
    prof = Profiles3D(haloes["coords"][:1000], haloes["halo_pos"][:3], haloes["r200"][:3], n, velocities=haloes["vel"][:1000])
    assert prof.cum_N_particles.tolist() == [0, 100, 100]
    _, sig = prof.get_profiles("velocity dispersion", nbins=4, min_rad=0.1, max_rad=50.0)
    c2, m2, _ = orc.profiles(haloes["coords"][:1000], haloes["halo_pos"][:3], haloes["r200"][:3],
                             log_bins(4, 0.1, 50.0), vel=haloes["vel"][:1000],
                             segments=[(0, 100), (100, 0), (100, 900)])
    with np.errstate(invalid="ignore"):
        npt.assert_allclose(sig, np.sqrt(m2[..., 3] / m2[..., 0]), rtol=1e-9)
    assert np.all(np.isnan(sig[1])) and np.isfinite(sig[0]).any() and np.isfinite(sig[2]).any()


def test_membership_across_a_face_equals_the_search_on_the_members(haloes):
    i = 3
    members = np.mod(haloes["coords"][haloes["cum"][i]:haloes["cum"][i] + haloes["N"][i]], 100.0)
    assert (members[:, 0] < 5).any() and (members[:, 0] > 95).any() and (members[:, 1] > 95).any()
    coords = np.mod(haloes["coords"], 100.0)
    seg = np.stack([haloes["cum"], haloes["N"]], axis=1)
    kw = dict(boxsize=100.0, vel=haloes["vel"])
    mem_c, mem_m = gpu(coords, haloes["halo_pos"], haloes["r200"], EDGES, segments=seg, **kw)
    sea_c, sea_m = gpu(members, haloes["halo_pos"][i:i + 1], haloes["r200"][i:i + 1], EDGES, boxsize=100.0,
                       vel=haloes["vel"][haloes["cum"][i]:haloes["cum"][i] + haloes["N"][i]])
    ref_c, ref_m, scale = orc.profiles(coords, haloes["halo_pos"], haloes["r200"], EDGES, segments=seg, **kw)
    npt.assert_array_equal(mem_c, ref_c)
    npt.assert_array_equal(mem_c[i], sea_c[0])
    assert sea_c.sum() > 1000
    assert_moments(mem_m[i], sea_m[0], scale[i])
    open_c, _ = gpu(coords, haloes["halo_pos"], haloes["r200"], EDGES, segments=seg)
    assert open_c[i].sum() < mem_c[i].sum()


# ---------------------------------------------------------------- empty and degenerate inputs
def test_empty_and_degenerate_inputs(catalogue):
    from astrild_amd.profiles import radial_profiles
    pos = catalogue["pos"]
    c, m = gpu(pos, np.zeros((0, 3)), np.zeros(0), EDGES, boxsize=L)
    assert c.shape == (0, 20) and m.shape == (0, 20, 1) and c.dtype == np.int64
    c, m = gpu(np.zeros((0, 3)), catalogue["centres"], catalogue["radii"], EDGES, boxsize=L, vel=np.zeros((0, 3)))
    assert c.shape == (300, 20) and m.shape == (300, 20, 4) and not c.any() and not m.any()
    # a centre with nothing in reach, periodic and open (there: also far outside the particles' bounding box)
    far = np.array([[250.0, 250.0, 250.0], [3000.0, -2000.0, 250.0]])
    lone = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    for box, centres in ((L, far[:1]), (None, far)):
        out = radial_profiles(lone, centres, np.ones(len(centres)), EDGES, boxsize=box, vel=np.ones((2, 3)))
        assert not out["counts"].any() and not out["mass"].any() and not out["density"].any()
        for key in ("v_r", "sigma_r", "sigma_3d"):
            assert out[key].shape == (len(centres), 20) and np.all(np.isnan(out[key]))
    # all particles in one cell: one point many times, periodic and open (a bounding box without extent)
    same = np.tile([[123.0, 45.0, 67.0]], (5000, 1))
    for box in (L, None):
        c, m = gpu(same, [[123.0, 45.0, 67.0], [124.0, 45.0, 67.0], [200.0, 45.0, 67.0]], [1.0, 2.0, 1.0], [0.0, 0.5, 1.0],
                   boxsize=box)
        assert c.tolist() == [[5000, 0], [0, 5000], [0, 0]]
        npt.assert_array_equal(m[..., 0], c)
    # radial_profiles' dict
    out, counts, moments = radial_profiles(pos, catalogue["centres"][:5], catalogue["radii"][:5], EDGES, boxsize=L,
                                           weights=catalogue["weights"], vel=catalogue["vel"], return_counts=True)
    npt.assert_array_equal(counts, catalogue["ref"]["plain"][0][:5])
    npt.assert_array_equal(out["radii"], 0.5 * (EDGES[1:] + EDGES[:-1]))
    npt.assert_array_equal(out["mass"], moments[..., 0])
    npt.assert_array_equal(out["density"], moments[..., 0] / (4.0 / 3.0 * np.pi * (EDGES[1:] ** 3 - EDGES[:-1] ** 3)))
    full = counts > 0
    npt.assert_array_equal(out["v_r"][full], moments[..., 1][full] / moments[..., 0][full])
    assert np.all(out["sigma_3d"][full] >= out["sigma_r"][full] * (1 - 1e-12)) and np.all(np.isnan(out["v_r"][~full]))


# ---------------------------------------------------------------- argument checks
def test_errors_and_a_valid_call_after_each(catalogue):
    pos, centres, radii = catalogue["pos"][:2000], catalogue["centres"][:4], catalogue["radii"][:4]
    good = lambda: gpu(pos, centres, radii, EDGES, boxsize=L)[0]
    first = good()
    bad = [
        dict(pos=pos[:, :2]), dict(weights=np.ones(1999)), dict(vel=np.ones((2000, 2))), dict(edges=[1.0]),
        dict(edges=[0.0, 2.0, 1.0]), dict(edges=[-1.0, 1.0]), dict(edges=[0.0, np.nan]), dict(centres=centres[:, :2]),
        dict(radii=radii[:3]), dict(radii=[1.0, 0.0, 1.0, 1.0]), dict(radii=[1.0, np.inf, 1.0, 1.0]),
        dict(radii=[1.0, np.nan, 1.0, 1.0]), dict(centre_vel=np.zeros((4, 3))),
        dict(vel=np.ones((2000, 3)), centre_vel=np.zeros((3, 3))), dict(boxsize=-1.0),
        dict(edges=[0.0, 2.0], radii=[1.0, 1.0, 1.0, L / 4.0]),                     # reach 2 R = L / 2 exactly
        dict(segments=[(0, 10), (10, 10), (20, 1981), (0, 0)]), dict(segments=[(0, 10), (-1, 10), (20, 10), (0, 0)]),
        dict(segments=[(0, 10)]),
        dict(pos=pos + 1.0), dict(pos=pos - 1.0), dict(pos=np.where(np.arange(2000)[:, None] == 7, np.nan, pos)),
        dict(boxsize=None, pos=np.where(np.arange(2000)[:, None] == 7, np.inf, pos)),
        dict(boxsize=None, pos=np.where(np.arange(2000)[:, None] == 1999, np.nan, pos), segments=[(0, 10)] * 4),
    ]
    for change in bad:
        kw = {"pos": pos, "centres": centres, "radii": radii, "edges": EDGES, "boxsize": L, **change}
        args = [kw.pop(k) for k in ("pos", "centres", "radii", "edges")]
        with pytest.raises(ValueError):
            gpu(*args, **kw)
        npt.assert_array_equal(good(), first)
    assert (pos + 1.0).max() > L and (pos - 1.0).min() < 0.0


# ---------------------------------------------------------------- dirty memory, call order, repeats
@pytest.fixture(scope="module")
def clean_runs(catalogue, haloes):
    """Solo runs on clean memory: (arguments, keyword arguments, result) of a periodic search with multi-item centres,
    an open search and a membership call with a multi-chunk halo, each of another size."""
    radii = catalogue["radii"].copy()
    radii[::50] = np.minimum(6.0 * radii[::50], 80.0)
    runs = {"periodic": ((catalogue["pos"], catalogue["centres"], radii, EDGES), dict(boxsize=L, **catalogue["kw"]["all"])),
            "open": ((catalogue["pos"][:7001], catalogue["centres"][:120], radii[:120], EDGES[:12]),
                     dict(weights=catalogue["weights"][:7001])),
            "members": ((haloes["coords"], haloes["halo_pos"], haloes["r200"], EDGES[3:]),
                        dict(vel=haloes["vel"], segments=np.stack([haloes["cum"], haloes["N"]], axis=1)))}
    out = {}
    for name, (args, kw) in runs.items():
        ref = orc.profiles(*args, **kw)
        got = gpu(*args, **kw)
        npt.assert_array_equal(got[0], ref[0])
        out[name] = (args, kw, got, ref[2])
    return out


@pytest.mark.parametrize("name", ["periodic", "open", "members"])
def test_dirty_scratch_gives_the_clean_result(clean_runs, dirty_alloc, name):
    args, kw, (clean_c, clean_m), scale = clean_runs[name]
    mark = dirty_alloc.mark()
    counts, moments = gpu(*args, **kw)
    assert dirty_alloc.since(mark) >= 4                  # workspace, bounds, counts, moments
    npt.assert_array_equal(counts, clean_c)
    assert_moments(moments, clean_m, scale)


def test_interleaved_calls_equal_their_solo_runs(clean_runs, dirty_alloc):
    from astrild_amd import device as dev
    order = ["periodic", "members", "open", "members", "periodic", "open"]
    results = [dev.sphere_profiles(*clean_runs[n][0], **clean_runs[n][1]) for n in order]
    for n, (counts, moments) in zip(order, results):
        _, _, (clean_c, clean_m), scale = clean_runs[n]
        npt.assert_array_equal(dev.to_numpy(counts), clean_c)
        assert_moments(dev.to_numpy(moments), clean_m, scale)


def test_repeated_calls(clean_runs):
    """Counts are bit-identical; the moments differ at most by the order of the LDS additions inside a bin:
    4 n_bin eps sum|term|."""
    for name, (args, kw, (c1, m1), scale) in clean_runs.items():
        c2, m2 = gpu(*args, **kw)
        npt.assert_array_equal(c2, c1)
        bound = 4.0 * c1[..., None] * EPS * scale
        print(name, "max |m2 - m1| / bound =", np.max(np.abs(m2 - m1) / np.where(bound > 0, bound, 1.0)))
        assert np.all(np.abs(m2 - m1) <= bound)
