"""GPU: the periodic two-point correlation function (ast_tpcf_prepare / ast_tpcf_pair_counts through
device.tpcf_pair_counts and astrild_amd.particles.hutils.tpcf): lattice known answers, int64 pair counts exactly equal
to the numpy oracle (tests/tpcf_oracle.py), pairs across every face, edge and corner of the box, xi and its multipoles
against the oracle's, the grid against one cell, and the input edge cases."""
import itertools

import numpy as np
import numpy.testing as npt
import pytest

from tests import pair_geometry as pg
from tests import tpcf_oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LAT_S = [0.5, 1.2, 1.6, 1.9, 2.1, 2.5]
LAT_MU = [0.0, 0.25, 0.6, 0.8, 1.0]
L = 500.0
S50 = np.linspace(0.0, 50.0, 40)
MU40 = np.sort(1.0 - np.geomspace(0.001, 1.0, 40))


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


def gpu_counts(pos, boxsize, s_edges, mu_edges=None, vel=None, los=2):
    from astrild_amd import device as dev
    return dev.to_numpy(dev.tpcf_pair_counts(pos, boxsize, s_edges, mu_edges=mu_edges, vel=vel, los=los))


def oracle_counts(pos, boxsize, s_edges, mu_edges=None, vel=None, los=2):
    return orc.pair_counts(orc.shift_and_wrap(pos, vel, boxsize, los), boxsize, s_edges, mu_edges, los=los)


@pytest.mark.parametrize("cells", ["1", "0"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lattice_known_answer(dtype, cells, monkeypatch):
    monkeypatch.setenv("ASTRILD_TPCF_CELLS", cells)
    pos = orc.lattice(16).astype(dtype)
    for los in (0, 1, 2):
        exp = orc.lattice_expected(16, LAT_S, LAT_MU, los, 2.5)
        got = gpu_counts(pos, 16.0, LAT_S, LAT_MU, los=los)
        npt.assert_array_equal(got, exp)
        assert got[4].tolist() == [0, (8 + 16) * 2048, 0, (8 + 8) * 2048]   # |m|^2 = 5 and 6
    npt.assert_array_equal(gpu_counts(pos, 16.0, LAT_S), orc.lattice_expected(16, LAT_S, LAT_MU, 2, 2.5).sum(axis=1)
                           + 2048 * np.array([4, 4, 0, 4, 8]))             # + the mu = 0 vectors: |m|^2 = 1, 2, 4, 5


@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_catalogues_equal_the_oracle(kind):
    pos = orc.uniform(20_000, L, 1) if kind == "uniform" else orc.clustered(20_000, L, 2, blobs=60, sigma=6.0)
    got = gpu_counts(pos, L, S50, MU40)
    npt.assert_array_equal(got, oracle_counts(pos, L, S50, MU40))
    assert got.sum() > 100_000


def test_edges_and_real_space():
    pos = orc.clustered(20_000, L, 3, blobs=100, sigma=10.0)
    uneven_s = np.array([0.0, 0.3, 1.0, 2.2, 5.0, 11.0, 12.0, 30.0, 33.0, 70.0, 166.0])
    uneven_mu = np.array([0.0, 0.05, 0.4, 0.41, 0.9, 0.97, 1.0])
    npt.assert_array_equal(gpu_counts(pos, L, uneven_s, uneven_mu, los=1),
                           oracle_counts(pos, L, uneven_s, uneven_mu, los=1))
    s40 = np.linspace(0.1, 60.0, 40)                                      # the reference's tuple defaults
    npt.assert_array_equal(gpu_counts(pos, L, s40, MU40), oracle_counts(pos, L, s40, MU40))
    real = gpu_counts(pos, L, uneven_s)
    assert real.shape == (10,)
    npt.assert_array_equal(real, oracle_counts(pos, L, uneven_s))


@pytest.mark.parametrize("pdt,vdt", list(itertools.product([np.float32, np.float64], repeat=2)))
def test_velocities_wrap_in_every_dtype(pdt, vdt):
    rng = np.random.default_rng(5)
    pos = orc.uniform(8000, L, 6).astype(pdt)
    vel = rng.normal(0.0, 3000.0, (8000, 3)).astype(vdt)           # shifts of up to ~100 Mpc/h cross the faces
    for los in (0, 2):
        shifted = orc.shift_and_wrap(pos, vel, L, los)
        raw = pos[:, los].astype(np.float64) + vel[:, los] / 100.0
        assert np.sum((raw > L) | (raw < 0)) > 100                    # the wrap is exercised
        npt.assert_array_equal(gpu_counts(pos, L, S50, MU40, vel=vel, los=los),
                               orc.pair_counts(shifted, L, S50, MU40, los=los))


@pytest.mark.parametrize("cells", ["1", "0"])
def test_pairs_across_every_face_edge_and_corner(cells, monkeypatch):
    monkeypatch.setenv("ASTRILD_TPCF_CELLS", cells)
    box = 10.0
    s = np.array([0.0, 0.6, 1.0, 1.4, 2.0, 3.0])
    mu = np.array([0.0, 0.3, 0.6, 0.9, 1.0])
    sep = np.array([0.5, 0.75, 1.25])                                 # per-axis separations, exact in binary
    s2 = s * s
    for o in itertools.product((-1, 0, 1), repeat=3):
        if o == (0, 0, 0):
            continue
        a = np.array([sep[k] if o[k] else 0.0 for k in range(3)])
        # object A within 0.25 of the face on each axis of o (the high face for +1, the low one for -1), B across it
        pa = np.array([box - 0.25 if o[k] > 0 else (0.25 if o[k] < 0 else 5.0) for k in range(3)])
        pb = np.array([(pa[k] + o[k] * a[k]) % box for k in range(3)])
        pos = np.stack([pa, pb])
        d2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
        for los in (0, 2):
            exp = np.zeros((5, 4), dtype=np.int64)
            m = a[los] / np.sqrt(d2)
            k = np.searchsorted(s2, d2, side="left") - 1
            if m > 0:
                exp[k, np.searchsorted(mu, m, side="left") - 1] = 1
            got = gpu_counts(pos, box, s, mu, los=los)
            npt.assert_array_equal(got, exp, err_msg=f"offset {o}, los {los}")
            npt.assert_array_equal(gpu_counts(pos.astype(np.float32), box, s, mu, los=los), exp)
            assert got.sum() == (1 if m > 0 else 0)


def test_xi_and_multipoles_equal_the_oracle_formula():
    from astrild_amd.particles.hutils import TPCF, tpcf_multipole, tpcf_r
    pos = orc.clustered(20_000, L, 7, blobs=80, sigma=8.0)
    vel = np.random.default_rng(8).normal(0.0, 400.0, pos.shape)
    s, mu, xi, dd = TPCF.compute(pos, vel, L, "redshift", (0.1, 60.0), (0.001, 1.0), return_counts=True)
    s_e = np.linspace(0.1, 60.0, 40)
    ref = oracle_counts(pos, L, s_e, MU40, vel=vel)
    npt.assert_array_equal(dd, ref)
    npt.assert_array_equal(mu, MU40)
    npt.assert_allclose(xi, orc.xi(ref, len(pos), L, s_e, MU40), rtol=1e-12)
    xs = TPCF.tpcf_s(pos, vel, s_e, MU40, 2, L)
    npt.assert_allclose(xs, orc.xi(ref, len(pos), L, s_e, MU40), rtol=1e-12)
    for order in (0, 2, 4):
        npt.assert_allclose(tpcf_multipole(xi, mu, order), orc.multipole(orc.xi(ref, len(pos), L, s_e, MU40), mu, order),
                            rtol=1e-12, atol=1e-12)
    r = np.geomspace(0.5, 80.0, 25)
    xr, ddr = tpcf_r(pos, r, L, estimator="Landy-Szalay", return_counts=True)
    rref = orc.pair_counts(pos, L, r)
    npt.assert_array_equal(ddr, rref)
    npt.assert_allclose(xr, orc.xi(rref, len(pos), L, r), rtol=1e-12)
    assert xr[0] > 10.0                                                # clustered: strong small-scale signal


def test_grid_equals_single_cell(monkeypatch):
    pos = orc.clustered(200_000, 1000.0, 9, blobs=500, sigma=10.0)
    s = np.linspace(0.0, 100.0, 40)
    grid = gpu_counts(pos, 1000.0, s, MU40)
    monkeypatch.setenv("ASTRILD_TPCF_CELLS", "0")
    single = gpu_counts(pos, 1000.0, s, MU40)
    npt.assert_array_equal(grid, single)
    assert grid.sum() > 10_000_000


@pytest.mark.parametrize("case", list(pg.PERIODIC_CASES))
def test_tpcf_plans_the_intended_grid(case, hip):
    """ast_tpcf_prepare + ast_tpcf_pair_counts called directly: the GridBoxParams at the head of the workspace is the
    periodic plan that tests/pair_geometry.py restates (dims, ncells, lo = 0, inv_cs = d / L bit for bit, ntiles), so
    that a case which silently collapsed to one cell would be noticed, and the counts are the oracle's."""
    from astrild_amd import _lib, device as dev
    top, n, single, d = pg.PERIODIC_CASES[case]
    box = pg.PERIODIC_L
    pos = orc.uniform(n, box, 21)
    s_edges, mu_edges = np.linspace(0.0, top, 6), np.array(LAT_MU)
    ns, nmu = len(s_edges) - 1, len(mu_edges) - 1
    p, s_d, mu_d = dev.as_device(pos), dev.as_device(s_edges), dev.as_device(mu_edges)
    ws_bytes = hip.ast_tpcf_workspace_bytes(n, ns, nmu)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    bounds = torch.empty(6, dtype=torch.float64, device="cuda")
    st = dev.stream()
    _lib.check(hip.ast_tpcf_prepare(dev.ptr(p), _lib.F64, None, _lib.F64, 2, box, n, dev.ptr(work), ws_bytes,
                                    dev.ptr(bounds), st), "ast_tpcf_prepare")
    counts = torch.full((ns, nmu), -1, dtype=torch.int64, device="cuda")
    _lib.check(hip.ast_tpcf_pair_counts(dev.ptr(work), ws_bytes, n, box, 2, dev.ptr(s_d), ns, dev.ptr(mu_d), nmu,
                                        int(single), dev.ptr(counts), st), "ast_tpcf_pair_counts")
    torch.cuda.synchronize()
    got, want = pg.parse_grid_params(work[:128].cpu().numpy()), pg.plan_periodic(pos, box, top, single)
    assert want.dims.tolist() == [d, d, d]
    assert got["dims"].tolist() == [d, d, d]
    assert got["ncells"] == d ** 3
    assert got["ntiles"] == pg.tiles(want)
    npt.assert_array_equal(got["lo"], np.zeros(3))
    npt.assert_array_equal(got["inv_cs"], np.full(3, d / box if d > 1 else 0.0))
    npt.assert_array_equal(got["inv_cs"], want.inv_cs)
    ref = orc.pair_counts(pos, box, s_edges, mu_edges, los=2)
    assert ref.sum() > 0
    npt.assert_array_equal(counts.cpu().numpy(), ref)


def test_counts_survive_lds_flushes(monkeypatch):
    # AST_TPCF_FLUSH_AT=0 flushes the 32-bit LDS counters into the 64-bit workgroup rows before every stage
    pos = orc.clustered(20_000, L, 10, blobs=40, sigma=5.0)
    ref = gpu_counts(pos, L, S50, MU40)
    monkeypatch.setenv("AST_TPCF_FLUSH_AT", "0")
    npt.assert_array_equal(gpu_counts(pos, L, S50, MU40), ref)
    monkeypatch.setenv("ASTRILD_TPCF_CELLS", "0")
    npt.assert_array_equal(gpu_counts(pos, L, S50, MU40), ref)


def test_max_bins_and_repeat_stability():
    from astrild_amd import device as dev
    from astrild_amd import _lib
    assert _lib.lib().ast_tpcf_max_bins() >= 100 * 100
    pos = orc.clustered(20_000, L, 11, blobs=60, sigma=6.0)
    s, mu = np.linspace(0.0, 60.0, 101), np.linspace(0.0, 1.0, 101)
    a = gpu_counts(pos, L, s, mu)
    b = gpu_counts(pos, L, s, mu)
    npt.assert_array_equal(a, b)
    npt.assert_array_equal(a, oracle_counts(pos, L, s, mu))
    with pytest.raises(ValueError):
        dev.tpcf_pair_counts(pos, L, np.linspace(0.0, 60.0, 102), mu)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_tensor_inputs(dtype):
    pos = orc.uniform(10_000, L, 12).astype(dtype)
    vel = np.random.default_rng(13).normal(0.0, 500.0, pos.shape).astype(dtype)
    host = gpu_counts(pos, L, S50, MU40, vel=vel)
    dev_in = gpu_counts(torch.from_numpy(pos).cuda(), L, S50, MU40, vel=torch.from_numpy(vel).cuda())
    npt.assert_array_equal(dev_in, host)
    npt.assert_array_equal(host, oracle_counts(pos, L, S50, MU40, vel=vel))


@pytest.mark.parametrize("n", [0, 1])
def test_fewer_than_two_objects(n):
    from astrild_amd.particles.hutils import TPCF
    pos = np.full((n, 3), 10.0)
    got = gpu_counts(pos, L, S50, MU40, vel=np.zeros((n, 3)))
    assert got.shape == (39, 39) and not got.any()
    _, _, _, dd = TPCF.compute(pos, np.zeros((n, 3)), L, "redshift", (0.1, 50.0), (0.001, 1.0), return_counts=True)
    assert dd.shape == (39, 39) and not dd.any()
    torch.cuda.synchronize()


def test_out_of_box_positions_raise_from_the_device_bounds():
    pos = orc.uniform(1000, L, 14)
    bad = pos.copy()
    bad[17, 1] = L + 0.5
    with pytest.raises(ValueError, match="must lie in"):
        gpu_counts(bad, L, S50, MU40)
    bad = pos.copy()
    bad[3, 0] = -1e-9
    with pytest.raises(ValueError, match="must lie in"):
        gpu_counts(bad, L, S50)
    bad = pos.copy()
    bad[5, 2] = np.nan
    with pytest.raises(ValueError, match="must lie in"):
        gpu_counts(bad, L, S50)
    vel = np.zeros_like(pos)
    vel[9, 2] = 200.0 * L                                             # shifted by 2 L: one wrap is not enough
    with pytest.raises(ValueError, match="must lie in"):
        gpu_counts(pos, L, S50, MU40, vel=vel)
    edge = pos.copy()
    edge[0] = [0.0, L, L]                                              # on the faces: allowed, as halotools does
    npt.assert_array_equal(gpu_counts(edge, L, S50, MU40), oracle_counts(edge, L, S50, MU40))
