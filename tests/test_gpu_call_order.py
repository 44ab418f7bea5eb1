"""GPU: state that survives a call.  Long-lived objects and caches - SmoothPlan's weights and scratch shared by three
routes, LensPlan's lazily built kernel spectra, the host ABI's global plan, the pair finders' prepared workspaces, the
cached fused-power scratch, the per-n twiddle / lane / disc tables, StagedPaint's workspace - are used more than once
here, in an order no other test uses, and every result must be bit-identical (``torch.equal``) to the one a fresh
object, or the first call, gives.

This is also the only way the suite reaches memory the library allocates itself with hipMalloc (plan internals,
twiddle tables, side-stream scratch): tests/dirty_memory.py cannot poison what never passes through torch.
"""
import ctypes as ct

import numpy as np
import numpy.testing as npt
import pytest

from oracle import kappa as ok
from tests import pairwise_oracle as tv_orc
from tests import tpcf_oracle as tpcf_orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def dev(hip):
    from astrild_amd import device
    return device


@pytest.fixture(scope="module")
def lens(hip):
    from astrild_amd import lensing
    return lensing


# ------------------------------------------------------------------ SmoothPlan
SMOOTH_CALLS = [("gaussianFFT", 3.0),          # the periodic real-space route
                ("gaussian", 1.2),             # scipy's reflect route: overwrites the cached weights
                ("gaussianFFT", 3.0),
                ("gaussianFFT", 1.0),          # below 2.5 px: the true FFT route
                ("gaussianFFT", 7.5),
                ("gaussianFFT", 3.0),
                ("gaussian_mirror", 1.5)]      # what resize_antialiased runs through a plan of this size (96 -> 24: 1.5)


@pytest.mark.parametrize("npix", [256, 64])
def test_smooth_plan_routes_in_sequence_equal_fresh_plans(dev, lens, npix):
    """npix = 64: the real-space routes' 1024-pixel line laps the map."""
    img = dev.as_device(np.random.default_rng(npix).standard_normal((npix, npix)))
    fresh = []
    for kind, sigma in SMOOTH_CALLS:
        t = img.clone()
        lens.SmoothPlan(npix).gaussian(t, sigma, kind)
        fresh.append(t)
    assert not torch.equal(fresh[0], fresh[3]) and not torch.equal(fresh[0], fresh[4])
    plan = lens.SmoothPlan(npix)
    for step, (kind, sigma) in enumerate(SMOOTH_CALLS):
        t = img.clone()
        plan.gaussian(t, sigma, kind)
        assert bool(torch.isfinite(t).all())
        assert torch.equal(t, fresh[step]), (npix, step, kind, sigma)


def test_resize_antialiased_after_other_uses_of_the_cached_plan(dev, lens):
    img = np.random.default_rng(96).standard_normal((96, 96))
    first = lens.resize_antialiased(img, 24)
    t = dev.as_device(img.copy())
    lens.smooth_plan(96).gaussian(t, 3.0, "gaussianFFT")
    lens.smooth_plan(96).gaussian(t, 1.2, "gaussian")
    assert torch.equal(lens.resize_antialiased(img, 24), first)
    want = ok.resize_antialiased(img, 24)
    npt.assert_allclose(first.cpu().numpy(), want, rtol=0, atol=1e-13 * np.abs(want).max())


# ------------------------------------------------------------------ LensPlan
@pytest.mark.parametrize("nc", [128, 100], ids=["hand_written_128", "embedded_100"])
def test_lens_plan_alphas_phi_alphas(dev, lens, nc):
    """The kernel spectra are built lazily into a buffer that is also the inverse passes' output."""
    bsz = np.deg2rad(3.0)
    kappa = np.random.default_rng(nc).standard_normal((nc, nc)) * 0.01
    kd = dev.as_device(kappa)
    plan = lens.LensPlan(nc, bsz)
    a1, a2 = plan.alphas(kd)
    phi = plan.phi(kd)
    b1, b2 = plan.alphas(kd)
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    assert torch.equal(lens.LensPlan(nc, bsz).phi(kd), phi)             # phi first, on a fresh plan
    phi_then = lens.LensPlan(nc, bsz)
    p0 = phi_then.phi(kd)
    c1, c2 = phi_then.alphas(kd)
    assert torch.equal(p0, phi) and torch.equal(c1, a1) and torch.equal(c2, a2)
    rp = ok.kappa0_to_phi(kappa, nc, bsz)
    npt.assert_allclose(phi.cpu().numpy(), rp, rtol=0, atol=1e-10 * abs(rp).max())


def test_host_abi_replaces_its_global_plan(hip):
    """kappa0_to_alphas / kappa0_to_phi keep ONE plan keyed by (Nc, bsz): (64, a), then (100, b), then (64, a) again."""
    own = ct.CDLL(hip._name)
    dbl = np.ctypeslib.ndpointer(dtype=ct.c_double)
    fa, fp = own.kappa0_to_alphas, own.kappa0_to_phi
    fa.restype = fp.restype = ct.c_void_p
    fa.argtypes = [dbl, ct.c_int, ct.c_double, dbl, dbl]
    fp.argtypes = [dbl, ct.c_int, ct.c_double, dbl]

    def alphas(kappa, nc, bsz):
        a1, a2 = np.zeros((nc, nc)), np.zeros((nc, nc))
        fa(kappa, nc, bsz, a1, a2)
        return a1, a2

    def phi(kappa, nc, bsz):
        out = np.zeros((nc, nc))
        fp(kappa, nc, bsz, out)
        return out
    rng = np.random.default_rng(4)
    k64, k100 = rng.standard_normal((64, 64)) * 0.01, rng.standard_normal((100, 100)) * 0.01
    bsz_a, bsz_b = np.deg2rad(3.0), np.deg2rad(7.0)
    first = alphas(k64, 64, bsz_a)
    other = alphas(k100, 100, bsz_b)
    third = alphas(k64, 64, bsz_a)
    assert np.array_equal(first[0], third[0]) and np.array_equal(first[1], third[1])
    for got, ref in zip(first + other, ok.kappa0_to_alphas(k64, 64, bsz_a) + ok.kappa0_to_alphas(k100, 100, bsz_b)):
        npt.assert_allclose(got, ref, rtol=0, atol=1e-10 * abs(ref).max())
    # phi right after the plan was replaced (the 64 plan is resident), and once more with another opening angle
    for kappa, nc, bsz in ((k100, 100, bsz_b), (k64, 64, bsz_b), (k64, 64, bsz_a)):
        rp = ok.kappa0_to_phi(kappa, nc, bsz)
        npt.assert_allclose(phi(kappa, nc, bsz), rp, rtol=0, atol=1e-10 * abs(rp).max())
    again = alphas(k64, 64, bsz_a)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


# ------------------------------------------------------------------ pair finders at the C ABI
from tests import test_gpu_pairwise as t_tv                        # noqa: E402
from tests import test_gpu_pairwise_pdf as t_pdf                   # noqa: E402


def test_pairwise_tv_one_prepare_three_pair_calls(dev, hip):
    from astrild_amd import _lib
    pos, _ = tv_orc.light_cone(4000, seed=9, clusters=200, sigma=6.0)
    vel = t_tv.coherent_velocities(pos, 2)
    n = len(pos)
    p, v = dev.as_device(pos), dev.as_device(vel)
    ws_bytes = hip.ast_pairwise_workspace_bytes(n, 40)
    assert ws_bytes >= hip.ast_pairwise_workspace_bytes(n, 10) > 0
    work = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    s = dev.stream()
    _lib.check(hip.ast_pairwise_tv_prepare(dev.ptr(p), _lib.F64, dev.ptr(v), _lib.F64, 2, None, None, 0, n, dev.ptr(work),
                                           ws_bytes, s), "ast_pairwise_tv_prepare")
    settings = [(40, 50.0 / 39, 0), (10, 2.5, 1), (40, 50.0 / 39, 0)]
    counts = []
    for binnr, bw, single in settings:
        nom = torch.full((binnr,), float("nan"), dtype=torch.float64, device="cuda")
        den = torch.full((binnr,), float("nan"), dtype=torch.float64, device="cuda")
        cnt = torch.full((binnr,), -1, dtype=torch.int64, device="cuda")
        _lib.check(hip.ast_pairwise_tv(dev.ptr(work), ws_bytes, n, binnr, bw, single, dev.ptr(nom), dev.ptr(den), dev.ptr(cnt), s),
                   "ast_pairwise_tv")
        got = (nom.cpu().numpy(), den.cpu().numpy(), cnt.cpu().numpy())
        ref = t_tv.oracle_sums(pos, vel, binnr, bw)
        assert ref[2].sum() > 1000
        t_tv.assert_same(got, ref)                                   # counts exact, sums within RTOL
        counts.append(got[2])
    assert np.array_equal(counts[0], counts[2])


def test_tpcf_one_prepare_three_pair_calls(dev, hip):
    from astrild_amd import _lib
    L = 500.0
    pos = tpcf_orc.clustered(5000, L, 2, blobs=30, sigma=6.0)
    n = len(pos)
    s_a, mu_a = np.linspace(0.0, 50.0, 40), np.sort(1.0 - np.geomspace(0.001, 1.0, 40))
    s_b, mu_b = np.array([0.0, 0.3, 1.0, 2.2, 5.0, 11.0, 12.0, 30.0]), np.array([0.0, 0.05, 0.4, 0.41, 0.9, 1.0])
    ws_bytes = hip.ast_tpcf_workspace_bytes(n, 39, 39)
    assert ws_bytes >= hip.ast_tpcf_workspace_bytes(n, 7, 5) > 0
    p = dev.as_device(pos)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    bounds = torch.empty(6, dtype=torch.float64, device="cuda")
    st = dev.stream()
    _lib.check(hip.ast_tpcf_prepare(dev.ptr(p), _lib.F64, None, _lib.F64, 2, L, n, dev.ptr(work), ws_bytes, dev.ptr(bounds), st),
               "ast_tpcf_prepare")
    results = []
    for s, mu, single in ((s_a, mu_a, 0), (s_b, mu_b, 1), (s_b, None, 0), (s_a, mu_a, 0)):
        ns, nmu = len(s) - 1, 0 if mu is None else len(mu) - 1
        s_d, mu_d = dev.as_device(s), None if mu is None else dev.as_device(mu)
        counts = torch.full((ns, nmu) if nmu else (ns,), -1, dtype=torch.int64, device="cuda")
        _lib.check(hip.ast_tpcf_pair_counts(dev.ptr(work), ws_bytes, n, L, 2, dev.ptr(s_d), ns, dev.ptr(mu_d), nmu, single,
                                            dev.ptr(counts), st), "ast_tpcf_pair_counts")
        ref = tpcf_orc.pair_counts(pos, L, s, mu)
        assert ref.sum() > 1000
        npt.assert_array_equal(counts.cpu().numpy(), ref)
        results.append(counts)
    assert torch.equal(results[0], results[3])


def test_pairwise_pdf_one_prepare_three_pair_calls(dev, hip):
    from astrild_amd import _lib
    pos, vel, par = t_pdf.catalogue("compact")
    n = len(pos)
    p, v = dev.as_device(pos), dev.as_device(vel)
    # (kind, dist_bin, vel_bin, dist_width, vel_width, single cell, histogram forced into global memory)
    settings = [("z_sign", 9, 40, 4.0, 1.0, 0, 0), ("radial", 9, 40, 2.5, 0.5, 1, 1), ("z_sign", 9, 40, 4.0, 1.0, 0, 0),
                ("radial", 9, 40, 4.0, 1.0, 0, 0)]
    ws_bytes = max(hip.ast_pairwise_pdf_workspace_bytes(n, db, vb, 1) for _, db, vb, *_ in settings)
    assert ws_bytes > 0 and 9 * 40 <= t_pdf.lds_bins(9, True)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    st = dev.stream()
    _lib.check(hip.ast_pairwise_pdf_prepare(dev.ptr(p), _lib.F64, dev.ptr(v), _lib.F64, n, dev.ptr(work), ws_bytes, st),
               "ast_pairwise_pdf_prepare")
    hists = []
    for kind, db, vb, dw, vw, single, force_global in settings:
        hist = torch.full((db, vb), -1, dtype=torch.int64, device="cuda")
        outside = torch.full((), -1, dtype=torch.int64, device="cuda")
        count = torch.full((db,), -1, dtype=torch.int64, device="cuda")
        s1 = torch.full((db,), float("nan"), dtype=torch.float64, device="cuda")
        s2 = torch.full((db,), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(hip.ast_pairwise_pdf(dev.ptr(work), ws_bytes, n, _lib.PVPDF_KIND[kind], par["r"], db, vb, dw, vw, 0, n, single,
                                        force_global, dev.ptr(hist), dev.ptr(outside), dev.ptr(s1), dev.ptr(s2), dev.ptr(count), st),
                   "ast_pairwise_pdf")
        got = dict(hist=hist.cpu().numpy(), outside=int(outside.item()), count=count.cpu().numpy(), s1=s1.cpu().numpy(),
                   s2=s2.cpu().numpy())
        ref = t_pdf.oracle("compact", kind, tuple(sorted(dict(dist_bin=db, vel_bin=vb, dist_width=dw, vel_width=vw).items())))
        assert ref["hist"].sum() > 0
        t_pdf.assert_same(got, ref)
        hists.append(got)
    assert np.array_equal(hists[0]["hist"], hists[2]["hist"]) and hists[0]["outside"] == hists[2]["outside"]
    assert np.array_equal(hists[0]["count"], hists[2]["count"])


# ------------------------------------------------------------------ the cached fused-power scratch and the per-n tables
def test_paint_power_1d_on_one_cached_scratch(dev):
    """CIC with the default binning, TSC under the other shell rule, CIC again: the first and the third are the same
    bits (test_repeated_fused_pipeline_calls_are_bit_identical establishes that repeats are)."""
    n, L = 256, 1000.0
    pos = dev.synth_lattice_particles(n, n, L, seed=11, dtype=torch.float32)
    first = dev.paint_power_1d(pos, None, n, L, "cic")
    assert (torch.cuda.current_device(), n) in dev._power_scratch
    scratch = dev._power_scratch[torch.cuda.current_device(), n]
    other = dev.paint_power_1d(pos, None, n, L, "tsc", binning="integer")
    third = dev.paint_power_1d(pos, None, n, L, "cic")
    assert dev._power_scratch[torch.cuda.current_device(), n] is scratch          # one scratch served all three
    assert np.isfinite(first["power"]).all() and not np.array_equal(first["power"], other["power"])
    for key in ("k", "power", "modes"):
        assert np.asarray(first[key]).tobytes() == np.asarray(third[key]).tobytes(), key


def test_tile_r2c_tables_of_another_side_in_between(dev):
    """Twiddle and lane tables are cached per side: 256, then 512, then 256 again."""
    g = torch.Generator(device="cuda").manual_seed(3)
    small = torch.randn((256, 256, 256), generator=g, device="cuda", dtype=torch.float32) + 1.0
    first = dev.r2c(small, engine="tile")
    big = torch.randn((512, 512, 512), generator=g, device="cuda", dtype=torch.float32)
    mid = dev.r2c(big, engine="tile")
    assert bool(torch.isfinite(torch.view_as_real(mid)).all())
    del big, mid
    third = dev.r2c(small, engine="tile")
    assert torch.equal(torch.view_as_real(first), torch.view_as_real(third))
    assert abs(complex(first[0, 0, 0]) - float(small.double().mean())) < 3e-7


def test_lowk_modes_tables_of_another_side_in_between(dev):
    g = torch.Generator(device="cuda").manual_seed(5)
    small = torch.randn((256, 256, 256), generator=g, device="cuda", dtype=torch.float32) + 0.5
    first = dev.lowk_modes(small, 256)
    big = torch.randn((512, 512, 512), generator=g, device="cuda", dtype=torch.float32)
    mid = dev.lowk_modes(big, 512)
    assert bool(torch.isfinite(torch.view_as_real(mid)).all())
    del big, mid
    third = dev.lowk_modes(small, 256)
    assert first.abs().max().item() > 1e3
    assert torch.equal(torch.view_as_real(first), torch.view_as_real(third))


# ------------------------------------------------------------------ StagedPaint
@pytest.mark.parametrize("window", ["cic", "tsc"])
def test_staged_paint_second_cycle_on_the_same_object(dev, window):
    """A full group / walk / fold cycle, ``out`` refilled with NaN, the whole cycle again in the same workspace."""
    from oracle import mesh as omesh
    n, L = 64, 1000.0
    host = omesh.lattice_particles(n, n, L, seed=3, dtype=np.float32)
    pos = dev.as_device(host)
    mass = dev.as_device(np.random.default_rng(8).uniform(0.5, 2.0, size=n ** 3).astype(np.float32))
    out = torch.full((n, n, n), float("nan"), dtype=torch.float32, device="cuda")
    sp = dev.StagedPaint(pos, mass, n, L, window, out)

    def cycle():
        sp.group()
        for r in range(sp.nrows_total):
            sp.walk(r, 1)
        sp.fold(0, sp.nrows_total)
        sp.check()
        return out.clone()
    first = cycle()
    out.fill_(float("nan"))
    second = cycle()
    assert bool(torch.isfinite(first).all())
    assert torch.equal(first, second)
    assert torch.equal(first, dev.paint(pos, mass, n, L, window, method="tiled", accumulate=False))
