"""GPU: the plane paint (astrild_amd/plane_paint.py, astrild_amd/csrc/plane_paint.hip) against the numpy restatement of
its contract (tests/plane_paint_oracle.py).  The contract fixes every operation, and the sums are integers, so ``sums``,
``out`` and the counters are compared ``tobytes()``: this is also the check that the device's float64 division, square
root and double -> integer rounding give numpy's results.  Every oracle result is computed once and shared."""
import functools

import numpy as np
import pytest

from tests import dirty_memory as dm
from tests import input_layouts as il
from tests import plane_paint_oracle as orc
from tests import stream_order as so

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

L = 100.0
WINDOWS = ("ngp", "cic", "tsc")
DTYPES = {"f32": np.float32, "f64": np.float64}
SHAPES = [(P, npix) for npix in (1, 2, 5, 8) for P in (1, 3)]
ANGLE = 50.0
MUL = np.array([1.37e-15, 2.91e-15, 0.77e-15])
ADD = np.array([-0.7, 0.31, -12.9])


@pytest.fixture(scope="module", autouse=True)
def _dev(hip):
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def dev(hip):
    from astrild_amd import device
    return device


@pytest.fixture(scope="module")
def pp(hip):
    from astrild_amd import plane_paint
    return plane_paint


def geometry_kw(geometry, P, los=2):
    """The keyword arguments product and oracle share.  Cone: the observer sits half a box in front of the particles'
    centre on the line of sight, a little off axis, so that some particles lie behind it, some outside the shells and
    some across the map's edges."""
    if geometry == "box":
        return dict(boxsize=L)
    origin = [0.53 * L, 0.47 * L, 0.51 * L]
    origin[los] = -0.45 * L
    return dict(opening_angle_deg=ANGLE, chi_edges=tuple(np.linspace(0.31 * L, 2.23 * L, P + 1)), origin=tuple(origin))


def same_bits(got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


@functools.lru_cache(maxsize=None)
def case(geometry, window, pdt, P, npix, los=2, count=1000, seed=11):
    """(pos, mass, vmax, sums, counters) - host arrays, made once."""
    pos, mass = orc.particles(count, L, seed, DTYPES[pdt])
    vmax = float(mass.max())
    sums, counters, _ = orc.paint(pos, mass, geometry, P, npix, window, los, vmax=vmax, **geometry_kw(geometry, P, los))
    for a in (pos, mass, sums, counters):
        a.setflags(write=False)
    return pos, mass, vmax, sums, counters


def c1_of(geometry, npix):
    return orc.cone_coefficients(npix, ANGLE)[0] if geometry == "cone" else 0.0


# ------------------------------------------------------------------ 1. bit equality
@pytest.mark.parametrize("pdt", DTYPES)
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("geometry", ["box", "cone"])
def test_bit_equal_to_the_oracle(dev, pp, geometry, window, pdt):
    deposits = 0
    for P, npix in SHAPES:
        for los in (0, 1, 2):
            pos, mass, vmax, want, want_c = case(geometry, window, pdt, P, npix, los)
            kw = geometry_kw(geometry, P, los)
            sums, counters = pp.plane_paint_sums(dev.as_device(pos), dev.as_device(mass), geometry, P, npix, window, los,
                                                 vmax=vmax, **kw)
            assert sums.is_cuda and sums.dtype == torch.int64 and counters.is_cuda
            assert same_bits(sums, want), (P, npix, los, "sums")
            assert same_bits(counters, want_c), (P, npix, los, "counters", counters.tolist(), want_c.tolist())
            deposits += int(np.count_nonzero(want))
            for name, T in DTYPES.items():
                out = pp.plane_paint_finish(sums, MUL[:P], ADD[:P], geometry, c1_of(geometry, npix), getattr(torch, T.__name__))
                assert same_bits(out, orc.finish(want, MUL[:P], ADD[:P], geometry, T, c1_of(geometry, npix))), (P, npix, los, name)
            if los == 1:                                          # numpy arrays in, the default vmax (max |mass|)
                host, host_c = pp.plane_paint_sums(pos, mass, geometry.upper(), P, npix, window.upper(), los, **kw)
                assert same_bits(host, want) and same_bits(host_c, want_c), (P, npix, "numpy arrays")
    assert deposits > 100


def test_unit_masses_and_scale(dev, pp):
    """mass None is 1.0 * scale; a negative scale deposits negative integers."""
    pos, _ = orc.particles(1000, L, 12, np.float32)
    for geometry in ("box", "cone"):
        kw = geometry_kw(geometry, 3)
        for scale in (1.0, -0.37):
            want, want_c, _ = orc.paint(pos, None, geometry, 3, 5, "tsc", 0, scale=scale, **kw)
            got, got_c = pp.plane_paint_sums(pos, None, geometry, 3, 5, "tsc", 0, scale=scale, **kw)
            assert same_bits(got, want) and same_bits(got_c, want_c), (geometry, scale)
            assert (want.sum() < 0) == (scale < 0)


# ------------------------------------------------------------------ 2. order and launch geometry
@pytest.mark.parametrize("geometry, window, pdt", [("box", "tsc", "f32"), ("cone", "cic", "f64"), ("cone", "ngp", "f32")])
def test_any_order_chunking_and_launch_geometry(dev, pp, geometry, window, pdt):
    """One thread, one short of a block, a block, one more, and three more than the capped grid covers in one sweep;
    the same particles shuffled, and added in three chunks: identical bytes.  Float atomics cannot pass this."""
    P, npix, most = 3, 5, 2048 * 256 + 3
    pos, mass = orc.particles(most, L, 21, DTYPES[pdt])
    vmax, kw = float(mass.max()), geometry_kw(geometry, P)
    pd, md = dev.as_device(pos), dev.as_device(mass)
    run = lambda p, m, **more: pp.plane_paint_sums(p, m, geometry, P, npix, window, np_total=most, vmax=vmax, **kw, **more)
    for count in (1, 255, 256, 257, most):
        want, want_c, _ = orc.paint(pos[:count], mass[:count], geometry, P, npix, window, np_total=most, vmax=vmax, **kw)
        for _ in range(2):
            got, got_c = run(pd[:count], md[:count])
            assert same_bits(got, want) and same_bits(got_c, want_c), count
    perm = torch.from_numpy(np.random.default_rng(22).permutation(most)).cuda()
    shuffled, shuffled_c = run(pd[perm], md[perm])
    assert same_bits(shuffled, want) and same_bits(shuffled_c, want_c)
    sums, counters = None, None
    for lo, hi in ((0, 1), (1, 70001), (70001, most)):
        sums, counters = run(pd[lo:hi], md[lo:hi], sums=sums, counters=counters)
    assert same_bits(sums, want) and same_bits(counters, want_c)


# ------------------------------------------------------------------ 3. edges
def _box_edge_positions(P, npix, dtype):
    big = 1e300 if dtype == np.float64 else 3e38                   # finite in the particles' type: deposited, modulo the period
    marks = [0.0, -0.0, L, -L, 2 * L, big, -big] + [k * L / npix for k in range(npix + 1)] + [k * L / P for k in range(P + 1)] + \
        [(k + 0.5) * L / npix for k in range(npix)]
    vals = []
    for m in marks:
        m = dtype(m)
        vals += [m, np.nextafter(m, dtype(-np.inf)), np.nextafter(m, dtype(np.inf))]
    v = np.array(vals, dtype=dtype)
    return np.concatenate([np.stack([v, v, v], axis=1), np.stack([v, np.roll(v, 1), np.roll(v, 5)], axis=1),
                           np.stack([np.roll(v, 7), v, np.roll(v, 3)], axis=1)])


@pytest.mark.parametrize("pdt", DTYPES)
@pytest.mark.parametrize("window", WINDOWS)
def test_box_edges(dev, pp, window, pdt):
    """Coordinates exactly on plane and pixel boundaries and their neighbours, x = L, -0.0, and the largest finite
    values: all deposited (nothing outside), each where the oracle puts it."""
    for P, npix in ((3, 5), (1, 8), (3, 1)):
        pos = _box_edge_positions(P, npix, DTYPES[pdt])
        for los in (0, 2):
            for shift in (-0.5, 0.0):
                want, want_c, invq = orc.paint(pos, None, "box", P, npix, window, los, boxsize=L, shift=shift)
                got, got_c = pp.plane_paint_sums(pos, None, "box", P, npix, window, los, boxsize=L, shift=shift)
                assert same_bits(got, want) and same_bits(got_c, want_c), (P, npix, los, shift)
                assert want_c.tolist() == [0, 0, 0]
                if window == "ngp":
                    assert want.sum() == len(pos) * int(invq)


E2_EDGES = (3.0, 5.0, 13.0)


def _cone_edge_particles(npix, c1, c0):
    """d vectors (observer at 0, los = 2): radii exactly on the squared edges 9, 25, 169 and beside them; d_los zero,
    negative and the smallest positive number; stencils across every edge and corner of the map."""
    d = [(0.0, 0.0, 3.0), (0.0, 0.0, np.nextafter(3.0, 0)), (0.0, 0.0, 5.0), (0.0, 0.0, np.nextafter(5.0, 0)), (0.0, 0.0, 13.0),
         (0.0, 0.0, np.nextafter(13.0, 0)), (3.0, 4.0, 12.0), (3.0, 4.0, np.nextafter(12.0, 0)), (0.0, 3.0, 4.0), (3.0, 0.0, 4.0),
         (3.0, 0.0, 0.0), (0.0, 5.0, 0.0), (3.0, 0.5, -0.0), (1.0, 1.0, -4.0), (3.0, 0.5, 5e-324), (0.0, 4.0, 5e-324),
         (1e200, 0.0, 4.0), (0.0, 0.0, 1e-300)]
    for sa in (-1.7, -0.6, -0.3, 0.2, 0.5, npix / 2.0, npix - 0.5, npix - 0.2, npix + 0.3, npix + 0.6, npix + 1.7):
        for sb in (-1.7, -0.6, -0.3, 0.2, npix / 2.0, npix - 0.2, npix + 0.3, npix + 0.6, npix + 1.7):
            d.append(((sa - c0) / c1 * 4.0, (sb - c0) / c1 * 4.0, 4.0))
    return np.array(d, dtype=np.float64)


@pytest.mark.parametrize("window", WINDOWS)
def test_cone_edges(dev, pp, window):
    npix, angle = 5, 60.0
    c1, c0 = orc.cone_coefficients(npix, angle)
    origin = (0.3, -1.1, 2.7)
    d = _cone_edge_particles(npix, c1, c0)
    kw = dict(opening_angle_deg=angle, chi_edges=E2_EDGES)
    # the shell rule is half-open: each particle alone, on the exact d (observer at 0)
    # (radius 3: in, plane 0; just below: out; 5: plane 1; just below: plane 0; 13 and (3, 4, 12): out; just below: plane 1)
    planes = {0: 0, 1: None, 2: 1, 3: 0, 4: None, 5: 1, 6: None, 7: 1}
    for i, plane in planes.items():
        outside = int(plane is None)
        got, got_c = pp.plane_paint_sums(d[i:i + 1], None, "cone", 2, npix, "ngp", 2, origin=(0.0, 0.0, 0.0), **kw)
        assert got_c.tolist() == [outside, 0, 0], (i, d[i])
        if not outside:
            assert int(got[planes[i]].sum()) == 2 ** 50 and int(got[1 - planes[i]].abs().sum()) == 0, (i, d[i])
    # d_los zero, negative, the smallest positive: outside, whatever the radius
    for i in range(10, 18):
        _, got_c = pp.plane_paint_sums(d[i:i + 1], None, "cone", 2, npix, window, 2, origin=(0.0, 0.0, 0.0), **kw)
        assert got_c.tolist() == [1, 0, 0], (i, d[i])
    # everything at once, seen from a displaced observer and along every axis, against the oracle
    for los in (0, 1, 2):
        a, b = [c for c in range(3) if c != los]
        pos = np.empty_like(d)
        pos[:, a], pos[:, b], pos[:, los] = d[:, 0], d[:, 1], d[:, 2]
        pos = pos + np.asarray(origin)[None, :]
        want, want_c, _ = orc.paint(pos, None, "cone", 2, npix, window, los, origin=origin, **kw)
        got, got_c = pp.plane_paint_sums(pos, None, "cone", 2, npix, window, los, origin=origin, **kw)
        assert same_bits(got, want) and same_bits(got_c, want_c), (los, got_c.tolist(), want_c.tolist())
        assert want_c[0] > 8 and want_c[2] == 0 and (want_c[1] > 0) == (window != "ngp")
    # one particle across the corner (0, 0): CIC keeps one of its four points, TSC four of nine
    corner = np.array([[(-0.3 - c0) / c1 * 4.0, (-0.3 - c0) / c1 * 4.0, 4.0]])
    got, got_c = pp.plane_paint_sums(corner, None, "cone", 2, npix, window, 2, **kw)
    kept = {"ngp": 1, "cic": 1, "tsc": 4}[window]
    assert int(torch.count_nonzero(got)) == kept and got_c.tolist() == [0, 0 if window == "ngp" else 1, 0]
    assert int(torch.count_nonzero(got[1, :2, :2])) == kept


@pytest.mark.parametrize("geometry", ["box", "cone"])
@pytest.mark.parametrize("window", WINDOWS)
def test_non_finite_coordinates_deposit_nothing(dev, pp, geometry, window):
    """NaN and +-Inf on each axis: no deposit, counted as outside, the other particles' result unchanged, and the bytes
    around ``sums`` and ``out`` untouched."""
    P, npix, guard = 3, 5, 64
    pos, mass, vmax, _, _ = case(geometry, window, "f64", P, npix)
    kw = geometry_kw(geometry, P)
    bad = np.array(pos[:9])
    for axis in range(3):
        bad[3 * axis + 0, axis], bad[3 * axis + 1, axis], bad[3 * axis + 2, axis] = np.nan, np.inf, -np.inf
    every = np.concatenate([pos[:500], bad, pos[500:]])
    every_m = np.concatenate([mass[:500], mass[:9], mass[500:]])
    want, want_c, _ = orc.paint(pos, mass, geometry, P, npix, window, np_total=2000, vmax=vmax, **kw)
    count = P * npix * npix
    sbuf = il.pad(torch.empty(count + 2 * guard, dtype=torch.int64, device="cuda"))
    obuf = il.pad(torch.empty(count + 2 * guard, dtype=torch.float32, device="cuda"))
    sums = sbuf[guard:guard + count].view(P, npix, npix).zero_()
    out = obuf[guard:guard + count].view(P, npix, npix)
    before_s, before_o = il.raw_bytes(sbuf), il.raw_bytes(obuf)
    got, got_c = pp.plane_paint_sums(every, every_m, geometry, P, npix, window, sums=sums, np_total=2000, vmax=vmax, **kw)
    assert got is sums
    res = pp.plane_paint_finish(sums, MUL, ADD, geometry, c1_of(geometry, npix), out=out)
    assert res is out
    assert same_bits(got, want)
    assert got_c.tolist() == [int(want_c[0]) + 9, int(want_c[1]), 0]
    assert same_bits(out, orc.finish(want, MUL, ADD, geometry, np.float32, c1_of(geometry, npix)))
    after_s, after_o = il.raw_bytes(sbuf), il.raw_bytes(obuf)
    for before, after, item in ((before_s, after_s, 8), (before_o, after_o, 4)):
        assert after[:guard * item] == before[:guard * item] and after[-guard * item:] == before[-guard * item:]


# ------------------------------------------------------------------ 4. refusal
@pytest.mark.parametrize("geometry", ["box", "cone"])
def test_refused_masses(dev, pp, geometry):
    """NaN, +-Inf and masses above vmax, handed to the C entry as they are (an explicit ``vmax`` skips the wrapper's own
    reduction): counted in counters[2], no deposit, the others unchanged - also when the refused particle's coordinates are
    not finite (refusal comes first)."""
    P, npix = 3, 5
    pos, mass, vmax, want, want_c = case(geometry, "tsc", "f32", P, npix)
    kw = geometry_kw(geometry, P)
    extra_m = np.array([np.nan, np.inf, -np.inf, np.nextafter(np.float32(vmax), np.float32(np.inf)), -3.0 * vmax, np.nan], dtype=np.float32)
    extra_p = np.array(pos[:6])
    extra_p[5, 1] = np.nan
    every, every_m = np.concatenate([extra_p[:3], pos, extra_p[3:]]), np.concatenate([extra_m[:3], mass, extra_m[3:]])
    # (1006 particles declared; the oracle's 1000 give the same exponent, 50)
    got, got_c = pp.plane_paint_sums(every, every_m, geometry, P, npix, "tsc", np_total=1006, vmax=vmax, **kw)
    assert same_bits(got, want)
    assert got_c.tolist() == [int(want_c[0]), int(want_c[1]), 6]
    with pytest.raises(ValueError, match="NaN or Inf"):            # the default vmax is a reduction that refuses them up front
        pp.plane_paint_sums(every, every_m, geometry, P, npix, "tsc", **kw)


# ------------------------------------------------------------------ 5. contention
@pytest.mark.parametrize("window", WINDOWS)
def test_contention_on_one_pixel(dev, pp, window):
    """2^16 particles of mass vmax on one pixel centre: np_total = 2^16 gives k = 45 and each adds 2^45 in all.  NGP and
    CIC (weights 1 and 0 at a centre) put it into one pixel, which holds exactly 2^61; TSC (1/8, 3/4, 1/8) puts 9/16 of it
    there and the rest around it.  Every sum is exact and nothing wraps."""
    box, npix, P, n = 64.0, 8, 2, 1 << 16
    pos = np.tile(np.array([[(3 + 0.5) * box / npix, (6 + 0.5) * box / npix, 0.7 * box]]), (n, 1))
    mass = np.full(n, 1.5)
    sums, counters = pp.plane_paint_sums(pos, mass, "box", P, npix, window, vmax=1.5, boxsize=box)
    share, touched = (9, 9) if window == "tsc" else (16, 1)
    assert orc.exponent(n) == 45 and int(sums[1, 3, 6]) == share * 2 ** 57 and int(sums.sum()) == 2 ** 61
    assert int(torch.count_nonzero(sums)) == touched and counters.tolist() == [0, 0, 0]
    want, _, _ = orc.paint(pos, mass, "box", P, npix, window, boxsize=box)
    assert same_bits(sums, want)
    out = pp.plane_paint_finish(sums, [1.5 / 2.0 ** 45] * P, [0.0] * P, "box", dtype=torch.float64)
    assert float(out[1, 3, 6]) == 1.5 * n * share / 16


# ------------------------------------------------------------------ 6. element indices past 2^31
def test_large_index(dev, pp):
    """2 planes of 32771^2: 2.15e9 elements, 17.2 GB of sums and 8.6 GB of float32 planes.  Particles either side of
    element 2^31 (plane 1), in the first pixel and in the last; checked on the device, nothing is copied to the host."""
    P, npix, box = 2, 32771, 32771.0
    torch.cuda.empty_cache()                                       # (blocks the allocator caches for earlier tests count as used)
    free, _ = torch.cuda.mem_get_info()
    if free < 40e9:
        pytest.skip(f"{free / 1e9:.1f} GB of device memory free, the planes and their checks need 40")
    count = P * npix * npix
    assert count > 2 ** 31
    ia, ib = divmod(2 ** 31 - npix * npix, npix)                  # element 2^31 is pixel (ia, ib) of plane 1
    assert 2 <= ib < npix - 2
    pix = [(0, 0, 0), (1, ia, ib - 1), (1, ia, ib), (1, ia, ib + 1), (1, ia - 1, ib), (1, npix - 1, npix - 1), (0, npix - 1, npix - 1)]
    # NGP at pixel centres, and CIC a quarter pixel past a centre on both axes (4 deposits; the last pixel wraps to 0)
    for window, off in (("ngp", 0.5), ("cic", 0.75)):
        pos = np.array([[(a + off), (b + off), (p + 0.5) * box / P] for p, a, b in pix])
        mass = np.linspace(0.6, 1.9, len(pix))
        cl, c1, c0 = orc.box_coefficients(P, npix, box)
        plane, _ = orc._locate(pos[:, 2] * cl, P, "cic")
        ba, fa = orc._locate(pos[:, 0] * c1 + c0, npix, window)
        bb, fb = orc._locate(pos[:, 1] * c1 + c0, npix, window)
        assert plane.tolist() == [p for p, _, _ in pix] and ba.tolist() == [a for _, a, _ in pix] and bb.tolist() == [b for _, _, b in pix]
        wa, wb = orc._weights(fa, window), orc._weights(fb, window)
        invq = 2.0 ** 50 / float(mass.max())
        expect = {}
        for i in range(len(wa)):
            for j in range(len(wb)):
                r = np.rint(((mass * wa[i]) * wb[j]) * invq).astype(np.int64)
                flat = (plane * npix + orc._wrap1(ba + i, npix)) * npix + orc._wrap1(bb + j, npix)
                for f, v in zip(flat.tolist(), r.tolist()):
                    expect[f] = expect.get(f, 0) + v
        flat = np.array(sorted(expect), dtype=np.int64)
        assert (flat < 2 ** 31).any() and (flat >= 2 ** 31).any() and 2 ** 31 in expect and count - 1 in expect
        values = np.array([expect[f] for f in flat.tolist()], dtype=np.int64)
        sums = out = None
        try:
            sums, counters = pp.plane_paint_sums(pos, mass, "box", P, npix, window, boxsize=box)
            fd, vd = torch.from_numpy(flat).cuda(), torch.from_numpy(values).cuda()
            assert torch.equal(sums.view(-1)[fd], vd), window
            assert int(torch.count_nonzero(sums)) == int(np.count_nonzero(values)) and int(sums.sum()) == int(values.sum())
            assert counters.tolist() == [0, 0, 0]
            q = float(mass.max()) / 2.0 ** 50
            out = pp.plane_paint_finish(sums, [q, 2 * q], [0.25, -0.5], "box")
            want = (values.astype(np.float64) * np.where(flat >= npix * npix, 2 * q, q) + np.where(flat >= npix * npix, -0.5, 0.25)).astype(np.float32)
            assert torch.equal(out.view(-1)[fd], torch.from_numpy(want).cuda()), window
            for p, add in ((0, 0.25), (1, -0.5)):
                touched = int(np.count_nonzero(values[(flat >= npix * npix) == bool(p)]))
                assert int(torch.count_nonzero(out[p] != add)) == touched, (window, p)
        finally:
            del sums, out
            torch.cuda.empty_cache()


# ------------------------------------------------------------------ 7. streams, layouts, dirty memory
def _plumbing_case(pp, geometry):
    P, npix = 3, 5
    kw = geometry_kw(geometry, P)
    edges = np.asarray(kw.pop("chi_edges")) if geometry == "cone" else np.linspace(1.0, 2.0, P + 1)

    def make():
        real = list(orc.particles(4000, L, 31, np.float32)) + [edges * edges]
        decoy = list(orc.particles(4000, L, 32, np.float32)) + [(edges * 1.1) ** 2]
        return real, decoy

    def call(dev, lens, pos, mass, e2):
        more = dict(chi_edges=edges, e2=e2, **kw) if geometry == "cone" else kw
        sums, counters = pp.plane_paint_sums(pos, mass, geometry, P, npix, "tsc", np_total=4000, vmax=2.0, **more)
        out = pp.plane_paint_finish(sums, MUL, ADD, geometry, c1_of(geometry, npix), torch.float32)
        return sums, counters, out

    def oracle():
        real, _ = make()
        more = dict(chi_edges=edges, **kw) if geometry == "cone" else kw
        sums, counters, _ = orc.paint(real[0], real[1], geometry, P, npix, "tsc", np_total=4000, vmax=2.0, **more)
        return sums, counters, orc.finish(sums, MUL, ADD, geometry, np.float32, c1_of(geometry, npix))
    # built directly: stream_order.case() would append to the registry the other test modules walk
    return so.Case(name="plane_paint_" + geometry, covers=(), make=make, compare="equal", call=call), oracle()


@pytest.mark.parametrize("geometry", ["box", "cone"])
def test_streams_layouts_dirty_memory(dev, pp, geometry):
    from astrild_amd import lensing
    c, want = _plumbing_case(pp, geometry)
    ins, dec = c.make()
    be = so.cuda_backend()
    fn = lambda *a: c.call(dev, lensing, *a)
    for pattern in dm.PATTERNS:                                    # wrapper-allocated sums, counters and planes
        with dm.dirty(pattern):
            assert so.same_bits(fn(*[be.upload(a) for a in ins]), want), dm.PATTERN_IDS[pattern]
    with dm.dirty(dm.HUGE_BYTES):
        assert not so.same_bits(fn(*[be.upload(a) for a in dec]), want), "the decoy gives the real answer"
        with torch.cuda.stream(be.stream(0)):                     # under S, nothing late
            plain = fn(*[be.upload(a) for a in ins])
        torch.cuda.synchronize()
        assert so.same_bits(plain, want)
        so.late_call(fn, ins, dec)                                # (first launches of the probe's own kernels under S)
        got, armed = so.late_call(fn, ins, dec)
    torch.cuda.synchronize()
    assert armed, "the plane paint waited for the device: it must only queue work on the caller's stream"
    assert so.same_bits(got, want), "behind the late producer"
    outcomes = il.run_layouts(c, dev, lensing)                    # offset, strided, transposed: bit equal to plain
    assert {o for _, o in outcomes} == {"same"}, outcomes
    assert {label.split(":")[0] for label, _ in outcomes} == {"input 0", "input 1", "input 2", "all inputs"}
    # host arrays: Fortran order, negative strides, read-only
    for i in (0, 1):
        for v in il.host_variants(ins[i]):
            if v.name == "byteswapped":
                continue
            args = [v.view if j == i else ins[j] for j in range(2)] + [be.upload(ins[2])]
            assert so.same_bits(fn(*args), want), (i, v.name)


def test_no_particles_no_library_call(dev, pp):
    with il.LibraryGuard() as guard:
        sums, counters = pp.plane_paint_sums(np.empty((0, 3), dtype=np.float32), None, "box", 2, 4, boxsize=L)
    assert guard.calls == 0 and tuple(sums.shape) == (2, 4, 4) and not sums.any() and counters.tolist() == [0, 0, 0]


# ------------------------------------------------------------------ 8. against the 3D paint
@pytest.mark.parametrize("los", [0, 1, 2])
def test_against_the_3d_paint_summed_along_the_line_of_sight(dev, pp, los):
    """Box, one plane, shift 0, CIC, float64: the plane is the 3D CIC grid of ``device.paint`` summed along ``los``.

    Both form s = x n / L the same way (adding the shift 0.0 is exact), so the float64 weights wa, wb are the same numbers.
    With E = sum ms wa wb in real arithmetic per pixel, A its sum of absolute values, u = 2^-53:
      plane paint: each term (ms wa) wb carries two roundings, 2 u (1 + u) |t|; the product with invq a third that moves
        it by at most 2^(k - 53) quanta, and the rounding to the quantum by 1/2:  |sums q - E| <= K2 q (1/2 + 2^(k - 53))
        + 2 u (1 + u) A, K2 the number of terms of the pixel, k = 50 here; q stands for 1 / invq = (vmax / 2^k) (1 + u)^+-1.
      3D paint: the cell sums differ from their exact values S_c by at most tests/paint_accuracy.py's any-path bound
        (direct path: (2 K + 13) u A_c + 3 u D_c + u |S_c| + the reference's own (K + 8) 2^-64 A_c); the sum over the
        column in longdouble adds n 2^-64 of its size; and sum_c S_c = sum ms wa wb (wz0 + wz1) where the two
        float64 weights 1 - f and f add up to 1 within u, so |sum_c S_c - E| <= u A.
    A <= sum_c A_c (1 + 2 u).  Rounded up: |plane - column sum| <= K2 q (1/2 + 1/8) (1 + 2^-50) + 4 u sum_c A_c +
    sum_c any_bound_c.  No tuned number."""
    from tests import paint_accuracy as pa
    n, box, count = 32, 64.0, 1000                                 # (32: the smallest grid tests/paint_accuracy.py describes)
    rng = np.random.default_rng(81)
    pos = rng.uniform(0.0, box, size=(count, 3))
    mass = rng.uniform(0.5, 2.0, size=count)
    vmax = float(mass.max())
    sums, counters = pp.plane_paint_sums(pos, mass, "box", 1, n, "cic", los, shift=0.0, vmax=vmax, boxsize=box)
    q = vmax / 2.0 ** 50
    plane = sums[0].cpu().numpy().astype(np.longdouble) * np.longdouble(q)
    grid = dev.paint(dev.as_device(pos), dev.as_device(mass), n, box, "cic", method="direct").cpu().numpy()
    column = grid.astype(np.longdouble).sum(axis=los)
    ref = pa.Reference(pos, mass, n, box, "cic")
    K2 = ref.K.sum(axis=los) // 2
    A = ref.A.astype(np.float64).sum(axis=los)
    u = 2.0 ** -53
    bound = K2 * q * 0.625 * (1 + 2.0 ** -50) + 4 * u * A + ref.any_bound(np.float64).sum(axis=los) + n * 2.0 ** -64 * A
    err = np.abs((plane - column).astype(np.float64))
    hit = bound > 0                                                # (a pixel no particle touches: 0 on both sides)
    print(f"PLANE vs 3D paint los={los}: max |plane - column| / bound = {(err[hit] / bound[hit]).max():.3f}, "
          f"max |plane - column| / A = {(err[hit] / A[hit]).max():.3g}")
    assert counters.tolist() == [0, 0, 0] and K2.sum() == 4 * count
    assert np.all(err <= bound)
    # and the bound has power: a plane short of one particle's deposit misses it by orders of magnitude
    assert float(mass.min()) / 4 > 1e6 * bound.max()
