"""GPU: the order of device work (Streams).  Every entry family runs under a side stream behind a late
producer while the null stream is busy (tests/stream_order.py: ``late_call``); hidden caches are filled under one
delayed stream and hit from another; explicit plans and workspaces are handed from one stream to the next.  A failure
here is a wrong value, never a fault: the decoys are valid inputs.
"""
import contextlib

import numpy as np
import pytest

from tests import dirty_memory as dm
from tests import stream_order as so
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


@pytest.fixture(scope="module")
def be():
    b = so.cuda_backend()
    print(f"\nSTREAM_ORDER torch.cuda._sleep: {b.cycles_per_ms():.0f} cycles per ms, D = {so.TARGET_MS} ms = "
          f"{int(b.cycles_per_ms() * so.TARGET_MS)} cycles")
    # the first launch of a kernel loads its code object, which waits for the device: the torch kernels of the probe and
    # of the controls run once, on every pooled stream, before anything is asked of ``armed``
    x = torch.arange(N_CTRL, dtype=torch.float64, device="cuda")
    for s in [torch.cuda.default_stream()] + [b.stream(i) for i in range(so.MAX_STREAMS)]:
        with torch.cuda.stream(s), dm.dirty(dm.HUGE_BYTES):
            out = torch.empty_like(x)
            torch.mul(x, 2.0, out=out)
            out.copy_(x * out.clone().fill_(3.0))
            s.wait_stream(torch.cuda.default_stream())
    torch.cuda.synchronize()
    return b


N_CTRL = 1 << 16


def host(v):
    """An output as host values (tensors -> numpy), waited for."""
    torch.cuda.synchronize()
    return so.tree_map(lambda t: t.detach().cpu().numpy(), v)


# ------------------------------------------------------------------ controls: the probe's own power
def _ctrl_inputs():
    return [np.arange(N_CTRL, dtype=np.float64)], [np.arange(N_CTRL, dtype=np.float64)[::-1].copy()]


def _correct(x):
    out = torch.empty_like(x)
    torch.mul(x, 2.0, out=out)
    return out


def test_calibration_and_a_correct_op_passes(be):
    cpm = be.cycles_per_ms()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    be.sleep(torch.cuda.current_stream(), so.TARGET_MS)
    b.record()
    b.synchronize()
    assert 0.5 * so.TARGET_MS < a.elapsed_time(b) < 2.0 * so.TARGET_MS, (cpm, a.elapsed_time(b))
    ins, dec = _ctrl_inputs()
    with dm.dirty(dm.HUGE_BYTES):
        so.late_call(_correct, ins, dec)                          # (first launches: code objects are loaded)
        got, armed = so.late_call(_correct, ins, dec)
    assert armed
    assert np.array_equal(host(got), 2.0 * ins[0])


def test_control_input_read_on_the_default_stream(be):
    """Planted: the op runs on the default stream instead of the caller's."""
    def op(x):
        out = torch.empty_like(x)
        with torch.cuda.stream(torch.cuda.default_stream()):
            torch.mul(x, 2.0, out=out)
        return out
    ins, dec = _ctrl_inputs()
    with dm.dirty(dm.HUGE_BYTES):
        got, armed = so.late_call(op, ins, dec)
    assert armed and not np.array_equal(host(got), 2.0 * ins[0])


def test_control_input_read_on_a_side_stream_that_does_not_wait(be):
    """Planted: a library-owned side stream that joins back but never waited for the caller's stream reads the decoy."""
    S, null, side = be.stream(0), torch.cuda.default_stream(), be.stream(1)
    assert be.runs_beside(side, S) and be.runs_beside(side, null) and be.runs_beside(S, null)

    def op(x):
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        with torch.cuda.stream(side):
            torch.mul(x, 2.0, out=out)
        torch.cuda.current_stream().wait_stream(side)
        return out
    ins, dec = _ctrl_inputs()
    got, armed = so.late_call(op, ins, dec)                       # (no dirty fill of `out` on S behind the side stream's store)
    got = host(got)
    print(f"STREAM_ORDER side-stream control: armed={armed} stale={np.array_equal(got, 2.0 * dec[0])}")
    assert armed
    assert not np.array_equal(got, 2.0 * ins[0])
    assert np.array_equal(got, 2.0 * dec[0])                      # exactly the stale read


def test_control_output_written_on_the_default_stream(be):
    """Planted: the input is read on the caller's stream, the result is stored from the default stream."""
    def op(x):
        tmp = x * 2.0
        out = torch.empty_like(x)
        ready = torch.cuda.Event()
        ready.record()
        null = torch.cuda.default_stream()
        null.wait_event(ready)
        with torch.cuda.stream(null):
            out.copy_(tmp)
        return out
    ins, dec = _ctrl_inputs()
    with dm.dirty(dm.HUGE_BYTES):
        got, armed = so.late_call(op, ins, dec)
    assert armed and not np.array_equal(host(got), 2.0 * ins[0])


def test_control_cache_filled_under_a_delayed_stream(be):
    """Planted: a table cached by a call under a delayed stream is read by the next call under another."""
    cache = {}
    filler = be.stream(1)

    def op(x):
        if "table" not in cache:
            with torch.cuda.stream(filler):
                table = torch.empty_like(x)                      # (dirty at once)
                be.sleep(filler, 2 * so.TARGET_MS)
                table.fill_(3.0)
            cache["table"] = table
        return x * cache["table"]
    ins, dec = _ctrl_inputs()
    with dm.dirty(dm.HUGE_BYTES):
        got, armed = so.late_call(op, ins, dec)
    assert armed and not np.array_equal(host(got), 3.0 * ins[0])
    with dm.dirty(dm.HUGE_BYTES):                                 # the table is complete by now: the same op passes
        got, armed = so.late_call(op, ins, dec)
    assert armed and np.array_equal(host(got), 3.0 * ins[0])


# ------------------------------------------------------------------ one case per entry family
def _compare(c, got, want, ins):
    """The case's comparison: bit-identity, or its own test's assertion against its own oracle (``verify``), or that
    test's rtol / atol against ``want`` (the oracle where the case names one, else the default-stream result)."""
    if c.compare == "equal":
        return so.same_bits(got, want)
    if c.verify is not None:
        return c.verify(got, *ins)
    return so.close(got, want, *c.compare)


@pytest.mark.parametrize("c", so.CASES, ids=[c.name for c in so.CASES])
def test_entry_family_behind_a_late_producer(dev, lens, be, c):
    ins, dec = c.make()
    fn = lambda *a: c.call(dev, lens, *a)
    S = be.stream(0)
    with so.environment(c.env), dm.dirty(dm.HUGE_BYTES):
        dev_ins = ins if c.host_inputs else [be.upload(a) for a in ins]
        ref = host(fn(*dev_ins))                                  # the default stream: warm-up and reference
        if ins:
            dev_dec = dec if c.host_inputs else [be.upload(a) for a in dec]
            assert not so.same_bits(host(fn(*dev_dec)), ref), "the decoy gives the real answer: a stale read would not show"
        with torch.cuda.stream(S):                                # S, nothing late: what is built per stream exists now
            plain = fn(*dev_ins)
        plain = host(plain)
        got, armed = so.late_call(fn, ins, dec, host_inputs=c.host_inputs)
        got = host(got)
    print(f"\nSTREAM_ORDER {c.name}: armed={armed} host_syncs={c.host_syncs}")
    want = ref if c.oracle is None else c.oracle(*ins)
    assert _compare(c, ref, want, ins), "the default-stream result misses the reference"
    assert _compare(c, plain, want, ins), "under a side stream, nothing late"
    assert _compare(c, got, want, ins), "behind the late producer"
    assert armed == (not c.host_syncs), (c.name, armed, c.sync_line)


# ------------------------------------------------------------------ hidden caches across streams (rule 2)
def _two_streams(be, fn, streams=(0, 1), delay=(True, False)):
    """fn() under each of the pooled streams in turn, the delayed ones behind a sleep of D; clones made on the same
    stream, returned as host values once everything has run."""
    outs = []
    for i, late in zip(streams, delay):
        s = be.stream(i)
        if late:
            be.sleep(s, so.TARGET_MS)
        with torch.cuda.stream(s):
            outs.append(so.tree_map(be.clone, fn()))
    return [host(o) for o in outs]


@pytest.fixture
def empty_caches():
    with dm.dirty(dm.HUGE_BYTES) as alloc:
        yield alloc


def _geometry_matches(got, ref):
    """(ksum, psum, nmodes) of a fused power call against a reference from another filling of the geometry cache: psum
    and nmodes to the bit, ksum - float atomics, refilled - as the geometry's own test holds it (so.GEOMETRY_TOL)."""
    return np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and so.close(got[0], ref[0], *so.GEOMETRY_TOL)


def test_power_scratch_two_streams_at_the_same_time(dev, be):
    """Both streams are let go by ONE event and run the fused power of a 512^3 grid in the one cached scratch: without
    the hand-over in device._power_scratch_for they work in it side by side.  The shell geometry is cold as well: the
    first call fills it behind the event, the second stream's call hits it at once."""
    g = torch.Generator(device="cuda").manual_seed(12)
    fa = torch.randn((512, 512, 512), generator=g, device="cuda", dtype=torch.float32) + 1.0
    fb = torch.randn((512, 512, 512), generator=g, device="cuda", dtype=torch.float32) + 1.0
    ref_a = host(dev.power_sums_fused(fa, so.L_BOX, mean=1.0))
    ref_b = host(dev.power_sums_fused(fb, so.L_BOX, mean=1.0))
    assert not np.array_equal(ref_a[1], ref_b[1])
    with dm.dirty(dm.HUGE_BYTES):
        s0, s1, null = be.stream(0), be.stream(1), torch.cuda.default_stream()
        be.sleep(null, so.TARGET_MS)
        go = be.record()
        outs = []
        for s, f in ((s0, fa), (s1, fb), (s0, fa), (s1, fb)):
            s.wait_event(go)
            with torch.cuda.stream(s):
                outs.append(so.tree_map(be.clone, dev.power_sums_fused(f, so.L_BOX, mean=1.0)))
        outs = host(outs)
    for got, want in zip(outs, (ref_a, ref_b, ref_a, ref_b)):               # psum: bit-identical on repeat
        assert np.array_equal(got[1], want[1])
        assert _geometry_matches(got, want)
        assert so.same_bits((got[0], got[2]), (outs[0][0], outs[0][2]))     # one filling of the geometry: the same bits for all


def test_power_scratch_released_under_another_stream(dev, be):
    """The scratch is allocated under A and used under B; while B still works in it (three 512^3 spectra, queued without
    a host wait) a call of another size under A releases it, and dirty blocks of its size are taken under A at once:
    without record_stream the allocator hands B's working memory out, and the fills land in it.  The geometry of both
    sides is filled under A and read under B without a host wait in between for side 128."""
    g = torch.Generator(device="cuda").manual_seed(13)
    f512 = torch.randn((512, 512, 512), generator=g, device="cuda", dtype=torch.float32) + 1.0
    f128 = dev.as_device(so._cube(128, np.float64, 1))
    ref = host(dev.power_sums_fused(f512, so.L_BOX, mean=1.0))
    ref128 = host(dev.power_sums_fused64(f128, so.L_BOX))
    with dm.dirty(dm.HUGE_BYTES):
        a, b = be.stream(0), be.stream(1)
        with torch.cuda.stream(a):
            first = so.tree_map(be.clone, dev.power_sums_fused(f512, so.L_BOX, mean=1.0))    # the scratch: a block of A's
            nbytes = next(iter(dev._power_scratch.values())).numel()
        torch.cuda.synchronize()
        with torch.cuda.stream(b):
            late = [so.tree_map(be.clone, dev.power_sums_fused(f512, so.L_BOX, mean=1.0)) for _ in range(3)]
        with torch.cuda.stream(a):
            other = dev.power_sums_fused64(f128, so.L_BOX)                           # another size: the scratch is released
            fillers = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(2)]      # dirty, under A, now
            other = so.tree_map(be.clone, other)
        first, late, other = host(first), host(late), host(other)
        del fillers
    assert np.array_equal(first[1], ref[1]) and _geometry_matches(first, ref)
    for got in late:
        assert np.array_equal(got[1], ref[1]) and _geometry_matches(got, ref)
        assert so.same_bits((got[0], got[2]), (first[0], first[2]))
    assert so.close(other[1], ref128[1], 1e-11) and np.array_equal(other[2], ref128[2])      # (rtol: the registry's, power_sums_fused64)
    assert so.close(other[0], ref128[0], *so.GEOMETRY_TOL)


def test_lensing_plan_caches_give_every_stream_its_own_plan(dev, lens, be, empty_caches):
    """lens_plan / smooth_plan are keyed by stream: the call under S2 does not get the plan made under the delayed S1
    (whose kernel spectra are only queued), it builds its own - and, for lens_plan, which keeps one resident plan, that
    destroys S1's plan while S1's work is still queued in it: hipFree waits for the device first."""
    bsz = float(np.deg2rad(3.0))
    kd = dev.as_device(so._kappa(100)(1)[0])
    img = dev.as_device(so._kappa(64)(1)[0])
    fresh = lens.LensPlan(100, bsz)
    ref_alphas = host(fresh.alphas(kd))
    ref_smooth = host(lens.SmoothPlan(64).gaussian(img.clone(), 1.2, "gaussian"))
    del fresh
    a, b = _two_streams(be, lambda: lens.lens_plan(100, bsz).alphas(kd))
    assert so.same_bits(a, ref_alphas) and so.same_bits(b, ref_alphas)
    a, b = _two_streams(be, lambda: lens.smooth_plan(64).gaussian(img.clone(), 1.2, "gaussian"))
    assert so.same_bits(a, ref_smooth) and so.same_bits(b, ref_smooth)


def test_fused_power_low_k_side_stream_per_caller_stream(dev, be):
    field = dev.as_device(so._cube(256, np.float32, 1))
    ref = host(dev.power_sums_fused(field, so.L_BOX, mean=1.0, lowk=True))
    outs = _two_streams(be, lambda: dev.power_sums_fused(field, so.L_BOX, mean=1.0, lowk=True), streams=(0, 1, 2),
                        delay=(True, True, False))
    assert all(so.same_bits(o, ref) for o in outs)


# ------------------------------------------------------------------ cold caches, two streams (rule 2, every entry family)
@contextlib.contextmanager
def cold_caches():
    """Every entry of so.HIDDEN_STATE that can be made cold in this process is: the dirty allocator empties four of the
    Python caches, ``clear`` of each entry the rest (the rocFFT plans are swapped out and put back afterwards, so that
    the session does not compile them again).  The device is idle when the old entries come back."""
    with dm.dirty(dm.HUGE_BYTES) as alloc:
        mp = pytest.MonkeyPatch()
        try:
            for h in so.HIDDEN_STATE:
                if h.clear is not None:
                    h.clear(mp)
            yield alloc
        finally:
            torch.cuda.synchronize()
            mp.undo()


def _compare_refilled(c, got, want, ins):
    """``_compare`` for a result whose geometry comes from ANOTHER filling of the cache than the reference's: the
    leaves the case names as the geometry's float sums are held to so.GEOMETRY_TOL, all others as the case says."""
    if not c.geometry_leaves:
        return _compare(c, got, want, ins)
    g, w = list(so.leaves(got)), list(so.leaves(want))
    rest = lambda v: [x for i, x in enumerate(v) if i not in c.geometry_leaves]
    geom = lambda v: [v[i] for i in c.geometry_leaves]
    return len(g) == len(w) and so.same_bits(rest(g), rest(w)) and so.close(geom(g), geom(w), *so.GEOMETRY_TOL)


@pytest.mark.parametrize("c", so.CASES, ids=[c.name for c in so.CASES])
def test_entry_family_on_cold_caches_from_two_streams(dev, lens, be, c):
    """The reference on the default stream; then, with every hidden cache empty and nothing run in between: the call
    under stream 0 behind a sleep of D (whatever it caches is queued, not done), under stream 1 at once, under stream 0
    again.  What a call builds per STREAM inside the library (side streams, code objects) exists beforehand: it cannot
    be made cold, and building it waits for the device."""
    ins, dec = c.make()
    fn = lambda *a: c.call(dev, lens, *a)
    s0, s1 = be.stream(0), be.stream(1)
    up = lambda: ins if c.host_inputs else [be.upload(a) for a in ins]
    with so.environment(c.env):
        ref = host(fn(*up()))
        for s in (s0, s1):
            with torch.cuda.stream(s):
                fn(*up())
        torch.cuda.synchronize()
        with cold_caches():
            three = [up() for _ in range(3)]
            torch.cuda.synchronize()
            be.sleep(s0, so.TARGET_MS)
            with torch.cuda.stream(s0):
                asleep = be.record()
                first = fn(*three[0])
                armed = not be.done(asleep)
                first = so.tree_map(be.clone, first)
            with torch.cuda.stream(s1):
                second = so.tree_map(be.clone, fn(*three[1]))
            with torch.cuda.stream(s0):
                third = so.tree_map(be.clone, fn(*three[2]))
            outs = [host(o) for o in (first, second, third)]
    want = ref if c.oracle is None else c.oracle(*ins)
    geom = lambda v: [x for i, x in enumerate(so.leaves(v)) if i in c.geometry_leaves]
    print(f"\nSTREAM_ORDER cold {c.name}: armed={armed} host_syncs={c.host_syncs} "
          f"bitwise={[so.same_bits(o, ref) for o in outs]}")
    assert _compare(c, ref, want, ins), "the default-stream result misses the reference"
    for o, what in zip(outs, ("stream 0, filling behind the sleep", "stream 1, at once", "stream 0 again")):
        assert _compare_refilled(c, o, want, ins), what
        assert so.same_bits(geom(o), geom(outs[0])), what + ": one filling of the geometry, other bits"
    assert armed == (not c.host_syncs), (c.name, armed, c.sync_line)


# ------------------------------------------------------------------ the shell geometry: filled under a delayed stream, hit at once
BOX_OF_ITS_OWN = 987.625                   # no other test uses it: the float64-edge table (n, boxsize) is cold as well


def _spec64(dev):
    return dev.as_device(so._half_spectrum(64, np.complex128, 1))


GEOMETRY_CALLS = {
    # name: (call, indices of the outputs that come out of the geometry cache, (rtol, atol_rel) of the others)
    "power_bin_1d": (lambda dev: (lambda spec=_spec64(dev): dev.power_bin_1d(spec, None, 64, so.L_BOX)), (0, 2), (1e-12, 1e-12)),
    "power_bin_2d": (lambda dev: (lambda spec=_spec64(dev): dev.power_bin_2d(spec, None, 64, so.L_BOX, Nmu=5, los=2, poles=(0, 2, 4))),
                     (0, 1, 3), (1e-12, 1e-12)),
    "shell_geometry_block": (lambda dev: (lambda: dev.shell_geometry(64, so.L_BOX, (0, 64), (16, 16))), (0, 1), None),
    "shell_geometry_2d_block": (lambda dev: (lambda: dev.shell_geometry_2d(64, so.L_BOX, 5, 2, (0, 64), (16, 16))), (0, 1, 2), None),
    "power_sums_fused_256": (lambda dev: (lambda f=dev.as_device(so._cube(256, np.float32, 1)):
                                          dev.power_sums_fused(f, BOX_OF_ITS_OWN, mean=1.0)), (0, 2), (0.0, 0.0)),
}


def _filled_late_hit_at_once(dev, be, name):
    """(under the delayed stream 0, under stream 1 at once, a synchronous call afterwards), the geometry cache empty at
    the start: all three see ONE filling of it."""
    make, cached, tol = GEOMETRY_CALLS[name]
    fn = make(dev)
    torch.cuda.synchronize()
    with dm.dirty(dm.HUGE_BYTES):
        a, b = _two_streams(be, fn)
        sync = host(fn())
    return a, b, sync, cached, tol


@pytest.mark.parametrize("name", list(GEOMETRY_CALLS))
def test_geometry_filled_under_a_delayed_stream_and_hit_from_another(dev, be, name):
    """ksum / nmodes (/ musum) come out of device._geom_cache: to the byte those of a synchronous call made after
    everything ran.  The sums over the data are held to that call as the function's own test holds them (tolerances of
    tests/test_gpu_fftpower2d.py as in the registry; the fused psum is bit-identical on repeat)."""
    a, b, sync, cached, tol = _filled_late_hit_at_once(dev, be, name)
    assert int(np.asarray(sync[cached[-1]]).sum()) > 0                      # nmodes: there is a geometry to miss
    for got, what in ((a, "the filling call"), (b, "the hit from the second stream")):
        assert so.same_bits([got[i] for i in cached], [sync[i] for i in cached]), what
        rest = [i for i in range(len(sync)) if i not in cached]
        assert not rest or so.close([got[i] for i in rest], [sync[i] for i in rest], *tol), what


def test_control_geometry_handed_out_without_the_wait(dev, be, monkeypatch):
    """Planted: the hand-over of device._geom_cached is switched off (a foreign stream's wait_event does nothing), so the
    entry is handed out as the parent handed it out.  The fill sits behind a sleep of D: the second stream copies a
    geometry that is not there yet."""
    monkeypatch.setattr(torch.cuda.Stream, "wait_event", lambda self, event: None)
    a, b, sync, cached, tol = _filled_late_hit_at_once(dev, be, "power_bin_1d")
    monkeypatch.undo()
    assert so.same_bits([a[i] for i in cached], [sync[i] for i in cached])
    assert not so.same_bits([b[i] for i in cached], [sync[i] for i in cached])


# ------------------------------------------------------------------ rocFFT plans: one per stream
ROCFFT_SIDE = 99                            # float64: 48, 96 and 100 plan without a work buffer, an odd side has one


def _rocfft_two_grids(dev, n):
    """((r2c, grid a, grid b), (c2r, spectrum a, spectrum b)) of side ``n``, float64, through rocFFT."""
    fa, fb = (dev.as_device(so._cube(n, np.float64, seed)) for seed in (1, 2))
    sa, sb = (dev.as_device(so._half_spectrum(n, np.complex128, seed)) for seed in (1, 2))
    return ((lambda f: dev.r2c(f, engine="rocfft")), fa, fb), ((lambda s: dev.c2r(s.clone(), (n, n, n))), sa, sb)


def _four_calls_two_streams(be, call, xa, xb):
    """call(xa) and call(xb) alternating over two streams, all four let go by ONE event behind a null-stream sleep."""
    s0, s1, null = be.stream(0), be.stream(1), torch.cuda.default_stream()
    with dm.dirty(dm.HUGE_BYTES):
        be.sleep(null, so.TARGET_MS)
        go = be.record()
        outs = []
        for s, x in ((s0, xa), (s1, xb), (s0, xa), (s1, xb)):
            s.wait_event(go)
            with torch.cuda.stream(s):
                outs.append(be.clone(call(x)))
        return host(outs)


def test_fft_plan_two_streams_at_the_same_time(dev, hip, be):
    """r2c and c2r of two different float64 grids of a side the hand-written passes refuse, four calls alternating over
    two streams that ONE event lets go: every plan has a work buffer, and the parent's cache gave both streams the same
    plan.  Now the key holds the stream."""
    from astrild_amd import _lib
    n = ROCFFT_SIDE
    assert not hip.ast_fft64_supported(n)
    args = {"r2c": (_lib.FFT_R2C, _lib.F64, (n, n, n), 1, 1.0 / (n * n * n), False), "c2r": (_lib.FFT_C2R, _lib.F64, (n, n, n), 1, 1.0, False)}
    s0, s1 = be.stream(0), be.stream(1)
    for kind, a in args.items():
        work = dev.fft_plan(*a).work_bytes
        print(f"\nSTREAM_ORDER rocFFT {kind} float64 {n}^3: work buffer {work} bytes")
        assert work > 0, f"{kind} at side {n} has no work buffer: two streams in one plan would share nothing"
        with torch.cuda.stream(s0):                                         # two streams, two plans; one stream, one plan
            p0, again = dev.fft_plan(*a), dev.fft_plan(*a)
        with torch.cuda.stream(s1):
            p1 = dev.fft_plan(*a)
        assert p0 is again and p0 is not p1 and p0.handle.value != p1.handle.value and p1 is not dev.fft_plan(*a)
    for call, xa, xb in _rocfft_two_grids(dev, n):
        ref_a, ref_b = host(call(xa)), host(call(xb))
        assert not so.same_bits(ref_a, ref_b)
        for got, want in zip(_four_calls_two_streams(be, call, xa, xb), (ref_a, ref_b, ref_a, ref_b)):
            assert so.same_bits(got, want)


def test_clear_plan_cache_drops_the_plans_of_every_stream(dev, be):
    from astrild_amd import _lib
    a = (_lib.FFT_R2C, _lib.F64, (16, 16), 1, 1.0, False)
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(dev, "_plan_cache", {})                                  # (the session's plans stay)
        with torch.cuda.stream(be.stream(0)):
            p0 = dev.fft_plan(*a)
        p = dev.fft_plan(*a)
        assert len(dev._plan_cache) == 2 and p is not p0
        torch.cuda.synchronize()
        dev.clear_plan_cache()
        assert not dev._plan_cache and dev.fft_plan(*a) is not p
    finally:
        torch.cuda.synchronize()
        mp.undo()


# ------------------------------------------------------------------ what a call returns is the caller's
_OWNED = [c for c in so.CASES if not c.shares]      # (``shares``: the words of a docstring, tests/test_stream_order_cpu.py)


@pytest.mark.parametrize("c", _OWNED, ids=[c.name for c in _OWNED])
def test_outputs_are_the_callers(dev, lens, be, c):
    """Every device tensor among the outputs is overwritten in place with the dirty pattern; the next call must not
    notice.  (Fresh inputs for each call: an output that IS an input - an in-place operation - is the caller's too.)"""
    ins, dec = c.make()
    fn = lambda *a: c.call(dev, lens, *a)
    up = lambda: ins if c.host_inputs else [be.upload(a) for a in ins]
    with so.environment(c.env), dm.dirty(dm.HUGE_BYTES):
        ref = host(fn(*up()))
        out = fn(*up())
        torch.cuda.synchronize()
        so.tree_map(lambda t: dm.fill_bytes(t, dm.HUGE_BYTES) if t.is_cuda else t, out)
        torch.cuda.synchronize()
        again = host(fn(*up()))
    want = ref if c.oracle is None else c.oracle(*ins)
    assert _compare(c, ref, want, ins), "the first result misses the reference"
    assert _compare(c, again, want, ins), "after the caller overwrote what the call before had returned"


# ------------------------------------------------------------------ explicit objects handed from stream to stream (rule 3)
def _hand_over(be, first, second):
    """first() under a delayed S1, S2.wait_stream(S1), second() under S2."""
    s1, s2 = be.stream(0), be.stream(1)
    be.sleep(s1, so.TARGET_MS)
    with torch.cuda.stream(s1):
        a = so.tree_map(be.clone, first())
    s2.wait_stream(s1)
    with torch.cuda.stream(s2):
        b = so.tree_map(be.clone, second())
    return host(a), host(b)


@pytest.mark.parametrize("nc", [128, 100], ids=["hand_written_128", "embedded_100"])
def test_lens_plan_handed_over(dev, lens, be, nc):
    bsz = float(np.deg2rad(3.0))
    kd = dev.as_device(so._kappa(nc)(1)[0])
    ref_phi, ref_alphas = host(lens.LensPlan(nc, bsz).phi(kd)), host(lens.LensPlan(nc, bsz).alphas(kd))
    with dm.dirty(dm.HUGE_BYTES):
        plan = lens.LensPlan(nc, bsz)
        phi, alphas = _hand_over(be, lambda: plan.phi(kd), lambda: plan.alphas(kd))
    assert so.same_bits(phi, ref_phi) and so.same_bits(alphas, ref_alphas)


@pytest.mark.parametrize("npix", [64, 256])
def test_smooth_plan_handed_over(dev, lens, be, npix):
    img = dev.as_device(so._kappa(npix)(1)[0])
    ref_real = host(lens.SmoothPlan(npix).gaussian(img.clone(), 1.2, "gaussian"))
    ref_fft = host(lens.SmoothPlan(npix).gaussian(img.clone(), 3.0, "gaussianFFT"))
    with dm.dirty(dm.HUGE_BYTES):
        plan = lens.SmoothPlan(npix)
        plan.gaussian(img.clone(), 3.0, "gaussianFFT")             # the periodic route's weights are cached in the plan
        real, fft = _hand_over(be, lambda: plan.gaussian(img.clone(), 1.2, "gaussian"),      # ... and overwritten here
                               lambda: plan.gaussian(img.clone(), 3.0, "gaussianFFT"))
    assert so.same_bits(real, ref_real) and so.same_bits(fft, ref_fft)


def test_tpcf_workspace_handed_over(dev, hip, be):
    from astrild_amd import _lib
    pos = so._pairs(1)[0]
    n, L = len(pos), so.L_PAIR
    s_edges, mu_edges = so._S_EDGES, so._MU_EDGES
    ns, nmu = len(s_edges) - 1, len(mu_edges) - 1
    ref = tpcf_orc.pair_counts(pos, L, s_edges, mu_edges)
    assert ref.sum() > 1000
    p, s_d, mu_d = dev.as_device(pos), dev.as_device(s_edges), dev.as_device(mu_edges)
    ws_bytes = hip.ast_tpcf_workspace_bytes(n, ns, nmu)
    torch.cuda.synchronize()
    with dm.dirty(dm.HUGE_BYTES):
        work = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        bounds = torch.empty(6, dtype=torch.float64, device="cuda")
        counts = torch.empty((ns, nmu), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def prepare():
            _lib.check(hip.ast_tpcf_prepare(dev.ptr(p), _lib.F64, None, _lib.F64, 2, L, n, dev.ptr(work), ws_bytes,
                                            dev.ptr(bounds), dev.stream()), "ast_tpcf_prepare")
            return bounds

        def count():
            _lib.check(hip.ast_tpcf_pair_counts(dev.ptr(work), ws_bytes, n, L, 2, dev.ptr(s_d), ns, dev.ptr(mu_d), nmu, 0,
                                                dev.ptr(counts), dev.stream()), "ast_tpcf_pair_counts")
            return counts
        got_bounds, got = _hand_over(be, prepare, count)
    assert np.array_equal(got, ref)
    assert np.allclose(got_bounds[:3], pos.min(0)) and np.allclose(got_bounds[3:], pos.max(0))
