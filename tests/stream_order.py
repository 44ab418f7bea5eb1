"""The order of device work: a probe that shows whether a call queues ALL its work on the caller's stream, and the
registry of the entry points it is pointed at (tests/test_gpu_stream_order.py on the GPU, tests/test_stream_order_cpu.py
for the registry, the decoys and the bookkeeping without one).  A helper module: no test functions.

``late_call(fn, inputs, decoys)`` runs ``fn`` under a side stream S while
  * the DEFAULT stream sits in a sleep of 3 D: a launch that went to the null stream is held back, and the consumer - clones
    of every output, queued on S right behind the call - copies an unfinished output;
  * S itself sits in a sleep of D, behind which a PRODUCER overwrites the device inputs - valid decoys until then - with
    the real ones: work sent to another stream without waiting for S reads the decoy.
Outputs the wrapper allocates come back dirty (tests/dirty_memory.py, 0x7F) in the GPU tests, so an unwritten output is
not right by accident.  ``armed`` - the producer had not run when the call returned on the host - says whether the
first half of the check had power for this call; a wrapper that reads a device value on the host waits for the
producer and is checked by the null-stream sleep and the consumer only (``Case.host_syncs``, with the line that reads).

D: ``torch.cuda._sleep`` is timed once per session with a pair of events and the cycle count for TARGET_MS = 40 ms taken
from that.  On the MI355X: 2.40 M cycles per millisecond, so D = 40 ms is 96 M cycles and the null stream's 3 D sleep
289 M.  Nothing relies on D being long enough: every case asserts
``armed`` against the registry and the control tests plant the mistakes the probe is for.  The first launch of a kernel
loads its code object, which waits for the device - and clears ``armed`` -, so every case runs on the default stream
and once plainly under S before the probed run.
"""
import contextlib
import dataclasses
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

TARGET_MS = 40.0
MAX_STREAMS = 3                            # pooled side streams; with the default stream: four alive in the process


# ------------------------------------------------------------------ trees of outputs
def tree_map(f, v):
    """``f`` over the tensors of an output (tensor, tuple / list / dict of outputs); everything else - numpy arrays,
    Python numbers, None: values that are on the host already - is kept as it is."""
    if isinstance(v, torch.Tensor):
        return f(v)
    if isinstance(v, dict):
        return {k: tree_map(f, x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return tuple(tree_map(f, x) for x in v)
    return v


def leaves(v):
    """The leaves of an output as numpy arrays, dicts in key order."""
    if isinstance(v, dict):
        for k in sorted(v):
            yield from leaves(v[k])
    elif isinstance(v, (tuple, list)):
        for x in v:
            yield from leaves(x)
    elif isinstance(v, torch.Tensor):
        yield v.detach().cpu().numpy()
    elif v is not None:
        yield np.asarray(v)


def same_bits(a, b):
    a, b = list(leaves(a)), list(leaves(b))
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and
                                    np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
                                    for x, y in zip(a, b))


def close(a, b, rtol, atol_rel=0.0):
    """numpy's assert_allclose leaf by leaf: integers exact; floats |a - b| <= rtol |b| + atol_rel max|b| (the absolute
    term only where the test the tolerance is taken from has one), NaN exactly where the reference is NaN."""
    a, b = list(leaves(a)), list(leaves(b))
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x.shape != y.shape:
            return False
        if x.dtype.kind in "iub" or y.dtype.kind in "iub":
            if not np.array_equal(x, y):
                return False
            continue
        if x.dtype.kind == "c":
            x, y = x.view(x.real.dtype), y.view(y.real.dtype)
        x, y = x.astype(np.float64), y.astype(np.float64)
        fin = np.isfinite(y)
        if not np.array_equal(np.isnan(x), np.isnan(y)) or not np.isfinite(x[fin]).all():
            return False
        scale = float(np.abs(y[fin]).max()) if fin.any() else 0.0
        if fin.any() and not np.all(np.abs(x[fin] - y[fin]) <= rtol * np.abs(y[fin]) + atol_rel * scale):
            return False
    return True


# ------------------------------------------------------------------ the device side of the probe
class CudaBackend:
    """What late_call needs of the device; tests/test_stream_order_cpu.py drives late_call with a host stand-in."""

    def __init__(self):
        self._pool = []
        self._cycles_per_ms = None

    def stream(self, i=0):
        """Pooled side stream ``i``.  The runtime maps streams onto a few hardware queues, and two streams on one queue run
        in the order they were fed: behind a stream that shares the null stream's queue the consumer would wait for a
        launch that strayed there, and the probe would see nothing.  So a stream enters the pool only after it was seen
        to run beside the null stream and beside the streams already pooled; the others are dropped.
        This departs from "at most four torch streams" and "no retry loops" as first planned: the POOL holds three
        streams and only they carry work, but finding them may take more torch.cuda.Stream objects (torch hands out its
        own pooled streams round robin and never destroys them), and the search is a bounded loop.  With four hardware
        queues three side streams beside the null stream need all four distinct; a runtime with fewer fails the
        assertion below, which says so, rather than running a probe that cannot see."""
        assert 0 <= i < MAX_STREAMS
        tried = 0
        while len(self._pool) <= i:
            tried += 1
            assert tried <= 16, "no stream was found that runs beside the null stream and the pooled streams"
            s = torch.cuda.Stream()
            if all(self.runs_beside(s, other) and self.runs_beside(other, s)
                   for other in [torch.cuda.default_stream()] + self._pool):
                self._pool.append(s)
        return self._pool[i]

    def runs_beside(self, s, busy, ms=8.0):
        """Does work queued on ``s`` run while ``busy`` sleeps?"""
        torch.cuda.synchronize()
        self.sleep(busy, ms)
        with torch.cuda.stream(busy):
            still = self.record()
        with torch.cuda.stream(s):
            marker = torch.zeros(1, device="cuda")
            done = self.record()
        done.synchronize()
        beside = not still.query()
        torch.cuda.synchronize()
        del marker
        return beside

    def default_stream(self):
        return torch.cuda.default_stream()

    def on(self, s):
        return torch.cuda.stream(s)

    def cycles_per_ms(self):
        if self._cycles_per_ms is None:
            torch.cuda.synchronize()
            torch.cuda._sleep(1_000_000)                      # (first launch: module load)
            probe = 20_000_000
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(probe)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            assert ms > 0.05, f"torch.cuda._sleep({probe}) took {ms} ms: it cannot be calibrated"
            self._cycles_per_ms = probe / ms
        return self._cycles_per_ms

    def sleep(self, s, ms):
        with torch.cuda.stream(s):
            torch.cuda._sleep(int(self.cycles_per_ms() * ms))

    def upload(self, a):
        """A device copy on the current stream of a host array; anything that is not an array passes through."""
        if isinstance(a, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
        if isinstance(a, torch.Tensor):
            return a.to("cuda").clone()
        return a

    def overwrite(self, dst, src):
        if isinstance(dst, torch.Tensor):
            dst.copy_(src, non_blocking=True)

    def record(self):
        e = torch.cuda.Event()
        e.record()
        return e

    def done(self, e):
        return e.query()

    def clone(self, t):
        return t.clone()

    def wait_all(self, s):
        s.synchronize()
        torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def cuda_backend():
    return CudaBackend()


def late_call(fn, inputs, decoys, host_inputs=False, backend=None):
    """``(outputs, armed)`` of ``fn(*device_inputs)`` under a pooled side stream S behind a late producer (module
    docstring).  ``inputs`` / ``decoys``: lists of host arrays (None and plain values pass through unchanged).
    ``host_inputs``: the wrapper under test takes host arrays only - its producer is inside itself - and gets ``inputs``
    as they are; it is still checked through the null-stream sleep and the consumer.  The outputs are clones made on S
    right behind the call, returned after S and the device have been waited for."""
    be = backend or cuda_backend()
    assert len(inputs) == len(decoys)
    S = be.stream(0)
    real = [be.upload(a) for a in inputs]                      # staged on the default stream, complete before the sleeps
    be.wait_all(S)
    with be.on(S):
        dev = [be.upload(d) for d in decoys]                   # 1. the decoys, under S
    be.sleep(be.default_stream(), 3 * TARGET_MS)               # 2. the null stream is busy for 3 D, S for D
    be.sleep(S, TARGET_MS)
    with be.on(S):
        for dst, src in zip(dev, real):                        # 3. the producer, behind S's sleep
            be.overwrite(dst, src)
        produced = be.record()
        out = fn(*(list(inputs) if host_inputs else dev))      # 4. the call under test
        armed = not be.done(produced)                          # 5. had the producer run when it returned?
        out = tree_map(be.clone, out)                          # 6. the consumer
    be.wait_all(S)                                             # 7.
    return out, armed


# ------------------------------------------------------------------ the registry
@dataclasses.dataclass
class Case:
    """One entry family.  ``make()`` -> (inputs, decoys), host arrays; ``call(dev, lens, *inputs)`` -> outputs.
    ``covers``: the public functions of device.py (plain names) and lensing.py ("lensing." + name) it runs.
    ``compare``: "equal" (the function's own test asserts bit-identity or exact integers: torch.equal with the
    default-stream result) or ``(rtol, atol_rel)`` exactly as the named test (``tol_from``) has them - atol_rel in units
    of the reference's largest magnitude, 0.0 where that test has no absolute term - for sums whose order of addition
    is not fixed.  The reference of a tolerance case, first match: ``verify(got, *inputs)``, the named test's own
    assertion against its own oracle; ``oracle(*inputs)`` under ``compare``; else the default-stream result - for
    spectra whose own test compares two GPU routes with that tolerance, or whose oracle that test already holds the
    default-stream result to: what is asked here is that the stream changes nothing beyond the order of atomic additions.
    ``host_syncs`` / ``sync_line``: the wrapper reads a device value on the host, and where.
    ``check(*inputs)``: the argument validator the inputs - and the decoys - must pass.
    For tests/input_layouts.py: ``mutates`` - the indices of the inputs the call is documented to write; ``refuses`` -
    {input index: variant names}, the COMPLETE list of re-layouts of an input the call may refuse because the wrapper
    asserts a contiguous tensor ("offset" never: a contiguous tensor of the right dtype is valid input everywhere);
    ``refused_by`` - the functions (named as in ``covers``, private helpers of device.py included) whose source holds
    that ``is_contiguous`` check.
    ``shares`` / ``shares_doc``: the outputs are NOT the caller's to overwrite - the reason is a sentence of the
    docstring of the function ``shares_doc`` names (as in ``covers``) which says that the result is shared or owned by a
    plan (tests/test_stream_order_cpu.py holds the field to that docstring).  Explicit plan objects only: no hidden cache
    hands out its own memory.
    ``geometry_leaves``: the leaves of the output (numbered as ``leaves`` yields them) that are the shell geometry's
    float sums, for the cases that compare bitwise.  They are sums of float64 atomics: the same to the last bit while
    the geometry stays cached, not between two fills (tests/input_layouts.py keeps one cache per case for that
    reason).  A test that empties the cache between the reference and the call compares these leaves with
    GEOMETRY_TOL, the tolerance the geometry's own test holds them to, and every other leaf as the case says."""
    name: str
    covers: tuple
    make: object
    call: object
    compare: object = "equal"
    tol_from: str = ""
    oracle: object = None
    verify: object = None
    host_syncs: bool = False
    sync_line: str = ""
    host_inputs: bool = False
    check: object = None
    env: dict = dataclasses.field(default_factory=dict)
    mutates: tuple = ()
    refuses: dict = dataclasses.field(default_factory=dict)
    refused_by: tuple = ()
    shares: str = ""
    shares_doc: str = ""
    geometry_leaves: tuple = ()


#: ksum of a refilled geometry cache against the one before: tests/test_gpu_fftpower2d.py holds the power_bin_1d / 2d
#: sums to each other and to the oracle with rtol 1e-12, no atol
GEOMETRY_TOL = (1e-12, 0.0)

#: what a contiguity assert refuses of a 1-D or 3-D input, and of a square map or an (N, 3) table
_NC, _NCT = frozenset({"strided"}), frozenset({"strided", "transposed"})
_PAINT_REFUSES = dict(refuses={0: _NCT, 1: _NC}, refused_by=("_check_paint_tensors",))
CASES = []


def case(**kw):
    CASES.append(Case(**kw))


def _rng(seed):
    return np.random.default_rng(seed)


def _two(f):
    """(inputs, decoys) from one generator run with two seeds."""
    return lambda: (f(1), f(2))


# ---- paint
N_MESH, L_BOX = 64, 1000.0


def _particles(dtype, masses=True):
    def gen(seed):
        from oracle import mesh as omesh
        pos = omesh.lattice_particles(32, N_MESH, L_BOX, seed=seed, dtype=dtype)
        mass = _rng(seed + 10).uniform(0.5, 2.0, size=len(pos)).astype(dtype) if masses else None
        return [pos, mass]
    return gen


def _check_particles(pos, mass):
    assert pos.ndim == 2 and pos.shape[1] == 3 and np.isfinite(pos).all()
    assert mass is None or (mass.shape == (len(pos),) and (mass > 0).all())


def _paint_oracle(window):
    def ref(pos, mass):
        from oracle import mesh as omesh
        return omesh.paint(pos, mass, N_MESH, L_BOX, window)
    return ref


PAINT_TOL = {np.float32: 2e-6, np.float64: 1e-12}             # test_paint_random_particles_with_mass
for _dtype in (np.float32, np.float64):
    for _window in ("cic", "tsc"):
        _id = f"{_window}_{np.dtype(_dtype).name}"
        case(name=f"paint_direct_{_id}", covers=("paint",), make=_two(_particles(_dtype)), check=_check_particles,
             call=lambda dev, lens, p, m, w=_window: dev.paint(p, m, N_MESH, L_BOX, w, method="direct"),
             compare=(PAINT_TOL[_dtype],) * 2, tol_from="tests/test_gpu_mesh.py::test_paint_random_particles_with_mass",
             oracle=_paint_oracle(_window), host_syncs=True, sync_line="paint: nd = int(dropped.item())", **_PAINT_REFUSES)
        for _method in ("tiled", "tiled2"):
            case(name=f"paint_{_method}_{_id}", covers=("paint",), make=_two(_particles(_dtype)), check=_check_particles,
                 call=lambda dev, lens, p, m, w=_window, me=_method: dev.paint(p, m, N_MESH, L_BOX, w, method=me,
                                                                                accumulate=False),
                 host_syncs=True, sync_line="_mass_bound: flag_max.tolist(); paint: st.cpu().tolist(), dropped.item()",
                 **_PAINT_REFUSES)
case(name="paint_tiled_unchecked", covers=("paint",), make=_two(_particles(np.float32, masses=False)),
     check=_check_particles,
     call=lambda dev, lens, p, m: dev.paint(p, None, N_MESH, L_BOX, "cic", method="tiled", accumulate=False,
                                            check_dropped=False), **_PAINT_REFUSES)
case(name="paint_direct_unchecked", covers=("paint",), make=_two(_particles(np.float32, masses=False)),
     check=_check_particles,
     call=lambda dev, lens, p, m: dev.paint(p, None, N_MESH, L_BOX, "tsc", method="direct", check_dropped=False),
     compare=(PAINT_TOL[np.float32],) * 2, tol_from="tests/test_gpu_mesh.py::test_paint_random_particles_with_mass",
     oracle=_paint_oracle("tsc"), **_PAINT_REFUSES)
case(name="paint_accumulate_tiled", covers=("paint",), make=_two(_particles(np.float64)), check=_check_particles,
     call=lambda dev, lens, p, m: dev.paint(p, m, N_MESH, L_BOX, "cic", method="tiled",
                                            out=torch.zeros((N_MESH,) * 3, dtype=p.dtype, device=p.device)),
     compare=(PAINT_TOL[np.float64],) * 2, tol_from="tests/test_gpu_mesh.py::test_paint_random_particles_with_mass",
     oracle=_paint_oracle("cic"), host_syncs=True, sync_line="paint: nd = int(dropped.item())", **_PAINT_REFUSES)


def _lattice(npside, nmesh, seed, dtype):
    from oracle import mesh as omesh
    return [omesh.lattice_particles(npside, nmesh, L_BOX, seed=seed, dtype=dtype), None]


@functools.lru_cache(maxsize=None)
def _lattice_128(seed):
    pos = _lattice(128, 256, seed, np.float32)[0]
    return pos


def _staged_paint(dev, lens, pos, mass):
    """A full group / walk / fold cycle of the staged paint (an explicit object: made and used under one stream)."""
    out = torch.empty((N_MESH,) * 3, dtype=pos.dtype, device=pos.device)
    sp = dev.StagedPaint(pos, mass, N_MESH, L_BOX, "cic", out)
    sp.group()
    for r in range(sp.nrows_total):
        sp.walk(r, 1)
    sp.fold(0, sp.nrows_total)
    sp.check()
    return out


case(name="staged_paint", covers=("StagedPaint.group", "StagedPaint.walk", "StagedPaint.fold"),
     make=_two(_particles(np.float32)), check=_check_particles, call=_staged_paint,
     host_syncs=True, sync_line="StagedPaint.__init__: _mass_bound(mass); check(): int(self.dropped.item())", **_PAINT_REFUSES)


def _xsorted_particles(seed):
    return [_lattice_128(seed), None]


case(name="paint_xsorted_two_streams", covers=("paint",), make=_two(_xsorted_particles), check=_check_particles,
     env={"AST_PAINT_XSTREAMS": "2", "AST_PAINT_XCHUNK_MB": "1"},
     call=lambda dev, lens, p, m: dev.paint(p, None, 256, L_BOX, "cic", method="tiled", accumulate=False, hint="xsorted",
                                            check_dropped=False), **_PAINT_REFUSES)


def _defer_fold(dev, lens, p, m):
    grid, halo = dev.paint(p, None, 128, L_BOX, "cic", method="tiled", accumulate=False, defer_fold=True,
                           check_dropped=False, hint="ordered")
    return dev.power_sums_fused64(grid, L_BOX, halo=halo)


case(name="paint_defer_fold_halo_f64", covers=("paint", "power_sums_fused64"),
     make=_two(lambda seed: _lattice(64, 128, seed, np.float64)),
     check=_check_particles, call=_defer_fold, compare=(1e-11, 0.0), tol_from="tests/test_gpu_fft_tile.py: psum of power_sums_fused64 against power_bin_1d, two GPU routes, rtol 1e-11, no atol",
     **_PAINT_REFUSES)


def _unit_cube(seed):
    r = _rng(seed)
    return [r.uniform(0.0, 1.0, 5001) for _ in range(3)] + [r.standard_normal(5001)]


def _check_unit(x, y, z, v):
    assert all(((a >= 0) & (a < 1)).all() for a in (x, y, z)) and np.isfinite(v).all()


case(name="ngp_assign", covers=("ngp_assign",), make=_two(_unit_cube), check=_check_unit,
     call=lambda dev, lens, x, y, z, v: dev.ngp_assign(x, y, z, v, 16),
     host_syncs=True, sync_line="ngp_assign: nd = int(dropped.item())")


def _pos_vel(n, box, sigma, dtype=np.float64):
    def gen(seed):
        r = _rng(seed)
        return [r.uniform(0.0, box, (n, 3)).astype(dtype), r.normal(0.0, sigma, (n, 3)).astype(dtype)]
    return gen


def _check_in_box(box):
    def check(pos, *rest):
        assert pos.shape[1] == 3 and (pos >= 0).all() and (pos <= box).all()
        assert all(a is None or np.isfinite(a).all() for a in rest)
    return check


case(name="rsd_shift", covers=("rsd_shift",), make=_two(_pos_vel(5001, 500.0, 3000.0)), check=_check_in_box(500.0),
     call=lambda dev, lens, p, v: dev.rsd_shift(p, v, 500.0, los=2),
     host_syncs=True, sync_line="rsd_shift: float(v) for v in torch.aminmax(res[:, los])",
     refuses={0: _NCT, 1: _NCT}, refused_by=("rsd_shift",))
case(name="synth_particles", covers=("synth_lattice_particles", "synth_clustered_particles"), make=lambda: ([], []),
     call=lambda dev, lens: (dev.synth_lattice_particles(32, 64, L_BOX, seed=5, dtype=torch.float32),
                             dev.synth_lattice_particles(32, 64, L_BOX, seed=5, shuffle=True, dtype=torch.float64),
                             dev.synth_clustered_particles(32, 64, L_BOX, seed=5, nattractors=16)))
case(name="total_mass", covers=("total_mass",), make=_two(lambda seed: [_rng(seed).uniform(0.5, 2.0, 70001)]),
     call=lambda dev, lens, m: dev.total_mass(m, m.numel()),
     host_syncs=True, sync_line="total_mass: float(out[0].item())")
def _ordered_and_not():
    """The lattice in lattice order; the decoy: as many particles without any order in memory."""
    pos = _particles(np.float32, masses=False)(1)
    return pos, [_rng(2).uniform(0.0, L_BOX, pos[0].shape).astype(np.float32), None]


case(name="paint_input_probes", covers=("sample_is_unordered", "probe_input"), make=_ordered_and_not,
     check=_check_particles,
     call=lambda dev, lens, p, m: (dev.sample_is_unordered(p, N_MESH, L_BOX, fraction=True),
                                   dev.probe_input(p, N_MESH, L_BOX)),
     host_syncs=True, sync_line="sample_is_unordered: int(cnt.item()); probe_input: out.cpu().tolist()")


# ---- fused power
@functools.lru_cache(maxsize=None)
def _cube(n, dtype, seed):
    a = _rng(seed).standard_normal((n, n, n), dtype=dtype) + dtype(1.0)
    return a


def _field(n, dtype):
    return lambda seed: [_cube(n, dtype, seed)]


def _check_finite(*arrays):
    assert all(a is None or np.isfinite(a).all() for a in arrays)


case(name="power_sums_fused_lowk_256", covers=("power_sums_fused", "shell_geometry"), make=_two(_field(256, np.float32)),
     check=_check_finite, call=lambda dev, lens, f: dev.power_sums_fused(f, L_BOX, mean=1.0, lowk=True), geometry_leaves=(0,))
case(name="power_sums_fused_nolowk_256", covers=("power_sums_fused",), make=_two(_field(256, np.float32)),
     check=_check_finite, call=lambda dev, lens, f: dev.power_sums_fused(f, L_BOX, mean=1.0, lowk=False), geometry_leaves=(0,))


def _fused_halo(dev, lens, p, m):
    grid, halo = dev.paint(p, None, 256, L_BOX, "cic", method="tiled", accumulate=False, defer_fold=True,
                           check_dropped=False, offset=p.shape[0] / 256.0 ** 3, hint="ordered")
    return dev.power_sums_fused(grid, L_BOX, halo=halo, lowk=True)


case(name="power_sums_fused_halo_256", covers=("power_sums_fused", "paint"), make=_two(_xsorted_particles),
     check=_check_particles, call=_fused_halo, geometry_leaves=(0,), **_PAINT_REFUSES)
case(name="power_sums_fused64_f64_128", covers=("power_sums_fused64",), make=_two(_field(128, np.float64)),
     check=_check_finite, call=lambda dev, lens, f: dev.power_sums_fused64(f, L_BOX), compare=(1e-11, 0.0),
     tol_from="tests/test_gpu_fft_tile.py: psum of power_sums_fused64 against power_bin_1d, two GPU routes, rtol 1e-11, no atol")
case(name="power_sums_fused64_f32_128", covers=("power_sums_fused64",), make=_two(_field(128, np.float32)),
     check=_check_finite, call=lambda dev, lens, f: dev.power_sums_fused64(f, L_BOX), compare=(1e-11, 0.0),
     tol_from="tests/test_gpu_fft_tile.py: psum of power_sums_fused64 against power_bin_1d, two GPU routes, rtol 1e-11, no atol")
case(name="power_sums_fused64_big32_256", covers=("power_sums_fused64",), make=_two(_field(256, np.float32)),
     check=_check_finite, call=lambda dev, lens, f: dev.power_sums_fused64(f, L_BOX, mean=1.0), geometry_leaves=(0,))
case(name="paint_power_1d_256", covers=("paint_power_1d",), make=_two(_xsorted_particles), check=_check_particles,
     call=lambda dev, lens, p, m: dev.paint_power_1d(p, None, 256, L_BOX, "cic"),
     host_syncs=True, sync_line="paint -> total_mass / dropped.item(); finish_power: t.cpu().numpy()",
     geometry_leaves=(0,))                                      # (the dict of finish_power: "k" = ksum / nmodes comes first)
case(name="fftpower_1d_64", covers=("fftpower_1d", "power_bin_1d", "r2c"), make=_two(_field(64, np.float64)),
     check=_check_finite, call=lambda dev, lens, f: dev.fftpower_1d(f, L_BOX), compare=(1e-12, 0.0),
     tol_from="tests/test_gpu_fftpower2d.py: power_bin_1d / 2d sums against each other and the oracle, rtol 1e-12, no atol",
     host_syncs=True, sync_line="finish_power: t.cpu().numpy()")
case(name="fftpower_2d_64", covers=("fftpower_2d", "power_bin_2d", "shell_geometry_2d"), make=_two(_field(64, np.float64)),
     check=_check_finite, call=lambda dev, lens, f: dev.fftpower_2d(f, L_BOX, Nmu=5, los=2, poles=(0, 2, 4)),
     compare=(1e-12, 1e-12), tol_from="tests/test_gpu_fftpower2d.py: rtol 1e-12, and for the multipoles (signed sums) an atol of 1e-12 of the monopole; here of the leaf's own largest value, which is no larger",
     host_syncs=True, sync_line="finish_power_2d: t.cpu().numpy()")
case(name="power_bin_1d_2d_device", covers=("power_bin_1d", "power_bin_2d", "r2c"), make=_two(_field(64, np.float64)),
     check=_check_finite,
     call=lambda dev, lens, f: (dev.power_bin_1d(dev.r2c(f), None, 64, L_BOX),
                                dev.power_bin_2d(dev.r2c(f), None, 64, L_BOX, Nmu=5, los=2, poles=(0, 2, 4))),
     compare=(1e-12, 1e-12), tol_from="tests/test_gpu_fftpower2d.py: rtol 1e-12, and for the multipoles (signed sums) an atol of 1e-12 of the monopole; here of the leaf's own largest value, which is no larger",
     refuses={0: _NC}, refused_by=("r2c",))


def _catalogue(seed):
    r = _rng(seed)
    return [r.uniform(0.0, L_BOX, (20000, 3)), r.uniform(0.5, 2.0, 20000), r.normal(0.0, 300.0, (20000, 3))]


case(name="catalog_power_1d_64", covers=("catalog_power_1d", "catalog_mesh_complex", "interlace_compensate",
                                         "triple_product_sum"),
     make=_two(_catalogue), check=_check_in_box(L_BOX),
     call=lambda dev, lens, p, m, v: dev.catalog_power_1d(p, m, 64, L_BOX, "tsc"),
     compare=(1e-9, 1e-9), tol_from="tests/test_gpu_fftpower2d.py::test_catalog_power_2d_in_redshift_space: rtol 1e-9, atol 1e-9 of the top (direct paint: float atomics)",
     host_syncs=True, sync_line="total_mass: out[0].item(); paint: dropped.item(); finish_power: t.cpu().numpy()")
case(name="catalog_power_2d_64", covers=("catalog_power_2d", "rsd_shift"), make=_two(_catalogue), check=_check_in_box(L_BOX),
     call=lambda dev, lens, p, m, v: dev.catalog_power_2d(p, m, 64, L_BOX, "tsc", vel1=v, Nmu=5, los=2),
     compare=(1e-9, 1e-9), tol_from="tests/test_gpu_fftpower2d.py::test_catalog_power_2d_in_redshift_space: rtol 1e-9, atol 1e-9 of the top (direct paint: float atomics)",
     host_syncs=True, sync_line="rsd_shift: torch.aminmax; total_mass: out[0].item(); finish_power_2d: t.cpu().numpy()")
case(name="lowk_modes_shell_sums", covers=("lowk_modes", "lowk_shell_sums"), make=_two(_field(256, np.float32)),
     check=_check_finite,
     call=lambda dev, lens, f: (lambda modes: (modes, dev.lowk_shell_sums(modes, 256, L_BOX)))(dev.lowk_modes(f, 256)),
     refuses={0: _NC}, refused_by=("lowk_modes",))


# ---- transforms
def _spectrum(n, cdtype):
    return lambda seed: [_half_spectrum(n, cdtype, seed)]


@functools.lru_cache(maxsize=None)
def _half_spectrum(n, cdtype, seed):
    real = np.float32 if cdtype == np.complex64 else np.float64
    a = _rng(seed).standard_normal((n, n, n // 2 + 1, 2), dtype=real).view(cdtype)[..., 0]
    return a


case(name="r2c_rocfft_64", covers=("r2c", "fft_plan", "FFTPlan.execute"), make=_two(_field(64, np.float32)),
     check=_check_finite, call=lambda dev, lens, f: dev.r2c(f, engine="rocfft"), refuses={0: _NC}, refused_by=("r2c",))
case(name="r2c_tile_256", covers=("r2c",), make=_two(_field(256, np.float32)), check=_check_finite,
     call=lambda dev, lens, f: dev.r2c(f, engine="tile"), refuses={0: _NC}, refused_by=("r2c",))
case(name="r2c_fft64_128", covers=("r2c",), make=_two(_field(128, np.float64)), check=_check_finite,
     call=lambda dev, lens, f: dev.r2c(f), refuses={0: _NC}, refused_by=("r2c",))
case(name="c2r_rocfft_64", covers=("c2r", "fft_plan", "FFTPlan.execute"), make=_two(_spectrum(64, np.complex128)),
     check=_check_finite, call=lambda dev, lens, s: dev.c2r(s.clone(), (64, 64, 64)))
case(name="c2r_tile_256", covers=("c2r_tile",), make=_two(_spectrum(256, np.complex64)), check=_check_finite,
     call=lambda dev, lens, s: (dev.c2r_tile(s), dev.c2r_tile(s, m_lo=3, m_hi=9)), refuses={0: _NC}, refused_by=("c2r_tile",))
case(name="c2r_tile_batch_256", covers=("c2r_tile_batch", "tile_work_pitch"), make=_two(_spectrum(256, np.complex64)),
     check=_check_finite,
     call=lambda dev, lens, s: dev.c2r_tile_batch(
         s, [(1, 4), (4, 9), (9, 20)],
         [torch.empty((256, 256, dev.tile_work_pitch(256)), dtype=torch.complex64, device=s.device) for _ in range(3)]),
     refuses={0: _NC}, refused_by=("c2r_tile_batch",))
case(name="shell_filter_64", covers=("shell_filter",), make=_two(_spectrum(64, np.complex128)), check=_check_finite,
     call=lambda dev, lens, s: (dev.shell_filter(s, 64, 3, 9), dev.shell_filter(None, 64, 3, 9, dtype=torch.complex128)),
     refuses={0: _NC}, refused_by=("shell_filter",))


def _three_fields(seed):
    r = _rng(seed)
    return [r.standard_normal((64, 64, 64)) for _ in range(3)]


case(name="triple_product_sums_64", covers=("triple_product_sums",), make=_two(_three_fields),
     check=_check_finite,      # (repeated calls are torch.equal in tests/test_gpu_bispectrum_kernels.py)
     call=lambda dev, lens, a, b, c: dev.triple_product_sums({0: a, 1: b, 2: c}, [(0, 1, 2), (0, 0, 1), (2, 2, 2)]),
     host_syncs=True, sync_line="triple_product_sums: torch.tensor(...).to(device()) - a pageable upload waits for the stream",
     refuses={0: _NC, 1: _NC, 2: _NC}, refused_by=("triple_product_sums",))
case(name="bispectrum_32", covers=("bispectrum",), make=_two(_field(32, np.float64)), check=_check_finite,
     call=lambda dev, lens, f: (lambda r: (r["B"], r["ntri"]))(dev.bispectrum(f, L_BOX, [1, 4, 8, 12],
                                                                              [(0, 0, 0), (0, 1, 1), (1, 1, 2), (0, 1, 2)])),
     compare=(1e-8, 1e-9), tol_from="tests/test_gpu_api.py::test_bispectrum_3d_vs_oracle: rtol 1e-8, atol 1e-9 of the largest |B|",
     host_syncs=True, sync_line="bispectrum: triple_product_sums(...).cpu().numpy()", refuses={0: _NC}, refused_by=("r2c",))


# ---- grid operations
def _vector_grid(shape, dtype):
    return lambda seed: [_rng(seed).standard_normal(shape + (3,)).astype(dtype)]


def _check_vector_grid(v):
    from astrild_amd import device
    device.check_divergence_args(v.shape, v.dtype, 0.5)


for _periodic in (False, True):
    for _variant in ("0", "1"):
        case(name=f"divergence_{'periodic' if _periodic else 'edges'}_{'tiled' if _variant == '1' else 'cell'}",
             covers=("divergence",), make=_two(_vector_grid((16, 17, 18), np.float64)), check=_check_vector_grid,
             env={"ASTRILD_DIVERGENCE_TILED": _variant},
             call=lambda dev, lens, v, per=_periodic: dev.divergence(v, 0.5, periodic=per))
case(name="vector_magnitude", covers=("vector_magnitude",), make=_two(_vector_grid((16, 17, 18), np.float32)),
     check=_check_finite, call=lambda dev, lens, v: dev.vector_magnitude(v))
case(name="spectral_divergence_16", covers=("spectral_divergence",),
     make=_two(lambda seed: [_spectrum(16, np.complex128)(seed + k)[0] for k in range(3)]), check=_check_finite,
     call=lambda dev, lens, a, b, c: dev.spectral_divergence(a, b, c, 16, L_BOX),
     refuses={0: _NC, 1: _NC, 2: _NC}, refused_by=("spectral_divergence",))
case(name="velocity_divergence_power_32", covers=("velocity_divergence_power",),
     make=_two(_vector_grid((32, 32, 32), np.float64)), check=_check_finite,
     call=lambda dev, lens, v: dev.velocity_divergence_power(v, L_BOX), compare=(1e-12, 0.0),
     tol_from="tests/test_gpu_fftpower2d.py: power_bin_1d / 2d sums against each other and the oracle, rtol 1e-12, no atol",
     host_syncs=True, sync_line="finish_power: t.cpu().numpy()")


# ---- lensing
def _planes(seed):
    return [(_rng(seed).standard_normal((5, 64, 64)) * 0.01)]


_WNUM, _WDEN = np.linspace(0.5, 1.5, 5), np.linspace(2.0, 1.0, 5)
case(name="kappa_stack_weighted", covers=("lensing.kappa_stack",), make=_two(_planes), check=_check_finite,
     call=lambda dev, lens, p: lens.kappa_stack(p, _WNUM, _WDEN), refuses={0: _NC}, refused_by=("lensing.kappa_stack",))
case(name="convert_units_add", covers=("lensing.convert_code_to_phy_units", "lensing.add"), make=_two(_planes),
     check=_check_finite,
     call=lambda dev, lens, p: lens.add(lens.convert_code_to_phy_units("kappa_2", p[0].clone()), p[1]))

_PLANS = {}


def _explicit_plan(lens, kind, *args):
    """One explicit plan per (kind, arguments), made by the warm-up run and used by the late one."""
    if (kind, args) not in _PLANS:
        _PLANS[kind, args] = getattr(lens, kind)(*args)
    return _PLANS[kind, args]


def _kappa(nc):
    return lambda seed: [_rng(seed).standard_normal((nc, nc)) * 0.01]


for _nc in (128, 100):
    case(name=f"lens_plan_alphas_phi_{_nc}", covers=("lensing.LensPlan.alphas", "lensing.LensPlan.phi"),
         make=_two(_kappa(_nc)), check=_check_finite,
         call=lambda dev, lens, k, nc=_nc: (_explicit_plan(lens, "LensPlan", nc, float(np.deg2rad(3.0))).alphas(k),
                                            _explicit_plan(lens, "LensPlan", nc, float(np.deg2rad(3.0))).phi(k)))
for _npix in (64, 256):
    for _kind, _sigma in (("gaussianFFT", 3.0), ("gaussianFFT", 1.0), ("gaussian", 1.2), ("gaussian_mirror", 1.5)):
        case(name=f"smooth_plan_{_kind}_{_sigma}_{_npix}", covers=("lensing.SmoothPlan.gaussian",), make=_two(_kappa(_npix)),
             check=_check_finite,
             call=lambda dev, lens, k, n=_npix, kd=_kind, sg=_sigma: _explicit_plan(lens, "SmoothPlan", n).gaussian(k.clone(), sg, kd),
             # (in place: the clone of a strided view is contiguous, the clone of a transposed map keeps its strides)
             refuses={0: frozenset({"transposed"})}, refused_by=("lensing.SmoothPlan.gaussian",))
case(name="resize_antialiased_96_24", covers=("lensing.resize_antialiased", "lensing.smooth_plan"), make=_two(_kappa(96)),
     check=_check_finite, call=lambda dev, lens, k: lens.resize_antialiased(k, 24))
case(name="histogram_minmax", covers=("lensing.histogram", "lensing.minmax", "lensing.PendingHistogram.__init__"),
     make=_two(_kappa(64)), check=_check_finite,
     call=lambda dev, lens, k: (lens.histogram(k, 20), lens.histogram(k, 20, range=(-0.02, 0.02)), lens.minmax(k)),
     host_syncs=True, sync_line="PendingHistogram.result: event.synchronize(); histogram: counts.cpu(); minmax: out.cpu()")
case(name="order_statistics_percentile", covers=("lensing.order_statistics", "lensing.percentile"), make=_two(_kappa(64)),
     check=_check_finite,
     call=lambda dev, lens, k: (lens.order_statistics(k, [0, 17, 4095]), lens.percentile(k, [5.0, 50.0, 99.5])),
     host_syncs=True, sync_line="ast_order_statistics writes its results into a host array (ctypes out)")
case(name="peak_find_129", covers=("lensing.peak_find",), make=_two(_kappa(129)), check=_check_finite,
     call=lambda dev, lens, k: lens.peak_find(k),
     host_syncs=True, sync_line="peak_find: n = int(count.item())", refuses={0: _NCT}, refused_by=("lensing.peak_find",))
_L_EDGES = np.linspace(200.0, 4000.0, 9)
case(name="flat_power_spectrum_64", covers=("lensing.flat_power_spectrum",), make=_two(_kappa(64)), check=_check_finite,
     call=lambda dev, lens, k: lens.flat_power_spectrum(k, 3.0, _L_EDGES),
     compare=(1e-12, 1e-14), tol_from="tests/test_gpu_map_statistics.py: flat power against the oracle, rtol 1e-12, atol 1e-14 of the largest",
     host_syncs=True, sync_line="flat_power_spectrum: as_device(l_edges) (pageable upload), psum.cpu()")
case(name="flat_bispectrum_64", covers=("lensing.flat_bispectrum_equilateral",), make=_two(_kappa(64)),
     check=_check_finite, call=lambda dev, lens, k: lens.flat_bispectrum_equilateral(k, 3.0, _L_EDGES),
     compare=(1e-9, 1e-12), tol_from="tests/test_gpu_map_statistics.py: flat bispectrum against the oracle, rtol 1e-9, atol 1e-12 of the largest",
     host_syncs=True, sync_line="flat_bispectrum_equilateral: triple_product_sum(...).item()")
_CL = 1.0 / (np.arange(3000) + 10.0) ** 2
case(name="gaussian_random_map_64", covers=("lensing.gaussian_random_map", "lensing.gaussian_random_spectrum"),
     make=lambda: ([], []),
     call=lambda dev, lens: lens.gaussian_random_map(64, 3.0, _CL, seed=7, realisation=2, nreal=2),
     host_syncs=True, sync_line="gaussian_random_spectrum: as_device(cl) (pageable upload waits for the stream)")


def _haloes(seed):
    r, nh, npix = _rng(seed), 6, 128
    return [{"r200_deg": r.uniform(0.02, 0.08, nh), "r200_pix": r.integers(4, 12, nh).astype(float),
             "m200": 10 ** r.uniform(13, 14.5, nh), "c_NFW": r.uniform(2, 8, nh), "Dc": r.uniform(500, 2000, nh),
             "theta1_pix": r.integers(-5, npix + 5, nh), "theta2_pix": r.integers(-5, npix + 5, nh),
             "theta1_tv": r.normal(0, 300, nh), "theta2_tv": r.normal(0, 300, nh)}]


case(name="nfw_paint_128", covers=("lensing.nfw_paint",), make=_two(_haloes), host_inputs=True,
     call=lambda dev, lens, cat: (lens.nfw_paint(cat, 3, [0, 1], True, 2, 128, "dT"),
                                  lens.nfw_paint(cat, 3, [0], True, 2, 128, "alpha")),
     host_syncs=True, sync_line="nfw_paint: as_device(...) of the catalogue columns (pageable uploads)")


def _patch(seed):
    r = _rng(seed)
    return [r.standard_normal((37, 37)), r.standard_normal((9, 9)), r.standard_normal((37, 37))]


case(name="add_patch_shear_37", covers=("lensing.add_patch", "lensing.deflection_to_shear"), make=_two(_patch),
     check=_check_finite,
     call=lambda dev, lens, big, small, other: (lens.add_patch(big.clone(), small, (3, 35)),
                                               lens.deflection_to_shear(big, other, 0.01)),
     # (add_patch writes its first argument: the clone of a transposed map keeps its strides)
     refuses={0: frozenset({"transposed"})}, refused_by=("lensing.add_patch",))


def _filters(dev, lens, img, _small, _other):
    from astrild_amd.rays.utils.filters import Filters
    return (Filters.gaussian(img, 3.0, theta_i=5.0), Filters.gaussian_high_pass(img, 3.0, theta_i=5.0),
            Filters.gaussian_third_derivative(img, 3.0, 0.2, 0), Filters.gaussian_first_derivative(img, 3.0, 0.2, 1),
            Filters.apodization(img), Filters.gaussian_third_derivative_convolution(img, 3.0, 0.1, 1),
            Filters.gaussian_compensated(img, 3.0, 0.2, 0.4), Filters.aperture_photometry(img.clone(), 3.0, 0.3))


case(name="filters_37", covers=("lensing.smooth_plan", "lensing.SmoothPlan.gaussian"), make=_two(_patch), check=_check_finite,
     call=_filters, host_syncs=True,
     sync_line="Filters.gaussian_compensated: to_device(window) (pageable upload); ast_gaussian_smooth: pageable weights")


# ---- pair finders
N_OBJ, L_PAIR, TOP = 3000, 100.0, 10.0
_S_EDGES, _MU_EDGES = np.linspace(0.0, TOP, 11), np.linspace(0.0, 1.0, 5)
_RP_EDGES, _PI_EDGES = np.linspace(0.0, TOP, 6), np.linspace(0.0, TOP, 5)
_BOUNDS = "_check_device_bounds(to_numpy(bounds)): the prepare call's bounds are read on the host"


def _pairs(seed):
    r = _rng(seed)
    centres = r.uniform(0.0, L_PAIR, (60, 3))
    pos = np.mod(centres[r.integers(0, 60, N_OBJ)] + r.normal(0.0, 3.0, (N_OBJ, 3)), L_PAIR)
    return [pos, r.normal(0.0, 300.0, (N_OBJ, 3)), r.integers(0, 8, N_OBJ).astype(np.int32)]


def _check_pairs(pos, vel, tags):
    from astrild_amd import device
    assert (pos >= 0).all() and (pos <= L_PAIR).all() and np.isfinite(vel).all() and ((tags >= 0) & (tags < 8)).all()
    device.check_pair_velocity_args(pos.shape, vel.shape, _S_EDGES, boxsize=L_PAIR)
    device.check_jackknife_args(8, pos.shape, tags1_shape=tags.shape, nbins=10)


case(name="tpcf_pair_counts", covers=("tpcf_pair_counts",), make=_two(_pairs), check=_check_pairs,
     call=lambda dev, lens, p, v, t: (dev.tpcf_pair_counts(p, L_PAIR, _S_EDGES, _MU_EDGES),
                                      dev.tpcf_pair_counts(p, L_PAIR, _S_EDGES, vel=v)),
     host_syncs=True, sync_line=_BOUNDS)
case(name="tpcf_cross_counts", covers=("tpcf_cross_counts",), make=_two(_pairs), check=_check_pairs,
     call=lambda dev, lens, p, v, t: (dev.tpcf_cross_counts(p[:2000], p[2000:], _S_EDGES, _MU_EDGES, boxsize=L_PAIR),
                                      dev.tpcf_cross_counts(p, None, _S_EDGES)),
     host_syncs=True, sync_line=_BOUNDS)
case(name="tpcf_jackknife_counts", covers=("tpcf_jackknife_counts",), make=_two(_pairs), check=_check_pairs,
     call=lambda dev, lens, p, v, t: (dev.tpcf_jackknife_counts(p, 2, _S_EDGES, boxsize=L_PAIR),
                                      dev.tpcf_jackknife_counts(p, 8, _S_EDGES, _MU_EDGES, boxsize=L_PAIR, tags1=t)),
     host_syncs=True, sync_line=_BOUNDS)
case(name="rp_pi_counts", covers=("rp_pi_pair_counts", "rp_pi_cross_counts", "rp_pi_jackknife_counts"), make=_two(_pairs),
     check=_check_pairs,
     call=lambda dev, lens, p, v, t: (dev.rp_pi_pair_counts(p, L_PAIR, _RP_EDGES, _PI_EDGES),
                                      dev.rp_pi_cross_counts(p[:2000], p[2000:], _RP_EDGES, _PI_EDGES, boxsize=L_PAIR),
                                      dev.rp_pi_jackknife_counts(p, 2, _RP_EDGES, _PI_EDGES, boxsize=L_PAIR)),
     host_syncs=True, sync_line=_BOUNDS)
_ORACLES = {}


def _once(name, compute):
    """The oracle of a case, computed once and shared by the three results it is held against."""
    if name not in _ORACLES:
        _ORACLES[name] = compute()
    return _ORACLES[name]


def _verify_pair_velocity(got, p, v, t):
    from tests import pair_velocity_oracle as orc
    from tests import test_gpu_pair_velocity as own
    refs = _once("pair_velocity", lambda: (
        orc.moments(p, v, _S_EDGES, boxsize=L_PAIR, kind="radial", with_abs=True),
        orc.moments(p, v, _RP_EDGES, boxsize=L_PAIR, kind="los", pi_max=8.0, with_abs=True)))
    for g, ref in zip(got, refs):
        assert ref[0].sum() > 1000
        own.assert_moments(tuple(np.asarray(x) for x in g), ref)
    return True


def _verify_pairwise_tv(got, p, v, t):
    from tests import pairwise_oracle as orc
    from tests import test_gpu_pairwise as own
    u = p / np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])[:, None]
    ref = _once("pairwise_tv", lambda: orc.pair_sums(p, u, v, 20, 0.5))
    assert ref[2].sum() > 1000
    own.assert_same(tuple(np.asarray(x) for x in got), ref)
    return True


def _verify_pdf(got, p, v, t):
    from tests import pairwise_pdf_oracle as orc
    from tests import test_gpu_pairwise_pdf as own
    refs = _once("pdf", lambda: [orc.pair_pdf(p, v, TOP, 10, 40, kind, 1.0, 50.0) for kind in ("radial", "z_sign")])
    (hist, outside, (count, s1, s2)), (hist_z, outside_z) = got
    assert refs[0]["hist"].sum() > 1000
    own.assert_same(dict(hist=np.asarray(hist), outside=int(outside), count=np.asarray(count), s1=np.asarray(s1),
                         s2=np.asarray(s2)), refs[0])
    own.assert_same(dict(hist=np.asarray(hist_z), outside=int(outside_z)), refs[1])
    return True


case(name="pair_velocity_moments", covers=("pair_velocity_moments",), make=_two(_pairs), check=_check_pairs,
     call=lambda dev, lens, p, v, t: (dev.pair_velocity_moments(p, v, _S_EDGES, boxsize=L_PAIR, kind="radial"),
                                      dev.pair_velocity_moments(p, v, _RP_EDGES, boxsize=L_PAIR, kind="los", pi_max=8.0)),
     compare=(0.0, 0.0), verify=_verify_pair_velocity,
     tol_from="tests/test_gpu_pair_velocity.py::assert_moments against tests/pair_velocity_oracle.py", host_syncs=True,
     sync_line=_BOUNDS)
case(name="pairwise_tv", covers=("pairwise_tv",), make=_two(_pairs), check=_check_pairs,
     call=lambda dev, lens, p, v, t: dev.pairwise_tv(p, v, 20, 0.5),
     compare=(1e-10, 0.0), verify=_verify_pairwise_tv,
     tol_from="tests/test_gpu_pairwise.py::assert_same (RTOL 1e-10, no atol) against tests/pairwise_oracle.py")


def _check_pdf(pos, vel, tags):
    from astrild_amd import device
    device.check_pairwise_pdf_args(pos.shape, vel.shape, TOP, 10, 40, "radial", 1.0, 50.0, 0, None, True)
    _check_pairs(pos, vel, tags)


case(name="pairwise_velocity_pdf", covers=("pairwise_velocity_pdf",), make=_two(_pairs), check=_check_pdf,
     call=lambda dev, lens, p, v, t: (dev.pairwise_velocity_pdf(p, v, TOP, 10, 40, "radial", 1.0, 50.0, moments=True),
                                      dev.pairwise_velocity_pdf(p, v, TOP, 10, 40, "z_sign", 1.0, 50.0)),
     compare=(0.0, 0.0), verify=_verify_pdf,
     tol_from="tests/test_gpu_pairwise_pdf.py::assert_same against tests/pairwise_pdf_oracle.py")


# ---- profiles and finders
def _profile3d(seed):
    r = _rng(seed)
    centres = r.uniform(0.0, L_PAIR, (20, 3))                   # 250 particles around each centre, segment after segment
    pos = np.mod(np.repeat(centres, 250, axis=0) + r.normal(0.0, 6.0, (5000, 3)), L_PAIR)
    return [pos, r.uniform(0.5, 2.0, 5000), r.normal(0.0, 300.0, (5000, 3)), centres]


_P3_EDGES, _P3_RADII = np.linspace(0.0, 2.0, 9), np.linspace(3.0, 8.0, 20)
_P3_SEGMENTS = np.stack([np.arange(20) * 250, np.full(20, 250)], axis=1)


def _check_profile3d(pos, w, v, centres):
    from astrild_amd import device
    device.check_profile3d_args(pos.shape, centres, _P3_RADII, _P3_EDGES, L_PAIR, w.shape, v.shape, None, _P3_SEGMENTS)


_P3_SYNC = "sphere_profiles: prepare() -> to_numpy(bounds)"


def _verify_profile3d(segments):
    def verify(got, pos, w, v, centres):
        from tests import profile3d_oracle as orc
        from tests import test_gpu_profile3d as own
        counts, moments, scale = _once(("profile3d", segments is None), lambda: orc.profiles(
            pos, centres, _P3_RADII, _P3_EDGES, boxsize=L_PAIR, weights=w, vel=v, segments=segments))
        assert counts.sum() > 100
        assert np.array_equal(np.asarray(got[0]), counts)
        own.assert_moments(np.asarray(got[1]), moments, scale)
        return True
    return verify


case(name="sphere_profiles_search", covers=("sphere_profiles",), make=_two(_profile3d), check=_check_profile3d,
     call=lambda dev, lens, p, w, v, c: dev.sphere_profiles(p, c, _P3_RADII, _P3_EDGES, boxsize=L_PAIR,
                                                            weights=w, vel=v),
     compare=(1e-10, 0.0), verify=_verify_profile3d(None),
     tol_from="tests/test_gpu_profile3d.py::assert_moments (RTOL 1e-10 of the sum of |term|) against tests/profile3d_oracle.py",
     host_syncs=True, sync_line=_P3_SYNC)
case(name="sphere_profiles_members", covers=("sphere_profiles",), make=_two(_profile3d), check=_check_profile3d,
     call=lambda dev, lens, p, w, v, c: dev.sphere_profiles(p, c, _P3_RADII, _P3_EDGES, boxsize=L_PAIR,
                                                            weights=w, vel=v, segments=_P3_SEGMENTS),
     compare=(1e-10, 0.0), verify=_verify_profile3d(_P3_SEGMENTS),
     tol_from="tests/test_gpu_profile3d.py::assert_moments (RTOL 1e-10 of the sum of |term|) against tests/profile3d_oracle.py",
     host_syncs=True, sync_line=_P3_SYNC)


def _annuli(seed):
    r = _rng(seed)
    return [r.standard_normal((128, 128))]


_ANN_X, _ANN_Y = np.arange(10) * 11 + 9, np.arange(10) * 7 + 20
_ANN_R = np.arange(10) % 4 + 3
case(name="annulus_profiles_128", covers=("annulus_profiles",), make=_two(_annuli), check=_check_finite,
     call=lambda dev, lens, m: dev.annulus_profiles(m, _ANN_X, _ANN_Y, _ANN_R, 3.0, 10),
     host_syncs=True, sync_line="annulus_profiles: as_device(np.stack([y, x])) (pageable uploads of the work list)")


def _tracers(seed):
    r = _rng(seed)
    flat = r.choice(256 * 256, 200, replace=False)
    return [(flat % 256).astype(np.int32), (flat // 256).astype(np.int32)]


def _check_tracers(x, y):
    from astrild_amd import device
    device.check_tunnels_tracers(x, y, 256)


case(name="tunnels_voids_256", covers=("tunnels_voids",), make=_two(_tracers), check=_check_tracers,
     call=lambda dev, lens, x, y: dev.tunnels_voids(x, y, 256),
     host_syncs=True, sync_line="check_tunnels_tracers: int(x.min()); tunnels_voids: count.cpu()")


def _check_map(img):
    from astrild_amd import device
    device.check_watershed_map(img)
    assert np.isfinite(img).all()


def _watershed(dev, lens, img):
    basins = dev.watershed_basins(img)
    merged = dev.watershed_merge(basins, 0.5)
    exact = {k: v for k, v in basins.items() if k != "sum_f"}
    return exact, {k: v for k, v in merged.items() if k != "sum_f"}, dev.watershed_void_map(basins, merged["void_of_basin"])


case(name="watershed_65", covers=("watershed_basins", "watershed_void_map"),
     make=_two(lambda seed: [_rng(seed).standard_normal((65, 65))]), check=_check_map, call=_watershed,
     host_syncs=True, sync_line="watershed_basins: int(count.item()); ast_watershed_jump's pass loop reads `pending` per pass")


# ---- slab operations (one GPU, no communicator)
def _slab_planes(seed):
    return [(_rng(seed).standard_normal((16, 256, 256)) + 1.0).astype(np.float32)]


def _slab_fft(dev, lens, planes):
    from astrild_amd import slab
    ops = slab.HipSlabOps(torch.float32)
    parts, nloc, n = 2, planes.shape[0], 256
    pitch = ops.spectrum_pitch(n, parts)
    spec = ops.empty((nloc, n, pitch), ops.cdtype)
    packed = ops.zeros((parts, nloc, n // parts, pitch), ops.cdtype)
    mine = ops.zeros((nloc, n // parts, pitch), ops.cdtype)
    ops.fft2d_planes_packed(planes, spec, packed, parts, 0, mine)
    plain = ops.fft2d_planes(planes, ops.empty((nloc, n, n // 2 + 1), ops.cdtype))
    pk = ops.pack(plain, ops.empty((parts, nloc, n // parts, n // 2 + 1), ops.cdtype), parts)
    return packed[1], mine, plain, pk


case(name="slab_fft2d_pack", covers=(), make=_two(_slab_planes), check=_check_finite, call=_slab_fft)


def _slab_block(seed):
    r = _rng(seed)
    shape = (256, 16, 144)
    return [(r.standard_normal(shape) + 1j * r.standard_normal(shape)).astype(np.complex64)]


def _slab_axis0(dev, lens, block):
    from astrild_amd import slab
    ops = _PLANS.setdefault("slab_ops", slab.HipSlabOps(torch.float32))
    psum = ops.zeros((127,), torch.float64)
    ops.fft1d_axis0_power(block.clone(), 1.0 / 256.0 ** 3, 256, L_BOX, 32, psum, 0)
    return psum, ops.fft1d_axis0(block.clone(), 1.0 / 256.0 ** 3)


case(name="slab_axis0_power", covers=(), make=_two(_slab_block), check=_check_finite, call=_slab_axis0)


def _slab_route(dev, lens, pos, mass):
    from astrild_amd import slab
    ops = slab.HipSlabOps(torch.float32)
    counts = ops.route_count(pos, N_MESH, L_BOX, "cic", 4)
    spos, smass = ops.route_scatter(pos, mass, N_MESH, L_BOX, "cic", 4, counts)
    # the order within a slab's range is the order of the scatter's atomics: rows sorted within their range (torch, on
    # the caller's stream)
    rows = torch.cat([spos, smass[:, None]], dim=1)
    part = torch.bucketize(torch.arange(rows.shape[0], device=rows.device), torch.cumsum(counts, 0), right=True)
    for column in (3, 2, 1, 0, None):                           # stable sorts, the last key first
        order = torch.argsort(part if column is None else rows[:, column], stable=True)
        rows, part = rows[order], part[order]
    return counts, rows


case(name="slab_route", covers=(), make=_two(_particles(np.float32)), check=_check_particles, call=_slab_route)


# ------------------------------------------------------------------ what no case runs, by name and with the reason
EXEMPT = {
    "stream": "the helper that names the current stream for all the others: it launches nothing",
}


def covered():
    return {name for c in CASES for name in c.covers}


@contextlib.contextmanager
def environment(env):
    mp = pytest.MonkeyPatch()
    try:
        for k, v in env.items():
            mp.setenv(k, v)
        yield
    finally:
        mp.undo()


# ------------------------------------------------------------------ the registry of hidden state
KINDS = ("event", "per_stream", "built_synchronously", "host_only", "explicit_object")


@dataclasses.dataclass
class Hidden:
    """One thing in the package that outlives a call and holds device memory, a plan, a stream or an event (DESIGN.md,
    Streams, rule 2).  ``where``: the file, relative to the package; ``name``: the module attribute, or the C object.
    ``kind``: how it is handed between streams -
      "event"               an event on the entry, waited for by a foreign stream;
      "per_stream"          keyed by device.stream_key() or by the caller's stream: every stream gets its own;
      "built_synchronously" complete (hipMemcpy, or a fill followed by hipStreamSynchronize) before it is cached;
      "host_only"           no device memory, no stream, no event: host values, mutexes, once-flags;
      "explicit_object"     rule 3: not hidden, or used by one call at a time under a lock - the caller orders it.
    ``filled_by``: Python - the function of the module whose source holds the hand-over (``wait_event`` for "event",
    ``stream_key()`` for "per_stream"); C - the struct whose ``get`` fills a "built_synchronously" table.
    ``clear``: ``clear(monkeypatch)`` makes it cold inside this process (undone with the monkeypatch), or None with
    ``no_clear``, the reason."""
    where: str
    name: str
    holds: str
    kind: str
    filled_by: str = ""
    clear: object = None
    no_clear: str = ""


def _swap_for_empty(module, attr):
    def clear(mp):
        import importlib
        mp.setattr(importlib.import_module(module), attr, {})
    return clear


_FRESH = "lives in the library, which has no entry that drops it: cold only in a fresh process"
_HOST = "host state: nothing on the device to make cold"
_ONCE = "a flag per device that an idempotent attribute call was made: " + _HOST

HIDDEN_STATE = [
    # ---- Python
    Hidden("device.py", "_plan_cache", "rocFFT plans with one hipMalloc'ed work buffer each", "per_stream",
           filled_by="fft_plan", clear=_swap_for_empty("astrild_amd.device", "_plan_cache")),
    Hidden("device.py", "_geom_cache", "shell geometry (ksum, [musum,] nmodes), 1-D and 2-D, with the fill's stream and event",
           "event", filled_by="_geom_cached", clear=_swap_for_empty("astrild_amd.device", "_geom_cache")),
    Hidden("device.py", "_power_scratch", "the one scratch tensor of the fused power paths, with its last use's stream and event",
           "event", filled_by="_power_scratch_for", clear=_swap_for_empty("astrild_amd.device", "_power_scratch")),
    Hidden("device.py", "_tri_cache", "triangle counts of the bispectrum as numpy arrays and floats", "host_only",
           clear=_swap_for_empty("astrild_amd.device", "_tri_cache")),
    Hidden("lensing.py", "_lens_plans", "ONE resident LensPlan (kernel spectra, work buffers)", "per_stream",
           filled_by="lens_plan", clear=_swap_for_empty("astrild_amd.lensing", "_lens_plans")),
    Hidden("lensing.py", "_smooth_plans", "SmoothPlans (rocFFT plans, cached weights)", "per_stream",
           filled_by="smooth_plan", clear=_swap_for_empty("astrild_amd.lensing", "_smooth_plans")),
    # ---- C: tables
    Hidden("csrc/fft_tile.hip", "g_tw", "fp32 twiddle tables per (device, N)", "built_synchronously",
           filled_by="TwiddleCache", no_clear=_FRESH),
    Hidden("csrc/fft_tile.hip", "g_edge", "float64-edge tables per (device, N, boxsize), at most four", "built_synchronously",
           filled_by="EdgeFallCache", no_clear=_FRESH + "; a boxsize no other test uses reaches a cold entry"),
    Hidden("csrc/fft_tile.hip", "g_disc", "disc layouts: host tables and their device copies", "built_synchronously",
           filled_by="DiscCache", no_clear=_FRESH),
    Hidden("csrc/fft_tile.hip", "g_lowk_lane", "lane factors of the fused low-k z sums per (device, N)", "built_synchronously",
           filled_by="LowkLaneCache", no_clear=_FRESH),
    Hidden("csrc/fft_tile.hip", "g_side", "low-k side stream and event pair per (device, caller stream)", "per_stream",
           no_clear=_FRESH),
    Hidden("csrc/fft_three_stage.h", "g_tw", "float64 twiddle tables per (device, length)", "built_synchronously",
           filled_by="TwCache", no_clear=_FRESH),
    Hidden("csrc/cube_fft.hip", "g_tw32", "fp32 twiddle tables per (device, length)", "built_synchronously",
           filled_by="TwCache32", no_clear=_FRESH),
    # ---- C: plans, streams, communicators
    Hidden("csrc/kappa.hip", "g_host_plan", "the lens plan of the libglsg-compatible host entries", "explicit_object",
           no_clear=_FRESH + "; host_lens holds g_host_mutex, works on the null stream and ends with hipDeviceSynchronize"),
    Hidden("csrc/kappa.hip", "g_host_mutex", "the lock of g_host_plan", "host_only", no_clear=_HOST),
    Hidden("csrc/mesh_paint_tiled.hip", "pipes", "SidePipe per device: the x-sorted paint's side stream and events",
           "explicit_object",
           no_clear=_FRESH + "; a pipelined paint holds SidePipe::run, every walk waits for an event of the caller's stream "
                             "and the caller's stream waits for the last walk"),
    Hidden("csrc/mesh_paint_tiled.hip", "mu", "the lock of side_pipe's table", "host_only", no_clear=_HOST),
    Hidden("csrc/mesh_paint_tiled.hip", "g_stamps", "device global: time stamps of the paint's profiling build", "explicit_object",
           no_clear="written only by kernels compiled with the stamp macro on, read by the script that enables it"),
    Hidden("csrc/mesh_paint_tiled.hip", "g_nstamp", "device global: the count beside g_stamps", "explicit_object",
           no_clear="as g_stamps"),
    Hidden("csrc/comm.hip", "g_rccl", "the dlopen'ed RCCL entry points", "host_only", no_clear=_HOST),
    Hidden("csrc/comm.hip", "g_rccl_mu", "the lock of g_rccl", "host_only", no_clear=_HOST),
    Hidden("csrc/fft_plan.hip", "g_setup_once", "rocfft_setup was called", "host_only", no_clear=_HOST),
    Hidden("csrc/util.hip", "g_err", "the thread's last error message", "host_only", no_clear=_HOST),
    Hidden("csrc/util.hip", "g_prof", "the profiler's records: a pair of events per launch site visit, on the launch stream",
           "host_only", no_clear="ast_profile_report waits for every pair and drops them; off unless a script enables it"),
    Hidden("csrc/util.hip", "g_prof_on", "the profiler's switch", "host_only", no_clear=_HOST),
    Hidden("csrc/util.hip", "g_prof_mutex", "the lock of g_prof", "host_only", no_clear=_HOST),
] + [Hidden("csrc/" + f, n, "PerDeviceOnce: the kernel's dynamic-LDS limit was raised on this device", "host_only", no_clear=_ONCE)
     for f, n in (("fft_tile.hip", "attr_once"), ("pairwise_pdf.hip", "attr_once"), ("tpcf.hip", "attr_once"),
                  ("power_bin.hip", "attr_once"), ("power_bin_2d.hip", "attr_once"), ("mesh_paint_tiled.hip", "attr_once"),
                  ("kappa.hip", "y_once"), ("lens_fft.hip", "once"), ("cube_fft.hip", "once"),
                  ("fft_three_stage.h", "once"))]
