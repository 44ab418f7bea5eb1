"""HBM-resident building blocks of the hot path, one Python call per C-ABI entry.

PyTorch-ROCm tensors are used only as device-memory holders (allocation,
streams, lifetime); every computation is a call into ``libastrild_hip.so``.
Arrays follow the reference's layouts: grids are ``(N, N, N)`` C order with
axis 0 slowest (``value_map[x, y, z]``, power_spectrum_3d.py:142-148), particle
positions ``(Np, 3)`` like pmesh's ``paint`` (stats_subfind.py:125-131).
"""
import contextlib
import ctypes as ct
import itertools
import os
import warnings

import numpy as np
import torch

from . import _lib
from ._lib import F32, F64, check

_REAL = {torch.float32: F32, torch.float64: F64}
_CPLX = {torch.complex64: F32, torch.complex128: F64}
_TO_CPLX = {torch.float32: torch.complex64, torch.float64: torch.complex128}
_TO_REAL = {torch.complex64: torch.float32, torch.complex128: torch.float64}


def device():
    if not torch.cuda.is_available():
        raise _lib.AstrildHipError("astrild_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                                   "there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else ct.c_void_p(t.data_ptr())


def as_device(a, dtype=None):
    """numpy / torch -> contiguous CUDA tensor (the H2D hop of the Python API)."""
    if isinstance(a, torch.Tensor):
        t = a.to(device=device(), dtype=dtype or a.dtype)
    else:
        arr = np.ascontiguousarray(a)
        if arr.flags.writeable:
            t = torch.from_numpy(arr).to(device=device(), dtype=dtype)
        else:                                 # a read-only array (a memory map): only copied from, torch's warning is moot
            with warnings.catch_warnings():
                warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
                t = torch.from_numpy(arr).to(device=device(), dtype=dtype)
    return t.contiguous()


def dense(t, align=1):
    """``t`` itself when it is contiguous and its first byte lies on a multiple of ``align`` bytes; otherwise a
    contiguous copy in a fresh allocation (the caching allocator's blocks start on a multiple of 512 bytes).  The ONE
    place where a wrapper fits a caller's tensor to a C entry that reads it flat or demands an alignment (DESIGN.md,
    Input layouts): an aligned, contiguous tensor passes through without a kernel and without an allocation.  Only for
    tensors the call reads; what it writes in place is checked with an assert instead."""
    if t is None or (t.is_contiguous() and t.data_ptr() % align == 0):
        return t
    return t.clone(memory_format=torch.contiguous_format)


def upload_planes(arrays, dtype=torch.float64, flat=True):
    """Equal-sized host arrays -> views into ONE device allocation, plane after plane.  A kernel that reads the same pixel
    of all planes at once (`ast_kappa_stack`: 64 streams) runs 8-10 % faster over one large allocation than over 64
    separate 134 MB blocks of the caching allocator (scripts/micro/kappa_stack_skew.py: 6.3 against 5.7 TB/s - larger
    page-table fragments, fewer translation misses for the 64 concurrent streams).  Arrays of different sizes: one
    allocation each, as before."""
    arrays = [a if isinstance(a, torch.Tensor) else np.ascontiguousarray(a) for a in arrays]
    sizes = {int(np.prod(a.shape)) for a in arrays}
    if len(arrays) < 2 or len(sizes) != 1:
        out = [as_device(a, dtype) for a in arrays]
        return [t.reshape(-1) for t in out] if flat else out
    count = sizes.pop()
    slab = torch.empty((len(arrays), count), dtype=dtype, device=device())
    for p, a in enumerate(arrays):
        src = a if isinstance(a, torch.Tensor) else torch.from_numpy(a)
        slab[p].copy_(src.reshape(-1))
    return [slab[p] if flat else slab[p].view(tuple(arrays[p].shape)) for p in range(len(arrays))]


def to_numpy(t):
    """CUDA tensor -> numpy array (the D2H hop of the Python API).  A large result lands in page-locked memory - torch's caching
    host allocator; the block goes back to its pool when the array is dropped - so that the copy runs at the link's rate: a
    pageable destination gets a third of it (4096^2 float64, 134 MB: 5.6 ms against 16.4)."""
    if t.is_cuda and t.numel() * t.element_size() >= (1 << 20):
        buf = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        buf.copy_(t)
        return buf.numpy()
    return t.cpu().numpy()


def real_code(t):
    try:
        return _REAL[t.dtype]
    except KeyError:
        raise TypeError(f"expected float32/float64 tensor, got {t.dtype}") from None


def profile_enable(on=True):
    check(_lib.lib().ast_profile_enable(int(bool(on))), "ast_profile_enable")


def profile_report():
    """{launch site: (calls, total_ms)} measured with HIP events on the launch stream."""
    buf = ct.create_string_buffer(1 << 16)
    check(_lib.lib().ast_profile_report(buf, len(buf)), "ast_profile_report")
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, ms = line.rsplit(",", 2)
        out[name] = (int(calls), float(ms))
    return out


# ------------------------------------------------------------------ FFT plans
class FFTPlan:
    """Owns one rocFFT plan created through the C-ABI."""

    def __init__(self, kind, dtype_code, lengths, batch=1, scale=1.0, inplace=False, strided=None):
        self.handle = ct.c_void_p()
        L = _lib.lib()
        if strided is None:
            arr = (ct.c_size_t * len(lengths))(*[int(v) for v in lengths])
            check(L.ast_fft_plan_create(ct.byref(self.handle), kind, dtype_code, len(lengths), arr,
                                        int(batch), float(scale), int(bool(inplace))), "ast_fft_plan_create")
        else:
            length, stride, dist = strided
            check(L.ast_fft_plan_create_strided_1d(ct.byref(self.handle), kind, dtype_code, int(length),
                                                   int(stride), int(batch), int(dist), float(scale)),
                  "ast_fft_plan_create_strided_1d")

    @property
    def work_bytes(self):
        return int(_lib.lib().ast_fft_plan_work_bytes(self.handle))

    def execute(self, src, dst=None):
        check(_lib.lib().ast_fft_exec(self.handle, ptr(src), ptr(dst), stream()), "ast_fft_exec")

    def __del__(self):
        try:
            if self.handle:
                _lib.lib().ast_fft_plan_destroy(self.handle)
                self.handle = ct.c_void_p()
        except Exception:
            pass


_plan_cache = {}


def stream_key():
    """(device, handle of the current stream): what the hidden plan caches (``fft_plan`` here, lensing's two) add to their
    keys.  A plan owns ONE set of device buffers, so two streams must never share one; keyed this way every stream gets
    its own (Streams)."""
    return torch.cuda.current_device(), int(torch.cuda.current_stream().cuda_stream)


def fft_plan(kind, dtype_code, lengths, batch=1, scale=1.0, inplace=False, strided=None):
    """The cached rocFFT plan of the CURRENT stream for these parameters.  A plan owns one work buffer (as large as the
    grid for a 3-D transform), so the key holds the stream: two streams that ask for the same transform get a plan and
    a work buffer each and may run side by side; a caller that stays on one stream holds exactly the one plan it held
    before.  Plans of streams that no longer exist stay until :func:`clear_plan_cache`."""
    key = (*stream_key(), kind, dtype_code, tuple(lengths), batch, scale, inplace, strided)
    p = _plan_cache.get(key)
    if p is None:
        p = _plan_cache[key] = FFTPlan(kind, dtype_code, lengths, batch, scale, inplace, strided)
    return p


def clear_plan_cache():
    """Drops every cached plan, those of streams that are gone included (their work buffers are freed with hipFree,
    which waits for the device: work still queued in a plan finishes first)."""
    _plan_cache.clear()


# ------------------------------------------------------------ mass assignment
def ngp_assign(x, y, z, values, npar, dtype=torch.float64):
    """``value_map[(npar*x).astype(int), ...] = values`` with last-write-wins
    (PowerSpectrum3D._read_data, power_spectrum_3d.py:142-148)."""
    x, y, z, values = (as_device(a, dtype) for a in (x, y, z, values))
    n = int(npar)
    grid = torch.empty((n, n, n), dtype=dtype, device=device())
    owner = torch.empty(n * n * n, dtype=torch.int32, device=device())
    dropped = torch.zeros(1, dtype=torch.int64, device=device())
    check(_lib.lib().ast_ngp_assign(ptr(x), ptr(y), ptr(z), ptr(values), real_code(grid), x.numel(), n,
                                    ptr(grid), ptr(owner), ptr(dropped), stream()), "ast_ngp_assign")
    nd = int(dropped.item())
    if nd:
        raise IndexError(f"{nd} particles have coordinates outside [0, 1) (numpy raises for >= 1 and wraps negative "
                         f"indices, i.e. coordinates in [-1, 0), silently; both are rejected here)")
    return grid


def total_mass(mass, npart):
    """Sum of the particle masses in double, fixed order (``npart`` for unit masses)."""
    if mass is None:
        return float(npart)
    mass = dense(mass)
    out = torch.empty(1 + _lib.SUM_PARTS, dtype=torch.float64, device=mass.device)
    check(_lib.lib().ast_sum(ptr(mass), real_code(mass), mass.numel(), ptr(out), stream()), "ast_sum")
    return float(out[0].item())


class PaintHalo:
    """Halo records of a ``paint(..., defer_fold=True)``: the grid is complete only once they are
    folded in, which ``power_sums_fused(grid, ..., halo=)`` does while its z pass loads the rows.
    Keeps the paint's workspace alive."""

    def __init__(self, workspace, rec_ptr, window_code):
        self.workspace, self.rec_ptr, self.window_code = workspace, rec_ptr, window_code


def sample_run_starts(npart, windows=256):
    """First particles of ``windows`` runs of 32 spread evenly over ``npart`` particles, each a multiple of 32 and at most
    npart - 32.  Host integers: a float32 ``linspace`` rounds 2^30 - 32 UP and the last run would start past the end."""
    npart, windows = int(npart), max(2, int(windows))
    assert npart >= 32
    return [min(i * (npart - 32) // (windows - 1) // 32 * 32, npart - 32) for i in range(windows)]


def sample_is_unordered(pos, nmesh, boxsize, shift=0.0, windows=256, fraction=False):
    """Looks at ``windows`` runs of 32 consecutive particles spread over ``pos``: in input with spatial order in memory
    (lattice order, cell- or curve-sorted snapshots, halo by halo) at least 8 particles of a run share the 8 x 8 x 32-cell
    tile of the run's middle particle - that is what the grouping kernel of the tiled paint turns into group records; in
    shuffled input next to none do and the paint belongs on the two-level bucket scatter from the start.  True when fewer
    than a quarter of the runs are groupable (``fraction=True``: that fraction itself).  On the device: ``ast_paint_order_probe`` and ONE 4-byte fetch; CPU tensors
    (tests) go through the same arithmetic in torch."""
    npart = int(pos.shape[0])
    if npart < 64:
        return False
    n = int(nmesh)
    if pos.is_cuda:                                    # one small kernel + a 4-byte fetch (the torch ops below: 0.25 ms)
        pos = dense(pos)
        cnt = torch.empty(1, dtype=torch.int32, device=pos.device)
        check(_lib.lib().ast_paint_order_probe(ptr(pos), real_code(pos), npart, n, float(boxsize), float(shift), int(windows),
                                               ptr(cnt), stream()), "ast_paint_order_probe")
        frac = int(cnt.item()) / max(2, int(windows))
        return frac if fraction else frac < 0.25
    starts = torch.tensor(sample_run_starts(npart, windows), dtype=torch.int64, device=pos.device)
    idx = (starts[:, None] + torch.arange(32, device=pos.device)[None, :]).reshape(-1)
    cell = torch.floor(pos[idx].double() * (n / float(boxsize)) + float(shift)).long() % n
    tile = ((cell[:, 0] // 8) * n + cell[:, 1] // 8) * n + cell[:, 2] // 32
    tile = tile.view(-1, 32)
    groupable = float(((tile == tile[:, 15:16]).sum(dim=1) >= 8).double().mean().item())
    return groupable if fraction else groupable < 0.25


def probe_input(pos, nmesh, boxsize, shift=0.0, windows=256):
    """Looks at the particle array BEFORE a tiled paint (two small kernels, one 24-byte fetch): returns a dict with
    ``groupable`` - the fraction of sampled runs of 32 consecutive particles the grouping kernel could turn into group records
    (:func:`sample_is_unordered`; < 0.25: no spatial order in memory) -, ``overflow`` - the estimated number of particles beyond
    the single pass's fixed tile segments (ast_paint_occupancy_probe: a sample of >= 8 particles per 8 x 8 x 32-cell tile) -
    and ``max_tile`` - the largest estimated tile occupancy.  What ``paint`` makes of them: :func:`first_paint_path`."""
    L = _lib.lib()
    n, npart = int(nmesh), int(pos.shape[0])
    cbytes = int(L.ast_paint_occupancy_probe_bytes(n))
    if cbytes == 0 or npart < 64:
        return None
    ntiles = cbytes // 4
    pos = dense(pos)
    samples = min(npart, max(65536, 8 * ntiles))
    counts = torch.empty(cbytes, dtype=torch.uint8, device=pos.device)
    out = torch.zeros(3, dtype=torch.int64, device=pos.device)       # [overflow, max tile, groupable runs (low 4 bytes)]
    check(L.ast_paint_occupancy_probe(ptr(pos), real_code(pos), npart, n, float(boxsize), float(shift), samples, ptr(counts),
                                      cbytes, ptr(out), stream()), "ast_paint_occupancy_probe")
    check(L.ast_paint_order_probe(ptr(pos), real_code(pos), npart, n, float(boxsize), float(shift), int(windows),
                                  ct.c_void_p(out.data_ptr() + 16), stream()), "ast_paint_order_probe")
    o = out.cpu().tolist()
    return {"overflow": int(o[0]), "max_tile": int(o[1]), "groupable": (int(o[2]) & 0xffffffff) / max(2, int(windows)),
            "mean_tile": npart / ntiles, "samples": samples}


def scatter_late_capacity(dtype, npart):
    """Records the late list of the bucket scatter (AST_PAINT_SCATTERED) holds for ``npart`` particles of ``dtype``:
    npart / 4 at float32, npart / 8 at float64 (ast_paint_scatter_late_capacity, host only)."""
    return int(_lib.lib().ast_paint_scatter_late_capacity(_REAL[dtype], int(npart)))


def scatter_overflow_limit(dtype, npart):
    """The largest estimated overflow (:func:`probe_input`) for which ``paint`` takes the bucket scatter: four fifths of
    the late list (npart / 5 at float32, npart / 10 at float64).  The late list also takes what level A's bucket segments
    cannot hold, so it fills beyond the estimate; what still does not fit is repainted two-pass."""
    return scatter_late_capacity(dtype, npart) * 4 // 5


def synth_clustered_particles(npside, nmesh, boxsize, seed=20240601, sigma_cells=0.5, nattractors=256, amplitude=0.95,
                              shuffle=False, dtype=torch.float32):
    """A clustered synthetic set (ast_synth_clustered_particles): the lattice collapsing onto ``nattractors`` centres - tile
    occupancies ~100 x the mean, like an evolved snapshot - in lattice order or (shuffle) in pseudo-random order."""
    count = int(npside) ** 3
    pos = torch.empty((count, 3), dtype=dtype, device=device())
    check(_lib.lib().ast_synth_clustered_particles(ptr(pos), real_code(pos), count, int(npside), float(boxsize),
                                                   float(sigma_cells) * boxsize / nmesh, int(seed), int(nattractors),
                                                   float(amplitude), int(bool(shuffle)), stream()), "ast_synth_clustered_particles")
    return pos


def auto_paint_method(npart, n, nx, window, hint=None, accumulate=False):
    """What ``paint(method="auto")`` runs (measured on the MI355X, scripts/perf_sparse.py: 256^3 and 512^3 grids, halo-like
    catalogues of 1 ... 64 objects per 8 x 8 x 32-cell tile).  The tiled paint walks every column of the grid, so below ~16
    (CIC) / ~8 (TSC) objects per tile - SubFind haloes on nbins = 1024 - global atomics on a zero-filled grid win:
    "direct".  Above that, catalogues too small for the input probe (< 2^20 objects), or still sparse (< 64 per tile:
    halo catalogues, stats_subfind.py:125-131, clumpy by nature), take the exact two-pass lists - as fast as the single
    pass there and without its per-tile capacity (512^3, 32 per tile, TSC float64: direct 2.7 ms, tiled2 1.45; a clumpy
    256^3 set at 64 per tile: single pass 1.0 ms through its overflow list, tiled2 0.2).  Dense input goes to "tiled"."""
    per_tile = npart * 2048 / max(1, nx * n * n)
    if accumulate:                                   # (adding onto a grid: index lists + atomic tile flush; the round-1 threshold)
        return "tiled" if n % 32 == 0 and npart >= 65536 and per_tile >= 64 else "direct"
    if n % 32 or npart < 65536 or per_tile < (8 if window.lower() == "tsc" else 16):
        return "direct"
    if hint is None and (npart < (1 << 20) or per_tile < 64):
        return "tiled2"
    return "tiled"


def paint_flags(path, accumulate=False, defer_fold=False, xsorted=False):
    """The AST_PAINT_* word of a tiled paint on ``path`` ("single-pass", "scattered", "two-pass").  XSORTED (the "xsorted" hint)
    lives on the overwriting single pass only: a repaint on another path drops it."""
    assert path in ("single-pass", "two-pass") or (path == "scattered" and not accumulate), (path, accumulate)
    flags = (0 if accumulate else _lib.PAINT_OVERWRITE) | (_lib.PAINT_DEFER_FOLD if defer_fold else 0)
    if path == "single-pass":
        return flags | (_lib.PAINT_XSORTED if xsorted and not accumulate else 0)
    return flags | (_lib.PAINT_TWO_PASS if path == "two-pass" else _lib.PAINT_SCATTERED)


def paint_probe_kind(method, accumulate, hint, whole, check_dropped, npart):
    """The probe a tiled paint runs before its first attempt (the table in :func:`paint`): "input" (:func:`probe_input`),
    "order" (:func:`sample_is_unordered` alone - only for callers that synchronise anyway) or None."""
    if method == "tiled2" or accumulate or hint is not None or npart < (1 << 20):
        return None
    return "input" if whole else "order" if check_dropped else None


def first_paint_path(method, accumulate, hint, whole, check_dropped, npart, probed=None, unordered=None, limit=None):
    """The path of a tiled paint's first attempt (the table in :func:`paint`).  ``probed``: what ``probe_input`` returned,
    ``unordered``: what ``sample_is_unordered`` returned (None: not run, :func:`paint_probe_kind`), ``limit``:
    ``scatter_overflow_limit``.  A wrong guess costs time, never correctness.  No spatial order in memory (under a quarter of
    the sampled runs groupable): the bucket scatter, clustered or not - the two-pass variant makes two global atomics per
    particle on such input (1024^3 clustered + shuffled: 130 ms against 24); tiles that overflow their segments go through the
    late list, reserved once per workgroup and chunk.  The list holds a quarter of the particles at float32, an eighth at
    float64: beyond four fifths of that estimated (``limit``), and for clustered input in file order (estimate above
    npart / 64), the exact two-pass variant at once - slow on unordered input, but without any capacity."""
    if method == "tiled2" or hint == "clustered":
        return "two-pass"
    if accumulate or hint in ("xsorted", "ordered"):        # (accumulate: index lists + atomic tile flush, no other path)
        return "single-pass"
    if hint == "scattered":
        return "scattered"
    kind = paint_probe_kind(method, accumulate, hint, whole, check_dropped, npart)
    if kind == "input" and probed is not None:
        if probed["groupable"] < 0.25 and probed["overflow"] <= limit:
            return "scattered"
        if probed["overflow"] > npart // 64:
            return "two-pass"
    return "scattered" if kind == "order" and unordered else "single-pass"


def next_paint_path(path, probed, whole, check_dropped, npart, overflow=None, dropped=None):
    """The path to paint again on after an attempt on ``path``, or None when it stands.  ``probed``: ``probe_input`` gave a
    result for this call; ``overflow`` (the list statistics') and ``dropped``: None when not fetched - ``paint`` reads the drop
    count after a scattered paint of the whole grid that R1 lets stand, 8 bytes.
    R1 (callers that synchronise anyway: ``check_dropped``): too much went through the overflow list.  Particles without spatial
    order in memory overflow the default stray segments: paint again with the two-level bucket scatter.  If that still
    overflows, the input is strongly CLUSTERED (tiles far above twice the mean occupancy): the exact two-pass variant has no
    capacity limit.  A scattered paint of a call the probe informed - unordered AND clustered - keeps its late list: it is the
    fastest path for such input, and the result is complete either way.
    R2: nothing falls outside the whole periodic grid, so a dropped deposit of the bucket scatter is a record its late list had
    no room for (more than the probe estimated, or a "scattered" hint) - never lost, never reported as outside the buffer: the
    exact two-pass lists paint it again."""
    if path == "two-pass":
        return None
    if overflow is not None and check_dropped and overflow > npart // 64 and not (probed and path == "scattered"):
        return "scattered" if path == "single-pass" else "two-pass"
    return "two-pass" if path == "scattered" and whole and dropped else None


def _check_paint_tensors(pos, mass=None, out=None, cells=0):
    assert pos.is_cuda and pos.dim() == 2 and pos.shape[1] == 3 and pos.is_contiguous()
    for t, count in ((mass, pos.shape[0]), (out, cells)):
        assert t is None or (t.is_cuda and t.dtype == pos.dtype and t.numel() == count and t.is_contiguous())


def _max_abs(t, count):
    """max |t| over the first ``count`` elements (ast_minmax, one 16-byte fetch); 1.0 for None, nothing or all zeros: the
    paint's mass bound (what its fixed-point tiles are scaled by), the bispectrum's field amplitude."""
    if t is None or not count:
        return 1.0
    lo_hi = torch.empty(2, dtype=torch.float64, device=t.device)
    check(_lib.lib().ast_minmax(ptr(t), real_code(t), count, ptr(lo_hi), stream()), "ast_minmax")
    return float(lo_hi.abs().max()) or 1.0


def _mass_bound(mass, count):
    """The tiled overwrite paint's mass bound, max |mass| (1.0 for None, nothing or all zeros), what its fixed-point quantum is
    scaled by - and the place where a NaN or Inf mass is refused, before any paint kernel runs: the column walk adds the bit
    pattern of ``fma(NaN, ...)`` as an integer (finite garbage in the cells the particle touches), and one Inf mass makes the
    quantum infinite (the whole grid NaN).  One reduction for both (ast_absmax_finite), one 16-byte fetch."""
    if mass is None or not count:
        return 1.0
    flag_max = torch.empty(2, dtype=torch.float64, device=mass.device)
    check(_lib.lib().ast_absmax_finite(ptr(mass), real_code(mass), count, ptr(flag_max), stream()), "ast_absmax_finite")
    flag, bound = flag_max.tolist()
    if flag != 0.0:
        raise ValueError("paint: a mass is NaN or Inf (the tiled paint accumulates in fixed point, scaled by max |mass|)")
    return bound or 1.0


def _offset_planes(offset_planes):          # (first buffer plane, count) that get the offset; default: all
    return (0, -1) if offset_planes is None else (int(offset_planes[0]), int(offset_planes[1]))


def _paint_in_chunks(chunk, pos, mass, n, boxsize, window, **kw):
    """The tile lists hold 32-bit particle indices: more than 2^32 - 65 particles (2048^3 on the largest grid one GPU
    holds) are painted in chunks - the first one as asked for, the others accumulated onto it through the same LDS tiles."""
    if kw["defer_fold"]:
        raise _lib.AstrildHipError("defer_fold is not available for a paint in chunks (more than 2^32 - 65 particles)")
    if isinstance(kw["offset"], str):        # "mean" means the mean of ALL particles, not of the first chunk
        if kw["offset"] != "mean":
            raise ValueError(kw["offset"])
        kw["offset"] = total_mass(mass, pos.shape[0]) * float(kw["scale"]) / float(n) ** 3
    for a in range(0, pos.shape[0], chunk):
        kw["out"] = paint(pos[a:a + chunk], None if mass is None else mass[a:a + chunk], n, boxsize, window, **kw)
        kw.update(accumulate=True, offset=0.0, hint=None)
    return kw["out"]


def paint(pos, mass, nmesh, boxsize, window="cic", scale=1.0, out=None, method="auto",
          x_start=0, nx_alloc=None, check_dropped=True, accumulate=None, defer_fold=False, offset=0.0,
          hint=None, stats=None, shift=0.0, offset_planes=None):
    """pmesh ``ParticleMesh.paint(pos, mass=, resampler=)`` on the GPU.

    pos: (Np, 3) CUDA tensor (float32/float64); mass: (Np,) or None.
    Returns the grid ``(nx_alloc, nmesh, nmesh)`` in pos.dtype.
    method: "direct" (global float atomics), "tiled" (LDS tiles, single pass over the
    particles), "tiled2" (LDS tiles, exact two-pass counting) or "auto" (:func:`auto_paint_method`).
    accumulate: add into ``out`` (default when ``out`` is given) or overwrite it (default
    for a fresh grid; the tiled path then needs no zero-fill and flushes without atomics).
    defer_fold: (tiled overwrite of the whole grid only) skip the paint's last kernel and return
    ``(grid, PaintHalo)`` for ``power_sums_fused(..., halo=)``; the grid alone is incomplete.
    offset: (tiled overwrite only) owned cells are stored as ``sum - offset``, subtracted in double
    before the one rounding to the grid dtype; ``offset="mean"`` uses total mass * scale / nmesh^3,
    i.e. the grid holds rho - mean (only the DC mode changes, which FFTPower discards).
    hint: what the caller knows of the particles' order in memory (below; a wrong hint costs time, never correctness).
    stats: a dict that receives the list statistics of the tiled overwrite paint, ``path`` and ``attempts``.
    shift: added to every coordinate in grid units (0.5 paints the second mesh of an interlaced pair).
    offset_planes: (first, count) of the buffer planes the offset applies to (default: all) - a slab buffer's
    ghost planes are added onto other ranks' cells and must stay plain sums.

    Paths of a tiled paint: "single-pass" (fixed tile segments, an overflow list for the rest), "scattered"
    (AST_PAINT_SCATTERED: bucket scatter of particles without spatial order in memory, a late list for what the segments
    cannot hold), "two-pass" (AST_PAINT_TWO_PASS: exact index lists, no capacity).  The first attempt's
    (:func:`first_paint_path`), first match, with whole = ``nx_alloc == nmesh and x_start == 0``:
      method "tiled2", or hint "clustered" with "auto" / "tiled"   two-pass
      accumulate                                                   single-pass; no list statistics, no repaint
      hint "scattered" / "ordered"                                 scattered / single-pass
      hint "xsorted" (ascending x: lattice order, slab files)      single-pass, grouping and walk overlapped chunk by chunk
      no hint, >= 2^20 particles, whole (any check_dropped)        probe_input: None -> single-pass; groupable < 0.25 and
                                                                   overflow <= scatter_overflow_limit -> scattered; else
                                                                   overflow > Np // 64 -> two-pass; else single-pass
      no hint, >= 2^20 particles, not whole, check_dropped         sample_is_unordered -> scattered, else single-pass
      otherwise                                                    single-pass
    Repaints after an attempt (overflow list too long, late list full): :func:`next_paint_path`.

    Accuracy (derived in tests/paint_accuracy.py, measured in DESIGN.md 4.1 "Accuracy of a painted cell").  A tiled overwrite
    paint whose overflow / late list stays empty stores in every cell the sum S of its K deposits with
      |cell - (S - offset)| <= K q / 2 + u |S - offset| + (c_h u + c_d 2^-53) (A + |offset|),
    A = sum of |deposits|, u = 2^-24 (float32) or 2^-53 (float64), c_h = 0, 1 or 3 (cells on the border of the 8 x 8 tile
    footprint), c_d = 18 (CIC) or 36 (TSC), and the quantum q = max |mass| * |scale| / 2^k, k = min(50, B - bits), B = 47
    (float32) or 62 (float64), 2^bits > 2 cmax >= 2^(bits - 1), cmax = 5 tile capacities ("tiled": k = 31 / 46 at 1024^3 with
    one particle per cell) or the fullest tile of the cell's tile column ("tiled2").  So a cell whose mean deposit is rho
    times lighter than the heaviest particle's is good to rho / 2^(k + 1) of itself - rho 2^-32 / rho 2^-47 at 1024^3 - and
    deposits below q / 2 vanish; only for rho <= 2^(k - 23) (float32) is that under the rounding of the grid dtype.  The grid
    is bit-reproducible and scales exactly with powers of two in mass, scale and (positions, boxsize).  Deposits made with
    float atomics ("direct", accumulate, the overflow and late lists) form weights and products in the grid dtype: add
    (2 K + 13) u (A + |prefill|) + 3 u D, D = sum over the deposits of |m scale| (wy wz + wx wz + wx wy): a particle leaves an
    error of up to 3 u of its own mass in a cell it touches with a tiny weight.
    A NaN or Inf mass raises ValueError before a tiled overwrite paint launches anything (found by the reduction that computes
    max |mass|); "direct" and accumulating paints have no such reduction and carry it into the cells the particle touches.
    """
    L = _lib.lib()
    n = int(nmesh)
    nx = n if nx_alloc is None else int(nx_alloc)
    _check_paint_tensors(pos, mass)
    code = real_code(pos)
    if accumulate is None:
        accumulate = out is not None
    win = _lib.WIN[window.lower()]
    npart = pos.shape[0]
    # ASTRILD_PAINT_CHUNK (particles) forces chunking at smaller sizes (tests).
    chunk = int(os.environ.get("ASTRILD_PAINT_CHUNK", 0)) or (2 ** 31 if npart >= 2 ** 32 - 65 else 0)
    if chunk and npart > chunk and method != "direct" and win != 0:
        return _paint_in_chunks(chunk, pos, mass, n, boxsize, window, scale=scale, out=out, method=method, x_start=x_start,
                                nx_alloc=nx_alloc, check_dropped=check_dropped, accumulate=accumulate, defer_fold=defer_fold,
                                offset=offset, hint=hint, shift=shift, offset_planes=offset_planes)
    if hint not in (None, "scattered", "xsorted", "clustered", "ordered"):
        raise ValueError(hint)
    if hint == "clustered" and method in ("auto", "tiled"):
        method = "tiled2"
    was_auto = method == "auto"
    if was_auto and win != 0:
        method = auto_paint_method(npart, n, nx, window, hint, accumulate)
    # (no workspace at any flags: a buffer geometry the tiles do not cover)
    use_tiled = method in ("tiled", "tiled2") and win != 0 and npart < 2**32 - 65 and \
        int(L.ast_paint_tiled_workspace_bytes(win, code, npart, n, nx, paint_flags("single-pass", accumulate))) > 0
    if method in ("tiled", "tiled2") and not use_tiled and not was_auto:
        raise _lib.AstrildHipError("tiled paint needs a CIC/TSC window and nmesh a multiple of 32")
    whole = nx == n and int(x_start) == 0
    if defer_fold and not (use_tiled and not accumulate and whole):
        raise _lib.AstrildHipError("defer_fold needs the tiled overwrite paint of the whole periodic grid")
    if out is None:
        out = (torch.empty if use_tiled and not accumulate else torch.zeros)((nx, n, n), dtype=pos.dtype, device=pos.device)
    else:
        _check_paint_tensors(pos, None, out, nx * n * n)
        if not accumulate and not use_tiled:
            out.zero_()
    if offset != 0.0 and not (use_tiled and not accumulate):
        raise _lib.AstrildHipError("offset needs the tiled overwrite paint")
    if isinstance(offset, str):
        if offset != "mean":
            raise ValueError(offset)
        offset = total_mass(mass, npart) * float(scale) / float(n) ** 3
    dropped, nd = torch.zeros(1, dtype=torch.int64, device=pos.device), None
    if use_tiled:
        mass_bound = 1.0 if accumulate else _mass_bound(mass, npart)      # (raises on a NaN / Inf mass: before the probes)
        choice = (method, accumulate, hint, whole, check_dropped, npart)
        kind = paint_probe_kind(*choice)
        probed = probe_input(pos, n, boxsize, shift) if kind == "input" else None
        unordered = sample_is_unordered(pos, n, boxsize, shift) if kind == "order" else None
        path = first_paint_path(*choice, probed, unordered, scatter_overflow_limit(pos.dtype, npart) if probed else None)
        attempts = 0
        while True:
            attempts += 1
            flags = paint_flags(path, accumulate, defer_fold, hint == "xsorted")
            ws_bytes = int(L.ast_paint_tiled_workspace_bytes(win, code, npart, n, nx, flags))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pos.device)
            check(L.ast_paint_tiled(win, code, ptr(pos), ptr(mass), npart, n, float(boxsize), float(scale),
                                    int(x_start), nx, ptr(out), ptr(ws), ws_bytes, ptr(dropped), flags,
                                    mass_bound, float(offset), *_offset_planes(offset_planes), float(shift), stream()),
                  "ast_paint_tiled")
            st, nd = None, None
            if not accumulate and path != "two-pass" and (stats is not None or check_dropped):     # group / stray lists exist
                st = torch.empty(4, dtype=torch.int64, device=pos.device)
                check(L.ast_paint_tiled_list_stats(ptr(ws), win, code, npart, n, nx, flags, ptr(st), stream()),
                      "ast_paint_tiled_list_stats")
                st = dict(zip(("groups", "strays", "overflow", "max_strays_per_tile"), st.cpu().tolist()))
            after = (path, probed is not None, whole, check_dropped, npart, st["overflow"] if st else None)
            again = next_paint_path(*after)
            if again is None and path == "scattered" and whole:
                nd = int(dropped.item())                                # (a zero is reused by the check below)
                again = next_paint_path(*after, nd)
            if again is None:
                break
            dropped.zero_()
            del ws                                # released BEFORE the next attempt's is allocated (peak memory at 1024^3)
            path = again
        if stats is not None:
            stats.update(st or {}, scattered=path == "scattered", attempts=attempts, path=path)
            if probed is not None:
                stats["probe"] = probed
    else:
        check(L.ast_paint(win, code, ptr(pos), ptr(mass), npart, n, float(boxsize), float(scale),
                          int(x_start), nx, ptr(out), ptr(dropped), float(shift), stream()), "ast_paint")
    if check_dropped:
        if nd is None:
            nd = int(dropped.item())
        if nd:
            raise _lib.AstrildHipError(f"{nd} deposits fell outside the grid buffer (x_start={x_start}, nx_alloc={nx})")
    if defer_fold:
        rec = ct.c_void_p()
        check(L.ast_paint_tiled_halo(ptr(ws), win, code, npart, n, nx, flags, ct.byref(rec)), "ast_paint_tiled_halo")
        return out, PaintHalo(ws, rec, win)
    return out


class StagedPaint:
    """The single-pass overwrite paint of ``paint(..., method="tiled", accumulate=False)`` in parts
    (``ast_paint_tiled_stage``): ``group()`` once, then ``walk(row0, nrows)`` and ``fold(row0, nrows)`` per range of tile
    rows (``row_planes`` consecutive buffer planes each, ``nrows_total`` rows), in any order that walks a row's
    neighbours (``fold_needs``) before the row is folded.  After every row has been walked and folded ``out`` equals
    the one-call paint bit for bit.  Calls go to the current stream; the workspace lives as long as the object.
    The reference paints on one rank in one call (stats_subfind.py:130-131); this is what lets the slab pipeline send
    finished planes while the rest of the slab is still being painted."""

    def __init__(self, pos, mass, nmesh, boxsize, window, out, x_start=0, nx_alloc=None, scale=1.0, offset=0.0,
                 offset_planes=None, hint=None, shift=0.0):
        L = _lib.lib()
        self.n = int(nmesh)
        self.nx = self.n if nx_alloc is None else int(nx_alloc)
        _check_paint_tensors(pos, mass, out, self.nx * self.n * self.n)
        if hint not in (None, "scattered"):
            raise ValueError(hint)
        self.pos, self.mass, self.out = pos, mass, out
        self.code = real_code(pos)
        self.win = _lib.WIN[window.lower()]
        self.window = window.lower()
        self.flags = paint_flags("scattered" if hint == "scattered" else "single-pass")
        self.npart = pos.shape[0]
        self.ws_bytes = int(L.ast_paint_tiled_workspace_bytes(self.win, self.code, self.npart, self.n, self.nx, self.flags))
        if self.ws_bytes == 0 or self.win == 0 or self.npart >= 2**32 - 65:
            raise _lib.AstrildHipError("staged paint needs a CIC/TSC window and nmesh a multiple of 32")
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=pos.device)
        self.dropped = torch.zeros(1, dtype=torch.int64, device=pos.device)
        self.mass_bound = _mass_bound(mass, self.npart)
        self.args = (float(boxsize), float(scale), int(x_start), self.nx)
        self.tail = (self.mass_bound, float(offset), *_offset_planes(offset_planes), float(shift))
        self.row_planes = int(L.ast_paint_tile_row_planes())
        self.nrows_total = int(L.ast_paint_tile_rows(self.nx))
        self.periodic = self.nx == self.n and int(x_start) == 0

    def _stage(self, stage, row0, nrows, closed_row0=0, closed_nrows=0):
        check(_lib.lib().ast_paint_tiled_stage(self.win, self.code, ptr(self.pos), ptr(self.mass), self.npart, self.n,
                                               *self.args, ptr(self.out), ptr(self.ws), self.ws_bytes, ptr(self.dropped),
                                               self.flags, *self.tail, int(stage), int(row0), int(nrows), int(closed_row0),
                                               int(closed_nrows), stream()),
              "ast_paint_tiled_stage")

    def fold_needs(self, row):
        """Tile rows whose walk must be complete before ``fold(row, 1)``: the row itself and the neighbours whose
        window reaches into it (CIC deposits reach one plane up, TSC one plane either way)."""
        rows = [row - 1, row] + ([row + 1] if self.window == "tsc" else [])
        if self.periodic:
            return sorted({r % self.nrows_total for r in rows})
        return [r for r in rows if 0 <= r < self.nrows_total]

    def group(self):
        self.dropped.zero_()
        self._stage(_lib.PAINT_STAGE_GROUP, 0, 0)

    def reset(self):
        """Instead of group(), before the first group_part()."""
        self.dropped.zero_()
        self._stage(_lib.PAINT_STAGE_RESET, 0, 0)

    def group_part(self, k, parts, closed_row0=0, closed_nrows=0, span=1):
        """The lists of parts k .. k + span - 1 of `parts` equal parts of the particle array, in one launch (x-ordered input,
        slab buffers).  closed_*: the tile rows walked so far, one range modulo the buffer's rows; a particle that turns up
        for one of them is counted as dropped (check() raises): the order that was promised did not hold."""
        assert 1 <= parts <= 65535 and span >= 1 and 0 <= k and k + span <= parts
        self._stage(_lib.PAINT_STAGE_GROUP_PART, k, parts | ((span - 1) << 16), closed_row0, closed_nrows)

    def walk(self, row0, nrows):
        self._stage(_lib.PAINT_STAGE_WALK, row0, nrows)

    def fold(self, row0, nrows):
        """FOLD of the tile rows [row0, row0 + nrows).  After :meth:`defer_folds` only the rows named there get their records
        added here; the others get their overflow-list deposits only (AST_PAINT_STAGE_LATE) and their records when the
        consumer's z pass loads the planes (:meth:`halo_args`)."""
        if self._explicit_rows is None:
            self._stage(_lib.PAINT_STAGE_FOLD, row0, nrows)
            return
        for explicit, run in itertools.groupby(range(row0, row0 + nrows), key=self._explicit_rows.__contains__):
            self._stage(_lib.PAINT_STAGE_FOLD if explicit else _lib.PAINT_STAGE_LATE, next(run), 1 + len(list(run)))

    _explicit_rows = None

    def defer_folds(self, explicit_rows):
        """From now on only ``explicit_rows`` (the tile rows that hold ghost planes: their planes travel before any transform)
        are folded by fold(); every other row's halo records are added by the z pass that reads its planes
        (ast_fft_tile_rows_r2c_slab_halo) - one kernel and one read-modify-write of the border lines less per row.  The rows
        folded on load must form one range [lo, hi) of the buffer's rows."""
        explicit = set(int(r) for r in explicit_rows)
        rest = [r for r in range(self.nrows_total) if r not in explicit]
        if rest and rest != list(range(rest[0], rest[-1] + 1)):
            raise ValueError("the rows folded on load must be one contiguous range")
        rec = ct.c_void_p()
        check(_lib.lib().ast_paint_tiled_halo(ptr(self.ws), self.win, self.code, self.npart, self.n, self.nx, self.flags, ct.byref(rec)),
              "ast_paint_tiled_halo")
        self._explicit_rows = explicit
        self._halo = (rec, self.win, rest[0] if rest else 0, rest[-1] + 1 if rest else 0)

    def halo_args(self):
        """(record pointer, window code, first tile row folded on load, one past the last) or None."""
        return None if self._explicit_rows is None else self._halo

    def check(self):
        nd = int(self.dropped.item())
        if nd:
            raise _lib.AstrildHipError(f"{nd} deposits fell outside the grid buffer (x_start={self.args[2]}, nx_alloc={self.nx}) "
                                       f"or, with group_part(), belong to a tile row that had been walked already (the particles "
                                       f"do not come in ascending x as promised)")


def synth_lattice_particles(npside, nmesh, boxsize, seed=20240601, sigma_cells=0.5, shuffle=False,
                            dtype=torch.float32, first=0, count=None):
    """Synthetic particle set of SURVEY.md §8(d), generated directly in HBM.  shuffle=True: the particles of the range in
    a pseudo-random order (a fixed permutation keyed by seed + 1); shuffle="stride": t -> t * stride mod count, the
    low-discrepancy order of rounds 1-4 (every chunk of the array feeds every tile almost evenly: a friendlier input)."""
    n3 = int(npside) ** 3
    count = n3 - first if count is None else int(count)
    pos = torch.empty((count, 3), dtype=dtype, device=device())
    stride = 0
    if shuffle == "stride" and count > 1:
        stride = 2654435761 % count or 1
        while np.gcd(stride, count) != 1:
            stride += 1
    elif shuffle and count > 1:
        stride = 2 ** 64 - 1
    check(_lib.lib().ast_synth_lattice_particles(ptr(pos), real_code(pos), int(first), count, int(npside),
                                                 float(boxsize), float(sigma_cells) * boxsize / nmesh,
                                                 int(seed), int(stride), stream()), "ast_synth_lattice_particles")
    return pos


# ---------------------------------------------------------------- 3D spectra
def r2c(field, out=None, engine="auto"):
    """pmesh-normalised forward transform: ``rfftn(field) / Ng``.

    engine "tile": the hand-written three-pass LDS FFT (fp32 cubes of side 256/512/1024, fp64 cubes of side 128 ... 2048);
    "rocfft": the rocFFT 3D R2C plan; "auto": tile when supported.  A field that does not start on a multiple of 16
    bytes (a view into a larger buffer) is transformed from an aligned copy: every engine reads the real rows as pairs."""
    assert field.is_cuda and field.dim() == 3 and field.is_contiguous()
    field = dense(field, 16)
    n0, n1, n2 = field.shape
    code = real_code(field)
    if out is None:
        out = torch.empty((n0, n1, n2 // 2 + 1), dtype=_TO_CPLX[field.dtype], device=field.device)
    L = _lib.lib()
    tile_ok = n0 == n1 == n2 and bool(L.ast_fft_tile_supported(code, n0))
    tile64 = n0 == n1 == n2 and field.dtype == torch.float64 and bool(L.ast_fft64_supported(n0)) and out.is_contiguous()
    if tile64 and engine in ("auto", "tile"):
        check(L.ast_fft64_r2c_3d(ptr(field), ptr(out), n0, 1.0 / float(n0) ** 3, stream()), "ast_fft64_r2c_3d")
        return out
    if engine == "tile" and not tile_ok:
        raise _lib.AstrildHipError("tile FFT supports cubes of side 256, 512 or 1024")
    if tile_ok and engine in ("auto", "tile"):
        check(L.ast_fft_tile_r2c_3d(ptr(field), ptr(out), code, n0, 1.0 / float(n0) ** 3, stream()),
              "ast_fft_tile_r2c_3d")
        return out
    plan = fft_plan(_lib.FFT_R2C, code, (n0, n1, n2), 1, 1.0 / (n0 * n1 * n2), False)
    plan.execute(field, out)
    return out


_geom_cache = {}

#: How lattice vectors of exactly integer norm (they sit on a shell edge) are assigned: "float64" follows the
#: rounding of nbodykit's float64 comparison (the reference's behaviour, as far as its published source fixes it),
#: "integer" assigns them to the shell they open.  See ast_power_bin_1d in include/astrild_hip.h.
DEFAULT_BINNING = "float64"


def _bin_code(binning):
    return _lib.BIN[binning or DEFAULT_BINNING]


def _geom_cached(key, fill):
    """The cached geometry tensors of ``key`` as COPIES on the current stream; ``fill()`` computes them, on the current
    stream, when the key is new.  The entry is (tensors, stream of the fill, event recorded behind the fill): a hit
    under another stream waits for that event first - the fill may still be queued - and tells the allocator about the
    new reader (Streams).  What the caller gets is its own: the cached tensors never leave this function, so
    a caller's ``ksum /= nmodes`` cannot reach the next spectrum of that size (two copies of nmesh/2-1 numbers each)."""
    cur = torch.cuda.current_stream()
    hit = _geom_cache.get(key)
    if hit is None:
        tensors = fill()
        filled = torch.cuda.Event()
        filled.record(cur)
        hit = _geom_cache[key] = (tensors, cur, filled)
    elif hit[1] != cur:
        cur.wait_event(hit[2])
        for t in hit[0]:
            t.record_stream(cur)
    return tuple(t.clone() for t in hit[0])


def shell_geometry(nmesh, boxsize, i0=None, i1=None, binning=None):
    """(sum w|k|, sum w) per shell of a spectrum block — data independent, cached; the caller's own copies."""
    n = int(nmesh)
    i0 = (0, n) if i0 is None else tuple(i0)
    i1 = (0, n) if i1 is None else tuple(i1)
    key = (torch.cuda.current_device(), n, float(boxsize), i0, i1, _bin_code(binning))

    def fill():
        nb = n // 2 - 1
        ksum = torch.zeros(nb, dtype=torch.float64, device=device())
        nmodes = torch.zeros(nb, dtype=torch.int64, device=device())
        check(_lib.lib().ast_power_bin_1d(None, None, F64, n, float(boxsize), int(i0[0]), int(i0[1]),
                                          int(i1[0]), int(i1[1]), ptr(ksum), None, ptr(nmodes), _bin_code(binning), stream()),
              "ast_power_bin_1d[geometry]")
        return ksum, nmodes
    return _geom_cached(key, fill)


def power_bin_1d(spec1, spec2, nmesh, boxsize, i0=None, i1=None, psum=None, binning=None):
    """Shell sums (ksum, psum, nmodes) of a block of the half spectrum (device tensors; ksum and nmodes are copies of
    the cached geometry: the caller's own)."""
    n = int(nmesh)
    nb = n // 2 - 1
    i0 = (0, n) if i0 is None else tuple(i0)
    i1 = (0, n) if i1 is None else tuple(i1)
    assert spec1.is_cuda and spec1.is_contiguous() and spec1.numel() == i0[1] * i1[1] * (n // 2 + 1)
    code = _CPLX[spec1.dtype]
    if spec2 is not None:
        assert spec2.dtype == spec1.dtype and spec2.numel() == spec1.numel() and spec2.is_contiguous()
    if psum is None:
        psum = torch.zeros(nb, dtype=torch.float64, device=spec1.device)
    ksum, nmodes = shell_geometry(n, boxsize, i0, i1, binning)
    check(_lib.lib().ast_power_bin_1d(ptr(spec1), ptr(spec2), code, n, float(boxsize), int(i0[0]), int(i0[1]),
                                      int(i1[0]), int(i1[1]), None, ptr(psum), None, _bin_code(binning), stream()),
          "ast_power_bin_1d")
    return ksum, psum, nmodes


def finish_power(ksum, psum, nmodes):
    """k = ksum/N, P = psum/N on the host; empty shells are NaN like nbodykit's 0/0."""
    ks, ps, nm = (t.cpu().numpy() for t in (ksum, psum, nmodes))
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"k": ks / nm, "power": ps / nm, "modes": nm, "shotnoise": 0.0}


POLES_ALLOWED = (0, 2, 4, 6, 8)
MAX_NMU = 1024


def check_fftpower_2d_args(Nmu, los, poles):
    """Host-only argument check of the (k, mu) / multipole binning: ``(Nmu, los, poles)`` as ints and a tuple, or
    ValueError.  ``Nmu`` in 1 .. 1024; ``los`` a box axis 0, 1 or 2; ``poles`` distinct even orders from
    {0, 2, 4, 6, 8} (may be empty) - the spectrum is folded onto mu in [0, 1] and cannot represent an odd multipole."""
    if isinstance(Nmu, bool) or not isinstance(Nmu, (int, np.integer)) or not 1 <= Nmu <= MAX_NMU:
        raise ValueError(f"Nmu must be an integer in 1 .. {MAX_NMU}, got {Nmu!r}")
    if isinstance(los, bool) or not isinstance(los, (int, np.integer)) or los not in (0, 1, 2):
        raise ValueError(f"los must be a box axis 0, 1 or 2, got {los!r}")
    poles = tuple(() if poles is None else poles)
    for l in poles:
        if isinstance(l, bool) or not isinstance(l, (int, np.integer)) or l not in POLES_ALLOWED:
            raise ValueError(f"poles must be even orders from {POLES_ALLOWED} (odd multipoles vanish on the folded "
                             f"spectrum), got {l!r}")
    if len(set(poles)) != len(poles):
        raise ValueError(f"poles repeat an order: {poles}")
    return int(Nmu), int(los), tuple(int(l) for l in poles)


def _poles_arg(poles):
    return (ct.c_int * max(len(poles), 1))(*poles)


def shell_geometry_2d(nmesh, boxsize, Nmu, los, i0=None, i1=None, binning=None):
    """(sum w|k|, sum w mu, sum w) per (shell, mu bin) of a spectrum block, (nmesh/2-1, Nmu) each - data independent,
    cached; the caller's own copies."""
    Nmu, los, _ = check_fftpower_2d_args(Nmu, los, ())
    n = int(nmesh)
    i0 = (0, n) if i0 is None else tuple(i0)
    i1 = (0, n) if i1 is None else tuple(i1)
    key = (torch.cuda.current_device(), n, float(boxsize), i0, i1, _bin_code(binning), Nmu, los)

    def fill():
        nb = n // 2 - 1
        ksum = torch.zeros((nb, Nmu), dtype=torch.float64, device=device())
        musum = torch.zeros((nb, Nmu), dtype=torch.float64, device=device())
        nmodes = torch.zeros((nb, Nmu), dtype=torch.int64, device=device())
        check(_lib.lib().ast_power_bin_2d(None, None, F64, n, float(boxsize), int(i0[0]), int(i0[1]), int(i1[0]), int(i1[1]),
                                          los, Nmu, None, 0, ptr(ksum), ptr(musum), ptr(nmodes), None, None,
                                          _bin_code(binning), stream()), "ast_power_bin_2d[geometry]")
        return ksum, musum, nmodes
    return _geom_cached(key, fill)


def power_bin_2d(spec1, spec2, nmesh, boxsize, Nmu=5, los=2, poles=(0, 2, 4), i0=None, i1=None, psum=None, polesum=None,
                 binning=None):
    """Wedge and multipole sums (ksum, musum, psum, nmodes, polesum) of a block of the half spectrum (device tensors):
    the first four (nmesh/2-1, Nmu), polesum (len(poles), nmesh/2-1) without the factor 2l + 1 - see ast_power_bin_2d.
    ``psum`` / ``polesum`` given: accumulated into (blocks and ranks add).  ksum, musum and nmodes are copies of the
    cached geometry: the caller's own."""
    Nmu, los, poles = check_fftpower_2d_args(Nmu, los, poles)
    n = int(nmesh)
    nb = n // 2 - 1
    i0 = (0, n) if i0 is None else tuple(i0)
    i1 = (0, n) if i1 is None else tuple(i1)
    assert spec1.is_cuda and spec1.is_contiguous() and spec1.numel() == i0[1] * i1[1] * (n // 2 + 1)
    code = _CPLX[spec1.dtype]
    if spec2 is not None:
        assert spec2.dtype == spec1.dtype and spec2.numel() == spec1.numel() and spec2.is_contiguous()
    if psum is None:
        psum = torch.zeros((nb, Nmu), dtype=torch.float64, device=spec1.device)
    if polesum is None:
        polesum = torch.zeros((len(poles), nb), dtype=torch.float64, device=spec1.device)
    assert psum.dtype == torch.float64 and tuple(psum.shape) == (nb, Nmu) and psum.is_contiguous()
    assert polesum.dtype == torch.float64 and tuple(polesum.shape) == (len(poles), nb) and polesum.is_contiguous()
    ksum, musum, nmodes = shell_geometry_2d(n, boxsize, Nmu, los, i0, i1, binning)
    check(_lib.lib().ast_power_bin_2d(ptr(spec1), ptr(spec2), code, n, float(boxsize), int(i0[0]), int(i0[1]),
                                      int(i1[0]), int(i1[1]), los, Nmu, _poles_arg(poles), len(poles), None, None, None,
                                      ptr(psum), ptr(polesum) if len(poles) else None, _bin_code(binning), stream()),
          "ast_power_bin_2d")
    return ksum, musum, psum, nmodes, polesum


def finish_power_2d(ksum, musum, psum, nmodes, polesum, poles=(0, 2, 4), shotnoise=0.0):
    """Wedges k, mu, power = sums / modes on the host (empty bins NaN like finish_power) and the multipoles
    ``power_l = (2l + 1) polesum_l / modes`` of the 1-D shells, whose k and modes are the wedge sums added over mu."""
    ks, mus, ps, nm, pol = (t.cpu().numpy() for t in (ksum, musum, psum, nmodes, polesum))
    nm1 = nm.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        res = {"k": ks / nm, "mu": mus / nm, "power": ps / nm, "modes": nm, "shotnoise": float(shotnoise),
               "poles": {"k": ks.sum(axis=1) / nm1, "modes": nm1}}
        for q, l in enumerate(poles):
            res["poles"]["power_%d" % l] = (2 * l + 1) * pol[q] / nm1
    return res


def fftpower_2d(field1, boxsize, field2=None, Nmu=5, los=2, poles=(0, 2, 4), binning=None):
    """``FFTPower(first, mode="2d", Nmu=, los=, poles=, kmin=2*pi/L[, second])`` for in-memory grids, the line of sight
    along box axis ``los``: r2c, then the (k, mu) / Legendre binning of the half spectrum (ast_power_bin_2d).  fp32
    grids are transformed in double, as in the non-fused branch of :func:`fftpower_1d` and for its reason."""
    Nmu, los, poles = check_fftpower_2d_args(Nmu, los, poles)
    field1, field2 = dense(field1), dense(field2)
    n = field1.shape[0]
    assert tuple(field1.shape) == (n, n, n) and n % 2 == 0
    if field1.dtype == torch.float32:
        field1 = field1.double()
        field2 = None if field2 is None else field2.double()
    s1 = r2c(field1)
    s2 = None if field2 is None else r2c(field2)
    return finish_power_2d(*power_bin_2d(s1, s2, n, boxsize, Nmu, los, poles, binning=binning), poles=poles)


def rsd_shift(pos, vel, boxsize, los=2, factor=0.01, out=None):
    """Redshift-space positions ``s = pos; s[:, los] += factor * vel[:, los]`` with one periodic wrap into [0, boxsize)
    (ast_rsd_shift); ``factor`` 0.01 is TPCF's ``vel / 100``.  (N, 3) device tensors of one dtype, float32 or float64,
    arithmetic in that dtype.  Like TPCF, a shift that one wrap does not bring back into the box (more than a box
    length, or a position outside it) is a ValueError; the test reads the extremes of the shifted column back (one host
    sync per call, like tpcf_pair_counts' bounds).  ``out`` may be ``pos``: the shift then runs into a scratch tensor
    that is copied over ``pos`` only once it has passed, so a rejected call leaves the caller's positions as they
    were; a separate ``out`` holds the unwrapped result when the call raises."""
    if los not in (0, 1, 2):
        raise ValueError(f"los must be 0, 1 or 2, got {los}")
    boxsize = float(boxsize)
    if not (np.isfinite(boxsize) and boxsize > 0):
        raise ValueError(f"boxsize must be positive and finite, got {boxsize}")
    n = pos.shape[0] if pos.dim() == 2 else -1
    if tuple(pos.shape) != (n, 3) or tuple(vel.shape) != (n, 3) or pos.dtype not in _REAL or vel.dtype != pos.dtype:
        raise ValueError(f"pos and vel must be (N, 3) of one dtype, float32 or float64: got {tuple(pos.shape)} "
                         f"{pos.dtype} and {tuple(vel.shape)} {vel.dtype}")
    assert pos.is_cuda and vel.is_cuda and pos.is_contiguous() and vel.is_contiguous()
    if out is not None:
        assert out.is_cuda and out.is_contiguous() and out.dtype == pos.dtype and out.shape == pos.shape
    in_place = out is not None and out.data_ptr() == pos.data_ptr()
    res = torch.empty_like(pos) if out is None or in_place else out
    check(_lib.lib().ast_rsd_shift(ptr(pos), ptr(vel), real_code(pos), n, int(los), float(factor), boxsize, ptr(res),
                                   stream()), "ast_rsd_shift")
    if n:
        lo, hi = (float(v) for v in torch.aminmax(res[:, los]))
        if not (lo >= 0.0 and hi < boxsize):
            raise ValueError(f"positions after the redshift-space shift and one wrap must lie in [0, {boxsize}): "
                             f"min {lo}, max {hi}")
    if in_place:
        out.copy_(res)
        return out
    return res


def catalog_power_2d(pos1, mass1, nmesh, boxsize, window="tsc", interlaced=True, compensated=True, pos2=None, mass2=None,
                     vel1=None, vel2=None, rsd_factor=0.01, Nmu=5, los=2, poles=(0, 2, 4)):
    """``FFTPower(CatalogMesh(cat1, ...), mode="2d", Nmu=, los=, poles=[, second=CatalogMesh(cat2, ...)])`` with the
    catalogues moved to redshift space first where velocities are given (:func:`rsd_shift`): the dict of
    :func:`finish_power_2d`; the shot noise is reported, not subtracted (auto: L^3 sum w^2 / (sum w)^2; cross: 0)."""
    Nmu, los, poles = check_fftpower_2d_args(Nmu, los, poles)
    n = int(nmesh)
    if vel1 is not None:
        pos1 = rsd_shift(dense(pos1), dense(vel1), boxsize, los, rsd_factor)
    c1, sn = catalog_mesh_complex(pos1, mass1, n, boxsize, window, interlaced, compensated)
    c2 = None
    if pos2 is not None:
        if vel2 is not None:
            pos2 = rsd_shift(dense(pos2), dense(vel2), boxsize, los, rsd_factor)
        c2, _ = catalog_mesh_complex(pos2, mass2, n, boxsize, window, interlaced, compensated)
        sn = 0.0
    return finish_power_2d(*power_bin_2d(c1, c2, n, boxsize, Nmu, los, poles), poles=poles, shotnoise=sn)


_power_scratch = {}


@contextlib.contextmanager
def _power_scratch_for(key, nbytes, device_):
    """``with _power_scratch_for(key, nbytes, device) as scratch``: the ONE cached scratch tensor of the fused power
    paths (another key releases it: peak memory at 1024^3), taken for a call on the current stream.  The stream and the
    event of its last use travel with the tensor, as an attribute: the dict's values stay the tensors themselves (the
    tests look them up, and tests/dirty_memory.py swaps the dict for a while).  A call on another stream waits for that
    event first - two streams take turns on the scratch - and tells the allocator about the new stream, so that a
    release (the ``clear()`` below) does not hand the block out again while that stream still works in it.  The end of
    the use is recorded on the way out, also when the call raised: whatever it had queued still runs."""
    cur = torch.cuda.current_stream()
    scratch = _power_scratch.get(key)
    if scratch is None:
        _power_scratch.clear()
        scratch = _power_scratch[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=device_)
        scratch.ast_last_use = None
    last = getattr(scratch, "ast_last_use", None)
    if last is not None and last[0] != cur:
        cur.wait_event(last[1])
        scratch.record_stream(cur)
    try:
        yield scratch
    finally:
        done = last[1] if last is not None else torch.cuda.Event()
        done.record(cur)
        scratch.ast_last_use = (cur, done)


def power_sums_fused(field, boxsize, psum=None, mean=0.0, halo=None, lowk=True, binning=None):
    """(ksum, psum, nmodes) of the auto power of an fp32 cube of side 256/512/1024 through
    the fused tile-FFT + shell-binning path (the spectrum is never written to HBM).
    ``mean`` is subtracted from the cells on load: it only touches the discarded DC mode
    and keeps fp32 round-off from scaling with the mean density (pass total_mass/Ng).
    ``lowk``: the five lowest shells come from double-precision DFT sums of the modes |m_i| <= 5 (one more read
    of the grid): the fp32 transform's round-off floor would otherwise cap them at ~2e-6 / |m|^2.
    ksum and nmodes are copies of the cached geometry: the caller's own."""
    field = dense(field, 16)                  # (the z pass reads the rows as pairs: ast_fft_tile_power_3d refuses less than 8)
    n = field.shape[0]
    L = _lib.lib()
    key = (torch.cuda.current_device(), n)
    if psum is None:
        psum = torch.zeros(n // 2 - 1, dtype=torch.float64, device=field.device)
    ksum, nmodes = shell_geometry(n, boxsize, binning=binning)
    with _power_scratch_for(key, L.ast_fft_tile_power_scratch_bytes(n), field.device) as scratch:
        if halo is not None:                  # grid from paint(..., defer_fold=True)
            check(L.ast_fft_tile_power_3d_halo(ptr(field), halo.rec_ptr, halo.window_code, ptr(scratch), scratch.numel(),
                                               real_code(field), n, float(boxsize), float(mean), int(bool(lowk)), _bin_code(binning), ptr(psum), stream()),
                  "ast_fft_tile_power_3d_halo")
        else:
            check(L.ast_fft_tile_power_3d(ptr(field), ptr(scratch), scratch.numel(), real_code(field), n, float(boxsize),
                                          float(mean), int(bool(lowk)), _bin_code(binning), ptr(psum), stream()), "ast_fft_tile_power_3d")
    return ksum, psum, nmodes


def lowk_modes(planes, nmesh, x0=0, out=None):
    """Contribution of the planes x0 .. x0 + nx - 1 (an (nx, n, n) fp32 tensor) to the low-k modes |m_i| <= 6 in
    double (complex128 tensor of ast_lowk_mode_count() entries; accumulated into ``out`` when given)."""
    L = _lib.lib()
    n, nx = int(nmesh), planes.shape[0]
    assert planes.is_cuda and planes.is_contiguous() and planes.dtype == torch.float32 and tuple(planes.shape[1:]) == (n, n)
    work_bytes = int(L.ast_lowk_work_bytes(n, nx))
    work = torch.empty(work_bytes, dtype=torch.uint8, device=planes.device)
    acc = out is not None
    if out is None:
        out = torch.empty(int(L.ast_lowk_mode_count()), dtype=torch.complex128, device=planes.device)
    check(L.ast_lowk_modes(ptr(planes), F32, n, int(x0), nx, int(acc), ptr(out), ptr(work), work_bytes, stream()),
          "ast_lowk_modes")
    return out


def lowk_shell_sums(modes, nmesh, boxsize, binning=None):
    """psum entries of the lowest shells from the (complete) low-k modes."""
    L = _lib.lib()
    sums = torch.empty(int(L.ast_lowk_shell_count()), dtype=torch.float64, device=modes.device)
    check(L.ast_lowk_shell_sums(ptr(modes), int(nmesh), float(boxsize), _bin_code(binning), ptr(sums), stream()),
          "ast_lowk_shell_sums")
    return sums


def fused_power64_supported(field, allow_f32=False):
    """float64 cubes of side 128 ... 2048; with allow_f32 also float32 cubes (transformed in double, widened on load)."""
    n = field.shape[0]
    ok = (torch.float64, torch.float32) if allow_f32 else (torch.float64,)
    return field.dim() == 3 and tuple(field.shape) == (n, n, n) and field.dtype in ok and field.is_contiguous() \
        and bool(_lib.lib().ast_fft64_supported(n))


def power_sums_fused64(field, boxsize, psum=None, binning=None, halo=None, mean=None):
    """(ksum, psum, nmodes) of the auto power of a float64 cube of side 128 ... 2048 through the hand-written
    double-precision passes (ast_fft64_power_3d): one pass per axis, the last one fused with the shell binning.  fp32 cubes
    of the sides the fp32 tile passes do not cover take the same passes, widened on load - or, at side 2048 and with the
    grid's ``mean`` given (0.0 for a grid that holds rho - mean), single-precision passes of their own
    (ast_fft32_big_power_3d).  ksum and nmodes are copies of the cached geometry: the caller's own."""
    import os
    field = dense(field, 16)                  # (the C entries refuse a grid off 16 bytes, 8 for fp32)
    n = field.shape[0]
    L = _lib.lib()
    if psum is None:
        psum = torch.zeros(n // 2 - 1, dtype=torch.float64, device=field.device)
    ksum, nmodes = shell_geometry(n, boxsize, binning=binning)
    if field.dtype == torch.float32 and mean is not None and bool(L.ast_fft32_big_supported(n)) \
            and not os.environ.get("ASTRILD_FFT32_BIG_OFF"):
        # side 2048: single-precision passes (half the bytes of the double route below); the grid's mean leaves as the rows
        # are loaded and the sixteen lowest shells come from double-precision sums over the grid (inside the call) - fp32
        # round-off of an O(1) field on shells of little power - as the fp32 tile pipeline takes its five lowest
        key32 = (torch.cuda.current_device(), n, "f32big")
        with _power_scratch_for(key32, L.ast_fft32_big_power_scratch_bytes(n), field.device) as scratch:
            if halo is not None:              # grid from paint(..., defer_fold=True): the fold rides on the z rows
                check(L.ast_fft32_big_power_3d_halo(ptr(field), halo.rec_ptr, halo.window_code, ptr(scratch), scratch.numel(), n,
                                                    float(boxsize), _bin_code(binning), float(mean), ptr(psum), stream()),
                      "ast_fft32_big_power_3d_halo")
            else:
                check(L.ast_fft32_big_power_3d(ptr(field), ptr(scratch), scratch.numel(), n, float(boxsize), _bin_code(binning), float(mean),
                                               ptr(psum), stream()), "ast_fft32_big_power_3d")
        return ksum, psum, nmodes
    key = (torch.cuda.current_device(), n, "f64")
    with _power_scratch_for(key, L.ast_fft64_power_scratch_bytes(n), field.device) as scratch:
        if field.dtype == torch.float32:      # an fp32 grid through the double passes (sizes without fp32 tile passes)
            assert halo is None
            check(L.ast_fft64_power_3d_f32(ptr(field), ptr(scratch), scratch.numel(), n, float(boxsize), _bin_code(binning), ptr(psum),
                                           stream()), "ast_fft64_power_3d_f32")
        elif halo is not None:                # grid from paint(..., defer_fold=True)
            check(L.ast_fft64_power_3d_halo(ptr(field), halo.rec_ptr, halo.window_code, ptr(scratch), scratch.numel(), n,
                                            float(boxsize), _bin_code(binning), ptr(psum), stream()), "ast_fft64_power_3d_halo")
        else:
            check(L.ast_fft64_power_3d(ptr(field), ptr(scratch), scratch.numel(), n, float(boxsize), _bin_code(binning), ptr(psum), stream()),
                  "ast_fft64_power_3d")
    return ksum, psum, nmodes


def fused_power_supported(field):
    n = field.shape[0]
    return field.dim() == 3 and tuple(field.shape) == (n, n, n) and field.dtype == torch.float32 \
        and bool(_lib.lib().ast_fft_tile_supported(F32, n))


def paint_power_1d(pos, mass, nmesh, boxsize, window="cic", scale=1.0, binning=None, defer_fold64=True, pos_scale=1.0):
    """``pm.paint(...)`` followed by ``FFTPower(ArrayMesh(grid), mode="1d")`` (stats_subfind.py:130-150)
    as one pipeline: where the fused fp32 path applies, the paint's halo fold rides on the FFT's z pass.
    pos_scale: the positions are in units of 1 / pos_scale box units (``pos * pos_scale`` is what the reference paints,
    stats_subfind.py:121-122: kpc -> Mpc/h): folded into the cell lookup - the catalogue is painted as it was read."""
    n = int(nmesh)
    pos, mass = dense(pos), dense(mass)
    paint_box = float(boxsize) / float(pos_scale)
    # which tiled variant (None: a catalogue too sparse for the tiles - global atomics, then the plain transform)
    tiled = auto_paint_method(pos.shape[0], n, n, window) if n % 32 == 0 else "direct"
    tiled = None if tiled == "direct" else tiled
    fast = pos.dtype == torch.float32 and tiled is not None and bool(_lib.lib().ast_fft_tile_supported(F32, n))
    if fast:
        # the grid holds rho - mean (subtracted before the fp32 rounding): only the discarded DC mode differs
        grid, halo = paint(pos, mass, n, paint_box, window, scale=scale, method=tiled, defer_fold=True,
                           offset="mean")
        return finish_power(*power_sums_fused(grid, boxsize, halo=halo, binning=binning))
    if pos.dtype == torch.float32 and tiled is not None and bool(_lib.lib().ast_fft64_supported(n)):
        # fp32 particles on a grid without fp32 tile passes (128^3, 2048^3): the grid holds rho - mean (only the discarded DC
        # mode differs), the transform runs in double straight from the fp32 grid
        # (side 2048 takes its fp32 passes.  Their z rows could fold the halo records on load - power_sums_fused64(halo=) -
        # but TWO kernels read every row there, the transform and the low-k sums, and both would fetch the 9 GB of records:
        # 86.6 ms against 83.5 with the paint's own fold kernel, so the grid is folded here)
        grid = paint(pos, mass, n, paint_box, window, scale=scale, method=tiled, offset="mean")
        return finish_power(*power_sums_fused64(grid, boxsize, binning=binning, mean=0.0))
    fast64 = pos.dtype == torch.float64 and tiled is not None and bool(_lib.lib().ast_fft64_supported(n))
    if fast64 and defer_fold64:               # float64: the halo fold inside the double z pass (26.2 vs 26.5 ms at 1024^3)
        grid, halo = paint(pos, mass, n, paint_box, window, scale=scale, method=tiled, defer_fold=True)
        return finish_power(*power_sums_fused64(grid, boxsize, halo=halo, binning=binning))
    return fftpower_1d(paint(pos, mass, n, paint_box, window, scale=scale), boxsize, binning=binning)


def fftpower_1d(field1, boxsize, field2=None, fused=True, binning=None):
    """``FFTPower(first, mode="1d", kmin=2*pi/L[, second])`` for in-memory grids
    (nbodykit call sites: power_spectrum_3d.py:189-224, stats_subfind.py:142-150)."""
    field1, field2 = dense(field1), dense(field2)
    n = field1.shape[0]
    assert tuple(field1.shape) == (n, n, n) and n % 2 == 0
    if fused and field2 is None and fused_power_supported(field1):
        # the grid's mean is removed as the z pass loads the cells (it only feeds the discarded DC mode): an fp32
        # transform of an O(1) mean would leave its round-off on every shell
        mean = total_mass(field1.reshape(-1), 0) / float(field1.numel())
        return finish_power(*power_sums_fused(field1, boxsize, mean=mean, binning=binning))
    if fused and field2 is None and fused_power64_supported(field1, allow_f32=True):
        # float64 cubes of side 128 ... 2048 - and fp32 cubes of the sides the fp32 tile passes do not cover (128, 2048),
        # transformed in double without a float64 copy of the grid
        mean = total_mass(field1.reshape(-1), 0) / float(field1.numel()) if field1.dtype == torch.float32 else None
        return finish_power(*power_sums_fused64(field1, boxsize, binning=binning, mean=mean))
    if field1.dtype == torch.float32:
        # fp32 grids that do not take the fused path above - cross spectra, sizes the tile FFT does not cover: an fp32
        # transform would carry the O(1) mean's round-off into the low shells (2e-6 and worse: only the fused path
        # removes the mean and patches the lowest shells); the transforms run in double instead
        field1 = field1.double()
        field2 = None if field2 is None else field2.double()
    s1 = r2c(field1)
    s2 = None if field2 is None else r2c(field2)
    return finish_power(*power_bin_1d(s1, s2, n, boxsize, binning=binning))


# ------------------------------------------ catalogue meshes: interlacing + compensation
def interlace_compensate(c1, c2, nmesh, window, compensated=True, i0=None, i1=None):
    """In place on c1 (half spectrum of the plain paint): combine with c2 (spectrum of the paint shifted by half
    a cell, or None) and divide by the mass-assignment window - nbodykit CatalogMesh, interlaced / compensated."""
    n = int(nmesh)
    i0 = (0, n) if i0 is None else tuple(i0)
    i1 = (0, n) if i1 is None else tuple(i1)
    assert c1.is_cuda and c1.is_contiguous() and c1.numel() == i0[1] * i1[1] * (n // 2 + 1)
    assert c2 is None or (c2.dtype == c1.dtype and c2.numel() == c1.numel() and c2.is_contiguous())
    if c2 is None and not compensated:
        return c1
    check(_lib.lib().ast_interlace_compensate(ptr(c1), ptr(c2), _CPLX[c1.dtype], n, _lib.WIN[window.lower()],
                                              int(bool(compensated)), int(i0[0]), int(i0[1]), int(i1[0]), int(i1[1]),
                                              stream()), "ast_interlace_compensate")
    return c1


def catalog_mesh_complex(pos, mass, nmesh, boxsize, window="tsc", interlaced=True, compensated=True):
    """delta_k of a particle catalogue like nbodykit ``CatalogMesh(..., Nmesh, BoxSize, window=, interlaced=,
    compensated=).compute(mode="complex")``: the painted field is normalised to 1 + delta (mean weight per cell 1),
    transformed with pmesh's 1/Ng convention, interlaced with a second paint shifted by half a cell and divided
    by the window.  Returns (half spectrum, shotnoise = L^3 sum w^2 / (sum w)^2)."""
    n = int(nmesh)
    pos, mass = dense(pos), dense(mass)
    wsum = total_mass(mass, pos.shape[0])
    scale = float(n) ** 3 / wsum
    c1 = r2c(paint(pos, mass, n, boxsize, window, scale=scale))
    c2 = r2c(paint(pos, mass, n, boxsize, window, scale=scale, shift=0.5)) if interlaced else None
    interlace_compensate(c1, c2, n, window, compensated)
    if mass is None:
        w2 = float(pos.shape[0])
    else:
        w2 = float(triple_product_sum(mass, mass, torch.ones_like(mass)).item())
    return c1, float(boxsize) ** 3 * w2 / wsum ** 2


def catalog_power_1d(pos1, mass1, nmesh, boxsize, window="tsc", interlaced=True, compensated=True, pos2=None, mass2=None):
    """``FFTPower(CatalogMesh(cat1, ...), mode="1d", kmin=2 pi / L[, second=CatalogMesh(cat2, ...)])``: dict(k, power,
    modes, shotnoise); the shot noise is reported, not subtracted (auto: L^3 sum w^2 / (sum w)^2; cross: 0)."""
    n = int(nmesh)
    c1, sn = catalog_mesh_complex(pos1, mass1, n, boxsize, window, interlaced, compensated)
    c2 = None
    if pos2 is not None:
        c2, _ = catalog_mesh_complex(pos2, mass2, n, boxsize, window, interlaced, compensated)
        sn = 0.0
    res = finish_power(*power_bin_1d(c1, c2, n, boxsize))
    res["shotnoise"] = sn
    return res


# ----------------------------------------------------------------- bispectrum
def c2r(spec, shape, out=None):
    """Unnormalised inverse of :func:`r2c`'s layout: sum_k spec_k e^{ikx} (rocFFT C2R;
    the input spectrum is used as scratch)."""
    n0, n1, n2 = shape
    code = _CPLX[spec.dtype]
    assert spec.is_cuda and spec.is_contiguous()
    if out is None:
        out = torch.empty(shape, dtype=_TO_REAL[spec.dtype], device=spec.device)
    assert out.is_contiguous()
    fft_plan(_lib.FFT_C2R, code, (n0, n1, n2), 1, 1.0, False).execute(spec, out)
    return out


def c2r_tile(spec, work=None, out=None, m_lo=0, m_hi=0, scale=1.0):
    """Unnormalised inverse of :func:`r2c`'s layout through the hand-written tile passes (complex64 cubes of side
    256/512/1024), optionally restricted to the shell m_lo <= |m| < m_hi (the bispectrum estimator's masked inverse
    transform in one call).  ``spec`` is left intact; ``work`` (same shape) is scratch."""
    n = spec.shape[0]
    assert spec.is_cuda and spec.is_contiguous() and spec.dtype == torch.complex64 and tuple(spec.shape) == (n, n, n // 2 + 1)
    work = torch.empty_like(spec) if work is None else work
    out = torch.empty((n, n, n), dtype=torch.float32, device=spec.device) if out is None else out
    check(_lib.lib().ast_fft_tile_c2r_3d(ptr(spec), ptr(work), ptr(out), F32, n, int(m_lo), int(m_hi), float(scale), stream()),
          "ast_fft_tile_c2r_3d")
    return out


def tile_work_pitch(n):
    """Row pitch (complex elements) of the scratch spectra of :func:`c2r_tile_batch`: n/2+1 rounded up to 16 elements, so
    that the 128-byte row pieces of the x / y passes' 16-column tiles are whole lines (at n/2+1 every piece straddles two
    lines, both shared with the neighbouring tiles: 19 % more bytes written and re-read, profiles/r04_bispec_pruning.txt)."""
    return (int(n) // 2 + 1 + 15) // 16 * 16


def c2r_tile_batch(spec, shells, works, outs=None, scale=1.0, xy_batch=None):
    """:func:`c2r_tile` for up to 8 shells ``[(m_lo, m_hi), ...]`` of one spectrum (the shell is the launches' second grid
    dimension).  ``works``: one scratch spectrum per shell, shaped like ``spec`` or (n, n, pitch) with any pitch >= n/2+1
    (:func:`tile_work_pitch`).  xy_batch: shells per launch of the x and y passes (default 1:
    shell by shell, so that a shell's y pass reads its x pass's output out of the Infinity Cache; measured at 512^3:
    eight per launch 8.4 ms for the 31 shells' x / y passes against 6.7); the z passes always go in one launch.
    Returns the real fields."""
    n = spec.shape[0]
    k = len(shells)
    assert 1 <= k <= 8 and len(works) >= k
    pitch = int(works[0].shape[-1])
    for w in works[:k]:
        assert w.is_cuda and w.is_contiguous() and w.dtype == torch.complex64 and tuple(w.shape) == (n, n, pitch) and pitch >= n // 2 + 1
    assert spec.is_cuda and spec.is_contiguous() and spec.dtype == torch.complex64 and tuple(spec.shape) == (n, n, n // 2 + 1)
    if outs is None:
        outs = [torch.empty((n, n, n), dtype=torch.float32, device=spec.device) for _ in range(k)]
    wp = (ct.c_void_p * k)(*[w.data_ptr() for w in works[:k]])
    op = (ct.c_void_p * k)(*[o.data_ptr() for o in outs[:k]])
    lo = (ct.c_int * k)(*[int(s[0]) for s in shells])
    hi = (ct.c_int * k)(*[int(s[1]) for s in shells])
    L = _lib.lib()
    if xy_batch is None:
        import os
        xy_batch = int(os.environ.get("ASTRILD_BISPEC_XY_BATCH", "1"))
    xy_batch = max(1, min(int(xy_batch), k))
    if xy_batch >= k:
        check(L.ast_fft_tile_c2r_3d_batch(ptr(spec), wp, op, F32, n, lo, hi, k, float(scale), 3, pitch, stream()), "ast_fft_tile_c2r_3d_batch")
        return list(outs[:k])
    for b0 in range(0, k, xy_batch):
        kb = min(xy_batch, k - b0)
        sub = lambda arr, typ: (typ * kb)(*arr[b0:b0 + kb])
        check(L.ast_fft_tile_c2r_3d_batch(ptr(spec), sub(wp, ct.c_void_p), sub(op, ct.c_void_p), F32, n, sub(lo, ct.c_int),
                                          sub(hi, ct.c_int), kb, float(scale), 1, pitch, stream()), "ast_fft_tile_c2r_3d_batch")
    check(L.ast_fft_tile_c2r_3d_batch(ptr(spec), wp, op, F32, n, lo, hi, k, float(scale), 2, pitch, stream()), "ast_fft_tile_c2r_3d_batch")
    return list(outs[:k])


def shell_filter(spec, nmesh, m_lo, m_hi, out=None, i0=None, i1=None, dtype=None):
    """out = spec * 1[m_lo <= |m| < m_hi]; spec=None writes the bare indicator."""
    n = int(nmesh)
    i0 = (0, n) if i0 is None else tuple(i0)
    i1 = (0, n) if i1 is None else tuple(i1)
    if out is None:
        cd = spec.dtype if spec is not None else dtype
        out = torch.empty((i0[1], i1[1], n // 2 + 1), dtype=cd, device=device())
    assert (spec is None or spec.is_contiguous()) and out.is_contiguous()
    check(_lib.lib().ast_shell_filter(ptr(spec), ptr(out), _CPLX[out.dtype], n, int(m_lo), int(m_hi),
                                      int(i0[0]), int(i0[1]), int(i1[0]), int(i1[1]), stream()),
          "ast_shell_filter")
    return out


def triple_product_sum(a, b, c):
    a, b, c = dense(a), dense(b), dense(c)
    out = torch.zeros(1, dtype=torch.float64, device=a.device)
    check(_lib.lib().ast_triple_product_sum(ptr(a), ptr(b), ptr(c), real_code(a), a.numel(), ptr(out), stream()),
          "ast_triple_product_sum")
    return out


def triple_product_sums(fields, triangles):
    """sum over cells of f_i f_j f_l for every (i, j, l) in ``triangles`` (keys of the dict ``fields``), every field read
    once per batch of <= 256 triangles (ast_triple_product_sums).  Returns a float64 tensor, one entry per triangle."""
    L = _lib.lib()
    triangles = [tuple(t) for t in triangles]
    out = torch.zeros(len(triangles), dtype=torch.float64, device=device())
    scratch = torch.empty(L.ast_triple_product_sums_scratch_bytes() // 8, dtype=torch.float64, device=device())
    for b0 in range(0, len(triangles), 256):
        batch = triangles[b0:b0 + 256]
        used = sorted({s for t in batch for s in t})
        first = fields[used[0]]
        if len(used) * 257 * first.element_size() > 160 * 1024:          # more shells than one LDS chunk holds
            for n, (i, j, l) in enumerate(batch):
                out[b0 + n:b0 + n + 1] = triple_product_sum(fields[i], fields[j], fields[l])
            continue
        for s in used:
            f = fields[s]
            assert f.is_contiguous() and f.dtype == first.dtype and f.numel() == first.numel()
        slot = {s: n for n, s in enumerate(used)}
        ptrs = torch.tensor([fields[s].data_ptr() for s in used], dtype=torch.int64).to(device())
        tri = torch.tensor([[slot[s] for s in t] for t in batch], dtype=torch.int32).to(device())
        check(L.ast_triple_product_sums(ptr(ptrs), len(used), real_code(first), first.numel(), ptr(tri), len(batch),
                                        ptr(scratch), ptr(out[b0:]), stream()), "ast_triple_product_sums")
    return out


_tri_cache = {}


def bispectrum(field, boxsize, edges, triangles):
    """FFT (Scoccimarro) bispectrum estimator on integer-|m| shells [edges[i], edges[i+1]).

    Returns dict(B, ntri, k) with one entry per (i, j, l) in ``triangles``; ntri is
    the exact integer count of closed triangles.  The reference's Bispectrum3D has
    no bispectrum arithmetic (bispectrum_3d.py:165-215 computes P(k)); this is the
    estimator its docstring cites (:42-44).
    """
    n = field.shape[0]
    assert tuple(field.shape) == (n, n, n) and n % 2 == 0
    edges = [int(e) for e in edges]
    triangles = [tuple(int(v) for v in t) for t in triangles]
    used = sorted({s for t in triangles for s in t})
    spec = r2c(field)
    tile = spec.dtype == torch.complex64 and bool(_lib.lib().ast_fft_tile_supported(F32, n))
    # (the tile passes' scratch spectrum has line-aligned rows)
    scratch = torch.empty((n, n, tile_work_pitch(n)), dtype=spec.dtype, device=spec.device) if tile else torch.empty_like(spec)
    key = (torch.cuda.current_device(), n, tuple(edges), tuple(triangles))
    ntri = _tri_cache.get(key)
    if ntri is None:
        # Triangle counts depend on the geometry only; they are computed ONCE per (N, edges, triangles), always in
        # float64: I_s(0) equals the shell's mode count (1e6 at 512^3), and the fp32 round-off of that one cell
        # alone would move sum I_i I_j I_l / Ng by thousands.  In double the sum is within ~1e-3 of the integer.
        iscratch = torch.empty(spec.shape, dtype=torch.complex128, device=spec.device)
        ifields = {}
        L = _lib.lib()
        forward_only = bool(L.ast_fft64_supported(n))
        for s in used:
            if forward_only:
                # the indicator is real and even: its inverse transform is its forward one (hand-written double
                # passes, no rocFFT), real up to round-off, unfolded from the half lattice onto the full one
                mask = torch.empty((n, n, n), dtype=torch.float64, device=spec.device)
                check(L.ast_shell_mask_real(ptr(mask), n, edges[s], edges[s + 1], stream()), "ast_shell_mask_real")
                check(L.ast_fft64_r2c_3d(ptr(mask), ptr(iscratch), n, 1.0, stream()), "ast_fft64_r2c_3d")
                check(L.ast_half_real_to_full(ptr(iscratch), ptr(mask), n, stream()), "ast_half_real_to_full")
                ifields[s] = mask
                continue
            shell_filter(None, n, edges[s], edges[s + 1], out=iscratch)
            ifields[s] = c2r(iscratch, (n, n, n))
        dens = triple_product_sums(ifields, triangles).cpu().numpy()
        del ifields, iscratch
        exact = dens / float(n) ** 3
        ntri = np.rint(exact).astype(np.int64)
        worst = float(np.abs(exact - ntri).max()) if len(exact) else 0.0
        if worst > 0.05:
            raise _lib.AstrildHipError(f"triangle counts are not integers to 0.05 (worst {worst:.3g})")
        _tri_cache[key] = ntri
        _tri_cache[key + ("residual",)] = worst
    # The triangle sums form f_i f_j f_l of fp32 fields in fp32 (only the running sums are double): a field in physical units
    # (a mass-weighted grid in Msun/h per cell) would overflow the product above |D| ~ 7e12.  The shell fields are therefore
    # built from the spectrum divided by A = max |field| - values of order one - and the sums multiplied back by A^3.
    amp = _max_abs(field, field.numel()) if field.dtype == torch.float32 else 1.0
    if not np.isfinite(amp):
        raise _lib.AstrildHipError("bispectrum: the field holds inf / NaN")
    # FUSED tail (default where it applies: fp32 tile sizes, <= 32 shells): every shell's masked x and y passes into its OWN
    # scratch spectrum, then ONE kernel that runs the z passes of all shells row by row and forms the triangle sums from
    # LDS (ast_fft_tile_c2r_triangles) - the 31 real cubes (0.5 GB each at 512^3, written once and read back once) never
    # exist.  ASTRILD_BISPEC_FUSED=0: the cubes and ast_triple_product_sums, as before.
    import os
    if tile and len(used) <= 32 and os.environ.get("ASTRILD_BISPEC_FUSED", "1") != "0":
        L = _lib.lib()
        pitch = tile_work_pitch(n)
        works = [scratch] + [torch.empty_like(scratch) for _ in range(len(used) - 1)]
        wp = (ct.c_void_p * len(used))(*[w.data_ptr() for w in works])
        hi = (ct.c_int * len(used))(*[edges[s + 1] for s in used])
        for i, s_ in enumerate(used):           # shell by shell: a shell's y pass finds its x pass's output in the Infinity Cache
            one_w = (ct.c_void_p * 1)(works[i].data_ptr())
            one_o = (ct.c_void_p * 1)(None)                          # (no output: passes = 1 stops before the z pass)
            check(L.ast_fft_tile_c2r_3d_batch(ptr(spec), one_w, one_o, F32, n, (ct.c_int * 1)(edges[s_]), (ct.c_int * 1)(edges[s_ + 1]),
                                              1, 1.0, 1, pitch, stream()), "ast_fft_tile_c2r_3d_batch")
        slot = {s_: i for i, s_ in enumerate(used)}
        tri_d = torch.tensor([[slot[v] for v in t] for t in triangles], dtype=torch.int32).to(spec.device)
        out = torch.empty(len(triangles), dtype=torch.float64, device=spec.device)
        fscr = torch.empty(int(L.ast_fft_tile_c2r_triangles_scratch_bytes()) // 8, dtype=torch.float64, device=spec.device)
        for b0 in range(0, len(triangles), 512):
            nb_ = min(512, len(triangles) - b0)
            check(L.ast_fft_tile_c2r_triangles(wp, hi, len(used), F32, n, pitch, 1.0 / amp, ptr(tri_d[b0:]), nb_, ptr(fscr), ptr(out[b0:]),
                                               stream()), "ast_fft_tile_c2r_triangles")
        num = out.cpu().numpy() * amp ** 3
        del works
        kf = 2.0 * np.pi / boxsize
        kmid = np.array([[kf * 0.5 * (edges[s] + edges[s + 1]) for s in t] for t in triangles])
        with np.errstate(invalid="ignore", divide="ignore"):
            b = float(boxsize) ** 6 * num / (ntri * float(n) ** 3)
        return {"B": b, "ntri": ntri, "k": kmid, "ntri_residual": _tri_cache[key + ("residual",)]}
    dfields = {}
    if tile:
        # the masked, pruned inverse tile passes (shell mask fused into the first pass's loads), shell by shell through ONE
        # scratch spectrum.  ASTRILD_BISPEC_BATCH=k runs k shells per launch (ast_fft_tile_c2r_3d_batch) - measured at
        # 512^3 / 31 shells: the z passes gain (5.9 -> 5.1 ms, the small shells fill the large ones' tails) but the x / y
        # passes lose more (6.9 -> 8.0 ms: k scratch spectra instead of one that stays in the Infinity Cache)
        import os
        batch = max(1, min(8, int(os.environ.get("ASTRILD_BISPEC_BATCH", "1")))) if len(used) > 1 else 1
        works = [scratch] + [torch.empty_like(scratch) for _ in range(min(batch, len(used)) - 1)]
        for b0 in range(0, len(used), batch):
            group = used[b0:b0 + batch]
            fields = c2r_tile_batch(spec, [(edges[s], edges[s + 1]) for s in group], works, scale=1.0 / amp)
            dfields.update(zip(group, fields))
        del works
    if not tile and amp != 1.0:
        sr = torch.view_as_real(spec)
        check(_lib.lib().ast_divide(ptr(sr), real_code(sr), sr.numel(), amp, stream()), "ast_divide")
    for s in ([] if tile else used):
        shell_filter(spec, n, edges[s], edges[s + 1], out=scratch)
        dfields[s] = c2r(scratch, (n, n, n))
    num = triple_product_sums(dfields, triangles).cpu().numpy() * amp ** 3
    kf = 2.0 * np.pi / boxsize
    kmid = np.array([[kf * 0.5 * (edges[s] + edges[s + 1]) for s in t] for t in triangles])
    with np.errstate(invalid="ignore", divide="ignore"):
        b = float(boxsize) ** 6 * num / (ntri * float(n) ** 3)
    return {"B": b, "ntri": ntri, "k": kmid, "ntri_residual": _tri_cache[key + ("residual",)]}


# ------------------------------------------------------------------ pair finders: the host checks they share
def _real_device(a):
    """``as_device``, with any dtype but float32 / float64 widened to float64."""
    t = as_device(a)
    return t if t.dtype in _REAL else t.to(torch.float64)


def _pair_sample(pos, vel, pos_msg, vel_msg, widths=(3,)):
    """One sample of a pair finder as real device tensors: ``(p, v, n)``, positions (N, 3) and, unless ``vel`` is None,
    velocities (N, w) with w in ``widths``.  ValueError with ``pos_msg`` / ``vel_msg``, in which ``{p}`` and ``{v}``
    stand for the two shapes."""
    p = _real_device(pos)
    v = None if vel is None else _real_device(vel)
    n = p.shape[0] if p.dim() == 2 else -1
    bad_pos = p.shape != (n, 3)
    if bad_pos or (v is not None and (v.dim() != 2 or v.shape[0] != n or v.shape[1] not in widths)):
        raise ValueError((pos_msg if bad_pos else vel_msg).format(p=tuple(p.shape), v=v is not None and tuple(v.shape)))
    return p, v, n


def _check_edges(edges, noun, top=None, max_bins=None):
    """Bin edges as an fp64 array, or ValueError: at least two finite, non-negative, strictly increasing values, at most
    ``max_bins`` bins, the largest below ``top`` (boxsize / 3 of a periodic box).  ``noun``: "s edge" or "bin edge"."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    if len(e) < 2 or not np.all(np.isfinite(e)) or np.any(np.diff(e) <= 0) or e[0] < 0:
        raise ValueError(f"{noun}s must be at least two finite, non-negative, strictly increasing values")
    if max_bins is not None and len(e) - 1 > max_bins:
        raise ValueError(f"{len(e) - 1} bins: at most {max_bins}")
    if top is not None and not e[-1] < top:
        raise ValueError(f"the largest {noun} ({e[-1]}) must be below boxsize / 3 ({top})")
    return e


def _positive_real(name, v, echo_float=False):
    """``float(v)`` of a positive, finite real number (not None, str or bytes), or ValueError naming ``name`` and the
    value as given, or (``echo_float``) as the float it was read as."""
    try:
        x = float("nan") if v is None or isinstance(v, (str, bytes)) else float(v)
    except (TypeError, ValueError):
        x = float("nan")
    if not (np.isfinite(x) and x > 0):
        raise ValueError(f"{name} must be a positive, finite real number, got {x if echo_float else v!r}")
    return x


def _check_device_bounds(bounds, ns, box, periodic=True, shifted=False):
    """ValueError unless every non-empty sample lies in the box.  ``bounds``: per sample min x, y, z and max x, y, z as
    a prepare call returned them (a NaN coordinate counts as -inf and +inf); ``ns``: the sample sizes.  Periodic: all of
    [0, box]; open boundaries: all finite.  The message numbers the samples when there are two, and says when the
    bounds are those ``shifted`` into redshift space."""
    b = np.asarray(bounds).reshape(len(ns), 6)
    for k, n in enumerate(ns):
        inside = (np.all(b[k, :3] >= 0.0) and np.all(b[k, 3:] <= box)) if periodic else np.all(np.isfinite(b[k]))
        if n and not inside:
            who = "positions" + (f" of sample {k + 1}" if len(ns) > 1 else "") + \
                (" (after the redshift-space shift)" if shifted else "")
            rule = f"must lie in [0, {box}]" if periodic else "must be finite"
            raise ValueError(f"{who} {rule}: min {b[k, :3].tolist()}, max {b[k, 3:].tolist()}")


# ------------------------------------------------------------------ mean pairwise velocity
def pairwise_tv(pos, vel_cart_or_ang, binnr, binwidth, theta1=None, theta2=None):
    """Pair sums of the transverse-velocity pairwise estimator (mean_pairwise_velocity.py, Yasini et al. 2018) on the
    GPU: ``(nom, denom, counts)``, device tensors of ``binnr`` float64 / float64 / int64.  A pair lands in bin
    ``int(|r_i - r_j| / binwidth)`` when that is below ``binnr``.  ``pos`` (N, 3); ``vel_cart_or_ang`` (N, 2): RA / DEC
    transverse velocities, turned cartesian with the angles (``theta1`` / ``theta2``: radians, or degrees when
    ``max(theta1) > 2 pi``; None: arctan(x / z), arctan(y / z) + 10 deg, as the reference), or (N, 3): cartesian
    already.  numpy arrays or device tensors, float32 or float64 (widened to float64 on load).
    ASTRILD_PV_CELLS=0 forces one cell (all pairs) instead of the cell grid."""
    lib = _lib.lib()
    binnr = int(binnr)
    if not 1 <= binnr <= lib.ast_pairwise_max_bins():
        raise ValueError(f"binnr={binnr}: 1..{lib.ast_pairwise_max_bins()} bins")
    shapes = "pos must be (N, 3) and velocities (N, 2) or (N, 3), got {p} and {v}"
    p, v, n = _pair_sample(pos, vel_cart_or_ang, shapes, shapes, widths=(2, 3))
    th1 = th2 = None
    mode = 0
    if theta1 is not None and v.shape[1] == 2:
        th1, th2 = as_device(theta1, torch.float64).reshape(-1), as_device(theta2, torch.float64).reshape(-1)
        if th1.numel() != n or th2.numel() != n:
            raise ValueError("theta1 / theta2 need one angle per object")
        tmax = (theta1.max().item() if isinstance(theta1, torch.Tensor) else np.max(theta1)) if n else 0.0
        mode = 2 if tmax > 2 * np.pi else 1
    single = os.environ.get("ASTRILD_PV_CELLS", "1") == "0"
    ws_bytes = lib.ast_pairwise_workspace_bytes(n, binnr)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device=p.device)
    nom = torch.empty(binnr, dtype=torch.float64, device=p.device)
    denom = torch.empty(binnr, dtype=torch.float64, device=p.device)
    counts = torch.empty(binnr, dtype=torch.int64, device=p.device)
    s = stream()
    check(lib.ast_pairwise_tv_prepare(ptr(p), real_code(p), ptr(v), real_code(v), v.shape[1], ptr(th1), ptr(th2), mode,
                                      n, ptr(work), ws_bytes, s), "ast_pairwise_tv_prepare")
    check(lib.ast_pairwise_tv(ptr(work), ws_bytes, n, binnr, float(binwidth), int(single), ptr(nom), ptr(denom),
                              ptr(counts), s), "ast_pairwise_tv")
    return nom, denom, counts


# ------------------------------------------------------------------ pairwise-velocity histograms
def check_pairwise_pdf_args(pos_shape, vel_shape, r, dist_bin, vel_bin, kind, dist_width, vel_width, ffirst, ssecond,
                            moments):
    """The argument checks of ``pairwise_velocity_pdf`` on the host, without a library call:
    ``(n, dist_bin, vel_bin, ffirst, ssecond)`` as ints, or ValueError.  The bin numbers and the row range must be
    integers (anything with ``__index__``); a fractional value is refused, not truncated."""
    import operator
    if kind not in _lib.PVPDF_KIND:
        raise ValueError(f"kind must be one of {sorted(_lib.PVPDF_KIND)}, got {kind!r}")
    pos_shape, vel_shape = tuple(pos_shape), tuple(vel_shape)
    if len(pos_shape) != 2 or pos_shape[1] != 3 or vel_shape != pos_shape:
        raise ValueError(f"pos and vel must both be (N, 3), got {pos_shape} and {vel_shape}")
    n = pos_shape[0]
    if n >= 1 << 31:
        raise ValueError(f"N={n}: fewer than 2^31 objects")
    for name, v in (("r", r), ("dist_width", dist_width), ("vel_width", vel_width)):
        _positive_real(name, v, echo_float=True)
    if not np.float32(r) > 0:
        raise ValueError(f"r={r} is not positive as a float32, the reference's type of r")
    ints = dict(dist_bin=dist_bin, vel_bin=vel_bin, ffirst=ffirst, ssecond=n if ssecond is None else ssecond)
    for name, v in ints.items():
        try:
            ints[name] = operator.index(v)
        except TypeError:
            raise ValueError(f"{name} must be an integer, got {v!r}") from None
    dist_bin, vel_bin, ffirst, ssecond = ints.values()
    if dist_bin < 1 or vel_bin < 1:
        raise ValueError(f"dist_bin={dist_bin}, vel_bin={vel_bin}: at least one bin each")
    if dist_bin * vel_bin > _lib.PVPDF_MAX_BINS:
        raise ValueError(f"{dist_bin} x {vel_bin} bins: at most {_lib.PVPDF_MAX_BINS} counters")
    if moments and dist_bin > _lib.PVPDF_MAX_MOMENT_ROWS:
        raise ValueError(f"dist_bin={dist_bin}: the moments take at most {_lib.PVPDF_MAX_MOMENT_ROWS} distance bins")
    if not 0 <= ffirst <= ssecond <= n:
        raise ValueError(f"row range [{ffirst}, {ssecond}) must satisfy 0 <= ffirst <= ssecond <= N = {n}")
    return n, dist_bin, vel_bin, ffirst, ssecond


def pairwise_velocity_pdf(pos, vel, r, dist_bin, vel_bin, kind, dist_width=1.0, vel_width=1.0, ffirst=0, ssecond=None,
                          moments=False):
    """The (separation bin, velocity bin) pair counts of the reference's mean_pv_z_sign / mean_pv_radial
    (particles/utils_cython/pairwise_velocity.pyx) on the GPU: ``(hist, outside)``, device tensors, int64 of
    (dist_bin, vel_bin) and an int64 scalar; with ``moments`` also ``(count, s1, s2)``, (dist_bin,) int64 / float64 /
    float64.  ``kind``: "z_sign" (v12 = (vz_j - vz_i) sign(z_j - z_i)) or "radial" (v12 = dv . dr / |dr|).  The
    pair i < j is seen when |dr| <= float32(r) and ffirst <= i < ssecond; it counts in
    ``hist[int(ds), int(vs)]``, ds = float32(|dr| / dist_width), vs = float32(v12 / vel_width + vel_bin // 2), when
    int(ds) < dist_bin and 0 <= vs < vel_bin, else in ``outside``.  The moments are over the seen pairs of a row with
    finite v12, whatever vs is.  ``pos`` / ``vel``: (N, 3), numpy arrays or device tensors, float32 or float64 (widened
    to float64 on load).  ValueError, before any library call, for bad arguments.
    ASTRILD_PVPDF_CELLS=0 forces one cell (all pairs) instead of the cell grid; ASTRILD_PVPDF_LDS=0 forces the
    histogram into global memory, whatever its size."""
    n, dist_bin, vel_bin, ffirst, ssecond = check_pairwise_pdf_args(
        np.shape(pos), np.shape(vel), r, dist_bin, vel_bin, kind, dist_width, vel_width, ffirst, ssecond, moments)
    lib = _lib.lib()
    p, v = _real_device(pos), _real_device(vel)
    single = os.environ.get("ASTRILD_PVPDF_CELLS", "1") == "0"
    force_global = os.environ.get("ASTRILD_PVPDF_LDS", "1") == "0"
    ws_bytes = lib.ast_pairwise_pdf_workspace_bytes(n, dist_bin, vel_bin, int(bool(moments)))
    work = torch.empty(ws_bytes, dtype=torch.uint8, device=p.device)
    hist = torch.empty((dist_bin, vel_bin), dtype=torch.int64, device=p.device)
    outside = torch.empty((), dtype=torch.int64, device=p.device)
    count = s1 = s2 = None
    if moments:
        count = torch.empty(dist_bin, dtype=torch.int64, device=p.device)
        s1 = torch.empty(dist_bin, dtype=torch.float64, device=p.device)
        s2 = torch.empty(dist_bin, dtype=torch.float64, device=p.device)
    st = stream()
    check(lib.ast_pairwise_pdf_prepare(ptr(p), real_code(p), ptr(v), real_code(v), n, ptr(work), ws_bytes, st),
          "ast_pairwise_pdf_prepare")
    check(lib.ast_pairwise_pdf(ptr(work), ws_bytes, n, _lib.PVPDF_KIND[kind], float(r), dist_bin, vel_bin,
                               float(dist_width), float(vel_width), ffirst, ssecond, int(single), int(force_global),
                               ptr(hist), ptr(outside), ptr(s1), ptr(s2), ptr(count), st), "ast_pairwise_pdf")
    if moments:
        return hist, outside, (count, s1, s2)
    return hist, outside


# ------------------------------------------------------------------ two-point correlation function
def check_tpcf_edges(s_edges, mu_edges, boxsize, periodic=True):
    """halotools' argument checks of a periodic (s, mu) pair count, on the host: fp64 edges ``(s, mu)`` (``mu`` None
    stays None) or ValueError.  s edges strictly increasing, >= 0, max < boxsize / 3; mu edges strictly increasing
    within [0, 1]; at most ``ast_tpcf_max_bins()`` bins.  ``periodic=False`` (open boundaries): ``boxsize`` is not
    looked at and the top s edge is free."""
    if periodic:
        boxsize = float(boxsize)
        if not (np.isfinite(boxsize) and boxsize > 0):
            raise ValueError(f"boxsize must be positive and finite, got {boxsize}")
    s = _check_edges(s_edges, "s edge", top=boxsize / 3.0 if periodic else None)
    mu = None
    if mu_edges is not None:
        mu = np.asarray(mu_edges, dtype=np.float64).reshape(-1)
        if len(mu) < 2 or not np.all(np.isfinite(mu)) or np.any(np.diff(mu) <= 0) or not (mu[0] >= 0 and mu[-1] <= 1):
            raise ValueError("mu edges must be at least two strictly increasing values within [0, 1]")
    ns, nmu = len(s) - 1, 0 if mu is None else len(mu) - 1
    if ns > 1000 or nmu > 1000 or ns * max(nmu, 1) > _lib.lib().ast_tpcf_max_bins():
        raise ValueError(f"{ns} x {nmu} bins: at most 1000 edges per axis and {_lib.lib().ast_tpcf_max_bins()} bins")
    return s, mu


def tpcf_pair_counts(pos, boxsize, s_edges, mu_edges=None, vel=None, los=2):
    """Unordered pair counts of a periodic box for the two-point correlation function (particles/hutils/tpcf.py):
    an int64 device tensor, (ns, nmu) with ``mu_edges``, else (ns,).  ``vel`` given: the redshift-space shift
    pos[:, los] += vel[:, los] / 100 and one wrap into [0, boxsize], in the input dtypes (tpcf.py:74-97).  Minimum image
    per axis; a pair counts in (k, l) when s_k^2 < d^2 <= s_{k+1}^2 and mu_l < mu <= mu_{l+1}, mu = |d_los| / d.
    ``pos`` / ``vel``: (N, 3), numpy arrays or device tensors, float32 or float64.  ValueError (before any GPU work)
    for bad edges or ``los``, and (from the device bounds) for shifted positions outside [0, boxsize].
    ASTRILD_TPCF_CELLS=0 forces one cell (all pairs) instead of the cell grid."""
    s, mu = check_tpcf_edges(s_edges, mu_edges, boxsize)
    if los not in (0, 1, 2):
        raise ValueError(f"los must be 0, 1 or 2, got {los}")
    one = _pair_sample(pos, vel, "pos must be (N, 3), got {p}", "vel must be (N, 3) like pos, got {v}")
    return _tpcf_counts([one], None, s, mu, float(boxsize), True, los)


def _rppi_plan():
    """The ``plan`` argument of ast_rppi_*: 0, cells of a width per axis; with ASTRILD_RPPI_ANISO=0 the isotropic 1."""
    return 1 if os.environ.get("ASTRILD_RPPI_ANISO", "1") == "0" else 0


def _tpcf_counts(sets, auto, s, mu, box, periodic, los, rppi=False):
    """The calls of tpcf_pair_counts (``sets``: its one ``_pair_sample``; ast_tpcf_prepare / ast_tpcf_pair_counts) and
    of tpcf_cross_counts (two, the second (None, None, 0) for ``auto``; ast_tpcf_cross_prepare / ast_tpcf_cross_counts),
    with the check of the device bounds between the two.  ``rppi``: ``s`` / ``mu`` are r_p / pi edges and the counts
    are ast_rppi_pair_counts' / ast_rppi_cross_counts', on the same prepared workspace."""
    lib = _lib.lib()
    cross = len(sets) == 2
    sizes = [n for _, _, n in sets]
    ns, nmu = len(s) - 1, 0 if mu is None else len(mu) - 1
    single = os.environ.get("ASTRILD_TPCF_CELLS", "1") == "0"
    device_ = sets[0][0].device
    ws_bytes = (lib.ast_tpcf_cross_workspace_bytes if cross else lib.ast_tpcf_workspace_bytes)(*sizes, ns, nmu)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device=device_)
    bounds = torch.empty(6 * len(sets), dtype=torch.float64, device=device_)
    st = stream()
    code = lambda t: real_code(t) if t is not None else F64
    if cross:
        (p1, v1, n1), (p2, v2, n2) = sets
        check(lib.ast_tpcf_cross_prepare(ptr(p1), code(p1), ptr(v1), code(v1), n1, ptr(p2), code(p2), ptr(v2), code(v2),
                                         n2, los, box, ptr(work), ws_bytes, ptr(bounds), st), "ast_tpcf_cross_prepare")
    else:
        p, v, n = sets[0]
        check(lib.ast_tpcf_prepare(ptr(p), code(p), ptr(v), code(v), los, box, n, ptr(work), ws_bytes, ptr(bounds), st),
              "ast_tpcf_prepare")
    _check_device_bounds(to_numpy(bounds), sizes, box, periodic, shifted=True)
    s_d = as_device(s)
    mu_d = as_device(mu) if mu is not None else None
    counts = torch.empty((ns, nmu) if nmu else (ns,), dtype=torch.int64, device=device_)
    tail = (int(single), _rppi_plan()) if rppi else (int(single),)
    if cross:
        count, name = (lib.ast_rppi_cross_counts, "ast_rppi_cross_counts") if rppi else \
            (lib.ast_tpcf_cross_counts, "ast_tpcf_cross_counts")
        check(count(ptr(work), ws_bytes, n1, n2, int(auto), box, los, ptr(s_d), ns, ptr(mu_d), nmu, *tail, ptr(counts),
                    st), name)
    else:
        count, name = (lib.ast_rppi_pair_counts, "ast_rppi_pair_counts") if rppi else \
            (lib.ast_tpcf_pair_counts, "ast_tpcf_pair_counts")
        check(count(ptr(work), ws_bytes, n, box, los, ptr(s_d), ns, ptr(mu_d), nmu, *tail, ptr(counts), st), name)
    return counts


def tpcf_cross_counts(pos1, pos2, s_edges, mu_edges=None, boxsize=None, vel1=None, vel2=None, los=2):
    """Pair counts between two samples for the two-point correlation function (ast_tpcf_cross_prepare /
    ast_tpcf_cross_counts): an int64 device tensor, (ns, nmu) with ``mu_edges``, else (ns,), of every pair (i of
    ``pos1``, j of ``pos2``); ``pos2=None``: the unordered pairs i < j of ``pos1``.  ``boxsize`` given: a periodic
    cube, minimum image per axis, as tpcf_pair_counts; ``boxsize=None``: open boundaries, plain separations.
    ``vel1`` / ``vel2``: the redshift-space shift pos[:, los] += vel[:, los] / 100 per sample in its own dtypes, with
    the single wrap only when periodic.  Bins as tpcf_pair_counts; a pair at distance 0 never counts.  ValueError
    (before any pair work) for bad edges (the top s edge is bounded by boxsize / 3 only when periodic), shapes or
    ``los``, and from the device bounds: periodic, shifted coordinates outside [0, boxsize]; open, any non-finite
    coordinate.  ASTRILD_TPCF_CELLS=0 forces one cell (all pairs) instead of the cell grid."""
    periodic = boxsize is not None
    s, mu = check_tpcf_edges(s_edges, mu_edges, boxsize, periodic=periodic)
    if los not in (0, 1, 2):
        raise ValueError(f"los must be 0, 1 or 2, got {los}")
    auto = pos2 is None
    if auto and vel2 is not None:
        raise ValueError("vel2 given without pos2")
    sample = lambda pos, vel, name: _pair_sample(pos, vel, name + " must be (N, 3), got {p}",
                                                 "the velocities of " + name + " must be (N, 3) like it, got {v}")
    sets = [sample(pos1, vel1, "pos1"), (None, None, 0) if auto else sample(pos2, vel2, "pos2")]
    return _tpcf_counts(sets, auto, s, mu, float(boxsize) if periodic else 0.0, periodic, los)


def check_jackknife_args(nsub, pos1_shape, pos2_shape=None, tags1_shape=None, tags2_shape=None, extent=None,
                         boxsize=None, nbins=1):
    """The argument checks of ``tpcf_jackknife_counts`` that are its own, on the host and without a library call:
    ``(nsub3, ntot, lo, hi)`` or ValueError.  ``nsub``: an int or three ints >= 1 (anything with ``__index__``, no
    bools) -> ``nsub3`` and their product ``ntot``, with ``ntot * nbins <= _lib.TPCF_JK_MAX_TABLE``.  Positions (N, 3).
    Explicit tags: one integer per object, for every sample given or for none, with ``nsub`` a single int (the number
    of regions, ``nsub3 = (nsub, 1, 1)``) and no ``extent``.  ``extent = (lo, hi)``, each a scalar or three values,
    finite with hi > lo -> fp64 ``lo``, ``hi`` of three; without one ``[0, boxsize]`` when periodic, else ``None, None``:
    the caller takes the bounding box of the positions."""
    import operator
    shapes = [tuple(pos1_shape)] + ([] if pos2_shape is None else [tuple(pos2_shape)])
    for k, ps in enumerate(shapes):
        if len(ps) != 2 or ps[1] != 3:
            raise ValueError(f"pos{k + 1} must be (N, 3), got {ps}")
    if pos2_shape is None and tags2_shape is not None:
        raise ValueError("tags2 given without pos2")
    tagged = tags1_shape is not None
    if pos2_shape is not None and (tags2_shape is not None) != tagged:
        raise ValueError("explicit tags are given for both samples or for neither")
    try:
        many = np.ndim(nsub) != 0
        vals = [operator.index(v) for v in nsub] if many else [operator.index(nsub)]
        if any(isinstance(v, (bool, np.bool_)) for v in (nsub if many else [nsub])):
            raise TypeError
    except TypeError:
        raise ValueError(f"nsub must be an int or three ints, got {nsub!r}") from None
    if len(vals) not in (1, 3) or min(vals) < 1:
        raise ValueError(f"nsub must be one or three integers >= 1, got {nsub!r}")
    if tagged:
        if len(vals) != 1:
            raise ValueError("with explicit tags nsub is the number of regions, a single int")
        if extent is not None:
            raise ValueError("extent has no meaning with explicit tags")
        for k, (ps, ts) in enumerate(zip(shapes, (tags1_shape, tags2_shape))):
            if tuple(ts) != (ps[0],):
                raise ValueError(f"tags{k + 1} must be ({ps[0]},), one region per object, got {tuple(ts)}")
        nsub3 = (vals[0], 1, 1)
    else:
        nsub3 = tuple(vals * 3 if len(vals) == 1 else vals)
    ntot = nsub3[0] * nsub3[1] * nsub3[2]
    if ntot * int(nbins) > _lib.TPCF_JK_MAX_TABLE:
        raise ValueError(f"{ntot} regions x {nbins} bins: at most {_lib.TPCF_JK_MAX_TABLE} counters")
    lo = hi = None
    if tagged:
        lo, hi = np.zeros(3), np.ones(3)
    elif extent is not None:
        try:
            lo, hi = (np.broadcast_to(np.asarray(e, dtype=np.float64), (3,)).copy() for e in extent)
        except (TypeError, ValueError):
            raise ValueError(f"extent must be (lo, hi), each a scalar or three values, got {extent!r}") from None
        if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(hi > lo)):
            raise ValueError(f"extent must be finite with hi > lo, got lo {lo.tolist()}, hi {hi.tolist()}")
    elif boxsize is not None:
        lo, hi = np.zeros(3), np.full(3, float(boxsize))
    return nsub3, ntot, lo, hi


def tpcf_jackknife_counts(pos1, nsub, s_edges, mu_edges=None, pos2=None, boxsize=None, vel1=None, vel2=None, los=2,
                          tags1=None, tags2=None, extent=None):
    """The pair counts of tpcf_cross_counts with the endpoint table of a leave-one-region-out jackknife
    (ast_tpcf_jk_prepare / ast_tpcf_jk_counts): ``(counts, ends)``, int64 device tensors of (ns[, nmu]) and
    (ntot, ns[, nmu]).  ``counts`` is tpcf_cross_counts' on the same input (``pos2=None``: unordered pairs of ``pos1``);
    ``ends[k, b]`` is the number of pair ends in region k over the pairs of bin b (both ends in k: 2), so that
    ``2 counts - ends[k]`` is the ordered auto pairs (twice the cross pairs) with region k left out, a pair weighing
    1 / 1/2 / 0 with 0 / 1 / 2 ends in k, and ``ends.sum(0) == 2 counts``.  Regions: ``nsub`` an int or three ints,
    a grid of nsub_x x nsub_y x nsub_z boxes over ``extent = (lo, hi)`` (default: [0, boxsize] when periodic, else the
    bounding box of the given positions of both samples); an object is in box ``floor((x - lo) / ((hi - lo) / nsub))``
    per axis of its position AFTER the redshift-space shift, clamped to the grid, numbered in C order (ntot their
    product).  Or ``tags1`` / ``tags2``: a region in [0, nsub) per object (``nsub`` one int = ntot); a tag out of range
    is a ValueError from the device check, before any pair work.  Everything else as tpcf_cross_counts, including its
    ValueErrors; check_jackknife_args holds the host checks of the arguments above.  ASTRILD_TPCF_CELLS=0 forces one
    cell; ASTRILD_TPCF_JK_LDS=0 forces the table into global memory, whatever its size."""
    periodic = boxsize is not None
    s, mu = check_tpcf_edges(s_edges, mu_edges, boxsize, periodic=periodic)
    return _tpcf_jk_counts(pos1, nsub, s, mu, pos2, boxsize, vel1, vel2, los, tags1, tags2, extent)


def _tpcf_jk_counts(pos1, nsub, s, mu, pos2, boxsize, vel1, vel2, los, tags1, tags2, extent, rppi=False):
    """tpcf_jackknife_counts after its edge check (``s`` / ``mu``: checked edges): the other checks, ast_tpcf_jk_prepare,
    the device checks and ast_tpcf_jk_counts.  ``rppi``: ``s`` / ``mu`` are r_p / pi edges and the counts are
    ast_rppi_jk_counts', on the same prepared workspace."""
    periodic = boxsize is not None
    if los not in (0, 1, 2):
        raise ValueError(f"los must be 0, 1 or 2, got {los}")
    auto = pos2 is None
    if auto and vel2 is not None:
        raise ValueError("vel2 given without pos2")
    ns, nmu = len(s) - 1, 0 if mu is None else len(mu) - 1
    nsub3, ntot, lo, hi = check_jackknife_args(
        nsub, np.shape(pos1), None if auto else np.shape(pos2), None if tags1 is None else np.shape(tags1),
        None if tags2 is None else np.shape(tags2), extent, boxsize, ns * max(nmu, 1))
    sample = lambda pos, vel, name: _pair_sample(pos, vel, name + " must be (N, 3), got {p}",
                                                 "the velocities of " + name + " must be (N, 3) like it, got {v}")
    (p1, v1, n1), (p2, v2, n2) = sample(pos1, vel1, "pos1"), (None, None, 0) if auto else sample(pos2, vel2, "pos2")
    t1 = None if tags1 is None else as_device(tags1).to(torch.int32)
    t2 = None if tags2 is None else as_device(tags2).to(torch.int32)
    if lo is None:
        filled = [p for p in (p1, p2) if p is not None and p.shape[0]]
        lo = np.min([to_numpy(p.amin(0)).astype(np.float64) for p in filled], axis=0) if filled else np.zeros(3)
        hi = np.max([to_numpy(p.amax(0)).astype(np.float64) for p in filled], axis=0) if filled else np.zeros(3)
        if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
            raise ValueError(f"positions must be finite: min {lo.tolist()}, max {hi.tolist()}")
    lib = _lib.lib()
    box = float(boxsize) if periodic else 0.0
    single = os.environ.get("ASTRILD_TPCF_CELLS", "1") == "0"
    force_global = os.environ.get("ASTRILD_TPCF_JK_LDS", "1") == "0"
    ws_bytes = lib.ast_tpcf_jk_workspace_bytes(n1, n2, ns, nmu, ntot)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device=p1.device)
    bounds = torch.empty(13, dtype=torch.float64, device=p1.device)
    st = stream()
    code = lambda t: real_code(t) if t is not None else F64
    nsub_h, lo_h, hi_h = (ct.c_int * 3)(*nsub3), (ct.c_double * 3)(*lo), (ct.c_double * 3)(*hi)
    check(lib.ast_tpcf_jk_prepare(ptr(p1), code(p1), ptr(v1), code(v1), ptr(t1), n1, ptr(p2), code(p2), ptr(v2), code(v2),
                                  ptr(t2), n2, los, box, nsub_h, lo_h, hi_h, ptr(work), ws_bytes, ptr(bounds), st),
          "ast_tpcf_jk_prepare")
    b = to_numpy(bounds)
    _check_device_bounds(b[:12], (n1, n2), box, periodic, shifted=True)
    if b[12] != 0.0:
        raise ValueError(f"explicit tags must lie in [0, {ntot}), the regions of nsub")
    s_d = as_device(s)
    mu_d = as_device(mu) if mu is not None else None
    shape = (ns, nmu) if nmu else (ns,)
    counts = torch.empty(shape, dtype=torch.int64, device=p1.device)
    ends = torch.empty((ntot,) + shape, dtype=torch.int64, device=p1.device)
    count, name = (lib.ast_rppi_jk_counts, "ast_rppi_jk_counts") if rppi else \
        (lib.ast_tpcf_jk_counts, "ast_tpcf_jk_counts")
    tail = (int(force_global), _rppi_plan()) if rppi else (int(force_global),)
    check(count(ptr(work), ws_bytes, n1, n2, int(auto), box, los, ptr(s_d), ns, ptr(mu_d), nmu, ntot, int(single), *tail,
                ptr(counts), ptr(ends), st), name)
    return counts, ends


# ------------------------------------------------------------------ xi(r_p, pi): pairs across and along a line of sight
def check_rp_pi_edges(rp_edges, pi_edges, boxsize, periodic=True):
    """The argument checks of an (r_p, pi) pair count, on the host: fp64 edges ``(rp, pi)`` or ValueError.  Each set
    of edges: at least two values, finite, >= 0, strictly increasing; ``periodic``: ``boxsize`` positive and finite,
    and both top edges below boxsize / 3 (``periodic=False``, open boundaries: ``boxsize`` is not looked at and the
    top edges are free); at most 1000 bins per axis and ``ast_tpcf_max_bins()`` bins in all."""
    if periodic:
        boxsize = float(boxsize)
        if not (np.isfinite(boxsize) and boxsize > 0):
            raise ValueError(f"boxsize must be positive and finite, got {boxsize}")
    top = boxsize / 3.0 if periodic else None
    rp = _check_edges(rp_edges, "rp edge", top=top)
    if pi_edges is None:
        raise ValueError("pi edges must be at least two finite, non-negative, strictly increasing values")
    pi = _check_edges(pi_edges, "pi edge", top=top)
    nrp, npi = len(rp) - 1, len(pi) - 1
    if nrp > 1000 or npi > 1000 or nrp * npi > _lib.lib().ast_tpcf_max_bins():
        raise ValueError(f"{nrp} x {npi} bins: at most 1000 edges per axis and {_lib.lib().ast_tpcf_max_bins()} bins")
    return rp, pi


def rp_pi_pair_counts(pos, boxsize, rp_edges, pi_edges, vel=None, los=2):
    """Unordered pair counts of a periodic box in bins of (r_p, pi) (ast_tpcf_prepare / ast_rppi_pair_counts): an int64
    device tensor (n_rp, n_pi), the twin of tpcf_pair_counts.  Minimum image p_c per axis as there; with a < b the axes
    other than ``los``, rp^2 = p_a^2 + p_b^2 and pi = p_los; a pair counts in (k, l) when rp_k^2 < rp^2 <= rp_{k+1}^2
    and pi_l < pi <= pi_{l+1}, so one with pi on the lowest pi edge (pi = 0 when that edge is 0) or r_p on the lowest
    r_p edge is in no bin, and coincident points never count.  ``vel``, the dtypes, ``los`` and the ValueErrors (edges:
    check_rp_pi_edges) as tpcf_pair_counts.  ASTRILD_TPCF_CELLS=0 forces one cell; ASTRILD_RPPI_ANISO=0 plans the
    isotropic grid of cells sqrt(rp_max^2 + pi_max^2) wide instead of cells r_p,max across and pi_max along ``los``."""
    rp, pi = check_rp_pi_edges(rp_edges, pi_edges, boxsize)
    if los not in (0, 1, 2):
        raise ValueError(f"los must be 0, 1 or 2, got {los}")
    one = _pair_sample(pos, vel, "pos must be (N, 3), got {p}", "vel must be (N, 3) like pos, got {v}")
    return _tpcf_counts([one], None, rp, pi, float(boxsize), True, los, rppi=True)


def rp_pi_cross_counts(pos1, pos2, rp_edges, pi_edges, boxsize=None, vel1=None, vel2=None, los=2):
    """Pair counts between two samples in bins of (r_p, pi) (ast_tpcf_cross_prepare / ast_rppi_cross_counts): an int64
    device tensor (n_rp, n_pi) of every pair (i of ``pos1``, j of ``pos2``); ``pos2=None``: the unordered pairs of
    ``pos1``.  The twin of tpcf_cross_counts - ``boxsize`` (None: open boundaries), ``vel1`` / ``vel2``, dtypes,
    ``los`` and ValueErrors as there - with the geometry, bins and switches of rp_pi_pair_counts."""
    periodic = boxsize is not None
    rp, pi = check_rp_pi_edges(rp_edges, pi_edges, boxsize, periodic=periodic)
    if los not in (0, 1, 2):
        raise ValueError(f"los must be 0, 1 or 2, got {los}")
    auto = pos2 is None
    if auto and vel2 is not None:
        raise ValueError("vel2 given without pos2")
    sample = lambda pos, vel, name: _pair_sample(pos, vel, name + " must be (N, 3), got {p}",
                                                 "the velocities of " + name + " must be (N, 3) like it, got {v}")
    sets = [sample(pos1, vel1, "pos1"), (None, None, 0) if auto else sample(pos2, vel2, "pos2")]
    return _tpcf_counts(sets, auto, rp, pi, float(boxsize) if periodic else 0.0, periodic, los, rppi=True)


def rp_pi_jackknife_counts(pos1, nsub, rp_edges, pi_edges, pos2=None, boxsize=None, vel1=None, vel2=None, los=2,
                           tags1=None, tags2=None, extent=None):
    """rp_pi_cross_counts with the endpoint table of a leave-one-region-out jackknife (ast_tpcf_jk_prepare /
    ast_rppi_jk_counts): ``(counts, ends)``, int64 device tensors of (n_rp, n_pi) and (ntot, n_rp, n_pi).  The twin of
    tpcf_jackknife_counts: regions, tags, ``extent``, the identities ``ends.sum(0) == 2 counts`` and ``2 counts -
    ends[k]``, ValueErrors and ASTRILD_TPCF_JK_LDS as there; geometry, bins and switches as rp_pi_pair_counts."""
    rp, pi = check_rp_pi_edges(rp_edges, pi_edges, boxsize, periodic=boxsize is not None)
    return _tpcf_jk_counts(pos1, nsub, rp, pi, pos2, boxsize, vel1, vel2, los, tags1, tags2, extent, rppi=True)


# ------------------------------------------------------------------ pairwise-velocity moments in a box
def check_pair_velocity_args(pos1_shape, vel1_shape, edges, pos2_shape=None, vel2_shape=None, boxsize=None,
                             kind="radial", pi_max=None, los=2):
    """The argument checks of ``pair_velocity_moments`` on the host, without a library call:
    ``(edges, box, pi_max, n1, n2)`` - fp64 edges, ``box`` 0.0 for open boundaries, ``pi_max`` 0.0 for "radial",
    ``n2`` 0 without a second sample - or ValueError.  Edges finite, >= 0, strictly increasing, at most
    ``_lib.PAIRVEL_MAX_BINS`` bins; with a ``boxsize`` (positive, finite) the top edge, and for "los" also ``pi_max``,
    below boxsize / 3 (as check_tpcf_edges); "los" needs a positive, finite ``pi_max``; ``los`` 0, 1 or 2; positions
    (N, 3) with velocities shaped like them; a second sample has both positions and velocities or neither."""
    if kind not in _lib.PAIRVEL_KIND:
        raise ValueError(f"kind must be one of {sorted(_lib.PAIRVEL_KIND)}, got {kind!r}")
    if isinstance(los, bool) or los not in (0, 1, 2):
        raise ValueError(f"los must be 0, 1 or 2, got {los!r}")
    periodic = boxsize is not None
    box = 0.0
    if periodic:
        box = float(boxsize)
        if not (np.isfinite(box) and box > 0):
            raise ValueError(f"boxsize must be positive and finite, got {box}")
    e = _check_edges(edges, "bin edge", top=box / 3.0 if periodic else None, max_bins=_lib.PAIRVEL_MAX_BINS)
    pmax = 0.0
    if kind == "los":
        pmax = _positive_real("pi_max", pi_max)
        if periodic and not pmax < box / 3.0:
            raise ValueError(f"pi_max ({pmax}) must be below boxsize / 3 ({box / 3.0})")
    if pos2_shape is None and vel2_shape is not None:
        raise ValueError("vel2 given without pos2")
    if pos2_shape is not None and vel2_shape is None:
        raise ValueError("pos2 given without vel2")
    ns = []
    for k, (ps, vs) in enumerate(((pos1_shape, vel1_shape), (pos2_shape, vel2_shape))):
        if ps is None:
            ns.append(0)
            continue
        if vs is None:
            raise ValueError(f"sample {k + 1} needs velocities")
        ps, vs = tuple(ps), tuple(vs)
        if len(ps) != 2 or ps[1] != 3 or vs != ps:
            raise ValueError(f"positions and velocities of sample {k + 1} must both be (N, 3), got {ps} and {vs}")
        if ps[0] >= 1 << 31:
            raise ValueError(f"sample {k + 1}: fewer than 2^31 objects")
        ns.append(ps[0])
    return e, box, pmax, ns[0], ns[1]


def pair_velocity_moments(pos1, vel1, edges, pos2=None, vel2=None, boxsize=None, kind="radial", pi_max=None, los=2):
    """Count, sum v and sum v^2 per separation bin of the pairwise velocity (ast_pairvel_prepare /
    ast_pairvel_moments): device tensors ``(count, s1, s2)``, (nb,) int64 / float64 / float64, over every pair (i of
    sample 1, j of sample 2); ``pos2=None``: the unordered pairs i < j of sample 1.  ``boxsize`` given: a periodic
    cube, each separation component s = x_j - x_i moved by -+ boxsize when beyond +- boxsize / 2; ``boxsize=None``: open
    boundaries, plain separations.  With dv = v_j - v_i, all in fp64:
    "radial": d^2 = (s_x^2 + s_y^2) + s_z^2 in bin k when edges_k^2 < d^2 <= edges_{k+1}^2 (a pair at distance 0 is in
    no bin), v = dv . s / d;  "los": rp^2 = s_a^2 + s_b^2 over the two axes other than ``los`` in bin k when
    edges_k^2 < rp^2 <= edges_{k+1}^2 and |s_los| <= pi_max, v = dv_los sign(s_los).  The counts of "radial" are those
    of tpcf_cross_counts on the same edges.  Positions and velocities: (N, 3), numpy arrays or device tensors, float32
    or float64 in any combination (widened to float64 on load).  ValueError before any library call for bad arguments
    (check_pair_velocity_args), and from the device bounds before any pair work: periodic, coordinates outside
    [0, boxsize]; open, any non-finite coordinate.  ASTRILD_PAIRVEL_CELLS=0 forces one cell (all pairs)."""
    e, box, pmax, n1, n2 = check_pair_velocity_args(
        np.shape(pos1), np.shape(vel1), edges, None if pos2 is None else np.shape(pos2),
        None if vel2 is None else np.shape(vel2), boxsize, kind, pi_max, los)
    periodic = boxsize is not None
    auto = pos2 is None
    lib = _lib.lib()
    p1, v1 = _real_device(pos1), _real_device(vel1)
    p2, v2 = (None, None) if auto else (_real_device(pos2), _real_device(vel2))
    nb = len(e) - 1
    single = os.environ.get("ASTRILD_PAIRVEL_CELLS", "1") == "0"
    ws_bytes = lib.ast_pairvel_workspace_bytes(n1, n2, nb)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device=p1.device)
    bounds = torch.empty(12, dtype=torch.float64, device=p1.device)
    st = stream()
    code = lambda t: real_code(t) if t is not None else F64
    check(lib.ast_pairvel_prepare(ptr(p1), code(p1), ptr(v1), code(v1), n1, ptr(p2), code(p2), ptr(v2), code(v2), n2,
                                  ptr(work), ws_bytes, ptr(bounds), st), "ast_pairvel_prepare")
    _check_device_bounds(to_numpy(bounds), (n1, n2), box, periodic)
    e_d = as_device(e)
    count = torch.empty(nb, dtype=torch.int64, device=p1.device)
    s1 = torch.empty(nb, dtype=torch.float64, device=p1.device)
    s2 = torch.empty(nb, dtype=torch.float64, device=p1.device)
    check(lib.ast_pairvel_moments(ptr(work), ws_bytes, n1, n2, int(auto), box, _lib.PAIRVEL_KIND[kind], int(los), pmax,
                                  ptr(e_d), nb, int(single), ptr(count), ptr(s1), ptr(s2), st), "ast_pairvel_moments")
    return count, s1, s2


def finish_pair_velocity(count, s1, s2):
    """``(mean, sigma)`` per bin from the moments, host fp64: mean = s1 / count,
    sigma = sqrt(max(s2 / count - mean^2, 0)); NaN in empty bins.  Device tensors or arrays."""
    c, a, b = (to_numpy(x) if isinstance(x, torch.Tensor) else np.asarray(x) for x in (count, s1, s2))
    c, a, b = c.astype(np.float64), a.astype(np.float64), b.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = a / c
        var = b / c - mean * mean
        sigma = np.sqrt(np.where(var > 0.0, var, np.where(np.isnan(var), np.nan, 0.0)))
    return mean, sigma


def annulus_profiles(skymap, x_pix, y_pix, rad_pix, extend, nbins, delta_eta=None):
    """Per-annulus sums and pixel counts of objects on a 2D map (profiles/profile_2d.py: from_map / profiling): device
    tensors ``(sums, counts)``, (N, nbins) float64 and int64, the true sums and counts (not the reference's count
    alignment, which ``profile_2d.aligned_values`` applies).  Object i reads skymap[y + a, x + b] for -R <= a, b < R,
    R = ceil(r * extend), into bin eta = int(sqrt(a^2 + b^2) / r / delta_eta) when eta < nbins, with r, x, y truncated
    to integers and delta_eta = extend / nbins unless given; negative indices wrap as numpy's do.  The bins are decided
    on the host with exact integer thresholds (``profile_2d.annulus_geometry``), which also raises IndexError /
    ValueError before any GPU work.  ``skymap``: a 2D numpy array or device tensor, float32 or float64.
    ASTRILD_PROFILE_BANDS=0 makes each object one work item instead of bands of rows."""
    import os
    from .profiles import profile_2d as p2d
    lib = _lib.lib()
    shape = tuple(skymap.shape)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"skymap must be a non-empty 2D map, got shape {shape}")
    if int(nbins) == nbins and not 1 <= nbins <= lib.ast_profile2d_max_bins():
        raise ValueError(f"nbins must be in 1..{lib.ast_profile2d_max_bins()}, got {nbins}")
    y, x, R, m, T = p2d.annulus_geometry(shape, x_pix, y_pix, rad_pix, extend, nbins, delta_eta)
    nbins = int(nbins)
    t = as_device(skymap)
    t = t if t.dtype in _REAL else t.to(torch.float64)
    n = len(R)
    rows = m + np.minimum(m, R - 1) + 1
    bands = os.environ.get("ASTRILD_PROFILE_BANDS", "1") != "0"
    band_rows = lib.ast_profile2d_band_rows() if bands else 0
    per_obj = -(-rows // band_rows) if bands else np.ones(n, dtype=np.int64)
    item_start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(per_obj, out=item_start[1:])
    n_work = int(item_start[-1])
    centres = as_device(np.stack([y, x], axis=1))
    reach = as_device(np.stack([R, m], axis=1))
    thr = as_device(np.ascontiguousarray(T, dtype=np.int64))
    starts = as_device(item_start)
    ws_bytes = lib.ast_profile2d_workspace_bytes(n, n_work, nbins)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device=t.device)
    sums = torch.empty((n, nbins), dtype=torch.float64, device=t.device)
    counts = torch.empty((n, nbins), dtype=torch.int64, device=t.device)
    check(lib.ast_profile2d(ptr(t), real_code(t), shape[0], shape[1], n, ptr(centres), ptr(reach), ptr(thr), nbins,
                            band_rows, ptr(starts), n_work, ptr(work), ws_bytes, ptr(sums), ptr(counts), stream()),
          "ast_profile2d")
    return sums, counts


# ------------------------------------------------------------------ spherical profiles around centres
PROFILE3D_OCCUPANCY = 4             # mean particles per cell the search grid aims at
PROFILE3D_CELL_CAP = 1 << 21        # default cap on the search grid's cells (128^3)


def _host_array(a, dtype=None):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def _icbrt(n):
    """Largest integer d with d^3 <= n."""
    d = int(round(float(n) ** (1.0 / 3.0)))
    while d ** 3 > n:
        d -= 1
    while (d + 1) ** 3 <= n:
        d += 1
    return d


def profile3d_dims(npart, cell_cap=None):
    """Cells per axis of the search grid of ``sphere_profiles``: a pure function of the particle count and the cell cap
    (no look at the data, so the host can plan the work list without a read-back): about PROFILE3D_OCCUPANCY particles
    per cell, at most ``cell_cap`` (default PROFILE3D_CELL_CAP) cells, at least one."""
    cap = PROFILE3D_CELL_CAP if cell_cap is None else int(cell_cap)
    if cap < 1:
        raise ValueError(f"cell_cap must be at least 1, got {cell_cap}")
    cap = min(cap, 1 << 24)                 # ast_profile3d_max_cells()
    return max(1, min(_icbrt(max(int(npart), 1) // PROFILE3D_OCCUPANCY), _icbrt(cap)))


def check_profile3d_args(pos_shape, centres, radii, edges, boxsize=None, weights_shape=None, vel_shape=None,
                         centre_vel=None, segments=None, max_bins=256):
    """The host-side argument checks of ``sphere_profiles``: fp64 ``(centres, radii, edges, centre_vel, segments)``
    (the last two None when not given) or ValueError."""
    if len(pos_shape) != 2 or pos_shape[1] != 3:
        raise ValueError(f"pos must be (Np, 3), got {tuple(pos_shape)}")
    n = pos_shape[0]
    if weights_shape is not None and tuple(weights_shape) != (n,):
        raise ValueError(f"weights must be (Np,) = ({n},), got {tuple(weights_shape)}")
    if vel_shape is not None and tuple(vel_shape) != (n, 3):
        raise ValueError(f"vel must be (Np, 3) like pos, got {tuple(vel_shape)}")
    e = _host_array(edges, np.float64).reshape(-1)
    if len(e) < 2 or not np.all(np.isfinite(e)) or np.any(np.diff(e) <= 0) or e[0] < 0:
        raise ValueError("edges must be at least two finite, non-negative, strictly increasing values")
    if len(e) - 1 > max_bins:
        raise ValueError(f"{len(e) - 1} bins: at most {max_bins}")
    c = _host_array(centres, np.float64)
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError(f"centres must be (Nc, 3), got {c.shape}")
    nc = c.shape[0]
    if not np.all(np.isfinite(c)):
        raise ValueError("centres must be finite")
    r = _host_array(radii, np.float64)
    if r.shape != (nc,):
        raise ValueError(f"radii must be (Nc,) = ({nc},), got {r.shape}")
    if not (np.all(np.isfinite(r)) and np.all(r > 0)):
        raise ValueError("radii must be positive and finite")
    cv = None
    if centre_vel is not None:
        if vel_shape is None:
            raise ValueError("centre_vel given without vel")
        cv = _host_array(centre_vel, np.float64)
        if cv.shape != (nc, 3) or not np.all(np.isfinite(cv)):
            raise ValueError(f"centre_vel must be finite and (Nc, 3) = ({nc}, 3), got {cv.shape}")
    if boxsize is not None:
        box = float(boxsize)
        if not (np.isfinite(box) and box > 0):
            raise ValueError(f"boxsize must be positive and finite, got {boxsize}")
        if nc and not np.max(e[-1] * r) < box / 2.0:
            raise ValueError(f"the largest reach edges[-1] * radius ({np.max(e[-1] * r)}) must be below boxsize / 2 "
                             f"({box / 2.0})")
        if nc and not (np.all(c >= 0.0) and np.all(c <= box)):
            raise ValueError(f"centres must lie in [0, {box}]")
    seg = None
    if segments is not None:
        seg = _host_array(segments)
        if seg.shape != (nc, 2) or not np.issubdtype(seg.dtype, np.integer):
            raise ValueError(f"segments must be integer (offset, count) pairs, (Nc, 2) = ({nc}, 2), got {seg.shape} "
                             f"{seg.dtype}")
        seg = seg.astype(np.int64)
        if nc and not (np.all(seg >= 0) and np.all(seg[:, 0] + seg[:, 1] <= n)):
            raise ValueError(f"segments must lie within [0, Np] = [0, {n}]")
    return c, r, e, cv, seg


def _profile3d_axis_range(c, reach, lo, inv, dims, periodic):
    """(first cell, number of cells) that [c - reach, c + reach] touches on one axis: p3_axis_range of profile3d.hip."""
    big = float(1 << 30)
    a = np.clip(np.floor((c - reach - lo) * inv), -big, big).astype(np.int64)
    b = np.clip(np.floor((c + reach - lo) * inv), -big, big).astype(np.int64)
    if periodic:
        full = b - a + 1 >= dims
        return np.where(full, 0, np.mod(a, dims)), np.where(full, dims, b - a + 1)
    a, b = np.maximum(a, 0), np.minimum(b, dims - 1)
    ok = b >= a
    return np.where(ok, a, 0), np.where(ok, b - a + 1, 0)


def sphere_profiles(pos, centres, radii, edges, boxsize=None, weights=None, vel=None, centre_vel=None, segments=None,
                    cell_cap=None):
    """Radial histograms of particles around centres (ast_profile3d_*; the reference's profiles/profile_3d.py): device
    tensors ``(counts, moments)``, (Nc, nbins) int64 and (Nc, nbins, M) float64 with M = 1 (the sum of w) or, with
    ``vel``, M = 4 (the sums of w, w v_r, w v_r^2, w |u|^2; u = v - centre_vel, v_r = u.s / d, 0 at d = 0).  ``edges``
    are in units of each centre's radius.  Per particle s = p - c, with ``boxsize`` wrapped once per axis (s > L/2 ->
    s - L, else s < -L/2 -> s + L; ``boxsize=None``: open, plain separations), d^2 = (sx^2 + sy^2) + sz^2 in fp64 and
    x = sqrt(d^2) / R goes to bin k when e_k <= x < e_{k+1}, the last bin also taking x == e_last: np.histogram's rule.
    A particle at distance 0 counts when e_0 == 0 - unlike the pair counts of the TPCF, which never count d = 0.
    ``segments=None``: every particle in reach is found through a cell grid of ``profile3d_dims(Np, cell_cap)``^3 cells.
    ``segments`` (Nc, 2) integer (offset, count): centre i bins only particles offset_i .. offset_i + count_i - 1 (the
    reference's cum_N_particles / N_particles).  ``pos`` / ``weights`` / ``vel``: numpy arrays or device tensors,
    float32 or float64; centres, radii and centre_vel: host arrays or tensors (the work list is built on the host).
    ValueError before any GPU work for shapes, dtypes, edges, radii that are not positive and finite, a periodic reach
    max(edges[-1] * radii) >= boxsize / 2, periodic centres outside [0, boxsize], segments outside [0, Np]; and from the
    device bounds for periodic positions outside [0, boxsize] or open positions that are not finite.  Nc = 0 or Np = 0
    returns zeros without a launch.  ASTRILD_PROFILE3D_CELLS=0 forces one cell, ASTRILD_PROFILE3D_LAYERS=0 one work
    item per centre (both for the tests)."""
    lib = _lib.lib()
    shape = lambda t: None if t is None else tuple(np.shape(t))
    c, r, e, cv, seg = check_profile3d_args(shape(pos), centres, radii, edges, boxsize, shape(weights), shape(vel),
                                            centre_vel, segments, max_bins=lib.ast_profile3d_max_bins())
    periodic = boxsize is not None
    box = float(boxsize) if periodic else 0.0
    n, nc, nbins, nmom = int(shape(pos)[0]), len(r), len(e) - 1, 4 if vel is not None else 1
    real = lambda t: None if t is None else (lambda d: d if d.dtype in _REAL else d.to(torch.float64))(as_device(t))
    p, w, v = real(pos), real(weights), real(vel)
    if nc == 0 or n == 0:
        return (torch.zeros((nc, nbins), dtype=torch.int64, device=p.device),
                torch.zeros((nc, nbins, nmom), dtype=torch.float64, device=p.device))
    search = seg is None
    single = os.environ.get("ASTRILD_PROFILE3D_CELLS", "1") == "0"
    dims = (1 if single else profile3d_dims(n, cell_cap)) if search else 0
    ncells = dims ** 3
    st = stream()
    code = lambda t: real_code(t) if t is not None else F64
    bounds = torch.empty(6, dtype=torch.float64, device=p.device)

    def prepare(work, ws_bytes, bounds_only=False):
        check(lib.ast_profile3d_prepare(ptr(p), code(p), ptr(w), code(w), ptr(v), code(v), n, int(bounds_only),
                                        ptr(work), ws_bytes, ptr(bounds), st), "ast_profile3d_prepare")
        b = to_numpy(bounds)
        if periodic and not (np.all(b[:3] >= 0.0) and np.all(b[3:] <= box)):
            raise ValueError(f"positions must lie in [0, {box}]: min {b[:3].tolist()}, max {b[3:].tolist()}")
        if not periodic and not np.all(np.isfinite(b)):
            raise ValueError(f"positions must be finite: min {b[:3].tolist()}, max {b[3:].tolist()}")
        return b

    if search and not periodic:
        # open boundaries: the grid spans the bounding box and the work list (hence the workspace's size) follows from
        # it, so a bounds-only pass over the positions comes first; it writes no records
        b = prepare(torch.empty(256, dtype=torch.uint8, device=p.device), 256, bounds_only=True)
        lo, ext = b[:3].copy(), b[3:] - b[:3]
        inv = np.where(ext > 0.0, dims / np.where(ext > 0.0, ext, 1.0), 0.0) if dims > 1 else np.zeros(3)
        pad = 1e-12 * float(np.max(np.abs(b)))
    elif search:
        lo = np.zeros(3)
        inv = np.full(3, dims / box if dims > 1 else 0.0)
        pad = 1e-12 * box
    if search:
        reach = (e[-1] * r) * (1.0 + 1e-9) + pad
        z0, nz = _profile3d_axis_range(c[:, 2], reach, lo[2], inv[2], dims, periodic)
        per = lib.ast_profile3d_layers() if os.environ.get("ASTRILD_PROFILE3D_LAYERS", "1") != "0" else 0
        per_centre = np.maximum(1, -(-nz // per)) if per else np.ones(nc, dtype=np.int64)
        zrange = as_device(np.ascontiguousarray(np.stack([z0, nz], axis=1), dtype=np.int32))
    else:
        per = lib.ast_profile3d_chunk()
        per_centre = np.maximum(1, -(-seg[:, 1] // per))
        seg_d = as_device(seg)
    item_start = np.zeros(nc + 1, dtype=np.int64)
    np.cumsum(per_centre, out=item_start[1:])
    part_start = np.zeros(nc + 1, dtype=np.int64)
    np.cumsum(np.where(per_centre > 1, per_centre, 0), out=part_start[1:])
    n_items, n_part = int(item_start[-1]), int(part_start[-1])
    ws_bytes = lib.ast_profile3d_workspace_bytes(n, ncells, n_part, nbins, nmom)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device=p.device)
    prepare(work, ws_bytes)
    c_d, r_d, e_d, cv_d = as_device(c), as_device(r), as_device(e), as_device(cv) if cv is not None else None
    starts, parts = as_device(item_start), as_device(part_start)
    counts = torch.empty((nc, nbins), dtype=torch.int64, device=p.device)
    moments = torch.empty((nc, nbins, nmom), dtype=torch.float64, device=p.device)
    if search:
        check(lib.ast_profile3d_search(ptr(work), ws_bytes, n, dims, lo[0], lo[1], lo[2], inv[0], inv[1], inv[2], box,
                                       pad, nc, ptr(c_d), ptr(r_d), ptr(cv_d), ptr(zrange), per, ptr(starts), n_items,
                                       ptr(parts), n_part, ptr(e_d), nbins, nmom, ptr(counts), ptr(moments), st),
              "ast_profile3d_search")
    else:
        check(lib.ast_profile3d_members(ptr(work), ws_bytes, n, box, nc, ptr(c_d), ptr(r_d), ptr(cv_d), ptr(seg_d), per,
                                        ptr(starts), n_items, ptr(parts), n_part, ptr(e_d), nbins, nmom, ptr(counts),
                                        ptr(moments), st), "ast_profile3d_members")
    return counts, moments


# ------------------------------------------------------------------ tunnels void finder
def check_tunnels_tracers(x_pix, y_pix, npix):
    """The argument checks of ``tunnels_voids``, before any GPU work: ``(x, y, npix, on_device)`` with x, y 1D integer
    arrays (numpy, or device tensors when they came as tensors) or ValueError."""
    npix = int(npix)
    if npix < 1:
        raise ValueError(f"npix must be positive, got {npix}")
    on_device = isinstance(x_pix, torch.Tensor) and isinstance(y_pix, torch.Tensor)
    if on_device:
        x, y = x_pix.reshape(-1), y_pix.reshape(-1)
        integer = not (x.dtype.is_floating_point or x.dtype.is_complex or y.dtype.is_floating_point
                       or y.dtype.is_complex or x.dtype == torch.bool or y.dtype == torch.bool)
    else:
        x, y = np.asarray(x_pix).reshape(-1), np.asarray(y_pix).reshape(-1)
        integer = (x.dtype.kind in "iu" and y.dtype.kind in "iu") or (x.size == 0 and y.size == 0)
    if not integer:
        raise ValueError(f"tracer coordinates must be integer pixel indices, got {x.dtype} and {y.dtype}")
    n = int(x.shape[0])
    if int(y.shape[0]) != n:
        raise ValueError(f"x_pix and y_pix must have one entry per tracer, got {n} and {int(y.shape[0])}")
    if n >= 1 << 31:
        raise ValueError(f"{n} tracers: fewer than 2^31 are supported")
    if n:
        lo, hi = min(int(x.min()), int(y.min())), max(int(x.max()), int(y.max()))
        if lo < 0 or hi >= npix:
            raise ValueError(f"tracer coordinates must lie in [0, {npix}), got {lo} .. {hi}")
        key = (y.to(torch.int64) if on_device else y.astype(np.int64)) * npix + x
        distinct = int(torch.unique(key).numel()) if on_device else len(np.unique(key))
        if distinct != n:
            raise ValueError(f"{n - distinct} duplicate tracers: all tracers must be distinct")
    if not on_device:
        x, y = x.astype(np.int32), y.astype(np.int32)
    return x, y, npix, on_device


def tunnels_voids(x_pix, y_pix, npix, return_violations=False):
    """The tunnels voids of tracers on an ``npix``^2 map (rays/voids/tunnel.py; ``ast_tunnels_find``): the circles
    through at least three tracers with no tracer strictly inside and their centre in the map, as an (M, 7) int64 array
    of records (i, e, k, n_on, X, Y, W) sorted by (i, e, k): i the smallest tracer index on the circle, e the tracer on
    it with all others strictly left of i -> e, k the next one counter-clockwise, n_on the number of tracers on it,
    centre (X / W, Y / W) (``tunnels_circles`` forms the floats).  ``x_pix`` (column) / ``y_pix`` (row): distinct integer
    pixel coordinates in [0, npix), npix <= ``ast_tunnels_max_npix()``; numpy arrays give a numpy array, device tensors
    a device tensor.  ValueError before any GPU work otherwise.  Fewer than three tracers, or only collinear ones,
    give an empty array.  All decisions are exact integers, so repeated calls are bit-identical.  The device also counts
    violations (circles it found with a tracer inside, walks that did not end): any raises AstrildHipError, unless
    ``return_violations`` asks for ``(records, violations)`` instead.
    ASTRILD_TUNNELS_CELLS=0 forces a single cell (every scan sees all tracers) instead of the cell grid."""
    x, y, npix, on_device = check_tunnels_tracers(x_pix, y_pix, npix)
    lib = _lib.lib()
    if npix > lib.ast_tunnels_max_npix():
        raise ValueError(f"npix={npix}: at most {lib.ast_tunnels_max_npix()} (the in-circle test is exact in int64)")
    n = int(x.shape[0])
    if n < 3:
        none = torch.zeros((0, 7), dtype=torch.int64, device=device()) if on_device else np.zeros((0, 7), np.int64)
        return (none, 0) if return_violations else none
    xd, yd = as_device(x, torch.int32), as_device(y, torch.int32)
    single = os.environ.get("ASTRILD_TUNNELS_CELLS", "1") == "0"
    ws_bytes = lib.ast_tunnels_workspace_bytes(n, npix)
    work = torch.empty(ws_bytes, dtype=torch.uint8, device=xd.device)
    records = torch.empty((2 * n, 7), dtype=torch.int64, device=xd.device)
    count = torch.empty(2, dtype=torch.int64, device=xd.device)
    check(lib.ast_tunnels_find(ptr(xd), ptr(yd), n, npix, int(single), ptr(work), ws_bytes, ptr(records), ptr(count),
                               stream()), "ast_tunnels_find")
    m, violations = (int(v) for v in count.cpu())
    if (violations and not return_violations) or m > 2 * n:
        raise _lib.AstrildHipError(f"ast_tunnels_find: {violations} violations (circles with a tracer inside or walks "
                                   f"that did not end), {m} records for {n} tracers")
    records = records[:m]
    records = records[torch.argsort(records[:, 0] * (1 << 31) + records[:, 1])]     # (i, e) is unique per circle
    records = records if on_device else to_numpy(records)
    return (records, violations) if return_violations else records


def tunnels_circles(records, x_pix, y_pix):
    """``(cx, cy, r)`` in pixels, float64 numpy arrays, from the integer records of ``tunnels_voids``: cx = X / W,
    cy = Y / W, r = hypot(X - W x_i, Y - W y_i) / W."""
    rec = to_numpy(records) if isinstance(records, torch.Tensor) else np.asarray(records, dtype=np.int64)
    rec = rec.reshape(-1, 7)
    x = to_numpy(x_pix) if isinstance(x_pix, torch.Tensor) else np.asarray(x_pix)
    y = to_numpy(y_pix) if isinstance(y_pix, torch.Tensor) else np.asarray(y_pix)
    x, y = x.reshape(-1).astype(np.int64), y.reshape(-1).astype(np.int64)
    X, Y, W = rec[:, 4], rec[:, 5], rec[:, 6]
    ux, uy = X - W * x[rec[:, 0]], Y - W * y[rec[:, 0]]
    return X / W, Y / W, np.hypot(ux, uy) / W


# ------------------------------------------------------------------ watershed void finder
WATERSHED_INT_SUMS = ("area", "sum_x", "sum_y", "edge_pix")


def check_watershed_map(img):
    """The argument checks of ``watershed_basins``, before any GPU work: a square 2D float32 / float64 map (numpy array
    or tensor) with 3 <= npix and npix^2 < 2^31.  Returns ``(npix, on_device)`` or raises ValueError."""
    on_device = isinstance(img, torch.Tensor)
    if not on_device:
        img = np.asarray(img)
    shape = tuple(int(s) for s in img.shape)
    if len(shape) != 2 or shape[0] != shape[1]:
        raise ValueError(f"a square 2D map is expected, got shape {shape}")
    floating = img.dtype in (torch.float32, torch.float64) if on_device else img.dtype in (np.float32, np.float64)
    if not floating:
        raise ValueError(f"the map must be float32 or float64, got {img.dtype}")
    npix = shape[0]
    if npix < 3 or npix * npix >= 1 << 31:
        raise ValueError(f"npix={npix}: 3 <= npix and npix^2 < 2^31 are required")
    return npix, on_device


def watershed_basins(img, return_passes=False):
    """The watershed basins of a square map (``ast_watershed_*``).  Pixels are ordered by (f[p], p) with
    p = y npix + x, values compared in the map's dtype; every pixel links to the smallest of itself and its up-to-8
    neighbours inside the map; a basin is the set of pixels whose links end at the same minimum.  Returns a dict:

    * ``labels`` (npix, npix) int32: the basin of every pixel, basins numbered 0 .. M - 1 in ascending flat index of
      their minimum;
    * ``minima`` (M,) int64 flat indices, ``f_min`` (M,) their values in the map's dtype;
    * ``area``, ``sum_x``, ``sum_y``, ``edge_pix`` (M,) int64: pixel count, sums of column and row, pixels on the
      outermost rows / columns; ``sum_f`` (M,) float64 (atomic additions: the last bits may differ between calls);
    * ``edges`` (E, 2) int32 pairs a < b of basins with 8-adjacent pixels, sorted by (a, b), and ``saddle`` (E,) in the
      map's dtype: the minimum over those pixel pairs of max(f[p], f[q]) (a zero saddle is +0.0).

    A numpy array gives numpy arrays, a device tensor device tensors; the map is not changed.  ValueError before any
    launch for a map that is not square, float32 / float64 and of 3 <= npix, npix^2 < 2^31, and with no result when the
    device finds a NaN or an infinity in it.  ``return_passes``: ``(dict, pointer-jumping passes taken)``."""
    npix, on_device = check_watershed_map(img)
    lib = _lib.lib()
    t = as_device(img)
    code, n = real_code(t), npix * npix
    link = torch.empty(n, dtype=torch.int32, device=t.device)
    count = torch.empty(1, dtype=torch.int64, device=t.device)
    check(lib.ast_watershed_link(ptr(t), code, npix, ptr(link), ptr(count), stream()), "ast_watershed_link")
    bad = int(count.item())
    if bad:
        raise ValueError(f"the map holds {bad} pixels that are NaN or infinite")
    pending = torch.empty(lib.ast_watershed_max_passes(npix), dtype=torch.int32, device=t.device)
    passes = ct.c_int(0)
    check(lib.ast_watershed_jump(ptr(link), npix, ptr(pending), ct.byref(passes), stream()), "ast_watershed_jump")
    # compact ids in ascending index of the minimum (torch: plumbing), then labels = id[minimum of the pixel]
    minima = torch.nonzero(link == torch.arange(n, dtype=torch.int32, device=t.device)).reshape(-1)
    m = int(minima.numel())
    ids = torch.empty(n, dtype=torch.int32, device=t.device)        # read at minima only
    ids[minima] = torch.arange(m, dtype=torch.int32, device=t.device)
    labels = torch.empty(n, dtype=torch.int32, device=t.device)
    check(lib.ast_watershed_relabel(ptr(link), ptr(ids), n, n, ptr(labels), stream()), "ast_watershed_relabel")
    del link, ids
    isums = torch.empty((4, m), dtype=torch.int64, device=t.device)
    sum_f = torch.empty(m, dtype=torch.float64, device=t.device)
    check(lib.ast_watershed_sums(ptr(t), code, ptr(labels), npix, m, ptr(isums), ptr(sum_f), stream()),
          "ast_watershed_sums")
    # boundary pairs: count, allocate exactly, fill; then one minimum per pair (sort and segment minimum in torch)
    blocks = torch.empty(lib.ast_watershed_edge_blocks(npix), dtype=torch.int64, device=t.device)
    check(lib.ast_watershed_edges(ptr(t), code, ptr(labels), npix, ptr(blocks), 0, None, None, stream()),
          "ast_watershed_edges")
    ends = torch.cumsum(blocks, 0)
    nrec = int(ends[-1].item())
    if nrec:
        first = ends - blocks                        # every tile's first record
        keys = torch.empty(nrec, dtype=torch.int64, device=t.device)
        sad = torch.empty(nrec, dtype=t.dtype, device=t.device)
        check(lib.ast_watershed_edges(ptr(t), code, ptr(labels), npix, ptr(first), nrec, ptr(keys), ptr(sad), stream()),
              "ast_watershed_edges")
        keys, order = torch.sort(keys)
        pairs, inverse = torch.unique_consecutive(keys, return_inverse=True)
        saddle = torch.full((int(pairs.numel()),), float("inf"), dtype=t.dtype, device=t.device)
        saddle = saddle.scatter_reduce(0, inverse, sad[order], "amin")
        edges = torch.stack([pairs >> 32, pairs & 0xFFFFFFFF], dim=1).to(torch.int32)
    else:
        edges = torch.zeros((0, 2), dtype=torch.int32, device=t.device)
        saddle = torch.zeros(0, dtype=t.dtype, device=t.device)
    out = {"labels": labels.view(npix, npix), "minima": minima, "f_min": t.reshape(-1)[minima],
           "area": isums[0], "sum_x": isums[1], "sum_y": isums[2], "edge_pix": isums[3], "sum_f": sum_f,
           "edges": edges, "saddle": saddle}
    if not on_device:
        out = {k: to_numpy(v.contiguous()) for k, v in out.items()}
    return (out, passes.value) if return_passes else out


def _host(v):
    return to_numpy(v) if isinstance(v, torch.Tensor) else np.asarray(v)


def watershed_merge(basins, h):
    """Merge the basins of ``watershed_basins`` at height ``h`` >= 0 (persistence), on the host.  The edges are taken
    in ascending (saddle, a, b); with ra, rb the current roots of a and b, ra != rb, the two sets merge iff
    saddle - max(m_ra, m_rb) < h in float64, m_r being the lowest minimum of the root's set, and the root of the
    merged set is the one with the smaller (m, id).  h = 0 merges nothing, h = inf every connected pair.  Every final
    set is a void; voids are numbered in ascending id of their root basin.  Returns a dict of numpy arrays:
    ``void_of_basin`` (M,) int32, and per void ``root`` (basin id), ``area``, ``sum_x``, ``sum_y``, ``edge_pix`` (int64),
    ``sum_f`` (float64), ``kappa_min`` (the root's minimum, map dtype) and ``min_index`` (its flat pixel index)."""
    h = float(h)
    if not h >= 0.0:
        raise ValueError(f"the merge height must be >= 0, got {h}")
    f_min, minima = _host(basins["f_min"]), _host(basins["minima"])
    edges, saddle = _host(basins["edges"]).reshape(-1, 2), _host(basins["saddle"])
    m = len(f_min)
    depth = f_min.astype(np.float64)                # exact for float32
    parent = list(range(m))
    low = depth.tolist()                            # lowest minimum of each root's set; the root is where it sits

    def find(i):
        root = i
        while parent[root] != root:
            root = parent[root]
        while parent[i] != root:
            parent[i], i = root, parent[i]
        return root

    if h > 0.0 and len(edges):
        s64 = saddle.astype(np.float64)
        for e in np.lexsort((edges[:, 1], edges[:, 0], s64)):
            ra, rb = find(int(edges[e, 0])), find(int(edges[e, 1]))
            if ra == rb:
                continue
            if float(s64[e]) - max(low[ra], low[rb]) < h:
                keep, gone = (ra, rb) if (low[ra], ra) < (low[rb], rb) else (rb, ra)
                parent[gone] = keep
    root_of = np.array([find(i) for i in range(m)], dtype=np.int64)
    roots, void_of_basin = np.unique(root_of, return_inverse=True)
    out = {"void_of_basin": void_of_basin.astype(np.int32).reshape(-1), "root": roots}
    for k in WATERSHED_INT_SUMS:
        out[k] = _segment_sum_int(void_of_basin, _host(basins[k]), len(roots))
    out["sum_f"] = np.bincount(void_of_basin.reshape(-1), weights=_host(basins["sum_f"]), minlength=len(roots))
    out["kappa_min"] = f_min[roots]
    out["min_index"] = minima[roots].astype(np.int64)
    return out


def _segment_sum_int(index, values, nseg):
    out = np.zeros(nseg, dtype=np.int64)
    np.add.at(out, np.asarray(index).reshape(-1), np.asarray(values, dtype=np.int64))
    return out


def watershed_void_map(basins, void_of_basin):
    """The (npix, npix) int32 map of void ids: ``basins["labels"]`` through the basin -> void table of
    ``watershed_merge`` (``ast_watershed_relabel``).  Numpy labels give a numpy map, device labels a device map."""
    labels = basins["labels"]
    on_device = isinstance(labels, torch.Tensor)
    table = np.ascontiguousarray(_host(void_of_basin), dtype=np.int32).reshape(-1)
    if len(table) == 0:
        raise ValueError("void_of_basin is empty")
    lab = as_device(labels, torch.int32)
    if lab.dim() != 2 or lab.shape[0] != lab.shape[1]:
        raise ValueError(f"labels must be a square map, got shape {tuple(lab.shape)}")
    tab = as_device(table)
    out = torch.empty_like(lab)
    check(_lib.lib().ast_watershed_relabel(ptr(lab), ptr(tab), tab.numel(), lab.numel(), ptr(out), stream()),
          "ast_watershed_relabel")
    return out if on_device else to_numpy(out)


# ------------------------------------------------------------------ vector grids
def check_divergence_args(shape, dtype, spacing):
    """The argument checks of ``divergence``, host only: ``shape`` (n0, n1, n2, 3) with every side >= 3, ``dtype``
    float32 or float64 (torch or numpy), ``spacing`` a positive finite number.  Returns ``(shape, spacing)`` as ints and
    a float, or raises ValueError."""
    shape = tuple(int(s) for s in shape)
    if len(shape) != 4:
        raise ValueError(f"a vector grid (n0, n1, n2, 3) is expected, got {len(shape)}D")
    if shape[3] != 3:
        raise ValueError(f"the last axis must hold 3 components, got {shape[3]}")
    if min(shape[:3]) < 3:
        raise ValueError(f"every side must be at least 3 cells (second-order edges), got {shape[:3]}")
    try:
        name = str(dtype)[6:] if str(dtype).startswith("torch.") else np.dtype(dtype).name
    except TypeError:
        name = str(dtype)
    if name not in ("float32", "float64"):
        raise ValueError(f"dtype must be float32 or float64, got {dtype}")
    try:
        h = float(spacing)
    except (TypeError, ValueError):
        raise ValueError(f"spacing must be a number, got {spacing!r}") from None
    if not (h > 0.0 and np.isfinite(h)):
        raise ValueError(f"spacing must be positive and finite, got {spacing!r}")
    return shape, h


def divergence(v, spacing, periodic=False, out=None):
    """Finite-difference divergence of a vector grid ``(n0, n1, n2, 3)`` (MapTransform._compute_divergence,
    map_transform.py:92-104): ``np.gradient(v[..., a], spacing, axis=a, edge_order=2)`` summed over a = 0, 1, 2 in that
    order, bit for bit, as a device tensor ``(n0, n1, n2)`` of v's dtype.  ``periodic``: central differences with
    wrapped indices in every cell instead of numpy's one-sided edges.  ``v``: numpy array or tensor, float32 or float64.
    ASTRILD_DIVERGENCE_TILED=0 selects the one-work-item-per-cell kernel instead of the streaming one (same bits)."""
    shape, h = check_divergence_args(v.shape, v.dtype, spacing)
    t = as_device(v)
    if out is None:
        out = torch.empty(shape[:3], dtype=t.dtype, device=t.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == t.dtype and tuple(out.shape) == shape[:3]
    variant = 0 if os.environ.get("ASTRILD_DIVERGENCE_TILED", "1") == "0" else 1
    check(_lib.lib().ast_grid_divergence(ptr(t), ptr(out), real_code(t), shape[0], shape[1], shape[2], h,
                                         int(bool(periodic)), variant, stream()), "ast_grid_divergence")
    return out


def vector_magnitude(v, out=None):
    """``sqrt(sum(square(v), axis=-1))`` of a ``(..., 3)`` array (PowerSpectrum3D._get_vector_magnitude,
    power_spectrum_3d.py:155-162), the squares added left to right as numpy adds a last axis of length 3; a device
    tensor of v's dtype without the last axis."""
    if len(v.shape) < 1 or int(v.shape[-1]) != 3:
        raise ValueError(f"the last axis must hold 3 components, got shape {tuple(v.shape)}")
    t = as_device(v)
    code = real_code(t)
    if out is None:
        out = torch.empty(tuple(t.shape[:-1]), dtype=t.dtype, device=t.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == t.dtype and out.numel() * 3 == t.numel()
    check(_lib.lib().ast_vector_magnitude(ptr(t), ptr(out), code, out.numel(), stream()), "ast_vector_magnitude")
    return out


def spectral_divergence(cx, cy, cz, nmesh, boxsize, out=None):
    """``i (k0 cx + k1 cy + k2 cz)`` of three half spectra ``(n, n, n/2 + 1)`` in the layout of ``r2c``, with
    k_a = (2 pi / boxsize) m_a and m_a = 0 on the Nyquist planes.  ``out`` may be ``cx``."""
    n = int(nmesh)
    shape = (n, n, n // 2 + 1)
    code = _CPLX[cx.dtype]
    for c in (cx, cy, cz):
        assert c.is_cuda and c.is_contiguous() and c.dtype == cx.dtype and tuple(c.shape) == shape
    if out is None:
        out = torch.empty_like(cx)
    assert out.is_cuda and out.is_contiguous() and out.dtype == cx.dtype and tuple(out.shape) == shape
    check(_lib.lib().ast_spectral_divergence(ptr(cx), ptr(cy), ptr(cz), ptr(out), code, n, float(boxsize), stream()),
          "ast_spectral_divergence")
    return out


def velocity_divergence_power(v, boxsize, binning=None):
    """P_theta-theta(k) of a velocity grid ``(n, n, n, 3)``, theta = div v formed in Fourier space: each component is
    transformed (``r2c``), ``spectral_divergence`` combines the three spectra, and the shells are binned as in
    ``fftpower_1d``; the same dict and normalisation as ``fftpower_1d`` of the real-space theta grid, shotnoise 0.  A
    float32 ``v`` is widened to double, as ``fftpower_1d`` does off its fused path: an fp32 transform would leave the
    round-off of a component's O(1) mean on the low shells.

    The finite-difference theta of ``divergence`` put through ``fftpower_1d`` is not the same spectrum: a central
    difference of spacing h multiplies the term of axis a by sin(k_a h) / (k_a h), so its power falls below this one
    towards the Nyquist frequency.  The spectral derivative carries no such factor."""
    n = int(v.shape[0])
    if tuple(v.shape) != (n, n, n, 3) or n % 2 != 0:
        raise ValueError(f"a velocity grid (n, n, n, 3) with even n is expected, got shape {tuple(v.shape)}")
    t = as_device(v)
    real_code(t)
    spectra = [r2c(t[..., a].to(torch.float64).contiguous()) for a in range(3)]
    theta = spectral_divergence(*spectra, n, boxsize, out=spectra[0])
    return finish_power(*power_bin_1d(theta, None, n, boxsize, binning=binning))
