"""GPU: the bispectrum estimator's tail kernel by kernel - the fused z pass + triangle sums (ast_fft_tile_c2r_triangles) called
through its C entry, ast_triple_product_sums at its variant and LDS boundaries, and the small helpers of the triangle counts
(ast_shell_mask_real, ast_half_real_to_full, ast_shell_filter on sub-blocks) - against float64 references formed with plain
torch / numpy (tests/bispectrum_reference.py, checked on the CPU by tests/test_bispectrum_reference.py)."""
import ctypes as ct
import itertools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import bispectrum_reference as br

F32_PRODUCTS = 1.5e-7        # two fp32 product roundings of 2^-24 each per term, relative to sum |f_a f_b f_c|


@pytest.fixture(scope="module")
def dev(hip):
    from astrild_amd import device
    torch.cuda.set_device(0)
    return device


def _spectrum(dev, n, seed):
    """rfftn / Ng of randn + 0.3 randn^2 in fp32 (a field with a bispectrum), through the product's forward transform."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    f = torch.randn((n, n, n), dtype=torch.float32, device="cuda", generator=g)
    f.add_(0.3 * f * f)
    return dev.r2c(f)


def _poisoned(shape):
    w = torch.empty(shape, dtype=torch.complex64, device="cuda")
    torch.view_as_real(w).fill_(float("nan"))                 # both components
    return w


class _Case:
    """One spectrum and a list of shells: the work spectra after the masked x / y passes (what the fused kernel reads),
    and - formed once, per distinct unordered triple of shells - the float64 reference sums, their scale S and the error of
    an independent fp32 route (ast_shell_filter + rocFFT C2R fields, products and sums in float64)."""

    def __init__(self, dev, hip, spec, shells, chunk=1 << 24, lean=False, works=True):
        self.dev, self.hip, self.spec, self.shells, self.chunk, self.lean = dev, hip, spec, [tuple(s) for s in shells], chunk, lean
        self.n = n = spec.shape[0]
        self.pitch = dev.tile_work_pitch(n)
        self.keep = spec.clone() if n <= 512 else None
        self.works = []
        self._ref, self._roc, self._sums = None, None, {}
        if not works:                         # the references only (the caller has its sums from elsewhere)
            return
        from astrild_amd import _lib
        for lo, hi in self.shells:            # shell by shell into NaN: columns k_z >= m_hi stay uninitialised, as in production
            w = _poisoned((n, n, self.pitch))
            _lib.check(hip.ast_fft_tile_c2r_3d_batch(dev.ptr(spec), (ct.c_void_p * 1)(w.data_ptr()), (ct.c_void_p * 1)(None), 0, n,
                                                     (ct.c_int * 1)(lo), (ct.c_int * 1)(hi), 1, 1.0, 1, self.pitch, dev.stream()),
                       "ast_fft_tile_c2r_3d_batch")
            self.works.append(w)
        self.scratch = torch.empty(int(hip.ast_fft_tile_c2r_triangles_scratch_bytes()) // 8, dtype=torch.float64, device="cuda")

    def fused(self, tri, order=None, scale=1.0):
        """(return code, sums) of one ast_fft_tile_c2r_triangles call; slot i of the call is shell order[i]."""
        order = list(range(len(self.shells))) if order is None else list(order)
        k = len(order)
        wp = (ct.c_void_p * k)(*[self.works[s].data_ptr() for s in order])
        hi = (ct.c_int * k)(*[self.shells[s][1] for s in order])
        tri_d = torch.tensor(tri, dtype=torch.int32).reshape(-1, 3).cuda()
        out = torch.full((len(tri),), float("nan"), dtype=torch.float64, device="cuda")
        rc = self.hip.ast_fft_tile_c2r_triangles(wp, hi, k, 0, self.n, self.pitch, float(scale), self.dev.ptr(tri_d), len(tri),
                                                 self.dev.ptr(self.scratch), self.dev.ptr(out), self.dev.stream())
        return rc, out

    def run(self, tri, label, order=None):
        """One fused call with every assertion the cases share: accepted, a second call returns the same bits, the sums
        against the references (:meth:`check`), the spectrum left intact."""
        rc, out = self.fused(tri, order)
        assert rc == 0, label
        rc2, again = self.fused(tri, order)
        assert rc2 == 0 and torch.equal(out, again), label         # fixed summation order
        self.check(tri, out.cpu().numpy(), label, order)
        if self.keep is not None:
            assert torch.equal(self.spec, self.keep), label
        return out

    def free_works(self):
        self.works = None

    def sums(self, tri):
        """(ref, S, err_rocfft_route) per entry of ``tri`` (shell indices).  ``lean``: the float64 cubes are freed before the
        fp32 ones are built and neither is kept - ask for every triple in one call."""
        dev, n = self.dev, self.n
        tri = [tuple(t) for t in tri]
        new = sorted({tuple(sorted(t)) for t in tri} - set(self._sums))
        if new:
            if self._ref is None:
                m2 = br.m2_half(n, "cuda")
                fields = [br.shell_field(self.spec, lo, hi, m2) for lo, hi in self.shells]           # cube by cube
                del m2
            else:
                fields = self._ref
            ref, scale = br.triangle_sums(fields, new, self.chunk)
            if not self.lean:
                self._ref = fields
            del fields
            if self._roc is None:
                fields = [dev.c2r(dev.shell_filter(self.spec, n, lo, hi), (n, n, n)) for lo, hi in self.shells]
            else:
                fields = self._roc
            roc, _ = br.triangle_sums(fields, new, self.chunk)
            if not self.lean:
                self._roc = fields
            del fields
            for key, r, s, o in zip(new, ref, scale, roc):
                self._sums[key] = (r, s, abs(o - r))
        got = np.array([self._sums[tuple(sorted(t))] for t in tri])
        return got[:, 0], got[:, 1], got[:, 2]

    def check(self, tri, got, label, order=None):
        """The assertions every fused case makes; ``tri`` in slots of the call, ``got`` its sums as a numpy array.
        Returns the worst ratio of the error to the bound."""
        order = list(range(len(self.shells))) if order is None else list(order)
        named = [tuple(order[s] for s in t) for t in tri]
        ref, S, err_roc = self.sums(named)
        assert np.all(np.isfinite(got)), label                                         # nothing of the NaN poison was read
        err = np.abs(got - ref)
        # err_fused <= 3 err_rocfft_route + 1.5e-7 S: the floor is the two fp32 product roundings, the factor 3 covers the fp32
        # partial sums over one row part.  Measured on an MI355X, worst err / bound per case: 0.29 (256^3, the shell past the
        # Nyquist disc, where both fp32 routes are 1.5e-7 S and 1.7e-7 S off), 0.18 (512^3), 0.16 (the shell (0, 1) alone),
        # 0.09 (1024^3), 0.055 (256^3, 32 shells, any triangle count), 0.053 (device.bispectrum, 600 triangles); err / S is
        # 2e-9 .. 4e-8 otherwise, the rocFFT route's 1e-9 .. 3e-8.  The factor 3 holds with room everywhere.
        bound = 3.0 * err_roc + F32_PRODUCTS * S
        ratio = float((err / bound).max())
        print(f"[fused {label}] ntri {len(tri)}: worst err / (3 err_rocfft + 1.5e-7 S) = {ratio:.3g}, worst err / S = "
              f"{float((err / S).max()):.3g}, worst err_rocfft / S = {float((err_roc / S).max()):.3g}")
        assert np.all(err <= bound), (label, ratio)
        # the project's own criterion for B (test_bispectrum_fused_z_passes_and_triangle_sums)
        assert np.all(err <= 2e-4 * np.abs(ref) + 1e-5 * np.abs(ref).max()), label
        groups = {}
        for i, t in enumerate(named):
            groups.setdefault(tuple(sorted(t)), []).append(i)
        for idx in groups.values():                       # the same unordered triple in whatever order: the same sum
            assert np.ptp(got[idx]) <= bound[idx[0]], (label, named[idx[0]])
        return ratio


def _slots(tri):
    return {s for t in tri for s in t}


def _triangle_list(count, ns):
    """``count`` triangles over slots 0..ns-1, built from these blocks (thread t of a launch takes entry t % count):

    count >= 74    entries 0..63: isosceles, all three placements of the repeated slot in turn - the first wave takes the
                   pair path whole; where count < thread count the next wave wraps round and mixes them with scalene ones
    count >= 10    then the six orders of one scalene triple, the placements (a, b, b), (b, a, b), (b, b, a) with b the
                   LAST slot, one equilateral entry
                   then ceil(ns / 2) isosceles entries (2i, 2i+1, 2i+1), placements in turn, that walk through EVERY slot
                   then scalene / isosceles / equilateral entries in turn over the first 12 slots until the list is full
    count == 7     the six orders and the equilateral entry (no isosceles entry)
    count == 3     the three placements only
    count == 1     one scalene entry

    The list names every slot from 74 + ceil(ns / 2) entries on (10 + ceil(ns / 2) when count < 74); the callers that need
    that assert it with _slots()."""
    lim = min(ns, 12)
    pairs = [(a, b) for b in range(1, lim) for a in range(b)][:24]                    # a < b: (b, b, a) always closes
    combos = list(itertools.combinations(range(lim), 3))
    scalene = ([t for t in combos if t[2] <= t[0] + t[1] + 1 and t[0] > 0] or combos)[:12]
    orders = lambda t: [tuple(t[i] for i in p) for p in itertools.permutations(range(3))]
    places = lambda a, b: [(a, b, b), (b, a, b), (b, b, a)]
    eq = min(4, ns - 1)
    rep = (0 if ns < 4 else 2, ns - 1)
    if count == 1:
        return [scalene[0]]
    if count == 3:
        return places(*rep)
    if count == 7:
        return orders(scalene[0]) + [(eq, eq, eq)]
    assert count >= 10
    tri = []
    if count >= 74:
        tri += [places(*pairs[i % len(pairs)])[i % 3] for i in range(64)]
    tri += orders(scalene[0]) + places(*rep) + [(eq, eq, eq)]
    tri += [places(2 * i, (2 * i + 1) % ns)[i % 3] for i in range((ns + 1) // 2)]
    tri = tri[:count]
    j = 0
    while len(tri) < count:
        kind = j % 5
        if kind in (0, 2):
            tri.append(orders(scalene[(j // 5) % len(scalene)])[j % 6])
        elif kind in (1, 3):
            tri.append(places(*pairs[(j // 5) % len(pairs)])[j % 3])
        else:
            tri.append(((j // 5) % ns,) * 3)
        j += 1
    assert len(tri) == count
    return tri


# ------------------------------------------------------------------ 1. fused z pass + triangle sums, through the C entry
@pytest.fixture(scope="module")
def case256(dev, hip):
    """256^3, 32 shells of width 4 from m = 1 (exactly TRI_ROWS shells: every LDS row is a real shell)."""
    n = 256
    return _Case(dev, hip, _spectrum(dev, n, 256), [(1 + 4 * i, 5 + 4 * i) for i in range(32)])


@pytest.mark.parametrize("count", [1, 3, 7, 100, 257, 511, 512])
def test_fused_triangle_counts_with_32_shells(case256, count):
    """Thread (t, part) = (tid % ntri, tid / ntri) of 512: ntri = 1 (512 parts of 2 cells, the trailing ones empty), 3 and 7
    and 100 (idle threads, odd N / parts rounded up to even), 257 and 511 (one part, idle threads), 512 (no idle thread)."""
    c = case256
    tri = _triangle_list(count, 32)
    assert count < 100 or _slots(tri) == set(range(32))        # every LDS row enters a product
    c.run(tri, f"256/32 shells/{count}")


def test_fused_refuses_more_triangles_than_threads(case256):
    c = case256
    tri = _triangle_list(512, 32) + [(1, 2, 3)]
    rc, out = c.fused(tri)
    assert rc < 0 and torch.isnan(out).all()                   # refused before anything is launched
    assert c.fused(tri[:512])[0] == 0
    assert c.fused(tri[:3], order=list(range(32)) + [0])[0] < 0          # 33 shells


def test_fused_slots_pair_by_position_not_by_radius(case256):
    """works[i] / m_hi[i] in a shuffled order: every LDS row gets its own pruning radius, large shells before small ones."""
    c = case256
    order = [int(v) for v in np.random.default_rng(1).permutation(32)]
    assert order != sorted(order)
    tri = _triangle_list(100, 32)
    assert _slots(tri) == set(range(32))
    c.run(tri, "256/shuffled slots", order=order)
    # fewer slots than shells, in descending radius: rows past the last slot are zero rows
    order = [20, 9, 5, 2]
    tri = _triangle_list(12, 4)
    assert _slots(tri) == set(range(4))
    c.run(tri, "256/4 of 32 shells, descending", order=order)


@pytest.fixture(scope="module")
def edge256(dev, hip):
    n = 256
    return _Case(dev, hip, _spectrum(dev, n, 257), [(0, 1), (n // 2 - 4, n // 2 + 40), (1, 5), (100, 128)])


def test_fused_single_shell_zero_mode_only(edge256):
    """The shell (0, 1) alone: one slot, only column k_z = 0 of its work spectrum is written (and only its mode 0 is not
    zero); the field is the constant spec[0, 0, 0]."""
    c = edge256
    out = c.run([(0, 0, 0)], "256/shell (0,1) alone", order=[0])
    got = out.cpu().numpy()
    dc = float(c.spec[0, 0, 0].real)
    assert abs(got[0] - dc ** 3 * 256.0 ** 3) <= 1e-6 * abs(dc) ** 3 * 256.0 ** 3
    rc, half = c.fused([(0, 0, 0)], order=[0], scale=0.5)       # scale multiplies the fields: cubic in the sums, exactly
    assert rc == 0 and torch.equal(half * 8.0, out)


def test_fused_shell_past_the_nyquist_disc(edge256):
    """m_hi = n/2 + 40 >= n/2 + 1: kmax is clamped to the n/2 + 1 columns there are; the shell reaches into the corners."""
    c = edge256
    tri = [(1, 1, 1), (1, 1, 2), (2, 1, 1), (1, 2, 1), (3, 3, 1), (1, 3, 3), (3, 1, 2), (2, 3, 1), (1, 1, 0), (0, 1, 1), (3, 3, 3),
           (0, 0, 0), (0, 2, 2), (2, 2, 2), (2, 2, 3)]
    c.run(tri, "256/clamped kmax")


@pytest.fixture(scope="module")
def case512(dev, hip):
    return _Case(dev, hip, _spectrum(dev, 512, 512), [(1, 9), (9, 17), (100, 108), (250, 300)])


@pytest.mark.parametrize("count", [10, 300])
def test_fused_kernel_at_side_512(case512, count):
    """rows_c2r_triangles_kernel<16, 16>: 4 shells (28 zero rows); 10 triangles (51 parts of 22 cells, two idle threads) and
    300 (one part, 212 idle threads)."""
    c = case512
    tri = _triangle_list(count, 4)
    c.run(tri, f"512/4 shells/{count}")
    assert c.fused(_triangle_list(513, 4))[0] < 0


def test_fused_kernel_at_side_1024(dev, hip):
    """rows_c2r_triangles_kernel<16, 32>: 1024 threads, no register prefetch, up to 1024 triangles, 140 KB of LDS.  The fused
    sums first (three 4.4 GB work spectra), then the float64 reference cube by cube and the fp32 rocFFT-route cubes.
    The float64 inverse goes slab by slab (bispectrum_reference.inverse_in_slabs) and the float64 cubes are freed before the
    fp32 ones are built."""
    n = 1024
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()                       # (the smaller cases' module fixtures)
    c = _Case(dev, hip, _spectrum(dev, n, 1024), [(1, 9), (9, 17), (500, 540)], chunk=1 << 26, lean=True)
    lists = {10: _triangle_list(10, 3), 1024: _triangle_list(1024, 3)}
    got = {}
    for count, tri in lists.items():
        rc, out = c.fused(tri)
        assert rc == 0, count
        assert torch.equal(c.fused(tri)[1], out), count
        got[count] = out.cpu().numpy()
    assert c.fused(_triangle_list(1025, 3))[0] < 0
    c.free_works()
    c.sums(lists[10] + lists[1024])                            # every triple at once: the cubes are built once and freed
    # Peak device memory (torch.cuda.max_memory_allocated) on an MI355X: 38.8 GiB, while the third float64 cube is built
    # (two finished 8 GiB cubes, the complex128 copy of the spectrum, the new cube, the 4 GiB spectrum and the 2 GiB |m|^2
    # lattice); the kernels under test hold 17.5 GiB (the spectrum and three work spectra).
    for count, tri in lists.items():
        c.check(tri, got[count], f"1024/3 shells/{count}")
    peak = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 30
    print(f"[fused 1024] peak device memory of this test {peak:.1f} GiB (on top of {base / 2.0 ** 30:.1f} GiB held by the module's fixtures)")
    del c
    torch.cuda.empty_cache()


def test_bispectrum_batches_of_512_triangles(dev, hip):
    """device.bispectrum with 600 triangles over 8 shells at 256^3: the second call of the fused kernel starts at
    tri_d[512:] / out[512:].  B ntri n^3 / L^6 is the plain sum over cells of f_a f_b f_c."""
    n, L = 256, 500.0
    g = torch.Generator(device="cuda").manual_seed(600)
    f = torch.randn((n, n, n), dtype=torch.float32, device="cuda", generator=g)
    f.add_(0.3 * f * f)
    edges = [1 + 8 * i for i in range(9)]
    closed = [t for t in itertools.combinations_with_replacement(range(8), 3) if t[2] <= t[0] + t[1]]
    tri = [tuple(closed[i % len(closed)][j] for j in list(itertools.permutations(range(3)))[i % 6]) for i in range(600)]
    tri[512:600] = tri[100:188]                                # entries of the second batch that name triples of the first
    dev._tri_cache.clear()
    res = dev.bispectrum(f, L, edges, tri)
    dev._tri_cache.clear()
    assert np.all(res["ntri"] > 0)
    got = res["B"] * res["ntri"] * float(n) ** 3 / L ** 6
    c = _Case(dev, hip, dev.r2c(f), list(zip(edges[:-1], edges[1:])), works=False)
    c.check(tri, got, "device.bispectrum 600 triangles")
    ref, S, err_roc = c.sums(tri)
    for i in range(512, 600):
        assert tuple(sorted(tri[i])) == tuple(sorted(tri[i - 412]))
        assert abs(got[i] - got[i - 412]) <= 3.0 * err_roc[i] + F32_PRODUCTS * S[i]


# ------------------------------------------------------------------ 3. ast_triple_product_sums at its boundaries
BIG = 3 * 1024 * 256 + 77          # 3073 chunks of 256 cells: 1024 resident workgroups at 32 fields, three chunks each (one four)


@pytest.fixture(scope="module")
def host_fields():
    rng = np.random.default_rng(33)
    return rng.standard_normal((33, BIG)).astype(np.float32)


def _products(host, tri):
    """float64 numpy: (sum, sum of magnitudes) per triangle, once per distinct unordered triple."""
    done = {}
    for key in {tuple(sorted(t)) for t in tri}:
        p = host[key[0]].astype(np.float64) * host[key[1]].astype(np.float64) * host[key[2]].astype(np.float64)
        done[key] = (p.sum(), np.abs(p).sum())
    v = np.array([done[tuple(sorted(t))] for t in tri])
    return v[:, 0], v[:, 1]


@pytest.fixture(scope="module")
def device_fields(dev, host_fields):
    return [dev.as_device(h) for h in host_fields]            # 33 fields of BIG cells; a shorter count reads their heads


def _sums_of_all_fields(dev, hip, fields, nf, count, tri):
    """ast_triple_product_sums itself with ALL of the first nf fields (device.triple_product_sums would pass only the
    fields the triangles name): nfields = nf decides the kernel variant and the LDS layout."""
    ptrs = torch.tensor([f.data_ptr() for f in fields[:nf]], dtype=torch.int64).cuda()
    assert ptrs.numel() == nf and all(f.numel() >= count for f in fields[:nf])
    tri_d = torch.tensor(tri, dtype=torch.int32).reshape(-1, 3).cuda()
    assert int(tri_d.min()) >= 0 and int(tri_d.max()) < nf
    scratch = torch.empty(hip.ast_triple_product_sums_scratch_bytes() // 8, dtype=torch.float64, device="cuda")
    out = torch.full((len(tri),), float("nan"), dtype=torch.float64, device="cuda")
    from astrild_amd import _lib
    _lib.check(hip.ast_triple_product_sums(dev.ptr(ptrs), nf, 0, count, dev.ptr(tri_d), len(tri), dev.ptr(scratch), dev.ptr(out),
                                           dev.stream()), "ast_triple_product_sums")
    return out


@pytest.mark.parametrize("count,ntri", [(1, 1), (255, 3), (256, 100), (257, 129), (BIG, 256), (257, 256), (BIG, 3), (BIG, 100)])
@pytest.mark.parametrize("nf", [16, 17, 32, 33])
def test_triple_product_sums_at_the_pipelined_variant_s_boundaries(dev, hip, host_fields, device_fields, nf, count, ntri):
    """fp32, nfields = nf in every case (the C entry is called with all nf pointers): 16 and 33 take the plain kernel, 17 and
    32 the pipelined one (the next chunk's loads in flight across the product loop).  Counts below one chunk (1, 255), one
    chunk exactly, one cell more, and 3073 chunks - three or four per workgroup at 32 fields, a fetch in flight; 1, 3, 100,
    129 and 256 triangles in one launch (256, 85, 2, 1, 1 parts).  The triangles reach the last field.  The two variants
    form the same products and add them in the same order: AST_TRI_NO_PIPE=1 changes no bit."""
    assert "AST_TRI_NO_PIPE" not in os.environ
    if ntri == 1:
        tri = [(nf - 1, 0, nf // 2)]
    else:
        tri = _triangle_list(ntri, nf)
        assert nf - 1 in _slots(tri) and (ntri < 100 or _slots(tri) == set(range(nf)))
    got = _sums_of_all_fields(dev, hip, device_fields, nf, count, tri)
    assert torch.equal(got, _sums_of_all_fields(dev, hip, device_fields, nf, count, tri))
    ref, scale = _products(host_fields[:nf, :count], tri)
    err = np.abs(got.cpu().numpy() - ref)
    print(f"[triple sums] nf {nf} count {count} ntri {ntri}: worst err / scale = {float((err / scale).max()):.3g}")
    assert np.all(err <= F32_PRODUCTS * scale)
    if nf in (17, 32):
        os.environ["AST_TRI_NO_PIPE"] = "1"
        try:
            plain = _sums_of_all_fields(dev, hip, device_fields, nf, count, tri)
        finally:
            del os.environ["AST_TRI_NO_PIPE"]
        assert torch.equal(plain, got)
    if ntri >= 100:                  # the Python wrapper passes the fields the list names - here all nf: the same launch
        fields = {s: device_fields[s][:count] for s in range(nf)}
        assert torch.equal(dev.triple_product_sums(fields, tri), got)


def test_triple_product_sums_more_triangles_than_one_launch(dev, host_fields, device_fields):
    """300 > 256 triangles through device.triple_product_sums: two launches, each with its own field numbering; both batches
    name all 17 fields (the pipelined kernel twice), the second through a shuffled subset of keys."""
    nf, count = 17, 2 * 256 + 9
    fields = {s: device_fields[s][:count] for s in range(nf)}
    tri = _triangle_list(256, nf) + [(s, (s + 1) % nf, (s + 5) % nf) for s in range(nf)] * 2 + [(16, 15, 14)] * 10
    assert len(tri) == 300 and _slots(tri[:256]) == _slots(tri[256:]) == set(range(nf))
    got = dev.triple_product_sums(fields, tri).cpu().numpy()
    ref, scale = _products(host_fields[:nf, :count], tri)
    assert np.all(np.abs(got - ref) <= F32_PRODUCTS * scale)
    assert np.all(got[290:] == got[290])


@pytest.mark.parametrize("dtype,nf,kernel", [(torch.float32, 159, True), (torch.float64, 79, True),
                                             (torch.float32, 160, False), (torch.float64, 80, False)])
def test_triple_product_sums_largest_lds_request_and_fallback(dev, hip, dtype, nf, kernel):
    """nf * 257 * sizeof(T) <= 160 KB: 159 fp32 / 79 fp64 fields are the most one LDS chunk holds (163 452 and 162 424 bytes);
    one field more and device.triple_product_sums falls back to one ast_triple_product_sum per triangle (the C entry refuses)."""
    count = 4 * 256 + 5
    rng = np.random.default_rng(nf)
    host = rng.standard_normal((nf, count)).astype(np.float32 if dtype == torch.float32 else np.float64)
    fields = {s: dev.as_device(host[s]) for s in range(nf)}
    tri = [(nf - 1, nf - 1, nf - 1), (0, nf - 1, nf // 2), (nf - 1, 0, 0), (nf - 2, nf - 1, nf - 2)]
    tri += [(s, (s * 7 + 3) % nf, (s * 13 + 5) % nf) for s in range(nf)]                 # every field is used
    assert {s for t in tri for s in t} == set(range(nf))
    esz = 4 if dtype == torch.float32 else 8
    assert (nf * 257 * esz <= 160 * 1024) == kernel
    ptrs = torch.tensor([fields[s].data_ptr() for s in range(nf)], dtype=torch.int64).cuda()
    tri_d = torch.tensor(tri, dtype=torch.int32).cuda()
    scratch = torch.empty(hip.ast_triple_product_sums_scratch_bytes() // 8, dtype=torch.float64, device="cuda")
    direct = torch.zeros(len(tri), dtype=torch.float64, device="cuda")
    rc = hip.ast_triple_product_sums(dev.ptr(ptrs), nf, 0 if dtype == torch.float32 else 1, count, dev.ptr(tri_d), len(tri),
                                     dev.ptr(scratch), dev.ptr(direct), dev.stream())
    assert (rc == 0) == kernel
    got = dev.triple_product_sums(fields, tri)
    if kernel:
        assert torch.equal(got, direct)
    ref, scale = _products(host, tri)
    tol = F32_PRODUCTS if dtype == torch.float32 else 1e-13
    assert np.all(np.abs(got.cpu().numpy() - ref) <= tol * scale)


# ------------------------------------------------------------------ 4. the helpers of the triangle counts
def _freq(n):
    m = np.arange(n)
    m[m > n // 2] -= n
    return m


def _m2_full(n):
    m = _freq(n)
    return m[:, None, None] ** 2 + m[None, :, None] ** 2 + m[None, None, :] ** 2


def _shells_small(n):
    # (0, 1); edges on exact integer norms (|m| = 2, 3, 5 exist on the lattice: (2,0,0), (1,2,2), (3,4,0)); past the Nyquist disc
    return [(0, 1), (1, 2), (2, 3), (3, 5), (5, 6), (1, n // 2), (n // 2, n // 2 + 1), (n // 2, n)]


@pytest.mark.parametrize("n", [8, 16])
def test_shell_mask_real_is_the_integer_norm_test(dev, hip, n):
    m2 = _m2_full(n)
    for lo, hi in _shells_small(n):
        out = torch.full((n, n, n), float("nan"), dtype=torch.float64, device="cuda")
        assert hip.ast_shell_mask_real(dev.ptr(out), n, lo, hi, dev.stream()) == 0
        want = ((m2 >= lo * lo) & (m2 < hi * hi)).astype(np.float64)
        assert np.array_equal(out.cpu().numpy(), want), (lo, hi)
    assert hip.ast_shell_mask_real(dev.ptr(out), n, 3, 3, dev.stream()) < 0


def _unfold(half, n):
    """Re of the full-lattice spectrum from the half one: X(k) = conj X(-k) for k_z > n/2, index 0 its own mirror image."""
    full = np.empty((n, n, n))
    nz = n // 2 + 1
    full[:, :, :nz] = half.real
    ix = (n - np.arange(n)) % n
    for z in range(nz, n):
        full[:, :, z] = half.real[ix][:, ix][:, :, n - z]
    return full


@pytest.mark.parametrize("n", [8, 16])
def test_half_real_to_full_reflects_every_index(dev, hip, n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, n, n))
    half = np.fft.rfftn(x)
    out = torch.full((n, n, n), float("nan"), dtype=torch.float64, device="cuda")
    spec = dev.as_device(half)
    assert spec.dtype == torch.complex128
    assert hip.ast_half_real_to_full(dev.ptr(spec), dev.ptr(out), n, dev.stream()) == 0
    got = out.cpu().numpy()
    assert np.array_equal(got, _unfold(half, n))                 # a copy: exact
    full = np.fft.fftn(x).real
    assert np.abs(got - full).max() <= 1e-13 * np.abs(full).max()
    assert np.abs(_unfold(half, n) - full).max() <= 1e-13 * np.abs(full).max()


@pytest.mark.parametrize("n", [8, 16, 128])
def test_triangle_count_chain_mask_forward_transform_unfold(dev, hip, n):
    """What device.bispectrum runs for I_s(x) where ast_fft64_supported: mask -> ast_fft64_r2c_3d -> ast_half_real_to_full,
    against np.fft.fftn(mask).real to 1e-9 of the shell's mode count (= I_s(0)).  Below 128 the forward transform is not
    the hand-written one: numpy's takes its place and the two helpers are checked alone."""
    from astrild_amd import _lib
    m2 = _m2_full(n)
    own = bool(hip.ast_fft64_supported(n))
    assert own == (n >= 128)
    for lo, hi in ([(0, 1), (1, 9), (60, 70), (63, 65)] if n == 128 else _shells_small(n)):
        mask = torch.empty((n, n, n), dtype=torch.float64, device="cuda")
        _lib.check(hip.ast_shell_mask_real(dev.ptr(mask), n, lo, hi, dev.stream()))
        want_mask = ((m2 >= lo * lo) & (m2 < hi * hi)).astype(np.float64)
        host_mask = mask.cpu().numpy()
        assert np.array_equal(host_mask, want_mask)
        count = want_mask.sum()
        if own:
            half = torch.empty((n, n, n // 2 + 1), dtype=torch.complex128, device="cuda")
            _lib.check(hip.ast_fft64_r2c_3d(dev.ptr(mask), dev.ptr(half), n, 1.0, dev.stream()))
        else:
            half = dev.as_device(np.fft.rfftn(host_mask))
        full = torch.full((n, n, n), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(hip.ast_half_real_to_full(dev.ptr(half), dev.ptr(full), n, dev.stream()))
        got = full.cpu().numpy()
        want = np.fft.fftn(want_mask).real
        assert np.abs(got - want).max() <= 1e-9 * count, (lo, hi)
        assert abs(got[0, 0, 0] - count) <= 1e-9 * count


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
@pytest.mark.parametrize("n", [8, 16])
def test_shell_filter_on_sub_blocks(dev, hip, n, dtype):
    """ast_shell_filter with an (i0, i1) sub-block (what the slab code passes: the block's own rows in, the same rows out)
    equals the masked slice of the whole lattice, bit for bit; in = NULL writes the bare indicator; a block that ends on the
    last plane; an empty block touches nothing."""
    rng = np.random.default_rng(n)
    nz = n // 2 + 1
    host = (rng.standard_normal((n, n, nz)) + 1j * rng.standard_normal((n, n, nz))).astype(
        np.complex64 if dtype == torch.complex64 else np.complex128)
    m = _freq(n)
    m2 = m[:, None, None] ** 2 + m[None, :, None] ** 2 + np.arange(nz)[None, None, :] ** 2
    blocks = [((0, n), (0, n)), ((0, 3), (0, n)), ((n - 3, 3), (0, n)), ((2, 5), (n - 2, 2)), ((n // 2, 1), (n // 2, 1)),
              ((n - 1, 1), (n - 1, 1)), ((1, n - 1), (3, n - 4))]
    for lo, hi in _shells_small(n):
        inside = (m2 >= lo * lo) & (m2 < hi * hi)
        for (s0, c0), (s1, c1) in blocks:
            sl = (slice(s0, s0 + c0), slice(s1, s1 + c1))
            block = dev.as_device(np.ascontiguousarray(host[sl]))
            got = dev.shell_filter(block, n, lo, hi, i0=(s0, c0), i1=(s1, c1))
            assert got.dtype == dtype and tuple(got.shape) == (c0, c1, nz)
            assert np.array_equal(got.cpu().numpy(), host[sl] * inside[sl]), (lo, hi, s0, c0, s1, c1)
            ind = dev.shell_filter(None, n, lo, hi, i0=(s0, c0), i1=(s1, c1), dtype=dtype)
            assert np.array_equal(ind.cpu().numpy(), inside[sl].astype(host.dtype)), (lo, hi, s0, c0, s1, c1)
    # an empty block: accepted, nothing written
    guard = torch.full((4, nz), 7.0, dtype=dtype, device="cuda")
    code = 0 if dtype == torch.complex64 else 1
    for (s0, c0), (s1, c1) in [((n, 0), (0, n)), ((3, 0), (0, n)), ((0, n), (n, 0)), ((n - 1, 1), (5, 0))]:
        assert hip.ast_shell_filter(None, dev.ptr(guard), code, n, 1, 3, s0, c0, s1, c1, dev.stream()) == 0
    assert bool((guard == 7.0).all())
    assert hip.ast_shell_filter(None, dev.ptr(guard), code, n, 1, 3, n - 1, 2, 0, 1, dev.stream()) < 0        # past the last plane
