// What the hand-written three-stage transforms share: lens_fft.hip (rows of the padded lens convolution) and cube_fft.hip
// (3-D transforms of float64 and of side-2048 fp32 grids).  Register FFTs in double2 or float2, the three-stage scheme
// over one padded LDS line, the table points -> radices, the forward row kernel (zero-padded lens rows; the z rows of a
// cube are its ZPAD = false instantiation) and the float64 twiddle cache.  Everything is in the anonymous namespace:
// each of the two translation units has its own twiddle cache (they ask for almost disjoint lengths).
#pragma once
#include "../../include/astrild_hip.h"
#include "ast_common.h"
#include "fft_roots.h"
#include "paint_tile_geom.h"
#include <cmath>
#include <mutex>
#include <type_traits>
#include <vector>

#define LENS_FWD(call)                 \
    do {                               \
        int rc_ = (call);              \
        if (rc_ != AST_OK) return rc_; \
    } while (0)

namespace {

__device__ inline double2 cmul(double2 a, double2 w) {
    return make_double2(fma(a.x, w.x, -a.y * w.y), fma(a.x, w.y, a.y * w.x));
}
__device__ inline float2 cmul(float2 a, float2 w) {
    return make_float2(fmaf(a.x, w.x, -a.y * w.y), fmaf(a.x, w.y, a.y * w.x));
}
template <typename V> struct ScalarOf;
template <> struct ScalarOf<double2> { typedef double type; };
template <> struct ScalarOf<float2> { typedef float type; };

// forward FFT of R <= 32 points in registers, decimation in frequency: X[k] ends up in v[bitrev(k)]
// (V = double2, or float2 for the single-precision passes of cubes of side 2048 in cube_fft.hip)
template <int R, typename V>
__device__ inline void fft_reg(V (&v)[R]) {
    typedef typename ScalarOf<V>::type S;
#pragma unroll
    for (int h = R / 2; h >= 1; h /= 2) {
#pragma unroll
        for (int blk = 0; blk < R; blk += 2 * h) {
#pragma unroll
            for (int j = 0; j < h; ++j) {
                const V a = v[blk + j], b = v[blk + j + h];
                v[blk + j] = V(a.x + b.x, a.y + b.y);
                const V d = V(a.x - b.x, a.y - b.y);
                const int t = j * (16 / h);                  // W_{2h}^j = W_32^{j * 32 / (2h)}, t < 16
                if (t == 0) v[blk + j + h] = d;
                else if (t == 8) v[blk + j + h] = V(d.y, -d.x);          // * (-i)
                else if (t % 2 == 0) v[blk + j + h] = cmul(d, V((S)kC16[t / 2], (S)kS16[t / 2]));
                else v[blk + j + h] = cmul(d, V((S)kC32o[t / 2], (S)kS32o[t / 2]));
            }
        }
    }
}

// e^{-2 pi i m / len}, m < len, per (device, len)
__global__ void tw_table_kernel(double2* out, int len) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    double sn, cs;
    sincospi(-2.0 * (double)i / (double)len, &sn, &cs);
    out[i] = make_double2(cs, sn);
}
struct TwCache {
    std::mutex m;
    struct E { int dev, len; double2* d; };
    std::vector<E> tabs;
    const double2* get(int len, hipStream_t s) {
        std::lock_guard<std::mutex> lock(m);
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return nullptr;
        for (auto& t : tabs) if (t.dev == dev && t.len == len) return t.d;
        double2* d = nullptr;
        if (hipMalloc(&d, (size_t)len * sizeof(double2)) != hipSuccess) return nullptr;
        tw_table_kernel<<<(len + 255) / 256, 256, 0, s>>>(d, len);
        // once per (device, length): the table must be complete before ANY stream reads it (the pointer is handed
        // to later callers without an event)
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { (void)hipFree(d); return nullptr; }
        tabs.push_back({dev, len, d});
        return d;
    }
} g_tw;
// the translation unit's table of length `len` (nullptr: the allocation or the fill failed)
inline const double2* twiddles64(int len, hipStream_t s) { return g_tw.get(len, s); }

// ------------------------------------------------------------------ the three-stage scheme
// M = RA RB RC points go through three register FFTs with two exchanges through one LDS line (M + M / 8 elements: 74 KB
// of double2 at M = 4096, two workgroups per CU):
//   j = RB RC a + RC b + c,  k = alpha + RA beta + RA RB gamma
//   stage 1 (thread j' = RC b + c):  y[alpha][j'] = W_M^{j' alpha} sum_a z[RB RC a + j'] W_RA^{a alpha}
//   stage 2 (thread (alpha, c)):     y'[alpha][beta][c] = W_{RB RC}^{c beta} sum_b y[alpha][RC b + c] W_RB^{b beta}
//   stage 3 (thread (alpha, beta)):  Z[alpha + RA beta + RA RB gamma] = sum_c y'[alpha][beta][c] W_RC^{c gamma}
__device__ inline int lds_pad(int i) { return i + (i >> 3); }

template <int RA, int RB, int RC>
struct RowGeo {
    static constexpr int M = RA * RB * RC;
    static constexpr int T1 = RB * RC, T2 = RA * RC, T3 = RA * RB;
    static constexpr int NT = T1 > T2 ? (T1 > T3 ? T1 : T3) : (T2 > T3 ? T2 : T3);
    static constexpr int RMAX = RA > RB ? (RA > RC ? RA : RC) : (RB > RC ? RB : RC);
};

// THE table points -> (RA, RB, RC): f(integral_constant<int, RA>{}, <RB>{}, <RC>{}) for the transform of `points` points,
// AST_ERR_ARG for any other length.  SIZES: the sum of the lengths (powers of two, 64 ... 8192) the caller accepts - f is
// instantiated for those only, so a caller gets the kernels of the sizes its *_supported function names and no others.
template <int V> using RadixOf = std::integral_constant<int, V>;
template <unsigned SIZES, typename F>
int with_radices(size_t points, F&& f) {
    static_assert(SIZES != 0 && (SIZES & ~(unsigned)(2 * 8192 - 64)) == 0, "lengths 64 ... 8192");
    if constexpr ((SIZES & 8192) != 0) if (points == 8192) return f(RadixOf<32>{}, RadixOf<16>{}, RadixOf<16>{});
    if constexpr ((SIZES & 4096) != 0) if (points == 4096) return f(RadixOf<16>{}, RadixOf<16>{}, RadixOf<16>{});
    if constexpr ((SIZES & 2048) != 0) if (points == 2048) return f(RadixOf<16>{}, RadixOf<16>{}, RadixOf<8>{});
    if constexpr ((SIZES & 1024) != 0) if (points == 1024) return f(RadixOf<16>{}, RadixOf<8>{}, RadixOf<8>{});
    if constexpr ((SIZES & 512) != 0) if (points == 512) return f(RadixOf<8>{}, RadixOf<8>{}, RadixOf<8>{});
    if constexpr ((SIZES & 256) != 0) if (points == 256) return f(RadixOf<8>{}, RadixOf<8>{}, RadixOf<4>{});
    if constexpr ((SIZES & 128) != 0) if (points == 128) return f(RadixOf<8>{}, RadixOf<4>{}, RadixOf<4>{});
    if constexpr ((SIZES & 64) != 0) if (points == 64) return f(RadixOf<4>{}, RadixOf<4>{}, RadixOf<4>{});
    return AST_ERR_ARG;
}
constexpr unsigned radix_sizes(unsigned lo, unsigned hi) { return (2 * hi - 1) & ~(lo - 1); }      // lo, 2 lo, ..., hi

// On entry (threads t < T1): va[a] = input[RB RC a + t].  On exit (threads t < T3, t = alpha * RB + beta): vc[bitrev(gamma)] =
// output[alpha + RA beta + RA RB gamma].
template <int RA, int RB, int RC, typename V>
__device__ inline void three_stage(V (&va)[RA], V (&vc)[RC], V* Y, const V* __restrict__ twM, int t) {
    using G = RowGeo<RA, RB, RC>;
    if (t < G::T1) {
        fft_reg<RA>(va);
#pragma unroll
        for (int al = 0; al < RA; ++al) {
            V y = va[bitrev(al, ilog2(RA))];
            if (al != 0) y = cmul(y, twM[t * al]);
            Y[lds_pad(al * G::T1 + t)] = y;
        }
    }
    __syncthreads();
    if (t < G::T2) {
        const int al = t / RC, c = t % RC;
        V vb[RB];
#pragma unroll
        for (int b = 0; b < RB; ++b) vb[b] = Y[lds_pad(al * G::T1 + RC * b + c)];
        fft_reg<RB>(vb);
        // the slots this thread read are the slots it writes: no barrier in between
#pragma unroll
        for (int be = 0; be < RB; ++be) {
            V y = vb[bitrev(be, ilog2(RB))];
            if (be != 0 && c != 0) y = cmul(y, twM[RA * c * be]);
            Y[lds_pad(al * G::T1 + RC * be + c)] = y;
        }
    }
    __syncthreads();
    if (t < G::T3) {
#pragma unroll
        for (int c = 0; c < RC; ++c) vc[c] = Y[lds_pad(t * RC + c)];      // t = alpha * RB + beta: RC consecutive (padded) slots
        fft_reg<RC>(vc);
    }
}

// ------------------------------------------------------------------ real rows -> half spectrum, one row per workgroup
// The real-to-complex transform of 2 M reals is the M-point complex transform of z[j] = x[2j] + i x[2j+1] followed by the
// even/odd split.
// ZPAD: the row holds M reals followed by M zeros that are not in memory (the lens plan: z[j] = 0 for j >= M / 2, so stage 1
// loads a < RA / 2 only); otherwise 2 M reals (the rows of a 3-D grid: the z pass of the double-precision power spectrum).
// in_pitch: reals between rows; the spectrum is multiplied by `scale`.
// FOLDW = 2 / 3 (CIC / TSC, grids only): the grid is what a deferred-fold paint left and `rec` its halo records; the up to
// three record lines that end in a border row are added as the row is loaded - records first, then onto the row, the
// order of the paint's own fold kernel (as in fft_tile.hip's float row pass).
// TIN = float: the rows are read from a single-precision grid and widened on load (the double transform of an fp32 grid
// without a 2x copy of it: cubes the fp32 tile passes do not cover - 128^3, 2048^3; no FOLDW).
template <typename TIN> struct PairOf { typedef double2 type; };
template <> struct PairOf<float> { typedef float2 type; };
__device__ inline double2 widen(double2 v) { return v; }
__device__ inline double2 widen(float2 v) { return make_double2((double)v.x, (double)v.y); }

template <int RA, int RB, int RC, bool ZPAD, int FOLDW = 0, typename TIN = double>
__global__ void __launch_bounds__((RowGeo<RA, RB, RC>::NT))
lens_rows_forward_kernel(const TIN* __restrict__ kappa, size_t in_pitch, double2* __restrict__ spec, size_t pitch,
                         const double2* __restrict__ twM, const double2* __restrict__ twL, double scale,
                         const double* __restrict__ rec = nullptr) {
    using G = RowGeo<RA, RB, RC>;
    constexpr int M = G::M;
    static_assert(FOLDW == 0 || sizeof(TIN) == 8, "halo records are folded in the grid's own precision: double rows only");
    extern __shared__ double2 Y[];
    const int t = threadIdx.x;
    const size_t row = blockIdx.x;
    const typename PairOf<TIN>::type* z = reinterpret_cast<const typename PairOf<TIN>::type*>(kappa + row * in_pitch);        // packed pairs: M / 2 (ZPAD) or M
    double2 va[RA], vc[RC];
    // the halo sources of this row first (integer work, the same for the whole workgroup: one row per workgroup), so
    // that the row's loads and the records' loads are all in flight together
    const double* src[3] = {nullptr, nullptr, nullptr};
    int ns = 0;
    if (FOLDW != 0) {
        constexpr int W = FOLDW != 0 ? FOLDW : 2;
        const int ng = 2 * M;
        ns = ast::halo_sources<double, W>(rec, (int)(row / ng), (int)(row % ng), ng, ng / ast::TX, ng / ast::TY, src);
    }
    if (t < G::T1) {
#pragma unroll
        for (int a = 0; a < RA; ++a) va[a] = (!ZPAD || a < RA / 2) ? widen(z[G::T1 * a + t]) : make_double2(0.0, 0.0);
        if (FOLDW != 0 && ns > 0) {
            double2 h0[RA], h1[RA], h2[RA];
#pragma unroll
            for (int a = 0; a < RA; ++a) h0[a] = reinterpret_cast<const double2*>(src[0])[G::T1 * a + t];
            if (ns > 1) {
#pragma unroll
                for (int a = 0; a < RA; ++a) h1[a] = reinterpret_cast<const double2*>(src[1])[G::T1 * a + t];
            }
            if (ns > 2) {
#pragma unroll
                for (int a = 0; a < RA; ++a) h2[a] = reinterpret_cast<const double2*>(src[2])[G::T1 * a + t];
            }
            // records first, then onto the row: the fold kernel's order
#pragma unroll
            for (int a = 0; a < RA; ++a) {
                double2 h = h0[a];
                if (ns > 1) { h.x += h1[a].x; h.y += h1[a].y; }
                if (ns > 2) { h.x += h2[a].x; h.y += h2[a].y; }
                va[a].x += h.x;
                va[a].y += h.y;
            }
        }
    }
    three_stage<RA, RB, RC>(va, vc, Y, twM, t);
    // the untangling twiddles of this thread's outputs, in flight across the exchange below
    constexpr int IT = (M / 2) / G::NT;
    static_assert(IT * G::NT == M / 2, "row length and thread count");
    double2 wk[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) wk[it] = twL[t + it * G::NT];
    __syncthreads();                                      // everyone has read its stage-3 inputs: Y becomes Z[k]
    if (t < G::T3) {
#pragma unroll
        for (int ga = 0; ga < RC; ++ga) Y[lds_pad((t / RB) + RA * (t % RB) + RA * RB * ga)] = vc[bitrev(ga, ilog2(RC))];
    }
    __syncthreads();
    double2* orow = spec + row * pitch;
    auto emit = [&](int k, double2 w) {
        const double2 zk = Y[lds_pad(k)];
        const double2 zm = Y[lds_pad(M - k)];
        const double2 e = make_double2(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));      // (Zk + conj Zm) / 2
        const double2 o = make_double2(0.5 * (zk.x - zm.x), 0.5 * (zk.y + zm.y));      // (Zk - conj Zm) / 2
        const double2 tt = cmul(o, w);                                                  // w^k o, w = e^{-2 pi i / L}
        orow[k] = make_double2((e.x + tt.y) * scale, (e.y - tt.x) * scale);             // e - i t
        orow[M - k] = make_double2((e.x - tt.y) * scale, (-e.y - tt.x) * scale);        // conj(e + i t)
    };
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int k = t + it * G::NT;
        if (k == 0) {
            const double2 zk = Y[lds_pad(0)];
            orow[0] = make_double2((zk.x + zk.y) * scale, 0.0);
            orow[M] = make_double2((zk.x - zk.y) * scale, 0.0);
        } else {
            emit(k, wk[it]);
        }
    }
    if (t == 0) emit(M / 2, twL[M / 2]);
}

template <int RA, int RB, int RC, bool ZPAD = true, int FOLDW = 0, typename TIN = double>
int rows_forward_launch(const TIN* kappa, size_t nrows, double2* spec, size_t pitch, const double2* twM, const double2* twL, hipStream_t s,
                        size_t in_pitch = 0, double scale = 1.0, const double* rec = nullptr) {
    using G = RowGeo<RA, RB, RC>;
    const size_t lds = (size_t)(G::M + G::M / 8) * sizeof(double2);
    static ast::PerDeviceOnce once;
    if (once.need() && lds > 48 * 1024) {
        AST_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&lens_rows_forward_kernel<RA, RB, RC, ZPAD, FOLDW, TIN>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        once.mark();
    }
    AST_CHECK_ARG(nrows < 0x7fffffffull);
    lens_rows_forward_kernel<RA, RB, RC, ZPAD, FOLDW, TIN><<<(unsigned)nrows, G::NT, lds, s>>>(kappa, in_pitch ? in_pitch : (size_t)G::M, spec, pitch,
                                                                                             twM, twL, scale, rec);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

}  // namespace
