// Pairwise-velocity histograms (particles/utils_cython/pairwise_velocity.pyx: mean_pv_z_sign, mean_pv_radial,
// :194-313): the (separation bin, velocity bin) pair counts from which the mean streaming velocity v12(r) and the
// pairwise dispersion sigma12(r) follow.  Per-object prep, the bounding-box cell grid of cell_grid.h as the pair finder
// (as pairwise.hip), and a tiled pair kernel that counts into an exact integer histogram: 32-bit counters in LDS,
// flushed into the 64-bit global histogram before they could overflow, or, for a histogram beyond the LDS budget, one
// 64-bit global atomic per counted pair.  Integer adds commute, so both paths give the same counts in any order.
// All pair arithmetic is fp64 (the library is built with -ffp-contract=off: op-by-op IEEE, like numpy).
#include "ast_common.h"
#include "cell_grid.h"
#include <cmath>
#include <cstdlib>

namespace {

constexpr int PD_BLOCK = 256;               // i objects per tile = j objects per LDS stage
constexpr int PD_WAVES = PD_BLOCK / 64;
constexpr int PD_GRID = 1024;               // persistent pair-kernel workgroups (256 CUs x 4)
constexpr int PD_MAX_BINS = 1 << 22;        // dist_bin * vel_bin counters (32 MiB of 64-bit counts)
constexpr int PD_MAX_MOMENT_ROWS = AST_PVPDF_MAX_MOMENT_ROWS;    // 4 wave rows x 24 B x dist_bin beside the j stage
// Dynamic LDS of the pair kernel on the LDS path: all of a gfx950 CU's 160 KiB.  Measured: LDS
// counters take at most 0.52 of the time of global atomics at every size that fits, also past 80 KiB where one
// workgroup has the CU to itself.
constexpr size_t PD_LDS_BUDGET = 160 * 1024;
constexpr unsigned long long PD_FLUSH_AT = 0xffffffffull;        // 32-bit LDS counters: at most this many adds

struct PdObj { double r[3], v[3]; unsigned idx, pad; };

struct PdBins {
    int kind, dist_bin, vel_bin, moments;
    double reach, reach2, dist_width, vel_width, offset;
    unsigned first, second;
};

inline GridLayout pd_layout(size_t n, int moment_rows) {
    return GridLayout(1, n, 0, grid_cells_cap(n, 1), sizeof(PdObj), (size_t)PD_GRID * (size_t)moment_rows * 24);
}

inline bool bins_ok(int dist_bin, int vel_bin, int moments) {
    return dist_bin >= 1 && vel_bin >= 1 && (long long)dist_bin * vel_bin <= PD_MAX_BINS &&
           (!moments || dist_bin <= PD_MAX_MOMENT_ROWS);
}

// LDS of the pair kernel without the histogram: the j stage (r, v, index) and the per-wave moment rows.
inline size_t fixed_lds(int dist_bin, int moments) {
    return (size_t)6 * PD_BLOCK * sizeof(double) + (size_t)PD_BLOCK * 4 +
           (moments ? (size_t)PD_WAVES * dist_bin * 24 : 0);
}

// Counters that the LDS path can hold (0: none, the histogram goes to global memory).
inline int lds_bins(int dist_bin, int moments) {
    const size_t fixed = fixed_lds(dist_bin, moments);
    return PD_LDS_BUDGET > fixed ? (int)((PD_LDS_BUDGET - fixed) / 4) : 0;
}

// One thread per object: r and v widened to fp64, the original index, and the bounding box of r to `box`
// (grid_bounds_commit).
template <typename TP, typename TV>
__global__ void __launch_bounds__(256)
pd_prep_kernel(const TP* __restrict__ pos, const TV* __restrict__ vel, size_t n, PdObj* __restrict__ obj,
               GridBounds* box) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        PdObj o;
        for (int a = 0; a < 3; ++a) { o.r[a] = (double)pos[3 * i + a]; o.v[a] = (double)vel[3 * i + a]; }
        o.idx = (unsigned)i;
        o.pad = 0u;
        obj[i] = o;
        for (int a = 0; a < 3; ++a) { lo[a] = fmin(lo[a], o.r[a]); hi[a] = fmax(hi[a], o.r[a]); }
    }
    grid_bounds_commit<256>(lo, hi, box);
}

// The walk of cell_grid.h (grid_pair_walk: one set, open boundaries) with the staged j objects in LDS as rows r, v and
// original index.  A pair is seen when d = sqrt((dx dx + dy dy) + dz dz)
// <= reach and the smaller of its two original indices lies in [first, second).  With the differences taken j - i,
//   kind 0 (z_sign): v12 = (vz_j - vz_i) sign(z_j - z_i),   kind 1 (radial): v12 = ((dvx dx + dvy dy) + dvz dz) / d;
// both are unchanged bit for bit when i and j swap (two exact negations per product), so which of the two the thread
// holds does not matter.  ds = float(d / dist_width), vs = float(v12 / vel_width + offset); the pair counts in
// (int(ds), int(vs)) when ds < dist_bin and 0 <= vs < vel_bin, else in `outside` (kept per thread, one 64-bit integer
// atomic per wave at the end).
// LDS_HIST: each counted pair adds 1 to a 32-bit LDS counter; before an LDS stage that could take a counter past
// flush_at pairs since the last flush, the workgroup adds its non-zero counters into hist_g with 64-bit integer atomics
// and clears them.  Otherwise each counted pair is one 64-bit integer atomic on hist_g.
// Moments (bn.moments): a seen pair with ds < dist_bin and finite v12 adds (v12, v12^2, 1) to its wave's LDS row of
// that distance bin; at the end the workgroup's row (waves summed in order) is stored to part - no global float
// atomics.
template <bool LDS_HIST>
__global__ void __launch_bounds__(PD_BLOCK)
pd_pair_kernel(const PdObj* __restrict__ sorted, const unsigned* __restrict__ cell_start,
               const unsigned* __restrict__ tile_start, const GridBoxParams* prm, PdBins bn, unsigned long long flush_at,
               unsigned long long* __restrict__ hist_g, unsigned long long* __restrict__ outside_g,
               double* __restrict__ part) {
    extern __shared__ double lds[];
    const int mrows = bn.moments ? bn.dist_bin : 0;
    double* jr = lds;                                   // [6][PD_BLOCK]: r, v of the staged j objects
    double* h1 = lds + 6 * PD_BLOCK;                    // [PD_WAVES][mrows]
    double* h2 = h1 + PD_WAVES * mrows;
    unsigned long long* hc = (unsigned long long*)(h2 + PD_WAVES * mrows);
    unsigned* jidx = (unsigned*)(hc + PD_WAVES * mrows);    // [PD_BLOCK]
    unsigned* hist = jidx + PD_BLOCK;                   // [nbins] (LDS_HIST)
    const int tid = threadIdx.x, w = tid / 64;
    const int nbins = bn.dist_bin * bn.vel_bin;
    for (int k = tid; k < PD_WAVES * mrows; k += PD_BLOCK) { h1[k] = 0.0; h2[k] = 0.0; hc[k] = 0ull; }
    if (LDS_HIST)
        for (int k = tid; k < nbins; k += PD_BLOCK) hist[k] = 0u;
    double* wh1 = h1 + w * mrows;
    double* wh2 = h2 + w * mrows;
    unsigned long long* whc = hc + w * mrows;
    unsigned long long pending = 0;                     // bound on the pairs added to any LDS counter since the last flush
    unsigned long long outside = 0;

    auto flush = [&]() {
        __syncthreads();
        for (int b = tid; b < nbins; b += PD_BLOCK) {
            const unsigned c = hist[b];
            if (c) {
                atomicAdd(&hist_g[b], (unsigned long long)c);
                hist[b] = 0u;
            }
        }
        pending = 0;
        __syncthreads();
    };

    const float fdist = (float)bn.dist_bin, fvel = (float)bn.vel_bin;
    PdObj oi;
    grid_pair_walk<PD_BLOCK>(
        cell_start, tile_start, cell_start, prm, false, true,
        [&](unsigned i) { oi = sorted[i]; },
        [&](unsigned ni, int m) {
            if (LDS_HIST) {
                const unsigned long long stage = (unsigned long long)ni * (unsigned long long)m;
                if (pending + stage > flush_at) flush();
                pending += stage;
            }
        },
        [&](unsigned j, int t) {
            const PdObj oj = sorted[j];
            for (int c = 0; c < 3; ++c) {
                jr[c * PD_BLOCK + t] = oj.r[c];
                jr[(3 + c) * PD_BLOCK + t] = oj.v[c];
            }
            jidx[t] = oj.idx;
        },
        [&](int q) {
            const double ddx = jr[q] - oi.r[0], ddy = jr[PD_BLOCK + q] - oi.r[1], ddz = jr[2 * PD_BLOCK + q] - oi.r[2];
            const double d2 = (ddx * ddx + ddy * ddy) + ddz * ddz;
            if (!(d2 <= bn.reach2)) return;
            const double d = sqrt(d2);
            if (!(d <= bn.reach)) return;
            const unsigned row = min(oi.idx, jidx[q]);
            if (row < bn.first || row >= bn.second) return;
            const double wz = jr[5 * PD_BLOCK + q] - oi.v[2];
            double v12;
            if (bn.kind == 0) {
                v12 = wz * (double)((int)(ddz > 0.0) - (int)(ddz < 0.0));
            } else {
                const double wx = jr[3 * PD_BLOCK + q] - oi.v[0], wy = jr[4 * PD_BLOCK + q] - oi.v[1];
                v12 = ((wx * ddx + wy * ddy) + wz * ddz) / d;
            }
            const float ds = (float)(d / bn.dist_width);
            const float vs = (float)(v12 / bn.vel_width + bn.offset);
            const bool in_rows = ds < fdist;
            const int ra = in_rows ? (int)ds : 0;
            if (in_rows && vs >= 0.0f && vs < fvel) {
                const int bin = ra * bn.vel_bin + (int)vs;
                if (LDS_HIST) atomicAdd(&hist[bin], 1u);
                else atomicAdd(&hist_g[bin], 1ull);
            } else {
                ++outside;
            }
            if (mrows && in_rows && isfinite(v12)) {
                atomicAdd(&wh1[ra], v12);
                atomicAdd(&wh2[ra], v12 * v12);
                atomicAdd(&whc[ra], 1ull);
            }
        });
    if (LDS_HIST) flush();
    for (int o = 32; o > 0; o >>= 1) outside += __shfl_xor(outside, o, 64);
    if (tid % 64 == 0 && outside) atomicAdd(outside_g, outside);
    if (!mrows) return;
    __syncthreads();
    grid_store_rows<PD_WAVES, PD_GRID>(h1, h2, hc, mrows, part);
}

}  // namespace

extern "C" size_t ast_pairwise_pdf_workspace_bytes(size_t n, int dist_bin, int vel_bin, int moments) {
    if (!bins_ok(dist_bin, vel_bin, moments)) return 0;
    return pd_layout(n, moments ? dist_bin : 0).total;
}

extern "C" int ast_pairwise_pdf_max_bins(void) { return PD_MAX_BINS; }

extern "C" int ast_pairwise_pdf_lds_bins(int dist_bin, int moments) {
    if (dist_bin < 1 || (moments && dist_bin > PD_MAX_MOMENT_ROWS)) return 0;
    return lds_bins(dist_bin, moments);
}

extern "C" int ast_pairwise_pdf_prepare(const void* pos_d, int pos_dtype, const void* vel_d, int vel_dtype, size_t n,
                                        void* work_d, size_t work_bytes, void* stream) {
    AST_CHECK_ARG(pos_dtype == AST_F32 || pos_dtype == AST_F64);
    AST_CHECK_ARG(vel_dtype == AST_F32 || vel_dtype == AST_F64);
    AST_CHECK_ARG(grid_count_ok(n));
    AST_CHECK_ARG(n == 0 || (pos_d && vel_d));
    const GridLayout L = pd_layout(n, 0);
    AST_CHECK_ARG(work_d && work_bytes >= L.sorted[0]);
    hipStream_t s = ast::as_stream(stream);
    return grid_prepare<1, PdObj>((char*)work_d, L, &n, nullptr, "pairwise_pdf_prep", s,
                                  [&](int, PdObj* obj, GridBounds* box) {
        ast::dispatch_f32_f64(pos_dtype == AST_F32, vel_dtype == AST_F32, [&](auto tp, auto tv) {
            using TP = decltype(tp);
            using TV = decltype(tv);
            pd_prep_kernel<TP, TV><<<ast::stream_grid(n, 256), 256, 0, s>>>((const TP*)pos_d, (const TV*)vel_d, n, obj,
                                                                             box);
        });
    });
}

extern "C" int ast_pairwise_pdf(void* work_d, size_t work_bytes, size_t n, int kind, double r, int dist_bin,
                                int vel_bin, double dist_width, double vel_width, size_t first, size_t second,
                                int single_cell, int force_global, unsigned long long* hist_d,
                                unsigned long long* outside_d, double* s1_d, double* s2_d,
                                unsigned long long* mcount_d, void* stream) {
    const int moments = s1_d || s2_d || mcount_d;
    AST_CHECK_ARG(kind == AST_PVPDF_Z_SIGN || kind == AST_PVPDF_RADIAL);
    AST_CHECK_ARG(dist_bin >= 1 && vel_bin >= 1 && (long long)dist_bin * vel_bin <= PD_MAX_BINS);
    AST_CHECK_ARG(!moments || (s1_d && s2_d && mcount_d && dist_bin <= PD_MAX_MOMENT_ROWS));
    const double reach = (double)(float)r;              // the reference declares `float r`
    AST_CHECK_ARG(reach > 0.0 && std::isfinite(reach));
    AST_CHECK_ARG(dist_width > 0.0 && std::isfinite(dist_width));
    AST_CHECK_ARG(vel_width > 0.0 && std::isfinite(vel_width));
    AST_CHECK_ARG(grid_count_ok(n));
    AST_CHECK_ARG(first <= second && second <= n);
    AST_CHECK_ARG(hist_d && outside_d);
    AST_CHECK_ARG(work_d && work_bytes >= ast_pairwise_pdf_workspace_bytes(n, dist_bin, vel_bin, moments));
    hipStream_t s = ast::as_stream(stream);
    const int nbins = dist_bin * vel_bin;
    AST_CHECK_HIP(hipMemsetAsync(hist_d, 0, (size_t)nbins * sizeof(unsigned long long), s));
    AST_CHECK_HIP(hipMemsetAsync(outside_d, 0, sizeof(unsigned long long), s));
    if (grid_no_pairs(1, n, 0) || first == second) {
        if (moments) {
            AST_CHECK_HIP(hipMemsetAsync(s1_d, 0, dist_bin * sizeof(double), s));
            AST_CHECK_HIP(hipMemsetAsync(s2_d, 0, dist_bin * sizeof(double), s));
            AST_CHECK_HIP(hipMemsetAsync(mcount_d, 0, dist_bin * sizeof(unsigned long long), s));
        }
        return AST_OK;
    }
    const GridLayout L = pd_layout(n, moments ? dist_bin : 0);
    char* ws = (char*)work_d;
    const GridSorted<PdObj> g(ws, L, 0);
    {
        AST_PROF("pairwise_pdf_grid", s);
        grid_box_plan_kernel<<<1, 64, 0, s>>>(g.prm, reach, (unsigned)L.cap, single_cell);
        AST_CHECK_LAUNCH();
        if (int rc = grid_sort_sets<PD_BLOCK, PdObj>(ws, L, 0, &n, s)) return rc;
    }
    PdBins bn;
    bn.kind = kind;
    bn.dist_bin = dist_bin;
    bn.vel_bin = vel_bin;
    bn.moments = moments;
    bn.reach = reach;
    // Pre-test on d^2 with a relative margin far above the rounding of d^2 and of its root: every pair with
    // sqrt(d^2) <= reach passes it; the decision itself is the fp64 d <= reach.
    bn.reach2 = reach * reach * (1.0 + 1e-12);
    bn.dist_width = dist_width;
    bn.vel_width = vel_width;
    bn.offset = (double)(vel_bin / 2);
    bn.first = (unsigned)first;
    bn.second = (unsigned)second;
    const size_t fixed = fixed_lds(dist_bin, moments);
    const bool use_lds = !force_global && nbins <= lds_bins(dist_bin, moments);
    const size_t lds = fixed + (use_lds ? (size_t)nbins * 4 : 0);
    AST_CHECK_ARG(lds <= PD_LDS_BUDGET);
    // AST_PVPDF_FLUSH_AT (tests only): flush the LDS counters after at most this many pairs per stage bound.
    unsigned long long flush_at = PD_FLUSH_AT;
    if (const char* f = getenv("AST_PVPDF_FLUSH_AT")) flush_at = strtoull(f, nullptr, 10);
    if (flush_at > PD_FLUSH_AT) flush_at = PD_FLUSH_AT;
    static ast::PerDeviceOnce attr_once;
    if (attr_once.need()) {
        AST_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pd_pair_kernel<true>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)PD_LDS_BUDGET));
        AST_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pd_pair_kernel<false>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)PD_LDS_BUDGET));
        attr_once.mark();
    }
    {
        AST_PROF(use_lds ? "pairwise_pdf_pairs_lds" : "pairwise_pdf_pairs_global", s);
        const auto pairs = use_lds ? pd_pair_kernel<true> : pd_pair_kernel<false>;
        pairs<<<PD_GRID, PD_BLOCK, lds, s>>>(g.sorted1, g.cell_start1, g.tile_start1, g.prm, bn, flush_at, hist_d,
                                             outside_d, g.part);
        AST_CHECK_LAUNCH();
    }
    if (moments) {
        AST_PROF("pairwise_pdf_reduce", s);
        grid_reduce3_kernel<PD_GRID><<<(dist_bin + 255) / 256, 256, 0, s>>>(g.part, dist_bin, s1_d, s2_d, mcount_d);
        AST_CHECK_LAUNCH();
    }
    return AST_OK;
}
