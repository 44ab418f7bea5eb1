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

using PdParams = GridBoxParams;

struct PdBins {
    int kind, dist_bin, vel_bin, moments;
    double reach, reach2, dist_width, vel_width, offset;
    unsigned first, second;
};

struct PdLayout {
    size_t params, cnt, cell_start, tile_start, cursor, cell_of, obj, sorted, part, total;
    PdLayout(size_t n, int moment_rows) {
        const size_t cap = grid_box_cells_cap(n);
        size_t o = 0;
        params = o;     o += align256(sizeof(PdParams));
        cnt = o;        o += align256(cap * 4);
        cell_start = o; o += align256((cap + 1) * 4);
        tile_start = o; o += align256((cap + 1) * 4);
        cursor = o;     o += align256(cap * 4);
        cell_of = o;    o += align256(n * 4);
        obj = o;        o += align256(n * sizeof(PdObj));
        sorted = o;     o += align256(n * sizeof(PdObj));
        part = o;       o += align256((size_t)PD_GRID * (size_t)moment_rows * 24);
        total = o;
    }
};

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

// One thread per object: r and v widened to fp64, the original index, and the bounding box of r to prm->kmin / kmax
// (one atomic per workgroup and axis).
template <typename TP, typename TV>
__global__ void __launch_bounds__(256)
pd_prep_kernel(const TP* __restrict__ pos, const TV* __restrict__ vel, size_t n, PdObj* __restrict__ obj,
               PdParams* prm) {
    __shared__ double wlo[3][4], whi[3][4];
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
    const int w = threadIdx.x / 64, l = threadIdx.x % 64;
    for (int a = 0; a < 3; ++a) {
        const double mn = wave_min(lo[a]), mx = wave_max(hi[a]);
        if (l == 0) { wlo[a][w] = mn; whi[a][w] = mx; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        double mn = wlo[a][0], mx = whi[a][0];
        for (int k = 1; k < 4; ++k) { mn = fmin(mn, wlo[a][k]); mx = fmax(mx, whi[a][k]); }
        if (mn <= mx) {
            atomicMin(&prm->kmin[a], d2key(mn));
            atomicMax(&prm->kmax[a], d2key(mx));
        }
    }
}

// Work item = (tile of PD_BLOCK objects of cell a, neighbour k), walked by a persistent grid as in pairwise.hip: each
// thread holds one i of the tile, the j objects of cell a + offset[k] pass through LDS PD_BLOCK at a time as rows r, v
// and original index (k = 0: the cell itself, j > i only).  A pair is seen when d = sqrt((dx dx + dy dy) + dz dz)
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
               const unsigned* __restrict__ tile_start, const PdParams* prm, PdBins bn, unsigned long long flush_at,
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
    const int dx = prm->dims[0], dy = prm->dims[1], dz = prm->dims[2];
    const unsigned ncells = prm->ncells;
    const unsigned long long nitems = (unsigned long long)prm->ntiles * GRID_NEIGH;
    for (unsigned long long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const unsigned tile = (unsigned)(item / GRID_NEIGH);
        const int k = (int)(item % GRID_NEIGH);
        const unsigned a = grid_cell_of_tile(tile_start, ncells, tile);
        const int ax = (int)(a % (unsigned)dx), ay = (int)((a / (unsigned)dx) % (unsigned)dy), az = (int)(a / ((unsigned)dx * (unsigned)dy));
        const int bx = ax + grid_offsets[k][0], by = ay + grid_offsets[k][1], bz = az + grid_offsets[k][2];
        if (bx < 0 || bx >= dx || by < 0 || by >= dy || bz < 0 || bz >= dz) continue;
        const unsigned b = ((unsigned)bz * (unsigned)dy + (unsigned)by) * (unsigned)dx + (unsigned)bx;
        const unsigned i0 = cell_start[a] + (tile - tile_start[a]) * PD_BLOCK;
        const unsigned i1 = min(i0 + PD_BLOCK, cell_start[a + 1]);
        const unsigned j0 = k == 0 ? i0 + 1 : cell_start[b];
        const unsigned j1 = cell_start[b + 1];
        if (j0 >= j1) continue;

        const unsigned i = i0 + tid;
        const bool valid = i < i1;
        PdObj oi;
        if (valid) oi = sorted[i];
        for (unsigned jc = j0; jc < j1; jc += PD_BLOCK) {
            const int m = (int)min((unsigned)PD_BLOCK, j1 - jc);
            if (LDS_HIST) {
                const unsigned long long stage = (unsigned long long)(i1 - i0) * (unsigned long long)m;
                if (pending + stage > flush_at) flush();
                pending += stage;
            }
            __syncthreads();
            if (jc + tid < j1) {
                const PdObj oj = sorted[jc + tid];
                for (int c = 0; c < 3; ++c) {
                    jr[c * PD_BLOCK + tid] = oj.r[c];
                    jr[(3 + c) * PD_BLOCK + tid] = oj.v[c];
                }
                jidx[tid] = oj.idx;
            }
            __syncthreads();
            if (!valid) continue;
            const int q0 = (k == 0 && i + 1 > jc) ? (int)min((unsigned)m, i + 1 - jc) : 0;
            for (int q = q0; q < m; ++q) {
                const double ddx = jr[q] - oi.r[0], ddy = jr[PD_BLOCK + q] - oi.r[1], ddz = jr[2 * PD_BLOCK + q] - oi.r[2];
                const double d2 = (ddx * ddx + ddy * ddy) + ddz * ddz;
                if (!(d2 <= bn.reach2)) continue;
                const double d = sqrt(d2);
                if (!(d <= bn.reach)) continue;
                const unsigned row = min(oi.idx, jidx[q]);
                if (row < bn.first || row >= bn.second) continue;
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
            }
        }
    }
    if (LDS_HIST) flush();
    for (int o = 32; o > 0; o >>= 1) outside += __shfl_xor(outside, o, 64);
    if (tid % 64 == 0 && outside) atomicAdd(outside_g, outside);
    if (!mrows) return;
    __syncthreads();
    double* p1 = part;
    double* p2 = part + (size_t)PD_GRID * mrows;
    unsigned long long* pc = (unsigned long long*)(part + 2 * (size_t)PD_GRID * mrows);
    for (int bin = tid; bin < mrows; bin += PD_BLOCK) {
        double s1 = h1[bin], s2 = h2[bin];
        unsigned long long sc = hc[bin];
        for (int v = 1; v < PD_WAVES; ++v) { s1 += h1[v * mrows + bin]; s2 += h2[v * mrows + bin]; sc += hc[v * mrows + bin]; }
        const size_t o = (size_t)blockIdx.x * mrows + bin;
        p1[o] = s1;
        p2[o] = s2;
        pc[o] = sc;
    }
}

// out[bin] = sum of the PD_GRID workgroup rows, in row order.
__global__ void __launch_bounds__(256)
pd_reduce_kernel(const double* __restrict__ part, int mrows, double* __restrict__ s1, double* __restrict__ s2,
                 unsigned long long* __restrict__ counts) {
    const int bin = blockIdx.x * blockDim.x + threadIdx.x;
    if (bin >= mrows) return;
    const double* p1 = part;
    const double* p2 = part + (size_t)PD_GRID * mrows;
    const unsigned long long* pc = (const unsigned long long*)(part + 2 * (size_t)PD_GRID * mrows);
    double a1 = 0.0, a2 = 0.0;
    unsigned long long sc = 0;
    for (int g = 0; g < PD_GRID; ++g) {
        const size_t o = (size_t)g * mrows + bin;
        a1 += p1[o];
        a2 += p2[o];
        sc += pc[o];
    }
    s1[bin] = a1;
    s2[bin] = a2;
    counts[bin] = sc;
}

template <typename TP, typename TV>
void launch_prep(const void* pos, const void* vel, size_t n, PdObj* obj, PdParams* prm, hipStream_t s) {
    pd_prep_kernel<TP, TV><<<ast::stream_grid(n, 256), 256, 0, s>>>((const TP*)pos, (const TV*)vel, n, obj, prm);
}

}  // namespace

extern "C" size_t ast_pairwise_pdf_workspace_bytes(size_t n, int dist_bin, int vel_bin, int moments) {
    if (!bins_ok(dist_bin, vel_bin, moments)) return 0;
    return PdLayout(n, moments ? dist_bin : 0).total;
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
    AST_CHECK_ARG(n < (size_t(1) << 31));
    AST_CHECK_ARG(n == 0 || (pos_d && vel_d));
    const PdLayout L(n, 0);
    AST_CHECK_ARG(work_d && work_bytes >= L.obj + align256(n * sizeof(PdObj)));
    hipStream_t s = ast::as_stream(stream);
    char* ws = (char*)work_d;
    PdParams* prm = (PdParams*)(ws + L.params);
    AST_CHECK_HIP(hipMemsetAsync(prm->kmin, 0xff, sizeof(prm->kmin), s));
    AST_CHECK_HIP(hipMemsetAsync(prm->kmax, 0x00, sizeof(prm->kmax), s));
    if (n == 0) return AST_OK;
    AST_PROF("pairwise_pdf_prep", s);
    PdObj* obj = (PdObj*)(ws + L.obj);
    if (pos_dtype == AST_F32 && vel_dtype == AST_F32)
        launch_prep<float, float>(pos_d, vel_d, n, obj, prm, s);
    else if (pos_dtype == AST_F32)
        launch_prep<float, double>(pos_d, vel_d, n, obj, prm, s);
    else if (vel_dtype == AST_F32)
        launch_prep<double, float>(pos_d, vel_d, n, obj, prm, s);
    else
        launch_prep<double, double>(pos_d, vel_d, n, obj, prm, s);
    AST_CHECK_LAUNCH();
    return AST_OK;
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
    AST_CHECK_ARG(n < (size_t(1) << 31));
    AST_CHECK_ARG(first <= second && second <= n);
    AST_CHECK_ARG(hist_d && outside_d);
    AST_CHECK_ARG(work_d && work_bytes >= ast_pairwise_pdf_workspace_bytes(n, dist_bin, vel_bin, moments));
    hipStream_t s = ast::as_stream(stream);
    const int nbins = dist_bin * vel_bin;
    AST_CHECK_HIP(hipMemsetAsync(hist_d, 0, (size_t)nbins * sizeof(unsigned long long), s));
    AST_CHECK_HIP(hipMemsetAsync(outside_d, 0, sizeof(unsigned long long), s));
    if (n < 2 || first == second) {
        if (moments) {
            AST_CHECK_HIP(hipMemsetAsync(s1_d, 0, dist_bin * sizeof(double), s));
            AST_CHECK_HIP(hipMemsetAsync(s2_d, 0, dist_bin * sizeof(double), s));
            AST_CHECK_HIP(hipMemsetAsync(mcount_d, 0, dist_bin * sizeof(unsigned long long), s));
        }
        return AST_OK;
    }
    const PdLayout L(n, moments ? dist_bin : 0);
    char* ws = (char*)work_d;
    PdParams* prm = (PdParams*)(ws + L.params);
    unsigned* cnt = (unsigned*)(ws + L.cnt);
    unsigned* cell_start = (unsigned*)(ws + L.cell_start);
    unsigned* tile_start = (unsigned*)(ws + L.tile_start);
    unsigned* cursor = (unsigned*)(ws + L.cursor);
    unsigned* cell_of = (unsigned*)(ws + L.cell_of);
    const PdObj* obj = (const PdObj*)(ws + L.obj);
    PdObj* sorted = (PdObj*)(ws + L.sorted);
    double* part = (double*)(ws + L.part);
    const size_t cap = grid_box_cells_cap(n);
    {
        AST_PROF("pairwise_pdf_grid", s);
        grid_box_plan_kernel<<<1, 64, 0, s>>>(prm, reach, (unsigned)cap, single_cell);
        AST_CHECK_LAUNCH();
        AST_CHECK_HIP(hipMemsetAsync(cnt, 0, cap * 4, s));
        grid_box_count_kernel<<<ast::stream_grid(n, 256), 256, 0, s>>>(obj, n, prm, cell_of, cnt);
        AST_CHECK_LAUNCH();
        grid_scan_kernel<PD_BLOCK><<<1, 1024, 0, s>>>(cnt, prm, cell_start, tile_start, cursor);
        AST_CHECK_LAUNCH();
        grid_scatter_kernel<<<ast::stream_grid(n, 256), 256, 0, s>>>(obj, n, cell_of, cursor, sorted);
        AST_CHECK_LAUNCH();
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
        if (use_lds)
            pd_pair_kernel<true><<<PD_GRID, PD_BLOCK, lds, s>>>(sorted, cell_start, tile_start, prm, bn, flush_at, hist_d,
                                                                outside_d, part);
        else
            pd_pair_kernel<false><<<PD_GRID, PD_BLOCK, lds, s>>>(sorted, cell_start, tile_start, prm, bn, flush_at,
                                                                 hist_d, outside_d, part);
        AST_CHECK_LAUNCH();
    }
    if (moments) {
        AST_PROF("pairwise_pdf_reduce", s);
        pd_reduce_kernel<<<(dist_bin + 255) / 256, 256, 0, s>>>(part, dist_bin, s1_d, s2_d, mcount_d);
        AST_CHECK_LAUNCH();
    }
    return AST_OK;
}
