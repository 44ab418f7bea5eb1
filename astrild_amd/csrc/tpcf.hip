// Two-point correlation function (particles/hutils/tpcf.py, halotools' s_mu_tpcf / tpcf) of one sample in a periodic
// box, or of two samples in a periodic box or with open boundaries: per-object prep (redshift-space shift, wrap,
// bounds), the uniform cell grid of cell_grid.h (counting sort by cell) as the pair finder, a tiled pair kernel that
// counts minimum-image pairs into an exact integer (s, mu) histogram in LDS, and a fixed-order sum of the workgroup
// rows.  All pair arithmetic is fp64 (the library is built with -ffp-contract=off).
#include "ast_common.h"
#include "cell_grid.h"
#include <cmath>
#include <cstdlib>

namespace {

constexpr int TP_BLOCK = 256;               // i objects per tile = j objects per LDS stage
constexpr int TP_WAVES = TP_BLOCK / 64;
constexpr int TP_GRID = 1024;               // persistent pair-kernel workgroups (256 CUs x 4)
constexpr int TP_MAX_BINS = 10000;          // ns * max(nmu, 1): 100 x 100
constexpr int TP_MAX_EDGES = 1001;          // ns + 1 and nmu + 1 each
constexpr size_t TP_LDS = 65536;            // dynamic LDS budget of the pair kernel
constexpr unsigned long long TP_FLUSH_AT = 0xffffffffull;    // 32-bit LDS counters: at most this many adds

struct TpObj { double r[3]; };

inline int nbins_of(int ns, int nmu) { return ns * (nmu > 0 ? nmu : 1); }

inline bool bins_ok(int ns, int nmu) {
    return ns >= 1 && ns < TP_MAX_EDGES && nmu >= 0 && nmu < TP_MAX_EDGES && nbins_of(ns, nmu) <= TP_MAX_BINS;
}

// One set (ast_tpcf_*), or two (ast_tpcf_cross_*) on one shared grid with room for the larger set's cells.
inline GridLayout tp_layout(int nsets, size_t n1, size_t n2, int nbins) {
    return GridLayout(nsets, n1, n2, grid_cells_cap(n1 > n2 ? n1 : n2, 27), sizeof(TpObj),
                      (size_t)TP_GRID * (size_t)nbins * 8);
}

// numpy's arithmetic in the input dtypes, each float32 operation done in fp64 and rounded once (exact: fp64 carries
// more than 2 x 24 + 2 bits, so the result is the correctly rounded float32 one).
template <typename T> __device__ inline T div_as(T a, double b) { return (T)((double)a / b); }
template <typename T> __device__ inline T add_as(T a, T b) { return (T)((double)a + (double)b); }
template <typename T> __device__ inline T sub_as(T a, T b) { return (T)((double)a - (double)b); }

// One thread per object, as tpcf.py:74-97: pos_s = pos; pos_s[los] += vel[los] / 100. (TV / 100 in TV, the add in
// the wider of TP and TV, stored back as TP); then pos_s[los] > L -> - L, and < 0 -> + L, in TP (boxsize == 0, open:
// the wrap subtracts or adds 0, which changes nothing).  vel == nullptr: no shift, no wrap.  Widened to fp64 into obj;
// the min / max of all shifted coordinates (NaN counts as -inf / +inf) go to `box` (grid_bounds_commit).
template <typename TP, typename TV>
__global__ void __launch_bounds__(256)
tp_prep_kernel(const TP* __restrict__ pos, const TV* __restrict__ vel, int los, double boxsize, size_t n,
               TpObj* __restrict__ obj, GridBounds* box) {
    using TC = decltype(TP() + TV());
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const TP bx = (TP)boxsize;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        TpObj o;
        for (int a = 0; a < 3; ++a) o.r[a] = (double)pos[3 * i + a];
        if (vel) {
            const TV q = div_as<TV>(vel[3 * i + los], 100.0);
            TP s = (TP)add_as<TC>((TC)pos[3 * i + los], (TC)q);
            if (s > bx) s = sub_as<TP>(s, bx);
            if (s < (TP)0) s = add_as<TP>(s, bx);
            o.r[los] = (double)s;
        }
        obj[i] = o;
        for (int a = 0; a < 3; ++a) {
            const double v = o.r[a];
            lo[a] = fmin(lo[a], v == v ? v : -INFINITY);
            hi[a] = fmax(hi[a], v == v ? v : INFINITY);
        }
    }
    grid_bounds_commit<256>(lo, hi, box);
}

// What a pair kernel needs beside the grid: the box, the edges in device memory, and tp_bins' choices.
struct TpBins {
    double boxsize;
    int los;
    const double* s_edges;
    int ns;
    const double* mu_edges;
    int nmu, hcopies;
    unsigned long long flush_at;
};

// The walk of cell_grid.h (grid_pair_walk) with the positions of the staged j objects in LDS; `periodic` and
// `auto_pairs` as there.  A pair counts in bin (k, l) when s2[k] < d^2 <= s2[k + 1] and (nmu > 0)
// mu[l] < mu <= mu[l + 1], with a = |x_i - x_j| per axis, periodic: the minimum image a = min(a, L - a),
// d^2 = (a_x^2 + a_y^2) + a_z^2 and mu = a_los / sqrt(d^2); both bins by binary search on fp64 comparisons.
// Each pair adds 1 to a 32-bit LDS counter of the wave's histogram copy (hcopies copies, wave w uses w % hcopies).
// Before an LDS stage that could take a counter past flush_at pairs since the last flush, the workgroup adds its
// counters into its own 64-bit row of part (plain loads and stores: no other workgroup touches the row) and clears
// them; the row is complete after the final flush.  No global atomics.
__device__ __forceinline__ void tp_count_pairs(const TpObj* __restrict__ sorted1, const unsigned* __restrict__ cell_start1,
                                               const unsigned* __restrict__ tile_start,
                                               const TpObj* __restrict__ sorted2,
                                               const unsigned* __restrict__ cell_start2, const GridBoxParams* prm,
                                               bool periodic, bool auto_pairs, const TpBins& bn,
                                               unsigned long long* __restrict__ part) {
    extern __shared__ double lds[];
    const int ns = bn.ns, nmu = bn.nmu, hcopies = bn.hcopies, los = bn.los;
    const double boxsize = bn.boxsize;
    double* jr = lds;                                   // [3][TP_BLOCK]: the staged j objects
    double* s2 = jr + 3 * TP_BLOCK;                     // [ns + 1] squared s edges
    double* me = s2 + (ns + 1);                         // [nmu + 1] mu edges
    unsigned* hist = (unsigned*)(me + (nmu + 1));       // [hcopies][nbins]
    const int tid = threadIdx.x, w = tid / 64;
    const int nbins = ns * (nmu > 0 ? nmu : 1);
    for (int k = tid; k <= ns; k += TP_BLOCK) s2[k] = bn.s_edges[k] * bn.s_edges[k];
    for (int k = tid; k <= nmu && nmu > 0; k += TP_BLOCK) me[k] = bn.mu_edges[k];
    for (int k = tid; k < hcopies * nbins; k += TP_BLOCK) hist[k] = 0u;
    unsigned* whist = hist + (w % hcopies) * nbins;
    unsigned long long* row = part + (size_t)blockIdx.x * nbins;
    bool flushed = false;                               // row holds a partial sum (else it is not yet written)
    unsigned long long pending = 0;                     // bound on the pairs added to any counter since the last flush

    auto flush = [&]() {
        __syncthreads();
        for (int b = tid; b < nbins; b += TP_BLOCK) {
            unsigned long long sum = 0;
            for (int c = 0; c < hcopies; ++c) { sum += hist[c * nbins + b]; hist[c * nbins + b] = 0u; }
            row[b] = flushed ? row[b] + sum : sum;
        }
        flushed = true;
        pending = 0;
        __syncthreads();
    };

    __syncthreads();
    const double s2lo = s2[0], s2hi = s2[ns];
    const double mulo = nmu > 0 ? me[0] : 0.0, muhi = nmu > 0 ? me[nmu] : 0.0;
    TpObj oi;
    grid_pair_walk<TP_BLOCK>(
        cell_start1, tile_start, cell_start2, prm, periodic, auto_pairs,
        [&](unsigned i) { oi = sorted1[i]; },
        [&](unsigned ni, int m) {
            const unsigned long long stage = (unsigned long long)ni * (unsigned long long)m;
            if (pending + stage > bn.flush_at) flush();
            pending += stage;
        },
        [&](unsigned j, int t) {
            const TpObj oj = sorted2[j];
            for (int c = 0; c < 3; ++c) jr[c * TP_BLOCK + t] = oj.r[c];
        },
        [&](int q) {
            double px = fabs(oi.r[0] - jr[q]), py = fabs(oi.r[1] - jr[TP_BLOCK + q]),
                   pz = fabs(oi.r[2] - jr[2 * TP_BLOCK + q]);
            if (periodic) {
                px = fmin(px, boxsize - px);
                py = fmin(py, boxsize - py);
                pz = fmin(pz, boxsize - pz);
            }
            const double d2 = (px * px + py * py) + pz * pz;
            if (!(d2 <= s2hi) || !(d2 > s2lo)) return;
            int lo = 0, hi = ns;                        // s2[lo] < d2 <= s2[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (d2 <= s2[mid]) hi = mid; else lo = mid;
            }
            int bin = lo;
            if (nmu > 0) {
                const double alos = los == 0 ? px : (los == 1 ? py : pz);
                const double mu = alos / sqrt(d2);
                if (!(mu > mulo) || !(mu <= muhi)) return;
                int ml = 0, mh = nmu;                   // me[ml] < mu <= me[mh]
                while (mh - ml > 1) {
                    const int mid = (ml + mh) >> 1;
                    if (mu <= me[mid]) mh = mid; else ml = mid;
                }
                bin = lo * nmu + ml;
            }
            atomicAdd(&whist[bin], 1u);
        });
    flush();
}

// One set in a periodic box: the topology is known when the kernel is compiled.
__global__ void __launch_bounds__(TP_BLOCK)
tp_pair_kernel(const TpObj* __restrict__ sorted, const unsigned* __restrict__ cell_start,
               const unsigned* __restrict__ tile_start, const GridBoxParams* prm, TpBins bn,
               unsigned long long* __restrict__ part) {
    tp_count_pairs(sorted, cell_start, tile_start, sorted, cell_start, prm, true, true, bn, part);
}

// Two sets (auto_pairs != 0: sorted2 / cell_start2 are set 1's own), periodic when bn.boxsize > 0.
__global__ void __launch_bounds__(TP_BLOCK)
tpx_pair_kernel(const TpObj* __restrict__ sorted1, const unsigned* __restrict__ cell_start1,
                const unsigned* __restrict__ tile_start, const TpObj* __restrict__ sorted2,
                const unsigned* __restrict__ cell_start2, const GridBoxParams* prm, int auto_pairs, TpBins bn,
                unsigned long long* __restrict__ part) {
    tp_count_pairs(sorted1, cell_start1, tile_start, sorted2, cell_start2, prm, bn.boxsize > 0.0, auto_pairs != 0, bn,
                   part);
}

// counts[bin] = sum of the TP_GRID workgroup rows, in row order.
__global__ void __launch_bounds__(256)
tp_reduce_kernel(const unsigned long long* __restrict__ part, int nbins, unsigned long long* __restrict__ counts) {
    const int bin = blockIdx.x * blockDim.x + threadIdx.x;
    if (bin >= nbins) return;
    unsigned long long sum = 0;
    for (int g = 0; g < TP_GRID; ++g) sum += part[(size_t)g * nbins + bin];
    counts[bin] = sum;
}

// The launch of the prep kernel of one non-empty set.
void tp_prep(const void* pos, int pos_dtype, const void* vel, int vel_dtype, int los, double boxsize, size_t n,
             TpObj* obj, GridBounds* box, hipStream_t s) {
    ast::dispatch_f32_f64(pos_dtype == AST_F32, vel && vel_dtype == AST_F32, [&](auto tp, auto tv) {
        using TP = decltype(tp);
        using TV = decltype(tv);
        tp_prep_kernel<TP, TV><<<ast::stream_grid(n, 256), 256, 0, s>>>((const TP*)pos, (const TV*)vel, los, boxsize, n,
                                                                         obj, box);
    });
}

// The bins of a call and the dynamic LDS of its pair kernel.  Histogram copies: one per wave where the LDS budget
// allows, else 2 or 1 shared by the waves.  AST_TPCF_FLUSH_AT (tests only): flush the LDS counters after at most this
// many pairs per stage bound.
TpBins tp_bins(double boxsize, int los, const double* s_edges, int ns, const double* mu_edges, int nmu, size_t* lds) {
    const int nbins = nbins_of(ns, nmu);
    const size_t fixed = (size_t)3 * TP_BLOCK * sizeof(double) + (size_t)(ns + 1 + nmu + 1) * sizeof(double);
    int hcopies = TP_WAVES;
    while (hcopies > 1 && fixed + (size_t)hcopies * nbins * 4 > TP_LDS) hcopies /= 2;
    *lds = fixed + (size_t)hcopies * nbins * 4;
    unsigned long long flush_at = TP_FLUSH_AT;
    if (const char* f = getenv("AST_TPCF_FLUSH_AT")) flush_at = strtoull(f, nullptr, 10);
    if (flush_at > TP_FLUSH_AT) flush_at = TP_FLUSH_AT;
    return TpBins{boxsize, los, s_edges, ns, mu_edges, nmu, hcopies, flush_at};
}

// The pair counts of a prepared workspace with pairs in it: the plan for the top s edge, the sort, the pair kernel -
// tp_pair_kernel for the one set of ast_tpcf_* (`cross` false), else tpx_pair_kernel - and the reduce.
int tp_counts(bool cross, char* ws, const GridLayout& L, const size_t* n, int auto_pairs, double boxsize, int los,
              const double* s_edges_d, int ns, const double* mu_edges_d, int nmu, int single_cell,
              unsigned long long* counts_d, hipStream_t s) {
    const int nbins = nbins_of(ns, nmu);
    const int q2 = cross && !auto_pairs ? 1 : 0;
    const GridSorted<TpObj, unsigned long long> g(ws, L, q2);
    {
        AST_PROF(cross ? "tpcf_cross_grid" : "tpcf_grid", s);
        grid_edge_plan_kernel<<<1, 64, 0, s>>>(g.prm, s_edges_d, ns, 0.0, boxsize, (unsigned)L.cap, single_cell);
        AST_CHECK_LAUNCH();
        if (int rc = grid_sort_sets<TP_BLOCK, TpObj>(ws, L, q2, n, s)) return rc;
    }
    size_t lds;
    const TpBins bn = tp_bins(boxsize, los, s_edges_d, ns, mu_edges_d, nmu, &lds);
    AST_CHECK_ARG(lds <= TP_LDS);
    {
        AST_PROF(cross ? "tpcf_cross_pairs" : "tpcf_pairs", s);
        if (cross)
            tpx_pair_kernel<<<TP_GRID, TP_BLOCK, lds, s>>>(g.sorted1, g.cell_start1, g.tile_start1, g.sorted2,
                                                           g.cell_start2, g.prm, auto_pairs, bn, g.part);
        else
            tp_pair_kernel<<<TP_GRID, TP_BLOCK, lds, s>>>(g.sorted1, g.cell_start1, g.tile_start1, g.prm, bn, g.part);
        AST_CHECK_LAUNCH();
    }
    {
        AST_PROF(cross ? "tpcf_cross_reduce" : "tpcf_reduce", s);
        tp_reduce_kernel<<<(nbins + 255) / 256, 256, 0, s>>>(g.part, nbins, counts_d);
        AST_CHECK_LAUNCH();
    }
    return AST_OK;
}

}  // namespace

extern "C" size_t ast_tpcf_workspace_bytes(size_t n, int ns, int nmu) {
    if (!bins_ok(ns, nmu)) return 0;
    return tp_layout(1, n, 0, nbins_of(ns, nmu)).total;
}

extern "C" int ast_tpcf_max_bins(void) { return TP_MAX_BINS; }

extern "C" int ast_tpcf_prepare(const void* pos_d, int pos_dtype, const void* vel_d, int vel_dtype, int los,
                                double boxsize, size_t n, void* work_d, size_t work_bytes, double* bounds_d,
                                void* stream) {
    AST_CHECK_ARG(pos_dtype == AST_F32 || pos_dtype == AST_F64);
    AST_CHECK_ARG(vel_d == nullptr || vel_dtype == AST_F32 || vel_dtype == AST_F64);
    AST_CHECK_ARG(los >= 0 && los <= 2);
    AST_CHECK_ARG(boxsize > 0.0 && std::isfinite(boxsize));
    AST_CHECK_ARG(grid_count_ok(n));
    AST_CHECK_ARG(n == 0 || pos_d);
    AST_CHECK_ARG(bounds_d);
    const GridLayout L = tp_layout(1, n, 0, 1);
    AST_CHECK_ARG(work_d && work_bytes >= L.sorted[0]);
    hipStream_t s = ast::as_stream(stream);
    return grid_prepare<1, TpObj>((char*)work_d, L, &n, bounds_d, "tpcf_prep", s, [&](int, TpObj* obj, GridBounds* box) {
        tp_prep(pos_d, pos_dtype, vel_d, vel_dtype, los, boxsize, n, obj, box, s);
    });
}

extern "C" int ast_tpcf_pair_counts(void* work_d, size_t work_bytes, size_t n, double boxsize, int los,
                                    const double* s_edges_d, int ns, const double* mu_edges_d, int nmu,
                                    int single_cell, unsigned long long* counts_d, void* stream) {
    AST_CHECK_ARG(bins_ok(ns, nmu));
    AST_CHECK_ARG(los >= 0 && los <= 2);
    AST_CHECK_ARG(boxsize > 0.0 && std::isfinite(boxsize));
    AST_CHECK_ARG(grid_count_ok(n));
    AST_CHECK_ARG(s_edges_d && (nmu == 0 || mu_edges_d) && counts_d);
    AST_CHECK_ARG(work_d && work_bytes >= ast_tpcf_workspace_bytes(n, ns, nmu));
    hipStream_t s = ast::as_stream(stream);
    const int nbins = nbins_of(ns, nmu);
    if (grid_no_pairs(1, n, 0)) {
        AST_CHECK_HIP(hipMemsetAsync(counts_d, 0, nbins * sizeof(unsigned long long), s));
        return AST_OK;
    }
    return tp_counts(false, (char*)work_d, tp_layout(1, n, 0, nbins), &n, 1, boxsize, los, s_edges_d, ns, mu_edges_d,
                     nmu, single_cell, counts_d, s);
}

// ---- two sets, periodic cube or open boundaries

extern "C" size_t ast_tpcf_cross_workspace_bytes(size_t n1, size_t n2, int ns, int nmu) {
    if (!bins_ok(ns, nmu)) return 0;
    return tp_layout(2, n1, n2, nbins_of(ns, nmu)).total;
}

extern "C" int ast_tpcf_cross_prepare(const void* pos1_d, int pos1_dtype, const void* vel1_d, int vel1_dtype,
                                      size_t n1, const void* pos2_d, int pos2_dtype, const void* vel2_d,
                                      int vel2_dtype, size_t n2, int los, double boxsize, void* work_d,
                                      size_t work_bytes, double* bounds_d, void* stream) {
    AST_CHECK_ARG(n1 == 0 || pos1_dtype == AST_F32 || pos1_dtype == AST_F64);
    AST_CHECK_ARG(n2 == 0 || pos2_dtype == AST_F32 || pos2_dtype == AST_F64);
    AST_CHECK_ARG(vel1_d == nullptr || vel1_dtype == AST_F32 || vel1_dtype == AST_F64);
    AST_CHECK_ARG(vel2_d == nullptr || vel2_dtype == AST_F32 || vel2_dtype == AST_F64);
    AST_CHECK_ARG(los >= 0 && los <= 2);
    AST_CHECK_ARG(boxsize >= 0.0 && std::isfinite(boxsize));
    AST_CHECK_ARG(grid_count_ok(n1) && grid_count_ok(n2));
    AST_CHECK_ARG((n1 == 0 || pos1_d) && (n2 == 0 || pos2_d));
    AST_CHECK_ARG(bounds_d);
    const GridLayout L = tp_layout(2, n1, n2, 1);
    AST_CHECK_ARG(work_d && work_bytes >= L.part);
    hipStream_t s = ast::as_stream(stream);
    const void* pos[2] = {pos1_d, pos2_d};
    const void* vel[2] = {vel1_d, vel2_d};
    const int pos_dtype[2] = {pos1_dtype, pos2_dtype}, vel_dtype[2] = {vel1_dtype, vel2_dtype};
    const size_t n[2] = {n1, n2};
    return grid_prepare<2, TpObj>((char*)work_d, L, n, bounds_d, "tpcf_cross_prep", s,
                                  [&](int q, TpObj* obj, GridBounds* box) {
        tp_prep(pos[q], pos_dtype[q], vel[q], vel_dtype[q], los, boxsize, n[q], obj, box, s);
    });
}

extern "C" int ast_tpcf_cross_counts(void* work_d, size_t work_bytes, size_t n1, size_t n2, int auto_pairs,
                                     double boxsize, int los, const double* s_edges_d, int ns,
                                     const double* mu_edges_d, int nmu, int single_cell,
                                     unsigned long long* counts_d, void* stream) {
    AST_CHECK_ARG(bins_ok(ns, nmu));
    AST_CHECK_ARG(los >= 0 && los <= 2);
    AST_CHECK_ARG(boxsize >= 0.0 && std::isfinite(boxsize));
    AST_CHECK_ARG(grid_count_ok(n1) && grid_count_ok(n2));
    AST_CHECK_ARG(s_edges_d && (nmu == 0 || mu_edges_d) && counts_d);
    AST_CHECK_ARG(work_d && work_bytes >= ast_tpcf_cross_workspace_bytes(n1, n2, ns, nmu));
    hipStream_t s = ast::as_stream(stream);
    const int nbins = nbins_of(ns, nmu);
    if (grid_no_pairs(auto_pairs, n1, n2)) {
        AST_CHECK_HIP(hipMemsetAsync(counts_d, 0, nbins * sizeof(unsigned long long), s));
        return AST_OK;
    }
    const size_t n[2] = {n1, n2};
    return tp_counts(true, (char*)work_d, tp_layout(2, n1, n2, nbins), n, auto_pairs, boxsize, los, s_edges_d, ns,
                     mu_edges_d, nmu, single_cell, counts_d, s);
}

