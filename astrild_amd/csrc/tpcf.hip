// Two-point correlation function (particles/hutils/tpcf.py, halotools' s_mu_tpcf / tpcf), first of one sample in a
// periodic box, then (second half of the file) of two samples in a periodic box or with open boundaries: per-object
// prep (redshift-space shift, wrap, bounds), a periodic uniform cell grid (counting sort by cell, cell_grid.h) as the
// pair finder, a tiled pair kernel that counts minimum-image pairs into an exact integer (s, mu) histogram in LDS, and a
// fixed-order sum of the workgroup rows.  All pair arithmetic is fp64 (the library is built with -ffp-contract=off).
#include "ast_common.h"
#include "cell_grid.h"
#include <cmath>
#include <cstdlib>

namespace {

constexpr int TP_BLOCK = 256;               // i objects per tile = j objects per LDS stage
constexpr int TP_WAVES = TP_BLOCK / 64;
constexpr int TP_GRID = 1024;               // persistent pair-kernel workgroups (256 CUs x 4)
constexpr size_t TP_MAX_CELLS = size_t(1) << 20;
constexpr int TP_MAX_BINS = 10000;          // ns * max(nmu, 1): 100 x 100
constexpr int TP_MAX_EDGES = 1001;          // ns + 1 and nmu + 1 each
constexpr size_t TP_LDS = 65536;            // dynamic LDS budget of the pair kernel
constexpr unsigned long long TP_FLUSH_AT = 0xffffffffull;    // 32-bit LDS counters: at most this many adds

struct TpObj { double r[3]; };

struct TpParams {
    unsigned long long kmin[3], kmax[3];    // bounds of the shifted coordinates as order-preserving keys
    double inv_cs;                          // dims / L (0 for one cell)
    int dims;                               // cells per axis
    unsigned ncells, ntiles;
};

inline size_t cells_cap(size_t n) {
    const size_t c = n < TP_MAX_CELLS ? n : TP_MAX_CELLS;
    return c < 27 ? 27 : c;
}

inline int nbins_of(int ns, int nmu) { return ns * (nmu > 0 ? nmu : 1); }

inline bool bins_ok(int ns, int nmu) {
    return ns >= 1 && ns < TP_MAX_EDGES && nmu >= 0 && nmu < TP_MAX_EDGES && nbins_of(ns, nmu) <= TP_MAX_BINS;
}

struct TpLayout {
    size_t params, cnt, cell_start, tile_start, cursor, cell_of, obj, sorted, part, total;
    TpLayout(size_t n, int nbins) {
        const size_t cap = cells_cap(n);
        size_t o = 0;
        params = o;     o += align256(sizeof(TpParams));
        cnt = o;        o += align256(cap * 4);
        cell_start = o; o += align256((cap + 1) * 4);
        tile_start = o; o += align256((cap + 1) * 4);
        cursor = o;     o += align256(cap * 4);
        cell_of = o;    o += align256(n * 4);
        obj = o;        o += align256(n * sizeof(TpObj));
        sorted = o;     o += align256(n * sizeof(TpObj));
        part = o;       o += align256((size_t)TP_GRID * (size_t)nbins * 8);
        total = o;
    }
};

// numpy's arithmetic in the input dtypes, each float32 operation done in fp64 and rounded once (exact: fp64 carries
// more than 2 x 24 + 2 bits, so the result is the correctly rounded float32 one).
template <typename T> __device__ inline T div_as(T a, double b) { return (T)((double)a / b); }
template <typename T> __device__ inline T add_as(T a, T b) { return (T)((double)a + (double)b); }
template <typename T> __device__ inline T sub_as(T a, T b) { return (T)((double)a - (double)b); }

// One thread per object, as tpcf.py:74-97: pos_s = pos; pos_s[los] += vel[los] / 100. (TV / 100 in TV, the add in
// the wider of TP and TV, stored back as TP); then pos_s[los] > L -> - L, and < 0 -> + L, in TP.  vel == nullptr: no
// shift, no wrap.  Widened to fp64 into obj; the min / max of all shifted coordinates (NaN counts as -inf / +inf) go
// to prm->kmin / kmax, one atomic per workgroup and axis.
template <typename TP, typename TV>
__global__ void __launch_bounds__(256)
tp_prep_kernel(const TP* __restrict__ pos, const TV* __restrict__ vel, int los, double boxsize, size_t n,
               TpObj* __restrict__ obj, TpParams* prm) {
    using TC = decltype(TP() + TV());
    __shared__ double wlo[3][TP_WAVES], whi[3][TP_WAVES];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const TP box = (TP)boxsize;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        TpObj o;
        for (int a = 0; a < 3; ++a) o.r[a] = (double)pos[3 * i + a];
        if (vel) {
            const TV q = div_as<TV>(vel[3 * i + los], 100.0);
            TP s = (TP)add_as<TC>((TC)pos[3 * i + los], (TC)q);
            if (s > box) s = sub_as<TP>(s, box);
            if (s < (TP)0) s = add_as<TP>(s, box);
            o.r[los] = (double)s;
        }
        obj[i] = o;
        for (int a = 0; a < 3; ++a) {
            const double v = o.r[a];
            lo[a] = fmin(lo[a], v == v ? v : -INFINITY);
            hi[a] = fmax(hi[a], v == v ? v : INFINITY);
        }
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
        for (int k = 1; k < TP_WAVES; ++k) { mn = fmin(mn, wlo[a][k]); mx = fmax(mx, whi[a][k]); }
        if (mn <= mx) {
            atomicMin(&prm->kmin[a], d2key(mn));
            atomicMax(&prm->kmax[a], d2key(mx));
        }
    }
}

// bounds[0..2] = min, bounds[3..5] = max of the shifted coordinates; (+inf, -inf) when there are no objects.
__global__ void tp_bounds_kernel(const TpParams* prm, double* __restrict__ bounds) {
    const int a = threadIdx.x;
    if (a >= 3) return;
    const unsigned long long kmn = prm->kmin[a], kmx = prm->kmax[a];
    bounds[a] = kmn > kmx ? INFINITY : key2d(kmn);
    bounds[3 + a] = kmn > kmx ? -INFINITY : key2d(kmx);
}

// One thread: cells per axis of the periodic grid, floor(L / (smax (1 + 1e-6))) with smax = the top s edge, fewer
// while the cube exceeds `cap`, at least 3 so that the 27 neighbours of a cell are distinct; one cell when even 3 would
// be narrower than the reach (smax >= L / 3, which the Python API refuses) or when `single` is set.
__global__ void tp_plan_kernel(TpParams* prm, const double* __restrict__ s_edges, int ns, double boxsize, unsigned cap,
                               int single) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int d = 1;
    const double m = floor(boxsize / (s_edges[ns] * (1.0 + 1e-6)));
    if (!single && m >= 3.0) {
        d = m > 1024.0 ? 1024 : (int)m;
        while ((unsigned long long)d * d * d > cap) --d;
    }
    prm->dims = d;
    prm->inv_cs = d > 1 ? (double)d / boxsize : 0.0;
    prm->ncells = (unsigned)(d * d * d);
}

// Cell of a coordinate in [0, L]: floor(x * dims / L), clamped to [0, dims - 1] (x == L goes to the last cell; a
// NaN to cell 0).
__device__ inline int tp_axis_cell(double x, double inv_cs, int dims) {
    double v = x * inv_cs;
    const double top = (double)(dims - 1);
    if (!(v >= 0.0)) v = 0.0;
    if (v > top) v = top;
    return (int)v;
}

__global__ void __launch_bounds__(256)
tp_count_kernel(const TpObj* __restrict__ obj, size_t n, const TpParams* prm, unsigned* __restrict__ cell_of,
                unsigned* __restrict__ cnt) {
    const int dims = prm->dims;
    const double inv_cs = prm->inv_cs;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const TpObj o = obj[i];
        const unsigned cx = tp_axis_cell(o.r[0], inv_cs, dims), cy = tp_axis_cell(o.r[1], inv_cs, dims),
                       cz = tp_axis_cell(o.r[2], inv_cs, dims);
        const unsigned c = (cz * (unsigned)dims + cy) * (unsigned)dims + cx;
        cell_of[i] = c;
        atomicAdd(&cnt[c], 1u);
    }
}

// Work item = (tile of TP_BLOCK objects of cell a, neighbour k): each thread holds one i of the tile, the j objects of
// cell a + offset[k] (wrapped periodically) pass through LDS TP_BLOCK at a time (k = 0: the cell itself, j > i only).
// dims == 1 (one cell): only k = 0.  A pair counts in bin (k, l) when s2[k] < d^2 <= s2[k + 1] and (nmu > 0)
// mu[l] < mu <= mu[l + 1], with the minimum image per axis a = min(|x_i - x_j|, L - |x_i - x_j|),
// d^2 = (a_x^2 + a_y^2) + a_z^2 and mu = a_los / sqrt(d^2); both bins by binary search on fp64 comparisons.
// Each pair adds 1 to a 32-bit LDS counter of the wave's histogram copy (hcopies copies, wave w uses w % hcopies).
// Before an LDS stage that could take a counter past flush_at pairs since the last flush, the workgroup adds its
// counters into its own 64-bit row of part (plain loads and stores: no other workgroup touches the row) and clears
// them; the row is complete after the final flush.  No global atomics.
__global__ void __launch_bounds__(TP_BLOCK)
tp_pair_kernel(const TpObj* __restrict__ sorted, const unsigned* __restrict__ cell_start,
               const unsigned* __restrict__ tile_start, const TpParams* prm, double boxsize, int los,
               const double* __restrict__ s_edges, int ns, const double* __restrict__ mu_edges, int nmu, int hcopies,
               unsigned long long flush_at, unsigned long long* __restrict__ part) {
    extern __shared__ double lds[];
    double* jr = lds;                                   // [3][TP_BLOCK]: the staged j objects
    double* s2 = jr + 3 * TP_BLOCK;                     // [ns + 1] squared s edges
    double* me = s2 + (ns + 1);                         // [nmu + 1] mu edges
    unsigned* hist = (unsigned*)(me + (nmu + 1));       // [hcopies][nbins]
    const int tid = threadIdx.x, w = tid / 64;
    const int nbins = ns * (nmu > 0 ? nmu : 1);
    for (int k = tid; k <= ns; k += TP_BLOCK) s2[k] = s_edges[k] * s_edges[k];
    for (int k = tid; k <= nmu && nmu > 0; k += TP_BLOCK) me[k] = mu_edges[k];
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

    const int dims = prm->dims;
    const unsigned ncells = prm->ncells;
    const unsigned long long nitems = (unsigned long long)prm->ntiles * GRID_NEIGH;
    __syncthreads();
    const double s2lo = s2[0], s2hi = s2[ns];
    const double mulo = nmu > 0 ? me[0] : 0.0, muhi = nmu > 0 ? me[nmu] : 0.0;
    for (unsigned long long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const unsigned tile = (unsigned)(item / GRID_NEIGH);
        const int k = (int)(item % GRID_NEIGH);
        if (dims == 1 && k != 0) continue;
        const unsigned a = grid_cell_of_tile(tile_start, ncells, tile);
        const unsigned d = (unsigned)dims;
        const int ax = (int)(a % d), ay = (int)((a / d) % d), az = (int)(a / (d * d));
        const unsigned bx = (unsigned)(ax + grid_offsets[k][0] + dims) % d;
        const unsigned by = (unsigned)(ay + grid_offsets[k][1] + dims) % d;
        const unsigned bz = (unsigned)(az + grid_offsets[k][2] + dims) % d;
        const unsigned b = (bz * d + by) * d + bx;
        const unsigned i0 = cell_start[a] + (tile - tile_start[a]) * TP_BLOCK;
        const unsigned i1 = min(i0 + TP_BLOCK, cell_start[a + 1]);
        const unsigned j0 = k == 0 ? i0 + 1 : cell_start[b];
        const unsigned j1 = cell_start[b + 1];
        if (j0 >= j1) continue;

        const unsigned i = i0 + tid;
        const bool valid = i < i1;
        TpObj oi;
        if (valid) oi = sorted[i];
        for (unsigned jc = j0; jc < j1; jc += TP_BLOCK) {
            const int m = (int)min((unsigned)TP_BLOCK, j1 - jc);
            const unsigned long long stage = (unsigned long long)(i1 - i0) * (unsigned long long)m;
            if (pending + stage > flush_at) flush();
            pending += stage;
            __syncthreads();
            if (jc + tid < j1) {
                const TpObj oj = sorted[jc + tid];
                for (int c = 0; c < 3; ++c) jr[c * TP_BLOCK + tid] = oj.r[c];
            }
            __syncthreads();
            if (!valid) continue;
            const int q0 = (k == 0 && i + 1 > jc) ? (int)min((unsigned)m, i + 1 - jc) : 0;
            for (int q = q0; q < m; ++q) {
                double px = fabs(oi.r[0] - jr[q]), py = fabs(oi.r[1] - jr[TP_BLOCK + q]),
                       pz = fabs(oi.r[2] - jr[2 * TP_BLOCK + q]);
                px = fmin(px, boxsize - px);
                py = fmin(py, boxsize - py);
                pz = fmin(pz, boxsize - pz);
                const double d2 = (px * px + py * py) + pz * pz;
                if (!(d2 <= s2hi) || !(d2 > s2lo)) continue;
                int lo = 0, hi = ns;                    // s2[lo] < d2 <= s2[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (d2 <= s2[mid]) hi = mid; else lo = mid;
                }
                int bin = lo;
                if (nmu > 0) {
                    const double alos = los == 0 ? px : (los == 1 ? py : pz);
                    const double mu = alos / sqrt(d2);
                    if (!(mu > mulo) || !(mu <= muhi)) continue;
                    int ml = 0, mh = nmu;               // me[ml] < mu <= me[mh]
                    while (mh - ml > 1) {
                        const int mid = (ml + mh) >> 1;
                        if (mu <= me[mid]) mh = mid; else ml = mid;
                    }
                    bin = lo * nmu + ml;
                }
                atomicAdd(&whist[bin], 1u);
            }
        }
    }
    flush();
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

template <typename TP, typename TV>
void launch_prep(const void* pos, const void* vel, int los, double boxsize, size_t n, TpObj* obj, TpParams* prm,
                 hipStream_t s) {
    tp_prep_kernel<TP, TV><<<ast::stream_grid(n, 256), 256, 0, s>>>((const TP*)pos, (const TV*)vel, los, boxsize, n,
                                                                     obj, prm);
}

}  // namespace

extern "C" size_t ast_tpcf_workspace_bytes(size_t n, int ns, int nmu) {
    if (!bins_ok(ns, nmu)) return 0;
    return TpLayout(n, nbins_of(ns, nmu)).total;
}

extern "C" int ast_tpcf_max_bins(void) { return TP_MAX_BINS; }

extern "C" int ast_tpcf_prepare(const void* pos_d, int pos_dtype, const void* vel_d, int vel_dtype, int los,
                                double boxsize, size_t n, void* work_d, size_t work_bytes, double* bounds_d,
                                void* stream) {
    AST_CHECK_ARG(pos_dtype == AST_F32 || pos_dtype == AST_F64);
    AST_CHECK_ARG(vel_d == nullptr || vel_dtype == AST_F32 || vel_dtype == AST_F64);
    AST_CHECK_ARG(los >= 0 && los <= 2);
    AST_CHECK_ARG(boxsize > 0.0 && std::isfinite(boxsize));
    AST_CHECK_ARG(n < (size_t(1) << 31));
    AST_CHECK_ARG(n == 0 || pos_d);
    AST_CHECK_ARG(bounds_d);
    const TpLayout L(n, 1);
    AST_CHECK_ARG(work_d && work_bytes >= L.obj + align256(n * sizeof(TpObj)));
    hipStream_t s = ast::as_stream(stream);
    char* ws = (char*)work_d;
    TpParams* prm = (TpParams*)(ws + L.params);
    AST_CHECK_HIP(hipMemsetAsync(prm->kmin, 0xff, sizeof(prm->kmin), s));
    AST_CHECK_HIP(hipMemsetAsync(prm->kmax, 0x00, sizeof(prm->kmax), s));
    if (n > 0) {
        AST_PROF("tpcf_prep", s);
        TpObj* obj = (TpObj*)(ws + L.obj);
        const bool v32 = vel_d && vel_dtype == AST_F32;
        if (pos_dtype == AST_F32 && v32)
            launch_prep<float, float>(pos_d, vel_d, los, boxsize, n, obj, prm, s);
        else if (pos_dtype == AST_F32)
            launch_prep<float, double>(pos_d, vel_d, los, boxsize, n, obj, prm, s);
        else if (v32)
            launch_prep<double, float>(pos_d, vel_d, los, boxsize, n, obj, prm, s);
        else
            launch_prep<double, double>(pos_d, vel_d, los, boxsize, n, obj, prm, s);
        AST_CHECK_LAUNCH();
    }
    tp_bounds_kernel<<<1, 64, 0, s>>>(prm, bounds_d);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

extern "C" int ast_tpcf_pair_counts(void* work_d, size_t work_bytes, size_t n, double boxsize, int los,
                                    const double* s_edges_d, int ns, const double* mu_edges_d, int nmu,
                                    int single_cell, unsigned long long* counts_d, void* stream) {
    AST_CHECK_ARG(bins_ok(ns, nmu));
    AST_CHECK_ARG(los >= 0 && los <= 2);
    AST_CHECK_ARG(boxsize > 0.0 && std::isfinite(boxsize));
    AST_CHECK_ARG(n < (size_t(1) << 31));
    AST_CHECK_ARG(s_edges_d && (nmu == 0 || mu_edges_d) && counts_d);
    AST_CHECK_ARG(work_d && work_bytes >= ast_tpcf_workspace_bytes(n, ns, nmu));
    hipStream_t s = ast::as_stream(stream);
    const int nbins = nbins_of(ns, nmu);
    if (n < 2) {
        AST_CHECK_HIP(hipMemsetAsync(counts_d, 0, nbins * sizeof(unsigned long long), s));
        return AST_OK;
    }
    const TpLayout L(n, nbins);
    char* ws = (char*)work_d;
    TpParams* prm = (TpParams*)(ws + L.params);
    unsigned* cnt = (unsigned*)(ws + L.cnt);
    unsigned* cell_start = (unsigned*)(ws + L.cell_start);
    unsigned* tile_start = (unsigned*)(ws + L.tile_start);
    unsigned* cursor = (unsigned*)(ws + L.cursor);
    unsigned* cell_of = (unsigned*)(ws + L.cell_of);
    const TpObj* obj = (const TpObj*)(ws + L.obj);
    TpObj* sorted = (TpObj*)(ws + L.sorted);
    unsigned long long* part = (unsigned long long*)(ws + L.part);
    const size_t cap = cells_cap(n);
    {
        AST_PROF("tpcf_grid", s);
        tp_plan_kernel<<<1, 64, 0, s>>>(prm, s_edges_d, ns, boxsize, (unsigned)cap, single_cell);
        AST_CHECK_LAUNCH();
        AST_CHECK_HIP(hipMemsetAsync(cnt, 0, cap * 4, s));
        tp_count_kernel<<<ast::stream_grid(n, 256), 256, 0, s>>>(obj, n, prm, cell_of, cnt);
        AST_CHECK_LAUNCH();
        grid_scan_kernel<TP_BLOCK><<<1, 1024, 0, s>>>(cnt, prm, cell_start, tile_start, cursor);
        AST_CHECK_LAUNCH();
        grid_scatter_kernel<<<ast::stream_grid(n, 256), 256, 0, s>>>(obj, n, cell_of, cursor, sorted);
        AST_CHECK_LAUNCH();
    }
    // Histogram copies: one per wave where the LDS budget allows, else 2 or 1 shared by the waves.
    const size_t fixed = (size_t)3 * TP_BLOCK * sizeof(double) + (size_t)(ns + 1 + nmu + 1) * sizeof(double);
    int hcopies = TP_WAVES;
    while (hcopies > 1 && fixed + (size_t)hcopies * nbins * 4 > TP_LDS) hcopies /= 2;
    const size_t lds = fixed + (size_t)hcopies * nbins * 4;
    AST_CHECK_ARG(lds <= TP_LDS);
    // AST_TPCF_FLUSH_AT (tests only): flush the LDS counters after at most this many pairs per stage bound.
    unsigned long long flush_at = TP_FLUSH_AT;
    if (const char* f = getenv("AST_TPCF_FLUSH_AT")) flush_at = strtoull(f, nullptr, 10);
    if (flush_at > TP_FLUSH_AT) flush_at = TP_FLUSH_AT;
    {
        AST_PROF("tpcf_pairs", s);
        tp_pair_kernel<<<TP_GRID, TP_BLOCK, lds, s>>>(sorted, cell_start, tile_start, prm, boxsize, los, s_edges_d,
                                                      ns, mu_edges_d, nmu, hcopies, flush_at, part);
        AST_CHECK_LAUNCH();
    }
    {
        AST_PROF("tpcf_reduce", s);
        tp_reduce_kernel<<<(nbins + 255) / 256, 256, 0, s>>>(part, nbins, counts_d);
        AST_CHECK_LAUNCH();
    }
    return AST_OK;
}

// ---- two sets, periodic cube or open boundaries (ast_tpcf_cross_prepare / ast_tpcf_cross_counts)
namespace {

constexpr int TPX_NEIGH = 27;               // cross pairs: the cell itself and all 26 neighbours

inline size_t tpx_cells_cap(size_t n1, size_t n2) { return cells_cap(n1 > n2 ? n1 : n2); }

// One grid (GridBoxParams) shared by both sets; per set its own bounds (TpParams, only kmin / kmax used), counts,
// cell starts, cell numbers, fp64 objects and their cell-sorted copy.  Only set 1 has tiles; tile_start[1] is where
// the scan of set 2 puts the tile list nobody reads.  Everything before `part` is independent of the bin counts.
struct TpxLayout {
    size_t grid, set_prm[2], cnt[2], cell_start[2], tile_start[2], cursor, cell_of[2], obj[2], sorted[2], part, total;
    TpxLayout(size_t n1, size_t n2, int nbins) {
        const size_t cap = tpx_cells_cap(n1, n2);
        const size_t n[2] = {n1, n2};
        size_t o = 0;
        grid = o; o += align256(sizeof(GridBoxParams));
        for (int s = 0; s < 2; ++s) {
            set_prm[s] = o;    o += align256(sizeof(TpParams));
            cnt[s] = o;        o += align256(cap * 4);
            cell_start[s] = o; o += align256((cap + 1) * 4);
            tile_start[s] = o; o += align256((cap + 1) * 4);
            cell_of[s] = o;    o += align256(n[s] * 4);
            obj[s] = o;        o += align256(n[s] * sizeof(TpObj));
            sorted[s] = o;     o += align256(n[s] * sizeof(TpObj));
        }
        cursor = o; o += align256(cap * 4);
        part = o;   o += align256((size_t)TP_GRID * (size_t)nbins * 8);
        total = o;
    }
};

// bounds[6 s + 0..2] = min, bounds[6 s + 3..5] = max of set s (as tp_bounds_kernel); the union of both boxes goes to
// the shared grid's kmin / kmax (an empty set leaves the other's box; both empty: kmin > kmax, and nothing is planned).
__global__ void tpx_bounds_kernel(const TpParams* prm1, const TpParams* prm2, GridBoxParams* grid,
                                  double* __restrict__ bounds) {
    const int a = threadIdx.x;
    if (a >= 3) return;
    const TpParams* prm[2] = {prm1, prm2};
    unsigned long long umn = ~0ull, umx = 0ull;
    for (int s = 0; s < 2; ++s) {
        const unsigned long long kmn = prm[s]->kmin[a], kmx = prm[s]->kmax[a];
        bounds[6 * s + a] = kmn > kmx ? INFINITY : key2d(kmn);
        bounds[6 * s + 3 + a] = kmn > kmx ? -INFINITY : key2d(kmx);
        umn = kmn < umn ? kmn : umn;
        umx = kmx > umx ? kmx : umx;
    }
    grid->kmin[a] = umn;
    grid->kmax[a] = umx;
}

// One thread: the shared grid.  boxsize > 0: tp_plan_kernel's periodic plan (dims cells per axis from the origin,
// >= 3 or one cell); boxsize == 0: grid_box_plan over the union bounding box, per-axis dims that may be 1.
__global__ void tpx_plan_kernel(GridBoxParams* prm, const double* __restrict__ s_edges, int ns, double boxsize,
                                unsigned cap, int single) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!(boxsize > 0.0)) {
        grid_box_plan(prm, s_edges[ns], cap, single);
        return;
    }
    int d = 1;
    const double m = floor(boxsize / (s_edges[ns] * (1.0 + 1e-6)));
    if (!single && m >= 3.0) {
        d = m > 1024.0 ? 1024 : (int)m;
        while ((unsigned long long)d * d * d > cap) --d;
    }
    for (int a = 0; a < 3; ++a) {
        prm->lo[a] = 0.0;
        prm->dims[a] = d;
        prm->inv_cs[a] = d > 1 ? (double)d / boxsize : 0.0;
    }
    prm->ncells = (unsigned)(d * d * d);
}

// tp_pair_kernel for two sets.  Work item = (tile of TP_BLOCK set-1 objects of cell a, neighbour k); the j objects are
// those of set 2 in cell a + offset[k], staged through LDS TP_BLOCK at a time.
//   auto_pairs == 0: k over all 27 offsets, every (i, j) once.
//   auto_pairs != 0: sorted2 / cell_start2 are set 1's own; k over the 14 half-shell offsets, j > i at k = 0.
//   boxsize > 0: minimum image, neighbours wrap (dims >= 3 on every axis, or one cell: offset 0 only).
//   boxsize == 0: a = |dx|, a neighbour outside [0, dims) on any axis is skipped.
// Bins, LDS counters, flushes and the workgroup rows are tp_pair_kernel's.
__global__ void __launch_bounds__(TP_BLOCK)
tpx_pair_kernel(const TpObj* __restrict__ sorted1, const unsigned* __restrict__ cell_start1,
                const unsigned* __restrict__ tile_start, const TpObj* __restrict__ sorted2,
                const unsigned* __restrict__ cell_start2, const GridBoxParams* prm, double boxsize, int auto_pairs,
                int los, const double* __restrict__ s_edges, int ns, const double* __restrict__ mu_edges, int nmu,
                int hcopies, unsigned long long flush_at, unsigned long long* __restrict__ part) {
    extern __shared__ double lds[];
    double* jr = lds;                                   // [3][TP_BLOCK]: the staged j objects
    double* s2 = jr + 3 * TP_BLOCK;                     // [ns + 1] squared s edges
    double* me = s2 + (ns + 1);                         // [nmu + 1] mu edges
    unsigned* hist = (unsigned*)(me + (nmu + 1));       // [hcopies][nbins]
    const int tid = threadIdx.x, w = tid / 64;
    const int nbins = ns * (nmu > 0 ? nmu : 1);
    for (int k = tid; k <= ns; k += TP_BLOCK) s2[k] = s_edges[k] * s_edges[k];
    for (int k = tid; k <= nmu && nmu > 0; k += TP_BLOCK) me[k] = mu_edges[k];
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

    const bool periodic = boxsize > 0.0;
    const int dims[3] = {prm->dims[0], prm->dims[1], prm->dims[2]};
    const unsigned ncells = prm->ncells;
    const int nneigh = auto_pairs ? GRID_NEIGH : TPX_NEIGH;
    const unsigned long long nitems = (unsigned long long)prm->ntiles * (unsigned long long)nneigh;
    __syncthreads();
    const double s2lo = s2[0], s2hi = s2[ns];
    const double mulo = nmu > 0 ? me[0] : 0.0, muhi = nmu > 0 ? me[nmu] : 0.0;
    for (unsigned long long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const unsigned tile = (unsigned)(item / (unsigned)nneigh);
        const int k = (int)(item % (unsigned)nneigh);
        int off[3];
        if (auto_pairs) {
            for (int c = 0; c < 3; ++c) off[c] = grid_offsets[k][c];
        } else {
            off[0] = k % 3 - 1; off[1] = (k / 3) % 3 - 1; off[2] = k / 9 - 1;
        }
        const unsigned a = grid_cell_of_tile(tile_start, ncells, tile);
        const int ac[3] = {(int)(a % (unsigned)dims[0]), (int)((a / (unsigned)dims[0]) % (unsigned)dims[1]),
                           (int)(a / ((unsigned)dims[0] * (unsigned)dims[1]))};
        int bc[3];
        bool skip = false;
        for (int c = 0; c < 3; ++c) {
            int v = ac[c] + off[c];
            if (periodic && dims[c] >= 3) v = (v + dims[c]) % dims[c];
            else if (v < 0 || v >= dims[c]) skip = true;    // open boundary, or the one cell of a periodic box
            bc[c] = v;
        }
        if (skip) continue;
        const unsigned b = ((unsigned)bc[2] * (unsigned)dims[1] + (unsigned)bc[1]) * (unsigned)dims[0] + (unsigned)bc[0];
        const bool self = auto_pairs && k == 0;
        const unsigned i0 = cell_start1[a] + (tile - tile_start[a]) * TP_BLOCK;
        const unsigned i1 = min(i0 + TP_BLOCK, cell_start1[a + 1]);
        const unsigned j0 = self ? i0 + 1 : cell_start2[b];
        const unsigned j1 = cell_start2[b + 1];
        if (j0 >= j1) continue;

        const unsigned i = i0 + tid;
        const bool valid = i < i1;
        TpObj oi;
        if (valid) oi = sorted1[i];
        for (unsigned jc = j0; jc < j1; jc += TP_BLOCK) {
            const int m = (int)min((unsigned)TP_BLOCK, j1 - jc);
            const unsigned long long stage = (unsigned long long)(i1 - i0) * (unsigned long long)m;
            if (pending + stage > flush_at) flush();
            pending += stage;
            __syncthreads();
            if (jc + tid < j1) {
                const TpObj oj = sorted2[jc + tid];
                for (int c = 0; c < 3; ++c) jr[c * TP_BLOCK + tid] = oj.r[c];
            }
            __syncthreads();
            if (!valid) continue;
            const int q0 = (self && i + 1 > jc) ? (int)min((unsigned)m, i + 1 - jc) : 0;
            for (int q = q0; q < m; ++q) {
                double px = fabs(oi.r[0] - jr[q]), py = fabs(oi.r[1] - jr[TP_BLOCK + q]),
                       pz = fabs(oi.r[2] - jr[2 * TP_BLOCK + q]);
                if (periodic) {
                    px = fmin(px, boxsize - px);
                    py = fmin(py, boxsize - py);
                    pz = fmin(pz, boxsize - pz);
                }
                const double d2 = (px * px + py * py) + pz * pz;
                if (!(d2 <= s2hi) || !(d2 > s2lo)) continue;
                int lo = 0, hi = ns;                    // s2[lo] < d2 <= s2[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (d2 <= s2[mid]) hi = mid; else lo = mid;
                }
                int bin = lo;
                if (nmu > 0) {
                    const double alos = los == 0 ? px : (los == 1 ? py : pz);
                    const double mu = alos / sqrt(d2);
                    if (!(mu > mulo) || !(mu <= muhi)) continue;
                    int ml = 0, mh = nmu;               // me[ml] < mu <= me[mh]
                    while (mh - ml > 1) {
                        const int mid = (ml + mh) >> 1;
                        if (mu <= me[mid]) mh = mid; else ml = mid;
                    }
                    bin = lo * nmu + ml;
                }
                atomicAdd(&whist[bin], 1u);
            }
        }
    }
    flush();
}

int tpx_prep(const void* pos, int pos_dtype, const void* vel, int vel_dtype, int los, double boxsize, size_t n,
             TpObj* obj, TpParams* prm, hipStream_t s) {
    AST_CHECK_HIP(hipMemsetAsync(prm->kmin, 0xff, sizeof(prm->kmin), s));
    AST_CHECK_HIP(hipMemsetAsync(prm->kmax, 0x00, sizeof(prm->kmax), s));
    if (n == 0) return AST_OK;
    const bool v32 = vel && vel_dtype == AST_F32;
    if (pos_dtype == AST_F32 && v32)
        launch_prep<float, float>(pos, vel, los, boxsize, n, obj, prm, s);
    else if (pos_dtype == AST_F32)
        launch_prep<float, double>(pos, vel, los, boxsize, n, obj, prm, s);
    else if (v32)
        launch_prep<double, float>(pos, vel, los, boxsize, n, obj, prm, s);
    else
        launch_prep<double, double>(pos, vel, los, boxsize, n, obj, prm, s);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

}  // namespace

extern "C" size_t ast_tpcf_cross_workspace_bytes(size_t n1, size_t n2, int ns, int nmu) {
    if (!bins_ok(ns, nmu)) return 0;
    return TpxLayout(n1, n2, nbins_of(ns, nmu)).total;
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
    AST_CHECK_ARG(n1 < (size_t(1) << 31) && n2 < (size_t(1) << 31));
    AST_CHECK_ARG((n1 == 0 || pos1_d) && (n2 == 0 || pos2_d));
    AST_CHECK_ARG(bounds_d);
    const TpxLayout L(n1, n2, 1);
    AST_CHECK_ARG(work_d && work_bytes >= L.part);
    hipStream_t s = ast::as_stream(stream);
    char* ws = (char*)work_d;
    TpParams* prm1 = (TpParams*)(ws + L.set_prm[0]);
    TpParams* prm2 = (TpParams*)(ws + L.set_prm[1]);
    {
        // boxsize == 0 (open): tp_prep_kernel's wrap subtracts or adds 0, which changes nothing
        AST_PROF("tpcf_cross_prep", s);
        int rc = tpx_prep(pos1_d, pos1_dtype, vel1_d, vel1_dtype, los, boxsize, n1, (TpObj*)(ws + L.obj[0]), prm1, s);
        if (rc != AST_OK) return rc;
        rc = tpx_prep(pos2_d, pos2_dtype, vel2_d, vel2_dtype, los, boxsize, n2, (TpObj*)(ws + L.obj[1]), prm2, s);
        if (rc != AST_OK) return rc;
    }
    tpx_bounds_kernel<<<1, 64, 0, s>>>(prm1, prm2, (GridBoxParams*)(ws + L.grid), bounds_d);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

extern "C" int ast_tpcf_cross_counts(void* work_d, size_t work_bytes, size_t n1, size_t n2, int auto_pairs,
                                     double boxsize, int los, const double* s_edges_d, int ns,
                                     const double* mu_edges_d, int nmu, int single_cell,
                                     unsigned long long* counts_d, void* stream) {
    AST_CHECK_ARG(bins_ok(ns, nmu));
    AST_CHECK_ARG(los >= 0 && los <= 2);
    AST_CHECK_ARG(boxsize >= 0.0 && std::isfinite(boxsize));
    AST_CHECK_ARG(n1 < (size_t(1) << 31) && n2 < (size_t(1) << 31));
    AST_CHECK_ARG(s_edges_d && (nmu == 0 || mu_edges_d) && counts_d);
    AST_CHECK_ARG(work_d && work_bytes >= ast_tpcf_cross_workspace_bytes(n1, n2, ns, nmu));
    hipStream_t s = ast::as_stream(stream);
    const int nbins = nbins_of(ns, nmu);
    if (auto_pairs ? n1 < 2 : (n1 == 0 || n2 == 0)) {
        AST_CHECK_HIP(hipMemsetAsync(counts_d, 0, nbins * sizeof(unsigned long long), s));
        return AST_OK;
    }
    const TpxLayout L(n1, n2, nbins);
    char* ws = (char*)work_d;
    GridBoxParams* prm = (GridBoxParams*)(ws + L.grid);
    unsigned* cursor = (unsigned*)(ws + L.cursor);
    unsigned long long* part = (unsigned long long*)(ws + L.part);
    const size_t cap = tpx_cells_cap(n1, n2);
    const size_t n[2] = {n1, n2};
    {
        AST_PROF("tpcf_cross_grid", s);
        tpx_plan_kernel<<<1, 64, 0, s>>>(prm, s_edges_d, ns, boxsize, (unsigned)cap, single_cell);
        AST_CHECK_LAUNCH();
        // set 2 first: the scan of set 1 then leaves its tile count in prm->ntiles
        for (int q = auto_pairs ? 0 : 1; q >= 0; --q) {
            unsigned* cnt = (unsigned*)(ws + L.cnt[q]);
            unsigned* cell_of = (unsigned*)(ws + L.cell_of[q]);
            const TpObj* obj = (const TpObj*)(ws + L.obj[q]);
            AST_CHECK_HIP(hipMemsetAsync(cnt, 0, cap * 4, s));
            grid_box_count_kernel<<<ast::stream_grid(n[q], 256), 256, 0, s>>>(obj, n[q], prm, cell_of, cnt);
            AST_CHECK_LAUNCH();
            grid_scan_kernel<TP_BLOCK><<<1, 1024, 0, s>>>(cnt, prm, (unsigned*)(ws + L.cell_start[q]),
                                                          (unsigned*)(ws + L.tile_start[q]), cursor);
            AST_CHECK_LAUNCH();
            grid_scatter_kernel<<<ast::stream_grid(n[q], 256), 256, 0, s>>>(obj, n[q], cell_of, cursor,
                                                                             (TpObj*)(ws + L.sorted[q]));
            AST_CHECK_LAUNCH();
        }
    }
    const int q2 = auto_pairs ? 0 : 1;
    const size_t fixed = (size_t)3 * TP_BLOCK * sizeof(double) + (size_t)(ns + 1 + nmu + 1) * sizeof(double);
    int hcopies = TP_WAVES;
    while (hcopies > 1 && fixed + (size_t)hcopies * nbins * 4 > TP_LDS) hcopies /= 2;
    const size_t lds = fixed + (size_t)hcopies * nbins * 4;
    AST_CHECK_ARG(lds <= TP_LDS);
    unsigned long long flush_at = TP_FLUSH_AT;
    if (const char* f = getenv("AST_TPCF_FLUSH_AT")) flush_at = strtoull(f, nullptr, 10);
    if (flush_at > TP_FLUSH_AT) flush_at = TP_FLUSH_AT;
    {
        AST_PROF("tpcf_cross_pairs", s);
        tpx_pair_kernel<<<TP_GRID, TP_BLOCK, lds, s>>>(
            (const TpObj*)(ws + L.sorted[0]), (const unsigned*)(ws + L.cell_start[0]),
            (const unsigned*)(ws + L.tile_start[0]), (const TpObj*)(ws + L.sorted[q2]),
            (const unsigned*)(ws + L.cell_start[q2]), prm, boxsize, auto_pairs, los, s_edges_d, ns, mu_edges_d, nmu,
            hcopies, flush_at, part);
        AST_CHECK_LAUNCH();
    }
    {
        AST_PROF("tpcf_cross_reduce", s);
        tp_reduce_kernel<<<(nbins + 255) / 256, 256, 0, s>>>(part, nbins, counts_d);
        AST_CHECK_LAUNCH();
    }
    return AST_OK;
}
