// Two-point correlation function (particles/hutils/tpcf.py, halotools' s_mu_tpcf / tpcf) of one sample in a periodic
// box, or of two samples in a periodic box or with open boundaries: per-object prep (redshift-space shift, wrap,
// bounds), the uniform cell grid of cell_grid.h (counting sort by cell) as the pair finder, a tiled pair kernel that
// counts minimum-image pairs into an exact integer (s, mu) histogram in LDS, and a fixed-order sum of the workgroup
// rows.  The same kernels, compiled for another pair geometry, count (r_p, pi) bins across and along the line of sight
// (ast_rppi_*: halotools' rp_pi_tpcf / wp), on a grid planned with a reach per axis.  For jackknife errors (ast_tpcf_jk_*) every object also carries a region tag, and the same walk counts the pair
// ends per (region, bin) instead, from which all leave-one-region-out counts follow as integers.  All pair arithmetic
// is fp64 (the library is built with -ffp-contract=off).
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
struct TjObj { double r[3]; unsigned tag; };    // jackknife: the region of the object, 0 .. nsub - 1

// The jackknife's own limits: the endpoint table [nsub][nbins] has at most TJ_MAX_TABLE counters (32 MiB of 64-bit
// counts); it is kept in LDS, up to TJ_LDS bytes with the fixed part, in wave copies while those fit TJ_LDS_COPIES:
// measured at 125 x 20 counters (jackknife), four copies (47 KiB, three workgroups per CU) take 1.8 x the time of
// two (27 KiB, five per CU) or one, which are equal - the walk needs the waves more than the counters need the copies.
constexpr int TJ_MAX_TABLE = 1 << 22;
constexpr size_t TJ_LDS = 160 * 1024;
constexpr size_t TJ_LDS_COPIES = 32 * 1024;

struct TpNoTag {
    __device__ void set(TpObj&, size_t) const {}
};

// The region of an object.  tags != nullptr: the caller's, and one outside [0, ntot) sets *bad and becomes region 0 (so
// no kernel ever indexes past the table).  Else from the shifted position: i_a = floor((x_a - lo_a) / dl_a), a true
// fp64 division, clamped to [0, nsub_a - 1] on both sides (NaN: 0), and tag = (i_x nsub_y + i_y) nsub_z + i_z.
struct TjTagging {
    const int* tags;
    int nsub[3], ntot;
    double lo[3], dl[3];
    double* bad;
    __device__ void set(TjObj& o, size_t i) const {
        if (tags) {
            const int t = tags[i];
            if (t < 0 || t >= ntot) *bad = 1.0;
            o.tag = t < 0 || t >= ntot ? 0u : (unsigned)t;
            return;
        }
        unsigned tag = 0;
        for (int a = 0; a < 3; ++a) {
            double v = floor((o.r[a] - lo[a]) / dl[a]);
            const double top = (double)(nsub[a] - 1);
            if (!(v >= 0.0)) v = 0.0;
            if (v > top) v = top;
            tag = tag * (unsigned)nsub[a] + (unsigned)v;
        }
        o.tag = tag;
    }
};

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
// Obj: TpObj, or TjObj with tg.set(o, i) giving the record its jackknife region from the shifted position.
template <typename TP, typename TV, typename Obj, typename Tagging>
__global__ void __launch_bounds__(256)
tp_prep_kernel(const TP* __restrict__ pos, const TV* __restrict__ vel, int los, double boxsize, size_t n,
               Obj* __restrict__ obj, GridBounds* box, Tagging tg) {
    using TC = decltype(TP() + TV());
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const TP bx = (TP)boxsize;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        Obj o;
        for (int a = 0; a < 3; ++a) o.r[a] = (double)pos[3 * i + a];
        if (vel) {
            const TV q = div_as<TV>(vel[3 * i + los], 100.0);
            TP s = (TP)add_as<TC>((TC)pos[3 * i + los], (TC)q);
            if (s > bx) s = sub_as<TP>(s, bx);
            if (s < (TP)0) s = add_as<TP>(s, bx);
            o.r[los] = (double)s;
        }
        tg.set(o, i);
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

// The outer edges of both axes, read once per workgroup from the LDS copies of the edges.
struct TpRange {
    double s2lo, s2hi, mulo, muhi;
    __device__ TpRange(const double* s2, int ns, const double* me, int nmu)
        : s2lo(s2[0]), s2hi(s2[ns]), mulo(nmu > 0 ? me[0] : 0.0), muhi(nmu > 0 ? me[nmu] : 0.0) {}
};

// The bin of one pair, for every pair kernel of this file, or -1 when it counts nowhere.  A pair counts in bin (k, l)
// when s2[k] < d^2 <= s2[k + 1] and (nmu > 0) mu[l] < mu <= mu[l + 1], with a = |x_i - x_j| per axis, periodic: the
// minimum image a = min(a, L - a), d^2 = (a_x^2 + a_y^2) + a_z^2 and mu = a_los / sqrt(d^2); both bins by binary
// search on fp64 comparisons.  s2 (ns + 1 squared s edges) and me (nmu + 1 mu edges) are in LDS.
__device__ __forceinline__ int tp_pair_bin(const double (&ri)[3], double xj, double yj, double zj, bool periodic,
                                           double boxsize, int los, const double* s2, int ns, const double* me, int nmu,
                                           const TpRange& rg) {
    double px = fabs(ri[0] - xj), py = fabs(ri[1] - yj), pz = fabs(ri[2] - zj);
    if (periodic) {
        px = fmin(px, boxsize - px);
        py = fmin(py, boxsize - py);
        pz = fmin(pz, boxsize - pz);
    }
    const double d2 = (px * px + py * py) + pz * pz;
    if (!(d2 <= rg.s2hi) || !(d2 > rg.s2lo)) return -1;
    int lo = 0, hi = ns;                                // s2[lo] < d2 <= s2[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (d2 <= s2[mid]) hi = mid; else lo = mid;
    }
    if (nmu <= 0) return lo;
    const double alos = los == 0 ? px : (los == 1 ? py : pz);
    const double mu = alos / sqrt(d2);
    if (!(mu > rg.mulo) || !(mu <= rg.muhi)) return -1;
    int ml = 0, mh = nmu;                               // me[ml] < mu <= me[mh]
    while (mh - ml > 1) {
        const int mid = (ml + mh) >> 1;
        if (mu <= me[mid]) mh = mid; else ml = mid;
    }
    return lo * nmu + ml;
}

// The geometry of a pair kernel, a compile-time parameter: (s, mu) bins of tp_pair_bin, or (r_p, pi) bins of
// tp_rppi_bin (ast_rppi_*), where TpBins' s_edges / ns are the r_p edges and mu_edges / nmu (> 0) the pi edges.
enum TpGeom { TP_SMU = 0, TP_RPPI = 1 };

// The axes a < b other than los.
__device__ __forceinline__ int tp_axis_a(int los) { return los == 0 ? 1 : 0; }
__device__ __forceinline__ int tp_axis_b(int los) { return los == 2 ? 1 : 2; }

// The (r_p, pi) bin of one pair, or -1 when it counts nowhere.  Both objects come with their axes in the order
// (a, b, los), a < b the axes other than the line of sight (the kernels permute on load).  p_c = |x_i - x_j| per axis,
// periodic: p_c = min(p_c, L - p_c), tp_pair_bin's arithmetic; rp2 = p_a p_a + p_b p_b (the operand order of
// pair_velocity.hip's AST_PAIRVEL_LOS) and pi = p_los.  A pair counts in bin (k, l) when s2[k] < rp2 <= s2[k + 1] and
// me[l] < pi <= me[l + 1]: s2 the nrp + 1 squared r_p edges, me the npi + 1 pi edges as given, both in LDS, both
// bins by binary search on fp64 comparisons.
__device__ __forceinline__ int tp_rppi_bin(const double (&ri)[3], double aj, double bj, double lj, bool periodic,
                                           double boxsize, const double* s2, int nrp, const double* me, int npi,
                                           const TpRange& rg) {
    double pa = fabs(ri[0] - aj), pb = fabs(ri[1] - bj), pl = fabs(ri[2] - lj);
    if (periodic) {
        pa = fmin(pa, boxsize - pa);
        pb = fmin(pb, boxsize - pb);
        pl = fmin(pl, boxsize - pl);
    }
    const double rp2 = pa * pa + pb * pb;
    if (!(rp2 <= rg.s2hi) || !(rp2 > rg.s2lo) || !(pl <= rg.muhi) || !(pl > rg.mulo)) return -1;
    int lo = 0, hi = nrp;                               // s2[lo] < rp2 <= s2[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rp2 <= s2[mid]) hi = mid; else lo = mid;
    }
    int ml = 0, mh = npi;                               // me[ml] < pl <= me[mh]
    while (mh - ml > 1) {
        const int mid = (ml + mh) >> 1;
        if (pl <= me[mid]) mh = mid; else ml = mid;
    }
    return lo * npi + ml;
}

// The bin of the pair (i, staged j in slot q) in the geometry GEOM; for TP_RPPI ri and the stage hold (a, b, los).
template <int GEOM>
__device__ __forceinline__ int tp_bin_of(const double (&ri)[3], const double* jr, int q, bool periodic, double boxsize,
                                         int los, const double* s2, int ns, const double* me, int nmu,
                                         const TpRange& rg) {
    if (GEOM == TP_RPPI)
        return tp_rppi_bin(ri, jr[q], jr[TP_BLOCK + q], jr[2 * TP_BLOCK + q], periodic, boxsize, s2, ns, me, nmu, rg);
    return tp_pair_bin(ri, jr[q], jr[TP_BLOCK + q], jr[2 * TP_BLOCK + q], periodic, boxsize, los, s2, ns, me, nmu, rg);
}

// A record's position as a pair kernel of geometry GEOM holds it: as stored, or for TP_RPPI in the order (a, b, los).
template <int GEOM>
__device__ __forceinline__ void tp_axes(const double (&r)[3], int los, double (&out)[3]) {
    if (GEOM == TP_RPPI) {
        const int la = tp_axis_a(los), lb = tp_axis_b(los);
        out[0] = la == 0 ? r[0] : r[1];
        out[1] = lb == 1 ? r[1] : r[2];
        out[2] = los == 0 ? r[0] : (los == 1 ? r[1] : r[2]);
    } else {
        for (int c = 0; c < 3; ++c) out[c] = r[c];
    }
}

// The walk of cell_grid.h (grid_pair_walk) with the positions of the staged j objects in LDS; `periodic` and
// `auto_pairs` as there; the bin of a pair is tp_pair_bin's, or tp_rppi_bin's for GEOM = TP_RPPI.
// Each pair adds 1 to a 32-bit LDS counter of the wave's histogram copy (hcopies copies, wave w uses w % hcopies).
// Before an LDS stage that could take a counter past flush_at pairs since the last flush, the workgroup adds its
// counters into its own 64-bit row of part (plain loads and stores: no other workgroup touches the row) and clears
// them; the row is complete after the final flush.  No global atomics.
template <int GEOM>
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
    const TpRange rg(s2, ns, me, nmu);
    TpObj oi;
    grid_pair_walk<TP_BLOCK>(
        cell_start1, tile_start, cell_start2, prm, periodic, auto_pairs,
        [&](unsigned i) { tp_axes<GEOM>(sorted1[i].r, los, oi.r); },
        [&](unsigned ni, int m) {
            const unsigned long long stage = (unsigned long long)ni * (unsigned long long)m;
            if (pending + stage > bn.flush_at) flush();
            pending += stage;
        },
        [&](unsigned j, int t) {
            TpObj oj;
            tp_axes<GEOM>(sorted2[j].r, los, oj.r);
            for (int c = 0; c < 3; ++c) jr[c * TP_BLOCK + t] = oj.r[c];
        },
        [&](int q) {
            const int bin = tp_bin_of<GEOM>(oi.r, jr, q, periodic, boxsize, los, s2, ns, me, nmu, rg);
            if (bin < 0) return;
            atomicAdd(&whist[bin], 1u);
        });
    flush();
}

// One set in a periodic box: the topology is known when the kernel is compiled.
template <int GEOM>
__global__ void __launch_bounds__(TP_BLOCK)
tp_pair_kernel(const TpObj* __restrict__ sorted, const unsigned* __restrict__ cell_start,
               const unsigned* __restrict__ tile_start, const GridBoxParams* prm, TpBins bn,
               unsigned long long* __restrict__ part) {
    tp_count_pairs<GEOM>(sorted, cell_start, tile_start, sorted, cell_start, prm, true, true, bn, part);
}

// Two sets (auto_pairs != 0: sorted2 / cell_start2 are set 1's own), periodic when bn.boxsize > 0.
template <int GEOM>
__global__ void __launch_bounds__(TP_BLOCK)
tpx_pair_kernel(const TpObj* __restrict__ sorted1, const unsigned* __restrict__ cell_start1,
                const unsigned* __restrict__ tile_start, const TpObj* __restrict__ sorted2,
                const unsigned* __restrict__ cell_start2, const GridBoxParams* prm, int auto_pairs, TpBins bn,
                unsigned long long* __restrict__ part) {
    tp_count_pairs<GEOM>(sorted1, cell_start1, tile_start, sorted2, cell_start2, prm, bn.boxsize > 0.0, auto_pairs != 0,
                         bn, part);
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

// ---- jackknife: the endpoint table ends[k][b] = the pair ends in region k over the counted pairs of bin b (a pair
// with both ends in k adds 2), so that the ordered pairs with region k left out are 2 counts[b] - ends[k][b].
// tp_count_pairs' walk, stage and bins, with tag * nbins of each staged j in LDS beside its position.  LDS: 32-bit
// counters [hcopies][table] (table = nsub nbins; wave w uses copy w % hcopies), added into the zeroed 64-bit `ends`
// with one global atomicAdd per non-zero counter before a stage that could take a counter past flush_at (a pair adds
// up to 2 to one counter: 2 ni m per stage) and at the end; integer sums, so the order does not matter.  !LDS (the
// table does not fit): 64-bit global atomics straight into `ends`.
template <bool LDS, int GEOM>
__global__ void __launch_bounds__(TP_BLOCK)
tj_pair_kernel(const TjObj* __restrict__ sorted1, const unsigned* __restrict__ cell_start1,
               const unsigned* __restrict__ tile_start, const TjObj* __restrict__ sorted2,
               const unsigned* __restrict__ cell_start2, const GridBoxParams* prm, int auto_pairs, TpBins bn, int table,
               unsigned long long* __restrict__ ends) {
    extern __shared__ double lds[];
    const int ns = bn.ns, nmu = bn.nmu, hcopies = bn.hcopies, los = bn.los;
    const double boxsize = bn.boxsize;
    const bool periodic = boxsize > 0.0;
    double* jr = lds;                                   // [3][TP_BLOCK]: the staged j objects
    double* s2 = jr + 3 * TP_BLOCK;                     // [ns + 1] squared s edges
    double* me = s2 + (ns + 1);                         // [nmu + 1] mu edges
    unsigned* jt = (unsigned*)(me + (nmu + 1));         // [TP_BLOCK]: tag * nbins of the staged j objects
    unsigned* hist = jt + TP_BLOCK;                     // LDS: [hcopies][table]
    const int tid = threadIdx.x;
    const unsigned nbins = (unsigned)(ns * (nmu > 0 ? nmu : 1));
    const unsigned tmax = (unsigned)table / nbins - 1;  // a tag of a prepare call with more regions: the last one
    for (int k = tid; k <= ns; k += TP_BLOCK) s2[k] = bn.s_edges[k] * bn.s_edges[k];
    for (int k = tid; k <= nmu && nmu > 0; k += TP_BLOCK) me[k] = bn.mu_edges[k];
    if (LDS)
        for (int k = tid; k < hcopies * table; k += TP_BLOCK) hist[k] = 0u;
    unsigned* whist = hist + (LDS ? ((tid / 64) % hcopies) * table : 0);
    unsigned long long pending = 0;                     // bound on what any counter gained since the last flush

    auto flush = [&]() {
        __syncthreads();
        for (int e = tid; e < table; e += TP_BLOCK) {
            unsigned long long sum = 0;
            for (int c = 0; c < hcopies; ++c) { sum += hist[c * table + e]; hist[c * table + e] = 0u; }
            if (sum) atomicAdd(&ends[e], sum);
        }
        pending = 0;
        __syncthreads();
    };

    __syncthreads();
    const TpRange rg(s2, ns, me, nmu);
    TjObj oi;
    unsigned ti = 0;                                    // tag * nbins of the thread's i
    grid_pair_walk<TP_BLOCK>(
        cell_start1, tile_start, cell_start2, prm, periodic, auto_pairs != 0,
        [&](unsigned i) {
            const TjObj o = sorted1[i];
            tp_axes<GEOM>(o.r, los, oi.r);
            ti = min(o.tag, tmax) * nbins;
        },
        [&](unsigned ni, int m) {
            if (!LDS) return;
            const unsigned long long stage = 2ull * (unsigned long long)ni * (unsigned long long)m;
            if (pending + stage > bn.flush_at) flush();
            pending += stage;
        },
        [&](unsigned j, int t) {
            const TjObj oj = sorted2[j];
            double rj[3];
            tp_axes<GEOM>(oj.r, los, rj);
            for (int c = 0; c < 3; ++c) jr[c * TP_BLOCK + t] = rj[c];
            jt[t] = min(oj.tag, tmax) * nbins;
        },
        [&](int q) {
            const int bin = tp_bin_of<GEOM>(oi.r, jr, q, periodic, boxsize, los, s2, ns, me, nmu, rg);
            if (bin < 0) return;
            const unsigned ei = ti + (unsigned)bin, ej = jt[q] + (unsigned)bin;
            if (LDS) {
                if (ei == ej) atomicAdd(&whist[ei], 2u);
                else { atomicAdd(&whist[ei], 1u); atomicAdd(&whist[ej], 1u); }
            } else {
                if (ei == ej) atomicAdd(&ends[ei], 2ull);
                else { atomicAdd(&ends[ei], 1ull); atomicAdd(&ends[ej], 1ull); }
            }
        });
    if (LDS) flush();
}

// counts[b] = sum_k ends[k][b] / 2: every counted pair has two ends.
__global__ void __launch_bounds__(256)
tj_counts_kernel(const unsigned long long* __restrict__ ends, int nsub, int nbins,
                 unsigned long long* __restrict__ counts) {
    const int bin = blockIdx.x * blockDim.x + threadIdx.x;
    if (bin >= nbins) return;
    unsigned long long sum = 0;
    for (int k = 0; k < nsub; ++k) sum += ends[(size_t)k * nbins + bin];
    counts[bin] = sum / 2;
}

// The launch of the prep kernel of one non-empty set (TpObj with TpNoTag, TjObj with TjTagging).
template <typename Obj, typename Tagging>
void tp_prep(const void* pos, int pos_dtype, const void* vel, int vel_dtype, int los, double boxsize, size_t n,
             Obj* obj, GridBounds* box, const Tagging& tg, hipStream_t s) {
    ast::dispatch_f32_f64(pos_dtype == AST_F32, vel && vel_dtype == AST_F32, [&](auto tp, auto tv) {
        using TP = decltype(tp);
        using TV = decltype(tv);
        tp_prep_kernel<TP, TV, Obj, Tagging><<<ast::stream_grid(n, 256), 256, 0, s>>>(
            (const TP*)pos, (const TV*)vel, los, boxsize, n, obj, box, tg);
    });
}

// The bins of a call and the dynamic LDS of its pair kernel.  Histogram copies: one per wave where the LDS budget
// allows, else 2 or 1 shared by the waves.  AST_TPCF_FLUSH_AT (tests only): flush the LDS counters after at most this
// many pairs per stage bound.  nsub > 0: the jackknife's kernel, with the tags of a stage in the fixed part and
// nsub nbins counters per copy (its caller takes a single copy up to TJ_LDS, or global memory).
inline size_t tp_fixed_lds(int ns, int nmu, int nsub) {
    return (size_t)3 * TP_BLOCK * sizeof(double) + (size_t)(ns + 1 + nmu + 1) * sizeof(double) +
           (nsub > 0 ? (size_t)TP_BLOCK * 4 : 0);
}

TpBins tp_bins(double boxsize, int los, const double* s_edges, int ns, const double* mu_edges, int nmu, size_t* lds,
               int nsub = 0) {
    const size_t counters = (size_t)nbins_of(ns, nmu) * (nsub > 0 ? nsub : 1);
    const size_t fixed = tp_fixed_lds(ns, nmu, nsub);
    const size_t budget = nsub > 0 ? TJ_LDS_COPIES : TP_LDS;
    int hcopies = TP_WAVES;
    while (hcopies > 1 && fixed + (size_t)hcopies * counters * 4 > budget) hcopies /= 2;
    *lds = fixed + (size_t)hcopies * counters * 4;
    unsigned long long flush_at = TP_FLUSH_AT;
    if (const char* f = getenv("AST_TPCF_FLUSH_AT")) flush_at = strtoull(f, nullptr, 10);
    if (flush_at > TP_FLUSH_AT) flush_at = TP_FLUSH_AT;
    return TpBins{boxsize, los, s_edges, ns, mu_edges, nmu, hcopies, flush_at};
}

// The plan of a call's grid, by one thread.  TP_SMU: cells of the top s edge.  TP_RPPI (s / mu edges: the r_p / pi
// edges): the cylinder's own plan, or with `iso` the isotropic one for sqrt(rp_top^2 + pi_max^2).
int tp_plan(int geom, int iso, GridBoxParams* prm, const GridLayout& L, double boxsize, int los, const double* s_edges_d,
            int ns, const double* mu_edges_d, int nmu, int single_cell, hipStream_t s) {
    if (geom == TP_RPPI)
        grid_cyl_plan_kernel<<<1, 64, 0, s>>>(prm, s_edges_d, ns, mu_edges_d, nmu, los, boxsize, (unsigned)L.cap,
                                              single_cell, iso);
    else
        grid_edge_plan_kernel<<<1, 64, 0, s>>>(prm, s_edges_d, ns, 0.0, boxsize, (unsigned)L.cap, single_cell);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

// The pair counts of a prepared workspace with pairs in it: the plan for the top s edge (tp_plan), the sort, the pair
// kernel - tp_pair_kernel for the one set of ast_tpcf_* (`cross` false), else tpx_pair_kernel - and the reduce.
// geom: TP_SMU, or TP_RPPI with `iso` choosing its plan.
int tp_counts(int geom, int iso, bool cross, char* ws, const GridLayout& L, const size_t* n, int auto_pairs,
              double boxsize, int los, const double* s_edges_d, int ns, const double* mu_edges_d, int nmu,
              int single_cell, unsigned long long* counts_d, hipStream_t s) {
    const int nbins = nbins_of(ns, nmu);
    const int q2 = cross && !auto_pairs ? 1 : 0;
    const bool rppi = geom == TP_RPPI;
    const GridSorted<TpObj, unsigned long long> g(ws, L, q2);
    {
        AST_PROF(rppi ? (cross ? "rppi_cross_grid" : "rppi_grid") : (cross ? "tpcf_cross_grid" : "tpcf_grid"), s);
        if (int rc = tp_plan(geom, iso, g.prm, L, boxsize, los, s_edges_d, ns, mu_edges_d, nmu, single_cell, s))
            return rc;
        if (int rc = grid_sort_sets<TP_BLOCK, TpObj>(ws, L, q2, n, s)) return rc;
    }
    size_t lds;
    const TpBins bn = tp_bins(boxsize, los, s_edges_d, ns, mu_edges_d, nmu, &lds);
    AST_CHECK_ARG(lds <= TP_LDS);
    {
        AST_PROF(rppi ? (cross ? "rppi_cross_pairs" : "rppi_pairs") : (cross ? "tpcf_cross_pairs" : "tpcf_pairs"), s);
        if (cross) {
            const auto pairs = rppi ? tpx_pair_kernel<TP_RPPI> : tpx_pair_kernel<TP_SMU>;
            pairs<<<TP_GRID, TP_BLOCK, lds, s>>>(g.sorted1, g.cell_start1, g.tile_start1, g.sorted2, g.cell_start2,
                                                 g.prm, auto_pairs, bn, g.part);
        } else {
            const auto pairs = rppi ? tp_pair_kernel<TP_RPPI> : tp_pair_kernel<TP_SMU>;
            pairs<<<TP_GRID, TP_BLOCK, lds, s>>>(g.sorted1, g.cell_start1, g.tile_start1, g.prm, bn, g.part);
        }
        AST_CHECK_LAUNCH();
    }
    {
        AST_PROF(rppi ? (cross ? "rppi_cross_reduce" : "rppi_reduce") : (cross ? "tpcf_cross_reduce" : "tpcf_reduce"),
                 s);
        tp_reduce_kernel<<<(nbins + 255) / 256, 256, 0, s>>>(g.part, nbins, counts_d);
        AST_CHECK_LAUNCH();
    }
    return AST_OK;
}

// ---- jackknife: the host side
inline bool tj_ok(int ns, int nmu, int nsub) {
    return bins_ok(ns, nmu) && nsub >= 1 && (long long)nsub * nbins_of(ns, nmu) <= TJ_MAX_TABLE;
}

// Two sets of TjObj on one shared grid; no workgroup rows (the table is the caller's ends_d).
inline GridLayout tj_layout(size_t n1, size_t n2) {
    return GridLayout(2, n1, n2, grid_cells_cap(n1 > n2 ? n1 : n2, 27), sizeof(TjObj), 0);
}

// The largest table (nsub nbins counters) that the pair kernel keeps in LDS.
inline int tj_lds_table(int ns, int nmu) { return (int)((TJ_LDS - tp_fixed_lds(ns, nmu, 1)) / 4); }

// tp_counts for the jackknife: the plan, the sort, the zeroed table, the pair kernel (LDS or global) and the counts.
int tj_counts(int geom, int iso, char* ws, const GridLayout& L, const size_t* n, int auto_pairs, double boxsize, int los,
              const double* s_edges_d, int ns, const double* mu_edges_d, int nmu, int nsub, int single_cell,
              int force_global, unsigned long long* counts_d, unsigned long long* ends_d, hipStream_t s) {
    const int nbins = nbins_of(ns, nmu), table = nsub * nbins;
    const int q2 = auto_pairs ? 0 : 1;
    const bool rppi = geom == TP_RPPI;
    const GridSorted<TjObj, unsigned long long> g(ws, L, q2);
    {
        AST_PROF(rppi ? "rppi_jk_grid" : "tpcf_jk_grid", s);
        if (int rc = tp_plan(geom, iso, g.prm, L, boxsize, los, s_edges_d, ns, mu_edges_d, nmu, single_cell, s))
            return rc;
        if (int rc = grid_sort_sets<TP_BLOCK, TjObj>(ws, L, q2, n, s)) return rc;
    }
    const bool use_lds = !force_global && table <= tj_lds_table(ns, nmu);
    size_t lds;
    const TpBins bn = tp_bins(boxsize, los, s_edges_d, ns, mu_edges_d, nmu, &lds, nsub);
    if (!use_lds) lds = tp_fixed_lds(ns, nmu, nsub);
    AST_CHECK_ARG(lds <= TJ_LDS);
    static ast::PerDeviceOnce attr_once;
    if (attr_once.need()) {
        AST_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&tj_pair_kernel<true, TP_SMU>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)TJ_LDS));
        AST_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&tj_pair_kernel<true, TP_RPPI>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)TJ_LDS));
        attr_once.mark();
    }
    AST_CHECK_HIP(hipMemsetAsync(ends_d, 0, (size_t)table * sizeof(unsigned long long), s));
    {
        AST_PROF(rppi ? (use_lds ? "rppi_jk_pairs_lds" : "rppi_jk_pairs_global")
                      : (use_lds ? "tpcf_jk_pairs_lds" : "tpcf_jk_pairs_global"), s);
        const auto pairs = rppi ? (use_lds ? tj_pair_kernel<true, TP_RPPI> : tj_pair_kernel<false, TP_RPPI>)
                                : (use_lds ? tj_pair_kernel<true, TP_SMU> : tj_pair_kernel<false, TP_SMU>);
        pairs<<<TP_GRID, TP_BLOCK, lds, s>>>(g.sorted1, g.cell_start1, g.tile_start1, g.sorted2, g.cell_start2, g.prm,
                                             auto_pairs, bn, table, ends_d);
        AST_CHECK_LAUNCH();
    }
    {
        AST_PROF(rppi ? "rppi_jk_counts" : "tpcf_jk_counts", s);
        tj_counts_kernel<<<(nbins + 255) / 256, 256, 0, s>>>(ends_d, nsub, nbins, counts_d);
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
        tp_prep(pos_d, pos_dtype, vel_d, vel_dtype, los, boxsize, n, obj, box, TpNoTag{}, s);
    });
}

namespace {
// The entry point of one set in a periodic box, for either geometry (TP_RPPI: nmu >= 1).
int tp_pair_counts_entry(int geom, int iso, void* work_d, size_t work_bytes, size_t n, double boxsize, int los,
                         const double* s_edges_d, int ns, const double* mu_edges_d, int nmu, int single_cell,
                         unsigned long long* counts_d, void* stream) {
    AST_CHECK_ARG(bins_ok(ns, nmu));
    AST_CHECK_ARG(geom == TP_SMU || nmu >= 1);
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
    return tp_counts(geom, iso, false, (char*)work_d, tp_layout(1, n, 0, nbins), &n, 1, boxsize, los, s_edges_d, ns,
                     mu_edges_d, nmu, single_cell, counts_d, s);
}
}  // namespace

extern "C" int ast_tpcf_pair_counts(void* work_d, size_t work_bytes, size_t n, double boxsize, int los,
                                    const double* s_edges_d, int ns, const double* mu_edges_d, int nmu,
                                    int single_cell, unsigned long long* counts_d, void* stream) {
    return tp_pair_counts_entry(TP_SMU, 0, work_d, work_bytes, n, boxsize, los, s_edges_d, ns, mu_edges_d, nmu,
                                single_cell, counts_d, stream);
}

extern "C" int ast_rppi_pair_counts(void* work_d, size_t work_bytes, size_t n, double boxsize, int los,
                                    const double* rp_edges_d, int nrp, const double* pi_edges_d, int npi,
                                    int single_cell, int plan, unsigned long long* counts_d, void* stream) {
    AST_CHECK_ARG(plan == 0 || plan == 1);
    return tp_pair_counts_entry(TP_RPPI, plan, work_d, work_bytes, n, boxsize, los, rp_edges_d, nrp, pi_edges_d, npi,
                                single_cell, counts_d, stream);
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
        tp_prep(pos[q], pos_dtype[q], vel[q], vel_dtype[q], los, boxsize, n[q], obj, box, TpNoTag{}, s);
    });
}

namespace {
// The entry point of two sets, for either geometry (TP_RPPI: nmu >= 1).
int tp_cross_counts_entry(int geom, int iso, void* work_d, size_t work_bytes, size_t n1, size_t n2, int auto_pairs,
                          double boxsize, int los, const double* s_edges_d, int ns, const double* mu_edges_d, int nmu,
                          int single_cell, unsigned long long* counts_d, void* stream) {
    AST_CHECK_ARG(bins_ok(ns, nmu));
    AST_CHECK_ARG(geom == TP_SMU || nmu >= 1);
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
    return tp_counts(geom, iso, true, (char*)work_d, tp_layout(2, n1, n2, nbins), n, auto_pairs, boxsize, los, s_edges_d,
                     ns, mu_edges_d, nmu, single_cell, counts_d, s);
}
}  // namespace

extern "C" int ast_tpcf_cross_counts(void* work_d, size_t work_bytes, size_t n1, size_t n2, int auto_pairs,
                                     double boxsize, int los, const double* s_edges_d, int ns,
                                     const double* mu_edges_d, int nmu, int single_cell,
                                     unsigned long long* counts_d, void* stream) {
    return tp_cross_counts_entry(TP_SMU, 0, work_d, work_bytes, n1, n2, auto_pairs, boxsize, los, s_edges_d, ns,
                                 mu_edges_d, nmu, single_cell, counts_d, stream);
}

extern "C" int ast_rppi_cross_counts(void* work_d, size_t work_bytes, size_t n1, size_t n2, int auto_pairs,
                                     double boxsize, int los, const double* rp_edges_d, int nrp,
                                     const double* pi_edges_d, int npi, int single_cell, int plan,
                                     unsigned long long* counts_d, void* stream) {
    AST_CHECK_ARG(plan == 0 || plan == 1);
    return tp_cross_counts_entry(TP_RPPI, plan, work_d, work_bytes, n1, n2, auto_pairs, boxsize, los, rp_edges_d, nrp,
                                 pi_edges_d, npi, single_cell, counts_d, stream);
}


// ---- jackknife: pair counts with the endpoint table of the leave-one-region-out resampling

extern "C" size_t ast_tpcf_jk_workspace_bytes(size_t n1, size_t n2, int ns, int nmu, int nsub) {
    if (!tj_ok(ns, nmu, nsub)) return 0;
    return tj_layout(n1, n2).total;
}

extern "C" int ast_tpcf_jk_max_table(void) { return TJ_MAX_TABLE; }

extern "C" int ast_tpcf_jk_lds_table(int ns, int nmu) { return bins_ok(ns, nmu) ? tj_lds_table(ns, nmu) : 0; }

extern "C" int ast_tpcf_jk_prepare(const void* pos1_d, int pos1_dtype, const void* vel1_d, int vel1_dtype,
                                   const int* tags1_d, size_t n1, const void* pos2_d, int pos2_dtype,
                                   const void* vel2_d, int vel2_dtype, const int* tags2_d, size_t n2, int los,
                                   double boxsize, const int* nsub, const double* lo, const double* hi, void* work_d,
                                   size_t work_bytes, double* bounds_d, void* stream) {
    AST_CHECK_ARG(n1 == 0 || pos1_dtype == AST_F32 || pos1_dtype == AST_F64);
    AST_CHECK_ARG(n2 == 0 || pos2_dtype == AST_F32 || pos2_dtype == AST_F64);
    AST_CHECK_ARG(vel1_d == nullptr || vel1_dtype == AST_F32 || vel1_dtype == AST_F64);
    AST_CHECK_ARG(vel2_d == nullptr || vel2_dtype == AST_F32 || vel2_dtype == AST_F64);
    AST_CHECK_ARG(los >= 0 && los <= 2);
    AST_CHECK_ARG(boxsize >= 0.0 && std::isfinite(boxsize));
    AST_CHECK_ARG(grid_count_ok(n1) && grid_count_ok(n2));
    AST_CHECK_ARG((n1 == 0 || pos1_d) && (n2 == 0 || pos2_d));
    AST_CHECK_ARG(nsub && lo && hi && bounds_d);
    long long ntot = 1;
    TjTagging tg{};
    for (int a = 0; a < 3; ++a) {
        AST_CHECK_ARG(nsub[a] >= 1 && nsub[a] <= TJ_MAX_TABLE);
        AST_CHECK_ARG(std::isfinite(lo[a]) && std::isfinite(hi[a]) && hi[a] >= lo[a]);
        ntot *= nsub[a];
        AST_CHECK_ARG(ntot <= TJ_MAX_TABLE);
        tg.nsub[a] = nsub[a];
        tg.lo[a] = lo[a];
        tg.dl[a] = (hi[a] - lo[a]) / (double)nsub[a];
    }
    tg.ntot = (int)ntot;
    tg.bad = bounds_d + 12;
    const GridLayout L = tj_layout(n1, n2);
    AST_CHECK_ARG(work_d && work_bytes >= L.part);
    hipStream_t s = ast::as_stream(stream);
    AST_CHECK_HIP(hipMemsetAsync(tg.bad, 0, sizeof(double), s));
    const void* pos[2] = {pos1_d, pos2_d};
    const void* vel[2] = {vel1_d, vel2_d};
    const int* tags[2] = {tags1_d, tags2_d};
    const int pos_dtype[2] = {pos1_dtype, pos2_dtype}, vel_dtype[2] = {vel1_dtype, vel2_dtype};
    const size_t n[2] = {n1, n2};
    return grid_prepare<2, TjObj>((char*)work_d, L, n, bounds_d, "tpcf_jk_prep", s,
                                  [&](int q, TjObj* obj, GridBounds* box) {
        tg.tags = tags[q];
        tp_prep(pos[q], pos_dtype[q], vel[q], vel_dtype[q], los, boxsize, n[q], obj, box, tg, s);
    });
}

namespace {
// The entry point of the jackknife counts, for either geometry (TP_RPPI: nmu >= 1).
int tj_counts_entry(int geom, int iso, void* work_d, size_t work_bytes, size_t n1, size_t n2, int auto_pairs,
                    double boxsize, int los, const double* s_edges_d, int ns, const double* mu_edges_d, int nmu,
                    int nsub, int single_cell, int force_global, unsigned long long* counts_d, unsigned long long* ends_d,
                    void* stream) {
    AST_CHECK_ARG(tj_ok(ns, nmu, nsub));
    AST_CHECK_ARG(geom == TP_SMU || nmu >= 1);
    AST_CHECK_ARG(los >= 0 && los <= 2);
    AST_CHECK_ARG(boxsize >= 0.0 && std::isfinite(boxsize));
    AST_CHECK_ARG(grid_count_ok(n1) && grid_count_ok(n2));
    AST_CHECK_ARG(s_edges_d && (nmu == 0 || mu_edges_d) && counts_d && ends_d);
    AST_CHECK_ARG(work_d && work_bytes >= ast_tpcf_jk_workspace_bytes(n1, n2, ns, nmu, nsub));
    hipStream_t s = ast::as_stream(stream);
    const int nbins = nbins_of(ns, nmu);
    if (grid_no_pairs(auto_pairs, n1, n2)) {
        AST_CHECK_HIP(hipMemsetAsync(counts_d, 0, nbins * sizeof(unsigned long long), s));
        AST_CHECK_HIP(hipMemsetAsync(ends_d, 0, (size_t)nsub * nbins * sizeof(unsigned long long), s));
        return AST_OK;
    }
    const size_t n[2] = {n1, n2};
    return tj_counts(geom, iso, (char*)work_d, tj_layout(n1, n2), n, auto_pairs, boxsize, los, s_edges_d, ns, mu_edges_d,
                     nmu, nsub, single_cell, force_global, counts_d, ends_d, s);
}
}  // namespace

extern "C" int ast_tpcf_jk_counts(void* work_d, size_t work_bytes, size_t n1, size_t n2, int auto_pairs,
                                  double boxsize, int los, const double* s_edges_d, int ns, const double* mu_edges_d,
                                  int nmu, int nsub, int single_cell, int force_global,
                                  unsigned long long* counts_d, unsigned long long* ends_d, void* stream) {
    return tj_counts_entry(TP_SMU, 0, work_d, work_bytes, n1, n2, auto_pairs, boxsize, los, s_edges_d, ns, mu_edges_d,
                           nmu, nsub, single_cell, force_global, counts_d, ends_d, stream);
}

extern "C" int ast_rppi_jk_counts(void* work_d, size_t work_bytes, size_t n1, size_t n2, int auto_pairs,
                                  double boxsize, int los, const double* rp_edges_d, int nrp, const double* pi_edges_d,
                                  int npi, int nsub, int single_cell, int force_global, int plan,
                                  unsigned long long* counts_d, unsigned long long* ends_d, void* stream) {
    AST_CHECK_ARG(plan == 0 || plan == 1);
    return tj_counts_entry(TP_RPPI, plan, work_d, work_bytes, n1, n2, auto_pairs, boxsize, los, rp_edges_d, nrp,
                           pi_edges_d, npi, nsub, single_cell, force_global, counts_d, ends_d, stream);
}
