// Pairwise-velocity moments per separation bin of one or two samples, in a periodic cube or with open boundaries
// (particles/hutils/pair_velocity_box.py: halotools' mean_radial_velocity_vs_r / radial_pvd_vs_r / mean_los_velocity_vs_rp
// / los_pvd_vs_rp, which the reference's commented-out SubFind.mean_pairwise_velocity calls): per-object prep, the
// two-set cell grid and pair walk of cell_grid.h as the pair finder, a tiled pair kernel that carries the
// velocities through the walk and adds count, sum v, sum v^2 per bin into per-wave LDS rows, and a fixed-order sum of
// the workgroup rows.  All pair arithmetic is fp64 (the library is built with -ffp-contract=off).
#include "ast_common.h"
#include "cell_grid.h"
#include <cmath>

namespace {

constexpr int PB_BLOCK = 256;               // i objects per tile = j objects per LDS stage
constexpr int PB_WAVES = PB_BLOCK / 64;
constexpr int PB_GRID = 1024;               // persistent pair-kernel workgroups (256 CUs x 4)
constexpr size_t PB_LDS = 65536;            // dynamic LDS budget of the pair kernel
// 6 x 256 x 8 B of j stage + (bins + 1) x 8 B of squared edges + 4 wave rows x 24 B x bins <= 64 KiB
constexpr int PB_MAX_BINS = AST_PAIRVEL_MAX_BINS;
static_assert((size_t)6 * PB_BLOCK * 8 + (size_t)(PB_MAX_BINS + 1) * 8 + (size_t)PB_WAVES * PB_MAX_BINS * 24 <= PB_LDS,
              "AST_PAIRVEL_MAX_BINS does not fit the LDS budget");
static_assert((size_t)6 * PB_BLOCK * 8 + (size_t)(PB_MAX_BINS + 2) * 8 + (size_t)PB_WAVES * (PB_MAX_BINS + 1) * 24 > PB_LDS,
              "AST_PAIRVEL_MAX_BINS is not the largest that fits");

struct PbObj { double r[3], v[3]; };

inline bool pb_bins_ok(int nb) { return nb >= 1 && nb <= PB_MAX_BINS; }

inline size_t pb_lds_bytes(int nb) {
    return (size_t)6 * PB_BLOCK * sizeof(double) + (size_t)(nb + 1) * sizeof(double) + (size_t)PB_WAVES * nb * 24;
}

// Two sets on one shared grid with room for the larger set's cells.
inline GridLayout pb_layout(size_t n1, size_t n2, int nb) {
    return GridLayout(2, n1, n2, grid_cells_cap(n1 > n2 ? n1 : n2, 27), sizeof(PbObj),
                      (size_t)PB_GRID * (size_t)nb * 24);
}

// One thread per object: positions and velocities widened exactly to one fp64 record (no shift, no wrap); the min /
// max of all coordinates (NaN counts as -inf / +inf) go to `box` (grid_bounds_commit).
template <typename TP, typename TV>
__global__ void __launch_bounds__(256)
pb_prep_kernel(const TP* __restrict__ pos, const TV* __restrict__ vel, size_t n, PbObj* __restrict__ obj,
               GridBounds* box) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        PbObj o;
        for (int a = 0; a < 3; ++a) {
            o.r[a] = (double)pos[3 * i + a];
            o.v[a] = (double)vel[3 * i + a];
        }
        obj[i] = o;
        for (int a = 0; a < 3; ++a) {
            const double x = o.r[a];
            lo[a] = fmin(lo[a], x == x ? x : -INFINITY);
            hi[a] = fmax(hi[a], x == x ? x : INFINITY);
        }
    }
    grid_bounds_commit<256>(lo, hi, box);
}

__device__ inline double pb_pick(const double* r, int k) { return k == 0 ? r[0] : (k == 1 ? r[1] : r[2]); }

// The signed separation of one axis: with a period, the image within half a box.  Exactly antisymmetric under i <-> j,
// and |s| is bit for bit tpcf.hip's min(|dx|, L - |dx|).
__device__ inline double pb_wrap(double s, bool periodic, double boxsize, double half) {
    if (periodic) {
        if (s > half) s = s - boxsize;
        else if (s < -half) s = s + boxsize;
    }
    return s;
}

// The walk of cell_grid.h (grid_pair_walk: two sets; auto_pairs != 0: sorted2 / cell_start2 are set 1's own; periodic
// when boxsize > 0, with the signed minimum image, else plain separations).
// With s = x_j - x_i (wrapped) and dv = v_j - v_i:
//   AST_PAIRVEL_RADIAL: d2 = (sx^2 + sy^2) + sz^2, bin k when e_k^2 < d2 <= e_{k+1}^2,
//                       v = ((dvx sx + dvy sy) + dvz sz) / sqrt(d2).  The j stage holds r and v, axis by axis.
//   AST_PAIRVEL_LOS:    rp2 = s_a^2 + s_b^2 (a < b the axes other than los), bin k when e_k^2 < rp2 <= e_{k+1}^2 and
//                       |s_los| <= pi_max, v = dv_los sign(s_los).  The j stage holds r_a, r_b, r_los, v_los.
// Both v are the same bit for bit under i <-> j.  Each wave adds into its own LDS rows (sum v, sum v^2: fp64 LDS
// atomics; count: 64-bit integers); at the end the workgroup's row, waves summed in wave order, is stored to part
// with plain stores - every workgroup stores its whole row, so part needs no clearing.  No global atomics.
template <int KIND>
__global__ void __launch_bounds__(PB_BLOCK)
pb_pair_kernel(const PbObj* __restrict__ sorted1, const unsigned* __restrict__ cell_start1,
               const unsigned* __restrict__ tile_start, const PbObj* __restrict__ sorted2,
               const unsigned* __restrict__ cell_start2, const GridBoxParams* prm, double boxsize, int auto_pairs,
               int los, double pi_max, const double* __restrict__ edges, int nb, double* __restrict__ part) {
    extern __shared__ double lds[];
    double* jr = lds;                                   // [6][PB_BLOCK]: the staged j objects
    double* e2 = jr + 6 * PB_BLOCK;                     // [nb + 1] squared edges
    double* h1 = e2 + (nb + 1);                         // [PB_WAVES][nb] sum v
    double* h2 = h1 + PB_WAVES * nb;                    // [PB_WAVES][nb] sum v^2
    unsigned long long* hc = (unsigned long long*)(h2 + PB_WAVES * nb);
    const int tid = threadIdx.x, w = tid / 64;
    for (int k = tid; k <= nb; k += PB_BLOCK) e2[k] = edges[k] * edges[k];
    for (int k = tid; k < PB_WAVES * nb; k += PB_BLOCK) { h1[k] = 0.0; h2[k] = 0.0; hc[k] = 0ull; }
    double* wh1 = h1 + w * nb;
    double* wh2 = h2 + w * nb;
    unsigned long long* whc = hc + w * nb;

    const bool periodic = boxsize > 0.0;
    const double half = 0.5 * boxsize;
    const int la = los == 0 ? 1 : 0, lb = los == 2 ? 1 : 2;     // the axes other than los, in axis order
    __syncthreads();
    const double e2lo = e2[0], e2hi = e2[nb];
    double ir[3] = {0.0, 0.0, 0.0}, iv[3] = {0.0, 0.0, 0.0};
    grid_pair_walk<PB_BLOCK>(
        cell_start1, tile_start, cell_start2, prm, periodic, auto_pairs != 0,
        [&](unsigned i) {
            const PbObj oi = sorted1[i];
            if (KIND == AST_PAIRVEL_LOS) {
                ir[0] = pb_pick(oi.r, la); ir[1] = pb_pick(oi.r, lb); ir[2] = pb_pick(oi.r, los);
                iv[0] = pb_pick(oi.v, los);
            } else {
                for (int c = 0; c < 3; ++c) { ir[c] = oi.r[c]; iv[c] = oi.v[c]; }
            }
        },
        [](unsigned, int) {},
        [&](unsigned j, int t) {
            const PbObj oj = sorted2[j];
            if (KIND == AST_PAIRVEL_LOS) {
                jr[t] = pb_pick(oj.r, la);
                jr[PB_BLOCK + t] = pb_pick(oj.r, lb);
                jr[2 * PB_BLOCK + t] = pb_pick(oj.r, los);
                jr[3 * PB_BLOCK + t] = pb_pick(oj.v, los);
            } else {
                for (int c = 0; c < 3; ++c) {
                    jr[c * PB_BLOCK + t] = oj.r[c];
                    jr[(3 + c) * PB_BLOCK + t] = oj.v[c];
                }
            }
        },
        [&](int q) {
            // the candidate test needs |s| only: m = |x_j - x_i|, or L - m beyond half a box - the magnitude of
            // pb_wrap's result bit for bit, and tpcf.hip's min(|dx|, L - |dx|); the signs are put back on the
            // pairs that fall into a bin
            const double r0 = jr[q] - ir[0], r1 = jr[PB_BLOCK + q] - ir[1], r2 = jr[2 * PB_BLOCK + q] - ir[2];
            double m0 = fabs(r0), m1 = fabs(r1), m2 = fabs(r2);
            if (periodic) {
                m0 = m0 > half ? boxsize - m0 : m0;
                m1 = m1 > half ? boxsize - m1 : m1;
                m2 = m2 > half ? boxsize - m2 : m2;
            }
            double t2, v;
            if (KIND == AST_PAIRVEL_LOS) {
                t2 = m0 * m0 + m1 * m1;
                if (!(t2 <= e2hi) || !(t2 > e2lo) || !(m2 <= pi_max)) return;
                const double s2 = pb_wrap(r2, periodic, boxsize, half);
                const double dv = jr[3 * PB_BLOCK + q] - iv[0];
                v = s2 > 0.0 ? dv : (s2 < 0.0 ? -dv : dv * 0.0);
            } else {
                t2 = (m0 * m0 + m1 * m1) + m2 * m2;
                if (!(t2 <= e2hi) || !(t2 > e2lo)) return;
                const double s0 = pb_wrap(r0, periodic, boxsize, half), s1 = pb_wrap(r1, periodic, boxsize, half),
                             s2 = pb_wrap(r2, periodic, boxsize, half);
                const double dv0 = jr[3 * PB_BLOCK + q] - iv[0], dv1 = jr[4 * PB_BLOCK + q] - iv[1],
                             dv2 = jr[5 * PB_BLOCK + q] - iv[2];
                v = ((dv0 * s0 + dv1 * s1) + dv2 * s2) / sqrt(t2);
            }
            int lo = 0, hi = nb;                        // e2[lo] < t2 <= e2[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (t2 <= e2[mid]) hi = mid; else lo = mid;
            }
            atomicAdd(&wh1[lo], v);
            atomicAdd(&wh2[lo], v * v);
            atomicAdd(&whc[lo], 1ull);
        });
    __syncthreads();
    grid_store_rows<PB_WAVES, PB_GRID>(h1, h2, hc, nb, part);
}

}  // namespace

extern "C" size_t ast_pairvel_workspace_bytes(size_t n1, size_t n2, int nb) {
    if (!pb_bins_ok(nb)) return 0;
    return pb_layout(n1, n2, nb).total;
}

extern "C" int ast_pairvel_max_bins(void) { return PB_MAX_BINS; }

extern "C" int ast_pairvel_prepare(const void* pos1_d, int pos1_dtype, const void* vel1_d, int vel1_dtype, size_t n1,
                                   const void* pos2_d, int pos2_dtype, const void* vel2_d, int vel2_dtype, size_t n2,
                                   void* work_d, size_t work_bytes, double* bounds_d, void* stream) {
    AST_CHECK_ARG(n1 == 0 || ((pos1_dtype == AST_F32 || pos1_dtype == AST_F64) &&
                              (vel1_dtype == AST_F32 || vel1_dtype == AST_F64)));
    AST_CHECK_ARG(n2 == 0 || ((pos2_dtype == AST_F32 || pos2_dtype == AST_F64) &&
                              (vel2_dtype == AST_F32 || vel2_dtype == AST_F64)));
    AST_CHECK_ARG(grid_count_ok(n1) && grid_count_ok(n2));
    AST_CHECK_ARG((n1 == 0 || (pos1_d && vel1_d)) && (n2 == 0 || (pos2_d && vel2_d)));
    AST_CHECK_ARG(bounds_d);
    const GridLayout L = pb_layout(n1, n2, 1);
    AST_CHECK_ARG(work_d && work_bytes >= L.part);
    hipStream_t s = ast::as_stream(stream);
    const void* pos[2] = {pos1_d, pos2_d};
    const void* vel[2] = {vel1_d, vel2_d};
    const int pos_dtype[2] = {pos1_dtype, pos2_dtype}, vel_dtype[2] = {vel1_dtype, vel2_dtype};
    const size_t n[2] = {n1, n2};
    return grid_prepare<2, PbObj>((char*)work_d, L, n, bounds_d, "pairvel_prep", s,
                                  [&](int q, PbObj* obj, GridBounds* box) {
        ast::dispatch_f32_f64(pos_dtype[q] == AST_F32, vel_dtype[q] == AST_F32, [&](auto tp, auto tv) {
            using TP = decltype(tp);
            using TV = decltype(tv);
            pb_prep_kernel<TP, TV><<<ast::stream_grid(n[q], 256), 256, 0, s>>>((const TP*)pos[q], (const TV*)vel[q],
                                                                                 n[q], obj, box);
        });
    });
}

extern "C" int ast_pairvel_moments(void* work_d, size_t work_bytes, size_t n1, size_t n2, int auto_pairs,
                                   double boxsize, int kind, int los, double pi_max, const double* edges_d, int nb,
                                   int single_cell, unsigned long long* count_d, double* s1_d, double* s2_d,
                                   void* stream) {
    AST_CHECK_ARG(pb_bins_ok(nb));
    AST_CHECK_ARG(kind == AST_PAIRVEL_RADIAL || kind == AST_PAIRVEL_LOS);
    AST_CHECK_ARG(los >= 0 && los <= 2);
    AST_CHECK_ARG(kind == AST_PAIRVEL_RADIAL || (pi_max > 0.0 && std::isfinite(pi_max)));
    AST_CHECK_ARG(boxsize >= 0.0 && std::isfinite(boxsize));
    AST_CHECK_ARG(grid_count_ok(n1) && grid_count_ok(n2));
    AST_CHECK_ARG(edges_d && count_d && s1_d && s2_d);
    AST_CHECK_ARG(work_d && work_bytes >= ast_pairvel_workspace_bytes(n1, n2, nb));
    hipStream_t s = ast::as_stream(stream);
    if (grid_no_pairs(auto_pairs, n1, n2)) {
        AST_CHECK_HIP(hipMemsetAsync(count_d, 0, nb * sizeof(unsigned long long), s));
        AST_CHECK_HIP(hipMemsetAsync(s1_d, 0, nb * sizeof(double), s));
        AST_CHECK_HIP(hipMemsetAsync(s2_d, 0, nb * sizeof(double), s));
        return AST_OK;
    }
    const GridLayout L = pb_layout(n1, n2, nb);
    char* ws = (char*)work_d;
    const size_t n[2] = {n1, n2};
    const int q2 = auto_pairs ? 0 : 1;
    const GridSorted<PbObj> g(ws, L, q2);
    if (kind == AST_PAIRVEL_RADIAL) pi_max = 0.0;       // the reach is the top edge itself
    {
        AST_PROF("pairvel_grid", s);
        grid_edge_plan_kernel<<<1, 64, 0, s>>>(g.prm, edges_d, nb, pi_max, boxsize, (unsigned)L.cap, single_cell);
        AST_CHECK_LAUNCH();
        if (int rc = grid_sort_sets<PB_BLOCK, PbObj>(ws, L, q2, n, s)) return rc;
    }
    const size_t lds = pb_lds_bytes(nb);
    AST_CHECK_ARG(lds <= PB_LDS);
    {
        AST_PROF("pairvel_pairs", s);
        const auto pairs = kind == AST_PAIRVEL_LOS ? pb_pair_kernel<AST_PAIRVEL_LOS> : pb_pair_kernel<AST_PAIRVEL_RADIAL>;
        pairs<<<PB_GRID, PB_BLOCK, lds, s>>>(g.sorted1, g.cell_start1, g.tile_start1, g.sorted2, g.cell_start2, g.prm,
                                             boxsize, auto_pairs, los, pi_max, edges_d, nb, g.part);
        AST_CHECK_LAUNCH();
    }
    {
        AST_PROF("pairvel_reduce", s);
        grid_reduce3_kernel<PB_GRID><<<(nb + 255) / 256, 256, 0, s>>>(g.part, nb, s1_d, s2_d, count_d);
        AST_CHECK_LAUNCH();
    }
    return AST_OK;
}
