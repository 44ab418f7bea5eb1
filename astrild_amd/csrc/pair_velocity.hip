// Pairwise-velocity moments per separation bin of one or two samples, in a periodic cube or with open boundaries
// (particles/hutils/pair_velocity_box.py: halotools' mean_radial_velocity_vs_r / radial_pvd_vs_r / mean_los_velocity_vs_rp
// / los_pvd_vs_rp, which the reference's commented-out SubFind.mean_pairwise_velocity calls): per-object prep, the
// two-sample cell grid of tpcf.hip's second half (cell_grid.h) as the pair finder, a tiled pair kernel that carries the
// velocities through the walk and adds count, sum v, sum v^2 per bin into per-wave LDS rows, and a fixed-order sum of
// the workgroup rows.  All pair arithmetic is fp64 (the library is built with -ffp-contract=off).
#include "ast_common.h"
#include "cell_grid.h"
#include <cmath>

namespace {

constexpr int PB_BLOCK = 256;               // i objects per tile = j objects per LDS stage
constexpr int PB_WAVES = PB_BLOCK / 64;
constexpr int PB_GRID = 1024;               // persistent pair-kernel workgroups (256 CUs x 4)
constexpr int PB_NEIGH = 27;                // cross pairs: the cell itself and all 26 neighbours
constexpr size_t PB_MAX_CELLS = size_t(1) << 20;
constexpr size_t PB_LDS = 65536;            // dynamic LDS budget of the pair kernel
// 6 x 256 x 8 B of j stage + (bins + 1) x 8 B of squared edges + 4 wave rows x 24 B x bins <= 64 KiB
constexpr int PB_MAX_BINS = AST_PAIRVEL_MAX_BINS;
static_assert((size_t)6 * PB_BLOCK * 8 + (size_t)(PB_MAX_BINS + 1) * 8 + (size_t)PB_WAVES * PB_MAX_BINS * 24 <= PB_LDS,
              "AST_PAIRVEL_MAX_BINS does not fit the LDS budget");
static_assert((size_t)6 * PB_BLOCK * 8 + (size_t)(PB_MAX_BINS + 2) * 8 + (size_t)PB_WAVES * (PB_MAX_BINS + 1) * 24 > PB_LDS,
              "AST_PAIRVEL_MAX_BINS is not the largest that fits");

struct PbObj { double r[3], v[3]; };

struct PbBounds { unsigned long long kmin[3], kmax[3]; };   // bounding box of one set as order-preserving keys

inline size_t pb_cells_cap(size_t n1, size_t n2) {
    const size_t n = n1 > n2 ? n1 : n2;
    const size_t c = n < PB_MAX_CELLS ? n : PB_MAX_CELLS;
    return c < 27 ? 27 : c;
}

inline bool pb_bins_ok(int nb) { return nb >= 1 && nb <= PB_MAX_BINS; }

inline size_t pb_lds_bytes(int nb) {
    return (size_t)6 * PB_BLOCK * sizeof(double) + (size_t)(nb + 1) * sizeof(double) + (size_t)PB_WAVES * nb * 24;
}

// One grid (GridBoxParams) shared by both sets; per set its own bounds, counts, cell starts, cell numbers, fp64 records
// and their cell-sorted copy (TpxLayout of tpcf.hip with the wider record).  Only set 1 has tiles; tile_start[1] is
// where the scan of set 2 puts the tile list nobody reads.  Everything before `part` is independent of the bin count.
struct PbLayout {
    size_t grid, set_prm[2], cnt[2], cell_start[2], tile_start[2], cursor, cell_of[2], obj[2], sorted[2], part, total;
    PbLayout(size_t n1, size_t n2, int nb) {
        const size_t cap = pb_cells_cap(n1, n2);
        const size_t n[2] = {n1, n2};
        size_t o = 0;
        grid = o; o += align256(sizeof(GridBoxParams));
        for (int s = 0; s < 2; ++s) {
            set_prm[s] = o;    o += align256(sizeof(PbBounds));
            cnt[s] = o;        o += align256(cap * 4);
            cell_start[s] = o; o += align256((cap + 1) * 4);
            tile_start[s] = o; o += align256((cap + 1) * 4);
            cell_of[s] = o;    o += align256(n[s] * 4);
            obj[s] = o;        o += align256(n[s] * sizeof(PbObj));
            sorted[s] = o;     o += align256(n[s] * sizeof(PbObj));
        }
        cursor = o; o += align256(cap * 4);
        part = o;   o += align256((size_t)PB_GRID * (size_t)nb * 24);
        total = o;
    }
};

// One thread per object: positions and velocities widened exactly to one fp64 record (no shift, no wrap); the min /
// max of all coordinates (NaN counts as -inf / +inf) go to prm->kmin / kmax, one atomic per workgroup and axis.
template <typename TP, typename TV>
__global__ void __launch_bounds__(256)
pb_prep_kernel(const TP* __restrict__ pos, const TV* __restrict__ vel, size_t n, PbObj* __restrict__ obj,
               PbBounds* prm) {
    __shared__ double wlo[3][4], whi[3][4];
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

// bounds[6 s + 0..2] = min, bounds[6 s + 3..5] = max of set s ((+inf, -inf) for an empty set); the union of both boxes
// goes to the shared grid's kmin / kmax (an empty set leaves the other's box).
__global__ void pb_bounds_kernel(const PbBounds* prm1, const PbBounds* prm2, GridBoxParams* grid,
                                 double* __restrict__ bounds) {
    const int a = threadIdx.x;
    if (a >= 3) return;
    const PbBounds* prm[2] = {prm1, prm2};
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

// One thread: the shared grid, tpx_plan_kernel's of tpcf.hip with the reach of the kind: the top edge (radial), or
// sqrt(top^2 + pi_max^2) (los).  boxsize > 0: floor(L / (reach (1 + 1e-6))) cells per axis, lowered to the cap, at
// least 3, else one cell; boxsize == 0: grid_box_plan over the union bounding box, per-axis dims that may be 1.
__global__ void pb_plan_kernel(GridBoxParams* prm, const double* __restrict__ edges, int nb, int kind, double pi_max,
                               double boxsize, unsigned cap, int single) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double top = edges[nb];
    const double reach = kind == AST_PAIRVEL_LOS ? sqrt(top * top + pi_max * pi_max) : top;
    if (!(boxsize > 0.0)) {
        grid_box_plan(prm, reach, cap, single);
        return;
    }
    int d = 1;
    const double m = floor(boxsize / (reach * (1.0 + 1e-6)));
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

// Work item = (tile of PB_BLOCK set-1 objects of cell a, neighbour k), as tpx_pair_kernel of tpcf.hip; the j objects
// are those of set 2 in cell a + offset[k], staged through LDS PB_BLOCK at a time.
//   auto_pairs == 0: k over all 27 offsets, every (i, j) once.
//   auto_pairs != 0: sorted2 / cell_start2 are set 1's own; k over the 14 half-shell offsets, j > i at k = 0.
//   boxsize > 0: signed minimum image, neighbours wrap (dims >= 3 on every axis, or one cell: offset 0 only).
//   boxsize == 0: plain separations, a neighbour outside [0, dims) on any axis is skipped.
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
    const int dims[3] = {prm->dims[0], prm->dims[1], prm->dims[2]};
    const unsigned ncells = prm->ncells;
    const int nneigh = auto_pairs ? GRID_NEIGH : PB_NEIGH;
    const unsigned long long nitems = (unsigned long long)prm->ntiles * (unsigned long long)nneigh;
    __syncthreads();
    const double e2lo = e2[0], e2hi = e2[nb];
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
        const unsigned i0 = cell_start1[a] + (tile - tile_start[a]) * PB_BLOCK;
        const unsigned i1 = min(i0 + PB_BLOCK, cell_start1[a + 1]);
        const unsigned j0 = self ? i0 + 1 : cell_start2[b];
        const unsigned j1 = cell_start2[b + 1];
        if (j0 >= j1) continue;

        const unsigned i = i0 + tid;
        const bool valid = i < i1;
        double ir[3] = {0.0, 0.0, 0.0}, iv[3] = {0.0, 0.0, 0.0};
        if (valid) {
            const PbObj oi = sorted1[i];
            if (KIND == AST_PAIRVEL_LOS) {
                ir[0] = pb_pick(oi.r, la); ir[1] = pb_pick(oi.r, lb); ir[2] = pb_pick(oi.r, los);
                iv[0] = pb_pick(oi.v, los);
            } else {
                for (int c = 0; c < 3; ++c) { ir[c] = oi.r[c]; iv[c] = oi.v[c]; }
            }
        }
        for (unsigned jc = j0; jc < j1; jc += PB_BLOCK) {
            __syncthreads();
            if (jc + tid < j1) {
                const PbObj oj = sorted2[jc + tid];
                if (KIND == AST_PAIRVEL_LOS) {
                    jr[tid] = pb_pick(oj.r, la);
                    jr[PB_BLOCK + tid] = pb_pick(oj.r, lb);
                    jr[2 * PB_BLOCK + tid] = pb_pick(oj.r, los);
                    jr[3 * PB_BLOCK + tid] = pb_pick(oj.v, los);
                } else {
                    for (int c = 0; c < 3; ++c) {
                        jr[c * PB_BLOCK + tid] = oj.r[c];
                        jr[(3 + c) * PB_BLOCK + tid] = oj.v[c];
                    }
                }
            }
            __syncthreads();
            if (!valid) continue;
            const int m = (int)min((unsigned)PB_BLOCK, j1 - jc);
            const int q0 = (self && i + 1 > jc) ? (int)min((unsigned)m, i + 1 - jc) : 0;
            for (int q = q0; q < m; ++q) {
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
                    if (!(t2 <= e2hi) || !(t2 > e2lo) || !(m2 <= pi_max)) continue;
                    const double s2 = pb_wrap(r2, periodic, boxsize, half);
                    const double dv = jr[3 * PB_BLOCK + q] - iv[0];
                    v = s2 > 0.0 ? dv : (s2 < 0.0 ? -dv : dv * 0.0);
                } else {
                    t2 = (m0 * m0 + m1 * m1) + m2 * m2;
                    if (!(t2 <= e2hi) || !(t2 > e2lo)) continue;
                    const double s0 = pb_wrap(r0, periodic, boxsize, half), s1 = pb_wrap(r1, periodic, boxsize, half),
                                 s2 = pb_wrap(r2, periodic, boxsize, half);
                    const double dv0 = jr[3 * PB_BLOCK + q] - iv[0], dv1 = jr[4 * PB_BLOCK + q] - iv[1],
                                 dv2 = jr[5 * PB_BLOCK + q] - iv[2];
                    v = ((dv0 * s0 + dv1 * s1) + dv2 * s2) / sqrt(t2);
                }
                int lo = 0, hi = nb;                    // e2[lo] < t2 <= e2[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (t2 <= e2[mid]) hi = mid; else lo = mid;
                }
                atomicAdd(&wh1[lo], v);
                atomicAdd(&wh2[lo], v * v);
                atomicAdd(&whc[lo], 1ull);
            }
        }
    }
    __syncthreads();
    double* p1 = part;
    double* p2 = part + (size_t)PB_GRID * nb;
    unsigned long long* pc = (unsigned long long*)(part + 2 * (size_t)PB_GRID * nb);
    for (int bin = tid; bin < nb; bin += PB_BLOCK) {
        double a1 = h1[bin], a2 = h2[bin];
        unsigned long long ac = hc[bin];
        for (int v = 1; v < PB_WAVES; ++v) { a1 += h1[v * nb + bin]; a2 += h2[v * nb + bin]; ac += hc[v * nb + bin]; }
        const size_t o = (size_t)blockIdx.x * nb + bin;
        p1[o] = a1;
        p2[o] = a2;
        pc[o] = ac;
    }
}

// out[bin] = sum of the PB_GRID workgroup rows, in row order.
__global__ void __launch_bounds__(256)
pb_reduce_kernel(const double* __restrict__ part, int nb, unsigned long long* __restrict__ count,
                 double* __restrict__ s1, double* __restrict__ s2) {
    const int bin = blockIdx.x * blockDim.x + threadIdx.x;
    if (bin >= nb) return;
    const double* p1 = part;
    const double* p2 = part + (size_t)PB_GRID * nb;
    const unsigned long long* pc = (const unsigned long long*)(part + 2 * (size_t)PB_GRID * nb);
    double a1 = 0.0, a2 = 0.0;
    unsigned long long ac = 0;
    for (int g = 0; g < PB_GRID; ++g) {
        const size_t o = (size_t)g * nb + bin;
        a1 += p1[o];
        a2 += p2[o];
        ac += pc[o];
    }
    s1[bin] = a1;
    s2[bin] = a2;
    count[bin] = ac;
}

template <typename TP, typename TV>
void launch_prep(const void* pos, const void* vel, size_t n, PbObj* obj, PbBounds* prm, hipStream_t s) {
    pb_prep_kernel<TP, TV><<<ast::stream_grid(n, 256), 256, 0, s>>>((const TP*)pos, (const TV*)vel, n, obj, prm);
}

int pb_prep(const void* pos, int pos_dtype, const void* vel, int vel_dtype, size_t n, PbObj* obj, PbBounds* prm,
            hipStream_t s) {
    AST_CHECK_HIP(hipMemsetAsync(prm->kmin, 0xff, sizeof(prm->kmin), s));
    AST_CHECK_HIP(hipMemsetAsync(prm->kmax, 0x00, sizeof(prm->kmax), s));
    if (n == 0) return AST_OK;
    if (pos_dtype == AST_F32 && vel_dtype == AST_F32)
        launch_prep<float, float>(pos, vel, n, obj, prm, s);
    else if (pos_dtype == AST_F32)
        launch_prep<float, double>(pos, vel, n, obj, prm, s);
    else if (vel_dtype == AST_F32)
        launch_prep<double, float>(pos, vel, n, obj, prm, s);
    else
        launch_prep<double, double>(pos, vel, n, obj, prm, s);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

}  // namespace

extern "C" size_t ast_pairvel_workspace_bytes(size_t n1, size_t n2, int nb) {
    if (!pb_bins_ok(nb)) return 0;
    return PbLayout(n1, n2, nb).total;
}

extern "C" int ast_pairvel_max_bins(void) { return PB_MAX_BINS; }

extern "C" int ast_pairvel_prepare(const void* pos1_d, int pos1_dtype, const void* vel1_d, int vel1_dtype, size_t n1,
                                   const void* pos2_d, int pos2_dtype, const void* vel2_d, int vel2_dtype, size_t n2,
                                   void* work_d, size_t work_bytes, double* bounds_d, void* stream) {
    AST_CHECK_ARG(n1 == 0 || ((pos1_dtype == AST_F32 || pos1_dtype == AST_F64) &&
                              (vel1_dtype == AST_F32 || vel1_dtype == AST_F64)));
    AST_CHECK_ARG(n2 == 0 || ((pos2_dtype == AST_F32 || pos2_dtype == AST_F64) &&
                              (vel2_dtype == AST_F32 || vel2_dtype == AST_F64)));
    AST_CHECK_ARG(n1 < (size_t(1) << 31) && n2 < (size_t(1) << 31));
    AST_CHECK_ARG((n1 == 0 || (pos1_d && vel1_d)) && (n2 == 0 || (pos2_d && vel2_d)));
    AST_CHECK_ARG(bounds_d);
    const PbLayout L(n1, n2, 1);
    AST_CHECK_ARG(work_d && work_bytes >= L.part);
    hipStream_t s = ast::as_stream(stream);
    char* ws = (char*)work_d;
    PbBounds* prm1 = (PbBounds*)(ws + L.set_prm[0]);
    PbBounds* prm2 = (PbBounds*)(ws + L.set_prm[1]);
    {
        AST_PROF("pairvel_prep", s);
        int rc = pb_prep(pos1_d, pos1_dtype, vel1_d, vel1_dtype, n1, (PbObj*)(ws + L.obj[0]), prm1, s);
        if (rc != AST_OK) return rc;
        rc = pb_prep(pos2_d, pos2_dtype, vel2_d, vel2_dtype, n2, (PbObj*)(ws + L.obj[1]), prm2, s);
        if (rc != AST_OK) return rc;
    }
    pb_bounds_kernel<<<1, 64, 0, s>>>(prm1, prm2, (GridBoxParams*)(ws + L.grid), bounds_d);
    AST_CHECK_LAUNCH();
    return AST_OK;
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
    AST_CHECK_ARG(n1 < (size_t(1) << 31) && n2 < (size_t(1) << 31));
    AST_CHECK_ARG(edges_d && count_d && s1_d && s2_d);
    AST_CHECK_ARG(work_d && work_bytes >= ast_pairvel_workspace_bytes(n1, n2, nb));
    hipStream_t s = ast::as_stream(stream);
    if (auto_pairs ? n1 < 2 : (n1 == 0 || n2 == 0)) {
        AST_CHECK_HIP(hipMemsetAsync(count_d, 0, nb * sizeof(unsigned long long), s));
        AST_CHECK_HIP(hipMemsetAsync(s1_d, 0, nb * sizeof(double), s));
        AST_CHECK_HIP(hipMemsetAsync(s2_d, 0, nb * sizeof(double), s));
        return AST_OK;
    }
    const PbLayout L(n1, n2, nb);
    char* ws = (char*)work_d;
    GridBoxParams* prm = (GridBoxParams*)(ws + L.grid);
    unsigned* cursor = (unsigned*)(ws + L.cursor);
    double* part = (double*)(ws + L.part);
    const size_t cap = pb_cells_cap(n1, n2);
    const size_t n[2] = {n1, n2};
    if (kind == AST_PAIRVEL_RADIAL) pi_max = 0.0;
    {
        AST_PROF("pairvel_grid", s);
        pb_plan_kernel<<<1, 64, 0, s>>>(prm, edges_d, nb, kind, pi_max, boxsize, (unsigned)cap, single_cell);
        AST_CHECK_LAUNCH();
        // set 2 first: the scan of set 1 then leaves its tile count in prm->ntiles
        for (int q = auto_pairs ? 0 : 1; q >= 0; --q) {
            unsigned* cnt = (unsigned*)(ws + L.cnt[q]);
            unsigned* cell_of = (unsigned*)(ws + L.cell_of[q]);
            const PbObj* obj = (const PbObj*)(ws + L.obj[q]);
            AST_CHECK_HIP(hipMemsetAsync(cnt, 0, cap * 4, s));
            grid_box_count_kernel<<<ast::stream_grid(n[q], 256), 256, 0, s>>>(obj, n[q], prm, cell_of, cnt);
            AST_CHECK_LAUNCH();
            grid_scan_kernel<PB_BLOCK><<<1, 1024, 0, s>>>(cnt, prm, (unsigned*)(ws + L.cell_start[q]),
                                                          (unsigned*)(ws + L.tile_start[q]), cursor);
            AST_CHECK_LAUNCH();
            grid_scatter_kernel<<<ast::stream_grid(n[q], 256), 256, 0, s>>>(obj, n[q], cell_of, cursor,
                                                                             (PbObj*)(ws + L.sorted[q]));
            AST_CHECK_LAUNCH();
        }
    }
    const int q2 = auto_pairs ? 0 : 1;
    const size_t lds = pb_lds_bytes(nb);
    AST_CHECK_ARG(lds <= PB_LDS);
    const PbObj* sorted1 = (const PbObj*)(ws + L.sorted[0]);
    const PbObj* sorted2 = (const PbObj*)(ws + L.sorted[q2]);
    const unsigned* cs1 = (const unsigned*)(ws + L.cell_start[0]);
    const unsigned* cs2 = (const unsigned*)(ws + L.cell_start[q2]);
    const unsigned* ts1 = (const unsigned*)(ws + L.tile_start[0]);
    {
        AST_PROF("pairvel_pairs", s);
        if (kind == AST_PAIRVEL_LOS)
            pb_pair_kernel<AST_PAIRVEL_LOS><<<PB_GRID, PB_BLOCK, lds, s>>>(sorted1, cs1, ts1, sorted2, cs2, prm, boxsize,
                                                                           auto_pairs, los, pi_max, edges_d, nb, part);
        else
            pb_pair_kernel<AST_PAIRVEL_RADIAL><<<PB_GRID, PB_BLOCK, lds, s>>>(sorted1, cs1, ts1, sorted2, cs2, prm,
                                                                              boxsize, auto_pairs, los, pi_max, edges_d,
                                                                              nb, part);
        AST_CHECK_LAUNCH();
    }
    {
        AST_PROF("pairvel_reduce", s);
        pb_reduce_kernel<<<(nb + 255) / 256, 256, 0, s>>>(part, nb, count_d, s1_d, s2_d);
        AST_CHECK_LAUNCH();
    }
    return AST_OK;
}
