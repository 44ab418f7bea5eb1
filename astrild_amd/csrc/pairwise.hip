// Mean pairwise velocity from transverse velocities (Yasini et al. 2018), the estimator of
// particles/hutils/mean_pairwise_velocity.py: per-object prep, a uniform cell grid (counting sort by cell) as the
// pair finder, a tiled pair kernel with per-workgroup LDS histograms, and a fixed-order sum of the workgroup rows.
// All pair arithmetic is fp64 (the library is built with -ffp-contract=off: op-by-op IEEE, like numpy).
#include "ast_common.h"
#include "cell_grid.h"
#include <cmath>

namespace {

constexpr int PV_BLOCK = 256;               // i objects per tile = j objects per LDS stage
constexpr int PV_WAVES = PV_BLOCK / 64;
constexpr int PV_GRID = 1024;               // persistent pair-kernel workgroups (256 CUs x 4)
constexpr int PV_MAX_BINS = 480;            // 4 wave histograms x 24 B x bins + the j stage fit 64 KiB of LDS

struct PvObj { double r[3], u[3], t[3]; };

inline GridLayout pv_layout(size_t n, int binnr) {
    return GridLayout(1, n, 0, grid_cells_cap(n, 1), sizeof(PvObj), (size_t)PV_GRID * (size_t)binnr * 24);
}

// One thread per object: r (widened to fp64), u = r / |r|, and the cartesian transverse velocity
// t = J(th = theta2, ph = theta1)^T (0, v1, v2) of get_sph_to_cart_jacobian (or v itself when 3 components are given).
// angle_mode 0: theta1 = arctan(x / z), theta2 = arctan(y / z), both + 10 deg; 1: given in radians; 2: given in degrees.
// The bounding box of r goes to `box` (grid_bounds_commit).
template <typename TP, typename TV>
__global__ void __launch_bounds__(256)
pv_prep_kernel(const TP* __restrict__ pos, const TV* __restrict__ vel, int vel_ncomp, const double* __restrict__ th1,
               const double* __restrict__ th2, int angle_mode, size_t n, PvObj* __restrict__ obj, GridBounds* box) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        PvObj o;
        const double x = (double)pos[3 * i], y = (double)pos[3 * i + 1], z = (double)pos[3 * i + 2];
        o.r[0] = x; o.r[1] = y; o.r[2] = z;
        const double nr = sqrt((x * x + y * y) + z * z);
        o.u[0] = x / nr; o.u[1] = y / nr; o.u[2] = z / nr;
        if (vel_ncomp == 3) {
            o.t[0] = (double)vel[3 * i]; o.t[1] = (double)vel[3 * i + 1]; o.t[2] = (double)vel[3 * i + 2];
        } else {
            double ph, th;
            if (angle_mode == 0) {
                constexpr double shift = 10 * M_PI / 180;
                ph = atan(x / z) + shift;
                th = atan(y / z) + shift;
            } else if (angle_mode == 2) {
                ph = th1[i] * (M_PI / 180.0);
                th = th2[i] * (M_PI / 180.0);
            } else {
                ph = th1[i];
                th = th2[i];
            }
            const double v1 = (double)vel[2 * i], v2 = (double)vel[2 * i + 1];
            const double st = sin(th), ct = cos(th), sp = sin(ph), cp = cos(ph);
            // einsum('ij...,i...->j...', J, (0, v1, v2)): rows 2 and 3 of J weighted by v1, v2
            o.t[0] = (0.0 + v1 * (ct * cp)) + v2 * (-sp);
            o.t[1] = (0.0 + v1 * (ct * sp)) + v2 * cp;
            o.t[2] = (0.0 + v1 * (-st)) + v2 * (0.0 * ct);
        }
        obj[i] = o;
        for (int a = 0; a < 3; ++a) { lo[a] = fmin(lo[a], o.r[a]); hi[a] = fmax(hi[a], o.r[a]); }
    }
    grid_bounds_commit<256>(lo, hi, box);
}

// The walk of cell_grid.h (grid_pair_walk: one set, open boundaries) with r, u, t of the staged j objects in LDS.  Each
// wave adds into its own LDS histogram (nom, denom, pairs), and at the end the workgroup's row (waves summed in order)
// is stored to part - no global atomics.
__global__ void __launch_bounds__(PV_BLOCK)
pv_pair_kernel(const PvObj* __restrict__ sorted, const unsigned* __restrict__ cell_start,
               const unsigned* __restrict__ tile_start, const GridBoxParams* prm, int binnr, double binwidth,
               double reach2, double* __restrict__ part) {
    extern __shared__ double lds[];
    double* jr = lds;                                   // [9][PV_BLOCK]: r, u, t of the staged j objects
    double* hn = lds + 9 * PV_BLOCK;                    // [PV_WAVES][binnr]
    double* hd = hn + PV_WAVES * binnr;
    unsigned long long* hc = (unsigned long long*)(hd + PV_WAVES * binnr);
    const int tid = threadIdx.x, w = tid / 64;
    for (int k = tid; k < PV_WAVES * binnr; k += PV_BLOCK) { hn[k] = 0.0; hd[k] = 0.0; hc[k] = 0ull; }
    double* whn = hn + w * binnr;
    double* whd = hd + w * binnr;
    unsigned long long* whc = hc + w * binnr;

    PvObj oi;
    grid_pair_walk<PV_BLOCK>(
        cell_start, tile_start, cell_start, prm, false, true,
        [&](unsigned i) { oi = sorted[i]; },
        [](unsigned, int) {},
        [&](unsigned j, int t) {
            const PvObj oj = sorted[j];
            for (int c = 0; c < 3; ++c) {
                jr[c * PV_BLOCK + t] = oj.r[c];
                jr[(3 + c) * PV_BLOCK + t] = oj.u[c];
                jr[(6 + c) * PV_BLOCK + t] = oj.t[c];
            }
        },
        [&](int q) {
            const double ddx = oi.r[0] - jr[q], ddy = oi.r[1] - jr[PV_BLOCK + q], ddz = oi.r[2] - jr[2 * PV_BLOCK + q];
            const double d2 = (ddx * ddx + ddy * ddy) + ddz * ddz;
            if (!(d2 <= reach2)) return;
            const double d = sqrt(d2);
            const int bin = (int)(d / binwidth);
            if (bin >= binnr) return;
            const double px = ddx / d, py = ddy / d, pz = ddz / d;
            const double ujx = jr[3 * PV_BLOCK + q], ujy = jr[4 * PV_BLOCK + q], ujz = jr[5 * PV_BLOCK + q];
            const double pi_ = (px * oi.u[0] + py * oi.u[1]) + pz * oi.u[2];
            const double pj_ = (px * ujx + py * ujy) + pz * ujz;
            const double qx = 0.5 * ((2.0 * px - oi.u[0] * pi_) - ujx * pj_);
            const double qy = 0.5 * ((2.0 * py - oi.u[1] * pi_) - ujy * pj_);
            const double qz = 0.5 * ((2.0 * pz - oi.u[2] * pi_) - ujz * pj_);
            const double tx = oi.t[0] - jr[6 * PV_BLOCK + q], ty = oi.t[1] - jr[7 * PV_BLOCK + q],
                         tz = oi.t[2] - jr[8 * PV_BLOCK + q];
            atomicAdd(&whn[bin], (tx * qx + ty * qy) + tz * qz);
            atomicAdd(&whd[bin], (qx * qx + qy * qy) + qz * qz);
            atomicAdd(&whc[bin], 1ull);
        });
    __syncthreads();
    grid_store_rows<PV_WAVES, PV_GRID>(hn, hd, hc, binnr, part);
}

}  // namespace

extern "C" size_t ast_pairwise_workspace_bytes(size_t n, int binnr) {
    if (binnr < 1 || binnr > PV_MAX_BINS) return 0;
    return pv_layout(n, binnr).total;
}

extern "C" int ast_pairwise_max_bins(void) { return PV_MAX_BINS; }

extern "C" int ast_pairwise_tv_prepare(const void* pos_d, int pos_dtype, const void* vel_d, int vel_dtype, int vel_ncomp,
                                       const double* theta1_d, const double* theta2_d, int angle_mode, size_t n,
                                       void* work_d, size_t work_bytes, void* stream) {
    AST_CHECK_ARG(pos_dtype == AST_F32 || pos_dtype == AST_F64);
    AST_CHECK_ARG(vel_dtype == AST_F32 || vel_dtype == AST_F64);
    AST_CHECK_ARG(vel_ncomp == 2 || vel_ncomp == 3);
    AST_CHECK_ARG(angle_mode >= 0 && angle_mode <= 2);
    AST_CHECK_ARG(angle_mode == 0 || vel_ncomp == 3 || n == 0 || (theta1_d && theta2_d));
    AST_CHECK_ARG(grid_count_ok(n));
    AST_CHECK_ARG(n == 0 || (pos_d && vel_d));
    const GridLayout L = pv_layout(n, 1);
    AST_CHECK_ARG(work_d && work_bytes >= L.sorted[0]);
    hipStream_t s = ast::as_stream(stream);
    return grid_prepare<1, PvObj>((char*)work_d, L, &n, nullptr, "pairwise_prep", s,
                                  [&](int, PvObj* obj, GridBounds* box) {
        ast::dispatch_f32_f64(pos_dtype == AST_F32, vel_dtype == AST_F32, [&](auto tp, auto tv) {
            using TP = decltype(tp);
            using TV = decltype(tv);
            pv_prep_kernel<TP, TV><<<ast::stream_grid(n, 256), 256, 0, s>>>(
                (const TP*)pos_d, (const TV*)vel_d, vel_ncomp, theta1_d, theta2_d, angle_mode, n, obj, box);
        });
    });
}

extern "C" int ast_pairwise_tv(void* work_d, size_t work_bytes, size_t n, int binnr, double binwidth, int single_cell,
                               double* nom_d, double* denom_d, unsigned long long* counts_d, void* stream) {
    AST_CHECK_ARG(binnr >= 1 && binnr <= PV_MAX_BINS);
    AST_CHECK_ARG(binwidth > 0.0 && std::isfinite(binwidth));
    AST_CHECK_ARG(grid_count_ok(n));
    AST_CHECK_ARG(nom_d && denom_d && counts_d);
    AST_CHECK_ARG(work_d && work_bytes >= ast_pairwise_workspace_bytes(n, binnr));
    hipStream_t s = ast::as_stream(stream);
    if (grid_no_pairs(1, n, 0)) {
        AST_CHECK_HIP(hipMemsetAsync(nom_d, 0, binnr * sizeof(double), s));
        AST_CHECK_HIP(hipMemsetAsync(denom_d, 0, binnr * sizeof(double), s));
        AST_CHECK_HIP(hipMemsetAsync(counts_d, 0, binnr * sizeof(unsigned long long), s));
        return AST_OK;
    }
    const GridLayout L = pv_layout(n, binnr);
    char* ws = (char*)work_d;
    const GridSorted<PvObj> g(ws, L, 0);
    const double rmax = (double)binnr * binwidth;
    {
        AST_PROF("pairwise_grid", s);
        grid_box_plan_kernel<<<1, 64, 0, s>>>(g.prm, rmax, (unsigned)L.cap, single_cell);
        AST_CHECK_LAUNCH();
        if (int rc = grid_sort_sets<PV_BLOCK, PvObj>(ws, L, 0, &n, s)) return rc;
    }
    // Pre-test on d^2 with a relative margin far above the rounding of d and d / binwidth: every pair whose
    // int(d / binwidth) < binnr passes it; the bin decision itself is the fp64 int(d / binwidth) < binnr.
    const double reach2 = rmax * rmax * (1.0 + 1e-12);
    const size_t lds = (size_t)9 * PV_BLOCK * sizeof(double) + (size_t)PV_WAVES * binnr * 24;
    {
        AST_PROF("pairwise_pairs", s);
        pv_pair_kernel<<<PV_GRID, PV_BLOCK, lds, s>>>(g.sorted1, g.cell_start1, g.tile_start1, g.prm, binnr, binwidth,
                                                      reach2, g.part);
        AST_CHECK_LAUNCH();
    }
    {
        AST_PROF("pairwise_reduce", s);
        grid_reduce3_kernel<PV_GRID><<<(binnr + 255) / 256, 256, 0, s>>>(g.part, binnr, nom_d, denom_d, counts_d);
        AST_CHECK_LAUNCH();
    }
    return AST_OK;
}
