// Radial profiles of objects on a 2D map (profiles/profile_2d.py: from_map / profiling): per object, the sums and counts
// of the map pixels in each annulus of its (2R)^2 square.  The host decides every bin with exact integer thresholds on
// d2 = a^2 + b^2 (profile_2d.py restates numpy's eta there), so the device only compares integers.  Work items are
// (object, band of rows); a persistent grid walks them, each band writes its own partial row, and a second kernel sums
// an object's bands in band order.  Map values are widened to fp64 on load; all sums are fp64 in an order fixed by the
// object's geometry, so repeated calls are bit-identical.  No float atomics.
#include "ast_common.h"
#include <cmath>

namespace {

constexpr int PF_BLOCK = 256;
constexpr int PF_GRID = 2048;               // persistent band-kernel workgroups (256 CUs x 8)
constexpr int PF_MAX_BINS = 1024;
constexpr int PF_BAND_ROWS = 32;            // map rows per work item

inline size_t pf_align(size_t b) { return (b + 255) & ~size_t(255); }

struct PfLayout {
    size_t part_s, part_c, total;
    PfLayout(size_t n_work, int nbins) {
        size_t o = 0;
        part_s = o; o += pf_align(n_work * (size_t)nbins * sizeof(double));
        part_c = o; o += pf_align(n_work * (size_t)nbins * sizeof(long long));
        total = o;
    }
};

// Rows of map per LDS stage: (row, bin) tasks fill at most one task per thread.
__host__ __device__ inline int pf_chunk_rows(int nbins) { return nbins >= PF_BLOCK ? 1 : PF_BLOCK / nbins; }

inline size_t pf_lds_bytes(int nbins) {
    const size_t chunk = (size_t)pf_chunk_rows(nbins);
    return (size_t)(nbins + 1) * 8 + chunk * nbins * 16 + (size_t)nbins * 16;
}

// Smallest t >= 0 with t * t >= n.
__device__ inline long long ceil_sqrt(long long n) {
    if (n <= 0) return 0;
    long long t = (long long)sqrt((double)n);
    while (t * t < n) ++t;
    while (t > 0 && (t - 1) * (t - 1) >= n) --t;
    return t;
}

// The object whose items hold `item`: item_start[o] <= item < item_start[o + 1].
__device__ inline size_t pf_object_of(const long long* __restrict__ item_start, size_t n_obj, long long item) {
    size_t lo = 0, hi = n_obj;
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) / 2;
        if (item_start[mid] <= item) lo = mid; else hi = mid;
    }
    return lo;
}

// Work item = (object o, rows [a0, a1) of its square), a0 = -m + band * band_rows (band_rows == 0: all rows
// [-m, min(m, R - 1)] in one item).  The rows pass through LDS pf_chunk_rows(nbins) at a time: one thread per
// (row a, bin k) sums the pixels of the bin in that row, T_k <= a^2 + b^2 < T_{k+1} with -R <= b < R, which are two
// runs of columns symmetric about b = 0: the negative run in ascending b, then the non-negative one.  Then thread k adds
// the chunk's row sums to the band's running sum in row order.  Row and column indices below 0 wrap once (numpy's
// negative indices); an object whose reach leaves [-n, n) on either axis is not read: its rows get NaN and count -1
// (the host checks this before the launch).
template <typename T>
__global__ void __launch_bounds__(PF_BLOCK)
pf_band_kernel(const T* __restrict__ map, long long ny, long long nx, size_t n_obj, const long long* __restrict__ centres,
               const long long* __restrict__ reach, const long long* __restrict__ thresholds, int nbins, int band_rows,
               const long long* __restrict__ item_start, size_t n_work, double* __restrict__ part_s,
               long long* __restrict__ part_c) {
    extern __shared__ double lds[];
    const int chunk = pf_chunk_rows(nbins);
    long long* thr = (long long*)lds;                           // [nbins + 1]: T_0 = 0, T_1 .. T_nbins
    double* rs = lds + (nbins + 1);                             // [chunk][nbins] row sums
    long long* rc = (long long*)(rs + (size_t)chunk * nbins);   // [chunk][nbins] row counts
    double* acs = (double*)(rc + (size_t)chunk * nbins);        // [nbins] band sums
    long long* acc = (long long*)(acs + nbins);                 // [nbins] band counts
    const int tid = threadIdx.x;
    for (size_t item = blockIdx.x; item < n_work; item += gridDim.x) {
        const size_t o = pf_object_of(item_start, n_obj, (long long)item);
        const long long y = centres[2 * o], x = centres[2 * o + 1];
        const long long R = reach[2 * o], m = reach[2 * o + 1];
        const long long mtop = m < R - 1 ? m : R - 1;
        const bool valid = y - m >= -ny && y + mtop < ny && x - m >= -nx && x + mtop < nx;
        long long a0 = -m, a1 = mtop + 1;
        if (band_rows > 0) {
            a0 = -m + (long long)(item - (size_t)item_start[o]) * band_rows;
            a1 = a0 + band_rows < mtop + 1 ? a0 + band_rows : mtop + 1;
        }
        __syncthreads();                                        // the previous item is done with LDS
        for (int k = tid; k <= nbins; k += PF_BLOCK) thr[k] = k == 0 ? 0 : thresholds[o * nbins + (k - 1)];
        for (int k = tid; k < nbins; k += PF_BLOCK) { acs[k] = 0.0; acc[k] = 0; }
        __syncthreads();
        for (long long c0 = a0; valid && c0 < a1; c0 += chunk) {
            const int rows = (int)(a1 - c0 < chunk ? a1 - c0 : chunk);
            for (int task = tid; task < rows * nbins; task += PF_BLOCK) {
                const long long a = c0 + task / nbins;
                const int k = task % nbins;
                const long long a2 = a * a;
                const long long hi2 = thr[k + 1] - a2;
                double s = 0.0;
                long long c = 0;
                if (hi2 > 0) {
                    const long long lo2 = thr[k] - a2;
                    const long long blo = ceil_sqrt(lo2 > 0 ? lo2 : 0), bhi = ceil_sqrt(hi2) - 1;
                    long long row = y + a;
                    if (row < 0) row += ny;
                    const T* rp = map + (size_t)row * (size_t)nx;
                    const long long nlo = blo > 1 ? blo : 1, nhi = bhi < R ? bhi : R;
                    for (long long b = -nhi; b <= -nlo; ++b) {
                        long long col = x + b;
                        if (col < 0) col += nx;
                        s += (double)rp[col];
                    }
                    const long long phi = bhi < R - 1 ? bhi : R - 1;
                    for (long long b = blo; b <= phi; ++b) {
                        long long col = x + b;
                        if (col < 0) col += nx;
                        s += (double)rp[col];
                    }
                    c = (nhi >= nlo ? nhi - nlo + 1 : 0) + (phi >= blo ? phi - blo + 1 : 0);
                }
                rs[task] = s;
                rc[task] = c;
            }
            __syncthreads();
            for (int k = tid; k < nbins; k += PF_BLOCK) {
                double s = acs[k];
                long long c = acc[k];
                for (int r = 0; r < rows; ++r) { s += rs[r * nbins + k]; c += rc[r * nbins + k]; }
                acs[k] = s;
                acc[k] = c;
            }
            __syncthreads();
        }
        for (int k = tid; k < nbins; k += PF_BLOCK) {
            part_s[item * nbins + k] = valid ? acs[k] : NAN;
            part_c[item * nbins + k] = valid ? acc[k] : -1;
        }
    }
}

// sums[o][k] = the object's band rows of part_s added in band order (counts likewise).
__global__ void __launch_bounds__(256)
pf_reduce_kernel(const double* __restrict__ part_s, const long long* __restrict__ part_c,
                 const long long* __restrict__ item_start, size_t n_obj, int nbins, size_t n_work,
                 double* __restrict__ sums, long long* __restrict__ counts) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_obj * (size_t)nbins) return;
    const size_t o = idx / nbins;
    const int k = (int)(idx % nbins);
    const size_t i0 = (size_t)item_start[o] < n_work ? (size_t)item_start[o] : n_work;
    const size_t i1 = (size_t)item_start[o + 1] < n_work ? (size_t)item_start[o + 1] : n_work;
    double s = 0.0;
    long long c = 0;
    for (size_t i = i0; i < i1; ++i) { s += part_s[i * nbins + k]; c += part_c[i * nbins + k]; }
    sums[idx] = s;
    counts[idx] = c;
}

}  // namespace

extern "C" int ast_profile2d_max_bins(void) { return PF_MAX_BINS; }

extern "C" int ast_profile2d_band_rows(void) { return PF_BAND_ROWS; }

extern "C" size_t ast_profile2d_workspace_bytes(size_t n_obj, size_t n_work, int nbins) {
    if (nbins < 1 || nbins > PF_MAX_BINS || n_work < n_obj) return 0;
    return PfLayout(n_work, nbins).total;
}

extern "C" int ast_profile2d(const void* map_d, int dtype, size_t ny, size_t nx, size_t n_obj,
                             const long long* centres_d, const long long* reach_d, const long long* thresholds_d,
                             int nbins, int band_rows, const long long* item_start_d, size_t n_work, void* work_d,
                             size_t work_bytes, double* sums_d, long long* counts_d, void* stream) {
    AST_CHECK_ARG(dtype == AST_F32 || dtype == AST_F64);
    AST_CHECK_ARG(nbins >= 1 && nbins <= PF_MAX_BINS);
    AST_CHECK_ARG(band_rows >= 0);
    AST_CHECK_ARG(ny >= 1 && nx >= 1 && ny < (size_t(1) << 31) && nx < (size_t(1) << 31));
    AST_CHECK_ARG(n_obj >= 1 && n_work >= n_obj && n_work < (size_t(1) << 40));
    AST_CHECK_ARG(map_d && centres_d && reach_d && thresholds_d && item_start_d && sums_d && counts_d);
    AST_CHECK_ARG(work_d && work_bytes >= ast_profile2d_workspace_bytes(n_obj, n_work, nbins));
    hipStream_t s = ast::as_stream(stream);
    const PfLayout L(n_work, nbins);
    char* ws = (char*)work_d;
    double* part_s = (double*)(ws + L.part_s);
    long long* part_c = (long long*)(ws + L.part_c);
    const size_t lds = pf_lds_bytes(nbins);
    const unsigned grid = (unsigned)(n_work < (size_t)PF_GRID ? n_work : (size_t)PF_GRID);
    {
        AST_PROF("profile2d_bands", s);
        if (dtype == AST_F32)
            pf_band_kernel<float><<<grid, PF_BLOCK, lds, s>>>((const float*)map_d, (long long)ny, (long long)nx, n_obj,
                                                               centres_d, reach_d, thresholds_d, nbins, band_rows,
                                                               item_start_d, n_work, part_s, part_c);
        else
            pf_band_kernel<double><<<grid, PF_BLOCK, lds, s>>>((const double*)map_d, (long long)ny, (long long)nx,
                                                                n_obj, centres_d, reach_d, thresholds_d, nbins,
                                                                band_rows, item_start_d, n_work, part_s, part_c);
        AST_CHECK_LAUNCH();
    }
    {
        AST_PROF("profile2d_reduce", s);
        const size_t n = n_obj * (size_t)nbins;
        pf_reduce_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(part_s, part_c, item_start_d, n_obj, nbins,
                                                                     n_work, sums_d, counts_d);
        AST_CHECK_LAUNCH();
    }
    return AST_OK;
}
