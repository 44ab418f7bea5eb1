// Uniform cell grid shared by the pair finders (pairwise.hip, pairwise_pdf.hip, tpcf.hip): objects sorted by cell with a
// counting sort (a count kernel -> grid_scan_kernel -> grid_scatter_kernel), and a work list of (tile of BLOCK objects of
// a cell, one of the GRID_NEIGH half-shell neighbours) that a persistent pair kernel walks.  The grid_box_* part is the
// non-periodic grid over the catalogue's bounding box (pairwise.hip, pairwise_pdf.hip, and tpcf.hip for open
// boundaries); tpcf.hip plans its own periodic one.  Everything here has internal linkage: each translation unit gets
// its own copy of the kernels and of the offset table.
#pragma once
#include "ast_common.h"

namespace {

constexpr int GRID_NEIGH = 14;              // the cell itself + 13 half-shell neighbours

// Half-shell neighbour offsets: with every other cell's 13 opposite offsets, each unordered pair of adjacent cells is
// visited once (the cell itself, k = 0, covers the pairs inside a cell).
__constant__ int grid_offsets[GRID_NEIGH][3] = {
    {0, 0, 0},
    {1, 0, 0},
    {-1, 1, 0}, {0, 1, 0}, {1, 1, 0},
    {-1, -1, 1}, {0, -1, 1}, {1, -1, 1},
    {-1, 0, 1}, {0, 0, 1}, {1, 0, 1},
    {-1, 1, 1}, {0, 1, 1}, {1, 1, 1},
};

inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

// One workgroup of 1024: exclusive scans of the cell counts (-> cell_start, cursor) and of the tiles per cell,
// ceil(count / BLOCK) (-> tile_start); prm->ntiles = the total.  Each thread scans a contiguous chunk of the
// prm->ncells cells.
template <int BLOCK, typename Params>
__global__ void __launch_bounds__(1024)
grid_scan_kernel(const unsigned* __restrict__ cnt, Params* prm, unsigned* __restrict__ cell_start,
                 unsigned* __restrict__ tile_start, unsigned* __restrict__ cursor) {
    __shared__ unsigned s_obj[1024], s_til[1024];
    const unsigned nc = prm->ncells;
    const unsigned chunk = (nc + 1023) / 1024;
    const unsigned c0 = threadIdx.x * chunk, c1 = min(nc, c0 + chunk);
    unsigned so = 0, st = 0;
    for (unsigned c = c0; c < c1; ++c) { so += cnt[c]; st += (cnt[c] + BLOCK - 1) / BLOCK; }
    s_obj[threadIdx.x] = so;
    s_til[threadIdx.x] = st;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned ao = 0, at = 0;
        for (int k = 0; k < 1024; ++k) {
            const unsigned vo = s_obj[k], vt = s_til[k];
            s_obj[k] = ao; s_til[k] = at;
            ao += vo; at += vt;
        }
        cell_start[nc] = ao;
        tile_start[nc] = at;
        prm->ntiles = at;
    }
    __syncthreads();
    so = s_obj[threadIdx.x];
    st = s_til[threadIdx.x];
    for (unsigned c = c0; c < c1; ++c) {
        cell_start[c] = so;
        cursor[c] = so;
        tile_start[c] = st;
        so += cnt[c];
        st += (cnt[c] + BLOCK - 1) / BLOCK;
    }
}

template <typename Obj>
__global__ void __launch_bounds__(256)
grid_scatter_kernel(const Obj* __restrict__ obj, size_t n, const unsigned* __restrict__ cell_of,
                    unsigned* __restrict__ cursor, Obj* __restrict__ sorted) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const unsigned slot = atomicAdd(&cursor[cell_of[i]], 1u);
        sorted[slot] = obj[i];
    }
}

// The cell whose tiles hold `tile`: tile_start[cell] <= tile < tile_start[cell + 1].
__device__ inline unsigned grid_cell_of_tile(const unsigned* __restrict__ tile_start, unsigned ncells, unsigned tile) {
    unsigned lo = 0, hi = ncells;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) / 2;
        if (tile_start[mid] <= tile) lo = mid; else hi = mid;
    }
    return lo;
}

// Order-preserving keys of doubles, for a bounding box kept with integer atomicMin / atomicMax.
__device__ inline unsigned long long d2key(double d) {
    unsigned long long u = (unsigned long long)__double_as_longlong(d);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline double key2d(unsigned long long k) {
    unsigned long long u = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}
__device__ inline double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ inline double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- the non-periodic grid over a bounding box; Obj needs `double r[3]`
constexpr size_t GRID_BOX_MAX_CELLS = size_t(1) << 20;

struct GridBoxParams {
    unsigned long long kmin[3], kmax[3];    // bounding box as order-preserving keys (atomicMin / atomicMax)
    double lo[3], inv_cs[3];
    int dims[3];
    unsigned ncells, ntiles;
};

inline size_t grid_box_cells_cap(size_t n) { return n < 1 ? 1 : (n < GRID_BOX_MAX_CELLS ? n : GRID_BOX_MAX_CELLS); }

// The grid, planned by one thread (grid_box_plan_kernel, or a caller's own plan kernel whose reach lives in device
// memory).  Cells are at least s = rmax (1 + 1e-6) wide per axis, plus a margin for the rounding
// of coordinates far from the origin, so a pair within reach lies in the same or an adjacent cell; at most `cap`
// cells in all (wider cells past that).  single != 0: one cell.  (A template so that only the files that launch it
// carry a copy.)
template <typename Params>
__device__ inline void grid_box_plan(Params* prm, double rmax, unsigned cap, int single) {
    double lo[3], ext[3], amax = 0.0;
    for (int a = 0; a < 3; ++a) {
        lo[a] = key2d(prm->kmin[a]);
        const double hi = key2d(prm->kmax[a]);
        ext[a] = hi - lo[a];
        amax = fmax(amax, fmax(fabs(lo[a]), fabs(hi)));
    }
    int dims[3] = {1, 1, 1};
    if (!single) {
        double s = rmax * (1.0 + 1e-6) + amax * 1e-12;
        for (;;) {
            double prod = 1.0;
            for (int a = 0; a < 3; ++a) {
                double m = floor(ext[a] / s);
                if (!(m >= 1.0)) m = 1.0;
                if (m > (double)GRID_BOX_MAX_CELLS) m = (double)GRID_BOX_MAX_CELLS;
                dims[a] = (int)m;
                prod *= m;
            }
            if (prod <= (double)cap) break;
            s *= 1.25;
        }
    }
    for (int a = 0; a < 3; ++a) {
        prm->lo[a] = lo[a];
        prm->dims[a] = dims[a];
        prm->inv_cs[a] = dims[a] > 1 ? (double)dims[a] / ext[a] : 0.0;
    }
    prm->ncells = (unsigned)dims[0] * (unsigned)dims[1] * (unsigned)dims[2];
}

template <typename Params>
__global__ void grid_box_plan_kernel(Params* prm, double rmax, unsigned cap, int single) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    grid_box_plan(prm, rmax, cap, single);
}

template <typename Obj>
__device__ inline unsigned grid_box_cell(const Obj& o, const GridBoxParams& p) {
    int c[3];
    for (int a = 0; a < 3; ++a) {
        double v = (o.r[a] - p.lo[a]) * p.inv_cs[a];
        const double top = (double)(p.dims[a] - 1);
        if (!(v >= 0.0)) v = 0.0;
        if (v > top) v = top;
        c[a] = (int)v;
    }
    return ((unsigned)c[2] * (unsigned)p.dims[1] + (unsigned)c[1]) * (unsigned)p.dims[0] + (unsigned)c[0];
}

template <typename Obj>
__global__ void __launch_bounds__(256)
grid_box_count_kernel(const Obj* __restrict__ obj, size_t n, const GridBoxParams* prm, unsigned* __restrict__ cell_of,
                      unsigned* __restrict__ cnt) {
    const GridBoxParams p = *prm;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const unsigned c = grid_box_cell(obj[i], p);
        cell_of[i] = c;
        atomicAdd(&cnt[c], 1u);
    }
}

}  // namespace
