// Uniform cell grid shared by the pair finders (pairwise.hip, pairwise_pdf.hip, tpcf.hip, pair_velocity.hip); its bounds
// and scatter also serve profile3d.hip, its scan and scatter tunnels.hip.  In the order of a call:
//   bounds     GridBounds (order-preserving keys), grid_bounds_reset, grid_bounds_commit (the workgroup tail of every
//              prep kernel) and grid_bounds_kernel (the box of one set, or of two and their union, to the caller);
//   plan       grid_box_plan over a bounding box, grid_periodic_plan over a periodic cube, grid_plan choosing by boxsize;
//              grid_cyl_plan, either of them with a reach per axis, for a cylinder along a line of sight;
//   sort       grid_sort_set: clear, grid_box_count_kernel, grid_scan_kernel, grid_scatter_kernel;
//   workspace  GridLayout, the one layout of a pair finder's scratch memory for one or two sets;
//   host       grid_prepare, grid_sort_sets and GridSorted: a pair finder's entry points around its own kernels;
//   walk       grid_pair_walk, the one walk of (tile of BLOCK objects of a cell, neighbour cell) work items by a
//              persistent pair kernel, for one set or two, open or periodic;
//   rows       grid_store_rows and grid_reduce3_kernel for kernels that sum (fp64, fp64, u64) per bin.
// Everything here has internal linkage: each translation unit gets its own copy of what it uses (the kernels are
// templates, so a file carries only those it launches).
#pragma once
#include "ast_common.h"
#include <cstddef>
#include <type_traits>

namespace {

constexpr int GRID_NEIGH = 14;              // the cell itself + 13 half-shell neighbours
constexpr int GRID_NEIGH_ALL = 27;          // two sets: the cell itself and all 26 neighbours

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

// ---- bounds: a bounding box kept with integer atomicMin / atomicMax on order-preserving keys of doubles
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

struct GridBounds { unsigned long long kmin[3], kmax[3]; };     // empty: kmin > kmax

// The empty box, before a prep kernel.
inline int grid_bounds_reset(GridBounds* b, hipStream_t s) {
    AST_CHECK_HIP(hipMemsetAsync(b->kmin, 0xff, sizeof(b->kmin), s));
    AST_CHECK_HIP(hipMemsetAsync(b->kmax, 0x00, sizeof(b->kmax), s));
    return AST_OK;
}

// The tail of a prep kernel of BLOCK threads, called by all of them: each thread's min / max over its objects (what a
// NaN coordinate counts as is the caller's choice) -> wave -> workgroup -> one atomic per workgroup and axis.
template <int BLOCK>
__device__ inline void grid_bounds_commit(const double (&lo)[3], const double (&hi)[3], GridBounds* b) {
    static_assert(BLOCK % 64 == 0, "whole waves");
    constexpr int WAVES = BLOCK / 64;
    __shared__ double wlo[3][WAVES], whi[3][WAVES];
    const int w = threadIdx.x / 64, l = threadIdx.x % 64;
    for (int a = 0; a < 3; ++a) {
        const double mn = wave_min(lo[a]), mx = wave_max(hi[a]);
        if (l == 0) { wlo[a][w] = mn; whi[a][w] = mx; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        double mn = wlo[a][0], mx = whi[a][0];
        for (int k = 1; k < WAVES; ++k) { mn = fmin(mn, wlo[a][k]); mx = fmax(mx, whi[a][k]); }
        if (mn <= mx) {
            atomicMin(&b->kmin[a], d2key(mn));
            atomicMax(&b->kmax[a], d2key(mx));
        }
    }
}

// bounds[6 s + 0..2] = min, bounds[6 s + 3..5] = max of set s; (+inf, -inf) for an empty set.  NSETS == 2: the union
// of both boxes goes to `uni`, the shared grid's box (an empty set leaves the other's box; both empty: kmin > kmax, and
// nothing is planned).
template <int NSETS>
__global__ void grid_bounds_kernel(const GridBounds* b1, const GridBounds* b2, GridBounds* uni,
                                   double* __restrict__ bounds) {
    const int a = threadIdx.x;
    if (a >= 3) return;
    const GridBounds* b[2] = {b1, b2};
    unsigned long long umn = ~0ull, umx = 0ull;
    for (int s = 0; s < NSETS; ++s) {
        const unsigned long long kmn = b[s]->kmin[a], kmx = b[s]->kmax[a];
        bounds[6 * s + a] = kmn > kmx ? INFINITY : key2d(kmn);
        bounds[6 * s + 3 + a] = kmn > kmx ? -INFINITY : key2d(kmx);
        umn = kmn < umn ? kmn : umn;
        umx = kmx > umx ? kmx : umx;
    }
    if (NSETS == 2) {
        uni->kmin[a] = umn;
        uni->kmax[a] = umx;
    }
}

// ---- plan; Obj needs `double r[3]`
constexpr size_t GRID_MAX_CELLS = size_t(1) << 20;

struct GridBoxParams {
    GridBounds box;                         // of the objects (one set) or of both sets (two)
    double lo[3], inv_cs[3];
    int dims[3];
    unsigned ncells, ntiles;
};
static_assert(offsetof(GridBoxParams, lo) == 48 && offsetof(GridBoxParams, inv_cs) == 72 &&
              offsetof(GridBoxParams, dims) == 96 && offsetof(GridBoxParams, ncells) == 108 &&
              offsetof(GridBoxParams, ntiles) == 112, "the tests read GridBoxParams back at these offsets");

// Cells that a grid for n objects may have: n, within [min_cells, GRID_MAX_CELLS] (a periodic grid needs 27).
inline size_t grid_cells_cap(size_t n, size_t min_cells) {
    return n < min_cells ? min_cells : (n < GRID_MAX_CELLS ? n : GRID_MAX_CELLS);
}

// The non-periodic grid over prm->box, planned by one thread.  Cells are at least s = rmax (1 + 1e-6) wide per axis,
// plus a margin for the rounding of coordinates far from the origin, so a pair within reach lies in the same or an
// adjacent cell; at most `cap` cells in all (wider cells past that).  single != 0: one cell.
__device__ inline void grid_box_plan(GridBoxParams* prm, double rmax, unsigned cap, int single) {
    double lo[3], ext[3], amax = 0.0;
    for (int a = 0; a < 3; ++a) {
        lo[a] = key2d(prm->box.kmin[a]);
        const double hi = key2d(prm->box.kmax[a]);
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
                if (m > (double)GRID_MAX_CELLS) m = (double)GRID_MAX_CELLS;
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

// The periodic grid of the cube [0, boxsize]^3, planned by one thread: floor(L / (reach (1 + 1e-6))) cells per axis,
// at most 1024, fewer while the cube exceeds `cap`, at least 3 so that the 27 neighbours of a cell are distinct; one
// cell when even 3 would be narrower than the reach (reach >= L / 3, which the Python API refuses) or when `single` is
// set.
__device__ inline void grid_periodic_plan(GridBoxParams* prm, double reach, double boxsize, unsigned cap, int single) {
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

// boxsize > 0: the periodic plan; boxsize == 0: the plan over the bounding box, per-axis dims that may be 1.
__device__ inline void grid_plan(GridBoxParams* prm, double reach, double boxsize, unsigned cap, int single) {
    if (boxsize > 0.0) grid_periodic_plan(prm, reach, boxsize, cap, single);
    else grid_box_plan(prm, reach, cap, single);
}

// For a reach that the host knows.
// (Params is always GridBoxParams: a template only because a plain __global__ function is emitted into every file that
// includes this header, launched or not.)
template <typename Params>
__global__ void grid_box_plan_kernel(Params* prm, double rmax, unsigned cap, int single) {
    static_assert(std::is_same<Params, GridBoxParams>::value, "grid_box_plan_kernel plans a GridBoxParams");
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    grid_box_plan(prm, rmax, cap, single);
}

// For a reach in device memory: the top edge, edges[nb], itself (pi_max <= 0), or sqrt(top^2 + pi_max^2) for pairs
// within the top edge across and pi_max along a line of sight (grid_plan: periodic when boxsize > 0, else over the
// bounding box).
template <typename Params>
__global__ void grid_edge_plan_kernel(Params* prm, const double* __restrict__ edges, int nb, double pi_max,
                                      double boxsize, unsigned cap, int single) {
    static_assert(std::is_same<Params, GridBoxParams>::value, "grid_edge_plan_kernel plans a GridBoxParams");
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double top = edges[nb];
    grid_plan(prm, pi_max > 0.0 ? sqrt(top * top + pi_max * pi_max) : top, boxsize, cap, single);
}

// The grid of a cylinder search, planned by one thread: pairs within rp_top across and pi_max along axis `los`, so
// the reach of an axis is pi_max on `los` and rp_top on the other two, and every axis gets cells of its own width.
// boxsize > 0, the periodic cube: floor(L / (reach_c (1 + 1e-6))) cells on axis c, at most 1024; an axis that would
// get fewer than 3 gets exactly 1 (the walk skips its +-1 offsets, as for the one cell of a periodic plan, and the
// minimum image of the pair arithmetic does the rest); while the grid exceeds `cap`, both reaches times 1.25.
// boxsize == 0: grid_box_plan's rule over prm->box with the reach of each axis, its amax 1e-12 margin and its 1.25
// growth (of every axis' width) until the grid fits `cap`.  single != 0, or a reach that is not positive (which no
// growth would change): one cell.
__device__ inline void grid_cyl_plan(GridBoxParams* prm, double rp_top, double pi_max, int los, double boxsize,
                                     unsigned cap, int single) {
    double reach[3], lo[3] = {0.0, 0.0, 0.0}, ext[3] = {boxsize, boxsize, boxsize};
    for (int a = 0; a < 3; ++a) reach[a] = (a == los ? pi_max : rp_top) * (1.0 + 1e-6);
    const bool periodic = boxsize > 0.0;
    if (!periodic) {
        double amax = 0.0;
        for (int a = 0; a < 3; ++a) {
            lo[a] = key2d(prm->box.kmin[a]);
            const double hi = key2d(prm->box.kmax[a]);
            ext[a] = hi - lo[a];
            amax = fmax(amax, fmax(fabs(lo[a]), fabs(hi)));
        }
        for (int a = 0; a < 3; ++a) reach[a] += amax * 1e-12;
    }
    int dims[3] = {1, 1, 1};
    if (!single && reach[0] > 0.0 && reach[1] > 0.0 && reach[2] > 0.0) {
        for (;;) {
            double prod = 1.0;
            for (int a = 0; a < 3; ++a) {
                double m = floor(ext[a] / reach[a]);
                if (periodic) m = m >= 3.0 ? (m > 1024.0 ? 1024.0 : m) : 1.0;
                else m = !(m >= 1.0) ? 1.0 : (m > (double)GRID_MAX_CELLS ? (double)GRID_MAX_CELLS : m);
                dims[a] = (int)m;
                prod *= m;
            }
            if (prod <= (double)cap) break;
            for (int a = 0; a < 3; ++a) reach[a] *= 1.25;
        }
    }
    for (int a = 0; a < 3; ++a) {
        prm->lo[a] = lo[a];
        prm->dims[a] = dims[a];
        prm->inv_cs[a] = dims[a] > 1 ? (double)dims[a] / ext[a] : 0.0;
    }
    prm->ncells = (unsigned)dims[0] * (unsigned)dims[1] * (unsigned)dims[2];
}

// For a cylinder whose reaches are in device memory: the top edges rp_edges[nrp] and pi_edges[npi].  iso == 0: the
// plan above; iso != 0: the isotropic plan that grid_edge_plan_kernel makes for pi_max = pi_edges[npi], cells of
// sqrt(rp_top^2 + pi_max^2) on every axis.
template <typename Params>
__global__ void grid_cyl_plan_kernel(Params* prm, const double* __restrict__ rp_edges, int nrp,
                                     const double* __restrict__ pi_edges, int npi, int los, double boxsize,
                                     unsigned cap, int single, int iso) {
    static_assert(std::is_same<Params, GridBoxParams>::value, "grid_cyl_plan_kernel plans a GridBoxParams");
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double top = rp_edges[nrp], pi_max = pi_edges[npi];
    if (iso) grid_plan(prm, sqrt(top * top + pi_max * pi_max), boxsize, cap, single);
    else grid_cyl_plan(prm, top, pi_max, los, boxsize, cap, single);
}

// ---- sort: objects ordered by cell with a counting sort
// Cell of an object: floor((x - lo) * inv_cs) per axis, clamped to [0, dims - 1] (the top face goes to the last cell,
// a NaN to cell 0); x-fastest.
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

// One workgroup of 1024: exclusive scans of the cell counts (-> cell_start, cursor) and of the tiles per cell,
// ceil(count / BLOCK) (-> tile_start); prm->ntiles = the total.  Each thread scans a contiguous chunk of the
// prm->ncells cells (Params: GridBoxParams, or another grid's with ncells and ntiles).
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

// ---- workspace of a pair finder.  One set: the grid (at byte 0), whose box is the set's own (bounds[0] == grid).  Two
// sets: one grid shared by both, whose box is the union, and per set its own bounds.  Then the scatter's cursor; per
// set: counts, cell starts, tile starts, cell numbers, records of `rec` bytes and their cell-sorted copy; at the end
// `part_bytes` of workgroup rows.  Only set 1 has tiles; tile_start[1] is where the scan of set 2 puts the tile list
// nobody reads.  Everything before `part` is independent of the bin counts, and a prepare call writes nothing past
// the last set's obj.
struct GridLayout {
    size_t cap, grid, cursor, bounds[2] = {}, cnt[2] = {}, cell_start[2] = {}, tile_start[2] = {}, cell_of[2] = {},
           obj[2] = {}, sorted[2] = {}, part, total;
    GridLayout(int nsets, size_t n1, size_t n2, size_t cells_cap, size_t rec, size_t part_bytes) : cap(cells_cap) {
        const size_t n[2] = {n1, n2};
        size_t o = 0;
        grid = o;   o += align256(sizeof(GridBoxParams));
        cursor = o; o += align256(cap * 4);
        for (int s = 0; s < nsets; ++s) {
            bounds[s] = nsets == 1 ? grid : o;
            if (nsets == 2) o += align256(sizeof(GridBounds));
            cnt[s] = o;        o += align256(cap * 4);
            cell_start[s] = o; o += align256((cap + 1) * 4);
            tile_start[s] = o; o += align256((cap + 1) * 4);
            cell_of[s] = o;    o += align256(n[s] * 4);
            obj[s] = o;        o += align256(n[s] * rec);
            sorted[s] = o;     o += align256(n[s] * rec);
        }
        part = o; o += align256(part_bytes);
        total = o;
    }
};

// Sort set q (n objects at L.obj[q]) into the planned grid at ws + L.grid: clear the counts, count, scan, scatter.
// The scan leaves the set's tile count in prm->ntiles, so set 1 is sorted last.
template <int BLOCK, typename Obj>
int grid_sort_set(char* ws, const GridLayout& L, int q, size_t n, hipStream_t s) {
    GridBoxParams* prm = (GridBoxParams*)(ws + L.grid);
    unsigned* cnt = (unsigned*)(ws + L.cnt[q]);
    unsigned* cursor = (unsigned*)(ws + L.cursor);
    unsigned* cell_of = (unsigned*)(ws + L.cell_of[q]);
    const Obj* obj = (const Obj*)(ws + L.obj[q]);
    AST_CHECK_HIP(hipMemsetAsync(cnt, 0, L.cap * 4, s));
    grid_box_count_kernel<<<ast::stream_grid(n, 256), 256, 0, s>>>(obj, n, prm, cell_of, cnt);
    AST_CHECK_LAUNCH();
    grid_scan_kernel<BLOCK><<<1, 1024, 0, s>>>(cnt, prm, (unsigned*)(ws + L.cell_start[q]),
                                               (unsigned*)(ws + L.tile_start[q]), cursor);
    AST_CHECK_LAUNCH();
    grid_scatter_kernel<<<ast::stream_grid(n, 256), 256, 0, s>>>(obj, n, cell_of, cursor, (Obj*)(ws + L.sorted[q]));
    AST_CHECK_LAUNCH();
    return AST_OK;
}

// ---- host: what the entry points of every pair finder do around their own prep and pair kernels
// The counting sort and the walk index objects with 32 bits.
inline bool grid_count_ok(size_t n) { return n < (size_t(1) << 31); }

// No pair to visit: the outputs are zeroed and nothing is planned or sorted.
inline bool grid_no_pairs(int auto_pairs, size_t n1, size_t n2) { return auto_pairs ? n1 < 2 : (n1 == 0 || n2 == 0); }

// The prepare call of NSETS sets of n[q] objects, under the AST_PROF scope `prof`: per set the empty box and, when it
// has objects, prep(q, obj, box), which launches the finder's prep kernel of set q into its records and its box.  Then
// grid_bounds_kernel into bounds_d, for a caller that checks the coordinates; one that does not passes a literal
// nullptr, and its file gets no bounds kernel.
template <int NSETS, typename Obj, typename Bounds, typename Prep>
int grid_prepare(char* ws, const GridLayout& L, const size_t* n, Bounds bounds_d, const char* prof, hipStream_t s,
                 Prep&& prep) {
    GridBounds* box[2] = {(GridBounds*)(ws + L.bounds[0]), (GridBounds*)(ws + L.bounds[NSETS - 1])};
    {
        AST_PROF(prof, s);
        for (int q = 0; q < NSETS; ++q) {
            if (int rc = grid_bounds_reset(box[q], s)) return rc;
            if (n[q] == 0) continue;
            prep(q, (Obj*)(ws + L.obj[q]), box[q]);
            AST_CHECK_LAUNCH();
        }
    }
    if constexpr (!std::is_same<Bounds, std::nullptr_t>::value) {
        grid_bounds_kernel<NSETS><<<1, 64, 0, s>>>(box[0], box[1], &((GridBoxParams*)(ws + L.grid))->box, bounds_d);
        AST_CHECK_LAUNCH();
    }
    return AST_OK;
}

// Sort sets q2 .. 0 of n[q] objects into the planned grid.  Set 1 (q = 0) last: its tile count stays in prm->ntiles.
template <int BLOCK, typename Obj>
int grid_sort_sets(char* ws, const GridLayout& L, int q2, const size_t* n, hipStream_t s) {
    for (int q = q2; q >= 0; --q)
        if (int rc = grid_sort_set<BLOCK, Obj>(ws, L, q, n[q], s)) return rc;
    return AST_OK;
}

// What a pair kernel reads of a sorted workspace: the grid, set 1 with its tiles, set 2 = set q2 (0: set 1 itself, for
// one set or the pairs within one), and the workgroup rows of Part.
template <typename Obj, typename Part = double>
struct GridSorted {
    GridBoxParams* prm;
    Part* part;
    const Obj *sorted1, *sorted2;
    const unsigned *cell_start1, *tile_start1, *cell_start2;
    GridSorted(char* ws, const GridLayout& L, int q2)
        : prm((GridBoxParams*)(ws + L.grid)), part((Part*)(ws + L.part)), sorted1((const Obj*)(ws + L.sorted[0])),
          sorted2((const Obj*)(ws + L.sorted[q2])), cell_start1((const unsigned*)(ws + L.cell_start[0])),
          tile_start1((const unsigned*)(ws + L.tile_start[0])), cell_start2((const unsigned*)(ws + L.cell_start[q2])) {}
};

// ---- walk
// The cell whose tiles hold `tile`: tile_start[cell] <= tile < tile_start[cell + 1].
__device__ inline unsigned grid_cell_of_tile(const unsigned* __restrict__ tile_start, unsigned ncells, unsigned tile) {
    unsigned lo = 0, hi = ncells;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) / 2;
        if (tile_start[mid] <= tile) lo = mid; else hi = mid;
    }
    return lo;
}

// The pair walk of a persistent kernel of BLOCK threads.  Work item = (tile of BLOCK set-1 objects of cell a, neighbour
// k), walked with a stride of the grid; each thread holds one object i of the tile, and the objects j of set 2 in cell
// a + offset[k] pass through LDS BLOCK at a time.
//   auto_pairs: cell_start2 is set 1's own; k over the 14 half-shell offsets, and at k = 0 (the cell itself) j > i
//               only: every unordered pair once.  Otherwise k over all 27 offsets: every (i, j) once.
//   periodic:   neighbours wrap (dims >= 3 on every axis, or one cell: offset 0 only).  Otherwise a neighbour outside
//               [0, dims) on any axis is skipped.
// Callers whose topology is fixed pass literals, which fold.  The kernel supplies
//   load_i(i)         load sorted record i of set 1 (called by the threads that hold one);
//   before_stage(ni, m)  workgroup-uniform, before a stage of m objects j against the tile's ni objects i (at most
//                     ni m pairs): where 32-bit counters are flushed;
//   stage_j(j, t)     put sorted record j of set 2 into LDS slot t (between two barriers of the walk);
//   pair(q)           the pair of the thread's i with the j in slot q.
template <int BLOCK, typename LoadI, typename BeforeStage, typename StageJ, typename Pair>
__device__ __forceinline__ void grid_pair_walk(const unsigned* __restrict__ cell_start1,
                                               const unsigned* __restrict__ tile_start,
                                               const unsigned* __restrict__ cell_start2, const GridBoxParams* prm,
                                               bool periodic, bool auto_pairs, LoadI&& load_i,
                                               BeforeStage&& before_stage, StageJ&& stage_j, Pair&& pair) {
    const unsigned tid = threadIdx.x;
    const int dims[3] = {prm->dims[0], prm->dims[1], prm->dims[2]};
    const unsigned ncells = prm->ncells;
    const unsigned nneigh = auto_pairs ? GRID_NEIGH : GRID_NEIGH_ALL;
    const unsigned long long nitems = (unsigned long long)prm->ntiles * nneigh;
    for (unsigned long long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const unsigned tile = (unsigned)(item / nneigh);
        const int k = (int)(item % nneigh);
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
            if (periodic && dims[c] >= 3) v = v < 0 ? v + dims[c] : (v >= dims[c] ? v - dims[c] : v);
            else if (v < 0 || v >= dims[c]) skip = true;    // open boundary, or the one cell of a periodic box
            bc[c] = v;
        }
        if (skip) continue;
        const unsigned b = ((unsigned)bc[2] * (unsigned)dims[1] + (unsigned)bc[1]) * (unsigned)dims[0] + (unsigned)bc[0];
        const bool self = auto_pairs && k == 0;
        const unsigned i0 = cell_start1[a] + (tile - tile_start[a]) * BLOCK;
        const unsigned i1 = min(i0 + BLOCK, cell_start1[a + 1]);
        const unsigned j0 = self ? i0 + 1 : cell_start2[b];
        const unsigned j1 = cell_start2[b + 1];
        if (j0 >= j1) continue;

        const unsigned i = i0 + tid;
        const bool valid = i < i1;
        if (valid) load_i(i);
        for (unsigned jc = j0; jc < j1; jc += BLOCK) {
            const int m = (int)min((unsigned)BLOCK, j1 - jc);
            before_stage(i1 - i0, m);
            __syncthreads();
            if (jc + tid < j1) stage_j(jc + tid, (int)tid);
            __syncthreads();
            if (!valid) continue;
            const int q0 = (self && i + 1 > jc) ? (int)min((unsigned)m, i + 1 - jc) : 0;
            // The q loop is placed from a 64-byte instruction line, so that its speed does not depend on the length
            // of the code before it: measured, the same loop instructions run up to 2 % (pairwise) and 4 %
            // (pairwise_pdf) slower or faster with the loop shifted by a few dwords.
            asm volatile(".p2align 6");
            for (int q = q0; q < m; ++q) pair(q);
        }
    }
}

// ---- rows: kernels that add (fp64, fp64, u64) per bin into per-wave LDS rows h1, h2, hc of nb bins each
// part = [3][ROWS][nb], ROWS the workgroups of the kernel: the two sums, then the counts.  The workgroup's row, waves
// summed in wave order, with plain stores: every workgroup stores its whole row, so part needs no clearing.  After a
// barrier, by all threads.
template <int WAVES, int ROWS>
__device__ inline void grid_store_rows(const double* h1, const double* h2, const unsigned long long* hc, int nb,
                                       double* __restrict__ part) {
    double* p1 = part;
    double* p2 = part + (size_t)ROWS * nb;
    unsigned long long* pc = (unsigned long long*)(part + 2 * (size_t)ROWS * nb);
    for (int bin = threadIdx.x; bin < nb; bin += blockDim.x) {
        double s1 = h1[bin], s2 = h2[bin];
        unsigned long long sc = hc[bin];
        for (int v = 1; v < WAVES; ++v) { s1 += h1[v * nb + bin]; s2 += h2[v * nb + bin]; sc += hc[v * nb + bin]; }
        const size_t o = (size_t)blockIdx.x * nb + bin;
        p1[o] = s1;
        p2[o] = s2;
        pc[o] = sc;
    }
}

// out[bin] = sum of the ROWS workgroup rows, in row order.
template <int ROWS>
__global__ void __launch_bounds__(256)
grid_reduce3_kernel(const double* __restrict__ part, int nb, double* __restrict__ s1, double* __restrict__ s2,
                    unsigned long long* __restrict__ counts) {
    const int bin = blockIdx.x * blockDim.x + threadIdx.x;
    if (bin >= nb) return;
    const double* p1 = part;
    const double* p2 = part + (size_t)ROWS * nb;
    const unsigned long long* pc = (const unsigned long long*)(part + 2 * (size_t)ROWS * nb);
    double a1 = 0.0, a2 = 0.0;
    unsigned long long sc = 0;
    for (int g = 0; g < ROWS; ++g) {
        const size_t o = (size_t)g * nb + bin;
        a1 += p1[o];
        a2 += p2[o];
        sc += pc[o];
    }
    s1[bin] = a1;
    s2[bin] = a2;
    counts[bin] = sc;
}

}  // namespace
