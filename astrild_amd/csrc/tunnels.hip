// Tunnels void finder on a 2D map (rays/voids/tunnel.py: TunnelsFinder.find_voids; Cautun et al., arXiv:1710.01730):
// the empty circles through at least three tracers, i.e. the distinct circumcircles of the tracers' Delaunay triangles,
// as canonical integer records (i, e, k, n_on, X, Y, W).  The tracers (integer pixel coordinates) are sorted into a
// uniform 2D cell grid with a counting sort (cell_grid.h); a persistent grid of waves then takes one tracer each and
// walks its star by gift wrapping (tunnels_walk.h).  No floating point is used anywhere, and no float atomics: the
// set of records is the same on every call; their order is not, and the host sorts them.
#include "ast_common.h"
#include "cell_grid.h"

#define TN_DEV __device__
#define TN_WAVE 64
#define TN_SHFL_XOR(v, o) __shfl_xor((v), (o), 64)
#define TN_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#include "tunnels_walk.h"

namespace {

constexpr int TN_BLOCK = 256;
constexpr int TN_GRID = 2048;               // persistent walk workgroups (256 CUs x 8); each wave draws tracers
constexpr int TN_MAX_NPIX = 16384;          // coordinate differences below 2^14: the in-circle determinant fits int64
constexpr int TN_PER_CELL = 4;              // tracers per cell the grid aims at
constexpr int TN_MAX_GDIM = 2048;

struct TnParams {
    unsigned ncells, ntiles;                // as grid_scan_kernel expects them
    unsigned next;                          // the next sorted position a wave draws
};

// Cells per axis and their size in pixels: about n / TN_PER_CELL cells over the map.
struct TnDims {
    int cs, gdim;
    TnDims(size_t n, int npix, int single) {
        int d = 1;
        if (!single)
            while (d < TN_MAX_GDIM && d < npix && (size_t)(d + 1) * (size_t)(d + 1) * TN_PER_CELL <= n) ++d;
        cs = (npix + d - 1) / d;
        gdim = (npix + cs - 1) / cs;
    }
    size_t ncells() const { return (size_t)gdim * (size_t)gdim; }
};

struct TnLayout {
    size_t params, cnt, cell_start, tile_start, cursor, cell_of, obj, sorted, total;
    TnLayout(size_t n, int npix) {
        const size_t cap = TnDims(n, npix, 0).ncells();     // a single cell needs no more
        size_t o = 0;
        params = o;     o += align256(sizeof(TnParams));
        cnt = o;        o += align256(cap * 4);
        cell_start = o; o += align256((cap + 1) * 4);
        tile_start = o; o += align256((cap + 1) * 4);      // grid_scan_kernel writes it; the walk has no tiles
        cursor = o;     o += align256(cap * 4);
        cell_of = o;    o += align256(n * 4);
        obj = o;        o += align256(n * sizeof(tn::Obj));
        sorted = o;     o += align256(n * sizeof(tn::Obj));
        total = o;
    }
};

__global__ void tn_init_kernel(TnParams* prm, unsigned ncells, unsigned long long* count) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    prm->ncells = ncells;
    prm->ntiles = 0;
    prm->next = 0;
    count[0] = 0;
    count[1] = 0;
}

// One thread per tracer: its cell (coordinates outside the map are clamped into the border cells; the host refuses
// them before the call), the count of that cell, and the tracer with its index.
__global__ void __launch_bounds__(256)
tn_count_kernel(const int* __restrict__ x, const int* __restrict__ y, size_t n, int cs, int gdim,
                tn::Obj* __restrict__ obj, unsigned* __restrict__ cell_of, unsigned* __restrict__ cnt) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int xi = x[i], yi = y[i];
        const int cx = min(max(xi / cs, 0), gdim - 1), cy = min(max(yi / cs, 0), gdim - 1);
        const unsigned c = (unsigned)cy * (unsigned)gdim + (unsigned)cx;
        obj[i] = tn::Obj{xi, yi, (unsigned)i, 0u};
        cell_of[i] = c;
        atomicAdd(&cnt[c], 1u);
    }
}

// Each wave draws sorted positions from prm->next until none is left and walks that tracer's star.
__global__ void __launch_bounds__(TN_BLOCK)
tn_walk_kernel(tn::Grid g, TnParams* prm, tn::Out out) {
    const int lane = threadIdx.x & 63;
    for (;;) {
        unsigned s = 0;
        if (lane == 0) s = atomicAdd(&prm->next, 1u);
        s = __shfl(s, 0, 64);
        if (s >= g.n) return;
        tn::walk_star(g, s, lane, out);
    }
}

}  // namespace

extern "C" int ast_tunnels_max_npix(void) { return TN_MAX_NPIX; }

extern "C" size_t ast_tunnels_workspace_bytes(size_t n, int npix) {
    if (npix < 1 || npix > TN_MAX_NPIX || n >= (size_t(1) << 31)) return 0;
    return TnLayout(n, npix).total;
}

extern "C" int ast_tunnels_find(const int* x_d, const int* y_d, size_t n, int npix, int single_cell, void* work_d,
                                size_t work_bytes, long long* records_d, unsigned long long* count_d, void* stream) {
    AST_CHECK_ARG(npix >= 1 && npix <= TN_MAX_NPIX);
    AST_CHECK_ARG(n < (size_t(1) << 31));
    AST_CHECK_ARG(count_d);
    AST_CHECK_ARG(work_d && work_bytes >= ast_tunnels_workspace_bytes(n, npix));
    hipStream_t s = ast::as_stream(stream);
    const TnLayout L(n, npix);
    const TnDims dims(n, npix, single_cell);
    char* ws = (char*)work_d;
    TnParams* prm = (TnParams*)(ws + L.params);
    tn_init_kernel<<<1, 64, 0, s>>>(prm, (unsigned)dims.ncells(), count_d);
    AST_CHECK_LAUNCH();
    if (n < 3) return AST_OK;
    AST_CHECK_ARG(x_d && y_d && records_d);
    unsigned* cnt = (unsigned*)(ws + L.cnt);
    unsigned* cell_start = (unsigned*)(ws + L.cell_start);
    unsigned* tile_start = (unsigned*)(ws + L.tile_start);
    unsigned* cursor = (unsigned*)(ws + L.cursor);
    unsigned* cell_of = (unsigned*)(ws + L.cell_of);
    tn::Obj* obj = (tn::Obj*)(ws + L.obj);
    tn::Obj* sorted = (tn::Obj*)(ws + L.sorted);
    {
        AST_PROF("tunnels_grid", s);
        AST_CHECK_HIP(hipMemsetAsync(cnt, 0, dims.ncells() * 4, s));
        tn_count_kernel<<<ast::stream_grid(n, 256), 256, 0, s>>>(x_d, y_d, n, dims.cs, dims.gdim, obj, cell_of, cnt);
        AST_CHECK_LAUNCH();
        grid_scan_kernel<TN_WAVE><<<1, 1024, 0, s>>>(cnt, prm, cell_start, tile_start, cursor);
        AST_CHECK_LAUNCH();
        grid_scatter_kernel<<<ast::stream_grid(n, 256), 256, 0, s>>>(obj, n, cell_of, cursor, sorted);
        AST_CHECK_LAUNCH();
    }
    {
        AST_PROF("tunnels_walk", s);
        const tn::Grid g = {npix, dims.cs, dims.gdim, (unsigned)n, sorted, cell_start};
        const tn::Out out = {records_d, count_d, 2 * (unsigned long long)n};
        const size_t waves = TN_BLOCK / TN_WAVE;
        const size_t need = (n + waves - 1) / waves;
        tn_walk_kernel<<<(unsigned)(need < (size_t)TN_GRID ? need : (size_t)TN_GRID), TN_BLOCK, 0, s>>>(g, prm, out);
        AST_CHECK_LAUNCH();
    }
    return AST_OK;
}
