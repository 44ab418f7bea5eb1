// Watershed void finder on sky maps (rays/voids/watershed.py): the basins of steepest descent of an
// npix x npix map, their sums, and the passes between them.  The reference has no runnable counterpart (its
// rays/voids/watershed.py only writes files for an external program), so the result is defined in DESIGN.md 6j and
// restated by tests/watershed_oracle.py.
//
// Pixels are totally ordered by (f[p], p), p = y * npix + x, values compared in the map's own type (-0.0 == +0.0: a tie,
// broken by the lower index).  link[p] = the smallest of p and its up-to-8 neighbours inside the map; a minimum has
// link[p] == p; following links from p ends at the minimum of p's basin.
#include "ast_common.h"

namespace {

template <typename T>
__device__ inline bool finite_value(T v) { return v - v == T(0); }      // false for NaN and +-inf

// (fa, pa) < (fb, pb) in the pixel order
template <typename T>
__device__ inline bool pixel_less(T fa, int pa, T fb, int pb) { return fa < fb || (fa == fb && pa < pb); }

template <typename T>
__global__ void __launch_bounds__(256)
ws_link_kernel(const T* __restrict__ img, int npix, int* __restrict__ link, unsigned long long* __restrict__ nonfinite) {
    // 16 x 16 pixel tile per workgroup, the 18 x 18 footprint staged in LDS.  A footprint position outside the map is
    // clamped to the nearest pixel inside, which is the pixel itself or one of its neighbours inside the map: the
    // candidates of a border pixel are then exactly its neighbours inside the map, some of them seen twice.
    __shared__ T tile[18][19];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
    for (int i = threadIdx.x; i < 18 * 18; i += 256) {
        const int ly = i / 18, lx = i % 18;
        const int gy = min(max(y0 + ly - 1, 0), npix - 1), gx = min(max(x0 + lx - 1, 0), npix - 1);
        tile[ly][lx] = img[(size_t)gy * npix + gx];
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= npix || y >= npix) return;
    T best = tile[ty + 1][tx + 1];
    int at = y * npix + x;
    if (!finite_value(best)) atomicAdd(nonfinite, 1ull);      // rare: an error the host raises
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            if (dy == 1 && dx == 1) continue;
            const int gy = min(max(y + dy - 1, 0), npix - 1), gx = min(max(x + dx - 1, 0), npix - 1);
            const T v = tile[ty + dy][tx + dx];
            const int q = gy * npix + gx;
            if (pixel_less(v, q, best, at)) {
                best = v;
                at = q;
            }
        }
    link[y * npix + x] = at;
}

// One pass of pointer jumping, in place: link[p] <- link[link[link[p]]].  Another work item may be rewriting the
// entries read here; a 4-byte load sees the old or the new value whole, and both are ancestors of the entry's pixel
// on the way to its minimum (an entry only ever moves further along that way), so the race is benign: every read
// returns a pointer at least as far as the one a pass reading the state before the launch would, and the distance an
// entry covers at least doubles per pass.  A minimum is the only pixel with link[r] == r, before and after any pass,
// so "g2 == g1" says that g1 is a minimum whatever else is in flight.  *pending is raised when some g1 was not one:
// when it stays 0, every entry points at its minimum.  Pass k finds g1 at distance >= min(2^k, depth), so
// ceil(log2(longest path)) passes are enough.
__global__ void __launch_bounds__(256)
ws_jump_kernel(int* link, size_t n, int* __restrict__ pending) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    bool more = false;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const int g0 = link[p];
        const int g1 = link[g0];
        if (g1 == g0) continue;                  // g0 is a minimum
        const int g2 = link[g1];
        link[p] = g2;
        more = more || g2 != g1;
    }
    if (more) *pending = 1;
}

// out[i] = table[src[i]]; an index outside the table gives -1
__global__ void __launch_bounds__(256)
ws_relabel_kernel(const int* src, const int* __restrict__ table, size_t table_len, size_t n, int* out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int s = src[i];
        out[i] = (s >= 0 && (size_t)s < table_len) ? table[s] : -1;
    }
}

constexpr int WS_RUN = 16;      // consecutive pixels per work item in the sums

struct WsAcc {
    long long area, sx, sy, edge;
    double sf;
};

__device__ inline void ws_flush(int label, const WsAcc& a, size_t nbasins, unsigned long long* __restrict__ isums,
                                double* __restrict__ sum_f) {
    if (label < 0 || (size_t)label >= nbasins) return;
    atomicAdd(&isums[label], (unsigned long long)a.area);
    atomicAdd(&isums[nbasins + label], (unsigned long long)a.sx);
    atomicAdd(&isums[2 * nbasins + label], (unsigned long long)a.sy);
    if (a.edge) atomicAdd(&isums[3 * nbasins + label], (unsigned long long)a.edge);
    atomicAdd(&sum_f[label], a.sf);
}

// 16 consecutive elements of src from p0 on: as 16-byte loads when the run is whole and src is 16-byte aligned (p0 is a
// multiple of WS_RUN, so the run then is too), one by one otherwise.  Elements past `count` read as 0.
template <typename U>
__device__ inline void ws_load_run(const U* __restrict__ src, size_t p0, int count, bool wide, U (&dst)[WS_RUN]) {
    constexpr int per = 16 / (int)sizeof(U);
    struct alignas(16) Chunk { U v[per]; };
    if (wide && count == WS_RUN) {
        const Chunk* c = reinterpret_cast<const Chunk*>(src + p0);
#pragma unroll
        for (int i = 0; i < WS_RUN / per; ++i) {
            const Chunk t = c[i];
#pragma unroll
            for (int j = 0; j < per; ++j) dst[i * per + j] = t.v[j];
        }
    } else {
#pragma unroll
        for (int k = 0; k < WS_RUN; ++k) dst[k] = k < count ? src[p0 + k] : U(0);
    }
}

// Per-basin sums.  A work item walks WS_RUN consecutive pixels of the row-major map and keeps the sums of the current
// label in registers; it goes to the global accumulators only when the label changes - a basin is tens of pixels wide,
// so this is one to three flushes per 16 pixels instead of 16.
template <typename T>
__global__ void __launch_bounds__(256)
ws_sums_kernel(const T* __restrict__ img, const int* __restrict__ labels, int npix, size_t nbasins, bool wide,
               unsigned long long* __restrict__ isums, double* __restrict__ sum_f) {
    const size_t n = (size_t)npix * npix;
    const size_t runs = (n + WS_RUN - 1) / WS_RUN;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < runs; r += stride) {
        const size_t p0 = r * WS_RUN;
        int y = (int)(p0 / (size_t)npix), x = (int)(p0 - (size_t)y * npix);
        const int count = (int)min((size_t)WS_RUN, n - p0);
        int l[WS_RUN];
        T f[WS_RUN];
        ws_load_run(labels, p0, count, wide, l);
        ws_load_run(img, p0, count, wide, f);
        int cur = -1;
        WsAcc a = {0, 0, 0, 0, 0.0};
#pragma unroll
        for (int k = 0; k < WS_RUN; ++k) {
            if (k >= count) break;
            if (l[k] != cur) {
                ws_flush(cur, a, nbasins, isums, sum_f);
                cur = l[k];
                a = {0, 0, 0, 0, 0.0};
            }
            a.area += 1;
            a.sx += x;
            a.sy += y;
            a.edge += (x == 0 || y == 0 || x == npix - 1 || y == npix - 1) ? 1 : 0;
            a.sf += (double)f[k];
            if (++x == npix) {
                x = 0;
                ++y;
            }
        }
        ws_flush(cur, a, nbasins, isums, sum_f);
    }
}

// Boundary pairs.  Every pixel looks at its E, SW, S and SE neighbours, so that each 8-adjacent pair is seen once, and
// for every other label among them it has one record: key (a << 32 | b) with a < b, and the smallest
// max(f[p], f[q]) + 0 over the neighbours q of that label (the sum turns a -0.0 into +0.0 and changes no other value,
// so that a minimum over records does not depend on their order).  FILL = false writes the number of records of each
// block to blocks[]; the host turns the counts into the blocks' first record indices (an exclusive prefix sum), and
// FILL = true writes the records there: no global atomics, and every block's range is the same on every call.
template <typename T, bool FILL>
__global__ void __launch_bounds__(256)
ws_edges_kernel(const T* __restrict__ img, const int* __restrict__ labels, int npix, size_t cap,
                long long* __restrict__ keys, T* __restrict__ saddle, long long* __restrict__ blocks) {
    __shared__ int lab[18][19];
    __shared__ T val[FILL ? 18 : 1][19];
    __shared__ unsigned int block_count;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
    const size_t block = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (threadIdx.x == 0) block_count = 0;
    for (int i = threadIdx.x; i < 18 * 18; i += 256) {
        const int ly = i / 18, lx = i % 18;
        const int gy = y0 + ly - 1, gx = x0 + lx - 1;
        const bool in = gy >= 0 && gy < npix && gx >= 0 && gx < npix;
        lab[ly][lx] = in ? labels[(size_t)gy * npix + gx] : -1;
        if constexpr (FILL) val[ly][lx] = in ? img[(size_t)gy * npix + gx] : T(0);
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    const bool active = x < npix && y < npix;
    const int ddx[4] = {1, -1, 0, 1}, ddy[4] = {0, 1, 1, 1};
    const int mine = active ? lab[ty + 1][tx + 1] : -1;
    int other[4];
    T top[4];
    unsigned int found = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int l = lab[ty + 1 + ddy[k]][tx + 1 + ddx[k]];
        other[k] = (active && l >= 0 && l != mine) ? l : -1;
        if constexpr (FILL) {
            const T c = val[ty + 1][tx + 1], v = val[ty + 1 + ddy[k]][tx + 1 + ddx[k]];
            top[k] = (c < v ? v : c) + T(0);
        }
#pragma unroll
        for (int j = 0; j < k; ++j)
            if (other[k] >= 0 && other[j] == other[k]) {        // the first neighbour of a label keeps its record
                if constexpr (FILL) top[j] = top[k] < top[j] ? top[k] : top[j];
                other[k] = -1;
            }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) found += other[k] >= 0 ? 1u : 0u;
    unsigned int slot = 0;
    if (found) slot = atomicAdd(&block_count, found);
    if constexpr (!FILL) {
        __syncthreads();
        if (threadIdx.x == 0) blocks[block] = (long long)block_count;
    } else {
        if (!found) return;
        unsigned long long at = (unsigned long long)blocks[block] + slot;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (other[k] < 0) continue;
            if (at < cap) {
                const long long a = min(mine, other[k]), b = max(mine, other[k]);
                keys[at] = (a << 32) | b;
                saddle[at] = top[k];
            }
            ++at;
        }
    }
}

inline bool tile_grid_ok(int npix) { return npix >= 3 && (long long)npix * npix < (1ll << 31); }

}  // namespace

extern "C" int ast_watershed_max_passes(int npix) {
    if (!tile_grid_ok(npix)) return 0;
    const unsigned long long n = (unsigned long long)npix * npix;
    int bits = 0;
    while ((1ull << bits) < n) ++bits;           // ceil(log2(npix^2)): no path is longer than npix^2 - 1 links
    return bits;
}

extern "C" int ast_watershed_link(const void* img, int dtype, int npix, int* link, unsigned long long* nonfinite,
                                  void* stream) {
    AST_CHECK_ARG(img && link && nonfinite && tile_grid_ok(npix));
    AST_CHECK_ARG(dtype == AST_F32 || dtype == AST_F64);
    hipStream_t s = ast::as_stream(stream);
    AST_CHECK_HIP(hipMemsetAsync(nonfinite, 0, sizeof(unsigned long long), s));
    const dim3 grid((npix + 15) / 16, (npix + 15) / 16);
    AST_PROF("watershed_link", s);
    if (dtype == AST_F32)
        ws_link_kernel<float><<<grid, 256, 0, s>>>((const float*)img, npix, link, nonfinite);
    else
        ws_link_kernel<double><<<grid, 256, 0, s>>>((const double*)img, npix, link, nonfinite);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

extern "C" int ast_watershed_jump(int* link, int npix, int* pending, int* passes_host, void* stream) {
    AST_CHECK_ARG(link && pending && passes_host && tile_grid_ok(npix));
    hipStream_t s = ast::as_stream(stream);
    const size_t n = (size_t)npix * npix;
    const int bound = ast_watershed_max_passes(npix);
    AST_CHECK_HIP(hipMemsetAsync(pending, 0, sizeof(int) * (size_t)bound, s));
    const unsigned g = ast::stream_grid(n, 256);
    *passes_host = 0;
    for (int pass = 0; pass < bound; ++pass) {
        int more = 0;
        {
            AST_PROF("watershed_jump", s);
            ws_jump_kernel<<<g, 256, 0, s>>>(link, n, pending + pass);
            AST_CHECK_LAUNCH();
        }
        AST_CHECK_HIP(hipMemcpyAsync(&more, pending + pass, sizeof(int), hipMemcpyDeviceToHost, s));
        AST_CHECK_HIP(hipStreamSynchronize(s));
        *passes_host = pass + 1;
        if (!more) return AST_OK;
    }
    ast::set_error("%s: links not resolved after %d passes (npix %d): the link array is not a forest", __func__, bound,
                   npix);
    return AST_ERR_LIMIT;
}

extern "C" int ast_watershed_relabel(const int* src, const int* table, size_t table_len, size_t n, int* out,
                                     void* stream) {
    AST_CHECK_ARG(src && table && out && n > 0 && table_len > 0);
    hipStream_t s = ast::as_stream(stream);
    AST_PROF("watershed_relabel", s);
    ws_relabel_kernel<<<ast::stream_grid(n, 256), 256, 0, s>>>(src, table, table_len, n, out);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

extern "C" int ast_watershed_sums(const void* img, int dtype, const int* labels, int npix, size_t nbasins,
                                  long long* isums, double* sum_f, void* stream) {
    AST_CHECK_ARG(img && labels && isums && sum_f && nbasins > 0 && tile_grid_ok(npix));
    AST_CHECK_ARG(dtype == AST_F32 || dtype == AST_F64);
    hipStream_t s = ast::as_stream(stream);
    AST_CHECK_HIP(hipMemsetAsync(isums, 0, 4 * nbasins * sizeof(long long), s));
    AST_CHECK_HIP(hipMemsetAsync(sum_f, 0, nbasins * sizeof(double), s));
    const size_t runs = ((size_t)npix * npix + WS_RUN - 1) / WS_RUN;
    const unsigned g = ast::stream_grid(runs, 256);
    const bool wide = ((uintptr_t)img | (uintptr_t)labels) % 16 == 0;
    AST_PROF("watershed_sums", s);
    if (dtype == AST_F32)
        ws_sums_kernel<float><<<g, 256, 0, s>>>((const float*)img, labels, npix, nbasins, wide, (unsigned long long*)isums, sum_f);
    else
        ws_sums_kernel<double><<<g, 256, 0, s>>>((const double*)img, labels, npix, nbasins, wide, (unsigned long long*)isums, sum_f);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

extern "C" size_t ast_watershed_edge_blocks(int npix) {
    if (!tile_grid_ok(npix)) return 0;
    const size_t side = ((size_t)npix + 15) / 16;
    return side * side;
}

extern "C" int ast_watershed_edges(const void* img, int dtype, const int* labels, int npix, long long* blocks, size_t cap,
                                   long long* keys, void* saddle, void* stream) {
    AST_CHECK_ARG(img && labels && blocks && tile_grid_ok(npix));
    AST_CHECK_ARG(dtype == AST_F32 || dtype == AST_F64);
    AST_CHECK_ARG(cap == 0 || (keys && saddle));
    hipStream_t s = ast::as_stream(stream);
    const dim3 grid((npix + 15) / 16, (npix + 15) / 16);
    AST_PROF(cap ? "watershed_edges_fill" : "watershed_edges_count", s);
    if (dtype == AST_F32) {
        if (cap) ws_edges_kernel<float, true><<<grid, 256, 0, s>>>((const float*)img, labels, npix, cap, keys, (float*)saddle, blocks);
        else ws_edges_kernel<float, false><<<grid, 256, 0, s>>>((const float*)img, labels, npix, 0, nullptr, nullptr, blocks);
    } else {
        if (cap) ws_edges_kernel<double, true><<<grid, 256, 0, s>>>((const double*)img, labels, npix, cap, keys, (double*)saddle, blocks);
        else ws_edges_kernel<double, false><<<grid, 256, 0, s>>>((const double*)img, labels, npix, 0, nullptr, nullptr, blocks);
    }
    AST_CHECK_LAUNCH();
    return AST_OK;
}
