// Spherical profiles of particles around centres (profiles/profile_3d.py: Profiles3D.get_one_profile /
// from_particle_data): per centre, the count and the weight and velocity moments of the particles in each radial bin,
// with edges in units of the centre's own radius.  Prep widens every particle to one fp64 record and returns the
// bounding box.  Search mode sorts the records into a uniform cell grid (count -> scan -> cell_grid.h's scatter; the scan
// runs over tiles of cells in many workgroups, since this grid has up to 2^24 cells; cell index x-fastest, so the cells
// [x0, x1] of one (cy, cz) row are one contiguous span of the sorted array) and walks, per
// centre, the cells its reach touches; membership mode bins a given segment of the unsorted records per centre.  Work
// items (centre, run of z layers) or (centre, chunk of members) are laid out centre by centre on the host and walked by
// a persistent grid; each item fills per-wave LDS histograms (u64 counts, fp64 sums: LDS atomics only) and stores its
// row with plain stores, straight into the output when the centre has one item, else into a partial row that a second
// kernel sums in item order.  All arithmetic is fp64 (the library is built with -ffp-contract=off); the bin of a
// particle is decided by x = sqrt(d2) / R against the edges with np.histogram's rule.
#include "ast_common.h"
#include "cell_grid.h"
#include <cmath>

namespace {

constexpr int P3_BLOCK = 256;
constexpr int P3_WAVES = P3_BLOCK / 64;
constexpr int P3_GRID = 2048;               // persistent workgroups (256 CUs x 8)
constexpr int P3_MAX_BINS = 256;
constexpr int P3_LAYERS = 4;                // z layers of a centre's cell range per work item
constexpr int P3_CHUNK = 8192;              // members per work item
constexpr size_t P3_MAX_CELLS = size_t(1) << 24;

constexpr int P3_SCAN_TILE = 2048;          // cells per workgroup of the scan: 256 threads x 8

struct P3Rec { double r[3], w, v[3], pad; };            // 64 bytes

struct P3Grid { double lo[3], inv_cs[3]; int dims; };

// params | obj (np records) | cnt, cell_start (+ 1), cursor (ncells each) | tile_sum (ncells / P3_SCAN_TILE) | cell_of (np) |
// sorted (np records) | part_c (n_part x nbins) | part_m (n_part x nbins x nmom).  ncells == 0 (membership mode): no
// grid arrays and no sorted copy.  n_part counts only the items of centres with more than one item.
struct P3Layout {
    size_t params, obj, cnt, cell_start, tile_sum, cursor, cell_of, sorted, part_c, part_m, total;
    P3Layout(size_t np, size_t ncells, size_t n_part, int nbins, int nmom) {
        size_t o = 0;
        params = o;     o += align256(sizeof(GridBounds));
        obj = o;        o += align256(np * sizeof(P3Rec));
        cnt = o;        o += ncells ? align256(ncells * 4) : 0;
        cell_start = o; o += ncells ? align256((ncells + 1) * 4) : 0;
        tile_sum = o;   o += ncells ? align256((ncells + P3_SCAN_TILE - 1) / P3_SCAN_TILE * 4) : 0;
        cursor = o;     o += ncells ? align256(ncells * 4) : 0;
        cell_of = o;    o += ncells ? align256(np * 4) : 0;
        sorted = o;     o += ncells ? align256(np * sizeof(P3Rec)) : 0;
        part_c = o;     o += align256(n_part * (size_t)nbins * 8);
        part_m = o;     o += align256(n_part * (size_t)nbins * (size_t)nmom * 8);
        total = o;
    }
};

inline bool shape_ok(int nbins, int nmom) { return nbins >= 1 && nbins <= P3_MAX_BINS && (nmom == 1 || nmom == 4); }

__device__ inline double p3_load(const void* p, int dtype, size_t i) {
    return dtype == AST_F32 ? (double)((const float*)p)[i] : ((const double*)p)[i];
}

// One thread per particle: the fp64 record (r, w, v), a missing weight 1 and a missing velocity 0; the min / max of the
// positions (NaN counts as -inf / +inf) go to `box` (grid_bounds_commit).  obj == nullptr: only the bounds.
__global__ void __launch_bounds__(256)
p3_prep_kernel(const void* __restrict__ pos, int pos_dtype, const void* __restrict__ wgt, int w_dtype,
               const void* __restrict__ vel, int vel_dtype, size_t n, P3Rec* __restrict__ obj, GridBounds* box) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        P3Rec o;
        for (int a = 0; a < 3; ++a) {
            o.r[a] = p3_load(pos, pos_dtype, 3 * i + a);
            o.v[a] = vel ? p3_load(vel, vel_dtype, 3 * i + a) : 0.0;
        }
        o.w = wgt ? p3_load(wgt, w_dtype, i) : 1.0;
        o.pad = 0.0;
        if (obj) obj[i] = o;
        for (int a = 0; a < 3; ++a) {
            const double v = o.r[a];
            lo[a] = fmin(lo[a], v == v ? v : -INFINITY);
            hi[a] = fmax(hi[a], v == v ? v : INFINITY);
        }
    }
    grid_bounds_commit<256>(lo, hi, box);
}

// Exclusive scan of the cell counts in three launches.  First: tile_sum[t] = the sum of the counts of cells
// [t P3_SCAN_TILE, (t + 1) P3_SCAN_TILE).
__global__ void __launch_bounds__(256)
p3_scan_sums_kernel(const unsigned* __restrict__ cnt, unsigned ncells, unsigned* __restrict__ tile_sum) {
    __shared__ unsigned ws[4];
    const unsigned base = blockIdx.x * (unsigned)P3_SCAN_TILE;
    unsigned s = 0;
    for (int k = 0; k < P3_SCAN_TILE / 256; ++k) {
        const unsigned c = base + (unsigned)k * 256u + threadIdx.x;
        if (c < ncells) s += cnt[c];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x % 64 == 0) ws[threadIdx.x / 64] = s;
    __syncthreads();
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// Second, one workgroup of 1024: tile_sum becomes its own exclusive scan (ntiles <= 8192: at most 8 per thread), and
// cell_start[ncells] = the total.
__global__ void __launch_bounds__(1024)
p3_scan_tiles_kernel(unsigned* __restrict__ tile_sum, unsigned ntiles, unsigned* __restrict__ cell_start,
                     unsigned ncells) {
    __shared__ unsigned sh[1024];
    const unsigned chunk = (ntiles + 1023) / 1024;
    const unsigned t0 = threadIdx.x * chunk, t1 = min(ntiles, t0 + chunk);
    unsigned s = 0;
    for (unsigned t = t0; t < t1; ++t) s += tile_sum[t];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned acc = 0;
        for (int k = 0; k < 1024; ++k) { const unsigned v = sh[k]; sh[k] = acc; acc += v; }
        cell_start[ncells] = acc;
    }
    __syncthreads();
    s = sh[threadIdx.x];
    for (unsigned t = t0; t < t1; ++t) { const unsigned v = tile_sum[t]; tile_sum[t] = s; s += v; }
}

// Third: each thread scans 8 consecutive cells of its tile on top of the tile's offset -> cell_start and cursor.
__global__ void __launch_bounds__(256)
p3_scan_write_kernel(const unsigned* __restrict__ cnt, unsigned ncells, const unsigned* __restrict__ tile_off,
                     unsigned* __restrict__ cell_start, unsigned* __restrict__ cursor) {
    constexpr int PER = P3_SCAN_TILE / 256;
    __shared__ unsigned ws[4];
    const int w = threadIdx.x / 64, lane = threadIdx.x % 64;
    const unsigned c0 = blockIdx.x * (unsigned)P3_SCAN_TILE + threadIdx.x * (unsigned)PER;
    unsigned v[PER], local = 0;
    for (int k = 0; k < PER; ++k) { v[k] = c0 + k < ncells ? cnt[c0 + k] : 0u; local += v[k]; }
    unsigned inc = local;                                   // inclusive scan of `local` across the wave
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned n = __shfl_up(inc, o, 64);
        if (lane >= o) inc += n;
    }
    if (lane == 63) ws[w] = inc;
    __syncthreads();
    unsigned start = tile_off[blockIdx.x] + inc - local;
    for (int q = 0; q < w; ++q) start += ws[q];
    for (int k = 0; k < PER; ++k) {
        if (c0 + k < ncells) { cell_start[c0 + k] = start; cursor[c0 + k] = start; }
        start += v[k];
    }
}

// Cell of a coordinate: floor((x - lo) * inv_cs) clamped to [0, dims - 1] (a NaN goes to cell 0).
__device__ inline int p3_axis_cell(double x, double lo, double inv_cs, int dims) {
    double v = (x - lo) * inv_cs;
    const double top = (double)(dims - 1);
    if (!(v >= 0.0)) v = 0.0;
    if (v > top) v = top;
    return (int)v;
}

__global__ void __launch_bounds__(256)
p3_count_kernel(const P3Rec* __restrict__ obj, size_t n, P3Grid g, unsigned* __restrict__ cell_of,
                unsigned* __restrict__ cnt) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double* r = obj[i].r;
        const unsigned cx = p3_axis_cell(r[0], g.lo[0], g.inv_cs[0], g.dims), cy = p3_axis_cell(r[1], g.lo[1], g.inv_cs[1], g.dims),
                       cz = p3_axis_cell(r[2], g.lo[2], g.inv_cs[2], g.dims);
        const unsigned c = (cz * (unsigned)g.dims + cy) * (unsigned)g.dims + cx;
        cell_of[i] = c;
        atomicAdd(&cnt[c], 1u);
    }
}

// The cells [first, first + n) (periodic: modulo dims) that a centre's reach touches on one axis, as the host computes
// them for z: floor((c -+ reach - lo) * inv_cs).  Periodic: n >= dims means every cell once (first = 0, n = dims).
// Open: clamped to [0, dims - 1], n = 0 when the reach misses the grid.
__device__ inline void p3_axis_range(double c, double reach, double lo, double inv_cs, int dims, bool periodic,
                                     int* first, int* n) {
    double a = floor((c - reach - lo) * inv_cs), b = floor((c + reach - lo) * inv_cs);
    const double big = 1073741824.0;
    a = fmin(fmax(a, -big), big);
    b = fmin(fmax(b, -big), big);
    if (!(a == a)) a = -big;                 // NaN: all cells
    if (!(b == b)) b = big;
    long long ia = (long long)a, ib = (long long)b;
    if (periodic) {
        if (ib - ia + 1 >= dims) { *first = 0; *n = dims; return; }
        long long f = ia % dims;
        if (f < 0) f += dims;
        *first = (int)f;
        *n = (int)(ib - ia + 1);
    } else {
        if (ia < 0) ia = 0;
        if (ib > dims - 1) ib = dims - 1;
        *first = ib >= ia ? (int)ia : 0;
        *n = ib >= ia ? (int)(ib - ia + 1) : 0;
    }
}

// The centre whose items hold `item`: item_start[o] <= item < item_start[o + 1].
__device__ inline size_t p3_centre_of(const long long* __restrict__ item_start, size_t nc, long long item) {
    size_t lo = 0, hi = nc;
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) / 2;
        if (item_start[mid] <= item) lo = mid; else hi = mid;
    }
    return lo;
}

struct P3Centre { double c[3], cv[3], R, lim2; };

// One particle against one centre: s = p - c, wrapped once per axis when periodic (s > L/2 -> s - L, else s < -L/2 ->
// s + L), d2 = (sx^2 + sy^2) + sz^2, x = sqrt(d2) / R; bin k when e_k <= x < e_{k+1}, the last bin also x == e_last
// (np.histogram).  M == 4: u = v - centre velocity, v_r = ((ux sx + uy sy) + uz sz) / sqrt(d2), 0 at d2 == 0.
template <int M>
__device__ inline void p3_bin(const P3Rec* __restrict__ p, const P3Centre& ct, double box, const double* edges, int nbins,
                              unsigned long long* hc, double* hm) {
    double s[3];
    const double half = 0.5 * box;
    for (int a = 0; a < 3; ++a) {
        s[a] = p->r[a] - ct.c[a];
        if (box > 0.0) {
            if (s[a] > half) s[a] -= box;
            else if (s[a] < -half) s[a] += box;
        }
    }
    const double d2 = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2];
    if (!(d2 <= ct.lim2)) return;
    const double d = sqrt(d2);
    const double x = d / ct.R;
    if (!(x >= edges[0]) || !(x <= edges[nbins])) return;
    int lo = 0, hi = nbins;                             // edges[lo] <= x, and x < edges[hi] or hi == nbins
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (x >= edges[mid]) lo = mid; else hi = mid;
    }
    const double w = p->w;
    atomicAdd(&hc[lo], 1ull);
    atomicAdd(&hm[lo * M], w);
    if (M == 4) {
        const double ux = p->v[0] - ct.cv[0], uy = p->v[1] - ct.cv[1], uz = p->v[2] - ct.cv[2];
        const double vr = d2 > 0.0 ? ((ux * s[0] + uy * s[1]) + uz * s[2]) / d : 0.0;
        atomicAdd(&hm[lo * M + 1], w * vr);
        atomicAdd(&hm[lo * M + 2], w * (vr * vr));
        atomicAdd(&hm[lo * M + 3], w * ((ux * ux + uy * uy) + uz * uz));
    }
}

// SEARCH: work item = (centre o, z layers [k layers, (k + 1) layers) of its nz = zrange[2 o + 1] layers from cell
// zrange[2 o]; layers == 0: all of them), k = item - item_start[o].  Wave w takes the rows (layer, cy) w, w + 4, ... of
// the item; a row's cells [x0, x0 + nx) are one span of `rec` (the cell-sorted records), or two when they wrap, and the
// wave's lanes stride through it.
// !SEARCH: work item = (centre o, members [k chunk, (k + 1) chunk) of its segment segs[2 o] .. + segs[2 o + 1] of `rec`
// (the unsorted records)), all threads striding through it.
// Either way each wave adds into its own LDS histogram; the four are then summed in wave order and stored: into
// counts / moments row o when the centre has one item, else into partial row part_start[o] + k.
template <int M, bool SEARCH>
__global__ void __launch_bounds__(P3_BLOCK)
p3_item_kernel(const P3Rec* __restrict__ rec, size_t np, const unsigned* __restrict__ cell_start, P3Grid g,
               double boxsize, double pad, size_t nc, const double* __restrict__ centres,
               const double* __restrict__ radii, const double* __restrict__ cvel, const int* __restrict__ zrange,
               const long long* __restrict__ segs, int per_item, const long long* __restrict__ item_start,
               long long n_items, const long long* __restrict__ part_start, long long n_part,
               const double* __restrict__ edges_g, int nbins, long long* __restrict__ counts,
               double* __restrict__ moments, long long* __restrict__ part_c, double* __restrict__ part_m) {
    extern __shared__ double lds[];
    double* edges = lds;                                                        // [nbins + 1]
    double* hm = edges + (nbins + 1);                                           // [P3_WAVES][nbins][M]
    unsigned long long* hc = (unsigned long long*)(hm + P3_WAVES * nbins * M);  // [P3_WAVES][nbins]
    const int tid = threadIdx.x, w = tid / 64, lane = tid % 64;
    for (int k = tid; k <= nbins; k += P3_BLOCK) edges[k] = edges_g[k];
    double* whm = hm + w * nbins * M;
    unsigned long long* whc = hc + w * nbins;
    const bool periodic = boxsize > 0.0;
    for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
        const size_t o = p3_centre_of(item_start, nc, item);
        const long long k = item - item_start[o];
        const long long n_it = item_start[o + 1] - item_start[o];
        __syncthreads();                                // the previous item is done with LDS (and edges are in)
        for (int b = tid; b < P3_WAVES * nbins * M; b += P3_BLOCK) hm[b] = 0.0;
        for (int b = tid; b < P3_WAVES * nbins; b += P3_BLOCK) hc[b] = 0ull;
        __syncthreads();
        P3Centre ct;
        for (int a = 0; a < 3; ++a) {
            ct.c[a] = centres[3 * o + a];
            ct.cv[a] = (M == 4 && cvel) ? cvel[3 * o + a] : 0.0;
        }
        ct.R = radii[o];
        const double top = edges[nbins] * ct.R;
        ct.lim2 = (top * top) * (1.0 + 1e-12);
        if (SEARCH) {
            const double reach = top * (1.0 + 1e-9) + pad;
            int x0, nx, y0, ny;
            p3_axis_range(ct.c[0], reach, g.lo[0], g.inv_cs[0], g.dims, periodic, &x0, &nx);
            p3_axis_range(ct.c[1], reach, g.lo[1], g.inv_cs[1], g.dims, periodic, &y0, &ny);
            const int z0 = zrange[2 * o], nz = zrange[2 * o + 1];
            const int l0 = per_item > 0 ? (int)k * per_item : 0;
            const int l1 = per_item > 0 ? min(nz, l0 + per_item) : nz;
            const int nrows = nx > 0 && ny > 0 && l1 > l0 ? (l1 - l0) * ny : 0;
            const unsigned d = (unsigned)g.dims;
            for (int row = w; row < nrows; row += P3_WAVES) {
                const unsigned cz = ((unsigned)z0 + (unsigned)(l0 + row / ny)) % d;
                const unsigned cy = ((unsigned)y0 + (unsigned)(row % ny)) % d;
                const unsigned base = (cz * d + cy) * d;
                const unsigned xe = (unsigned)x0 + (unsigned)nx;            // one past the last cell, before the wrap
                const unsigned a1 = min(xe, d);
                unsigned i0 = cell_start[base + (unsigned)x0], i1 = cell_start[base + a1];
                for (unsigned i = i0 + lane; i < i1; i += 64) p3_bin<M>(rec + i, ct, boxsize, edges, nbins, whc, whm);
                if (xe > d) {                                               // wrapped part: cells [0, xe - d)
                    i0 = cell_start[base];
                    i1 = cell_start[base + (xe - d)];
                    for (unsigned i = i0 + lane; i < i1; i += 64) p3_bin<M>(rec + i, ct, boxsize, edges, nbins, whc, whm);
                }
            }
        } else {
            long long off = segs[2 * o], cnt = segs[2 * o + 1];
            if (off < 0) off = 0;
            long long end = off + (cnt > 0 ? cnt : 0);
            if (end > (long long)np) end = (long long)np;
            const long long m0 = off + k * (long long)per_item;
            const long long m1 = min(end, m0 + (long long)per_item);
            for (long long i = m0 + tid; i < m1; i += P3_BLOCK) p3_bin<M>(rec + i, ct, boxsize, edges, nbins, whc, whm);
        }
        __syncthreads();
        long long* oc = counts + o * (size_t)nbins;
        double* om = moments + o * (size_t)nbins * M;
        if (n_it > 1) {
            const long long slot = part_start[o] + k;
            if (slot < 0 || slot >= n_part) continue;   // an inconsistent work list: nothing is written out of bounds
            oc = part_c + (size_t)slot * nbins;
            om = part_m + (size_t)slot * nbins * M;
        }
        for (int b = tid; b < nbins; b += P3_BLOCK) {
            unsigned long long c = 0;
            for (int q = 0; q < P3_WAVES; ++q) c += hc[q * nbins + b];
            oc[b] = (long long)c;
        }
        for (int b = tid; b < nbins * M; b += P3_BLOCK) {
            double s = 0.0;
            for (int q = 0; q < P3_WAVES; ++q) s += hm[q * nbins * M + b];
            om[b] = s;
        }
    }
}

// Centres with more than one item: counts / moments row o = its partial rows added in item order.
__global__ void __launch_bounds__(256)
p3_reduce_kernel(const long long* __restrict__ part_c, const double* __restrict__ part_m,
                 const long long* __restrict__ item_start, const long long* __restrict__ part_start, size_t nc,
                 long long n_part, int nbins, int nmom, long long* __restrict__ counts, double* __restrict__ moments) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nc * (size_t)nbins) return;
    const size_t o = idx / nbins;
    const int b = (int)(idx % nbins);
    const long long n_it = item_start[o + 1] - item_start[o];
    if (n_it <= 1) return;
    const long long p0 = part_start[o];
    if (p0 < 0 || p0 + n_it > n_part) return;
    long long c = 0;
    for (long long i = p0; i < p0 + n_it; ++i) c += part_c[(size_t)i * nbins + b];
    counts[idx] = c;
    for (int m = 0; m < nmom; ++m) {
        double s = 0.0;
        for (long long i = p0; i < p0 + n_it; ++i) s += part_m[((size_t)i * nbins + b) * nmom + m];
        moments[idx * nmom + m] = s;
    }
}

inline size_t p3_lds_bytes(int nbins, int nmom) {
    return (size_t)(nbins + 1) * 8 + (size_t)P3_WAVES * nbins * nmom * 8 + (size_t)P3_WAVES * nbins * 8;
}

struct P3Call {
    const P3Rec* rec; size_t np; const unsigned* cell_start; P3Grid g; double boxsize, pad; size_t nc;
    const double *centres, *radii, *cvel; const int* zrange; const long long* segs; int per_item;
    const long long* item_start; long long n_items; const long long* part_start; long long n_part;
    const double* edges; int nbins, nmom; long long* counts; double* moments; long long* part_c; double* part_m;
};

template <int M, bool SEARCH>
void p3_launch(const P3Call& c, hipStream_t s) {
    const unsigned grid = (unsigned)(c.n_items < P3_GRID ? c.n_items : P3_GRID);
    p3_item_kernel<M, SEARCH><<<grid, P3_BLOCK, p3_lds_bytes(c.nbins, M), s>>>(
        c.rec, c.np, c.cell_start, c.g, c.boxsize, c.pad, c.nc, c.centres, c.radii, c.cvel, c.zrange, c.segs,
        c.per_item, c.item_start, c.n_items, c.part_start, c.n_part, c.edges, c.nbins, c.counts, c.moments, c.part_c,
        c.part_m);
}

int p3_run(const P3Call& c, bool search, hipStream_t s) {
    {
        AST_PROF(search ? "profile3d_search" : "profile3d_members", s);
        if (search && c.nmom == 4) p3_launch<4, true>(c, s);
        else if (search) p3_launch<1, true>(c, s);
        else if (c.nmom == 4) p3_launch<4, false>(c, s);
        else p3_launch<1, false>(c, s);
        AST_CHECK_LAUNCH();
    }
    if (c.n_part > 0) {
        AST_PROF("profile3d_reduce", s);
        const size_t n = c.nc * (size_t)c.nbins;
        p3_reduce_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(c.part_c, c.part_m, c.item_start, c.part_start,
                                                                     c.nc, c.n_part, c.nbins, c.nmom, c.counts,
                                                                     c.moments);
        AST_CHECK_LAUNCH();
    }
    return AST_OK;
}

}  // namespace

extern "C" int ast_profile3d_max_bins(void) { return P3_MAX_BINS; }

extern "C" int ast_profile3d_layers(void) { return P3_LAYERS; }

extern "C" int ast_profile3d_chunk(void) { return P3_CHUNK; }

extern "C" size_t ast_profile3d_max_cells(void) { return P3_MAX_CELLS; }

extern "C" size_t ast_profile3d_workspace_bytes(size_t np, size_t ncells, size_t n_part, int nbins, int nmom) {
    if (!shape_ok(nbins, nmom) || ncells > P3_MAX_CELLS || np >= (size_t(1) << 31)) return 0;
    return P3Layout(np, ncells, n_part, nbins, nmom).total;
}

extern "C" int ast_profile3d_prepare(const void* pos_d, int pos_dtype, const void* weights_d, int weights_dtype,
                                     const void* vel_d, int vel_dtype, size_t np, int bounds_only, void* work_d,
                                     size_t work_bytes, double* bounds_d, void* stream) {
    AST_CHECK_ARG(pos_dtype == AST_F32 || pos_dtype == AST_F64);
    AST_CHECK_ARG(weights_d == nullptr || weights_dtype == AST_F32 || weights_dtype == AST_F64);
    AST_CHECK_ARG(vel_d == nullptr || vel_dtype == AST_F32 || vel_dtype == AST_F64);
    AST_CHECK_ARG(np < (size_t(1) << 31));
    AST_CHECK_ARG(np == 0 || pos_d);
    AST_CHECK_ARG(bounds_d);
    const P3Layout L(np, 0, 0, 1, 1);
    AST_CHECK_ARG(work_d && work_bytes >= (bounds_only ? L.obj : L.cnt));
    hipStream_t s = ast::as_stream(stream);
    char* ws = (char*)work_d;
    GridBounds* box = (GridBounds*)(ws + L.params);
    if (int rc = grid_bounds_reset(box, s)) return rc;
    if (np > 0) {
        AST_PROF("profile3d_prep", s);
        p3_prep_kernel<<<ast::stream_grid(np, 256), 256, 0, s>>>(pos_d, pos_dtype, weights_d, weights_dtype, vel_d,
                                                                 vel_dtype, np, bounds_only ? nullptr : (P3Rec*)(ws + L.obj),
                                                                 box);
        AST_CHECK_LAUNCH();
    }
    grid_bounds_kernel<1><<<1, 64, 0, s>>>(box, nullptr, nullptr, bounds_d);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

extern "C" int ast_profile3d_search(void* work_d, size_t work_bytes, size_t np, int dims, double lo_x, double lo_y,
                                    double lo_z, double inv_x, double inv_y, double inv_z, double boxsize, double pad,
                                    size_t nc, const double* centres_d, const double* radii_d,
                                    const double* centre_vel_d, const int* zrange_d, int layers,
                                    const long long* item_start_d, size_t n_items, const long long* part_start_d,
                                    size_t n_part, const double* edges_d, int nbins, int nmom, long long* counts_d,
                                    double* moments_d, void* stream) {
    AST_CHECK_ARG(shape_ok(nbins, nmom));
    AST_CHECK_ARG(dims >= 1 && (size_t)dims * dims * dims <= P3_MAX_CELLS);
    AST_CHECK_ARG(boxsize >= 0.0 && std::isfinite(boxsize) && pad >= 0.0 && std::isfinite(pad));
    AST_CHECK_ARG(std::isfinite(lo_x) && std::isfinite(lo_y) && std::isfinite(lo_z));
    AST_CHECK_ARG(inv_x >= 0.0 && inv_y >= 0.0 && inv_z >= 0.0 && std::isfinite(inv_x) && std::isfinite(inv_y) && std::isfinite(inv_z));
    AST_CHECK_ARG(np >= 1 && np < (size_t(1) << 31) && nc >= 1 && layers >= 0);
    AST_CHECK_ARG(n_items >= nc && n_items < (size_t(1) << 40) && n_part < (size_t(1) << 40));
    AST_CHECK_ARG(centres_d && radii_d && zrange_d && item_start_d && part_start_d && edges_d && counts_d && moments_d);
    const size_t ncells = (size_t)dims * dims * dims;
    AST_CHECK_ARG(work_d && work_bytes >= ast_profile3d_workspace_bytes(np, ncells, n_part, nbins, nmom));
    hipStream_t s = ast::as_stream(stream);
    const P3Layout L(np, ncells, n_part, nbins, nmom);
    char* ws = (char*)work_d;
    unsigned* cnt = (unsigned*)(ws + L.cnt);
    unsigned* cell_start = (unsigned*)(ws + L.cell_start);
    unsigned* cursor = (unsigned*)(ws + L.cursor);
    unsigned* cell_of = (unsigned*)(ws + L.cell_of);
    const P3Rec* obj = (const P3Rec*)(ws + L.obj);
    P3Rec* sorted = (P3Rec*)(ws + L.sorted);
    P3Grid g;
    g.lo[0] = lo_x; g.lo[1] = lo_y; g.lo[2] = lo_z;
    g.inv_cs[0] = inv_x; g.inv_cs[1] = inv_y; g.inv_cs[2] = inv_z;
    g.dims = dims;
    {
        AST_PROF("profile3d_grid", s);
        AST_CHECK_HIP(hipMemsetAsync(cnt, 0, ncells * 4, s));
        p3_count_kernel<<<ast::stream_grid(np, 256), 256, 0, s>>>(obj, np, g, cell_of, cnt);
        AST_CHECK_LAUNCH();
        const unsigned ntiles = (unsigned)((ncells + P3_SCAN_TILE - 1) / P3_SCAN_TILE);
        unsigned* tile_sum = (unsigned*)(ws + L.tile_sum);
        p3_scan_sums_kernel<<<ntiles, 256, 0, s>>>(cnt, (unsigned)ncells, tile_sum);
        AST_CHECK_LAUNCH();
        p3_scan_tiles_kernel<<<1, 1024, 0, s>>>(tile_sum, ntiles, cell_start, (unsigned)ncells);
        AST_CHECK_LAUNCH();
        p3_scan_write_kernel<<<ntiles, 256, 0, s>>>(cnt, (unsigned)ncells, tile_sum, cell_start, cursor);
        AST_CHECK_LAUNCH();
        grid_scatter_kernel<<<ast::stream_grid(np, 256), 256, 0, s>>>(obj, np, cell_of, cursor, sorted);
        AST_CHECK_LAUNCH();
    }
    P3Call c{sorted, np, cell_start, g, boxsize, pad, nc, centres_d, radii_d, centre_vel_d, zrange_d, nullptr, layers,
             item_start_d, (long long)n_items, part_start_d, (long long)n_part, edges_d, nbins, nmom, counts_d,
             moments_d, (long long*)(ws + L.part_c), (double*)(ws + L.part_m)};
    return p3_run(c, true, s);
}

extern "C" int ast_profile3d_members(void* work_d, size_t work_bytes, size_t np, double boxsize, size_t nc,
                                     const double* centres_d, const double* radii_d, const double* centre_vel_d,
                                     const long long* segments_d, int chunk, const long long* item_start_d,
                                     size_t n_items, const long long* part_start_d, size_t n_part,
                                     const double* edges_d, int nbins, int nmom, long long* counts_d,
                                     double* moments_d, void* stream) {
    AST_CHECK_ARG(shape_ok(nbins, nmom));
    AST_CHECK_ARG(boxsize >= 0.0 && std::isfinite(boxsize));
    AST_CHECK_ARG(np >= 1 && np < (size_t(1) << 31) && nc >= 1 && chunk >= 1);
    AST_CHECK_ARG(n_items >= nc && n_items < (size_t(1) << 40) && n_part < (size_t(1) << 40));
    AST_CHECK_ARG(centres_d && radii_d && segments_d && item_start_d && part_start_d && edges_d && counts_d && moments_d);
    AST_CHECK_ARG(work_d && work_bytes >= ast_profile3d_workspace_bytes(np, 0, n_part, nbins, nmom));
    hipStream_t s = ast::as_stream(stream);
    const P3Layout L(np, 0, n_part, nbins, nmom);
    char* ws = (char*)work_d;
    P3Grid g = {};
    g.dims = 1;
    P3Call c{(const P3Rec*)(ws + L.obj), np, nullptr, g, boxsize, 0.0, nc, centres_d, radii_d, centre_vel_d, nullptr,
             segments_d, chunk, item_start_d, (long long)n_items, part_start_d, (long long)n_part, edges_d, nbins, nmom,
             counts_d, moments_d, (long long*)(ws + L.part_c), (double*)(ws + L.part_m)};
    return p3_run(c, false, s);
}
