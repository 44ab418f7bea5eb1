// Friends-of-friends group finder (particles/hutils/fof.py; nbodykit's FOF, halotools' FoFGroups):
// particles whose separation is within a linking length are friends, and a group is a connected component of the
// friendship graph.  The pairs come from the uniform cell grid of cell_grid.h (the walk that visits every unordered
// pair within a reach once), the components from a union-find forest that the pair kernel builds with compare-and-swap
// and that pointer-jumping passes (watershed.hip's form) then flatten.  All pair arithmetic is fp64 (the library is
// built with -ffp-contract=off), so labels, sizes and the link count are integers that equal the numpy oracle of
// tests/fof_oracle.py exactly.
//
// Sphere linking: a = |x_i - x_j| per axis, periodic a = min(a, L - a); d^2 = (a_x^2 + a_y^2) + a_z^2; friends when
// d^2 <= b b (tpcf.hip's tp_pair_bin arithmetic).  Cylinder linking along `los`: rp^2 = a_a a_a + a_b a_b over the two
// other axes a < b, pi = a_los; friends when rp^2 <= b_perp b_perp and pi <= b_para (tp_rppi_bin's).
#include "ast_common.h"
#include "cell_grid.h"
#include <cmath>
#include <cstdlib>

namespace {

constexpr int FOF_BLOCK = 256;              // i objects per tile = j objects per LDS stage
constexpr int FOF_WAVES = FOF_BLOCK / 64;
constexpr int FOF_GRID = 1024;              // persistent link-kernel workgroups (256 CUs x 4)
constexpr size_t FOF_CELL_OBJECTS = 64;     // cells planned: n / this (measured), at least 27

struct FofObj { double r[3]; unsigned id; };    // id: the particle's index in the caller's array

enum FofGeom { FOF_SPHERE = 0, FOF_CYLINDER = 1 };

// One GridLayout of one set; its `part` holds parent[n] (int32).
inline GridLayout fof_layout(size_t n) {
    return GridLayout(1, n, 0, grid_cells_cap(n, 27), sizeof(FofObj), n * sizeof(int));
}

// One thread per particle: the record (position widened to fp64, own index), parent[i] = i, and the min / max of the
// coordinates (NaN counts as -inf / +inf) to `box`.
template <typename T>
__global__ void __launch_bounds__(256)
fof_prep_kernel(const T* __restrict__ pos, size_t n, FofObj* __restrict__ obj, int* __restrict__ parent,
                GridBounds* box) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        FofObj o;
        for (int a = 0; a < 3; ++a) o.r[a] = (double)pos[3 * i + a];
        o.id = (unsigned)i;
        obj[i] = o;
        parent[i] = (int)i;
        for (int a = 0; a < 3; ++a) {
            const double v = o.r[a];
            lo[a] = fmin(lo[a], v == v ? v : -INFINITY);
            hi[a] = fmax(hi[a], v == v ? v : INFINITY);
        }
    }
    grid_bounds_commit<256>(lo, hi, box);
}

__global__ void fof_plan_kernel(GridBoxParams* prm, int geom, double b_perp, double b_para, int los, double boxsize,
                                unsigned cap, int single) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (geom == FOF_CYLINDER) grid_cyl_plan(prm, b_perp, b_para, los, boxsize, cap, single);
    else grid_plan(prm, b_perp, boxsize, cap, single);
}

// A record's position as the link kernel holds it: as stored, or for the cylinder in the order (a, b, los).
template <int GEOM>
__device__ __forceinline__ void fof_axes(const double (&r)[3], int los, double (&out)[3]) {
    if (GEOM == FOF_CYLINDER) {
        out[0] = los == 0 ? r[1] : r[0];
        out[1] = los == 2 ? r[1] : r[2];
        out[2] = los == 0 ? r[0] : (los == 1 ? r[1] : r[2]);
    } else {
        for (int c = 0; c < 3; ++c) out[c] = r[c];
    }
}

template <int GEOM>
__device__ __forceinline__ bool fof_friends(const double (&ri)[3], double xj, double yj, double zj, bool periodic,
                                            double boxsize, double bb, double b_para) {
    double px = fabs(ri[0] - xj), py = fabs(ri[1] - yj), pz = fabs(ri[2] - zj);
    if (periodic) {
        px = fmin(px, boxsize - px);
        py = fmin(py, boxsize - py);
        pz = fmin(pz, boxsize - pz);
    }
    if (GEOM == FOF_CYLINDER) {
        const double rp2 = px * px + py * py;
        return rp2 <= bb && pz <= b_para;
    }
    const double d2 = (px * px + py * py) + pz * pz;
    return d2 <= bb;
}

// A relaxed load of agent scope: served past the CU's L1, which no other CU's compare-and-swap refreshes.
__device__ __forceinline__ int fof_load(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x as this thread sees it.  parent[y] <= y always, so the walk goes down in index and ends.
__device__ __forceinline__ int fof_find(const int* parent, int x) {
    for (;;) {
        const int p = fof_load(parent + x);
        if (p == x) return x;
        x = p;
    }
}

// Join the trees of a and b; returns a root above both (as seen at the return).
//
// The forest: parent[] is indexed by the caller's particle index, starts as parent[x] = x and keeps parent[x] <= x.
// The ONLY write of the link kernel is atomicCAS(&parent[a], a, b) with b < a: it changes the entry of a root, once,
// from itself to a smaller index; an entry that is not a root never changes again in this kernel (no path compression
// here).  So every value an entry ever held is an ancestor of x (or x itself) in the final forest.
// Visibility: the per-XCD L2s are not coherent and a CU's L1 is never refreshed by another CU; only the atomics are
// coherent.  The reads are relaxed agent-scope atomic loads, and nothing relies on their being fresh: a stale read
// returns x for an entry that has since been linked, i.e. it takes x for a root when it no longer is one - and then
// the compare-and-swap on parent[x], which is coherent, fails and returns the entry's true value, from which the walk
// goes on.  A compare-and-swap that succeeds was applied to a true root.
// Termination: every step replaces the index in hand by a strictly smaller one (fof_find by parent[x] < x; a failed
// compare-and-swap by the returned value, which differs from a and is <= a), indices are >= 0, so every loop ends
// whatever other workgroups do.  No spin-waits, no fences, no hand-offs between workgroups.
// Completeness: when the kernel has ended, every friend pair (i, j) had a call that ended with both under one root at
// some moment, and entries only ever gain ancestors: i and j are in one tree.
__device__ __forceinline__ int fof_unite(int* parent, int a, int b) {
    for (;;) {
        a = fof_find(parent, a);
        b = fof_find(parent, b);
        if (a == b) return a;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicCAS(parent + a, a, b);
        if (old == a) return b;
        a = old;                                // a was no root any more: old < a is its parent
    }
}

// The walk of cell_grid.h (grid_pair_walk, auto pairs: every unordered pair of the same or adjacent cells once) with
// the positions of the staged j objects in LDS.  Each friend pair adds 1 to the thread's link count and unites the two
// particles.  A find per friend pair is a chain of dependent loads from L2, and in a dense cell, where almost every
// pair is a friend pair of one group, that chain is all the kernel does (measured: DESIGN.md 6l).  So the thread keeps
// a root above its i in a register (`root`: an ancestor of i, found once per work item, possibly no longer the top),
// the staging thread finds a root above its j once per stage into LDS (jroot), and a pair whose two hints are equal is
// in one tree already and touches no global memory.  After a union the new root goes back into both hints; another
// wave may read or overwrite jroot[q] meanwhile - a 4-byte LDS word is read and written whole, and every value it
// ever holds is an ancestor of j, which is all the argument above needs.  The hints live in registers and LDS only:
// parent[] is still written by nothing but fof_unite's compare-and-swap.
template <int GEOM>
__global__ void __launch_bounds__(FOF_BLOCK)
fof_link_kernel(const FofObj* __restrict__ sorted, const unsigned* __restrict__ cell_start,
                const unsigned* __restrict__ tile_start, const GridBoxParams* prm, double boxsize, double b_perp,
                double b_para, int los, int* parent, unsigned long long* links) {
    __shared__ double jr[3 * FOF_BLOCK];
    __shared__ int jroot[FOF_BLOCK];
    __shared__ unsigned long long wsum[FOF_WAVES];
    const bool periodic = boxsize > 0.0;
    const double bb = b_perp * b_perp;
    double ri[3] = {0.0, 0.0, 0.0};
    int root = 0;
    unsigned long long count = 0;
    grid_pair_walk<FOF_BLOCK>(
        cell_start, tile_start, cell_start, prm, periodic, true,
        [&](unsigned i) {
            const FofObj o = sorted[i];
            fof_axes<GEOM>(o.r, los, ri);
            root = fof_find(parent, (int)o.id);
        },
        [&](unsigned, int) {},
        [&](unsigned j, int t) {
            const FofObj o = sorted[j];
            double rj[3];
            fof_axes<GEOM>(o.r, los, rj);
            for (int c = 0; c < 3; ++c) jr[c * FOF_BLOCK + t] = rj[c];
            jroot[t] = fof_find(parent, (int)o.id);
        },
        [&](int q) {
            if (!fof_friends<GEOM>(ri, jr[q], jr[FOF_BLOCK + q], jr[2 * FOF_BLOCK + q], periodic, boxsize, bb, b_para))
                return;
            ++count;
            const int rj = jroot[q];
            if (rj == root) return;
            root = fof_unite(parent, root, rj);
            jroot[q] = root;
        });
    // links: thread -> wave -> workgroup -> one atomic
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
    __syncthreads();
    if (threadIdx.x % 64 == 0) wsum[threadIdx.x / 64] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
        for (int w = 0; w < FOF_WAVES; ++w) sum += wsum[w];
        if (sum) atomicAdd(links, sum);
    }
}

// One pass of pointer jumping, in place: parent[p] <- parent[parent[parent[p]]] (watershed.hip's ws_jump_kernel, whose
// comment gives the argument: a racing read sees the old or the new value, both ancestors; a root is the only entry
// with parent[r] == r; the distance an entry covers at least doubles per pass).  *pending is raised when some
// grandparent was not a root.
__global__ void __launch_bounds__(256)
fof_jump_kernel(int* parent, size_t n, int* __restrict__ pending) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    bool more = false;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const int g0 = parent[p];
        const int g1 = parent[g0];
        if (g1 == g0) continue;                  // g0 is a root
        const int g2 = parent[g1];
        parent[p] = g2;
        more = more || g2 != g1;
    }
    if (more) *pending = 1;
}

// root[i] = parent[i] (resolved) and size[root[i]] += 1 (size zeroed before).
__global__ void __launch_bounds__(256)
fof_sizes_kernel(const int* __restrict__ parent, size_t n, int* __restrict__ root, unsigned* __restrict__ size) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int r = parent[i];
        root[i] = r;
        atomicAdd(&size[r], 1u);
    }
}

// labels[i] = table[root[i]]
__global__ void __launch_bounds__(256)
fof_relabel_kernel(const int* __restrict__ root, const int* __restrict__ table, size_t n, int* __restrict__ labels) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) labels[i] = table[root[i]];
}

// Seven sums of a wave, lane l ending with lane 0's total: a fixed xor butterfly, the same additions on every call.
__device__ __forceinline__ double fof_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per group (a stride of the grid's waves over the groups).  Lane l adds the members offset + l, l + 64, ...
// of the segment in that order - the fixed chunking - and the 64 lane sums are combined by fof_wave_sum's fixed
// butterfly: the same additions in the same order on every call, no atomics.
// s = pos_i - p_ref (p_ref = pos[first]), periodic: wrapped once per axis (s > L/2 -> s - L, else s < -L/2 -> s + L);
// cm = p_ref + sum(w s) / sum(w), periodic: wrapped once into [0, L); cmv = sum(w v) / sum(w); weight = sum(w).
template <typename TP, typename TV, typename TW>
__global__ void __launch_bounds__(256)
fof_features_kernel(const TP* __restrict__ pos, const TV* __restrict__ vel, const TW* __restrict__ weights, size_t n,
                    const int* __restrict__ members, const long long* __restrict__ offsets,
                    const long long* __restrict__ first, size_t ngroups, double boxsize, double* __restrict__ cm,
                    double* __restrict__ cmv, double* __restrict__ weight) {
    const int lane = threadIdx.x % 64;
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
    const size_t nwaves = (size_t)gridDim.x * blockDim.x / 64;
    const double half = 0.5 * boxsize;
    for (size_t g = wave; g < ngroups; g += nwaves) {
        const long long m0 = offsets[g], m1 = offsets[g + 1];
        const size_t f = (size_t)first[g];
        double ref[3];
        for (int a = 0; a < 3; ++a) ref[a] = (double)pos[3 * f + a];
        double ss[3] = {0.0, 0.0, 0.0}, sv[3] = {0.0, 0.0, 0.0}, sw = 0.0;
        for (long long m = m0 + lane; m < m1; m += 64) {
            const size_t i = (size_t)members[m];
            const double w = weights ? (double)weights[i] : 1.0;
            for (int a = 0; a < 3; ++a) {
                double s = (double)pos[3 * i + a] - ref[a];
                if (boxsize > 0.0) {
                    if (s > half) s = s - boxsize;
                    else if (s < -half) s = s + boxsize;
                }
                ss[a] += w * s;
                if (vel) sv[a] += w * (double)vel[3 * i + a];
            }
            sw += w;
        }
        for (int a = 0; a < 3; ++a) {
            ss[a] = fof_wave_sum(ss[a]);
            if (vel) sv[a] = fof_wave_sum(sv[a]);
        }
        sw = fof_wave_sum(sw);
        if (lane == 0) {
            for (int a = 0; a < 3; ++a) {
                double c = ref[a] + ss[a] / sw;
                if (boxsize > 0.0) {
                    if (c < 0.0) c = c + boxsize;
                    else if (c >= boxsize) c = c - boxsize;
                }
                cm[3 * g + a] = c;
                if (vel) cmv[3 * g + a] = sv[a] / sw;
            }
            weight[g] = sw;
        }
    }
}

inline bool fof_length_ok(double b) { return b > 0.0 && std::isfinite(b); }

// The cells the plan may use: a work item of the walk is (tile of up to 256 objects of a cell, neighbour cell), and
// with the pair finders' one cell per object a workgroup spends its time fetching items of a few pairs each.  One cell
// per FOF_CELL_OBJECTS objects, within [27, the layout's cap]; AST_FOF_CELL_OBJECTS (tests and measurements) sets
// another number, 1 giving the pair finders' plan.
inline unsigned fof_plan_cap(size_t n, const GridLayout& L) {
    size_t per = FOF_CELL_OBJECTS;
    if (const char* e = getenv("AST_FOF_CELL_OBJECTS")) per = strtoull(e, nullptr, 10);
    if (per < 1) per = 1;
    size_t cap = n / per;
    if (cap < 27) cap = 27;
    return (unsigned)(cap < L.cap ? cap : L.cap);
}

}  // namespace

extern "C" size_t ast_fof_workspace_bytes(size_t n) {
    if (!grid_count_ok(n)) return 0;
    return fof_layout(n).total;
}

extern "C" int ast_fof_max_passes(size_t n) {
    if (!grid_count_ok(n)) return 0;
    int bits = 0;
    while ((size_t(1) << bits) < n) ++bits;      // ceil(log2 n): no path is longer than n - 1 links
    return bits + 1;                             // and the pass that sees nothing pending
}

extern "C" int ast_fof_prepare(const void* pos_d, int pos_dtype, size_t n, void* work_d, size_t work_bytes,
                               double* bounds_d, void* stream) {
    AST_CHECK_ARG(pos_dtype == AST_F32 || pos_dtype == AST_F64);
    AST_CHECK_ARG(grid_count_ok(n));
    AST_CHECK_ARG(n == 0 || pos_d);
    AST_CHECK_ARG(bounds_d);
    const GridLayout L = fof_layout(n);
    AST_CHECK_ARG(work_d && work_bytes >= L.total);
    hipStream_t s = ast::as_stream(stream);
    char* ws = (char*)work_d;
    int* parent = (int*)(ws + L.part);
    return grid_prepare<1, FofObj>(ws, L, &n, bounds_d, "fof_prep", s, [&](int, FofObj* obj, GridBounds* box) {
        if (pos_dtype == AST_F32)
            fof_prep_kernel<float><<<ast::stream_grid(n, 256), 256, 0, s>>>((const float*)pos_d, n, obj, parent, box);
        else
            fof_prep_kernel<double><<<ast::stream_grid(n, 256), 256, 0, s>>>((const double*)pos_d, n, obj, parent, box);
    });
}

extern "C" int ast_fof_link(void* work_d, size_t work_bytes, size_t n, double boxsize, int cylinder, double b_perp,
                            double b_para, int los, int single_cell, unsigned long long* links_d, void* stream) {
    AST_CHECK_ARG(cylinder == 0 || cylinder == 1);
    AST_CHECK_ARG(fof_length_ok(b_perp) && (!cylinder || fof_length_ok(b_para)));
    AST_CHECK_ARG(los >= 0 && los <= 2);
    AST_CHECK_ARG(boxsize >= 0.0 && std::isfinite(boxsize));
    AST_CHECK_ARG(grid_count_ok(n));
    AST_CHECK_ARG(links_d);
    const GridLayout L = fof_layout(n);
    AST_CHECK_ARG(work_d && work_bytes >= L.total);
    hipStream_t s = ast::as_stream(stream);
    AST_CHECK_HIP(hipMemsetAsync(links_d, 0, sizeof(unsigned long long), s));
    if (grid_no_pairs(1, n, 0)) return AST_OK;
    char* ws = (char*)work_d;
    const GridSorted<FofObj, int> g(ws, L, 0);
    {
        AST_PROF("fof_grid", s);
        fof_plan_kernel<<<1, 64, 0, s>>>(g.prm, cylinder, b_perp, b_para, los, boxsize, fof_plan_cap(n, L), single_cell);
        AST_CHECK_LAUNCH();
        if (int rc = grid_sort_sets<FOF_BLOCK, FofObj>(ws, L, 0, &n, s)) return rc;
    }
    {
        AST_PROF("fof_link", s);
        const auto link = cylinder ? fof_link_kernel<FOF_CYLINDER> : fof_link_kernel<FOF_SPHERE>;
        link<<<FOF_GRID, FOF_BLOCK, 0, s>>>(g.sorted1, g.cell_start1, g.tile_start1, g.prm, boxsize, b_perp, b_para, los,
                                            g.part, links_d);
        AST_CHECK_LAUNCH();
    }
    return AST_OK;
}

extern "C" int ast_fof_compress(void* work_d, size_t work_bytes, size_t n, int* pending_d, int* passes_host, int* root_d,
                                unsigned* size_d, void* stream) {
    AST_CHECK_ARG(grid_count_ok(n) && n > 0);
    AST_CHECK_ARG(pending_d && passes_host && root_d && size_d);
    const GridLayout L = fof_layout(n);
    AST_CHECK_ARG(work_d && work_bytes >= L.total);
    hipStream_t s = ast::as_stream(stream);
    int* parent = (int*)((char*)work_d + L.part);
    const int bound = ast_fof_max_passes(n);
    AST_CHECK_HIP(hipMemsetAsync(pending_d, 0, sizeof(int) * (size_t)bound, s));
    const unsigned grid = ast::stream_grid(n, 256);
    *passes_host = 0;
    bool done = false;
    for (int pass = 0; pass < bound && !done; ++pass) {
        int more = 0;
        {
            AST_PROF("fof_jump", s);
            fof_jump_kernel<<<grid, 256, 0, s>>>(parent, n, pending_d + pass);
            AST_CHECK_LAUNCH();
        }
        AST_CHECK_HIP(hipMemcpyAsync(&more, pending_d + pass, sizeof(int), hipMemcpyDeviceToHost, s));
        AST_CHECK_HIP(hipStreamSynchronize(s));
        *passes_host = pass + 1;
        done = !more;
    }
    if (!done) {
        ast::set_error("%s: parents not resolved after %d passes (n %zu): the parent array is not a forest", __func__,
                       bound, n);
        return AST_ERR_LIMIT;                    // root_d and size_d are untouched
    }
    AST_CHECK_HIP(hipMemsetAsync(size_d, 0, sizeof(unsigned) * n, s));
    AST_PROF("fof_sizes", s);
    fof_sizes_kernel<<<grid, 256, 0, s>>>(parent, n, root_d, size_d);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

extern "C" int ast_fof_relabel(const int* root_d, const int* table_d, size_t n, int* labels_d, void* stream) {
    AST_CHECK_ARG(root_d && table_d && labels_d && n > 0 && grid_count_ok(n));
    hipStream_t s = ast::as_stream(stream);
    AST_PROF("fof_relabel", s);
    fof_relabel_kernel<<<ast::stream_grid(n, 256), 256, 0, s>>>(root_d, table_d, n, labels_d);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

extern "C" int ast_fof_features(const void* pos_d, int pos_dtype, const void* vel_d, int vel_dtype,
                                const void* weights_d, int weights_dtype, size_t n, const int* members_d,
                                const long long* offsets_d, const long long* first_d, size_t ngroups, double boxsize,
                                double* cm_d, double* cmv_d, double* weight_d, void* stream) {
    AST_CHECK_ARG(pos_dtype == AST_F32 || pos_dtype == AST_F64);
    AST_CHECK_ARG(vel_d == nullptr || vel_dtype == AST_F32 || vel_dtype == AST_F64);
    AST_CHECK_ARG(weights_d == nullptr || weights_dtype == AST_F32 || weights_dtype == AST_F64);
    AST_CHECK_ARG(grid_count_ok(n) && n > 0 && ngroups > 0 && ngroups <= n);
    AST_CHECK_ARG(pos_d && members_d && offsets_d && first_d && cm_d && weight_d && (vel_d == nullptr || cmv_d));
    AST_CHECK_ARG(boxsize >= 0.0 && std::isfinite(boxsize));
    hipStream_t s = ast::as_stream(stream);
    const unsigned grid = ast::stream_grid(ngroups * 64, 256);
    AST_PROF("fof_features", s);
    ast::dispatch_f32_f64(pos_dtype == AST_F32, vel_d && vel_dtype == AST_F32, [&](auto tp, auto tv) {
        using TP = decltype(tp);
        using TV = decltype(tv);
        if (weights_d && weights_dtype == AST_F32)
            fof_features_kernel<TP, TV, float><<<grid, 256, 0, s>>>(
                (const TP*)pos_d, (const TV*)vel_d, (const float*)weights_d, n, members_d, offsets_d, first_d, ngroups,
                boxsize, cm_d, cmv_d, weight_d);
        else
            fof_features_kernel<TP, TV, double><<<grid, 256, 0, s>>>(
                (const TP*)pos_d, (const TV*)vel_d, (const double*)weights_d, n, members_d, offsets_d, first_d, ngroups,
                boxsize, cm_d, cmv_d, weight_d);
    });
    AST_CHECK_LAUNCH();
    return AST_OK;
}
