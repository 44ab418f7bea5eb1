// Operations on vector grids (N0, N1, N2, 3), components interleaved as np.load / read_density_grid deliver them:
// the finite-difference divergence of particles/hutils/map_transform.py (three np.gradient calls, edge_order=2), the
// vector magnitude of PowerSpectrum3D._get_vector_magnitude, and the divergence of three half spectra.  The stencil's
// arithmetic is fixed op by op (the library is built with -ffp-contract=off) so that it equals numpy's bit for bit;
// every constant is rounded to the array dtype before use, as numpy does with a Python scalar.  All indexing is 64-bit.
#include "ast_common.h"
#include <cmath>

namespace {

// The constants of np.gradient(f, h, edge_order=2), formed in double on the host and rounded to T once.
template <typename T>
struct GdConst {
    T two_h;            // interior: (f[i+1] - f[i-1]) / T(2 h)
    T a0, a1, a2;       // first cell: (a0 f[0] + a1 f[1]) + a2 f[2]
    T b0, b1, b2;       // last cell:  (b0 f[n-3] + b1 f[n-2]) + b2 f[n-1]
};

template <typename T>
GdConst<T> gd_const(double h) {
    GdConst<T> k;
    k.two_h = (T)(2.0 * h);
    k.a0 = (T)(-1.5 / h); k.a1 = (T)(2.0 / h); k.a2 = (T)(-0.5 / h);
    k.b0 = (T)(0.5 / h); k.b1 = (T)(-2.0 / h); k.b2 = (T)(1.5 / h);
    return k;
}

// The derivative at index i of the line f[0], f[stride], ..., f[(n - 1) stride], read from global memory.
template <typename T>
__device__ inline T gd_line(const T* __restrict__ f, size_t stride, long long i, long long n, bool periodic,
                            const GdConst<T>& k) {
    if (periodic || (i > 0 && i < n - 1)) {
        const long long ip = i + 1 == n ? 0 : i + 1, im = i == 0 ? n - 1 : i - 1;
        return (f[(size_t)ip * stride] - f[(size_t)im * stride]) / k.two_h;
    }
    if (i == 0) return (k.a0 * f[0] + k.a1 * f[stride]) + k.a2 * f[2 * stride];
    return (k.b0 * f[(size_t)(n - 3) * stride] + k.b1 * f[(size_t)(n - 2) * stride]) + k.b2 * f[(size_t)(n - 1) * stride];
}

// Variant 0: one work item per cell, every neighbour a plain load.
template <typename T>
__global__ void __launch_bounds__(256)
gd_cell_kernel(const T* __restrict__ v, T* __restrict__ out, long long n0, long long n1, long long n2, int periodic,
               GdConst<T> k) {
    const size_t cells = (size_t)n0 * (size_t)n1 * (size_t)n2;
    const size_t s1 = (size_t)n2 * 3, s0 = (size_t)n1 * s1;
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (size_t)gridDim.x * blockDim.x) {
        const long long z = (long long)(c % (size_t)n2);
        const size_t xy = c / (size_t)n2;
        const long long y = (long long)(xy % (size_t)n1), x = (long long)(xy / (size_t)n1);
        const T d0 = gd_line(v + ((size_t)y * s1 + (size_t)z * 3), s0, x, n0, periodic != 0, k);
        const T d1 = gd_line(v + ((size_t)x * s0 + (size_t)z * 3 + 1), s1, y, n1, periodic != 0, k);
        const T d2 = gd_line(v + ((size_t)x * s0 + (size_t)y * s1 + 2), (size_t)3, z, n2, periodic != 0, k);
        out[c] = (d0 + d1) + d2;
    }
}

// Variant 1.  A workgroup owns a tile of TY x TZ cells in (y, z) and marches along axis 0 over the planes [x0, x1) of
// its chunk.  Per plane the interleaved row segments of the tile and its halo of one cell, rows ylo .. yhi - 1 and
// cells zlo .. zhi - 1 clipped to the grid, go to LDS with 16-byte accesses: a row segment starts at scalar
// ((x n1 + y) n2 + zlo) 3 of the array, which is off the 16-byte grid by `mis` scalars, so the row is fetched from the
// aligned address below it and lands `mis` scalars into its LDS row (the head vector overhangs into the previous
// cells of the array, harmlessly; only a vector past the array's end is read scalar by scalar).  The next plane is
// fetched into registers while the current one is used, and written to the other LDS buffer: one barrier per plane.
// v_0 of the planes x - 1 and x + 1 is kept in registers; v_1 and v_2 of the plane take their +-1 neighbours from LDS.
// Cells on a face of the grid (first or last index on an axis) take that axis's derivative from global memory
// through gd_line: the one-sided formulas and the periodic wrap are surface work.
template <typename T, int RPT>
struct GdTile {
    static constexpr int V = 16 / (int)sizeof(T);
    static constexpr int TZ = 64, TY = 4 * RPT, ROWS = TY + 2;
    static constexpr int PITCH = (3 * (TZ + 2) + 2 * (V - 1)) / V * V;      // room for mis <= V - 1 in front
    static constexpr int VPR = PITCH / V, NVEC = ROWS * VPR, NV = (NVEC + 255) / 256;
    struct alignas(16) Vec { T e[V]; };
};

template <typename T, int RPT, bool PER>
__global__ void __launch_bounds__(256)
gd_tiled_kernel(const T* __restrict__ v, T* __restrict__ out, int n0, int n1, int n2, GdConst<T> k, unsigned nty,
                unsigned ntz, unsigned nchunks) {
    using G = GdTile<T, RPT>;
    using Vec = typename G::Vec;
    constexpr int V = G::V;
    __shared__ Vec lds_v[2][G::NVEC];
    const int tid = threadIdx.x, tz = tid & 63, ty = tid >> 6;
    const unsigned bid = blockIdx.x;
    const int z0 = (int)(bid % ntz) * G::TZ, y0 = (int)((bid / ntz) % nty) * G::TY;
    const unsigned ch = bid / (ntz * nty);
    const int x0 = (int)((long long)ch * n0 / nchunks), x1 = (int)((long long)(ch + 1) * n0 / nchunks);
    const int ylo = y0 > 0 ? y0 - 1 : 0, yhi = y0 + G::TY + 1 < n1 ? y0 + G::TY + 1 : n1;
    const int zlo = z0 > 0 ? z0 - 1 : 0, zhi = z0 + G::TZ + 1 < n2 ? z0 + G::TZ + 1 : n2;
    const int nrows = yhi - ylo, len = 3 * (zhi - zlo);
    const size_t s1 = (size_t)n2 * 3, s0 = (size_t)n1 * s1, total = (size_t)n0 * s0;
    const int z = z0 + tz;

    // A row's offset from the 16-byte grid: its first scalar's index (x s0 + y s1 + 3 zlo) mod V, in 32-bit arithmetic
    // (V is a power of two).
    const int s0m = (int)(s0 & (size_t)(V - 1)), s1m = (int)(s1 & (size_t)(V - 1)), zm = (3 * (zlo & (V - 1))) & (V - 1);
    auto row_mis = [&](int x, int y) { return ((x & (V - 1)) * s0m + (y & (V - 1)) * s1m + zm) & (V - 1); };

    // This thread's 16-byte pieces of a plane: piece u is vector ju[u] of tile row q / VPR, whose first scalar is
    // x s0 + rowu[u] in the array.
    Vec reg[G::NV];
    size_t rowu[G::NV];
    int ju[G::NV], yu[G::NV];
    bool useu[G::NV];
#pragma unroll
    for (int u = 0; u < G::NV; ++u) {
        const int q = tid + 256 * u, r = q / G::VPR;
        useu[u] = q < G::NVEC && r < nrows;
        ju[u] = (q % G::VPR) * V;
        yu[u] = ylo + r;
        rowu[u] = (size_t)(ylo + r) * s1 + (size_t)zlo * 3;
    }
    auto prefetch = [&](int x) {
        const size_t plane = (size_t)x * s0;
#pragma unroll
        for (int u = 0; u < G::NV; ++u) {
            const int mis = row_mis(x, yu[u]);
            if (!useu[u] || ju[u] >= mis + len) continue;
            const size_t g = plane + rowu[u] - (size_t)mis + (size_t)ju[u];
            if (g + V <= total) {
                reg[u] = *reinterpret_cast<const Vec*>(v + g);
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) reg[u].e[e] = g + e < total ? v[g + e] : (T)0;
            }
        }
    };
    auto commit = [&](int buf) {                    // a slot that prefetch skipped is never read
#pragma unroll
        for (int u = 0; u < G::NV; ++u)
            if (useu[u]) lds_v[buf][tid + 256 * u] = reg[u];
    };
    auto phys = [&](int p) -> int {                 // plane of the array behind march position p, -1: none
        if (p < 0) return PER ? p + n0 : -1;
        if (p >= n0) return PER ? p - n0 : -1;
        return p;
    };

    // This thread's cells: row y0 + ty + 4 r of the tile, column z.
    T a[RPT], b[RPT], h1[RPT], h2[RPT];             // v_0 of planes p - 2, p - 1; d1, d2 of plane p - 1
    int yc[RPT], atc[RPT];                          // the cell's row, and its LDS index less the row's misalignment
    bool live[RPT], y_in[RPT];
    size_t outc[RPT];
    const bool z_in = z > 0 && z < n2 - 1;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        a[r] = b[r] = h1[r] = h2[r] = (T)0;
        yc[r] = y0 + ty + 4 * r;
        live[r] = yc[r] < n1 && z < n2;
        y_in[r] = yc[r] > 0 && yc[r] < n1 - 1;
        atc[r] = (yc[r] - ylo) * G::PITCH + 3 * (z - zlo);
        outc[r] = (size_t)yc[r] * (size_t)n2 + (size_t)z;
    }
    const size_t cells_per_plane = (size_t)n1 * (size_t)n2;

    int buf = 0;
    {
        const int xf = phys(x0 - 1);
        if (xf >= 0) { prefetch(xf); commit(0); }
    }
    __syncthreads();
    for (int p = x0 - 1; p <= x1; ++p) {
        const int xp = phys(p), xn = p < x1 ? phys(p + 1) : -1;
        if (xn >= 0) prefetch(xn);
        const T* lds = reinterpret_cast<const T*>(lds_v[buf]);
        const bool plane_out = p >= x0 && p < x1;   // this plane's d1, d2 are needed (then xp == p)
        const int q = p - 1;
        const bool prev_out = q >= x0 && q < x1;
        const bool x_in = PER || (q > 0 && q < n0 - 1);
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            if (!live[r]) continue;
            const int y = yc[r];
            T c = (T)0, d1 = (T)0, d2 = (T)0;
            if (xp >= 0) {
                const int at = atc[r] + row_mis(xp, y);
                c = lds[at];
                if (plane_out) {
                    if (y_in[r]) {
                        const int up = atc[r] + G::PITCH + row_mis(xp, y + 1), dn = atc[r] - G::PITCH + row_mis(xp, y - 1);
                        d1 = (lds[up + 1] - lds[dn + 1]) / k.two_h;
                    } else {
                        d1 = gd_line(v + ((size_t)xp * s0 + (size_t)z * 3 + 1), s1, y, n1, PER, k);
                    }
                    if (z_in)
                        d2 = (lds[at + 5] - lds[at - 1]) / k.two_h;
                    else
                        d2 = gd_line(v + ((size_t)xp * s0 + (size_t)y * s1 + 2), (size_t)3, z, n2, PER, k);
                }
            }
            if (prev_out) {
                T d0;
                if (x_in)
                    d0 = (c - a[r]) / k.two_h;
                else
                    d0 = gd_line(v + ((size_t)y * s1 + (size_t)z * 3), s0, q, n0, false, k);
                __builtin_nontemporal_store((d0 + h1[r]) + h2[r], out + ((size_t)q * cells_per_plane + outc[r]));
            }
            a[r] = b[r]; b[r] = c; h1[r] = d1; h2[r] = d2;
        }
        if (xn >= 0) commit(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
vector_magnitude_kernel(const T* __restrict__ v, T* __restrict__ out, size_t count) {
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < count; c += (size_t)gridDim.x * blockDim.x) {
        const T v0 = v[3 * c], v1 = v[3 * c + 1], v2 = v[3 * c + 2];
        out[c] = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    }
}

// m of index j on an axis of n cells: j below n/2, j - n above, 0 on the Nyquist plane of an even n.
__device__ inline int sd_mode(int j, int n) {
    if (2 * j == n) return 0;
    return 2 * j < n ? j : j - n;
}

template <typename T>
__global__ void __launch_bounds__(256)
spectral_divergence_kernel(const T* cx, const T* cy, const T* cz, T* out, int n,      // out may be cx
                           double kf) {
    const int nh = n / 2 + 1;
    const size_t count = (size_t)n * (size_t)n * (size_t)nh;
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < count; c += (size_t)gridDim.x * blockDim.x) {
        const int j2 = (int)(c % (size_t)nh);
        const size_t xy = c / (size_t)nh;
        const int j1 = (int)(xy % (size_t)n), j0 = (int)(xy / (size_t)n);
        const T k0 = (T)(kf * (double)sd_mode(j0, n)), k1 = (T)(kf * (double)sd_mode(j1, n)),
                k2 = (T)(kf * (double)sd_mode(j2, n));
        const T re = (k0 * cx[2 * c] + k1 * cy[2 * c]) + k2 * cz[2 * c];
        const T im = (k0 * cx[2 * c + 1] + k1 * cy[2 * c + 1]) + k2 * cz[2 * c + 1];
        out[2 * c] = -im;           // i (re + i im)
        out[2 * c + 1] = re;
    }
}

// Tile rows per thread (the tile is 4 RPT x 64 cells) and the workgroups a launch aims at, as measured
// (profiles/grid_divergence_perf.txt): small tiles win, the kernel wants workgroups in flight more than
// it minds the halo rows it reads again.  -D overrides are for scripts/build_variants.sh.
#ifndef GD_RPT_F32
#define GD_RPT_F32 1
#endif
#ifndef GD_RPT_F64
#define GD_RPT_F64 2
#endif
#ifndef GD_GROUPS
#define GD_GROUPS 4096                          // 256 CUs x 16
#endif
constexpr unsigned GD_TARGET_GROUPS = GD_GROUPS;
constexpr long long GD_MIN_CHUNK = 8;           // planes per march chunk at least: 2 of its loads are halo planes

template <typename T, int RPT>
int gd_launch_tiled(const T* v, T* out, long long n0, long long n1, long long n2, int periodic, double h, hipStream_t s,
                    bool* declined) {
    using G = GdTile<T, RPT>;
    const size_t nty = (size_t)(n1 + G::TY - 1) / G::TY, ntz = (size_t)(n2 + G::TZ - 1) / G::TZ;
    const size_t tiles = nty * ntz;
    size_t nchunks = (GD_TARGET_GROUPS + tiles - 1) / tiles;
    const size_t most = (size_t)(n0 / GD_MIN_CHUNK) > 0 ? (size_t)(n0 / GD_MIN_CHUNK) : 1;
    if (nchunks > most) nchunks = most;
    // declined: more workgroups than one launch takes, an input off the 16-byte grid, sides whose tile arithmetic
    // would leave 32 bits
    const long long side_max = 0x7fffffffLL - 4 * (G::TY + G::TZ);
    if (tiles * nchunks > (size_t)0x7fffffff || ((uintptr_t)v & 15) != 0 || n1 > side_max || n2 > side_max) {
        *declined = true;
        return AST_OK;
    }
    *declined = false;
    AST_PROF("grid_divergence_tiled", s);
    const unsigned grid = (unsigned)(tiles * nchunks);
    if (periodic)
        gd_tiled_kernel<T, RPT, true><<<grid, 256, 0, s>>>(v, out, (int)n0, (int)n1, (int)n2, gd_const<T>(h),
                                                           (unsigned)nty, (unsigned)ntz, (unsigned)nchunks);
    else
        gd_tiled_kernel<T, RPT, false><<<grid, 256, 0, s>>>(v, out, (int)n0, (int)n1, (int)n2, gd_const<T>(h),
                                                            (unsigned)nty, (unsigned)ntz, (unsigned)nchunks);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

template <typename T>
int gd_launch(const void* v_d, void* out_d, size_t n0, size_t n1, size_t n2, double h, int periodic, int variant,
              hipStream_t s) {
    const T* v = (const T*)v_d;
    T* out = (T*)out_d;
    if (variant == 1) {
        bool declined = false;
        constexpr int RPT = sizeof(T) == 4 ? GD_RPT_F32 : GD_RPT_F64;
        const int rc = gd_launch_tiled<T, RPT>(v, out, (long long)n0, (long long)n1, (long long)n2, periodic, h, s, &declined);
        if (rc != AST_OK || !declined) return rc;
    }
    AST_PROF("grid_divergence_cell", s);
    gd_cell_kernel<T><<<ast::stream_grid(n0 * n1 * n2, 256), 256, 0, s>>>(v, out, (long long)n0, (long long)n1,
                                                                         (long long)n2, periodic, gd_const<T>(h));
    AST_CHECK_LAUNCH();
    return AST_OK;
}

}  // namespace

extern "C" int ast_grid_divergence(const void* v_d, void* out_d, int dtype, size_t n0, size_t n1, size_t n2, double h,
                                   int periodic, int variant, void* stream) {
    AST_CHECK_ARG(dtype == AST_F32 || dtype == AST_F64);
    AST_CHECK_ARG(v_d && out_d);
    AST_CHECK_ARG(n0 >= 3 && n1 >= 3 && n2 >= 3);
    AST_CHECK_ARG(n0 < (size_t(1) << 31) && n1 < (size_t(1) << 31) && n2 < (size_t(1) << 31));
    AST_CHECK_ARG((double)n0 * (double)n1 * (double)n2 < 1.0e18);
    AST_CHECK_ARG(std::isfinite(h) && h > 0.0);
    AST_CHECK_ARG(periodic == 0 || periodic == 1);
    AST_CHECK_ARG(variant == 0 || variant == 1);
    hipStream_t s = ast::as_stream(stream);
    if (dtype == AST_F32) return gd_launch<float>(v_d, out_d, n0, n1, n2, h, periodic, variant, s);
    return gd_launch<double>(v_d, out_d, n0, n1, n2, h, periodic, variant, s);
}

extern "C" int ast_vector_magnitude(const void* v_d, void* out_d, int dtype, size_t count, void* stream) {
    AST_CHECK_ARG(dtype == AST_F32 || dtype == AST_F64);
    AST_CHECK_ARG(count < (size_t(1) << 60));
    if (count == 0) return AST_OK;
    AST_CHECK_ARG(v_d && out_d);
    hipStream_t s = ast::as_stream(stream);
    AST_PROF("vector_magnitude", s);
    if (dtype == AST_F32)
        vector_magnitude_kernel<float><<<ast::stream_grid(count, 256), 256, 0, s>>>((const float*)v_d, (float*)out_d, count);
    else
        vector_magnitude_kernel<double><<<ast::stream_grid(count, 256), 256, 0, s>>>((const double*)v_d, (double*)out_d, count);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

extern "C" int ast_spectral_divergence(const void* cx_d, const void* cy_d, const void* cz_d, void* out_d, int cdtype,
                                       int nmesh, double boxsize, void* stream) {
    AST_CHECK_ARG(cdtype == AST_F32 || cdtype == AST_F64);
    AST_CHECK_ARG(cx_d && cy_d && cz_d && out_d);
    AST_CHECK_ARG(nmesh >= 2 && nmesh <= 8192);
    AST_CHECK_ARG(std::isfinite(boxsize) && boxsize > 0.0);
    hipStream_t s = ast::as_stream(stream);
    const double kf = 2.0 * M_PI / boxsize;
    const size_t count = (size_t)nmesh * (size_t)nmesh * (size_t)(nmesh / 2 + 1);
    AST_PROF("spectral_divergence", s);
    if (cdtype == AST_F32)
        spectral_divergence_kernel<float><<<ast::stream_grid(count, 256), 256, 0, s>>>(
            (const float*)cx_d, (const float*)cy_d, (const float*)cz_d, (float*)out_d, nmesh, kf);
    else
        spectral_divergence_kernel<double><<<ast::stream_grid(count, 256), 256, 0, s>>>(
            (const double*)cx_d, (const double*)cy_d, (const double*)cz_d, (double*)out_d, nmesh, kf);
    AST_CHECK_LAUNCH();
    return AST_OK;
}
