// Particles -> P lens planes of npix x npix: projected mass assignment for a periodic box and for a light cone.
//
//   ast_plane_paint_exponent   : host only, the fixed-point exponent k of a declared particle count
//   ast_plane_paint_accumulate : sums[P, npix, npix] (int64) += the deposits of np particles, NGP / CIC / TSC
//   ast_plane_paint_finish     : out = (T)(sums * mul[p] (* cos^-3 in the cone) + add[p]), every element written
//
// No reference counterpart: the reference reads its planes from Ray-Ramses output (hard part 6).
//
// The contract (tests/plane_paint_oracle.py restates it in numpy and the GPU tests compare bytes): every
// deposit is formed in double in one fixed order, rounded ONCE to a multiple of q = vmax / 2^k and added as a 64-bit
// integer.  Integer addition is associative, so the planes hold the same bits for every particle order, chunking and
// launch geometry - which global float atomics cannot give.  One work item per particle, no LDS, no workspace.
#include "ast_common.h"
#include "paint_window.h"

#include <cfloat>
#include <cmath>

namespace {

using ast::Window;

constexpr int GEOM_BOX = 0, GEOM_CONE = 1;

struct PlaneGeom {
    int los, a, b;               // line of sight, and the two other axes in increasing order
    int nplanes, npix;
    double cl, c1, c0;           // box: plane = floor(x_los cl) mod P; both: s = u c1 + c0 (u = x, or d / d_los)
    double o0, o1, o2;           // cone: observer minus replication offset
    const double* e2;            // cone: nplanes + 1 squared shell edges, ascending (device)
};

__device__ inline double pick(double v0, double v1, double v2, int axis) { return axis == 0 ? v0 : axis == 1 ? v1 : v2; }

__device__ inline bool is_finite(double v) { return fabs(v) <= DBL_MAX; }

// periodic base pixel: locate<W>, then clamped in integer arithmetic (locate removes the period exactly for
// |s| < 2^52; beyond that its double -> int conversion saturates, and the clamp keeps the index inside the plane)
template <int W>
__device__ inline int periodic_base(double s, int n, double& frac) {
    const int b = ast::locate<W>(s, n, frac);
    return min(max(b, 0), n - 1);
}

// open base pixel: no wrap; clamped in double to [-2, n + 1], where every stencil point is outside [0, n)
template <int W>
__device__ inline int open_base(double s, int n, double& frac) {
    const double fl = floor(W == 2 ? s : s + 0.5);
    frac = s - fl;
    return (int)fmin(fmax(fl, -2.0), (double)n + 1.0);
}

template <typename Pt, int W, int G>
__global__ void __launch_bounds__(256)
plane_accumulate_kernel(const Pt* __restrict__ pos, const Pt* __restrict__ mass, size_t np, PlaneGeom g, double scale,
                        double vmax, double invq, long long* __restrict__ sums, unsigned long long* counters) {
    constexpr int LO = Window<W>::LO;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int npix = g.npix;
    unsigned long long n_outside = 0, n_clipped = 0, n_refused = 0;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < np; p += stride) {
        const double ms = (mass ? (double)mass[p] : 1.0) * scale;
        if (!(fabs(ms) <= vmax)) {                               // NaN, Inf, or a bound that was wrong
            ++n_refused;
            continue;
        }
        const double x0 = (double)pos[3 * p + 0], x1 = (double)pos[3 * p + 1], x2 = (double)pos[3 * p + 2];
        int plane, ba, bb;
        double fa, fb;
        if (G == GEOM_BOX) {
            const double sl = pick(x0, x1, x2, g.los) * g.cl;
            const double sa = pick(x0, x1, x2, g.a) * g.c1 + g.c0;
            const double sb = pick(x0, x1, x2, g.b) * g.c1 + g.c0;
            if (!(is_finite(sl) && is_finite(sa) && is_finite(sb))) {
                ++n_outside;
                continue;
            }
            double unused;
            plane = periodic_base<2>(sl, g.nplanes, unused);
            ba = periodic_base<W>(sa, npix, fa);
            bb = periodic_base<W>(sb, npix, fb);
        } else {
            const double d0 = x0 - g.o0, d1 = x1 - g.o1, d2 = x2 - g.o2;
            const double dl = pick(d0, d1, d2, g.los);
            const double r2 = (d0 * d0 + d1 * d1) + d2 * d2;
            if (!(is_finite(d0) && is_finite(d1) && is_finite(d2) && dl > 0.0 && r2 >= g.e2[0] && r2 < g.e2[g.nplanes])) {
                ++n_outside;
                continue;
            }
            int lo = 0, hi = g.nplanes;                          // e2[lo] <= r2 < e2[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (r2 >= g.e2[mid]) lo = mid;
                else hi = mid;
            }
            plane = lo;
            const double ta = pick(d0, d1, d2, g.a) / dl, tb = pick(d0, d1, d2, g.b) / dl;
            ba = open_base<W>(ta * g.c1 + g.c0, npix, fa);
            bb = open_base<W>(tb * g.c1 + g.c0, npix, fb);
        }
        double wa[W], wb[W];
        Window<W>::weights(fa, wa);
        Window<W>::weights(fb, wb);
        int kept = 0;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            int ia = ba - LO + i;
            if (G == GEOM_BOX) ia = ast::wrap1(ia, npix);
            else if ((unsigned)ia >= (unsigned)npix) continue;
            const double ma = ms * wa[i];
            long long* row = sums + ((size_t)plane * npix + ia) * npix;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                int ib = bb - LO + j;
                if (G == GEOM_BOX) ib = ast::wrap1(ib, npix);
                else if ((unsigned)ib >= (unsigned)npix) continue;
                const long long r = __double2ll_rn((ma * wb[j]) * invq);
                atomicAdd(reinterpret_cast<unsigned long long*>(row + ib), (unsigned long long)r);
                ++kept;
            }
        }
        if (G == GEOM_CONE) {
            if (kept == 0) ++n_outside;
            else if (kept < W * W) ++n_clipped;
        }
    }
    if (n_outside) atomicAdd(counters + 0, n_outside);
    if (n_clipped) atomicAdd(counters + 1, n_clipped);
    if (n_refused) atomicAdd(counters + 2, n_refused);
}

// V consecutive elements per work item (V * 8 bytes of sums read as 16-byte pieces, one store of V * sizeof(T) bytes);
// plane, row and pixel of the first element by two 64-bit divisions, the others by carry.
template <typename T, int G, int V>
__global__ void __launch_bounds__(256)
plane_finish_kernel(const long long* __restrict__ sums, const double* __restrict__ mul, const double* __restrict__ add,
                    int npix, double c1, size_t count, T* __restrict__ out) {
    typedef long long pair_t __attribute__((ext_vector_type(2)));
    typedef T vec_t __attribute__((ext_vector_type(V)));
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const double half = 0.5 * (double)npix;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count / V; i += stride) {
        const size_t e0 = i * V;
        long long s[V];
        if (V == 1) {
            s[0] = sums[e0];
        } else {
#pragma unroll
            for (int k = 0; k < V; k += 2) {
                const pair_t v = *reinterpret_cast<const pair_t*>(sums + e0 + k);
                s[k] = v.x;
                s[k + 1] = v.y;
            }
        }
        const size_t row = e0 / (size_t)npix;                    // p * npix + ia
        size_t p = row / (size_t)npix;
        int ia = (int)(row - p * (size_t)npix), ib = (int)(e0 - row * (size_t)npix);
        T r[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            double v = (double)s[k] * mul[p];
            if (G == GEOM_CONE) {
                const double ta = (((double)ia + 0.5) - half) / c1, tb = (((double)ib + 0.5) - half) / c1;
                const double w = (1.0 + ta * ta) + tb * tb;
                v = v * (w * sqrt(w));
            }
            r[k] = (T)(v + add[p]);
            if (++ib == npix) {
                ib = 0;
                if (++ia == npix) {
                    ia = 0;
                    ++p;
                }
            }
        }
        if (V == 1) {
            out[e0] = r[0];
        } else {
            vec_t o;
#pragma unroll
            for (int k = 0; k < V; ++k) o[k] = r[k];
            *reinterpret_cast<vec_t*>(out + e0) = o;
        }
    }
}

template <typename Pt, int G>
void launch_accumulate(int window, const Pt* pos, const Pt* mass, size_t np, const PlaneGeom& g, double scale, double vmax,
                       double invq, long long* sums, unsigned long long* counters, hipStream_t s) {
    const unsigned grid = ast::stream_grid(np, 256);
    switch (window) {
        case AST_WIN_NGP:
            plane_accumulate_kernel<Pt, 1, G><<<grid, 256, 0, s>>>(pos, mass, np, g, scale, vmax, invq, sums, counters);
            break;
        case AST_WIN_CIC:
            plane_accumulate_kernel<Pt, 2, G><<<grid, 256, 0, s>>>(pos, mass, np, g, scale, vmax, invq, sums, counters);
            break;
        default:
            plane_accumulate_kernel<Pt, 3, G><<<grid, 256, 0, s>>>(pos, mass, np, g, scale, vmax, invq, sums, counters);
            break;
    }
}

template <typename T, int G>
void launch_finish(const long long* sums, const double* mul, const double* add, int npix, double c1, size_t count, T* out,
                   hipStream_t s) {
    constexpr int V = 16 / (int)sizeof(T);
    const bool wide = count % V == 0 && (uintptr_t)sums % 16 == 0 && (uintptr_t)out % 16 == 0;
    if (wide) plane_finish_kernel<T, G, V><<<ast::stream_grid(count / V, 256), 256, 0, s>>>(sums, mul, add, npix, c1, count, out);
    else plane_finish_kernel<T, G, 1><<<ast::stream_grid(count, 256), 256, 0, s>>>(sums, mul, add, npix, c1, count, out);
}

// nplanes * npix^2 elements of 8 bytes are addressable, and base + stencil stays far inside int
bool planes_fit(int nplanes, int npix) {
    if (nplanes < 1 || npix < 1 || npix > (1 << 30)) return false;
    const size_t n = (size_t)npix;
    return n * n <= SIZE_MAX / 8 / (size_t)nplanes;
}

}  // namespace

extern "C" int ast_plane_paint_exponent(size_t np_total) {
    int bits = 0;
    for (size_t v = np_total; v; v >>= 1) ++bits;
    if (bits > 60) return -1;
    return bits <= 12 ? 50 : 62 - bits;
}

extern "C" int ast_plane_paint_accumulate(int geometry, int window, int dtype, const void* pos_d, const void* mass_d,
                                          size_t np, size_t np_total, int los, int nplanes, int npix, double cl, double c1,
                                          double c0, const double* origin, const double* e2_d, double scale, double vmax,
                                          long long* sums_d, unsigned long long* counters_d, void* stream) {
    AST_CHECK_ARG(geometry == AST_PLANE_BOX || geometry == AST_PLANE_CONE);
    AST_CHECK_ARG(window == AST_WIN_NGP || window == AST_WIN_CIC || window == AST_WIN_TSC);
    AST_CHECK_ARG(dtype == AST_F32 || dtype == AST_F64);
    AST_CHECK_ARG(los >= 0 && los <= 2);
    AST_CHECK_ARG(planes_fit(nplanes, npix));
    AST_CHECK_ARG(std::isfinite(c1) && c1 > 0.0 && std::isfinite(c0));
    AST_CHECK_ARG(std::isfinite(scale));
    AST_CHECK_ARG(std::isfinite(vmax) && vmax > 0.0);
    AST_CHECK_ARG(np_total >= np);
    const int k = ast_plane_paint_exponent(np_total);
    AST_CHECK_ARG(k >= 0);
    const double invq = std::ldexp(1.0, k) / vmax;
    AST_CHECK_ARG(std::isfinite(invq) && invq > 0.0);
    PlaneGeom g{};
    g.los = los;
    g.a = los == 0 ? 1 : 0;
    g.b = los == 2 ? 1 : 2;
    g.nplanes = nplanes;
    g.npix = npix;
    g.c1 = c1;
    g.c0 = c0;
    if (geometry == AST_PLANE_BOX) {
        AST_CHECK_ARG(std::isfinite(cl) && cl > 0.0);
        g.cl = cl;
    } else {
        AST_CHECK_ARG(origin != nullptr && e2_d != nullptr);
        AST_CHECK_ARG(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]));
        g.o0 = origin[0];
        g.o1 = origin[1];
        g.o2 = origin[2];
        g.e2 = e2_d;
    }
    if (np == 0) return AST_OK;
    AST_CHECK_ARG(pos_d != nullptr && sums_d != nullptr && counters_d != nullptr);
    hipStream_t s = ast::as_stream(stream);
    AST_PROF("plane_accumulate", s);
    if (dtype == AST_F32) {
        if (geometry == AST_PLANE_BOX)
            launch_accumulate<float, GEOM_BOX>(window, (const float*)pos_d, (const float*)mass_d, np, g, scale, vmax, invq, sums_d, counters_d, s);
        else
            launch_accumulate<float, GEOM_CONE>(window, (const float*)pos_d, (const float*)mass_d, np, g, scale, vmax, invq, sums_d, counters_d, s);
    } else {
        if (geometry == AST_PLANE_BOX)
            launch_accumulate<double, GEOM_BOX>(window, (const double*)pos_d, (const double*)mass_d, np, g, scale, vmax, invq, sums_d, counters_d, s);
        else
            launch_accumulate<double, GEOM_CONE>(window, (const double*)pos_d, (const double*)mass_d, np, g, scale, vmax, invq, sums_d, counters_d, s);
    }
    AST_CHECK_LAUNCH();
    return AST_OK;
}

extern "C" int ast_plane_paint_finish(int geometry, int out_dtype, const long long* sums_d, const double* mul_d,
                                      const double* add_d, int nplanes, int npix, double c1, void* out_d, void* stream) {
    AST_CHECK_ARG(geometry == AST_PLANE_BOX || geometry == AST_PLANE_CONE);
    AST_CHECK_ARG(out_dtype == AST_F32 || out_dtype == AST_F64);
    AST_CHECK_ARG(planes_fit(nplanes, npix));
    AST_CHECK_ARG(geometry == AST_PLANE_BOX || (std::isfinite(c1) && c1 > 0.0));
    AST_CHECK_ARG(sums_d != nullptr && mul_d != nullptr && add_d != nullptr && out_d != nullptr);
    const size_t count = (size_t)nplanes * (size_t)npix * (size_t)npix;
    hipStream_t s = ast::as_stream(stream);
    AST_PROF("plane_finish", s);
    if (out_dtype == AST_F32) {
        if (geometry == AST_PLANE_BOX) launch_finish<float, GEOM_BOX>(sums_d, mul_d, add_d, npix, c1, count, (float*)out_d, s);
        else launch_finish<float, GEOM_CONE>(sums_d, mul_d, add_d, npix, c1, count, (float*)out_d, s);
    } else {
        if (geometry == AST_PLANE_BOX) launch_finish<double, GEOM_BOX>(sums_d, mul_d, add_d, npix, c1, count, (double*)out_d, s);
        else launch_finish<double, GEOM_CONE>(sums_d, mul_d, add_d, npix, c1, count, (double*)out_d, s);
    }
    AST_CHECK_LAUNCH();
    return AST_OK;
}
