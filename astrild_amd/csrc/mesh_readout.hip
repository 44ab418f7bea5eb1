// Grid -> particles: a periodic grid field evaluated at positions with the NGP / CIC / TSC window.
//
//   ast_readout : pmesh RealField.readout(pos, resampler=), the adjoint of the ParticleMesh.paint that ast_paint
//                 replaces (particles/hutils/stats_subfind.py:130-131), for fields of 1 .. 4 interleaved components.
//
// The gather twin of paint_direct_kernel (mesh_paint.hip): the same s = fma(x, n/L, shift), the same locate<W>, the same
// Window<W>::weights in the field's precision.  The sum itself is a contract: weights widened to double,
// terms (wx[a] wy[b]) wz[c] * f added in the order a, b, c into a double that starts at 0, one rounding to the field's
// type at the end - so a numpy restatement (tests/readout_oracle.py) gives the same bits, on every call and for every
// launch geometry.  No LDS, no atomics, no workspace.
#include "ast_common.h"
#include "paint_window.h"

#include <cmath>

namespace {

using ast::Window;

// base cell of one axis: locate<W>, then clamped in integer arithmetic.  locate's (int) conversion saturates: a NaN
// or +-Inf coordinate comes out as 0, 1e300 as INT_MAX.  After the clamp no bit pattern addresses outside the field.
template <int W>
__device__ inline int base_cell(double s, int n, double& frac) {
    const int b = ast::locate<W>(s, n, frac);
    return min(max(b, 0), n - 1);
}

template <typename P, typename R, int W, int C>
__global__ void __launch_bounds__(256)
readout_kernel(const P* __restrict__ pos, size_t np, const R* __restrict__ field, int n, double inv_dx, double shift,
               R* __restrict__ out) {
    constexpr int LO = Window<W>::LO;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t pitch = (size_t)n * C;                          // elements of one z row
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < np; p += stride) {
        double fx, fy, fz;
        const int bx = base_cell<W>(__fma_rn((double)pos[3 * p + 0], inv_dx, shift), n, fx);
        const int by = base_cell<W>(__fma_rn((double)pos[3 * p + 1], inv_dx, shift), n, fy);
        const int bz = base_cell<W>(__fma_rn((double)pos[3 * p + 2], inv_dx, shift), n, fz);
        R wx[W], wy[W], wz[W];
        Window<W>::weights(fx, wx);
        Window<W>::weights(fy, wy);
        Window<W>::weights(fz, wz);
        int jx[W], jy[W], jz[W];
#pragma unroll
        for (int a = 0; a < W; ++a) {
            jx[a] = ast::wrap1(bx - LO + a, n);
            jy[a] = ast::wrap1(by - LO + a, n);
            jz[a] = ast::wrap1(bz - LO + a, n);
        }
        // the W cells along z are W * C contiguous elements unless the stencil wraps (always when n < W)
        const int z0 = bz - LO;
        const bool whole = z0 >= 0 && z0 + W <= n;
        double acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.0;
#pragma unroll
        for (int a = 0; a < W; ++a) {
#pragma unroll
            for (int b = 0; b < W; ++b) {
                const double wab = (double)wx[a] * (double)wy[b];
                const R* row = field + ((size_t)jx[a] * n + jy[b]) * pitch;
                R v[W * C];
                if (whole) {
                    const R* q = row + (size_t)z0 * C;
#pragma unroll
                    for (int k = 0; k < W * C; ++k) v[k] = q[k];
                } else {
#pragma unroll
                    for (int cz = 0; cz < W; ++cz) {
                        const R* q = row + (size_t)jz[cz] * C;
#pragma unroll
                        for (int c = 0; c < C; ++c) v[cz * C + c] = q[c];
                    }
                }
#pragma unroll
                for (int cz = 0; cz < W; ++cz) {
                    const double w = wab * (double)wz[cz];
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c] += w * (double)v[cz * C + c];
                }
            }
        }
        // a non-finite coordinate has frac = NaN (Inf - Inf, or NaN itself).  CIC and TSC weights carry it into every
        // term; the NGP weight is the constant 1, so the rule is applied by hand and holds for the three windows alike.
        const bool finite = fx == fx && fy == fy && fz == fz;
#pragma unroll
        for (int c = 0; c < C; ++c) out[p * C + c] = finite ? (R)acc[c] : (R)NAN;
    }
}

template <typename P, typename R, int W>
void launch_components(int ncomp, const P* pos, size_t np, const R* field, int n, double inv_dx, double shift, R* out,
                       hipStream_t s) {
    const unsigned g = ast::stream_grid(np, 256);
    switch (ncomp) {
        case 1: readout_kernel<P, R, W, 1><<<g, 256, 0, s>>>(pos, np, field, n, inv_dx, shift, out); break;
        case 2: readout_kernel<P, R, W, 2><<<g, 256, 0, s>>>(pos, np, field, n, inv_dx, shift, out); break;
        case 3: readout_kernel<P, R, W, 3><<<g, 256, 0, s>>>(pos, np, field, n, inv_dx, shift, out); break;
        default: readout_kernel<P, R, W, 4><<<g, 256, 0, s>>>(pos, np, field, n, inv_dx, shift, out); break;
    }
}

template <typename P, typename R>
void launch_readout(int window, int ncomp, const P* pos, size_t np, const R* field, int n, double inv_dx, double shift,
                    R* out, hipStream_t s) {
    switch (window) {
        case AST_WIN_NGP: launch_components<P, R, 1>(ncomp, pos, np, field, n, inv_dx, shift, out, s); break;
        case AST_WIN_CIC: launch_components<P, R, 2>(ncomp, pos, np, field, n, inv_dx, shift, out, s); break;
        default: launch_components<P, R, 3>(ncomp, pos, np, field, n, inv_dx, shift, out, s); break;
    }
}

}  // namespace

extern "C" int ast_readout(int window, int field_dtype, int pos_dtype, const void* field_d, int nmesh, int ncomp,
                           const void* pos_d, size_t np, double boxsize, double shift_cells, void* out_d, void* stream) {
    AST_CHECK_ARG(window == AST_WIN_NGP || window == AST_WIN_CIC || window == AST_WIN_TSC);
    AST_CHECK_ARG(field_dtype == AST_F32 || field_dtype == AST_F64);
    AST_CHECK_ARG(pos_dtype == AST_F32 || pos_dtype == AST_F64);
    AST_CHECK_ARG(nmesh >= 1);
    AST_CHECK_ARG(ncomp >= 1 && ncomp <= 4);
    const size_t n = (size_t)nmesh;
    AST_CHECK_ARG(n * n <= SIZE_MAX / n / (size_t)ncomp);        // nmesh^3 * ncomp fits in size_t
    AST_CHECK_ARG(boxsize > 0.0 && std::isfinite(boxsize));
    AST_CHECK_ARG(std::isfinite(shift_cells));
    if (np == 0) return AST_OK;
    AST_CHECK_ARG(field_d != nullptr && pos_d != nullptr && out_d != nullptr);
    hipStream_t s = ast::as_stream(stream);
    const double inv_dx = (double)nmesh / boxsize;
    AST_PROF("readout", s);
    ast::dispatch_f32_f64(pos_dtype == AST_F32, field_dtype == AST_F32, [&](auto tp, auto tr) {
        using P = decltype(tp);
        using R = decltype(tr);
        launch_readout<P, R>(window, ncomp, (const P*)pos_d, np, (const R*)field_d, nmesh, inv_dx, shift_cells,
                             (R*)out_d, s);
    });
    AST_CHECK_LAUNCH();
    return AST_OK;
}
