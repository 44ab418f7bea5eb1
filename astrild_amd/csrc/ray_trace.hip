// Multi-plane ray tracing over lens planes: the potential of one plane, one ray step, one source.
//
//   ast_lens_green_multiply : the half spectrum of a padded plane times the discrete Green's function of the 5-point
//                             Laplacian, in place (between an R2C and a C2R of ast_fft_exec)
//   ast_ray_step            : advance every ray to the plane, then deflect it there; the state is updated in place
//   ast_ray_emit            : state -> kappa, gamma1, gamma2, omega, alpha1, alpha2 of one source distance
//
// No reference counterpart: the reference reads ray-traced maps from Ray-Ramses output.  Everything is double, one
// rounding per written operation (the library is built with -ffp-contract=off), in the order that the header states and
// tests/ray_trace_oracle.py restates in numpy; the GPU tests compare bytes.  One work item per ray (or per mode), no
// LDS, no workspace, nothing that outlives a call.  The per-ray arithmetic of the step and the emit is ray_step.h, which
// a host compiler takes too (tests/host/ray_step_test.cpp).
#include "ast_common.h"
#include "ray_step.h"

#include <cmath>

namespace {

constexpr int RAY_BX = 64, RAY_BY = 4;       // a workgroup: 4 rows of 64 consecutive rays (one wavefront per row)
using ast_ray::EMIT_PLANES;
using ast_ray::emit_ray;
using ast_ray::step_ray;

__global__ void __launch_bounds__(256)
green_multiply_kernel(double2* __restrict__ spec, int m, int nh, double scale) {
    const size_t count = (size_t)m * (size_t)nh;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const double dm = (double)m, top = -2.0 * scale;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += stride) {
        const int a = (int)(e / (size_t)nh), b = (int)(e - (size_t)a * (size_t)nh);
        const double sa = sinpi((double)a / dm), sb = sinpi((double)b / dm);
        const double g = e == 0 ? 0.0 : top / (4.0 * (sa * sa + sb * sb));
        double2 v = spec[e];
        v.x = e == 0 ? 0.0 : v.x * g;
        v.y = e == 0 ? 0.0 : v.y * g;
        spec[e] = v;
    }
}

template <bool BORN>
__global__ void __launch_bounds__(RAY_BX * RAY_BY)
ray_step_kernel(const double* __restrict__ psi, double* __restrict__ state, int m, int npix, double h, double chi_prev,
                double dchi, double chi_k) {
    const int j = blockIdx.x * RAY_BX + threadIdx.x, i = blockIdx.y * RAY_BY + threadIdx.y;
    if (i < npix && j < npix) step_ray<BORN>(psi, state, m, npix, i, j, h, chi_prev, dchi, chi_k);
}

__global__ void __launch_bounds__(256)
ray_emit_kernel(const double* __restrict__ state, size_t plane, double chi_k, double dchi, double chi_s,
                double* __restrict__ out, size_t out_stride) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < plane; e += stride)
        emit_ray(state, plane, e, chi_k, dchi, chi_s, out, out_stride);
}

// m x m doubles are addressable, and a node index plus the stencil stays far inside int
bool grid_fits(int m) { return m >= 1 && m <= (1 << 30); }

}  // namespace

extern "C" int ast_lens_green_multiply(void* spec_d, int m, double scale, void* stream) {
    AST_CHECK_ARG(grid_fits(m));
    AST_CHECK_ARG(std::isfinite(scale));
    AST_CHECK_ARG(spec_d != nullptr);
    const int nh = m / 2 + 1;
    hipStream_t s = ast::as_stream(stream);
    AST_PROF("lens_green_multiply", s);
    green_multiply_kernel<<<ast::stream_grid((size_t)m * (size_t)nh, 256), 256, 0, s>>>((double2*)spec_d, m, nh, scale);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

extern "C" int ast_ray_step(const double* psi_d, int m, double* state_d, int npix, double h, double chi_prev, double chi_k,
                            int born, void* stream) {
    AST_CHECK_ARG(grid_fits(m));
    AST_CHECK_ARG(npix >= 1 && npix <= m);
    AST_CHECK_ARG((npix + RAY_BY - 1) / RAY_BY <= 65535);
    AST_CHECK_ARG(std::isfinite(h) && h > 0.0 && std::isfinite(h * h) && h * h > 0.0);
    AST_CHECK_ARG(std::isfinite(chi_prev) && std::isfinite(chi_k) && chi_prev >= 0.0 && chi_k > chi_prev);
    AST_CHECK_ARG(born == 0 || born == 1);
    AST_CHECK_ARG(psi_d != nullptr && state_d != nullptr);
    hipStream_t s = ast::as_stream(stream);
    AST_PROF("ray_step", s);
    const dim3 block(RAY_BX, RAY_BY), grid((npix + RAY_BX - 1) / RAY_BX, (npix + RAY_BY - 1) / RAY_BY);
    const double dchi = chi_k - chi_prev;
    if (born) ray_step_kernel<true><<<grid, block, 0, s>>>(psi_d, state_d, m, npix, h, chi_prev, dchi, chi_k);
    else ray_step_kernel<false><<<grid, block, 0, s>>>(psi_d, state_d, m, npix, h, chi_prev, dchi, chi_k);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

extern "C" int ast_ray_emit(const double* state_d, int npix, double chi_k, double chi_s, double* out_d, size_t out_stride,
                            void* stream) {
    AST_CHECK_ARG(grid_fits(npix));
    AST_CHECK_ARG(std::isfinite(chi_k) && std::isfinite(chi_s) && chi_k > 0.0 && chi_s > chi_k);
    const size_t plane = (size_t)npix * (size_t)npix;
    AST_CHECK_ARG(out_stride >= plane && out_stride <= SIZE_MAX / 8 / EMIT_PLANES);
    AST_CHECK_ARG(state_d != nullptr && out_d != nullptr);
    hipStream_t s = ast::as_stream(stream);
    AST_PROF("ray_emit", s);
    ray_emit_kernel<<<ast::stream_grid(plane, 256), 256, 0, s>>>(state_d, plane, chi_k, chi_s - chi_k, chi_s, out_d, out_stride);
    AST_CHECK_LAUNCH();
    return AST_OK;
}
