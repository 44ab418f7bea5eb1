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
// LDS, no workspace, nothing that outlives a call.
#include "ast_common.h"

#include <cmath>

namespace {

constexpr int RAY_BX = 64, RAY_BY = 4;       // a workgroup: 4 rows of 64 consecutive rays (one wavefront per row)
constexpr int STATE_PLANES = 12;             // d1 d2 s1 s2 A11 A12 A21 A22 B11 B12 B21 B22
constexpr int EMIT_PLANES = 6;               // kappa gamma1 gamma2 omega alpha1 alpha2
constexpr double INDEX_CLAMP = 1073741824.0; // 2^30: a ray further out than this many pixels is held there

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

// floor(p) reduced into [0, m): the clamp keeps the conversion defined for every bit pattern of p (fmax(NaN, x) = x),
// so no state of any content makes the kernel read outside psi
__host__ __device__ inline int wrapped_node(double fl, int m) {
    int a = (int)fmin(fmax(fl, -INDEX_CLAMP), INDEX_CLAMP);
    if ((unsigned)a >= (unsigned)m) {
        a %= m;
        if (a < 0) a += m;
    }
    return a;
}

__host__ __device__ inline double bilinear(double w00, double w10, double w01, double w11, double q00, double q10, double q01,
                                  double q11) {
    return ((w00 * q00 + w10 * q10) + w01 * q01) + w11 * q11;
}

// ray (i, j) of npix x npix through one plane (host-callable: the arithmetic can be run and checked without a device)
template <bool BORN>
__host__ __device__ inline void step_ray(const double* __restrict__ psi, double* __restrict__ state, int m, int npix, int i,
                                         int j, double h, double chi_prev, double dchi, double chi_k) {
    const size_t plane = (size_t)npix * (size_t)npix;
    double* st = state + (size_t)i * (size_t)npix + (size_t)j;
    double v[STATE_PLANES];
#pragma unroll
    for (int q = 0; q < STATE_PLANES; ++q) v[q] = st[q * plane];
    // advance: d from s, A from B
    const double d1 = (chi_prev * v[0] + dchi * v[2]) / chi_k, d2 = (chi_prev * v[1] + dchi * v[3]) / chi_k;
    const double A11 = (chi_prev * v[4] + dchi * v[8]) / chi_k, A12 = (chi_prev * v[5] + dchi * v[9]) / chi_k;
    const double A21 = (chi_prev * v[6] + dchi * v[10]) / chi_k, A22 = (chi_prev * v[7] + dchi * v[11]) / chi_k;
    // where the ray meets the plane, in nodes of psi
    const double p1 = BORN ? (double)i : (double)i + d1 / h, p2 = BORN ? (double)j : (double)j + d2 / h;
    const double f1 = floor(p1), f2 = floor(p2);
    const double fx = p1 - f1, fy = p2 - f2;
    int r[4], c[4];                                               // rows a - 1 .. a + 2, columns b - 1 .. b + 2
    r[1] = wrapped_node(f1, m);
    c[1] = wrapped_node(f2, m);
    r[0] = r[1] == 0 ? m - 1 : r[1] - 1;
    c[0] = c[1] == 0 ? m - 1 : c[1] - 1;
    r[2] = r[1] + 1 == m ? 0 : r[1] + 1;
    c[2] = c[1] + 1 == m ? 0 : c[1] + 1;
    r[3] = r[2] + 1 == m ? 0 : r[2] + 1;
    c[3] = c[2] + 1 == m ? 0 : c[2] + 1;
    double s[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const double* row = psi + (size_t)r[a] * (size_t)m;
#pragma unroll
        for (int b = 0; b < 4; ++b) s[a][b] = row[c[b]];
    }
    const double h2 = 2.0 * h, hh = h * h, hh4 = 4.0 * hh;
    double a1[2][2], a2[2][2], u11[2][2], u22[2][2], u12[2][2];   // at the nodes (a + x, b + y)
#pragma unroll
    for (int x = 0; x < 2; ++x) {
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int a = x + 1, b = y + 1;
            a1[x][y] = (s[a + 1][b] - s[a - 1][b]) / h2;
            a2[x][y] = (s[a][b + 1] - s[a][b - 1]) / h2;
            u11[x][y] = ((s[a + 1][b] - 2.0 * s[a][b]) + s[a - 1][b]) / hh;
            u22[x][y] = ((s[a][b + 1] - 2.0 * s[a][b]) + s[a][b - 1]) / hh;
            u12[x][y] = (((s[a + 1][b + 1] - s[a + 1][b - 1]) - s[a - 1][b + 1]) + s[a - 1][b - 1]) / hh4;
        }
    }
    const double w00 = (1.0 - fx) * (1.0 - fy), w10 = fx * (1.0 - fy), w01 = (1.0 - fx) * fy, w11 = fx * fy;
    const double al1 = bilinear(w00, w10, w01, w11, a1[0][0], a1[1][0], a1[0][1], a1[1][1]);
    const double al2 = bilinear(w00, w10, w01, w11, a2[0][0], a2[1][0], a2[0][1], a2[1][1]);
    const double U11 = bilinear(w00, w10, w01, w11, u11[0][0], u11[1][0], u11[0][1], u11[1][1]);
    const double U22 = bilinear(w00, w10, w01, w11, u22[0][0], u22[1][0], u22[0][1], u22[1][1]);
    const double U12 = bilinear(w00, w10, w01, w11, u12[0][0], u12[1][0], u12[0][1], u12[1][1]);
    // deflect
    st[0 * plane] = d1;
    st[1 * plane] = d2;
    st[2 * plane] = v[2] - al1;
    st[3 * plane] = v[3] - al2;
    st[4 * plane] = A11;
    st[5 * plane] = A12;
    st[6 * plane] = A21;
    st[7 * plane] = A22;
    if (BORN) {
        st[8 * plane] = v[8] - U11;
        st[9 * plane] = v[9] - U12;
        st[10 * plane] = v[10] - U12;
        st[11 * plane] = v[11] - U22;
    } else {
        st[8 * plane] = v[8] - (U11 * (1.0 + A11) + U12 * A21);
        st[9 * plane] = v[9] - (U11 * A12 + U12 * (1.0 + A22));
        st[10 * plane] = v[10] - (U12 * (1.0 + A11) + U22 * A21);
        st[11 * plane] = v[11] - (U12 * A12 + U22 * (1.0 + A22));
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
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < plane; e += stride) {
        double v[STATE_PLANES];
#pragma unroll
        for (int q = 0; q < STATE_PLANES; ++q) v[q] = state[q * plane + e];
        const double d1 = (chi_k * v[0] + dchi * v[2]) / chi_s, d2 = (chi_k * v[1] + dchi * v[3]) / chi_s;
        const double A11 = (chi_k * v[4] + dchi * v[8]) / chi_s, A12 = (chi_k * v[5] + dchi * v[9]) / chi_s;
        const double A21 = (chi_k * v[6] + dchi * v[10]) / chi_s, A22 = (chi_k * v[7] + dchi * v[11]) / chi_s;
        out[0 * out_stride + e] = -0.5 * (A11 + A22);
        out[1 * out_stride + e] = -0.5 * (A11 - A22);
        out[2 * out_stride + e] = -0.5 * (A12 + A21);
        out[3 * out_stride + e] = 0.5 * (A21 - A12);
        out[4 * out_stride + e] = -d1;
        out[5 * out_stride + e] = -d2;
    }
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
