// The per-ray arithmetic of the multi-plane ray tracer (ray_trace.hip): one ray through one plane
// (step_ray) and one ray's maps of one source (emit_ray).  Plain C++ that a host compiler takes as it is - the kernels
// of ray_trace.hip call these functions, tests/host/ray_step_test.cpp runs them under sanitizers and compares their
// bits with tests/ray_trace_oracle.py.  Everything is double, one rounding per written operation (build with
// -ffp-contract=off).
#pragma once
#include <cmath>
#include <cstddef>

#ifdef __HIPCC__
#define AST_RAY_HD __host__ __device__
#else
#define AST_RAY_HD
#endif

namespace ast_ray {

constexpr int STATE_PLANES = 12;             // d1 d2 s1 s2 A11 A12 A21 A22 B11 B12 B21 B22
constexpr int EMIT_PLANES = 6;               // kappa gamma1 gamma2 omega alpha1 alpha2
constexpr double INDEX_CLAMP = 1073741824.0; // 2^30: a ray further out than this many pixels is held there

// floor(p) reduced into [0, m): the clamp keeps the conversion defined for every bit pattern of p (fmax(NaN, x) = x),
// so no state of any content makes the kernel read outside psi
AST_RAY_HD inline int wrapped_node(double fl, int m) {
    int a = (int)fmin(fmax(fl, -INDEX_CLAMP), INDEX_CLAMP);
    if ((unsigned)a >= (unsigned)m) {
        a %= m;
        if (a < 0) a += m;
    }
    return a;
}

AST_RAY_HD inline double bilinear(double w00, double w10, double w01, double w11, double q00, double q10, double q01,
                                  double q11) {
    return ((w00 * q00 + w10 * q10) + w01 * q01) + w11 * q11;
}

// ray (i, j) of npix x npix through one plane (host-callable: the arithmetic can be run and checked without a device)
template <bool BORN>
AST_RAY_HD inline void step_ray(const double* __restrict__ psi, double* __restrict__ state, int m, int npix, int i,
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

// ray e of ``plane`` rays: the state after the plane at chi_k -> the six maps of a source at chi_s = chi_k + dchi,
// map q at out + q out_stride
AST_RAY_HD inline void emit_ray(const double* __restrict__ state, size_t plane, size_t e, double chi_k, double dchi,
                                double chi_s, double* __restrict__ out, size_t out_stride) {
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

}  // namespace ast_ray
