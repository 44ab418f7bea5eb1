// Double-precision transforms written by hand: column and row transforms of the zero-padded lens convolution.  (The
// register FFTs, the three-stage scheme and the forward row kernel are in fft_three_stage.h, shared with cube_fft.hip.)
//
// Column transforms of the zero-padded lens convolution (kappa -> alpha / phi, lensing_funcs.c:85-115 with
// fft_convolve.c:60-90) in double precision, hand-written because the half that is zero can be skipped and rocFFT's
// strided 8192-point double transform moves its data at 1.1 TB/s (0.98 ms per pass over the 537 MB half spectrum).
//
// A column of L = N1 * N2 points (8192 = 64 * 128) does not fit LDS with enough neighbours for whole cache lines
// (16 columns x 8192 x 16 B = 2 MB), so it is transformed in TWO in-place passes over the array (four-step FFT):
//   pass A   for every n2: the N1-point transform over n1 of x[N2 n1 + n2] (rows N2 apart), times W_L^{n2 k1},
//            stored at row N2 k1 + n2;
//   pass B   for every k1: the N2-point transform over n2 of the N2 CONSECUTIVE rows N2 k1 + n2, stored at row
//            N2 k1 + k2.
// Frequency k = k1 + N1 k2 therefore ends up at row N2 k1 + k2: a fixed permutation of the rows.  Nothing downstream
// needs the natural order - the spectra are only multiplied point by point with kernel spectra that went through the
// same two passes, and the inverse (pass B backwards, conjugate twiddle, pass A backwards) undoes it.
// A convolution (ast_lens_cols_convolve) runs forward pass B, the product(s) and inverse pass B as ONE pass
// (col_mid_kernel): they touch the same N2 rows x 16 columns, and the spectrum is then never written to memory.
// Zero padding: the forward pass A reads the first `in_points` of its N1 points only (rows >= Nc hold zeros that are
// never stored either), the last inverse pass writes the first `out_points` only (the corner that is kept).
// Each workgroup works on 16 adjacent columns (256-byte row pieces): R1 x R2 register FFTs with one LDS exchange,
// the scheme of fft_tile.hip's strided pass in double.
#include "fft_three_stage.h"

namespace {

// One pass.  Workgroup (column tile, group g): points j < NP = R1 * R2 at rows row0(g) + j * point_rows, 16 columns.
//   in_points:  points >= in_points are zero and not loaded (a multiple of R2);
//   out_points: points >= out_points are not stored;
//   twist:      multiply output point j by W_L^{+-(g j)} (the four-step twiddle; tw_big has L entries);
//   mul:        multiply every loaded value by mul[same index] (the convolution's kernel spectrum, fused into the first
//               inverse pass), the result goes to `out` (may equal `in`).
// INV: conj(FFT(conj(.))), the twist conjugated.
template <int R1, int R2, int C, bool INV>
__global__ void __launch_bounds__(C * (R1 > R2 ? R1 : R2))
col_pass_kernel(const double2* __restrict__ in, const double2* __restrict__ mul, double2* __restrict__ out, size_t pitch,
                int ncols, size_t group_rows, size_t point_rows, int in_points, int out_points, int twist,
                const double2* __restrict__ tw_big, int big_len) {
    constexpr int NP = R1 * R2;
    constexpr int NT = C * (R1 > R2 ? R1 : R2);
    __shared__ double2 Y[NP * C];
    __shared__ double2 tw[NP];                            // e^{-2 pi i m / NP}
    for (int i = threadIdx.x; i < NP; i += NT) tw[i] = tw_big[(size_t)i * (big_len / NP)];
    const int c = threadIdx.x % C, sub = threadIdx.x / C;
    const size_t c0 = (size_t)blockIdx.x * C;
    const int g = blockIdx.y;
    const bool col_ok = c0 + c < (size_t)ncols;
    const size_t base = (size_t)g * group_rows * pitch + min(c0 + c, (size_t)ncols - 1);
    const size_t pstride = point_rows * pitch;
    if (sub < R2) {                                       // stage 1: task (c, n2 = sub)
        double2 v[R1];
#pragma unroll
        for (int n1 = 0; n1 < R1; ++n1) {
            v[n1] = make_double2(0.0, 0.0);
            if (n1 * R2 < in_points) {                    // uniform: in_points is a multiple of R2
                const size_t idx = base + (size_t)(n1 * R2 + sub) * pstride;
                v[n1] = in[idx];
                if (mul) v[n1] = cmul(v[n1], mul[idx]);
            }
        }
        if (INV) {
#pragma unroll
            for (int n1 = 0; n1 < R1; ++n1) v[n1].y = -v[n1].y;
        }
        fft_reg<R1>(v);
        __syncthreads();                                  // the twiddle table is in LDS
#pragma unroll
        for (int k1 = 0; k1 < R1; ++k1) {
            double2 y = v[bitrev(k1, ilog2(R1))];
            if (k1 != 0) y = cmul(y, tw[sub * k1]);
            Y[(sub * R1 + k1) * C + c] = y;
        }
    } else {
        __syncthreads();
    }
    __syncthreads();
    if (sub < R1) {                                       // stage 2: task (c, k1 = sub)
        double2 u[R2];
#pragma unroll
        for (int n2 = 0; n2 < R2; ++n2) u[n2] = Y[(n2 * R1 + sub) * C + c];
        fft_reg<R2>(u);
        if (col_ok) {
#pragma unroll
            for (int k2 = 0; k2 < R2; ++k2) {
                const int j = sub + R1 * k2;              // output point
                if (j >= out_points) continue;
                double2 x = u[bitrev(k2, ilog2(R2))];
                if (twist) x = cmul(x, tw_big[(size_t)((g * j) % big_len)]);     // W_L^{g j}; INV: conjugated below with x
                if (INV) x.y = -x.y;
                out[base + (size_t)j * pstride] = x;
            }
        }
    }
}

// The middle of a column convolution in one pass: the forward transform's second pass (group g = k1, points n2 at
// consecutive rows), the product with NMUL kernel spectra and the inverse's first pass (back to n2, times conj W_L^{k1 n2})
// all work on the same NP rows x C columns, so the spectrum itself is never written: `in` holds pass A's output, out_m
// what the inverse's last pass (pass A backwards) reads.  Forward as NP = RA * RB (RA-point transforms in registers, LDS
// exchange, RB-point transforms), which leaves thread (c, sub < RA) with the points sub + RA k2 - exactly the input
// layout of an inverse split the other way round (RB-point transforms first), so the products are formed in place.
// Three workgroups per CU, and the second kernel spectrum is fetched only when its turn comes.  Measured at 8192 rows, two
// kernels: 0.585 ms; fetching it ahead cost 34 spilled registers (0.629 ms), or one workgroup per CU less (0.690 ms).
constexpr int MID_WAVES = 3;
template <int RA, int RB, int C, int NMUL>
__global__ void __launch_bounds__(C * (RA > RB ? RA : RB)) __attribute__((amdgpu_waves_per_eu(MID_WAVES)))
col_mid_kernel(const double2* __restrict__ in, const double2* __restrict__ mul0, const double2* __restrict__ mul1,
               double2* __restrict__ out0, double2* __restrict__ out1, size_t pitch, int ncols,
               const double2* __restrict__ tw_big, int big_len) {
    constexpr int NP = RA * RB;
    constexpr int NT = C * (RA > RB ? RA : RB);
    __shared__ double2 Y[NP * C];
    __shared__ double2 tw[NP];                            // e^{-2 pi i m / NP}
    for (int i = threadIdx.x; i < NP; i += NT) tw[i] = tw_big[(size_t)i * (big_len / NP)];
    const int c = threadIdx.x % C, sub = threadIdx.x / C;
    const size_t c0 = (size_t)blockIdx.x * C;
    const int g = blockIdx.y;
    const bool col_ok = c0 + c < (size_t)ncols;
    // addresses: a uniform row base per point plus ONE 32-bit lane offset (host check: pitch < 2^24)
    const size_t gbase = (size_t)g * NP * pitch;
    const uint32_t voff = (uint32_t)sub * (uint32_t)pitch + min((uint32_t)c0 + (uint32_t)c, (uint32_t)ncols - 1u);
    double2 m[RB];                                        // the kernel spectrum at this thread's points (sub < RA)
    auto fetch_mul = [&](const double2* __restrict__ mul) {
#pragma unroll
        for (int k2 = 0; k2 < RB; ++k2) m[k2] = (mul + gbase + (size_t)(RA * k2) * pitch)[voff];
    };
    // (every barrier of this kernel is reached by ALL threads outside any branch: ADVICE r3 - the <16, 8> shape used to
    // execute two different s_barrier instructions in the two arms of `if (sub < RB)`)
    const bool task1 = sub < RB;                          // forward stage 1: task (c, n2 = sub)
    double2 v[RA];
    if (task1) {
#pragma unroll
        for (int n1 = 0; n1 < RA; ++n1) v[n1] = (in + gbase + (size_t)(n1 * RB) * pitch)[voff];
    }
    if (sub < RA) fetch_mul(mul0);                        // in flight across the exchange
    if (task1) fft_reg<RA>(v);
    __syncthreads();                                      // the twiddle table is in LDS
    if (task1) {
#pragma unroll
        for (int k1 = 0; k1 < RA; ++k1) {
            double2 y = v[bitrev(k1, ilog2(RA))];
            if (k1 != 0) y = cmul(y, tw[sub * k1]);
            Y[(sub * RA + k1) * C + c] = y;
        }
    }
    __syncthreads();
    double2 X[RB];                                        // sub < RA: spectrum point sub + RA k2 in X[bitrev(k2)]
    if (sub < RA) {
#pragma unroll
        for (int n2 = 0; n2 < RB; ++n2) X[n2] = Y[(n2 * RA + sub) * C + c];
        fft_reg<RB>(X);
    }
#pragma unroll
    for (int which = 0; which < NMUL; ++which) {
        double2* __restrict__ out = which ? out1 : out0;
        __syncthreads();                                  // Y has been read by everyone
        if (which && sub < RA) fetch_mul(mul1);
        if (sub < RA) {                                   // inverse stage 1: task (c, n2' = sub), points n1' RA + sub, n1' = k2
            double2 w[RB];
#pragma unroll
            for (int k2 = 0; k2 < RB; ++k2) {
                w[k2] = cmul(X[bitrev(k2, ilog2(RB))], m[k2]);
                w[k2].y = -w[k2].y;
            }
            fft_reg<RB>(w);
#pragma unroll
            for (int k1 = 0; k1 < RB; ++k1) {
                double2 y = w[bitrev(k1, ilog2(RB))];
                if (k1 != 0) y = cmul(y, tw[sub * k1]);
                Y[(sub * RB + k1) * C + c] = y;
            }
        }
        __syncthreads();
        if (sub < RB) {                                   // inverse stage 2: task (c, k1' = sub)
            double2 u[RA];
#pragma unroll
            for (int n2 = 0; n2 < RA; ++n2) u[n2] = Y[(n2 * RB + sub) * C + c];
            fft_reg<RA>(u);
            if (col_ok) {
#pragma unroll
                for (int k2 = 0; k2 < RA; ++k2) {
                    const int j = sub + RB * k2;          // output point n2
                    double2 x = cmul(u[bitrev(k2, ilog2(RA))], tw_big[(size_t)((g * j) % big_len)]);
                    x.y = -x.y;
                    (out + gbase + (size_t)(RB * k2) * pitch)[voff] = x;
                }
            }
        }
    }
}

// ------------------------------------------------------------------ row transforms of the padded convolution
// Row r < nc of the padded (2nc)^2 array holds nc reals followed by nc zeros.  Its real-to-complex transform of length
// L = 2nc is the M = nc point complex transform of z[j] = x[2j] + i x[2j+1] (z[j] = 0 for j >= M / 2) followed by the
// even/odd split; the M = RA RB RC points (with_radices) go through the three-stage scheme of fft_three_stage.h, one row
// per workgroup; the forward kernel (lens_rows_forward_kernel, ZPAD) is there too.
// rocFFT's batched 1-D plans did these rows at 2.2 TB/s and needed the zero half in memory, a pad kernel before and a
// crop kernel after; here kappa is read as it is (134 MB per map) and the inverse stores the kept, scaled corner.

// rows of the product spectrum -> the kept corner: out[row][0 .. nc) = scale * (first nc reals of the length-2nc C2R)
template <int RA, int RB, int RC>
__global__ void __launch_bounds__((RowGeo<RA, RB, RC>::NT))
lens_rows_inverse_kernel(const double2* __restrict__ spec, size_t pitch, int nc, double scale, double* __restrict__ out,
                         const double2* __restrict__ twM, const double2* __restrict__ twL) {
    using G = RowGeo<RA, RB, RC>;
    constexpr int M = G::M;
    extern __shared__ double2 Y[];
    const int t = threadIdx.x;
    const size_t row = blockIdx.x;
    const double2* xrow = spec + row * pitch;
    // Z[k] = (X[k] + conj X[M-k]) / 2 + i w^{-k} (X[k] - conj X[M-k]) / 2, conjugated for the conj-FFT-conj inverse
    auto emit = [&](int k, double2 xk, double2 xm, double2 w) {
        const double2 e = make_double2(0.5 * (xk.x + xm.x), 0.5 * (xk.y - xm.y));
        const double2 d = make_double2(0.5 * (xk.x - xm.x), 0.5 * (xk.y + xm.y));
        const double2 tt = make_double2(fma(d.x, w.x, d.y * w.y), fma(d.y, w.x, -d.x * w.y));       // conj(w^k) d
        // Z[k] = e + i t;  Z[M-k] follows from the same formula with k -> M - k:
        //   e' = conj e, d' = -conj d, w^{-(M-k)} = -conj(w^{-k})  ->  t' = conj t,  Z[M-k] = conj(e) + i conj(t)
        if (k < M) Y[lds_pad(k)] = make_double2(e.x - tt.y, -(e.y + tt.x));                         // conj(Z[k])
        if (k != 0 && k != M / 2) Y[lds_pad(M - k)] = make_double2(e.x + tt.y, -(tt.x - e.y));      // conj(Z[M-k]) = e - i t
    };
    // the whole row in flight before the first use: (M / 2) / NT pairs per thread, k = M / 2 by thread 0
    constexpr int IT = (M / 2) / G::NT;
    static_assert(IT * G::NT == M / 2, "row length and thread count");
    {
        double2 xk[IT], xm[IT], wk[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int k = t + it * G::NT;
            xk[it] = xrow[k];
            xm[it] = xrow[M - k];
            wk[it] = twL[k];
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) emit(t + it * G::NT, xk[it], xm[it], wk[it]);
        if (t == 0) emit(M / 2, xrow[M / 2], xrow[M / 2], twL[M / 2]);
    }
    __syncthreads();
    double2 va[RA], vc[RC];
    if (t < G::T1) {
#pragma unroll
        for (int a = 0; a < RA; ++a) va[a] = Y[lds_pad(G::T1 * a + t)];
    }
    __syncthreads();                                      // the line is overwritten by the stages
    three_stage<RA, RB, RC>(va, vc, Y, twM, t);
    __syncthreads();
    // z[j], j = alpha + RA beta + RA RB gamma < M / 2, i.e. gamma < RC / 2: the kept half
    if (t < G::T3) {
#pragma unroll
        for (int ga = 0; ga < RC / 2; ++ga) Y[lds_pad((t / RB) + RA * (t % RB) + RA * RB * ga)] = vc[bitrev(ga, ilog2(RC))];
    }
    __syncthreads();
    double2* orow = reinterpret_cast<double2*>(out + row * (size_t)nc);
    const double s2 = 2.0 * scale;
    for (int j = t; j < M / 2; j += G::NT) {
        const double2 zz = Y[lds_pad(j)];                 // conj of z[j]
        orow[j] = make_double2(zz.x * s2, -zz.y * s2);    // x[2j] = 2 Re z, x[2j+1] = 2 Im z
    }
}

template <int R1, int R2, bool INV>
int launch_pass(const double2* in, const double2* mul, double2* out, size_t pitch, int ncols, int groups, size_t group_rows,
                size_t point_rows, int in_points, int out_points, int twist, const double2* tw_big, int big_len, hipStream_t s) {
    constexpr int C = 16, NT = C * (R1 > R2 ? R1 : R2);
    const dim3 grid((unsigned)((ncols + C - 1) / C), (unsigned)groups);
    col_pass_kernel<R1, R2, C, INV><<<grid, NT, 0, s>>>(in, mul, out, pitch, ncols, group_rows, point_rows, in_points, out_points,
                                                       twist, tw_big, big_len);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

// L = N1 * N2 with N1 = R1a * R2a (pass A, rows N2 apart) and N2 = R1b * R2b (pass B, consecutive rows)
struct Split { int n1, n2; };
bool split_of(size_t len, Split& sp) {
    switch (len) {
        case 16384: sp = {128, 128}; return true;
        case 8192: sp = {64, 128}; return true;
        case 4096: sp = {64, 64}; return true;
        case 2048: sp = {32, 64}; return true;
        case 1024: sp = {32, 32}; return true;
        case 512: sp = {16, 32}; return true;
        case 256: sp = {16, 16}; return true;
        default: return false;
    }
}

template <bool INV>
int pass_of(int np, const double2* in, const double2* mul, double2* out, size_t pitch, int ncols, int groups, size_t group_rows,
            size_t point_rows, int in_points, int out_points, int twist, const double2* tw_big, int big_len, hipStream_t s) {
    switch (np) {
        case 128: return launch_pass<8, 16, INV>(in, mul, out, pitch, ncols, groups, group_rows, point_rows, in_points, out_points, twist, tw_big, big_len, s);
        case 64: return launch_pass<8, 8, INV>(in, mul, out, pitch, ncols, groups, group_rows, point_rows, in_points, out_points, twist, tw_big, big_len, s);
        case 32: return launch_pass<4, 8, INV>(in, mul, out, pitch, ncols, groups, group_rows, point_rows, in_points, out_points, twist, tw_big, big_len, s);
        default: return launch_pass<4, 4, INV>(in, mul, out, pitch, ncols, groups, group_rows, point_rows, in_points, out_points, twist, tw_big, big_len, s);
    }
}

template <int RA, int RB, int NMUL>
int launch_mid(const double2* in, const double2* const* muls, double2* const* outs, size_t pitch, int ncols, int groups,
               const double2* tw_big, int big_len, hipStream_t s) {
    constexpr int C = 16, NT = C * (RA > RB ? RA : RB);
    const dim3 grid((unsigned)((ncols + C - 1) / C), (unsigned)groups);
    col_mid_kernel<RA, RB, C, NMUL><<<grid, NT, 0, s>>>(in, muls[0], muls[NMUL - 1], outs[0], outs[NMUL - 1], pitch, ncols, tw_big,
                                                        big_len);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

template <int NMUL>
int mid_of(int np, const double2* in, const double2* const* muls, double2* const* outs, size_t pitch, int ncols, int groups,
           const double2* tw_big, int big_len, hipStream_t s) {
    switch (np) {
        case 128: return launch_mid<16, 8, NMUL>(in, muls, outs, pitch, ncols, groups, tw_big, big_len, s);
        case 64: return launch_mid<8, 8, NMUL>(in, muls, outs, pitch, ncols, groups, tw_big, big_len, s);
        case 32: return launch_mid<4, 8, NMUL>(in, muls, outs, pitch, ncols, groups, tw_big, big_len, s);
        default: return launch_mid<4, 4, NMUL>(in, muls, outs, pitch, ncols, groups, tw_big, big_len, s);
    }
}

}  // namespace

extern "C" int ast_lens_cols_supported(size_t len) {
    Split sp;
    return split_of(len, sp) ? 1 : 0;
}

// Forward column transform, in place, of data_d[len][pitch] (complex double; `ncols` <= pitch columns used): rows >=
// nonzero_rows are taken as zero and never read (nonzero_rows = len: a full transform; otherwise len / 2).  The result
// is in the permuted row order described at the top of this file.
extern "C" int ast_lens_cols_forward(void* data, size_t len, size_t pitch, size_t ncols, size_t nonzero_rows, void* stream) {
    AST_CHECK_ARG(data != nullptr && ncols >= 1 && ncols <= pitch);
    Split sp;
    AST_CHECK_ARG(split_of(len, sp));
    AST_CHECK_ARG(nonzero_rows == len || nonzero_rows == len / 2);
    hipStream_t s = ast::as_stream(stream);
    const double2* tw = twiddles64((int)len, s);
    if (!tw) { ast::set_error("ast_lens_cols_forward: twiddle table allocation failed"); return AST_ERR_HIP; }
    double2* d = (double2*)data;
    AST_PROF("lens.cols_fwd", s);
    // pass A: group = n2 (first row n2), points n1 at rows N2 apart; rows >= len / 2 are points n1 >= N1 / 2
    int rc = pass_of<false>(sp.n1, d, nullptr, d, pitch, (int)ncols, sp.n2, 1, (size_t)sp.n2,
                            nonzero_rows == len ? sp.n1 : sp.n1 / 2, sp.n1, 1, tw, (int)len, s);
    if (rc != AST_OK) return rc;
    // pass B: group = k1 (first row N2 k1), points n2 at consecutive rows
    return pass_of<false>(sp.n2, d, nullptr, d, pitch, (int)ncols, sp.n1, (size_t)sp.n2, 1, sp.n2, sp.n2, 0, tw, (int)len, s);
}

// Inverse column transform (unnormalised) of spec_d * mul_d (point by point; mul_d may be NULL) into out_d (may equal
// spec_d when mul_d is NULL), all [len][pitch] in the permuted order; only the first keep_rows rows of the result are
// written (keep_rows = len or len / 2), in natural order.
extern "C" int ast_lens_cols_inverse(const void* spec, const void* mul, void* out, size_t len, size_t pitch, size_t ncols,
                                     size_t keep_rows, void* stream) {
    AST_CHECK_ARG(spec != nullptr && out != nullptr && ncols >= 1 && ncols <= pitch);
    AST_CHECK_ARG(mul == nullptr || (mul != out && spec != out));
    Split sp;
    AST_CHECK_ARG(split_of(len, sp));
    AST_CHECK_ARG(keep_rows == len || keep_rows == len / 2);
    hipStream_t s = ast::as_stream(stream);
    const double2* tw = twiddles64((int)len, s);
    if (!tw) { ast::set_error("ast_lens_cols_inverse: twiddle table allocation failed"); return AST_ERR_HIP; }
    AST_PROF("lens.cols_inv", s);
    double2* o = (double2*)out;
    // pass B backwards: group = k1, points k2 at consecutive rows -> n2, times conj W_L^{k1 n2}
    int rc = pass_of<true>(sp.n2, (const double2*)spec, (const double2*)mul, o, pitch, (int)ncols, sp.n1, (size_t)sp.n2, 1, sp.n2,
                           sp.n2, 1, tw, (int)len, s);
    if (rc != AST_OK) return rc;
    // pass A backwards: group = n2, points k1 at rows N2 apart -> n1; rows >= len / 2 are points n1 >= N1 / 2
    return pass_of<true>(sp.n1, o, nullptr, o, pitch, (int)ncols, sp.n2, 1, (size_t)sp.n2, sp.n1,
                         keep_rows == len ? sp.n1 : sp.n1 / 2, 0, tw, (int)len, s);
}

// out_m = the first keep_rows rows of IFFT_cols(FFT_cols(data) * mul_m) (unnormalised, natural order), m < nmul <= 2:
// forward pass A in place on data_d, then ONE pass that finishes the forward transform, forms the products and starts
// the inverses (col_mid_kernel: the spectrum is never written), then pass A backwards on each out_m.  mul_m are spectra
// in the permuted order ast_lens_cols_forward leaves.
extern "C" int ast_lens_cols_convolve(void* data, size_t len, size_t pitch, size_t ncols, size_t nonzero_rows,
                                      const void* const* muls, void* const* outs, int nmul, size_t keep_rows, void* stream) {
    AST_CHECK_ARG(data != nullptr && muls != nullptr && outs != nullptr && ncols >= 1 && ncols <= pitch);
    AST_CHECK_ARG(nmul == 1 || nmul == 2);
    AST_CHECK_ARG(pitch < ((size_t)1 << 24));             // col_mid_kernel: 16 rows of lane offset in 32-bit BYTES
    for (int i = 0; i < nmul; ++i) AST_CHECK_ARG(muls[i] != nullptr && outs[i] != nullptr && outs[i] != data && outs[i] != muls[i]);
    AST_CHECK_ARG(nmul == 1 || outs[0] != outs[1]);
    Split sp;
    AST_CHECK_ARG(split_of(len, sp));
    AST_CHECK_ARG(nonzero_rows == len || nonzero_rows == len / 2);
    AST_CHECK_ARG(keep_rows == len || keep_rows == len / 2);
    hipStream_t s = ast::as_stream(stream);
    const double2* tw = twiddles64((int)len, s);
    if (!tw) { ast::set_error("ast_lens_cols_convolve: twiddle table allocation failed"); return AST_ERR_HIP; }
    double2* d = (double2*)data;
    {
        AST_PROF("lens.cols_fwd", s);
        LENS_FWD(pass_of<false>(sp.n1, d, nullptr, d, pitch, (int)ncols, sp.n2, 1, (size_t)sp.n2,
                               nonzero_rows == len ? sp.n1 : sp.n1 / 2, sp.n1, 1, tw, (int)len, s));
    }
    {
        AST_PROF("lens.cols_mid", s);
        const double2* const* m = (const double2* const*)muls;
        double2* const* o = (double2* const*)outs;
        LENS_FWD(nmul == 2 ? mid_of<2>(sp.n2, d, m, o, pitch, (int)ncols, sp.n1, tw, (int)len, s)
                          : mid_of<1>(sp.n2, d, m, o, pitch, (int)ncols, sp.n1, tw, (int)len, s));
    }
    AST_PROF("lens.cols_inv", s);
    for (int i = 0; i < nmul; ++i) {
        double2* o = (double2*)outs[i];
        LENS_FWD(pass_of<true>(sp.n1, o, nullptr, o, pitch, (int)ncols, sp.n2, 1, (size_t)sp.n2, sp.n1,
                              keep_rows == len ? sp.n1 : sp.n1 / 2, 0, tw, (int)len, s));
    }
    return AST_OK;
}

extern "C" int ast_lens_rows_supported(size_t nc) {
    return nc == 8192 || nc == 4096 || nc == 2048 || nc == 1024 || nc == 512 || nc == 256 || nc == 128;
}

namespace {
constexpr unsigned LENS_ROW_SIZES = radix_sizes(128, 8192);      // what ast_lens_rows_supported accepts (8192: the reference's npix default, sky_array.py:266)
template <int RA, int RB, int RC>
int rows_inverse_launch(const double2* spec, size_t pitch, size_t nc, double scale, double* out, const double2* twM, const double2* twL,
                        hipStream_t s) {
    using G = RowGeo<RA, RB, RC>;
    const size_t lds = (size_t)(G::M + G::M / 8) * sizeof(double2);
    static ast::PerDeviceOnce once;
    if (once.need() && lds > 48 * 1024) {
        AST_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&lens_rows_inverse_kernel<RA, RB, RC>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        once.mark();
    }
    lens_rows_inverse_kernel<RA, RB, RC><<<(unsigned)nc, G::NT, lds, s>>>(spec, pitch, (int)nc, scale, out, twM, twL);
    AST_CHECK_LAUNCH();
    return AST_OK;
}
}  // namespace

// spec_d[r][0 .. nc] (row pitch `pitch` complex) = R2C of length 2 nc of (kappa_d[r][0 .. nc), nc zeros), r < nc.
extern "C" int ast_lens_rows_forward(const double* kappa, size_t nc, void* spec, size_t pitch, void* stream) {
    AST_CHECK_ARG(kappa != nullptr && spec != nullptr && ast_lens_rows_supported(nc) && pitch >= nc + 1);
    AST_CHECK_ARG(((uintptr_t)kappa & 15) == 0);
    hipStream_t s = ast::as_stream(stream);
    const double2* twM = twiddles64((int)nc, s);
    const double2* twL = twiddles64((int)(2 * nc), s);
    if (!twM || !twL) { ast::set_error("ast_lens_rows_forward: twiddle table allocation failed"); return AST_ERR_HIP; }
    AST_PROF("lens.rows_fwd", s);
    double2* o = (double2*)spec;
    return with_radices<LENS_ROW_SIZES>(nc, [&](auto ra, auto rb, auto rc) {
        return rows_forward_launch<ra.value, rb.value, rc.value>(kappa, nc, o, pitch, twM, twL, s);
    });
}

// spec_d[r][0 .. nc] = R2C of length 2 nc of the FULL row in_d[r][0 .. 2 nc) (no zero padding), r < nrows: the rows of the
// convolution kernels (lensing_funcs.c:45-83 fills all of the padded array), so that a plan needs no rocFFT at all.
extern "C" int ast_lens_rows_forward_full(const double* in, size_t nc, size_t nrows, void* spec, size_t pitch, void* stream) {
    AST_CHECK_ARG(in != nullptr && spec != nullptr && ast_lens_rows_supported(nc) && pitch >= nc + 1 && nrows >= 1);
    AST_CHECK_ARG(((uintptr_t)in & 15) == 0);
    hipStream_t s = ast::as_stream(stream);
    const double2* twM = twiddles64((int)nc, s);
    const double2* twL = twiddles64((int)(2 * nc), s);
    if (!twM || !twL) { ast::set_error("ast_lens_rows_forward_full: twiddle table allocation failed"); return AST_ERR_HIP; }
    AST_PROF("lens.rows_fwd", s);
    double2* o = (double2*)spec;
    return with_radices<LENS_ROW_SIZES>(nc, [&](auto ra, auto rb, auto rc) {
        return rows_forward_launch<ra.value, rb.value, rc.value, false>(in, nrows, o, pitch, twM, twL, s, 2 * nc);
    });
}

// out_d[r][0 .. nc) = scale * (the first nc reals of the length-2nc C2R of spec_d[r][0 .. nc]), r < nc (unnormalised C2R).
extern "C" int ast_lens_rows_inverse(const void* spec, size_t pitch, size_t nc, double scale, double* out, void* stream) {
    AST_CHECK_ARG(spec != nullptr && out != nullptr && ast_lens_rows_supported(nc) && pitch >= nc + 1);
    AST_CHECK_ARG(((uintptr_t)out & 15) == 0);
    hipStream_t s = ast::as_stream(stream);
    const double2* twM = twiddles64((int)nc, s);
    const double2* twL = twiddles64((int)(2 * nc), s);
    if (!twM || !twL) { ast::set_error("ast_lens_rows_inverse: twiddle table allocation failed"); return AST_ERR_HIP; }
    AST_PROF("lens.rows_inv", s);
    const double2* x = (const double2*)spec;
    return with_radices<LENS_ROW_SIZES>(nc, [&](auto ra, auto rb, auto rc) {
        return rows_inverse_launch<ra.value, rb.value, rc.value>(x, pitch, nc, scale, out, twM, twL, s);
    });
}

