// What the two double-precision low-k side channels share: fft_tile.hip's (modes |m_i| <= MBOX = 6 beside the fp32 tile
// passes) and cube_fft.hip's (|m_i| <= BIGBOX = 17 beside the fp32 passes of side 2048).  Their z, y and shell kernels differ
// in summation scheme and stay in their files; the direct sum over one axis and the sum of the parts are the same code.
#pragma once
#include "ast_common.h"

namespace {

// One axis of the low-k transform: in[(outer * nt + t) * inner + i], t < nt, is summed with e^{-2 pi i k (t0 + t) / n} for
// k = -BOX..BOX.  Block (outer, part) adds up the t of part `part` (of gridDim.y), four independent accumulators so
// that several loads are in flight, and writes out[((outer * nparts + part) * (2 BOX + 1) + k + BOX) * inner + i].
// BOX = 6, y pass: outer = x plane, inner = BOX + 1, one part.  x pass (either box): outer = 1, inner = (2 BOX + 1)(BOX + 1),
// several parts, then lowk_parts_reduce_kernel adds the parts in order.
template <int BOX>
__global__ void __launch_bounds__(256)
lowk_axis_kernel(const double2* __restrict__ in, int n, int nt, int t0, int inner, double2* __restrict__ out) {
    extern __shared__ double2 tw[];                       // e^{-2 pi i t / n}
    for (int t = threadIdx.x; t < n; t += 256) {
        double sn, cs;
        sincospi(-2.0 * (double)t / (double)n, &sn, &cs);
        tw[t] = make_double2(cs, sn);
    }
    __syncthreads();
    const size_t outer = blockIdx.x;
    const int nparts = gridDim.y, part = blockIdx.y;
    const int per = (nt + nparts - 1) / nparts, ta = part * per, tb = min(nt, ta + per);
    const int nout = (2 * BOX + 1) * inner;
    if (nout <= 128) {
        // few outputs (the y pass: 91): 256 / nout thread groups share the t range, interleaved, and their partial
        // sums are added in group order
        __shared__ double2 part_sum[256];
        const int groups = 256 / nout, o = threadIdx.x % nout, gq = threadIdx.x / nout;
        double re = 0.0, im = 0.0, re2 = 0.0, im2 = 0.0;
        if (gq < groups) {
            const int k = o / inner - BOX, i = o % inner;
            int t = ta + gq;
            for (; t + groups < tb; t += 2 * groups) {           // two loads in flight
                const double2 v = in[(outer * nt + t) * inner + i], v2 = in[(outer * nt + t + groups) * inner + i];
                const double2 w = tw[(unsigned)(k * (t0 + t)) & (unsigned)(n - 1)];
                const double2 w2 = tw[(unsigned)(k * (t0 + t + groups)) & (unsigned)(n - 1)];
                re += v.x * w.x - v.y * w.y;
                im += v.x * w.y + v.y * w.x;
                re2 += v2.x * w2.x - v2.y * w2.y;
                im2 += v2.x * w2.y + v2.y * w2.x;
            }
            if (t < tb) {
                const double2 v = in[(outer * nt + t) * inner + i];
                const double2 w = tw[(unsigned)(k * (t0 + t)) & (unsigned)(n - 1)];
                re += v.x * w.x - v.y * w.y;
                im += v.x * w.y + v.y * w.x;
            }
        }
        part_sum[threadIdx.x] = make_double2(re + re2, im + im2);
        __syncthreads();
        if (gq == 0) {
            double sr = 0.0, si = 0.0;
            for (int q = 0; q < groups; ++q) { sr += part_sum[q * nout + o].x; si += part_sum[q * nout + o].y; }
            const int k = o / inner - BOX, i = o % inner;
            out[((outer * nparts + part) * (2 * BOX + 1) + k + BOX) * inner + i] = make_double2(sr, si);
        }
        return;
    }
    for (int o = threadIdx.x; o < nout; o += 256) {
        const int k = o / inner - BOX, i = o % inner;
        double re[4] = {0.0, 0.0, 0.0, 0.0}, im[4] = {0.0, 0.0, 0.0, 0.0};
        for (int tq = ta; tq < tb; tq += 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int t = min(tq + q, tb - 1);        // unconditional load; the duplicate is not added
                const double2 v = in[(outer * nt + t) * inner + i];
                const double2 w = tw[(unsigned)(k * (t0 + t)) & (unsigned)(n - 1)];       // n is a power of two
                if (tq + q < tb) {
                    re[q] += v.x * w.x - v.y * w.y;
                    im[q] += v.x * w.y + v.y * w.x;
                }
            }
        }
        out[((outer * nparts + part) * (2 * BOX + 1) + k + BOX) * inner + i] =
            make_double2((re[0] + re[1]) + (re[2] + re[3]), (im[0] + im[1]) + (im[2] + im[3]));
    }
}

// acc[i] (+)= sum over parts of in[part * count + i], parts in index order
__global__ void __launch_bounds__(256)
lowk_parts_reduce_kernel(const double2* __restrict__ in, int nparts, int count, int accumulate, double2* __restrict__ acc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double re = accumulate ? acc[i].x : 0.0, im = accumulate ? acc[i].y : 0.0;
    for (int p = 0; p < nparts; ++p) {
        re += in[(size_t)p * count + i].x;
        im += in[(size_t)p * count + i].y;
    }
    acc[i] = make_double2(re, im);
}

}  // namespace
