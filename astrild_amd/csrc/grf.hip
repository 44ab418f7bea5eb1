// Gaussian random fields on the flat sky: the half-plane spectrum of a real n x n map with a given angular power
// spectrum C(l), ready for the C2R transform (lensing.gaussian_random_map; SkyArray.create_cmb / add_cmb,
// rays/skys/sky_array.py:709-777, whose NaMaster synfast_flat call is commented out in the reference).
//
// The value of a pixel is a pure function of (seed, realisation, pixel): a counter-based generator (Philox4x32-10,
// Salmon et al. 2011) keyed by the seed and counted by (pixel, realisation), Box-Muller in fp64 op by op.  The
// contract is spelled out at ast_grf_spectrum in include/astrild_hip.h and restated in numpy by tests/grf_oracle.py.
//
// A C2R transform reads the self-conjugate columns (j = 0, and j = n/2 for even n) as they are: row i and row n - i of
// such a column must be complex conjugates or the result is not the inverse transform of any spectrum.  A pixel in
// the lower half of such a column therefore draws from its partner's counter and negates the imaginary part: no
// thread reads what another wrote, there is no second pass and the result does not depend on the launch shape.
#include <cmath>
#include "ast_common.h"

namespace {

__device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                     uint32_t* w) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// One thread per pixel of the nreal stacked half planes, grid-strided over the flat index p = (R n + i) nh + j.  The
// host splits the stride (grid x 256, below 2^32) into (sR, si, sj) and (R, i, j) advance by carries: no division in
// the loop, and 32-bit ones for a thread's first pixel.
__global__ void __launch_bounds__(256)
grf_spectrum_kernel(double2* __restrict__ spec, int n, double dl, const double* __restrict__ cl, int ncl, double top,
                    double scale, uint32_t k0, uint32_t k1, unsigned long long first, int nreal, int sR, int si, int sj) {
    const int nh = n / 2 + 1;
    const bool even = (n & 1) == 0;
    const uint32_t p0 = blockIdx.x * blockDim.x + threadIdx.x, q0 = p0 / (uint32_t)nh;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t p = p0;
    int j = (int)(p0 % (uint32_t)nh), i = (int)(q0 % (uint32_t)n);
    long long R = (long long)(q0 / (uint32_t)n);
    for (; R < nreal; p += stride) {
        const int ip = i ? n - i : 0;                              // (n - i) mod n
        const long long m = min(i, n - i);
        const double l = dl * sqrt((double)(m * m + (long long)j * j));
        double A = 0.0;
        if (l <= top) {                                            // top <= ncl - 1: k and k + 1 (clamped) are inside
            const int k = (int)floor(l);
            const double t = l - (double)k, ck = cl[k];
            A = sqrt(ck + t * (cl[min(k + 1, ncl - 1)] - ck)) * scale;
        }
        double2 v = make_double2(0.0, 0.0);
        if (A != 0.0) {
            const bool selfc = j == 0 || (even && j == n / 2);
            const int ic = selfc ? min(i, ip) : i;
            const unsigned long long c = (unsigned long long)ic * (unsigned long long)nh + (unsigned long long)j;
            const unsigned long long real = first + (unsigned long long)R;
            uint32_t w[4];
            philox4x32_10((uint32_t)c, (uint32_t)(c >> 32), (uint32_t)real, (uint32_t)(real >> 32), k0, k1, w);
            const unsigned long long x = ((unsigned long long)(w[0] >> 5) << 26) + (w[1] >> 6);
            const unsigned long long y = ((unsigned long long)(w[2] >> 5) << 26) + (w[3] >> 6);
            const double u1 = ((double)x + 1.0) * 0x1p-53, u2 = (double)y * 0x1p-53;      // (0, 1] and [0, 1), exact
            const double r = sqrt(-2.0 * log(u1)), phi = (2.0 * M_PI) * u2;
            double sn, cs;
            sincos(phi, &sn, &cs);
            const double a = r * cs, b = r * sn;
            if (selfc && i == ip) {
                v.x = A * a;                                       // its own conjugate: real, full variance
            } else {
                v.x = A * a / M_SQRT2;
                v.y = A * b / M_SQRT2;
                if (selfc && i > ip) v.y = -v.y;
            }
        }
        spec[p] = v;
        j += sj;
        const int cj = j >= nh;
        j -= cj ? nh : 0;
        i += si + cj;
        const int ci = i >= n;
        i -= ci ? n : 0;
        R += sR + ci;
    }
}

}  // namespace

extern "C" int ast_grf_spectrum(void* spec, int npix, double angle_rad, const double* cl_d, int ncl, double lmax,
                                unsigned long long seed, unsigned long long first_realisation, int nreal, void* stream) {
    AST_CHECK_ARG(spec && cl_d && npix >= 2 && angle_rad > 0.0 && std::isfinite(angle_rad));
    AST_CHECK_ARG(ncl >= 1 && nreal >= 1 && lmax == lmax);
    hipStream_t s = ast::as_stream(stream);
    AST_PROF("grf_spectrum", s);
    const size_t total = (size_t)nreal * (size_t)npix * (size_t)(npix / 2 + 1);
    const double top = fmin(lmax, (double)(ncl - 1));
    const double scale = ((double)npix * (double)npix) / angle_rad;
    const unsigned grid = ast::stream_grid(total, 256);
    const size_t nh = (size_t)(npix / 2 + 1), stride = (size_t)grid * 256;
    grf_spectrum_kernel<<<grid, 256, 0, s>>>((double2*)spec, npix, 2.0 * M_PI / angle_rad, cl_d, ncl, top, scale,
                                            (uint32_t)seed, (uint32_t)(seed >> 32), first_realisation, nreal,
                                            (int)(stride / nh / (size_t)npix), (int)(stride / nh % (size_t)npix),
                                            (int)(stride % nh));
    AST_CHECK_LAUNCH();
    return AST_OK;
}
