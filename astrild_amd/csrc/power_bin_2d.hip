// FFTPower(mode="2d") of the half spectrum: (k, mu) wedges and Legendre multipoles P_l(k) about a line of sight
// along a box axis, plus the redshift-space position shift that feeds it.  nbodykit's published semantics
// (FFTPower: mode="2d", Nmu, los, poles; nbodykit is un-vendored), restated:
//
//   lattice, k shell, dropped modes (DC, |m| >= nmesh/2), Hermitian weight w and the `binning` switch: exactly those
//       of ast_power_bin_1d (power_bin.hip); AST_BIN_INTEGER / AST_BIN_FLOAT64 touch the k shell only.
//   mu = |m_los| / |m|, folded onto [0, 1] (valid for auto spectra and the real part of cross spectra).
//   mu bins: nmu uniform bins on [0, 1], left-closed, mu = 1 in the last one.  Membership in exact integer arithmetic:
//       j = min(nmu - 1, max{ j : j^2 |m|^2 <= nmu^2 m_los^2 })   (int64: nmu <= 1024, nmesh <= 8192).
//       Vectors with mu exactly on an edge exist (3-4-5 triples: mu = 3/5, 4/5 at nmu = 5) and open the bin they sit
//       on.  nbodykit digitizes a float64 mu: only such on-edge vectors could land differently there (parity unpinned).
//   wedges (nb, nmu): sum w |k|, sum w mu, sum w Re(d1 conj(d2)) L^3, sum w.
//   poles (npoles, nb): sum over ALL modes of the 1-D shell of w Re(d1 conj(d2)) L^3 L_l(mu), mu = m_los / sqrt(|m|^2)
//       in double, L_l from the three-term recurrence; the caller multiplies by (2l + 1) and divides by sum w.
//
// Layout as in power_bin.hip: one wave walks one (i0, i1) row with its 64 lanes along the contiguous half axis
// (coalesced 8/16-byte loads); products and sums in double; lanes add into the workgroup's LDS tables (wedge table
// (nb+2) x nmu, pole table npoles x (nb+2)), flushed to HBM once per workgroup.  The row part of the mu decision
// (m0^2 + m1^2, and m_los when the line of sight is not the half axis) is hoisted out of the lane loop.  The bin comes
// without an integer division: mu in double is needed for the Legendre terms anyway, floor(mu nmu) is within one of
// the answer and two exact int64 comparisons repair it.  Tables beyond the LDS budget (large nmu or nmesh) take a
// second variant of the same kernel that adds into the global tables with fp64 atomics.
#include "ast_common.h"
#include <cstdlib>

namespace {

__device__ inline int freq2(int i, int n) { return i > n / 2 ? i - n : i; }

__device__ inline int isqrt2_i(long long v) {
    // |m|^2 <= 3 * 4096^2 < 2^26: the float sqrt is within 1 of the integer root
    int r = (int)__fsqrt_rn((float)v);
    if ((long long)r * r > v) --r;
    if ((long long)(r + 1) * (r + 1) <= v) ++r;
    return r;
}

constexpr int P2_MAX_SHELLS = 4096;            // nmesh <= 8192
constexpr int P2_MAX_NMU = 1024;
constexpr int P2_MAX_POLES = 5;                // l in {0, 2, 4, 6, 8}
constexpr size_t P2_LDS_BUDGET = 160 * 1024;   // a CU's LDS
constexpr unsigned P2_GRID = 2048;             // 256 CUs x 8 workgroups, grid-stride over the rows

// slot[e]: row of the pole table that holds l = 2 e, or -1; lmax: the largest requested l (-1: none)
struct P2Poles {
    int slot[P2_MAX_POLES];
    int lmax;
};

// the data pass's table in doubles: (nb + 2) rows of the wedge table and of every pole
inline size_t data_table(int nmesh, int nmu, int npoles) { return (size_t)(nmesh / 2 + 1) * (size_t)(nmu + npoles); }
inline bool data_fits(int nmesh, int nmu, int npoles) { return data_table(nmesh, nmu, npoles) * sizeof(double) <= P2_LDS_BUDGET; }
// the geometry pass: sum w|k|, sum w mu (double) and sum w (uint64) per (shell, mu bin)
inline size_t geom_table(int nmesh, int nmu) { return (size_t)(nmesh / 2 + 1) * (size_t)nmu * 3; }
inline bool geom_fits(int nmesh, int nmu) { return geom_table(nmesh, nmu) * sizeof(double) <= P2_LDS_BUDGET; }

// mu bin of a mode: the largest j with j^2 m2 <= nmu^2 a^2, capped at nmu - 1.  mu = a / sqrt(m2) (double) gives the
// estimate; the exact comparisons decide.
__device__ inline int mu_bin(double mu, long long m2, long long a2n, int nmu) {
    int j = (int)(mu * (double)nmu);
    while (j > 0 && (long long)j * j * m2 > a2n) --j;
    while ((long long)(j + 1) * (j + 1) * m2 <= a2n) ++j;      // ends at j = nmu at the latest (a2n <= nmu^2 m2)
    return j < nmu ? j : nmu - 1;
}

// What both passes need of a mode, decided in ONE place so that the data pass and the geometry pass agree bit for bit.
// The row part: the integer frequencies of the first two axes and |m_los| when the line of sight is one of them.
struct P2Row {
    int m0, m1, a_row;
    long long base;                                         // m0^2 + m1^2
};
__device__ inline P2Row p2_row(long long row, int n, int i0_start, int i1_start, int i1_count, int los) {
    P2Row r;
    r.m0 = freq2(i0_start + (int)(row / i1_count), n);
    r.m1 = freq2(i1_start + (int)(row % i1_count), n);
    r.base = (long long)r.m0 * r.m0 + (long long)r.m1 * r.m1;
    r.a_row = los == 0 ? abs(r.m0) : abs(r.m1);             // los = 2: the lane's iz instead
    return r;
}
// The mode iz of the row: false when FFTPower drops it (DC, |m| >= nmesh/2); else sh (shell = sh - 1), the mu bin j,
// |m| and mu = |m_los| / |m| in double.
struct P2Mode {
    int sh, j;
    double norm, mu;
};
__device__ inline bool p2_mode(const P2Row& r, int iz, int nb, int los, int nmu, double kf_rule, P2Mode& m) {
    const long long m2 = r.base + (long long)iz * iz;
    int sh = isqrt2_i(m2);                                  // sh == 0 is the DC mode
    if (kf_rule != 0.0 && (long long)sh * sh == m2 && sh > 0) sh = ast::float64_edge_norm(sh, r.m0, r.m1, iz, kf_rule);
    if (sh < 1 || sh > nb) return false;
    const int al = los == 2 ? iz : r.a_row;
    m.sh = sh;
    m.norm = sqrt((double)m2);
    m.mu = (double)al / m.norm;
    m.j = mu_bin(m.mu, m2, (long long)nmu * nmu * al * al, nmu);
    return true;
}

template <typename C, bool LDS>
__global__ void __launch_bounds__(256)
power_bin_2d_kernel(const C* __restrict__ s1, const C* __restrict__ s2, int n, double pnorm, double kf_rule,
                    int i0_start, int i0_count, int i1_start, int i1_count, int los, int nmu, P2Poles pl, int npoles,
                    double* psum, double* polesum) {
    extern __shared__ double p2_lds[];
    const int nb = n / 2 - 1;
    double* lw = p2_lds;                                   // [nb + 2][nmu]
    double* lp = p2_lds + (size_t)(nb + 2) * nmu;          // [npoles][nb + 2]
    if (LDS) {
        const int cells = (nb + 2) * (nmu + npoles);
        for (int i = threadIdx.x; i < cells; i += blockDim.x) p2_lds[i] = 0.0;
        __syncthreads();
    }
    const int nz = n / 2 + 1;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int waves_per_block = blockDim.x >> 6;
    const long long nrows = (long long)i0_count * i1_count;
    for (long long row = (long long)blockIdx.x * waves_per_block + wave; row < nrows;
         row += (long long)gridDim.x * waves_per_block) {
        const P2Row rw = p2_row(row, n, i0_start, i1_start, i1_count, los);
        const C* r1 = s1 + (size_t)row * nz;
        const C* r2 = s2 ? s2 + (size_t)row * nz : nullptr;
        for (int iz = lane; iz < nz; iz += 64) {
            P2Mode md;
            if (!p2_mode(rw, iz, nb, los, nmu, kf_rule, md)) continue;
            const C x = r1[iz];
            const C y = r2 ? r2[iz] : x;
            const double w = (iz > 0 && iz < n / 2) ? 2.0 : 1.0;
            const double p = w * ((double)x.x * (double)y.x + (double)x.y * (double)y.y);
            const int sh = md.sh, j = md.j;
            const double mu = md.mu;
            if (LDS) atomicAdd(&lw[sh * nmu + j], p);
            else atomicAdd(&psum[(size_t)(sh - 1) * nmu + j], p * pnorm);
            // L_0 = 1, L_1 = mu, (l + 1) L_{l+1} = (2 l + 1) mu L_l - l L_{l-1}; the even ones are kept
            double lm = 1.0, lc = mu;                       // L_{l-1}, L_l at l = 1
#pragma unroll
            for (int e = 0; e < P2_MAX_POLES; ++e) {        // here lm = L_{2e}
                if (2 * e > pl.lmax) break;
                if (pl.slot[e] >= 0) {
                    if (LDS) atomicAdd(&lp[pl.slot[e] * (nb + 2) + sh], p * lm);
                    else atomicAdd(&polesum[(size_t)pl.slot[e] * nb + sh - 1], p * lm * pnorm);
                }
                const int l = 2 * e + 1;                    // two steps: (lm, lc) = (L_{l-1}, L_l) -> (L_{l+1}, L_{l+2})
                const double l1 = ((double)(2 * l + 1) * mu * lc - (double)l * lm) / (double)(l + 1);
                const double l2 = ((double)(2 * l + 3) * mu * l1 - (double)(l + 1) * lc) / (double)(l + 2);
                lm = l1;
                lc = l2;
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < nb * nmu; i += blockDim.x) {
            const double v = lw[nmu + i];                   // row sh = 1 is shell 0
            if (v != 0.0) atomicAdd(&psum[i], v * pnorm);
        }
        for (int i = threadIdx.x; i < npoles * nb; i += blockDim.x) {
            const int q = i / nb, s = i % nb;
            const double v = lp[q * (nb + 2) + s + 1];
            if (v != 0.0) atomicAdd(&polesum[i], v * pnorm);
        }
    }
}

// Geometry pass: sum w|k|, sum w mu and sum w per (shell, mu bin) depend only on the lattice block and the line of
// sight, not on the data; callers cache them.
template <bool LDS>
__global__ void __launch_bounds__(256)
wedge_geometry_kernel(int n, double kf, double kf_rule, int i0_start, int i0_count, int i1_start, int i1_count, int los,
                      int nmu, double* ksum, double* musum, unsigned long long* nmodes) {
    extern __shared__ double g2_lds[];
    const int nb = n / 2 - 1;
    const int cells = (nb + 2) * nmu;
    double* lk = g2_lds;
    double* lu = g2_lds + cells;
    unsigned long long* lm = reinterpret_cast<unsigned long long*>(g2_lds + 2 * (size_t)cells);
    if (LDS) {
        for (int i = threadIdx.x; i < cells; i += blockDim.x) { lk[i] = 0.0; lu[i] = 0.0; lm[i] = 0ull; }
        __syncthreads();
    }
    const int nz = n / 2 + 1;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int waves_per_block = blockDim.x >> 6;
    const long long nrows = (long long)i0_count * i1_count;
    for (long long row = (long long)blockIdx.x * waves_per_block + wave; row < nrows;
         row += (long long)gridDim.x * waves_per_block) {
        const P2Row rw = p2_row(row, n, i0_start, i1_start, i1_count, los);
        for (int iz = lane; iz < nz; iz += 64) {
            P2Mode md;
            if (!p2_mode(rw, iz, nb, los, nmu, kf_rule, md)) continue;
            const unsigned long long w = (iz > 0 && iz < n / 2) ? 2ull : 1ull;
            const int sh = md.sh, j = md.j;
            const double norm = md.norm, mu = md.mu;
            if (LDS) {
                atomicAdd(&lk[sh * nmu + j], (double)w * norm);
                atomicAdd(&lu[sh * nmu + j], (double)w * mu);
                atomicAdd(&lm[sh * nmu + j], w);
            } else {
                const size_t o = (size_t)(sh - 1) * nmu + j;
                atomicAdd(&ksum[o], (double)w * norm * kf);
                atomicAdd(&musum[o], (double)w * mu);
                atomicAdd(&nmodes[o], w);
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < nb * nmu; i += blockDim.x) {
            const unsigned long long m = lm[nmu + i];
            if (m) {
                atomicAdd(&ksum[i], lk[nmu + i] * kf);
                atomicAdd(&musum[i], lu[nmu + i]);
                atomicAdd(&nmodes[i], m);
            }
        }
    }
}

// s = pos; s[los] += factor * vel[los] in T, then ONE periodic wrap into [0, L): s >= L -> s - L, s < 0 -> s + L, and
// a sum that rounds up to L (float32 -1e-9 + 100 = 100) is 0.  A shift of more than a box length stays outside [0, L).
template <typename T>
__global__ void __launch_bounds__(256)
rsd_shift_kernel(const T* pos, const T* __restrict__ vel, size_t np, int los, T factor, double boxsize, T* out) {
    const T box = (T)boxsize;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < np; i += stride) {
        T p[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
        const T v = vel[3 * i + los];
        T s = (los == 0 ? p[0] : los == 1 ? p[1] : p[2]) + factor * v;
        if ((double)s >= boxsize) s -= box;
        else if (s < (T)0) {
            s += box;
            if ((double)s >= boxsize) s = (T)0;
        }
        if (los == 0) p[0] = s; else if (los == 1) p[1] = s; else p[2] = s;
        out[3 * i] = p[0];
        out[3 * i + 1] = p[1];
        out[3 * i + 2] = p[2];
    }
}

template <typename K>
int raise_lds_limit(K kernel) {
    AST_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)P2_LDS_BUDGET));
    return AST_OK;
}

}  // namespace

extern "C" int ast_power_bin_2d_lds_fits(int nmesh, int nmu, int npoles) {
    if (nmesh < 4 || nmesh % 2 || nmesh / 2 - 1 > P2_MAX_SHELLS || nmu < 1 || nmu > P2_MAX_NMU || npoles < 0 ||
        npoles > P2_MAX_POLES)
        return 0;
    return data_fits(nmesh, nmu, npoles) ? 1 : 0;
}

extern "C" int ast_power_bin_2d(const void* spec1, const void* spec2, int dtype, int nmesh, double boxsize,
                                int i0_start, int i0_count, int i1_start, int i1_count, int los, int nmu,
                                const int* poles, int npoles, double* ksum, double* musum, long long* nmodes,
                                double* psum, double* polesum, int binning, void* stream) {
    AST_CHECK_ARG((spec1 && psum) || (!spec1 && !spec2 && !psum && !polesum));
    AST_CHECK_ARG(binning == AST_BIN_INTEGER || binning == AST_BIN_FLOAT64);
    AST_CHECK_ARG((ksum == nullptr) == (nmodes == nullptr) && (ksum == nullptr) == (musum == nullptr));
    AST_CHECK_ARG(psum || ksum);
    AST_CHECK_ARG(dtype == AST_F32 || dtype == AST_F64);
    AST_CHECK_ARG(nmesh >= 4 && nmesh % 2 == 0 && nmesh / 2 - 1 <= P2_MAX_SHELLS && boxsize > 0.0);
    AST_CHECK_ARG(los >= 0 && los <= 2);
    AST_CHECK_ARG(nmu >= 1 && nmu <= P2_MAX_NMU);
    AST_CHECK_ARG(npoles >= 0 && npoles <= P2_MAX_POLES && (npoles == 0 || poles != nullptr));
    AST_CHECK_ARG(!psum || npoles == 0 || polesum != nullptr);
    AST_CHECK_ARG(i0_start >= 0 && i0_count >= 0 && i0_start + i0_count <= nmesh);
    AST_CHECK_ARG(i1_start >= 0 && i1_count >= 0 && i1_start + i1_count <= nmesh);
    P2Poles pl;
    for (int e = 0; e < P2_MAX_POLES; ++e) pl.slot[e] = -1;
    pl.lmax = -1;
    for (int q = 0; q < npoles; ++q) {
        const int l = poles[q];
        AST_CHECK_ARG(l >= 0 && l <= 2 * (P2_MAX_POLES - 1) && l % 2 == 0);     // even l only: the folded half spectrum
        AST_CHECK_ARG(pl.slot[l / 2] < 0);                                      // holds no odd multipole; no repeats
        pl.slot[l / 2] = q;
        if (l > pl.lmax) pl.lmax = l;
    }
    const long long nrows = (long long)i0_count * i1_count;
    if (nrows == 0) return AST_OK;
    const double kf = 2.0 * M_PI / boxsize;
    const double kf_rule = binning == AST_BIN_FLOAT64 ? kf : 0.0;
    const double pnorm = boxsize * boxsize * boxsize;
    const long long need = (nrows + 3) / 4;
    const unsigned g = (unsigned)(need > P2_GRID ? P2_GRID : need);
    hipStream_t s = ast::as_stream(stream);
    // ASTRILD_PK2D_LDS=0: the global-atomic variants also where the tables fit (A/B runs, tests)
    const char* env = getenv("ASTRILD_PK2D_LDS");
    const bool force_global = env && env[0] == '0';
    static ast::PerDeviceOnce attr_once;
    if (attr_once.need()) {
        if (int rc = raise_lds_limit(&power_bin_2d_kernel<float2, true>)) return rc;
        if (int rc = raise_lds_limit(&power_bin_2d_kernel<double2, true>)) return rc;
        if (int rc = raise_lds_limit(&wedge_geometry_kernel<true>)) return rc;
        attr_once.mark();
    }
    if (psum) {
        const bool use_lds = !force_global && data_fits(nmesh, nmu, npoles);
        const size_t lds = use_lds ? data_table(nmesh, nmu, npoles) * sizeof(double) : 0;
        AST_PROF(use_lds ? "power_bin_2d" : "power_bin_2d_global", s);
#define P2_LAUNCH(C, L)                                                                                                  \
    power_bin_2d_kernel<C, L><<<g, 256, lds, s>>>((const C*)spec1, (const C*)spec2, nmesh, pnorm, kf_rule, i0_start,    \
                                                  i0_count, i1_start, i1_count, los, nmu, pl, npoles, psum, polesum)
        if (dtype == AST_F32) { if (use_lds) P2_LAUNCH(float2, true); else P2_LAUNCH(float2, false); }
        else { if (use_lds) P2_LAUNCH(double2, true); else P2_LAUNCH(double2, false); }
#undef P2_LAUNCH
    }
    if (ksum) {
        const bool use_lds = !force_global && geom_fits(nmesh, nmu);
        const size_t lds = use_lds ? geom_table(nmesh, nmu) * sizeof(double) : 0;
        AST_PROF(use_lds ? "wedge_geometry" : "wedge_geometry_global", s);
        if (use_lds)
            wedge_geometry_kernel<true><<<g, 256, lds, s>>>(nmesh, kf, kf_rule, i0_start, i0_count, i1_start, i1_count, los, nmu,
                                                            ksum, musum, reinterpret_cast<unsigned long long*>(nmodes));
        else
            wedge_geometry_kernel<false><<<g, 256, lds, s>>>(nmesh, kf, kf_rule, i0_start, i0_count, i1_start, i1_count, los, nmu,
                                                             ksum, musum, reinterpret_cast<unsigned long long*>(nmodes));
    }
    AST_CHECK_LAUNCH();
    return AST_OK;
}

extern "C" int ast_rsd_shift(const void* pos, const void* vel, int dtype, size_t np, int los, double factor,
                             double boxsize, void* out, void* stream) {
    AST_CHECK_ARG(dtype == AST_F32 || dtype == AST_F64);
    AST_CHECK_ARG(los >= 0 && los <= 2 && boxsize > 0.0);
    if (np == 0) return AST_OK;
    AST_CHECK_ARG(pos && vel && out);
    hipStream_t s = ast::as_stream(stream);
    AST_PROF("rsd_shift", s);
    const unsigned g = ast::stream_grid(np, 256);
    if (dtype == AST_F32)
        rsd_shift_kernel<float><<<g, 256, 0, s>>>((const float*)pos, (const float*)vel, np, los, (float)factor, boxsize, (float*)out);
    else
        rsd_shift_kernel<double><<<g, 256, 0, s>>>((const double*)pos, (const double*)vel, np, los, factor, boxsize, (double*)out);
    AST_CHECK_LAUNCH();
    return AST_OK;
}
