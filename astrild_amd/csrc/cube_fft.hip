// Hand-written 3-D transforms of cubes that fft_tile.hip's fp32 tile passes do not cover, both in the three-stage scheme of
// fft_three_stage.h: float64 grids (ast_fft64_*), and fp32 grids of side 2048 with their 16-shell double-precision low-k
// box (ast_fft32_big_*, second half of the file; it reuses the first half's shell reduction).
#include "fft_three_stage.h"
#include "lowk_sums.h"

// ------------------------------------------------------------------ 3-D power spectrum of a double-precision grid
// FFTPower of an in-memory grid in the reference's own dtype (power_spectrum_3d.py:183-224 on float64 arrays): z rows by
// the row kernel of fft_three_stage.h (no zero padding), y and x passes by col3_kernel - the three-stage scheme with the transform axis
// strided: a workgroup takes 4 or 8 adjacent k_z columns (64- or 128-byte row pieces) of all N = RA RB RC rows, one LDS
// line per column, ONE pass per axis where rocFFT's 3-D plan moves 2.1x the bytes.
// The x pass does not store: it adds w |delta_k|^2 of its modes to the workgroup's LDS shell table (integer rule or
// nbodykit's float64 edge rule, ast_common.h), written out as a row of `partial` and reduced in a fixed order.
template <int RA, int RB, int RC, int C, bool POWER>
__global__ void __launch_bounds__((C * RowGeo<RA, RB, RC>::NT))
col3_kernel(double2* __restrict__ data, const double2* __restrict__ twM, size_t elem_stride, size_t ncols, size_t batch_stride,
            unsigned tiles_per_batch, double scale, double* __restrict__ partial, double kf_rule, int prune2 = 0) {
    using G = RowGeo<RA, RB, RC>;
    constexpr int N = G::M, NB = N / 2 - 1, LINE = N + N / 8;
    extern __shared__ double2 lds64[];
    double* shell = reinterpret_cast<double*>(lds64 + C * LINE);          // [NB + 1] when POWER
    const int c = threadIdx.x % C, t = threadIdx.x / C;
    // C * 16 B < 128 B (N = 1024: four columns): a workgroup touches HALF of every 128-byte line, the workgroup of the next
    // tile the other half.  Workgroups go to the 8 XCDs round robin, so those two ran behind different L2s and every line
    // crossed HBM twice (x pass: 8.6 GB read in 3.3 ms = 2.6 TB/s apparent).  So consecutive tiles are mapped to consecutive
    // launch slots of ONE XCD, and the second one finds the line in that L2.  (All tiles of a batch row on one XCD, as
    // fft_tile.hip's strided passes do for arrays of the natural pitch, measured the same here: the pitch of the power
    // pipeline's scratch spectrum is a whole number of lines, only the two halves of a line are shared.)
    unsigned bid = blockIdx.x;
    const size_t row_pitch = elem_stride < batch_stride ? elem_stride : batch_stride;
    if ((row_pitch & 7) != 0 && (gridDim.x / tiles_per_batch) % 8u == 0u) {
        // rows that are NOT a whole number of lines (ast_fft64_r2c_3d's contiguous n / 2 + 1): a tile's pieces straddle into
        // the lines of the tiles on either side, so all tiles of a batch row follow each other on one XCD (batch b on XCD
        // b mod 8), as in fft_tile.hip's strided passes
        const unsigned xcd = bid % 8, slot = bid / 8;
        bid = ((slot / tiles_per_batch) * 8 + xcd) * tiles_per_batch + slot % tiles_per_batch;
    } else if (C * sizeof(double2) < 128) {
        const unsigned full = gridDim.x / 16 * 16;
        if (bid < full) {
            const unsigned xcd = bid % 8, slot = bid / 8;
            bid = ((slot >> 1) * 8 + xcd) * 2 + (slot & 1);
        }
    }
    const unsigned tile = bid % tiles_per_batch, b = bid / tiles_per_batch;
    const size_t c0 = (size_t)tile * C;
    const bool col_ok = c0 + c < ncols;
    // FORWARD PRUNING (prune2 = (N/2)^2 on the power pipeline's two strided passes, as in fft_tile.hip): FFTPower keeps
    // |m| < N/2 (power_spectrum_3d.py:189-195; the edge itself stays for the float64 rule), so a row (k_y, tile from k_z0)
    // with k_y^2 + k_z0^2 > (N/2)^2 is not stored by the y pass and its tile is left out by the binning pass (its row of
    // `partial` is zeros) - 21.5 % of the half plane, with C = 4 or 8 columns cut close to the circle.
    if (POWER && prune2 > 0) {
        const int ky = (int)b > N / 2 ? (int)b - N : (int)b;
        if (ky * ky + (int)(c0 * c0) > prune2) {                            // block-uniform, before any barrier
            for (int i = threadIdx.x; i < NB; i += C * G::NT) partial[(size_t)bid * NB + i] = 0.0;
            return;
        }
    }
    double2* base = data + (size_t)b * batch_stride + min(c0 + c, ncols - 1);
    double2* Y = lds64 + c * LINE;
    if (POWER)
        for (int i = threadIdx.x; i <= NB; i += C * G::NT) shell[i] = 0.0;
    double2 va[RA], vc[RC];
    if (t < G::T1) {
#pragma unroll
        for (int a = 0; a < RA; ++a) va[a] = base[(size_t)(G::T1 * a + t) * elem_stride];
    }
    three_stage<RA, RB, RC>(va, vc, Y, twM, t);
    if (t < G::T3 && col_ok) {
        const int al = t / RB, be = t % RB;
        if (!POWER) {
            const int room = prune2 > 0 ? prune2 - (int)(c0 * c0) : 0x7fffffff;        // rows are k_y: keep k_y^2 <= room
#pragma unroll
            for (int ga = 0; ga < RC; ++ga) {
                double2 x = vc[bitrev(ga, ilog2(RC))];
                x.x *= scale;
                x.y *= scale;
                const int row = al + RA * be + RA * RB * ga, aky = RA * RB * ga >= N / 2 ? N - row : row;
                if (aky * aky <= room) base[(size_t)row * elem_stride] = x;
            }
        } else {
            const int kz = (int)(c0 + c);
            const int ky = (int)b > N / 2 ? (int)b - N : (int)b;
            const int m2yz = ky * ky + kz * kz;
            const double w = (kz > 0 && kz < N / 2) ? 2.0 : 1.0;
#pragma unroll
            for (int ga = 0; ga < RC; ++ga) {
                const double2 x = vc[bitrev(ga, ilog2(RC))];
                const int row = al + RA * be + RA * RB * ga;
                const int kx = row > N / 2 ? row - N : row;
                const int m2 = kx * kx + m2yz;
                // floor(sqrt(m2)) for 0 <= m2 <= 3 * 512^2 from one raw v_sqrt_f32 of m2 + 1/2 (exact: fft_tile.hip's
                // tile_isqrt, checked exhaustively by test_gpu_fft_tile) - a double square root plus two repair loops per
                // mode were a third of this pass
                int r = (int)__builtin_amdgcn_sqrtf((float)m2 + 0.5f);
                if (N > 1024) {                           // (beyond the range of the exhaustive check: one repair step either way)
                    if (r * r > m2) --r;
                    else if ((r + 1) * (r + 1) <= m2) ++r;
                }
                if (kf_rule != 0.0 && r > 0 && r * r == m2) r = ast::float64_edge_norm(r, kx, ky, kz, kf_rule);
                if (r >= 1 && r <= NB) atomicAdd(&shell[r], (x.x * x.x + x.y * x.y) * w);      // shell = r - 1
            }
        }
    }
    if (POWER) {
        __syncthreads();
        const double s2 = scale * scale;
        for (int i = threadIdx.x; i < NB; i += C * G::NT) partial[(size_t)bid * NB + i] = shell[i + 1] * s2;
    }
}

// psum[bin] += pnorm * sum over workgroups of partial[wg][bin], fixed order: REDUCE64 blocks each add a contiguous range
// of workgroup rows (lanes = consecutive bins), then one block adds those.
constexpr int REDUCE64 = 1024;
__global__ void __launch_bounds__(256)
power64_stage1_kernel(const double* __restrict__ partial, size_t nwg, int nb, double* __restrict__ out) {
    const size_t per = (nwg + REDUCE64 - 1) / REDUCE64;
    const size_t w0 = (size_t)blockIdx.x * per, w1 = w0 + per < nwg ? w0 + per : nwg;
    for (int i = threadIdx.x; i < nb; i += 256) {
        double acc = 0.0;
        for (size_t wg = w0; wg < w1; ++wg) acc += partial[wg * nb + i];
        out[(size_t)blockIdx.x * nb + i] = acc;
    }
}
__global__ void __launch_bounds__(256)
power64_stage2_kernel(const double* __restrict__ part, int nb, double pnorm, double* __restrict__ psum) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nb) return;
    double acc = 0.0;
    for (int r = 0; r < REDUCE64; ++r) acc += part[(size_t)r * nb + i];
    psum[i] += pnorm * acc;
}

namespace {
// columns per workgroup: 4 at N = 1024 (74 KB of LDS: two workgroups per CU; measured 4.5 + 4.0 ms for the y and x passes
// against 5.4 + 4.5 with 8 columns and one workgroup per CU, 7.3 + 5.8 with 2), 8 below
// (N = 2048: 4 columns = 147 KB, one 1024-thread workgroup per CU; N = 128: 8 columns, 18 KB)
constexpr int col3_columns(size_t n) { return n >= 1024 ? 4 : 8; }
constexpr unsigned FFT64_SIZES = radix_sizes(128, 2048);         // what ast_fft64_supported accepts
template <int RA, int RB, int RC, bool POWER>
int col3_launch(double2* data, const double2* tw, size_t elem_stride, size_t ncols, size_t batch, size_t batch_stride, double scale,
                double* partial, double kf_rule, hipStream_t s, int prune2 = 0) {
    using G = RowGeo<RA, RB, RC>;
    constexpr int C = col3_columns(G::M), LINE = G::M + G::M / 8;
    const size_t lds = (size_t)C * LINE * sizeof(double2) + (POWER ? (G::M / 2) * sizeof(double) : 0);
    static ast::PerDeviceOnce once;
    if (once.need()) {
        AST_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&col3_kernel<RA, RB, RC, C, POWER>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        once.mark();
    }
    const size_t tiles = (ncols + C - 1) / C;
    AST_CHECK_ARG(tiles * batch < 0x7fffffffull);
    col3_kernel<RA, RB, RC, C, POWER><<<(unsigned)(tiles * batch), C * G::NT, lds, s>>>(data, tw, elem_stride, ncols, batch_stride,
                                                                                        (unsigned)tiles, scale, partial, kf_rule, prune2);
    AST_CHECK_LAUNCH();
    return AST_OK;
}
template <bool POWER>
int col3_dispatch(size_t n, double2* data, const double2* tw, size_t elem_stride, size_t ncols, size_t batch, size_t batch_stride,
                  double scale, double* partial, double kf_rule, hipStream_t s, int prune2 = 0) {
    return with_radices<FFT64_SIZES>(n, [&](auto ra, auto rb, auto rc) {
        return col3_launch<ra.value, rb.value, rc.value, POWER>(data, tw, elem_stride, ncols, batch, batch_stride, scale, partial, kf_rule, s, prune2);
    });
}
// the z rows of an (n, n, n) grid: the half-length transform of n * n rows of n reals, FOLDW as in lens_rows_forward_kernel
template <int FOLDW, typename TIN>
int rows64_dispatch(size_t n, const TIN* grid, double2* spec, size_t pitch, const double2* twH, const double2* twN, hipStream_t s,
                    const double* rec = nullptr) {
    return with_radices<FFT64_SIZES / 2>(n / 2, [&](auto ra, auto rb, auto rc) {
        return rows_forward_launch<ra.value, rb.value, rc.value, false, FOLDW, TIN>(grid, n * n, spec, pitch, twH, twN, s, n, 1.0, rec);
    });
}
}  // namespace

// 128 (BASELINE config A's own size) ... 2048 (the largest cube whose float64 grid and scratch spectrum - 69 GB each - fit one
// MI355X; domain_level is arbitrary in the reference, power_spectrum_3d.py:183-188)
extern "C" int ast_fft64_supported(size_t n) { return n == 128 || n == 256 || n == 512 || n == 1024 || n == 2048; }

// row pitch of the scratch spectrum (complex): n / 2 + 1 rounded up to 8 (128-byte pieces stay line aligned)
static size_t fft64_pitch(size_t n) { return (n / 2 + 1 + 7) / 8 * 8; }
extern "C" size_t ast_fft64_power_scratch_bytes(size_t n) {
    const size_t nzp = fft64_pitch(n), cw = (size_t)col3_columns(n), tiles = (n / 2 + 1 + cw - 1) / cw, nb = n / 2 - 1;
    return n * n * nzp * sizeof(double2) + n * tiles * nb * sizeof(double) + (size_t)REDUCE64 * nb * sizeof(double);
}

// psum_d[shell] += L^3 sum over the shell's modes of w |delta_k|^2, delta_k = rfftn(grid) / n^3, for an (n, n, n) double
// grid: FFTPower(ArrayMesh(grid), mode="1d", kmin = k_F)'s shell sums (power_spectrum_3d.py:183-224) without the
// spectrum's last pass ever reaching HBM.  grid_d is not modified.
static int fft64_power_impl(const double* grid, const double* rec, int window, void* scratch, size_t scratch_bytes, size_t n,
                            double boxsize, int binning, double* psum, void* stream, const float* grid32 = nullptr);
extern "C" int ast_fft64_power_3d(const double* grid, void* scratch, size_t scratch_bytes, size_t n, double boxsize, int binning,
                                  double* psum, void* stream) {
    return fft64_power_impl(grid, nullptr, 0, scratch, scratch_bytes, n, boxsize, binning, psum, stream);
}
// The same for a SINGLE-precision grid, transformed in double (widened as the z pass loads the rows): the route of fp32 cubes
// the fp32 tile passes do not cover (128^3, 2048^3) - instead of a float64 copy of the grid in front of the passes.
extern "C" int ast_fft64_power_3d_f32(const float* grid, void* scratch, size_t scratch_bytes, size_t n, double boxsize, int binning,
                                      double* psum, void* stream) {
    AST_CHECK_ARG(grid != nullptr);
    return fft64_power_impl(nullptr, nullptr, 0, scratch, scratch_bytes, n, boxsize, binning, psum, stream, grid);
}
// The same for a grid painted with AST_PAINT_OVERWRITE | AST_PAINT_DEFER_FOLD: halo_rec_d (ast_paint_tiled_halo) is folded
// into the border rows as the z pass loads them.
extern "C" int ast_fft64_power_3d_halo(const double* grid, const double* halo_rec, int window, void* scratch, size_t scratch_bytes,
                                       size_t n, double boxsize, int binning, double* psum, void* stream) {
    AST_CHECK_ARG(halo_rec != nullptr && (window == AST_WIN_CIC || window == AST_WIN_TSC));
    return fft64_power_impl(grid, halo_rec, window, scratch, scratch_bytes, n, boxsize, binning, psum, stream);
}
static int fft64_power_impl(const double* grid, const double* rec, int window, void* scratch, size_t scratch_bytes, size_t n,
                            double boxsize, int binning, double* psum, void* stream, const float* grid32) {
    AST_CHECK_ARG((grid != nullptr || grid32 != nullptr) && scratch != nullptr && psum != nullptr && boxsize > 0.0);
    AST_CHECK_ARG(ast_fft64_supported(n) && scratch_bytes >= ast_fft64_power_scratch_bytes(n));
    AST_CHECK_ARG(binning == AST_BIN_INTEGER || binning == AST_BIN_FLOAT64);
    AST_CHECK_ARG(((uintptr_t)grid & 15) == 0 && ((uintptr_t)grid32 & 7) == 0 && (grid32 == nullptr || rec == nullptr));
    hipStream_t s = ast::as_stream(stream);
    const size_t nz = n / 2 + 1, nzp = fft64_pitch(n), cw = (size_t)col3_columns(n), tiles = (nz + cw - 1) / cw, nb = n / 2 - 1;
    double2* spec = (double2*)scratch;
    double* partial = (double*)((char*)scratch + n * n * nzp * sizeof(double2));
    double* part2 = partial + n * tiles * nb;
    const double2* twH = twiddles64((int)(n / 2), s);       // the rows' half-length transform
    const double2* twN = twiddles64((int)n, s);
    if (!twH || !twN) { ast::set_error("ast_fft64_power_3d: twiddle table allocation failed"); return AST_ERR_HIP; }
    const int prune2 = getenv("AST_FFT_NO_PRUNE") ? 0 : (int)((n / 2) * (n / 2));      // what FFTPower drops is neither stored nor binned
    int rc;
    {
        AST_PROF("fft64.rows_r2c", s);
        if (grid32 != nullptr) rc = rows64_dispatch<0>(n, grid32, spec, nzp, twH, twN, s);
        else if (rec == nullptr) rc = rows64_dispatch<0>(n, grid, spec, nzp, twH, twN, s);
        else if (window == AST_WIN_CIC) rc = rows64_dispatch<2>(n, grid, spec, nzp, twH, twN, s, rec);
        else rc = rows64_dispatch<3>(n, grid, spec, nzp, twH, twN, s, rec);
        if (rc != AST_OK) return rc;
    }
    {
        AST_PROF("fft64.cols", s);
        rc = col3_dispatch<false>(n, spec, twN, nzp, nz, n, n * nzp, 1.0, nullptr, 0.0, s, prune2);       // y, per x plane
        if (rc != AST_OK) return rc;
    }
    const double kf_rule = binning == AST_BIN_FLOAT64 ? 2.0 * M_PI / boxsize : 0.0;
    {
        AST_PROF("fft64.cols_power", s);
        rc = col3_dispatch<true>(n, spec, twN, n * nzp, nz, n, nzp, 1.0 / ((double)n * (double)n * (double)n), partial, kf_rule, s, prune2);
        if (rc != AST_OK) return rc;
    }
    AST_PROF("fft64.shell_reduce", s);
    power64_stage1_kernel<<<REDUCE64, 256, 0, s>>>(partial, n * tiles, (int)nb, part2);
    power64_stage2_kernel<<<(unsigned)((nb + 255) / 256), 256, 0, s>>>(part2, (int)nb, boxsize * boxsize * boxsize, psum);
    AST_CHECK_LAUNCH();
    return AST_OK;
}

// rfftn(grid) * scale of an (n, n, n) float64 grid into spec_d (n, n, n / 2 + 1) complex, contiguous (pmesh's r2c with
// scale = 1 / n^3, power_spectrum_3d.py:189-195): the z rows and two strided passes above, in place on spec_d.
extern "C" int ast_fft64_r2c_3d(const double* grid, void* spec_out, size_t n, double scale, void* stream) {
    AST_CHECK_ARG(grid != nullptr && spec_out != nullptr && (const void*)grid != spec_out && ast_fft64_supported(n));
    AST_CHECK_ARG(((uintptr_t)grid & 15) == 0 && ((uintptr_t)spec_out & 15) == 0);
    hipStream_t s = ast::as_stream(stream);
    const size_t nz = n / 2 + 1;
    double2* spec = (double2*)spec_out;
    const double2* twH = twiddles64((int)(n / 2), s);
    const double2* twN = twiddles64((int)n, s);
    if (!twH || !twN) { ast::set_error("ast_fft64_r2c_3d: twiddle table allocation failed"); return AST_ERR_HIP; }
    int rc;
    {
        AST_PROF("fft64.rows_r2c", s);
        rc = rows64_dispatch<0>(n, grid, spec, nz, twH, twN, s);
        if (rc != AST_OK) return rc;
    }
    AST_PROF("fft64.cols", s);
    rc = col3_dispatch<false>(n, spec, twN, nz, nz, n, n * nz, 1.0, nullptr, 0.0, s);                      // y, per x plane
    if (rc != AST_OK) return rc;
    return col3_dispatch<false>(n, spec, twN, n * nz, nz, n, nz, scale, nullptr, 0.0, s);                 // x
}

// ================================================================== single-precision passes for cubes of side 2048
// The fp32 tile passes of fft_tile.hip are two register FFTs per axis (R1 x R2 <= 32 x 32 = 1024 points).  A cube of side
// 2048 - the largest whose fp32 grid (34 GB) and scratch spectrum (35 GB) one MI355X holds with room to spare - took the
// double passes above, widened on load: twice the bytes on every pass.  These are the same three-stage passes in float:
// z rows (half-length complex transform + untangling, the grid's mean subtracted as the rows are loaded), y pass, x pass
// fused with FFTPower's shell sums (power_spectrum_3d.py:189-224).  The strided passes take EIGHT k_z columns per workgroup
// (64-byte row pieces, the LDS of the double pass's four) and two columns per thread - one 16-byte access per row piece
// and lane, 1024 threads.  The lowest shells are patched from the double-precision side channel by the caller
// (ast_lowk_modes: fp32 round-off of an O(1) field on shells of a few dozen modes), as in the fp32 tile pipeline.
namespace {
__global__ void tw_table32_kernel(float2* out, int len) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    double sn, cs;
    sincospi(-2.0 * (double)i / (double)len, &sn, &cs);
    out[i] = make_float2((float)cs, (float)sn);
}
struct TwCache32 {
    std::mutex m;
    struct E { int dev, len; float2* d; };
    std::vector<E> tabs;
    const float2* get(int len, hipStream_t s) {
        std::lock_guard<std::mutex> lock(m);
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return nullptr;
        for (auto& t : tabs) if (t.dev == dev && t.len == len) return t.d;
        float2* d = nullptr;
        if (hipMalloc(&d, (size_t)len * sizeof(float2)) != hipSuccess) return nullptr;
        tw_table32_kernel<<<(len + 255) / 256, 256, 0, s>>>(d, len);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { (void)hipFree(d); return nullptr; }
        tabs.push_back({dev, len, d});
        return d;
    }
} g_tw32;

// one row per workgroup: 2 M reals -> M + 1 complex (lens_rows_forward_kernel without padding, fold or widening)
// FOLDW = 2 / 3 (CIC / TSC): the grid is what a deferred-fold paint left and `rec` its halo records; the up to three record
// lines that end in a border row are added as the row is loaded - records first, then onto the row, the order of the paint's
// own fold kernel (as in the double row kernel above and fft_tile.hip's).
template <int RA, int RB, int RC, int FOLDW = 0>
__global__ void __launch_bounds__((RowGeo<RA, RB, RC>::NT))
rows32_forward_kernel(const float* __restrict__ grid, size_t in_pitch, float2* __restrict__ spec, size_t pitch,
                      const float2* __restrict__ twM, const float2* __restrict__ twL, float scale, float mean,
                      const float* __restrict__ rec = nullptr) {
    using G = RowGeo<RA, RB, RC>;
    constexpr int M = G::M;
    extern __shared__ float2 Y32[];
    const int t = threadIdx.x;
    const size_t row = blockIdx.x;
    const float2* z = reinterpret_cast<const float2*>(grid + row * in_pitch);
    float2 va[RA], vc[RC];
    const float* src[3] = {nullptr, nullptr, nullptr};
    int ns = 0;
    if (FOLDW != 0) {
        constexpr int W = FOLDW != 0 ? FOLDW : 2;
        const int ng = 2 * M;
        ns = ast::halo_sources<float, W>(rec, (int)(row / ng), (int)(row % ng), ng, ng / ast::TX, ng / ast::TY, src);
    }
    if (t < G::T1) {
#pragma unroll
        for (int a = 0; a < RA; ++a) va[a] = z[G::T1 * a + t];
        if (FOLDW != 0 && ns > 0) {
            float2 h[RA];
#pragma unroll
            for (int a = 0; a < RA; ++a) h[a] = reinterpret_cast<const float2*>(src[0])[G::T1 * a + t];
            if (ns > 1) {
#pragma unroll
                for (int a = 0; a < RA; ++a) { const float2 g2 = reinterpret_cast<const float2*>(src[1])[G::T1 * a + t]; h[a].x += g2.x; h[a].y += g2.y; }
            }
            if (ns > 2) {
#pragma unroll
                for (int a = 0; a < RA; ++a) { const float2 g3 = reinterpret_cast<const float2*>(src[2])[G::T1 * a + t]; h[a].x += g3.x; h[a].y += g3.y; }
            }
#pragma unroll
            for (int a = 0; a < RA; ++a) { va[a].x += h[a].x; va[a].y += h[a].y; }
        }
#pragma unroll
        for (int a = 0; a < RA; ++a) {
            va[a].x -= mean;
            va[a].y -= mean;
        }
    }
    three_stage<RA, RB, RC>(va, vc, Y32, twM, t);
    constexpr int IT = (M / 2) / G::NT;
    static_assert(IT * G::NT == M / 2, "row length and thread count");
    float2 wk[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) wk[it] = twL[t + it * G::NT];
    __syncthreads();
    if (t < G::T3) {
#pragma unroll
        for (int ga = 0; ga < RC; ++ga) Y32[lds_pad((t / RB) + RA * (t % RB) + RA * RB * ga)] = vc[bitrev(ga, ilog2(RC))];
    }
    __syncthreads();
    float2* orow = spec + row * pitch;
    auto emit = [&](int k, float2 w) {
        const float2 zk = Y32[lds_pad(k)];
        const float2 zm = Y32[lds_pad(M - k)];
        const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
        const float2 o = make_float2(0.5f * (zk.x - zm.x), 0.5f * (zk.y + zm.y));
        const float2 tt = cmul(o, w);
        orow[k] = make_float2((e.x + tt.y) * scale, (e.y - tt.x) * scale);
        orow[M - k] = make_float2((e.x - tt.y) * scale, (-e.y - tt.x) * scale);
    };
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int k = t + it * G::NT;
        if (k == 0) {
            const float2 zk = Y32[lds_pad(0)];
            orow[0] = make_float2((zk.x + zk.y) * scale, 0.0f);
            orow[M] = make_float2((zk.x - zk.y) * scale, 0.0f);
        } else {
            emit(k, wk[it]);
        }
    }
    if (t == 0) emit(M / 2, twL[M / 2]);
}

// strided pass over N = RA RB RC rows, 8 adjacent columns per workgroup, 2 per thread (col3_kernel in float)
constexpr int C32 = 8, CT32 = 2;
constexpr unsigned FFT32_BIG_SIZES = 2048 | 256;                 // what ast_fft32_big_supported accepts
template <int RA, int RB, int RC, bool POWER>
__global__ void __launch_bounds__(((C32 / CT32) * RowGeo<RA, RB, RC>::NT))
col32_kernel(float2* __restrict__ data, const float2* __restrict__ twM, size_t elem_stride, size_t ncols, size_t batch_stride,
             unsigned tiles_per_batch, float scale, double* __restrict__ partial, double kf_rule, int prune2) {
    using G = RowGeo<RA, RB, RC>;
    constexpr int N = G::M, NB = N / 2 - 1, LINE = N + N / 8, CS = C32 / CT32, NTH = CS * G::NT;
    typedef float vf4 __attribute__((ext_vector_type(4)));
    extern __shared__ float2 L32[];
    double* shell = reinterpret_cast<double*>(L32 + C32 * LINE);          // [NB + 1] when POWER
    const int cs = threadIdx.x % CS, t = threadIdx.x / CS;
    // a workgroup touches HALF of every 128-byte line, the next tile the other half: both on one XCD (see col3_kernel)
    unsigned bid = blockIdx.x;
    {
        const unsigned full = gridDim.x / 16 * 16;
        if (bid < full) {
            const unsigned xcd = bid % 8, slot = bid / 8;
            bid = ((slot >> 1) * 8 + xcd) * 2 + (slot & 1);
        }
    }
    const unsigned tile = bid % tiles_per_batch, b = bid / tiles_per_batch;
    const size_t c0 = (size_t)tile * C32;
    if (prune2 > 0 && POWER) {
        const int ky = (int)b > N / 2 ? (int)b - N : (int)b;
        if (ky * ky + (int)(c0 * c0) > prune2) {                            // block-uniform, before any barrier
            for (int i = threadIdx.x; i < NB; i += NTH) partial[(size_t)bid * NB + i] = 0.0;
            return;
        }
    }
    // columns c0 + 2 cs, c0 + 2 cs + 1 as ONE 16-byte access (the row pitch is even and the tile starts at a multiple of 8);
    // a pair past the last column re-reads the last valid pair and is never stored or binned
    const size_t cpair = c0 + (size_t)(CT32 * cs);
    const size_t cload = cpair + 1 < ncols + (ncols & 1) ? cpair : ((ncols - 1) & ~(size_t)1);
    float2* base = data + (size_t)b * batch_stride + cload;
    const bool ok0 = cpair < ncols, ok1 = cpair + 1 < ncols;
    float2* Y0 = L32 + (CT32 * cs) * LINE;
    float2* Y1 = Y0 + LINE;
    if (POWER)
        for (int i = threadIdx.x; i <= NB; i += NTH) shell[i] = 0.0;
    float2 va0[RA], va1[RA], vc0[RC], vc1[RC];
    if (t < G::T1) {
#pragma unroll
        for (int a = 0; a < RA; ++a) {
            const vf4 v = *reinterpret_cast<const vf4*>(base + (size_t)(G::T1 * a + t) * elem_stride);
            va0[a] = make_float2(v.x, v.y);
            va1[a] = make_float2(v.z, v.w);
        }
    }
    // the two columns' stages between the same barriers
    if (t < G::T1) {
        fft_reg<RA>(va0);
        fft_reg<RA>(va1);
#pragma unroll
        for (int al = 0; al < RA; ++al) {
            float2 y0 = va0[bitrev(al, ilog2(RA))], y1 = va1[bitrev(al, ilog2(RA))];
            if (al != 0) { const float2 w = twM[t * al]; y0 = cmul(y0, w); y1 = cmul(y1, w); }
            Y0[lds_pad(al * G::T1 + t)] = y0;
            Y1[lds_pad(al * G::T1 + t)] = y1;
        }
    }
    __syncthreads();
    if (t < G::T2) {
        const int al = t / RC, c = t % RC;
#pragma unroll
        for (int j = 0; j < CT32; ++j) {
            float2* Y = j ? Y1 : Y0;
            float2 vb[RB];
#pragma unroll
            for (int bb = 0; bb < RB; ++bb) vb[bb] = Y[lds_pad(al * G::T1 + RC * bb + c)];
            fft_reg<RB>(vb);
#pragma unroll
            for (int be = 0; be < RB; ++be) {
                float2 y = vb[bitrev(be, ilog2(RB))];
                if (be != 0 && c != 0) y = cmul(y, twM[RA * c * be]);
                Y[lds_pad(al * G::T1 + RC * be + c)] = y;
            }
        }
    }
    __syncthreads();
    if (t < G::T3) {
#pragma unroll
        for (int c = 0; c < RC; ++c) { vc0[c] = Y0[lds_pad(t * RC + c)]; vc1[c] = Y1[lds_pad(t * RC + c)]; }
        fft_reg<RC>(vc0);
        fft_reg<RC>(vc1);
        const int al = t / RB, be = t % RB;
        if (!POWER) {
            if (ok0) {
                const int room = prune2 > 0 ? prune2 - (int)(c0 * c0) : 0x7fffffff;        // rows are k_y: keep k_y^2 <= room
#pragma unroll
                for (int ga = 0; ga < RC; ++ga) {
                    const float2 x0 = vc0[bitrev(ga, ilog2(RC))], x1 = vc1[bitrev(ga, ilog2(RC))];
                    const int row = al + RA * be + RA * RB * ga, aky = RA * RB * ga >= N / 2 ? N - row : row;
                    if (aky * aky <= room)
                        *reinterpret_cast<vf4*>(base + (size_t)row * elem_stride) = vf4{x0.x * scale, x0.y * scale, x1.x * scale, x1.y * scale};
                }
            }
        } else {
            const int ky = (int)b > N / 2 ? (int)b - N : (int)b;
#pragma unroll
            for (int j = 0; j < CT32; ++j) {
                if (!(j ? ok1 : ok0)) continue;
                const int kz = (int)cpair + j;
                const int m2yz = ky * ky + kz * kz;
                const float w = (kz > 0 && kz < N / 2) ? 2.0f : 1.0f;
#pragma unroll
                for (int ga = 0; ga < RC; ++ga) {
                    const float2 x = j ? vc1[bitrev(ga, ilog2(RC))] : vc0[bitrev(ga, ilog2(RC))];
                    const int row = al + RA * be + RA * RB * ga;
                    const int kx = row > N / 2 ? row - N : row;
                    const int m2 = kx * kx + m2yz;
                    int r = (int)__builtin_amdgcn_sqrtf((float)m2 + 0.5f);
                    if (r * r > m2) --r;                                      // (N = 2048: beyond the exhaustively checked range)
                    else if ((r + 1) * (r + 1) <= m2) ++r;
                    if (kf_rule != 0.0 && r > 0 && r * r == m2) r = ast::float64_edge_norm(r, kx, ky, kz, kf_rule);
                    // |delta_k|^2 in fp32 (one rounding per mode), accumulated in double - as in fft_tile.hip's binning pass
                    if (r >= 1 && r <= NB) atomicAdd(&shell[r], (double)(fmaf(x.x, x.x, x.y * x.y) * w));
                }
            }
        }
    }
    if (POWER) {
        __syncthreads();
        const double s2 = (double)scale * (double)scale;
        for (int i = threadIdx.x; i < NB; i += NTH) partial[(size_t)bid * NB + i] = shell[i + 1] * s2;
    }
}

template <int RA, int RB, int RC, bool POWER>
int col32_launch(float2* data, const float2* tw, size_t elem_stride, size_t ncols, size_t batch, size_t batch_stride, float scale,
                 double* partial, double kf_rule, hipStream_t s, int prune2) {
    using G = RowGeo<RA, RB, RC>;
    constexpr int LINE = G::M + G::M / 8;
    const size_t lds = (size_t)C32 * LINE * sizeof(float2) + (POWER ? (G::M / 2) * sizeof(double) : 0);
    static ast::PerDeviceOnce once;
    if (once.need()) {
        AST_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&col32_kernel<RA, RB, RC, POWER>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        once.mark();
    }
    const size_t tiles = (ncols + C32 - 1) / C32;
    AST_CHECK_ARG(tiles * batch < 0x7fffffffull);
    col32_kernel<RA, RB, RC, POWER><<<(unsigned)(tiles * batch), (C32 / CT32) * G::NT, lds, s>>>(data, tw, elem_stride, ncols, batch_stride,
                                                                                             (unsigned)tiles, scale, partial, kf_rule, prune2);
    AST_CHECK_LAUNCH();
    return AST_OK;
}
}  // namespace

// ------------------------------------------------------------------ the lowest shells in double, for the passes above
// A density painted from a lattice coarser than the grid carries O(1) power at the lattice's Bragg vectors and next to none
// at low k (1024^3 particles on 2048^3 cells: P(shell 5) = 1.4e-6 of the box volume): the fp32 passes' round-off - white,
// proportional to the field's rms - is 3e-6 of the signal at shell 5 and falls below 1e-6 only from shell 16 on (measured,
// scripts/perf_big32.py).  So the shells |m| < 17 come from double-precision sums over the grid, as the fp32 tile pipeline
// takes its five lowest (fft_tile.hip, MLOW) - with a box of |m_i| <= 17 instead of 6:
//   z  one wave per grid row: lane l holds f[l + 64 j]; per k_z the lane's NJ-term sum times e^{-2 pi i k_z l / n}, the 64
//      lanes' terms added in lane order through LDS                                   -> lowz[x][y][kz]
//   y  one workgroup per x plane, direct sums over y                                  -> lowy[x][ky][kz]
//   x  BIGLOW_XPARTS workgroups, each over its range of x, then the parts in order    -> modes[kx][ky][kz]
//   shells: one thread per shell walks all modes in a fixed order (integer rule, or nbodykit's float64 edge rule).
namespace {
constexpr int BIGLOW = 16;                         // shells 0 .. 15 (|m| in [1, 17))
constexpr int BIGBOX = BIGLOW + 1;                 // modes |m_i| <= 17: a vector of norm exactly 17 may fall into shell 15 (float64 rule)
constexpr int BIGKZ = BIGBOX + 1, BIGK = 2 * BIGBOX + 1;
constexpr int BIGLOW_MODES = BIGK * BIGK * BIGKZ;
constexpr int BIGLOW_XPARTS = 256;

template <int NJ, int FOLDW = 0>
__global__ void __launch_bounds__(256)
biglow_z_kernel(const float* __restrict__ grid, int n, size_t nrows, double mean, double2* __restrict__ out,
                const float* __restrict__ rec = nullptr) {
    __shared__ double part[4][2 * BIGKZ][65];                      // [wave][sum][lane] (65: the 36 readers on different banks)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double twc[BIGKZ], tws[BIGKZ];                                 // the lane's e^{-2 pi i kz lane / n}
#pragma unroll
    for (int kz = 0; kz < BIGKZ; ++kz) sincospi(-2.0 * (double)((kz * lane) % n) / (double)n, &tws[kz], &twc[kz]);
    const size_t nwaves = (size_t)gridDim.x * 4;
    for (size_t row = (size_t)blockIdx.x * 4 + wave; row < nrows; row += nwaves) {
        const float* in = grid + row * (size_t)n;
        // the lane's NJ samples z = lane + 64 j through ONE NJ-point register FFT (all NJ outputs for the price of the few
        // needed: 80 butterflies at NJ = 32 against 18 x 32 multiply-adds in a dependent chain, 105 ms -> ... at side 2048)
        float fr[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) fr[j] = in[lane + 64 * j];
        if (FOLDW != 0) {                                  // the fp32 value the z rows see: records first, then onto the row
            constexpr int W = FOLDW != 0 ? FOLDW : 2;      // (as in fft_tile.hip's lowk_z_kernel; see the note there)
            const float* src[3];
            const int ns = ast::halo_sources<float, W>(rec, (int)(row / n), (int)(row % n), n, n / ast::TX, n / ast::TY, src);
            if (ns > 0) {
                float h[NJ];
#pragma unroll
                for (int j = 0; j < NJ; ++j) h[j] = src[0][lane + 64 * j];
                if (ns > 1) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) h[j] += src[1][lane + 64 * j];
                }
                if (ns > 2) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) h[j] += src[2][lane + 64 * j];
                }
#pragma unroll
                for (int j = 0; j < NJ; ++j) fr[j] += h[j];
            }
        }
        double2 v[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) v[j] = make_double2((double)fr[j] - mean, 0.0);
        fft_reg<NJ>(v);
#pragma unroll
        for (int kz = 0; kz < BIGKZ; ++kz) {
            const double2 x = v[bitrev(kz % NJ, ilog2(NJ))];
            part[wave][2 * kz][lane] = x.x * twc[kz] - x.y * tws[kz];
            part[wave][2 * kz + 1][lane] = x.x * tws[kz] + x.y * twc[kz];
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < 2 * BIGKZ) {                                    // the 64 lanes' terms in a fixed order, eight sums in flight
            double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int l = 0; l < 64; ++l) acc[l & 7] += part[wave][lane][l];
            reinterpret_cast<double*>(out)[row * (size_t)(2 * BIGKZ) + lane] =
                ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// the y sums of one x plane: lowz[x][y][kz] -> lowy[x][ky][kz].  The plane's rows come through LDS 32 at a time (whole lines,
// read once); a thread owns up to three (ky, kz) outputs.  (The generic lowk_axis_kernel, which does the x sums, took 5.8 ms
// here: every term a dependent global load.)
__global__ void __launch_bounds__(256)
biglow_y_kernel(const double2* __restrict__ lowz, int n, double2* __restrict__ lowy) {
    extern __shared__ double2 lds64[];
    double2* tw = lds64;                                            // e^{-2 pi i t / n}
    double2* chunk = lds64 + n;                                     // [32][BIGKZ]
    constexpr int TC = 32, NOUT = BIGK * BIGKZ, PER = (NOUT + 255) / 256;
    for (int t = threadIdx.x; t < n; t += 256) {
        double sn, cs;
        sincospi(-2.0 * (double)t / (double)n, &sn, &cs);
        tw[t] = make_double2(cs, sn);
    }
    const double2* plane = lowz + (size_t)blockIdx.x * n * BIGKZ;
    double re[PER], im[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) { re[q] = 0.0; im[q] = 0.0; }
    for (int t0 = 0; t0 < n; t0 += TC) {
        __syncthreads();                                            // (the table; the previous chunk's readers)
        for (int e = threadIdx.x; e < TC * BIGKZ; e += 256) chunk[e] = plane[(size_t)t0 * BIGKZ + e];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int o = threadIdx.x + 256 * q;
            if (o < NOUT) {
                const int k = o / BIGKZ - BIGBOX, i = o % BIGKZ;
#pragma unroll 8
                for (int tt = 0; tt < TC; ++tt) {
                    const double2 v = chunk[tt * BIGKZ + i];
                    const double2 w = tw[(unsigned)(k * (t0 + tt)) & (unsigned)(n - 1)];
                    re[q] += v.x * w.x - v.y * w.y;
                    im[q] += v.x * w.y + v.y * w.x;
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int o = threadIdx.x + 256 * q;
        if (o < NOUT) lowy[(size_t)blockIdx.x * NOUT + o] = make_double2(re[q], im[q]);
    }
}

// psum[shell] += norm * sum over the box's modes of the shell of w |mode|^2, shells 0 .. BIGLOW - 1; modes[kx][ky][kz].
// 256 threads take the modes in turn, every thread its own 16 sums; thread `shell` then adds the 256 in thread order.
__global__ void __launch_bounds__(256)
biglow_shell_kernel(const double2* __restrict__ modes, double norm, double kf_rule, double* __restrict__ psum) {
    __shared__ double part[BIGLOW][257];
    double acc[BIGLOW];
#pragma unroll
    for (int sh = 0; sh < BIGLOW; ++sh) acc[sh] = 0.0;
    for (int o = threadIdx.x; o < BIGLOW_MODES; o += 256) {
        const int kz = o % BIGKZ, ky = (o / BIGKZ) % BIGK - BIGBOX, kx = o / (BIGKZ * BIGK) - BIGBOX;
        const int m2 = kx * kx + ky * ky + kz * kz;
        if (m2 == 0) continue;
        int r = (int)__builtin_amdgcn_sqrtf((float)m2 + 0.5f);       // m2 <= 3 * 17^2: exact after the repair step
        if (r * r > m2) --r;
        else if ((r + 1) * (r + 1) <= m2) ++r;
        if (kf_rule != 0.0 && r * r == m2) r = ast::float64_edge_norm(r, kx, ky, kz, kf_rule);
        const int shell = r - 1;
        if (shell < 0 || shell >= BIGLOW) continue;
        const double2 v = modes[o];
        const double p = (v.x * v.x + v.y * v.y) * (kz > 0 ? 2.0 : 1.0);
#pragma unroll
        for (int sh = 0; sh < BIGLOW; ++sh) acc[sh] += sh == shell ? p : 0.0;
    }
#pragma unroll
    for (int sh = 0; sh < BIGLOW; ++sh) part[sh][threadIdx.x] = acc[sh];
    __syncthreads();
    if (threadIdx.x < BIGLOW) {
        double total = 0.0;
        for (int t = 0; t < 256; ++t) total += part[threadIdx.x][t];
        psum[threadIdx.x] += norm * total;
    }
}

// the fp32 passes' sums for the shells from `first` on (the ones below come from the double-precision box)
__global__ void __launch_bounds__(256)
power32_stage2_kernel(const double* __restrict__ part, int nb, int first, double pnorm, double* __restrict__ psum) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nb || i < first) return;
    double acc = 0.0;
    for (int r = 0; r < REDUCE64; ++r) acc += part[(size_t)r * nb + i];
    psum[i] += pnorm * acc;
}

size_t biglow_bytes(size_t n) {
    return (n * n * BIGKZ + n * BIGK * BIGKZ + (size_t)(BIGLOW_XPARTS + 1) * BIGLOW_MODES) * sizeof(double2);
}
}  // namespace

// 2048 is what these passes are for; 256 (covered by the fp32 tile passes in production) is there so that the same kernels
// can be checked against the CPU oracle at a size it finishes in seconds
extern "C" int ast_fft32_big_supported(size_t n) { return n == 2048 || n == 256; }
static size_t fft32_pitch(size_t n) { return (n / 2 + 1 + 15) / 16 * 16; }        // complex64 elements: whole 128-byte lines
extern "C" size_t ast_fft32_big_power_scratch_bytes(size_t n) {
    const size_t nzp = fft32_pitch(n), tiles = (n / 2 + 1 + C32 - 1) / C32, nb = n / 2 - 1;
    return n * n * nzp * sizeof(float2) + n * tiles * nb * sizeof(double) + (size_t)REDUCE64 * nb * sizeof(double) + biglow_bytes(n);
}

// psum_d[shell] += L^3 sum over the shell's modes of w |delta_k|^2, delta_k = rfftn(grid - mean) / n^3, for an (n, n, n)
// float grid of side 2048: all passes in single precision, the shells |m| < 17 from double-precision sums over the grid
// (see the two section headers).  grid_d is not modified.
static int fft32_big_impl(const float* grid, const float* rec, int window, void* scratch, size_t scratch_bytes, size_t n,
                          double boxsize, int binning, double mean, double* psum, void* stream);
extern "C" int ast_fft32_big_power_3d(const float* grid, void* scratch, size_t scratch_bytes, size_t n, double boxsize, int binning,
                                      double mean, double* psum, void* stream) {
    return fft32_big_impl(grid, nullptr, 0, scratch, scratch_bytes, n, boxsize, binning, mean, psum, stream);
}
// The same for a grid painted with AST_PAINT_OVERWRITE | AST_PAINT_DEFER_FOLD: halo_rec_d (ast_paint_tiled_halo) is folded
// into the border rows as the z rows - and the low-k sums - load them.
extern "C" int ast_fft32_big_power_3d_halo(const float* grid, const float* halo_rec, int window, void* scratch, size_t scratch_bytes,
                                           size_t n, double boxsize, int binning, double mean, double* psum, void* stream) {
    AST_CHECK_ARG(halo_rec != nullptr && (window == AST_WIN_CIC || window == AST_WIN_TSC));
    return fft32_big_impl(grid, halo_rec, window, scratch, scratch_bytes, n, boxsize, binning, mean, psum, stream);
}
static int fft32_big_impl(const float* grid, const float* rec, int window, void* scratch, size_t scratch_bytes, size_t n,
                          double boxsize, int binning, double mean, double* psum, void* stream) {
    AST_CHECK_ARG(grid != nullptr && scratch != nullptr && psum != nullptr && boxsize > 0.0);
    AST_CHECK_ARG(ast_fft32_big_supported(n) && scratch_bytes >= ast_fft32_big_power_scratch_bytes(n));
    AST_CHECK_ARG(binning == AST_BIN_INTEGER || binning == AST_BIN_FLOAT64);
    AST_CHECK_ARG(((uintptr_t)grid & 7) == 0 && ((uintptr_t)scratch & 15) == 0);
    hipStream_t s = ast::as_stream(stream);
    const size_t nz = n / 2 + 1, nzp = fft32_pitch(n), tiles = (nz + C32 - 1) / C32, nb = n / 2 - 1;
    float2* spec = (float2*)scratch;
    double* partial = (double*)((char*)scratch + n * n * nzp * sizeof(float2));
    double* part2 = partial + n * tiles * nb;
    const float2* twH = g_tw32.get((int)(n / 2), s);
    const float2* twN = g_tw32.get((int)n, s);
    if (!twH || !twN) { ast::set_error("ast_fft32_big_power_3d: twiddle table allocation failed"); return AST_ERR_HIP; }
    const int prune2 = getenv("AST_FFT_NO_PRUNE") ? 0 : (int)((n / 2) * (n / 2));
    AST_CHECK_ARG(n * n < 0x7fffffffull);
    const float inv_ng = (float)(1.0 / ((double)n * (double)n * (double)n));
    const double kf_rule = binning == AST_BIN_FLOAT64 ? 2.0 * M_PI / boxsize : 0.0;
    {
        AST_PROF("fft32big.rows_r2c", s);
        LENS_FWD(with_radices<FFT32_BIG_SIZES / 2>(n / 2, [&](auto ha, auto hb, auto hc) -> int {      // the half-length rows
            constexpr int HA = ha.value, HB = hb.value, HC = hc.value;
            using G = RowGeo<HA, HB, HC>;
            const size_t lds = (size_t)(G::M + G::M / 8) * sizeof(float2);
            if (rec == nullptr) rows32_forward_kernel<HA, HB, HC, 0><<<(unsigned)(n * n), G::NT, lds, s>>>(grid, n, spec, nzp, twH, twN, 1.0f, (float)mean);
            else if (window == AST_WIN_CIC) rows32_forward_kernel<HA, HB, HC, 2><<<(unsigned)(n * n), G::NT, lds, s>>>(grid, n, spec, nzp, twH, twN, 1.0f, (float)mean, rec);
            else rows32_forward_kernel<HA, HB, HC, 3><<<(unsigned)(n * n), G::NT, lds, s>>>(grid, n, spec, nzp, twH, twN, 1.0f, (float)mean, rec);
            AST_CHECK_LAUNCH();
            return AST_OK;
        }));
    }
    LENS_FWD(with_radices<FFT32_BIG_SIZES>(n, [&](auto ra, auto rb, auto rc) -> int {
        {
            AST_PROF("fft32big.cols", s);
            LENS_FWD((col32_launch<ra.value, rb.value, rc.value, false>(spec, twN, nzp, nz, n, n * nzp, 1.0f, nullptr, 0.0, s, prune2)));     // y, per x plane
        }
        AST_PROF("fft32big.cols_power", s);
        return col32_launch<ra.value, rb.value, rc.value, true>(spec, twN, n * nzp, nz, n, nzp, inv_ng, partial, kf_rule, s, prune2);
    }));
    {
        AST_PROF("fft32big.shell_reduce", s);
        power64_stage1_kernel<<<REDUCE64, 256, 0, s>>>(partial, n * tiles, (int)nb, part2);
        power32_stage2_kernel<<<(unsigned)((nb + 255) / 256), 256, 0, s>>>(part2, (int)nb, BIGLOW, boxsize * boxsize * boxsize, psum);
        AST_CHECK_LAUNCH();
    }
    double2* lowz = (double2*)(part2 + (size_t)REDUCE64 * nb);
    double2* lowy = lowz + n * n * BIGKZ;
    double2* parts = lowy + n * BIGK * BIGKZ;
    double2* modes = parts + (size_t)BIGLOW_XPARTS * BIGLOW_MODES;
    const unsigned zblocks = (unsigned)std::min<size_t>((n * n + 3) / 4, (size_t)256 * 8);
    {
        AST_PROF("fft32big.lowk_z", s);
        auto lowz_launch = [&](auto nj) {
            constexpr int NJ = decltype(nj)::value;
            if (rec == nullptr) biglow_z_kernel<NJ, 0><<<zblocks, 256, 0, s>>>(grid, (int)n, n * n, mean, lowz);
            else if (window == AST_WIN_CIC) biglow_z_kernel<NJ, 2><<<zblocks, 256, 0, s>>>(grid, (int)n, n * n, mean, lowz, rec);
            else biglow_z_kernel<NJ, 3><<<zblocks, 256, 0, s>>>(grid, (int)n, n * n, mean, lowz, rec);
        };
        if (n == 2048) lowz_launch(std::integral_constant<int, 32>{});
        else lowz_launch(std::integral_constant<int, 4>{});
    }
    const size_t lds = n * sizeof(double2);
    {
        AST_PROF("fft32big.lowk_y", s);
        biglow_y_kernel<<<(unsigned)n, 256, lds + 32 * BIGKZ * sizeof(double2), s>>>(lowz, (int)n, lowy);                  // y, per x plane
    }
    {
        AST_PROF("fft32big.lowk_x", s);
        lowk_axis_kernel<BIGBOX><<<dim3(1, BIGLOW_XPARTS), 256, lds, s>>>(lowy, (int)n, (int)n, 0, BIGK * BIGKZ, parts);   // x, in parts
    }
    AST_PROF("fft32big.lowk_shells", s);
    lowk_parts_reduce_kernel<<<(BIGLOW_MODES + 255) / 256, 256, 0, s>>>(parts, BIGLOW_XPARTS, BIGLOW_MODES, 0, modes);
    const double ng = (double)n * (double)n * (double)n;
    biglow_shell_kernel<<<1, 256, 0, s>>>(modes, boxsize * boxsize * boxsize / (ng * ng), kf_rule, psum);
    AST_CHECK_LAUNCH();
    return AST_OK;
}
