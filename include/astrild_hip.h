/*
 * astrild_hip.h — C-ABI of libastrild_hip.so, the MI355X (gfx950) drop-in for
 * the numerics underneath astrild's post-processing hot path.
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes; no exceptions cross the boundary.
 *   - Every pointer named *_d / documented "device" is HBM (hipMalloc'd, or
 *     the data_ptr() of a PyTorch-ROCm tensor used as a memory holder).
 *   - The caller owns every buffer.  Plans own only their rocFFT work area.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); the
 *     call enqueues work on it and returns without synchronising, unless the
 *     doc says "synchronous".
 *   - Return value: AST_OK (0) or a negative AST_ERR_*; ast_last_error()
 *     returns a thread-local message for the last failure.
 *   - dtype: AST_F32 / AST_F64 selects the element type of particle and grid
 *     buffers (spectra are the matching interleaved complex type).
 *
 * Each entry cites the reference interface it replaces (paths relative to
 * /root/reference/src/astrild/).
 */
#ifndef ASTRILD_HIP_H
#define ASTRILD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AST_OK 0
#define AST_ERR_ARG (-1)
#define AST_ERR_HIP (-2)
#define AST_ERR_ROCFFT (-3)
#define AST_ERR_WORKSPACE (-4)
#define AST_ERR_LIMIT (-5) /* a bounded iteration did not end within its bound */

#define AST_F32 0
#define AST_F64 1

#define AST_WIN_NGP 0
#define AST_WIN_CIC 1
#define AST_WIN_TSC 2

#define AST_FFT_R2C 0 /* real forward  */
#define AST_FFT_C2R 1 /* real inverse  */
#define AST_FFT_C2C_FWD 2
#define AST_FFT_C2C_INV 3

int ast_version(void);
const char* ast_last_error(void);

/* Per-launch HIP-event timing for bench.py's roofline leg: while enabled every
 * kernel launch site records an event pair on its stream.  ast_profile_report
 * synchronises them and writes one "name,calls,total_ms" line per site into
 * buf (NUL terminated).  ast_profile_enable(0/1) also clears the records. */
int ast_profile_enable(int on);
int ast_profile_report(char* buf, size_t cap);

/* ---------------------------------------------------------------- utility */

/* buf[i] = value, i < count. */
int ast_fill(void* buf_d, int dtype, size_t count, double value, void* stream);

/* buf[i] /= divisor (IEEE division, bit-exact with numpy).  Replaces
 * SkyUtils.convert_code_to_phy_units (rays/skys/sky_utils.py:318-339:
 * kappa/shear/deflt / c^2, isw_rs / c^3) and the `/ dx**3` of
 * particles/hutils/stats_subfind.py:132. */
int ast_divide(void* buf_d, int dtype, size_t count, double divisor, void* stream);

/* Synthetic "Gaussian-random" particle set of SURVEY.md §8(d), generated in
 * HBM: lattice point q = (i+1/2, j+1/2, k+1/2) L/npside (k fastest) plus
 * sigma * N(0,1) per component, wrapped into [0, L).  Counter-based
 * generator keyed by (seed, particle index, component); particles
 * [first, first+count) of the lattice are written to pos_d as (count, 3).
 * `shuffle_stride` = UINT64_MAX writes them in a pseudo-random order, a fixed
 * permutation of the range keyed by seed + 1 (cycle-walked Feistel network over
 * the splitmix64 finaliser): the scatter-unfriendly ordering of SURVEY.md S8(d).
 * Any other non-zero value: t -> first + (t * shuffle_stride) mod count (a
 * permutation when the stride is coprime with count; low-discrepancy, kept for A/B).
 * Bench / test plumbing, not part of the reference. */
int ast_synth_lattice_particles(void* pos_d, int dtype, size_t first, size_t count,
                                int npside, double boxsize, double sigma,
                                uint64_t seed, uint64_t shuffle_stride, void* stream);
/* A CLUSTERED synthetic set (bench / test plumbing): the npside^3 lattice collapsing onto `nattractors` (<= 1024) centres,
 * x = q - sum_h amplitude exp(-r^2 / 2 R_h^2) (q - c_h) + sigma N(0,1), R_h between 6 and 48 lattice spacings (many small,
 * few large), centres and radii from hashes of seed.  amplitude 0.95: knots of several 10^5 particles in a few cells -
 * tile occupancies ~100 x the mean, like the evolved snapshots and halo catalogues the reference paints
 * (stats_subfind.py:125-131) - in lattice order (neighbours in memory stay neighbours in space outside the knots) or,
 * with shuffle != 0, in the pseudo-random order of ast_synth_lattice_particles.  count must be npside^3. */
int ast_synth_clustered_particles(void* pos_d, int dtype, size_t count, int npside, double boxsize, double sigma,
                                  uint64_t seed, int nattractors, double amplitude, int shuffle, void* stream);

/* ----------------------------------------------- a-1 / a-2: mass assignment */

/* NGP scatter-ASSIGN with numpy's last-write-wins semantics.  Replaces
 * PowerSpectrum3D._read_data, power_spectra/power_spectrum_3d.py:142-148:
 *     idx = (npar * coord).astype(int);  value_map[(x, y, z)] = values
 * x_d, y_d, z_d, values_d: np elements each (DataFrame columns, SoA).
 * grid_d: npar^3 elements, C order (axis 0 slowest); zero-filled by the call.
 * owner_d: npar^3 uint32 scratch.  np must be < 2^32 - 1.  Coordinates must
 * lie in [0, 1) like the reference requires (numpy would raise IndexError
 * otherwise); out-of-range particles are counted in *dropped_d (device
 * uint64, may be NULL) and skipped. */
int ast_ngp_assign(const void* x_d, const void* y_d, const void* z_d, const void* values_d,
                   int dtype, size_t np, int npar, void* grid_d, uint32_t* owner_d,
                   unsigned long long* dropped_d, void* stream);

/* Mass-weighted scatter-ADD with a separable NGP / CIC / TSC window.
 * Replaces pmesh ParticleMesh(Nmesh=[n]*3, BoxSize=L).paint(pos, mass=,
 * resampler=) as called at particles/hutils/stats_subfind.py:130-131 (and the
 * window='TSC' meshes of power_spectrum_3d.py:197-212).
 *   pos_d:  (np, 3) AoS, box units; any real value wraps periodically.
 *   mass_d: np elements or NULL (unit mass).
 *   scale:  every deposit is multiplied by it (1/dx^3 folds the division of
 *           stats_subfind.py:132 into the paint; 1.0 = pmesh behaviour).
 *   grid_d: ACCUMULATED into (caller zero-fills).  It holds nx_alloc planes
 *           of nmesh x nmesh cells: buffer plane p is global axis-0 plane
 *           (x_start + p) mod nmesh.  Single GPU: x_start = 0,
 *           nx_alloc = nmesh.  Slab-decomposed: the rank's owned planes plus
 *           its ghost planes.  Deposits falling outside the buffer are
 *           counted in *dropped_d (device uint64, may be NULL) and skipped.
 *   shift_cells: added to every coordinate in GRID units, s = x * nmesh/boxsize + shift_cells (one fma;
 *           0 = plain paint).  Interlacing (nbodykit CatalogMesh, interlaced=True) paints a second
 *           mesh with shift_cells = 0.5, see ast_interlace_compensate.
 * Index/fraction arithmetic is float64 for both dtypes; the accumulation is
 * in `dtype` with hardware atomics (sum order is not reproducible). */
int ast_paint(int window, int dtype, const void* pos_d, const void* mass_d, size_t np,
              int nmesh, double boxsize, double scale, int x_start, int nx_alloc,
              void* grid_d, unsigned long long* dropped_d, double shift_cells, void* stream);

/* Same result as ast_paint, for the CIC/TSC windows, through LDS-resident
 * grid tiles: particles are run-length grouped by the tile of their base
 * cell (no particle data is moved), each workgroup accumulates one tile in
 * LDS and flushes it once.  workspace_d must hold
 * ast_paint_tiled_workspace_bytes(window, dtype, np, nmesh, nx_alloc, flags) bytes. */
/* flags: 0 = single pass over the particles (fixed-capacity tile segments, overflow
 * deposited with global atomics); AST_PAINT_TWO_PASS = exact count + scan first
 * (one more read of the positions, no overflow path: for strongly clustered input). */
#define AST_PAINT_TWO_PASS 1
/* AST_PAINT_OVERWRITE: grid_d is OVERWRITTEN with this paint instead of accumulated into
 * (no zero-fill needed).  Each workgroup then walks a whole z-column of tiles with the z
 * halo carried in LDS; owned cells leave as plain stores, the x/y halo ring goes through
 * per-column records folded in by a second kernel — no global float atomics in the flush.
 * The LDS tiles then accumulate in 64-bit fixed point (order-independent, so the paint is
 * bit-reproducible); `mass_bound` must be >= max |mass| when mass_d is given (ast_minmax). */
#define AST_PAINT_OVERWRITE 2
/* AST_PAINT_DEFER_FOLD (with AST_PAINT_OVERWRITE, whole periodic grid only): the last kernel of the
 * paint - adding the columns' x/y halo records into their neighbours' border lines - is left out;
 * the grid is complete only after ast_fft_tile_power_3d_halo has read it, which folds the records
 * while its z pass loads the rows (one kernel and ~2 GB of traffic less at 1024^3). */
#define AST_PAINT_DEFER_FOLD 4
/* AST_PAINT_SCATTERED (single pass + AST_PAINT_OVERWRITE): a hint that the particles have no spatial order
 * in memory.  The single-pass overwrite paint groups each 32-particle window by tile (8-byte group records)
 * and copies the few particles that have no companions in their window ("strays", 16/32 bytes) into their
 * tile's segment; by default a tile's stray segment holds a quarter of its particle capacity, with this flag
 * all of it (3.4x the workspace).  Without the hint unordered input still paints correctly - what does not
 * fit goes through the (slow) overflow list. */
#define AST_PAINT_SCATTERED 8
/* AST_PAINT_XSORTED (single pass + AST_PAINT_OVERWRITE, not with AST_PAINT_SCATTERED): a hint that the particles
 * come in ascending x (buffer planes) - lattice order, slab-ordered snapshot files.  The paint then runs as a
 * pipeline over chunks of particles: while chunk k + 1 is grouped, the column walk of the tile rows that chunk
 * k completed runs beside it on a second stream (event-ordered against `stream`).  A particle that arrives for a
 * row already walked goes through the overflow list (global atomics): input that is not sorted after all still
 * paints correctly, only slower. */
#define AST_PAINT_XSORTED 16
/* offset (AST_PAINT_OVERWRITE only, else 0): every OWNED cell is stored as (sum - offset), the
 * subtraction done in double on the exact fixed-point sum before the single rounding to `dtype`
 * (halo records stay additive).  With offset = total mass * scale / nmesh^3 the grid holds the
 * density CONTRAST rho - mean: only the DC mode of its spectrum changes (FFTPower discards it),
 * and fp32 cells stop carrying the rounding error of the O(1) mean.  Only the buffer planes
 * [offset_start, offset_start + offset_count) receive it (offset_count < 0: all): the ghost planes of a slab
 * buffer are ADDED to other ranks' cells and must stay plain sums. */
size_t ast_paint_tiled_workspace_bytes(int window, int dtype, size_t np, int nmesh, int nx_alloc, int flags);
int ast_paint_tiled(int window, int dtype, const void* pos_d, const void* mass_d, size_t np,
                    int nmesh, double boxsize, double scale, int x_start, int nx_alloc,
                    void* grid_d, void* workspace_d, size_t workspace_bytes,
                    unsigned long long* dropped_d, int flags, double mass_bound, double offset,
                    int offset_start, int offset_count, double shift_cells, void* stream);
/* The single-pass AST_PAINT_OVERWRITE paint in parts (no TWO_PASS / DEFER_FOLD / XSORTED), for callers that consume the
 * grid plane range by plane range while the rest is still being painted - the slab pipeline (the
 * reference paints on one rank, stats_subfind.py:130-131): every call takes the arguments of ast_paint_tiled, all of
 * them identical from call to call, plus
 *   AST_PAINT_STAGE_GROUP          once: the particle lists of every tile (and the scatter levels of AST_PAINT_SCATTERED);
 *   AST_PAINT_STAGE_WALK  row0 n   the column walk (and z seams) of tile rows [row0, row0 + n): their owned cells are
 *                                  stored, their x / y halo goes to the rows' records;
 *   AST_PAINT_STAGE_FOLD  row0 n   adds the neighbours' records (and the overflow list's deposits) into these rows'
 *                                  planes: needs the WALK of rows row0 - 1 .. row0 + n (CIC: row0 - 1 .. row0 + n - 1)
 *                                  that exist in the buffer, and completes buffer planes [row0 * P, (row0 + n) * P),
 *                                  P = ast_paint_tile_row_planes().
 * A tile row is P consecutive buffer planes, row 0 starting at buffer plane 0; ast_paint_tile_rows(nx_alloc) rows.
 * After GROUP, WALK of every row and FOLD of every row the grid equals ast_paint_tiled's, bit for bit.  Calls may go to
 * different streams; ordering them as above is the caller's business. */
#define AST_PAINT_STAGE_ALL (-1)
#define AST_PAINT_STAGE_GROUP 0
#define AST_PAINT_STAGE_WALK 1
#define AST_PAINT_STAGE_FOLD 2
/* Grouping in PARTS, for particles that come in ascending x (slab-ordered input; slab buffers only, not AST_PAINT_SCATTERED):
 *   AST_PAINT_STAGE_RESET          once, instead of GROUP: clears the lists' counters;
 *   AST_PAINT_STAGE_GROUP_PART k K the lists of part k of K equal parts of the particle array (row0 = k, nrows = K), in any
 *                                  order of parts; nrows = K | (span - 1) << 16 (K <= 65535) takes the `span` consecutive
 *                                  parts k .. k + span - 1 in ONE launch (stages of unequal size).  closed_row0 / closed_nrows name the tile rows that have been WALKED
 *                                  already - one range, taken modulo the buffer's rows (the rows of the top ghost planes
 *                                  first, then 0, 1, ...).  A particle of a later part whose tile lies in a closed row
 *                                  cannot be painted any more (the row may have been transformed and sent): it is counted
 *                                  in *dropped_d - the caller's promise about the order did not hold - and skipped.
 * A row may be walked once every part that can hold a particle of it has been grouped; the walks, folds and the result
 * are those of the one-part GROUP.  closed_row0 / closed_nrows are ignored by the other stages. */
#define AST_PAINT_STAGE_GROUP_PART 3
#define AST_PAINT_STAGE_RESET 4
/*   AST_PAINT_STAGE_LATE  row0 n   FOLD without the record fold: only the overflow / late list's deposits into these rows'
 *                                  planes - for rows whose halo records are added by the consumer instead
 *                                  (ast_fft_tile_rows_r2c_slab_halo folds them as its z pass loads the rows). */
#define AST_PAINT_STAGE_LATE 5
int ast_paint_tiled_stage(int window, int dtype, const void* pos_d, const void* mass_d, size_t np,
                          int nmesh, double boxsize, double scale, int x_start, int nx_alloc,
                          void* grid_d, void* workspace_d, size_t workspace_bytes,
                          unsigned long long* dropped_d, int flags, double mass_bound, double offset,
                          int offset_start, int offset_count, double shift_cells, int stage, int row0, int nrows,
                          int closed_row0, int closed_nrows, void* stream);
int ast_paint_tile_rows(int nx_alloc);
int ast_paint_tile_row_planes(void);
/* Where a paint with AST_PAINT_OVERWRITE | AST_PAINT_DEFER_FOLD and these parameters left its halo
 * records inside workspace_d (for ast_fft_tile_power_3d_halo). */
int ast_paint_tiled_halo(void* workspace_d, int window, int dtype, size_t np, int nmesh, int nx_alloc, int flags,
                         void** rec_out);

/* What the single-pass AST_PAINT_OVERWRITE paint with these parameters left in workspace_d: out_d[0] group records,
 * out_d[1] stray copies, out_d[2] particles that went through the overflow list, out_d[3] the largest number of
 * strays a tile asked for (device uint64 x 4).  Diagnostics: a large out_d[2] says the input wants
 * AST_PAINT_SCATTERED or AST_PAINT_TWO_PASS. */
int ast_paint_tiled_list_stats(void* workspace_d, int window, int dtype, size_t np, int nmesh, int nx_alloc, int flags,
                               unsigned long long* out_d, void* stream);
/* Host only: the records {x, y, z, m} the AST_PAINT_SCATTERED paint's late list holds for np particles (np / 4 at
 * AST_F32, np / 8 at AST_F64; 0 for another dtype).  Records beyond it are counted in dropped_d, not deposited: on a
 * whole periodic grid a nonzero drop count after such a paint means the list ran out of room. */
size_t ast_paint_scatter_late_capacity(int dtype, size_t np);
/* Does the input have spatial order in memory?  `windows` (2 .. 65536) runs of 32 consecutive particles, evenly spread over
 * pos_d; *groupable_d (device, 4 bytes; zeroed by the call) = the number of runs in which at least 8 particles share the
 * 8 x 8 x 32-cell tile of the run's 16th particle - what the tiled paint's grouping kernel turns into group records.
 * Lattice-, cell- or curve-ordered input: nearly all runs; shuffled input: none, and the paint belongs on
 * AST_PAINT_SCATTERED from the start (device.paint decides so below a quarter).  np >= 32.  No reference counterpart:
 * pmesh's paint (stats_subfind.py:130-131) does not care about order. */
int ast_paint_order_probe(const void* pos_d, int dtype, size_t np, int nmesh, double boxsize, double shift_cells,
                          int windows, unsigned* groupable_d, void* stream);
/* Will the single-pass paint's fixed tile segments (room for max(2 mean, mean + 512) particles per 8 x 8 x 32-cell tile)
 * overflow?  `samples` particles, one from every stride of np / samples at a hashed offset, are counted per tile of the
 * periodic grid in counts_d (ast_paint_occupancy_probe_bytes(nmesh) bytes, zeroed by the call); out_d[0] = the estimated
 * number of particles beyond their tile's capacity, out_d[1] = the largest estimated tile occupancy (device uint64 x 2).
 * With >= 8 samples per tile on average a uniform input reads < 0.1 % of np; clustered input (evolved snapshots, the halo
 * catalogue of stats_subfind.py:125-131) reads what the overflow list would have held - before anything is painted, so
 * the caller can go to AST_PAINT_TWO_PASS at once.  nmesh a multiple of 32. */
size_t ast_paint_occupancy_probe_bytes(int nmesh);
int ast_paint_occupancy_probe(const void* pos_d, int dtype, size_t np, int nmesh, double boxsize, double shift_cells,
                              size_t samples, void* counts_d, size_t counts_bytes, unsigned long long* out_d, void* stream);

/* Interlacing and window compensation of a catalogue-painted mesh in Fourier space - what nbodykit's
 * CatalogMesh does for the parameters astrild writes at power_spectra/power_spectrum_3d.py:197-212
 * (compensated=True, interlaced=True, window='TSC'; they are inert for the ArrayMesh inputs the reference
 * passes, real for particle catalogues).  c1_d: half spectrum (block [i0, i1, nmesh/2+1], like
 * ast_power_bin_1d) of the plain paint, updated in place; c2_d: spectrum of the paint with shift_cells = 0.5,
 * or NULL (no interlacing):
 *   c1 <- (c1 + c2 exp(i (wx+wy+wz)/2)) / 2,   w = 2 pi m / nmesh;
 *   compensate != 0:  c1 <- c1 / prod_axes W(w):  sinc(w/2)^p (p = 2 CIC, 3 TSC) with interlacing,
 *   sqrt(1 - 2/3 s) / sqrt(1 - s + 2/15 s^2), s = sin^2(w/2), without (nbodykit's Compensate*Shotnoise). */
int ast_interlace_compensate(void* c1_d, const void* c2_d, int dtype, int nmesh, int window, int compensate,
                             int i0_start, int i0_count, int i1_start, int i1_count, void* stream);

/* Particle routing for input that is not partitioned by slab: the destination of a particle is
 * the slab (nmesh / nparts planes of axis 0) that owns its base plane - floor(s) for CIC, floor(s + 1/2) for NGP/TSC,
 * s = x nmesh / boxsize, wrapped.  ast_route_count: counts_d[part] (device uint64, caller zero-fills) += particles per
 * slab.  ast_route_scatter: cursor_d holds the exclusive prefix sums of the counts on entry (it is advanced); slab
 * `part`'s particles are written contiguously to out_pos_d (and out_mass_d when mass_d is given) from its cursor on,
 * ready for an all-to-all-v with the counts as split sizes.  nparts <= 64. */
int ast_route_count(const void* pos_d, int dtype, size_t np, int nmesh, double boxsize, int window, int nparts,
                    unsigned long long* counts_d, void* stream);
int ast_route_scatter(const void* pos_d, const void* mass_d, int dtype, size_t np, int nmesh, double boxsize, int window,
                      int nparts, unsigned long long* cursor_d, void* out_pos_d, void* out_mass_d, void* stream);

/* dst[i] += src[i] — ghost-plane fold after a slab paint. */
int ast_accumulate(void* dst_d, const void* src_d, int dtype, size_t count, void* stream);
/* Measurement aid (SURVEY.md §8d "also measure an on-box streaming-copy kernel"): streams `bytes` (a multiple of 16,
 * 16-byte aligned) with 16-byte accesses - mode 0 copy src -> dst, 1 read src only, 2 write dst only (the fastest access
 * variant of each; mode | 256 | variant << 4 picks one explicitly, scripts/micro/copy_rate.py).  bench.py times it
 * and quotes every roofline fraction against this ceiling beside the 8 TB/s of the data sheet.  No reference counterpart. */
int ast_stream_copy(void* dst_d, const void* src_d, size_t bytes, int mode, void* stream);

/* ------------------------------------------------------------- a-4: FFTs */

typedef struct ast_fft_plan ast_fft_plan;

/* rocFFT plan.  lengths[] are in C (row-major) order, slowest axis first,
 * like numpy shapes.  Real transforms keep the half spectrum on the LAST
 * axis (lengths[rank-1]/2+1 complex values).  `scale` multiplies every
 * output element (1/Ng gives pmesh's r2c normalisation used by nbodykit
 * FFTPower, power_spectrum_3d.py:189-195).  Contiguous layouts.  The plan
 * allocates its rocFFT work buffer with hipMalloc. */
int ast_fft_plan_create(ast_fft_plan** plan, int kind, int dtype, int rank,
                        const size_t* lengths, size_t batch, double scale, int inplace);

/* Complex 1-D transforms of length `length` with element stride `stride`,
 * `batch` of them `dist` elements apart (in place) — the axis-0 pass of the
 * slab-decomposed 3D FFT. */
int ast_fft_plan_create_strided_1d(ast_fft_plan** plan, int kind, int dtype, size_t length,
                                   size_t stride, size_t batch, size_t dist, double scale);

/* General strided layout: strides (in elements of the respective array, real or
 * complex) are given per axis in the same C order as lengths[]. */
int ast_fft_plan_create_general(ast_fft_plan** plan, int kind, int dtype, int rank, const size_t* lengths,
                                const size_t* in_strides, const size_t* out_strides, size_t batch,
                                size_t in_dist, size_t out_dist, double scale, int inplace);

size_t ast_fft_plan_work_bytes(const ast_fft_plan* plan);
int ast_fft_exec(ast_fft_plan* plan, void* in_d, void* out_d, void* stream);
int ast_fft_plan_destroy(ast_fft_plan* plan);

/* Hand-written LDS-tiled FFT passes (fp32, n in {256, 512, 1024}): the 3D R2C as
 * exactly three passes over the array (rocFFT's plan at 1024^3 runs six kernels
 * and moves ~2x the bytes).  Same results as the rocFFT plans above to fp32
 * round-off; callers fall back to rocFFT when ast_fft_tile_supported() is 0.
 *   ast_fft_tile_c2c: in-place forward transforms of length n over
 *       data[b*batch_stride + k*elem_stride + c], c < ncols contiguous columns.
 *   ast_fft_tile_rows_r2c: nrows contiguous real rows of n -> n/2+1 complex.
 *   ast_fft_tile_r2c_3d: (n,n,n) real -> (n,n,n/2+1), out = scale * sum f e^{-ikx}. */
int ast_fft_tile_supported(int dtype, size_t n);
int ast_fft_tile_c2c(void* data_d, int dtype, size_t n, size_t elem_stride, size_t ncols, size_t batch,
                     size_t batch_stride, double scale, void* stream);

/* ast_fft_tile_c2c over the k_y axis of a rank's local planes (planes_d: (nplanes, n, pitch) complex of which the first
 * ncols columns of every row are data; left intact) with ast_slab_pack fused into the stores: packed_d receives `parts`
 * blocks of (nplanes, n / parts, pitch), the send buffer of the slab transpose (pmesh's r2c transposes inside the
 * reference's FFTPower call, power_spectrum_3d.py:203-208).  parts: a power of two dividing n.  pitch >= ncols: a pitch
 * that is a multiple of 16 keeps every row piece on whole 128-byte lines (the columns ncols .. pitch - 1 are neither
 * read nor written).  With self_out_d, part self_part (the rank's own piece, which never travels) is written there
 * instead, as (nplanes, n / parts, pitch); packed_d may then be NULL when parts == 1. */
int ast_fft_tile_c2c_packed(const void* planes_d, void* packed_d, int dtype, size_t n, size_t ncols, size_t pitch,
                            size_t nplanes, int parts, int self_part, void* self_out_d, double scale, void* stream);
int ast_fft_tile_rows_r2c(const void* in_d, void* out_d, int dtype, size_t n, size_t nrows, size_t in_pitch,
                          size_t out_pitch, double scale, void* stream);
/* ast_fft_tile_rows_r2c that also leaves the low-k channel's z sums of its rows (sum_z f e^{-2 pi i kz z / n}, kz <= 6,
 * in double, from the samples the pass holds in registers anyway) at lowz_d: nrows x 7 complex128, [row][kz] - the
 * first stage of ast_lowk_modes without its second read of the planes.  fp32, n in {256, 512, 1024}. */
int ast_fft_tile_rows_r2c_lowz(const void* in_d, void* out_d, int dtype, size_t n, size_t nrows, size_t in_pitch,
                               size_t out_pitch, double scale, void* lowz_d, void* stream);
/* The z pass of a plane range of a SLAB buffer painted in stages (ast_paint_tiled_stage), folding the paint's halo records as
 * the rows are loaded - what AST_PAINT_STAGE_FOLD adds, in the same order (bit-identical): in_d = buffer plane xb0, nrows =
 * planes * n rows; halo_rec_d from ast_paint_tiled_halo for the same buffer (nx_alloc planes, not periodic in x); planes whose
 * tile row lies in [fold_row_lo, fold_row_hi) are folded here, the others must have had their FOLD stage (the rows that hold
 * ghost planes).  lowz_d: NULL, or the low-k z sums of these rows as ast_fft_tile_rows_r2c_lowz leaves them. */
int ast_fft_tile_rows_r2c_slab_halo(const void* in_d, void* out_d, int dtype, size_t n, size_t nrows, size_t out_pitch,
                                    double scale, const void* halo_rec_d, int window, int xb0, int nx_alloc, int fold_row_lo,
                                    int fold_row_hi, void* lowz_d, void* stream);
int ast_fft_tile_r2c_3d(const void* in_d, void* out_d, int dtype, size_t n, double scale, void* stream);
/* The unnormalised inverse in three tile passes (x, y, z): out_d[x] = scale * sum_k spec_k e^{+ikx} for an (n, n, n/2+1)
 * half spectrum (fp32, n in {256, 512, 1024}).  spec_d is not modified; work_d (as large as spec_d) is scratch.
 * m_hi > m_lo >= 0: only the modes with m_lo <= |m| < m_hi enter - the shell filter of the bispectrum estimator
 * (ast_shell_filter) fused into the first pass's loads; m_hi = 0: all modes. */
int ast_fft_tile_c2r_3d(const void* spec_d, void* work_d, void* out_d, int dtype, size_t n, int m_lo, int m_hi,
                        double scale, void* stream);
/* The same for up to 8 shells of one spectrum in three launches instead of 3 per shell (the x, y and z passes take the
 * shell from the launch's second grid dimension): works[i] / outs[i] - HOST arrays of device pointers, all distinct - are
 * shell i's scratch spectrum and real output, m_lo[i] < m_hi[i] (host ints) its radii.  Outputs bit-identical to the
 * single call's.  passes: 1 = the x and y passes only (works[i] then hold what the z pass reads), 2 = the z pass only, 3 = all -
 * so that a caller can run x / y shell by shell (the y pass finds the x pass's output in the Infinity Cache) and the z
 * passes of several shells in one launch (small shells fill the tails of large ones).
 * work_pitch: row pitch of the scratch spectra in complex elements, 0 or >= n/2+1 (0 = n/2+1; works[i] then hold
 * n * n * work_pitch elements).  A multiple of 16 keeps the 128-byte row pieces of the x / y passes on whole lines. */
int ast_fft_tile_c2r_3d_batch(const void* spec_d, void* const* works, void* const* outs, int dtype, size_t n,
                              const int* m_lo, const int* m_hi, int count, double scale, int passes, size_t work_pitch,
                              void* stream);
/* a-4 + a-5 fused: FFTPower's shell sums of an (n, n, n) real grid.  z and y passes
 * go through scratch_d (line-aligned row pitch); the x pass adds w |delta_k|^2 of its
 * modes to per-workgroup shell tables instead of storing delta_k, and a fixed-order
 * reduction adds them into psum_d (same meaning as in ast_power_bin_1d; auto power). */
/* The bispectrum estimator's last two steps in ONE kernel: the z passes (C2R) of all shells - works[s] = shell s's scratch
 * spectrum after the masked x and y passes (ast_fft_tile_c2r_3d_batch, passes = 1), (n, n, work_pitch) complex64, m_hi[s] its
 * outer radius - and the triangle sums out_d[t] = sum_x f_a f_b f_c, f_s = scale * C2R_z(works[s]), for the ntri triangles
 * tri_d[(ntri, 3)] of shell slots.  One workgroup transforms one (x, y) row of EVERY shell and forms the sums from LDS: the
 * real cubes (31 x 0.5 GB written and read back at 512^3) never reach HBM.  bispectrum_3d.py:165-215 holds no such
 * arithmetic; this is the estimator its docstring cites.  nshells <= 32; ntri <= 512 (1024 at n = 1024). */
size_t ast_fft_tile_c2r_triangles_scratch_bytes(void);
int ast_fft_tile_c2r_triangles(void* const* works, const int* m_hi, int nshells, int dtype, size_t n, size_t work_pitch,
                               double scale, const int* tri_d, int ntri, void* scratch_d, double* out_d, void* stream);
size_t ast_fft_tile_power_scratch_bytes(size_t n);
/* test hook: out_d[v] = the fused binning's floor(sqrt(v)) (one hardware sqrt, no repair), v < count */
int ast_fft_tile_isqrt_table(int* out_d, int count, void* stream);
/* `binning`: AST_BIN_INTEGER / AST_BIN_FLOAT64, see ast_power_bin_1d. */
#define AST_BIN_INTEGER 0
#define AST_BIN_FLOAT64 1
/* `mean`: a constant subtracted from every cell as it is loaded (0 = none).  It only
 * changes the DC mode, which FFTPower discards, but with it the fp32 round-off of all
 * other modes no longer scales with the O(1) mean density (cold low-k shells gain). */
/* `lowk` = 1: the modes with |m_i| <= 5 are ALSO evaluated as DFT sums in double (one more read of the grid) and the
 * five lowest shells, |m| in [1, 6), take their sums from there: the fp32 transform's white round-off floor
 * (~1e-7 of the rms amplitude per mode) otherwise limits shells that hold 1e-5 of the peak power to ~2e-6 / |m|^2. */
int ast_fft_tile_power_3d(const void* grid_d, void* scratch_d, size_t scratch_bytes, int dtype, size_t n,
                          double boxsize, double mean, int lowk, int binning, double* psum_d, void* stream);
/* The same for a grid painted with AST_PAINT_OVERWRITE | AST_PAINT_DEFER_FOLD (fp32, whole periodic grid):
 * halo_rec_d comes from ast_paint_tiled_halo on the paint's workspace; the records are added to the border
 * rows as the z pass loads them, in the order the paint's own fold kernel uses (bit-identical result). */
int ast_fft_tile_power_3d_halo(const void* grid_d, const void* halo_rec_d, int window, void* scratch_d,
                               size_t scratch_bytes, int dtype, size_t n, double boxsize, double mean,
                               int lowk, int binning, double* psum_d, void* stream);

/* The axis-0 pass of a slab-decomposed transform fused with the shell binning (the multi-GPU counterpart of the fused x
 * pass): block_d is the rank's (n, nloc, pitch) block of the spectrum after the all-to-all - all k_x, k_y = ky0 ..
 * ky0 + nloc - 1, half k_z, `pitch` >= n/2+1 complex per row.  psum_d[shell] += L^3 sum w |scale * X|^2 over the block's
 * modes; shells below first_bin are skipped (low-k channel); the block's contents afterwards are undefined.
 * scratch_d: ast_fft_tile_block_power_scratch_bytes(n, nloc). */
size_t ast_fft_tile_block_power_scratch_bytes(size_t n, size_t nloc);
int ast_fft_tile_block_power(void* block_d, void* scratch_d, size_t scratch_bytes, int dtype, size_t n, size_t nloc,
                             size_t ky0, size_t pitch, double scale, double boxsize, int first_bin, int binning,
                             double* psum_d, void* stream);

/* DISC LAYOUT of the half spectrum between the k_y pass and the last pass: only what FFTPower keeps.
 * FFTPower(mode="1d", kmin=k_F) drops every mode with |m| >= N/2 (power_spectrum_3d.py:189-195), so after the k_y pass a row
 * (k_y, 16-column k_z tile starting at k_z0) with k_y^2 + k_z0^2 > (N/2)^2 holds nothing any shell takes (the edge itself
 * stays: under AST_BIN_FLOAT64 a vector of norm exactly N/2 may fall into the last shell) - 21.5 % of the half plane.
 * The k_y rows are dealt to `parts` owners in blocks of r1 rows (32 at n = 1024, else 16), balanced by the area of the disc
 * they cover (contiguous ranges would leave the owners of the rows around k_y = 0 with full planes); a part's plane holds,
 * tile by tile, its rows that reach into the disc, 16 complex each.  The slab transpose sends these planes (pmesh transposes
 * inside the reference's one FFTPower call; nothing in the reference corresponds to the layout).  fp32, n in {256, 512,
 * 1024}, parts dividing n / r1.
 *   ast_fft_tile_disc_layout: plane_elems[parts] = complex elements per plane of each part, block_part[n / r1] = owner of
 *     every row block (or NULL), *r1_out = rows per block.  Host arithmetic only.
 *   ast_fft_tile_disc_table: the table [tile][row block] x (offb, S, cumS, lo | hi << 8 | part << 16) as int32 (host).
 *   ast_fft_tile_c2c_disc: the k_y pass of planes_d ((nplanes, n, pitch) complex, left intact) storing part q's rows of
 *     plane b at packed_d + nplanes * cumS[q] + b * S[q], the part self_part at self_out_d + b * S[self_part] (its place in
 *     the rank's own block; self_part < 0 and self_out_d NULL: none; packed_d may be NULL when parts == 1).
 *   ast_fft_tile_disc_block_power: the last pass over part `part`'s block ((n, S[part]) complex) fused with the shell
 *     binning, psum_d[shell] += L^3 sum w |scale * X|^2; shells below first_bin are skipped. */
int ast_fft_tile_disc_layout(size_t n, int parts, unsigned* plane_elems, unsigned char* block_part, int* r1_out);
int ast_fft_tile_disc_table(size_t n, int parts, int* out, size_t out_ints);
int ast_fft_tile_c2c_disc(const void* planes_d, void* packed_d, int dtype, size_t n, size_t pitch, size_t nplanes, int parts,
                          int self_part, void* self_out_d, double scale, void* stream);
size_t ast_fft_tile_disc_power_scratch_bytes(size_t n, int parts);
int ast_fft_tile_disc_block_power(void* block_d, void* scratch_d, size_t scratch_bytes, int dtype, size_t n, int parts, int part,
                                  double scale, double boxsize, int first_bin, int binning, double* psum_d, void* stream);

/* ------------------------------------------------------------- communication (ast_comm_init, ast_slab_transpose)
 * The multi-GPU exchange steps for a caller that binds this library alone: RCCL over xGMI, one process per GPU.  (The
 * Python side of this repository reaches RCCL through torch.distributed and does not call these.)  RCCL is loaded lazily
 * at the first call; the library has no link-time dependency on it.  The reference has no counterpart: pmesh / pfft
 * transpose over MPI inside the one FFTPower call (power_spectrum_3d.py:189-195).
 *   ast_comm_unique_id: 128 bytes from ncclGetUniqueId on ONE rank, to be handed to the others by the caller's own means.
 *   ast_comm_init / ast_comm_destroy: a communicator of `nranks` ranks for the current device.
 *   ast_slab_transpose: one group of point-to-point operations - to every peer q send_count[q] REAL elements of `dtype`
 *     (a complex value is two) from send_d + send_offset[q], from every peer recv_count[q] into recv_d + recv_offset[q];
 *     a piece addressed to the rank itself is copied on the stream.  With the disc layout of ast_fft_tile_c2c_disc for
 *     `nplanes` local planes: send_offset[q] = 2 nplanes cumS[q], send_count[q] = 2 nplanes S[q]; recv_offset[q] =
 *     2 (q nloc + p0) S[rank], recv_count[q] = 2 nplanes S[rank].  Asynchronous on `stream`.
 *   ast_comm_allreduce_sum: in-place sum of float64 values over the ranks (shell sums, low-k modes). */
typedef struct ast_comm ast_comm;
int ast_comm_unique_id(void* id_out, size_t id_bytes);
int ast_comm_init(ast_comm** out, int nranks, int rank, const void* id, size_t id_bytes);
int ast_comm_destroy(ast_comm* comm);
int ast_slab_transpose(ast_comm* comm, const void* send_d, const size_t* send_offset, const size_t* send_count, void* recv_d,
                       const size_t* recv_offset, const size_t* recv_count, int dtype, void* stream);
int ast_comm_allreduce_sum(ast_comm* comm, double* buf_d, size_t count, void* stream);

/* The low-k channel as separate calls, for slab-decomposed grids: every rank adds the contribution of its own
 * planes to the (2*6+1)^2 * 7 modes |m_i| <= 6, m_z >= 0 (complex128, [kx + 6][ky + 6][kz]); the modes are summed over
 * ranks; the sums of the ast_lowk_shell_count() lowest shells are then taken from them.
 *   planes_d: nx complete planes (x0 .. x0 + nx - 1 of the global axis 0) of n x n fp32 cells; n in {256, 512, 1024}.
 *   work_d: ast_lowk_work_bytes(n, nx) bytes.  accumulate: add into modes_d instead of overwriting it. */
size_t ast_lowk_work_bytes(size_t n, size_t nx);
int ast_lowk_mode_count(void);
int ast_lowk_shell_count(void);
int ast_lowk_modes(const void* planes_d, int dtype, size_t n, size_t x0, size_t nx, int accumulate, void* modes_d,
                   void* work_d, size_t work_bytes, void* stream);
/* The same from z sums that ast_fft_tile_rows_r2c_lowz has already left at the START of work_d ([plane][y][kz] for the
 * nx planes x0 .. x0 + nx - 1, any plane ranges in any order): the y and x sums only, no read of the planes. */
int ast_lowk_modes_from_z(size_t n, size_t x0, size_t nx, int accumulate, void* modes_d, void* work_d, size_t work_bytes,
                          void* stream);
/* sums_d[s] = L^3 sum w |modes / n^3|^2 over the modes of shell s (membership by `binning`), s < ast_lowk_shell_count(). */
int ast_lowk_shell_sums(const void* modes_d, size_t n, double boxsize, int binning, double* sums_d, void* stream);

/* ---------------------------------------------- a-5: k-shell power binning */

/* FFTPower(mode="1d", dk = kmin = 2 pi / L) shell sums over a block of the
 * half spectrum.  Replaces nbodykit project_to_basis as reached from
 * power_spectrum_3d.py:189-224 and stats_subfind.py:142-150.
 *   spec1_d, spec2_d: interleaved complex, dims (i0_count, i1_count,
 *       nmesh/2+1), C order, holding pmesh-normalised delta_k (spec2_d NULL =
 *       auto spectrum).  Global integer frequencies of the first two axes
 *       start at i0_start / i1_start (single GPU: 0, nmesh, 0, nmesh).
 *   ksum_d, psum_d (double) and nmodes_d (int64), nmesh/2-1 bins each, are
 *       ACCUMULATED into (caller zero-fills):  sum w |k|,
 *       sum w Re(d1 conj(d2)) L^3,  sum w,  with Hermitian weight w = 2 for
 *       0 < i2 < nmesh/2 else 1.  Shell of a mode: floor(|m|) - 1; the DC mode and |m| >= nmesh/2
 *       are dropped.
 *   binning: how lattice vectors of EXACTLY integer norm (perfect-square |m|^2, which sit on a shell
 *       edge) are assigned.  AST_BIN_INTEGER: to the shell they open, floor(|m|) - 1 (exact integer
 *       arithmetic, independent of L).  AST_BIN_FLOAT64: as nbodykit's float64 expressions round -
 *       digitize(kx^2 + ky^2 + kz^2, kedges^2) with k_i = (2 pi / L) m_i, kedges = arange(k_F, ..., k_F) -
 *       which puts some of them one shell lower (and some |m| = nmesh/2 vectors into the last shell),
 *       depending on L; this is the reference's behaviour as far as nbodykit's published source fixes it
 *       (nbodykit is un-vendored: parity unpinned).  All other vectors are unaffected.
 *   k = ksum/nmodes, P = psum/nmodes is left to the caller so that slab
 *       partials can be summed first.
 *   ksum_d / nmodes_d depend only on (nmesh, L, block), not on the data: pass
 *       both NULL to skip them (callers cache them), or spec1_d = psum_d = NULL
 *       to compute only them. */
int ast_power_bin_1d(const void* spec1_d, const void* spec2_d, int dtype, int nmesh,
                     double boxsize, int i0_start, int i0_count, int i1_start, int i1_count,
                     double* ksum_d, double* psum_d, long long* nmodes_d, int binning, void* stream);

/* FFTPower(mode="2d", Nmu, los, poles): (k, mu) wedge sums and Legendre multipole sums over the same block of the
 * half spectrum, with the line of sight along box axis `los` (0, 1 or 2).  nbodykit's published semantics restated
 * (un-vendored: parity unpinned); nothing in the reference computes it (power_spectrum_3d.py:189 asks for "1d").
 *   Lattice, k shell, dropped modes, Hermitian weight w and `binning`: exactly ast_power_bin_1d's; `binning` touches
 *       the k shell only.  nb = nmesh/2-1 shells.
 *   mu = |m_los| / |m|, folded onto [0, 1] (auto spectra, real part of cross spectra).  nmu (1 .. 1024) uniform bins,
 *       left-closed, mu = 1 in the last.  Membership in exact integer arithmetic:
 *       j = min(nmu - 1, max{ j : j^2 |m|^2 <= nmu^2 m_los^2 }) - a vector with mu exactly on an edge (3-4-5 triples:
 *       mu = 3/5 at nmu = 5) opens the bin it sits on.  nbodykit digitizes a float64 mu; only such on-edge vectors
 *       could land differently there.
 *   ksum_d, musum_d (double) and nmodes_d (int64), (nb, nmu) each:  sum w |k|, sum w mu, sum w.  Data independent:
 *       all three NULL skips them; spec1_d = psum_d = polesum_d = NULL computes only them.
 *   psum_d (nb, nmu): sum w Re(d1 conj(d2)) L^3.
 *   polesum_d (npoles, nb): row q = sum over ALL modes of the 1-D shell of w Re(d1 conj(d2)) L^3 L_l(mu), l = poles[q]
 *       (host array; distinct even values from {0, 2, 4, 6, 8} - the folded spectrum holds no odd multipole), mu in
 *       double, L_l by the three-term recurrence.  P_l = (2 l + 1) polesum / sum_shell w is left to the caller.
 *   Everything is ACCUMULATED into caller-zeroed buffers, so partials over (i0, i1) blocks and ranks add.
 *   The data pass sums in a workgroup's LDS table of (nb + 2)(nmu + npoles) doubles when that fits a CU's 160 KiB
 *       (ast_power_bin_2d_lds_fits = 1), else straight into the global tables with fp64 atomics; the environment
 *       variable ASTRILD_PK2D_LDS=0 forces the latter. */
int ast_power_bin_2d_lds_fits(int nmesh, int nmu, int npoles);
int ast_power_bin_2d(const void* spec1_d, const void* spec2_d, int dtype, int nmesh, double boxsize,
                     int i0_start, int i0_count, int i1_start, int i1_count, int los, int nmu,
                     const int* poles, int npoles, double* ksum_d, double* musum_d, long long* nmodes_d,
                     double* psum_d, double* polesum_d, int binning, void* stream);
/* Redshift-space positions: out = pos; out[:, los] += factor * vel[:, los], then ONE periodic wrap into [0, L)
 * (>= L: - L; < 0: + L, and a sum that rounds up to L becomes 0 - the result never equals L).  (np, 3) interleaved,
 * dtype AST_F32 / AST_F64, arithmetic in that dtype; factor 0.01 is TPCF's vel / 100 (particles/hutils/tpcf.py:74-97).
 * A shift of more than a box length leaves the coordinate outside [0, L): the caller decides (device.rsd_shift
 * raises).  out_d may alias pos_d. */
int ast_rsd_shift(const void* pos_d, const void* vel_d, int dtype, size_t np, int los, double factor, double boxsize,
                  void* out_d, void* stream);

/* --------------------------------------------------- a-10: bispectrum */

/* The reference's Bispectrum3D computes P(k) (bispectra/bispectrum_3d.py:165-215);
 * these two kernels carry the FFT (Scoccimarro) estimator its docstring cites
 * (:42-44): delta_i(x) = IFFT[delta_k 1(k in shell i)], I_i(x) = IFFT[1(k in i)],
 * B(i,j,l) = L^6 sum_x d_i d_j d_l / sum_x I_i I_j I_l.
 *
 * out = in * 1[m_lo <= |m| < m_hi] (or just the indicator when in_d is NULL),
 * exact integer comparison of |m|^2, over the same spectrum block layout as
 * ast_power_bin_1d. */
int ast_shell_filter(const void* in_d, void* out_d, int dtype, int nmesh, int m_lo, int m_hi,
                     int i0_start, int i0_count, int i1_start, int i1_count, void* stream);
/* I_s(x) = sum_{k in shell} e^{ikx} WITHOUT an inverse transform (bispectra/bispectrum_3d.py:42-44, the estimator's
 * triangle counts): the shell indicator m_lo <= |m| < m_hi on the full lattice as an (n, n, n) float64 array
 * (ast_shell_mask_real) is real and even, so its forward transform (ast_fft64_r2c_3d, scale 1) IS I_s on the half
 * lattice, real up to round-off; ast_half_real_to_full unfolds the real part onto the full (n, n, n) lattice. */
int ast_shell_mask_real(double* out_d, int nmesh, int m_lo, int m_hi, void* stream);
int ast_half_real_to_full(const void* spec_d, double* out_d, int nmesh, void* stream);

/* *out_d += sum_i a[i] * b[i] * c[i]  (double accumulator, device). */
int ast_triple_product_sum(const void* a_d, const void* b_d, const void* c_d, int dtype,
                           size_t count, double* out_d, void* stream);

/* out_d[t] = sum_i f[tri[3t]][i] * f[tri[3t+1]][i] * f[tri[3t+2]][i] for ntri <= 256 triangles over nfields device
 * arrays of `count` reals (fields_d: device array of nfields device pointers; tri_d: device int32 [ntri][3] of field
 * indices): every field is read ONCE (LDS-staged chunks), not once per triangle - the 75 cube sums of a 512^3
 * bispectrum (bispectrum_3d.py:42-44's estimator) in one pass.  Double products and sums in a fixed order
 * (deterministic).  scratch_d: ast_triple_product_sums_scratch_bytes() bytes.  nfields * 257 * sizeof(real) <= 160 KB. */
size_t ast_triple_product_sums_scratch_bytes(void);
int ast_triple_product_sums(const void* const* fields_d, int nfields, int dtype, size_t count, const int* tri_d,
                            int ntri, void* scratch_d, double* out_d, void* stream);

/* ------------------------------------------------- slab transpose helpers */

/* Pack the (n0, n1, n2) complex block so that the n1 axis is split into
 * `parts` equal chunks, each stored contiguously as (n0, n1/parts, n2):
 * the send layout of the slab all-to-all.  unpack is the inverse for the
 * receive side: `parts` blocks of (n0, n1, n2) -> one (parts*n0, n1, n2)
 * array is already contiguous, so only pack is needed on the way out and
 * this inverse on the way back (c2r). */
int ast_slab_pack(const void* in_d, void* out_d, int dtype, size_t n0, size_t n1, size_t n2,
                  int parts, void* stream);
int ast_slab_unpack(const void* in_d, void* out_d, int dtype, size_t n0, size_t n1, size_t n2,
                    int parts, void* stream);

/* ------------------------------------------------------ a-7: kappa stack */

/* out[i] = sum_p planes[p][i] * wnum[p] / wden[p], added in plane order
 * p = 0..nplanes-1 exactly like the reference's running `+=`
 * (rays/rayramses.py:224-232, simcoll.py:322-336) with the lensing-kernel
 * re-weighting quantity * g(x_mid, x_s') / g(x_mid, x_s) of
 * rayramses.py:306-312 / simcoll.py:424-430.  planes_d: device array of
 * nplanes device pointers; wnum_d / wden_d: device doubles or NULL (no
 * re-weighting).  fp64 results are bit-identical to numpy.  aligned16 != 0: the caller
 * promises that every plane pointer is 16-byte aligned (the pointers live on the device and are
 * not inspected); the kernel then moves 16 bytes per lane when `count` divides evenly. */
int ast_kappa_stack(const void* const* planes_d, const double* wnum_d, const double* wden_d,
                    int nplanes, size_t count, int dtype, void* out_d, int aligned16, void* stream);

/* --------------------------------------- a-8 / a-9: per-map kappa pipeline */

typedef struct ast_lens_plan ast_lens_plan;

/* Plan for kappa -> (alpha1, alpha2) / phi on an nc x nc map of side bsz
 * [rad]: owns the (2nc)^2 rocFFT plans, the padded work arrays and the cached
 * spectra of the isotropic kernels of lensing_funcs.c:45-83,117-148. */
int ast_lens_plan_create(ast_lens_plan** plan, int nc, double bsz);
int ast_lens_plan_destroy(ast_lens_plan* plan);
/* FFTPower of an in-memory float64 grid (the reference's dtype: power_spectrum_3d.py:183-224 on float64 arrays) for
 * n = 128 ... 2048 (powers of two) through hand-written double-precision passes (z rows, then ONE strided pass per axis, the last
 * one fused with the shell binning): psum_d[shell] += L^3 sum_modes w |delta_k|^2, delta_k = rfftn(grid) / n^3.
 * grid_d is not modified; scratch_d: ast_fft64_power_scratch_bytes(n) bytes. */
int ast_fft64_supported(size_t n);
size_t ast_fft64_power_scratch_bytes(size_t n);
int ast_fft64_power_3d(const double* grid_d, void* scratch_d, size_t scratch_bytes, size_t n, double boxsize, int binning,
                       double* psum_d, void* stream);
/* ast_fft64_power_3d of a SINGLE-precision grid, transformed in double (the z pass widens the rows as it loads them): fp32
 * cubes the fp32 tile passes do not cover (n = 128, 2048) without a float64 copy of the grid.  Same scratch. */
int ast_fft64_power_3d_f32(const float* grid_d, void* scratch_d, size_t scratch_bytes, size_t n, double boxsize, int binning,
                           double* psum_d, void* stream);
/* The same shell sums for a SINGLE-precision cube of side 2048 with every pass in single precision (three register FFTs
 * per axis; the fp32 tile passes end at 1024): psum_d[shell] += L^3 sum w |rfftn(grid - mean) / n^3|^2, FFTPower's sums
 * (power_spectrum_3d.py:189-224).  `mean` is subtracted as the rows are loaded (only the discarded DC mode sees it).  The
 * lowest shells carry fp32 round-off; callers patch them from ast_lowk_modes / ast_lowk_shell_sums (device.py does).
 * Half the bytes of ast_fft64_power_3d_f32 on every pass. */
int ast_fft32_big_supported(size_t n);
size_t ast_fft32_big_power_scratch_bytes(size_t n);
int ast_fft32_big_power_3d(const float* grid_d, void* scratch_d, size_t scratch_bytes, size_t n, double boxsize, int binning,
                           double mean, double* psum_d, void* stream);
/* ... of a grid painted with AST_PAINT_OVERWRITE | AST_PAINT_DEFER_FOLD: halo_rec_d (ast_paint_tiled_halo) is folded into the
 * border rows as the z rows and the low-k sums load them (the paint's fold kernel - 5 ms at side 2048 - is not run) */
int ast_fft32_big_power_3d_halo(const float* grid_d, const float* halo_rec_d, int window, void* scratch_d, size_t scratch_bytes,
                                size_t n, double boxsize, int binning, double mean, double* psum_d, void* stream);
/* spec_d (n, n, n / 2 + 1) complex double, contiguous = rfftn(grid_d) * scale (pmesh's r2c with scale = 1 / n^3) through
 * the same passes; grid_d is not modified */
int ast_fft64_r2c_3d(const double* grid_d, void* spec_d, size_t n, double scale, void* stream);
/* the same for a grid left by ast_paint_tiled(AST_PAINT_OVERWRITE | AST_PAINT_DEFER_FOLD): halo_rec_d
 * (ast_paint_tiled_halo) is folded into the border rows as the z pass loads them */
int ast_fft64_power_3d_halo(const double* grid_d, const double* halo_rec_d, int window, void* scratch_d, size_t scratch_bytes,
                            size_t n, double boxsize, int binning, double* psum_d, void* stream);

/* Column transforms of the zero-padded lens convolution (lensing_funcs.c:85-115 + fft_convolve.c:60-90), double,
 * hand-written two-pass (four-step) passes over data_d[len][pitch] complex that skip the half known to be zero.
 * len in {256 .. 8192}, powers of two (ast_lens_cols_supported).  The forward transform (in place) reads rows
 * < nonzero_rows only (len or len / 2) and leaves frequency k = k1 + N1 k2 at row N2 k1 + k2 (a fixed permutation;
 * spectra of one length are only ever multiplied with each other and transformed back).  The inverse
 * (unnormalised) transforms spec_d * mul_d (mul_d NULL: spec_d alone) into out_d and writes the first keep_rows rows
 * (len or len / 2), in natural order. */
int ast_lens_cols_supported(size_t len);
/* The row transforms of the same convolution for nc = 128 .. 4096, powers of two (ast_lens_rows_supported): forward - row r < nc of
 * spec_d (pitch complex per row) = the length-2nc R2C of (kappa_d[r][0 .. nc), nc zeros), kappa read unpadded
 * (zero_padding, lensing_funcs.c:8-19, never materialised); inverse - out_d[r][0 .. nc) = scale * the first nc reals of
 * the unnormalised length-2nc C2R of spec_d[r][0 .. nc] (corner_matrix, lensing_funcs.c:33-43, and the
 * 1 / (nx ny) dx dy of fft_convolve.c:88 in the store). */
int ast_lens_rows_supported(size_t nc);
int ast_lens_rows_forward(const double* kappa_d, size_t nc, void* spec_d, size_t pitch, void* stream);
/* The same for FULL rows of 2 nc reals (no zero padding), nrows of them with pitch 2 nc: the rows of the convolution
 * kernels (lensing_funcs.c:45-83), so that a lens plan of a supported size runs without rocFFT. */
int ast_lens_rows_forward_full(const double* in_d, size_t nc, size_t nrows, void* spec_d, size_t pitch, void* stream);
int ast_lens_rows_inverse(const void* spec_d, size_t pitch, size_t nc, double scale, double* out_d, void* stream);
int ast_lens_cols_forward(void* data_d, size_t len, size_t pitch, size_t ncols, size_t nonzero_rows, void* stream);
int ast_lens_cols_inverse(const void* spec_d, const void* mul_d, void* out_d, size_t len, size_t pitch, size_t ncols,
                          size_t keep_rows, void* stream);
/* The whole column part of a convolution with nmul (1 or 2) kernel spectra mul_d[m] (permuted order, as
 * ast_lens_cols_forward leaves them): out_d[m] = the first keep_rows rows of IFFT_cols(FFT_cols(data_d) * mul_d[m]),
 * unnormalised, natural order.  data_d is overwritten (forward pass A in place); the second forward pass, the products
 * and the first inverse pass are one kernel, so the spectrum of data_d never goes to memory (3 array passes fewer for
 * kappa -> alpha1, alpha2 than forward + 2 x inverse).  muls / outs are host arrays of device pointers. */
int ast_lens_cols_convolve(void* data_d, size_t len, size_t pitch, size_t ncols, size_t nonzero_rows, const void* const* muls,
                           void* const* outs, int nmul, size_t keep_rows, void* stream);

/* Device-pointer variants (fp64, C-contiguous nc*nc). */
int ast_kappa_to_alphas(ast_lens_plan* plan, const double* kappa_d, double* alpha1_d,
                        double* alpha2_d, void* stream);
int ast_kappa_to_phi(ast_lens_plan* plan, const double* kappa_d, double* phi_d, void* stream);

/* libglsg.so-compatible entry points (rays/skys/lib_so_cgls/lensing_funcs.h:5,7;
 * bound by ctypes at rays/skys/sky_utils.py:402-435): HOST pointers,
 * caller-allocated outputs, synchronous, void return like the original. */
void kappa0_to_alphas(double* kappa0, int Nc, double bsz, double* alpha1, double* alpha2);
void kappa0_to_phi(double* kappa0, int Nc, double bsz, double* phi);

typedef struct ast_smooth_plan ast_smooth_plan;

/* Gaussian smoothing of an npix x npix fp64 map (Filters.gaussian,
 * rays/utils/filters.py:181-225 -> lenstools ConvergenceMap.smooth):
 *   mode 0 "gaussianFFT": irfft2(exp(-0.5 l^2 (2 pi sigma_px)^2) rfft2(img)),
 *          l from (r)fftfreq(npix) — periodic.
 *   mode 1 "gaussian": separable real-space kernel, reflect boundary,
 *          truncate 4 sigma (scipy.ndimage.gaussian_filter).
 *   mode 2: as mode 1 with scipy's "mirror" boundary (d c b | a b c d | c b a, the edge
 *          pixel not repeated) - what skimage.transform.resize(mode="reflect", numpy's
 *          naming) hands to ndimage for its anti-aliasing prefilter (SkyArray.resize,
 *          rays/skys/sky_array.py:475-496).
 * In place on img_d. */
int ast_smooth_plan_create(ast_smooth_plan** plan, int npix);
int ast_smooth_plan_destroy(ast_smooth_plan* plan);
int ast_gaussian_smooth(ast_smooth_plan* plan, double* img_d, double sigma_px, int mode,
                        void* stream);

/* Flat-sky angular power spectrum binning (power_spectra/angular_power_spectrum.py:38-53 -> lenstools
 * ConvergenceMap.powerSpectrum, restated): ft1_d / ft2_d (or NULL = auto) are rfft2 half planes (npix x (npix/2+1),
 * complex128, unnormalised); pixel (i, j) has |l| = 2 pi / angle * sqrt(min(i, npix-i)^2 + j^2) and falls into bin k
 * when edges[k] < |l| <= edges[k+1].  psum_d[k] += sum Re(ft1 conj ft2), hits_d[k] += pixels (device uint64);
 * P(k) = psum / hits * (angle / npix^2)^2 on the host.  edges_d: nbins + 1 doubles on the device, ascending. */
int ast_flat_power_bin(const void* ft1_d, const void* ft2_d, int npix, double angle_rad, const double* edges_d,
                       int nbins, double* psum_d, unsigned long long* hits_d, void* stream);
/* out = in * 1[l_lo < |l| <= l_hi] on the same half plane (in_d = NULL: the indicator itself) - the ring fields of the
 * FFT estimator of the equilateral flat-sky bispectrum (bispectra/bispectrum_2d.py:33-50). */
int ast_ring_filter_2d(const void* in_d, void* out_d, int npix, double angle_rad, double l_lo, double l_hi, void* stream);

/* Gaussian random fields with a given flat-sky power spectrum (SkyArray.create_cmb / add_cmb,
 * rays/skys/sky_array.py:709-777; the reference's NaMaster synfast_flat call is commented out, this is the project's own
 * generator).  Fills nreal half-plane spectra, complex128, npix x (npix/2+1) row-major, one after the other in spec_d:
 * the layout of the rfft2 above and of the C2R plan, whose numpy-convention inverse (1 / npix^2) is the map, with
 * <|rfft2(map)|^2> (angle / npix^2)^2 = C(l), what ast_flat_power_bin measures.  Every slot is written; no scratch.
 * Pixel (i, j) of realisation R = first_realisation + r, n = npix, nh = n/2 + 1, fp64 op by op:
 *   l = (2 pi / angle) sqrt((double)(m^2 + j^2)), m = min(i, n - i);  cl_d[0 .. ncl-1] is C at integer l = 0 .. ncl-1;
 *   k = floor(l), t = l - k, C = cl[k] + t (cl[min(k+1, ncl-1)] - cl[k]), C = 0 where l > min(lmax, ncl-1);
 *   A = sqrt(C) s, s = (n n) / angle.
 *   Columns j = 0 and (n even) j = n/2 are self-conjugate: there ic = min(i, (n-i) mod n), elsewhere ic = i.
 *   (w0, w1, w2, w3) = Philox4x32-10(counter = (c lo, c hi, R lo, R hi), key = (seed lo, seed hi)), c = ic nh + j (64 bit);
 *   u1 = (((w0 >> 5) 2^26 + (w1 >> 6)) + 1) 2^-53, u2 = ((w2 >> 5) 2^26 + (w3 >> 6)) 2^-53 (both exact);
 *   r = sqrt(-2 log(u1)), phi = (2 pi) u2, a = r cos(phi), b = r sin(phi).
 *   A self-conjugate pixel with i = (n-i) mod n gets (A a, 0); every other pixel ((A a) / sqrt(2), (A b) / sqrt(2)), the
 *   imaginary part negated where i > (n-i) mod n in a self-conjugate column; A = 0 gives exactly (0, 0).
 * The result is bit-identical from call to call and for any launch shape.  Refused before any launch: a null pointer,
 * npix < 2, angle_rad not positive and finite, ncl < 1, nreal < 1, lmax NaN (+inf = no cut). */
int ast_grf_spectrum(void* spec_d, int npix, double angle_rad, const double* cl_d, int ncl, double lmax,
                     unsigned long long seed, unsigned long long first_realisation, int nreal, void* stream);

/* Local maxima of an npix x npix map (SkyArray.wl_peak_counts, rays/skys/sky_array.py:435-472 ->
 * lenstools ConvergenceMap.locatePeaks): interior pixels strictly larger than their 8 neighbours with a
 * value in [lo, hi).  Heights go to values_d (dtype), flat row-major pixel indices to index_d, at most
 * `cap` of each; *count_d (device uint64) receives the number FOUND (may exceed cap).  The order in the
 * output arrays is not defined (sort by index for lenstools' scan order). */
int ast_peak_find(const void* img_d, int dtype, int npix, double lo, double hi, size_t cap, void* values_d,
                  long long* index_d, unsigned long long* count_d, void* stream);

/* Exact order statistics: out_host[j] = the ks_host[j]-th smallest element (0-based) of buf_d - what
 * np.percentile interpolates between (sky_array.py:452-457).  Radix select on order-preserving keys, six
 * passes over the buffer per k; SYNCHRONOUS (host arrays in and out).  scratch_d: 2048 uint64 on the device. */
int ast_order_statistics(const void* buf_d, int dtype, size_t count, const size_t* ks_host, int nk,
                         double* out_host, unsigned long long* scratch_d, void* stream);

/* Sum of a buffer in double, fixed summation order (bit-reproducible): out_d[0]; out_d must hold
 * 1 + AST_SUM_PARTS doubles (the rest is scratch). */
#define AST_SUM_PARTS 1024
int ast_sum(const void* buf_d, int dtype, size_t count, double* out_d, void* stream);

/* min and max of a buffer -> out_d[0], out_d[1] (double, device). */
int ast_minmax(const void* buf_d, int dtype, size_t count, double* out_d, void* stream);

/* The paint's mass bound, in the same single pass: out_d[1] = max |x| and out_d[0] = 0.0 when every element is
 * finite, -1.0 when at least one is NaN or +-Inf (then out_d[1] skips the NaNs and is Inf if an Inf is among them). */
int ast_absmax_finite(const void* buf_d, int dtype, size_t count, double* out_d, void* stream);

/* np.histogram(data, bins=nbins, range=(lo, hi)) counts: uniform bins,
 * right-most bin closed (SkyArray.pdf, rays/skys/sky_array.py:428-433).
 * counts_d (int64, nbins) is ACCUMULATED into. */
int ast_histogram(const void* buf_d, int dtype, size_t count, double lo, double hi, int nbins,
                  long long* counts_d, void* stream);

/* np.histogram(buf, bins=nbins) with range=None (sky_array.py's PDF calls) without a host round trip between the
 * min/max pass and the counting pass: range_d[0..1] receives {min, max} (a degenerate range counts against
 * [min - 0.5, max + 0.5] like numpy), counts_d (zeroed by the caller) the bin counts. */
int ast_histogram_auto(const void* buf_d, int dtype, size_t count, int nbins, long long* counts_d, double* range_d,
                       void* stream);

/* out[i] = a[i] + b[i]  (add_galaxy_shape_noise, sky_array.py:693-706). */
int ast_add(const void* a_d, const void* b_d, void* out_d, int dtype, size_t count, void* stream);

/* ------------------------------------- f-2: analytic NFW halo signals (next row) */

/* Paint the deflection-angle (signal 0) or moving-lens temperature (signal 1) stamp
 * of every halo onto an npix x npix fp64 map, clipped at the map edge.  Replaces
 * SkyUtils.analytic_Halo_signal_to_SkyArray and the NFW_*_map / add_patch_to_map
 * helpers it loops over (rays/skys/sky_utils.py:79-282).  Per-halo device arrays:
 * r200 [deg], m200 [M_sun], concentration, angular diameter distance [Mpc] (the
 * reference passes Dc * 0.6774), transverse velocities [km/s] (signal 1 only), stamp
 * edge length int(2 * r200_pix * extent) + 1, stamp centre (theta1_pix = column,
 * theta2_pix = row).  dir_mask: bit 0 = direction 0 (x), bit 1 = direction 1 (y).
 * map_d is ACCUMULATED into. */
int ast_nfw_paint(const double* r200_deg_d, const double* m200_d, const double* c_nfw_d, const double* dist_d,
                  const double* vel_x_d, const double* vel_y_d, const int* stamp_npix_d, const int* cen_x_d,
                  const int* cen_y_d, size_t nhalo, double extent, int dir_mask, int suppress,
                  double suppression_r, int signal, double* map_d, int npix, void* stream);

/* limg[y, x] += simg[i, j] for the in-bounds part of a stamp centred at (cen_x, cen_y)
 * (SkyUtils.add_patch_to_map, sky_utils.py:140-173). */
int ast_add_patch(double* limg_d, int nl, const double* simg_d, int ns, int cen_x, int cen_y, void* stream);

/* --------------------------- f-3: flat-sky window filters (next row, first part) */

/* Filters.gaussian_third_derivative (order 3, "DGD3") and gaussian_first_derivative (order 1)
 * of rays/utils/filters.py:305-400: out = img * d^order/d(axis)^order W, W a sum of Gaussians of
 * the pixel distance to the map centre (sigma_pix = ceil(npix * theta_i / theta)), derivatives by
 * repeated np.gradient(.., h, edge_order=2) with h = theta_fov / npix.  work_d: 2 npix^2 doubles. */
int ast_dgd_filter(const double* img_d, double* out_d, double* work_d, int npix, double sigma_pix, double h,
                   int axis, int order, void* stream);

/* Filters.apodization (filters.py:150-178): img * outer(hann(npix), hann(npix)). */
int ast_hann_apodize(const double* img_d, double* out_d, int npix, void* stream);

/* SkyArray.resize (sky_array.py:475-496: skimage.transform.resize(img, (nout, nout), anti_aliasing=True), "lower the
 * nr. of pixels"), resampling half: scipy.ndimage.zoom(img, nout / nin, order=1, grid_mode=True) - bilinear samples at
 * (o + 1/2) nin / nout - 1/2 - for nout <= nin, fp64, out of place.  The anti-aliasing half is ast_gaussian_smooth
 * (mode 1, sigma = (nin / nout - 1) / 2) on the input first.  scikit-image is not pinned by the reference's lock file:
 * this is the algorithm of scikit-image >= 0.19 (Gaussian prefilter + ndimage.zoom), restated. */
int ast_zoom_linear(const double* img_d, int nin, double* out_d, int nout, void* stream);

/* SkyUtils.convert_deflection_to_shear (rays/skys/sky_utils.py:342-362, called by SkyArray.convert_deflection_to_shear,
 * sky_array.py:820-849): gamma1 = 0.5 ((1 - d0 alpha1) - (1 - d1 alpha2)), gamma2 = 0.5 (-d0 alpha2 - d1 alpha1) with
 * d0 / d1 = np.gradient along axis 0 / 1 (edge_order 1) at uniform spacing h.  The reference's body is unfinished (its
 * `coord` is undefined and the call site passes one array): h is the pixel size, opening_angle / npix, in the unit of
 * alpha.  npix x npix fp64 maps, out of place; bit-identical to the numpy expressions. */
int ast_deflection_to_shear(const double* alpha1_d, const double* alpha2_d, int npix, double h, double* gamma1_d,
                            double* gamma2_d, void* stream);

/* scipy.ndimage.gaussian_filter(img, sigma, order=(order0, order1), mode) as called by
 * Filters.gaussian_third_derivative_convolution (filters.py:260-304): mode 0 "reflect", 1 "nearest".
 * work_d: npix^2 + 2 (2 r + 1) doubles, r = int(4 sigma + 0.5). */
int ast_gaussian_filter_order(const double* img_d, double* out_d, double* work_d, size_t work_doubles, int npix,
                              double sigma, int order0, int order1, int mode, void* stream);

/* scipy.ndimage.convolve(img, window) with its defaults (reflect, origin 0), the last line of
 * Filters.gaussian_compensated (filters.py:415-459).  img_d != out_d. */
int ast_convolve2d(const double* img_d, const double* window_d, double* out_d, int npix, int kh, int kw,
                   void* stream);

/* Filters.aperture_photometry (filters.py:40-73): out = img - mean(img[alpha_pix < d < sqrt(2) alpha_pix]).
 * work_d: 2048 doubles. */
int ast_aperture_photometry(const double* img_d, double* out_d, double* work_d, int npix, double alpha_pix,
                            void* stream);

/* ------------------------------------------------- mean pairwise velocity */

/* Mean pairwise velocity from transverse velocities (Yasini et al. 2018), the estimator of
 * particles/hutils/mean_pairwise_velocity.py: mean_pv_from_tv (:16-118) with the pair loop of pairwise_one_row
 * (:121-176), and the BallTree pair finder of particles/utils_cython/pairwise_velocity.pyx.  No object cap (the
 * reference asserts N <= 50000).  Two calls on one workspace of ast_pairwise_workspace_bytes(n, binnr) bytes
 * (0: binnr outside 1..ast_pairwise_max_bins()):
 *
 * ast_pairwise_tv_prepare: per object, in fp64, r (pos_d (n, 3), pos_dtype widened), u = r / |r| and the cartesian
 * transverse velocity t = J^T (0, v1, v2), J = get_sph_to_cart_jacobian(th = theta2, ph = theta1)
 * (utils/geometrical_transforms.py:94-105), from vel_d (n, 2), vel_dtype; vel_ncomp = 3: vel_d is t itself (n, 3).
 * angle_mode 0: theta1 = arctan(x / z), theta2 = arctan(y / z) (angular_coordinate_in_lc), both + 10 deg, as the
 * reference does; 1: theta1_d / theta2_d (fp64, n) in radians; 2: in degrees.  Also the bounding box of r.
 *
 * ast_pairwise_tv: for every pair i != j with b = int(|r_i - r_j| / binwidth) < binnr (binnr = len(bins), the
 * reference's count, reach binnr * binwidth), with p = (r_i - r_j) / |r_i - r_j| and
 * q = (2 p - u_i (p.u_i) - u_j (p.u_j)) / 2:  nom_d[b] += (t_i - t_j).q, denom_d[b] += q.q, counts_d[b] += 1
 * (outputs are written, not accumulated; all zero for n < 2).  Coincident objects add NaN to bin 0, like the
 * reference.  Pair finder: a uniform cell grid of cells >= the reach over the bounding box (non-periodic);
 * single_cell != 0 forces one cell (all pairs).  The sums are not bit-reproducible from call to call (LDS atomics);
 * the counts are exact.  n < 2^31. */
size_t ast_pairwise_workspace_bytes(size_t n, int binnr);
int ast_pairwise_max_bins(void);
int ast_pairwise_tv_prepare(const void* pos_d, int pos_dtype, const void* vel_d, int vel_dtype, int vel_ncomp,
                            const double* theta1_d, const double* theta2_d, int angle_mode, size_t n, void* work_d,
                            size_t work_bytes, void* stream);
int ast_pairwise_tv(void* work_d, size_t work_bytes, size_t n, int binnr, double binwidth, int single_cell,
                    double* nom_d, double* denom_d, unsigned long long* counts_d, void* stream);

/* ------------------------------------------------- pairwise-velocity histograms */

/* The (separation bin, velocity bin) pair counts of particles/utils_cython/pairwise_velocity.pyx: mean_pv_z_sign
 * (:194-253) and mean_pv_radial (:256-313).  For every unordered pair of original indices i < j, in fp64 and op by
 * op, with the differences taken j - i:  d = sqrt((dx dx + dy dy) + dz dz); the pair is seen when d <= R,
 * R = (double)(float)r (the reference declares `float r`), and first <= i < second (the reference's chunking of its
 * i loop).  Its velocity is
 *   AST_PVPDF_Z_SIGN:  v12 = (vz_j - vz_i) sign(z_j - z_i)           (sign = -1, 0, +1)
 *   AST_PVPDF_RADIAL:  v12 = ((dvx dx + dvy dy) + dvz dz) / d         (mean_pv_radial does not run as shipped; this is
 *                                                                     z_sign's rule with the radial velocity)
 * and, rounded to float32 as the reference's `cdef float diff, dist`, ds = (float)(d / dist_width) and
 * vs = (float)(v12 / vel_width + vel_bin / 2) (integer division).  The pair adds 1 to hist_d[a * vel_bin + b],
 * a = (int)ds, b = (int)vs, when a < dist_bin and 0 <= vs < vel_bin; every other seen pair (NaN from coincident
 * objects included) adds 1 to *outside_d, the reference's rubbish_counter - also where the reference raises
 * IndexError (vs == vel_bin, a == dist_bin).  With the widths 1 this is the reference's own rule.
 * Moments (s1_d, s2_d, mcount_d all given, dist_bin entries each; all NULL: none): over the seen pairs of row
 * a < dist_bin with finite v12, whatever vs is, sum v12, sum v12^2 and their number.
 * All outputs are written, not accumulated; all zero for n < 2 or first == second.  hist_d, *outside_d and mcount_d
 * are exact and the same from call to call; s1_d / s2_d are fp64 sums in no fixed order (LDS atomics per wave, then
 * fixed-order sums of the waves and workgroups - no global float atomics).
 *
 * Two calls on one workspace of ast_pairwise_pdf_workspace_bytes(n, dist_bin, vel_bin, moments) bytes (0: a bin count
 * below 1, dist_bin * vel_bin > ast_pairwise_pdf_max_bins(), or moments with dist_bin > AST_PVPDF_MAX_MOMENT_ROWS):
 * ast_pairwise_pdf_prepare (pairwise_velocity.pyx:194-313: the arrays ppos, vvel) widens pos_d, vel_d (n, 3) to fp64,
 * keeps the original index and takes the bounding box; ast_pairwise_pdf (pairwise_velocity.pyx:194-313: the pair
 * loops) sorts the objects into a cell grid of cells >= R over the bounding box (non-periodic; single_cell != 0: one
 * cell, all pairs) and counts.  Histograms of up to ast_pairwise_pdf_lds_bins(dist_bin, moments) counters are
 * counted in LDS (32-bit counters, flushed into hist_d with 64-bit integer atomics before they could overflow);
 * larger ones, or any with force_global != 0, take one 64-bit integer atomic on hist_d per counted pair.  Both
 * paths give the same counts.  n < 2^31. */
#define AST_PVPDF_Z_SIGN 0
#define AST_PVPDF_RADIAL 1
#define AST_PVPDF_MAX_MOMENT_ROWS 480
/* pairwise_velocity.pyx:194-313 */
size_t ast_pairwise_pdf_workspace_bytes(size_t n, int dist_bin, int vel_bin, int moments);
/* pairwise_velocity.pyx:194-313: the largest dist_bin * vel_bin (at least 2^22) */
int ast_pairwise_pdf_max_bins(void);
/* pairwise_velocity.pyx:194-313: the largest dist_bin * vel_bin that is counted in LDS */
int ast_pairwise_pdf_lds_bins(int dist_bin, int moments);
/* pairwise_velocity.pyx:194-313 */
int ast_pairwise_pdf_prepare(const void* pos_d, int pos_dtype, const void* vel_d, int vel_dtype, size_t n, void* work_d,
                             size_t work_bytes, void* stream);
/* pairwise_velocity.pyx:194-313 */
int ast_pairwise_pdf(void* work_d, size_t work_bytes, size_t n, int kind, double r, int dist_bin, int vel_bin,
                     double dist_width, double vel_width, size_t first, size_t second, int single_cell,
                     int force_global, unsigned long long* hist_d, unsigned long long* outside_d, double* s1_d,
                     double* s2_d, unsigned long long* mcount_d, void* stream);

/* ------------------------------------------------- two-point correlation function */

/* Pair counts of the two-point correlation function of a periodic box: particles/hutils/tpcf.py (TPCF.compute /
 * TPCF.tpcf_s, :18-111), which calls halotools' s_mu_tpcf (and, commented out in halo.py / stats_subfind.py, its real-
 * space tpcf).  Two calls on one workspace of ast_tpcf_workspace_bytes(n, ns, nmu) bytes (0: ns outside 1..1000, nmu
 * outside 0..1000 or ns * max(nmu, 1) > ast_tpcf_max_bins()):
 *
 * ast_tpcf_prepare: per object, the redshift-space shift of tpcf.py:74-97 in the input dtypes, as numpy does it:
 * pos[los] += vel[los] / 100 (vel / 100 in vel_dtype, the add in the wider dtype, stored as pos_dtype), then
 * > boxsize -> - boxsize, < 0 -> + boxsize (in pos_dtype); vel_d == NULL: no shift and no wrap.  pos_d, vel_d (n, 3).
 * The shifted positions are widened to fp64 into the workspace, and bounds_d[6] receives their min (x, y, z) and
 * max (x, y, z) (NaN counts as out of range; (+inf, -inf) for n == 0) so the caller can check [0, boxsize].
 *
 * ast_tpcf_pair_counts: for every unordered pair i < j, with the minimum image a = min(|dx|, boxsize - |dx|) per
 * axis, d2 = (a_x^2 + a_y^2) + a_z^2 and mu = a_los / sqrt(d2) (fp64): the pair counts in bin (k, l) when
 * s_k^2 < d2 <= s_{k+1}^2 (s_edges_d: ns + 1 edges, squared in fp64) and mu_l < mu <= mu_{l+1} (mu_edges_d: nmu + 1
 * edges; nmu = 0: no mu test).  counts_d[k * max(nmu, 1) + l] (written, not accumulated; zero for n < 2) is exact for
 * n < 2^31.  Pair finder: a periodic cell grid of cells at least the top s edge wide, at least 3 per axis (one cell
 * when the top edge is >= boxsize / 3); single_cell != 0 forces one cell (all pairs, minimum image still applied). */
size_t ast_tpcf_workspace_bytes(size_t n, int ns, int nmu);
int ast_tpcf_max_bins(void);
int ast_tpcf_prepare(const void* pos_d, int pos_dtype, const void* vel_d, int vel_dtype, int los, double boxsize,
                     size_t n, void* work_d, size_t work_bytes, double* bounds_d, void* stream);
int ast_tpcf_pair_counts(void* work_d, size_t work_bytes, size_t n, double boxsize, int los, const double* s_edges_d,
                         int ns, const double* mu_edges_d, int nmu, int single_cell, unsigned long long* counts_d,
                         void* stream);

/* The same pair counts for two samples, in a periodic cube or with open boundaries: what halotools' tpcf / s_mu_tpcf
 * count for sample2= and randoms= (particles/hutils/tpcf.py; the reference's halo code correlates the two halves of a
 * mass-split catalogue that way, stats_subfind.py:155-218).  Two calls on one workspace of
 * ast_tpcf_cross_workspace_bytes(n1, n2, ns, nmu) bytes (0 for the bin counts ast_tpcf_workspace_bytes refuses):
 *
 * ast_tpcf_cross_prepare: ast_tpcf_prepare for each set, with dtypes of its own: the redshift-space shift along los
 * when velN_d != NULL, and boxsize > 0 the single wrap; boxsize == 0 means open boundaries (shift, no wrap).
 * bounds_d[12] receives min (x, y, z), max (x, y, z) of set 1, then of set 2 (NaN counts as -inf / +inf; (+inf, -inf)
 * for an empty set): the caller checks [0, boxsize], or that everything is finite.
 *
 * ast_tpcf_cross_counts: auto_pairs == 0: every pair (i of set 1, j of set 2) once; auto_pairs != 0: set 2 is
 * ignored and the unordered pairs i < j of set 1 are counted (with boxsize > 0 this is ast_tpcf_pair_counts; with
 * boxsize == 0 its open-boundary twin).  boxsize > 0: minimum image a = min(|dx|, boxsize - |dx|); boxsize == 0:
 * a = |dx|.  d2, mu, the bins (s_k^2 < d2 <= s_{k+1}^2, mu_l < mu <= mu_{l+1}; d2 = 0 never counts, so coincident
 * points of the two sets drop out) and counts_d are ast_tpcf_pair_counts'; counts are exact for n1, n2 < 2^31 and zero
 * when a set is empty (auto: n1 < 2).  Pair finder: one cell grid shared by both sets, each sorted on it: the periodic
 * grid of ast_tpcf_pair_counts, or for open boundaries a grid over the union bounding box with cells at least the top
 * s edge wide (1 cell on an axis without extent); single_cell != 0 forces one cell. */
size_t ast_tpcf_cross_workspace_bytes(size_t n1, size_t n2, int ns, int nmu);
int ast_tpcf_cross_prepare(const void* pos1_d, int pos1_dtype, const void* vel1_d, int vel1_dtype, size_t n1,
                           const void* pos2_d, int pos2_dtype, const void* vel2_d, int vel2_dtype, size_t n2, int los,
                           double boxsize, void* work_d, size_t work_bytes, double* bounds_d, void* stream);
int ast_tpcf_cross_counts(void* work_d, size_t work_bytes, size_t n1, size_t n2, int auto_pairs, double boxsize,
                          int los, const double* s_edges_d, int ns, const double* mu_edges_d, int nmu,
                          int single_cell, unsigned long long* counts_d, void* stream);

/* The pair counts of ast_tpcf_cross_counts together with what a leave-one-region-out jackknife needs (halotools'
 * tpcf_jackknife: a pair weighs 1 when neither end lies in the left-out region k, 1/2 when one does, 0 when both do):
 * every object carries a region tag in [0, nsub), and ends_d[k * nbins + b] is the number of pair ends in region k
 * over the counted pairs of bin b (a pair with both ends in k adds 2).  Then, as exact integers, the ordered auto
 * pairs (or twice the cross pairs) with region k left out are 2 counts[b] - ends[k][b], and sum_k ends[k][b] =
 * 2 counts[b].  Two calls on one workspace of ast_tpcf_jk_workspace_bytes(n1, n2, ns, nmu, nsub) bytes (0 for bins
 * that ast_tpcf_workspace_bytes refuses, nsub < 1 or nsub * nbins > ast_tpcf_jk_max_table()):
 *
 * ast_tpcf_jk_prepare: ast_tpcf_cross_prepare (shift, wrap, fp64 records, bounds_d[0..11]) plus the tag of every
 * object.  tagsN_d != NULL: int32 per object, copied; a value outside [0, nsub[0] nsub[1] nsub[2]) sets
 * bounds_d[12] = 1 (else 0) and is stored as region 0, so it is never an index past the table: the caller checks
 * bounds_d[12] before counting.  tagsN_d == NULL: from the SHIFTED position, i_a = floor((x_a - lo_a) / dl_a) with
 * dl_a = (hi_a - lo_a) / nsub_a (fp64, true divisions), clamped to [0, nsub_a - 1] on both sides (x = hi, a point
 * outside the volume and a NaN belong to a border region), tag = (i_x nsub_y + i_y) nsub_z + i_z.  nsub, lo, hi:
 * HOST pointers to 3 values each, nsub_a >= 1, lo / hi finite with hi_a >= lo_a.  bounds_d: 13 doubles.
 *
 * ast_tpcf_jk_counts: counts_d[nbins] as ast_tpcf_cross_counts (auto_pairs, boxsize, los, edges, bins and
 * single_cell as there) and ends_d[nsub * nbins], both written, not accumulated, and zero when there is no pair.  nsub
 * is the number of regions of the prepare call (a larger tag counts in the last region).  The table is counted in
 * 32-bit LDS counters while nsub * nbins <= ast_tpcf_jk_lds_table(ns, nmu) and force_global == 0, flushed into ends_d
 * with 64-bit integer atomics; else with 64-bit global atomics per pair end.  Integer sums: the same result either
 * way and from call to call. */
size_t ast_tpcf_jk_workspace_bytes(size_t n1, size_t n2, int ns, int nmu, int nsub);
int ast_tpcf_jk_max_table(void);
int ast_tpcf_jk_lds_table(int ns, int nmu);
int ast_tpcf_jk_prepare(const void* pos1_d, int pos1_dtype, const void* vel1_d, int vel1_dtype, const int* tags1_d,
                        size_t n1, const void* pos2_d, int pos2_dtype, const void* vel2_d, int vel2_dtype,
                        const int* tags2_d, size_t n2, int los, double boxsize, const int* nsub, const double* lo,
                        const double* hi, void* work_d, size_t work_bytes, double* bounds_d, void* stream);
int ast_tpcf_jk_counts(void* work_d, size_t work_bytes, size_t n1, size_t n2, int auto_pairs, double boxsize, int los,
                       const double* s_edges_d, int ns, const double* mu_edges_d, int nmu, int nsub, int single_cell,
                       int force_global, unsigned long long* counts_d, unsigned long long* ends_d, void* stream);

/* Pair counts in bins of (r_p, pi), the separation across and along a line of sight: what halotools' rp_pi_tpcf, wp
 * and their jackknife variants count (npairs_xy_z; the members of mock_observables beside the s_mu_tpcf that
 * particles/hutils/tpcf.py:7-9 imports).  The prepare calls and the workspaces do not depend on the geometry: each
 * count below runs on the workspace of its ast_tpcf_* twin, prepared by that twin's prepare call and sized by its
 * *_workspace_bytes with (nrp, npi) in place of (ns, nmu).
 *
 * With a < b the axes other than los, per pair and in fp64: p_c = |x_i[c] - x_j[c]|, with boxsize > 0 the minimum
 * image p_c = min(p_c, boxsize - p_c) (ast_tpcf_cross_counts' arithmetic, bit for bit); rp2 = p_a p_a + p_b p_b and
 * pi = p_los.  The pair counts in bin (k, l) when rp_k^2 < rp2 <= rp_{k+1}^2 (rp_edges_d: nrp + 1 edges, squared in
 * fp64 on the device) and pi_l < pi <= pi_{l+1} (pi_edges_d: npi + 1 edges, compared as given; npi >= 1).  So a pair
 * with pi on the lowest pi edge (pi = 0 when that edge is 0) or rp2 on the lowest r_p edge squared is in no bin, and
 * coincident points never count.  counts_d[k * npi + l], written, not accumulated; exact for n < 2^31.  Limits as
 * ast_tpcf_workspace_bytes: at most 1000 bins per axis and nrp * npi <= ast_tpcf_max_bins().
 *
 * Pair finder: the cell grid of the twin with cells of a width per axis.  plan == 0: the reach is the top pi edge
 * along los and the top r_p edge across.  Periodic: floor(boxsize / (reach (1 + 1e-6))) cells on an axis, at most
 * 1024, and 1 where that is fewer than 3 (the minimum image then finds the pairs of that axis); fewer cells on every
 * axis while the grid exceeds the workspace's cell capacity.  Open: the twin's rule over the bounding box, per axis.
 * plan == 1: the isotropic grid of ast_pairvel_moments' AST_PAIRVEL_LOS, cells of sqrt(rp_top^2 + pi_top^2) on every
 * axis.  single_cell != 0 forces one cell.  The counts do not depend on the plan.
 *
 * ast_rppi_pair_counts, ast_rppi_cross_counts, ast_rppi_jk_counts: all other arguments, the outputs (counts_d, and
 * ends_d[nsub * nrp * npi] of the jackknife) and the early returns are those of ast_tpcf_pair_counts,
 * ast_tpcf_cross_counts and ast_tpcf_jk_counts. */
/* halotools rp_pi_tpcf / wp for one sample in a periodic box (particles/hutils/tpcf.py:7-9) */
int ast_rppi_pair_counts(void* work_d, size_t work_bytes, size_t n, double boxsize, int los, const double* rp_edges_d,
                         int nrp, const double* pi_edges_d, int npi, int single_cell, int plan,
                         unsigned long long* counts_d, void* stream);
/* halotools rp_pi_tpcf / wp with sample2= or randoms=, periodic or open (particles/hutils/tpcf.py:7-9) */
int ast_rppi_cross_counts(void* work_d, size_t work_bytes, size_t n1, size_t n2, int auto_pairs, double boxsize,
                          int los, const double* rp_edges_d, int nrp, const double* pi_edges_d, int npi,
                          int single_cell, int plan, unsigned long long* counts_d, void* stream);
/* halotools rp_pi_tpcf_jackknife / wp_jackknife (particles/hutils/tpcf.py:7-9) */
int ast_rppi_jk_counts(void* work_d, size_t work_bytes, size_t n1, size_t n2, int auto_pairs, double boxsize, int los,
                       const double* rp_edges_d, int nrp, const double* pi_edges_d, int npi, int nsub, int single_cell,
                       int force_global, int plan, unsigned long long* counts_d, unsigned long long* ends_d,
                       void* stream);

/* ------------------------------------------------- pairwise-velocity moments of one or two samples in a box */

/* Count, sum v and sum v^2 per separation bin of the pairwise velocity of one or two samples, in a periodic cube or
 * with open boundaries: what halotools' mean_radial_velocity_vs_r / radial_pvd_vs_r / mean_los_velocity_vs_rp /
 * los_pvd_vs_rp accumulate (the reference's commented-out SubFind.mean_pairwise_velocity, stats_subfind.py:155-218,
 * asks the first of them for the two halves of a mass-split catalogue).  Two calls on one workspace of
 * ast_pairvel_workspace_bytes(n1, n2, nb) bytes (0 for nb < 1 or nb > ast_pairvel_max_bins() = AST_PAIRVEL_MAX_BINS):
 *
 * ast_pairvel_prepare (stats_subfind.py:155-218): positions and velocities of each set, (n, 3) each and each AST_F32
 * or AST_F64, are widened exactly to fp64 (no redshift-space shift, no wrap).  bounds_d[12] receives min (x, y, z),
 * max (x, y, z) of set 1, then of set 2 (NaN counts as -inf / +inf; (+inf, -inf) for an empty set): the caller checks
 * [0, boxsize], or that everything is finite.  n2 == 0 with NULL pointers for the auto term.
 *
 * ast_pairvel_moments (stats_subfind.py:155-218): auto_pairs == 0: every pair (i of set 1, j of set 2) once;
 * auto_pairs != 0: set 2 is ignored and the unordered pairs i < j of set 1 are taken.  In fp64, op by op:
 * s_a = x_j[a] - x_i[a], with boxsize > 0 moved by -+ boxsize when beyond +- boxsize / 2 (boxsize == 0: open boundaries,
 * plain separations), dv = v_j - v_i, and
 *   AST_PAIRVEL_RADIAL: d2 = (s_x^2 + s_y^2) + s_z^2; bin k when edges[k]^2 < d2 <= edges[k + 1]^2 (a pair at
 *                       distance 0 is in no bin); v = ((dv_x s_x + dv_y s_y) + dv_z s_z) / sqrt(d2).
 *   AST_PAIRVEL_LOS:    rp2 = s_a^2 + s_b^2 over the two axes other than los, in axis order; bin k when
 *                       edges[k]^2 < rp2 <= edges[k + 1]^2 and |s_los| <= pi_max; v = dv_los sign(s_los), sign in
 *                       {-1, 0, +1}.
 * |s_a| is bit for bit ast_tpcf_cross_counts' minimum image, so count_d of AST_PAIRVEL_RADIAL equals its counts on
 * the same edges.  count_d[nb] (exact, the same from call to call), s1_d[nb] = sum v, s2_d[nb] = sum v^2 (fp64 sums
 * in no fixed order within a workgroup: LDS atomics per wave, then fixed-order sums of the waves and workgroups - no
 * global float atomics).  All outputs are written, not accumulated; zero when a set is empty (auto: n1 < 2).  Pair
 * finder: the shared cell grid of ast_tpcf_cross_counts with the reach edges[nb] (radial) or
 * sqrt(edges[nb]^2 + pi_max^2) (los); single_cell != 0 forces one cell.  n1, n2 < 2^31. */
#define AST_PAIRVEL_RADIAL 0
#define AST_PAIRVEL_LOS 1
#define AST_PAIRVEL_MAX_BINS 511
/* stats_subfind.py:155-218 */
size_t ast_pairvel_workspace_bytes(size_t n1, size_t n2, int nb);
/* stats_subfind.py:155-218: the largest nb */
int ast_pairvel_max_bins(void);
/* stats_subfind.py:155-218 */
int ast_pairvel_prepare(const void* pos1_d, int pos1_dtype, const void* vel1_d, int vel1_dtype, size_t n1,
                        const void* pos2_d, int pos2_dtype, const void* vel2_d, int vel2_dtype, size_t n2,
                        void* work_d, size_t work_bytes, double* bounds_d, void* stream);
/* stats_subfind.py:155-218 */
int ast_pairvel_moments(void* work_d, size_t work_bytes, size_t n1, size_t n2, int auto_pairs, double boxsize, int kind,
                        int los, double pi_max, const double* edges_d, int nb, int single_cell,
                        unsigned long long* count_d, double* s1_d, double* s2_d, void* stream);

/* ------------------------------------------------- radial profiles on 2D maps */

/* Annulus sums and counts of objects on a 2D map: profiles/profile_2d.py (from_map, :10-59, and profiling, :92-153),
 * which rays/void.py (Voids.get_profiles / get_profile_stats, :188-410) and rays/peak.py (:95-239) call.  map_d: a
 * row-major (ny, nx) map of dtype AST_F32 / AST_F64, widened to fp64 on load.  Per object o: centres_d[2o] = y,
 * [2o + 1] = x (pixel indices, truncated by the host); reach_d[2o] = R = ceil(r * extend), [2o + 1] = m, the read reach;
 * thresholds_d[o * nbins + k - 1] = T_k, k = 1..nbins, the least d2 = a^2 + b^2 whose annulus index is >= k (2R^2 + 1
 * when none).  Pixel (a, b), -R <= a, b < R, adds map[y + a][x + b] to bin k when T_k <= d2 < T_{k+1} (T_0 = 0) and is
 * read when d2 < T_nbins; an index below 0 wraps once, as numpy's negative indices do.  The host must have checked
 * -ny <= y - m and y + min(m, R - 1) < ny (x likewise against nx); an object outside gets NaN sums and count -1.
 * Work items are bands of band_rows rows (ast_profile2d_band_rows(); 0: one item per object): object o owns items
 * item_start_d[o] .. item_start_d[o + 1] - 1 (item_start_d[0] = 0, item_start_d[n_obj] = n_work).  sums_d / counts_d
 * (n_obj, nbins) fp64 / int64 are written: the true per-annulus sums and pixel counts, each sum formed in an order fixed
 * by the object's geometry (bit-identical between calls).  The workspace holds the band rows: ast_profile2d_workspace_
 * bytes(n_obj, n_work, nbins) bytes (0: nbins outside 1..ast_profile2d_max_bins() or n_work < n_obj). */
int ast_profile2d_max_bins(void);
int ast_profile2d_band_rows(void);
size_t ast_profile2d_workspace_bytes(size_t n_obj, size_t n_work, int nbins);
int ast_profile2d(const void* map_d, int dtype, size_t ny, size_t nx, size_t n_obj, const long long* centres_d,
                  const long long* reach_d, const long long* thresholds_d, int nbins, int band_rows,
                  const long long* item_start_d, size_t n_work, void* work_d, size_t work_bytes, double* sums_d,
                  long long* counts_d, void* stream);

/* ------------------------------------------------- spherical profiles of particles around centres */

/* Per-centre radial histograms of particles: profiles/profile_3d.py (Profiles3D.get_one_profile / from_particle_data),
 * for haloes (edges in units of r200c) and voids (in units of the void radius).  For centre o with radius R_o and every
 * particle p it looks at: s = p - c_o, with boxsize > 0 wrapped once per axis (s > L/2 -> s - L, else s < -L/2 -> s + L;
 * boxsize == 0: plain separations), d2 = (sx^2 + sy^2) + sz^2, x = sqrt(d2) / R_o, all fp64.  The particle counts in bin
 * k when e_k <= x < e_{k+1}, and the last bin also takes x == e_nbins (np.histogram's rule; unlike the pair counts above a
 * particle at distance 0 counts when e_0 == 0).  counts_d (nc, nbins) int64 receives the counts and moments_d
 * (nc, nbins, nmom) fp64 the sums of w (nmom == 1) or of w, w v_r, w v_r^2, w |u|^2 (nmom == 4), u = v - centre
 * velocity (centre_vel_d == NULL: 0), v_r = ((ux sx + uy sy) + uz sz) / sqrt(d2), 0 at d2 == 0.  The counts are exact;
 * the sums are formed with LDS atomics inside a work item (their order is not fixed) and in item order across items.
 *
 * ast_profile3d_prepare: every particle becomes one 64-byte fp64 record (r, w, v); weights_d == NULL: w = 1, vel_d ==
 * NULL: v = 0; each array has its own dtype (AST_F32 / AST_F64).  bounds_d[6] receives min (x, y, z), max (x, y, z) of
 * the positions (NaN counts as -inf / +inf; (+inf, -inf) when np == 0): the caller checks [0, boxsize], or that
 * everything is finite, before it calls one of the two below.  bounds_only != 0: no records are written and the
 * workspace need only hold 256 bytes (a caller that must know the bounds before it can size the full workspace):
 *
 * ast_profile3d_search: the records are sorted into a grid of dims^3 cells (x fastest), cell of a coordinate =
 * floor((x - lo) * inv) clamped to [0, dims - 1] per axis (periodic: lo = 0, inv = dims / boxsize; open: the bounding
 * box, inv = 0 on an axis without extent).  Centre o visits the cells that [c - reach, c + reach] touches on each axis,
 * reach = e_nbins R_o (1 + 1e-9) + pad (pad: the caller's allowance for the rounding of large coordinates); periodic, a
 * range of >= dims cells visits each cell of the axis once.  zrange_d[2 o], [2 o + 1] = first z cell and number of z
 * layers of centre o, computed by the caller with that same expression.  Work items are runs of `layers` z layers
 * (ast_profile3d_layers(); 0: one item per centre).
 *
 * ast_profile3d_members: centre o looks only at records segments_d[2 o] .. + segments_d[2 o + 1] - 1 of the unsorted
 * array (the reference's cum_N_particles / N_particles); work items are chunks of `chunk` members
 * (ast_profile3d_chunk()).
 *
 * Both: centre o owns items item_start_d[o] .. item_start_d[o + 1] - 1, at least one each (item_start_d[0] = 0,
 * item_start_d[nc] = n_items).  A centre with one item is written straight into counts_d / moments_d; the items of a
 * centre with several go to partial rows part_start_d[o] + k (part_start_d[nc] = n_part, the number of such items) and
 * are summed in item order.  Workspace: ast_profile3d_workspace_bytes(np, ncells, n_part, nbins, nmom) =
 * 64 np (records) + [ncells > 0: 64 np (sorted) + 4 np + 12 ncells + 4 ceil(ncells / 2048) (grid)] +
 * 8 n_part nbins (1 + nmom), each array
 * rounded up to 256 bytes (ncells = dims^3 for the search, 0 for members); it does not grow with the number of
 * single-item centres.  0: nbins outside 1..ast_profile3d_max_bins(), nmom not 1 or 4, ncells >
 * ast_profile3d_max_cells(), or np >= 2^31. */
int ast_profile3d_max_bins(void);
int ast_profile3d_layers(void);
int ast_profile3d_chunk(void);
size_t ast_profile3d_max_cells(void);
size_t ast_profile3d_workspace_bytes(size_t np, size_t ncells, size_t n_part, int nbins, int nmom);
int ast_profile3d_prepare(const void* pos_d, int pos_dtype, const void* weights_d, int weights_dtype, const void* vel_d,
                          int vel_dtype, size_t np, int bounds_only, void* work_d, size_t work_bytes, double* bounds_d,
                          void* stream);
int ast_profile3d_search(void* work_d, size_t work_bytes, size_t np, int dims, double lo_x, double lo_y, double lo_z,
                         double inv_x, double inv_y, double inv_z, double boxsize, double pad, size_t nc,
                         const double* centres_d, const double* radii_d, const double* centre_vel_d,
                         const int* zrange_d, int layers, const long long* item_start_d, size_t n_items,
                         const long long* part_start_d, size_t n_part, const double* edges_d, int nbins, int nmom,
                         long long* counts_d, double* moments_d, void* stream);
int ast_profile3d_members(void* work_d, size_t work_bytes, size_t np, double boxsize, size_t nc,
                          const double* centres_d, const double* radii_d, const double* centre_vel_d,
                          const long long* segments_d, int chunk, const long long* item_start_d, size_t n_items,
                          const long long* part_start_d, size_t n_part, const double* edges_d, int nbins, int nmom,
                          long long* counts_d, double* moments_d, void* stream);

/* ------------------------------------------------- tunnels void finder */

/* The tunnels void finder of rays/voids/tunnel.py (TunnelsFinder.find_voids, :158-248; Cautun et al.,
 * arXiv:1710.01730), which there is an external program: the circles through at least three tracers with no tracer
 * strictly inside, i.e. the distinct circumcircles of the tracers' Delaunay triangles, whose centre lies in the map.
 * x_d, y_d: int32 pixel coordinates (x the column, y the row), 0 <= x, y < npix <= ast_tunnels_max_npix() (16384:
 * coordinate differences below 2^14 keep the in-circle determinant in int64), all distinct; the host checks this.
 * Every decision is exact integer arithmetic.  records_d[2 n][7] int64 receives, in no particular order, one record
 * (i, e, k, n_on, X, Y, W) per circle: i the smallest tracer index on it, e the tracer on it with every other one
 * strictly left of i -> e, k the next one counter-clockwise after e as seen from i, n_on >= 3 the number of tracers
 * on it, and the centre (X / W, Y / W) from the triple (i, e, k): b' = b - a, c' = c - a, D = b'x c'y - b'y c'x,
 * Ux = c'y |b'|^2 - b'y |c'|^2, Uy = b'x |c'|^2 - c'x |b'|^2, X = 2 D ax + Ux, Y = 2 D ay + Uy, W = 2 D > 0; kept when
 * 0 <= X, Y <= W (npix - 1).  count_d[0] = the number of records (never above 2 n), count_d[1] = violations: circles
 * found with a tracer inside, or walks that did not end; it must be 0.  The set of records is the same on every
 * call.  n < 3: no records.  single_cell != 0 puts all tracers into one cell, so that every scan sees all of them.
 * Workspace: ast_tunnels_workspace_bytes(n, npix) bytes (0: npix outside 1..16384 or n >= 2^31).  Nothing is
 * allocated and nothing synchronises. */
size_t ast_tunnels_workspace_bytes(size_t n, int npix);
int ast_tunnels_max_npix(void);
int ast_tunnels_find(const int* x_d, const int* y_d, size_t n, int npix, int single_cell, void* work_d,
                     size_t work_bytes, long long* records_d, unsigned long long* count_d, void* stream);

/* ------------------------------------------------- vector grids */

/* Finite-difference divergence of a vector grid: particles/hutils/map_transform.py:92-104 (_compute_divergence: three
 * np.gradient(value_map[:, :, :, a], 1 / boxsize, axis=a, edge_order=2) calls and their sum).  v_d: a contiguous
 * (n0, n1, n2, 3) array of dtype AST_F32 / AST_F64, axis 0 slowest, components interleaved; out_d: (n0, n1, n2) of the
 * same dtype.  Every side >= 3, sides need not be equal.  With T the dtype and every constant rounded to T:
 * interior cells, and all cells when periodic = 1 (indices wrap), d = (f[i+1] - f[i-1]) / T(2 h), a true division;
 * periodic = 0: first cell (T(-1.5/h) f[0] + T(2/h) f[1]) + T(-0.5/h) f[2], last cell (T(0.5/h) f[n-3] +
 * T(-2/h) f[n-2]) + T(1.5/h) f[n-1]; out = (d0(v_0) + d1(v_1)) + d2(v_2) - numpy's result bit for bit.  variant 0: one
 * work item per cell, plain loads; variant 1: a workgroup marches a (y, z) tile along axis 0, rows fetched once with
 * 16-byte accesses into LDS (an input that is not 16-byte aligned, or too many tiles for one launch, takes variant 0).
 * Both give the same bits.  All indexing is 64-bit. */
int ast_grid_divergence(const void* v_d, void* out_d, int dtype, size_t n0, size_t n1, size_t n2, double h,
                        int periodic, int variant, void* stream);
/* out[c] = sqrt((v[3c]^2 + v[3c+1]^2) + v[3c+2]^2), c < count: power_spectrum_3d.py:155-162 (_get_vector_magnitude,
 * np.sqrt(np.sum(np.square(value_map), axis=3))). */
int ast_vector_magnitude(const void* v_d, void* out_d, int dtype, size_t count, void* stream);
/* Divergence in Fourier space of three contiguous half spectra (n, n, n/2 + 1) in the layout of ast_fft_tile_r2c_3d,
 * complex64 (AST_F32) or complex128 (AST_F64): out = i ((k0 cx + k1 cy) + k2 cz), k_a = (2 pi / boxsize) m_a, m_a = j
 * for j < n/2, j - n for j > n/2 and 0 at j = n/2 (an odd derivative of a real field has no Nyquist component).  out_d
 * may be cx_d.  No reference counterpart (the reference differentiates in real space only). */
int ast_spectral_divergence(const void* cx_d, const void* cy_d, const void* cz_d, void* out_d, int cdtype, int nmesh,
                            double boxsize, void* stream);

/* ------------------------------------------------- watershed void finder */

/* The watershed void finder of rays/voids/watershed.py (which in the reference only writes files for an external
 * program; rays/utils/watershed_voids.py does not run).  Defined in DESIGN.md 6j: pixels of an npix x npix map
 * (AST_F32 / AST_F64, 3 <= npix, npix^2 < 2^31, flat index p = y npix + x) are totally ordered by (f[p], p), values
 * compared in the map's dtype; link[p] is the smallest of p and its up-to-8 neighbours inside the map; a minimum has
 * link[p] == p, and following links from p ends at the minimum of p's basin.
 *
 * ast_watershed_link writes link_d[npix^2] (int32) and *nonfinite_d (device uint64) = the number of NaN / inf pixels,
 * which the caller must find 0 before it goes on.
 * ast_watershed_jump resolves link_d in place to link[p] = the minimum of p's basin, by pointer jumping, at most
 * ast_watershed_max_passes(npix) = ceil(log2(npix^2)) passes (0: npix out of range), fewer when a pass reports that
 * every entry points at a minimum.  pending_d: that many int32 of device scratch.  *passes_host receives the number
 * of passes taken.  SYNCHRONOUS (one 4-byte read-back per pass).  AST_ERR_LIMIT when the bound did not suffice, which
 * no output of ast_watershed_link can cause.
 * ast_watershed_relabel: out_d[i] = table_d[src_d[i]], i < n (int32; -1 for an index outside [0, table_len)); out_d
 * may be src_d.  It makes the compact basin ids from the resolved links and the void map from the basin labels.
 * ast_watershed_sums: labels_d[npix^2] in [0, nbasins) -> isums_d[4][nbasins] int64 = area, sum of x, sum of y and
 * the number of pixels on the outermost rows / columns of every basin, sum_f_d[nbasins] = its sum of f in float64
 * (atomics: the order of the additions is not fixed).  Both are zeroed by the call.
 * ast_watershed_edges: every pixel looks at its E, SW, S and SE neighbours, so that every 8-adjacent pair is seen
 * once; for every other label among them it has one record, key (a << 32 | b) with a < b and the smallest
 * max(f[p], f[q]) + 0 (a -0.0 becomes +0.0) over those neighbours, in the map's dtype.  One 16 x 16 tile per workgroup,
 * ast_watershed_edge_blocks(npix) = ceil(npix / 16)^2 of them (0: npix out of range).  cap == 0: blocks_d[b] (int64)
 * receives the number of records of tile b (keys_d, saddle_d unused).  cap > 0: blocks_d[b] GIVES the index of tile
 * b's first record - the exclusive prefix sum of the counts, which the caller forms, cap being their total - and the
 * records go to keys_d[cap], saddle_d[cap], never past cap.  No global atomics: count, allocate exactly, fill. */
int ast_watershed_max_passes(int npix);
int ast_watershed_link(const void* img_d, int dtype, int npix, int* link_d, unsigned long long* nonfinite_d,
                       void* stream);
int ast_watershed_jump(int* link_d, int npix, int* pending_d, int* passes_host, void* stream);
int ast_watershed_relabel(const int* src_d, const int* table_d, size_t table_len, size_t n, int* out_d, void* stream);
int ast_watershed_sums(const void* img_d, int dtype, const int* labels_d, int npix, size_t nbasins, long long* isums_d,
                       double* sum_f_d, void* stream);
size_t ast_watershed_edge_blocks(int npix);
int ast_watershed_edges(const void* img_d, int dtype, const int* labels_d, int npix, long long* blocks_d, size_t cap,
                        long long* keys_d, void* saddle_d, void* stream);

/* ------------------------------------------------- friends-of-friends group finder */

/* Friends-of-friends groups of n < 2^31 particles (particles/hutils/fof.py).  Positions (n, 3), AST_F32 /
 * AST_F64, widened to fp64.  Per axis a = |x_i - x_j|, with boxsize > 0 the minimum image a = min(a, L - a) (boxsize
 * == 0: open).  Sphere (cylinder == 0): friends when (a_x^2 + a_y^2) + a_z^2 <= b_perp b_perp.  Cylinder along `los`:
 * friends when a_a a_a + a_b a_b <= b_perp b_perp (a < b the two other axes) and a_los <= b_para.  A group is a
 * connected component of the friendship graph.
 *
 * work_d: ast_fof_workspace_bytes(n) bytes (0: n out of range), contents undefined on entry; the calls below share it,
 * in this order, on one stream.
 * ast_fof_prepare writes the records and parent[i] = i into the workspace and bounds_d[6] = min x, y, z, max x, y, z
 * (a NaN counts as -inf and +inf; n == 0: +inf, -inf), which the caller checks: periodic within [0, boxsize], open
 * all finite.
 * ast_fof_link plans the cell grid (cells at least b_perp wide; the cylinder: grid_cyl_plan's per-axis cells; at most
 * one cell per 64 objects, or per AST_FOF_CELL_OBJECTS of the environment, and at least 27; single_cell != 0: one
 * cell), sorts, and unites every friend pair in the parent forest; *links_d (device uint64, zeroed by the call)
 * = the number of unordered friend pairs.  n < 2: only the zero.
 * ast_fof_compress resolves the forest by pointer jumping, at most ast_fof_max_passes(n) = ceil(log2 n) + 1 passes (0:
 * n out of range); pending_d: that many int32 of device scratch; *passes_host = the passes taken.  SYNCHRONOUS (one
 * 4-byte read-back per pass); AST_ERR_LIMIT when the bound did not suffice, which no output of ast_fof_link can
 * cause (a parent array that is not a forest; root_d and size_d are then left untouched).  Then root_d[i] (int32) =
 * the smallest index of i's group and size_d[r] (uint32, n entries, zeroed by the call) = the members of the group whose smallest index is r, 0 elsewhere.  n >= 1.
 * ast_fof_relabel: labels_d[i] = table_d[root_d[i]] (int32, n entries each).
 * ast_fof_features: for group g < ngroups with members members_d[offsets_d[g] .. offsets_d[g + 1]) (int32 particle
 * indices; offsets int64) and first_d[g] (int64) its reference particle: s_i = pos_i - pos[first], with boxsize > 0
 * wrapped once per axis (s > L/2 -> s - L, else s < -L/2 -> s + L); cm_d[g][3] = pos[first] + sum(w s) / sum(w),
 * with boxsize > 0 wrapped once into [0, L); cmv_d[g][3] = sum(w v) / sum(w) when vel_d is given; weight_d[g] =
 * sum(w); w = 1 without weights_d.  fp64; one wave per group, lane l adding members l, l + 64, ... in order and the
 * lanes combined by a fixed butterfly: the same bits on every call, no atomics. */
size_t ast_fof_workspace_bytes(size_t n);
int ast_fof_max_passes(size_t n);
int ast_fof_prepare(const void* pos_d, int pos_dtype, size_t n, void* work_d, size_t work_bytes, double* bounds_d,
                    void* stream);
int ast_fof_link(void* work_d, size_t work_bytes, size_t n, double boxsize, int cylinder, double b_perp, double b_para,
                 int los, int single_cell, unsigned long long* links_d, void* stream);
int ast_fof_compress(void* work_d, size_t work_bytes, size_t n, int* pending_d, int* passes_host, int* root_d,
                     unsigned* size_d, void* stream);
int ast_fof_relabel(const int* root_d, const int* table_d, size_t n, int* labels_d, void* stream);
int ast_fof_features(const void* pos_d, int pos_dtype, const void* vel_d, int vel_dtype, const void* weights_d,
                     int weights_dtype, size_t n, const int* members_d, const long long* offsets_d,
                     const long long* first_d, size_t ngroups, double boxsize, double* cm_d, double* cmv_d,
                     double* weight_d, void* stream);

/* ------------------------------------------------------------- mesh readout: grid -> particles
 * A periodic grid field evaluated at positions with the NGP / CIC / TSC window.  Replaces pmesh
 * RealField.readout(pos, resampler=), the adjoint of the ParticleMesh.paint that ast_paint replaces
 * (particles/hutils/stats_subfind.py:130-131); the reference never calls it - it takes grids to the host instead.
 *   field_d: the WHOLE grid, nmesh^3 * ncomp elements of field_dtype, C order, the ncomp (1 .. 4) components of a cell
 *            interleaved on the last axis: (n, n, n) or (n, n, n, ncomp).
 *   pos_d:   (np, 3) AoS of pos_dtype (independent of field_dtype), box units; any real value wraps periodically.
 *   out_d:   (np, ncomp) of field_dtype; every element is overwritten.  No workspace.
 * Per particle and axis s = fma((double)x, nmesh / boxsize, shift_cells); base cell and offset, weights and stencil
 * as in ast_paint (weights evaluated in field_dtype).  Then, weights widened to double, per component c
 *   acc = 0.0;  for a (x): for b (y): { wab = wx[a] * wy[b];  for cz (z): acc += (wab * wz[cz]) * (double)field[..] }
 *   out[p][c] = (field_dtype)acc
 * in exactly this order, without fused multiply-adds: the same bits on every call and for every launch geometry.
 * A NaN or infinite coordinate gives NaN in every component of that particle; no coordinate of any bit pattern
 * makes the call read outside field_d (base cells are clamped to [0, nmesh - 1]).
 * np == 0: AST_OK without a launch. */
int ast_readout(int window, int field_dtype, int pos_dtype, const void* field_d, int nmesh, int ncomp, const void* pos_d,
                size_t np, double boxsize, double shift_cells, void* out_d, void* stream);

/* ------------------------------------------------------------- lens planes: particles -> P planes of npix x npix
 * Projected mass assignment for a periodic box (plane-parallel) and a light cone (gnomonic map, radial shells), with
 * the NGP / CIC / TSC window on the two transverse axes.  No reference counterpart: the reference reads its planes
 * from Ray-Ramses output (hard part 6).  DESIGN.md 6n holds the contract in full; in short:
 *
 * ast_plane_paint_accumulate: sums_d (nplanes, npix, npix) int64 += the deposits of np particles.  pos_d (np, 3) and
 * mass_d (np; NULL: 1) of `dtype`.  All arithmetic in double, one rounding per written operation:
 *   ms = (double)mass * scale; a particle with !(|ms| <= vmax) is REFUSED (counters_d[2]) and deposits nothing.
 *   (a, b): the two axes other than `los`, in increasing order; sums is indexed [plane][ia][ib].
 *   AST_PLANE_BOX:  sl = x_los * cl, plane = floor(sl) mod nplanes; s_a = x_a * c1 + c0 (two roundings); base pixel,
 *       offset and the periodic stencil as in ast_paint.  A particle whose sl, s_a or s_b is not finite is outside
 *       (counters_d[0]).  Every finite coordinate is reduced modulo the period and deposited.
 *   AST_PLANE_CONE: d = x - origin (host, 3 doubles); outside (counters_d[0]) when a d is not finite, d_los <= 0, or
 *       r2 = (d0 d0 + d1 d1) + d2 d2 is not in [e2_d[0], e2_d[nplanes]); plane p has e2_d[p] <= r2 < e2_d[p + 1]
 *       (e2_d: nplanes + 1 ascending doubles on the device).  s_a = (d_a / d_los) * c1 + c0; base = floor(s) (CIC) or
 *       floor(s + 1/2), offset s - base, base clamped in double to [-2, npix + 1]; stencil points outside [0, npix)
 *       are dropped: all of them - outside; some - clipped (counters_d[1]).
 *   Weights as Window<W>::weights<double>, not renormalised.  Term (ms wa[i]) wb[j], times invq = 2^k / vmax, rounded
 *   to the nearest integer (ties to even) and added with a 64-bit integer atomic; k = ast_plane_paint_exponent(np_total),
 *   np_total >= np the declared bound on all particles ever added to these sums: they cannot overflow, and they hold
 *   the same bits for every particle order, chunking and launch geometry.
 * counters_d: 3 uint64 on the device, added to.  np == 0: AST_OK without a launch.
 *
 * ast_plane_paint_exponent: host only; min(50, 62 - bit_length(np_total)), -1 for np_total >= 2^60.
 *
 * ast_plane_paint_finish: out[p][ia][ib] = (out_dtype)(v + add_d[p]), v = (double)sums * mul_d[p], in the cone
 * v = v * (w * sqrt(w)), w = (1 + ta ta) + tb tb, ta = ((ia + 0.5) - npix / 2) / c1: the cos^-3 that gives gnomonic
 * pixels equal solid angle.  mul_d, add_d: nplanes doubles on the device.  Every element of out_d is written. */
#define AST_PLANE_BOX 0
#define AST_PLANE_CONE 1
int ast_plane_paint_exponent(size_t np_total);
int ast_plane_paint_accumulate(int geometry, int window, int dtype, const void* pos_d, const void* mass_d, size_t np,
                               size_t np_total, int los, int nplanes, int npix, double cl, double c1, double c0,
                               const double* origin, const double* e2_d, double scale, double vmax, long long* sums_d,
                               unsigned long long* counters_d, void* stream);
int ast_plane_paint_finish(int geometry, int out_dtype, const long long* sums_d, const double* mul_d, const double* add_d,
                           int nplanes, int npix, double c1, void* out_d, void* stream);

/* ------------------------------------------------------------- multi-plane ray tracing over lens planes
 * Flat sky, angles in radians, distances comoving.  Everything is double, one rounding per written operation, no fused
 * multiply-add; tests/ray_trace_oracle.py restates step and emit in numpy and the GPU tests compare bytes.  Nothing
 * outlives a call; all work goes to `stream`.
 *
 * ast_lens_green_multiply: spec_d, the (m, m/2 + 1) interleaved complex128 half spectrum of an m x m plane (what an R2C
 *   of ast_fft_exec leaves), in place: mode (a, b) times -2 scale / (4 (sin^2(pi a / m) + sin^2(pi b / m))), mode (0, 0)
 *   set to 0.  After an unnormalised C2R and with scale = c h^2 / m^2 the result psi has the 5-point Laplacian
 *   (psi[a+1,b] + psi[a-1,b] + psi[a,b+1] + psi[a,b-1] - 4 psi[a,b]) / h^2 = 2 c (plane - its mean), to rounding.
 *
 * ast_ray_step: one lens plane.  psi_d: (m, m), periodic.  state_d: 12 planes of (npix, npix), npix <= m and
 *   npix <= 4 * 65535 = 262140 (the launch has one row of workgroups per 4 rows of rays, at most 65535), in the order
 *   d1 d2 s1 s2 A11 A12 A21 A22 B11 B12 B21 B22 (d = beta - theta, s = dx/dchi - theta, A = d beta / d theta - I,
 *   B = d (dx/dchi) / d theta - I; component 1 is array axis 0), updated in place.  Ray (i, j) passes node (i, j) of psi
 *   undeflected.  With dchi = chi_k - chi_prev (formed on the host), 0 <= chi_prev < chi_k:
 *     advance   d <- (chi_prev d + dchi s) / chi_k, A <- (chi_prev A + dchi B) / chi_k, entry by entry
 *     position  p1 = i + d1 / h, p2 = j + d2 / h (born: p = (i, j)); a = floor(p1), fx = p1 - a, b and fy alike; node
 *               indices wrap modulo m (floor(p) is clamped to +-2^30 first: no state reads outside psi_d)
 *     at the nodes (a, b), (a+1, b), (a, b+1), (a+1, b+1), each written with ITS OWN a, b:
 *               a1 = (psi[a+1,b] - psi[a-1,b]) / (2 h)            u11 = ((psi[a+1,b] - 2 psi[a,b]) + psi[a-1,b]) / (h h)
 *               a2 = (psi[a,b+1] - psi[a,b-1]) / (2 h)            u22 = ((psi[a,b+1] - 2 psi[a,b]) + psi[a,b-1]) / (h h)
 *               u12 = (((psi[a+1,b+1] - psi[a+1,b-1]) - psi[a-1,b+1]) + psi[a-1,b-1]) / (4 (h h))
 *     bilinear  q = ((w00 q00 + w10 q10) + w01 q01) + w11 q11 in that node order, w00 = (1-fx)(1-fy), w10 = fx (1-fy),
 *               w01 = (1-fx) fy, w11 = fx fy: alpha1, alpha2, U11, U22, U12 (= U21)
 *     deflect   s <- s - alpha;  B11 <- B11 - (U11 (1 + A11) + U12 A21),  B12 <- B12 - (U11 A12 + U12 (1 + A22)),
 *               B21 <- B21 - (U12 (1 + A11) + U22 A21),  B22 <- B22 - (U12 A12 + U22 (1 + A22));  born: B <- B - U
 *
 * ast_ray_emit: the maps of a source at chi_s > chi_k, chi_k the plane the state was last stepped through:
 *   x_s = (chi_k x + (chi_s - chi_k) y) / chi_s for (x, y) = (d, s) and (A, B) entry by entry; then six planes of
 *   (npix, npix), plane q at out_d + q out_stride (doubles): kappa = -0.5 (A11 + A22), gamma1 = -0.5 (A11 - A22),
 *   gamma2 = -0.5 (A12 + A21), omega = 0.5 (A21 - A12), alpha1 = -d1, alpha2 = -d2.  Every element is written. */
int ast_lens_green_multiply(void* spec_d, int m, double scale, void* stream);
int ast_ray_step(const double* psi_d, int m, double* state_d, int npix, double h, double chi_prev, double chi_k, int born,
                 void* stream);
int ast_ray_emit(const double* state_d, int npix, double chi_k, double chi_s, double* out_d, size_t out_stride,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ASTRILD_HIP_H */
