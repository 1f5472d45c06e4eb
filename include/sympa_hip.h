/* sympa_hip.h -- C-ABI of the MI355X (gfx950) Siegel-distance library  (libsympa_hip.so)
 *
 * The reference (fedelopez77/sympa) is pure Python/torch and has no FFI layer; its drop-in boundary
 * for this path is the Python API  Model.forward -> manifold.dist  (SURVEY.md section 8b).  These
 * entry points are what a binding for that path binds: one call per reference method, plain
 * pointers and sizes, no torch types.  Each entry cites the reference interface it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless stated otherwise; the caller owns all buffers,
 *     the library allocates nothing and keeps no mutable global state (re-entrant);
 *   - a point is [2, n, n] fp64 row-major, plane 0 = Re, plane 1 = Im (sympa/math/csym_math.py:1-8);
 *     only the upper triangle (i <= j) of each plane is read (points on the manifold are symmetric);
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) and the
 *     call returns without synchronising; it is safe to capture into a hipGraph;
 *   - return value: 0 = enqueued, <0 = argument error (SYMPA_ERR_*), >0 = hipError_t of the launch;
 *     sympa_last_error() gives a thread-local message;
 *   - numeric-range violations the reference reports with `assert` (siegel_manifold.py:64-66) or a
 *     Python IndexError are reported through `status` (device int32[2], may be NULL):
 *         status[0] |= SYMPA_ST_* bits,   status[1] += number of offending pairs.
 *     The caller zeroes it and reads it back lazily (no host sync inside the library).
 */
#ifndef SYMPA_HIP_H
#define SYMPA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* models: ManifoldFactory.sympa_manifolds keys (sympa/embeddings.py:145-149) */
#define SYMPA_MODEL_UPPER 0   /* UpperHalfManifold   sympa/manifolds/upper_half.py:8 */
#define SYMPA_MODEL_BOUNDED 1 /* BoundedDomainManifold sympa/manifolds/bounded_domain.py:10 */
#define SYMPA_MODEL_DUAL 2    /* CompactDualManifold sympa/manifolds/compact_dual.py:8.  One pair (row) per lane and runtime-n kernels only:
                                 SYMPA_FLAG_COOP / SYMPA_FLAG_SPLIT are ignored, sympa_table_pack_bytes returns 0 (no packed path),
                                 sympa_table_pack* / sympa_model_forward*_packed / sympa_tangent_sqnorm / sympa_radam_step* /
                                 sympa_rsgd_step_fused return SYMPA_ERR_BAD_ARG (the reference's inner raises NotImplementedError,
                                 compact_dual.py:96), sympa_set/get_instance_fallback reject it, step_counter needs dims <= 8.
                                 eps is validated but unused: the model has no boundary and no clamp. */

/* metrics: MetricType values (sympa/manifolds/metrics.py:6-12) */
#define SYMPA_METRIC_RIEM 0
#define SYMPA_METRIC_FONE 1
#define SYMPA_METRIC_FINF 2
#define SYMPA_METRIC_FMIN 3
#define SYMPA_METRIC_WSUM 4

#define SYMPA_ST_NOT_PD 1         /* Im(z) (upper) or I - z z^H (bounded) not positive definite */
#define SYMPA_ST_NONFINITE 2      /* result is NaN/Inf */
#define SYMPA_ST_BAD_INDEX 4      /* gather index outside [0, num_rows) (reference: IndexError) */
#define SYMPA_ST_NO_CONVERGENCE 8 /* eigenvalue iteration hit its sweep cap */

#define SYMPA_ERR_BAD_ARG (-1)
#define SYMPA_ERR_UNSUPPORTED_DIMS (-2)

/* flags */
#define SYMPA_FLAG_LOW_LDS 1 /* stage one endpoint at a time: half the LDS per block, so blocks of two launches
                                that overlap (different streams / independent graph nodes) share a CU */

#define SYMPA_FLAG_GENERIC 2 /* run the runtime-n one-lane-per-pair kernel even where a sixteen-lanes-per-pair one applies
                                (spd n >= 6, upper / bounded n >= 9); the tests cross-check the two */

#define SYMPA_FLAG_ANY_ORDER 4 /* forward launches only: dispatch without the in-order barrier bit (hipExtAnyOrderLaunch), so
                                  the launch may start while earlier launches of the same stream still run.  Only for
                                  launches that do not depend on earlier work of that stream (independent batches);
                                  a later ordinary launch or synchronisation still waits for all of them.  MEASURED on
                                  gfx950 / ROCm 7.2 (profiles/r02_launch_overhead.txt): no overlap is obtained -- the
                                  runtime documents the flag as unsupported on GFX9 -- so the fused form below
                                  (SYMPA_FLAG_FUSE) is what overlaps independent batches */

#define SYMPA_FLAG_FUSE 8 /* sympa_model_forward_batches only (dims <= SYMPA_MAX_DIMS): up to SYMPA_MAX_FUSED_BATCHES
                             consecutive batches per kernel launch instead of one launch per batch */
#define SYMPA_MAX_FUSED_BATCHES 32
#define SYMPA_FLAG_COOP 32 /* A/B switch of the sixteen-lanes-per-pair layout (DESIGN.md sections 5, 8, 10):
                              forward, dims 6 and 8: run it instead of the one-pair-per-lane kernel (2-2.5x slower there);
                              backward entries, dims 5..8: the eight-lanes-per-pair kernels (two pairs per DPP row; the default
                              where measured faster: the fused step at n = 8, bounded n = 8 rows, bounded n = 7 fused);
                              SYMPA_FLAG_GENERIC forces the one-pair-per-lane kernels there;
                              sympa_spd_backward_rows: the single-round kernel instead of the one that runs the QL of two
                              rounds together */
#define SYMPA_FLAG_SPLIT 64 /* backward entries, dims 5..8, with a workspace: run the split (two-kernel, one pair per lane) backward
                             * wherever it is built -- by default it runs only where it measured faster than the one-launch kernels
                             * (upper model, dims 7 and 8: profiles/r04_n8_backward_split.txt) */
#define SYMPA_FLAG_NO_SYMMETRY 16 /* sympa_all_pairs_dist_packed: evaluate both (i, j) and (j, i) even for the full matrix */
#define SYMPA_FLAG_MERGE_SRC 128 /* sympa_model_train_backward, dims <= 6: consecutive pairs of a wave (64 pairs) with the SAME source id
                                  * are summed in pair order inside the wave's LDS tile.  Rows form (grad_rows): the sum is written ONCE,
                                  * into the source row slot of the LAST pair of the run, the other source slots of the run are NOT
                                  * written -- the caller's segmented sum must leave them out (sympa_amd.ops.sorted_slots(...,
                                  * merged_src=batch)); bitwise reproducible like the plain rows form.  Scatter form (grad_table): one
                                  * atomic row per run.  For batches sorted by their first column (~13 pairs per source row at the
                                  * headline shape) that is 45 % fewer rows through memory. */

#define SYMPA_MAX_DIMS 8          /* largest n with a register-resident forward kernel in this build */
#define SYMPA_MAX_DIMS_BACKWARD 16 /* largest n with a backward kernel in this build: n <= 6 one pair per lane in registers;
                                      n = 7, 8 one pair per lane or eight lanes per pair (the default where measured faster;
                                      SYMPA_FLAG_COOP forces the eight-lanes kernels at n = 5..8, SYMPA_FLAG_GENERIC the
                                      one-pair-per-lane ones); n = 9..16 sixteen lanes per pair (csrc/siegel_coop_bwd.hpp),
                                      SYMPA_FLAG_GENERIC selects the same adjoint as rolled loops over per-lane scratch */
#define SYMPA_MAX_DIMS_ALL_PAIRS_PACKED 8 /* sympa_all_pairs_dist_packed: per-point factor reuse, dims 1..8 (dims 8: the 64
                                             packed column points of a block live in an LDS tile, 55 / 70 KB) */
#define SYMPA_MAX_DIMS_GENERIC 16 /* n in (SYMPA_MAX_DIMS, 16]: the forward runs sixteen lanes per pair (csrc/siegel_coop.hpp;
                                     SYMPA_FLAG_GENERIC selects the runtime-n fallback over scratch).  The table operations
                                     (sympa_egrad2rgrad / sympa_projx / sympa_rsgd_step* / sympa_tangent_sqnorm) run one row
                                     per lane for n <= 6, eight lanes per row at n = 7, 8 and sixteen at n = 9..16
                                     (csrc/siegel_coop_table.hpp); the rolled one-row-per-lane kernels over scratch
                                     (siegel_table_rolled.hip) remain for the gated exact projection and behind
                                     SYMPA_TABLE_GENERIC=1 / an instance fallback */

/* Library / build identification. */
const char* sympa_version(void);
const char* sympa_last_error(void);
int sympa_max_dims(void);

/* Kernel families whose default instantiations use the sixteen- / eight-lanes-per-pair layout with inline-asm DPP
 * instructions (the compiler cannot see their hazards; the build scans the ISA, and a numerical self-check
 * compares every instantiation with the one-lane kernel on first use -- sympa_amd/selfcheck.py).  An instantiation
 * (family, model, n) marked here is routed to the one-lane-per-pair / one-row-per-lane kernel by every entry point, whatever
 * the flags; model is SYMPA_MODEL_* (0 for the spd families).  Process-wide, thread-safe, no GPU call.  No reference
 * counterpart (the reference has no native kernels). */
#define SYMPA_FAMILY_SIEGEL_FWD 0   /* sympa_siegel_dist_fwd / sympa_model_forward*, n = 9..16 */
#define SYMPA_FAMILY_SIEGEL_BWD 1   /* sympa_siegel_dist_bwd / sympa_model_backward / sympa_model_loss_backward*, n = 5..16 */
#define SYMPA_FAMILY_SIEGEL_TABLE 2 /* sympa_egrad2rgrad / sympa_projx / sympa_rsgd_step* / sympa_tangent_sqnorm, n = 7..16 */
#define SYMPA_FAMILY_SPD_FWD 3      /* sympa_spd_dist_fwd / sympa_spd_model_forward, n = 6..16 */
#define SYMPA_FAMILY_SPD_BWD 4      /* sympa_spd_backward_rows / sympa_spd_loss_backward, n = 3..16 */
#define SYMPA_FAMILY_SPD_TABLE 5    /* sympa_spd_egrad2rgrad / sympa_spd_rsgd_step / sympa_spd_radam_step /
                                       sympa_spd_expmap / _logmap / _geodesic / sympa_spd_rsgd_step_exp, n = 3..16 */
#define SYMPA_NUM_FAMILIES 6
int sympa_set_instance_fallback(int family, int model, int n, int on);
int sympa_get_instance_fallback(int family, int model, int n);

/* manifold.dist(z1, z2) for pre-gathered points.
 * Replaces SiegelManifold.dist (sympa/manifolds/siegel_manifold.py:41-72) for model = UPPER and
 * BoundedDomainManifold.dist (sympa/manifolds/bounded_domain.py:27-39) for model = BOUNDED,
 * including Metric.compute_metric (sympa/manifolds/metrics.py:42-121).
 *   z1, z2    [b, 2, n, n] fp64 contiguous
 *   metric_w  [n] fp64, the wsum weights (metrics.py:103-108); may be NULL unless metric = WSUM
 *   eps       clamp of (1 - d), reference EPS[float64] = 1e-5 (sympa/config.py:19)
 *   out       [b] fp64 distances
 *   vvd_out   [b, n] fp64 ascending vector-valued distance v (siegel_manifold.py:69-70), or NULL
 *   flags     0 or SYMPA_FLAG_*
 */
int sympa_siegel_dist_fwd(const double* z1, const double* z2, int64_t b, int n, int model, int metric,
                          const double* metric_w, double eps, double* out, double* vvd_out, int32_t* status,
                          int flags, void* stream);

/* Model.forward(input_triplet) fused: gather two table rows per pair, distance, times the scale.
 * Replaces Model.forward / Model.distance / Model.get_scale (sympa/model.py:16-41) and
 * Embeddings.forward (sympa/embeddings.py:29-34).
 *   table      [num_rows, 2, n, n] fp64 (the ManifoldParameter, embeddings.py:27,68)
 *   src, dst   int64 node ids, element i at src[i * src_stride] (so input_triplet[:, 0] / [:, 1] of a
 *              [b, 2|3] int64 tensor are passed without a copy: stride 2 or 3)
 *   scale      device pointer to the model's scale parameter (1 fp64) or NULL for 1.0;
 *              out = dist * max(scale / scale_coef, 0.1)          (model.py:40-41)
 */
int sympa_model_forward(const double* table, int64_t num_rows, int n, const int64_t* src, int64_t src_stride,
                        const int64_t* dst, int64_t dst_stride, int64_t b, int model, int metric,
                        const double* metric_w, double eps, const double* scale, double scale_coef, double* out,
                        int32_t* status, int flags, void* stream);

/* Model.forward over a LIST of batches: what Runner.evaluate's loop (sympa/runner.py:126-137) and the batch loop of
 * Runner.train_epoch's forward (runner.py:98-103) issue one call at a time.  Batch i reads the int64 triplets
 * triplets[i] ([b[i], stride], src = column 0, dst = column 1) and writes out[i] ([b[i]] fp64); `triplets`, `b`,
 * `out` and `streams` are HOST arrays (of device pointers / sizes / hipStream_t).  Launch i goes to
 * streams[i % num_streams]: the batches are independent, so consecutive launches overlap on the GPU (the next batch
 * gathers its rows while the previous one computes) -- with SYMPA_FLAG_LOW_LDS three blocks of different launches share
 * a CU.  One kernel launch per batch, exactly as num_batches calls of sympa_model_forward; nothing is synchronised.
 * With SYMPA_FLAG_FUSE (dims <= SYMPA_MAX_DIMS) groups of up to SYMPA_MAX_FUSED_BATCHES consecutive batches are
 * evaluated by ONE launch each (group g on streams[g % num_streams]): the grid is several blocks per CU deep, so
 * the batches overlap inside the launch with no kernel boundary between them -- the form to use when a batch is
 * about one wave per SIMD or less (65 536 pairs fill the 1 024 SIMDs of an MI355X exactly once).  Same results,
 * bit for bit. */
int sympa_model_forward_batches(const double* table, int64_t num_rows, int n, const int64_t* const* triplets,
                                int64_t stride, const int64_t* b, int num_batches, int model, int metric,
                                const double* metric_w, double eps, const double* scale, double scale_coef,
                                double* const* out, int32_t* status, int flags, void* const* streams, int num_streams);

/* ---- Packed table for the INDEXED forward, dims 5..8 (csrc/siegel_packed_kernel.hpp) ----------------------------------
 * The reference's loops run many batches over an unchanged table: Runner.evaluate (sympa/runner.py:124-135), the N forward
 * calls of the mAP matrix (runner.py:142-154), every Model.forward between two optimiser steps (sympa/model.py:16-30 with
 * Embeddings.forward, sympa/embeddings.py:29-34).  sympa_table_pack factors every point ONCE per table version -- Y = L L^T
 * (upper) / I - W W^H = C C^H (bounded) -- and writes one contiguous row per point: the upper triangles of both planes and the
 * INVERTED factor (row stride sympa_table_pack_bytes(1, n, model) bytes: 864 at n = 8 upper, where the reference row is 1 024).
 * The pair kernels then need no Cholesky and no solve: E = A1 (Z2 - Z1) A2^T.  A point outside the manifold is reported through
 * `status` here (SYMPA_ST_NOT_PD; `status` may be NULL) and flags every pair it enters later.  (sympa_amd passes NULL: the
 * reference's assertions sit in dist, siegel_manifold.py:64-66, so a point no batch touches raises nothing there.)
 *   pack   caller-owned device buffer, 16-byte aligned, sympa_table_pack_bytes(num_rows, n, model) bytes (0 = this build has no
 *          packed path for these dims / model: use sympa_model_forward); valid until the table changes (the caller keeps the
 *          version: sympa_amd/model.py repacks when the ManifoldParameter's version counter has moved).
 * sympa_model_forward_packed = sympa_model_forward reading `pack` instead of the table: one pair per lane, PERSISTENT one-wave blocks
 * (grid = what the chip holds at once), the next tile's ids and first rows in flight behind the current tile's arithmetic, the first
 * point's triangles subtracted from the second's in place as they arrive (no scratch in any instantiation: bounded n = 8 runs 245 ->
 * 163 us per 262 144 pairs, upper n = 8 135 -> 127, n = 6 85 -> 68; profiles/r05_packed_forward.txt).  Same distances as
 * sympa_model_forward to rounding (~1e-15 relative on the bench tables; the arithmetic differs: products with the inverted factor
 * instead of triangular solves).
 * sympa_model_forward_batches_packed: the list form (sympa_model_forward_batches); up to SYMPA_MAX_FUSED_BATCHES consecutive batches
 * share a launch; one stream. */
int64_t sympa_table_pack_bytes(int64_t num_rows, int n, int model);
int sympa_table_pack(const double* table, int64_t num_rows, int n, int model, void* pack, int64_t pack_bytes, int32_t* status,
                     void* stream);

/* Validity of a pack decided ON THE DEVICE (csrc/table_digest.hpp).  The reference writes its table through `.data`
 * (sympa/embeddings.py:36-39 `self.embeds.data = self.manifold.projx(...)`; geoopt / torch-1.5 optimisers `p.data.add_(...)`), which
 * no version counter sees, so a drop-in must not trust one.
 * sympa_table_digest: one kernel reads `bytes` bytes at `data` (16-byte aligned, a multiple of 8) and sums a 64-bit position-
 * weighted digest; its last block compares it with the one kept in `state` (caller-owned, SYMPA_DIGEST_STATE_BYTES of device memory,
 * zeroed once by the caller), stores the new one and writes ((uint32_t*)state)[SYMPA_DIGEST_CHANGED_WORD] = 1 when the bytes
 * changed since the previous call on this state (or with SYMPA_FLAG_DIGEST_FORCE), else 0.  No host synchronisation.
 * sympa_table_pack_refresh = that digest of the table + sympa_table_pack whose blocks return at once when the word is 0: the pack
 * is remade exactly when the table's bytes differ from those it was made from (first call on a zeroed state: always), on the
 * stream, graph-capturable -- a replayed graph with an optimiser step in front repacks by itself.  Cost when nothing changed: one
 * read of the table (measured: profiles/r06_pack_refresh.txt).  sympa_spd_table_pack_refresh: the same for sympa_spd_table_pack. */
#define SYMPA_DIGEST_STATE_BYTES 4096
#define SYMPA_DIGEST_CHANGED_WORD 6
#define SYMPA_FLAG_DIGEST_FORCE 1
int sympa_table_digest(const void* data, int64_t bytes, void* state, int flags, void* stream);
int sympa_table_pack_refresh(const double* table, int64_t num_rows, int n, int model, void* pack, int64_t pack_bytes,
                             void* digest_state, int flags, int32_t* status, void* stream);
int sympa_model_forward_packed(const void* pack, int64_t pack_bytes, int64_t num_rows, int n, const int64_t* src,
                               int64_t src_stride, const int64_t* dst, int64_t dst_stride, int64_t b, int model, int metric,
                               const double* metric_w, double eps, const double* scale, double scale_coef, double* out,
                               int32_t* status, int flags, void* stream);
int sympa_model_forward_batches_packed(const void* pack, int64_t pack_bytes, int64_t num_rows, int n,
                                       const int64_t* const* triplets, int64_t stride, const int64_t* b, int num_batches,
                                       int model, int metric, const double* metric_w, double eps, const double* scale,
                                       double scale_coef, double* const* out, int32_t* status, int flags, void* stream);

/* Measurement aid (bench.py `clock`): stamps the shader-cycle counter and the constant 100 MHz counter of SYMPA_CLOCK_STAMP_BLOCKS
 * one-wave blocks (several per CU) into out[block] = {s_memtime, s_memrealtime, XCC_ID | HW_ID << 8} (3 x uint64 per block,
 * device memory).  Two stamps around a stream-ordered region give the shader clock the chip HELD over that region:
 * d(s_memtime) / d(s_memrealtime) x 100 MHz between stamps taken on the SAME CU (bits 8..15 of HW_ID: CU, SH, SE; the counters of
 * different CUs are not comparable) -- what the fp64-issue roof of the timed kernels has to be priced at (the chip lowers
 * its clock under sustained load).  Not part of the reference's API; no product path calls it. */
#define SYMPA_CLOCK_STAMP_BLOCKS 2048
int sympa_clock_stamp(void* out, void* stream);

/* Block of rows of the all-pairs distance matrix that Runner.build_distance_matrix (sympa/runner.py:142-154)
 * assembles with N calls of Model.forward over N pairs each (for the mAP metric, sympa/metrics.py:39-63):
 *   out[(i - row_begin) * num_rows + j] = Model.forward((i, j)),  i in [row_begin, row_begin + row_count),  j in [0, N)
 * The diagonal is exactly 0 (the reference overwrites it with 0, runner.py:152).  For the FULL matrix (row_begin = 0,
 * row_count = num_rows) of dims >= 3 the symmetry d(i, j) = d(j, i) is used: the pairs i <= j are evaluated and every
 * value is stored at (i, j) and (j, i) (SYMPA_FLAG_NO_SYMMETRY evaluates both orders; a row block always does). */
int sympa_all_pairs_dist(const double* table, int64_t num_rows, int n, int64_t row_begin, int64_t row_count, int model,
                         int metric, const double* metric_w, double eps, const double* scale, double scale_coef,
                         double* out, int32_t* status, int flags, void* stream);

/* The same matrix with per-point factor reuse (dims <= SYMPA_MAX_DIMS_ALL_PAIRS_PACKED): every point is factored once
 * into `workspace` (sympa_all_pairs_workspace_bytes(num_rows, n, model) bytes of device memory owned by the caller,
 * overwritten; 0 = this build has no packed kernel for these dims), the pair kernel then needs neither a Cholesky nor
 * a gather, and for the FULL matrix (row_begin = 0, row_count = num_rows) of dims >= 3 only the pairs i <= j are
 * evaluated and each value is stored at (i, j) and (j, i) -- out is exactly symmetric -- unless SYMPA_FLAG_NO_SYMMETRY
 * is given; the diagonal is exactly 0 in every mode.  Same distances as
 * sympa_all_pairs_dist to rounding (1e-12 relative). */
int64_t sympa_all_pairs_workspace_bytes(int64_t num_rows, int n, int model);
int sympa_all_pairs_dist_packed(const double* table, int64_t num_rows, int n, int64_t row_begin, int64_t row_count,
                                int model, int metric, const double* metric_w, double eps, const double* scale,
                                double scale_coef, double* out, void* workspace, int64_t workspace_bytes,
                                int32_t* status, int flags, void* stream);

/* workspace (every backward entry below; caller-owned device scratch, 16-byte aligned, may be NULL): with at least
 * sympa_siegel_backward_workspace_bytes(b, n, model) bytes the SPLIT backward runs where it is built (dims 5..8, csrc/
 * siegel_bwd_split_kernel.hpp): ONE PAIR PER LANE in two kernels -- (1) factors, E, H = E^H E, Householder + QL with eigenvectors,
 * metric value, fused loss, Hbar = V diag(phi) V^H and K = Hbar H scaled by go * scale into the workspace ([entry][pair] layout);
 * (2) factors and E again from the table rows, Ebar = 2 E Hbar, G = Ebar E^H / 2, the solves and congruences, scatter / rows.  The
 * whole adjoint in one lane spills ~1100 registers at n = 8 and the eight-lanes-per-pair kernel repeats the scalar QL in the lanes
 * of a pair; the split form does neither (fused step, upper n = 8, 262 144 pairs: 1.42 -> 0.81 ms, 0.68 ms on batches sorted by source row).  It is the default where it
 * measured faster (upper model, dims 7, 8); SYMPA_FLAG_SPLIT runs it for every model and dims 5..8.  NULL / too small /
 * SYMPA_FLAG_GENERIC / SYMPA_FLAG_COOP: the other kernels, as before (same results to ~1e-11 relative: the split form takes the
 * spectral weights from the QL's eigenvalues instead of the Rayleigh quotients ||E v_i||^2).  Returns 0 where no kernel uses one.
 * Replaces the reference's autograd through siegel_manifold.py:41-72 (runner.py:105). */
int64_t sympa_siegel_backward_workspace_bytes(int64_t b, int n, int model);

/* Backward of manifold.dist for pre-gathered points: what torch autograd computes through
 * siegel_manifold.py:41-72 / bounded_domain.py:27-39 when runner.py:105 calls loss.backward().
 *   grad_out          [b] fp64 dLoss/d(dist)
 *   grad_z1, grad_z2  [b, 2, n, n] fp64, written (symmetric matrices, like the reference's gradients)
 *   grad_w            [n] fp64 gradient of the wsum weights, ACCUMULATED (zero it first), or NULL
 */
int sympa_siegel_dist_bwd(const double* z1, const double* z2, const double* grad_out, int64_t b, int n, int model,
                          int metric, const double* metric_w, double eps, double* grad_z1, double* grad_z2,
                          double* grad_w, int32_t* status, void* workspace, int64_t workspace_bytes, int flags, void* stream);

/* Backward of Model.forward (sympa/model.py:16-41 under runner.py:105): recomputes the distances and
 * ACCUMULATES (fp64 atomics; zero the buffers first)
 *   grad_table  [num_rows, 2, n, n]  the dense embeds.grad the reference's DDP all-reduces (train.py:59)
 *   grad_w      [n]  wsum weights (or NULL),      grad_scale  [1]  model scale (or NULL)
 * `out` (may be NULL) receives the forward values [b] again.
 */
int sympa_model_backward(const double* table, int64_t num_rows, int n, const int64_t* src, int64_t src_stride,
                         const int64_t* dst, int64_t dst_stride, int64_t b, int model, int metric,
                         const double* metric_w, double eps, const double* scale, double scale_coef,
                         const double* grad_out, double* grad_table, double* grad_w, double* grad_scale,
                         double* out, int32_t* status, void* workspace, int64_t workspace_bytes, int flags, void* stream);

/* One fused training step of the reference's loop (sympa/runner.py:98-105 with sympa/losses.py:10-19):
 *   d = Model.forward(triplets);  loss = loss_scale * sum |(d / graph_dist)^2 - 1|;  loss.backward()
 * in ONE kernel: distances, loss (accumulated into loss[0]), and the gradients of the table, of the wsum
 * weights and of the scale (all ACCUMULATED: zero them first, or keep accumulating over grad-accum steps;
 * loss_scale = 1 / grad_accum_steps, runner.py:104).  graph_dist: [b] fp64.  `out` (may be NULL): d.
 */
int sympa_model_loss_backward(const double* table, int64_t num_rows, int n, const int64_t* src, int64_t src_stride,
                              const int64_t* dst, int64_t dst_stride, const double* graph_dist, int64_t b, int model,
                              int metric, const double* metric_w, double eps, const double* scale, double scale_coef,
                              double loss_scale, double* loss, double* grad_table, double* grad_w, double* grad_scale,
                              double* out, int32_t* status, void* workspace, int64_t workspace_bytes, int flags, void* stream);

/* The same fused step with the table gradient left in per-pair form (no scatter): grad_src_rows[i] / grad_dst_rows[i]
 * ([b, 2, n, n] each, written) are the gradient rows of table[src[i]] / table[dst[i]] contributed by pair i.  This is
 * the message of the touched-row gradient exchange of data-parallel training (sympa_amd/distributed.py): 2 b rows per
 * rank instead of the dense [num_rows, 2, n, n] tensor the reference's DDP all-reduces (train.py:59) -- smaller
 * whenever 2 x global batch < num_rows.  sympa_scatter_add_rows then accumulates any list of such rows,
 *     grad_table[idx[r * idx_stride]] += alpha * rows[r],   r in [0, count)      (alpha = 1 / world for DDP's mean),
 * into the dense gradient the optimiser step reads (fp64 atomics; rows of 2 n^2 doubles). */
int sympa_model_loss_backward_rows(const double* table, int64_t num_rows, int n, const int64_t* src,
                                   int64_t src_stride, const int64_t* dst, int64_t dst_stride, const double* graph_dist,
                                   int64_t b, int model, int metric, const double* metric_w, double eps,
                                   const double* scale, double scale_coef, double loss_scale, double* loss,
                                   double* grad_src_rows, double* grad_dst_rows, double* grad_w, double* grad_scale,
                                   double* out, int32_t* status, void* workspace, int64_t workspace_bytes, int flags, void* stream);
int sympa_scatter_add_rows(const double* rows, const int64_t* idx, int64_t idx_stride, int64_t count, int n,
                           int64_t num_rows, double alpha, double* grad_table, int32_t* status, void* stream);
/* the same for rows of any length (spd: row_doubles = n^2) */
int sympa_scatter_add_flat_rows(const double* rows, const int64_t* idx, int64_t idx_stride, int64_t count, int row_doubles,
                                int64_t num_rows, double alpha, double* grad_table, int32_t* status, void* stream);

/* ---- the differentiable vector-valued distance ------------------------------------------------------------
 * v [b, n], ascending: the vector every metric of the library reduces (the reference's intermediate,
 * siegel_manifold.py:41-72; compact_dual.py:60 for model = DUAL).  With these entries ANY function of v -- an lp norm, a
 * learned weighting, a Weyl-chamber regulariser -- is ordinary code on the caller's side: the forward hands v out, the
 * backward takes dLoss/dv [b, n] (on the ascending v) and returns the gradients of the points.  Models UPPER, BOUNDED, DUAL;
 * n in [1, SYMPA_MAX_DIMS_BACKWARD]; one pair per lane (dims 1..6 in registers, dims 7..16 rolled loops over per-lane scratch).
 * The model scale is NOT part of these entries (callers multiply v by it).  `flags` is reserved and must be 0.  b == 0: no-op.
 *
 * sympa_model_vvd_forward: the gathered forward of sympa_model_forward (siegel_manifold.py:41-72 over model.py:16-30) with the
 * vector written instead of a metric of it: row i of vvd_out is bit for bit what sympa_siegel_dist_fwd(..., vvd_out) writes for
 * the points table[src[i]], table[dst[i]].  A pair with an out-of-range index sets SYMPA_ST_BAD_INDEX and gets a NaN row. */
int sympa_model_vvd_forward(const double* table, int64_t num_rows, int n, const int64_t* src, int64_t src_stride,
                            const int64_t* dst, int64_t dst_stride, int64_t b, int model, double eps, double* vvd_out,
                            int32_t* status, int flags, void* stream);
/* Backward of the vector-valued distance for pre-gathered points (what autograd computes through siegel_manifold.py:41-72 up to
 * the sorted v):  grad_v [b, n] in;  grad_z1, grad_z2 [b, 2, n, n] written (symmetric matrices);  vvd_out [b, n] or NULL receives
 * v again (from the backward's own eigen-decomposition: equal to the forward's to rounding, not bit for bit).  src == dst gives
 * v = 0 and a zero gradient; the cut locus of the dual model gives NaN and SYMPA_ST_NONFINITE. */
int sympa_siegel_vvd_bwd(const double* z1, const double* z2, const double* grad_v, int64_t b, int n, int model, double eps,
                         double* grad_z1, double* grad_z2, double* vvd_out, int32_t* status, int flags, void* stream);
/* The same through the table gather (siegel_manifold.py:41-72 under model.py:16-30): the two gradient rows of every pair are
 * ACCUMULATED into grad_table [num_rows, 2, n, n] (fp64 atomics; zero it first).  A pair with an out-of-range index sets
 * SYMPA_ST_BAD_INDEX, contributes nothing and gets a NaN row in vvd_out. */
int sympa_model_vvd_backward(const double* table, int64_t num_rows, int n, const int64_t* src, int64_t src_stride,
                             const int64_t* dst, int64_t dst_stride, int64_t b, int model, double eps, const double* grad_v,
                             double* grad_table, double* vvd_out, int32_t* status, int flags, void* stream);

/* ---- optimiser-side manifold operations over table rows (one [2,n,n] point per row) --------------------
 * egrad2rgrad: UpperHalfManifold.egrad2rgrad (sympa/manifolds/upper_half.py:25-40, Y G Y on both planes) /
 *              BoundedDomainManifold.egrad2rgrad (sympa/manifolds/bounded_domain.py:41-53, A G A, A = I - conj(Z) Z).
 */
int sympa_egrad2rgrad(const double* z, const double* u, int64_t b, int n, int model, double* out, void* stream);

/* inner(z, u, u) per row: UpperHalfManifold.inner (sympa/manifolds/upper_half.py:68-91, tr[y^-1 u y^-1 conj(u)]) /
 * BoundedDomainManifold.inner (sympa/manifolds/bounded_domain.py:86-116) for any complex tangent vector u:
 * out[i] = squared Riemannian norm of u[i] at z[i].  The second moment of geoopt's RiemannianAdam (train.py:69-70). */
int sympa_tangent_sqnorm(const double* z, const double* u, int64_t b, int n, int model, double* out, int32_t* status,
                         void* stream);

/* projx: SiegelManifold.projx + UpperHalfManifold.projx (siegel_manifold.py:130-137, upper_half.py:42-66,
 * csym_math.py:252-278): symmetrise, clamp the eigenvalues of Im z at eps, rows already inside are left
 * untouched; BoundedDomainManifold.projx as intended by bounded_domain.py:55-84: clamp the Takagi values
 * at 1 - eps.  projected_count[0] += number of rows that were moved (manifold.projected_points).
 * outside_word: caller-owned device int32 scratch word, one per call in flight (dims >= 7: the lanes-per-row kernel counts
 * the rows that left the eps-interior in it and the exact eigenvalue clamp runs gated on that count; the library keeps no
 * state of its own -- re-entrant across streams, devices and threads).  NULL: every row goes through the exact clamp
 * (one row per lane; same result, slower at dims >= 7).  Ignored at dims <= 6. */
int sympa_projx(const double* z, int64_t b, int n, int model, double eps, double* out, int32_t* projected_count,
                int32_t* status, int32_t* outside_word, void* stream);

/* One RiemannianSGD step over the whole table, in place (geoopt.optim.RiemannianSGD.step with momentum 0,
 * the optimiser train.py:66-68 builds; geoopt is absent from the reference tree, semantics restated):
 *     table <- retr(table, -lr * egrad2rgrad(table, grad + weight_decay * table)),  retr(x,u) = projx(x + u)
 * (sympa/manifolds/siegel_manifold.py:74-87).  outside_word: as in sympa_projx. */
int sympa_rsgd_step(double* table, const double* grad, int64_t num_rows, int n, int model, double lr,
                    double weight_decay, double eps, int32_t* projected_count, int32_t* status, int32_t* outside_word,
                    void* stream);

/* One RiemannianAdam step over the whole table, in place, ONE launch (geoopt.optim.RiemannianAdam as train.py:69-70 builds it:
 * `--optim radam`, eps = 1e-7, stabilize = None; geoopt is absent from the reference tree, the step is restated from
 * geoopt/optim/radam.py):  g = egrad2rgrad(x, grad + weight_decay x);  exp_avg <- beta1 exp_avg + (1 - beta1) g;
 * exp_avg_sq[row] <- beta2 exp_avg_sq[row] + (1 - beta2) inner(x, g, g);
 * x <- projx(x - lr (exp_avg / (1 - beta1^t)) / (sqrt(exp_avg_sq / (1 - beta2^t)) + eps_adam)).
 * exp_avg: [num_rows, 2, n, n], exp_avg_sq: [num_rows]; bias_pows: DEVICE words {beta1^t, beta2^t} of this step (the caller
 * advances them on the device, so a captured launch never carries a step count).  dims 1..6 (one row per lane); larger
 * tables use sympa_egrad2rgrad / sympa_tangent_sqnorm / sympa_projx. */
int sympa_radam_step(double* table, const double* grad, double* exp_avg, double* exp_avg_sq, int64_t num_rows, int n, int model,
                     double lr, double beta1, double beta2, double eps_adam, double weight_decay, const double* bias_pows,
                     double eps, int32_t* projected_count, int32_t* status, void* stream);

/* The gradient clip of the reference's loop (torch.nn.utils.clip_grad_norm_, sympa/runner.py:115) folded into the step:
 * sympa_sqnorm_accum adds sum(x^2) to acc[0] (device; call it once per gradient tensor after zeroing acc), and
 * sympa_rsgd_step_clipped is sympa_rsgd_step with every gradient row scaled by
 *     min(1, max_norm / (sqrt(total_sqnorm[0]) + 1e-6))
 * as it is loaded (the gradient buffer itself is left unscaled). */
int sympa_sqnorm_accum(const double* x, int64_t count, double* acc, void* stream);
/* The plain SGD step of the parameters that live on no manifold (the model's scale: RiemannianSGD on a Euclidean
 * parameter, geoopt/optim/rsgd.py) with the same folded clip: p <- p - lr * (coef * grad + weight_decay * p). */
int sympa_sgd_step_clipped(double* p, const double* grad, int64_t count, double lr, double weight_decay,
                           const double* total_sqnorm, double max_norm, void* stream);
int sympa_rsgd_step_clipped(double* table, const double* grad, int64_t num_rows, int n, int model, double lr,
                            double weight_decay, double eps, const double* total_sqnorm, double max_norm,
                            int32_t* projected_count, int32_t* status, int32_t* outside_word, void* stream);

/* ---- exponential and logarithm maps, upper and bounded models, dims 1..8 (one row or pair per lane) -----------------
 * The reference leaves both empty (sympa/manifolds/siegel_manifold.py:156-162) and retracts linearly (siegel_manifold.py:
 * 74-87: "Simple retraction: x + u. Correct retraction: exp_map(u)").  The maps belong to the invariant metric of the model,
 * the one the riem distance measures c times the length of (c = 1 upper, c = 2 bounded):
 *     riem dist(z, expmap(z, u)) = c |u|_z,    logmap(z, expmap(z, u)) = u,    expmap(z1, logmap(z1, z2)) = z2.
 * z, z1, z2, u, out: [b, 2, n, n]; tangent vectors are complex symmetric, both maps act on sym(u) and on the symmetric part of
 * the points.  sympa_expmap is pure: no clamp to the eps-interior (u = 0 returns sym(z) bit for bit).  sympa_logmap of two equal
 * points is an exact 0.  status: SYMPA_ST_NOT_PD (a point outside the domain), SYMPA_ST_NO_CONVERGENCE, SYMPA_ST_NONFINITE.
 * Other models / dims: SYMPA_ERR_BAD_ARG / SYMPA_ERR_UNSUPPORTED_DIMS.  Formulas and the solve route: siegel_expmap_math.hpp. */
int sympa_expmap(const double* z, const double* u, int64_t b, int n, int model, double* out, int32_t* status, void* stream);
int sympa_logmap(const double* z1, const double* z2, int64_t b, int n, int model, double* out, int32_t* status, void* stream);
/* One RiemannianSGD step over the whole table along the geodesic, in place, ONE launch:
 *     table <- projx(expmap(table, -lr * egrad2rgrad(table, grad + weight_decay * table)))
 * projected_count[0] += rows the clamp moved (the exponential map stays inside the domain; projx keeps the eps-interior). */
int sympa_rsgd_step_exp(double* table, const double* grad, int64_t num_rows, int n, int model, double lr, double weight_decay,
                        double eps, int32_t* projected_count, int32_t* status, void* stream);
/* One RiemannianAdam step over the whole table along the geodesic, in place, ONE launch, dims 1..8:
 *     g  = sym(egrad2rgrad(table, coef * grad + weight_decay * table)),   m1 = beta1 sym(exp_avg) + (1 - beta1) g,
 *     s1 = beta2 exp_avg_sq + (1 - beta2) |g|^2   with the norm of the invariant metric, the one the maps belong to,
 *     alpha = lr / ((1 - bias_pows[0]) (sqrt(s1 / (1 - bias_pows[1])) + eps_adam)),
 *     table <- projx(expmap(table, -alpha m1)),  exp_avg <- m1 parallel-transported along that geodesic (sympa_transp_exp with
 *     out_y: one factor, one eigendecomposition, one solve),  exp_avg_sq <- s1.
 * exp_avg [num_rows, 2, n, n], exp_avg_sq [num_rows]; bias_pows: device words (beta1^t, beta2^t) of this step, as in
 * sympa_radam_step.  total_sqnorm (device, may be NULL: no clip): coef = min(1, max_norm / (sqrt(total_sqnorm[0]) + 1e-6)), else
 * coef = 1.  projected_count[0] += rows the clamp moved; exp_avg of such a row stays as transported.  A zero gradient on zero
 * moments returns sym(table) bit for bit; so does lr = 0, with exp_avg <- m1.  status as sympa_rsgd_step_exp.  Other models /
 * dims: SYMPA_ERR_BAD_ARG / SYMPA_ERR_UNSUPPORTED_DIMS, before any launch. */
int sympa_radam_step_exp(double* table, const double* grad, double* exp_avg, double* exp_avg_sq, int64_t num_rows, int n, int model,
                         double lr, double beta1, double beta2, double eps_adam, double weight_decay, const double* bias_pows,
                         double eps, const double* total_sqnorm, double max_norm, int32_t* projected_count, int32_t* status,
                         void* stream);

/* ---- parallel transport along geodesics, upper and bounded models, dims 1..8 (one row per lane) ---------------------
 * The reference approximates (sympa/manifolds/siegel_manifold.py:142-154: "The formula for the parallel transport is very
 * complicated so we approximate it with the Euclidean parallel transport").  These are the transport of the invariant metric's
 * Levi-Civita connection, one congruence v' = G v G^T per row; z, z1, z2, u, v, out_y, out_v: [b, 2, n, n], tangent vectors
 * complex symmetric (the entries act on sym(u), sym(v) and the symmetric part of the points).
 * sympa_transp_exp (siegel_manifold.py:142-154): out_v = v transported from z along t -> expmap(z, t u) to expmap(z, u); with
 * out_y (may be NULL) out_y = expmap(z, u) from the same factor, eigendecomposition and solve.  u = 0 returns sym(v) (and
 * sym(z)) bit for bit.  out_v may alias v, out_y may alias z.  A tangent so long that tanh rounds to 1 sets status, as in
 * sympa_expmap.  status: SYMPA_ST_NOT_PD, SYMPA_ST_NO_CONVERGENCE, SYMPA_ST_NONFINITE.  Other models / dims:
 * SYMPA_ERR_BAD_ARG / SYMPA_ERR_UNSUPPORTED_DIMS.  Formulas and the evaluation form: siegel_transp_math.hpp. */
int sympa_transp_exp(const double* z, const double* u, const double* v, int64_t b, int n, int model, double* out_y, double* out_v,
                     int32_t* status, void* stream);
/* sympa_transp (siegel_manifold.py:142-154): out_v = v transported from z1 to z2 along the geodesic between them; logmap(z1, z2)
 * is never formed.  z2 = z1 returns sym(v) bit for bit.  out_v may alias v. */
int sympa_transp(const double* z1, const double* z2, const double* v, int64_t b, int n, int model, double* out_v, int32_t* status,
                 void* stream);

/* The backward half of a training step inside a replayed hipGraph (sympa/runner.py:98-105), dims 1..16 (wave_partials: dims
 * 1..8).  Like
 * sympa_model_loss_backward (grad_table given: fp64-atomic scatter into the dense gradient) or
 * sympa_model_loss_backward_rows (grad_rows [2 b, 2, n, n] given: rows [0, b) belong to src, [b, 2 b) to dst), plus
 *   step_counter   device int64 c (may be NULL = 0): the launch processes pairs [c b, (c + 1) b) of src / dst / graph_dist,
 *                  i.e. an epoch's shuffled triplets (train.py:105-110) stay in ONE buffer, sympa_rsgd_step_fused increments
 *                  c, and the replayed graph needs no per-step copy of the batch;
 *   wave_partials  (rows form; may be NULL) [ceil(b / 64)][2 + n] fp64, WRITTEN: per-wavefront sums of the loss, of
 *                  d loss / d scale and of d loss / d w_k, which sympa_segment_sum_rows adds to loss / grad_scale / grad_w in
 *                  a fixed order -- together with the row sums below this makes a training step bitwise reproducible
 *                  (the reference's CPU autograd is; fp64 atomics are not).  With wave_partials loss / grad_* are untouched. */
int sympa_model_train_backward(const double* table, int64_t num_rows, int n, const int64_t* src, int64_t src_stride,
                               const int64_t* dst, int64_t dst_stride, const double* graph_dist, int64_t b,
                               const int64_t* step_counter, int model, int metric, const double* metric_w, double eps,
                               const double* scale, double scale_coef, double loss_scale, double* loss, double* grad_table,
                               double* grad_rows, double* grad_w, double* grad_scale, double* wave_partials, int32_t* status,
                               void* workspace, int64_t workspace_bytes, int flags, void* stream);

/* Deterministic counterpart of sympa_scatter_add_flat_rows ("sort-by-row + segmented sum"):
 *   grad_table[r] (= | +=, by `accumulate`) alpha * sum_{p in [rowptr[r], rowptr[r + 1])} rows[order[p]]     r = 0 .. num_rows - 1
 * added in the order of `order`, no atomics: every element is written by exactly one thread, rows nobody touched are
 * written as 0 when accumulate = 0 (no zeroing pass).  order: int32 slot numbers (rows of `rows`, row_doubles each)
 * sorted by table row -- stable, so the order inside a row is the batch order; rowptr: int32 [num_rows + 1].  With
 * step_counter c (device int64, may be NULL) the lists of batch c are used: order + c * order_stride, rowptr + c *
 * (num_rows + 1) (sympa_amd/train_step.py builds them for a whole epoch with one sort).  wave_partials (may be NULL): see
 * sympa_model_train_backward; partial_stride = 2 + n (doubles per wavefront), num_weights = n for the wsum metric, else 0
 * (then grad_w may be NULL); grad_scale may be NULL.  sq_partials (may be NULL; needs wave_partials): [sympa_segment_sum_
 * partials(num_rows, row_doubles)] fp64, WRITTEN: one sum of squares of the finished gradient per block in a fixed tree, the
 * last one for the scale / weight gradients -- sympa_rsgd_step_fused adds them in index order instead of making its own pass. */
int64_t sympa_segment_sum_partials(int64_t num_rows, int row_doubles);
int sympa_segment_sum_rows(const double* rows, const int32_t* order, const int32_t* rowptr, int64_t num_rows, int row_doubles,
                           int64_t order_stride, const int64_t* step_counter, double alpha, int accumulate, double* grad_table,
                           const double* wave_partials, int64_t num_waves, int partial_stride, int num_weights, double* loss,
                           double* grad_scale, double* grad_w, double* sq_partials, void* stream);

/* The optimiser side of one training step as ONE launch (sympa/runner.py:113-118: clip_grad_norm_(parameters, max_norm),
 * optimizer.step(), zero_grad()), dims 1..6, tables of at most (CUs x 256) rows (a grid barrier inside: every block must be
 * resident; otherwise SYMPA_ERR_UNSUPPORTED_DIMS -- use sympa_sqnorm_accum + sympa_rsgd_step_clipped + sympa_sgd_step_clipped):
 *   total = ||grad||^2 + sum_k ||extra_grad[k]||^2, summed in a fixed order (bitwise reproducible);
 *   coef = max_norm > 0 ? min(1, max_norm / (sqrt(total) + 1e-6)) : 1;
 *   table <- retr(table, -lr * egrad2rgrad(table, coef * grad + weight_decay * table))           (sympa_rsgd_step)
 *   extra_param[k] <- extra_param[k] - extra_lr[k] * (coef * extra_grad[k] + extra_weight_decay[k] * extra_param[k])
 *   zero_grads != 0: grad and extra_grad[k] are zeroed (the next step's backward accumulates into them);
 *   step_counter (device int64, may be NULL) += 1: the batch index the next sympa_model_loss_backward_indexed call reads.
 * extra_*: up to 2 parameters without a manifold (the model's scale, the wsum weights), 1..64 elements each.
 * sq_partials (may be NULL): partial sums of squares that sympa_segment_sum_rows left -- then `total` is their sum in index
 * order and the kernel makes no pass over the gradient and needs no barrier (the deterministic training step).
 * workspace: sympa_rsgd_step_fused_workspace_bytes(num_rows) bytes of device memory, ZERO before the first call (the
 * kernel leaves it ready for the next one); one workspace per concurrently running step. */
int64_t sympa_rsgd_step_fused_workspace_bytes(int64_t num_rows);
int sympa_rsgd_step_fused(double* table, double* grad, int64_t num_rows, int n, int model, double lr, double weight_decay,
                          double eps, double max_norm, int zero_grads, double* const* extra_param, double* const* extra_grad,
                          const int* extra_count, const double* extra_lr, const double* extra_weight_decay, int num_extra,
                          void* workspace, int64_t workspace_bytes, const double* sq_partials, int num_sq_partials,
                          int64_t* step_counter, int32_t* projected_count, int32_t* status, void* stream);

/* The same launch for `--optim radam` (train.py:69-70: geoopt.optim.RiemannianAdam, eps = 1e-7): clip, one RiemannianAdam
 * step of the table (sympa_radam_step's formula), the ordinary Adam step of the plain parameters, zero_grad, step counter.
 * bias_pows / extra_bias_pows[k]: device words {beta1^t, beta2^t} as the PREVIOUS step left them (1, 1 before the first):
 * the kernel uses beta * word as this step's power and stores it back, so a replayed launch carries no step count.
 * Same limits and workspace as sympa_rsgd_step_fused. */
int sympa_radam_step_fused(double* table, double* grad, double* exp_avg, double* exp_avg_sq, double* bias_pows, int64_t num_rows,
                           int n, int model, double lr, double beta1, double beta2, double eps_adam, double weight_decay,
                           double eps, double max_norm, int zero_grads, double* const* extra_param, double* const* extra_grad,
                           double* const* extra_exp_avg, double* const* extra_exp_avg_sq, double* const* extra_bias_pows,
                           const int* extra_count, const double* extra_lr, const double* extra_weight_decay, int num_extra,
                           void* workspace, int64_t workspace_bytes, const double* sq_partials, int num_sq_partials,
                           int64_t* step_counter, int32_t* projected_count, int32_t* status, void* stream);

/* ---- SPD model (manifold "spd": geoopt.manifolds.SymmetricPositiveDefinite, sympa/embeddings.py:6,70-72,142) ----
 * Points are [n, n] fp64 symmetric positive definite matrices (upper triangle read), n <= 16.
 * dist = || log(x^-1/2 y x^-1/2) ||_F  (geoopt's default affine-invariant metric; geoopt is absent from the
 * reference tree: parity unpinned).  sympa_spd_model_forward is Model.forward for that model
 * (sympa/model.py:16-41) with a [num_rows, n, n] table.  flags: 0 or SYMPA_FLAG_GENERIC.
 * 6 <= n <= 16 run the sixteen-lanes-per-pair kernel (csrc/spd_coop.hpp: one instantiation per n, lanes r >= n of a group
 * are phantoms; factorisation, solves and the first n - 10 Householder steps sixteen lanes per pair, the trailing block of at
 * most 10 x 10 and the QL iteration one pair per lane), n <= 5 the runtime-n one-lane-per-pair kernel. */
int sympa_spd_dist_fwd(const double* x, const double* y, int64_t b, int n, double* out, int32_t* status, int flags,
                       void* stream);
int sympa_spd_model_forward(const double* table, int64_t num_rows, int n, const int64_t* src, int64_t src_stride,
                            const int64_t* dst, int64_t dst_stride, int64_t b, const double* scale, double scale_coef,
                            double* out, int32_t* status, int flags, void* stream);

/* Packed table of the spd model, n = 6..16 (csrc/spd.hip; the Siegel counterpart is sympa_table_pack): one row of n (n + 1)
 * doubles per point -- an n x n image whose upper triangle (diagonal included) is the point and whose strict lower triangle is the
 * UNIT factor Lh of x = Lh D Lh^T, then the n values D^-1/2 -- made once per table version.  sympa_spd_model_forward_packed is
 * sympa_spd_model_forward reading it: the sixteen-lanes-per-pair kernel without its factorisation (~310 of the ~1 170 VALU
 * instructions of a round of four pairs), the first point's image read twice (symmetric rows for y - x, then its factor rows), the
 * second point's upper triangle only.  Same values to rounding (the factor is the one the dense kernel computes).  A point that
 * is not positive definite is reported by the pack call (SYMPA_ST_NOT_PD) and every pair it enters later comes out NaN and
 * flagged.  sympa_spd_table_pack_bytes returns 0 where no packed kernel exists (n < 6).  Replaces the per-pair factorisation inside
 * geoopt's SymmetricPositiveDefinite.dist (sympa/embeddings.py:70-72,142; parity UNPINNED like every spd entry). */
int64_t sympa_spd_table_pack_bytes(int64_t num_rows, int n);
int sympa_spd_table_pack_refresh(const double* table, int64_t num_rows, int n, void* pack, int64_t pack_bytes, void* digest_state,
                                 int flags, int32_t* status, void* stream);
int sympa_spd_table_pack(const double* table, int64_t num_rows, int n, void* pack, int64_t pack_bytes, int32_t* status,
                         void* stream);
int sympa_spd_model_forward_packed(const void* pack, int64_t pack_bytes, int64_t num_rows, int n, const int64_t* src,
                                   int64_t src_stride, const int64_t* dst, int64_t dst_stride, int64_t b, const double* scale,
                                   double scale_coef, double* out, int32_t* status, int flags, void* stream);

/* ---- SPD model, training path (PARITY UNPINNED like the forward; formulas restated from geoopt's published source,
 * pinned by 50-digit finite differences, tests/golden/spd_n*.npz) ----
 * sympa_spd_backward_rows: backward of SymmetricPositiveDefinite.dist / of Model.forward for the spd model
 * (sympa/model.py:16-41 under runner.py:105).  Pair i = (x[src[i]], y[dst[i]]) (src = dst = NULL: rows i of x and y).
 * Either grad_out [b] (dLoss/d out) or graph_dist [b] is given; with graph_dist the AverageDistortionLoss of
 * sympa/losses.py:10-19 is fused in: loss[0] += loss_scale * sum |(out / graph_dist)^2 - 1|.
 * grad_x_rows / grad_y_rows [b, n, n] are WRITTEN with the (symmetric) gradient rows of the two points of each pair;
 * accumulate them into a table gradient with sympa_scatter_add_flat_rows.  grad_scale [1] accumulated, out [b] optional.
 * n >= 3 runs sixteen lanes per pair (csrc/spd_coop_bwd.hpp); flags: 0, SYMPA_FLAG_GENERIC (one lane per pair over scratch)
 * or SYMPA_FLAG_COOP (see above).  The row operations below run sixteen lanes per row for n >= 3 (csrc/spd_coop_table.hpp;
 * environment SYMPA_SPD_TABLE_GENERIC=1 keeps the one-row-per-lane kernel for measurements; projx always uses it). */
int sympa_spd_backward_rows(const double* x, const double* y, int64_t num_rows, int n, const int64_t* src,
                            int64_t src_stride, const int64_t* dst, int64_t dst_stride, int64_t b, const double* scale,
                            double scale_coef, const double* grad_out, const double* graph_dist, double loss_scale,
                            double* loss, double* grad_x_rows, double* grad_y_rows, double* grad_scale, double* out,
                            int32_t* status, void* workspace, int64_t workspace_bytes, int flags, void* stream);
/* workspace (both backward entries; caller-owned device scratch, 16-byte aligned, may be NULL): with at least
 * sympa_spd_backward_workspace_bytes(b, n) bytes the THREE-KERNEL backward runs where it is built (n = 9..16, csrc/
 * spd_coop_bwd3_kernel.hpp): Householder form sixteen lanes per pair, then eigenvalues (lockstep QL) and eigenvectors (inverse
 * iteration) ONE PAIR PER LANE with the vectors parked in the workspace, then the gradient rows sixteen lanes per pair again --
 * 3x the kernel that runs the QL with accumulated rotations in the sixteen-lanes layout; pairs with a block of more than four
 * close eigenvalues (y = c x) are finished by that kernel in a second launch behind it.  NULL, a size of 0 or SYMPA_FLAG_COOP /
 * SYMPA_FLAG_GENERIC: the other kernels, as before.  sympa_spd_backward_workspace_bytes returns 0 where no kernel uses one. */
int64_t sympa_spd_backward_workspace_bytes(int64_t b, int n);
/* The same with the scatter inside the kernel (n >= 3, index lists required): the gradient rows of each pair are added
 * into grad_table [num_rows, n, n] with fp64 atomics, consecutive lanes on consecutive doubles -- one launch for
 * Model.forward + AverageDistortionLoss + backward + embedding-gradient accumulation (runner.py:98-118 for the spd model). */
int sympa_spd_loss_backward(const double* table, int64_t num_rows, int n, const int64_t* src, int64_t src_stride,
                            const int64_t* dst, int64_t dst_stride, int64_t b, const double* scale, double scale_coef,
                            const double* grad_out, const double* graph_dist, double loss_scale, double* loss,
                            double* grad_table, double* grad_scale, double* out, int32_t* status, void* workspace, int64_t workspace_bytes, int flags,
                            void* stream);
/* geoopt SymmetricPositiveDefinite.egrad2rgrad (x sym(u) x), .projx (V |lambda| V^T of sym(x); projected_count += rows with
 * a negative eigenvalue), and one geoopt.optim.RiemannianSGD step over the table in place,
 *     x <- retr(x, -lr * egrad2rgrad(x, grad + weight_decay * x)),   retr(x, u) = sym(x + u + u x^-1 u / 2),
 * with the gradient clip of runner.py:115 folded in when total_sqnorm (device, squared total norm) is given. */
int sympa_spd_egrad2rgrad(const double* x, const double* u, int64_t b, int n, double* out, void* stream);
int sympa_spd_projx(const double* x, int64_t b, int n, double* out, int32_t* projected_count, int32_t* status, void* stream);
int sympa_spd_rsgd_step(double* table, const double* grad, int64_t num_rows, int n, double lr, double weight_decay,
                        const double* total_sqnorm, double max_norm, int32_t* status, void* stream);
/* One geoopt.optim.RiemannianAdam step (train.py:69-70, `--optim radam`) over the spd table in place, as one launch
 * (parity unpinned with respect to geoopt like every spd entry):
 *     S = coef sym(grad) + weight_decay x,  r = x S x,  I = tr(x^-1 r x^-1 r),
 *     m1 = beta1 m + (1 - beta1) r,  s1 = beta2 s + (1 - beta2) I,
 *     u = -lr / (1 - beta1^t) / (sqrt(s1 / (1 - beta2^t)) + eps_adam) m1,   x <- retr(x, u) (sympa_spd_rsgd_step's),
 *     exp_avg <- the affine-invariant parallel transport of m1 along the geodesic to the new point,  exp_avg_sq <- s1.
 * exp_avg: [num_rows, n, n] (read as sym(.)); exp_avg_sq: [num_rows], one value per point.  bias_pows: device pair
 * (beta1^t, beta2^t) of this step, as for sympa_radam_step; total_sqnorm / max_norm: the folded clip, as for sympa_spd_rsgd_step.
 * SYMPA_ERR_BAD_ARG: a null table, grad, exp_avg, exp_avg_sq or bias_pows, a beta outside [0, 1), eps_adam <= 0, total_sqnorm
 * with max_norm <= 0;  SYMPA_ERR_UNSUPPORTED_DIMS: n outside [1, 16].  A row that does not factor raises SYMPA_ST_NOT_PD. */
int sympa_spd_radam_step(double* table, const double* grad, double* exp_avg, double* exp_avg_sq, int64_t num_rows, int n,
                         double lr, double beta1, double beta2, double eps_adam, double weight_decay, const double* bias_pows,
                         const double* total_sqnorm, double max_norm, int32_t* status, void* stream);
/* The exponential map, logarithm and geodesic of the affine-invariant metric, and the RiemannianSGD step that moves along the
 * geodesic (parity unpinned with respect to geoopt like every spd entry).  With x = L L^T and, for a
 * symmetric W, A = L^-1 W L^-T = V diag(a) V^T:
 *     expmap(x, u)      = x + L V diag(expm1(a)) V^T L^T,            W = sym(u)     (= x^1/2 exp(x^-1/2 sym(u) x^-1/2) x^1/2)
 *     logmap(x, y)      =     L V diag(log1p(a)) V^T L^T,            W = y - x
 *     geodesic(t, x, y) = x + L V diag(expm1(t log1p(a))) V^T L^T,   W = y - x,  any finite t (0: x, 1: y to rounding)
 *     step:  x <- expmap(x, -lr x S x) = x + L V diag(expm1(-lr c)) V^T L^T,   L^T S L = V diag(c) V^T,
 *            S = coef sym(grad) + weight_decay x,  coef the folded clip of sympa_spd_rsgd_step (total_sqnorm, max_norm)
 * x, y, u, out: [b, n, n], fp64; x and y are read as their upper triangles, u as sym(u); the step reads sym(table row), sym(grad
 * row) and works in place (all of a row's loads stand before its stores).  out may alias nothing.  Outputs are symmetric bit for
 * bit; u = 0, t = 0, lr = 0 return the (symmetric) point bit for bit and y == x an exact zero logarithm.  The step's result is
 * positive definite for every step length: no projection, no counter.  n in [1, 16]; flags: 0 or SYMPA_FLAG_GENERIC (the
 * one-row-per-lane kernel at every n; the default runs sixteen lanes per row for n >= 3).  b == 0: no-op.
 * SYMPA_ERR_BAD_ARG: null required pointers, b < 0, other flags, a non-finite t, total_sqnorm with max_norm <= 0;
 * SYMPA_ERR_UNSUPPORTED_DIMS: n outside the range.  An x that does not factor (for logmap / geodesic also a y that is not
 * positive definite against x) raises SYMPA_ST_NOT_PD, is counted in status[1] as in sympa_spd_rsgd_step, and its output row is
 * NaN; SYMPA_ST_NONFINITE: a tangent so long that expm1 overflows. */
int sympa_spd_expmap(const double* x, const double* u, int64_t b, int n, double* out, int32_t* status, int flags, void* stream);
int sympa_spd_logmap(const double* x, const double* y, int64_t b, int n, double* out, int32_t* status, int flags, void* stream);
int sympa_spd_geodesic(const double* x, const double* y, double t, int64_t b, int n, double* out, int32_t* status, int flags,
                       void* stream);
int sympa_spd_rsgd_step_exp(double* table, const double* grad, int64_t num_rows, int n, double lr, double weight_decay,
                            const double* total_sqnorm, double max_norm, int32_t* status, int flags, void* stream);

/* ---- spd: the differentiable vector-valued distance ------------------------------------------
 * v [b, n] = log(lam_j) ASCENDING, lam = the eigenvalues of x^-1 y, evaluated as log(1 + a_j), a = the eigenvalues of
 * L^-1 (y - x) L^-T, x = L L^T.  v is SIGNED (lam_j < 1 gives v_j < 0), unlike the Siegel v above; the affine-invariant distance
 * is ||v||_2, the Finsler distances sum_j |v_j| and max_j |v_j|.  With these entries any function of v is ordinary code on the
 * caller's side: the forward hands v out, the backward takes dLoss/dv [b, n] (on the ascending v).  n in [1, 16]; flags: 0 or
 * SYMPA_FLAG_GENERIC (the one-pair-per-lane kernels at every n).  The model scale is NOT part of these entries.  b == 0: no-op.
 * Null required pointers, b < 0, other flags: SYMPA_ERR_BAD_ARG; n outside the range: SYMPA_ERR_UNSUPPORTED_DIMS.
 * Status bits as for sympa_spd_dist_fwd / sympa_spd_backward_rows; the row of v of a pair whose eigenvalues came out NaN (flagged
 * SYMPA_ST_NOT_PD / SYMPA_ST_NONFINITE) is unspecified.
 * Ties: eigenvalues that agree exactly are ranked in index order and their eigenvectors are whatever the QL returns; the backward
 * is well defined there whenever grad_v is constant across the tied block.  x == y gives v = 0 and exact zero gradients.
 *
 * sympa_spd_vvd_fwd: pre-gathered points x, y [b, n, n] (upper triangle read).  n <= 5 one lane per pair, n = 6..16 sixteen lanes
 * per pair (csrc/spd_vvd_kernel.hpp: spd_vvd_coop_fwd_kernel, the rounds of the distance kernel, rows of v staged through the LDS). */
int sympa_spd_vvd_fwd(const double* x, const double* y, int64_t b, int n, double* vvd_out, int32_t* status, int flags, void* stream);
/* The same for pair i = (table[src[i]], table[dst[i]]), table [num_rows, n, n]: row i is bit for bit what sympa_spd_vvd_fwd writes
 * for the gathered points.  A pair with an out-of-range index sets SYMPA_ST_BAD_INDEX and gets a NaN row. */
int sympa_spd_model_vvd_forward(const double* table, int64_t num_rows, int n, const int64_t* src, int64_t src_stride,
                                const int64_t* dst, int64_t dst_stride, int64_t b, double* vvd_out, int32_t* status, int flags,
                                void* stream);
/* Backward for pre-gathered points:  grad_v [b, n] in;  grad_x, grad_y [b, n, n] written (symmetric),
 *   grad_y =  sym(L^-T V diag(grad_v[rank(k)] / (1 + a_k)) V^T L^-1),   grad_x = -sym(L^-T V diag(grad_v[rank(k)]) V^T L^-1);
 * vvd_out [b, n] or NULL receives v again (from the backward's own eigen-decomposition: equal to the forward's to rounding).
 * n <= 2 one lane per pair (Rayleigh-refined eigenvalues), n = 3..16 sixteen lanes per pair (spd_vvd_coop_bwd_kernel: the
 * one-kernel form of sympa_spd_backward_rows with SYMPA_FLAG_COOP, a cotangent row per pair in place of log(1 + a_k) / dist). */
int sympa_spd_vvd_bwd(const double* x, const double* y, const double* grad_v, int64_t b, int n, double* grad_x, double* grad_y,
                      double* vvd_out, int32_t* status, int flags, void* stream);
/* The same through the table gather: the two gradient rows of every pair are ACCUMULATED into grad_table [num_rows, n, n] (fp64
 * atomics; zero it first; n >= 3 without SYMPA_FLAG_GENERIC: consecutive lanes on consecutive doubles).  A pair with an out-of-range
 * index sets SYMPA_ST_BAD_INDEX, contributes nothing and gets a NaN row in vvd_out (or NULL). */
int sympa_spd_model_vvd_backward(const double* table, int64_t num_rows, int n, const int64_t* src, int64_t src_stride,
                                 const int64_t* dst, int64_t dst_stride, int64_t b, const double* grad_v, double* grad_table,
                                 double* vvd_out, int32_t* status, int flags, void* stream);

/* ---- spd: rows of the all-pairs distance matrix under any of the three metrics --------------------
 * Runner.build_distance_matrix (sympa/runner.py:142-154) for the spd model, with the pair computed from its number (no pair list):
 *     out[(i - row_begin) * num_rows + j] = metric(v(x_i, x_j)) * max(scale[0] / scale_coef, 0.1),
 * i in [row_begin, row_begin + row_count), j in [0, num_rows); table [num_rows, n, n] (upper triangles read), n in [1, 16];
 * metric = SYMPA_METRIC_RIEM ||v||_2, SYMPA_METRIC_FONE sum_j |v_j|, SYMPA_METRIC_FINF max_j |v_j| of the vector-valued distance
 * above; scale may be NULL.  The diagonal is exactly 0, also for a point that is not positive definite; every off-diagonal pair
 * such a point enters comes out NaN and sets SYMPA_ST_NOT_PD; a non-finite value sets SYMPA_ST_NONFINITE.
 * n = 6..16: sixteen lanes per pair (csrc/spd_allpairs_kernel.hpp: a wave owns one source row and 64 consecutive columns and
 * factors the source once); n <= 5 or SYMPA_FLAG_GENERIC: one lane per pair.  flags: 0, SYMPA_FLAG_GENERIC and / or
 * SYMPA_FLAG_NO_SYMMETRY.  For the full matrix (row_begin = 0, row_count = num_rows) without SYMPA_FLAG_NO_SYMMETRY only i <= j
 * is evaluated and the value is stored at (i, j) and (j, i); a row block always evaluates both orders.
 * The value at (i, j) depends on x_i, x_j, n, metric, scale and the route (generic or not) alone: a row block is bit for bit the
 * same rows of the SYMPA_FLAG_NO_SYMMETRY full matrix, whatever the split into blocks, and a NaN pair changes no other pair.
 * row_count == 0: no-op.  A null table / out, a block outside [0, num_rows], another metric, other flags or scale_coef == 0 with
 * a scale: SYMPA_ERR_BAD_ARG; n outside [1, 16]: SYMPA_ERR_UNSUPPORTED_DIMS, like the other spd entries; all before any launch. */
int sympa_spd_all_pairs_dist(const double* table, int64_t num_rows, int n, int64_t row_begin, int64_t row_count,
                             int metric, const double* scale, double scale_coef, double* out, int32_t* status,
                             int flags, void* stream);

/* ---- Vector models (manifolds "euclidean", "poincare", "lorentz", "sphere", "prod-hysph", "prod-hyhy", "prod-hyeu",
 * "prod-sphsph": geoopt constructors behind ManifoldFactory, sympa/embeddings.py:130-158, and VectorEmbeddings,
 * sympa/embeddings.py:82-90).  geoopt is not in the reference tree: PARITY UNPINNED like the spd entries; the definitions are
 * the project's own and the kernels are pinned to 50-digit evaluations of them
 * (tests/golden/exact_vector_*.npz).  A point is a row of `dims` doubles (1 <= dims <= 1024, else SYMPA_ERR_UNSUPPORTED_DIMS),
 * split into one or two factors; products need even dims, sphere / lorentz factors at least two coordinates
 * (SYMPA_ERR_BAD_ARG).  Per factor, J = diag(-1, 1, ..., 1) for lorentz and I otherwise,
 *     dd = sum J_i (x_i - y_i)^2,  xx = sum x_i^2,  yy = sum y_i^2,
 *     E: d = sqrt(dd)    P: d = 2 asinh sqrt(dd / ((1 - xx)(1 - yy)))    L: d = 2 asinh sqrt(max(dd, 0) / 4)
 *     S: d = 2 asin sqrt(min(dd / 4, 1)),   a product: sqrt(d_1^2 + d_2^2).
 * A Poincare point with xx >= 1 gives NaN and SYMPA_ST_NOT_PD, a non-finite value NaN and SYMPA_ST_NONFINITE.  G lanes per
 * pair / row, G = 1..64 from dims (csrc/vector_models.hip); a pair's value is the same bits in all three forward entries.
 * `flags` is reserved (0). */
#define SYMPA_VECTOR_EUCLIDEAN 0
#define SYMPA_VECTOR_POINCARE 1
#define SYMPA_VECTOR_LORENTZ 2
#define SYMPA_VECTOR_SPHERE 3
#define SYMPA_VECTOR_PROD_HYSPH 4
#define SYMPA_VECTOR_PROD_HYHY 5
#define SYMPA_VECTOR_PROD_HYEU 6
#define SYMPA_VECTOR_PROD_SPHSPH 7
/* manifold.dist(x, y) on rows i of x and y [b, dims] (geoopt Manifold.dist behind sympa/model.py:32-38) */
int sympa_vector_dist_fwd(const double* x, const double* y, int64_t b, int dims, int model, double* out, int32_t* status,
                          int flags, void* stream);
/* Model.forward (sympa/model.py:16-41) over a [num_rows, dims] table: gather, distance, scale */
int sympa_vector_model_forward(const double* table, int64_t num_rows, int dims, const int64_t* src, int64_t src_stride,
                               const int64_t* dst, int64_t dst_stride, int64_t b, int model, const double* scale,
                               double scale_coef, double* out, int32_t* status, int flags, void* stream);
/* Runner.build_distance_matrix (sympa/runner.py:142-154): rows [row_begin, row_begin + row_count) of the N x N matrix into
 * out [row_count, num_rows]; the same pair kernel with i = row_begin + p / N, j = p % N computed in the kernel, no pair list.
 * The diagonal is exactly 0 and (i, j) is bit-equal to (j, i). */
int sympa_vector_all_pairs_dist(const double* table, int64_t num_rows, int dims, int64_t row_begin, int64_t row_count, int model,
                                const double* scale, double scale_coef, double* out, int32_t* status, int flags, void* stream);
/* Backward of the two entries above (sympa/model.py:16-41 under runner.py:105), shaped like sympa_spd_backward_rows: pair
 * i = (x[src[i]], y[dst[i]]) (src = dst = NULL: rows i); grad_out [b] or graph_dist [b] (AverageDistortionLoss of
 * sympa/losses.py:10-19 fused: loss[0] += loss_scale * sum |(out / graph_dist)^2 - 1|); grad_x_rows / grad_y_rows [b, dims]
 * are WRITTEN (accumulate them with sympa_scatter_add_flat_rows or sympa_segment_sum_rows, row_doubles = dims); grad_scale [1]
 * accumulated, out [b] optional.  A factor with q == 0 (src == dst among them) contributes a zero gradient, never NaN. */
int sympa_vector_backward_rows(const double* x, const double* y, int64_t num_rows, int dims, int model, const int64_t* src,
                               int64_t src_stride, const int64_t* dst, int64_t dst_stride, int64_t b, const double* scale,
                               double scale_coef, const double* grad_out, const double* graph_dist, double loss_scale,
                               double* loss, double* grad_x_rows, double* grad_y_rows, double* grad_scale, double* out,
                               int32_t* status, int flags, void* stream);
/* geoopt's egrad2rgrad, projx (projected_count += rows whose Poincare factor was rescaled to norm 1 - 1e-5) and one
 * geoopt.optim.RiemannianSGD step (momentum 0; train.py:66-68) over the table in place, per factor
 *     g <- grad + weight_decay x,   x <- retr(x, -lr egrad2rgrad(x, g)),
 * with the gradient clip of runner.py:115 folded in when total_sqnorm (device, squared total norm) is given. */
int sympa_vector_egrad2rgrad(const double* x, const double* u, int64_t b, int dims, int model, double* out, void* stream);
int sympa_vector_projx(const double* x, int64_t b, int dims, int model, double* out, int32_t* projected_count, int32_t* status,
                       void* stream);
int sympa_vector_rsgd_step(double* table, const double* grad, int64_t num_rows, int dims, int model, double lr, double weight_decay,
                           const double* total_sqnorm, double max_norm, int32_t* projected_count, int32_t* status, void* stream);
/* One geoopt.optim.RiemannianAdam step (geoopt optim/radam.py; train.py:69-70: `--optim radam`, eps = 1e-7) over the table in
 * place, as one kernel (geoopt is not in the reference tree: PARITY UNPINNED, pinned to 50-digit
 * evaluations of the project's definitions, tests/golden/exact_vector_*_radam*.npz).  Per factor
 *     g = coef grad + weight_decay x,  r = egrad2rgrad(x, g),  m1 = beta1 m + (1 - beta1) r,  s1 = beta2 s + (1 - beta2) I(x, r),
 *     y = retr(x, -lr (m1 / (1 - beta1^t)) / (sqrt(s1 / (1 - beta2^t)) + eps_adam)),
 *     table <- y,  exp_avg <- the parallel transport of m1 from x to y,  exp_avg_sq <- s1,
 * I = geoopt's component_inner: r_i^2 per coordinate for a euclidean factor; one value per factor otherwise (poincare
 * (2 / (1 - xx))^2 sum r_i^2, sphere sum r_i^2, lorentz max(<r, r>_L, 0)), held in every coordinate of the factor: exp_avg and
 * exp_avg_sq are [num_rows, dims] like the table, and the incoming value of a factor is read at its first coordinate.
 * bias_pows: device pair (beta1^t, beta2^t) of this step, as for sympa_radam_step; total_sqnorm / max_norm: the folded clip,
 * projected_count and status as for sympa_vector_rsgd_step.  num_rows == 0 is a no-op; a null table / grad / exp_avg /
 * exp_avg_sq / bias_pows, a beta outside [0, 1) or eps_adam <= 0 is SYMPA_ERR_BAD_ARG. */
int sympa_vector_radam_step(double* table, const double* grad, double* exp_avg, double* exp_avg_sq, int64_t num_rows, int dims,
                            int model, double lr, double beta1, double beta2, double eps_adam, double weight_decay,
                            const double* bias_pows, const double* total_sqnorm, double max_norm, int32_t* projected_count,
                            int32_t* status, void* stream);

/* Per-row average precision of a block of rows of the all-pairs distance matrix: the ranking half of
 * MeanAveragePrecisionMetric.calculate_metric (sympa/metrics.py:39-63) over the matrix Runner.calculate_mAP builds
 * (sympa/runner.py:137-154), without sorting the rows (csrc/map_rank.hip).
 *   dist        [row_count, ld] fp64: rows row_begin .. row_begin + row_count - 1 of the N x N matrix (N = num_rows), row i
 *               holding d(i, k) with i the source (sympa_all_pairs_dist / sympa_all_pairs_dist_packed with
 *               SYMPA_FLAG_NO_SYMMETRY); 8-byte aligned, ld >= num_rows
 *   rowptr      [num_rows + 1] int64, cols [rowptr[num_rows]] int32: neighbour lists (CSR, each row sorted and unique) of the
 *               rule metrics.py:33-37 applies (graph distance == 1, both directions); an entry equal to its own row is ignored
 *   max_degree  largest rowptr[i + 1] - rowptr[i]: rows above SYMPA_MAP_LDS_CAP entries need
 *               sympa_map_workspace_bytes(num_rows, max_degree) bytes of caller-owned, 16-byte aligned device `workspace`
 *               (returns 0 when none is needed)
 *   ap          [row_count] fp64, written: ap[r] = mean_t(t / r_t) over the neighbours t = 1..deg of row row_begin + r in key
 *               order, r_t their 1-based positions among the columns other than self; NaN for a row without neighbours
 *               (np.mean([]), metrics.py:61)
 *   flags       0 or SYMPA_FLAG_FP32_KEYS: every distance is rounded to fp32 before it is compared (the reference's
 *               float32 torch.zeros matrix, runner.py:144)
 * Order of a row: self first, the other columns k by the key (d[k], k): ascending distance, ties by column index (a stable
 * argsort; the reference's np.argsort is unstable, so its order of exactly tied entries is arbitrary), -0 counts as +0, NaN
 * after every number.  CSR entries outside [0, num_rows), or a row longer than max_degree, set SYMPA_ST_BAD_INDEX in `status`
 * and that row's ap to NaN. */
#define SYMPA_FLAG_FP32_KEYS 256
#define SYMPA_MAP_LDS_CAP 1024
int64_t sympa_map_workspace_bytes(int64_t num_rows, int64_t max_degree);
int sympa_map_rows(const double* dist, int64_t row_count, int64_t ld, int64_t row_begin, int64_t num_rows,
                   const int64_t* rowptr, const int32_t* cols, int64_t max_degree, double* ap, void* workspace,
                   int64_t workspace_bytes, int32_t* status, int flags, void* stream);

/* Hop distances (unweighted shortest paths) from the sources src_begin .. src_begin + src_count - 1 to every node of a graph:
 * what the reference's preprocessing computes for all pairs at once (preprocess.py:101-126), a block of rows at a time
 * (csrc/graph_bfs.hip: level-synchronous bit-parallel BFS, one workgroup per word of 64 sources).
 *   rowptr      [num_nodes + 1] int64, cols [num_entries] int32: the adjacency as a SYMMETRIC CSR (both directions of every
 *               edge present), self-loops and duplicate edges removed
 *   out         [src_count, row_stride] int32, row_stride >= num_nodes: out[s - src_begin][v] = hops from s to v, 0 on the
 *               diagonal, -1 where v cannot be reached.  Every element [r][v < num_nodes] is written; nothing is pre-filled.
 *   workspace   sympa_graph_hops_workspace_bytes(num_nodes, src_count) = ceil(src_count / 64) * 24 * num_nodes bytes of
 *               caller-owned, 8-byte aligned device memory (three uint64 node planes per word of sources)
 * The values do not depend on how the sources are split into calls.  A column outside [0, num_nodes) or a rowptr entry outside
 * [0, num_entries] is skipped and sets SYMPA_ST_BAD_INDEX in `status` (word 1 counts the entries).  Arguments are validated
 * before any launch. */
int64_t sympa_graph_hops_workspace_bytes(int64_t num_nodes, int64_t src_count);
int sympa_graph_hop_rows(const int64_t* rowptr, const int32_t* cols, int64_t num_nodes, int64_t num_entries, int64_t src_begin,
                         int64_t src_count, int32_t* out, int64_t row_stride, void* workspace, int64_t workspace_bytes,
                         int32_t* status, void* stream);

/* Distortion of a block of manifold distance rows against the hop rows of the same nodes (metrics.py:21 over the pairs i < j):
 *   row_sum[r]   = sum over j > i, hops[r][j] > 0 of |dist[r][j] - hops[r][j]| / hops[r][j],   i = row_begin + r
 *   row_pairs[r] = the number of those j
 * dist [row_count, ld_dist] fp64, hops [row_count, ld_hops] int32 (sympa_graph_hop_rows), both leading dimensions >= num_nodes.
 * Each row is summed in an order that depends on the row alone, so a row's value is bitwise the same in every blocking. */
int sympa_graph_distortion_rows(const double* dist, int64_t ld_dist, const int32_t* hops, int64_t ld_hops, int64_t row_begin,
                                int64_t row_count, int64_t num_nodes, double* row_sum, int64_t* row_pairs, void* stream);

/* Weighted shortest-path distances from the sources src_begin .. src_begin + src_count - 1 to every node of a graph with
 * non-negative edge weights: what the reference's preprocessing computes for all pairs of a weighted graph
 * (preprocess.py:108-114), a block of rows at a time (csrc/graph_sssp.hip: pull-based multi-source Bellman-Ford, one workgroup
 * per group of 8 consecutive sources, sweeps separated by workgroup barriers only).
 *   rowptr      [num_nodes + 1] int64, cols [num_entries] int32, weights [num_entries] fp64: the adjacency as a SYMMETRIC CSR
 *               (both directions of every edge present, with the same weight), self-loops and duplicate edges removed.  A
 *               weight of 0 is legal and -0.0 is taken as 0.
 *   out         [src_count, row_stride] fp64, row_stride >= num_nodes: out[s - src_begin][v] = the minimum over the paths from
 *               s to v of the left-to-right fp64 sum of their weights, starting at s: bit for bit what Dijkstra from s
 *               computes.  0 on the diagonal, +inf where v cannot be reached.  Every element [r][v < num_nodes] is written
 *               exactly once; nothing is pre-filled and the padding beyond num_nodes is untouched.  out[i][j] and out[j][i]
 *               may differ in their last bits (each row is summed from its own source); nothing symmetrises them.
 *   workspace   sympa_graph_weighted_workspace_bytes(num_nodes, src_count) = ceil(src_count / 8) * 8 * (num_nodes + 1) * 8
 *               bytes of caller-owned, 8-byte aligned device memory: one fp64 [num_nodes][8] plane per group of sources, then
 *               one int64 per source, which on return holds the number of sweeps the group of that source ran (timing
 *               tools read it).  0 for num_nodes <= 0 or src_count <= 0.
 * The values do not depend on how the sources are split into calls: the result is the unique least fixed point of the
 * relaxation.
 * A column outside [0, num_nodes) or a rowptr entry outside [0, num_entries] is skipped and sets SYMPA_ST_BAD_INDEX in
 * `status`; a weight that is NaN, negative or infinite is skipped and sets SYMPA_ST_NONFINITE; word 1 counts the entries of
 * both kinds.  Arguments are validated before any launch; src_count == 0 is a no-op. */
int64_t sympa_graph_weighted_workspace_bytes(int64_t num_nodes, int64_t src_count);
int sympa_graph_weighted_rows(const int64_t* rowptr, const int32_t* cols, const double* weights, int64_t num_nodes,
                              int64_t num_entries, int64_t src_begin, int64_t src_count, double* out, int64_t row_stride,
                              void* workspace, int64_t workspace_bytes, int32_t* status, void* stream);

/* Distortion of a block of manifold distance rows against the weighted graph distance rows of the same nodes (metrics.py:21
 * over the pairs i < j): the fp64 twin of sympa_graph_distortion_rows.
 *   row_sum[r]   = sum over j > i, 0 < gdist[r][j] < inf of |dist[r][j] - gdist[r][j]| / gdist[r][j],   i = row_begin + r
 *   row_pairs[r] = the number of those j
 * dist [row_count, ld_dist] and gdist [row_count, ld_g] (sympa_graph_weighted_rows) fp64, both leading dimensions >= num_nodes.
 * Each row is summed in an order that depends on the row alone, so a row's value is bitwise the same in every blocking. */
int sympa_graph_weighted_distortion_rows(const double* dist, int64_t ld_dist, const double* gdist, int64_t ld_g,
                                         int64_t row_begin, int64_t row_count, int64_t num_nodes, double* row_sum,
                                         int64_t* row_pairs, void* stream);

/* Census, ball sizes and ball selection over a block of graph distance rows that is already on the device (csrc/graph_census.hip):
 * what the reference's --subsample and --scale_triplets (train.py:86-93, utils.py:71-102) need from a graph whose triplets cannot
 * be listed.  Row r of a block stands for node i = row_begin + r and only its columns j > i count: the pairs a triplet list
 * holds.  Integer sums only: no result depends on the grid or on how the rows are split into calls.  Arguments are validated
 * before any launch; row_count == 0 (or m == 0) is a no-op that returns 0.
 *
 * sympa_graph_hop_census_rows: the histogram behind d_max (utils.py:71-82) and behind the distance below which a fraction of the
 * triplets lies (utils.py:85-102).  hops [row_count, ld] int32 (sympa_graph_hop_rows), ld >= num_nodes.
 *   bins[d] += the number of (r, j) with j > row_begin + r and hops[r][j] == d, for 0 < d < num_bins; values >= num_bins are added
 *   to bins[0], an overflow counter (distance 0 and unreachable entries are never counted).  bins [num_bins] int64 ACCUMULATES:
 *   the caller zeroes it.  Each workgroup keeps the first SYMPA_GRAPH_CENSUS_LDS_BINS bins in LDS and flushes them with 64-bit
 *   global atomics; larger distances go to the global bins directly. */
#define SYMPA_GRAPH_CENSUS_LDS_BINS 512
int sympa_graph_hop_census_rows(const int32_t* hops, int64_t ld, int64_t row_begin, int64_t row_count, int64_t num_nodes,
                                int64_t* bins, int64_t num_bins, void* stream);

/* The ball of radius `radius` (utils.py:85-102: "the local neighbourhood of each node"), row by row:
 *   upper_count[r] = #{j > row_begin + r : 0 < rows[r][j] <= radius}      (int64 [row_count], written, not accumulated)
 * rows [row_count, ld]: int32 hop rows (rows_fp64 == 0) or fp64 weighted rows (rows_fp64 == 1; +inf marks an unreachable node).
 * A NaN, negative or infinite radius is SYMPA_ERR_BAD_ARG. */
int sympa_graph_ball_count_rows(const void* rows, int rows_fp64, int64_t ld, int64_t row_begin, int64_t row_count,
                                int64_t num_nodes, double radius, int64_t* upper_count, void* stream);

/* Elements of that ball by (row, rank) (the draw of utils.py:85-102's subsample without its list).  Request k: i = req_row[k], a
 * global row id inside [row_begin, row_begin + row_count), in any order, repeats allowed;
 *   out_col[k]  = the column j > i of the ball that has exactly req_rank[k] ball columns strictly between i and j
 *   out_dist[k] = rows[i - row_begin][j] as fp64 (out_dist may be NULL)
 * A row outside the block or a rank >= upper_count of its row writes -1 (NaN for the distance) and sets SYMPA_ST_BAD_INDEX in
 * `status` (word 1 counts the requests; `status` may be NULL).  A wave answers a run of consecutive requests and keeps its place
 * in a row between them, so requests sorted by (row, rank) cost one scan of a row per wave; any order is answered. */
int sympa_graph_ball_select_rows(const void* rows, int rows_fp64, int64_t ld, int64_t row_begin, int64_t row_count,
                                 int64_t num_nodes, double radius, const int64_t* req_row, const int64_t* req_rank, int64_t m,
                                 int64_t* out_col, double* out_dist, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYMPA_HIP_H */
