/*
 * include/celerite_hip.h -- C ABI of libcelerite_hip.so, the MI355X (gfx950)
 * implementation of celerite's semiseparable-Cholesky hot path.
 *
 * This is the drop-in boundary: every entry point below replaces one member of
 * the reference's C++ solver class as it is bound by the reference's pybind11
 * translation unit (celerite/solver.cpp).  The reference-side binding a
 * maintainer would add is shown in INTEGRATION.md.  Conventions:
 *
 *   - extern "C", plain pointers + sizes, no C++ types, no exceptions: every
 *     call returns a clr_status (the pybind11 layer maps CLR_NOT_POSITIVE_DEFINITE
 *     -> celerite.solver.LinAlgError and the other non-zero codes ->
 *     RuntimeError with the reference's what() strings, exceptions.h:14-36).
 *   - all pointers are caller-owned HOST memory unless a name says `_dev`;
 *     inputs are const and are not retained past the call (the reference's
 *     pybind11/Eigen casters copy every argument, solver.cpp:467-483).
 *   - a handle is thread-compatible (one thread at a time), like the reference
 *     object; distinct handles may be used concurrently.
 *   - there is NO CPU fallback: without a usable gfx950 device every compute
 *     entry returns CLR_NO_DEVICE.
 *   - fp64 throughout.  Matrices of the factor use the reference's storage
 *     (Eigen column-major J x N: element (j, n) at [j + J*n], cholesky.h:703-706).
 *     U and V (general terms) are ROW-major [J_general][N], as the NumPy arrays
 *     arrive at the Python boundary.
 */
#ifndef CELERITE_HIP_H
#define CELERITE_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum clr_status {
  CLR_OK = 0,
  CLR_DIMENSION_MISMATCH = 1,    /* celerite::dimension_mismatch  exceptions.h:20-24 */
  CLR_NOT_POSITIVE_DEFINITE = 2, /* celerite::linalg_exception    exceptions.h:32-36 */
  CLR_NOT_COMPUTED = 3,          /* celerite::compute_exception   exceptions.h:14-18 */
  CLR_NO_DEVICE = 4,             /* no gfx950 GPU visible / HIP runtime unusable    */
  CLR_HIP_ERROR = 5,             /* a HIP call failed; see clr_last_error()          */
  CLR_INVALID_ARGUMENT = 6,
  CLR_UNSUPPORTED = 7,           /* e.g. width above CLR_MAX_WIDTH                   */
  CLR_CARMA_INSTABILITY = 8      /* celerite::carma_exception     exceptions.h:8-12  */
} clr_status;

/* Widest semiseparable rank J = J_real + 2 J_comp + J_general of the batched plans (fused log-likelihood; the scans stop
 * at 64) and of the one-workgroup kernels of the object API. */
#define CLR_MAX_WIDTH 128
/* The object API -- CholeskySolver.compute / log_determinant / dot_solve / solve / dot_L / dot / predict and the pickled
 * state -- takes ANY width up to this one (round 6; the reference's dynamic-width arm, cholesky.h:203, has no limit and
 * its benchmark goes to 512): compute above 64 keeps S in the registers of 1 .. 64 workgroups (csrc/rows_kernels.hip),
 * dot_L / dot are diagonal scans with one thread per row, solve / dot_solve above 64 chunked affine scans with
 * J x J chunk maps built once per factor (csrc/bigsweep_kernels.hip; short series: one workgroup per right-hand side);
 * grad_log_likelihood above width 64: one workgroup per partial, S and its tangent in an HBM / L2 workspace
 * (csrc/grad_any_kernels.hip; sequential in n). */
#define CLR_MAX_WIDTH_ANY 1024
#define CLR_CARMA_MAX_ORDER 32 /* autoregressive order p of clr_carma (state p, covariance p x p in LDS) */

/* ---- library / device ------------------------------------------------------ */

/* CELERITE_VERSION_STRING, cpp/include/celerite/version.h:4-13 ("0.3.0");
 * bound as solver.get_library_version (solver.cpp:76). */
const char* clr_version(void);
/* Message of the last non-OK status on the calling thread. */
const char* clr_last_error(void);
/* what() string of the reference exception a status stands for. */
const char* clr_status_string(int status);
/* Number of visible gfx950 devices (0 without a GPU; never fails). */
int clr_device_count(void);
/* Device used by handles created afterwards on this thread (default 0). */
int clr_set_device(int device);
int clr_get_device(int* device);
/* hipDeviceSynchronize on the current device. */
int clr_device_synchronize(void);
/* Name + CU count of the current device (for logs). */
int clr_device_info(char* name, size_t name_len, int* compute_units, size_t* hbm_bytes);
/* Free / total HBM of the current device right now (hipMemGetInfo): for sizing a batch to the 288 GB of a
 * GPU -- a plan of B problems x N samples x width J holds about 8 B N (3 + [3 J + 1 when materialising]) bytes
 * of series and factor plus 8 B nchunk (J^2 + J (J + 1) + 4 J) of scan workspace. */
int clr_device_memory(size_t* free_bytes, size_t* total_bytes);

/* Tuning and cross-check switches of the library, ONE table per process (round 5 read 19 environment variables
 * directly: a stray variable silently changed kernel selection).  `value` NULL removes the option.  Environment variables
 * of the same names are honoured only when the process was started with CLR_ALLOW_ENV=1.  The keys (all "CLR_..."):
 *   CLR_GRAD_SEQUENTIAL      the sequential tangent kernel for every gradient (cross-checks); with CLR_GRAD_ANY_WIDTH the
 *                            workgroup-per-partial kernel of the widths above 64 at every width
 *   CLR_GRAD_REBUILD_SPAN    reverse-mode gradient: distance of the stored states
 *   CLR_WIDE_WALK            widths 17..32: prefix + corrections as one walk per problem (cross-check of the two-kernel path)
 *   CLR_WIDE_NO_PAIRED       widths 17..64, complex terms only: the kernels without the term-paired features (cross-check)
 *   CLR_OUTPUT_CHECK_CAP, CLR_OUTPUT_CHECK_TOL   materialising replays at widths 9..64 whose end states miss the scanned start
 *                            states by more than the certificate's bound but less than CAP (default 1e-6; 0: off) are
 *                            settled by comparing what a second replay writes (within TOL, default 2e-11) instead of
 *                            going to the sequential recurrence
 *   CLR_NO_ROWS_KERNEL       CholeskySolver above width 64 / general terms above 32: the one-workgroup kernels (S in LDS / L2)
 *                            instead of the row-distributed one (cross-checks)
 *   CLR_NO_BIG_SWEEP         dot_solve / solve above width 64: the sequential sweeps instead of the chunked affine scans
 *   CLR_SPLIT_GENERIC        lazy role-split summarize (widths 7, 8): "1" the general kernel for every batch, also where
 *                            every b_comp is zero (cross-checks, A/B runs; clr_batch_get_split_variant)
 * Any other key is refused with CLR_INVALID_ARGUMENT.
 * clr_get_option: the value in force (NULL: not set); the pointer is valid until the calling thread's next call. */
int clr_set_option(const char* key, const char* value);
const char* clr_get_option(const char* key);

/* ---- single-problem solver: celerite::solver::CholeskySolver<double> ----------
 * (cpp/include/celerite/solver/cholesky.h, solver.h), the object behind
 * celerite.solver.CholeskySolver (solver.cpp:241-244).  The factor
 * (phi, u, W, D) stays resident in HBM between calls. */

typedef struct clr_solver clr_solver;

clr_solver* clr_solver_create(void);       /* CholeskySolver()   solver.cpp:244 */
void clr_solver_destroy(clr_solver* s);

/* CholeskySolver::compute, cholesky.h:41-210 (bound at solver.cpp:467-483).
 * Each array carries its own length so the reference's dimension checks
 * (cholesky.h:59-69) are made here.  n_A == 0 means "no general terms".
 * On CLR_NOT_POSITIVE_DEFINITE (some D_n < 0, n >= 1: cholesky.h:176) or
 * CLR_DIMENSION_MISMATCH the handle is left "not computed" (cholesky.h:57). */
int clr_solver_compute(clr_solver* s, double jitter,
                       int n_a_real, const double* a_real,
                       int n_c_real, const double* c_real,
                       int n_a_comp, const double* a_comp,
                       int n_b_comp, const double* b_comp,
                       int n_c_comp, const double* c_comp,
                       int n_d_comp, const double* d_comp,
                       int n_A, const double* A,
                       int U_rows, int U_cols, const double* U,
                       int V_rows, int V_cols, const double* V,
                       int n_x, const double* x,
                       int n_diag, const double* diag);

/* Optional, not in the reference: announce the vector the caller is about to hand to dot_solve (GP.log_likelihood
 * knows y before it factorises, celerite.py:180-215).  The NEXT clr_solver_compute then folds b^T K^-1 b into its own
 * pass over the series (widths 1..64 without general terms) and clr_solver_dot_solve returns that value when it is
 * called with the very same vector (compared byte for byte); any other vector takes the ordinary sweep.  One shot:
 * the hint is consumed by the next clr_solver_compute whatever its outcome (a hint of another length is dropped
 * there); n_b = 0 withdraws a hint that will not be followed by a compute. */
int clr_solver_hint_rhs(clr_solver* s, int n_b, const double* b);

/* Solver::computed / log_determinant, solver.h:74-81 (solver.cpp:620-634). */
int clr_solver_computed(const clr_solver* s);
int clr_solver_log_determinant(const clr_solver* s, double* out);

/* CholeskySolver::dot_solve, cholesky.h:326-401 (solver.cpp:527-529):
 * out = b^T K^-1 b. */
int clr_solver_dot_solve(const clr_solver* s, int n_b, const double* b, double* out);

/* CholeskySolver::solve, cholesky.h:218-318 (solver.cpp:507-509).
 * b, x: COLUMN-major (N, nrhs): right-hand side k is b + k*N. */
int clr_solver_solve(const clr_solver* s, int b_rows, int nrhs, const double* b, double* x);

/* CholeskySolver::dot_L, cholesky.h:409-431 (solver.cpp:547-549): y = L z with
 * K = L L^T.  Column-major (N, nrhs). */
int clr_solver_dot_L(const clr_solver* s, int z_rows, int nrhs, const double* z, double* y);

/* CholeskySolver::dot, cholesky.h:444-590 (solver.cpp:567-581): y = K z without
 * factorising (stateless; the handle only supplies the device).  z, y:
 * column-major (N, nrhs). */
int clr_solver_dot(clr_solver* s, double jitter,
                   int n_a_real, const double* a_real,
                   int n_c_real, const double* c_real,
                   int n_a_comp, const double* a_comp,
                   int n_b_comp, const double* b_comp,
                   int n_c_comp, const double* c_comp,
                   int n_d_comp, const double* d_comp,
                   int n_A, const double* A,
                   int U_rows, int U_cols, const double* U,
                   int V_rows, int V_cols, const double* V,
                   int n_x, const double* x,
                   int z_rows, int nrhs, const double* z, double* y);

/* CholeskySolver::predict, cholesky.h:599-698 (solver.cpp:611-615): conditional
 * mean at the M sorted-or-not coordinates xs given observations y. */
int clr_solver_predict(const clr_solver* s, int n_y, const double* y,
                       int M, const double* xs, double* pred);

/* grad_log_likelihood, celerite/solver.cpp:347-463 (the reference runs compute +
 * dot_solve on forward-mode dual numbers; the handle's factorisation is neither used
 * nor changed, as in the reference where the bound object is ignored).  Same argument
 * conventions as clr_solver_compute plus the observations y.
 *   *value = -(y^T K^-1 y + log det K + pi log N) / 2   (the reference's constant,
 *            solver.cpp:415 -- not N log 2 pi);
 *   grad[0] = d/d jitter (0 when jitter <= DBL_EPSILON, solver.cpp:379-389,419-426),
 *   then d/d a_real, c_real, a_comp, b_comp, c_comp, d_comp: n_grad must be
 *   1 + 2 n_a_real + 4 n_a_comp.
 * Returns CLR_NOT_POSITIVE_DEFINITE where the reference throws linalg_exception.
 * Any total width up to CLR_MAX_WIDTH_ANY: widths 1..8 from N = 1024 and widths 9..64 from N = 4096 run parallel in n on a
 * one-problem plan (general terms: up to a total width of 32); otherwise one wave per partial, sequential in n, up to
 * width 64 (csrc/grad_kernels.hip) and one workgroup per partial above (round 6: csrc/grad_any_kernels.hip). */
int clr_solver_grad_log_likelihood(clr_solver* s, double jitter,
                                   int n_a_real, const double* a_real,
                                   int n_c_real, const double* c_real,
                                   int n_a_comp, const double* a_comp,
                                   int n_b_comp, const double* b_comp,
                                   int n_c_comp, const double* c_comp,
                                   int n_d_comp, const double* d_comp,
                                   int n_A, const double* A,
                                   int U_rows, int U_cols, const double* U,
                                   int V_rows, int V_cols, const double* V,
                                   int n_x, const double* x,
                                   int n_y, const double* y,
                                   int n_diag, const double* diag,
                                   double* value, int n_grad, double* grad);

/* PicklableCholeskySolver::serialize / deserialize, solver.cpp:36-58 (bound as
 * __getstate__/__setstate__, solver.cpp:644-663).  get_dims first, then
 * get_state into caller buffers of J*(N-1), J*(N-1), J*N and N doubles
 * (reference storage order). */
int clr_solver_get_dims(const clr_solver* s, int* computed, int* N, int* J, double* log_det);
int clr_solver_get_state(const clr_solver* s, double* phi, double* u, double* W, double* D);
int clr_solver_set_state(clr_solver* s, int computed, int N, int J, double log_det,
                         const double* phi, const double* u, const double* W, const double* D);

/* ---- batched log-likelihood (new; the data-parallel axis) ---------------------
 * B independent problems = (time series x hyper-parameter draw) pairs that
 * share N, J_real and J_comp.  One call evaluates, for every problem p,
 *     loglike[p] = -0.5 (y^T K_p^-1 y + log det K_p + N log 2 pi)
 * i.e. exactly GP.compute + GP.log_likelihood (celerite/celerite.py:103-219)
 * with the -inf rules of celerite.py:205-218 applied (quiet=True semantics:
 * status[p] = CLR_NOT_POSITIVE_DEFINITE and loglike[p] = -inf instead of an
 * exception; a bad problem never disturbs its neighbours).
 *
 * Coefficients are [B][J_real] / [B][J_comp] row-major, jitter is [B].
 * A series array is [B][N] with *_stride = N, or one shared [N] series with
 * *_stride = 0 (the "one light curve, B posterior draws" case). */

typedef struct clr_batch clr_batch;

/* Plans device buffers + workspace for (B, N, J_real, J_comp) on `device`.
 * General terms: clr_batch_set_general.  Width W = J_real + 2 J_comp:
 *   1..8   chunked scan over n, one lane per (problem, chunk)  (the headline path);
 *   9..64  one wave per (problem, chunk), S distributed over the lanes (BASELINE
 *          config 5: 16 complex terms); fused log-likelihood only.  One chunk = the
 *          reference recurrence itself; the series is cut into chunks (two-pass
 *          scan) when B alone leaves SIMDs idle (clr_batch_set_chunks(h, 0) picks
 *          2048 / B, at most 16, at widths <= 32; 1024 / B, at most 16, at widths 33..64 -- one
 *          wave per SIMD there, the chunks chained by one walk per problem: csrc/wide64_kernels.hip).
 *          Materialising runs write the reference's storage directly
 *          (every chunk replayed from its scanned start state and checked, as CholeskySolver.compute
 *          does); layouts do not apply;
 *   65..128 (round 5) the any-width sequential recurrence, one workgroup per problem with S in LDS (the kernel of
 *          plans with general terms): fused log-likelihood only, sequential in n;
 *   else   CLR_UNSUPPORTED (the reference's dynamic-width arm, cholesky.h:203, takes any J). */
clr_batch* clr_batch_create(int B, int N, int J_real, int J_comp, int device);
void clr_batch_destroy(clr_batch* h);

/* Host -> HBM. */
int clr_batch_set_series(clr_batch* h,
                         const double* t, long t_stride,
                         const double* diag, long diag_stride,
                         const double* y, long y_stride);
/* Per-problem series lengths (ragged batches): problem b is the first lengths[b] samples of its rows, 1 <= lengths[b]
 * <= N (host, [B]).  NULL is exactly clr_batch_set_series, lengths that all equal N are the uniform plan, and a later
 * clr_batch_set_series returns the plan to uniform.  With lengths in force t, diag and y are each [B][N] (stride N): a
 * shared array (stride 0) is CLR_INVALID_ARGUMENT -- the padded device copy is per problem -- and so is a length outside
 * [1, N]; both leave the plan as it was.
 *   The tail is never read: entries n >= lengths[b] of a row may be NaN, unsorted, anything.  After the upload a small
 *   kernel rewrites them IN the resident arrays to the padding a recurrence step ignores -- t held at t[lengths[b] - 1],
 *   diagonal 1e300, y = 0 -- before any scan looks at them, so clr_batch_get_series_order, the selection bounds and
 *   every copy of the series see the first lengths[b] entries alone.  A padded step changes no state above rounding; the
 *   kernels leave it out of the log-determinant, the quadratic form, the flags and the riders by a select on n < n_b,
 *   with n_b loaded once per lane (BatchParams::len).  A mean (clr_batch_set_mean, _set_mean_basis) leaves the residual's
 *   tail at 0, not -mu.
 *   What carries n_b: the fused evaluation of narrow plans (widths 1..8, no general terms) on every layout, prefix
 *   mode and route -- the replay-free route, the checked replay, the sequential recurrence, the re-planned
 *   side plan (clr_batch_set_rescue), clr_batch_set_exact -- and the gradient (reverse, forward, the sequential
 *   fallback, the mean's partial); loglike, logdet, quad, gradient, status and the gradient value's pi log n_b are those
 *   of the problem's own samples.
 *   What stays off: the warm-started recurrence and the one-launch small mode do not run while lengths are in force
 *   (clr_batch_get_warm_start and clr_batch_get_small_mode report inactive; forcing either is CLR_UNSUPPORTED, as is
 *   setting lengths while one is forced).  Nor do the role-split summarize kernels of widths 7 and 8: such a plan runs
 *   the single-wave summarize under the modes -1 and 0 (clr_batch_get_summarize_kernel reports 0), and
 *   clr_batch_set_summarize_mode(h, 1 or 2) -- or lengths on a plan where one of them is set -- is CLR_UNSUPPORTED.  The
 *   role-split kernels are exactly what uniform plans ran before; a ragged batch of width 7 or 8 costs about 1.5 x the
 *   uniform plan of its shape (profiles/ragged_timing.txt).  clr_batch_clear_series drops the lengths with the series.
 *   What refuses (CLR_UNSUPPORTED, "the plan has per-problem lengths"; the plan still evaluates afterwards): wide plans
 *   (widths above 8) and plans with general terms, every materialising run, and every consumer of the materialised
 *   factor or of the padded rows: clr_batch_get_factor, _solve, _dot_L, _dot, _predict*, _one_step_ahead, _forecast,
 *   _predict_terms, _predict_cov, _sample_conditional, _leave_one_out, _grad_mean_weights, _fit_mean_weights,
 *   _grad_noise_weights, _grad_amplitudes.
 * clr_batch_get_lengths: the lengths in force (N for every problem of a uniform plan). */
int clr_batch_set_series_ragged(clr_batch* h,
                                const double* t, long t_stride,
                                const double* diag, long diag_stride,
                                const double* y, long y_stride, const int* lengths);
int clr_batch_get_lengths(const clr_batch* h, int* lengths);
/* Short narrow problems (widths 1..4, 512 <= N <= 32768; BASELINE configs[1]: 256 x 1e4 x width 4): the whole fused
 * evaluation in ONE launch, one workgroup per problem -- chunk elements composed by a Kogge-Stone scan in LDS, the
 * reference recurrence per chunk from the scanned states, every chunk boundary checked; a problem that fails the check
 * (or has a flagged pivot) goes through the scan pipeline before results are handed out.  mode: -1 automatic (up to
 * 1024 problems), 0 off, 1 whenever supported.  clr_batch_get_small_mode: whether the next evaluation takes it. */
int clr_batch_set_small_mode(clr_batch* h, int mode);
int clr_batch_get_small_mode(const clr_batch* h, int* active);
/* The smallest step t[n + 1] - t[n] over the plan's series, found by the device-side scan of clr_batch_set_series
 * (negative: some series is not sorted -- GP.compute's check, celerite.py:126-129, without a host pass over t -- and
 * that holds whatever else the batch contains: the minimum is taken over the finite steps, as np.diff(t) < 0 would;
 * NaN: no negative step, but a NaN time somewhere).  clr_batch_clear_series drops the series (a front end that
 * rejects unsorted input calls it).
 * clr_batch_set_series replaces the plan's series IN PLACE: from the moment it starts copying, the previous series is
 * gone -- a call that fails midway, or whose input the front end then rejects, leaves the plan WITHOUT a series
 * (set one again before the next evaluation), never with a half-overwritten one. */
int clr_batch_get_series_order(const clr_batch* h, double* dtmin);
int clr_batch_clear_series(clr_batch* h);
/* (jitter may be NULL: no jitter) */
int clr_batch_set_coefficients(clr_batch* h, const double* jitter,
                               const double* a_real, const double* c_real,
                               const double* a_comp, const double* b_comp,
                               const double* c_comp, const double* d_comp);

/* General semiseparable terms for the whole batch (cholesky.h:65-72,148-152: A added to the diagonal, rows U, V
 * appended to U~, V~ with phi = 1): A [N], U and V row-major [J_general][N] per problem, *_stride doubles between
 * problems (N resp. J_general * N) or 0 for one block shared by all problems; J_general = 0 removes them.  A plan
 * with general terms evaluates, up to a total width J_real + 2 J_comp + J_general of 64, on the wave-per-(problem,
 * chunk) kernels of the widths 9..64 with the general rows as a third row class (per-sample features fetched a few
 * steps ahead; chunked scan up to total width 64, as clr_batch_set_chunks(h, 0) would pick for a wide plan), above
 * that -- or after clr_batch_set_general_route(h, 1) -- through the any-width sequential kernel (one workgroup per
 * problem, the reference's step order) up to CLR_MAX_WIDTH; fused log-likelihood only (materialising runs:
 * CholeskySolver). */
int clr_batch_set_general(clr_batch* h, int J_general, const double* A, long A_stride, const double* U, long U_stride,
                          const double* V, long V_stride);
int clr_batch_set_general_route(clr_batch* h, int route);

/* Tuning: how the kernels read the series.
 *   2 (default) staged: each wave loads the row-major arrays in coalesced tiles of
 *       8 steps x 64 chunks and transposes them through LDS; no extra pass or copy.
 *   1 interleaved: enqueue first builds a chunk-interleaved copy ([problem][i][chunk])
 *       with a tiled-transpose kernel whenever the series or the chunking changed;
 *       marginally faster per evaluation when the SAME series are evaluated many
 *       times, but costs a 0.87 ms pass (B=1024, N=1e5) whenever they change.
 *   0 row-major direct: every lane streams its own run (slow; kept for A/B). */
int clr_batch_set_layout(clr_batch* h, int layout);
/* (The kernels evaluate sin/cos(d_comp * t) with a 25-instruction FMA Cody-Waite
 * routine (abs. error < 1 ulp(1)) when the host-side check max|d_comp| * max|t| <
 * 1e9 holds, and with the library (ocml) sincos otherwise.) */
/* summarize kernel of widths 7 and 8 (csrc/clr_split_kernels.h):
 *   0  the single-wave kernel (one wave per SIMD, part of the state in AGPRs);
 *   1  two roles on two waves per SIMD: a "trajectory" wave (C, b) and a "riders" wave (A, eta in
 *      registers, Jm in LDS) linked through LDS; reads a chunk-interleaved copy of the series made
 *      once per clr_batch_set_series (layout 1 below is implied);
 *   2  the same with the decay factored out of the state ("lazy": one FMA per state entry and step
 *      instead of FMA + MUL, renormalised every 64 steps) when the series is densely sampled
 *      (max c * max dx < 2^-7 and max d * max dx < 2^-5: the phases then advance by small-angle
 *      rotations, re-anchored with the full sincos every 64 steps), else as 1;
 *  -1  (default) 2 at widths 7 and 8 on a dense series; otherwise 1 at width 7 and at width 8 with at least two
 *      complex terms, else 0.
 * Wide plans (widths 9..64: csrc/wide_kernels.hip) know two flavours: 0 plain, 2 (and -1 where eligible) lazy.  At widths
 * 17..64 the lazy flavour is eligible whenever max c * max dx < 2 -- a lane whose interval is too long for the small-step
 * series sends its wave through the full sincos / exp for that batch -- at widths 9..16 under the dense-series rule above. */
int clr_batch_set_summarize_mode(clr_batch* h, int mode);
/* Series that FORGET their past (the decay between samples is not small: e.g. the paper's accuracy family,
 * paper/figures/error/error.py:24-25, or most real light curves) do not need the scan: every chunk runs the
 * reference recurrence itself from the zero state `K` samples before its first sample, and the state it has reached
 * at its first sample is checked against the state the previous chunk reaches there (relative mismatch <= the
 * max_residual of clr_batch_set_certificate); the first chunk starts from the true zero state, so agreement at every
 * boundary certifies all of them.  A problem with a mismatch, a flagged pivot or no usable K goes through the scan
 * pipeline when the results are fetched.  mode -1 (default): per problem, the smallest K of 8, 12, 16, ... 128 with
 * exp(-c_min x (time the K samples before any chunk boundary span)) <= exp(-32), used when at least half of the batch
 * has one; 0: off; 1: every problem with `forced_warmup` steps (tests: the check then decides).  Widths 1..8, fused
 * log-likelihood only (materialising / forced-exact runs take the scan). */
int clr_batch_set_warm_start(clr_batch* h, int mode, int forced_warmup);
/* What the current (series, coefficients) pair runs and how the last evaluation went: active, the warm path's chunk
 * count and length, smallest / largest warm-up in the batch, problems it settled / left to the scan (after the last
 * clr_batch_get_results).  Any pointer may be NULL. */
int clr_batch_get_warm_start(const clr_batch* h, int* active, int* nchunk, int* chunk_len, int* warmup_min,
                             int* warmup_max, int* settled, int* fallbacks);
/* Which one the next evaluation will run (0, 1 or 2 as above), given the series and coefficients set. */
int clr_batch_get_summarize_kernel(const clr_batch* h, int* kind);
/* The variant of the lazy role-split summarize (kind 2, widths 7 and 8) the next evaluation runs: 1 the one without the
 * b_comp terms of the features (every b_comp of the current coefficients is exactly zero), 0 the general one -- and 0 for
 * any other kernel and under CLR_SPLIT_GENERIC=1.  Results do not depend on it (the sign of an exact zero apart). */
int clr_batch_get_split_variant(const clr_batch* h, int* variant);
/* Prefix phase of the scan (widths 1..8): how the chunk elements are turned into chunk start states.
 *   2 (default) multi-level: groups of consecutive elements are composed in parallel (element o element, the
 *       associative operator of the scan; csrc/clr_prefix_kernels.h), the few composed elements are walked, and the
 *       start states fan out group by group -- the dependent chain is ~2.2 (g - 1) per level + the top level instead
 *       of nchunk (the reference's loop being parallelised: cholesky.h:126-179);
 *   1 16 lanes per problem walking the chunks one after the other;
 *   0 the single-lane version (the host-checked form; on-device cross-check and A/B).
 * Widths 9..32 (and plans with general terms): 2 = a Kogge-Stone scan over composed elements when the plan has few
 * problems with many chunks (B x nchunk <= 1024 at widths <= 16, 512 above, nchunk >= 8; csrc/wide_prefix_scan.hip) --
 * such plans then choose N / 256 chunks by themselves --, else and for 1: a workgroup per problem walking the chunks. */
int clr_batch_set_prefix_mode(clr_batch* h, int mode);
/* Level structure of mode 2: `levels` (0..3) levels of groups of `group` (>= 2) elements; levels < 0 (default):
 * chosen from the chunk count by a cost model (clr_core.h: plan_prefix).  Re-plans the workspace. */
int clr_batch_set_prefix_plan(clr_batch* h, int levels, int group);
/* The plan in force: number of composition levels (0 = plain walk), group size per level [3], element count per
 * level [4] (counts[0] = chunks). */
int clr_batch_get_prefix_plan(const clr_batch* h, int* levels, int* groups, int* counts);


/* The maxima the kernel selection looks at -- max |t|, largest time step, largest |d_comp|, largest decay rate of the
 * plan's own series / coefficients -- and the host time of the last clr_batch_set_series (scan + uploads, ms).  Any
 * pointer may be NULL. */
int clr_batch_get_selection_bounds(const clr_batch* h, double* tmax, double* dxmax, double* dmax, double* cmax,
                                   double* set_series_host_ms);
/* Floors for those maxima (negative: keep): a sharded plan passes the maxima of the WHOLE batch so that every shard
 * selects the same kernels as the unsharded plan would. */
int clr_batch_set_selection_bounds(clr_batch* h, double tmax, double dxmax, double dmax, double cmax);
/* The fused log-likelihood normally needs no second pass over the series: each
 * chunk's true log-det / quadratic contributions follow from its zero-start sums and
 * its start state (determinant lemma + Woodbury), and only
 * problems with a chunk the positive-definiteness certificate or the error estimate
 * cannot settle are re-run through the exact replay.  force != 0 replays every
 * problem (the reference's recurrence step by step; for A/B measurements and as the
 * on-device cross-check).  Materialising runs always replay. */
int clr_batch_set_exact(clr_batch* h, int force);
/* After a synchronised run: how many problems went through the exact replay. */
int clr_batch_get_exact_count(clr_batch* h, int* count);
/* ... and how: level[p] = 0 settled from the chunk summaries (no second pass); 1 = the
 * conditioning record was above the bound, the chunked replay ran and every chunk's end state
 * met the scanned start state of the next chunk; 2 = settled by the truly sequential recurrence
 * (certificate failed, or the replay's end states did not meet the scanned ones).  On forced
 * exact / single-chunk runs every problem is at least 1. */
int clr_batch_get_exact_flags(clr_batch* h, int* level /* [B] */);
/* Conditioning record of the last run (widths 1..8), per problem: gamma_max = the largest
 * a_n / D_n over the zero-start pivots of its chunks (the cancellation in D_n = a_n - u.Su,
 * cholesky.h:162-175), mu_min = the smallest pivot of the chunk certificates (1 = the start
 * state does not eat into the chunk's pivots), resid_max = (after a replay) the largest
 * relative mismatch between a replayed chunk's end state and the scanned start state of the
 * next chunk.  Any pointer may be NULL. */
int clr_batch_get_conditioning(clr_batch* h, double* gamma_max, double* mu_min, double* resid_max);
/* ... the largest measured relative error eG of the chunks' G = (I + P Jm)^-1 P, per problem ... */
int clr_batch_get_measured_error(clr_batch* h, double* eg_max);
/* ... and max over chunks of gamma_c / mu_c taken chunk by chunk (diagnostic). */
int clr_batch_get_conditioning_chunkwise(clr_batch* h, double* ratio_max);
/* Routing of ill-conditioned problems.  A problem whose gamma_max / mu_min reaches
 * max_gamma_over_mu (default 1e7; <= 0: never), or whose gamma_max alone reaches the bound of
 * clr_batch_set_certificate_gamma (default 1e4), is not settled from the chunk summaries: the
 * chunked replay (the reference recurrence from the scanned start states, parallel over chunks)
 * runs for it and its end states are compared with the scanned start states; a mismatch above
 * max_residual (default 1e-11, relative) sends it to the truly sequential recurrence (one lane
 * walks the whole series; slow, exact).  Calibration: profiles/r02n_adv_probe.txt, r03_conditioning_calibration.txt. */
int clr_batch_set_certificate(clr_batch* h, double max_gamma_over_mu, double max_residual);
/* The bound on gamma_max alone (default 1e4; <= 0: no such test) -- gamma = a_n / D_n is the cancellation in the
 * recurrence itself: it is what the deviation from the reference follows (profiles/r03_conditioning_calibration.txt)
 * -- and on gamma_max x eG_max (default 3e-9; <= 0: no test), eG = the MEASURED relative accuracy of a chunk's
 * G = (I + P Jm)^-1 P (first-order forward error from the residual, computed by the correct kernels). */
int clr_batch_set_certificate_gamma(clr_batch* h, double max_gamma, double max_gamma_times_error);
/* Number of chunks the N axis is cut into for the scan (0 = auto). */
int clr_batch_set_chunks(clr_batch* h, int nchunk);
int clr_batch_get_chunks(const clr_batch* h, int* nchunk, int* chunk_len);

/* Problems whose conditioning record sends them to the checked chunked replay (route 1, see
 * clr_batch_get_exact_flags) used to be replayed inline: every chunk of such a problem sequentially, beside an otherwise
 * idle chip -- ONE borderline problem cost the whole batch a chunk-time (BASELINE configs[4]: +11 ms on 12.7).  Now the
 * evaluation leaves them pending and, before results are handed out, re-plans them as a small plan of their own with
 * many short chunks (n problems -> ~1024 / n chunks each at width 32): summarize, parallel prefix, replay of every chunk
 * from its scanned start state with the end-state check -- the same route with the same certificates (a mismatch goes to
 * the sequential recurrence, cholesky.h:176 semantics unchanged), a tenth of the chunk length.
 *   mode -1 (default): plans whose chunks hold >= 1024 samples; 0: never (the inline replay; also restores bit-identical
 *   results under any sharding for route-1 problems, whose side plan's chunking depends on how many there are per shard);
 *   1: whenever the plan has more than one chunk.  More pending problems than a quarter of the batch (or 256) are
 *   replayed inline after all.  Forced-exact and materialising runs replay everything and never defer. */
int clr_batch_set_rescue(clr_batch* h, int mode);
/* Of the last evaluation whose results were fetched: how many problems were re-planned (negative: that many were
 * replayed inline instead), the running total, and the side plan's chunking.  Any pointer may be NULL. */
int clr_batch_get_rescue(const clr_batch* h, int* last_count, long* total, int* nchunk, int* chunk_len);

/* What a materialising run (clr_batch_enqueue(h, 1), widths 1..8) keeps in HBM:
 *   0 (default) the reference's four arrays phi, u, W, D (cholesky.h:76-78; 8 N (3 J + 1) bytes per problem);
 *   1 LEAN: W and D only (8 N (J + 1) bytes per problem, SURVEY.md 8d row A-lean).  phi[:, n] = exp(-c (t_{n+1} - t_n))
 *     and u[:, n - 1] = U~(t_n) are pure functions of the times and the coefficients (cholesky.h:127-147): the replay does
 *     not store them, and clr_batch_get_factor regenerates them on the device with the very functions the replay
 *     evaluates -- W, D and u come back bit-identical to layout 0's, phi to one ulp (the exp tier of a step is chosen per
 *     wave, and the expanding kernel groups samples into waves differently from the replay).  At B = 1024, N = 1e5, width 8 the factor shrinks
 *     from 20.5 to 7.4 GB and the materialising replay is no longer bound by its stores.  The lean factor can be
 *     expanded as long as the plan still holds the series and coefficients of the materialising run (else
 *     clr_batch_get_factor returns CLR_NOT_COMPUTED). */
int clr_batch_set_factor_layout(clr_batch* h, int layout);
/* Accuracy of the materialised factor at the chunk heads (widths 1..8).  The chunked replay starts every chunk from its
 * SCANNED start state; the scan algebra's rounding in that state -- amplified by the cancellation in
 * D_n = a - u^T S u (cholesky.h:162-175) -- shows in W and D for the ~32 samples the recurrence needs to forget it:
 * 4e-11 (of the largest entry) at a chunk's first sample against 4e-13 from sample 32 on, which is the distance of the
 * reference's own sequential recurrence from a binary128 evaluation (profiles/r06d_factor_error.txt; N = 1e5, width 8).
 * With `samples` > 0 (default 64) a materialising run recomputes the first `samples` entries of every chunk from the
 * state the PREVIOUS chunk's replay reached at the boundary -- the reference recurrence carried across it -- in a
 * second, short launch (samples / chunk_len of a replay: 4 % at the bench shape).  0: round 5's factor. */
int clr_batch_set_factor_refine(clr_batch* h, int samples);
/* Bytes of factor one problem occupies in HBM under the layout and chunking in force. */
int clr_batch_get_factor_bytes(const clr_batch* h, size_t* bytes_per_problem);


/* Enqueue one evaluation of all B problems on the handle's stream (inputs
 * already resident in HBM).  `materialize` != 0 additionally writes the factor
 * (phi, u, W, D per problem; 8 N (3J+1) bytes each) to HBM, as B separate
 * CholeskySolver.compute calls would.  On the device it is kept chunk-interleaved
 * ([i][j][chunk]: every store instruction of a wave writes 512 contiguous bytes);
 * clr_batch_get_factor returns it in the reference's storage order. */
int clr_batch_enqueue(clr_batch* h, int materialize);
/* Wait for the stream. */
int clr_batch_synchronize(clr_batch* h);
/* HBM -> host; any pointer may be NULL. */
int clr_batch_get_results(clr_batch* h, double* loglike, double* logdet,
                          double* quad, int* status);
/* One optimiser / MCMC evaluation (celerite.py:160-219 per problem: new parameters -> compute -> log_likelihood) in
 * one call: clr_batch_set_coefficients + clr_batch_enqueue(h, 0) + clr_batch_get_results.  For launch-latency-sized
 * batches (BASELINE configs[1]: a 65-us kernel) the three separate calls of a Python caller cost as much as the kernel. */
int clr_batch_evaluate(clr_batch* h, const double* jitter, const double* a_real, const double* c_real,
                       const double* a_comp, const double* b_comp, const double* c_comp, const double* d_comp,
                       double* loglike, double* logdet, double* quad, int* status);
/* A constant mean per problem (GP(kernel, mean=mu) of celerite.py for B problems): every route that reads y -- the
 * evaluation, clr_batch_solve with b == NULL, clr_batch_predict, the gradient -- then sees the residual r = y - mu[p].
 * mu_stride 1: mu[B], one value per problem; 0: mu[0] for every problem; mu == NULL removes the mean.  The caller's y
 * stays on the device untouched; the residual is formed there by one elementwise pass (a shared series with a
 * per-problem mean becomes a per-problem residual), and clr_batch_set_series keeps the mean in force and applies it to
 * the new series.  A non-finite value or a stride other than 0 / 1: CLR_INVALID_ARGUMENT, the plan unchanged.
 * clr_batch_predict returns mu[p] + K_* K^-1 r (celerite.py:279). */
int clr_batch_set_mean(clr_batch* h, const double* mu, long mu_stride);
/* clr_batch_evaluate with the mean as one more input (clr_batch_set_mean(h, mean, mean_stride) first): one library call
 * per optimiser step over (kernel parameters, mean). */
int clr_batch_evaluate_mean(clr_batch* h, const double* mean, long mean_stride, const double* jitter,
                            const double* a_real, const double* c_real, const double* a_comp, const double* b_comp,
                            const double* c_comp, const double* d_comp, double* loglike, double* logdet, double* quad,
                            int* status);
/* A mean that is LINEAR IN ITS PARAMETERS, mean_p(t_n) = sum_k w[p][k] Phi_k(t_n) with K <= CLR_MAX_MEAN_BASIS basis
 * functions: what a celerite.modeling.Model subclass passed as GP(kernel, mean=model, fit_mean=True) is when its
 * get_value(t) is linear in the parameter vector (a polynomial trend, per-instrument offsets, a sinusoid of fixed period,
 * a transit template; celerite.py:202 subtracts mean.get_value(t) on every evaluation).  The caller evaluates the basis
 * once; the plan keeps it in HBM, and an optimiser step sends B x K weights instead of a new y.
 *
 * clr_batch_set_mean_basis -- the model's design matrix, d get_value(t) / d parameter: phi is host [K][N] with
 * phi_stride == 0 (one basis for all problems) or [B][K][N] with phi_stride == K * N; uploaded once.  The weights start at
 * zero (the residual is y), also when a basis replaces another.  K == 0 or phi == NULL removes the linear mean and
 * restores the caller's y.  CLR_INVALID_ARGUMENT, the plan unchanged: a non-finite entry, K > CLR_MAX_MEAN_BASIS, another
 * stride, or a constant mean in force -- the two means are mutually exclusive (clr_batch_set_mean likewise refuses while
 * a basis is in force; a constant is the basis function 1).  Before or after clr_batch_set_series: a later
 * clr_batch_set_series keeps basis and weights in force and applies them to the new series.
 *
 * clr_batch_set_mean_weights -- mean.set_parameter_vector for B problems: w is host [B][K].  Every route that reads y --
 * the evaluation, clr_batch_solve with b == NULL, clr_batch_predict, the gradient -- then sees the residual
 *     r[p][n] = y[p][n] - m ,   m = w[p][0] Phi_0[n] ,  m = m + w[p][k] Phi_k[n]  (k = 1 .. K - 1, in this order),
 * every product and sum rounded on its own (no FMA): the bits of the same expression in NumPy.  It is formed on the
 * device by one elementwise pass over the caller's y, which stays in HBM untouched (a shared y becomes a per-problem
 * residual).  The factor of a materialising run does not depend on y and stays valid.  Weights equal to the ones in
 * force: nothing is done.  CLR_INVALID_ARGUMENT: a non-finite weight, or no basis set.
 *
 * clr_batch_grad_mean_weights -- the mean's block of GP.grad_log_likelihood (celerite.py: fit_mean): dw host [B][K],
 *     dw[p][k] = d loglike_p / d w[p][k] = Phi_k^T K_p^-1 r_p ,
 * from the factor of the last materialising run (CLR_NOT_COMPUTED without one, as clr_batch_solve): the batched solve of
 * the residual, left on the device, and one projection pass onto the resident basis -- workgroups over fixed slabs of
 * 4096 samples, their partials added in order, no atomics: the same bits on every run, for any batch size and any
 * sharding.  New weights need no new materialising run.  status (may be NULL) receives the statuses of the evaluation in
 * force; a problem whose status is not CLR_OK gets a row of zeros (clr_batch_grad's quiet semantics).  Plans of widths
 * 1..64, as clr_batch_solve (its errors otherwise).  clr_batch_get_solve_ms then reports the solve's device time and
 * clr_batch_get_mean_project_ms the projection's.
 *
 * With a linear mean in force clr_batch_grad_mean and clr_batch_grad_params(..., with_mean = 1) -- the constant mean's
 * partial -- return CLR_UNSUPPORTED, and clr_batch_predict returns the conditional mean OF THE RESIDUAL, K_* K^-1 r: the
 * caller adds sum_k w[p][k] Phi_k(x*), the model at the prediction points (celerite.py:279). */
#define CLR_MAX_MEAN_BASIS 16
int clr_batch_set_mean_basis(clr_batch* h, int K, const double* phi, long phi_stride);
int clr_batch_set_mean_weights(clr_batch* h, const double* w);
int clr_batch_grad_mean_weights(clr_batch* h, double* dw, int* status);
int clr_batch_get_mean_project_ms(const clr_batch* h, double* device_ms);
/* A noise model that is LINEAR IN ITS PARAMETERS: the variances every route reads become
 *     diag_eff[p][n] = diag[p][n] + sum_k s[p][k] Psi_k[p][n] ,   K <= CLR_MAX_NOISE_BASIS basis functions,
 * with the plan's scalar jitter added on top as before -- a jitter per instrument (diag = sigma^2, Psi_g the indicator of
 * instrument g, s_g its jitter^2), an error-bar inflation f^2 sigma^2 (Psi_0 = sigma^2, s_0 = f^2 - 1), a noise level per
 * observing season.  The caller evaluates the basis once; the plan keeps it in HBM, and an optimiser or sampler step sends
 * B x K weights instead of a new diagonal through clr_batch_set_series.
 *
 * clr_batch_set_noise_basis -- psi is host [K][N] with psi_stride == 0 (one basis for all problems) or [B][K][N] with
 * psi_stride == K * N; uploaded once.  The weights start at zero (the plan is the plain plan), also when a basis replaces
 * another.  K == 0 or psi == NULL removes the noise model and restores the caller's diagonal.  CLR_INVALID_ARGUMENT, the
 * plan unchanged: a non-finite entry (with per-problem lengths in force: within a problem's length), K >
 * CLR_MAX_NOISE_BASIS, another stride.  Before or after clr_batch_set_series: a later clr_batch_set_series /
 * _set_series_ragged keeps basis and weights in force and applies them to the new diagonal.
 *
 * clr_batch_set_noise_weights -- s is host [B][K].  Every route that reads the diagonal -- the evaluation on each of its
 * routes, the materialising runs, the gradient, the rescue side plan -- then sees
 *     diag_eff = diag + m ,   m = s[p][0] Psi_0[n] ,  m = m + s[p][k] Psi_k[n]  (k = 1 .. K - 1, in this order),
 * every product and sum rounded on its own (no FMA): the bits of NumPy's diag + (s_0 * Psi_0 + s_1 * Psi_1 + ...).  It is
 * formed on the device by one elementwise pass over the caller's diagonal, which stays in HBM untouched (a shared
 * diagonal becomes B x N variances); with per-problem lengths the tail of a row stays padding and Psi's tail is never
 * looked at.  Nothing derived from t alone is rebuilt.  The weights and the basis need only be finite: a variance that
 * comes out non-positive shows in the problem's status, as for a bad diag.  The factor of an earlier materialising run
 * is that of the earlier variances.  Weights equal to the ones in force: nothing is done.  CLR_INVALID_ARGUMENT: a
 * non-finite weight, or no basis set.
 *
 * clr_batch_grad_noise_weights -- ds host [B][K],
 *     ds[p][k] = d loglike_p / d s[p][k] = 1/2 sum_n Psi_k[p][n] (alpha_n^2 - c_n) ,  alpha = K_p^-1 r_p ,  c = diag(K_p^-1),
 * from the factor of a materialising run MADE AFTER the weights (and the basis, and the series) were set: CLR_NOT_COMPUTED
 * without one, or when any of them changed since -- materialise again.  It runs clr_batch_leave_one_out's two device
 * parts (the diagonal's recurrence, the solve of the residual) and one projection pass onto the resident basis --
 * workgroups over fixed slabs of 4096 samples, their partials added in order, no atomics: the same bits on every run, for
 * any batch size and any sharding.  status (may be NULL) receives the statuses of the evaluation in force; a problem whose
 * status is not CLR_OK gets a row of zeros.  clr_batch_leave_one_out's domain (its refusals otherwise, naming this
 * entry): celerite-only plans of widths 1..64, narrow plans chunked, wide plans N >= 512, no per-problem lengths.
 * clr_batch_get_leave_one_out_ms then reports the device time of the diagonal and the solve,
 * clr_batch_get_noise_project_ms the projection's. */
#define CLR_MAX_NOISE_BASIS 16
int clr_batch_set_noise_basis(clr_batch* h, int K, const double* psi, long psi_stride);
int clr_batch_set_noise_weights(clr_batch* h, const double* s);
int clr_batch_grad_noise_weights(clr_batch* h, double* ds, int* status);
int clr_batch_get_noise_project_ms(const clr_batch* h, double* device_ms);
/* A PER-SAMPLE AMPLITUDE MODEL (multi-band): the same latent process f seen with another amplitude per band,
 *     y_n = s_n f(t_n) + eps_n ,   s[p][n] = sum_k a[p][k] Gamma_k[p][n] ,   K <= CLR_MAX_AMPLITUDE_BASIS basis functions
 * -- multi-colour photometry of one variable source (Gamma_k the indicator of band k, a_k its amplitude), a radial velocity
 * next to an activity indicator, a chromatic amplitude law (Gamma a polynomial in wavelength): the rank-one Kronecker case
 * of multi-band celerite models.  With S = diag(s) the data's covariance is K_y = S K S + D = S (K + S^-1 D S^-1) S, so
 *     log det K_y = log det K' + 2 sum_n log|s_n| ,   r^T K_y^-1 r = y'^T K'^-1 y' ,   K' = K + diag(d'),
 *     y'_n = r_n / s_n ,   d'_n = d_n / (s_n * s_n)
 * and no new factorisation is needed: every route of the plan evaluates the model once the device has rewritten the
 * series it reads.  An optimiser or sampler step sends B x K amplitudes.
 *
 * clr_batch_set_amplitude_basis -- gamma is host [K][N] with gamma_stride == 0 (one basis for all problems) or [B][K][N]
 * with gamma_stride == K * N; uploaded once, before or after clr_batch_set_series.  Setting a basis alone changes nothing:
 * zero amplitudes are no neutral start (s = 0), so the plan stays the plain plan until the first clr_batch_set_amplitudes;
 * a new basis drops the amplitudes in force.  K == 0 or gamma == NULL removes the model and restores the plain plan, bit
 * for bit.  CLR_INVALID_ARGUMENT, the plan unchanged: a non-finite entry (with per-problem lengths in force: within a
 * problem's length, of a shared basis up to the longest problem), K > CLR_MAX_AMPLITUDE_BASIS, another stride, a constant
 * mean in force -- the constant mean (clr_batch_set_mean) and the amplitude model are mutually exclusive, as the two means
 * are: a constant in data units is the mean-basis function 1; clr_batch_set_mean refuses likewise while an amplitude
 * basis is set.  A later clr_batch_set_series / _set_series_ragged keeps basis and amplitudes in force and applies them
 * to the new series.
 *
 * clr_batch_set_amplitudes -- a is host [B][K].  The device forms, every product, sum and quotient rounded on its own (no
 * FMA),
 *     s  = a[p][0] Gamma_0[n] ,  s = s + a[p][k] Gamma_k[n]  (k = 1 .. K - 1, in this order)
 *     y' = r / s          r: the caller's y, or the residual of the linear mean in force
 *     d' = d / (s * s)    d: the caller's diag, or diag_eff of the noise model in force
 * -- the bits of those NumPy expressions -- and every route reads y' and d'; the plan's scalar jitter is added on top of
 * d' as before: it is part of the kernel, in latent units.  The caller's arrays stay in HBM untouched (a shared y or diag
 * becomes per problem), s stays resident as [B][N] doubles.  After clr_batch_set_mean_weights / _set_noise_weights the
 * division is applied again.  With per-problem lengths the tails stay padding; the tails of Gamma and s are never looked
 * at.  The factor of an earlier materialising run is that of the earlier amplitudes.  Amplitudes equal to the ones in
 * force: nothing is done.  CLR_INVALID_ARGUMENT: a non-finite amplitude, or no basis set.
 *     The same pass sums L[p] = sum_n log|s[p][n]| over the problem's length (fixed slabs of 4096 samples, the slabs'
 * partials added in slab order, no atomics: a problem's bits depend on neither the batch size, a sharding nor the run);
 * clr_batch_get_log_amplitude_sum returns it (zeros while no amplitudes are in force).  Every entry that returns a plan's
 * results -- clr_batch_get_results, hence _evaluate*, the value of clr_batch_grad / _grad_params -- then reports, computed
 * on the host in double with exactly these operations,
 *     logdet = logdet' + (L + L) ,   loglike = loglike' - L ,   quad = quad'     (primed: of the system K', y').
 * A zero or non-finite s_n inside a problem's length: that problem reports NaN and CLR_INVALID_ARGUMENT (the quiet
 * semantics of a draw the kernel program refuses; its scans ran on the stand-in s_n = 1); no other problem is affected.
 *
 * clr_batch_grad_amplitudes -- da host [B][K]: with alpha' = K'^-1 y', c' = diag(K'^-1) and d' without the jitter,
 *     da[p][k] = d loglike_p / d a[p][k] = sum_n Gamma_k[p][n] (alpha'_n y'_n + d'_n (c'_n - alpha'_n^2) - 1) / s_n ,
 * from the factor of a materialising run MADE AFTER the amplitudes (and the basis, the noise weights, the series) were set:
 * CLR_NOT_COMPUTED otherwise.  clr_batch_grad_noise_weights' steps, domain, refusals (naming this entry) and status
 * semantics; clr_batch_get_amplitude_project_ms reports the projection's device time.
 *     With amplitudes in force clr_batch_grad_mean_weights returns sum_n Phi_k alpha'_n / s_n and
 * clr_batch_grad_noise_weights 1/2 sum_n Psi_k (alpha'_n^2 - c'_n) / s_n^2 -- the data-unit alpha_y = alpha' / s and
 * diag(K_y^-1) = c' / s^2 --; without amplitudes their bits are unchanged.  clr_batch_fit_mean_weights returns
 * CLR_UNSUPPORTED while amplitudes are in force (its right-hand sides would be Phi / s); so does clr_batch_grad_mean's
 * partial with respect to a constant mean.
 *     The factor's consumers run on the system in force, K' and y': clr_batch_predict*, _forecast, _predict_terms,
 * _predict_cov and _sample_conditional return the posterior of the LATENT process f, exactly (k*^T S K_y^-1 r = k*^T K'^-1
 * y', k** - k*^T S K_y^-1 S k* = k** - k*^T K'^-1 k*): a band's curve is a_band f.  clr_batch_solve(b) is K'^-1 b, _dot and
 * _dot_L multiply by K' and its factor; leave-one-out and the one-step-ahead innovations are those of the scaled samples. */
#define CLR_MAX_AMPLITUDE_BASIS 16
int clr_batch_set_amplitude_basis(clr_batch* h, int K, const double* gamma, long gamma_stride);
int clr_batch_set_amplitudes(clr_batch* h, const double* a);
int clr_batch_get_log_amplitude_sum(clr_batch* h, double* L);
int clr_batch_grad_amplitudes(clr_batch* h, double* da, int* status);
int clr_batch_get_amplitude_project_ms(const clr_batch* h, double* device_ms);
/* clr_batch_fit_mean_weights -- the weights that MAXIMISE the log-likelihood of every problem at the coefficients in
 * force.  The log-likelihood is exactly quadratic in the weights, so they need no optimiser: with r = y - Phi w0 the
 * residual at the weights w0 in force,
 *     G = Phi^T K^-1 Phi ,  d = Phi^T K^-1 r ,  w_hat = w0 + G^-1 d ,  cov(w_hat) = G^-1 ,
 *     quad_profiled = r^T K^-1 r - d^T G^-1 d     (the quadratic form at w_hat),
 * one generalised-least-squares solve from the factor of the last materialising run (CLR_NOT_COMPUTED without one, as
 * clr_batch_solve; new weights or a new y need no new run).  The K + 1 right-hand sides (Phi_0 .. Phi_K-1, r) are formed on
 * the device from the resident basis and residual -- nothing is uploaded but the B x K weights in force -- and solved by
 * the batched solve's kernels a tile of columns at a time (clr_batch_set_mean_fit_tile: right-hand sides per tile, 0 =
 * as many as fit 1 GiB of buffers; no result depends on it); a Gram pass over fixed slabs of 4096 samples, partials
 * added in order, no atomics, forms the bordered matrix [[G, d], [d^T, q]] with its symmetric part stored; one thread per
 * problem then scales G to unit diagonal, factors it by an unpivoted Cholesky and solves.  A problem's bits depend on
 * neither the batch size, the tile, a sharding nor the run.
 *   w_hat host [B][K], cov [B][K][K], gram [B][K+1][K+1] (the bordered matrix), quad_profiled [B], logdet_gram [B]
 *   (log det G), status [B]; any of them may be NULL.  min_pivot: finite, in [0, 1).
 * Per problem: when the status of the evaluation in force is not CLR_OK (no factor, or a draw the kernel program refused)
 * the problem reports that status, w_hat is the weights in force and every other output of it is NaN.  When a diagonal
 * entry of G is not positive, or a pivot of the scaled G is not positive or lies below min_pivot (a rank-deficient
 * basis), the status is CLR_NOT_POSITIVE_DEFINITE, w_hat is the weights in force, cov, quad_profiled and logdet_gram are
 * NaN, and gram is still returned.  No problem's refusal changes another's bits.
 * With a flat prior on the weights the marginal log-likelihood follows on the host:
 *     loglike_profiled = -1/2 (quad_profiled + log det K + N log 2 pi) ,
 *     loglike_marginal = loglike_profiled - 1/2 log det G + 1/2 K log 2 pi .
 * The weights in force are NOT changed (clr_batch_set_mean_weights(w_hat) applies them).  CLR_INVALID_ARGUMENT, the plan
 * unchanged: no basis set, a constant mean in force, min_pivot out of range.  CLR_UNSUPPORTED: what clr_batch_solve
 * refuses (general terms, widths above 64, unchunked plans), or more than 65535 problems in the plan (a grid axis).
 * clr_batch_get_mean_fit_ms: the device time of the last call's solves, Gram pass (with its finish) and small solve.
 *
 * clr_gram_solve -- the small solve alone, on the host (no GPU): the routine the device runs per problem, the same bits.
 * gram_bordered [nprob][K+1][K+1], w0 [nprob][K] (NULL: zeros); outputs as above, any may be NULL; 1 <= K <=
 * CLR_MAX_MEAN_BASIS.  Returns CLR_INVALID_ARGUMENT for a bad K or min_pivot; refusals are per problem, in status. */
int clr_batch_fit_mean_weights(clr_batch* h, double min_pivot, double* w_hat, double* cov, double* gram,
                               double* quad_profiled, double* logdet_gram, int* status);
int clr_batch_set_mean_fit_tile(clr_batch* h, int rhs);
int clr_batch_get_mean_fit_ms(const clr_batch* h, double* solve_ms, double* gram_ms, double* small_ms);
int clr_gram_solve(int nprob, int K, const double* gram_bordered, const double* w0, double min_pivot, double* w_hat,
                   double* cov, double* quad_profiled, double* logdet_gram, int* status);
/* CholeskySolver::solve (cholesky.h:218-318) for every problem of the plan at once: x = K_p^-1 b_p from the factor of
 * the last materialising run (clr_batch_enqueue(h, 1); either factor layout), parallel in n -- forward substitution,
 * division by D and backward substitution as two chunked affine scans whose chunk maps are formed once and shared by
 * all right-hand sides and both sweeps (csrc/clr_bsolve_kernels.h).  b and x: host arrays [B][nrhs][N] (row-major:
 * right-hand side k of problem p at (p * nrhs + k) * N); b == NULL with nrhs == 1: the plan's own y (already in HBM --
 * GP.apply_inverse(y) of celerite.py:307-328 for B problems without an upload).  Widths 1..8: chunked plans (N >= 128).
 * Widths 9..64 (round 6): the factor lies in the reference's storage and the sweeps are the object API's wave-per-chunk
 * affine scans (csrc/wsweep_kernels.hip) launched once for the whole batch, grid.z = problem; N >= 512.  A problem
 * whose materialising run reported CLR_NOT_POSITIVE_DEFINITE has no factor: its x is undefined (non-finite).  With the
 * LEAN layout the sweeps regenerate phi and u from (t, coefficients) and move 9 instead of 25 doubles per sample through
 * HBM four times: the plan must still hold the series and coefficients of the materialising run. */
int clr_batch_solve(clr_batch* h, int nrhs, const double* b, double* x);
/* CholeskySolver::predict (cholesky.h:599-698: the conditional mean K_p(x*, t_p) K_p^-1 y_p behind GP.predict,
 * celerite.py:330-420) for every problem of the plan, M prediction points each: xs host [B][M] (xs_stride = M) or one
 * set of M points shared by all problems (xs_stride = 0); pred host [B][M].  alpha = K^-1 y comes from the batched solve
 * on the factor of the last materialising run (any layout, widths 1..64) and stays on the device; the two passes over
 * the prediction points are the object API's chunked diagonal scans on the plan's resident times and coefficients
 * (sorted points: parallel in n; unsorted: the sequential walk of the reference).  Under a linear mean
 * (clr_batch_set_mean_basis) y is the residual and pred its conditional mean alone: the model at x* is the caller's. */
int clr_batch_predict(clr_batch* h, int M, const double* xs, long xs_stride, double* pred);
/* The other half of GP.predict (return_var=True, celerite.py:465-470): the conditional variance
 *     var_p(x*) = k_p(0) - k*^T K_p^-1 k* ,  k*_n = k_p(x* - t_{p,n}) ,  k_p(0) = sum a_real + sum a_comp
 * (no jitter, no observational variance) for every problem of the plan at M points each; xs as for clr_batch_predict
 * (host [B][M] with xs_stride = M, or M shared points with xs_stride = 0; the points need not be sorted), var host
 * [B][M].  Only xs goes up and only var comes down: the cross-covariances are formed on the device from the plan's
 * times, the coefficients in force and the points, and k*^T K^-1 k* = sum_n z_n^2 / D_n with z = L^-1 k* needs the
 * forward half of a solve only, on the factor of the last materialising run (either layout).  The points are worked
 * through in tiles (clr_batch_set_predict_tile), so device scratch is bounded whatever M is, and a point's result does
 * not depend on the tile size or on the tile it falls in (bit for bit).  Widths 1..8: csrc/clr_bpredvar_kernels.h on
 * chunked plans (N >= 128), the chunk maps shared with clr_batch_solve; widths 9..64: the forward sweep of
 * clr_batch_solve's wide route, N >= 512 (else CLR_UNSUPPORTED).  A mean (clr_batch_set_mean) does not enter.  A
 * problem whose materialising run reported CLR_NOT_POSITIVE_DEFINITE has no factor: its var, like its pred, is
 * undefined (usually non-finite) -- read the statuses.  clr_batch_get_solve_ms then reports this call's device time. */
int clr_batch_predict_var(clr_batch* h, int M, const double* xs, long xs_stride, double* var);
/* Prediction points per tile of clr_batch_predict_var; points <= 0 (the default): automatic -- the most whose
 * right-hand-side, offset and start-state buffers fit in 1 GiB, at most 65535 (grid.z), at least 1.  The 1 GiB rule
 * bounds the automatic choice only: a tile set here is taken as given up to 65535 and M, and clr_batch_predict_var
 * returns the allocation's status if the device cannot hold its buffers. */
int clr_batch_set_predict_tile(clr_batch* h, int points);
/* clr_batch_predict_var -- same arguments, same meaning, same preconditions -- in O((N + M) J^2) per problem instead of
 * O(M N J): with the factorisation's forward state S (S+_n = S_n + D_n W_n W_n^T, S_{n+1} = Phi S+_n Phi) and the backward
 * matrix recurrence Q of clr_batch_leave_one_out, for a point x with m samples at or before it
 *     psi = exp(-c (x - t_{m-1})) ,  w = psi o u(x) ,  e = v(x) - psi o (S+_{m-1} w) ,  e' = exp(-c (t_m - x)) o e
 *     var(x) = k(0) - w^T S+_{m-1} w - e'^T Q_m e'
 * (csrc/clr_bpredvar_rec_kernels.h): one forward and one backward pass over the series per tile plus O(J^2) per point.
 * Narrow plans only (widths 1..8, chunked: N >= 128, either factor layout); a wide plan returns CLR_UNSUPPORTED -- take
 * clr_batch_predict_var there.  The points need not be sorted: ascending input is detected in O(M), anything else is
 * sorted as an index permutation on the host (shared points once) and the results are scattered back.  Tiles are runs
 * of consecutive sorted points: automatic -- the most whose per-point buffers (2 J + 1 doubles per problem) fit in
 * 1 GiB -- or clr_batch_set_predict_tile's, up to M; a point's result depends on neither the tile, the batch nor the
 * sharding, bit for bit.  The chunks' start states of both recurrences depend on the factor only and are kept until
 * the next materialising run (the backward ones shared with clr_batch_leave_one_out, the chunk maps with
 * clr_batch_solve).  Agrees with clr_batch_predict_var to rounding (both within 1e-10 k(0) of the reference), not bit
 * for bit; a point's features are evaluated at its absolute phase d x, as the factor's are at d t_n, so where d t
 * reaches ~1e9 the result carries that phase's rounding (1e-8 k(0) at t ~ 3e8), which clr_batch_predict_var's
 * cross-covariances of x - t_n do not.  clr_batch_get_solve_ms then reports this call's device time. */
int clr_batch_predict_var_recurrence(clr_batch* h, int M, const double* xs, long xs_stride, double* var);
/* The causal half of the factor of the last materialising run, K = L diag(D) L^T: the one-step-ahead residuals
 * (innovations) z = L^-1 b and their variances D for every problem.  b host [B][nrhs][N] as for clr_batch_solve; b == NULL
 * with nrhs == 1: the residual in force (y less the mean of clr_batch_set_mean / _set_mean_weights, already in HBM, no
 * upload), any other nrhs with b == NULL is CLR_INVALID_ARGUMENT.  innovation [B][nrhs][N] = L^-1 b, undivided;
 * variance [B][N] = D (diag_n + jitter enters it), shared by all right-hand sides; status [B].  Each may be NULL, not all:
 * CLR_INVALID_ARGUMENT.  For the residual r:  E[y_n | y_<n] = y_n - z_n with variance D_n, z_n / sqrt(D_n) is white and
 * standard normal under the model, and sum_n -1/2 (log 2 pi D_n + z_n^2 / D_n) is the log-likelihood.  With
 *     z_n = b_n - u[n] . g_n ,  g+_n = g_n + W[n] z_n ,  g_{n+1} = phi[n] o g+_n ,  g_0 = 0
 * this is the forward sweep of clr_batch_solve before its division by D, and none of its backward half: widths 1..8 one
 * forward chunked scan on chunked plans (N >= 128, either factor layout; csrc/clr_bfilter_kernels.h), the chunk maps shared
 * with clr_batch_solve under its validity rule; widths 9..64 the forward sweep of clr_batch_solve's wide route, N >= 512
 * (else CLR_UNSUPPORTED, as clr_batch_solve).  Statuses are those of the evaluation in force (clr_batch_get_results); rows
 * of problems whose status is not CLR_OK are NaN in every output.  clr_batch_get_solve_ms then reports this call's device
 * time. */
int clr_batch_one_step_ahead(clr_batch* h, int nrhs, const double* b, double* innovation, double* variance, int* status);
/* The causal forecast: mean and variance of every problem's process at M points each given only the samples STRICTLY
 * before the point, p(f(x) | y_n : t_n < x), from the factor of the last materialising run -- xs, xs_stride, sorting and
 * tiling exactly as clr_batch_predict_var_recurrence (host [B][M] with xs_stride = M, or M shared points with
 * xs_stride = 0; unsorted points go through a host index permutation, NaN last, and the results are scattered back; tiles
 * follow clr_batch_set_predict_tile).  With m = #{n : t_n < x}, g+ the forward state of clr_batch_one_step_ahead on the
 * residual in force and S+ the factorisation's own state (S+_n = S_n + D_n W_n W_n^T, S_{n+1} = Phi_n S+_n Phi_n, S_0 = 0)
 *     psi = exp(-c (x - t_{m-1})) ,  w = psi o u(x) ,  mean(x) = w^T g+_{m-1} ,  var(x) = k(0) - w^T S+_{m-1} w
 * and m = 0 gives the prior: mean 0, var k(0).  mean host [B][M]: the conditional mean of the residual process plus, as
 * in clr_batch_predict, the constant mean of clr_batch_set_mean; under a linear mean the residual's alone -- the model at
 * the points is the caller's.  var host [B][M]: the conditional variance of the latent process (no jitter, no
 * observational variance), as clr_batch_predict_var.  Either may be NULL, not both; with var == NULL the state S is
 * neither formed nor carried.  Strict < is deliberate: at x = t_n the result is the one-step-ahead prediction of sample n,
 * y_n - z_n and D_n - diag_n - jitter.  One forward pass over the series per tile plus O(J^2) per point
 * (csrc/clr_bfilter_kernels.h): narrow plans only (widths 1..8, chunked: N >= 128, either factor layout); a wide plan
 * returns CLR_UNSUPPORTED -- take clr_batch_predict / clr_batch_predict_var there.  The start states of S are shared with
 * clr_batch_predict_var_recurrence and kept until the next materialising run; those of g follow the residual and are
 * formed by every call.  A point's exponentials are the library's: its result depends on neither the tile, the batch nor
 * the sharding, bit for bit.  A NaN point gives NaN; rows of problems whose status is not CLR_OK are NaN.
 * clr_batch_get_solve_ms then reports this call's device time. */
int clr_batch_forecast(clr_batch* h, int M, const double* xs, long xs_stride, double* mean, double* var);
/* The periodogram under the plan's covariance: for every problem b and F trial angular frequencies the generalised-
 * least-squares fit of A cos(w tau) + B sin(w tau), tau_n = t_n - t_ref, plus a constant with `offset` != 0, to the
 * residual in force r (as clr_batch_one_step_ahead's b == NULL) with K^-1 as the metric, from the factor of the last
 * materialising run.  omega host [F] shared by all problems (omega_stride 0) or [B][F] (omega_stride F), the xs /
 * xs_stride convention of the point consumers.  The columns are c_n = cos(w tau_n), s_n = sin(w tau_n) evaluated as one
 * subtraction, one product and the library's sincos; X = (c, s), K = 2, or X = (1, c, s), K = 3.  With G = X^T K^-1 X,
 * d = X^T K^-1 r, q = r^T K^-1 r:
 *     gram   [B][F][K+1][K+1] = [[G, d], [d^T, q]] -- clr_gram_solve's layout, its symmetric part stored symmetric;
 *     coef   [B][F][K]        = G^-1 d: the fitted amplitudes, the offset first (on top of the mean in force);
 *     cov    [B][F][K][K]     = G^-1;
 *     power  [B][F]           = 1/2 d^T coef, with the offset less 1/2 d_0^2 / G_00: the gain in maximised log-likelihood
 *                               over the model without the sinusoid (not clamped at 0);
 *     status [B][F].
 * Any output may be NULL, not all.  The small solve is clr_batch_fit_mean_weights' (unit-diagonal scaling, unpivoted
 * Cholesky, min_pivot), per (b, f), the bits of clr_gram_solve on the returned gram; power is the sum above from left to
 * right, every operation rounded on its own.  A (b, f) whose G has a diagonal entry that is not positive, or a pivot of the
 * scaled G not above zero or below min_pivot (w = 0; with the offset a frequency far below 1 / T), has status
 * CLR_NOT_POSITIVE_DEFINITE, coef, cov and power NaN and its gram returned; no other entry changes.  The status of the
 * evaluation in force comes first: where it is not CLR_OK it is the status of every frequency of the problem, whose other
 * outputs are NaN.  With K = L diag(D) L^T every inner product is sum_n z_x[n] z_y[n] / D_n, z_x = L^-1 x: the columns are
 * formed on the fly from the resident times, whitened by the forward recurrence of clr_batch_one_step_ahead and folded
 * into running sums (csrc/clr_bperiodogram_kernels.h) -- nothing is uploaded but the frequencies, no right-hand side is
 * written.  A noise model in force is part of the factor.  A result's bits depend on the plan's chunking and on nothing
 * else: not on F, the tile, the batch, the sharding or the frequency's place in omega.
 * CLR_INVALID_ARGUMENT, the plan unchanged: F < 0, omega NULL with F > 0, a stride other than 0 or F, a non-finite
 * frequency or t_ref, min_pivot outside [0, 1), all outputs NULL.  F == 0: CLR_OK, nothing written.  CLR_NOT_COMPUTED
 * without a materialising run.  CLR_UNSUPPORTED: wide plans (widths 9..64; take clr_batch_set_mean_basis with (cos, sin)
 * and clr_batch_fit_mean_weights per frequency), general terms, unchunked plans (N < 128), per-problem lengths, amplitudes
 * in force (the resident series are y / s), B > 65535. */
int clr_batch_periodogram(clr_batch* h, int F, const double* omega, long omega_stride, double t_ref, int offset, double min_pivot,
                          double* power, double* coef, double* cov, double* gram, int* status);
/* Frequencies per tile of clr_batch_periodogram; 0 (the default): as many as fit 1 GiB of scratch.  Results do not depend
 * on it. */
int clr_batch_set_periodogram_tile(clr_batch* h, int frequencies);
/* Device time of the last clr_batch_periodogram's kernels (HIP events; no copies). */
int clr_batch_get_periodogram_ms(const clr_batch* h, double* device_ms);
/* Component separation: the posterior of the process of a GROUP of kernel terms, for G groups at M points per problem,
 * from the factor of the last materialising run:  mean_g(x) = k_g*^T K^-1 r  and  var_g(x) = k_g(0) - k_g*^T K^-1 k_g*,
 * where k_g is the sum of the group's terms and K the full kernel with its diagonal.  groups host [G][T], T = J_real +
 * J_comp bytes per group in the order of the coefficients (real terms first, then the complex ones), each 0 or 1 -- any
 * other byte is CLR_INVALID_ARGUMENT; G >= 1.  mean, var host [B][G][M]; either may be NULL, not both.  xs, xs_stride,
 * sorting and tiling exactly as clr_batch_forecast (the per-point buffers grow with G: 2 J doubles per problem, and
 * G (J + 1) more with var).  The group with every term gives clr_batch_predict's conditional mean of the residual and
 * clr_batch_predict_var_recurrence's variance to rounding; the empty group gives exactly 0 twice.  NO mean is added: the
 * mean of clr_batch_set_mean / _set_mean_weights belongs to no term, and the residual in force (y less that mean) is what
 * is decomposed.  The variance of a group is not the sum of its terms' variances, which is why groups are an input.
 * m = #{n : t_n <= x} as in clr_batch_predict_var_recurrence.  Cost: with mean the batched solve of the residual plus
 * one forward and one backward pass over the times and alpha alone; with var one forward and one backward pass over the
 * factor; O(G J^2) per point; whatever G (csrc/clr_bterms_kernels.h).  Narrow plans only (widths 1..8, chunked: N >= 128,
 * either factor layout): a wide plan returns CLR_UNSUPPORTED -- clr_batch_predict covers the full kernel there -- and so
 * does an unchunked one, as for clr_batch_predict.  With var the start states of S and Q are shared with clr_batch_predict_var_recurrence / clr_batch_leave_one_out
 * and kept until the next materialising run; a call without var neither forms nor invalidates them.  A point's
 * exponentials are the library's: its result depends on neither the tile, the batch nor the sharding, bit for bit.  A NaN
 * point gives NaN; rows of problems whose status is not CLR_OK are NaN.  clr_batch_get_solve_ms then reports this call's
 * device time, the solve included. */
int clr_batch_predict_terms(clr_batch* h, int M, const double* xs, long xs_stride, int G, const unsigned char* groups,
                            double* mean, double* var);
/* The posterior covariance of the latent process between M points per problem (GP.predict(..., return_cov = True),
 * celerite.py:283-291, for B problems, without its dense N x M solve), from the factor of the last materialising run:
 * cov host [B][M][M], cov[b][i][j] = k(x_i - x_j) - k*_i^T K^-1 k*_j -- no jitter, no observational variance, as
 * clr_batch_predict_var, whose value is the diagonal -- full and symmetric to the bit.  xs, xs_stride and unsorted input as
 * clr_batch_forecast (both axes of cov come back in the caller's order); a NaN point is CLR_INVALID_ARGUMENT.  With the
 * per-point vectors e_j, r_j and the J x J transports T_j of the forward substitution's state between consecutive sorted
 * points (csrc/clr_bcond_kernels.h) cov_ij = r_j^T T_{j-1} ... T_i e_i for i <= j: one forward and two backward passes
 * over the factor, O(J^3) per point and chunk, O(J^2) per pair.  Device scratch is bounded by tiling over PROBLEMS -- a
 * problem needs all its points at once: about M (J^2 + 4 J) + M^2 doubles each, as many problems per tile as fit 1 GiB
 * (clr_batch_set_conditional_tile: the caller's; 0: automatic); a single problem that does not fit returns the
 * allocation's status.  A problem's bits depend on neither the tile, the batch nor the sharding.  Narrow plans only
 * (widths 1..8, chunked: N >= 128, either factor layout): CLR_UNSUPPORTED otherwise.  The start states of S and Q are
 * shared with clr_batch_predict_var_recurrence / clr_batch_leave_one_out.  Rows of problems whose status is not CLR_OK are
 * NaN.  clr_batch_get_solve_ms then reports this call's device time (the kernels of every tile). */
int clr_batch_predict_cov(clr_batch* h, int M, const double* xs, long xs_stride, double* cov);
int clr_batch_set_conditional_tile(clr_batch* h, int problems);
/* Joint draws of the latent process at M points per problem given the data (GP.sample_conditional, celerite.py:327-332,
 * for B problems, without its dense covariance and its O(M^3) factorisation): normals and draws host [B][size][M],
 * size >= 1; draws = L diag(d)^1/2 n with C + regularize I = L diag(d) L^T, C the covariance of clr_batch_predict_cov --
 * the ZERO-MEAN part: the mean is clr_batch_predict's and the caller's to add.  normals[..][r] belongs to the caller's point
 * r; the factor is taken in ascending order of the points (ties in the caller's order).  L and d follow from the celerite
 * recurrence over the points with the transports in place of the diagonal decay: O(J^3) per point, O(J^2) per point and
 * draw; no M x M matrix is formed.  The rule for a pivot d_j, k(0) the problem's own:  d_j < -min_pivot k(0) or not finite
 * -- the problem is refused, status[b] = CLR_NOT_POSITIVE_DEFINITE, its rows NaN;  |d_j| <= min_pivot k(0) -- the point
 * is a function of the earlier ones (a repeated point, a point on a sample without noise): its own normal does not enter.
 * min_pivot finite in [0, 1), regularize finite and >= 0, else CLR_INVALID_ARGUMENT.  status [B] or NULL: the
 * evaluation's status where that is not CLR_OK (rows NaN), else the factorisation's.  Points, tiles (2 size M doubles in
 * place of M^2), coverage, shared state and timing as clr_batch_predict_cov. */
int clr_batch_sample_conditional(clr_batch* h, int M, const double* xs, long xs_stride, int size, const double* normals,
                                 double regularize, double min_pivot, double* draws, int* status);
/* diag(K^-1), K^-1 r and the leave-one-out log predictive density of every problem from the factor of the last
 * materialising run.  kinv_diag [B][N], alpha [B][N], loo_logpdf [B], status [B]: each may be NULL and is then neither
 * computed beyond need nor copied down (alpha or loo_logpdf: the batched solve of the residual in force runs); all four
 * NULL: CLR_INVALID_ARGUMENT.  With c_n = (K^-1)_nn and alpha = K^-1 r (r = y less the mean in force):
 *     y_n - mu_-n = alpha_n / c_n ,  sigma^2_-n = 1 / c_n ,  log p(y_n | y_-n) = -1/2 log(2 pi / c_n) - 1/2 alpha_n^2 / c_n
 * and loo_logpdf is the sum over n; the in-sample GP.predict (celerite.py:270-272) is mu_n = y_n - s_n alpha_n,
 * var_n = s_n - s_n^2 c_n with s_n = diag_n + jitter.  All N entries of c come from ONE backward matrix recurrence on
 * the factor, O(N J^2) per problem (csrc/clr_binvdiag_kernels.h): widths 1..8 on chunked plans (N >= 128), either factor
 * layout, the chunk maps shared with clr_batch_solve; widths 9..64 one wave per problem, sequential in n, N >= 512 (else
 * CLR_UNSUPPORTED, as clr_batch_solve).  loo_logpdf is summed by one workgroup per problem in a fixed order (samples
 * i, i + 256, ... per thread, then a tree): no atomics, a problem's bits depend on neither the batch nor the sharding.
 * Statuses are those of the evaluation in force (clr_batch_get_results); rows of problems whose status is not CLR_OK are
 * NaN in every output. */
int clr_batch_leave_one_out(clr_batch* h, double* kinv_diag, double* alpha, double* loo_logpdf, int* status);
/* Device time of the last clr_batch_leave_one_out's three parts (HIP events): the diagonal, the solve, the reduction; a
 * part that did not run reports 0. */
int clr_batch_get_leave_one_out_ms(const clr_batch* h, double* diag_ms, double* solve_ms, double* reduce_ms);
/* CholeskySolver::dot_L (cholesky.h:409-431: y = L z with K = L L^T, what GP.sample draws, celerite.py:422-451) for
 * every problem of the plan from the factor of its last materialising run (either layout): z, y host [B][nrhs][N].
 * Widths 1..8: a chunked diagonal scan on the chunk-interleaved factor, lane = (problem, chunk)
 * (csrc/clr_bdotl_kernels.h); widths 9..64: the object API's wave-per-chunk scan launched once for the whole batch
 * (grid.z = problem; series shorter than 2048 samples: the sequential kernel per problem).  clr_batch_get_solve_ms
 * then reports this call's device time. */
int clr_batch_dot_L(clr_batch* h, int nrhs, const double* z, double* y);
/* CholeskySolver::dot (cholesky.h:441-596: y = K z, GP.dot of celerite.py:453-489) for every problem of the plan, K_p given
 * by the plan's resident times and the coefficients in force -- its diagonal is sum a_real + sum a_comp + jitter, the
 * observational variance is not part of it (:483-485); no factor and no materialising run are needed.  z, y host
 * [B][nrhs][N].  Widths 1..8: both triangles as chunked diagonal scans with the features evaluated on the fly, lane =
 * (problem, chunk) (csrc/clr_bdot_kernels.h); widths 9..64: the object API's kernels problem by problem. */
int clr_batch_dot(clr_batch* h, int nrhs, const double* z, double* y);
/* Device time of the last clr_batch_solve (HIP events around its kernels: relayout, the five phases, relayout back;
 * the host <-> HBM copies of b and x are outside). */
int clr_batch_get_solve_ms(const clr_batch* h, double* device_ms);
/* After a materialising run: copy problem p's factor to host buffers. */
int clr_batch_get_factor(clr_batch* h, int p, double* phi, double* u, double* W, double* D);

/* Runs `steps` evaluations back to back, bracketing every kernel with HIP
 * events recorded on the handle's stream.  kernel_ms[6] receives the SUMMED
 * device time of the relayout / summarise / prefix / correct / replay / finalise
 * kernels, total_ms the first-event-to-last-event time.  In layout 1 only:
 * with relayout_each_step != 0 the row-major -> interleaved transposition is
 * redone inside every step (the cost when every evaluation brings NEW series);
 * otherwise it is done once, outside the timed region (fixed series, new
 * hyper-parameters: the MCMC / optimiser loop of celerite.py:160-219). */
int clr_batch_run_timed(clr_batch* h, int materialize, int steps, int relayout_each_step,
                        double* total_ms, double* kernel_ms /* [6] */);

/* Per-kernel device times of the REAL loop: with profiling on, every clr_batch_enqueue
 * brackets its kernels with HIP events on the plan's stream (up to 4096 evaluations since
 * the switch); clr_batch_get_profile synchronises and returns the summed milliseconds per
 * kernel (same order as clr_batch_run_timed) and the number of evaluations recorded. */
/* on = 2: only the summarize kernel (the dominant one; the warm-started recurrence when that runs) is bracketed --
 * two event records per evaluation instead of seven (an event record costs ~5 us of stream time); widths 1..8. */
int clr_batch_set_profiling(clr_batch* h, int on);
int clr_batch_get_profile(clr_batch* h, double* kernel_ms /* [6] */, int* steps);



/* Convenience: create + set + enqueue + get + destroy, host pointers in/out. */
int clr_batch_log_likelihood(int B, int N, int J_real, int J_comp,
                             const double* jitter,
                             const double* a_real, const double* c_real,
                             const double* a_comp, const double* b_comp,
                             const double* c_comp, const double* d_comp,
                             const double* t, long t_stride,
                             const double* diag, long diag_stride,
                             const double* y, long y_stride,
                             double* loglike, double* logdet, double* quad,
                             int* status, int device);

/* Batched grad_log_likelihood (celerite/solver.cpp:347-463 per problem; no general terms): one wave per
 * (problem, partial derivative), the forward-mode tangent recurrence of csrc/grad_kernels.hip.  Host
 * pointers in and out, one shot.  value[b] = -(y^T K^-1 y + log det K + pi log N) / 2 (the reference's
 * constant, solver.cpp:415), grad is [B][1 + 2 J_real + 4 J_comp] in the order jitter, a_real, c_real,
 * a_comp, b_comp, c_comp, d_comp (d/d jitter = 0 where jitter <= DBL_EPSILON, solver.cpp:379-389);
 * status[b] = CLR_NOT_POSITIVE_DEFINITE gives value -inf and a zero gradient (GP's quiet semantics,
 * celerite.py:285-291).  Widths 1..64. */
int clr_batch_grad_log_likelihood(int B, int N, int J_real, int J_comp, const double* jitter,
                                  const double* a_real, const double* c_real, const double* a_comp,
                                  const double* b_comp, const double* c_comp, const double* d_comp,
                                  const double* t, long t_stride, const double* diag, long diag_stride,
                                  const double* y, long y_stride, double* value, double* grad, int* status,
                                  int device);

/* The same on a plan (widths 1..8, no general terms): value and gradient of every problem at the coefficients in
 * force, PARALLEL IN n (csrc/clr_grad_core.h).  The tangent recurrences of solver.cpp:347-463 are linear in the
 * tangent state once the base trajectory is fixed, so after an evaluation by the scan every (chunk, direction) runs
 * its tangent from a zero tangent state at the chunk's scanned start state; three riders of the base trajectory per
 * chunk carry the tangent states across the chunk boundaries in a walk over the chunks per direction.  Problems the
 * scan routed to the sequential recurrence take the sequential kernel above (count: clr_batch_get_grad_fallbacks).
 * Synchronous; conventions of value / grad / status as above.  clr_batch_grad_log_likelihood uses this path for
 * widths 1..8 and N >= 512.  Chunked plans of widths 9..32 (and with general terms up to a total width of 32) run the
 * same decomposition with a wave per (chunk, direction) (csrc/wide_grad_kernels.hip); round 6: chunked plans of widths
 * 33..64 too (the riders at the padded width 64 under a workgroup of 256 threads); plans of widths 33..64 with ONE chunk
 * run the sequential tangent kernel on their resident arrays (every problem counted in clr_batch_get_grad_fallbacks);
 * above 64: CLR_UNSUPPORTED (CholeskySolver.grad_log_likelihood takes any width). */
int clr_batch_grad(clr_batch* h, double* value, double* grad, int* status);
/* clr_batch_grad plus the mean's partial: dmean[b] = d loglike_b / d mu_b = 1^T K_b^-1 r_b (0 where status[b] != 0),
 * r_b the residual of clr_batch_set_mean (y itself when no mean is set).  value, grad and status are clr_batch_grad's.
 * Narrow plans in reverse mode (the default at widths 1..8): dmean = 1/2 sum_n xbar_n, xbar the adjoint of y, summed by
 * the reverse sweep itself (one add per sample and one double per chunk) -- parallel in n.  Every other problem (forward
 * mode, wide plans, general terms, problems settled sequentially or redone forwards): one pass of the reference
 * recurrence (cholesky.h:154-178) carrying both forward substitutions, x = L^-1 r and x1 = L^-1 1:
 * dmean = sum_n x1_n x_n / D_n; one workgroup per problem, sequential in n. */
int clr_batch_grad_mean(clr_batch* h, double* value, double* grad, double* dmean, int* status);
int clr_batch_get_grad_fallbacks(const clr_batch* h, int* count);
/* The information matrix of every problem at the coefficients and on the series in force (Fisher scoring, Harvey 1989
 * section 3.4).  With z = L^-1 r the one-step-ahead innovations and D their variances,
 * loglike = -1/2 sum_n (log D_n + z_n^2 / D_n + log 2 pi), and for two directions i, j
 *     info[b][i][j] = sum_n 1/2 (d_i D_n / D_n)(d_j D_n / D_n) + (d_i z_n)(d_j z_n) / D_n :
 * first-order tangents only, a Gram matrix of 2 N numbers per direction -- positive semi-definite by construction, its
 * D half independent of the data, its expectation over data drawn from the model the Fisher information
 * 1/2 tr(K^-1 K_i K^-1 K_j).  It is NOT the Hessian of the log-likelihood (no second derivative enters).
 * info is [B][M][M] row-major, M = 1 + 2 J_real + 4 J_comp (+ 1 with mean_partial), the directions in the order of
 * clr_batch_grad's columns (jitter, a_real, c_real, a_comp, b_comp, c_comp, d_comp), then the constant mean (d D = 0,
 * d r = -1); status is [B] (may be null).  The residual, variances and amplitude-scaled series in force are what every
 * route reads, as for clr_batch_grad.  Written symmetric bit for bit.  A problem whose status is not CLR_OK (not positive
 * definite, a draw or a scale refused) gets an all-NaN matrix and its status, the others are unaffected; a problem with
 * jitter <= DBL_EPSILON gets a zero jitter row and column (the rule of the gradient's column).
 * Narrow plans (widths 1..8), celerite terms, any N >= 1, per-problem lengths included (problem b's matrix is that of its
 * first n_b samples); wide plans and general terms: CLR_UNSUPPORTED.  Parallel in n on chunked plans (the chunks'
 * tangent start states from a walk over the gradient's riders, then every chunk again for its rows, then the Gram pass
 * in slabs of a fixed size and order: no atomics, a problem's bits depend on neither the batch, the tile nor a sharding);
 * problems the scan sent to the sequential recurrence, and every problem under clr_batch_set_exact, take a sequential
 * form.  The rows of a tile of problems (16 M bytes per sample and problem) live in scratch of at most 1 GiB, the tiles
 * run one after another; clr_batch_set_information_tile: problems per tile (0: automatic).  The blocks of linear-mean,
 * noise and amplitude WEIGHTS are not covered (the mean weights' own block is clr_batch_fit_mean_weights' Gram matrix);
 * mean_partial with a linear mean or amplitudes in force: CLR_UNSUPPORTED.  The plan's results, gradient state and any
 * materialised factor are left as they were.  Synchronous. */
int clr_batch_information(clr_batch* h, int mean_partial, double* info, int* status);
int clr_batch_set_information_tile(clr_batch* h, int problems);
/* Device time of the last clr_batch_information in ms (HIP events on the plan's stream): from its evaluation to the last
 * tile's Gram pass, the tiles' downloads and host round trips in between included. */
int clr_batch_get_information_ms(const clr_batch* h, double* ms);
/* How clr_batch_grad differentiates.  mode 0 (default): REVERSE mode -- the riders pass also records w, D, x per
 * sample and the state every K steps, the adjoint at every chunk end follows from the riders in a walk backwards over
 * the chunks, and ONE reverse sweep per chunk yields all partials (cost ~4x an evaluation instead of ~20x; needs
 * 8 (J + 2) bytes per sample of HBM plus the stored states, falls back to mode 1 when that does not fit).  The sweep
 * reconstructs the states between the stored ones; the drift it measures at every stored state certifies them, and a
 * problem that drifts beyond `drift_tolerance` (default 1e-9; <= 0 keeps the current one) is redone in mode 1.
 * mode 1: FORWARD mode, one tangent per partial (the description above).  stored_state_distance: a state every K steps;
 * 0 (default) = wherever the decay accumulated since the last stored state reaches the growth budget (c T <= 3 over any
 * rebuilt stretch: a few states per chunk on dense series, one every few samples on sparse ones).
 * In reverse mode the three riders of a chunk come from the scan's own element of that chunk (one J x J solve per chunk
 * instead of ~190 FMAs per sample) whenever a gradient chunk is a scan chunk; the sweep's second certificate -- the
 * adjoint it arrives at for the chunk's first sample against the one predicted from the riders -- vouches for them.
 * mode 2 = reverse mode with the riders accumulated along the trajectory (A/B runs). */
int clr_batch_set_grad_mode(clr_batch* h, int mode, int stored_state_distance, double drift_tolerance);
/* Of the last clr_batch_grad: whether the reverse sweep ran, how many problems were redone in forward mode, the
 * largest drift among the problems the reverse sweep settled. */
int clr_batch_get_grad_info(const clr_batch* h, int* reverse_used, int* forward_reruns, double* drift_max);

/* ---- the batch axis over several GPUs (BASELINE config 4) ---------
 * Problems are independent -- every member of the reference solver is per object
 * (cholesky.h:703-706) -- so the batch axis shards embarrassingly: shard s of S owns the
 * contiguous slice clr_shard_bounds(B, S, s) and is an ordinary clr_batch plan on
 * devices[s], driven by its own host thread (stream + pinned staging per shard).  No
 * collective, no device-to-device traffic; results are concatenated on the host.
 * A device may be listed more than once (the shards then share it).
 * Results do not depend on the sharding, BIT FOR BIT, with the default settings, as long as every
 * sharding uses the same chunk count (clr_sharded_set_chunks; the automatic choice looks at a shard's
 * batch size -- what fills one GPU): every decision a plan takes from a count over its problems --
 * kernel selection, the prefix plan, the warm-started recurrence's activation and adaptation, side
 * plan or inline replay of level-1 problems and the side plan's chunk count -- is taken once, from
 * the counts over the WHOLE batch (csrc/sharded.cpp, csrc/clr_group_hooks.h). */
/* ---- kernel programs: a `terms` kernel as a fixed formula from its parameter vector to the coefficients -------------
 *
 * A tree of built-in terms (RealTerm, ComplexTerm, SHOTerm, Matern32Term, JitterTerm, sums and products of them) is
 * compiled once (celerite_amd.batch.compile_kernel) into a flat program and evaluated per draw: on the host by
 * clr_kernel_coefficients / clr_kernel_jacobian (no GPU needed), on the device by a plan (clr_batch_set_kernel,
 * clr_batch_evaluate_params, clr_batch_grad_params), where the coefficients never leave HBM.
 *
 * Encoding.  `ops` is a sequence of instructions of int words, `opcode, operands...`; `consts` holds doubles:
 *
 *    1 REAL        dst  pa pc             a = exp(pa), c = exp(pc)
 *    2 COMPLEX     dst  pa pb pc pd       a, b, c, d = exp(.)
 *    3 COMPLEX_B0  dst  pa pc pd          the same with b = 0
 *    4 SHO_OVER    dst0 dst1 pS pQ pw     SHOTerm with Q <  1/2: two real terms
 *    5 SHO_UNDER   dst  pS pQ pw          SHOTerm with Q >= 1/2: one complex term
 *    6 MATERN32    dst  ps pr keps        Matern32Term, eps = consts[keps]
 *    7 JITTER      ps                     jitter += exp(2 ps)
 *    8 MUL_RR      dst  r1 r2             real x real:       (a1 a2, c1 + c2)
 *    9 MUL_RC      dst  r1 c2             real x complex:    (a1 a2, a1 b2, c1 + c2, d2)
 *   10 MUL_CC      dstm dstp c1 c2        complex x complex: the two terms at d1 - d2 and d1 + d2
 *
 * A parameter operand p* >= 0 is an index into the draw's parameter vector (the kernel's unfrozen parameters, in
 * get_parameter_vector() order); p* < 0 is the constant consts[-(p + 1)] (a frozen parameter).  A destination dst >= 0
 * is the index of a real (complex) term in the output blocks a_real, c_real (a_comp, b_comp, c_comp, d_comp); dst < 0
 * is the temporary real (complex) term -(dst + 1), at most 16 of each kind.  The factors r*, c* of a product are
 * temporaries written by an earlier instruction, given by their index >= 0.  An SHO instruction fixes its regime: a
 * draw on the other side of Q = 1/2 is refused for that draw (status[b]), never evaluated to another shape.
 *
 * clr_kernel_create validates the program -- known opcodes, every operand in range, temporaries written once and
 * before they are read, every output term written exactly once -- and refuses it with CLR_INVALID_ARGUMENT otherwise
 * (at most 2048 words, 256 constants, 256 parameters). */
typedef struct clr_kernel clr_kernel;
int clr_kernel_create(int n_ops, const int* ops, int n_consts, const double* consts, int n_params, int J_real,
                      int J_comp, clr_kernel** kernel);
void clr_kernel_destroy(clr_kernel* kernel);
int clr_kernel_get_shape(const clr_kernel* kernel, int* n_params, int* J_real, int* J_comp);
/* The coefficient tables of B draws: params[B][n_params] -> a_real, c_real [B][J_real], a_comp .. d_comp [B][J_comp],
 * jitter[B] (what clr_batch_set_coefficients takes).  status[b] = CLR_INVALID_ARGUMENT and a row of NaN for a draw the
 * program refuses: a non-finite parameter or coefficient, an SHO term in the other regime.  The other rows are not
 * affected.  status and jitter may be NULL. */
int clr_kernel_coefficients(const clr_kernel* kernel, int B, const double* params, double* a_real, double* c_real,
                            double* a_comp, double* b_comp, double* c_comp, double* d_comp, double* jitter,
                            int* status);
/* The Jacobians of the same formulas, evaluated on forward dual numbers: jac[B][n_params][2 J_real + 4 J_comp] with the
 * coefficients in the column order of the batched gradient (a_real | c_real | a_comp | b_comp | c_comp | d_comp) and
 * jitter_jac[B][n_params].  Either may be NULL. */
int clr_kernel_jacobian(const clr_kernel* kernel, int B, const double* params, double* jac, double* jitter_jac,
                        int* status);
/* A plan evaluated straight from kernel parameters.  clr_batch_set_kernel copies the program to the plan's device
 * (CLR_DIMENSION_MISMATCH when its J_real, J_comp are not the plan's; NULL removes it).  clr_batch_set_parameters is
 * clr_batch_set_coefficients for params[B][n_params]: kernel_program_eval_kernel forms the coefficients in the plan's
 * resident block, and the statistics the kernel selection looks at come back from the same kernel in one small
 * transfer -- the routes and the warm-start decision are the ones clr_batch_set_coefficients takes for the same
 * coefficients.  A draw the program refuses is given stand-in coefficients on the device (every term exp(-tau), no
 * jitter), so that it disturbs no other problem, and is reported by clr_batch_evaluate_params / _grad_params /
 * clr_batch_get_parameter_status with CLR_INVALID_ARGUMENT and NaN results.
 * clr_batch_evaluate_params: [clr_batch_set_mean +] clr_batch_set_parameters + clr_batch_enqueue + clr_batch_get_results
 * in one call (mean == NULL: the mean in force stays).
 * clr_batch_grad_params: after it, clr_batch_grad (with_mean: clr_batch_grad_mean) chained to the parameters on the
 * device: grad_params[B][n_params (+ 1)] = jitter_jac grad[0] + sum_c jac[.][c] grad[1 + c], the mean's partial last.
 * Needs coefficients formed by clr_batch_set_parameters (CLR_NOT_COMPUTED otherwise).
 * clr_batch_get_coefficients reads the resident block back (any pointer may be NULL), however it was set. */
int clr_batch_set_kernel(clr_batch* h, const clr_kernel* kernel);
int clr_batch_set_parameters(clr_batch* h, const double* params);
int clr_batch_get_parameter_status(const clr_batch* h, int* status);
int clr_batch_evaluate_params(clr_batch* h, const double* params, const double* mean, long mean_stride,
                              double* loglike, double* logdet, double* quad, int* status);
int clr_batch_grad_params(clr_batch* h, double* value, double* grad_params, int* status, int with_mean);
int clr_batch_get_coefficients(clr_batch* h, double* jitter, double* a_real, double* c_real, double* a_comp,
                               double* b_comp, double* c_comp, double* d_comp);

typedef struct clr_sharded clr_sharded;

/* [lo, hi) of `shard` when `total` problems are cut into `nshards` contiguous slices
 * (the first total % nshards slices are one longer).  Pure host arithmetic. */
int clr_shard_bounds(int total, int nshards, int shard, int* lo, int* hi);
/* nshards = number of entries of `devices` (clamped to B).  NULL on failure:
 * clr_sharded_last_error() says why (no device, bad index, allocation). */
clr_sharded* clr_sharded_create(int B, int N, int J_real, int J_comp, const int* devices, int nshards);
void clr_sharded_destroy(clr_sharded* h);
const char* clr_sharded_last_error(void);
int clr_sharded_num_shards(const clr_sharded* h);
int clr_sharded_get_shard(const clr_sharded* h, int shard, int* device, int* lo, int* hi);
/* As the clr_batch_* entries of the same name, over the whole batch (host arrays of B
 * problems; every shard takes its slice).  The calls return when every shard has. */
int clr_sharded_set_chunks(clr_sharded* h, int nchunk);
int clr_sharded_get_chunks(const clr_sharded* h, int shard, int* nchunk, int* chunk_len);
/* (the automatic choice of the summarize kernel is resolved once for the whole batch: the shards are handed the
 * batch-wide maxima of the series and coefficients, so the choice does not depend on the sharding) */
int clr_sharded_set_summarize_mode(clr_sharded* h, int mode);
/* clr_batch_set_warm_start on every shard.  The warm-started recurrence is switched on when at least half of the
 * problems OF THE BATCH are eligible and lengthens its warm-ups by the fallbacks OF THE BATCH (the shards' counts are
 * added up between the two halves of every evaluation's resolve): the same route under any sharding.  Its chunking
 * follows the chunk count when that is pinned, else the shard's batch size. */
int clr_sharded_set_warm_start(clr_sharded* h, int mode, int forced_warmup);
/* clr_batch_set_rescue on every shard.  Side plan or inline replay, and the side plan's chunk count, follow the number
 * of route-1 problems of the WHOLE batch: bit-identical under any sharding (round 5: per shard).
 * clr_sharded_get_rescue: problems of the last fetched evaluation that took the checked route outside the main pass,
 * summed over the shards. */
int clr_sharded_set_rescue(clr_sharded* h, int mode);
int clr_sharded_get_rescue(const clr_sharded* h, int* last_count);
/* clr_batch_set_certificate + clr_batch_set_certificate_gamma on every shard (the routing bounds of ill-conditioned
 * problems; a negative max_gamma / max_gamma_times_error leaves the gamma bounds as they are). */
int clr_sharded_set_certificate(clr_sharded* h, double max_gamma_over_mu, double max_residual, double max_gamma,
                                double max_gamma_times_error);
/* The summarize kernel all shards will run (clr_batch_get_summarize_kernel; -1 if they disagree). */
int clr_sharded_get_summarize_kernel(const clr_sharded* h, int* kind);
/* clr_batch_get_series_order / clr_batch_clear_series over all shards (the smallest step of the whole batch) */
int clr_sharded_get_series_order(const clr_sharded* h, double* dtmin);
int clr_sharded_clear_series(clr_sharded* h);
int clr_sharded_set_series(clr_sharded* h, const double* t, long t_stride, const double* diag,
                           long diag_stride, const double* y, long y_stride);
/* clr_batch_set_series_ragged / clr_batch_get_lengths over all shards: `lengths` is [B] for the whole batch, each shard
 * takes its slice.  Whether lengths are in force is decided once for the batch (a shard whose own lengths all equal N is
 * still a plan with lengths then), so results are the same bits under any sharding. */
int clr_sharded_set_series_ragged(clr_sharded* h, const double* t, long t_stride, const double* diag, long diag_stride,
                                  const double* y, long y_stride, const int* lengths);
int clr_sharded_get_lengths(const clr_sharded* h, int* lengths);
int clr_sharded_set_coefficients(clr_sharded* h, const double* jitter, const double* a_real,
                                 const double* c_real, const double* a_comp, const double* b_comp,
                                 const double* c_comp, const double* d_comp);
int clr_sharded_enqueue(clr_sharded* h);
int clr_sharded_synchronize(clr_sharded* h);
int clr_sharded_get_results(clr_sharded* h, double* loglike, double* logdet, double* quad, int* status);
/* clr_batch_grad on every shard concurrently (coefficients in force: clr_sharded_set_coefficients); grad is
 * [B][1 + 2 J_real + 4 J_comp]. */
int clr_sharded_grad(clr_sharded* h, double* value, double* grad, int* status);
/* clr_batch_information on every shard concurrently: info is [B][M][M], M = 1 + 2 J_real + 4 J_comp (+ 1 with
 * mean_partial); clr_batch_set_information_tile on every shard. */
int clr_sharded_information(clr_sharded* h, int mean_partial, double* info, int* status);
int clr_sharded_set_information_tile(clr_sharded* h, int problems);
/* One optimiser / MCMC evaluation: new coefficients in, B log-likelihoods out
 * (set_coefficients + enqueue + get_results on every shard concurrently). */
int clr_sharded_evaluate(clr_sharded* h, const double* jitter, const double* a_real, const double* c_real,
                         const double* a_comp, const double* b_comp, const double* c_comp,
                         const double* d_comp, double* loglike, double* logdet, double* quad, int* status);
/* clr_batch_set_mean / _evaluate_mean / _grad_mean over the whole batch: every shard takes its slice of mu (mu_stride
 * 1) or the one value (0); an invalid mean leaves every shard unchanged.  dmean is [B]. */
int clr_sharded_set_mean(clr_sharded* h, const double* mu, long mu_stride);
int clr_sharded_evaluate_mean(clr_sharded* h, const double* mean, long mean_stride, const double* jitter,
                              const double* a_real, const double* c_real, const double* a_comp, const double* b_comp,
                              const double* c_comp, const double* d_comp, double* loglike, double* logdet,
                              double* quad, int* status);
int clr_sharded_grad_mean(clr_sharded* h, double* value, double* grad, double* dmean, int* status);
/* clr_batch_set_mean_basis / _set_mean_weights / _grad_mean_weights over the whole batch: every shard takes its slice of
 * phi (phi_stride K * N) or the one basis (0), of w[B][K] and of dw[B][K]; an invalid basis or weight leaves every shard
 * unchanged.  The results are those of the unsharded plan, bit for bit (given one chunk count, as above). */
int clr_sharded_set_mean_basis(clr_sharded* h, int K, const double* phi, long phi_stride);
int clr_sharded_set_mean_weights(clr_sharded* h, const double* w);
int clr_sharded_grad_mean_weights(clr_sharded* h, double* dw, int* status);
/* The linear noise model over the shards (clr_batch_set_noise_basis / _set_noise_weights / _grad_noise_weights): every
 * shard takes its slice of psi (psi_stride K * N) or the one basis (0), of s[B][K] and of ds[B][K]; an invalid basis or
 * weight leaves every shard unchanged.  The results are those of the unsharded plan, bit for bit. */
int clr_sharded_set_noise_basis(clr_sharded* h, int K, const double* psi, long psi_stride);
int clr_sharded_set_noise_weights(clr_sharded* h, const double* s);
int clr_sharded_grad_noise_weights(clr_sharded* h, double* ds, int* status);
int clr_sharded_get_noise_project_ms(const clr_sharded* h, double* device_ms);  /* the largest over the shards */
/* The amplitude model over the shards (clr_batch_set_amplitude_basis / _set_amplitudes / _get_log_amplitude_sum /
 * _grad_amplitudes): every shard takes its slice of gamma (gamma_stride K * N) or the one basis (0), of a[B][K], L[B] and
 * da[B][K]; an invalid basis or amplitude leaves every shard unchanged.  The results are those of the unsharded plan, bit
 * for bit. */
int clr_sharded_set_amplitude_basis(clr_sharded* h, int K, const double* gamma, long gamma_stride);
int clr_sharded_set_amplitudes(clr_sharded* h, const double* a);
int clr_sharded_get_log_amplitude_sum(clr_sharded* h, double* L);
int clr_sharded_grad_amplitudes(clr_sharded* h, double* da, int* status);
int clr_sharded_get_amplitude_project_ms(const clr_sharded* h, double* device_ms);  /* the largest over the shards */
/* clr_batch_fit_mean_weights over the whole batch: every shard fits its slice; the same bits as the unsharded plan */
int clr_sharded_fit_mean_weights(clr_sharded* h, double min_pivot, double* w_hat, double* cov, double* gram,
                                 double* quad_profiled, double* logdet_gram, int* status);
/* clr_batch_set_kernel / _evaluate_params / _grad_params / _get_coefficients over the whole batch: every shard forms the
 * coefficients of its slice of params[B][n_params] on its own device; the selection bounds are taken over the batch. */
int clr_sharded_set_kernel(clr_sharded* h, const clr_kernel* kernel);
int clr_sharded_evaluate_params(clr_sharded* h, const double* params, const double* mean, long mean_stride,
                                double* loglike, double* logdet, double* quad, int* status);
int clr_sharded_grad_params(clr_sharded* h, double* value, double* grad_params, int* status, int with_mean);
int clr_sharded_get_coefficients(clr_sharded* h, double* jitter, double* a_real, double* c_real, double* a_comp,
                                 double* b_comp, double* c_comp, double* d_comp);
/* The consumers of the factor on a sharded batch (GP.apply_inverse / .sample / .predict for B problems over several
 * GPUs): clr_sharded_materialize runs clr_batch_enqueue(plan, 1) on every shard, settles the evaluation with the
 * batch-wide counts (results as clr_sharded_get_results; any pointer may be NULL) and leaves every shard's factor in
 * its HBM; clr_sharded_solve / _dot_L / _dot / _predict / _predict_var / _predict_var_recurrence / _leave_one_out /
 * _one_step_ahead / _forecast / _predict_terms / _predict_cov / _sample_conditional are clr_batch_solve / _dot_L / _dot / _predict / _predict_var / _predict_var_recurrence /
 * _leave_one_out / _one_step_ahead / _forecast / _predict_terms / _predict_cov / _sample_conditional on every shard concurrently,
 * each on its contiguous slice of the host arrays ([B][nrhs][N]; xs [B][M] or shared with xs_stride = 0).  No
 * collective: every problem's state is its own (cholesky.h:703-706). */
int clr_sharded_materialize(clr_sharded* h, double* loglike, double* logdet, double* quad, int* status);
int clr_sharded_solve(clr_sharded* h, int nrhs, const double* b, double* x);
int clr_sharded_dot_L(clr_sharded* h, int nrhs, const double* z, double* y);
int clr_sharded_dot(clr_sharded* h, int nrhs, const double* z, double* y);
int clr_sharded_predict(clr_sharded* h, int M, const double* xs, long xs_stride, double* pred);
int clr_sharded_predict_var(clr_sharded* h, int M, const double* xs, long xs_stride, double* var);
int clr_sharded_predict_var_recurrence(clr_sharded* h, int M, const double* xs, long xs_stride, double* var);
int clr_sharded_leave_one_out(clr_sharded* h, double* kinv_diag, double* alpha, double* loo_logpdf, int* status);
int clr_sharded_one_step_ahead(clr_sharded* h, int nrhs, const double* b, double* innovation, double* variance, int* status);
int clr_sharded_forecast(clr_sharded* h, int M, const double* xs, long xs_stride, double* mean, double* var);
int clr_sharded_predict_terms(clr_sharded* h, int M, const double* xs, long xs_stride, int G, const unsigned char* groups,
                              double* mean, double* var);
int clr_sharded_predict_cov(clr_sharded* h, int M, const double* xs, long xs_stride, double* cov);
int clr_sharded_sample_conditional(clr_sharded* h, int M, const double* xs, long xs_stride, int size, const double* normals,
                                   double regularize, double min_pivot, double* draws, int* status);
int clr_sharded_set_conditional_tile(clr_sharded* h, int problems);
/* clr_batch_periodogram, every shard its slice of omega (when per problem) and of the outputs: the unsharded plan's bits. */
int clr_sharded_periodogram(clr_sharded* h, int F, const double* omega, long omega_stride, double t_ref, int offset,
                            double min_pivot, double* power, double* coef, double* cov, double* gram, int* status);
int clr_sharded_set_periodogram_tile(clr_sharded* h, int frequencies);
int clr_sharded_get_periodogram_ms(const clr_sharded* h, double* device_ms); /* the largest over the shards */
/* `steps` back-to-back evaluations on every shard concurrently (HIP events per shard);
 * shard_ms[s] = that shard's first-to-last event time. */
int clr_sharded_run_timed(clr_sharded* h, int steps, double* shard_ms);
/* clr_batch_log_likelihood over `ndevices` shards (create + set + evaluate + destroy). */
int clr_batch_log_likelihood_sharded(int B, int N, int J_real, int J_comp, const double* jitter,
                                     const double* a_real, const double* c_real, const double* a_comp,
                                     const double* b_comp, const double* c_comp, const double* d_comp,
                                     const double* t, long t_stride, const double* diag, long diag_stride,
                                     const double* y, long y_stride, double* loglike, double* logdet,
                                     double* quad, int* status, const int* devices, int ndevices);

/* ---- celerite::carma::CARMASolver (cpp/include/celerite/carma.h; solver.cpp:200-235) ----
 * The reference's comparison solver: a CARMA(p, q) process in carma_pack's parameterisation, its log-likelihood by
 * a Kalman filter, and the conversion to celerite coefficients (tests/test_celerite.py:22-42 checks that the two
 * likelihoods agree).  The model algebra runs on the host at creation; the filter -- sequential in n -- runs as one
 * wave on the device.  Errors: q >= p -> CLR_DIMENSION_MISMATCH (carma.h:59); p > CLR_CARMA_MAX_ORDER ->
 * CLR_UNSUPPORTED; a negative predicted variance -> CLR_CARMA_INSTABILITY (carma.h:185-186). */
typedef struct clr_carma clr_carma;
/* CARMASolver(log_sigma, arparams[p], maparams[q]), carma.h:54-72.  NULL on error (see clr_last_error). */
clr_carma* clr_carma_create(double log_sigma, int p, const double* arparams, int q, const double* maparams,
                            int* status);
void clr_carma_destroy(clr_carma* h);
/* CARMASolver::log_likelihood(t, y, yerr), carma.h:221-239; host pointers, copied in. */
int clr_carma_log_likelihood(clr_carma* h, int n_t, const double* t, int n_y, const double* y, int n_yerr,
                             const double* yerr, double* out);
/* CARMASolver::get_celerite_coeffs, carma.h:74-139.  Counts first (pass NULL arrays), then the values: a_real,
 * c_real [n_real]; a_comp, b_comp, c_comp, d_comp [n_comp].  No device work. */
int clr_carma_get_celerite_coeffs(const clr_carma* h, int* n_real, int* n_comp, double* a_real, double* c_real,
                                  double* a_comp, double* b_comp, double* c_comp, double* d_comp);

/* ---- O(J) host helpers the Python layer imports (celerite/terms.py:18) --------
 * Plain host C++ (no device work): cpp/include/celerite/utils.h:106-163,27-104. */
double clr_kernel_value(int J_real, const double* a_real, const double* c_real,
                        int J_comp, const double* a_comp, const double* b_comp,
                        const double* c_comp, const double* d_comp, double tau);
double clr_psd_value(int J_real, const double* a_real, const double* c_real,
                     int J_comp, const double* a_comp, const double* b_comp,
                     const double* c_comp, const double* d_comp, double omega);
int clr_check_coefficients(int n_a_real, const double* a_real, int n_c_real, const double* c_real,
                           int n_a_comp, const double* a_comp, int n_b_comp, const double* b_comp,
                           int n_c_comp, const double* c_comp, int n_d_comp, const double* d_comp);

#ifdef __cplusplus
}
#endif
#endif /* CELERITE_HIP_H */
