// celerite_amd/csrc/api_internal.h -- shared by the translation units of the C ABI (include/celerite_hip.h):
//   api_misc.hip    library / device entries, the CARMA handle
//   api_solver.hip  clr_solver_*: the object API (one problem per handle)
//   api_batch.hip   clr_batch_*: plans, HBM residency, path selection, evaluation, results
//   api_batch_consumers.hip  clr_batch_*: the consumers of a plan's factor and coefficients (solve .. grad_noise_weights)
//   api_grad.hip    clr_batch_grad*: the gradient entry points
//   api_information.hip  clr_batch_information: the information matrix of every problem
//   api_kernels.hip the small kernels the plans launch themselves (finalize, relayouts, factor de-interleave)
// Here: error reporting, the device buffer types, the two handle structs, and the functions that turn a plan's state into
// kernel parameters (used by the evaluation and by the gradient).  Everything is internal to libcelerite_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/celerite_hip.h"
#include "../../include/celerite_hip_debug.h"
#include "clr_batch_kernels.h"
#include "clr_carma.h"
#include "clr_generic_kernels.h"
#include "clr_series_io.h"
#include "clr_small.h"
#include "clr_wide.h"
#include "clr_options.h"
#include "clr_handles.h"
#include "clr_kernel.h"

// the last error message of the calling thread (clr_last_error) and its current device: ONE object per thread for the
// whole library (defined in api_misc.hip)
extern thread_local std::string clr_api_last_error;
extern thread_local int clr_api_device;
#define g_last_error clr_api_last_error
#define g_device clr_api_device

namespace {


int fail(int status, const std::string& msg) {
  g_last_error = msg;
  return status;
}

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(CLR_HIP_ERROR, std::string(#expr) + ": " + hipGetErrorString(e_));   \
  } while (0)

int visible_gfx950() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  int ok = 0;
  for (int d = 0; d < n; ++d) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d) == hipSuccess &&
        strncmp(prop.gcnArchName, "gfx950", 6) == 0)
      ++ok;
  }
  return ok;
}

int require_device(int device) {
  static int count = -1;
  if (count < 0) count = visible_gfx950();
  if (count <= 0)
    return fail(CLR_NO_DEVICE,
                "no gfx950 (MI355X) device is visible; libcelerite_hip has no CPU path");
  if (device < 0 || device >= count) return fail(CLR_INVALID_ARGUMENT, "bad device index");
  HIP_TRY(hipSetDevice(device));
  return CLR_OK;
}

// Grow-only device arrays (clr_handles.h): freed with the plan, solver or scope that holds them.
using DevBuf = clr::Buffer<double>;
template <class T>
using DevArray = clr::Buffer<T>;

// returns `code` once `s` has drained (early returns of a function whose kernels may still use its local buffers)
int synced(hipStream_t s, int code) {
  (void)hipStreamSynchronize(s);
  return code;
}

int upload(DevBuf& buf, const double* host, size_t n, hipStream_t s) {
  int st = buf.reserve(n);
  if (st != CLR_OK) return st;
  if (n) HIP_TRY(hipMemcpyAsync(buf.p, host, n * sizeof(double), hipMemcpyHostToDevice, s));
  return CLR_OK;
}

// max |t| over a series (NaN sticks).  A full O(N) pass, not the two ends: the C ABI does
// not require sorted times (GP.compute(check_sorted=False) reaches it unsorted), and the
// fast sincos is only valid for |d t| < CLR_FAST_TRIG_LIMIT at EVERY sample.
double max_abs(const double* x, long n) {
  double m = 0.0;
  for (long i = 0; i < n; ++i) {
    const double a = fabs(x[i]);
    if (!(a <= m)) m = a;
  }
  return m;
}

// Chunk count for the scan on `B` problems of `N` samples of width `J`.
int auto_chunks(int B, int N, int J, bool with_replay = false) {
  if (N < 128) return 1;
  // Cost model (measured on MI355X): the big kernels run
  // ceil(B * ceil(nchunk / 64) / 1024) rounds of waves (one per SIMD) over L = N / nchunk
  // steps at ~2.4 us per step at width 8 (3.3 us when the replay pass runs too), less at
  // smaller widths; the prefix phase costs what its plan says (clr_core.h: plan_prefix --
  // a walk over the chunks, or a multi-level prefix when the chip has room for it).  Many
  // problems want exactly one wave per SIMD; a single long series wants many short chunks.
  const double w = (0.25 + 0.75 * J * J / 64.0);
  const double c_step = (with_replay ? 3.3e-6 : 2.4e-6) * w;
  const long max_by_len = std::max<long>(1, N / 16);
  auto cost = [&](long nc) {
    long L = (N + nc - 1) / nc;
    if (nc > 1 && L > 8) L = (L + 7) & ~7L;
    const long waves = (long)B * ((nc + 63) / 64);
    const long rounds = (waves + 1023) / 1024;
    return rounds * L * c_step + clr::plan_prefix((int)nc, -1, 0, B, J).time_us * 1e-6 + (nc > 1 ? 15e-6 : 0.0);
  };
  long best = 1;
  double best_cost = cost(1);
  auto consider = [&](long nc) {
    if (nc < 1 || nc > max_by_len) return;
    const double c = cost(nc);
    if (c < best_cost) { best_cost = c; best = nc; }
  };
  for (long nc : {2L, 3L, 4L, 6L, 8L, 12L, 16L, 24L, 32L, 48L}) consider(nc);
  for (long nc = 64; nc <= max_by_len && nc <= 65536; nc += 64) consider(nc);
  return (int)best;
}

}  // namespace

/* ======================================================================== */
// a plan owned by another handle (a side plan, the solver's gradient plan)
struct BatchDeleter { void operator()(clr_batch* b) const { clr_batch_destroy(b); } };
using BatchPtr = std::unique_ptr<clr_batch, BatchDeleter>;

// The handles own their device memory, pinned memory, streams and events (clr_handles.h): members are freed in reverse
// order of declaration after the destructor's body, so each stream is declared before everything queued on it.
struct clr_solver {
  int device = 0;
  clr::Stream stream;
  bool have_stream = false;
  // grad_log_likelihood parallel in n (widths 1..8, no general terms): a one-problem plan kept between calls, and
  // the series it holds (an optimiser calls with the same t, diag, y and new coefficients)
  BatchPtr grad_plan;
  int grad_N = 0, grad_JR = -1, grad_JC = -1;
  bool grad_wide = false, grad_had_general = false;
  int grad_route = -1;                  // the last grad_log_likelihood's route (clr_solver_debug_grad_route)
  std::vector<double> grad_series;
  int computed = 0, N = 0, J = 0;
  double log_det = 0.0;
  int J_real = 0, J_comp = 0, J_general = 0;
  DevBuf phi, u, W, D;                  // the factor (reference layout)
  DevBuf coeffs;                        // a_real c_real a_comp b_comp c_comp d_comp
  DevBuf t, U, V;                       // inputs kept for predict / dot
  DevBuf scratch, scratch2, scalars;    // right-hand sides, results
  DevBuf dot_buf[11];                            // clr_solver_dot's own buffers (it must not disturb a computed factor)
  DevBuf pred_buf[2];                            // clr_solver_predict: the prediction points, the predictions
  DevBuf ws_elems, ws_starts, ws_part, ws_cond;  // scan workspace
  DevBuf ws_lvl_elems, ws_lvl_starts;            // upper levels of the multi-level prefix; level buffers of the wide parallel prefix
  DevBuf gradbuf;                       // grad_log_likelihood staging
  DevBuf gradws;                        // ... above width 64: S and dS of a round of directions (grad_any_kernels.hip)
  // The factor's chunk heads (clr_batch_kernels.h, BatchParams::ends): compute() writes the factor from the SCANNED
  // start states, whose rounding shows in W and D for the ~32 samples the recurrence needs to forget it -- with the ~50
  // to 100-sample chunks of one long series that is most of the factor (N = 1e5, width 8: W 1.1e-10, solve 1.8e-10 of
  // the oracle, profiles/r06n_solver_factor_error.txt).  log_determinant and the hinted dot_solve do not depend on it,
  // so GP.log_likelihood pays nothing: the FIRST call that reads the factor (solve, dot_solve of another vector, dot_L,
  // predict, __getstate__) replays every chunk once more from the state the previous chunk's replay reached.
  DevBuf keep_diag, keep_jitter, ws_ends;  // compute's diag / jitter (kept for that pass), the chunks' end states
  clr::BatchParams refine_P;
  int refine_pending = 0;               // 0 nothing to do, 1 narrow plan kernels, 2 wide kernels
  // chunk maps of the affine scans over the stored factor at widths above 64 (bigsweep_kernels.hip): per direction, built by
  // the first sweep that needs them, dropped with the factor
  DevBuf big_maps[2];
  bool big_maps_valid[2] = {false, false};
  // the route the last compute took through the chunked flow (clr_solver_debug_route): device pointers into the workspace
  const int* route_level = nullptr;
  const double* route_cond = nullptr;
  int route_nchunk = 0;
  std::vector<double> host_coeffs;      // staging of the last upload (kept alive: async copy)
  // clr_solver_hint_rhs: the right-hand side the caller is about to pass to dot_solve; the next compute
  // folds b^T K^-1 b into its own pass over the series and dot_solve returns it for that very vector
  std::vector<double> host_rhs;
  DevBuf rhs;
  bool rhs_hint = false, have_quad = false;
  bool coeffs_lazy = false;             // host_coeffs not yet on the device (the one-launch route passes them as arguments)
  double cached_quad = 0.0;
  DevArray<int> ws_flags;
  DevArray<int> d_status;
  // pinned staging of compute's inputs and results: copies from pageable memory cost ~15 us of host time each
  // (six of them per GP.log_likelihood on a short series: profiles/r02zzz_config0_hip_trace.txt)
  clr::PinnedBuffer<double> pin;
  size_t pin_off = 0;

  ~clr_solver() {
    grad_plan.reset();
    if (have_stream) {
      (void)hipSetDevice(device);
      (void)hipStreamSynchronize(stream.get());
    }
  }
};

// A chunk-interleaved copy of a plan's three series arrays, and whether it still matches them.  Each of a plan's three
// has ONE function that builds it (build_scan_series; api_batch.hip: warm_copy, small_params) and that alone marks it
// fresh, exactly when it has queued the rebuild; only the cause functions below the plan (series_replaced, ...) mark it stale.
struct SeriesCopy {
  DevBuf T, D, Y;
  bool stale = true;     // the arrays, or the chunking the copy follows, changed since it was built (or it never was)
  bool y_stale = false;  // the scan's copy only: the residual y alone changed -- Y alone is rebuilt
  bool d_stale = false;  // ... the variances alone changed (variance_replaced) -- D alone is rebuilt
};

struct clr_batch {
  int device = 0;
  clr::Stream stream;
  int B = 0, N = 0, J_real = 0, J_comp = 0, J = 0;
  int nchunk = 1, L = 0;
  int L0 = 0;                      // wide plans: samples of the first chunk when it is longer than L (0: uniform)
  int general_route = -1;          // plans with general terms: -1 the wide kernels when the total width allows, 1 the any-width sequential kernel
  int small_mode = -1;             // one-launch evaluation of short narrow problems: -1 auto, 0 off, 1 whenever supported
  // general terms through the wide kernels (widths J + J_general <= 64): their own chunking and workspace
  int gen_nchunk = 0, gen_L = 0, gen_L0 = 0;
  DevBuf gen_elems, gen_starts, gen_part, gen_cond, gen_scan;
  size_t gen_scan_ws_doubles = 0, scan_ws_doubles = 0;  // workspace of the wide parallel prefix (0: sequential walk)
  DevArray<int> gen_flags;
  bool pipeline_pinned = false;    // the caller tuned the scan pipeline (chunks, prefix, summarize kernel, layout, certificate): auto small mode stays out
  double wide_first_ratio64 = 1.45;  // ... at widths 33..64 (2.3 before the summarize split the features' work between a row's lanes: profiles/r05k_wide_feature_batch.txt)
  double wide_first_ratio = 1.25;  // wide plans: cost of a chunk with riders / cost of the riderless first chunk (1.1-1.25 within 2 %: profiles/r04c, r04p)
  const clr::BatchLaunchers* launch = nullptr;
  DevBuf coeffs, t, diag, y;          // coefficients (| jitter at the end); series in the API's row-major layout
  clr::PinnedBuffer<double> pin;      // pinned host staging: coefficient uploads, result downloads
  SeriesCopy scan_series;             // the chunk-interleaved copy the scan's kernels read (scan_reads_copy)
  long t_stride = 0, diag_stride = 0, y_stride = 0;
  // clr_batch_set_series_ragged: problem b holds host_len[b] <= N samples.  `ragged` says that lengths are in force: the
  // rows of t, diag, y (and of the residual) are padded in place past each problem's length, every narrow kernel takes
  // its n_b from len_dev (BatchParams::len), the warm-started and the one-launch routes stay off, and the materialising
  // runs with every consumer of their factor are refused.  A slice of a larger batch is ragged when the WHOLE batch is
  // (clr_group::set_series_lengths), whatever its own lengths: the route decisions must not depend on the sharding.
  bool ragged = false;
  std::vector<int> host_len;          // [B]; empty: uniform
  DevArray<int> len_dev;              // [B]
  // clr_batch_set_mean: with a mean in force `y` holds the residual y - mu that every route reads, and `y_src` the
  // caller's series as uploaded (y_src_stride: its stride)
  bool have_mean = false;
  long mean_stride = 0;               // 1: one value per problem, 0: one value for all
  std::vector<double> host_mean;      // [B] or [1]
  DevBuf mean_dev, y_src, mean_out;   // the mean on the device; the caller's y; clr_batch_grad_mean's partials [B]
  long y_src_stride = 0;
  // clr_batch_set_mean_basis / _set_mean_weights: a mean linear in its parameters, sum_k w[b][k] Phi_k (mean_K > 0; never
  // together with have_mean).  `y` holds the residual and `y_src` the caller's series as for the constant mean; the
  // weights go up through mean_pin into mean_dev; the basis stays resident
  int mean_K = 0;
  long basis_stride = 0;              // 0: one basis [K][N] for all problems, K * N: [B][K][N]
  std::vector<double> host_weights;   // [B][K] (zero until clr_batch_set_mean_weights)
  DevBuf basis_dev, proj_part, proj_out;  // the basis; clr_batch_grad_mean_weights' slab partials and its result [B][K]
  clr::Event proj_ev[2];              // ... its two timing events around the projection's kernels
  double project_device_ms = 0.0;     // ... and their difference at the last call
  // clr_batch_fit_mean_weights: the Gram pass' slab partials, the bordered Gram matrices [B][K+1][K+1], the weights in
  // force, the small solve's results (clr_bmean_kernels.h: gram_solve_out_doubles per problem), statuses and workspace
  DevBuf fit_part, fit_gram, fit_w0, fit_out, fit_work;
  DevArray<int> fit_status;
  std::vector<clr::Event> fit_ev;     // ... its timing events: one in front, two per tile of right-hand sides, two behind
  int mean_fit_tile = 0;              // clr_batch_set_mean_fit_tile: right-hand sides per tile (0: automatic)
  double fit_solve_ms = 0.0, fit_gram_ms = 0.0, fit_small_ms = 0.0;  // device time of the last call's three parts
  // clr_batch_set_kernel / _set_parameters: the program (host copy and in HBM), the last parameter rows with the
  // evaluation kernel's statistics block behind them, the chain rule's staging (grad | dmean | result)
  bool have_kernel = false;
  bool kp_in_force = false;           // the coefficients in force were formed from kp_params by the program
  clr_kernel kp;
  DevArray<int> kp_ops;
  DevBuf kp_consts, kp_params, kp_grad;
  std::vector<char> kp_refused;       // [B] draws of the last clr_batch_set_parameters the program refused
  clr::PinnedBuffer<double> mean_pin; // pinned staging of the mean's upload ...
  clr::Event mean_ev;                 // ... recorded behind it: the staging is rewritten only once the copy has run
  // clr_batch_set_noise_basis / _set_noise_weights: a noise model linear in its parameters, diag_eff = diag + sum_k s[b][k]
  // Psi_k (noise_K > 0).  `diag` holds diag_eff, which every route reads, and `diag_src` the caller's diagonal as uploaded
  // (diag_src_stride: its stride) -- the y / y_src pattern of the mean; the weights go up through noise_pin into
  // noise_dev; the basis stays resident.  clr_batch_grad_noise_weights shares proj_part / proj_out / proj_ev with the mean's
  // projection (one call at a time uses them)
  int noise_K = 0;
  long noise_stride = 0;              // 0: one basis [K][N] for all problems, K * N: [B][K][N]
  std::vector<double> host_noise;     // [B][K] (zero until clr_batch_set_noise_weights)
  DevBuf noise_basis, noise_dev, diag_src;
  long diag_src_stride = 0;
  clr::PinnedBuffer<double> noise_pin;
  clr::Event noise_ev;
  double noise_project_ms = 0.0;      // device time of the last clr_batch_grad_noise_weights' projection
  bool variance_changed = false;      // the variances in `diag` were replaced since the last materialising run (its factor is another matrix')
  // clr_batch_set_amplitude_basis / _set_amplitudes: a per-sample amplitude, s[b][n] = sum_k a[b][k] Gamma_k[b][n] (amp_K > 0:
  // a basis is set; amp_active: amplitudes are in force).  With amplitudes in force `y` holds r / s and `diag` holds d / (s
  // * s), r and d the residual and the variances the plan would otherwise read: the caller's arrays stay in y_src /
  // diag_src ("a transform is in force": y_transformed / diag_transformed below), `amp_s` keeps s resident as [B][N], and
  // amp_L holds sum_n log|s_n| | the flags of problems with a zero or non-finite s_n, fetched behind the forming pass
  // (amp_ev) and folded into the results on the host (amplitude_adjust)
  int amp_K = 0;
  long amp_stride = 0;                // 0: one basis [K][N] for all problems, K * N: [B][K][N]
  bool amp_active = false;
  bool amp_formed = false;            // the forming pass has run for the amplitudes in force (a series is set)
  int amp_eval = 0;                   // the evaluation in force: 0 ran without amplitudes, 1 its log term is amp_back's, 2 host_amp_L's
  std::vector<double> host_amp_L;     // L[B] | flag[B] of the evaluation in force, once the forming pass has moved on
  std::vector<double> host_amp;       // [B][K] (empty until clr_batch_set_amplitudes)
  DevBuf amp_basis, amp_dev, amp_s, amp_part, amp_Lf;
  clr::PinnedBuffer<double> amp_pin, amp_back;  // staging of the amplitudes' upload; L[B] | flag[B] as downloaded
  clr::Event amp_ev, amp_back_ev;     // recorded behind the upload / the download
  double amp_project_ms = 0.0;        // device time of the last clr_batch_grad_amplitudes' projection
  // clr_batch_grad_mean: the narrow reverse sweep sums the adjoint of y per chunk (BatchParams::g_ysum) and reduces it
  // into mean_out; grad_mean_done[b] says which problems it settled (the rest take mean_partial_batch)
  bool grad_want_mean = false;
  std::vector<char> grad_mean_done;
  int layout = 2;                    // 0 row-major direct, 1 interleaved copy, 2 staged through LDS
  double tmax = 0.0, dmax = 0.0;      // max |t|, max |d_comp| (host side, O(B))
  double dxmax = 0.0, cmax = 0.0;     // max |t[n+1] - t[n]|, max decay rate: the lazy-decay kernels need cmax * dxmax < 2^-7
  // floors for the four maxima above (clr_batch_set_selection_bounds): a sharded plan hands every shard the maxima
  // of the WHOLE batch, so that all shards pick the same kernels whatever the sharding
  double floor_tmax = 0.0, floor_dxmax = 0.0, floor_dmax = 0.0, floor_cmax = 0.0;
  bool b_zero = false;                // every b_comp of the current coefficients is exactly zero (clr_batch_set_coefficients)
  double set_series_host_ms = 0.0;    // host time of the last clr_batch_set_series (scan + uploads)
  double dtmin = 0.0;                 // smallest step of t over the plan's series (negative: not sorted; NaN: a NaN time)
  clr::UploadStaging staging;         // pinned staging + copy streams of clr_batch_set_series (large series only)
  DevBuf scan;                        // results of the device-side scans of t
  int coop_prefix = 2;                // 0 single lane, 1 16 lanes walking the chunks, 2 multi-level (clr_prefix_kernels.h)
  int plan_levels = -1, plan_g = 0;   // clr_batch_set_prefix_plan: < 0 = chosen by clr::plan_prefix
  clr::PrefixPlan plan;
  DevBuf lvl_elems, lvl_starts;       // composed elements / start states of the upper levels
  DevBuf g_riders, g_out, g_res;      // chunk-parallel gradient (clr_grad_kernels.h): riders, records, result (+ fallback)
  int grad_rebuild_span = 4;          // reverse mode, adaptive rule: stored states at least this many steps apart (GradStore::span)
  DevBuf g_rec, g_ck;                 // reverse mode: w, D, x per sample; stored states (GradStore, clr_grad_core.h)
  DevArray<unsigned char> g_ckflag;   // what the forward pass did before each step, per wave of 64 chunks
  std::vector<double> host_cmax;      // per problem: largest decay rate (sizes the stored states)
  std::vector<double> grad_span;      // per problem (one entry when the series is shared): longest time a scan chunk spans
  bool grad_span_valid = false;
  int grad_mode = 0;                  // clr_batch_set_grad_mode: 0 auto (reverse), 1 forward (one tangent per partial)
  int grad_K = 0;                     // > 0: distance of the stored states (steps), else from c_max dt_max
  int grad_riders_mode = 0;           // 0 auto (from the scan's elements when a gradient chunk is a scan chunk), 1 along the trajectory
  double grad_drift_tol = 1e-9;       // a reverse sweep whose reconstructed states drift further is redone forward
  double grad_drift_max = 0.0;        // last gradient: largest drift among the problems it settled
  int grad_forward_reruns = 0;        // ... and the problems redone by the forward-mode kernels
  bool grad_reverse_used = false;
  std::vector<double> host_jitter;    // per problem, as set (the reference zeroes d/d jitter at jitter <= eps)
  // clr_batch_information (clr_binfo_kernels.h): the tangent states of every (gradient chunk, direction); a tile's rows;
  // its Gram pass' slab partials with the tile's matrices behind them.  Scratch of one call: nothing in them is cached
  DevBuf i_tan, i_rows, i_part;
  int information_tile = 0;           // clr_batch_set_information_tile: problems per tile (0: automatic)
  clr::Event info_ev[2];              // ... its two timing events, created by the first call
  double information_ms = 0.0;        // device time of the last call, from its evaluation to its last Gram pass
  bool grad_scan_only = false;        // the evaluation inside clr_batch_grad: by the scan, its start states are needed
  int grad_fallbacks = 0;             // problems of the last gradient that took the sequential kernel
  double cert_resid = 1e-11;          // end-state mismatch of the chunked replay that still counts as consistent
  double cert_gamma = 1e7;            // conditioning record gamma_max / mu_min above which a problem leaves the replay-free route
  double cert_gamma_abs = 1e4;        // ... and gamma_max alone (decide_kernel; calibration: profiles/r03_conditioning_calibration.txt)
  double cert_eg = 3e-9;              // ... and gamma_max x the largest measured G error of the chunks
  int summarize_mode = -1;            // -1 auto, 0 single wave, 1 role split (widths 7, 8)
  // warm-started plain recurrence for series that forget their past (clr_batch_kernels.h: warm_kernel)
  int warm_mode = -1;                 // -1 auto (per problem, from the decay over the samples before the chunk boundaries),
                                      // 0 off, 1 every problem with warm_forced_K warm-up steps (tests: the boundary check decides)
  int warm_forced_K = 0;
  int warm_explicit_chunks = 0;       // chunk count asked for through clr_batch_set_chunks (0: automatic)
  int wnchunk = 0, wL = 0;            // the warm path's own chunking
  static const int WARM_NK = 10;
  int warm_cand[WARM_NK] = {8, 12, 16, 24, 32, 48, 64, 80, 96, 128};
  std::vector<double> warm_span;      // [B or 1][WARM_NK] shortest time the K samples before a chunk boundary span
  std::vector<int> warm_K;            // [B] warm-up steps per problem of the current coefficients (0: scan)
  std::vector<double> host_cmin;      // [B] slowest decay rate of problem b (last set_coefficients)
  bool warm_K_dirty = false;          // warm_K changed on the host after the last upload (set_series re-selected it)
  bool warm_active = false;           // the current (series, coefficients) pair runs the warm path
  bool warm_inflight = false;         // results of a warm evaluation have not been looked at yet
  bool small_inflight = false;        // ... of a one-launch evaluation (small_batch_kernel): pending problems, no warm statistics
  int warm_boost = 0;                 // candidates skipped after an evaluation with many fallbacks
  int warm_clean = 0;                 // consecutive warm evaluations without a fallback (decays warm_boost)
  int warm_settled = 0, warm_fallbacks = 0;  // of the last evaluation
  DevBuf wstarts, wends, wpart, wresid;
  SeriesCopy warm_series;             // the warm kernel's padded chunk-interleaved copy of the series
  int wKpad = 0, wrows = 0;
  SeriesCopy small_series;            // the one-launch path's chunk-interleaved copy of the series (small_params, api_batch.hip)
  DevArray<int> wints;                // wflags [B * wnchunk] | need_scan [B] | K [B]
  // general terms for the whole batch (clr_batch_set_general): the plan then evaluates through the any-width sequential
  // kernel, one workgroup per problem (generic_kernels.hip: generic_loglike_batch_kernel)
  int J_general = 0;
  DevBuf gA, gU, gV;
  long gA_stride = 0, gU_stride = 0, gV_stride = 0;
  bool have_series = false, have_coeffs = false, have_factor = false;
  bool evaluated = false;             // an evaluation has been enqueued since the plan was (re)chunked
  DevBuf elems, starts, part, partx, cond, out;  // out: ll | logdet | quad | status (B ints)
  DevArray<int> flags;                     // flags [B*nchunk] | flagsx [B*nchunk] | need_exact [B]
  int force_exact = 0;
  bool factor_valid = false;  // a materialising run has written the factor under the chunking in force
  DevBuf bs_decay, bs_y;                        // clr_batch_dot_L / clr_batch_dot: the chunks' decay products; dot's output, chunk-interleaved
  DevBuf bs_rm, bs_x, bs_M, bs_off, bs_starts;  // clr_batch_solve: right-hand sides row-major / chunk-interleaved, chunk maps, offsets, start states
  bool bs_M_valid = false;                      // bs_M holds the chunk maps of the factor in HBM (they depend on the factor only)
  double solve_device_ms = 0.0;                 // device time of the last clr_batch_solve (HIP events around its kernels)
  // clr_batch_leave_one_out: diag(K^-1) row-major [B][N], the chunks' offsets / start matrices of its recurrence
  // [B][nchunk][J (J + 1) / 2] (narrow plans), the log predictive densities [B]; timing events around the diagonal's
  // kernels and the reduction, and the device time of the last call's three parts
  DevBuf loo_c, loo_Q, loo_out;
  clr::Event loo_ev[4];
  double loo_diag_ms = 0.0, loo_solve_ms = 0.0, loo_reduce_ms = 0.0;
  // clr_batch_predict_var_recurrence: the chunks' forward start states [B][nchunk][J (J + 1) / 2]; they and the backward
  // start matrices the leave-one-out diagonal's first two passes leave in loo_Q depend on the factor only, like bs_M, and
  // follow its validity rule (counted as formed only once the kernels that formed them have run to completion)
  DevBuf pv_S;
  bool pv_S_valid = false, loo_Q_valid = false;
  int predict_tile = 0;                         // clr_batch_set_predict_tile: prediction points per tile of the point consumers (predict_tile; 0: automatic)
  int periodogram_tile = 0;                     // clr_batch_set_periodogram_tile: frequencies per tile of clr_batch_periodogram (0: automatic)
  double periodogram_ms = 0.0;                  // device time of the last clr_batch_periodogram's kernels
  int conditional_tile = 0;                   // clr_batch_set_conditional_tile: problems per tile of clr_batch_predict_cov / _sample_conditional (0: automatic)
  clr::Event bs_ev[2];                          // ... its two timing events, created by the first solve, kept for the plan's life
  int factor_layout = 0;      // clr_batch_set_factor_layout: 0 the reference's four arrays, 1 lean (W, D; phi, u regenerated)
  bool factor_is_lean = false;  // what the factor in HBM holds (set by the materialising run that wrote it)
  bool factor_inputs_changed = false;  // series or coefficients replaced since that run (a lean factor can then no longer be expanded)
  DevBuf phi, u, W, D;        // materialised factor, chunk-interleaved device layout
  // heads of the chunks recomputed from the previous chunk's replayed end state (clr_batch_set_factor_refine; BatchParams::ends)
  int factor_refine = 64;     // samples per chunk head (0: off -- round 5's factor)
  DevBuf ends;                // [B][nchunk][START] states at the chunks' ends, written by the materialising replay
  DevBuf fphi, fu, fW, fD;    // one problem in the reference's storage (get_factor)
  // problems the conditioning record sends to the checked chunked replay (level 1), re-planned as a small plan of their
  // own with many short chunks instead of replaying long chunks sequentially beside an idle chip (clr_batch_set_rescue)
  int rescue_mode = -1;            // -1 auto (chunks of >= 1024 samples), 0 off: the inline chunked replay, 1 whenever possible
  bool rescue_inflight = false;    // the evaluation in flight deferred its level-1 problems (pending until resolved)
  bool is_rescue_plan = false;     // this plan IS such a side plan (never defers)
  BatchPtr rescue;
  DevArray<int> rescue_idx;        // device: the re-planned problems' indices
  int rescue_last = 0;             // problems of the last resolved evaluation that were re-planned (or replayed inline: negative)
  long rescue_total = 0;
  long rescue_plan_key = -1;       // the batch-wide count of pending problems the side plan in `rescue` was chunked for
  // A plan that is ONE SLICE of a larger batch (csrc/sharded.cpp, clr_group_hooks.h): every decision that looks at a
  // count over "the plan's problems" -- the prefix plan's time model, the one-launch path, the warm path's activation
  // and adaptation, deferring level-1 problems, side plan or inline replay and the side plan's chunk count -- is
  // taken from the counts over the WHOLE batch, so that a problem's result does not depend on the sharding.
  int group_B = 0;                 // problems of the whole batch (0: this plan is the whole batch)
  long warm_eligible = 0;          // problems of this plan the warm path could start at the coefficients in force
  long warm_eligible_total = -1;   // ... of the whole batch, as handed down (group_B > 0 only)
  // warm_resolve in two halves (resolve_begin / resolve_finish): the state between them
  bool res_open = false, res_was_warm = false, res_was_rescue = false;
  long res_pending = 0;
  bool pin_results = false;        // the pinned staging buffer holds the final results of the evaluation in force
  // optional per-kernel HIP events around the launches of clr_batch_enqueue (clr_batch_set_profiling)
  int prof_on = 0, prof_steps = 0;
  std::vector<clr::Event> prof_events;  // 7 per recorded step

  ~clr_batch() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream.get());
    rescue.reset();  // (its own plan: gone before this plan's members)
  }
};



// ---- defined in api_batch.hip, called by the consumers too (api_batch_consumers.hip) ---------------------------
// settles the evaluation in flight (pending problems of a warm, one-launch or re-planned evaluation); `pin_current`: set
// when that left the final results in the pinned staging buffer
int warm_resolve(clr_batch* h, bool* pin_current);
// draws the kernel program refused: NaN and CLR_INVALID_ARGUMENT in the arrays given
void mark_refused(const clr_batch* h, double* a, double* b, double* c, int* status);
// clr_batch_get_results before the amplitude model's log term: the scaled system's loglike', logdet', quad'
int batch_results_scaled(clr_batch* h, double* loglike, double* logdet, double* quad, int* status);
// the amplitude model's log term L = sum_n log|s_n| folded into results of the scaled system, in double on the host:
// logdet = logdet' + (L + L), loglike = loglike' - L, quad = quad'; a problem with a zero or non-finite s_n inside its
// length: NaN and CLR_INVALID_ARGUMENT (mark_refused's quiet semantics).  No amplitudes in force: nothing is touched.
int amplitude_adjust(clr_batch* h, double* loglike, double* logdet, double* quad, int* status);
// ... and the log term of the amplitudes IN FORCE into a value that was formed from the series in force with no evaluation
// in front (the sequential plan gradient of a one-chunk plan of widths 33..64): amp_eval and the results stay untouched.
int amplitude_adjust_in_force(clr_batch* h, double* loglike, int* status);

// ---- what a replaced input of a plan leaves stale: one function per cause, called by the entry points ----------
namespace {
// a materialising run has queued the writes of the factor, in the lean layout or the reference's
void factor_written(clr_batch* h, bool lean) {
  h->factor_is_lean = lean; h->factor_inputs_changed = false; h->factor_valid = true; h->bs_M_valid = false;
  h->pv_S_valid = h->loo_Q_valid = false;
  h->variance_changed = false;
}
// the factor's layout in HBM no longer is the one a materialising run would write (chunking, factor layout)
void factor_dropped(clr_batch* h) { h->have_factor = h->factor_valid = false; }

// t, diag and y are being overwritten: nothing derived from the old ones survives
void series_replaced(clr_batch* h) {
  h->scan_series.stale = h->warm_series.stale = h->small_series.stale = true;
  h->grad_span_valid = false;
  h->factor_inputs_changed = true;
  h->warm_active = false;  // (the warm path's spans and the warm-ups selected from them)
  h->warm_span.clear();
}
// `y` holds another residual, of stride `y_stride` (a mean set, changed or removed): of the scan's copy Y alone is
// rebuilt unless the stride changed (a shared series became a per-problem residual, or back)
void residual_replaced(clr_batch* h, long y_stride) {
  if (y_stride != h->y_stride) h->scan_series.stale = true;
  h->y_stride = y_stride;
  h->scan_series.y_stale = true;
  h->warm_series.stale = h->small_series.stale = true;
}
// `diag` holds other variances, of stride `diag_stride` (noise weights or a noise basis set, changed or removed): of the
// scan's copy D alone is rebuilt unless the stride changed (a shared diagonal became per-problem variances, or back); the
// warm and the one-launch copies are rebuilt whole; the factor in HBM is another matrix' (a lean one can no longer be
// expanded, clr_batch_grad_noise_weights asks for a new run).  Nothing derived from t alone -- the series' statistics and
// selection bounds, the warm path's spans and selection, the gradient's spans -- reads `diag`, and all of it stays.
void variance_replaced(clr_batch* h, long diag_stride) {
  if (diag_stride != h->diag_stride) h->scan_series.stale = true;
  h->diag_stride = diag_stride;
  h->scan_series.d_stale = true;
  h->warm_series.stale = h->small_series.stale = true;
  h->factor_inputs_changed = true;
  h->variance_changed = true;
}
// nchunk and L changed: the scan's copy, the gradient's spans and the factor's layout follow them
void chunking_replaced(clr_batch* h) {
  h->scan_series.stale = true;
  h->grad_span_valid = false;
  factor_dropped(h);
  h->evaluated = false;
}
// ... and the warm path's own chunking was planned again (warm_plan_chunks)
void warm_chunking_replaced(clr_batch* h) { h->warm_series.stale = h->small_series.stale = true; }
void coefficients_replaced(clr_batch* h) {  // (pin_results: the staging buffer is about to carry the coefficients)
  h->factor_inputs_changed = true; h->pin_results = false; h->kp_in_force = false;
}
// the layout or the summarize mode changed: whether the scan reads its copy may have changed with it
void scan_reader_changed(clr_batch* h) { h->scan_series.stale = true; }
}  // namespace

// ---- a plan's state as kernel parameters -----------------------------------------------------------------------
namespace {
// the maxima the kernel selection looks at: the plan's own, raised to the floors of a sharded parent
double sel_max(double own, double floor) {  // (NaN on either side wins: the conservative kernels)
  if (own != own) return own;
  if (floor != floor) return floor;
  return own >= floor ? own : floor;
}
// the batch size the selection rules look at: the whole batch's when the plan is a slice of one (clr_batch::group_B)
int sel_B(const clr_batch* h) { return h->group_B > 0 ? h->group_B : h->B; }
// The lazy flavours advance every row's (cos, sin) pair by a rotation through d (t_n+1 - t_n) between anchors, where the
// reference (cholesky.h:137) and every other kernel take sincos of fl(d t_n) at each sample.  The two phases differ by the
// rounding of d t, up to |d t| 2^-53 rad: at max |d| max |t| ~ 1.6e9 the wide summaries then settle values 5e-10 and
// gradient riders ~3e-4 away from the reference's recurrence (tests/test_gpu_grad_truth.py, library trig at t ~ 3e8).
// Below 2^20 the difference stays under 1.2e-10 rad.
constexpr double CLR_LAZY_PHASE_LIMIT = 1048576.0;
bool lazy_phases_ok(const clr_batch* h) {
  return sel_max(h->dmax, h->floor_dmax) * sel_max(h->tmax, h->floor_tmax) < CLR_LAZY_PHASE_LIMIT;
}
bool lazy_eligible(const clr_batch* h) {
  // |c dx| < 2^-7 at every step: Psi stays within [0.6, 1] over the 64 steps between renormalisations
  // (CLR_SPLIT_RENORM, clr_split_kernels.h);
  // |d dx| < 2^-5: the per-step rotation of the (cos, sin) pairs uses a short Taylor series
  const double cmax = sel_max(h->cmax, h->floor_cmax), dmax = sel_max(h->dmax, h->floor_dmax),
               dxmax = sel_max(h->dxmax, h->floor_dxmax);
  return h->have_series && h->have_coeffs && cmax * dxmax < 0.0078125 && dmax * dxmax < 0.03125 && lazy_phases_ok(h);
}

// Whether the lazy role-split summarize runs its b_comp == 0 variant on this plan (clr_split_kernels.h:
// split_trajectory_lazy); CLR_SPLIT_GENERIC=1: the general kernel for every batch.
bool split_lazy_bzero(const clr_batch* h) {
  const char* g = clr::option("CLR_SPLIT_GENERIC");
  return h->J_comp > 0 && h->b_zero && !(g && g[0] == '1');
}

// Wide plans (wave per (problem, chunk), widths 9..64): the lazy flavour of the summarize takes any series since round 5 --
// a lane whose own interval is too long for the Taylor steps sends its wave through the full sincos / exp for that batch
// (wide_scan_body, feature_batch) -- as long as the decay accumulated between two renormalisations (64 steps) stays far
// from the exponent range: Psi^-2 < e^(2 x 64 x 2) = e^256.
bool lazy_eligible_wide(const clr_batch* h) {
  // widths 9..16 (four lanes per row): the two flavours cost the same there -- 6.5 against 6.7 ms on a dense series, 7.4
  // against 7.0 on one where EVERY batch takes the slow path (profiles/r05m_wide_lazy_gaps.txt) -- so they keep the strict rule
  if (h->J + h->J_general <= 16) return lazy_eligible(h);
  const double cmax = sel_max(h->cmax, h->floor_cmax), dxmax = sel_max(h->dxmax, h->floor_dxmax);
  return h->have_series && h->have_coeffs && cmax * dxmax < 2.0 && lazy_phases_ok(h);
}

// `behind_fast_path` (here, in defer_runs and in batch_params): the question is asked for the scan behind the warm or
// the one-launch path -- the plan's row-major arrays, the single-wave summarize, pending problems only
bool split_active(const clr_batch* h, bool behind_fast_path) {
  // explicit modes 1 / 2, or auto (-1):
  //  * widths 7 and 8 on a densely sampled series: the split kernel with the decay factored out of the state
  //    (lazy) beats the single-wave kernel for every shape (2.0-2.5 ms against 2.3-3.6, profiles/r02zzz_split_ab_shapes.txt);
  //  * any other series: the plain split at width 7 (2.5-2.7 ms against 2.8-3.0 on the paper's sparse family) and at
  //    width 8 with at least two complex terms (3.1-3.2 against 3.8-4.2; profiles/r02zzz_sparse_ab.txt).  With
  //    fewer complex terms at width 8 its trajectory wave spills ((8,0), (6,1): 4.1-4.2 against 3.7): single wave.
  if (!(h->launch && h->nchunk > 1 && clr::have_summarize_split(h->J_real, h->J_comp))) return false;
  if (behind_fast_path) return false;
  // per-problem lengths: the single-wave kernel (forcing mode 1 or 2 is refused: clr_batch_set_summarize_mode).  The
  // role-split kernels sit at their register and scheduling limits: with the per-problem length in place of the kernel
  // argument N the UNIFORM headline plan ran 2 % slower, all of it in the summarize (profiles/ragged_timing.txt, second
  // part), and uniform plans must not pay
  if (h->ragged) return false;
  if (h->summarize_mode > 0) return true;
  if (h->summarize_mode < 0 && h->J >= 7 && lazy_eligible(h)) return true;
  return h->summarize_mode < 0 && (h->J == 7 || (h->J == 8 && h->J_comp >= 2));
}

// Level-1 problems (ill-conditioned, not flagged) are left pending and re-planned with short chunks instead of being
// replayed inline: when the plan's chunks are long enough that ONE such problem would cost the whole batch a sequential
// chunk-time (config 4: +11 ms on 12.7; profiles/r04zz_wide_midbatch.txt) -- a re-plan is three passes over chunks a
// tenth as long.  Never on forced-exact / materialising runs (they replay everything), inside the gradient's own
// evaluation, behind the warm path, or on a side plan.
bool defer_runs(const clr_batch* h, int materialize, bool behind_fast_path) {
  if (h->rescue_mode == 0 || h->is_rescue_plan || materialize || h->force_exact || h->grad_scan_only || behind_fast_path) return false;
  if (h->nchunk < 2 || h->J_general > 0 || sel_B(h) < 2) return false;
  if (h->rescue_mode == 1) return true;
  // widths 33..64: a side plan is itself <= 16 chunks chained by a walk of ~0.6 ms each -- it does not beat the inline
  // replay of one of the parent's chunks (profiles/r05d_wide64_chunks.txt)
  if (h->J > 32) return false;
  return h->L >= 1024;
}

// The plan's three series arrays and where each goes in the copy `c`, `cells` doubles per series (a shared series has
// ONE copy).  reserve() sizes the copy; the function that builds it launches its relayout kernel per job (pad: how the
// cells past the series' end are filled).
struct SeriesJobs {
  struct Job { const double* src; long stride; DevBuf* dst; int pad; int nsrc; long dst_stride; } job[3];
  size_t cells;
  SeriesJobs(const clr_batch* h, SeriesCopy& c, size_t cells_) : cells(cells_) {
    auto make = [&](const DevBuf& src, long stride, DevBuf& dst, int pad) {
      return Job{src.p, stride, &dst, pad, stride ? h->B : 1, stride ? (long)cells : 0};
    };
    job[0] = make(h->t, h->t_stride, c.T, 1);
    job[1] = make(h->diag, h->diag_stride, c.D, 2);
    job[2] = make(h->y, h->y_stride, c.Y, 0);
  }
  int reserve() {
    for (Job& j : job) {
      const int st = j.dst->reserve((size_t)j.nsrc * cells);
      if (st != CLR_OK) return st;
    }
    return CLR_OK;
  }
};

// whether the scan's kernels read the chunk-interleaved copy (the wide kernels, the warm-started recurrence and the scan
// behind it read the row-major arrays)
bool scan_reads_copy(const clr_batch* h) {
  return h->launch && (h->layout == 1 || split_active(h, false)) && h->nchunk > 1;
}

// what a plan with per-problem lengths refuses (`what`: the refused call or run)
int refuse_ragged(const clr_batch* h, const char* what) {
  if (!h->ragged) return CLR_OK;
  return fail(CLR_UNSUPPORTED, std::string(what) + ": the plan has per-problem lengths (clr_batch_set_series_ragged), which the "
                               "fused evaluation and the gradient of narrow plans carry -- set the series without lengths, or "
                               "one plan per length, for the materialised factor and its consumers");
}

int batch_params(clr_batch* h, int materialize, clr::BatchParams& P, bool behind_fast_path) {
  if (!h->have_series || !h->have_coeffs)
    return fail(CLR_INVALID_ARGUMENT, "set_series and set_coefficients must be called first");
  int st = CLR_OK;
  if (materialize && (st = refuse_ragged(h, "a materialising run")) != CLR_OK) return st;
  if (materialize && !h->have_factor) {
    // widths 1..8: chunk-interleaved device layout (replay_chunk, MATERIALIZE == 2); widths 9..64: the wide kernels
    // write the reference's own storage per problem (wide_scan_kernel, MODE 0: phi, u [N-1][J], W [N][J], D [N])
    const size_t B = (size_t)h->B, J = (size_t)h->J, cells = h->launch ? (size_t)h->L * h->nchunk : (size_t)h->N;
    const bool lean = h->launch && h->factor_layout == 1;  // (phi and u are not stored: 8 N (J + 1) instead of 8 N (3 J + 1) bytes per problem)
    if (!lean && (st = h->phi.reserve(B * J * cells)) != CLR_OK) return st;
    if (!lean && (st = h->u.reserve(B * J * cells)) != CLR_OK) return st;
    if ((st = h->W.reserve(B * J * cells)) != CLR_OK) return st;
    if ((st = h->D.reserve(B * cells)) != CLR_OK) return st;
    h->have_factor = true;
  }
  memset(&P, 0, sizeof(P));
  const size_t B = (size_t)h->B, nr = B * h->J_real, nc = B * h->J_comp;
  P.B = h->B; P.N = h->N; P.nchunk = h->nchunk; P.L = h->L; P.L0 = h->L0;
  P.len = h->ragged ? h->len_dev.p : nullptr;
  P.fast_trig = (sel_max(h->dmax, h->floor_dmax) * sel_max(h->tmax, h->floor_tmax) < CLR_FAST_TRIG_LIMIT) ? 1 : 0;
  P.coop_prefix = h->coop_prefix;
  P.plan = h->plan;
  P.lvl_elems = h->lvl_elems.p;
  P.scan_ws = (!h->launch && h->scan_ws_doubles) ? h->lvl_elems.p : nullptr;
  P.lvl_starts = h->lvl_starts.p;
  P.jitter = h->coeffs.p + 2 * nr + 4 * nc;
  P.a_real = h->coeffs.p;
  P.c_real = P.a_real + nr;
  P.a_comp = P.c_real + nr;
  P.b_comp = P.a_comp + nc;
  P.c_comp = P.b_comp + nc;
  P.d_comp = P.c_comp + nc;
  // role-split summarize (two waves per SIMD, clr_split_kernels.h) for the widths whose element
  // does not fit one wave's registers; it reads the chunk-interleaved copy of the series
  const bool split = split_active(h, behind_fast_path);
  P.split = split ? 1 : 0;
  P.split_lazy = (split && h->summarize_mode != 1 && lazy_eligible(h)) ? 1 : 0;
  P.split_bzero = (P.split_lazy && split_lazy_bzero(h)) ? 1 : 0;
  // wide plans: the lazy-decay flavour of the wide summarize on dense series (mode 0 / 1 switch it off)
  // (1: dense everywhere -- the strict rule; 2: only the relaxed one: the flavour with the per-batch range test)
  if (!h->launch && h->nchunk > 1 && (h->summarize_mode < 0 || h->summarize_mode == 2) && lazy_eligible_wide(h))
    P.split_lazy = lazy_eligible(h) ? 1 : 2;
  if (!behind_fast_path && scan_reads_copy(h)) {
    const long cells = (long)h->nchunk * h->L;
    SeriesCopy& c = h->scan_series;
    if ((st = SeriesJobs(h, c, (size_t)cells).reserve()) != CLR_OK) return st;
    P.t = c.T.p; P.diag = c.D.p; P.y = c.Y.p;
    P.t_stride = h->t_stride ? cells : 0;
    P.diag_stride = h->diag_stride ? cells : 0;
    P.y_stride = h->y_stride ? cells : 0;
    P.lane_is = h->nchunk; P.lane_cs = 1;
    P.staged = 0;
  } else {
    P.t = h->t.p; P.diag = h->diag.p; P.y = h->y.p;
    P.t_stride = h->t_stride; P.diag_stride = h->diag_stride; P.y_stride = h->y_stride;
    P.lane_is = 1; P.lane_cs = h->L;
    P.staged = ((h->layout == 2 || behind_fast_path) && h->nchunk > 1) ? 1 : 0;
  }
  P.elems = h->elems.p; P.starts = h->starts.p; P.part = h->part.p; P.flags = h->flags.p;
  P.cond = h->cond.p;
  P.cert_gamma = h->cert_gamma;
  P.cert_gamma_abs = h->cert_gamma_abs;
  P.cert_eg = h->cert_eg;
  P.egerr = h->cond.p + (size_t)h->B * h->nchunk * 3;
  P.cert_resid = h->cert_resid;
  P.head_cap = clr::output_check_cap(); P.head_tol = clr::output_check_tol();  // (materialising wide plans: BatchParams::head_check)
  {
    const size_t pc = B * (size_t)h->nchunk;
    P.partx = h->partx.p; P.flagsx = h->flags.p + pc; P.need_exact = h->flags.p + 2 * pc;
    // a single chunk starts from the zero state: its replay IS the whole recurrence
    P.force_exact = (materialize || h->force_exact || h->nchunk < 2) ? 1 : 0;
  }
  P.out_ll = h->out.p; P.out_logdet = h->out.p + B; P.out_quad = h->out.p + 2 * B;
  P.out_status = reinterpret_cast<int*>(h->out.p + 3 * B);
  if (h->wints.p) {
    const size_t wpc = B * (size_t)h->wnchunk;
    P.wflags = h->wints.p; P.need_scan = h->wints.p + wpc; P.wK = h->wints.p + wpc + B;
    P.wL = h->wL; P.wnchunk = h->wnchunk;
    P.wstarts = h->wstarts.p; P.wends = h->wends.p; P.wpart = h->wpart.p; P.wresid = h->wresid.p;
    P.warm_resid = h->cert_resid;
    const long cells = (long)h->wrows * h->wnchunk;
    P.wt = h->warm_series.T.p; P.wdiag = h->warm_series.D.p; P.wy = h->warm_series.Y.p;
    P.wt_stride = h->t_stride ? cells : 0; P.wdiag_stride = h->diag_stride ? cells : 0; P.wy_stride = h->y_stride ? cells : 0;
    P.wKpad = h->wKpad; P.wrows = h->wrows;
  }
  P.only_pending = behind_fast_path ? 1 : 0;
  P.defer_level1 = defer_runs(h, materialize, behind_fast_path) ? 1 : 0;
  P.wide_materialize = (materialize && !h->launch) ? 1 : 0;
  P.ends = nullptr; P.ends_alt = nullptr; P.ends_in = nullptr;
  P.fixup_steps = 0;
  P.refine_samples = 0;
  {  // (the rotation of the phases needs |d dx| < 2^-5 at every step and phases below CLR_LAZY_PHASE_LIMIT; the decay is not involved)
    const double dmax = sel_max(h->dmax, h->floor_dmax), dxmax = sel_max(h->dxmax, h->floor_dxmax);
    P.dense = (h->have_series && h->have_coeffs && dmax * dxmax < 0.03125 && lazy_phases_ok(h)) ? 1 : 0;
  }
  if (materialize && h->nchunk > 1 && h->factor_refine > 0 && h->J_general == 0 && h->J <= clr::wide_max_width()) {
    size_t START = 0;
    if (h->launch) START = (size_t)h->launch->start_doubles;
    else { const size_t JP = (size_t)clr::wide_padded_width(h->J); START = JP * (JP + 1) / 2 + JP; }
    if ((st = h->ends.reserve((size_t)h->B * h->nchunk * START * (h->launch ? 1 : 2))) != CLR_OK) return st;
    P.ends = h->ends.p;
    if (!h->launch) P.ends_alt = h->ends.p + (size_t)h->B * h->nchunk * START;  // (wide plans: the output check's second buffer)
    // (the recurrence needs a few J samples to forget a start state: wide plans take the setting per 16 rows of state)
    P.refine_samples = h->launch ? h->factor_refine : h->factor_refine * (clr::wide_padded_width(h->J) / 16);
  }
  P.phi = h->phi.p; P.u = h->u.p; P.W = h->W.p; P.D = h->D.p;
  return CLR_OK;
}

// Row-major API layout -> the chunk-interleaved copy the scan reads (sized by batch_params), if it is stale or
// `regardless`: 3 tiled transposes, Y alone when only the residual changed, D alone when only the variances did.  Returns
// whether the rebuild was queued: a copy that no route reads is not built and STAYS stale -- the need for it can appear
// later (a new coefficient draw can switch the summarize kernel, another evaluation can take another route) with the
// series unchanged.
bool build_scan_series(clr_batch* h, bool regardless) {
  SeriesCopy& c = h->scan_series;
  if (!(regardless || c.stale || c.y_stale || c.d_stale) || !scan_reads_copy(h)) return false;
  const bool all = regardless || c.stale;
  const SeriesJobs jobs(h, c, (size_t)h->nchunk * h->L);
  for (auto& j : jobs.job)
    if (all || (c.y_stale && j.dst == &c.Y) || (c.d_stale && j.dst == &c.D))
      clr::launch_relayout(j.src, j.stride, j.dst->p, j.dst_stride, j.nsrc, h->N, h->L, h->nchunk, j.pad, h->stream.get());
  c.stale = c.y_stale = c.d_stale = false;
  return true;
}


// CLR_OK, or CLR_HIP_ERROR when a kernel of the flow could not be configured (nothing after it is launched: the later
// kernels would run on stale start states)
int wide_flow(clr::BatchParams& P, int J_real, int J_comp, hipStream_t stream, const clr::Event* ev) {
  auto mark = [&](int i) { if (ev) (void)hipEventRecord(ev[i].get(), stream); };
  const int JP = clr::wide_padded_width(J_real + 2 * J_comp + P.J_general);
  mark(1);
  if (P.nchunk > 1) clr::launch_wide_summarize(P, J_real, J_comp, stream);
  mark(2);
  // widths 33..64: the prefix and the corrections in one walk per problem (wide64_kernels.hip); CLR_WIDE_WALK=1 takes
  // that kernel at the padded width 32 too (cross-check of the two-kernel path; tests)
  const bool walk32 = clr::option("CLR_WIDE_WALK") != nullptr;
  if (JP == 64 || (JP == 32 && walk32 && !(P.scan_ws && P.coop_prefix == 2))) {
    if (clr::launch_wide_walk(P, JP, stream) != 0)
      return fail(CLR_HIP_ERROR, "the width-64 walk kernel needs 132 KB of dynamic LDS per workgroup: the device refused the attribute");
    mark(3);
    clr::launch_wide_decide(P, JP, stream);
  } else {
    clr::launch_wide_prefix(P, JP, stream);
    mark(3);
    clr::launch_wide_correct(P, JP, stream);
  }
  mark(4);
  // one chunk: the sweep itself; several: the chunked replay of forced runs and of the problems the
  // conditioning record marked (level 1), with its end states checked against the scan
  clr::launch_wide_loglike(P, J_real, J_comp, stream);
  if (P.nchunk > 1) {
    clr::launch_wide_check_replay(P, stream);
    if (P.head_cap > 0.0 && P.ends && P.ends_alt && P.wide_materialize && P.cond) {
      // end states off the scanned start states, but not by much (level 3): the chunks again, each from the previous
      // chunk's replayed end state, until what two consecutive replays wrote agrees (BatchParams::head_check); an even
      // number of attempts, so that P.ends holds the last (or last but one: equal to head_tol) end states for the fix-up
      // (the mismatch reaches its floor at the second or third: profiles/r06q_output_check_convergence.txt)
      const int attempts = 4;
      for (int k = 0; k < attempts; ++k) {
        clr::BatchParams F = P;
        F.fixup_steps = P.L + (P.L0 > P.L ? P.L0 - P.L : 0);
        F.head_check = (k + 1 == attempts) ? 2 : 1;
        F.ends_in = (k & 1) ? P.ends_alt : P.ends;
        F.ends = (k & 1) ? P.ends : P.ends_alt;
        clr::launch_wide_loglike(F, J_real, J_comp, stream);
        clr::launch_wide_head_decide(F, stream);
      }
    }
  }
  if (P.nchunk > 1 && P.ends && P.wide_materialize && P.refine_samples > 0) {
    clr::BatchParams F = P;  // the heads of the chunks again, from the previous chunk's replayed end state
    F.fixup_steps = P.refine_samples;
    clr::launch_wide_loglike(F, J_real, J_comp, stream);
  }
  if (P.nchunk > 1) {
    clr::launch_finalize(P, stream);
    clr::BatchParams S = P;  // the flagged problems, sequentially
    S.nchunk = 1; S.L = P.N; S.L0 = 0; S.seq_only = 1; S.force_exact = 1; S.ends = nullptr; S.fixup_steps = 0;
    clr::launch_wide_loglike(S, J_real, J_comp, stream);
  }
  mark(5);
  mark(6);
  return CLR_OK;
}

const int PROF_NK = 6, PROF_MAX_STEPS = 4096;


// a plan with general terms on the wide kernels: its own chunking and workspace (clr_batch_set_general)
void general_wide_params(const clr_batch* h, const clr::BatchParams& P, clr::BatchParams& W) {
  W = P;
  const size_t pc = (size_t)h->B * h->gen_nchunk;
  W.nchunk = h->gen_nchunk; W.L = h->gen_L; W.L0 = h->gen_L0;
  W.t = h->t.p; W.diag = h->diag.p; W.y = h->y.p;
  W.t_stride = h->t_stride; W.diag_stride = h->diag_stride; W.y_stride = h->y_stride;
  W.lane_is = 1; W.lane_cs = W.L; W.staged = 0; W.split = 0; W.only_pending = 0;
  W.split_lazy = ((h->summarize_mode < 0 || h->summarize_mode == 2) && W.nchunk > 1 && lazy_eligible(h)) ? 1 : 0;  // (general terms: the strict rule)
  W.coop_prefix = h->coop_prefix == 2 ? 2 : 1;  // (2: the parallel prefix where its workspace exists, else the walk)
  W.J_general = h->J_general;
  W.gen_A = h->gA.p; W.gen_U = h->gU.p; W.gen_V = h->gV.p;
  W.gen_A_stride = h->gA_stride; W.gen_U_stride = h->gU_stride; W.gen_V_stride = h->gV_stride;
  W.elems = h->gen_elems.p; W.starts = h->gen_starts.p;
  W.scan_ws = h->gen_scan_ws_doubles ? h->gen_scan.p : nullptr;
  W.part = h->gen_part.p; W.partx = h->gen_part.p + pc * 2;
  W.cond = h->gen_cond.p; W.egerr = h->gen_cond.p + pc * 3;
  W.flags = h->gen_flags.p; W.flagsx = h->gen_flags.p + pc; W.need_exact = h->gen_flags.p + 2 * pc;
  W.force_exact = (h->force_exact || W.nchunk < 2) ? 1 : 0;
  W.wide_materialize = 0;
}

}  // namespace
