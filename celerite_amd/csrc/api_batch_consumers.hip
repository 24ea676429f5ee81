// celerite_amd/csrc/api_batch_consumers.hip -- C ABI of the batched plans, second part: the consumers of a plan's factor
// and coefficients (clr_batch_get_factor, _solve, _dot_L, _dot, _predict, _predict_var, _predict_var_recurrence,
// _one_step_ahead, _forecast, _predict_terms, _predict_cov, _sample_conditional, _leave_one_out, _grad_mean_weights,
// _fit_mean_weights, _grad_noise_weights, _grad_amplitudes, _periodogram) and the helpers they
// share: the factor and route checks, the frame of one call's device work, prediction points and tiles.
#include "api_internal.h"
#include "clr_bmean_kernels.h"
#include "clr_bnoise_kernels.h"
#include "clr_bamplitude_kernels.h"

#include <functional>
#include <limits>

extern "C" {

// ---- the batched consumers of a plan's factor and coefficients: clr_batch_get_factor, _solve, _dot_L, _dot, _predict

// the factor of the last materialising run, still usable (a lean one is not once its series or coefficients changed);
// `settle`: settle an evaluation in flight first and require a completed run -- all but clr_batch_get_factor
static int require_factor(clr_batch* h, bool settle) {
  int st;
  if ((st = refuse_ragged(h, "the materialised factor and its consumers")) != CLR_OK) return st;
  if (settle && (st = warm_resolve(h, nullptr)) != CLR_OK) return st;
  if (!h->have_factor || (settle && !h->factor_valid))
    return fail(CLR_NOT_COMPUTED, settle ? "no materialising run has been made (clr_batch_enqueue(h, 1))"
                                         : "no materialising run has been made");
  if (h->factor_is_lean && h->factor_inputs_changed)
    return fail(CLR_NOT_COMPUTED, "the lean factor's phi and u are regenerated from the plan's series and coefficients, "
                                  "which were replaced after the materialising run: materialise again");
  return CLR_OK;
}

// the consumers cover celerite terms up to width 64 (`entry`: the refused call)
static int require_celerite_width(const clr_batch* h, const char* entry) {
  if (h->ragged) return refuse_ragged(h, entry);
  if (h->J_general > 0 || h->J > clr::wide_max_width())
    return fail(CLR_UNSUPPORTED, std::string(entry) + " covers celerite-only plans of widths 1..64");
  return CLR_OK;
}

// Where a consumer's route ends on this plan: a narrow plan (widths 1..8) must be chunked; a wide one (widths 9..64) needs
// the wave-per-chunk sweeps' N >= 512, or -- the narrow-only consumers -- is refused with what it takes instead.
struct Route {
  const char* wide_instead = nullptr;  // narrow-only consumers: what a wide plan takes instead
  const char* short_hint = "";         // appended to the wide plan's refusal of a short series
  const char* chunk_hint = "";         // appended to the narrow plan's refusal of an unchunked plan
};
static int require_route(const clr_batch* h, const char* entry, const Route& r = Route()) {
  const std::string e(entry);
  if (h->launch)
    return h->nchunk >= 2 ? CLR_OK : fail(CLR_UNSUPPORTED, e + " needs a chunked plan (N >= 128)" + r.chunk_hint);
  if (r.wide_instead) return fail(CLR_UNSUPPORTED, e + " covers narrow plans (widths 1..8): a wide plan takes " + r.wide_instead);
  if (!clr::wsweep_scan_supported(h->N, h->J)) return fail(CLR_UNSUPPORTED, e + " on a wide plan needs N >= 512" + r.short_hint);
  return CLR_OK;
}

// a narrow consumer's parameters, the times read from the row-major series (lean: one time per step and lane) where the
// evaluation stages them through LDS (solve, dot_L), or always (`row_major`, clr_batch_dot: it must not depend on an
// evaluation having made the role-split summarize's chunk-interleaved copy)
static int consumer_params(clr_batch* h, bool row_major, clr::BatchParams& P) {
  const int st = batch_params(h, 0, P, false);
  if (st != CLR_OK) return st;
  if (row_major || P.staged) { P.t = h->t.p; P.t_stride = h->t_stride; P.lane_is = 1; P.lane_cs = h->L; P.staged = 0; }
  return CLR_OK;
}

// One consumer call's device work, made before it queues anything: every return waits for the stream, so no kernel or
// copy outlives the local buffers (declared before the frame) and host arrays it reads.  start() / stop() time the
// kernels, never the copies, into solve_device_ms; finish() downloads n doubles of `result` into `out` and drains.
//
// The frame also owns the validity rule of the cached factor state -- the chunk maps (bs_M), the forward start states of
// S (pv_S) and the backward start matrices Q (loo_Q), which depend on the factor only and are formed by whichever
// consumer needs them first after a materialising run.  claim(valid), made before the kernels that may rewrite the array
// are queued, returns whether it is formed (the kernels' have_*) and clears its flag; a finish() that succeeds sets every
// claimed flag, any other way out leaves them cleared -- a failed launch or copy must not leave the next consumer
// reading a half-written array.  Besides claim() and finish() only factor_written() (api_internal.h) writes the flags.
struct ConsumerFrame {
  clr_batch* h;
  bool timed = false, drained = false;
  std::vector<bool*> claimed;
  int claim(bool& valid) {
    const int formed = valid ? 1 : 0;
    valid = false;
    claimed.push_back(&valid);
    return formed;
  }
  ~ConsumerFrame() { if (!drained) (void)hipStreamSynchronize(h->stream.get()); }
  hipError_t start() {
    hipError_t r;
    for (clr::Event& e : h->bs_ev)
      if (!e && (r = clr::create_event(e)) != hipSuccess) return r;
    timed = true;
    return hipEventRecord(h->bs_ev[0].get(), h->stream.get());
  }
  hipError_t stop() { return hipEventRecord(h->bs_ev[1].get(), h->stream.get()); }
  int finish(double* out = nullptr, const double* result = nullptr, size_t n = 0) {
    HIP_TRY(hipGetLastError());
    if (out) HIP_TRY(hipMemcpyAsync(out, result, n * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
    drained = true;
    HIP_TRY(hipStreamSynchronize(h->stream.get()));
    float ms = 0.f;
    if (timed) HIP_TRY(hipEventElapsedTime(&ms, h->bs_ev[0].get(), h->bs_ev[1].get()));
    if (timed) h->solve_device_ms = ms;
    for (bool* valid : claimed) *valid = true;
    return CLR_OK;
  }
};

// a narrow consumer's kernels on the chunk-interleaved right-hand sides: the B * nrhs rows of `in` laid out into xT,
// kernels(), and the result they leave in outT back row-major into bs_rm
static void narrow_kernels(clr_batch* h, int nrhs, const double* in, long stride, double* xT, const double* outT,
                           const std::function<void()>& kernels) {
  const long cells = (long)h->L * h->nchunk;
  const int rows = h->B * nrhs;
  clr::launch_relayout(in, stride, xT, cells, rows, h->N, h->L, h->nchunk, 0, h->stream.get());
  kernels();
  clr::launch_relayout_back(outT, cells, h->bs_rm.p, (long)h->N, rows, h->N, h->L, h->nchunk, h->stream.get());
}

// problem p of the plan for the object API's kernels (the batched counterpart of generic_view)
static clr::GenericProblem problem_view(const clr_batch* h, const clr::BatchParams& P, size_t p) {
  clr::GenericProblem g;
  g.N = h->N; g.J = h->J; g.J_real = h->J_real; g.J_comp = h->J_comp; g.J_general = 0;
  g.a_real = P.a_real + p * h->J_real; g.c_real = P.c_real + p * h->J_real;
  g.a_comp = P.a_comp + p * h->J_comp; g.b_comp = P.b_comp + p * h->J_comp;
  g.c_comp = P.c_comp + p * h->J_comp; g.d_comp = P.d_comp + p * h->J_comp;
  g.U = nullptr; g.V = nullptr;
  g.t = h->t.p + p * (size_t)h->t_stride;
  return g;
}

int clr_batch_get_factor(clr_batch* h, int p, double* phi, double* u, double* W, double* D) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if ((st = require_factor(h, false)) != CLR_OK) return st;
  if (p < 0 || p >= h->B) return fail(CLR_INVALID_ARGUMENT, "problem index out of range");
  const size_t N = (size_t)h->N, J = (size_t)h->J, Nm1 = N - 1, cells = (size_t)h->L * h->nchunk;
  ConsumerFrame frame{h};
  const double *fphi, *fu, *fW, *fD;
  if (!h->launch) {  // widths 9..64: already in the reference's storage, problem after problem
    fphi = h->phi.p + p * J * Nm1; fu = h->u.p + p * J * Nm1; fW = h->W.p + p * J * N; fD = h->D.p + p * N;
  } else {
    if ((st = h->fphi.reserve(J * Nm1)) != CLR_OK) return st;
    if ((st = h->fu.reserve(J * Nm1)) != CLR_OK) return st;
    if ((st = h->fW.reserve(J * N)) != CLR_OK) return st;
    if ((st = h->fD.reserve(N)) != CLR_OK) return st;
    if (h->factor_is_lean) {
      // the lean layout holds W and D; phi and u are regenerated from the plan's times and the coefficients in force --
      // which must still be the ones of the materialising run (require_factor)
      clr::BatchParams P;
      if ((st = batch_params(h, 0, P, false)) != CLR_OK) return st;
      h->launch->expand(P, p, h->t.p + (size_t)p * (size_t)h->t_stride, h->fphi.p, h->fu.p, h->fW.p, h->fD.p, h->stream.get());
    } else {
      clr::launch_deinterleave_factor(h->phi.p + p * J * cells, h->u.p + p * J * cells,
                                      h->W.p + p * J * cells, h->D.p + p * cells, h->fphi.p, h->fu.p,
                                      h->fW.p, h->fD.p, h->N, h->J, h->L, h->nchunk, h->stream.get());
    }
    HIP_TRY(hipGetLastError());
    fphi = h->fphi.p; fu = h->fu.p; fW = h->fW.p; fD = h->fD.p;
  }
  if (phi && J * Nm1) HIP_TRY(hipMemcpyAsync(phi, fphi, J * Nm1 * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  if (u && J * Nm1) HIP_TRY(hipMemcpyAsync(u, fu, J * Nm1 * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  if (W) HIP_TRY(hipMemcpyAsync(W, fW, J * N * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  if (D) HIP_TRY(hipMemcpyAsync(D, fD, N * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  return frame.finish();
}

// one launch over every problem of a wide plan (grid.z = problem) on its factor, about `want` chunks per problem
static clr::SweepParams wide_sweep_params(const clr_batch* h, int nrhs, int want) {
  clr::SweepParams P;
  memset(&P, 0, sizeof(P));
  const long N = h->N, J = h->J;
  P.N = h->N; P.J = h->J; P.nrhs = nrhs; P.batch = h->B;
  clr::chunking(h->N - 1, want, &P.L, &P.nchunk);
  P.phi = h->phi.p; P.u = h->u.p; P.W = h->W.p; P.D = h->D.p;
  P.stride_phi = J * (N - 1); P.stride_W = J * N; P.stride_D = N;
  P.stride_in = P.stride_out = nrhs * N;
  return P;
}

// the batched solve's sweeps on a wide plan: chunks per problem about two rounds of the chip's SIMDs over the batch
// (2048 / B, at most the single solver's 1024, at least 2), chunks of at least 64 steps -- shared by clr_batch_solve,
// clr_batch_predict_var and clr_batch_fit_mean_weights
static clr::SweepParams wide_solve_params(const clr_batch* h, int nrhs) {
  int want = std::min(clr::wsweep_chunks(h->N, h->J), std::max(2, 2048 / h->B));
  if (want > (h->N - 1) / 64) want = std::max(1, (h->N - 1) / 64);
  return wide_sweep_params(h, nrhs, want);
}

// the two sweeps of CholeskySolver::solve on `nrhs` right-hand sides per problem, row-major in `in` (problems `stride_in`
// apart): forward into bs_x (undivided), backward into bs_rm [B][nrhs][N]; the workspace in bs_M.  The caller has
// reserved the three for at least nrhs right-hand sides.
static void wide_solve_sweeps(clr_batch* h, clr::SweepParams P, int nrhs, const double* in, long stride_in) {
  P.nrhs = nrhs;
  P.stride_out = (long)nrhs * (long)h->N;
  P.stride_ws = (long)clr::wsweep_workspace_doubles(h->J, P.nchunk, nrhs);
  P.in = in; P.stride_in = stride_in;
  P.out = h->bs_x.p;
  P.backward = 0;
  clr::launch_wsweep_scan(P, h->bs_M.p, h->stream.get());
  P.in = h->bs_x.p; P.stride_in = P.stride_out;
  P.out = h->bs_rm.p;
  P.backward = 1;
  clr::launch_wsweep_scan(P, h->bs_M.p, h->stream.get());
}

// clr_batch_solve on a wide plan (widths 9..64): the factor lies in the reference's storage, problem after problem
// (wide_scan_kernel, MODE 0), and the two sweeps of CholeskySolver::solve are the object API's chunked affine scans
// (wsweep_kernels.hip: one wave per chunk, one lane per column of the chunk's map) launched ONCE for the whole batch --
// grid.z = problem (SweepParams::batch).  Chunks per problem: about two rounds of the chip's SIMDs over the batch
// (2048 / B, at most the single solver's 1024, at least 2).
static int wide_batch_solve(clr_batch* h, int nrhs, const double* b, double* x) {
  int st;
  if ((st = require_celerite_width(h, "clr_batch_solve")) != CLR_OK) return st;
  Route route;
  route.short_hint = " (shorter series: CholeskySolver.solve)";
  if ((st = require_route(h, "clr_batch_solve", route)) != CLR_OK) return st;
  const size_t B = (size_t)h->B, N = (size_t)h->N, R = (size_t)nrhs;
  const clr::SweepParams P = wide_solve_params(h, nrhs);
  const size_t ws = clr::wsweep_workspace_doubles(h->J, P.nchunk, nrhs);
  if ((st = h->bs_M.reserve(B * ws)) != CLR_OK) return st;
  if ((st = h->bs_x.reserve(B * R * N)) != CLR_OK) return st;   // the forward sweep's output (undivided)
  if ((st = h->bs_rm.reserve(B * R * N)) != CLR_OK) return st;  // right-hand sides in, results out
  ConsumerFrame frame{h};
  if (b) HIP_TRY(hipMemcpyAsync(h->bs_rm.p, b, B * R * N * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
  HIP_TRY(frame.start());
  wide_solve_sweeps(h, P, nrhs, b ? h->bs_rm.p : h->y.p, b ? (long)(R * N) : h->y_stride);
  HIP_TRY(frame.stop());
  return frame.finish(x, h->bs_rm.p, B * R * N);  // (x null: the result stays in bs_rm)
}

// the narrow batched solve's buffers for R right-hand sides per problem: the chunk-interleaved right-hand sides and
// solutions, the chunk maps, the offsets and start states -- clr_batch_solve and clr_batch_fit_mean_weights
static int reserve_narrow_solve(clr_batch* h, size_t R) {
  const size_t B = (size_t)h->B, J = (size_t)h->J, nc = (size_t)h->nchunk;
  int st;
  if ((st = h->bs_x.reserve(B * R * (size_t)h->L * nc)) != CLR_OK) return st;
  if ((st = h->bs_M.reserve(B * nc * J * J)) != CLR_OK) return st;
  if ((st = h->bs_off.reserve(B * R * nc * J)) != CLR_OK) return st;
  return h->bs_starts.reserve(B * R * nc * J);
}

// ... and its parameters on those buffers, the chunk maps claimed through the caller's frame (formed by the first solve
// after a materialising run)
static clr::BSolveParams narrow_solve_begin(clr_batch* h, ConsumerFrame& frame, int nrhs) {
  clr::BSolveParams S;
  S.nrhs = nrhs; S.r = 0; S.lean = h->factor_is_lean ? 1 : 0;
  S.have_M = frame.claim(h->bs_M_valid);
  S.xT = h->bs_x.p; S.M = h->bs_M.p; S.off = h->bs_off.p; S.starts = h->bs_starts.p;
  return S;
}

// x == null: the result stays on the device, row-major [B][nrhs][N] in bs_rm (clr_batch_predict)
static int batch_solve_impl(clr_batch* h, int nrhs, const double* b, double* x) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (nrhs < 1) return fail(CLR_INVALID_ARGUMENT, "clr_batch_solve: nrhs >= 1");
  if (!b && nrhs != 1) return fail(CLR_INVALID_ARGUMENT, "clr_batch_solve: b == NULL means the plan's own y (one right-hand side)");
  if ((st = require_factor(h, true)) != CLR_OK) return st;
  if (!h->launch) return wide_batch_solve(h, nrhs, b, x);
  if ((st = require_route(h, "clr_batch_solve")) != CLR_OK) return st;
  clr::BatchParams P;
  if ((st = consumer_params(h, false, P)) != CLR_OK) return st;
  const size_t B = (size_t)h->B, N = (size_t)h->N, R = (size_t)nrhs;
  if ((st = reserve_narrow_solve(h, R)) != CLR_OK) return st;
  if ((st = h->bs_rm.reserve(B * R * N)) != CLR_OK) return st;
  ConsumerFrame frame{h};
  if (b) HIP_TRY(hipMemcpyAsync(h->bs_rm.p, b, B * R * N * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
  HIP_TRY(frame.start());
  const clr::BSolveParams S = narrow_solve_begin(h, frame, nrhs);
  narrow_kernels(h, nrhs, b ? h->bs_rm.p : h->y.p, b ? (long)N : h->y_stride, h->bs_x.p, h->bs_x.p,
                 [&] { h->launch->bsolve(P, S, h->stream.get()); });
  HIP_TRY(frame.stop());
  return frame.finish(x, h->bs_rm.p, B * R * N);
}

int clr_batch_solve(clr_batch* h, int nrhs, const double* b, double* x) {
  if (!x) return fail(CLR_INVALID_ARGUMENT, "clr_batch_solve: an output array");
  return batch_solve_impl(h, nrhs, b, x);
}

// CholeskySolver::dot_L (cholesky.h:409-431; GP.sample draws L z, celerite.py:422-451) for every problem of the plan from
// the factor of its last materialising run.  Narrow plans: the chunked diagonal scan of clr_bdotl_kernels.h on the
// chunk-interleaved factor (either layout), lane = (problem, chunk).  Wide plans (widths 9..64): the factor lies in the
// reference's storage and the object API's wave-per-chunk scan (wsweep_kernels.hip: wdotl_kernel) runs once for the whole
// batch, grid.z = problem; series too short for it: the sequential kernel, problem by problem.
int clr_batch_dot_L(clr_batch* h, int nrhs, const double* z, double* y) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (nrhs < 1 || nrhs > 65535 || !z || !y) return fail(CLR_INVALID_ARGUMENT, "clr_batch_dot_L: 1 <= nrhs <= 65535 (grid.z), z and an output array");
  if ((st = require_factor(h, true)) != CLR_OK) return st;
  if ((st = require_celerite_width(h, "clr_batch_dot_L")) != CLR_OK) return st;
  const size_t B = (size_t)h->B, N = (size_t)h->N, J = (size_t)h->J, R = (size_t)nrhs;
  if ((st = h->bs_rm.reserve(B * R * N)) != CLR_OK) return st;
  ConsumerFrame frame{h};
  HIP_TRY(hipMemcpyAsync(h->bs_rm.p, z, B * R * N * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
  if (!h->launch) {  // wide plans
    if ((st = h->bs_x.reserve(B * R * N)) != CLR_OK) return st;
    HIP_TRY(frame.start());
    if (clr::wdotl_scan_supported(h->N, h->J)) {
      // chunks per problem: about two rounds of the chip's SIMDs over the batch (not a function of nrhs: a right-hand
      // side's result does not depend on how many others ride along)
      clr::SweepParams P = wide_sweep_params(h, nrhs, std::min(clr::wdotl_chunks(h->N), std::max(2, (int)(2048 / B))));
      const size_t ws = R * (size_t)P.nchunk * 3 * J;
      if ((st = h->bs_off.reserve(B * ws)) != CLR_OK) return st;
      P.stride_ws = (long)ws;
      P.in = h->bs_rm.p; P.out = h->bs_x.p;
      clr::launch_wdotl_scan(P, h->bs_off.p, h->stream.get());
    } else {
      for (size_t p = 0; p < B; ++p)
        clr::launch_dot_L(h->N, h->J, nrhs, h->phi.p + p * J * (N - 1), h->u.p + p * J * (N - 1), h->W.p + p * J * N,
                          h->D.p + p * N, h->bs_rm.p + p * R * N, h->bs_x.p + p * R * N, h->stream.get());
    }
    HIP_TRY(frame.stop());
  } else {
    clr::BatchParams P;
    if ((st = consumer_params(h, false, P)) != CLR_OK) return st;
    const size_t cells = (size_t)h->L * h->nchunk;
    if ((st = h->bs_x.reserve(B * R * cells)) != CLR_OK) return st;
    if ((st = h->bs_decay.reserve(B * h->nchunk * J)) != CLR_OK) return st;
    if ((st = h->bs_off.reserve(B * R * h->nchunk * J)) != CLR_OK) return st;
    if ((st = h->bs_starts.reserve(B * R * h->nchunk * J)) != CLR_OK) return st;
    HIP_TRY(frame.start());
    clr::BDotLParams S;
    S.nrhs = nrhs; S.lean = h->factor_is_lean ? 1 : 0;
    S.xT = h->bs_x.p; S.decay = h->bs_decay.p; S.off = h->bs_off.p; S.starts = h->bs_starts.p;
    narrow_kernels(h, nrhs, h->bs_rm.p, (long)N, h->bs_x.p, h->bs_x.p, [&] { h->launch->bdotl(P, S, h->stream.get()); });
    HIP_TRY(frame.stop());
  }
  return frame.finish(y, h->launch ? h->bs_rm.p : h->bs_x.p, B * R * N);  // (bs_x as reserved above)
}

// the constant diagonal of one problem's K for dot: sum a_real + sum a_comp + jitter (cholesky.h:483-485), N copies
__global__ void __launch_bounds__(256) dot_diagonal_kernel(const double* a_real, const double* a_comp, const double* jitter, int JR,
                                                           int JC, double* dg, int N) {
  double sr = 0.0, sc = 0.0;
  for (int j = 0; j < JR; ++j) sr += a_real[j];
  for (int j = 0; j < JC; ++j) sc += a_comp[j];
  const double d = (sr + sc) + jitter[0];
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long)gridDim.x * blockDim.x) dg[n] = d;
}

// CholeskySolver::dot (cholesky.h:441-596; GP.dot, celerite.py:453-489) for every problem of the plan: y_p = K_p z_p with
// K_p given by the plan's resident times and the coefficients in force (diagonal sum a_real + sum a_comp + jitter: no
// observational variance, :483-485) -- no factor, no materialising run.  Narrow plans: the two triangles as chunked
// diagonal scans with the features evaluated on the fly (clr_bdot_kernels.h), lane = (problem, chunk).  Wide plans
// (widths 9..64): the object API's kernels problem by problem (launch_dot_setup + the wave-per-chunk scans of
// wsweep_kernels.hip, or the sequential kernel on short series) on the plan's resident arrays.
int clr_batch_dot(clr_batch* h, int nrhs, const double* z, double* y) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (nrhs < 1 || nrhs > 65535 || !z || !y) return fail(CLR_INVALID_ARGUMENT, "clr_batch_dot: 1 <= nrhs <= 65535 (grid.z), z and an output array");
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;
  if ((st = require_celerite_width(h, "clr_batch_dot")) != CLR_OK) return st;
  clr::BatchParams P;  // (wide plans read its coefficients only)
  if ((st = consumer_params(h, true, P)) != CLR_OK) return st;
  const size_t B = (size_t)h->B, N = (size_t)h->N, J = (size_t)h->J, R = (size_t)nrhs;
  if ((st = h->bs_rm.reserve(B * R * N)) != CLR_OK) return st;
  DevBuf feat, dgb, ws;  // (wide plans: one problem's features, its constant diagonal and the scan's workspace)
  ConsumerFrame frame{h};
  HIP_TRY(hipMemcpyAsync(h->bs_rm.p, z, B * R * N * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
  if (!h->launch) {  // wide plans: problem by problem
    if ((st = feat.reserve(3 * J * N)) != CLR_OK) return st;
    if ((st = dgb.reserve(N)) != CLR_OK) return st;  // (refilled per problem, same stream)
    if ((st = h->bs_x.reserve(B * R * N)) != CLR_OK) return st;
    const bool scan = clr::wdotl_scan_supported(h->N, h->J);
    clr::SweepParams SP;
    memset(&SP, 0, sizeof(SP));
    if (scan) {
      SP.N = h->N; SP.J = h->J; SP.nrhs = nrhs;
      clr::chunking(h->N - 1, clr::wdotl_chunks(h->N), &SP.L, &SP.nchunk);
      if ((st = ws.reserve(R * (size_t)SP.nchunk * 3 * J)) != CLR_OK) return st;
    }
    HIP_TRY(frame.start());
    for (size_t p = 0; p < B; ++p) {
      const clr::GenericProblem g = problem_view(h, P, p);
      double *phi = feat.p, *u = feat.p + J * N, *v = feat.p + 2 * J * N;
      clr::launch_dot_setup(g, phi, u, v, h->stream.get());
      hipLaunchKernelGGL(dot_diagonal_kernel, dim3((unsigned)std::min<size_t>((N + 255) / 256, 1024)), dim3(256), 0, h->stream.get(),
                         g.a_real, g.a_comp, P.jitter + p, h->J_real, h->J_comp, dgb.p, h->N);
      if (scan) {
        SP.phi = phi; SP.u = u;
        SP.in = h->bs_rm.p + p * R * N; SP.out = h->bs_x.p + p * R * N;
        clr::launch_wdot_scan(SP, v, dgb.p, ws.p, h->stream.get());
      } else {
        clr::launch_dot(h->N, h->J, nrhs, phi, u, v, dgb.p, h->bs_rm.p + p * R * N, h->bs_x.p + p * R * N, h->stream.get());
      }
    }
    HIP_TRY(frame.stop());
  } else {
    const size_t cells = (size_t)h->L * h->nchunk;
    if ((st = h->bs_x.reserve(B * R * cells)) != CLR_OK) return st;
    if ((st = h->bs_y.reserve(B * R * cells)) != CLR_OK) return st;
    if ((st = h->bs_decay.reserve(B * h->nchunk * J)) != CLR_OK) return st;
    if ((st = h->bs_off.reserve(B * R * h->nchunk * J)) != CLR_OK) return st;
    if ((st = h->bs_starts.reserve(B * R * h->nchunk * J)) != CLR_OK) return st;
    HIP_TRY(frame.start());
    clr::BDotParams S;
    S.nrhs = nrhs; S.zT = h->bs_x.p; S.yT = h->bs_y.p; S.decay = h->bs_decay.p; S.off = h->bs_off.p; S.starts = h->bs_starts.p;
    narrow_kernels(h, nrhs, h->bs_rm.p, (long)N, h->bs_x.p, h->bs_y.p, [&] { h->launch->bdot(P, S, h->stream.get()); });
    HIP_TRY(frame.stop());
  }
  return frame.finish(y, h->launch ? h->bs_rm.p : h->bs_x.p, B * R * N);  // (bs_x as reserved above)
}

// ---- prediction points, tiles and the epilogues the consumers share

// What every point consumer checks, in this order: the points' arguments (`asks`: what the entry takes, `arrays`: the
// arrays a call with M > 0 needs are there), their stride, the plan's width; *none: M == 0, nothing to do.  With a
// `route` also the factor (settling an evaluation in flight) and where the route ends on this plan; without one they are
// left to the solve the caller begins with (clr_batch_predict).
static int require_points(clr_batch* h, const char* entry, const char* asks, int M, bool arrays, long xs_stride, const Route* route,
                          bool* none) {
  const std::string e(entry);
  int st;
  *none = M == 0;
  if (M < 0 || (M > 0 && !arrays)) return fail(CLR_INVALID_ARGUMENT, e + ": " + asks);
  if (xs_stride != 0 && xs_stride != M) return fail(CLR_INVALID_ARGUMENT, e + ": the points' stride is 0 (shared by all problems) or M");
  if ((st = require_celerite_width(h, entry)) != CLR_OK) return st;
  if (M == 0 || !route) return CLR_OK;
  if ((st = require_factor(h, true)) != CLR_OK) return st;
  return require_route(h, entry, *route);
}

// points per tile: the caller's (clr_batch_set_predict_tile), or the most whose buffers -- `per_point` doubles each --
// fit in 1 GiB; never above `cap` (the solve route: grid.z's 65535) nor M, at least 1
static int predict_tile(const clr_batch* h, int M, size_t per_point, size_t cap = std::numeric_limits<size_t>::max()) {
  const size_t budget = (size_t)1 << 27;  // doubles
  const size_t R = h->predict_tile > 0 ? (size_t)h->predict_tile : std::max<size_t>(1, budget / std::max<size_t>(1, per_point));
  return (int)std::min<size_t>(std::min<size_t>(R, cap), (size_t)M);
}

// Every source's points ascending, for the kernels that walk them with a cursor (clr_batch_predict_var_recurrence,
// clr_batch_forecast, clr_batch_predict_terms): as given where they already are (detected in O(M)), else through an index
// permutation (NaN last; shared points once) that deliver() undoes on the results.  xmax: max |x| (a NaN stays).
struct SortedPoints {
  bool all_sorted = true;
  size_t nsrc = 0, Mm = 0;  // [nsrc][M]: one source shared by all problems, or one per problem
  std::vector<double> xsorted;
  std::vector<int> perm;
  const double* up = nullptr;  // the points to upload
  double xmax = 0.0;
  void sort(const double* xs, size_t sources, size_t M) {
    nsrc = sources; Mm = M;
    std::vector<char> sorted(nsrc, 1);
    for (size_t p = 0; p < nsrc; ++p) {
      const double* x = xs + p * Mm;
      for (size_t m = 1; m < Mm && sorted[p]; ++m) sorted[p] = x[m - 1] <= x[m];
      all_sorted = all_sorted && sorted[p];
    }
    if (!all_sorted) {
      xsorted.assign(xs, xs + nsrc * Mm);
      perm.resize(nsrc * Mm);
      for (size_t p = 0; p < nsrc; ++p) {
        int* pp = perm.data() + p * Mm;
        for (size_t m = 0; m < Mm; ++m) pp[m] = (int)m;
        if (sorted[p]) continue;
        const double* x = xs + p * Mm;
        std::stable_sort(pp, pp + Mm, [x](int a, int b) {
          const double xa = x[a], xb = x[b];
          if (xa != xa) return false;   // NaN last
          if (xb != xb) return true;
          return xa < xb;
        });
        for (size_t m = 0; m < Mm; ++m) xsorted[p * Mm + m] = x[pp[m]];
      }
    }
    up = all_sorted ? xs : xsorted.data();
    for (size_t k = 0; k < nsrc * Mm; ++k) {
      const double a = std::fabs(xs[k]);
      if (a > xmax || a != a) xmax = a;  // (a NaN stays: the library sincos)
    }
  }
  // the phases of the points' features: |d| |x*|, under the plan's own rule
  int xfast(const clr_batch* h) const { return (sel_max(h->dmax, h->floor_dmax) * xmax < CLR_FAST_TRIG_LIMIT) ? 1 : 0; }
  int upload(DevBuf& dxs, hipStream_t s) const { return ::upload(dxs, up, nsrc * Mm, s); }
  // the downloaded results in sorted order -- one [B][G][M] block after the other for those of `outs` that are asked for
  // -- into the caller's arrays, in the caller's order
  void deliver(const double* block, size_t B, size_t G, std::initializer_list<double*> outs) const {
    for (double* out : outs) {
      if (!out) continue;
      if (all_sorted) std::copy(block, block + B * G * Mm, out);
      else
        for (size_t b = 0; b < B; ++b) {
          const int* pp = perm.data() + (nsrc == 1 ? 0 : b * Mm);
          for (size_t g = 0; g < G; ++g) {
            const size_t at = (b * G + g) * Mm;
            for (size_t m = 0; m < Mm; ++m) out[at + pp[m]] = block[at + m];
          }
        }
      block += B * G * Mm;
    }
  }
};

// the constant mean in force plus the conditional mean of the residual, [B][M] (celerite.py:279); under a linear mean
// (clr_batch_set_mean_basis) the residual's alone -- the basis at the points is the caller's
static void add_constant_mean(const clr_batch* h, double* mean, size_t Mm) {
  if (!h->have_mean) return;
  for (size_t p = 0; p < (size_t)h->B; ++p) {
    const double m = h->host_mean[h->mean_stride ? p : 0];
    for (size_t k = 0; k < Mm; ++k) mean[p * Mm + k] = m + mean[p * Mm + k];
  }
}

// the statuses of the evaluation in force; a problem the kernel program refused has no factor either
static int evaluation_statuses(clr_batch* h, std::vector<int>& stat) {
  stat.resize((size_t)h->B);
  const int st = clr_batch_get_results(h, nullptr, nullptr, nullptr, stat.data());
  if (st != CLR_OK) return st;
  mark_refused(h, nullptr, nullptr, nullptr, stat.data());
  return CLR_OK;
}

// ... and the rows of problems without a factor -> NaN (`outs`: an array and its doubles per problem); the statuses into
// `status` where the caller asks for them
static int nan_rows_without_factor(clr_batch* h, std::initializer_list<std::pair<double*, size_t>> outs, int* status = nullptr) {
  std::vector<int> stat;
  const int st = evaluation_statuses(h, stat);
  if (st != CLR_OK) return st;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t b = 0; b < stat.size(); ++b) {
    if (stat[b] == CLR_OK) continue;
    for (const auto& o : outs)
      if (o.first) std::fill(o.first + b * o.second, o.first + (b + 1) * o.second, nan);
  }
  if (status) std::copy(stat.begin(), stat.end(), status);
  return CLR_OK;
}

// CholeskySolver::predict (cholesky.h:599-698; GP.predict's conditional mean, celerite.py:330-420) for every problem of
// the plan: mu*_p(x*) = K_p(x*, t_p) K_p^-1 y_p at M points per problem.  alpha = K^-1 y is the batched solve on the
// materialised factor (either layout, any width <= 64), left on the device; the reference's two passes over the sorted
// prediction points are the object API's chunked diagonal scans (generic_kernels.hip: launch_predict_scan, a parallel
// prefix over chunks of 16 samples + one thread per point) run problem by problem on the plan's resident times and
// coefficients -- they need nothing of the factor.  Unsorted points: the sequential walk (launch_predict).
int clr_batch_predict(clr_batch* h, int M, const double* xs, long xs_stride, double* pred) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  bool none;
  if ((st = require_points(h, "clr_batch_predict", "M >= 0, the points and an output array", M, xs && pred, xs_stride, nullptr, &none)) != CLR_OK || none)
    return st;
  if ((st = batch_solve_impl(h, 1, nullptr, nullptr)) != CLR_OK) return st;  // alpha = K^-1 y -> bs_rm [B][N]
  clr::BatchParams P;
  if ((st = batch_params(h, 0, P, false)) != CLR_OK) return st;
  const size_t B = (size_t)h->B, Mm = (size_t)M, nsrc = xs_stride == 0 ? 1 : B;
  DevBuf dxs, dpred, ws;
  if ((st = dxs.reserve(nsrc * Mm)) != CLR_OK) return st;
  if ((st = dpred.reserve(B * Mm)) != CLR_OK) return st;
  const bool scan_ok = clr::predict_scan_supported(h->N, h->J_real, h->J_comp);
  int pchunk = 0, pL = 0;
  if (scan_ok) {
    clr::chunking(h->N, std::max(1, std::min(h->N / 16, 8192)), &pL, &pchunk);
    if ((st = ws.reserve(clr::predict_workspace_doubles(pchunk, h->J))) != CLR_OK) return st;
  }
  ConsumerFrame frame{h};  // (untimed: solve_device_ms is the solve's)
  if (hipMemcpyAsync(dxs.p, xs, nsrc * Mm * sizeof(double), hipMemcpyHostToDevice, h->stream.get()) != hipSuccess ||
      hipMemsetAsync(dpred.p, 0, B * Mm * sizeof(double), h->stream.get()) != hipSuccess)
    return fail(CLR_HIP_ERROR, "clr_batch_predict: upload failed");
  std::vector<char> sorted(nsrc, 1);
  for (size_t p = 0; p < nsrc; ++p)
    for (size_t m = 1; m < Mm && sorted[p]; ++m) sorted[p] = xs[p * Mm + m - 1] <= xs[p * Mm + m];
  for (size_t p = 0; p < B; ++p) {
    const clr::GenericProblem g = problem_view(h, P, p);
    const double* alpha = h->bs_rm.p + p * (size_t)h->N;
    const double* xp = dxs.p + (xs_stride == 0 ? 0 : p * Mm);
    if (scan_ok && sorted[xs_stride == 0 ? 0 : p]) clr::launch_predict_scan(g, alpha, M, xp, dpred.p + p * Mm, ws.p, pchunk, pL, h->stream.get());
    else clr::launch_predict(g, alpha, M, xp, dpred.p + p * Mm, h->stream.get());
  }
  if (frame.finish(pred, dpred.p, B * Mm) != CLR_OK)
    return fail(CLR_HIP_ERROR, "clr_batch_predict: kernels or the download failed");
  add_constant_mean(h, pred, Mm);
  return CLR_OK;
}

// ---- clr_batch_predict_var: the conditional variance of GP.predict for every problem of the plan

// widths 9..64: the tile's cross-covariances k_p(x*_r - t_{p,n}) row-major [problem][rhs][n] (grid: n, rhs, problem);
// `fast`: the phases stay below CLR_FAST_TRIG_LIMIT (a launch-uniform branch: registers are no concern here)
__global__ void __launch_bounds__(256) predvar_cross_rowmajor_kernel(const double* a_real, const double* c_real, const double* a_comp,
                                                                     const double* b_comp, const double* c_comp, const double* d_comp,
                                                                     int JR, int JC, const double* t, long t_stride, int N,
                                                                     const double* xs, long xs_stride, int nrhs, int fast, double* out) {
  const long n = (long)blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, b = blockIdx.z;
  if (n >= N) return;
  const double tau = xs[b * xs_stride + r] - t[b * t_stride + n];
  const double *ar = a_real + b * JR, *cr = c_real + b * JR, *ac = a_comp + b * JC, *bc = b_comp + b * JC, *cc = c_comp + b * JC,
               *dc = d_comp + b * JC;
  out[(b * nrhs + r) * N + n] = fast ? clr::cross_covariance<true>(ar, cr, JR, ac, bc, cc, dc, JC, tau)
                                     : clr::cross_covariance<false>(ar, cr, JR, ac, bc, cc, dc, JC, tau);
}

// widths 9..64: var = k_p(0) - sum_n x_n^2 / D_n of one (problem, rhs) per workgroup (grid: rhs, problem) in a fixed
// order -- thread i sums the samples i, i + 256, ... in order, then a fixed tree over the 256 threads
__global__ void __launch_bounds__(256) predvar_reduce_kernel(const double* x, const double* D, int N, int nrhs, const double* a_real,
                                                             const double* a_comp, int JR, int JC, double* var, long var_stride) {
  __shared__ double sh[256];
  const long r = blockIdx.x, b = blockIdx.y;
  const double* xp = x + (b * nrhs + r) * N;
  const double* Dp = D + b * N;
  double s = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) s += xp[n] * xp[n] / Dp[n];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double sr = 0.0, sc = 0.0;
    for (int j = 0; j < JR; ++j) sr += a_real[b * JR + j];
    for (int j = 0; j < JC; ++j) sc += a_comp[b * JC + j];
    var[b * var_stride + r] = (sr + sc) - sh[0];
  }
}

// d loglike / d w[b][k] = Phi_k^T K_b^-1 r_b: the batched solve of the residual in `y` on the factor in HBM, left row-major
// in bs_rm, then the projection onto the resident basis (clr_bmean_kernels.h).  The gradient sweeps are not involved: the
// log-likelihood depends on the weights through r alone, d (-1/2 r^T K^-1 r) / d w_k = Phi_k^T K^-1 r.
int clr_batch_grad_mean_weights(clr_batch* h, double* dw, int* status) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (h->mean_K == 0) return fail(CLR_INVALID_ARGUMENT, "clr_batch_grad_mean_weights: no basis is set (clr_batch_set_mean_basis)");
  if (!dw) return fail(CLR_INVALID_ARGUMENT, "clr_batch_grad_mean_weights: an output array");
  if ((st = batch_solve_impl(h, 1, nullptr, nullptr)) != CLR_OK) return st;  // K^-1 r -> bs_rm [B][N]
  const size_t B = (size_t)h->B, K = (size_t)h->mean_K;
  if ((st = h->proj_part.reserve(clr::mean_project_workspace(h->B, h->N, h->mean_K))) != CLR_OK) return st;
  if ((st = h->proj_out.reserve(B * K)) != CLR_OK) return st;
  for (clr::Event& e : h->proj_ev)
    if (!e) HIP_TRY(clr::create_event(e));
  {
    ConsumerFrame frame{h};  // (untimed: solve_device_ms stays the solve's; the projection has its own events)
    HIP_TRY(hipEventRecord(h->proj_ev[0].get(), h->stream.get()));
    // (amplitudes in force: the solve is alpha' = K'^-1 y' of the scaled system, and alpha_y = alpha' / s in data units)
    const bool launched = h->amp_active
        ? clr::launch_mean_project_scaled(h->basis_dev.p, h->basis_stride, h->bs_rm.p, h->amp_s.p, h->mean_K, h->B, h->N,
                                          h->proj_part.p, h->proj_out.p, h->stream.get())
        : clr::launch_mean_project(h->basis_dev.p, h->basis_stride, h->bs_rm.p, h->mean_K, h->B, h->N, h->proj_part.p,
                                   h->proj_out.p, h->stream.get());
    if (!launched)
      return fail(CLR_UNSUPPORTED, "clr_batch_grad_mean_weights: B x N / 4096 workgroups do not fit one launch");
    HIP_TRY(hipEventRecord(h->proj_ev[1].get(), h->stream.get()));
    if ((st = frame.finish(dw, h->proj_out.p, B * K)) != CLR_OK) return st;
  }
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, h->proj_ev[0].get(), h->proj_ev[1].get()));
  h->project_device_ms = ms;
  // the statuses of the evaluation in force; a problem without a factor (or refused by the kernel program): zeros
  std::vector<int> stat;
  if ((st = evaluation_statuses(h, stat)) != CLR_OK) return st;
  for (size_t b = 0; b < B; ++b)
    if (stat[b] != CLR_OK) std::fill(dw + b * K, dw + (b + 1) * K, 0.0);  // (the gradient's quiet semantics)
  if (status) std::copy(stat.begin(), stat.end(), status);
  return CLR_OK;
}

int clr_batch_get_mean_project_ms(const clr_batch* h, double* device_ms) {
  if (device_ms) *device_ms = h->project_device_ms;
  return CLR_OK;
}

int clr_batch_set_predict_tile(clr_batch* h, int points) {
  h->predict_tile = points > 0 ? points : 0;
  return CLR_OK;
}

// The conditional variance of GP.predict (celerite.py:465-470) for every problem of the plan at M points each:
// var = k(0) - k*^T K^-1 k* = k(0) - sum_n z_n^2 / D_n with z = L^-1 k* -- the forward half of a solve per point, on
// right-hand sides formed on the device from the plan's times, the coefficients in force and the points, a tile of
// points at a time.  Narrow plans: clr_bpredvar_kernels.h on the chunk-interleaved factor (either layout), the chunk maps
// shared with clr_batch_solve.  Wide plans (widths 9..64): the cross-covariances row-major, the forward sweep of
// wide_batch_solve (launch_wsweep_scan, backward = 0) and one workgroup per (problem, point) for the quadratic form.
int clr_batch_predict_var(clr_batch* h, int M, const double* xs, long xs_stride, double* var) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  Route route;
  route.short_hint = " (shorter series: GP.predict)";
  bool none;
  if ((st = require_points(h, "clr_batch_predict_var", "M >= 0, the points and an output array", M, xs && var, xs_stride, &route, &none)) != CLR_OK || none)
    return st;
  clr::BatchParams P;  // (wide plans read its coefficients only)
  if ((st = consumer_params(h, false, P)) != CLR_OK) return st;
  const size_t B = (size_t)h->B, N = (size_t)h->N, J = (size_t)h->J, Mm = (size_t)M, nsrc = xs_stride == 0 ? 1 : B;
  // the phases of the cross-covariances: |d| |x* - t| <= max|d| (max|x*| + max|t|), under the plan's own rule
  double xmax = 0.0;
  for (size_t k = 0; k < nsrc * Mm; ++k) {
    const double a = std::fabs(xs[k]);
    if (a > xmax || a != a) xmax = a;  // (a NaN stays: the library sincos)
  }
  const int cross_fast = (sel_max(h->dmax, h->floor_dmax) * (sel_max(h->tmax, h->floor_tmax) + xmax) < CLR_FAST_TRIG_LIMIT) ? 1 : 0;
  DevBuf dxs, dvar;
  if ((st = dxs.reserve(nsrc * Mm)) != CLR_OK) return st;
  if ((st = dvar.reserve(B * Mm)) != CLR_OK) return st;
  if (!h->launch) {  // wide plans
    clr::SweepParams W = wide_solve_params(h, 1);
    const size_t ws_point = clr::wsweep_workspace_doubles(h->J, W.nchunk, 2) - clr::wsweep_workspace_doubles(h->J, W.nchunk, 1);
    const int R = predict_tile(h, M, B * (2 * N + ws_point), 65535);  // (the points ride on grid.y / grid.z)
    const size_t ws = clr::wsweep_workspace_doubles(h->J, W.nchunk, R);
    if ((st = h->bs_M.reserve(B * ws)) != CLR_OK) return st;
    if ((st = h->bs_x.reserve(B * R * N)) != CLR_OK) return st;   // the forward sweep's output (undivided)
    if ((st = h->bs_rm.reserve(B * R * N)) != CLR_OK) return st;  // the tile's cross-covariances
    ConsumerFrame frame{h};
    HIP_TRY(hipMemcpyAsync(dxs.p, xs, nsrc * Mm * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
    HIP_TRY(frame.start());
    for (int m0 = 0; m0 < M; m0 += R) {
      const int nr = std::min(R, M - m0);
      const dim3 cgrid((unsigned)((N + 255) / 256), nr, (unsigned)B);
      hipLaunchKernelGGL(predvar_cross_rowmajor_kernel, cgrid, dim3(256), 0, h->stream.get(), P.a_real, P.c_real, P.a_comp, P.b_comp, P.c_comp, P.d_comp,
                         h->J_real, h->J_comp, h->t.p, h->t_stride, h->N, dxs.p + m0, xs_stride, nr, cross_fast, h->bs_rm.p);
      W.nrhs = nr; W.stride_in = W.stride_out = (long)nr * (long)N;
      W.stride_ws = (long)clr::wsweep_workspace_doubles(h->J, W.nchunk, nr);
      W.in = h->bs_rm.p; W.out = h->bs_x.p; W.backward = 0;
      clr::launch_wsweep_scan(W, h->bs_M.p, h->stream.get());
      hipLaunchKernelGGL(predvar_reduce_kernel, dim3(nr, (unsigned)B), dim3(256), 0, h->stream.get(), h->bs_x.p, h->D.p, h->N, nr,
                         P.a_real, P.a_comp, h->J_real, h->J_comp, dvar.p + m0, (long)M);
    }
    HIP_TRY(frame.stop());
    return frame.finish(var, dvar.p, B * Mm);
  }
  const size_t cells = (size_t)h->L * h->nchunk, nc = (size_t)h->nchunk;
  const int R = predict_tile(h, M, B * (cells + 2 * nc * J), 65535);  // (the points ride on grid.z)
  if ((st = h->bs_x.reserve(B * R * cells)) != CLR_OK) return st;
  if ((st = h->bs_M.reserve(B * nc * J * J)) != CLR_OK) return st;
  if ((st = h->bs_off.reserve(B * R * nc * J)) != CLR_OK) return st;
  if ((st = h->bs_starts.reserve(B * R * nc * J)) != CLR_OK) return st;
  ConsumerFrame frame{h};
  HIP_TRY(hipMemcpyAsync(dxs.p, xs, nsrc * Mm * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
  HIP_TRY(frame.start());
  clr::BPredVarParams S;
  S.lean = h->factor_is_lean ? 1 : 0; S.cross_fast = cross_fast;
  S.have_M = frame.claim(h->bs_M_valid);  // (the batched solve's chunk maps: formed by the first tile unless a consumer has formed them)
  S.xs_stride = xs_stride; S.t = h->t.p; S.t_stride = h->t_stride;
  S.xT = h->bs_x.p; S.M = h->bs_M.p; S.off = h->bs_off.p; S.starts = h->bs_starts.p;
  S.part = h->bs_off.p;  // (the walk has consumed the offsets by the time the forward recurrence writes its sums)
  S.var_stride = (long)M;
  for (int m0 = 0; m0 < M; m0 += R) {
    S.nrhs = std::min(R, M - m0); S.xs = dxs.p + m0; S.var = dvar.p + m0;
    h->launch->bpredvar(P, S, h->stream.get());
    S.have_M = 1;
  }
  HIP_TRY(frame.stop());
  return frame.finish(var, dvar.p, B * Mm);
}

// The cached state of the two matrix recurrences (clr_batch_predict_var_recurrence, clr_batch_predict_terms with `var`):
// its buffers, with those the passes that form Q work in ...
static int reserve_recurrence_state(clr_batch* h) {
  const size_t B = (size_t)h->B, J = (size_t)h->J, nc = (size_t)h->nchunk, NS = J * (J + 1) / 2;
  int st;
  if ((st = h->pv_S.reserve(B * nc * NS)) != CLR_OK) return st;
  if ((st = h->loo_Q.reserve(B * nc * NS)) != CLR_OK) return st;
  if ((st = h->bs_M.reserve(B * nc * J * J)) != CLR_OK) return st;
  if ((st = h->bs_off.reserve(B * nc * J)) != CLR_OK) return st;
  return h->bs_x.reserve(B * (size_t)h->L * nc);  // (read beside by the solve's summarize when it forms the maps)
}
// ... and its claims for one call, with the parameters of the passes that form Q: the start states of S and the start
// matrices Q -- a formed one is not rewritten, and still counts as formed only once this call has finished --, and the
// chunk maps only where this call may write them: with Q, unless a consumer has formed them
static void claim_recurrence_state(clr_batch* h, ConsumerFrame& frame, int lean, int& have_S, int& have_Q, clr::BInvDiagParams& Q) {
  have_S = frame.claim(h->pv_S_valid);
  have_Q = frame.claim(h->loo_Q_valid);
  Q.lean = lean;
  Q.have_M = have_Q ? (h->bs_M_valid ? 1 : 0) : frame.claim(h->bs_M_valid);
  Q.cT = h->bs_x.p; Q.M = h->bs_M.p; Q.Q = h->loo_Q.p; Q.off = h->bs_off.p;
}

// The conditional variance of GP.predict for every problem of a narrow plan at M points each in O((N + M) J^2): the
// factorisation's forward state S and the backward matrix recurrence Q of the leave-one-out diagonal give var(x) in closed
// form (clr_bpredvar_rec_kernels.h) -- one forward and one backward pass over the series per tile of points, O(J^2) per
// point.  The kernels want every problem's points ascending: sorted input is detected in O(M), anything else is sorted
// as an index permutation on the host (NaN last) and the results are scattered back; shared points are sorted once.  The
// chunks' forward start states (pv_S) and backward start matrices (loo_Q, shared with clr_batch_leave_one_out) depend on
// the factor only and are formed by the first tile after a materialising run, the chunk maps under clr_batch_solve's rule.
int clr_batch_predict_var_recurrence(clr_batch* h, int M, const double* xs, long xs_stride, double* var) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  Route route;
  route.wide_instead = "clr_batch_predict_var";
  bool none;
  if ((st = require_points(h, "clr_batch_predict_var_recurrence", "M >= 0, the points and an output array", M, xs && var, xs_stride, &route,
                           &none)) != CLR_OK || none)
    return st;
  clr::BatchParams P;
  if ((st = consumer_params(h, false, P)) != CLR_OK) return st;
  const size_t B = (size_t)h->B, J = (size_t)h->J, Mm = (size_t)M, nsrc = xs_stride == 0 ? 1 : B;
  SortedPoints pts;
  pts.sort(xs, nsrc, Mm);
  std::vector<double> vtmp;  // (sorted points: the download goes straight to the caller's array)
  if (!pts.all_sorted) vtmp.resize(B * Mm);
  const int xfast = pts.xfast(h);
  const int R = predict_tile(h, M, B * (2 * J + 1));  // (per point: u(x), e, left)
  const size_t Rz = (size_t)R;
  DevBuf dxs, dvar, dux, de, dleft;
  if ((st = dvar.reserve(B * Mm)) != CLR_OK) return st;
  if ((st = dux.reserve(B * Rz * J)) != CLR_OK) return st;
  if ((st = de.reserve(B * Rz * J)) != CLR_OK) return st;
  if ((st = dleft.reserve(B * Rz)) != CLR_OK) return st;
  if ((st = reserve_recurrence_state(h)) != CLR_OK) return st;
  ConsumerFrame frame{h};
  if ((st = pts.upload(dxs, h->stream.get())) != CLR_OK) return st;
  HIP_TRY(frame.start());
  clr::BPredVarRecParams S;
  S.lean = h->factor_is_lean ? 1 : 0;
  claim_recurrence_state(h, frame, S.lean, S.have_S, S.have_Q, S.Q);
  S.xs_stride = xs_stride; S.t = h->t.p; S.t_stride = h->t_stride;
  S.S = h->pv_S.p; S.ux = dux.p; S.e = de.p; S.left = dleft.p;
  S.var_stride = (long)M;
  for (int m0 = 0; m0 < M; m0 += R) {
    S.npts = std::min(R, M - m0); S.xs = dxs.p + m0; S.var = dvar.p + m0;
    h->launch->bpredvar_rec(P, S, xfast, h->stream.get());
    S.have_S = S.have_Q = 1;
  }
  HIP_TRY(frame.stop());
  if ((st = frame.finish(pts.all_sorted ? var : vtmp.data(), dvar.p, B * Mm)) != CLR_OK) return st;
  if (!pts.all_sorted) pts.deliver(vtmp.data(), B, 1, {var});
  return CLR_OK;
}

// ---- clr_batch_one_step_ahead, clr_batch_forecast: the causal half of the factor (clr_bfilter_kernels.h)

// z = L^-1 b and D for every problem from the factor of the last materialising run: the forward half of clr_batch_solve
// without its division.  Narrow plans: the solve's summarize and forward walk for the chunks' start states, then
// bfilter_forward_kernel on the chunk-interleaved right-hand sides (the chunk maps under clr_batch_solve's validity rule),
// D de-interleaved beside.  Wide plans (widths 9..64): the forward sweep of wide_batch_solve (launch_wsweep_scan,
// backward = 0), whose output is z; D lies row-major in the factor.
int clr_batch_one_step_ahead(clr_batch* h, int nrhs, const double* b, double* innovation, double* variance, int* status) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (nrhs < 1) return fail(CLR_INVALID_ARGUMENT, "clr_batch_one_step_ahead: nrhs >= 1");
  if (!b && nrhs != 1) return fail(CLR_INVALID_ARGUMENT, "clr_batch_one_step_ahead: b == NULL means the residual in force (one right-hand side)");
  if (!innovation && !variance && !status) return fail(CLR_INVALID_ARGUMENT, "clr_batch_one_step_ahead: at least one output array");
  if ((st = require_celerite_width(h, "clr_batch_one_step_ahead")) != CLR_OK) return st;
  if ((st = require_factor(h, true)) != CLR_OK) return st;
  if ((st = require_route(h, "clr_batch_one_step_ahead")) != CLR_OK) return st;
  const size_t B = (size_t)h->B, N = (size_t)h->N, R = (size_t)nrhs;
  DevBuf dD;  // (narrow plans: D row-major)
  if (innovation || variance) {
    clr::BatchParams P;
    clr::SweepParams W;
    if (h->launch) {
      if ((st = consumer_params(h, false, P)) != CLR_OK) return st;
      if (innovation && (st = reserve_narrow_solve(h, R)) != CLR_OK) return st;
      if (variance && (st = dD.reserve(B * N)) != CLR_OK) return st;
    } else if (innovation) {
      W = wide_solve_params(h, nrhs);
      if ((st = h->bs_M.reserve(B * clr::wsweep_workspace_doubles(h->J, W.nchunk, nrhs))) != CLR_OK) return st;
      if ((st = h->bs_x.reserve(B * R * N)) != CLR_OK) return st;  // the forward sweep's output
    }
    if (innovation && (st = h->bs_rm.reserve(B * R * N)) != CLR_OK) return st;
    ConsumerFrame frame{h};
    hipStream_t s = h->stream.get();
    if (innovation && b) HIP_TRY(hipMemcpyAsync(h->bs_rm.p, b, B * R * N * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(frame.start());
    const double* zdev = nullptr;
    if (innovation && h->launch) {
      const clr::BSolveParams Q = narrow_solve_begin(h, frame, nrhs);
      clr::BFilterParams S{};
      S.nrhs = nrhs; S.lean = Q.lean; S.have_M = Q.have_M;
      S.xT = S.zT = Q.xT; S.M = Q.M; S.off = Q.off; S.starts = Q.starts;
      narrow_kernels(h, nrhs, b ? h->bs_rm.p : h->y.p, b ? (long)N : h->y_stride, h->bs_x.p, h->bs_x.p,
                     [&] { h->launch->bfilter(P, S, 0, s); });
      zdev = h->bs_rm.p;
    } else if (innovation) {
      W.nrhs = nrhs;
      W.stride_out = (long)(R * N);
      W.stride_ws = (long)clr::wsweep_workspace_doubles(h->J, W.nchunk, nrhs);
      W.in = b ? h->bs_rm.p : h->y.p; W.stride_in = b ? (long)(R * N) : h->y_stride;
      W.out = h->bs_x.p;
      W.backward = 0;
      clr::launch_wsweep_scan(W, h->bs_M.p, s);
      zdev = h->bs_x.p;
    }
    const double* Ddev = h->D.p;  // (wide plans: the reference's storage, problem after problem)
    if (variance && h->launch) {
      clr::launch_relayout_back(h->D.p, (long)h->L * h->nchunk, dD.p, (long)N, h->B, h->N, h->L, h->nchunk, s);
      Ddev = dD.p;
    }
    HIP_TRY(frame.stop());
    HIP_TRY(hipGetLastError());
    if (variance) HIP_TRY(hipMemcpyAsync(variance, Ddev, B * N * sizeof(double), hipMemcpyDeviceToHost, s));
    if ((st = frame.finish(innovation, zdev, innovation ? B * R * N : 0)) != CLR_OK) return st;
  }
  return nan_rows_without_factor(h, {{innovation, R * N}, {variance, N}}, status);
}

// The mean and variance at M points per problem given the samples strictly before each (clr_bfilter_kernels.h): the
// residual in force laid out chunk-interleaved once, the chunks' start states of g by the first tile (they follow the
// residual: never kept), those of S (pv_S, shared with clr_batch_predict_var_recurrence, only with `var`) unless formed,
// then one forward pass per tile of sorted points.  Points, sorting and tiles as clr_batch_predict_var_recurrence.
int clr_batch_forecast(clr_batch* h, int M, const double* xs, long xs_stride, double* mean, double* var) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (!mean && !var) return fail(CLR_INVALID_ARGUMENT, "clr_batch_forecast: at least one output array");
  Route route;
  route.wide_instead = "clr_batch_predict / clr_batch_predict_var";
  bool none;
  if ((st = require_points(h, "clr_batch_forecast", "M >= 0 and the points", M, xs != nullptr, xs_stride, &route, &none)) != CLR_OK || none)
    return st;
  clr::BatchParams P;
  if ((st = consumer_params(h, false, P)) != CLR_OK) return st;
  const size_t B = (size_t)h->B, J = (size_t)h->J, Mm = (size_t)M, nsrc = xs_stride == 0 ? 1 : B, nc = (size_t)h->nchunk;
  const size_t NS = J * (J + 1) / 2, nout = (mean ? 1 : 0) + (var ? 1 : 0);
  SortedPoints pts;
  pts.sort(xs, nsrc, Mm);
  const int xfast = pts.xfast(h);
  const int R = predict_tile(h, M, B * J);  // (per point: u(x))
  const size_t Rz = (size_t)R;
  DevBuf dxs, dout, dux;  // dout: mean [B][M] | var [B][M], those asked for
  if ((st = dout.reserve(nout * B * Mm)) != CLR_OK) return st;
  if ((st = dux.reserve(B * Rz * J)) != CLR_OK) return st;
  if (var && (st = h->pv_S.reserve(B * nc * NS)) != CLR_OK) return st;
  if ((st = reserve_narrow_solve(h, 1)) != CLR_OK) return st;
  ConsumerFrame frame{h};
  hipStream_t s = h->stream.get();
  if ((st = pts.upload(dxs, s)) != CLR_OK) return st;
  HIP_TRY(frame.start());
  const clr::BSolveParams Q = narrow_solve_begin(h, frame, 1);
  clr::BFilterParams S{};
  S.nrhs = 1; S.lean = Q.lean; S.have_M = Q.have_M;
  S.have_S = h->pv_S_valid ? 1 : 0;
  if (var && !S.have_S) (void)frame.claim(h->pv_S_valid);  // (formed by the first tile)
  S.xT = Q.xT; S.zT = nullptr; S.M = Q.M; S.off = Q.off; S.starts = Q.starts;
  S.S = h->pv_S.p; S.t = h->t.p; S.t_stride = h->t_stride;
  S.xs_stride = xs_stride; S.ux = dux.p; S.out_stride = (long)M;
  double* dmean = mean ? dout.p : nullptr;
  double* dvar = var ? dout.p + (mean ? B * Mm : 0) : nullptr;
  const long cells = (long)h->L * h->nchunk;
  clr::launch_relayout(h->y.p, h->y_stride, h->bs_x.p, cells, h->B, h->N, h->L, h->nchunk, 0, s);
  for (int m0 = 0; m0 < M; m0 += R) {
    S.npts = std::min(R, M - m0); S.xs = dxs.p + m0;
    S.mean = dmean ? dmean + m0 : nullptr; S.var = dvar ? dvar + m0 : nullptr;
    h->launch->bfilter(P, S, xfast, s);
    S.have_g = S.have_M = 1;
    if (var) S.have_S = 1;
  }
  HIP_TRY(frame.stop());
  std::vector<double> tmp(nout * B * Mm);
  if ((st = frame.finish(tmp.data(), dout.p, nout * B * Mm)) != CLR_OK) return st;
  pts.deliver(tmp.data(), B, 1, {mean, var});
  if (mean) add_constant_mean(h, mean, Mm);  // (as clr_batch_predict)
  return nan_rows_without_factor(h, {{mean, Mm}, {var, Mm}});
}

// ---- clr_batch_predict_terms: the posterior of every group of kernel terms (clr_bterms_kernels.h)

// The mean k_g*^T K^-1 r and the variance k_g(0) - k_g*^T K^-1 k_g* of G groups of coefficient terms at M points per
// problem.  With `mean`: alpha = K^-1 r by the batched solve (left on the device), laid out chunk-interleaved once, the
// chunks' start states of p and b by the first tile (they follow the residual: never kept).  With `var`: the start states
// of S (pv_S) and Q (loo_Q) under the rules of clr_batch_predict_var_recurrence -- a mean-only call touches neither.
// Points, sorting and tiles as clr_batch_forecast; the per-point buffers grow with G.  No mean is added: it belongs to no
// term.
int clr_batch_predict_terms(clr_batch* h, int M, const double* xs, long xs_stride, int G, const unsigned char* groups,
                            double* mean, double* var) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (G < 1 || !groups) return fail(CLR_INVALID_ARGUMENT, "clr_batch_predict_terms: G >= 1 and the groups");
  if (!mean && !var) return fail(CLR_INVALID_ARGUMENT, "clr_batch_predict_terms: at least one output array");
  const int T = h->J_real + h->J_comp;
  for (size_t k = 0; k < (size_t)G * T; ++k)
    if (groups[k] > 1) return fail(CLR_INVALID_ARGUMENT, "clr_batch_predict_terms: a group is 0 or 1 per coefficient term");
  Route route;
  route.wide_instead = "clr_batch_predict / clr_batch_predict_var for the full kernel";
  route.chunk_hint = ", as clr_batch_predict on a narrow plan does";
  bool none;
  if ((st = require_points(h, "clr_batch_predict_terms", "M >= 0 and the points", M, xs != nullptr, xs_stride, &route, &none)) != CLR_OK || none)
    return st;
  if (mean && (st = batch_solve_impl(h, 1, nullptr, nullptr)) != CLR_OK) return st;  // alpha = K^-1 r -> bs_rm [B][N]
  clr::BatchParams P;
  if ((st = consumer_params(h, false, P)) != CLR_OK) return st;
  const size_t B = (size_t)h->B, J = (size_t)h->J, Mm = (size_t)M, Gg = (size_t)G, nsrc = xs_stride == 0 ? 1 : B;
  const size_t nc = (size_t)h->nchunk, nout = (mean ? 1 : 0) + (var ? 1 : 0);
  const size_t cells = (size_t)h->L * nc;
  // a group's rows: a real term its one row, a complex term its cos and its sin row
  std::vector<unsigned> rowmask(Gg, 0u);
  for (size_t g = 0; g < Gg; ++g)
    for (int k = 0; k < T; ++k) {
      if (!groups[g * T + k]) continue;
      if (k < h->J_real) rowmask[g] |= 1u << k;
      else rowmask[g] |= 3u << (h->J_real + 2 * (k - h->J_real));
    }
  SortedPoints pts;
  pts.sort(xs, nsrc, Mm);
  const int xfast = pts.xfast(h);
  const int R = predict_tile(h, M, B * (2 * J + (var ? Gg * (J + 1) : 0)));  // (per point: u(x), v(x); e and left per group)
  const size_t Rz = (size_t)R;
  DevBuf dxs, dout, dux, dvx, de, dleft, dbstart;  // dout: mean [B][G][M] | var [B][G][M], those asked for
  clr::Buffer<unsigned> dmask;
  if ((st = dout.reserve(nout * B * Gg * Mm)) != CLR_OK) return st;
  if ((st = dux.reserve(B * Rz * J)) != CLR_OK) return st;
  if ((st = dvx.reserve(B * Rz * J)) != CLR_OK) return st;
  if ((st = dmask.reserve(Gg)) != CLR_OK) return st;
  if (mean) {
    if ((st = h->bs_x.reserve(B * cells)) != CLR_OK) return st;
    if ((st = h->bs_decay.reserve(B * nc * J)) != CLR_OK) return st;
    if ((st = h->bs_off.reserve(B * nc * J)) != CLR_OK) return st;
    if ((st = h->bs_starts.reserve(B * nc * J)) != CLR_OK) return st;
    if ((st = dbstart.reserve(B * nc * J)) != CLR_OK) return st;
  }
  if (var) {
    if ((st = de.reserve(B * Rz * Gg * J)) != CLR_OK) return st;
    if ((st = dleft.reserve(B * Rz * Gg)) != CLR_OK) return st;
    if ((st = reserve_recurrence_state(h)) != CLR_OK) return st;
  }
  const double solve_ms = mean ? h->solve_device_ms : 0.0;  // (the solve above: reported with this frame's kernels)
  ConsumerFrame frame{h};
  hipStream_t s = h->stream.get();
  if ((st = pts.upload(dxs, s)) != CLR_OK) return st;
  HIP_TRY(hipMemcpyAsync(dmask.p, rowmask.data(), Gg * sizeof(unsigned), hipMemcpyHostToDevice, s));
  HIP_TRY(frame.start());
  clr::BTermsParams S{};
  S.G = G; S.lean = h->factor_is_lean ? 1 : 0;
  S.xs_stride = xs_stride; S.rowmask = dmask.p;
  S.ux = dux.p; S.vx = dvx.p; S.e = de.p; S.left = dleft.p; S.out_stride = (long)M;
  if (mean) {  // the series of alpha chunk-interleaved, once per call
    clr::launch_relayout(h->bs_rm.p, (long)h->N, h->bs_x.p, (long)cells, h->B, h->N, h->L, h->nchunk, 0, s);
    S.aT = h->bs_x.p;
    S.pb.nrhs = 1; S.pb.zT = h->bs_x.p; S.pb.yT = h->bs_x.p; S.pb.decay = h->bs_decay.p; S.pb.off = h->bs_off.p;
    S.pstart = h->bs_starts.p; S.bstart = dbstart.p;
  }
  if (var) {
    // (with `mean` the chunk maps are the solve's and bs_x holds alpha: the summarize beside them is not run)
    claim_recurrence_state(h, frame, S.lean, S.have_S, S.have_Q, S.Q);
    S.t = h->t.p; S.t_stride = h->t_stride; S.S = h->pv_S.p;
  }
  double* dmean = mean ? dout.p : nullptr;
  double* dvar = var ? dout.p + (mean ? B * Gg * Mm : 0) : nullptr;
  for (int m0 = 0; m0 < M; m0 += R) {
    S.npts = std::min(R, M - m0); S.xs = dxs.p + m0;
    S.mean = dmean ? dmean + m0 : nullptr; S.var = dvar ? dvar + m0 : nullptr;
    h->launch->bterms(P, S, xfast, s);
    S.have_pb = 1;
    if (var) S.have_S = S.have_Q = 1;
  }
  HIP_TRY(frame.stop());
  std::vector<double> tmp(nout * B * Gg * Mm);
  if ((st = frame.finish(tmp.data(), dout.p, nout * B * Gg * Mm)) != CLR_OK) return st;
  h->solve_device_ms += solve_ms;
  pts.deliver(tmp.data(), B, Gg, {mean, var});
  return nan_rows_without_factor(h, {{mean, Gg * Mm}, {var, Gg * Mm}});
}

// ---- clr_batch_predict_cov, clr_batch_sample_conditional: the joint posterior at the points (clr_bcond_kernels.h)

int clr_batch_set_conditional_tile(clr_batch* h, int problems) {
  h->conditional_tile = problems > 0 ? problems : 0;
  return CLR_OK;
}

// problems b0 .. b0 + nb - 1 of a narrow plan as a plan of their own for a factor consumer's kernels: the factor, the
// times and the coefficients of the slice (what make_slots, the lanes' times and load_problem read)
static clr::BatchParams problem_slice(const clr_batch* h, clr::BatchParams P, size_t b0, int nb) {
  const size_t J = (size_t)h->J, cells = (size_t)h->L * h->nchunk, JR = (size_t)h->J_real, JC = (size_t)h->J_comp;
  P.B = nb;
  P.W += b0 * J * cells; P.D += b0 * cells;
  if (P.phi) P.phi += b0 * J * cells;
  if (P.u) P.u += b0 * J * cells;
  P.t += b0 * (size_t)P.t_stride;
  P.a_real += b0 * JR; P.c_real += b0 * JR;
  P.a_comp += b0 * JC; P.b_comp += b0 * JC; P.c_comp += b0 * JC; P.d_comp += b0 * JC;
  P.jitter += b0;
  return P;
}

// Both entries: `cov` [B][M][M] (clr_batch_predict_cov) or `draws` [B][size][M] from `normals` (clr_batch_sample_conditional).
// The points ascending through SortedPoints; the start states of S (pv_S) and Q (loo_Q) under the rules of
// clr_batch_predict_var_recurrence, the solve's chunk maps read where they are formed; then a tile of PROBLEMS at a time --
// a problem needs all its points at once: about M (J^2 + 4 J) doubles of generators and transports plus M^2 (the
// covariance) or 2 size M (normals, draws) each, as many problems per tile as fit the 1 GiB of predict_tile's automatic
// choice (clr_batch_set_conditional_tile: the caller's).  A single problem that does not fit: the allocation's status.
// The device time is the kernels' of every tile, never the copies'.
static int conditional_impl(clr_batch* h, const char* entry, int M, const double* xs, long xs_stride, int size, const double* normals,
                            double regularize, double min_pivot, double* cov, double* draws, int* status) {
  int st;
  const std::string e(entry);
  Route route;
  route.wide_instead = "clr_batch_predict / clr_batch_predict_var, point by point";
  bool none;
  if ((st = require_points(h, entry, cov ? "M >= 0, the points and an output array" : "M >= 0, the points, the normals and an output array", M,
                           xs && (cov || (normals && draws)), xs_stride, &route, &none)) != CLR_OK || none)
    return st;
  clr::BatchParams P;
  if ((st = consumer_params(h, false, P)) != CLR_OK) return st;
  const size_t B = (size_t)h->B, J = (size_t)h->J, Mm = (size_t)M, nsrc = xs_stride == 0 ? 1 : B, nc = (size_t)h->nchunk;
  const size_t NS = J * (J + 1) / 2, Sz = (size_t)size, out_pp = cov ? Mm * Mm : Sz * Mm;
  SortedPoints pts;
  pts.sort(xs, nsrc, Mm);
  if (pts.xmax != pts.xmax) return fail(CLR_INVALID_ARGUMENT, e + ": a point is NaN");
  const int xfast = pts.xfast(h);
  // per problem: u(x) / r, e, left, var, T, the chunks' transports and counts; omega, sqrt(d); the output (and the normals)
  const size_t per_problem = Mm * (J * J + 3 * J + 3) + nc * (J * J + 1) + (cov ? Mm * Mm : 2 * Sz * Mm);
  const size_t budget = (size_t)1 << 27;  // doubles (predict_tile's)
  const size_t want = h->conditional_tile > 0 ? (size_t)h->conditional_tile : std::max<size_t>(1, budget / per_problem);
  const size_t Bt = std::min<size_t>(std::min<size_t>(want, B), 65535);  // (the problems ride on grid.y)
  DevBuf dxs, dr, de, dleft, dvar, dT, dE, dout, dsd, dom, dnorm;
  clr::Buffer<int> down, dstat;
  if ((st = dr.reserve(Bt * Mm * J)) != CLR_OK) return st;
  if ((st = de.reserve(Bt * Mm * J)) != CLR_OK) return st;
  if ((st = dleft.reserve(Bt * Mm)) != CLR_OK) return st;
  if ((st = dvar.reserve(Bt * Mm)) != CLR_OK) return st;
  if ((st = dT.reserve(Bt * Mm * J * J)) != CLR_OK) return st;
  if ((st = dE.reserve(Bt * nc * J * J)) != CLR_OK) return st;
  if ((st = down.reserve(Bt * nc)) != CLR_OK) return st;
  if ((st = dout.reserve(Bt * out_pp)) != CLR_OK) return st;
  if (!cov) {
    if ((st = dsd.reserve(Bt * Mm)) != CLR_OK) return st;
    if ((st = dom.reserve(Bt * Mm * J)) != CLR_OK) return st;
    if ((st = dnorm.reserve(Bt * Sz * Mm)) != CLR_OK) return st;
    if ((st = dstat.reserve(B)) != CLR_OK) return st;
  }
  if ((st = reserve_recurrence_state(h)) != CLR_OK) return st;
  // the normals in the points' ascending order
  std::vector<double> nsorted, block;
  if (!cov && !pts.all_sorted) {
    nsorted.resize(B * Sz * Mm);
    for (size_t b = 0; b < B; ++b) {
      const int* pp = pts.perm.data() + (nsrc == 1 ? 0 : b * Mm);
      for (size_t s = 0; s < Sz; ++s) {
        const size_t at = (b * Sz + s) * Mm;
        for (size_t m = 0; m < Mm; ++m) nsorted[at + m] = normals[at + pp[m]];
      }
    }
    normals = nsorted.data();
  }
  if (!pts.all_sorted) block.resize(cov ? Bt * out_pp : B * out_pp);
  std::vector<int> fstat(B, 0);
  double total_ms = 0.0;
  {
    ConsumerFrame frame{h};
    hipStream_t s = h->stream.get();
    if ((st = pts.upload(dxs, s)) != CLR_OK) return st;
    clr::BPredVarRecParams V{};
    V.lean = h->factor_is_lean ? 1 : 0;
    const int have_M_before = h->bs_M_valid ? 1 : 0;
    claim_recurrence_state(h, frame, V.lean, V.have_S, V.have_Q, V.Q);
    clr::BCondParams S{};
    S.have_M = V.have_Q ? have_M_before : 1;  // (formed beside Q unless a consumer had formed them)
    V.npts = M; V.xs_stride = xs_stride; V.t_stride = h->t_stride; V.ux = dr.p; V.e = de.p; V.left = dleft.p; V.var = dvar.p; V.var_stride = (long)M;
    S.npts = M; S.lean = V.lean; S.size = size; S.xs_stride = xs_stride; S.t_stride = h->t_stride;
    S.r = dr.p; S.e = de.p; S.T = dT.p; S.E = dE.p; S.own = down.p;
    S.cov = cov ? dout.p : nullptr; S.draws = cov ? nullptr : dout.p;
    S.regularize = regularize; S.min_pivot = min_pivot; S.sd = dsd.p; S.omega = dom.p; S.normals = dnorm.p;
    for (size_t b0 = 0; b0 < B; b0 += Bt) {
      const size_t nb = std::min(Bt, B - b0);
      const clr::BatchParams Pt = problem_slice(h, P, b0, (int)nb);
      V.xs = S.xs = dxs.p + (xs_stride == 0 ? 0 : b0 * Mm);
      V.t = S.t = h->t.p + b0 * (size_t)h->t_stride;
      V.S = h->pv_S.p + b0 * nc * NS;
      S.Q = h->loo_Q.p + b0 * nc * NS;
      S.M = h->bs_M.p + b0 * nc * J * J;
      S.status = cov ? nullptr : dstat.p + b0;
      if (!cov) HIP_TRY(hipMemcpyAsync(dnorm.p, normals + b0 * out_pp, nb * out_pp * sizeof(double), hipMemcpyHostToDevice, s));
      if (b0 == 0) {  // the start states of the whole plan, unless formed
        HIP_TRY(frame.start());
        clr::BPredVarRecParams V0 = V;
        V0.t = h->t.p; V0.S = h->pv_S.p;
        h->launch->bcond(P, V0, S, 0, xfast, s);
        V.have_S = V.have_Q = 1;
      } else {
        HIP_TRY(hipEventRecord(h->bs_ev[0].get(), s));
      }
      h->launch->bcond(Pt, V, S, cov ? 1 : 2, xfast, s);
      HIP_TRY(frame.stop());
      HIP_TRY(hipGetLastError());
      double* dst = pts.all_sorted ? (cov ? cov : draws) + b0 * out_pp : block.data() + (cov ? 0 : b0 * out_pp);
      HIP_TRY(hipMemcpyAsync(dst, dout.p, nb * out_pp * sizeof(double), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, h->bs_ev[0].get(), h->bs_ev[1].get()));
      total_ms += ms;
      if (cov && !pts.all_sorted) {  // both axes back to the caller's order
        for (size_t b = 0; b < nb; ++b) {
          const int* pp = pts.perm.data() + (nsrc == 1 ? 0 : (b0 + b) * Mm);
          const double* src = block.data() + b * out_pp;
          double* out = cov + (b0 + b) * out_pp;
          for (size_t i = 0; i < Mm; ++i)
            for (size_t j = 0; j < Mm; ++j) out[(size_t)pp[i] * Mm + pp[j]] = src[i * Mm + j];
        }
      }
    }
    if (!cov) HIP_TRY(hipMemcpyAsync(fstat.data(), dstat.p, B * sizeof(int), hipMemcpyDeviceToHost, s));
    if ((st = frame.finish()) != CLR_OK) return st;
    h->solve_device_ms = total_ms;
  }
  if (!cov && !pts.all_sorted) pts.deliver(block.data(), B, Sz, {draws});
  std::vector<int> estat(B, 0);
  if ((st = nan_rows_without_factor(h, {{cov ? cov : draws, out_pp}}, estat.data())) != CLR_OK) return st;
  if (!cov) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t b = 0; b < B; ++b) {
      if (estat[b] == CLR_OK && fstat[b] != 0) {  // refused by the pivot rule
        estat[b] = CLR_NOT_POSITIVE_DEFINITE;
        std::fill(draws + b * out_pp, draws + (b + 1) * out_pp, nan);
      }
    }
    if (status) std::copy(estat.begin(), estat.end(), status);
  }
  return CLR_OK;
}

// The posterior covariance of the latent process between M points per problem (GP.predict(..., return_cov=True),
// celerite.py:283-291, without its N x M solve): C_ij = r_j^T T_{j-1} ... T_i e_i from the factor's two matrix
// recurrences and the transports between the points, O((N + M J) J^2 + M^2 J^2) per problem.
int clr_batch_predict_cov(clr_batch* h, int M, const double* xs, long xs_stride, double* cov) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  return conditional_impl(h, "clr_batch_predict_cov", M, xs, xs_stride, 0, nullptr, 0.0, 0.0, cov, nullptr, nullptr);
}

// Joint draws of the latent process at M points per problem given the data, the zero-mean part (GP.sample_conditional,
// celerite.py:327-332, without its dense covariance and its O(M^3) factorisation): draws = L diag(d)^1/2 n with
// C + regularize I = L diag(d) L^T by the celerite recurrence over the points, O((N + M J) J^2) per problem plus
// O(M J^2) per draw.  The mean is clr_batch_predict's and is the caller's to add.
int clr_batch_sample_conditional(clr_batch* h, int M, const double* xs, long xs_stride, int size, const double* normals,
                                 double regularize, double min_pivot, double* draws, int* status) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (size < 1) return fail(CLR_INVALID_ARGUMENT, "clr_batch_sample_conditional: size >= 1");
  if (!std::isfinite(min_pivot) || min_pivot < 0.0 || min_pivot >= 1.0)
    return fail(CLR_INVALID_ARGUMENT, "clr_batch_sample_conditional: min_pivot is finite and in [0, 1)");
  if (!std::isfinite(regularize) || regularize < 0.0)
    return fail(CLR_INVALID_ARGUMENT, "clr_batch_sample_conditional: regularize is finite and not negative");
  if (M > 0 && !draws) return fail(CLR_INVALID_ARGUMENT, "clr_batch_sample_conditional: M >= 0, the points, the normals and an output array");
  return conditional_impl(h, "clr_batch_sample_conditional", M, xs, xs_stride, size, normals, regularize, min_pivot, nullptr, draws, status);
}

// ---- clr_batch_leave_one_out: diag(K^-1), K^-1 r and the leave-one-out log predictive density of every problem

// widths 9..64: diag(K^-1) of one problem per wave from the factor in the reference's storage, sequential in n (the
// recurrence of clr_binvdiag_kernels.h: Q_n = P - u v^T - v u^T + c_n u u^T, c_n = 1 / D_n + g^T Q_{n+1} g).  Lane k holds
// column k of Q (JP doubles, the width padded with zeros); (Q g)_k is lane-local by symmetry, s one wave reduction; the
// steps' phi, g = phi o W and u are staged through LDS a tile of TILE samples at a time, v per step.
extern "C++" {
template <int JP>
__global__ void __launch_bounds__(64) wide_invdiag_kernel(const double* __restrict__ phi, const double* __restrict__ u,
                                                          const double* __restrict__ W, const double* __restrict__ D, int N, int J,
                                                          double* __restrict__ out) {
  constexpr int TILE = 16;
  __shared__ double s_phi[TILE][JP], s_g[TILE][JP], s_u[TILE][JP], s_v[2][JP], s_d[TILE];
  const long b = blockIdx.x;
  const int lane = threadIdx.x;
  const bool live = lane < JP;
  const int k = live ? lane : 0;
  const double *php = phi + b * (long)J * (N - 1), *up = u + b * (long)J * (N - 1), *Wp = W + b * (long)J * N, *Dp = D + b * (long)N;
  double* op = out + b * (long)N;
  double Q[JP];
#pragma unroll
  for (int j = 0; j < JP; ++j) Q[j] = 0.0;
  for (int hi = N; hi > 0; hi -= TILE) {
    const int lo = hi > TILE ? hi - TILE : 0, cnt = hi - lo;
    __syncthreads();  // (the previous tile has been read)
    for (int e = lane; e < cnt * JP; e += 64) {
      const int i = e / JP, j = e % JP, n = lo + i;
      double ph = 0.0, ww = 0.0, uu = 0.0;
      if (j < J) {
        ww = Wp[(long)n * J + j];
        if (n < N - 1) ph = php[(long)n * J + j];   // (the last sample's transition is 0)
        if (n >= 1) uu = up[(long)(n - 1) * J + j];  // (u_(:, n-1) = U~(t_n); U~(t_0) enters no entry)
      }
      s_phi[i][j] = ph; s_g[i][j] = ph * ww; s_u[i][j] = uu;
    }
    if (lane < cnt) s_d[lane] = Dp[lo + lane];
    __syncthreads();
    for (int i = cnt - 1; i >= 0; --i) {
      double qg = 0.0;
#pragma unroll
      for (int j = 0; j < JP; ++j) qg = fma(Q[j], s_g[i][j], qg);
      const double phk = s_phi[i][k], uk = s_u[i][k];
      double s = live ? s_g[i][k] * qg : 0.0;
      const double vk = phk * qg;
      if (live) s_v[i & 1][k] = vk;
#pragma unroll
      for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w, 64);
      const double cn = 1.0 / s_d[i] + s;
      if (lane == 0) op[lo + i] = cn;
      __syncthreads();
      {
#pragma clang fp contract(off)  // (entries (j, k) and (k, j) round alike: Q stays symmetric to the bit)
#pragma unroll
        for (int j = 0; j < JP; ++j) {
          const double pj = s_phi[i][j], uj = s_u[i][j], vj = s_v[i & 1][j];
          Q[j] = (pj * phk) * Q[j] - (uj * vk + vj * uk) + cn * (uj * uk);
        }
      }
    }
  }
}
}  // extern "C++"

// sum_n -1/2 log(2 pi / c_n) - 1/2 alpha_n^2 / c_n of one problem per workgroup in a fixed order -- thread i sums the
// samples i, i + 256, ... in order, then a fixed tree over the 256 threads (batch.leave_one_out_from does the same on the host)
__global__ void __launch_bounds__(256) loo_reduce_kernel(const double* __restrict__ c, const double* __restrict__ alpha, int N,
                                                         double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double sh[256];
  const long b = blockIdx.x;
  const double *cp = c + b * N, *ap = alpha + b * N;
  double s = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) {
    const double cn = cp[n], an = ap[n];
    s += -0.5 * log(6.283185307179586 / cn) - 0.5 * an * an / cn;
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[b] = sh[0];
}

int clr_batch_get_leave_one_out_ms(const clr_batch* h, double* diag_ms, double* solve_ms, double* reduce_ms) {
  if (diag_ms) *diag_ms = h->loo_diag_ms;
  if (solve_ms) *solve_ms = h->loo_solve_ms;
  if (reduce_ms) *reduce_ms = h->loo_reduce_ms;
  return CLR_OK;
}

// c = diag(K^-1), alpha = K^-1 r and sum_n log p(y_n | y_-n) = sum_n -1/2 log(2 pi / c_n) - 1/2 alpha_n^2 / c_n for every
// problem from the factor of the last materialising run.  c: narrow plans, the backward matrix recurrence of
// clr_binvdiag_kernels.h on the chunk-interleaved factor (either layout), the chunk maps shared with clr_batch_solve under
// its validity rule; wide plans (widths 9..64), one wave per problem, sequential in n (wide_invdiag_kernel).  alpha: the
// batched solve of the residual in force, left row-major in bs_rm.  The sum: one workgroup per problem, no atomics.
// The device parts, behind the caller's checks: c into loo_c (`need_c`) and alpha into bs_rm (`need_alpha`), both row-major
// [B][N] and left on the device -- clr_batch_grad_noise_weights projects them there; the host arrays that are not null
// are filled, the sum only when loo_logpdf is asked for.
static int leave_one_out_device(clr_batch* h, bool need_c, bool need_alpha, double* kinv_diag, double* alpha, double* loo_logpdf) {
  int st;
  const size_t B = (size_t)h->B, N = (size_t)h->N, J = (size_t)h->J;
  for (clr::Event& e : h->loo_ev)
    if (!e) HIP_TRY(clr::create_event(e));
  h->loo_diag_ms = h->loo_solve_ms = h->loo_reduce_ms = 0.0;
  float ms = 0.f;
  if (need_c) {
    if ((st = h->loo_c.reserve(B * N)) != CLR_OK) return st;
    clr::BatchParams P;
    if (h->launch) {
      if ((st = consumer_params(h, false, P)) != CLR_OK) return st;
      const size_t nc = (size_t)h->nchunk;
      if ((st = h->bs_x.reserve(B * (size_t)h->L * nc)) != CLR_OK) return st;
      if ((st = h->bs_M.reserve(B * nc * J * J)) != CLR_OK) return st;
      if ((st = h->bs_off.reserve(B * nc * J)) != CLR_OK) return st;
      if ((st = h->loo_Q.reserve(B * nc * (J * (J + 1) / 2))) != CLR_OK) return st;
    }
    ConsumerFrame frame{h};  // (untimed: the parts have their own events)
    hipStream_t s = h->stream.get();
    HIP_TRY(hipEventRecord(h->loo_ev[0].get(), s));
    if (h->launch) {
      clr::BInvDiagParams S;
      S.lean = h->factor_is_lean ? 1 : 0;
      S.have_M = frame.claim(h->bs_M_valid);  // (the batched solve's chunk maps: formed here unless a consumer has formed them)
      (void)frame.claim(h->loo_Q_valid);      // (rewritten: the offsets, then the start matrices -- as clr_batch_predict_var_recurrence reads them)
      S.cT = h->bs_x.p; S.M = h->bs_M.p; S.Q = h->loo_Q.p; S.off = h->bs_off.p;
      h->launch->binvdiag(P, S, s);
      clr::launch_relayout_back(h->bs_x.p, (long)h->L * h->nchunk, h->loo_c.p, (long)N, h->B, h->N, h->L, h->nchunk, s);
    } else {
      const int JP = clr::wide_padded_width(h->J);
#define CLR_GO(WIDTH) hipLaunchKernelGGL((wide_invdiag_kernel<WIDTH>), dim3((unsigned)B), dim3(64), 0, s, h->phi.p, h->u.p, h->W.p, h->D.p, h->N, h->J, h->loo_c.p)
      if (JP == 16) CLR_GO(16); else if (JP == 32) CLR_GO(32); else CLR_GO(64);
#undef CLR_GO
    }
    HIP_TRY(hipEventRecord(h->loo_ev[1].get(), s));
    if ((st = frame.finish(kinv_diag, h->loo_c.p, B * N)) != CLR_OK) return st;
    HIP_TRY(hipEventElapsedTime(&ms, h->loo_ev[0].get(), h->loo_ev[1].get()));
    h->loo_diag_ms = ms;
  }
  if (need_alpha) {
    if ((st = batch_solve_impl(h, 1, nullptr, nullptr)) != CLR_OK) return st;  // alpha = K^-1 r -> bs_rm [B][N]
    h->loo_solve_ms = h->solve_device_ms;
    if (loo_logpdf && (st = h->loo_out.reserve(B)) != CLR_OK) return st;
    ConsumerFrame frame{h};  // (untimed)
    hipStream_t s = h->stream.get();
    if (loo_logpdf) {
      HIP_TRY(hipEventRecord(h->loo_ev[2].get(), s));
      hipLaunchKernelGGL(loo_reduce_kernel, dim3((unsigned)B), dim3(256), 0, s, h->loo_c.p, h->bs_rm.p, h->N, h->loo_out.p);
      HIP_TRY(hipEventRecord(h->loo_ev[3].get(), s));
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(loo_logpdf, h->loo_out.p, B * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    if ((st = frame.finish(alpha, h->bs_rm.p, B * N)) != CLR_OK) return st;
    if (loo_logpdf) {
      HIP_TRY(hipEventElapsedTime(&ms, h->loo_ev[2].get(), h->loo_ev[3].get()));
      h->loo_reduce_ms = ms;
    }
  }
  return CLR_OK;
}

int clr_batch_leave_one_out(clr_batch* h, double* kinv_diag, double* alpha, double* loo_logpdf, int* status) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (!kinv_diag && !alpha && !loo_logpdf && !status)
    return fail(CLR_INVALID_ARGUMENT, "clr_batch_leave_one_out: at least one output array");
  if ((st = require_celerite_width(h, "clr_batch_leave_one_out")) != CLR_OK) return st;
  if ((st = require_factor(h, true)) != CLR_OK) return st;
  if ((st = require_route(h, "clr_batch_leave_one_out")) != CLR_OK) return st;
  if ((st = leave_one_out_device(h, kinv_diag || loo_logpdf, alpha || loo_logpdf, kinv_diag, alpha, loo_logpdf)) != CLR_OK) return st;
  const size_t N = (size_t)h->N;
  return nan_rows_without_factor(h, {{kinv_diag, N}, {alpha, N}, {loo_logpdf, 1}}, status);
}

// ---- clr_batch_grad_noise_weights: the gradient with respect to the weights of a linear noise model

// d loglike / d s[b][k] = 1/2 sum_n Psi_k[b][n] (alpha_n^2 - c_n), alpha = K_b^-1 r_b and c = diag(K_b^-1): d K / d s_k is
// the diagonal matrix Psi_k, so the partial is 1/2 alpha^T Psi_k alpha - 1/2 tr(K^-1 Psi_k).  Leave-one-out's two device
// parts (the diagonal's recurrence, the solve of the residual) leave c and alpha row-major in HBM; one projection pass
// onto the resident basis follows (clr_bnoise_kernels.h).  The gradient sweeps are not involved.
int clr_batch_grad_noise_weights(clr_batch* h, double* ds, int* status) {
  static const char* entry = "clr_batch_grad_noise_weights";
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (h->noise_K == 0) return fail(CLR_INVALID_ARGUMENT, std::string(entry) + ": no basis is set (clr_batch_set_noise_basis)");
  if (!ds) return fail(CLR_INVALID_ARGUMENT, std::string(entry) + ": an output array");
  if ((st = require_celerite_width(h, entry)) != CLR_OK) return st;
  if ((st = require_factor(h, true)) != CLR_OK) return fail(st, std::string(entry) + ": " + g_last_error);
  if (h->variance_changed)
    return fail(CLR_NOT_COMPUTED, std::string(entry) + ": the noise basis, the noise weights or the series were replaced after the "
                                  "materialising run whose factor is in HBM -- that factor is another matrix': materialise again "
                                  "(clr_batch_enqueue(h, 1))");
  if ((st = require_route(h, entry)) != CLR_OK) return st;
  if ((st = leave_one_out_device(h, true, true, nullptr, nullptr, nullptr)) != CLR_OK) return fail(st, std::string(entry) + ": " + g_last_error);
  const size_t B = (size_t)h->B, K = (size_t)h->noise_K;
  if ((st = h->proj_part.reserve(clr::mean_project_workspace(h->B, h->N, h->noise_K))) != CLR_OK) return st;
  if ((st = h->proj_out.reserve(B * K)) != CLR_OK) return st;
  for (clr::Event& e : h->proj_ev)
    if (!e) HIP_TRY(clr::create_event(e));
  {
    ConsumerFrame frame{h};  // (untimed: the projection has its own events)
    HIP_TRY(hipEventRecord(h->proj_ev[0].get(), h->stream.get()));
    // (amplitudes in force: diag(K_y^-1) = c' / s^2 and alpha_y = alpha' / s in data units)
    const bool launched = h->amp_active
        ? clr::launch_noise_project_scaled(h->noise_basis.p, h->noise_stride, h->bs_rm.p, h->loo_c.p, h->amp_s.p, h->noise_K,
                                           h->B, h->N, h->proj_part.p, h->proj_out.p, h->stream.get())
        : clr::launch_noise_project(h->noise_basis.p, h->noise_stride, h->bs_rm.p, h->loo_c.p, h->noise_K, h->B, h->N,
                                    h->proj_part.p, h->proj_out.p, h->stream.get());
    if (!launched)
      return fail(CLR_UNSUPPORTED, std::string(entry) + ": B x N / 4096 workgroups do not fit one launch");
    HIP_TRY(hipEventRecord(h->proj_ev[1].get(), h->stream.get()));
    if ((st = frame.finish(ds, h->proj_out.p, B * K)) != CLR_OK) return st;
  }
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, h->proj_ev[0].get(), h->proj_ev[1].get()));
  h->noise_project_ms = ms;
  // the statuses of the evaluation in force; a problem without a factor (or refused by the kernel program): zeros
  std::vector<int> stat;
  if ((st = evaluation_statuses(h, stat)) != CLR_OK) return st;
  for (size_t b = 0; b < B; ++b)
    if (stat[b] != CLR_OK) std::fill(ds + b * K, ds + (b + 1) * K, 0.0);  // (the gradient's quiet semantics)
  if (status) std::copy(stat.begin(), stat.end(), status);
  return CLR_OK;
}

int clr_batch_get_noise_project_ms(const clr_batch* h, double* device_ms) {
  if (device_ms) *device_ms = h->noise_project_ms;
  return CLR_OK;
}

// ---- clr_batch_grad_amplitudes: the gradient with respect to the amplitudes of the per-sample amplitude model

// loglike = -1/2 y'^T K'^-1 y' - 1/2 log det K' - sum_n log|s_n| + const with y' = r / s and K' = K + diag(d / s^2): s_n enters
// through y'_n (d y'_n / d s_n = -y'_n / s_n), d'_n (d d'_n / d s_n = -2 d'_n / s_n) and the log term, so with alpha' =
// K'^-1 y' and c' = diag(K'^-1)
//   d loglike / d s_n = (alpha'_n y'_n + d'_n (c'_n - alpha'_n^2) - 1) / s_n ,   da[b][k] = sum_n Gamma_k[b][n] d loglike / d s_n.
// clr_batch_grad_noise_weights' steps with another per-sample factor: leave-one-out's two device parts, one projection.
int clr_batch_grad_amplitudes(clr_batch* h, double* da, int* status) {
  static const char* entry = "clr_batch_grad_amplitudes";
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (h->amp_K == 0) return fail(CLR_INVALID_ARGUMENT, std::string(entry) + ": no basis is set (clr_batch_set_amplitude_basis)");
  if (!h->amp_active) return fail(CLR_INVALID_ARGUMENT, std::string(entry) + ": no amplitudes are in force (clr_batch_set_amplitudes)");
  if (!da) return fail(CLR_INVALID_ARGUMENT, std::string(entry) + ": an output array");
  if ((st = require_celerite_width(h, entry)) != CLR_OK) return st;
  if ((st = require_factor(h, true)) != CLR_OK) return fail(st, std::string(entry) + ": " + g_last_error);
  if (h->variance_changed)
    return fail(CLR_NOT_COMPUTED, std::string(entry) + ": the amplitudes, their basis, the noise weights or the series were replaced "
                                  "after the materialising run whose factor is in HBM -- that factor is another matrix': "
                                  "materialise again (clr_batch_enqueue(h, 1))");
  if ((st = require_route(h, entry)) != CLR_OK) return st;
  if ((st = leave_one_out_device(h, true, true, nullptr, nullptr, nullptr)) != CLR_OK) return fail(st, std::string(entry) + ": " + g_last_error);
  const size_t B = (size_t)h->B, K = (size_t)h->amp_K;
  if ((st = h->proj_part.reserve(clr::mean_project_workspace(h->B, h->N, h->amp_K))) != CLR_OK) return st;
  if ((st = h->proj_out.reserve(B * K)) != CLR_OK) return st;
  for (clr::Event& e : h->proj_ev)
    if (!e) HIP_TRY(clr::create_event(e));
  {
    ConsumerFrame frame{h};  // (untimed: the projection has its own events)
    HIP_TRY(hipEventRecord(h->proj_ev[0].get(), h->stream.get()));
    // (with amplitudes in force `y` and `diag` are y' and d' -- without the jitter --, both [B][N])
    if (!clr::launch_amplitude_project(h->amp_basis.p, h->amp_stride, h->bs_rm.p, h->loo_c.p, h->y.p, h->diag.p, h->amp_s.p,
                                       h->amp_K, h->B, h->N, h->proj_part.p, h->proj_out.p, h->stream.get()))
      return fail(CLR_UNSUPPORTED, std::string(entry) + ": B x N / 4096 workgroups do not fit one launch");
    HIP_TRY(hipEventRecord(h->proj_ev[1].get(), h->stream.get()));
    if ((st = frame.finish(da, h->proj_out.p, B * K)) != CLR_OK) return st;
  }
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, h->proj_ev[0].get(), h->proj_ev[1].get()));
  h->amp_project_ms = ms;
  // the statuses of the evaluation in force; a problem without a factor (or whose draw or scale was refused): zeros
  std::vector<int> stat;
  if ((st = evaluation_statuses(h, stat)) != CLR_OK) return st;
  for (size_t b = 0; b < B; ++b)
    if (stat[b] != CLR_OK) std::fill(da + b * K, da + (b + 1) * K, 0.0);  // (the gradient's quiet semantics)
  if (status) std::copy(stat.begin(), stat.end(), status);
  return CLR_OK;
}

int clr_batch_get_amplitude_project_ms(const clr_batch* h, double* device_ms) {
  if (device_ms) *device_ms = h->amp_project_ms;
  return CLR_OK;
}

// ---- clr_batch_fit_mean_weights: the generalised-least-squares fit of a linear mean's weights

int clr_batch_set_mean_fit_tile(clr_batch* h, int rhs) {
  h->mean_fit_tile = rhs > 0 ? rhs : 0;
  return CLR_OK;
}

int clr_batch_get_mean_fit_ms(const clr_batch* h, double* solve_ms, double* gram_ms, double* small_ms) {
  if (solve_ms) *solve_ms = h->fit_solve_ms;
  if (gram_ms) *gram_ms = h->fit_gram_ms;
  if (small_ms) *small_ms = h->fit_small_ms;
  return CLR_OK;
}

// right-hand sides per tile: the caller's (clr_batch_set_mean_fit_tile), or the most whose buffers -- `per_rhs` doubles
// each -- fit in predict_tile's 1 GiB; never above `most` (the K + 1 there are, or what a grid axis takes), at least 1
static int fit_tile(const clr_batch* h, size_t most, size_t per_rhs) {
  const size_t budget = (size_t)1 << 27;  // doubles
  const size_t R = h->mean_fit_tile > 0 ? (size_t)h->mean_fit_tile : std::max<size_t>(1, budget / std::max<size_t>(1, per_rhs));
  return (int)std::max<size_t>(1, std::min(R, most));
}

// For every problem of a plan with a linear mean: the weights that maximise the log-likelihood at the coefficients in
// force, w = w0 + G^-1 d with G = Phi^T K^-1 Phi, d = Phi^T K^-1 r, r the residual at the weights w0 in force -- the
// log-likelihood is exactly quadratic in the weights, so this one Newton step from any w0 is the optimum.  The K + 1
// right-hand sides (Phi_0 .. Phi_K-1, r) are formed on the device from the resident basis and residual, a tile of columns
// at a time, and solved on the factor in HBM by the batched solve's kernels (narrow plans: launch->bsolve on the
// chunk-interleaved factor, either layout, the chunk maps under clr_batch_solve's validity rule; wide plans: the two
// sweeps of wide_batch_solve); every tile's solutions go through the bordered Gram pass (clr_bmean_kernels.h), and one
// thread per problem runs the small solve (clr_gram_solve.h).  The weights in force stay as they are.
int clr_batch_fit_mean_weights(clr_batch* h, double min_pivot, double* w_hat, double* cov, double* gram, double* quad_profiled,
                               double* logdet_gram, int* status) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (!std::isfinite(min_pivot) || min_pivot < 0.0 || min_pivot >= 1.0)
    return fail(CLR_INVALID_ARGUMENT, "clr_batch_fit_mean_weights: min_pivot is finite and in [0, 1)");
  if (h->have_mean)
    return fail(CLR_INVALID_ARGUMENT, "clr_batch_fit_mean_weights: a constant mean is in force (clr_batch_set_mean): the fit is "
                                      "the linear mean's -- make the constant a basis function");
  if (h->mean_K == 0) return fail(CLR_INVALID_ARGUMENT, "clr_batch_fit_mean_weights: no basis is set (clr_batch_set_mean_basis)");
  if (h->amp_active)
    return fail(CLR_UNSUPPORTED, "clr_batch_fit_mean_weights: amplitudes are in force (clr_batch_set_amplitudes) -- the fit's "
                                 "right-hand sides would be Phi / s, which is not built: remove the amplitude model for the fit, "
                                 "or take clr_batch_grad_mean_weights' gradient");
  if ((st = require_celerite_width(h, "clr_batch_fit_mean_weights")) != CLR_OK) return st;
  if ((st = require_factor(h, true)) != CLR_OK) return st;
  if (h->B > 65535) return fail(CLR_UNSUPPORTED, "clr_batch_fit_mean_weights: at most 65535 problems per plan (a grid axis): shard the batch");
  if ((st = require_route(h, "clr_batch_fit_mean_weights")) != CLR_OK) return st;
  const size_t B = (size_t)h->B, N = (size_t)h->N, J = (size_t)h->J, K = (size_t)h->mean_K, K1 = K + 1;
  const size_t nout = clr::gram_solve_out_doubles(h->mean_K);
  clr::BatchParams P;  // (wide plans do not read it)
  clr::SweepParams W;
  int R;
  if (h->launch) {
    if ((st = consumer_params(h, false, P)) != CLR_OK) return st;
    const size_t cells = (size_t)h->L * h->nchunk, nc = (size_t)h->nchunk;
    // (rows of the relayouts ride on grid.z: B * R <= 65535; a column's buffers: its chunk-interleaved cells, its
    //  row-major solution in bs_rm, offsets and start states)
    R = fit_tile(h, std::min<size_t>(K1, 65535 / B), B * (cells + N + 2 * nc * J));
    if ((st = reserve_narrow_solve(h, (size_t)R)) != CLR_OK) return st;
  } else {
    W = wide_solve_params(h, 1);
    const size_t ws_rhs = clr::wsweep_workspace_doubles(h->J, W.nchunk, 2) - clr::wsweep_workspace_doubles(h->J, W.nchunk, 1);
    R = fit_tile(h, K1, B * (2 * N + ws_rhs));
    if ((st = h->bs_M.reserve(B * clr::wsweep_workspace_doubles(h->J, W.nchunk, R))) != CLR_OK) return st;
    if ((st = h->bs_x.reserve(B * R * N)) != CLR_OK) return st;  // the forward sweep's output (undivided)
  }
  if ((st = h->bs_rm.reserve(B * R * N)) != CLR_OK) return st;  // the tile's solutions, row-major
  if ((st = h->fit_part.reserve(clr::mean_gram_workspace(h->B, h->N, h->mean_K))) != CLR_OK) return st;
  if ((st = h->fit_gram.reserve(B * K1 * K1)) != CLR_OK) return st;
  if ((st = h->fit_w0.reserve(B * K)) != CLR_OK) return st;
  if ((st = h->fit_out.reserve(B * nout)) != CLR_OK) return st;
  if ((st = h->fit_work.reserve(clr::gram_solve_workspace(h->B, h->mean_K))) != CLR_OK) return st;
  if ((st = h->fit_status.reserve(B)) != CLR_OK) return st;
  const int ntile = ((int)K1 + R - 1) / R;
  if (h->fit_ev.size() < (size_t)(2 * ntile + 3)) h->fit_ev.resize(2 * ntile + 3);
  for (int i = 0; i < 2 * ntile + 3; ++i)
    if (!h->fit_ev[i]) HIP_TRY(clr::create_event(h->fit_ev[i]));
  const std::vector<double> w0 = h->host_weights;  // (the copy below is drained before this call returns)
  std::vector<double> out(B * nout);
  std::vector<int> solve_status(B);
  const clr::FitRhs rhs{h->basis_dev.p, h->basis_stride, h->y.p, h->y_stride, h->mean_K, h->N};
  {
    ConsumerFrame frame{h};  // (untimed: the three parts have their own events)
    hipStream_t s = h->stream.get();
    HIP_TRY(hipMemcpyAsync(h->fit_w0.p, w0.data(), B * K * sizeof(double), hipMemcpyHostToDevice, s));
    clr::BSolveParams S;  // (narrow plans: the chunk maps are the batched solve's, formed by the first tile unless a solve left them)
    if (h->launch) S = narrow_solve_begin(h, frame, R);
    HIP_TRY(hipEventRecord(h->fit_ev[0].get(), s));
    for (int t = 0, c0 = 0; t < ntile; ++t, c0 += R) {
      const int nr = std::min(R, (int)K1 - c0);
      if (h->launch) {
        const long cells = (long)h->L * h->nchunk;
        clr::launch_fit_rhs_interleaved(rhs, c0, nr, h->B, h->L, h->nchunk, h->bs_x.p, cells, s);
        S.nrhs = nr;
        h->launch->bsolve(P, S, s);
        S.have_M = 1;
        clr::launch_relayout_back(h->bs_x.p, cells, h->bs_rm.p, (long)h->N, h->B * nr, h->N, h->L, h->nchunk, s);
      } else {
        clr::launch_fit_rhs_rowmajor(rhs, c0, nr, h->B, h->bs_rm.p, s);
        wide_solve_sweeps(h, W, nr, h->bs_rm.p, (long)nr * (long)N);
      }
      HIP_TRY(hipEventRecord(h->fit_ev[2 * t + 1].get(), s));
      clr::launch_mean_gram(rhs, h->bs_rm.p, c0, nr, h->B, h->fit_part.p, s);
      HIP_TRY(hipEventRecord(h->fit_ev[2 * t + 2].get(), s));
    }
    clr::launch_mean_gram_finish(h->fit_part.p, h->mean_K, h->B, h->N, h->fit_gram.p, s);
    HIP_TRY(hipEventRecord(h->fit_ev[2 * ntile + 1].get(), s));
    clr::launch_gram_solve(h->fit_gram.p, h->fit_w0.p, min_pivot, h->mean_K, h->B, h->fit_out.p, h->fit_status.p, h->fit_work.p, s);
    HIP_TRY(hipEventRecord(h->fit_ev[2 * ntile + 2].get(), s));
    HIP_TRY(hipGetLastError());
    if (gram) HIP_TRY(hipMemcpyAsync(gram, h->fit_gram.p, B * K1 * K1 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(solve_status.data(), h->fit_status.p, B * sizeof(int), hipMemcpyDeviceToHost, s));
    if ((st = frame.finish(out.data(), h->fit_out.p, B * nout)) != CLR_OK) return st;
  }
  double ms_solve = 0.0, ms_gram = 0.0;
  float ms = 0.f;
  for (int t = 0; t < ntile; ++t) {
    HIP_TRY(hipEventElapsedTime(&ms, h->fit_ev[2 * t].get(), h->fit_ev[2 * t + 1].get()));
    ms_solve += ms;
    HIP_TRY(hipEventElapsedTime(&ms, h->fit_ev[2 * t + 1].get(), h->fit_ev[2 * t + 2].get()));
    ms_gram += ms;
  }
  HIP_TRY(hipEventElapsedTime(&ms, h->fit_ev[2 * ntile].get(), h->fit_ev[2 * ntile + 1].get()));
  ms_gram += ms;
  HIP_TRY(hipEventElapsedTime(&ms, h->fit_ev[2 * ntile + 1].get(), h->fit_ev[2 * ntile + 2].get()));
  h->fit_solve_ms = ms_solve; h->fit_gram_ms = ms_gram; h->fit_small_ms = ms;
  // the statuses of the evaluation in force come first: a problem without a factor (or refused by the kernel program)
  // keeps its weights, and everything else of it is NaN
  std::vector<int> stat;
  if ((st = evaluation_statuses(h, stat)) != CLR_OK) return st;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t b = 0; b < B; ++b) {
    const double* o = out.data() + b * nout;
    const bool evaluated = stat[b] == CLR_OK;
    const double* w = evaluated ? o : w0.data() + b * K;  // (a refused small solve has written w0 there itself)
    if (w_hat) std::copy(w, w + K, w_hat + b * K);
    if (cov && evaluated) std::copy(o + K, o + K + K * K, cov + b * K * K);
    if (cov && !evaluated) std::fill(cov + b * K * K, cov + (b + 1) * K * K, nan);
    if (gram && !evaluated) std::fill(gram + b * K1 * K1, gram + (b + 1) * K1 * K1, nan);
    if (quad_profiled) quad_profiled[b] = evaluated ? o[K + K * K] : nan;
    if (logdet_gram) logdet_gram[b] = evaluated ? o[K + K * K + 1] : nan;
    if (status) status[b] = evaluated ? solve_status[b] : stat[b];
  }
  return CLR_OK;
}

// ---- clr_batch_periodogram: the sinusoid fit under the plan's covariance at every trial frequency (clr_bperiodogram_kernels.h)

int clr_batch_set_periodogram_tile(clr_batch* h, int frequencies) {
  h->periodogram_tile = frequencies > 0 ? frequencies : 0;
  return CLR_OK;
}

int clr_batch_get_periodogram_ms(const clr_batch* h, double* device_ms) {
  if (device_ms) *device_ms = h->periodogram_ms;
  return CLR_OK;
}

int clr_batch_debug_get_periodogram_block(const clr_batch* h, int* frequencies) {
  if (frequencies) *frequencies = h->launch ? h->launch->periodogram_block : 0;
  return CLR_OK;
}

// For every problem and trial frequency: the bordered Gram matrix of the columns (cos, sin) or (1, cos, sin) and the
// residual in force under K^-1, and the small solve of clr_batch_fit_mean_weights on it.  The residual (and the constant
// column) are whitened once by the forward pass of clr_batch_one_step_ahead (the chunk maps under clr_batch_solve's
// validity rule); a tile of frequencies at a time -- as many as fit predict_tile's 1 GiB, or the caller's -- runs the two
// walks of clr_bperiodogram_kernels.h and the reduction.  Nothing goes up but the frequencies.
int clr_batch_periodogram(clr_batch* h, int F, const double* omega, long omega_stride, double t_ref, int offset, double min_pivot,
                          double* power, double* coef, double* cov, double* gram, int* status) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  const char* e = "clr_batch_periodogram";
  if (F < 0 || (F > 0 && !omega)) return fail(CLR_INVALID_ARGUMENT, std::string(e) + ": F >= 0 and the frequencies");
  if (omega_stride != 0 && omega_stride != F)
    return fail(CLR_INVALID_ARGUMENT, std::string(e) + ": the frequencies' stride is 0 (shared by all problems) or F");
  if (!power && !coef && !cov && !gram && !status) return fail(CLR_INVALID_ARGUMENT, std::string(e) + ": at least one output array");
  if (!std::isfinite(t_ref)) return fail(CLR_INVALID_ARGUMENT, std::string(e) + ": t_ref is finite");
  if (!std::isfinite(min_pivot) || min_pivot < 0.0 || min_pivot >= 1.0)
    return fail(CLR_INVALID_ARGUMENT, std::string(e) + ": min_pivot is finite and in [0, 1)");
  const size_t B = (size_t)h->B, Ff = (size_t)F, nsrc = omega_stride == 0 ? 1 : B;
  for (size_t i = 0; i < nsrc * Ff; ++i)
    if (!std::isfinite(omega[i])) return fail(CLR_INVALID_ARGUMENT, std::string(e) + ": the frequencies are finite");
  if ((st = refuse_ragged(h, e)) != CLR_OK) return st;
  if (h->J_general > 0)
    return fail(CLR_UNSUPPORTED, std::string(e) + " covers celerite-only plans: with general terms, fit (cos, sin) as a linear mean "
                                 "through the object API's solves");
  if (!h->launch)
    return fail(CLR_UNSUPPORTED, std::string(e) + " covers narrow plans (widths 1..8): a wide plan takes clr_batch_set_mean_basis with "
                                 "(cos, sin) and clr_batch_fit_mean_weights per frequency");
  if (h->amp_active)
    return fail(CLR_UNSUPPORTED, std::string(e) + ": amplitudes are in force (clr_batch_set_amplitudes) -- the resident series are y / s, "
                                 "where a sinusoid in observed units is none: remove the amplitude model for the scan");
  if (F == 0) return CLR_OK;
  if ((st = require_factor(h, true)) != CLR_OK) return st;
  if (h->B > 65535) return fail(CLR_UNSUPPORTED, std::string(e) + ": at most 65535 problems per plan (a grid axis): shard the batch");
  Route route;
  route.chunk_hint = " (shorter series: clr_batch_fit_mean_weights with (cos, sin) as the basis)";
  if ((st = require_route(h, e, route)) != CLR_OK) return st;
  clr::BatchParams P;
  if ((st = consumer_params(h, false, P)) != CLR_OK) return st;
  const size_t J = (size_t)h->J, nc = (size_t)h->nchunk, cells = (size_t)h->L * nc, nz = offset ? 2 : 1;
  const size_t K = offset ? 3 : 2, K1 = K + 1;
  // a frequency's scratch: the offsets and start states of its two columns, its chunks' sums
  const size_t per_f = B * nc * (4 * J + clr::BPG_SUMS);
  const size_t budget = (size_t)1 << 27;  // doubles (predict_tile's)
  size_t R = h->periodogram_tile > 0 ? (size_t)h->periodogram_tile : std::max<size_t>(1, budget / per_f);
  R = std::min(std::min<size_t>(R, 32767), Ff);  // (the frequency blocks ride on grid.z; 2 R right-hand sides)
  DevBuf dom, dpart, dbase, dbpart, dpower, dcoef, dcov, dgram;
  DevArray<int> dstat;
  if ((st = h->bs_x.reserve(B * nz * cells)) != CLR_OK) return st;
  if ((st = h->bs_M.reserve(B * nc * J * J)) != CLR_OK) return st;
  if ((st = h->bs_off.reserve(B * std::max(nz, 2 * R) * nc * J)) != CLR_OK) return st;
  if ((st = h->bs_starts.reserve(B * std::max(nz, 2 * R) * nc * J)) != CLR_OK) return st;
  if ((st = dpart.reserve(B * R * nc * clr::BPG_SUMS)) != CLR_OK) return st;
  if ((st = dbpart.reserve(B * nc * 3)) != CLR_OK) return st;
  if ((st = dbase.reserve(B * 3)) != CLR_OK) return st;
  if (power && (st = dpower.reserve(B * Ff)) != CLR_OK) return st;
  if (coef && (st = dcoef.reserve(B * Ff * K)) != CLR_OK) return st;
  if (cov && (st = dcov.reserve(B * Ff * K * K)) != CLR_OK) return st;
  if (gram && (st = dgram.reserve(B * Ff * K1 * K1)) != CLR_OK) return st;
  if ((st = dstat.reserve(B * Ff)) != CLR_OK) return st;
  std::vector<int> fstat(B * Ff);
  const double keep_solve_ms = h->solve_device_ms;
  {
    ConsumerFrame frame{h};
    hipStream_t s = h->stream.get();
    if ((st = upload(dom, omega, nsrc * Ff, s)) != CLR_OK) return st;
    HIP_TRY(frame.start());
    // z_r (and z_1) in bs_x: the residual in force and the constant column, whitened in place
    const clr::BSolveParams Q = narrow_solve_begin(h, frame, (int)nz);
    clr::launch_relayout(h->y.p, h->y_stride, h->bs_x.p, (long)(nz * cells), h->B, h->N, h->L, h->nchunk, 0, s);
    if (offset) clr::launch_fill_rows(h->bs_x.p + cells, (long)(nz * cells), h->B, (long)cells, 1.0, s);
    clr::BFilterParams Z{};
    Z.nrhs = (int)nz; Z.lean = Q.lean; Z.have_M = Q.have_M;
    Z.xT = Z.zT = Q.xT; Z.M = Q.M; Z.off = Q.off; Z.starts = Q.starts;
    h->launch->bfilter(P, Z, 0, s);
    clr::launch_periodogram_base(h->bs_x.p, h->D.p, (int)nz, h->B, h->N, h->L, h->nchunk, dbpart.p, dbase.p, s);
    clr::BPeriodogramParams S{};
    S.lean = Q.lean; S.offset = offset ? 1 : 0;
    S.omega_stride = omega_stride; S.t_ref = t_ref;
    S.zT = h->bs_x.p; S.M = h->bs_M.p; S.off = h->bs_off.p; S.starts = h->bs_starts.p; S.part = dpart.p;
    const clr::PeriodogramOut out{power ? dpower.p : nullptr, coef ? dcoef.p : nullptr, cov ? dcov.p : nullptr,
                                  gram ? dgram.p : nullptr, dstat.p};
    for (size_t f0 = 0; f0 < Ff; f0 += R) {
      S.nf = (int)std::min(R, Ff - f0);
      S.omega = dom.p + f0;
      h->launch->bperiodogram(P, S, s);
      clr::launch_periodogram_reduce(dpart.p, dbase.p, h->B, S.nf, h->nchunk, S.offset, min_pivot, (long)Ff, (long)f0, out, s);
    }
    HIP_TRY(frame.stop());
    HIP_TRY(hipGetLastError());
    if (power) HIP_TRY(hipMemcpyAsync(power, dpower.p, B * Ff * sizeof(double), hipMemcpyDeviceToHost, s));
    if (coef) HIP_TRY(hipMemcpyAsync(coef, dcoef.p, B * Ff * K * sizeof(double), hipMemcpyDeviceToHost, s));
    if (cov) HIP_TRY(hipMemcpyAsync(cov, dcov.p, B * Ff * K * K * sizeof(double), hipMemcpyDeviceToHost, s));
    if (gram) HIP_TRY(hipMemcpyAsync(gram, dgram.p, B * Ff * K1 * K1 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(fstat.data(), dstat.p, B * Ff * sizeof(int), hipMemcpyDeviceToHost, s));
    if ((st = frame.finish()) != CLR_OK) return st;
  }
  h->periodogram_ms = h->solve_device_ms;
  h->solve_device_ms = keep_solve_ms;  // (it stays the solve's)
  // the statuses of the evaluation in force come first: a problem without a factor is NaN at every frequency
  if ((st = nan_rows_without_factor(h, {{power, Ff}, {coef, Ff * K}, {cov, Ff * K * K}, {gram, Ff * K1 * K1}})) != CLR_OK) return st;
  if (status) {
    std::vector<int> stat;
    if ((st = evaluation_statuses(h, stat)) != CLR_OK) return st;
    for (size_t b = 0; b < B; ++b)
      for (size_t f = 0; f < Ff; ++f) status[b * Ff + f] = stat[b] == CLR_OK ? fstat[b * Ff + f] : stat[b];
  }
  return CLR_OK;
}

int clr_batch_get_solve_ms(const clr_batch* h, double* device_ms) {
  if (device_ms) *device_ms = h->solve_device_ms;
  return CLR_OK;
}

}  // extern "C"
