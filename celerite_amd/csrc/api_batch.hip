// celerite_amd/csrc/api_batch.hip -- C ABI of the batched plans (clr_batch_*): HBM residency, path selection
// (scan pipeline, warm-started recurrence, one-launch path, wide kernels, general terms), evaluation and results.  The
// consumers of a plan's factor and coefficients: api_batch_consumers.hip.
#include "api_internal.h"
#include "clr_options.h"
#include "clr_group_hooks.h"
#include "clr_kernel.h"
#include "clr_bmean_kernels.h"
#include "clr_bnoise_kernels.h"
#include "clr_bamplitude_kernels.h"

#include <limits>

extern "C" {

/* ---- batched log-likelihood ---------------------------------------------------- */
clr_batch* clr_batch_create(int B, int N, int J_real, int J_comp, int device) {
  if (B < 1 || N < 1 || J_real < 0 || J_comp < 0) {
    fail(CLR_INVALID_ARGUMENT, "clr_batch_create: bad sizes");
    return nullptr;
  }
  const clr::BatchLaunchers* L = clr::find_batch_launchers(J_real, J_comp);
  const int width = J_real + 2 * J_comp;
  if (!L && (width < 1 || width > CLR_MAX_WIDTH)) {
    fail(CLR_UNSUPPORTED, "batched path supports widths 1..128 (J_real + 2 J_comp)");
    return nullptr;
  }
  if (require_device(device) != CLR_OK) return nullptr;
  clr_batch* h = new clr_batch();
  h->device = device;
  h->B = B;
  h->N = N;
  h->J_real = J_real;
  h->J_comp = J_comp;
  h->J = J_real + 2 * J_comp;
  h->launch = L;  // null: widths 9..64, one wave per problem (wide_kernels.hip)
  if (clr::create_stream(h->stream) != hipSuccess) {
    fail(CLR_HIP_ERROR, "hipStreamCreate failed");
    delete h;
    return nullptr;
  }
  if (clr_batch_set_chunks(h, 0) != CLR_OK) {
    clr_batch_destroy(h);
    return nullptr;
  }
  return h;
}

void clr_batch_destroy(clr_batch* h) { delete h; }

static int warm_plan_chunks(clr_batch* h);
static int warm_scan_spans(clr_batch* h);
static void warm_select(clr_batch* h);
static int plan_general_chunks(clr_batch* h);

int clr_batch_set_chunks(clr_batch* h, int nchunk) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;
  h->warm_explicit_chunks = nchunk > 0 ? nchunk : 0;
  if (nchunk > 0) h->pipeline_pinned = true;
  if (!h->launch) {
    // wide path: one wave per (problem, chunk).  One chunk (the plain sequential sweep)
    // unless the batch alone leaves the chip underused: then ~2 waves per SIMD worth of
    // chunks, at ~1.25x the work per sample (profiles/r01s); widths above 32 stay sequential
    if (h->J > clr::wide_scan_max_width()) nchunk = 1;
    else if (h->J > 32) {
      // widths 33..64 (round 5): the summarize keeps S and A^T in 256 registers per lane -- ONE wave per SIMD -- so a round
      // of the chip is B x nchunk = 1024 waves; the chunks are chained by a walk per problem (~0.2 ms per chunk:
      // wide64_kernels.hip), so at most 16, each of >= 1024 samples.  Above 512 problems two chunks no longer pay.
      if (nchunk <= 0) {
        nchunk = h->B <= 512 ? std::max(2, 1024 / h->B) : 1;
        if (nchunk > 16) nchunk = 16;
        while (nchunk > 1 && h->N / nchunk < 1024) --nchunk;
      }
    } else if (nchunk <= 0) {
      // One round of two waves per SIMD: B x nchunk = 2048 waves.  (Round 2 used 4096 / B -- two rounds of half the
      //  length -- because the checked replay of borderline problems, 7 ms for config 4, got shorter with the chunks;
      //  with the round-3 routing that family is settled from the chunk summaries and the sequential prefix + the
      //  correct phase decide: B = 256: 8 chunks 17.1 ms, 16 chunks 18.5, 10 chunks 22.8 (2560 waves = a second,
      //  nearly empty round), B = 512: 4 chunks 32.2 ms, 8 chunks 32.7; profiles/r03_wide_chunks.txt)
      nchunk = h->B <= 1024 ? 2048 / h->B : 1;  // (above 1024 problems one sweep per problem already fills a round)
      if (nchunk < 2) nchunk = 1;
      if (nchunk > 16) nchunk = 16;
      while (nchunk > 1 && h->N / nchunk < 512) --nchunk;
      // few problems: the prefix is a parallel scan (wide_prefix_scan.hip) as long as B x nchunk <= 1024 / 512 -- chunks of
      // >= 64 / 96 samples instead of 16 long ones (one series of 1e5 samples: 1024 / 512 chunks)
      const int cap = clr::wide_prefix_scan_max_chunks(h->J <= 16 ? 16 : 32), Lmin = h->J <= 16 ? 64 : 96;  // (r04z_single_wide_short.txt)
      if (h->coop_prefix == 2 && h->B < 32 && std::min(cap / h->B, h->N / Lmin) > nchunk) nchunk = std::min(cap / h->B, h->N / Lmin);
      // 32..256 problems (profiles/r04zz_wide_midbatch.txt, N = 1e5): 16 long chunks leave the chip half empty -- width <= 16:
      // 64 chunks at B = 32 (4.1 -> 1.6 ms), 32 at B = 64..256 (3.9 -> 2.8, 5.2 -> 4.9, 9.9 -> 8.5 ms); width 32: 32 chunks at
      // B = 32 (5.4 -> 3.5 ms), the old counts above (the walk's 50 us per chunk and problem)
      // (width <= 16 up to 1024 problems: B = 512 19.6 -> 15.8 ms with 32 chunks, B = 1024 36.2 -> 30.6 ms with 16)
      if (h->coop_prefix == 2 && h->B >= 32 && h->B <= (h->J <= 16 ? 1024 : 256)) {
        int want = nchunk;
        if (h->J <= 16) want = h->B <= 512 ? std::max(32, 2048 / h->B) : 16;
        else if (h->B == 32) want = 32;
        if (want > nchunk && h->N / want >= 512) nchunk = want;
      }
    }
    if (nchunk > h->N / 64) nchunk = std::max(1, h->N / 64);
  } else if (nchunk <= 0) {
    nchunk = auto_chunks(h->B, h->N, h->J);
  }
  if (nchunk > h->N) nchunk = h->N;
  h->L = (h->N + nchunk - 1) / nchunk;
  if (nchunk > 1 && h->L > 8) h->L = (h->L + 7) & ~7;  // 64-B aligned chunk rows for the tile loads
  h->nchunk = (h->N + h->L - 1) / h->L;
  h->L0 = 0;
  const double first_ratio = h->J > 32 ? h->wide_first_ratio64 : h->wide_first_ratio;
  if (!h->launch && h->nchunk > 1 && first_ratio > 1.0) {
    // wide scan: the first chunk's summarize carries no riders (wide_scan_body, RIDERS == false) and costs
    // ~1 / wide_first_ratio of a later chunk's per sample: it gets that many more samples, so that all waves of the
    // one round finish together.  Chunks 1.. have exactly L samples, the first one the rest.
    const int nc = h->nchunk;
    int L = (int)ceil(h->N / (nc - 1 + first_ratio));
    L = (L + 7) & ~7;
    const long first = (long)h->N - (long)(nc - 1) * L;
    if (L >= 64 && first >= L) { h->L = L; h->L0 = (int)first; }
  }
  chunking_replaced(h);
  const size_t pc = (size_t)h->B * h->nchunk;
  h->plan = clr::plan_prefix(h->nchunk, 0, 0);
  h->scan_ws_doubles = 0;
  if (h->launch) {
    if ((st = h->elems.reserve(pc * h->launch->elem_doubles)) != CLR_OK) return st;
    if ((st = h->starts.reserve(pc * h->launch->start_doubles)) != CLR_OK) return st;
    // The prefix plan fixes the ORDER in which chunk elements are composed, i.e. the bits of every result: it must not
    // depend on how many problems happen to share the plan (a slice of a sharded batch, a side plan of pending problems
    // and the unsharded plan must agree bit for bit).  Its time model is asked for the batch size the automatic chunking
    // pairs with this chunk count -- about 65536 (problem, chunk) lanes, one round of the chip -- instead of the plan's own.
    h->plan = clr::plan_prefix(h->nchunk, h->plan_levels, h->plan_g, std::max(1, 65536 / std::max(1, h->nchunk)), h->J);
    size_t le = 0, ls = 0;
    clr::multilevel_workspace(h->plan, h->J, &le, &ls);
    if (le && (st = h->lvl_elems.reserve((size_t)h->B * le)) != CLR_OK) return st;
    if (ls && (st = h->lvl_starts.reserve((size_t)h->B * ls)) != CLR_OK) return st;
  } else if (h->nchunk > 1) {  // elements / start states at the padded width (16 or 32)
    const size_t JP = (size_t)clr::wide_padded_width(h->J), SZ = JP * (JP + 1) / 2;
    if ((st = h->elems.reserve(pc * (JP * JP + JP + SZ + JP + SZ))) != CLR_OK) return st;
    if ((st = h->starts.reserve(pc * (SZ + JP))) != CLR_OK) return st;
    // few problems with many chunks: the prefix as a parallel scan (wide_prefix_scan.hip); its level buffers
    h->scan_ws_doubles = clr::wide_prefix_scan_workspace(h->B, h->nchunk, (int)JP);
    if (h->scan_ws_doubles && (st = h->lvl_elems.reserve(h->scan_ws_doubles)) != CLR_OK) return st;
  }
  if ((st = h->part.reserve(pc * 2)) != CLR_OK) return st;
  if ((st = h->partx.reserve(pc * 2)) != CLR_OK) return st;
  if ((st = h->cond.reserve(pc * 4)) != CLR_OK) return st;  // gamma, mu, residual per chunk | measured G error
  if ((st = h->out.reserve((size_t)h->B * 3 + ((size_t)h->B + 1) / 2)) != CLR_OK) return st;
  h->flags.release();
  if ((st = h->flags.reserve(2 * pc + (size_t)h->B)) != CLR_OK) return st;
  // a single-chunk plan launches no prefix / correct kernel: nothing else would ever clear need_exact or fill
  // the conditioning record
  HIP_TRY(hipMemsetAsync(h->flags.p, 0, (2 * pc + (size_t)h->B) * sizeof(int), h->stream.get()));
  HIP_TRY(hipMemsetAsync(h->cond.p, 0, pc * 4 * sizeof(double), h->stream.get()));
  if ((st = warm_plan_chunks(h)) != CLR_OK) return st;
  if (h->J_general > 0 && (st = plan_general_chunks(h)) != CLR_OK) return st;  // (its chunking follows the plan's settings)
  return CLR_OK;
}

// The warm path's chunking: two waves per SIMD worth of (problem, chunk) lanes (the plain recurrence needs 189
// registers), chunks of at least 256 samples (the warm-up is at most half a chunk); an explicit chunk count is
// honoured (results then do not depend on the batch size, i.e. on a sharding).
static int warm_plan_chunks(clr_batch* h) {
  h->wnchunk = 0;
  h->wL = 0;
  h->warm_active = false;
  h->warm_span.clear();  // (the spans belong to a chunking: rescanned by the next set_series)
  if (!h->launch || h->N < 512) return CLR_OK;
  long want = h->warm_explicit_chunks ? h->warm_explicit_chunks : std::max<long>(1, 131072 / h->B);
  long L = (h->N + want - 1) / want;
  if (L < 256) L = 256;
  L = (L + 7) & ~7L;
  const long nc = (h->N + L - 1) / L;
  if (nc < 2) return CLR_OK;
  h->wL = (int)L;
  h->wnchunk = (int)nc;
  h->wKpad = std::min(128, h->wL / 2);  // rows of warm-up every chunk's column carries (the largest candidate)
  h->wrows = h->wKpad + h->wL + 8;
  warm_chunking_replaced(h);
  const size_t pc = (size_t)h->B * nc, START = (size_t)h->launch->start_doubles;
  int st;
  if ((st = h->wstarts.reserve(pc * START)) != CLR_OK) return st;
  if ((st = h->wends.reserve(pc * START)) != CLR_OK) return st;
  if ((st = h->wpart.reserve(pc * 2)) != CLR_OK) return st;
  if ((st = h->wresid.reserve((size_t)h->B)) != CLR_OK) return st;
  const size_t ints = pc + 2 * (size_t)h->B;
  if ((st = h->wints.reserve(ints)) != CLR_OK) return st;
  HIP_TRY(hipMemsetAsync(h->wints.p, 0, ints * sizeof(int), h->stream.get()));
  if (h->have_series) {  // the spans and the warm-ups follow the new chunking (the series are resident)
    if ((st = warm_scan_spans(h)) != CLR_OK) return st;
    warm_select(h);
  }
  return CLR_OK;
}

// For every problem (or the one shared series) and every candidate K: the shortest time the K samples in front of
// a chunk boundary of the warm path span.  O(B x chunks) lookups into the series resident in HBM (warm_spans_kernel),
// so the spans follow the chunking too (clr_batch_set_chunks after clr_batch_set_series).
static int warm_scan_spans(clr_batch* h) {
  h->warm_span.clear();
  if (h->wnchunk < 2 || !h->have_series) return CLR_OK;
  const int nb = h->t_stride == 0 ? 1 : h->B;
  const size_t n = (size_t)nb * clr_batch::WARM_NK;
  int st;
  if ((st = h->scan.reserve(std::max(n, (size_t)nb * 4))) != CLR_OK) return st;
  clr::WarmCands cands;
  cands.nk = clr_batch::WARM_NK;
  for (int k = 0; k < clr_batch::WARM_NK; ++k) cands.K[k] = h->warm_cand[k];
  clr::launch_warm_spans(h->t.p, h->t_stride, nb, h->wL, h->wnchunk, cands, h->scan.p, h->stream.get());
  h->warm_span.assign(n, 0.0);
  HIP_TRY(hipMemcpyAsync(h->warm_span.data(), h->scan.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  return CLR_OK;
}

int clr_batch_get_chunks(const clr_batch* h, int* nchunk, int* chunk_len) {
  if (nchunk) *nchunk = h->nchunk;
  if (chunk_len) *chunk_len = h->L;
  return CLR_OK;
}

// Warm-started recurrence: warm-up steps per problem from its slowest decay rate (host_cmin, kept from the last
// set_coefficients) and the time the samples in front of its chunk boundaries span (warm_span, from the last
// set_series): exp(-c_min x span) <= exp(-32) = 1.3e-14 -- what is left of ANY start state after the warm-up by the
// decay alone, three orders below the tolerance of the boundary check (the update by the data only forgets faster); the
// check of warm_check_kernel certifies the choice.  Called whenever either side changes, so that the K in force always
// belongs to the (series, coefficients) pair in force.
static void warm_select(clr_batch* h) {
  const size_t B = (size_t)h->B;
  h->warm_active = false;
  h->warm_K_dirty = false;
  h->warm_eligible = 0;
  h->warm_eligible_total = -1;
  if (h->warm_mode == 0 || h->wnchunk < 2 || !h->have_series || h->warm_span.empty() || h->host_cmin.size() != B) return;
  if (h->ragged) return;  // (per-problem lengths: the warm kernel's copy and boundary check know one length -- the scan takes the plan)
  h->warm_K.assign(B, 0);
  size_t eligible = 0;
  const bool shared = h->t_stride == 0;
  for (size_t b = 0; b < B; ++b) {
    int K = 0;
    if (h->warm_mode == 1) {
      K = std::min(h->warm_forced_K, h->wL / 2);
    } else {
      const double cmin = h->host_cmin[b];
      const double* span = &h->warm_span[(shared ? 0 : b) * clr_batch::WARM_NK];
      for (int k = 0; k < clr_batch::WARM_NK && cmin > 0.0; ++k)
        if (cmin * span[k] >= 32.0) {
          K = h->warm_cand[std::min(k + h->warm_boost, clr_batch::WARM_NK - 1)];
          if (K > h->wL / 2) K = 0;
          break;
        }
    }
    h->warm_K[b] = K;
    eligible += K > 0;
  }
  // (a batch with only a few eligible problems is not worth a second set of launches; a slice of a larger batch waits
  //  for the count over the whole batch: clr_group::set_warm_eligible_total)
  h->warm_eligible = (long)eligible;
  h->warm_eligible_total = -1;
  h->warm_active = h->group_B > 0 ? false : eligible * 2 >= B;
  h->warm_K_dirty = h->warm_active;  // (uploaded behind the next coefficients, or by the next enqueue)
}

// With amplitudes in force (clr_batch_set_amplitudes) every route reads y' = r / s and d' = d / (s * s): one elementwise pass
// over the resident scale `amp_s`, behind whatever formed r and d.  r is the residual of the linear mean in force, which
// apply_mean has just left in `y` (divided in place), or the caller's series in `y_src`; d is the noise model's variances
// that apply_noise has just left in `diag`, or the caller's diagonal in `diag_src`.  A second in-place pass, not a divisor
// fused into the forming kernels: those keep their bits and their registers, and a plan without amplitudes runs no other
// code.  An in-place division is never run twice on the same array: every caller forms r (or d) again first.
static int amplitude_divide(clr_batch* h, bool do_y, bool do_d) {
  const long N = h->N;
  int st;
  if (do_y && (st = h->y.reserve((size_t)h->B * N)) != CLR_OK) return st;
  if (do_d && (st = h->diag.reserve((size_t)h->B * N)) != CLR_OK) return st;
  const bool y_inplace = h->mean_K > 0, d_inplace = h->noise_K > 0;
  clr::launch_amplitude_divide(y_inplace ? h->y.p : h->y_src.p, y_inplace ? N : h->y_src_stride, do_y ? h->y.p : nullptr,
                               d_inplace ? h->diag.p : h->diag_src.p, d_inplace ? N : h->diag_src_stride,
                               do_d ? h->diag.p : nullptr, h->amp_s.p, h->B, (int)N, h->stream.get());
  // (per-problem lengths: the tails stay the padding y = 0 and 1e300)
  if (h->ragged && do_y) clr::launch_pad_tail(h->y.p, h->B, (int)N, h->len_dev.p, 0, h->stream.get());
  if (h->ragged && do_d) clr::launch_pad_tail(h->diag.p, h->B, (int)N, h->len_dev.p, 2, h->stream.get());
  HIP_TRY(hipGetLastError());
  if (do_y) residual_replaced(h, N);
  if (do_d) variance_replaced(h, N);
  return CLR_OK;
}

// The residual y - mu of clr_batch_set_mean -- or y - sum_k w_k Phi_k of clr_batch_set_mean_weights -- from the caller's
// series in `y_src`: one elementwise pass into `y`, where every route reads its series; the copies derived from `y` are
// then stale (a shared series with a per-problem mean becomes a per-problem residual: the copies are re-sized by the
// launches that rebuild them).  The factor of a materialising run does not depend on y and stays.
static int apply_mean(clr_batch* h, bool divide = true) {
  const long N = h->N;
  const bool linear = h->mean_K > 0;  // (its weights are per problem)
  const bool per_problem = linear || h->y_src_stride != 0 || h->mean_stride != 0;
  const int nout = per_problem ? h->B : 1;
  int st;
  if ((st = h->y.reserve((size_t)nout * N)) != CLR_OK) return st;
  const std::vector<double>& host = linear ? h->host_weights : h->host_mean;
  const size_t nm = host.size();
  if ((st = h->mean_dev.reserve(nm)) != CLR_OK) return st;
  // through pinned staging: the copy is asynchronous, and only the previous upload -- not the stream -- is waited for
  // before the staging is rewritten
  if (h->mean_ev) HIP_TRY(hipEventSynchronize(h->mean_ev.get()));
  else HIP_TRY(clr::create_event(h->mean_ev, hipEventDisableTiming));
  if ((st = h->mean_pin.reserve(nm)) != CLR_OK) return st;
  std::copy(host.begin(), host.end(), h->mean_pin.p);
  HIP_TRY(hipMemcpyAsync(h->mean_dev.p, h->mean_pin.p, nm * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
  HIP_TRY(hipEventRecord(h->mean_ev.get(), h->stream.get()));
  if (linear)
    clr::launch_linear_residual(h->y_src.p, h->y_src_stride, h->basis_dev.p, h->basis_stride, h->mean_dev.p, h->mean_K, nout,
                                (int)N, h->y.p, h->stream.get());
  else
    clr::launch_residual(h->y_src.p, h->y_src_stride, h->mean_dev.p, h->mean_stride, nout, (int)N, h->y.p, h->stream.get());
  // (per-problem lengths: the residual's tail stays the padding y = 0, not -mu -- the basis there is never looked at)
  if (h->ragged) clr::launch_pad_tail(h->y.p, h->B, (int)N, h->len_dev.p, 0, h->stream.get());
  HIP_TRY(hipGetLastError());
  residual_replaced(h, per_problem ? N : 0);
  if (divide && h->amp_active) return amplitude_divide(h, true, false);  // (every route reads r / s)
  return CLR_OK;
}

int clr_batch_set_mean(clr_batch* h, const double* mu, long mu_stride) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (mu && mu_stride != 0 && mu_stride != 1) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_mean: mu_stride is 1 (mu[B]) or 0 (one value)");
  const size_t n = mu ? (mu_stride ? (size_t)h->B : 1) : 0;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(mu[i])) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_mean: a non-finite mean");
  if (mu && h->mean_K > 0)
    return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_mean: a linear mean is in force (clr_batch_set_mean_basis) -- the two means "
                                      "are mutually exclusive: remove it first, or make the constant a basis function");
  if (mu && h->amp_K > 0)
    return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_mean: an amplitude basis is set (clr_batch_set_amplitude_basis) -- the constant "
                                      "mean and the amplitude model are mutually exclusive: a constant in data units is the "
                                      "mean-basis function 1 (clr_batch_set_mean_basis)");
  if (mu && h->have_mean && h->have_series && h->mean_stride == mu_stride && h->host_mean.size() == n &&
      memcmp(h->host_mean.data(), mu, n * sizeof(double)) == 0)
    return CLR_OK;  // (the residual in HBM is this mean's)
  if (!mu && !h->have_mean) return CLR_OK;
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;  // (an evaluation in flight is settled on ITS residual)
  if (!mu) {
    h->have_mean = false;
    h->host_mean.clear();
    if (h->have_series) {  // the caller's series is the pipeline's again
      std::swap(h->y, h->y_src);
      residual_replaced(h, h->y_src_stride);
    }
    return CLR_OK;
  }
  if (!h->have_mean && h->have_series) {  // the caller's series moves aside, `y` will hold the residual
    std::swap(h->y, h->y_src);
    h->y_src_stride = h->y_stride;
  }
  h->host_mean.assign(mu, mu + n);
  h->mean_stride = mu_stride;
  h->have_mean = true;
  if (!h->have_series) return CLR_OK;  // (clr_batch_set_series applies it)
  if ((st = apply_mean(h)) != CLR_OK) {
    h->have_series = false;  // (no half-formed residual is ever evaluated: set the series again)
    return st;
  }
  return CLR_OK;
}

/* ---- a mean linear in its parameters: clr_batch_set_mean_basis / _set_mean_weights / _grad_mean_weights ------------ */
int clr_batch_set_mean_basis(clr_batch* h, int K, const double* phi, long phi_stride) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (K <= 0 || !phi) {  // remove the linear mean: the caller's series is the pipeline's again
    if (K < 0) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_mean_basis: K >= 0");
    if (h->mean_K == 0) return CLR_OK;
    if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;  // (an evaluation in flight is settled on ITS residual)
    h->mean_K = 0;
    h->host_weights.clear();
    if (h->have_series && h->amp_active) {  // (the amplitudes stay: y' = y / s from the caller's series)
      if ((st = amplitude_divide(h, true, false)) != CLR_OK) h->have_series = false;
      return st;
    }
    if (h->have_series) {
      std::swap(h->y, h->y_src);
      residual_replaced(h, h->y_src_stride);
    }
    return CLR_OK;
  }
  if (K > CLR_MAX_MEAN_BASIS) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_mean_basis: at most CLR_MAX_MEAN_BASIS = 16 basis functions");
  const size_t per = (size_t)K * (size_t)h->N;
  if (phi_stride != 0 && phi_stride != (long)per)
    return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_mean_basis: phi_stride is 0 (phi[K][N], shared) or K * N (phi[B][K][N])");
  if (h->have_mean)
    return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_mean_basis: a constant mean is in force (clr_batch_set_mean) -- the two means "
                                      "are mutually exclusive: remove it first, or make the constant a basis function");
  const size_t n = phi_stride ? per * (size_t)h->B : per;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(phi[i])) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_mean_basis: a non-finite basis entry");
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;
  HIP_TRY(hipStreamSynchronize(h->stream.get()));  // (a residual pass in flight may still read the previous basis)
  if ((st = h->basis_dev.reserve(n)) != CLR_OK) return st;
  HIP_TRY(hipMemcpy(h->basis_dev.p, phi, n * sizeof(double), hipMemcpyHostToDevice));
  if (h->mean_K == 0 && h->have_series && !h->amp_active) {  // the caller's series moves aside, `y` will hold the residual
    std::swap(h->y, h->y_src);
    h->y_src_stride = h->y_stride;
  }
  h->mean_K = K;
  h->basis_stride = phi_stride;
  h->host_weights.assign((size_t)h->B * K, 0.0);  // (a new basis starts from zero weights: the residual is y)
  if (!h->have_series) return CLR_OK;  // (clr_batch_set_series applies it)
  if ((st = apply_mean(h)) != CLR_OK) {
    h->have_series = false;  // (no half-formed residual is ever evaluated: set the series again)
    return st;
  }
  return CLR_OK;
}

int clr_batch_set_mean_weights(clr_batch* h, const double* w) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (h->mean_K == 0) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_mean_weights: no basis is set (clr_batch_set_mean_basis)");
  if (!w) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_mean_weights: w is null");
  const size_t n = (size_t)h->B * h->mean_K;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(w[i])) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_mean_weights: a non-finite weight");
  if (memcmp(h->host_weights.data(), w, n * sizeof(double)) == 0) return CLR_OK;  // (the residual in force is these weights')
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;  // (an evaluation in flight is settled on ITS residual)
  h->host_weights.assign(w, w + n);
  if (!h->have_series) return CLR_OK;  // (clr_batch_set_series applies them)
  if ((st = apply_mean(h)) != CLR_OK) {
    h->have_series = false;
    return st;
  }
  return CLR_OK;
}

/* ---- a noise model linear in its parameters: clr_batch_set_noise_basis / _set_noise_weights ------------------------ */
// The variances diag + sum_k s_k Psi_k of clr_batch_set_noise_weights from the caller's diagonal in `diag_src`: one
// elementwise pass into `diag`, where every route reads its variances (apply_mean's pattern for y); what is derived from
// `diag` is then stale (variance_replaced).  The weights are per problem, so a shared diagonal becomes B x N variances.
static int apply_noise(clr_batch* h, bool divide = true) {
  const long N = h->N;
  int st;
  if ((st = h->diag.reserve((size_t)h->B * N)) != CLR_OK) return st;
  const size_t nw = h->host_noise.size();
  if ((st = h->noise_dev.reserve(nw)) != CLR_OK) return st;
  // through pinned staging: the copy is asynchronous, and only the previous upload -- not the stream -- is waited for
  // before the staging is rewritten
  if (h->noise_ev) HIP_TRY(hipEventSynchronize(h->noise_ev.get()));
  else HIP_TRY(clr::create_event(h->noise_ev, hipEventDisableTiming));
  if ((st = h->noise_pin.reserve(nw)) != CLR_OK) return st;
  std::copy(h->host_noise.begin(), h->host_noise.end(), h->noise_pin.p);
  HIP_TRY(hipMemcpyAsync(h->noise_dev.p, h->noise_pin.p, nw * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
  HIP_TRY(hipEventRecord(h->noise_ev.get(), h->stream.get()));
  clr::launch_noise_form(h->diag_src.p, h->diag_src_stride, h->noise_basis.p, h->noise_stride, h->noise_dev.p, h->noise_K, h->B,
                         (int)N, h->diag.p, h->stream.get());
  // (per-problem lengths: the variances' tail stays the padding 1e300 -- the basis there is never looked at)
  if (h->ragged) clr::launch_pad_tail(h->diag.p, h->B, (int)N, h->len_dev.p, 2, h->stream.get());
  HIP_TRY(hipGetLastError());
  variance_replaced(h, N);
  if (divide && h->amp_active) return amplitude_divide(h, false, true);  // (every route reads diag_eff / (s * s))
  return CLR_OK;
}

int clr_batch_set_noise_basis(clr_batch* h, int K, const double* psi, long psi_stride) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (K <= 0 || !psi) {  // remove the noise model: the caller's diagonal is the pipeline's again
    if (K < 0) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_noise_basis: K >= 0");
    if (h->noise_K == 0) return CLR_OK;
    if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;  // (an evaluation in flight is settled on ITS variances)
    h->noise_K = 0;
    h->host_noise.clear();
    if (h->have_series && h->amp_active) {  // (the amplitudes stay: d' = diag / (s * s) from the caller's diagonal)
      if ((st = amplitude_divide(h, false, true)) != CLR_OK) h->have_series = false;
      return st;
    }
    if (h->have_series) {
      std::swap(h->diag, h->diag_src);
      variance_replaced(h, h->diag_src_stride);
    }
    return CLR_OK;
  }
  if (K > CLR_MAX_NOISE_BASIS) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_noise_basis: at most CLR_MAX_NOISE_BASIS = 16 basis functions");
  const size_t per = (size_t)K * (size_t)h->N;
  if (psi_stride != 0 && psi_stride != (long)per)
    return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_noise_basis: psi_stride is 0 (psi[K][N], shared) or K * N (psi[B][K][N])");
  const size_t n = psi_stride ? per * (size_t)h->B : per;
  // (per-problem lengths in force: a row's tail is never looked at and may hold anything -- of a shared basis the tail past
  //  the longest problem)
  const size_t longest = h->ragged ? (size_t)*std::max_element(h->host_len.begin(), h->host_len.end()) : (size_t)h->N;
  for (size_t r = 0; r < n / (size_t)h->N; ++r) {
    const size_t len = (h->ragged && psi_stride) ? (size_t)h->host_len[r / (size_t)K] : longest;
    for (size_t i = 0; i < len; ++i)
      if (!std::isfinite(psi[r * (size_t)h->N + i])) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_noise_basis: a non-finite basis entry");
  }
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;
  HIP_TRY(hipStreamSynchronize(h->stream.get()));  // (a forming pass in flight may still read the previous basis)
  if ((st = h->noise_basis.reserve(n)) != CLR_OK) return st;
  HIP_TRY(hipMemcpy(h->noise_basis.p, psi, n * sizeof(double), hipMemcpyHostToDevice));
  if (h->noise_K == 0 && h->have_series && !h->amp_active) {  // the caller's diagonal moves aside, `diag` will hold the variances
    std::swap(h->diag, h->diag_src);
    h->diag_src_stride = h->diag_stride;
  }
  h->noise_K = K;
  h->noise_stride = psi_stride;
  h->host_noise.assign((size_t)h->B * K, 0.0);  // (a new basis starts from zero weights: the variances are diag)
  if (!h->have_series) return CLR_OK;  // (clr_batch_set_series applies it)
  if ((st = apply_noise(h)) != CLR_OK) {
    h->have_series = false;  // (no half-formed diagonal is ever evaluated: set the series again)
    return st;
  }
  return CLR_OK;
}

int clr_batch_set_noise_weights(clr_batch* h, const double* w) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (h->noise_K == 0) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_noise_weights: no basis is set (clr_batch_set_noise_basis)");
  if (!w) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_noise_weights: s is null");
  const size_t n = (size_t)h->B * h->noise_K;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(w[i])) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_noise_weights: a non-finite weight");
  if (memcmp(h->host_noise.data(), w, n * sizeof(double)) == 0) return CLR_OK;  // (the variances in force are these weights')
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;  // (an evaluation in flight is settled on ITS variances)
  h->host_noise.assign(w, w + n);
  if (!h->have_series) return CLR_OK;  // (clr_batch_set_series applies them)
  if ((st = apply_noise(h)) != CLR_OK) {
    h->have_series = false;
    return st;
  }
  return CLR_OK;
}

/* ---- a per-sample amplitude model: clr_batch_set_amplitude_basis / _set_amplitudes ---------------------------------- */
// The log terms of the evaluation in force move to the host before the forming pass overwrites them (amp_eval: 0 the
// evaluation in force ran without amplitudes, 1 its terms are still the ones in amp_back, 2 they are in host_amp_L)
static int amplitude_snapshot(clr_batch* h) {
  if (h->amp_eval != 1) return CLR_OK;
  HIP_TRY(hipEventSynchronize(h->amp_back_ev.get()));
  h->host_amp_L.assign(h->amp_back.p, h->amp_back.p + 2 * (size_t)h->B);
  h->amp_eval = 2;
  return CLR_OK;
}

// The scale s of the amplitudes in force into `amp_s`, its log term and flags (fetched asynchronously: amp_back); then the
// residual and the variances formed again where a mean or a noise model is in force, and the two divisions.
static int apply_amplitudes(clr_batch* h) {
  const long N = h->N;
  const size_t B = (size_t)h->B;
  int st;
  if ((st = amplitude_snapshot(h)) != CLR_OK) return st;
  if ((st = h->amp_s.reserve(B * (size_t)N)) != CLR_OK) return st;
  if ((st = h->amp_part.reserve(clr::amplitude_scale_workspace(h->B, h->N))) != CLR_OK) return st;
  if ((st = h->amp_Lf.reserve(2 * B)) != CLR_OK) return st;
  const size_t na = h->host_amp.size();
  if ((st = h->amp_dev.reserve(na)) != CLR_OK) return st;
  // through pinned staging, as the noise weights
  if (h->amp_ev) HIP_TRY(hipEventSynchronize(h->amp_ev.get()));
  else HIP_TRY(clr::create_event(h->amp_ev, hipEventDisableTiming));
  if ((st = h->amp_pin.reserve(na)) != CLR_OK) return st;
  std::copy(h->host_amp.begin(), h->host_amp.end(), h->amp_pin.p);
  HIP_TRY(hipMemcpyAsync(h->amp_dev.p, h->amp_pin.p, na * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
  HIP_TRY(hipEventRecord(h->amp_ev.get(), h->stream.get()));
  if (!clr::launch_amplitude_scale(h->amp_basis.p, h->amp_stride, h->amp_dev.p, h->amp_K, h->B, (int)N,
                                   h->ragged ? h->len_dev.p : nullptr, h->amp_s.p, h->amp_part.p, h->amp_Lf.p, h->stream.get()))
    return fail(CLR_UNSUPPORTED, "clr_batch_set_amplitudes: B x N / 4096 workgroups do not fit one launch");
  if (h->amp_back_ev) HIP_TRY(hipEventSynchronize(h->amp_back_ev.get()));
  else HIP_TRY(clr::create_event(h->amp_back_ev, hipEventDisableTiming));
  if ((st = h->amp_back.reserve(2 * B)) != CLR_OK) return st;
  HIP_TRY(hipMemcpyAsync(h->amp_back.p, h->amp_Lf.p, 2 * B * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  HIP_TRY(hipEventRecord(h->amp_back_ev.get(), h->stream.get()));
  h->amp_formed = true;
  if (h->mean_K > 0 && (st = apply_mean(h, false)) != CLR_OK) return st;
  if (h->noise_K > 0 && (st = apply_noise(h, false)) != CLR_OK) return st;
  return amplitude_divide(h, true, true);
}

// amplitudes in force -> none: the residual and the variances the plan read before them, bit for bit
static int amplitudes_dropped(clr_batch* h) {
  if (!h->amp_active) return CLR_OK;
  int st;
  if ((st = amplitude_snapshot(h)) != CLR_OK) return st;
  h->amp_active = h->amp_formed = false;
  h->host_amp.clear();
  if (!h->have_series) return CLR_OK;
  if (h->mean_K > 0) st = apply_mean(h);
  else { std::swap(h->y, h->y_src); residual_replaced(h, h->y_src_stride); }
  if (st == CLR_OK) {
    if (h->noise_K > 0) st = apply_noise(h);
    else { std::swap(h->diag, h->diag_src); variance_replaced(h, h->diag_src_stride); }
  }
  if (st != CLR_OK) h->have_series = false;  // (no half-formed series is ever evaluated: set the series again)
  return st;
}

int clr_batch_set_amplitude_basis(clr_batch* h, int K, const double* gamma, long gamma_stride) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (K <= 0 || !gamma) {  // remove the amplitude model: the plain plan again
    if (K < 0) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_amplitude_basis: K >= 0");
    if (h->amp_K == 0) return CLR_OK;
    if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;  // (an evaluation in flight is settled on ITS series)
    h->amp_K = 0;
    return amplitudes_dropped(h);
  }
  if (K > CLR_MAX_AMPLITUDE_BASIS)
    return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_amplitude_basis: at most CLR_MAX_AMPLITUDE_BASIS = 16 basis functions");
  const size_t per = (size_t)K * (size_t)h->N;
  if (gamma_stride != 0 && gamma_stride != (long)per)
    return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_amplitude_basis: gamma_stride is 0 (gamma[K][N], shared) or K * N (gamma[B][K][N])");
  if (h->have_mean)
    return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_amplitude_basis: a constant mean is in force (clr_batch_set_mean) -- the constant "
                                      "mean and the amplitude model are mutually exclusive: remove it first; a constant in data "
                                      "units is the mean-basis function 1 (clr_batch_set_mean_basis)");
  const size_t n = gamma_stride ? per * (size_t)h->B : per;
  // (per-problem lengths in force: a row's tail is never looked at and may hold anything -- of a shared basis the tail past
  //  the longest problem)
  const size_t longest = h->ragged ? (size_t)*std::max_element(h->host_len.begin(), h->host_len.end()) : (size_t)h->N;
  for (size_t r = 0; r < n / (size_t)h->N; ++r) {
    const size_t len = (h->ragged && gamma_stride) ? (size_t)h->host_len[r / (size_t)K] : longest;
    for (size_t i = 0; i < len; ++i)
      if (!std::isfinite(gamma[r * (size_t)h->N + i]))
        return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_amplitude_basis: a non-finite basis entry");
  }
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;
  HIP_TRY(hipStreamSynchronize(h->stream.get()));  // (a forming pass in flight may still read the previous basis)
  if ((st = h->amp_basis.reserve(n)) != CLR_OK) return st;
  HIP_TRY(hipMemcpy(h->amp_basis.p, gamma, n * sizeof(double), hipMemcpyHostToDevice));
  h->amp_K = K;
  h->amp_stride = gamma_stride;
  // a new basis drops the amplitudes in force: zero amplitudes are no neutral start (s = 0), so the plan is the plain plan
  // until clr_batch_set_amplitudes
  return amplitudes_dropped(h);
}

int clr_batch_set_amplitudes(clr_batch* h, const double* a) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (h->amp_K == 0) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_amplitudes: no basis is set (clr_batch_set_amplitude_basis)");
  if (!a) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_amplitudes: a is null");
  const size_t n = (size_t)h->B * h->amp_K;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_amplitudes: a non-finite amplitude");
  if (h->amp_active && memcmp(h->host_amp.data(), a, n * sizeof(double)) == 0) return CLR_OK;  // (the series in force are these amplitudes')
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;  // (an evaluation in flight is settled on ITS series)
  h->host_amp.assign(a, a + n);
  if (!h->amp_active && h->have_series) {
    // the caller's arrays move aside unless a mean / a noise model has moved them already
    if (h->mean_K == 0) { std::swap(h->y, h->y_src); h->y_src_stride = h->y_stride; }
    if (h->noise_K == 0) { std::swap(h->diag, h->diag_src); h->diag_src_stride = h->diag_stride; }
  }
  h->amp_active = true;
  if (!h->have_series) return CLR_OK;  // (clr_batch_set_series applies them)
  if ((st = apply_amplitudes(h)) != CLR_OK) {
    h->have_series = false;  // (no half-formed series is ever evaluated: set the series again)
    return st;
  }
  return CLR_OK;
}

int clr_batch_get_log_amplitude_sum(clr_batch* h, double* L) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (!L) return fail(CLR_INVALID_ARGUMENT, "clr_batch_get_log_amplitude_sum: L is null");
  std::fill(L, L + h->B, 0.0);
  if (!h->amp_active || !h->amp_formed) return CLR_OK;  // (no amplitudes in force, or no series to form them on yet)
  HIP_TRY(hipEventSynchronize(h->amp_back_ev.get()));
  std::copy(h->amp_back.p, h->amp_back.p + h->B, L);
  return CLR_OK;
}

// `L`: the log terms and, behind them, the flags of B problems
static void amplitude_fold(const clr_batch* h, const double* L, double* loglike, double* logdet, double* quad, int* status) {
  const double* flag = L + h->B;
  for (size_t b = 0; b < (size_t)h->B; ++b) {
    if (flag[b] != 0.0) {  // a zero or non-finite s_n inside the problem's length: the draw is refused
      if (loglike) loglike[b] = NAN;
      if (logdet) logdet[b] = NAN;
      if (quad) quad[b] = NAN;
      if (status) status[b] = CLR_INVALID_ARGUMENT;
      continue;
    }
    if (logdet) logdet[b] = logdet[b] + (L[b] + L[b]);
    if (loglike) loglike[b] = loglike[b] - L[b];
  }
}

// The log term of the EVALUATION in force, into its results
extern "C++" int amplitude_adjust(clr_batch* h, double* loglike, double* logdet, double* quad, int* status) {
  if (h->amp_eval == 0) return CLR_OK;
  const int st = amplitude_snapshot(h);
  if (st != CLR_OK) return st;
  amplitude_fold(h, h->host_amp_L.data(), loglike, logdet, quad, status);
  return CLR_OK;
}

// The log term of the AMPLITUDES in force, into a value formed from the series in force with no evaluation in front (the
// sequential plan gradient of widths 33..64): the evaluation in force, its results and amp_eval stay as they are
extern "C++" int amplitude_adjust_in_force(clr_batch* h, double* loglike, int* status) {
  if (!h->amp_active || !h->amp_formed) return CLR_OK;
  HIP_TRY(hipEventSynchronize(h->amp_back_ev.get()));
  amplitude_fold(h, h->amp_back.p, loglike, nullptr, nullptr, status);
  return CLR_OK;
}

// clr_batch_set_series and clr_batch_set_series_ragged.  `lengths` (host, [B], may be null): problem b is the first
// lengths[b] entries of its rows; `ragged`: lengths are in force -- some length of the WHOLE batch differs from N (a
// slice of a larger batch is told so: clr_group::set_series_lengths).  Everything is checked before the plan changes.
static int set_series_impl(clr_batch* h, const double* t, long t_stride, const double* diag, long diag_stride,
                           const double* y, long y_stride, const int* lengths, bool ragged) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  const long N = h->N;
  for (long sd : {t_stride, diag_stride, y_stride})
    if (sd != 0 && sd != N)
      return fail(CLR_INVALID_ARGUMENT, "series stride must be 0 (shared) or N");
  if (lengths)
    for (int b = 0; b < h->B; ++b)
      if (lengths[b] < 1 || lengths[b] > N)
        return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_series_ragged: length " + std::to_string(lengths[b]) + " of problem " +
                                          std::to_string(b) + " is outside [1, N = " + std::to_string(N) + "]");
  if (ragged) {
    if (t_stride == 0 || diag_stride == 0 || y_stride == 0)
      return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_series_ragged: with lengths t, diag and y are each [B][N] (stride N) -- "
                                        "the padded device copy is per problem");
    if (!h->launch || h->J_general > 0)
      return fail(CLR_UNSUPPORTED, "clr_batch_set_series_ragged: per-problem lengths cover narrow plans (widths 1..8) without "
                                   "general terms");
    if (h->warm_mode == 1 || h->small_mode == 1 || h->summarize_mode > 0)
      return fail(CLR_UNSUPPORTED, "clr_batch_set_series_ragged: the forced warm start, one-launch mode and role-split summarize "
                                   "(clr_batch_set_summarize_mode 1, 2) do not carry per-problem lengths: switch them back to "
                                   "automatic first");
  }
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;  // (an evaluation in flight is settled on ITS series)
  if (ragged && (st = h->len_dev.reserve((size_t)h->B)) != CLR_OK) return st;
  auto count = [&](long sd) { return (size_t)(sd == 0 ? N : N * (long)h->B); };
  const auto host_t0 = std::chrono::steady_clock::now();
  if ((st = h->t.reserve(count(t_stride))) != CLR_OK) return st;
  if ((st = h->diag.reserve(count(diag_stride))) != CLR_OK) return st;
  if ((st = h->y.reserve(count(y_stride))) != CLR_OK) return st;
  HIP_TRY(hipStreamSynchronize(h->stream.get()));  // (kernels of an earlier evaluation may still be reading the old series)
  // from here on the old series is being overwritten: the plan has NO series until every copy and scan below has
  // succeeded (a failed upload must not leave have_series set over half-written arrays), and nothing derived from
  // the old one -- interleaved copies, warm-up spans and their selection -- survives
  h->have_series = false;
  series_replaced(h);
  if (h->ragged != ragged) {  // (a factor and a rescue side plan belong to the other kind of plan)
    factor_dropped(h);
    h->rescue.reset();
    h->rescue_plan_key = -1;
  }
  h->ragged = ragged;
  if (ragged) h->host_len.assign(lengths, lengths + h->B); else h->host_len.clear();
  const clr::CopyJob jobs[3] = {{h->t.p, t, count(t_stride)}, {h->diag.p, diag, count(diag_stride)}, {h->y.p, y, count(y_stride)}};
  const size_t total = (jobs[0].n + jobs[1].n + jobs[2].n) * sizeof(double);
  bool staged = false;
  if (total >= ((size_t)32 << 20)) {
    // large series: NT host threads stage pieces through pinned buffers, their DMAs share the link (clr_series_io.h);
    // no pinned memory to be had (64 MB): the plain copies below
    if (clr::staging_create(h->staging, h->device) == 0) {
      const int e = clr::upload_parallel(h->staging, jobs, 3);
      if (e != 0) return fail(CLR_HIP_ERROR, hipGetErrorString((hipError_t)e));
      staged = true;
    } else {
      h->staging = clr::UploadStaging();
      (void)hipGetLastError();
    }
  }
  if (!staged) {
    for (const clr::CopyJob& j : jobs)
      if (j.n) HIP_TRY(hipMemcpyAsync(j.dst, j.src, j.n * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
    HIP_TRY(hipStreamSynchronize(h->stream.get()));
  }
  h->t_stride = t_stride;
  h->diag_stride = diag_stride;
  h->y_stride = y_stride;
  if (ragged) {
    // the tails become padding IN the resident arrays, before anything looks at them: t held, diagonal 1e300, y = 0 --
    // every scan below, every copy and every kernel then sees rows whose entries past len[b] a recurrence step ignores
    HIP_TRY(hipMemcpyAsync(h->len_dev.p, h->host_len.data(), (size_t)h->B * sizeof(int), hipMemcpyHostToDevice, h->stream.get()));
    clr::launch_pad_tail(h->t.p, h->B, (int)N, h->len_dev.p, 1, h->stream.get());
    clr::launch_pad_tail(h->diag.p, h->B, (int)N, h->len_dev.p, 2, h->stream.get());
    clr::launch_pad_tail(h->y.p, h->B, (int)N, h->len_dev.p, 0, h->stream.get());
    HIP_TRY(hipGetLastError());
  }
  // one pass over t ON THE DEVICE: max |t| over every sample (sortedness is not assumed), the largest and the smallest
  // step, NaN times; then the warm path's spans
  {
    const int nb = t_stride == 0 ? 1 : h->B;
    if ((st = h->scan.reserve((size_t)nb * std::max(4, (int)clr_batch::WARM_NK))) != CLR_OK) return st;
    clr::launch_series_stats(h->t.p, t_stride, nb, (int)N, ragged ? h->len_dev.p : nullptr, h->scan.p, h->stream.get());
    std::vector<double> stats((size_t)nb * 4);
    HIP_TRY(hipMemcpyAsync(stats.data(), h->scan.p, stats.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
    HIP_TRY(hipStreamSynchronize(h->stream.get()));
    double tm = 0.0, dm = 0.0, dmin = INFINITY;
    bool nan = false;
    for (int b = 0; b < nb; ++b) {
      tm = std::max(tm, stats[4 * b]); dm = std::max(dm, stats[4 * b + 1]); dmin = std::min(dmin, stats[4 * b + 2]);
      nan = nan || stats[4 * b + 3] != 0.0;
    }
    // (a NaN time: NaN bounds select the conservative kernels, sel_max)
    h->tmax = nan ? NAN : tm;
    h->dxmax = nan ? NAN : dm;
    // the smallest step over the finite differences (the device's fmin skips NaN); a negative one means "not sorted"
    // whatever else the series holds -- the reference's np.any(np.diff(t) < 0), celerite.py:126-129 -- and only a
    // series without a negative step reports its NaN times as NaN
    const double finite_min = (N > 1 && dmin != INFINITY) ? dmin : 0.0;  // (no step at all: one-sample series)
    h->dtmin = (finite_min < 0.0) ? finite_min : (nan ? NAN : finite_min);
  }
  h->have_series = true;
  if (h->have_mean || h->mean_K > 0 || h->amp_active) {  // (the upload went to `y`: it becomes the caller's series, `y` the residual)
    std::swap(h->y, h->y_src);
    h->y_src_stride = y_stride;
    if (!h->amp_active && (st = apply_mean(h)) != CLR_OK) { h->have_series = false; return st; }
  }
  if (h->noise_K > 0 || h->amp_active) {  // (the upload went to `diag`: it becomes the caller's diagonal, `diag` the variances)
    std::swap(h->diag, h->diag_src);
    h->diag_src_stride = diag_stride;
    if (!h->amp_active && (st = apply_noise(h)) != CLR_OK) { h->have_series = false; return st; }
  }
  // (amplitudes in force: the scale and its log term over the new lengths, then the residual, the variances and both divisions)
  if (h->amp_active && (st = apply_amplitudes(h)) != CLR_OK) { h->have_series = false; return st; }
  if ((st = warm_scan_spans(h)) != CLR_OK) { h->have_series = false; return st; }
  h->set_series_host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count();
  // a new series: the warm-ups chosen for the previous one's spans do not apply, nor does its history of fallbacks
  if (h->warm_mode < 0) h->warm_boost = 0;
  warm_select(h);
  return CLR_OK;
}

int clr_batch_set_series(clr_batch* h, const double* t, long t_stride, const double* diag,
                         long diag_stride, const double* y, long y_stride) {
  return set_series_impl(h, t, t_stride, diag, diag_stride, y, y_stride, nullptr, false);
}

int clr_batch_set_series_ragged(clr_batch* h, const double* t, long t_stride, const double* diag, long diag_stride,
                                const double* y, long y_stride, const int* lengths) {
  bool ragged = false;  // (lengths that all equal N are the uniform plan)
  if (lengths)
    for (int b = 0; b < h->B; ++b) ragged = ragged || lengths[b] != h->N;
  return set_series_impl(h, t, t_stride, diag, diag_stride, y, y_stride, lengths, ragged);
}

int clr_batch_get_lengths(const clr_batch* h, int* lengths) {
  if (!lengths) return fail(CLR_INVALID_ARGUMENT, "clr_batch_get_lengths: lengths is null");
  if (!h->have_series) return fail(CLR_INVALID_ARGUMENT, "no series set");
  for (int b = 0; b < h->B; ++b) lengths[b] = h->ragged ? h->host_len[b] : h->N;
  return CLR_OK;
}

int clr_batch_get_series_order(const clr_batch* h, double* dtmin) {
  if (!h->have_series) return fail(CLR_INVALID_ARGUMENT, "no series set");
  if (dtmin) *dtmin = h->dtmin;
  return CLR_OK;
}

int clr_batch_clear_series(clr_batch* h) {
  int st = warm_resolve(h, nullptr);
  if (st != CLR_OK) return st;
  h->have_series = false;
  h->warm_active = false;
  h->warm_span.clear();
  h->ragged = false;  // (the lengths belonged to the series)
  h->host_len.clear();
  return CLR_OK;
}

int clr_batch_get_selection_bounds(const clr_batch* h, double* tmax, double* dxmax, double* dmax, double* cmax,
                                   double* set_series_host_ms) {
  if (tmax) *tmax = h->tmax;
  if (dxmax) *dxmax = h->dxmax;
  if (dmax) *dmax = h->dmax;
  if (cmax) *cmax = h->cmax;
  if (set_series_host_ms) *set_series_host_ms = h->set_series_host_ms;
  return CLR_OK;
}

int clr_batch_set_selection_bounds(clr_batch* h, double tmax, double dxmax, double dmax, double cmax) {
  // negative: leave that floor as it is (NaN counts as "unbounded": the conservative kernels)
  if (!(tmax < 0.0)) h->floor_tmax = tmax;
  if (!(dxmax < 0.0)) h->floor_dxmax = dxmax;
  if (!(dmax < 0.0)) h->floor_dmax = dmax;
  if (!(cmax < 0.0)) h->floor_cmax = cmax;
  return CLR_OK;
}

static int reserve_pinned(clr_batch* h, size_t doubles) {
  if (doubles <= h->pin.cap && h->pin.p) return CLR_OK;
  h->pin_results = false;
  if (h->pin.p) HIP_TRY(hipStreamSynchronize(h->stream.get()));
  return h->pin.reserve(doubles);
}

// Coefficients come in two ways -- as tables from the host (clr_batch_set_coefficients) or formed on the device from
// kernel parameters (clr_batch_set_parameters) -- and both go through the same two halves: the statistics the
// selection looks at (largest frequency and decay rate of the batch, smallest / largest decay rate and jitter per
// problem) -> warm_select, then the coefficients placed in h->coeffs with the warm path's K per problem behind them.
static int begin_coefficients(clr_batch* h) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;  // (pending problems of the evaluation in flight: at ITS coefficients)
  coefficients_replaced(h);
  return CLR_OK;
}

// doubles of the pinned staging buffer a coefficient upload needs; the warm path's K per problem sits at warm_K_offset
static size_t warm_K_offset(const clr_batch* h) {
  const size_t B = (size_t)h->B;
  return std::max(B * (2 * (size_t)h->J_real + 4 * (size_t)h->J_comp + 1), 3 * B + (B + 1) / 2);
}

static int place_warm_K(clr_batch* h) {
  const size_t B = (size_t)h->B;
  if (h->warm_active) {  // K per problem, behind the coefficients in the staging buffer
    int* kk = reinterpret_cast<int*>(h->pin.p + warm_K_offset(h));
    memcpy(kk, h->warm_K.data(), B * sizeof(int));
    HIP_TRY(hipMemcpyAsync(h->wints.p + (size_t)h->B * h->wnchunk + B, kk, B * sizeof(int), hipMemcpyHostToDevice, h->stream.get()));
    h->warm_K_dirty = false;
  }
  h->have_coeffs = true;
  return CLR_OK;
}

int clr_batch_set_coefficients(clr_batch* h, const double* jitter, const double* a_real,
                               const double* c_real, const double* a_comp, const double* b_comp,
                               const double* c_comp, const double* d_comp) {
  int st = begin_coefficients(h);
  if (st != CLR_OK) return st;
  const size_t B = (size_t)h->B, nr = B * h->J_real, nc = B * h->J_comp;
  h->dmax = 0.0;
  h->cmax = 0.0;
  h->b_zero = true;
  for (size_t i = 0; i < nc; ++i) {
    const double m = fabs(d_comp[i]), c = fabs(c_comp[i]);
    if (!(m <= h->dmax)) h->dmax = m;
    if (!(c <= h->cmax)) h->cmax = c;
    if (!(b_comp[i] == 0.0)) h->b_zero = false;
  }
  for (size_t i = 0; i < nr; ++i) {
    const double c = fabs(c_real[i]);
    if (!(c <= h->cmax)) h->cmax = c;
  }
  h->host_cmax.assign(B, 0.0);
  for (size_t b = 0; b < B; ++b) {
    double m = 0.0;
    for (int j = 0; j < h->J_real; ++j) m = std::max(m, fabs(c_real[b * h->J_real + j]));
    for (int j = 0; j < h->J_comp; ++j) m = std::max(m, fabs(c_comp[b * h->J_comp + j]));
    h->host_cmax[b] = m;
  }
  h->host_cmin.assign(B, INFINITY);
  for (size_t b = 0; b < B; ++b) {
    double cmin = INFINITY;
    for (int j = 0; j < h->J_real; ++j) { const double c = c_real[b * h->J_real + j]; if (!(c >= cmin)) cmin = c; }
    for (int j = 0; j < h->J_comp; ++j) { const double c = c_comp[b * h->J_comp + j]; if (!(c >= cmin)) cmin = c; }
    h->host_cmin[b] = cmin;
  }
  if (jitter) h->host_jitter.assign(jitter, jitter + B);
  else h->host_jitter.assign(B, 0.0);  // NULL: no jitter
  warm_select(h);
  // one pinned staging buffer, one copy: a_real c_real a_comp b_comp c_comp d_comp | jitter
  const size_t total = 2 * nr + 4 * nc + B;
  if ((st = reserve_pinned(h, warm_K_offset(h) + (B + 1) / 2)) != CLR_OK) return st;
  HIP_TRY(hipStreamSynchronize(h->stream.get()));  // (a previous upload may still read the staging buffer)
  double* w = h->pin.p;
  auto put = [&](const double* p, size_t n) { if (n) memcpy(w, p, n * sizeof(double)); w += n; };
  put(a_real, nr); put(c_real, nr); put(a_comp, nc); put(b_comp, nc); put(c_comp, nc); put(d_comp, nc);
  if (jitter) put(jitter, B);
  else memset(w, 0, B * sizeof(double));
  if ((st = h->coeffs.reserve(total)) != CLR_OK) return st;
  HIP_TRY(hipMemcpyAsync(h->coeffs.p, h->pin.p, total * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
  return place_warm_K(h);
}

/* ---- coefficients from kernel parameters, formed on the device (kernel_program.hip) ------------------------------ */
int clr_batch_set_kernel(clr_batch* h, const clr_kernel* k) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (!k) {
    h->have_kernel = false;
    h->kp_in_force = false;
    return CLR_OK;
  }
  if (k->J_real != h->J_real || k->J_comp != h->J_comp)
    return fail(CLR_DIMENSION_MISMATCH, "clr_batch_set_kernel: the kernel's (J_real, J_comp) is not the plan's");
  if ((st = h->kp_ops.reserve(k->ops.size())) != CLR_OK) return st;
  if ((st = h->kp_consts.reserve(k->consts.size())) != CLR_OK) return st;
  HIP_TRY(hipStreamSynchronize(h->stream.get()));  // (a kernel in flight may still read the previous program)
  h->kp = *k;
  if (!k->ops.empty()) HIP_TRY(hipMemcpy(h->kp_ops.p, k->ops.data(), k->ops.size() * sizeof(int), hipMemcpyHostToDevice));
  if (!k->consts.empty()) HIP_TRY(hipMemcpy(h->kp_consts.p, k->consts.data(), k->consts.size() * sizeof(double), hipMemcpyHostToDevice));
  h->have_kernel = true;
  h->kp_in_force = false;
  return CLR_OK;
}

static clr::KernelProgramDevice device_program(const clr_batch* h) {
  return clr::KernelProgramDevice{h->kp_ops.p, h->kp_consts.p, (int)h->kp.ops.size(), (int)h->kp.consts.size(),
                                  h->kp.n_params, h->kp.J_real, h->kp.J_comp};
}

int clr_batch_set_parameters(clr_batch* h, const double* params) {
  int st = begin_coefficients(h);
  if (st != CLR_OK) return st;
  if (!h->have_kernel) return fail(CLR_NOT_COMPUTED, "clr_batch_set_parameters: no kernel is set (clr_batch_set_kernel)");
  const size_t B = (size_t)h->B, P = (size_t)h->kp.n_params, NC = 2 * (size_t)h->J_real + 4 * (size_t)h->J_comp;
  if (!params && P > 0) return fail(CLR_INVALID_ARGUMENT, "clr_batch_set_parameters: params is null");
  const size_t nstat = clr::KP_NSTAT * B;
  if ((st = reserve_pinned(h, std::max(warm_K_offset(h) + (B + 1) / 2, B * P + nstat))) != CLR_OK) return st;
  if ((st = h->kp_params.reserve(B * P + nstat)) != CLR_OK) return st;
  if ((st = h->coeffs.reserve(B * NC + B)) != CLR_OK) return st;
  HIP_TRY(hipStreamSynchronize(h->stream.get()));  // (a previous upload may still read the staging buffer)
  if (P) memcpy(h->pin.p, params, B * P * sizeof(double));
  if (P) HIP_TRY(hipMemcpyAsync(h->kp_params.p, h->pin.p, B * P * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
  double* dstats = h->kp_params.p + B * P;
  clr::launch_kernel_program_eval(device_program(h), h->B, h->kp_params.p, h->coeffs.p, dstats, h->stream.get());
  HIP_TRY(hipGetLastError());
  // the statistics of the coefficients just formed: one small block, one transfer
  const double* s = h->pin.p + B * P;
  HIP_TRY(hipMemcpyAsync(h->pin.p + B * P, dstats, nstat * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  h->dmax = 0.0;
  h->cmax = 0.0;
  h->b_zero = false;  // (the program's statistics do not say: the general features)
  for (size_t b = 0; b < B; ++b) {
    const double m = s[clr::KP_STAT_DMAX * B + b], c = s[clr::KP_STAT_CMAX * B + b];
    if (!(m <= h->dmax)) h->dmax = m;
    if (!(c <= h->cmax)) h->cmax = c;
  }
  h->host_cmin.assign(s + clr::KP_STAT_CMIN * B, s + clr::KP_STAT_CMIN * B + B);
  h->host_cmax.assign(s + clr::KP_STAT_CMAX * B, s + clr::KP_STAT_CMAX * B + B);
  h->host_jitter.assign(s + clr::KP_STAT_JITTER * B, s + clr::KP_STAT_JITTER * B + B);
  h->kp_refused.resize(B);
  for (size_t b = 0; b < B; ++b) h->kp_refused[b] = s[clr::KP_STAT_ERROR * B + b] != 0.0;
  warm_select(h);
  if ((st = place_warm_K(h)) != CLR_OK) return st;
  h->kp_in_force = true;
  return CLR_OK;
}

// draws the program refused (evaluated at their stand-in coefficients): NaN and CLR_INVALID_ARGUMENT
extern "C++" void mark_refused(const clr_batch* h, double* a, double* b, double* c, int* status) {
  if (!h->kp_in_force) return;
  for (size_t i = 0; i < (size_t)h->B; ++i) {
    if (!h->kp_refused[i]) continue;
    if (a) a[i] = NAN;
    if (b) b[i] = NAN;
    if (c) c[i] = NAN;
    if (status) status[i] = CLR_INVALID_ARGUMENT;
  }
}

int clr_batch_get_coefficients(clr_batch* h, double* jitter, double* a_real, double* c_real, double* a_comp,
                               double* b_comp, double* c_comp, double* d_comp) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (!h->have_coeffs) return fail(CLR_NOT_COMPUTED, "clr_batch_get_coefficients: no coefficients are set");
  const size_t B = (size_t)h->B, nr = B * h->J_real, nc = B * h->J_comp, total = 2 * nr + 4 * nc + B;
  std::vector<double> back(total);
  HIP_TRY(hipMemcpyAsync(back.data(), h->coeffs.p, total * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  const double* r = back.data();
  auto get = [&](double* p, size_t n) { if (p && n) memcpy(p, r, n * sizeof(double)); r += n; };
  get(a_real, nr); get(c_real, nr); get(a_comp, nc); get(b_comp, nc); get(c_comp, nc); get(d_comp, nc);
  get(jitter, B);
  return CLR_OK;
}

int clr_batch_get_parameter_status(const clr_batch* h, int* status) {
  if (!status) return fail(CLR_INVALID_ARGUMENT, "status is null");
  if (!h->kp_in_force) return fail(CLR_NOT_COMPUTED, "the coefficients in force were not formed from parameters");
  for (size_t b = 0; b < (size_t)h->B; ++b) status[b] = h->kp_refused[b] ? CLR_INVALID_ARGUMENT : CLR_OK;
  return CLR_OK;
}

int clr_batch_evaluate_params(clr_batch* h, const double* params, const double* mean, long mean_stride,
                              double* loglike, double* logdet, double* quad, int* status) {
  int st = mean ? clr_batch_set_mean(h, mean, mean_stride) : CLR_OK;
  if (st == CLR_OK) st = clr_batch_set_parameters(h, params);
  if (st == CLR_OK) st = clr_batch_enqueue(h, 0);
  if (st == CLR_OK) st = clr_batch_get_results(h, loglike, logdet, quad, status);
  if (st == CLR_OK) mark_refused(h, loglike, logdet, quad, status);
  return st;
}

int clr_batch_grad_params(clr_batch* h, double* value, double* grad_params, int* status, int with_mean) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (!h->have_kernel || !h->kp_in_force)
    return fail(CLR_NOT_COMPUTED, "clr_batch_grad_params: the coefficients in force were not formed from parameters");
  const size_t B = (size_t)h->B, P = (size_t)h->kp.n_params, NG = 1 + 2 * (size_t)h->J_real + 4 * (size_t)h->J_comp;
  const size_t ncol = P + (with_mean ? 1 : 0);
  // the coefficient gradient is assembled on the host from whichever route settled each problem (clr_batch_grad): it
  // goes back up as one block grad[B][NG] | dmean[B], so that the chain rule is the same kernel on every route
  std::vector<double> up(B * NG + B), val(B);
  std::vector<int> stt(B);
  st = with_mean ? clr_batch_grad_mean(h, val.data(), up.data(), up.data() + B * NG, stt.data())
                 : clr_batch_grad(h, val.data(), up.data(), stt.data());
  if (st != CLR_OK) return st;
  std::vector<double> back(B * ncol);
  if ((st = h->kp_grad.reserve(B * NG + B + B * ncol)) != CLR_OK) return st;
  double* dgrad = h->kp_grad.p;
  double* dout = dgrad + B * NG + B;
  HIP_TRY(hipMemcpyAsync(dgrad, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
  clr::launch_kernel_program_vjp(device_program(h), h->B, h->kp_params.p, dgrad, with_mean ? dgrad + B * NG : nullptr, dout,
                                 h->stream.get());
  HIP_TRY(hipGetLastError());
  if (ncol) HIP_TRY(hipMemcpyAsync(back.data(), dout, back.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  for (size_t b = 0; b < B; ++b) {
    const bool refused = h->kp_refused[b];
    if (value) value[b] = refused ? NAN : val[b];
    if (status) status[b] = refused ? (int)CLR_INVALID_ARGUMENT : stt[b];
    if (!grad_params) continue;
    for (size_t p = 0; p < ncol; ++p) grad_params[b * ncol + p] = refused ? NAN : back[b * ncol + p];
    if (with_mean && P == 0 && !refused) grad_params[b * ncol] = up[B * NG + b];
  }
  return CLR_OK;
}

int clr_batch_set_exact(clr_batch* h, int force) {
  h->force_exact = force ? 1 : 0;
  return CLR_OK;
}

int clr_batch_get_exact_count(clr_batch* h, int* count) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;  // (pending problems are settled first: their routes too)
  if (!count) return fail(CLR_INVALID_ARGUMENT, "count is null");
  if (h->nchunk < 2 || h->force_exact) {  // every problem went through the reference recurrence
    *count = h->B;
    return CLR_OK;
  }
  std::vector<int> need((size_t)h->B);
  const size_t pc = (size_t)h->B * h->nchunk;
  HIP_TRY(hipMemcpyAsync(need.data(), h->flags.p + 2 * pc, need.size() * sizeof(int),
                         hipMemcpyDeviceToHost, h->stream.get()));
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  int n = 0;
  for (int v : need) n += v != 0;
  *count = n;
  return CLR_OK;
}

int clr_batch_get_exact_flags(clr_batch* h, int* flags) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;  // (pending problems are settled first: their routes too)
  if (!flags) return fail(CLR_INVALID_ARGUMENT, "flags is null");
  if (h->nchunk < 2) {
    for (int b = 0; b < h->B; ++b) flags[b] = 2;  // one chunk: the replay from the zero state is the recurrence
    return CLR_OK;
  }
  const size_t pc = (size_t)h->B * h->nchunk;
  HIP_TRY(hipMemcpyAsync(flags, h->flags.p + 2 * pc, (size_t)h->B * sizeof(int), hipMemcpyDeviceToHost, h->stream.get()));
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  if (h->force_exact)
    for (int b = 0; b < h->B; ++b) flags[b] = flags[b] < 1 ? 1 : flags[b];
  return CLR_OK;
}

int clr_batch_get_conditioning_chunkwise(clr_batch* h, double* ratio_max) {
  // max over chunks of gamma_c / mu_c (both of the SAME chunk), per problem
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (!ratio_max) return fail(CLR_INVALID_ARGUMENT, "ratio_max is null");
  if (!h->evaluated) return fail(CLR_NOT_COMPUTED, "no evaluation has been enqueued on this plan");
  if (h->nchunk < 2) {  // one chunk: the recurrence itself ran, there is no record
    for (int b = 0; b < h->B; ++b) ratio_max[b] = 0.0;
    return CLR_OK;
  }
  const size_t pc = (size_t)h->B * h->nchunk;
  std::vector<double> c(pc * 3);
  HIP_TRY(hipMemcpyAsync(c.data(), h->cond.p, c.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  for (int b = 0; b < h->B; ++b) {
    double r = 0.0;
    for (int k = 0; k < h->nchunk; ++k) {
      const double* e = &c[((size_t)b * h->nchunk + k) * 3];
      const double q = e[0] / e[1];
      if (!(q <= r)) r = q;
    }
    ratio_max[b] = r;
  }
  return CLR_OK;
}

int clr_batch_get_conditioning(clr_batch* h, double* gamma_max, double* mu_min, double* resid_max) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (!h->evaluated) return fail(CLR_NOT_COMPUTED, "no evaluation has been enqueued on this plan");
  if (h->nchunk < 2) {  // one chunk: the recurrence itself ran, there is no record
    for (int b = 0; b < h->B; ++b) {
      if (gamma_max) gamma_max[b] = 0.0;
      if (mu_min) mu_min[b] = 1.0;
      if (resid_max) resid_max[b] = 0.0;
    }
    return CLR_OK;
  }
  const size_t pc = (size_t)h->B * h->nchunk;
  std::vector<double> c(pc * 3);
  HIP_TRY(hipMemcpyAsync(c.data(), h->cond.p, c.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  // problems the warm-started recurrence settled have no scan record: gamma 0, mu 1, and the largest boundary
  // mismatch of the warm path as the residual
  std::vector<int> scanned;
  std::vector<double> wres;
  if (h->warm_active && h->wints.p && h->warm_settled > 0) {
    scanned.resize((size_t)h->B);
    wres.resize((size_t)h->B);
    HIP_TRY(hipMemcpyAsync(scanned.data(), h->wints.p + (size_t)h->B * h->wnchunk, scanned.size() * sizeof(int),
                           hipMemcpyDeviceToHost, h->stream.get()));
    HIP_TRY(hipMemcpyAsync(wres.data(), h->wresid.p, wres.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
    HIP_TRY(hipStreamSynchronize(h->stream.get()));
  }
  for (int b = 0; b < h->B; ++b) {
    double g = 0.0, m = 1.0, r = 0.0;
    if (!scanned.empty() && scanned[b] == 0) {
      r = wres[b];
    } else {
      for (int k = 0; k < h->nchunk; ++k) {
        const double* e = &c[((size_t)b * h->nchunk + k) * 3];
        if (!(e[0] <= g)) g = e[0];
        if (!(e[1] >= m)) m = e[1];
        if (!(e[2] <= r)) r = e[2];
      }
    }
    if (gamma_max) gamma_max[b] = g;
    if (mu_min) mu_min[b] = m;
    if (resid_max) resid_max[b] = r;
  }
  return CLR_OK;
}

int clr_batch_get_measured_error(clr_batch* h, double* eg_max) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (!eg_max) return fail(CLR_INVALID_ARGUMENT, "eg_max is null");
  if (!h->evaluated) return fail(CLR_NOT_COMPUTED, "no evaluation has been enqueued on this plan");
  const size_t pc = (size_t)h->B * h->nchunk;
  std::vector<double> c(pc);
  if (h->nchunk >= 2) {
    HIP_TRY(hipMemcpyAsync(c.data(), h->cond.p + pc * 3, pc * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
    HIP_TRY(hipStreamSynchronize(h->stream.get()));
  }
  for (int b = 0; b < h->B; ++b) {
    double e = 0.0;
    for (int k = 0; k < h->nchunk && h->nchunk >= 2; ++k) {
      const double v = c[(size_t)b * h->nchunk + k];
      if (!(v <= e)) e = v;
    }
    eg_max[b] = e;
  }
  return CLR_OK;
}

int clr_batch_set_certificate(clr_batch* h, double max_gamma_over_mu, double max_residual) {
  h->cert_gamma = max_gamma_over_mu;
  h->cert_resid = max_residual;
  h->pipeline_pinned = true;
  return CLR_OK;
}

int clr_batch_set_certificate_gamma(clr_batch* h, double max_gamma, double max_gamma_times_error) {
  h->cert_gamma_abs = max_gamma;
  h->cert_eg = max_gamma_times_error;
  return CLR_OK;
}

int clr_batch_set_prefix_mode(clr_batch* h, int mode) {
  if (mode < 0 || mode > 2) return fail(CLR_INVALID_ARGUMENT, "prefix mode must be 0, 1 or 2");
  h->coop_prefix = mode;
  h->pipeline_pinned = true;
  if (h->J_general > 0) return plan_general_chunks(h);  // (the parallel prefix asks for other chunk counts)
  return CLR_OK;
}

int clr_batch_set_prefix_plan(clr_batch* h, int levels, int group) {
  if (levels > 3 || (levels > 0 && group < 2)) return fail(CLR_INVALID_ARGUMENT, "prefix plan: levels <= 3, group >= 2");
  h->plan_levels = levels;
  h->plan_g = group;
  const int keep = h->warm_explicit_chunks;  // (re-planning the workspace is not a request for a chunk count)
  int st = clr_batch_set_chunks(h, h->nchunk);
  h->warm_explicit_chunks = keep;
  if (st == CLR_OK) st = warm_plan_chunks(h);
  return st;
}

int clr_batch_get_prefix_plan(const clr_batch* h, int* levels, int* groups /* [3] */, int* counts /* [4] */) {
  if (levels) *levels = (h->launch && h->coop_prefix == 2) ? h->plan.levels : 0;
  for (int l = 0; l < 3; ++l) if (groups) groups[l] = h->plan.g[l];
  for (int l = 0; l < 4; ++l) if (counts) counts[l] = h->plan.n[l];
  return CLR_OK;
}

int clr_batch_debug_get_starts(clr_batch* h, double* starts) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (!h->launch || !starts) return fail(CLR_INVALID_ARGUMENT, "start states are kept for widths 1..8");
  const size_t n = (size_t)h->B * h->nchunk * h->launch->start_doubles;
  HIP_TRY(hipMemcpyAsync(starts, h->starts.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  return CLR_OK;
}

int clr_batch_debug_compose_check(clr_batch* h, int group, double* max_abs_diff, double* max_abs_value) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (!h->launch || group < 2 || !h->evaluated)
    return fail(CLR_INVALID_ARGUMENT, "compose check: widths 1..8, group >= 2, after an evaluation");
  clr::BatchParams P;
  if ((st = batch_params(h, 0, P, false)) != CLR_OK) return st;
  const size_t np = (size_t)(h->nchunk + group - 1) / group, E = (size_t)h->launch->elem_doubles;
  const size_t n = (size_t)h->B * np * E;
  DevBuf a, b;
  if ((st = a.reserve(n)) != CLR_OK || (st = b.reserve(n)) != CLR_OK) return st;
  h->launch->compose_check(P, group, a.p, b.p, h->stream.get());
  HIP_TRY(hipGetLastError());
  std::vector<double> ha(n), hb(n);
  HIP_TRY(hipMemcpyAsync(ha.data(), a.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  HIP_TRY(hipMemcpyAsync(hb.data(), b.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  a.release();
  b.release();
  // per element (one composed group) and per block of it (A | b | C | eta | Jm): the largest difference against the
  // block's largest magnitude; the last group of a problem may hold the padded last chunk (never applied): skipped
  const int J = h->J, SZ = J * (J + 1) / 2;
  const size_t off[6] = {0, (size_t)J * J, (size_t)J * J + J, (size_t)J * J + J + SZ, (size_t)J * J + 2 * J + SZ, E};
  double worst = 0.0, big = 0.0;
  for (size_t e = 0; e < (size_t)h->B * np; ++e) {
    if (e % np == np - 1) continue;
    for (int blk = 0; blk < 5; ++blk) {
      double d = 0.0, m = 0.0;
      for (size_t i = off[blk]; i < off[blk + 1]; ++i) {
        const double x = ha[e * E + i], y = hb[e * E + i];
        if (!(fabs(x - y) <= d)) d = fabs(x - y);
        if (!(fabs(y) <= m)) m = fabs(y);
      }
      const double r = m > 0.0 ? d / m : d;
      if (!(r <= worst)) worst = r;
      if (!(m <= big)) big = m;
    }
  }
  if (max_abs_diff) *max_abs_diff = worst;
  if (max_abs_value) *max_abs_value = big;
  return CLR_OK;
}

int clr_batch_set_summarize_mode(clr_batch* h, int mode) {
  if (mode < -1 || mode > 2) return fail(CLR_INVALID_ARGUMENT, "summarize mode must be -1, 0, 1 or 2");
  if (mode > 0 && h->ragged) return refuse_ragged(h, "the forced role-split summarize");
  if (mode != h->summarize_mode) scan_reader_changed(h);
  h->summarize_mode = mode;
  if (mode >= 0) h->pipeline_pinned = true;
  return CLR_OK;
}

int clr_batch_get_summarize_kernel(const clr_batch* h, int* kind) {
  if (!kind) return fail(CLR_INVALID_ARGUMENT, "kind is null");
  *kind = split_active(h, false) ? ((h->summarize_mode != 1 && lazy_eligible(h)) ? 2 : 1) : 0;
  if (!h->launch)  // wide plans: plain or lazy flavour of the one-wave-per-chunk summarize
    *kind = (h->nchunk > 1 && (h->summarize_mode < 0 || h->summarize_mode == 2) &&
             (h->J_general > 0 ? lazy_eligible(h) : lazy_eligible_wide(h))) ? 2 : 0;
  return CLR_OK;
}

int clr_batch_get_split_variant(const clr_batch* h, int* variant) {
  if (!variant) return fail(CLR_INVALID_ARGUMENT, "variant is null");
  *variant = (split_active(h, false) && h->summarize_mode != 1 && lazy_eligible(h)) ? (split_lazy_bzero(h) ? 1 : 0) : 0;
  return CLR_OK;
}

// A plan with general terms on the wide kernels (total width <= 64): its own chunking and workspace, derived from the
// plan's CURRENT settings -- batch size, explicit chunk count, prefix mode, first-chunk ratio.  Called by
// clr_batch_set_general and again by every setter that changes one of those (clr_batch_set_chunks and, through it,
// clr_batch_set_prefix_plan; clr_batch_set_prefix_mode), so that the chunking does not depend on the order of the calls.
static int plan_general_chunks(clr_batch* h) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  h->gen_nchunk = 0;
  const int J_general = h->J_general;
  if (J_general <= 0) return CLR_OK;
  // Total widths up to 64 run on the wave-per-(problem, chunk) kernels (wide_kernels.hip, GEN flavour): the general rows
  // are one more row class there.  Chunks as for any wide plan: one round of two waves per SIMD, the scan up to width 32.
  const int Wt = h->J + J_general;
  if (Wt <= clr::wide_max_width()) {
    int nchunk = (Wt <= clr::wide_scan_max_width() && h->B <= 1024) ? 2048 / h->B : 1;
    if (Wt > 32) nchunk = h->B <= 512 ? std::max(2, 1024 / h->B) : 1;  // (one wave per SIMD at total widths 33..64: clr_batch_set_chunks)
    if (nchunk > 16) nchunk = 16;
    while (nchunk > 1 && h->N / nchunk < (Wt > 32 ? 1024 : 512)) --nchunk;
    const int cap = clr::wide_prefix_scan_max_chunks(Wt <= 16 ? 16 : 32), Lmin = Wt <= 16 ? 64 : 96;
    if (Wt <= 32 && h->coop_prefix == 2 && h->B < 32 && std::min(cap / h->B, h->N / Lmin) > nchunk)
      nchunk = std::min(cap / h->B, h->N / Lmin);  // (few problems: the parallel prefix, clr_batch_set_chunks)
    if (h->warm_explicit_chunks > 0 && Wt <= clr::wide_scan_max_width())  // (an explicit clr_batch_set_chunks is honoured, whenever it was made)
      nchunk = std::min(h->warm_explicit_chunks, std::max(1, h->N / 64));
    if (nchunk < 1) nchunk = 1;
    int L = (h->N + nchunk - 1) / nchunk;
    if (nchunk > 1) L = (L + 7) & ~7;
    nchunk = (h->N + L - 1) / L;
    int L0 = 0;
    const double first_ratio = Wt > 32 ? h->wide_first_ratio64 : h->wide_first_ratio;
    if (nchunk > 1 && first_ratio > 1.0) {  // (the riderless, longer first chunk: clr_batch_set_chunks)
      int L2 = (int)ceil(h->N / (nchunk - 1 + first_ratio));
      L2 = (L2 + 7) & ~7;
      const long first = (long)h->N - (long)(nchunk - 1) * L2;
      if (L2 >= 64 && first >= L2) { L = L2; L0 = (int)first; }
    }
    const size_t pc = (size_t)h->B * nchunk, JP = (size_t)clr::wide_padded_width(Wt), SZ = JP * (JP + 1) / 2;
    if (nchunk > 1) {
      if ((st = h->gen_elems.reserve(pc * (JP * JP + JP + SZ + JP + SZ))) != CLR_OK) return st;
      if ((st = h->gen_starts.reserve(pc * (SZ + JP))) != CLR_OK) return st;
      h->gen_scan_ws_doubles = clr::wide_prefix_scan_workspace(h->B, nchunk, (int)JP);
      if (h->gen_scan_ws_doubles && (st = h->gen_scan.reserve(h->gen_scan_ws_doubles)) != CLR_OK) return st;
    } else {
      h->gen_scan_ws_doubles = 0;
    }
    if ((st = h->gen_part.reserve(pc * 4)) != CLR_OK) return st;
    if ((st = h->gen_cond.reserve(pc * 4)) != CLR_OK) return st;
    h->gen_flags.release();
    if ((st = h->gen_flags.reserve(2 * pc + (size_t)h->B)) != CLR_OK) return st;
    HIP_TRY(hipMemsetAsync(h->gen_flags.p, 0, (2 * pc + (size_t)h->B) * sizeof(int), h->stream.get()));
    HIP_TRY(hipMemsetAsync(h->gen_cond.p, 0, pc * 4 * sizeof(double), h->stream.get()));
    h->gen_nchunk = nchunk; h->gen_L = L; h->gen_L0 = L0;
  }
  return CLR_OK;
}

int clr_batch_set_general(clr_batch* h, int J_general, const double* A, long A_stride, const double* U, long U_stride,
                          const double* V, long V_stride) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (J_general < 0) return fail(CLR_INVALID_ARGUMENT, "J_general must be >= 0");
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;
  if (J_general == 0) {  // back to the celerite-terms-only plan
    h->J_general = 0;
    return CLR_OK;
  }
  if (!A || !U || !V) return fail(CLR_INVALID_ARGUMENT, "general terms need A, U and V");
  if ((st = refuse_ragged(h, "clr_batch_set_general")) != CLR_OK) return st;
  if (h->J + J_general > CLR_MAX_WIDTH) return fail(CLR_UNSUPPORTED, "width above CLR_MAX_WIDTH");
  const long N = h->N, UV = (long)J_general * N;
  if ((A_stride != 0 && A_stride != N) || (U_stride != 0 && U_stride != UV) || (V_stride != 0 && V_stride != UV))
    return fail(CLR_INVALID_ARGUMENT, "general-term strides must be 0 (shared) or the size of one problem's block");
  auto count = [&](long sd, long one) { return (size_t)(sd == 0 ? one : one * (long)h->B); };
  if ((st = upload(h->gA, A, count(A_stride, N), h->stream.get())) != CLR_OK) return st;
  if ((st = upload(h->gU, U, count(U_stride, UV), h->stream.get())) != CLR_OK) return st;
  if ((st = upload(h->gV, V, count(V_stride, UV), h->stream.get())) != CLR_OK) return st;
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  h->J_general = J_general;
  h->gA_stride = A_stride; h->gU_stride = U_stride; h->gV_stride = V_stride;
  if ((st = plan_general_chunks(h)) != CLR_OK) { h->J_general = 0; return st; }
  return CLR_OK;
}

static bool warm_runs(const clr_batch* h, int materialize);
static bool small_runs(const clr_batch* h, int materialize);

int clr_batch_set_general_route(clr_batch* h, int route) {
  if (route != -1 && route != 1) return fail(CLR_INVALID_ARGUMENT, "general route: -1 (automatic) or 1 (sequential kernel)");
  h->general_route = route;
  return CLR_OK;
}

int clr_batch_set_small_mode(clr_batch* h, int mode) {
  if (mode < -1 || mode > 1) return fail(CLR_INVALID_ARGUMENT, "small mode: -1 (auto), 0 (off) or 1 (whenever supported)");
  if (mode == 1 && h->ragged) return refuse_ragged(h, "the forced one-launch mode");
  int st = warm_resolve(h, nullptr);
  if (st != CLR_OK) return st;
  h->small_mode = mode;
  return CLR_OK;
}

int clr_batch_get_small_mode(const clr_batch* h, int* active) {
  if (active) *active = (!warm_runs(h, 0) && small_runs(h, 0)) ? 1 : 0;
  return CLR_OK;
}

int clr_batch_set_warm_start(clr_batch* h, int mode, int forced_warmup) {
  if (mode < -1 || mode > 1 || (mode == 1 && forced_warmup < 1))
    return fail(CLR_INVALID_ARGUMENT, "warm start: mode -1 (auto), 0 (off) or 1 (forced, with a warm-up length >= 1)");
  if (mode == 1 && h->ragged) return refuse_ragged(h, "the forced warm start");
  int st = warm_resolve(h, nullptr);
  if (st != CLR_OK) return st;
  h->warm_mode = mode;
  h->warm_forced_K = forced_warmup;
  h->warm_boost = 0;
  h->warm_active = false;  // (decided by the next clr_batch_set_coefficients)
  h->have_coeffs = false;
  return CLR_OK;
}

int clr_batch_get_warm_start(const clr_batch* h, int* active, int* nchunk, int* chunk_len, int* warmup_min,
                             int* warmup_max, int* settled, int* fallbacks) {
  if (active) *active = h->warm_active ? 1 : 0;
  if (nchunk) *nchunk = h->wnchunk;
  if (chunk_len) *chunk_len = h->wL;
  int lo = 0, hi = 0;
  if (h->warm_active)
    for (int k : h->warm_K) {
      if (k <= 0) continue;
      lo = (lo == 0 || k < lo) ? k : lo;
      hi = k > hi ? k : hi;
    }
  if (warmup_min) *warmup_min = lo;
  if (warmup_max) *warmup_max = hi;
  if (settled) *settled = h->warm_settled;
  if (fallbacks) *fallbacks = h->warm_fallbacks;
  return CLR_OK;
}

int clr_batch_set_layout(clr_batch* h, int layout) {
  if (layout < 0 || layout > 2) return fail(CLR_INVALID_ARGUMENT, "layout must be 0, 1 or 2");
  h->layout = layout;
  scan_reader_changed(h);
  h->pipeline_pinned = true;
  return CLR_OK;
}

// wide path.  One chunk: the sequential sweep (one wave per problem).  Several chunks: summarize ->
// prefix -> correct (+ conditioning decision) -> finalize from the chunk summaries.  Forced-exact runs
// and the problems whose conditioning record is above the bound replay every chunk from its scanned
// start state and check the end states against the scan.  Problems the certificate flagged, or whose
// replay did not meet the scan, are then walked by the sequential sweep itself (one wave per such
// problem over all N samples), which overwrites their results: nothing of theirs depends on the scan.
int clr_batch_set_profiling(clr_batch* h, int on) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  h->prof_on = (on == 2 && h->launch) ? 2 : (on ? 1 : 0);  // 2: only the summarize (dominant) kernel is bracketed (widths 1..8)
  h->prof_steps = 0;
  return CLR_OK;
}

int clr_batch_get_profile(clr_batch* h, double* kernel_ms /* [6] */, int* steps) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  double k[PROF_NK] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < h->prof_steps; ++i)
    for (int j = 0; j < PROF_NK; ++j) {
      if (h->prof_on == 2 && j != 1) continue;  // (only events 1 and 2 were recorded)
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, h->prof_events[(size_t)i * (PROF_NK + 1) + j].get(),
                                  h->prof_events[(size_t)i * (PROF_NK + 1) + j + 1].get()));
      k[j] += ms;
    }
  if (kernel_ms)
    for (int j = 0; j < PROF_NK; ++j) kernel_ms[j] = k[j];
  if (steps) *steps = h->prof_steps;
  return CLR_OK;
}

// the parameters of everything around the warm path -- the warm kernel, the one-launch kernel, the scan behind them for
// the problems they leave pending --: the plan's row-major arrays, the single-wave summarize, pending problems only
static int fallback_params(clr_batch* h, clr::BatchParams& P) { return batch_params(h, 0, P, true); }

// a batch of short, narrow problems: the whole fused evaluation in ONE launch, one workgroup per problem
// (small_batch_kernel, small_kernels.hip); problems it cannot certify stay pending for the scan pipeline
static bool small_runs(const clr_batch* h, int materialize) {
  if (h->grad_scan_only || h->small_mode == 0 || h->ragged) return false;  // (ragged: the kernel knows one length)
  if (!h->launch || materialize || h->force_exact || !h->wints.p || h->J_general > 0) return false;
  if (!clr::small_batch_supported(h->J_real, h->J_comp, h->N)) return false;
  // (automatic: while a workgroup per problem still fits one round of the chip -- above that the scan pipeline's
  //  throughput wins, profiles/r04i_small_batch.txt)
  if (h->small_mode == 1) return true;
  // automatic: not when the caller tuned the scan pipeline explicitly, and only while a workgroup per problem fits
  // one round of the chip (widths 3, 4: one workgroup per CU by registers and LDS; narrower: four) -- above that the
  // pipeline's throughput wins (profiles/r04i_small_batch.txt: 1024 x 1e4 x width 4 0.29 ms against 0.34)
  return !h->pipeline_pinned && sel_B(h) <= (h->J >= 3 ? 256 : 1024);
}

// The one-launch path's view of the series: lane = chunk of ceil(N / 256) samples, so the row-major arrays would be read
// with a stride of one chunk between the lanes -- every load instruction touches 64 cache lines of which it uses 8 bytes
// each, and the 768 lines a workgroup walks (256 lanes x 3 arrays) do not fit the CU's vector L1: each line is fetched
// from L2 sixteen times (BASELINE configs[1]: 3.8 MB per problem through a 64-B/clk port -- the summarize phase was
// bound by exactly that, profiles/r06l_config1_ab.txt).  The kernel therefore reads a chunk-interleaved copy
// [problem][i][chunk] made once per set_series (launch_relayout with the path's own chunking, padded as the plan's copy):
// one coalesced 512-B load per array, wave and step.  The copy is rebuilt here when it is stale, or `regardless`.
static int small_params(clr_batch* h, clr::BatchParams& Sp, bool regardless) {
  int st = fallback_params(h, Sp);
  if (st != CLR_OK) return st;
  const int T = 256, L = (h->N + T - 1) / T;
  const long cells = (long)L * T;
  SeriesCopy& c = h->small_series;
  SeriesJobs jobs(h, c, (size_t)cells);
  if ((st = jobs.reserve()) != CLR_OK) return st;
  if (c.stale || regardless) {
    for (auto& j : jobs.job)
      clr::launch_relayout(j.src, j.stride, j.dst->p, j.dst_stride, j.nsrc, h->N, L, T, j.pad, h->stream.get());
    c.stale = false;
  }
  Sp.t = c.T.p; Sp.diag = c.D.p; Sp.y = c.Y.p;
  Sp.t_stride = h->t_stride ? cells : 0;
  Sp.diag_stride = h->diag_stride ? cells : 0;
  Sp.y_stride = h->y_stride ? cells : 0;
  Sp.lane_is = T; Sp.lane_cs = 1;
  return CLR_OK;
}

static bool warm_runs(const clr_batch* h, int materialize) {
  if (h->grad_scan_only) return false;
  return h->launch && h->warm_active && !materialize && !h->force_exact && h->nchunk > 1 && h->wnchunk > 1;
}

// the warm kernel's copy of the series, (re)built when the series or the warm chunking changed -- or `regardless`
static int warm_copy(clr_batch* h, bool regardless) {
  if (!h->warm_series.stale && !regardless) return CLR_OK;
  SeriesJobs jobs(h, h->warm_series, (size_t)h->wrows * h->wnchunk);
  const int st = jobs.reserve();
  if (st != CLR_OK) return st;
  for (auto& j : jobs.job)
    clr::launch_relayout_warm(j.src, j.stride, j.dst->p, j.dst_stride, j.nsrc, h->N, h->wL, h->wnchunk, h->wKpad, h->wrows,
                              j.pad, h->stream.get());
  h->warm_series.stale = false;
  return CLR_OK;
}

// K per problem on the device, when set_series re-selected it after the coefficients were uploaded
static int warm_upload_K(clr_batch* h) {
  if (!h->warm_K_dirty || !h->wints.p) return CLR_OK;
  HIP_TRY(hipMemcpyAsync(h->wints.p + (size_t)h->B * h->wnchunk + h->B, h->warm_K.data(), (size_t)h->B * sizeof(int),
                         hipMemcpyHostToDevice, h->stream.get()));
  HIP_TRY(hipStreamSynchronize(h->stream.get()));  // (pageable source)
  h->warm_K_dirty = false;
  return CLR_OK;
}

// replay mode of a materialising run: 2 the four arrays chunk-interleaved, 3 the lean layout (W, D only)
static int replay_mode(const clr_batch* h, int materialize) {
  return materialize ? (h->factor_layout == 1 ? 3 : 2) : 0;
}

// the fix-up pass of a materialising run: the first `factor_refine` samples of every chunk from the previous chunk's
// replayed end state (BatchParams::ends / fixup_steps, replay_kernel)
static void refine_chunk_heads(const clr_batch* h, clr::BatchParams R, int materialize, hipStream_t s) {
  R.fixup_steps = R.refine_samples;
  h->launch->replay(R, replay_mode(h, materialize), s);
}

int clr_batch_set_rescue(clr_batch* h, int mode) {
  if (mode < -1 || mode > 1) return fail(CLR_INVALID_ARGUMENT, "rescue mode: -1 (auto), 0 (inline chunked replay) or 1 (whenever possible)");
  int st = warm_resolve(h, nullptr);
  if (st != CLR_OK) return st;
  h->rescue_mode = mode;
  return CLR_OK;
}

int clr_batch_get_rescue(const clr_batch* h, int* last_count, long* total, int* nchunk, int* chunk_len) {
  if (last_count) *last_count = h->rescue_last;
  if (total) *total = h->rescue_total;
  if (nchunk) *nchunk = h->rescue ? h->rescue->nchunk : 0;
  if (chunk_len) *chunk_len = h->rescue ? h->rescue->L : 0;
  return CLR_OK;
}

int clr_batch_set_factor_layout(clr_batch* h, int layout) {
  if (layout != 0 && layout != 1) return fail(CLR_INVALID_ARGUMENT, "factor layout: 0 (phi, u, W, D) or 1 (lean: W, D)");
  if (layout == 1 && !h->launch) return fail(CLR_UNSUPPORTED, "the lean factor layout covers widths 1..8 (wider plans write the reference's storage)");
  if (layout != h->factor_layout) factor_dropped(h);
  h->factor_layout = layout;
  return CLR_OK;
}

int clr_batch_set_factor_refine(clr_batch* h, int samples) {
  if (samples < 0) return fail(CLR_INVALID_ARGUMENT, "factor refine: samples per chunk head >= 0");
  h->factor_refine = samples;
  return CLR_OK;
}

int clr_batch_get_factor_bytes(const clr_batch* h, size_t* bytes_per_problem) {
  if (!bytes_per_problem) return fail(CLR_INVALID_ARGUMENT, "bytes_per_problem is null");
  const size_t cells = h->launch ? (size_t)h->L * h->nchunk : (size_t)h->N, J = (size_t)h->J;
  *bytes_per_problem = 8 * cells * ((h->launch && h->factor_layout == 1) ? (J + 1) : (3 * J + 1));
  return CLR_OK;
}

// "Record event i of this step now": the step's PROF_NK + 1 events on the plan's stream (null: none) and which of them
// are wanted.  A record that fails is not reported here: reading an elapsed time off it is (clr_batch_get_profile,
// clr_batch_run_timed).
struct StepMarks {
  const clr::Event* ev = nullptr;
  unsigned mask = ~0u;
  void operator()(int i, hipStream_t s) const {
    if (ev && (mask >> i & 1)) (void)hipEventRecord(ev[i].get(), s);
  }
  void from(int i, hipStream_t s) const {
    for (; i <= PROF_NK; ++i) (*this)(i, s);
  }
};

// The scan pipeline of a narrow plan (widths 1..8), the one place its order is written down: summarize -> prefix ->
// correct -> replay -> chunk heads -> sequential -> finalize.  `from_replay`: the tail only, on the start states and
// the routing an evaluation has left (rescue_inline).
static void narrow_scan(clr_batch* h, clr::BatchParams& P, int materialize, const StepMarks& mark, bool from_replay = false) {
  hipStream_t s = h->stream.get();
  const int mode = replay_mode(h, materialize);
  if (!from_replay) {
    mark(1, s);
    h->launch->summarize(P, s);
    mark(2, s);
    h->launch->prefix(P, s);
    mark(3, s);
    h->launch->correct(P, s);  // (also on forced-exact runs: flags + conditioning record)
    mark(4, s);
  }
  // forced-exact / materialising runs only.  The replay reads the series where the summarize did: from the role split's
  // chunk-interleaved copy 4.41 ms = 65 % of HBM for the materialising replay at B = 1024, N = 1e5, width 8, against
  // 4.77 ms from the row-major arrays through LDS-staged tiles (profiles/r03a_prefix_ab.txt)
  h->launch->replay(P, mode, s);
  if (P.ends) refine_chunk_heads(h, P, materialize, s);
  h->launch->sequential(P, mode, s);  // flagged / ill-conditioned problems only
  if (materialize) factor_written(h, h->factor_layout == 1);
  mark(5, s);
  clr::launch_finalize(P, s);
  mark(6, s);
  // (capturing these launches in a hipGraph was measured: no gain -- the gaps between
  //  dependent kernels are on the device side; profiles/r01r_small_batches.log)
}

// the scan pipeline for the problems the warm path left pending (single-wave summarize on the row-major arrays)
static int warm_fallback(clr_batch* h) {
  clr::BatchParams P;
  const int st = fallback_params(h, P);
  if (st != CLR_OK) return st;
  narrow_scan(h, P, 0, StepMarks());
  HIP_TRY(hipGetLastError());
  return CLR_OK;
}

// ONE evaluation of the plan on the parameters P of batch_params(h, materialize, P): the route test and every launch, for
// clr_batch_enqueue and for each step of clr_batch_run_timed alike.  `fresh_series`: the step stands for one on a new
// series -- the copy of the series its route reads is rebuilt inside it whether stale or not; otherwise only a stale copy
// is (the copy a step rebuilt is fresh afterwards, and no other).  The *_inflight flags describe this evaluation afterwards
// (every state-changing entry point resolves an evaluation in flight first, so none of an earlier one is relied on).
static int launch_step(clr_batch* h, int materialize, clr::BatchParams& P, const StepMarks& mark, bool fresh_series) {
  hipStream_t s = h->stream.get();
  int st;
  h->evaluated = true;
  h->amp_eval = h->amp_active ? 1 : 0;  // (whose log term the results of this evaluation carry: amplitude_adjust)
  h->warm_inflight = h->small_inflight = h->rescue_inflight = false;
  if (h->J_general > 0 || h->J > clr::wide_max_width()) {
    // general terms -- and (round 5) celerite-only kernels of widths 65..128, which have no wave-per-problem kernel --: the
    // any-width sequential recurrence, one workgroup per problem with S in LDS (generic_loglike_batch_kernel)
    if (materialize) return fail(CLR_UNSUPPORTED, "materialising runs with general terms or above width 64: use CholeskySolver");
    mark(0, s);
    if (h->gen_nchunk > 0 && h->general_route != 1) {
      // the wide kernels with the general rows as a third row class (chunked scan up to total width 32)
      clr::BatchParams W;
      general_wide_params(h, P, W);
      return wide_flow(W, h->J_real, h->J_comp, s, mark.ev);
    }
    clr::GenericBatch G;
    memset(&G, 0, sizeof(G));
    G.B = h->B; G.N = h->N; G.J_real = h->J_real; G.J_comp = h->J_comp; G.J_general = h->J_general;
    G.a_real = P.a_real; G.c_real = P.c_real; G.a_comp = P.a_comp; G.b_comp = P.b_comp; G.c_comp = P.c_comp;
    G.d_comp = P.d_comp; G.jitter = P.jitter;
    G.t = h->t.p; G.diag = h->diag.p; G.y = h->y.p;
    G.t_stride = h->t_stride; G.diag_stride = h->diag_stride; G.y_stride = h->y_stride;
    G.A = h->gA.p; G.U = h->gU.p; G.V = h->gV.p;
    G.A_stride = h->gA_stride; G.U_stride = h->gU_stride; G.V_stride = h->gV_stride;
    G.out_ll = P.out_ll; G.out_logdet = P.out_logdet; G.out_quad = P.out_quad; G.out_status = P.out_status;
    mark(1, s);
    // (round 6) total widths 33 .. 128: S in the registers of the problem's workgroup (rows_kernels.hip: 1.6 us per sample at
    // width 128 where the LDS-resident kernel takes 20)
    if (clr::factor_rows_batch_supported(h->J + h->J_general) && !clr::option("CLR_NO_ROWS_KERNEL"))
      clr::launch_factor_rows_batch(G, P.fast_trig, s);
    else
      clr::launch_generic_loglike_batch(G, s);
    mark.from(2, s);
    return CLR_OK;
  }
  mark(0, s);
  if (!h->launch) {  // wide path (one chunk: the whole sweep is in the "replay" slot)
    if ((st = wide_flow(P, h->J_real, h->J_comp, s, mark.ev)) != CLR_OK) return st;
    if (materialize) factor_written(h, false);
    h->rescue_inflight = P.defer_level1 != 0;
    return CLR_OK;
  }
  if (!warm_runs(h, materialize) && small_runs(h, materialize)) {  // (one launch, in the "summarize" slot)
    clr::BatchParams Sp;
    if ((st = small_params(h, Sp, fresh_series)) != CLR_OK) return st;
    mark(1, s);
    clr::launch_small_batch(h->J_real, h->J_comp, Sp, 256, s);
    mark.from(2, s);
    h->small_inflight = true;  // (pending problems are settled like the warm path's: warm_resolve)
    return CLR_OK;
  }
  if (warm_runs(h, materialize)) {
    // series that forget: the plain recurrence per chunk with a warm-up + the boundary check, in the "summarize" slot;
    // problems it cannot settle are marked pending and go through the scan pipeline when the results are asked for
    clr::BatchParams Wp;
    if ((st = warm_copy(h, fresh_series)) != CLR_OK) return st;
    if ((st = warm_upload_K(h)) != CLR_OK) return st;
    if ((st = fallback_params(h, Wp)) != CLR_OK) return st;
    mark(1, s);
    h->launch->warm(Wp, s);
    mark.from(2, s);
    h->warm_inflight = true;
    return CLR_OK;
  }
  build_scan_series(h, fresh_series);
  narrow_scan(h, P, materialize, mark);
  h->rescue_inflight = P.defer_level1 != 0;
  return CLR_OK;
}

int clr_batch_enqueue(clr_batch* h, int materialize) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  clr::BatchParams P;
  if ((st = batch_params(h, materialize, P, false)) != CLR_OK) return st;
  // profiling: one event per kernel boundary of this evaluation, on the plan's stream (mode 2: events 1 and 2 only)
  StepMarks mark;
  if (h->prof_on && h->prof_steps < PROF_MAX_STEPS) {
    const size_t need = (size_t)(h->prof_steps + 1) * (PROF_NK + 1);
    while (h->prof_events.size() < need) {
      clr::Event e;
      HIP_TRY(clr::create_event(e));
      h->prof_events.push_back(std::move(e));
    }
    mark.ev = &h->prof_events[(size_t)h->prof_steps * (PROF_NK + 1)];
    if (h->prof_on == 2) mark.mask = 1u << 1 | 1u << 2;
    ++h->prof_steps;
  }
  if (!P.defer_level1) h->rescue_last = 0;  // (nothing is re-planned behind this evaluation)
  h->pin_results = false;
  if ((st = launch_step(h, materialize, P, mark, false)) != CLR_OK) return st;
  HIP_TRY(hipGetLastError());
  return CLR_OK;
}

int clr_batch_fp32_probe(clr_batch* h, double* logdet, double* quad, double* ms) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (h->launch || h->J > clr::wide_f32_probe_max_width())
    return fail(CLR_UNSUPPORTED, "the fp32 probe covers widths 9..32");
  clr::BatchParams P;
  if ((st = batch_params(h, 0, P, false)) != CLR_OK) return st;
  const size_t B = (size_t)h->B;
  DevBuf tmp;
  if ((st = tmp.reserve(2 * B)) != CLR_OK) return st;
  clr::Event e0, e1;
  HIP_TRY(clr::create_event(e0));
  HIP_TRY(clr::create_event(e1));
  clr::launch_wide_f32_probe(P, h->J_real, h->J_comp, tmp.p, tmp.p + B, h->stream.get());  // warm-up
  HIP_TRY(hipEventRecord(e0.get(), h->stream.get()));
  clr::launch_wide_f32_probe(P, h->J_real, h->J_comp, tmp.p, tmp.p + B, h->stream.get());
  HIP_TRY(hipEventRecord(e1.get(), h->stream.get()));
  HIP_TRY(hipGetLastError());
  if (logdet) HIP_TRY(hipMemcpyAsync(logdet, tmp.p, B * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  if (quad) HIP_TRY(hipMemcpyAsync(quad, tmp.p + B, B * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  float t = 0.f;
  HIP_TRY(hipEventElapsedTime(&t, e0.get(), e1.get()));
  if (ms) *ms = t;
  return CLR_OK;
}

// ---- level-1 problems re-planned as a small plan of their own ----------------------------------
// The evaluation left the problems its conditioning record sends to the checked chunked replay PENDING (defer_runs,
// finalize_kernel).  Their checked replay is three passes -- summarize, prefix, replay + end-state check -- over the
// chunks of a plan sized for THEM: n problems cut into ~1024 / n chunks each, so that the chip is full and a chunk is a
// tenth of the parent's.  Same routes, same certificates (a side plan runs forced-exact: every chunk replayed from its
// scanned start state and checked, mismatches go to its own sequential recurrence), cholesky.h:176 semantics included.
static int rescue_inline(clr_batch* h) {
  // too many pending problems for a side plan to pay: the inline chunked replay after all (the flow's own tail)
  clr::BatchParams P;
  int st = batch_params(h, 0, P, false);
  if (st != CLR_OK) return st;
  P.defer_level1 = 0;
  if (!h->launch) {
    clr::launch_wide_loglike(P, h->J_real, h->J_comp, h->stream.get());
    clr::launch_wide_check_replay(P, h->stream.get());
    clr::launch_finalize(P, h->stream.get());
    clr::BatchParams S = P;
    S.nchunk = 1; S.L = P.N; S.L0 = 0; S.seq_only = 1; S.force_exact = 1;
    clr::launch_wide_loglike(S, h->J_real, h->J_comp, h->stream.get());
  } else {
    narrow_scan(h, P, 0, StepMarks(), true);
  }
  HIP_TRY(hipGetLastError());
  return CLR_OK;
}

// `n_total`: the pending problems of the WHOLE batch (the plan's own count unless it is a slice of a larger batch):
// side plan or inline replay, and the side plan's chunk count, follow that number -- never the slice's own -- so that
// a problem is re-planned the same way under any sharding.
static int rescue_run(clr_batch* h, const std::vector<int>& idx, long n_total) {
  const int n = (int)idx.size();
  h->rescue_total += n;
  if (n_total > std::max(1, sel_B(h) / 4) || n_total > 256) {
    h->rescue_last = -n;
    return rescue_inline(h);
  }
  h->rescue_last = n;
  int st;
  if (!h->rescue || h->rescue->B != n || h->rescue_plan_key != n_total) {
    h->rescue.reset();
    h->rescue_plan_key = -1;
    h->rescue.reset(clr_batch_create(n, h->N, h->J_real, h->J_comp, h->device));
    if (!h->rescue) return CLR_HIP_ERROR;
    clr_batch* r = h->rescue.get();
    r->is_rescue_plan = true;
    r->force_exact = 1;
    r->warm_mode = 0;
    r->small_mode = 0;
    int nchunk = 0;
    const int nt = (int)n_total;
    if (!h->launch) {  // wide: B x nchunk <= the parallel prefix's cap (1024 workgroups per level at width 32, 2048 below)
      const int JP = clr::wide_padded_width(h->J);
      if (JP <= 32) {
        nchunk = std::min(clr::wide_prefix_scan_cap(JP) / nt, clr::wide_prefix_scan_max_chunks(JP));
        nchunk = std::min(nchunk, h->N / (JP == 16 ? 64 : 96));
        if (nchunk < 8) nchunk = 0;  // (short series: the plan's own choice)
      }  // (widths 33..64: the plan's own rule -- 1024 / n chunks, at most 16, chained by the walk)
      if (nchunk == 0) {  // the automatic rule, asked as the side plan of the whole batch would ask it
        const BatchPtr probe((nt == n) ? nullptr : clr_batch_create(nt, h->N, h->J_real, h->J_comp, h->device));
        if (probe) nchunk = probe->nchunk;
      }
    } else {
      nchunk = auto_chunks(nt, h->N, h->J, true);
    }
    // (a failed set-up must not leave a half-initialised side plan behind: the next resolve would take it for ready)
    if ((st = clr_batch_set_chunks(r, nchunk)) != CLR_OK) {
      h->rescue.reset();
      return st;
    }
    h->rescue_plan_key = n_total;
  }
  clr_batch* r = h->rescue.get();
  // the parent's settings that decide routes and kernels
  r->cert_resid = h->cert_resid; r->cert_gamma = h->cert_gamma; r->cert_gamma_abs = h->cert_gamma_abs; r->cert_eg = h->cert_eg;
  r->floor_tmax = sel_max(h->tmax, h->floor_tmax); r->floor_dxmax = sel_max(h->dxmax, h->floor_dxmax);
  r->floor_dmax = sel_max(h->dmax, h->floor_dmax); r->floor_cmax = sel_max(h->cmax, h->floor_cmax);
  r->tmax = h->tmax; r->dxmax = h->dxmax; r->dmax = h->dmax; r->cmax = h->cmax; r->dtmin = h->dtmin;
  if ((st = h->rescue_idx.reserve((size_t)n)) != CLR_OK) return st;
  HIP_TRY(hipStreamSynchronize(r->stream.get()));
  HIP_TRY(hipMemcpyAsync(h->rescue_idx.p, idx.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, r->stream.get()));
  HIP_TRY(hipStreamSynchronize(r->stream.get()));  // (pageable source)
  // series and coefficients of the n problems, device to device (the parent's stream is idle: warm_resolve synchronised it)
  const size_t N = (size_t)h->N;
  struct { DevBuf* src; DevBuf* dst; long stride; long* sub_stride; } arrs[3] = {
      {&h->t, &r->t, h->t_stride, &r->t_stride}, {&h->diag, &r->diag, h->diag_stride, &r->diag_stride}, {&h->y, &r->y, h->y_stride, &r->y_stride}};
  for (auto& a : arrs) {
    if (a.stride == 0) {  // one series shared by all problems: shared by the side plan's too
      if ((st = a.dst->reserve(N)) != CLR_OK) return st;
      HIP_TRY(hipMemcpyAsync(a.dst->p, a.src->p, N * sizeof(double), hipMemcpyDeviceToDevice, r->stream.get()));
      *a.sub_stride = 0;
    } else {
      if ((st = a.dst->reserve((size_t)n * N)) != CLR_OK) return st;
      clr::launch_gather_series(a.src->p, a.stride, a.dst->p, h->rescue_idx.p, n, h->N, r->stream.get());
      *a.sub_stride = (long)N;
    }
  }
  r->have_series = true;
  series_replaced(r);
  r->ragged = h->ragged;  // the re-planned problems' lengths travel with them (their gathered rows are padded already)
  r->host_len.clear();
  if (h->ragged) {
    for (int b : idx) r->host_len.push_back(h->host_len[(size_t)b]);
    if ((st = r->len_dev.reserve((size_t)n)) != CLR_OK) return st;
    HIP_TRY(hipMemcpyAsync(r->len_dev.p, r->host_len.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, r->stream.get()));
    HIP_TRY(hipStreamSynchronize(r->stream.get()));  // (pageable source)
  }
  const size_t total = (size_t)n * (2 * h->J_real + 4 * h->J_comp + 1);
  if ((st = r->coeffs.reserve(total)) != CLR_OK) return st;
  clr::launch_gather_coeffs(h->coeffs.p, r->coeffs.p, h->rescue_idx.p, h->B, n, h->J_real, h->J_comp, r->stream.get());
  r->host_cmin.assign((size_t)n, 0.0);
  r->host_cmax.assign((size_t)n, h->cmax);
  r->host_jitter.assign((size_t)n, 0.0);
  r->have_coeffs = true;
  if ((st = clr_batch_enqueue(r, 0)) != CLR_OK) return st;
  const size_t pc = (size_t)n * r->nchunk, pcp = (size_t)h->B * h->nchunk;
  clr::launch_scatter_results(r->out.p, r->flags.p + 2 * pc, n, h->out.p, h->flags.p + 2 * pcp, h->B, h->rescue_idx.p, r->stream.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(r->stream.get()));
  return CLR_OK;
}

// Problems the warm path could not settle (boundary mismatch, flagged pivot, not eligible) carry a pending status
// until the scan pipeline has run for them.  That pipeline reads the plan's CURRENT coefficients, series and
// chunking, so it must run before any of them changes: every state-changing entry point, clr_batch_synchronize and
// clr_batch_get_results call this first.  *pin_current (may be null): the pinned staging buffer holds the final
// results (ll | logdet | quad | status) of this evaluation.
//
// Two halves (a plan that is a slice of a larger batch has the sharded layer add up the counts between them,
// clr_group_hooks.h): resolve_begin waits for the evaluation and counts, resolve_finish acts on the counts of the
// whole batch.
// the results in HBM (ll | logdet | quad | status) -> the pinned staging buffer, waited for
static int fetch_results(clr_batch* h) {
  const size_t B = (size_t)h->B, words = 3 * B + (B + 1) / 2;
  HIP_TRY(hipMemcpyAsync(h->pin.p, h->out.p, words * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  return CLR_OK;
}

static int resolve_begin(clr_batch* h, long* pending_out, long* eligible_out) {
  if (pending_out) *pending_out = 0;
  if (eligible_out) *eligible_out = 0;
  if (h->res_open) {  // (begin twice without a finish: the same counts again)
    if (pending_out) *pending_out = h->res_pending;
    if (eligible_out) *eligible_out = h->res_was_warm ? h->warm_eligible : 0;
    return CLR_OK;
  }
  if (!h->warm_inflight && !h->small_inflight && !h->rescue_inflight) return CLR_OK;
  // (the one-launch path of short narrow problems leaves pending problems the same way, but its outcome says nothing
  //  about the warm-up lengths: the warm path's statistics and its adaptation are not touched on its behalf)
  h->res_was_warm = h->warm_inflight;
  h->res_was_rescue = h->rescue_inflight;
  h->warm_inflight = false;
  h->small_inflight = false;
  h->rescue_inflight = false;
  const size_t B = (size_t)h->B, words = 3 * B + (B + 1) / 2;
  int st;
  if ((st = reserve_pinned(h, words)) != CLR_OK) return st;
  if ((st = fetch_results(h)) != CLR_OK) return st;
  const int* stw = reinterpret_cast<const int*>(h->pin.p + 3 * B);
  long pending = 0;
  for (size_t b = 0; b < B; ++b) pending += stw[b] == clr::CLR_PENDING_STATUS;
  if (h->res_was_warm) {
    h->warm_fallbacks = (int)pending;
    h->warm_settled = (int)B - (int)pending;
  }
  h->res_pending = pending;
  h->res_open = true;
  h->pin_results = true;  // (final unless something is pending: resolve_finish re-reads then)
  if (pending_out) *pending_out = pending;
  if (eligible_out) *eligible_out = h->res_was_warm ? h->warm_eligible : 0;
  return CLR_OK;
}

// `pending_total`, `eligible_total`: the counts over the whole batch (the plan's own when it is the whole batch)
static int resolve_finish(clr_batch* h, long pending_total, long eligible_total) {
  if (!h->res_open) return CLR_OK;
  h->res_open = false;
  const size_t B = (size_t)h->B;
  const bool was_warm = h->res_was_warm, was_rescue = h->res_was_rescue;
  const long pending = h->res_pending;
  const int* stw = reinterpret_cast<const int*>(h->pin.p + 3 * B);
  int st;
  if (was_rescue) {
    // the scan pipeline itself ran: what is pending are its level-1 problems, re-planned with short chunks
    h->rescue_last = 0;
    if (pending) {
      std::vector<int> idx;
      for (size_t b = 0; b < B; ++b) if (stw[b] == clr::CLR_PENDING_STATUS) idx.push_back((int)b);
      h->pin_results = false;
      if ((st = rescue_run(h, idx, pending_total)) != CLR_OK) return st;
      if ((st = fetch_results(h)) != CLR_OK) return st;
      h->pin_results = true;
    }
    return CLR_OK;
  }
  if (pending) {
    h->pin_results = false;
    if ((st = warm_fallback(h)) != CLR_OK) return st;
    if ((st = fetch_results(h)) != CLR_OK) return st;
    h->pin_results = true;
  }
  if (pending_total) {
    // many mismatches among the problems that did warm up: longer warm-ups from the next coefficients on
    const long failed = pending_total - ((long)sel_B(h) - eligible_total);
    if (was_warm && h->warm_mode < 0 && failed * 10 > eligible_total && h->warm_boost < clr_batch::WARM_NK - 1) ++h->warm_boost;
  } else if (was_warm && h->warm_mode < 0 && h->warm_boost > 0 && ++h->warm_clean >= 8) {
    --h->warm_boost;  // eight clean evaluations in a row: try the shorter warm-ups again
    h->warm_clean = 0;
  }
  if (pending_total && was_warm) h->warm_clean = 0;
  return CLR_OK;
}

extern "C++" int warm_resolve(clr_batch* h, bool* pin_current) {
  if (pin_current) *pin_current = false;
  if (!h->res_open && !h->warm_inflight && !h->small_inflight && !h->rescue_inflight) {
    // (nothing in flight; an evaluation the sharded layer has already resolved left its results in the staging buffer)
    if (pin_current) *pin_current = h->pin_results;
    return CLR_OK;
  }
  long pending = 0, eligible = 0;
  int st = resolve_begin(h, &pending, &eligible);
  if (st != CLR_OK) return st;
  // (a slice of a larger batch resolved on its own -- clr_batch_run_timed's steps, a direct call -- acts on its own
  //  counts scaled to nothing: the slice's numbers stand for the batch's)
  if ((st = resolve_finish(h, pending, eligible)) != CLR_OK) return st;
  if (pin_current) *pin_current = h->pin_results;
  return CLR_OK;
}

int clr_batch_synchronize(clr_batch* h) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  return CLR_OK;
}

int clr_batch_get_results(clr_batch* h, double* loglike, double* logdet, double* quad,
                          int* status) {
  const int st = batch_results_scaled(h, loglike, logdet, quad, status);
  return st != CLR_OK ? st : amplitude_adjust(h, loglike, logdet, quad, status);
}

extern "C++" int batch_results_scaled(clr_batch* h, double* loglike, double* logdet, double* quad, int* status) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  const size_t B = (size_t)h->B, words = 3 * B + (B + 1) / 2;
  if ((st = reserve_pinned(h, words)) != CLR_OK) return st;
  // pending problems of a warm evaluation first (they leave the final results in the staging buffer); otherwise one
  // copy into the pinned staging buffer (ll | logdet | quad | status), then host memcpys
  bool pin_current = false;
  if ((st = warm_resolve(h, &pin_current)) != CLR_OK) return st;
  if (!pin_current && (st = fetch_results(h)) != CLR_OK) return st;
  if (loglike) memcpy(loglike, h->pin.p, B * sizeof(double));
  if (logdet) memcpy(logdet, h->pin.p + B, B * sizeof(double));
  if (quad) memcpy(quad, h->pin.p + 2 * B, B * sizeof(double));
  if (status) memcpy(status, h->pin.p + 3 * B, B * sizeof(int));
  return CLR_OK;
}

int clr_batch_run_timed(clr_batch* h, int materialize, int steps, int relayout_each_step,
                        double* total_ms, double* kernel_ms) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  clr::BatchParams P;
  if ((st = batch_params(h, materialize, P, false)) != CLR_OK) return st;
  if (steps < 1) steps = 1;
  h->pin_results = false;
  if (h->J_general > 0 || h->J > clr::wide_max_width()) {
    // (plans on the any-width sequential kernel or with general terms: the evaluation itself, `steps` times, as one "replay" slot)
    clr::Event e0, e1;
    HIP_TRY(clr::create_event(e0));
    HIP_TRY(clr::create_event(e1));
    HIP_TRY(hipEventRecord(e0.get(), h->stream.get()));
    for (int i = 0; i < steps; ++i)
      if ((st = clr_batch_enqueue(h, materialize)) != CLR_OK) return st;
    HIP_TRY(hipEventRecord(e1.get(), h->stream.get()));
    HIP_TRY(hipStreamSynchronize(h->stream.get()));
    float tot = 0.f;
    HIP_TRY(hipEventElapsedTime(&tot, e0.get(), e1.get()));
    if (total_ms) *total_ms = tot;
    if (kernel_ms) { for (int j = 0; j < 6; ++j) kernel_ms[j] = 0.0; kernel_ms[4] = tot; }
    return CLR_OK;
  }
  if (!relayout_each_step && !warm_runs(h, materialize)) build_scan_series(h, false);  // (in front of the timed steps)
  // one event per kernel boundary per step, all recorded on the handle's stream
  const int NK = PROF_NK;
  std::vector<clr::Event> ev((size_t)steps * (NK + 1));
  for (clr::Event& e : ev) HIP_TRY(clr::create_event(e));
  for (int i = 0; i < steps; ++i) {
    const clr::Event* e = &ev[(size_t)i * (NK + 1)];
    if ((st = launch_step(h, materialize, P, StepMarks{e}, relayout_each_step != 0)) != CLR_OK) return st;
    // (a plan that re-planned level-1 problems at its last evaluation does so inside every timed step: the step's
    //  time then includes the side plan -- at the price of a host round trip per step)
    if (h->rescue_inflight && h->rescue_last != 0) {
      if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;
      HIP_TRY(hipEventRecord(e[NK].get(), h->stream.get()));
    }
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream.get()));
  double k[NK] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < steps; ++i) {
    const clr::Event* e = &ev[(size_t)i * (NK + 1)];
    for (int j = 0; j < NK; ++j) {
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, e[j].get(), e[j + 1].get()));
      k[j] += ms;
    }
  }
  float tot = 0.f;
  HIP_TRY(hipEventElapsedTime(&tot, ev.front().get(), ev.back().get()));
  if (total_ms) *total_ms = tot;
  if (kernel_ms)
    for (int j = 0; j < NK; ++j) kernel_ms[j] = k[j];
  return CLR_OK;
}

// one optimiser / MCMC evaluation in one call: new coefficients in, the B results out (celerite.py:160-219 per problem:
// set_parameter_vector -> compute -> log_likelihood)
int clr_batch_evaluate(clr_batch* h, const double* jitter, const double* a_real, const double* c_real,
                       const double* a_comp, const double* b_comp, const double* c_comp, const double* d_comp,
                       double* loglike, double* logdet, double* quad, int* status) {
  int st = clr_batch_set_coefficients(h, jitter, a_real, c_real, a_comp, b_comp, c_comp, d_comp);
  if (st == CLR_OK) st = clr_batch_enqueue(h, 0);
  if (st == CLR_OK) st = clr_batch_get_results(h, loglike, logdet, quad, status);
  return st;
}

int clr_batch_evaluate_mean(clr_batch* h, const double* mean, long mean_stride, const double* jitter,
                            const double* a_real, const double* c_real, const double* a_comp, const double* b_comp,
                            const double* c_comp, const double* d_comp, double* loglike, double* logdet, double* quad,
                            int* status) {
  const int st = clr_batch_set_mean(h, mean, mean_stride);
  if (st != CLR_OK) return st;
  return clr_batch_evaluate(h, jitter, a_real, c_real, a_comp, b_comp, c_comp, d_comp, loglike, logdet, quad, status);
}

int clr_batch_log_likelihood(int B, int N, int J_real, int J_comp, const double* jitter,
                             const double* a_real, const double* c_real, const double* a_comp,
                             const double* b_comp, const double* c_comp, const double* d_comp,
                             const double* t, long t_stride, const double* diag,
                             long diag_stride, const double* y, long y_stride, double* loglike,
                             double* logdet, double* quad, int* status, int device) {
  clr_batch* h = clr_batch_create(B, N, J_real, J_comp, device);
  if (!h) {
    // clr_batch_create recorded why (message in clr_last_error)
    if (B < 1 || N < 1 || J_real < 0 || J_comp < 0) return CLR_INVALID_ARGUMENT;
    const int width = J_real + 2 * J_comp;
    if (width < 1 || width > CLR_MAX_WIDTH) return CLR_UNSUPPORTED;
    return visible_gfx950() > 0 ? CLR_HIP_ERROR : CLR_NO_DEVICE;
  }
  int st = clr_batch_set_series(h, t, t_stride, diag, diag_stride, y, y_stride);
  if (st == CLR_OK)
    st = clr_batch_set_coefficients(h, jitter, a_real, c_real, a_comp, b_comp, c_comp, d_comp);
  if (st == CLR_OK) st = clr_batch_enqueue(h, 0);
  if (st == CLR_OK) st = clr_batch_get_results(h, loglike, logdet, quad, status);
  clr_batch_destroy(h);
  return st;
}

}  // extern "C"

// ---- hooks of the sharded layer (clr_group_hooks.h; not part of the C ABI) ----------------------------------------
namespace clr_group {

int set_series_lengths(clr_batch* h, const double* t, long t_stride, const double* diag, long diag_stride, const double* y,
                       long y_stride, const int* lengths, bool batch_ragged) {
  return set_series_impl(h, t, t_stride, diag, diag_stride, y, y_stride, lengths, batch_ragged);
}

void set_batch_context(clr_batch* h, int B_total) {
  h->group_B = B_total > h->B ? B_total : 0;  // (a single shard IS the whole batch)
}

long warm_eligible(const clr_batch* h) { return h->warm_eligible; }

void set_warm_eligible_total(clr_batch* h, long eligible_total) {
  if (h->group_B <= 0) return;
  const bool selectable = !h->ragged && h->warm_mode != 0 && h->wnchunk >= 2 && h->have_series && !h->warm_span.empty() &&
                          h->host_cmin.size() == (size_t)h->B && h->warm_K.size() == (size_t)h->B;
  h->warm_eligible_total = eligible_total;
  h->warm_active = selectable && eligible_total * 2 >= (long)h->group_B;
  h->warm_K_dirty = h->warm_active;  // (K per problem goes up with the next enqueue)
}

void mark_refused(const clr_batch* h, double* loglike, double* logdet, double* quad, int* status) {
  ::mark_refused(h, loglike, logdet, quad, status);
}

bool in_flight(const clr_batch* h) { return h->res_open || h->warm_inflight || h->small_inflight || h->rescue_inflight; }

int resolve_begin(clr_batch* h, long* pending, long* eligible) {
  const int st = require_device(h->device);
  if (st != CLR_OK) return st;
  return ::resolve_begin(h, pending, eligible);
}

int resolve_finish(clr_batch* h, long pending_total, long eligible_total) {
  const int st = require_device(h->device);
  if (st != CLR_OK) return st;
  return ::resolve_finish(h, pending_total, eligible_total);
}

}  // namespace clr_group
