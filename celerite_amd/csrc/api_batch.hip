// celerite_amd/csrc/api_batch.hip -- C ABI of the batched plans (clr_batch_*): HBM residency, path selection
// (scan pipeline, warm-started recurrence, one-launch path, wide kernels, general terms), evaluation and results.
#include "api_internal.h"
#include "clr_options.h"
#include "clr_group_hooks.h"
#include "clr_kernel.h"
#include "clr_bmean_kernels.h"

#include <functional>
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
static int warm_resolve(clr_batch* h, bool* pin_current);
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

// The residual y - mu of clr_batch_set_mean -- or y - sum_k w_k Phi_k of clr_batch_set_mean_weights -- from the caller's
// series in `y_src`: one elementwise pass into `y`, where every route reads its series; the copies derived from `y` are
// then stale (a shared series with a per-problem mean becomes a per-problem residual: the copies are re-sized by the
// launches that rebuild them).  The factor of a materialising run does not depend on y and stays.
static int apply_mean(clr_batch* h) {
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
  HIP_TRY(hipGetLastError());
  residual_replaced(h, per_problem ? N : 0);
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
  if (h->mean_K == 0 && h->have_series) {  // the caller's series moves aside, `y` will hold the residual
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

int clr_batch_set_series(clr_batch* h, const double* t, long t_stride, const double* diag,
                         long diag_stride, const double* y, long y_stride) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  const long N = h->N;
  for (long sd : {t_stride, diag_stride, y_stride})
    if (sd != 0 && sd != N)
      return fail(CLR_INVALID_ARGUMENT, "series stride must be 0 (shared) or N");
  if ((st = warm_resolve(h, nullptr)) != CLR_OK) return st;  // (an evaluation in flight is settled on ITS series)
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
  // one pass over t ON THE DEVICE: max |t| over every sample (sortedness is not assumed), the largest and the smallest
  // step, NaN times; then the warm path's spans
  {
    const int nb = t_stride == 0 ? 1 : h->B;
    if ((st = h->scan.reserve((size_t)nb * std::max(4, (int)clr_batch::WARM_NK))) != CLR_OK) return st;
    clr::launch_series_stats(h->t.p, t_stride, nb, (int)N, h->scan.p, h->stream.get());
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
    const double finite_min = N > 1 ? dmin : 0.0;
    h->dtmin = (finite_min < 0.0) ? finite_min : (nan ? NAN : finite_min);
  }
  h->have_series = true;
  if (h->have_mean || h->mean_K > 0) {  // (the upload went to `y`: it becomes the caller's series, `y` the residual)
    std::swap(h->y, h->y_src);
    h->y_src_stride = y_stride;
    if ((st = apply_mean(h)) != CLR_OK) { h->have_series = false; return st; }
  }
  if ((st = warm_scan_spans(h)) != CLR_OK) { h->have_series = false; return st; }
  h->set_series_host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count();
  // a new series: the warm-ups chosen for the previous one's spans do not apply, nor does its history of fallbacks
  if (h->warm_mode < 0) h->warm_boost = 0;
  warm_select(h);
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
  for (size_t i = 0; i < nc; ++i) {
    const double m = fabs(d_comp[i]), c = fabs(c_comp[i]);
    if (!(m <= h->dmax)) h->dmax = m;
    if (!(c <= h->cmax)) h->cmax = c;
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
static void mark_refused(const clr_batch* h, double* a, double* b, double* c, int* status) {
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
  if (h->grad_scan_only || h->small_mode == 0) return false;
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

static int warm_resolve(clr_batch* h, bool* pin_current) {
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

// ---- the batched consumers of a plan's factor and coefficients: clr_batch_get_factor, _solve, _dot_L, _dot, _predict

// the factor of the last materialising run, still usable (a lean one is not once its series or coefficients changed);
// `settle`: settle an evaluation in flight first and require a completed run -- all but clr_batch_get_factor
static int require_factor(clr_batch* h, bool settle) {
  int st;
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
  if (h->J_general > 0 || h->J > clr::wide_max_width())
    return fail(CLR_UNSUPPORTED, std::string(entry) + " covers celerite-only plans of widths 1..64");
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
struct ConsumerFrame {
  clr_batch* h;
  bool timed = false, drained = false;
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
  if (!clr::wsweep_scan_supported(h->N, h->J)) return fail(CLR_UNSUPPORTED, "clr_batch_solve on a wide plan needs N >= 512 (shorter series: CholeskySolver.solve)");
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

// ... and its parameters on those buffers.  The chunk maps depend on the factor only: formed by the first solve after a
// materialising run; they count as formed only once that solve's kernels have run to completion -- a failed launch or
// copy must not leave the next solve reading uninitialised maps.  So this CLEARS bs_M_valid, and the caller sets it
// again after its frame has finished.
static clr::BSolveParams narrow_solve_begin(clr_batch* h, int nrhs) {
  clr::BSolveParams S;
  S.nrhs = nrhs; S.r = 0; S.lean = h->factor_is_lean ? 1 : 0;
  S.have_M = h->bs_M_valid ? 1 : 0;
  h->bs_M_valid = false;
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
  if (h->nchunk < 2) return fail(CLR_UNSUPPORTED, "clr_batch_solve needs a chunked plan (N >= 128)");
  clr::BatchParams P;
  if ((st = consumer_params(h, false, P)) != CLR_OK) return st;
  const size_t B = (size_t)h->B, N = (size_t)h->N, R = (size_t)nrhs;
  if ((st = reserve_narrow_solve(h, R)) != CLR_OK) return st;
  if ((st = h->bs_rm.reserve(B * R * N)) != CLR_OK) return st;
  ConsumerFrame frame{h};
  if (b) HIP_TRY(hipMemcpyAsync(h->bs_rm.p, b, B * R * N * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
  HIP_TRY(frame.start());
  const clr::BSolveParams S = narrow_solve_begin(h, nrhs);
  narrow_kernels(h, nrhs, b ? h->bs_rm.p : h->y.p, b ? (long)N : h->y_stride, h->bs_x.p, h->bs_x.p,
                 [&] { h->launch->bsolve(P, S, h->stream.get()); });
  HIP_TRY(frame.stop());
  if ((st = frame.finish(x, h->bs_rm.p, B * R * N)) != CLR_OK) return st;
  h->bs_M_valid = true;
  return CLR_OK;
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

// CholeskySolver::predict (cholesky.h:599-698; GP.predict's conditional mean, celerite.py:330-420) for every problem of
// the plan: mu*_p(x*) = K_p(x*, t_p) K_p^-1 y_p at M points per problem.  alpha = K^-1 y is the batched solve on the
// materialised factor (either layout, any width <= 64), left on the device; the reference's two passes over the sorted
// prediction points are the object API's chunked diagonal scans (generic_kernels.hip: launch_predict_scan, a parallel
// prefix over chunks of 16 samples + one thread per point) run problem by problem on the plan's resident times and
// coefficients -- they need nothing of the factor.  Unsorted points: the sequential walk (launch_predict).
int clr_batch_predict(clr_batch* h, int M, const double* xs, long xs_stride, double* pred) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (M < 0 || (M > 0 && (!xs || !pred))) return fail(CLR_INVALID_ARGUMENT, "clr_batch_predict: M >= 0, the points and an output array");
  if (xs_stride != 0 && xs_stride != M) return fail(CLR_INVALID_ARGUMENT, "clr_batch_predict: the points' stride is 0 (shared by all problems) or M");
  if ((st = require_celerite_width(h, "clr_batch_predict")) != CLR_OK) return st;
  if (M == 0) return CLR_OK;
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
  // the mean plus the conditional mean of the residual (celerite.py:279); under a linear mean (clr_batch_set_mean_basis) the
  // conditional mean of the residual alone -- the basis at the prediction points is the caller's
  if (h->have_mean)
    for (size_t p = 0; p < B; ++p) {
      const double m = h->host_mean[h->mean_stride ? p : 0];
      for (size_t k = 0; k < Mm; ++k) pred[p * Mm + k] = m + pred[p * Mm + k];
    }
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
    if (!clr::launch_mean_project(h->basis_dev.p, h->basis_stride, h->bs_rm.p, h->mean_K, h->B, h->N, h->proj_part.p,
                                  h->proj_out.p, h->stream.get()))
      return fail(CLR_UNSUPPORTED, "clr_batch_grad_mean_weights: B x N / 4096 workgroups do not fit one launch");
    HIP_TRY(hipEventRecord(h->proj_ev[1].get(), h->stream.get()));
    if ((st = frame.finish(dw, h->proj_out.p, B * K)) != CLR_OK) return st;
  }
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, h->proj_ev[0].get(), h->proj_ev[1].get()));
  h->project_device_ms = ms;
  // the statuses of the evaluation in force; a problem without a factor (or refused by the kernel program): zeros
  std::vector<int> stat(B);
  if ((st = clr_batch_get_results(h, nullptr, nullptr, nullptr, stat.data())) != CLR_OK) return st;
  mark_refused(h, nullptr, nullptr, nullptr, stat.data());
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

// points per tile: the caller's (clr_batch_set_predict_tile), or the most whose buffers -- `per_point` doubles each --
// fit in 1 GiB; never above grid.z's 65535 nor M, at least 1
static int predict_tile(const clr_batch* h, int M, size_t per_point) {
  const size_t budget = (size_t)1 << 27;  // doubles
  size_t R = h->predict_tile > 0 ? (size_t)h->predict_tile : std::max<size_t>(1, budget / std::max<size_t>(1, per_point));
  return (int)std::min<size_t>(std::min<size_t>(R, 65535), (size_t)M);
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
  if (M < 0 || (M > 0 && (!xs || !var))) return fail(CLR_INVALID_ARGUMENT, "clr_batch_predict_var: M >= 0, the points and an output array");
  if (xs_stride != 0 && xs_stride != M) return fail(CLR_INVALID_ARGUMENT, "clr_batch_predict_var: the points' stride is 0 (shared by all problems) or M");
  if ((st = require_celerite_width(h, "clr_batch_predict_var")) != CLR_OK) return st;
  if (M == 0) return CLR_OK;
  if ((st = require_factor(h, true)) != CLR_OK) return st;
  if (!h->launch && !clr::wsweep_scan_supported(h->N, h->J))
    return fail(CLR_UNSUPPORTED, "clr_batch_predict_var on a wide plan needs N >= 512 (shorter series: GP.predict)");
  if (h->launch && h->nchunk < 2) return fail(CLR_UNSUPPORTED, "clr_batch_predict_var needs a chunked plan (N >= 128)");
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
    const int R = predict_tile(h, M, B * (2 * N + ws_point));
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
  const int R = predict_tile(h, M, B * (cells + 2 * nc * J));
  if ((st = h->bs_x.reserve(B * R * cells)) != CLR_OK) return st;
  if ((st = h->bs_M.reserve(B * nc * J * J)) != CLR_OK) return st;
  if ((st = h->bs_off.reserve(B * R * nc * J)) != CLR_OK) return st;
  if ((st = h->bs_starts.reserve(B * R * nc * J)) != CLR_OK) return st;
  ConsumerFrame frame{h};
  HIP_TRY(hipMemcpyAsync(dxs.p, xs, nsrc * Mm * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
  HIP_TRY(frame.start());
  clr::BPredVarParams S;
  S.lean = h->factor_is_lean ? 1 : 0; S.cross_fast = cross_fast;
  // (the chunk maps are the batched solve's, under its validity rule: formed by the first tile after a materialising run
  //  unless a solve has formed them, and counted as formed only once this call's kernels have run to completion)
  S.have_M = h->bs_M_valid ? 1 : 0;
  h->bs_M_valid = false;
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
  if ((st = frame.finish(var, dvar.p, B * Mm)) != CLR_OK) return st;
  h->bs_M_valid = true;
  return CLR_OK;
}

// Every source's points ascending, for the kernels that walk them with a cursor (clr_batch_predict_var_recurrence,
// clr_batch_forecast): as given where they already are (detected in O(M)), else through an index permutation (NaN last;
// shared points once) that scatter() undoes on the results.  xmax: max |x| (a NaN stays), for the points' phase rule.
struct SortedPoints {
  bool all_sorted = true;
  std::vector<double> xsorted;
  std::vector<int> perm;
  const double* up = nullptr;  // the points to upload, [nsrc][M]
  double xmax = 0.0;
  void sort(const double* xs, size_t nsrc, size_t Mm) {
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
  // results in sorted order [B][M] -> the caller's order
  void scatter(const double* tmp, double* out, size_t B, size_t Mm, bool shared) const {
    for (size_t b = 0; b < B; ++b) {
      const int* pp = perm.data() + (shared ? 0 : b * Mm);
      for (size_t m = 0; m < Mm; ++m) out[b * Mm + pp[m]] = tmp[b * Mm + m];
    }
  }
};

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
  if (M < 0 || (M > 0 && (!xs || !var))) return fail(CLR_INVALID_ARGUMENT, "clr_batch_predict_var_recurrence: M >= 0, the points and an output array");
  if (xs_stride != 0 && xs_stride != M) return fail(CLR_INVALID_ARGUMENT, "clr_batch_predict_var_recurrence: the points' stride is 0 (shared by all problems) or M");
  if ((st = require_celerite_width(h, "clr_batch_predict_var_recurrence")) != CLR_OK) return st;
  if (M == 0) return CLR_OK;
  if ((st = require_factor(h, true)) != CLR_OK) return st;
  if (!h->launch)
    return fail(CLR_UNSUPPORTED, "clr_batch_predict_var_recurrence covers narrow plans (widths 1..8): a wide plan takes clr_batch_predict_var");
  if (h->nchunk < 2) return fail(CLR_UNSUPPORTED, "clr_batch_predict_var_recurrence needs a chunked plan (N >= 128)");
  clr::BatchParams P;
  if ((st = consumer_params(h, false, P)) != CLR_OK) return st;
  const size_t B = (size_t)h->B, J = (size_t)h->J, Mm = (size_t)M, nsrc = xs_stride == 0 ? 1 : B, nc = (size_t)h->nchunk;
  const size_t NS = J * (J + 1) / 2;
  SortedPoints pts;
  pts.sort(xs, nsrc, Mm);
  const bool all_sorted = pts.all_sorted;
  std::vector<double> vtmp;
  if (!all_sorted) vtmp.resize(B * Mm);
  const double* xup = pts.up;
  const int xfast = (sel_max(h->dmax, h->floor_dmax) * pts.xmax < CLR_FAST_TRIG_LIMIT) ? 1 : 0;
  // points per tile: the caller's, or the most whose per-point buffers (u(x), e, left) fit in 1 GiB
  const size_t budget = (size_t)1 << 27, per_point = B * (2 * J + 1);
  const size_t Rz = std::min<size_t>(h->predict_tile > 0 ? (size_t)h->predict_tile : std::max<size_t>(1, budget / per_point), Mm);
  const int R = (int)Rz;
  DevBuf dxs, dvar, dux, de, dleft;
  if ((st = dxs.reserve(nsrc * Mm)) != CLR_OK) return st;
  if ((st = dvar.reserve(B * Mm)) != CLR_OK) return st;
  if ((st = dux.reserve(B * Rz * J)) != CLR_OK) return st;
  if ((st = de.reserve(B * Rz * J)) != CLR_OK) return st;
  if ((st = dleft.reserve(B * Rz)) != CLR_OK) return st;
  if ((st = h->pv_S.reserve(B * nc * NS)) != CLR_OK) return st;
  if ((st = h->loo_Q.reserve(B * nc * NS)) != CLR_OK) return st;
  if ((st = h->bs_M.reserve(B * nc * J * J)) != CLR_OK) return st;
  if ((st = h->bs_off.reserve(B * nc * J)) != CLR_OK) return st;
  if ((st = h->bs_x.reserve(B * (size_t)h->L * nc)) != CLR_OK) return st;  // (read beside by the solve's summarize when it forms the maps)
  ConsumerFrame frame{h};
  HIP_TRY(hipMemcpyAsync(dxs.p, xup, nsrc * Mm * sizeof(double), hipMemcpyHostToDevice, h->stream.get()));
  HIP_TRY(frame.start());
  clr::BPredVarRecParams S;
  S.lean = h->factor_is_lean ? 1 : 0;
  S.have_S = h->pv_S_valid ? 1 : 0;
  S.have_Q = h->loo_Q_valid ? 1 : 0;
  S.Q.lean = S.lean;
  S.Q.have_M = h->bs_M_valid ? 1 : 0;
  const bool forms_Q = !S.have_Q;        // ... and with them the chunk maps, unless a solve has formed those
  if (forms_Q) h->bs_M_valid = false;
  h->pv_S_valid = h->loo_Q_valid = false;
  S.Q.cT = h->bs_x.p; S.Q.M = h->bs_M.p; S.Q.Q = h->loo_Q.p; S.Q.off = h->bs_off.p;
  S.xs_stride = xs_stride; S.t = h->t.p; S.t_stride = h->t_stride;
  S.S = h->pv_S.p; S.ux = dux.p; S.e = de.p; S.left = dleft.p;
  S.var_stride = (long)M;
  for (int m0 = 0; m0 < M; m0 += R) {
    S.npts = std::min(R, M - m0); S.xs = dxs.p + m0; S.var = dvar.p + m0;
    h->launch->bpredvar_rec(P, S, xfast, h->stream.get());
    S.have_S = S.have_Q = 1;
  }
  HIP_TRY(frame.stop());
  if ((st = frame.finish(all_sorted ? var : vtmp.data(), dvar.p, B * Mm)) != CLR_OK) return st;
  h->pv_S_valid = h->loo_Q_valid = true;
  if (forms_Q) h->bs_M_valid = true;
  if (!all_sorted) pts.scatter(vtmp.data(), var, B, Mm, xs_stride == 0);
  return CLR_OK;
}

// ---- clr_batch_one_step_ahead, clr_batch_forecast: the causal half of the factor (clr_bfilter_kernels.h)

// rows of problems without a factor (or refused by the kernel program) -> NaN; the statuses of the evaluation in force
static int nan_rows_without_factor(clr_batch* h, std::vector<int>& stat, std::initializer_list<std::pair<double*, size_t>> outs) {
  const size_t B = (size_t)h->B;
  stat.resize(B);
  const int st = clr_batch_get_results(h, nullptr, nullptr, nullptr, stat.data());
  if (st != CLR_OK) return st;
  mark_refused(h, nullptr, nullptr, nullptr, stat.data());
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t b = 0; b < B; ++b) {
    if (stat[b] == CLR_OK) continue;
    for (const auto& o : outs)
      if (o.first) std::fill(o.first + b * o.second, o.first + (b + 1) * o.second, nan);
  }
  return CLR_OK;
}

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
  if (!h->launch && !clr::wsweep_scan_supported(h->N, h->J))
    return fail(CLR_UNSUPPORTED, "clr_batch_one_step_ahead on a wide plan needs N >= 512");
  if (h->launch && h->nchunk < 2) return fail(CLR_UNSUPPORTED, "clr_batch_one_step_ahead needs a chunked plan (N >= 128)");
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
    bool forms_M = false;
    if (innovation && h->launch) {
      const clr::BSolveParams Q = narrow_solve_begin(h, nrhs);  // (clears bs_M_valid: set again once the frame has finished)
      forms_M = true;
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
    if (forms_M) h->bs_M_valid = true;
  }
  std::vector<int> stat;
  if ((st = nan_rows_without_factor(h, stat, {{innovation, R * N}, {variance, N}})) != CLR_OK) return st;
  if (status) std::copy(stat.begin(), stat.end(), status);
  return CLR_OK;
}

// The mean and variance at M points per problem given the samples strictly before each (clr_bfilter_kernels.h): the
// residual in force laid out chunk-interleaved once, the chunks' start states of g by the first tile (they follow the
// residual: never kept), those of S (pv_S, shared with clr_batch_predict_var_recurrence, only with `var`) unless formed,
// then one forward pass per tile of sorted points.  Points, sorting and tiles as clr_batch_predict_var_recurrence.
int clr_batch_forecast(clr_batch* h, int M, const double* xs, long xs_stride, double* mean, double* var) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (M < 0 || (M > 0 && !xs)) return fail(CLR_INVALID_ARGUMENT, "clr_batch_forecast: M >= 0 and the points");
  if (!mean && !var) return fail(CLR_INVALID_ARGUMENT, "clr_batch_forecast: at least one output array");
  if (xs_stride != 0 && xs_stride != M) return fail(CLR_INVALID_ARGUMENT, "clr_batch_forecast: the points' stride is 0 (shared by all problems) or M");
  if ((st = require_celerite_width(h, "clr_batch_forecast")) != CLR_OK) return st;
  if (M == 0) return CLR_OK;
  if ((st = require_factor(h, true)) != CLR_OK) return st;
  if (!h->launch)
    return fail(CLR_UNSUPPORTED, "clr_batch_forecast covers narrow plans (widths 1..8): a wide plan takes clr_batch_predict / clr_batch_predict_var");
  if (h->nchunk < 2) return fail(CLR_UNSUPPORTED, "clr_batch_forecast needs a chunked plan (N >= 128)");
  clr::BatchParams P;
  if ((st = consumer_params(h, false, P)) != CLR_OK) return st;
  const size_t B = (size_t)h->B, J = (size_t)h->J, Mm = (size_t)M, nsrc = xs_stride == 0 ? 1 : B, nc = (size_t)h->nchunk;
  const size_t NS = J * (J + 1) / 2, nout = (mean ? 1 : 0) + (var ? 1 : 0);
  SortedPoints pts;
  pts.sort(xs, nsrc, Mm);
  // the phases of the points' features: |d| |x*|, under the plan's own rule
  const int xfast = (sel_max(h->dmax, h->floor_dmax) * pts.xmax < CLR_FAST_TRIG_LIMIT) ? 1 : 0;
  // points per tile: the caller's, or the most whose per-point buffer (u(x)) fits in 1 GiB
  const size_t budget = (size_t)1 << 27, per_point = B * J;
  const size_t Rz = std::min<size_t>(h->predict_tile > 0 ? (size_t)h->predict_tile : std::max<size_t>(1, budget / per_point), Mm);
  const int R = (int)Rz;
  DevBuf dxs, dout, dux;  // dout: mean [B][M] | var [B][M], those asked for
  if ((st = dxs.reserve(nsrc * Mm)) != CLR_OK) return st;
  if ((st = dout.reserve(nout * B * Mm)) != CLR_OK) return st;
  if ((st = dux.reserve(B * Rz * J)) != CLR_OK) return st;
  if (var && (st = h->pv_S.reserve(B * nc * NS)) != CLR_OK) return st;
  if ((st = reserve_narrow_solve(h, 1)) != CLR_OK) return st;
  ConsumerFrame frame{h};
  hipStream_t s = h->stream.get();
  HIP_TRY(hipMemcpyAsync(dxs.p, pts.up, nsrc * Mm * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(frame.start());
  const clr::BSolveParams Q = narrow_solve_begin(h, 1);  // (clears bs_M_valid: set again once the frame has finished)
  clr::BFilterParams S{};
  S.nrhs = 1; S.lean = Q.lean; S.have_M = Q.have_M;
  S.have_S = h->pv_S_valid ? 1 : 0;
  const bool forms_S = var && !h->pv_S_valid;
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
  h->bs_M_valid = true;
  if (forms_S) h->pv_S_valid = true;
  const double* tmean = tmp.data();
  const double* tvar = tmp.data() + (mean ? B * Mm : 0);
  if (pts.all_sorted) {
    if (mean) std::copy(tmean, tmean + B * Mm, mean);
    if (var) std::copy(tvar, tvar + B * Mm, var);
  } else {
    if (mean) pts.scatter(tmean, mean, B, Mm, xs_stride == 0);
    if (var) pts.scatter(tvar, var, B, Mm, xs_stride == 0);
  }
  // the constant mean plus the conditional mean of the residual, as clr_batch_predict; under a linear mean the residual's
  // alone -- the basis at the points is the caller's
  if (mean && h->have_mean)
    for (size_t p = 0; p < B; ++p) {
      const double m = h->host_mean[h->mean_stride ? p : 0];
      for (size_t k = 0; k < Mm; ++k) mean[p * Mm + k] = m + mean[p * Mm + k];
    }
  std::vector<int> stat;
  return nan_rows_without_factor(h, stat, {{mean, Mm}, {var, Mm}});
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
  if (M < 0 || (M > 0 && !xs)) return fail(CLR_INVALID_ARGUMENT, "clr_batch_predict_terms: M >= 0 and the points");
  if (G < 1 || !groups) return fail(CLR_INVALID_ARGUMENT, "clr_batch_predict_terms: G >= 1 and the groups");
  if (!mean && !var) return fail(CLR_INVALID_ARGUMENT, "clr_batch_predict_terms: at least one output array");
  if (xs_stride != 0 && xs_stride != M) return fail(CLR_INVALID_ARGUMENT, "clr_batch_predict_terms: the points' stride is 0 (shared by all problems) or M");
  if ((st = require_celerite_width(h, "clr_batch_predict_terms")) != CLR_OK) return st;
  const int T = h->J_real + h->J_comp;
  for (size_t k = 0; k < (size_t)G * T; ++k)
    if (groups[k] > 1) return fail(CLR_INVALID_ARGUMENT, "clr_batch_predict_terms: a group is 0 or 1 per coefficient term");
  if (M == 0) return CLR_OK;
  if ((st = require_factor(h, true)) != CLR_OK) return st;
  if (!h->launch)
    return fail(CLR_UNSUPPORTED, "clr_batch_predict_terms covers narrow plans (widths 1..8): a wide plan takes clr_batch_predict / clr_batch_predict_var for the full kernel");
  if (h->nchunk < 2) return fail(CLR_UNSUPPORTED, "clr_batch_predict_terms needs a chunked plan (N >= 128), as clr_batch_predict on a narrow plan does");
  if (mean && (st = batch_solve_impl(h, 1, nullptr, nullptr)) != CLR_OK) return st;  // alpha = K^-1 r -> bs_rm [B][N]
  clr::BatchParams P;
  if ((st = consumer_params(h, false, P)) != CLR_OK) return st;
  const size_t B = (size_t)h->B, J = (size_t)h->J, Mm = (size_t)M, Gg = (size_t)G, nsrc = xs_stride == 0 ? 1 : B;
  const size_t nc = (size_t)h->nchunk, NS = J * (J + 1) / 2, nout = (mean ? 1 : 0) + (var ? 1 : 0);
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
  const int xfast = (sel_max(h->dmax, h->floor_dmax) * pts.xmax < CLR_FAST_TRIG_LIMIT) ? 1 : 0;
  // points per tile: the caller's, or the most whose per-point buffers (u(x), v(x); e and left per group) fit in 1 GiB
  const size_t budget = (size_t)1 << 27, per_point = B * (2 * J + (var ? Gg * (J + 1) : 0));
  const size_t Rz = std::min<size_t>(h->predict_tile > 0 ? (size_t)h->predict_tile : std::max<size_t>(1, budget / per_point), Mm);
  const int R = (int)Rz;
  DevBuf dxs, dout, dux, dvx, de, dleft, dbstart;  // dout: mean [B][G][M] | var [B][G][M], those asked for
  clr::Buffer<unsigned> dmask;
  if ((st = dxs.reserve(nsrc * Mm)) != CLR_OK) return st;
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
    if ((st = h->pv_S.reserve(B * nc * NS)) != CLR_OK) return st;
    if ((st = h->loo_Q.reserve(B * nc * NS)) != CLR_OK) return st;
    if ((st = h->bs_M.reserve(B * nc * J * J)) != CLR_OK) return st;
    if ((st = h->bs_off.reserve(B * nc * J)) != CLR_OK) return st;
    if ((st = h->bs_x.reserve(B * cells)) != CLR_OK) return st;  // (read beside by the solve's summarize when it forms the maps)
  }
  const double solve_ms = mean ? h->solve_device_ms : 0.0;  // (the solve above: reported with this frame's kernels)
  ConsumerFrame frame{h};
  hipStream_t s = h->stream.get();
  HIP_TRY(hipMemcpyAsync(dxs.p, pts.up, nsrc * Mm * sizeof(double), hipMemcpyHostToDevice, s));
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
  bool forms_Q = false;
  if (var) {
    S.have_S = h->pv_S_valid ? 1 : 0;
    S.have_Q = h->loo_Q_valid ? 1 : 0;
    S.Q.lean = S.lean;
    S.Q.have_M = h->bs_M_valid ? 1 : 0;
    forms_Q = !S.have_Q;  // ... and with them the chunk maps, unless a solve has formed those
    if (forms_Q) h->bs_M_valid = false;
    h->pv_S_valid = h->loo_Q_valid = false;
    // (with `mean` the chunk maps are the solve's and bs_x holds alpha: the summarize beside them is not run)
    S.Q.cT = h->bs_x.p; S.Q.M = h->bs_M.p; S.Q.Q = h->loo_Q.p; S.Q.off = h->bs_off.p;
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
  if (var) {
    h->pv_S_valid = h->loo_Q_valid = true;
    if (forms_Q) h->bs_M_valid = true;
  }
  const double* tsrc[2] = {tmp.data(), tmp.data() + (mean ? B * Gg * Mm : 0)};
  double* tdst[2] = {mean, var};
  for (int o = 0; o < 2; ++o) {
    if (!tdst[o]) continue;
    if (pts.all_sorted) { std::copy(tsrc[o], tsrc[o] + B * Gg * Mm, tdst[o]); continue; }
    for (size_t b = 0; b < B; ++b) {
      const int* pp = pts.perm.data() + (xs_stride == 0 ? 0 : b * Mm);
      for (size_t g = 0; g < Gg; ++g) {
        const size_t at = (b * Gg + g) * Mm;
        for (size_t m = 0; m < Mm; ++m) tdst[o][at + pp[m]] = tsrc[o][at + m];
      }
    }
  }
  std::vector<int> stat;
  return nan_rows_without_factor(h, stat, {{mean, Gg * Mm}, {var, Gg * Mm}});
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
int clr_batch_leave_one_out(clr_batch* h, double* kinv_diag, double* alpha, double* loo_logpdf, int* status) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (!kinv_diag && !alpha && !loo_logpdf && !status)
    return fail(CLR_INVALID_ARGUMENT, "clr_batch_leave_one_out: at least one output array");
  if ((st = require_celerite_width(h, "clr_batch_leave_one_out")) != CLR_OK) return st;
  if ((st = require_factor(h, true)) != CLR_OK) return st;
  if (!h->launch && !clr::wsweep_scan_supported(h->N, h->J))
    return fail(CLR_UNSUPPORTED, "clr_batch_leave_one_out on a wide plan needs N >= 512");
  if (h->launch && h->nchunk < 2) return fail(CLR_UNSUPPORTED, "clr_batch_leave_one_out needs a chunked plan (N >= 128)");
  const size_t B = (size_t)h->B, N = (size_t)h->N, J = (size_t)h->J;
  const bool need_c = kinv_diag || loo_logpdf, need_alpha = alpha || loo_logpdf;
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
      // (the chunk maps are the batched solve's, under its validity rule: formed here unless a solve has formed them, and
      //  counted as formed only once this call's kernels have run to completion)
      S.have_M = h->bs_M_valid ? 1 : 0;
      h->bs_M_valid = false;
      h->loo_Q_valid = false;  // (loo_Q is rewritten: the offsets, then the start matrices -- as clr_batch_predict_var_recurrence reads them)
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
    if (h->launch) h->bs_M_valid = h->loo_Q_valid = true;
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
  // the statuses of the evaluation in force; a problem without a factor (or refused by the kernel program): NaN everywhere
  std::vector<int> stat(B);
  if ((st = clr_batch_get_results(h, nullptr, nullptr, nullptr, stat.data())) != CLR_OK) return st;
  mark_refused(h, nullptr, nullptr, nullptr, stat.data());
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t b = 0; b < B; ++b) {
    if (stat[b] == CLR_OK) continue;
    if (kinv_diag) std::fill(kinv_diag + b * N, kinv_diag + (b + 1) * N, nan);
    if (alpha) std::fill(alpha + b * N, alpha + (b + 1) * N, nan);
    if (loo_logpdf) loo_logpdf[b] = nan;
  }
  if (status) std::copy(stat.begin(), stat.end(), status);
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
  if ((st = require_celerite_width(h, "clr_batch_fit_mean_weights")) != CLR_OK) return st;
  if ((st = require_factor(h, true)) != CLR_OK) return st;
  if (h->B > 65535) return fail(CLR_UNSUPPORTED, "clr_batch_fit_mean_weights: at most 65535 problems per plan (a grid axis): shard the batch");
  if (!h->launch && !clr::wsweep_scan_supported(h->N, h->J))
    return fail(CLR_UNSUPPORTED, "clr_batch_fit_mean_weights on a wide plan needs N >= 512");
  if (h->launch && h->nchunk < 2) return fail(CLR_UNSUPPORTED, "clr_batch_fit_mean_weights needs a chunked plan (N >= 128)");
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
    if (h->launch) S = narrow_solve_begin(h, R);
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
  if (h->launch) h->bs_M_valid = true;
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
  std::vector<int> stat(B);
  if ((st = clr_batch_get_results(h, nullptr, nullptr, nullptr, stat.data())) != CLR_OK) return st;
  mark_refused(h, nullptr, nullptr, nullptr, stat.data());
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

int clr_batch_get_solve_ms(const clr_batch* h, double* device_ms) {
  if (device_ms) *device_ms = h->solve_device_ms;
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

void set_batch_context(clr_batch* h, int B_total) {
  h->group_B = B_total > h->B ? B_total : 0;  // (a single shard IS the whole batch)
}

long warm_eligible(const clr_batch* h) { return h->warm_eligible; }

void set_warm_eligible_total(clr_batch* h, long eligible_total) {
  if (h->group_B <= 0) return;
  const bool selectable = h->warm_mode != 0 && h->wnchunk >= 2 && h->have_series && !h->warm_span.empty() &&
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
