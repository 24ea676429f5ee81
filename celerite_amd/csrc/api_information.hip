// celerite_amd/csrc/api_information.hip -- C ABI of the information matrix of every problem of a narrow plan
// (clr_batch_information, clr_batch_set_information_tile): the evaluation by the scan, the forward-mode tangents of every
// direction chunk by chunk, the two numbers per sample and direction they carry, and their Gram matrix (clr_binfo_kernels.h).
#include "api_internal.h"

extern "C" {

int clr_batch_set_information_tile(clr_batch* h, int problems) {
  h->information_tile = problems > 0 ? problems : 0;
  return CLR_OK;
}

// The evaluation runs as clr_batch_grad's does (by the scan: its start states are the chunks' base states); then
//   * problems the scan settled: riders, zero-start tangents and the walk for the whole plan, which leave the true tangent
//     start state of every (gradient chunk, direction) in i_tan;
//   * a tile of problems at a time -- as many as hold their rows (2 M C doubles each) in the 1 GiB of the other tiled
//     consumers, or clr_batch_set_information_tile's -- the rows by the chunked route, or by the sequential form for the
//     problems the scan sent to the sequential recurrence (and for every problem of a plan under clr_batch_set_exact or
//     beyond the fast trigonometry's range), and their Gram matrix.
// A gradient chunk is g_m chunks of the scan, g_m from the chunking alone (never the batch size: a problem's bits must not
// depend on the batch or a sharding): the steps of a lane against the walk over the chunks, clr_batch_grad's model.
int clr_batch_information(clr_batch* h, int mean_partial, double* info, int* status) {
  int st = require_device(h->device);
  if (st != CLR_OK) return st;
  if (!h->launch || h->J_general > 0)
    return fail(CLR_UNSUPPORTED, "clr_batch_information: narrow plans (widths 1..8) with celerite terms only; wide plans and "
                                 "general terms are not covered");
  if (!info) return fail(CLR_INVALID_ARGUMENT, "clr_batch_information: info is null");
  if (mean_partial && h->mean_K > 0)
    return fail(CLR_UNSUPPORTED, "clr_batch_information: a linear mean is in force (clr_batch_set_mean_basis): its weights' "
                                 "block is the Gram matrix of clr_batch_fit_mean_weights");
  if (mean_partial && h->amp_active)
    return fail(CLR_UNSUPPORTED, "clr_batch_information: amplitudes are in force (clr_batch_set_amplitudes): a constant in data "
                                 "units is the mean-basis function 1");
  const size_t B = (size_t)h->B, J = (size_t)h->J, NG = 1 + 2 * (size_t)h->J_real + 4 * (size_t)h->J_comp;
  const size_t M = NG + (mean_partial ? 1 : 0), SZ = J * (J + 1) / 2, TAN = SZ + J, RID = J * J + J + SZ, NP = M * (M + 1) / 2;
  for (clr::Event& e : h->info_ev)
    if (!e) HIP_TRY(clr::create_event(e));
  HIP_TRY(hipEventRecord(h->info_ev[0].get(), h->stream.get()));
  h->grad_scan_only = true;
  st = clr_batch_enqueue(h, 0);
  h->grad_scan_only = false;
  if (st != CLR_OK) return st;
  clr::BatchParams P, Pi;
  if ((st = batch_params(h, 0, P, true)) != CLR_OK) return st;    // (the row-major arrays)
  if ((st = batch_params(h, 0, Pi, false)) != CLR_OK) return st;  // (the evaluation's own view)
  const bool seq_all = P.fast_trig == 0 || h->force_exact != 0;
  {
    int m = 1;
    double best = INFINITY;
    const double w2 = (double)(J * J) / 64.0, step = 0.3 + 2.4 * w2, walk = 0.5 + 4.5 * w2 * J / 8.0;
    for (int k = 1; k <= h->nchunk; ++k) {
      const double tm = (double)k * h->L * step + (double)((h->nchunk + k - 1) / k) * walk;
      if (tm < best) { best = tm; m = k; }
    }
    P.g_m = m;
    P.g_nchunk = (h->nchunk + m - 1) / m;
    if (m == 1 && Pi.lane_cs == 1 && !Pi.staged) {  // a gradient chunk is a scan chunk: read the interleaved copy
      P.t = Pi.t; P.diag = Pi.diag; P.y = Pi.y;
      P.t_stride = Pi.t_stride; P.diag_stride = Pi.diag_stride; P.y_stride = Pi.y_stride;
      P.lane_is = Pi.lane_is; P.lane_cs = Pi.lane_cs;
    } else {
      P.lane_is = 1; P.lane_cs = h->L;
    }
  }
  const size_t pc = B * (size_t)P.g_nchunk;
  clr::BInfoParams I;
  memset(&I, 0, sizeof(I));
  I.M = (int)M; I.mean = mean_partial ? 1 : 0; I.seq_all = seq_all ? 1 : 0;
  I.C = (long)P.g_nchunk * P.g_m * h->L;
  I.rm_t = h->t.p; I.rm_diag = h->diag.p; I.rm_y = h->y.p;
  I.rm_t_stride = h->t_stride; I.rm_diag_stride = h->diag_stride; I.rm_y_stride = h->y_stride;
  if (I.C > 2147483647L) return fail(CLR_UNSUPPORTED, "clr_batch_information: the series is too long");
  if (!seq_all) {
    if ((st = h->g_riders.reserve(pc * RID)) != CLR_OK) return st;
    if ((st = h->i_tan.reserve(pc * M * TAN)) != CLR_OK) return st;
    P.g_riders = h->g_riders.p;
    I.tan = h->i_tan.p;
    h->launch->information(P, I, 0, h->stream.get());
    HIP_TRY(hipGetLastError());
  }
  std::vector<int> stt(B), lvl(B);
  // (the scaled system's results; the call waits for the evaluation, and the routes are final behind it)
  if ((st = batch_results_scaled(h, nullptr, nullptr, nullptr, stt.data())) != CLR_OK) return st;
  HIP_TRY(hipMemcpyAsync(lvl.data(), P.need_exact, B * sizeof(int), hipMemcpyDeviceToHost, h->stream.get()));
  HIP_TRY(hipStreamSynchronize(h->stream.get()));

  const size_t per_problem = 2 * M * (size_t)I.C;
  const size_t budget = (size_t)1 << 27;  // doubles (predict_tile's)
  const size_t want = h->information_tile > 0 ? (size_t)h->information_tile : std::max<size_t>(1, budget / per_problem);
  const size_t Bt = std::min<size_t>(std::min<size_t>(want, B), 65535);  // (the problems ride on grid.y)
  I.nslab = (int)((2 * (size_t)I.C + clr::CLR_INFO_SLAB - 1) / clr::CLR_INFO_SLAB);
  if ((st = h->i_rows.reserve(Bt * per_problem)) != CLR_OK) return st;
  if ((st = h->i_part.reserve(Bt * (size_t)I.nslab * NP + Bt * M * M)) != CLR_OK) return st;
  I.rows = h->i_rows.p;
  I.part = h->i_part.p;
  I.out = h->i_part.p + Bt * (size_t)I.nslab * NP;
  for (size_t b0 = 0; b0 < B; b0 += Bt) {
    const size_t nb = std::min(Bt, B - b0);
    I.b0 = (int)b0; I.nb = (int)nb;
    bool any_seq = seq_all;
    for (size_t b = b0; b < b0 + nb; ++b) any_seq = any_seq || lvl[b] >= 2;
    if (!seq_all) h->launch->information(P, I, 1, h->stream.get());
    if (any_seq) h->launch->information(P, I, 2, h->stream.get());
    clr::launch_info_gram(I, h->stream.get());
    HIP_TRY(hipGetLastError());
    if (b0 + nb == B) HIP_TRY(hipEventRecord(h->info_ev[1].get(), h->stream.get()));
    HIP_TRY(hipMemcpyAsync(info + b0 * M * M, I.out, nb * M * M * sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
    HIP_TRY(hipStreamSynchronize(h->stream.get()));  // (the next tile overwrites the rows and the result)
  }
  {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->info_ev[0].get(), h->info_ev[1].get()));
    h->information_ms = ms;
  }

  // conventions: a problem that is not CLR_OK (not positive definite, a draw or a scale refused) gets NaN and its status; a
  // jitter the gradient treats as absent (clr_batch_grad) a zero row and column
  std::vector<double> dummy(B, 0.0);
  std::vector<int> refused(B, CLR_OK);
  if ((st = amplitude_adjust(h, dummy.data(), nullptr, nullptr, refused.data())) != CLR_OK) return st;
  for (size_t b = 0; b < B; ++b) {
    int sb = stt[b];
    if (refused[b] != CLR_OK) sb = refused[b];
    if (h->kp_in_force && h->kp_refused[b]) sb = CLR_INVALID_ARGUMENT;
    if (status) status[b] = sb;
    double* o = info + b * M * M;
    if (sb != CLR_OK) {
      std::fill(o, o + M * M, NAN);
    } else if (!(h->host_jitter[b] > 2.220446049250313e-16)) {
      for (size_t k = 0; k < M; ++k) o[k] = o[k * M] = 0.0;
    }
  }
  return CLR_OK;
}

int clr_batch_get_information_ms(const clr_batch* h, double* ms) {
  if (!ms) return fail(CLR_INVALID_ARGUMENT, "ms is null");
  *ms = h->information_ms;
  return CLR_OK;
}

}  // extern "C"
