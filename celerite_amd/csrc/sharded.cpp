// celerite_amd/csrc/sharded.cpp -- the batch axis over several GPUs (BASELINE
// config 4).  Problems are independent (all state of the reference solver is per object,
// cholesky.h:703-706), so a sharded plan is nothing but S single-device plans (clr_batch_*)
// over contiguous slices of the batch axis: no collective, no device-to-device traffic.
//
// EVERY decision a plan takes from a quantity over "its" problems is taken ONCE for the whole batch, so that a batch
// gives bit-identical results under any sharding with the default settings (given one chunk count, see below):
//  * kernel selection: the maxima the single-device plans look at (max |t|, largest time step, largest decay rate and
//    frequency) are taken over all problems and handed to every shard (clr_batch_set_selection_bounds);
//  * the prefix plan's time model, the one-launch path of short narrow problems and the deferral of level-1 problems
//    look at the size of the WHOLE batch (clr_group::set_batch_context);
//  * the warm-started recurrence (series that forget their past) is switched on when at least half
//    of the problems OF THE BATCH are eligible, and its warm-up lengths adapt to the fallbacks OF THE BATCH: the shards'
//    counts are added up here and handed back (reselect_all, resolve_all);
//  * level-1 problems left pending by an evaluation are re-planned as a side plan whose chunk count follows their number
//    IN THE BATCH (or replayed inline when the batch holds too many of them): resolve_all adds the pending counts up
//    between the two halves of every shard's resolve (clr_group_hooks.h).
// Round 5 left the last two per plan (bit-identity only with the warm start and the side plans switched off).
// The chunk count: all shards use the first shard's, i.e. the automatic choice looks at a SHARD's batch size -- what
// fills one GPU -- and may differ from the unsharded plan's; clr_sharded_set_chunks pins it (a pinned count also pins the
// warm path's chunking), and with equal chunk counts the bits are equal.
//
// Each shard has its own host worker thread (which owns the shard's HIP device binding,
// stream and pinned staging through its clr_batch handle); an API call posts one job to every
// worker and waits for all of them, so the shards' uploads, launches and downloads overlap.
// A device may be listed more than once: the shards then share that GPU.  That is how the
// sharding is tested on a one-GPU box (tests/test_gpu_batch.py: 1, 2, 3, 8 shards must give
// bit-identical results).
#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/celerite_hip.h"
#include "clr_group_hooks.h"

namespace {

struct Worker {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::function<int()> job;
  bool has_job = false, done = true, quit = false;
  int status = CLR_OK;
  std::string error;

  void loop() {
    for (;;) {
      std::function<int()> j;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return has_job || quit; });
        if (quit) return;
        j = std::move(job);
        has_job = false;
      }
      const int st = j();
      std::string msg;
      if (st != CLR_OK) msg = clr_last_error();  // (thread-local in the library: read it here)
      {
        std::lock_guard<std::mutex> lk(mu);
        status = st;
        error = std::move(msg);
        done = true;
      }
      cv.notify_all();
    }
  }
  void post(std::function<int()> j) {
    {
      std::lock_guard<std::mutex> lk(mu);
      job = std::move(j);
      has_job = true;
      done = false;
    }
    cv.notify_all();
  }
  int wait() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return done; });
    return status;
  }
  void stop() {
    {
      std::lock_guard<std::mutex> lk(mu);
      quit = true;
    }
    cv.notify_all();
    if (th.joinable()) th.join();
  }
  ~Worker() { stop(); }
};

thread_local std::string g_sharded_error;

}  // namespace

struct clr_sharded {
  int B = 0, N = 0, J_real = 0, J_comp = 0;
  int n_params = 0;  // of the kernel set by clr_sharded_set_kernel
  int mean_K = 0;    // of the basis set by clr_sharded_set_mean_basis
  int noise_K = 0;   // of the basis set by clr_sharded_set_noise_basis
  int amp_K = 0;     // of the basis set by clr_sharded_set_amplitude_basis
  std::vector<int> device, lo, hi;
  std::vector<clr_batch*> plan;
  std::vector<std::unique_ptr<Worker>> worker;

  // run f(shard) on every shard's worker; first non-OK status wins
  int all(const std::function<int(int)>& f) {
    const int S = (int)plan.size();
    for (int s = 0; s < S; ++s) worker[s]->post([=] { return f(s); });
    int st = CLR_OK;
    for (int s = 0; s < S; ++s) {
      const int r = worker[s]->wait();
      if (r != CLR_OK && st == CLR_OK) {
        st = r;
        g_sharded_error = "shard " + std::to_string(s) + " (device " + std::to_string(device[s]) +
                          "): " + worker[s]->error;
      }
    }
    return st;
  }
};

namespace {

// the warm path's activation: eligible problems of the whole batch -> every shard (host fields only; the workers idle)
void reselect_all(clr_sharded* h) {
  if (h->plan.size() < 2) return;
  long total = 0;
  for (clr_batch* p : h->plan) total += clr_group::warm_eligible(p);
  for (clr_batch* p : h->plan) clr_group::set_warm_eligible_total(p, total);
}

// the two halves of the shards' resolve around the batch-wide sums (pending problems, warm-eligible problems)
int resolve_finish_all(clr_sharded* h, const std::vector<long>& pend, const std::vector<long>& elig,
                       const std::function<int(int)>& then) {
  long P = 0, E = 0;
  for (long v : pend) P += v;
  for (long v : elig) E += v;
  return h->all([=](int s) {
    const int st = clr_group::resolve_finish(h->plan[s], P, E);
    return (st == CLR_OK && then) ? then(s) : st;
  });
}

int resolve_all(clr_sharded* h) {
  if (h->plan.size() < 2) return CLR_OK;  // (a single shard is the whole batch: its plan resolves by itself)
  bool any = false;
  for (clr_batch* p : h->plan) any = any || clr_group::in_flight(p);
  if (!any) return CLR_OK;
  const size_t S = h->plan.size();
  std::vector<long> pend(S, 0), elig(S, 0);
  long* pp = pend.data();
  long* ee = elig.data();
  const int st = h->all([=](int s) { return clr_group::resolve_begin(h->plan[s], pp + s, ee + s); });
  if (st != CLR_OK) return st;
  return resolve_finish_all(h, pend, elig, nullptr);
}

// the batched consumers on every shard concurrently, each on its slice of the host arrays (`f(plan, lo)`, lo = the
// shard's first problem): arguments that are not `valid` are refused before any shard runs
int on_slices(clr_sharded* h, bool valid, const std::function<int(clr_batch*, long)>& f) {
  if (!valid) return CLR_INVALID_ARGUMENT;
  const int st = resolve_all(h);
  if (st != CLR_OK) return st;
  return h->all([=](int s) { return f(h->plan[s], h->lo[s]); });
}

template <class T>
T* at(T* p, long off) { return p ? p + off : nullptr; }

// clr_batch_get_results of shard s into its slice of the caller's arrays (any of them may be null)
int slice_results(clr_sharded* h, int s, double* loglike, double* logdet, double* quad, int* status) {
  const long lo = h->lo[s];
  return clr_batch_get_results(h->plan[s], at(loglike, lo), at(logdet, lo), at(quad, lo), at(status, lo));
}

// two of the shards' selection maxima (the series' max |t| and largest step, or the coefficients' largest frequency and
// decay rate) over the WHOLE batch -> every shard
void spread_maxima(clr_sharded* h, bool of_series) {
  double m0 = 0.0, m1 = 0.0;
  for (clr_batch* p : h->plan) {
    double a = 0.0, b = 0.0;
    if (of_series) clr_batch_get_selection_bounds(p, &a, &b, nullptr, nullptr, nullptr);
    else clr_batch_get_selection_bounds(p, nullptr, nullptr, &a, &b, nullptr);
    if (!(a <= m0)) m0 = a;
    if (!(b <= m1)) m1 = b;
  }
  for (clr_batch* p : h->plan) {
    if (of_series) clr_batch_set_selection_bounds(p, m0, m1, -1.0, -1.0);
    else clr_batch_set_selection_bounds(p, -1.0, -1.0, m0, m1);
  }
}

// One evaluation of the whole batch, then results(shard) on every shard.  One shard: its plan is the whole batch and
// resolves by itself -- one job, with `before` (when given: the new coefficients) in front of the launch.  Several: two
// rounds of jobs with the batch-wide sums between them -- launches + the first half of the resolve (then the pending /
// eligible counts of the whole batch); the second half + the results.
int evaluate_rounds(clr_sharded* h, int materialize, const std::function<int(int)>& results,
                    const std::function<int(int)>& before = nullptr) {
  if (h->plan.size() < 2)
    return h->all([=](int s) {
      int st = before ? before(s) : (int)CLR_OK;
      if (st == CLR_OK) st = clr_batch_enqueue(h->plan[s], materialize);
      return st == CLR_OK ? results(s) : st;
    });
  const size_t S = h->plan.size();
  std::vector<long> pend(S, 0), elig(S, 0);
  long* pp = pend.data();
  long* ee = elig.data();
  const int st = h->all([=](int s) {
    const int e = clr_batch_enqueue(h->plan[s], materialize);
    return e != CLR_OK ? e : clr_group::resolve_begin(h->plan[s], pp + s, ee + s);
  });
  if (st != CLR_OK) return st;
  return resolve_finish_all(h, pend, elig, results);
}

}  // namespace

extern "C" {

int clr_shard_bounds(int total, int nshards, int shard, int* lo, int* hi) {
  if (total < 0 || nshards < 1 || shard < 0 || shard >= nshards) return CLR_INVALID_ARGUMENT;
  const int base = total / nshards, extra = total % nshards;
  const int l = shard * base + (shard < extra ? shard : extra);
  if (lo) *lo = l;
  if (hi) *hi = l + base + (shard < extra ? 1 : 0);
  return CLR_OK;
}

const char* clr_sharded_last_error(void) { return g_sharded_error.c_str(); }

void clr_sharded_destroy(clr_sharded* h) {
  if (!h) return;
  for (size_t s = 0; s < h->worker.size(); ++s) {
    clr_batch* p = s < h->plan.size() ? h->plan[s] : nullptr;
    if (p) {
      h->worker[s]->post([p] { clr_batch_destroy(p); return (int)CLR_OK; });
      h->worker[s]->wait();
    }
  }
  delete h;  // (stops and joins the worker threads)
}

clr_sharded* clr_sharded_create(int B, int N, int J_real, int J_comp, const int* devices, int nshards) {
  g_sharded_error.clear();
  if (B < 1 || N < 1 || nshards < 1 || !devices) {
    g_sharded_error = "clr_sharded_create: bad sizes";
    return nullptr;
  }
  if (nshards > B) nshards = B;  // (no empty shards)
  const int ndev = clr_device_count();
  if (ndev < 1) {
    g_sharded_error = "no gfx950 (MI355X) device is visible; libcelerite_hip has no CPU path";
    return nullptr;
  }
  for (int s = 0; s < nshards; ++s)
    if (devices[s] < 0 || devices[s] >= ndev) {
      g_sharded_error = "clr_sharded_create: device index " + std::to_string(devices[s]) + " out of range (" +
                        std::to_string(ndev) + " visible)";
      return nullptr;
    }
  clr_sharded* h = new clr_sharded();
  h->B = B; h->N = N; h->J_real = J_real; h->J_comp = J_comp;
  h->plan.assign(nshards, nullptr);
  for (int s = 0; s < nshards; ++s) {
    int lo = 0, hi = 0;
    clr_shard_bounds(B, nshards, s, &lo, &hi);
    h->device.push_back(devices[s]);
    h->lo.push_back(lo);
    h->hi.push_back(hi);
    h->worker.push_back(std::make_unique<Worker>());
    Worker* w = h->worker.back().get();
    w->th = std::thread([w] { w->loop(); });
  }
  const int st = h->all([h, N, J_real, J_comp](int s) {
    h->plan[s] = clr_batch_create(h->hi[s] - h->lo[s], N, J_real, J_comp, h->device[s]);
    return h->plan[s] ? (int)CLR_OK : (int)CLR_HIP_ERROR;
  });
  if (st != CLR_OK) {
    const std::string keep = g_sharded_error;
    clr_sharded_destroy(h);
    g_sharded_error = keep;
    return nullptr;
  }
  for (clr_batch* p : h->plan) clr_group::set_batch_context(p, nshards > 1 ? B : 0);
  // one chunk count for all shards (the automatic choice looks at the shard's own batch size, which differs by
  // one between shards when B is not a multiple of the shard count)
  int nchunk = 0;
  clr_batch_get_chunks(h->plan[0], &nchunk, nullptr);
  if (nshards > 1) (void)clr_sharded_set_chunks(h, nchunk);
  return h;
}

int clr_sharded_num_shards(const clr_sharded* h) { return (int)h->plan.size(); }

int clr_sharded_get_shard(const clr_sharded* h, int shard, int* device, int* lo, int* hi) {
  if (shard < 0 || shard >= (int)h->plan.size()) return CLR_INVALID_ARGUMENT;
  if (device) *device = h->device[shard];
  if (lo) *lo = h->lo[shard];
  if (hi) *hi = h->hi[shard];
  return CLR_OK;
}

int clr_sharded_set_chunks(clr_sharded* h, int nchunk) {
  int st = resolve_all(h);
  if (st != CLR_OK) return st;
  if (nchunk <= 0 && h->plan.size() > 1) {  // automatic: the first shard's choice for all
    clr_batch* p0 = h->plan[0];
    h->worker[0]->post([p0] { return clr_batch_set_chunks(p0, 0); });  // (on the shard's own thread: its device binding)
    if ((st = h->worker[0]->wait()) != CLR_OK) return st;
    clr_batch_get_chunks(p0, &nchunk, nullptr);
  }
  st = h->all([=](int s) { return clr_batch_set_chunks(h->plan[s], nchunk); });
  reselect_all(h);
  return st;
}

int clr_sharded_set_warm_start(clr_sharded* h, int mode, int forced_warmup) {
  int st = resolve_all(h);
  if (st != CLR_OK) return st;
  st = h->all([=](int s) { return clr_batch_set_warm_start(h->plan[s], mode, forced_warmup); });
  reselect_all(h);
  return st;
}

int clr_sharded_set_rescue(clr_sharded* h, int mode) {
  const int st = resolve_all(h);
  if (st != CLR_OK) return st;
  return h->all([=](int s) { return clr_batch_set_rescue(h->plan[s], mode); });
}

int clr_sharded_set_certificate(clr_sharded* h, double max_gamma_over_mu, double max_residual, double max_gamma,
                                double max_gamma_times_error) {
  const int st0 = resolve_all(h);
  if (st0 != CLR_OK) return st0;
  return h->all([=](int s) {
    int st = clr_batch_set_certificate(h->plan[s], max_gamma_over_mu, max_residual);
    if (st == CLR_OK && !(max_gamma < 0.0) && !(max_gamma_times_error < 0.0))
      st = clr_batch_set_certificate_gamma(h->plan[s], max_gamma, max_gamma_times_error);
    return st;
  });
}

int clr_sharded_get_rescue(const clr_sharded* h, int* last_count) {
  // problems of the last fetched evaluation that were re-planned, summed over the shards (inline replays count negative)
  int total = 0;
  for (clr_batch* p : h->plan) {
    int n = 0;
    const int st = clr_batch_get_rescue(p, &n, nullptr, nullptr, nullptr);
    if (st != CLR_OK) return st;
    total += n < 0 ? -n : n;
  }
  if (last_count) *last_count = total;
  return CLR_OK;
}

int clr_sharded_set_summarize_mode(clr_sharded* h, int mode) {
  const int st0 = resolve_all(h);
  if (st0 != CLR_OK) return st0;
  return h->all([=](int s) { return clr_batch_set_summarize_mode(h->plan[s], mode); });
}

int clr_sharded_get_chunks(const clr_sharded* h, int shard, int* nchunk, int* chunk_len) {
  if (shard < 0 || shard >= (int)h->plan.size()) return CLR_INVALID_ARGUMENT;
  return clr_batch_get_chunks(h->plan[shard], nchunk, chunk_len);
}

int clr_sharded_set_series(clr_sharded* h, const double* t, long t_stride, const double* diag,
                           long diag_stride, const double* y, long y_stride) {
  int st = resolve_all(h);  // (an evaluation in flight is settled on ITS series, by the counts of the whole batch)
  if (st != CLR_OK) return st;
  st = h->all([=](int s) {
    const long lo = h->lo[s];
    return clr_batch_set_series(h->plan[s], t + lo * t_stride, t_stride, diag + lo * diag_stride,
                                diag_stride, y + lo * y_stride, y_stride);
  });
  if (st != CLR_OK) return st;
  // the series' maxima over the WHOLE batch (every shard scanned its own slice during the upload)
  spread_maxima(h, true);
  reselect_all(h);
  return CLR_OK;
}

int clr_sharded_set_series_ragged(clr_sharded* h, const double* t, long t_stride, const double* diag, long diag_stride,
                                  const double* y, long y_stride, const int* lengths) {
  if (!lengths) return clr_sharded_set_series(h, t, t_stride, diag, diag_stride, y, y_stride);
  // whether lengths are in force is decided once, over the WHOLE batch; a bad length is refused before any shard changes
  bool ragged = false;
  for (int b = 0; b < h->B; ++b) {
    if (lengths[b] < 1 || lengths[b] > h->N) {
      g_sharded_error = "clr_sharded_set_series_ragged: length " + std::to_string(lengths[b]) + " of problem " +
                        std::to_string(b) + " is outside [1, N]";
      return CLR_INVALID_ARGUMENT;
    }
    ragged = ragged || lengths[b] != h->N;
  }
  if (ragged && (t_stride == 0 || diag_stride == 0 || y_stride == 0)) {
    g_sharded_error = "clr_sharded_set_series_ragged: with lengths t, diag and y are each [B][N] (stride N)";
    return CLR_INVALID_ARGUMENT;
  }
  int st = resolve_all(h);
  if (st != CLR_OK) return st;
  st = h->all([=](int s) {
    const long lo = h->lo[s];
    return clr_group::set_series_lengths(h->plan[s], t + lo * t_stride, t_stride, diag + lo * diag_stride, diag_stride,
                                         y + lo * y_stride, y_stride, lengths + lo, ragged);
  });
  if (st != CLR_OK) return st;
  spread_maxima(h, true);
  reselect_all(h);
  return CLR_OK;
}

int clr_sharded_get_lengths(const clr_sharded* h, int* lengths) {
  if (!lengths) {
    g_sharded_error = "clr_sharded_get_lengths: lengths is null";
    return CLR_INVALID_ARGUMENT;
  }
  for (size_t s = 0; s < h->plan.size(); ++s) {
    const int st = clr_batch_get_lengths(h->plan[s], lengths + h->lo[s]);
    if (st != CLR_OK) {
      g_sharded_error = "shard " + std::to_string(s) + ": " + clr_last_error();
      return st;
    }
  }
  return CLR_OK;
}

int clr_sharded_get_series_order(const clr_sharded* h, double* dtmin) {
  // the smallest step over the shards' finite values; a negative one ("not sorted") wins over a NaN time in any
  // shard, and only a batch without a negative step reports NaN (clr_batch_get_series_order has the same rule)
  double m = 1.0 / 0.0;
  bool nan = false;
  for (clr_batch* p : h->plan) {
    double d = 0.0;
    const int st = clr_batch_get_series_order(p, &d);
    if (st != CLR_OK) return st;
    if (d != d) nan = true;
    else if (d < m) m = d;
  }
  if (dtmin) *dtmin = (m < 0.0) ? m : (nan ? 0.0 / 0.0 : m);
  return CLR_OK;
}

int clr_sharded_clear_series(clr_sharded* h) {
  const int st0 = resolve_all(h);
  if (st0 != CLR_OK) return st0;
  return h->all([=](int s) { return clr_batch_clear_series(h->plan[s]); });
}

// largest |d_comp| and decay rate over the whole batch -> every shard (before it takes its slice)
static void global_coefficient_bounds(clr_sharded* h, const double* c_real, const double* c_comp, const double* d_comp) {
  double dmax = 0.0, cmax = 0.0;
  const size_t nr = (size_t)h->B * h->J_real, nc = (size_t)h->B * h->J_comp;
  for (size_t i = 0; i < nc; ++i) {
    const double m = d_comp[i] < 0 ? -d_comp[i] : d_comp[i], c = c_comp[i] < 0 ? -c_comp[i] : c_comp[i];
    if (!(m <= dmax)) dmax = m;
    if (!(c <= cmax)) cmax = c;
  }
  for (size_t i = 0; i < nr; ++i) {
    const double c = c_real[i] < 0 ? -c_real[i] : c_real[i];
    if (!(c <= cmax)) cmax = c;
  }
  for (clr_batch* p : h->plan) clr_batch_set_selection_bounds(p, -1.0, -1.0, dmax, cmax);
}

int clr_sharded_get_summarize_kernel(const clr_sharded* h, int* kind) {
  if (!kind) return CLR_INVALID_ARGUMENT;
  int k0 = 0;
  int st = clr_batch_get_summarize_kernel(h->plan[0], &k0);
  for (size_t s = 1; s < h->plan.size() && st == CLR_OK; ++s) {
    int k = 0;
    st = clr_batch_get_summarize_kernel(h->plan[s], &k);
    if (k != k0) k0 = -1;  // (cannot happen once series and coefficients went through this layer)
  }
  *kind = k0;
  return st;
}

int clr_sharded_set_coefficients(clr_sharded* h, const double* jitter, const double* a_real,
                                 const double* c_real, const double* a_comp, const double* b_comp,
                                 const double* c_comp, const double* d_comp) {
  const long JR = h->J_real, JC = h->J_comp;
  int st = resolve_all(h);  // (pending problems of an evaluation in flight: at ITS coefficients and selection bounds)
  if (st != CLR_OK) return st;
  global_coefficient_bounds(h, c_real, c_comp, d_comp);
  st = h->all([=](int s) {
    const long lo = h->lo[s];
    return clr_batch_set_coefficients(h->plan[s], jitter ? jitter + lo : nullptr, a_real + lo * JR, c_real + lo * JR,
                                      a_comp + lo * JC, b_comp + lo * JC, c_comp + lo * JC,
                                      d_comp + lo * JC);
  });
  reselect_all(h);
  return st;
}

int clr_sharded_enqueue(clr_sharded* h) {
  return h->all([=](int s) { return clr_batch_enqueue(h->plan[s], 0); });
}

int clr_sharded_synchronize(clr_sharded* h) {
  const int st0 = resolve_all(h);
  if (st0 != CLR_OK) return st0;
  return h->all([=](int s) { return clr_batch_synchronize(h->plan[s]); });
}

int clr_sharded_get_results(clr_sharded* h, double* loglike, double* logdet, double* quad, int* status) {
  const int st0 = resolve_all(h);
  if (st0 != CLR_OK) return st0;
  return h->all([=](int s) { return slice_results(h, s, loglike, logdet, quad, status); });
}

// value + gradient of every problem at the coefficients in force: clr_batch_grad on every shard concurrently
int clr_sharded_grad(clr_sharded* h, double* value, double* grad, int* status) {
  const long NG = 1 + 2 * (long)h->J_real + 4 * (long)h->J_comp;
  const int st0 = resolve_all(h);
  if (st0 != CLR_OK) return st0;
  return h->all([=](int s) {
    const long lo = h->lo[s];
    return clr_batch_grad(h->plan[s], value ? value + lo : nullptr, grad ? grad + lo * NG : nullptr,
                          status ? status + lo : nullptr);
  });
}

// the information matrix of every problem at the coefficients in force: clr_batch_information on every shard concurrently
int clr_sharded_information(clr_sharded* h, int mean_partial, double* info, int* status) {
  const long M = 1 + 2 * (long)h->J_real + 4 * (long)h->J_comp + (mean_partial ? 1 : 0);
  if (!info) return CLR_INVALID_ARGUMENT;
  const int st0 = resolve_all(h);
  if (st0 != CLR_OK) return st0;
  return h->all([=](int s) {
    const long lo = h->lo[s];
    return clr_batch_information(h->plan[s], mean_partial, info + lo * M * M, status ? status + lo : nullptr);
  });
}

int clr_sharded_set_information_tile(clr_sharded* h, int problems) {
  for (clr_batch* p : h->plan) clr_batch_set_information_tile(p, problems);
  return CLR_OK;
}

int clr_sharded_evaluate(clr_sharded* h, const double* jitter, const double* a_real, const double* c_real,
                         const double* a_comp, const double* b_comp, const double* c_comp,
                         const double* d_comp, double* loglike, double* logdet, double* quad, int* status) {
  // one shard: coefficients, launch and results in ONE job (the headline loop saves two worker round trips); several: the
  // coefficients first (then the warm path's activation over the whole batch)
  std::function<int(int)> coefficients;
  if (h->plan.size() < 2) {
    global_coefficient_bounds(h, c_real, c_comp, d_comp);
    coefficients = [=](int s) { return clr_batch_set_coefficients(h->plan[s], jitter, a_real, c_real, a_comp, b_comp, c_comp, d_comp); };
  } else {
    const int st = clr_sharded_set_coefficients(h, jitter, a_real, c_real, a_comp, b_comp, c_comp, d_comp);
    if (st != CLR_OK) return st;
  }
  return evaluate_rounds(h, 0, [=](int s) { return slice_results(h, s, loglike, logdet, quad, status); }, coefficients);
}

int clr_sharded_set_mean(clr_sharded* h, const double* mu, long mu_stride) {
  if (mu && mu_stride != 0 && mu_stride != 1) return CLR_INVALID_ARGUMENT;
  const long n = mu ? (mu_stride ? h->B : 1) : 0;
  for (long i = 0; i < n; ++i)  // (checked here: an invalid mean leaves EVERY shard unchanged)
    if (!std::isfinite(mu[i])) return CLR_INVALID_ARGUMENT;
  const int st = resolve_all(h);  // (an evaluation in flight is settled on ITS residual)
  if (st != CLR_OK) return st;
  return h->all([=](int s) { return clr_batch_set_mean(h->plan[s], mu ? mu + h->lo[s] * mu_stride : nullptr, mu_stride); });
}

int clr_sharded_evaluate_mean(clr_sharded* h, const double* mean, long mean_stride, const double* jitter,
                              const double* a_real, const double* c_real, const double* a_comp, const double* b_comp,
                              const double* c_comp, const double* d_comp, double* loglike, double* logdet,
                              double* quad, int* status) {
  const int st = clr_sharded_set_mean(h, mean, mean_stride);
  if (st != CLR_OK) return st;
  return clr_sharded_evaluate(h, jitter, a_real, c_real, a_comp, b_comp, c_comp, d_comp, loglike, logdet, quad, status);
}

int clr_sharded_grad_mean(clr_sharded* h, double* value, double* grad, double* dmean, int* status) {
  const long NG = 1 + 2 * (long)h->J_real + 4 * (long)h->J_comp;
  const int st0 = resolve_all(h);
  if (st0 != CLR_OK) return st0;
  return h->all([=](int s) {
    const long lo = h->lo[s];
    return clr_batch_grad_mean(h->plan[s], value ? value + lo : nullptr, grad ? grad + lo * NG : nullptr,
                               dmean ? dmean + lo : nullptr, status ? status + lo : nullptr);
  });
}

/* ---- a linear mean: clr_batch_set_mean_basis / _set_mean_weights / _grad_mean_weights over the shards ---- */
int clr_sharded_set_mean_basis(clr_sharded* h, int K, const double* phi, long phi_stride) {
  const bool remove = K == 0 || !phi;
  const long per = (long)K * h->N;
  if (!remove) {  // (checked here: an invalid basis leaves EVERY shard unchanged)
    g_sharded_error = "clr_sharded_set_mean_basis: 1 <= K <= CLR_MAX_MEAN_BASIS = 16, phi_stride 0 or K * N, finite entries";
    if (K < 0 || K > CLR_MAX_MEAN_BASIS || (phi_stride != 0 && phi_stride != per)) return CLR_INVALID_ARGUMENT;
    const long n = phi_stride ? per * h->B : per;
    for (long i = 0; i < n; ++i)
      if (!std::isfinite(phi[i])) return CLR_INVALID_ARGUMENT;
  }
  int st = resolve_all(h);  // (an evaluation in flight is settled on ITS residual)
  if (st != CLR_OK) return st;
  st = h->all([=](int s) {
    return clr_batch_set_mean_basis(h->plan[s], remove ? 0 : K, remove ? nullptr : phi + h->lo[s] * phi_stride, phi_stride);
  });
  if (st == CLR_OK) h->mean_K = remove ? 0 : K;
  return st;
}

int clr_sharded_set_mean_weights(clr_sharded* h, const double* w) {
  const long K = h->mean_K;
  g_sharded_error = "clr_sharded_set_mean_weights: a basis must be set (clr_sharded_set_mean_basis) and the weights finite";
  if (K == 0 || !w) return CLR_INVALID_ARGUMENT;
  for (long i = 0; i < K * h->B; ++i)
    if (!std::isfinite(w[i])) return CLR_INVALID_ARGUMENT;
  const int st = resolve_all(h);
  if (st != CLR_OK) return st;
  return h->all([=](int s) { return clr_batch_set_mean_weights(h->plan[s], w + h->lo[s] * K); });
}

int clr_sharded_grad_mean_weights(clr_sharded* h, double* dw, int* status) {
  const long K = h->mean_K;
  return on_slices(h, K > 0 && dw, [=](clr_batch* p, long lo) {
    return clr_batch_grad_mean_weights(p, dw + lo * K, status ? status + lo : nullptr);
  });
}

/* ---- a linear noise model: clr_batch_set_noise_basis / _set_noise_weights / _grad_noise_weights over the shards ---- */
int clr_sharded_set_noise_basis(clr_sharded* h, int K, const double* psi, long psi_stride) {
  const bool remove = K == 0 || !psi;
  const long per = (long)K * h->N;
  if (!remove) {  // (checked here: an invalid basis leaves EVERY shard unchanged)
    g_sharded_error = "clr_sharded_set_noise_basis: 1 <= K <= CLR_MAX_NOISE_BASIS = 16, psi_stride 0 or K * N, finite entries";
    if (K < 0 || K > CLR_MAX_NOISE_BASIS || (psi_stride != 0 && psi_stride != per)) return CLR_INVALID_ARGUMENT;
    // the lengths in force (N for every problem of a uniform batch, or before a series is set): a row's tail is never
    // looked at -- of the one shared basis the tail past the longest problem OF THE BATCH
    std::vector<int> len((size_t)h->B, h->N);
    for (size_t s = 0; s < h->plan.size(); ++s) (void)clr_batch_get_lengths(h->plan[s], len.data() + h->lo[s]);
    const int longest = *std::max_element(len.begin(), len.end());
    const long rows = psi_stride ? (long)K * h->B : K;
    for (long r = 0; r < rows; ++r) {
      const int upto = psi_stride ? len[(size_t)(r / K)] : longest;
      for (int i = 0; i < upto; ++i)
        if (!std::isfinite(psi[r * h->N + i])) return CLR_INVALID_ARGUMENT;
    }
  }
  int st = resolve_all(h);  // (an evaluation in flight is settled on ITS variances)
  if (st != CLR_OK) return st;
  st = h->all([=](int s) {
    return clr_batch_set_noise_basis(h->plan[s], remove ? 0 : K, remove ? nullptr : psi + h->lo[s] * psi_stride, psi_stride);
  });
  if (st == CLR_OK) h->noise_K = remove ? 0 : K;
  return st;
}

int clr_sharded_set_noise_weights(clr_sharded* h, const double* w) {
  const long K = h->noise_K;
  g_sharded_error = "clr_sharded_set_noise_weights: a basis must be set (clr_sharded_set_noise_basis) and the weights finite";
  if (K == 0 || !w) return CLR_INVALID_ARGUMENT;
  for (long i = 0; i < K * h->B; ++i)
    if (!std::isfinite(w[i])) return CLR_INVALID_ARGUMENT;
  const int st = resolve_all(h);
  if (st != CLR_OK) return st;
  return h->all([=](int s) { return clr_batch_set_noise_weights(h->plan[s], w + h->lo[s] * K); });
}

int clr_sharded_grad_noise_weights(clr_sharded* h, double* ds, int* status) {
  const long K = h->noise_K;
  g_sharded_error = "clr_sharded_grad_noise_weights: a basis must be set (clr_sharded_set_noise_basis), and an output array";
  return on_slices(h, K > 0 && ds, [=](clr_batch* p, long lo) {
    return clr_batch_grad_noise_weights(p, ds + lo * K, status ? status + lo : nullptr);
  });
}

// the projection's device time: the largest over the shards, which run concurrently
int clr_sharded_get_noise_project_ms(const clr_sharded* h, double* device_ms) {
  double m = 0.0;
  for (clr_batch* p : h->plan) {
    double v = 0.0;
    (void)clr_batch_get_noise_project_ms(p, &v);
    m = std::max(m, v);
  }
  if (device_ms) *device_ms = m;
  return CLR_OK;
}

/* ---- the amplitude model: clr_batch_set_amplitude_basis / _set_amplitudes / _grad_amplitudes over the shards -------- */
int clr_sharded_set_amplitude_basis(clr_sharded* h, int K, const double* gamma, long gamma_stride) {
  const bool remove = K == 0 || !gamma;
  const long per = (long)K * h->N;
  if (!remove) {  // (checked here: an invalid basis leaves EVERY shard unchanged)
    g_sharded_error = "clr_sharded_set_amplitude_basis: 1 <= K <= CLR_MAX_AMPLITUDE_BASIS = 16, gamma_stride 0 or K * N, finite entries";
    if (K < 0 || K > CLR_MAX_AMPLITUDE_BASIS || (gamma_stride != 0 && gamma_stride != per)) return CLR_INVALID_ARGUMENT;
    // the lengths in force, as clr_sharded_set_noise_basis: of the one shared basis the tail past the longest problem OF
    // THE BATCH is never looked at
    std::vector<int> len((size_t)h->B, h->N);
    for (size_t s = 0; s < h->plan.size(); ++s) (void)clr_batch_get_lengths(h->plan[s], len.data() + h->lo[s]);
    const int longest = *std::max_element(len.begin(), len.end());
    const long rows = gamma_stride ? (long)K * h->B : K;
    for (long r = 0; r < rows; ++r) {
      const int upto = gamma_stride ? len[(size_t)(r / K)] : longest;
      for (int i = 0; i < upto; ++i)
        if (!std::isfinite(gamma[r * h->N + i])) return CLR_INVALID_ARGUMENT;
    }
  }
  int st = resolve_all(h);  // (an evaluation in flight is settled on ITS series)
  if (st != CLR_OK) return st;
  st = h->all([=](int s) {
    return clr_batch_set_amplitude_basis(h->plan[s], remove ? 0 : K, remove ? nullptr : gamma + h->lo[s] * gamma_stride, gamma_stride);
  });
  if (st == CLR_OK) h->amp_K = remove ? 0 : K;
  return st;
}

int clr_sharded_set_amplitudes(clr_sharded* h, const double* a) {
  const long K = h->amp_K;
  g_sharded_error = "clr_sharded_set_amplitudes: a basis must be set (clr_sharded_set_amplitude_basis) and the amplitudes finite";
  if (K == 0 || !a) return CLR_INVALID_ARGUMENT;
  for (long i = 0; i < K * h->B; ++i)
    if (!std::isfinite(a[i])) return CLR_INVALID_ARGUMENT;
  const int st = resolve_all(h);
  if (st != CLR_OK) return st;
  return h->all([=](int s) { return clr_batch_set_amplitudes(h->plan[s], a + h->lo[s] * K); });
}

int clr_sharded_get_log_amplitude_sum(clr_sharded* h, double* L) {
  g_sharded_error = "clr_sharded_get_log_amplitude_sum: an output array";
  return on_slices(h, L != nullptr, [=](clr_batch* p, long lo) { return clr_batch_get_log_amplitude_sum(p, L + lo); });
}

int clr_sharded_grad_amplitudes(clr_sharded* h, double* da, int* status) {
  const long K = h->amp_K;
  g_sharded_error = "clr_sharded_grad_amplitudes: a basis must be set (clr_sharded_set_amplitude_basis), and an output array";
  return on_slices(h, K > 0 && da, [=](clr_batch* p, long lo) {
    return clr_batch_grad_amplitudes(p, da + lo * K, status ? status + lo : nullptr);
  });
}

// the projection's device time: the largest over the shards, which run concurrently
int clr_sharded_get_amplitude_project_ms(const clr_sharded* h, double* device_ms) {
  double m = 0.0;
  for (clr_batch* p : h->plan) {
    double v = 0.0;
    (void)clr_batch_get_amplitude_project_ms(p, &v);
    m = std::max(m, v);
  }
  if (device_ms) *device_ms = m;
  return CLR_OK;
}

// clr_batch_fit_mean_weights, every shard on its slice (a problem's fit does not depend on the sharding)
int clr_sharded_fit_mean_weights(clr_sharded* h, double min_pivot, double* w_hat, double* cov, double* gram,
                                 double* quad_profiled, double* logdet_gram, int* status) {
  const long K = h->mean_K, K1 = K + 1;
  g_sharded_error = "clr_sharded_fit_mean_weights: a basis must be set (clr_sharded_set_mean_basis), min_pivot finite and in [0, 1)";
  return on_slices(h, K > 0 && std::isfinite(min_pivot) && min_pivot >= 0.0 && min_pivot < 1.0, [=](clr_batch* p, long lo) {
    return clr_batch_fit_mean_weights(p, min_pivot, at(w_hat, lo * K), at(cov, lo * K * K), at(gram, lo * K1 * K1),
                                      at(quad_profiled, lo), at(logdet_gram, lo), at(status, lo));
  });
}

/* ---- coefficients from kernel parameters: clr_batch_set_kernel / _evaluate_params / _grad_params over the shards ---- */
int clr_sharded_set_kernel(clr_sharded* h, const clr_kernel* k) {
  const int st = resolve_all(h);
  if (st != CLR_OK) return st;
  h->n_params = 0;
  if (k && clr_kernel_get_shape(k, &h->n_params, nullptr, nullptr) != CLR_OK) return CLR_INVALID_ARGUMENT;
  return h->all([=](int s) { return clr_batch_set_kernel(h->plan[s], k); });
}

int clr_sharded_evaluate_params(clr_sharded* h, const double* params, const double* mean, long mean_stride,
                                double* loglike, double* logdet, double* quad, int* status) {
  int st = mean ? clr_sharded_set_mean(h, mean, mean_stride) : resolve_all(h);
  if (st != CLR_OK) return st;
  // every shard forms the coefficients of its slice on its device; the largest frequency and decay rate of the WHOLE
  // batch then go to every shard, as clr_sharded_set_coefficients hands them out from the host tables
  const long P = h->n_params;
  st = h->all([=](int s) { return clr_batch_set_parameters(h->plan[s], params ? params + h->lo[s] * P : nullptr); });
  if (st != CLR_OK) return st;
  spread_maxima(h, false);
  reselect_all(h);
  return evaluate_rounds(h, 0, [=](int s) {
    const long lo = h->lo[s];
    const int r = slice_results(h, s, loglike, logdet, quad, status);
    if (r == CLR_OK) clr_group::mark_refused(h->plan[s], at(loglike, lo), at(logdet, lo), at(quad, lo), at(status, lo));
    return r;
  });
}

int clr_sharded_grad_params(clr_sharded* h, double* value, double* grad_params, int* status, int with_mean) {
  const long ncol = h->n_params + (with_mean ? 1 : 0);
  const int st0 = resolve_all(h);
  if (st0 != CLR_OK) return st0;
  return h->all([=](int s) {
    const long lo = h->lo[s];
    return clr_batch_grad_params(h->plan[s], value ? value + lo : nullptr, grad_params ? grad_params + lo * ncol : nullptr,
                                 status ? status + lo : nullptr, with_mean);
  });
}

int clr_sharded_get_coefficients(clr_sharded* h, double* jitter, double* a_real, double* c_real, double* a_comp,
                                 double* b_comp, double* c_comp, double* d_comp) {
  const long JR = h->J_real, JC = h->J_comp;
  const int st0 = resolve_all(h);
  if (st0 != CLR_OK) return st0;
  return h->all([=](int s) {
    const long lo = h->lo[s];
    return clr_batch_get_coefficients(h->plan[s], at(jitter, lo), at(a_real, lo * JR), at(c_real, lo * JR), at(a_comp, lo * JC),
                                      at(b_comp, lo * JC), at(c_comp, lo * JC), at(d_comp, lo * JC));
  });
}

// a materialising evaluation of every shard (clr_batch_enqueue(plan, 1)) settled with the batch-wide counts: what
// clr_sharded_solve / _dot_L / _predict read
int clr_sharded_materialize(clr_sharded* h, double* loglike, double* logdet, double* quad, int* status) {
  const int st0 = resolve_all(h);
  if (st0 != CLR_OK) return st0;
  return evaluate_rounds(h, 1, [=](int s) { return slice_results(h, s, loglike, logdet, quad, status); });
}

int clr_sharded_solve(clr_sharded* h, int nrhs, const double* b, double* x) {
  const long per = (long)nrhs * h->N;
  return on_slices(h, nrhs >= 1 && x, [=](clr_batch* p, long lo) {
    return clr_batch_solve(p, nrhs, b ? b + lo * per : nullptr, x + lo * per);
  });
}

int clr_sharded_dot_L(clr_sharded* h, int nrhs, const double* z, double* y) {
  const long per = (long)nrhs * h->N;
  return on_slices(h, nrhs >= 1 && z && y, [=](clr_batch* p, long lo) {
    return clr_batch_dot_L(p, nrhs, z + lo * per, y + lo * per);
  });
}

int clr_sharded_dot(clr_sharded* h, int nrhs, const double* z, double* y) {
  const long per = (long)nrhs * h->N;
  return on_slices(h, nrhs >= 1 && z && y, [=](clr_batch* p, long lo) {
    return clr_batch_dot(p, nrhs, z + lo * per, y + lo * per);
  });
}

int clr_sharded_predict(clr_sharded* h, int M, const double* xs, long xs_stride, double* pred) {
  return on_slices(h, M >= 0 && (M == 0 || (xs && pred)) && (xs_stride == 0 || xs_stride == M), [=](clr_batch* p, long lo) {
    return clr_batch_predict(p, M, xs + lo * xs_stride, xs_stride, pred + lo * (long)M);
  });
}

int clr_sharded_predict_var(clr_sharded* h, int M, const double* xs, long xs_stride, double* var) {
  return on_slices(h, M >= 0 && (M == 0 || (xs && var)) && (xs_stride == 0 || xs_stride == M), [=](clr_batch* p, long lo) {
    return clr_batch_predict_var(p, M, xs + lo * xs_stride, xs_stride, var + lo * (long)M);
  });
}

int clr_sharded_predict_var_recurrence(clr_sharded* h, int M, const double* xs, long xs_stride, double* var) {
  return on_slices(h, M >= 0 && (M == 0 || (xs && var)) && (xs_stride == 0 || xs_stride == M), [=](clr_batch* p, long lo) {
    return clr_batch_predict_var_recurrence(p, M, xs + lo * xs_stride, xs_stride, var + lo * (long)M);
  });
}

int clr_sharded_leave_one_out(clr_sharded* h, double* kinv_diag, double* alpha, double* loo_logpdf, int* status) {
  const long N = h->N;
  return on_slices(h, kinv_diag || alpha || loo_logpdf || status, [=](clr_batch* p, long lo) {
    return clr_batch_leave_one_out(p, at(kinv_diag, lo * N), at(alpha, lo * N), at(loo_logpdf, lo), at(status, lo));
  });
}

int clr_sharded_one_step_ahead(clr_sharded* h, int nrhs, const double* b, double* innovation, double* variance, int* status) {
  const long N = h->N, per = (long)nrhs * h->N;
  return on_slices(h, nrhs >= 1 && (b || nrhs == 1) && (innovation || variance || status), [=](clr_batch* p, long lo) {
    return clr_batch_one_step_ahead(p, nrhs, b ? b + lo * per : nullptr, at(innovation, lo * per), at(variance, lo * N), at(status, lo));
  });
}

int clr_sharded_forecast(clr_sharded* h, int M, const double* xs, long xs_stride, double* mean, double* var) {
  return on_slices(h, M >= 0 && (M == 0 || (xs && (mean || var))) && (xs_stride == 0 || xs_stride == M), [=](clr_batch* p, long lo) {
    return clr_batch_forecast(p, M, xs + lo * xs_stride, xs_stride, at(mean, lo * (long)M), at(var, lo * (long)M));
  });
}

int clr_sharded_predict_terms(clr_sharded* h, int M, const double* xs, long xs_stride, int G, const unsigned char* groups,
                              double* mean, double* var) {
  const long per = (long)G * M;  // (the groups are the same on every shard)
  return on_slices(h, M >= 0 && (M == 0 || xs) && G >= 1 && groups && (mean || var) && (xs_stride == 0 || xs_stride == M),
                   [=](clr_batch* p, long lo) {
    return clr_batch_predict_terms(p, M, xs + lo * xs_stride, xs_stride, G, groups, at(mean, lo * per), at(var, lo * per));
  });
}

int clr_sharded_predict_cov(clr_sharded* h, int M, const double* xs, long xs_stride, double* cov) {
  const long per = (long)M * M;
  return on_slices(h, M >= 0 && (M == 0 || (xs && cov)) && (xs_stride == 0 || xs_stride == M), [=](clr_batch* p, long lo) {
    return clr_batch_predict_cov(p, M, xs + lo * xs_stride, xs_stride, at(cov, lo * per));
  });
}

int clr_sharded_sample_conditional(clr_sharded* h, int M, const double* xs, long xs_stride, int size, const double* normals,
                                   double regularize, double min_pivot, double* draws, int* status) {
  const long per = (long)size * M;
  return on_slices(h, M >= 0 && size >= 1 && (M == 0 || (xs && normals && draws)) && (xs_stride == 0 || xs_stride == M) &&
                          std::isfinite(min_pivot) && min_pivot >= 0.0 && min_pivot < 1.0 && std::isfinite(regularize) && regularize >= 0.0,
                   [=](clr_batch* p, long lo) {
    return clr_batch_sample_conditional(p, M, xs + lo * xs_stride, xs_stride, size, at(normals, lo * per), regularize, min_pivot,
                                        at(draws, lo * per), at(status, lo));
  });
}

int clr_sharded_set_conditional_tile(clr_sharded* h, int problems) {
  for (clr_batch* p : h->plan) clr_batch_set_conditional_tile(p, problems);
  return CLR_OK;
}

// clr_batch_periodogram, every shard on its slice (a (problem, frequency)'s result does not depend on the sharding); the
// other arguments are checked by the shards
int clr_sharded_periodogram(clr_sharded* h, int F, const double* omega, long omega_stride, double t_ref, int offset,
                            double min_pivot, double* power, double* coef, double* cov, double* gram, int* status) {
  const long Ff = F, K = offset ? 3 : 2, K1 = K + 1;
  g_sharded_error = "clr_sharded_periodogram: F >= 0, the frequencies with stride 0 or F, and at least one output array";
  return on_slices(h, F >= 0 && (F == 0 || omega) && (omega_stride == 0 || omega_stride == F) && (power || coef || cov || gram || status),
                   [=](clr_batch* p, long lo) {
    return clr_batch_periodogram(p, F, omega ? omega + lo * omega_stride : nullptr, omega_stride, t_ref, offset, min_pivot,
                                 at(power, lo * Ff), at(coef, lo * Ff * K), at(cov, lo * Ff * K * K), at(gram, lo * Ff * K1 * K1),
                                 at(status, lo * Ff));
  });
}

int clr_sharded_set_periodogram_tile(clr_sharded* h, int frequencies) {
  for (clr_batch* p : h->plan) clr_batch_set_periodogram_tile(p, frequencies);
  return CLR_OK;
}

// the scan's device time: the largest over the shards, which run concurrently
int clr_sharded_get_periodogram_ms(const clr_sharded* h, double* device_ms) {
  double m = 0.0;
  for (clr_batch* p : h->plan) {
    double v = 0.0;
    (void)clr_batch_get_periodogram_ms(p, &v);
    m = std::max(m, v);
  }
  if (device_ms) *device_ms = m;
  return CLR_OK;
}

int clr_sharded_run_timed(clr_sharded* h, int steps, double* shard_ms /* [nshards] or NULL */) {
  // (a timing tool: every shard times its own steps and settles them by its own counts)
  const int st0 = resolve_all(h);
  if (st0 != CLR_OK) return st0;
  return h->all([=](int s) {
    double total = 0.0, k[6];
    const int st = clr_batch_run_timed(h->plan[s], 0, steps, 0, &total, k);
    if (shard_ms) shard_ms[s] = total;
    return st;
  });
}

int clr_batch_log_likelihood_sharded(int B, int N, int J_real, int J_comp, const double* jitter,
                                     const double* a_real, const double* c_real, const double* a_comp,
                                     const double* b_comp, const double* c_comp, const double* d_comp,
                                     const double* t, long t_stride, const double* diag, long diag_stride,
                                     const double* y, long y_stride, double* loglike, double* logdet,
                                     double* quad, int* status, const int* devices, int ndevices) {
  clr_sharded* h = clr_sharded_create(B, N, J_real, J_comp, devices, ndevices);
  if (!h) return clr_device_count() > 0 ? CLR_INVALID_ARGUMENT : CLR_NO_DEVICE;
  int st = clr_sharded_set_series(h, t, t_stride, diag, diag_stride, y, y_stride);
  if (st == CLR_OK)
    st = clr_sharded_evaluate(h, jitter, a_real, c_real, a_comp, b_comp, c_comp, d_comp, loglike, logdet,
                              quad, status);
  const std::string keep = g_sharded_error;
  clr_sharded_destroy(h);
  g_sharded_error = keep;
  return st;
}

}  // extern "C"
