// celerite_amd/csrc/gram_solve.cpp -- clr_gram_solve: the small solve of clr_batch_fit_mean_weights on the host
// (clr_gram_solve.h: the routine the device runs, one thread per problem; the same bits).  Needs no GPU.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/celerite_hip.h"
#include "clr_gram_solve.h"

extern "C" int clr_gram_solve(int nprob, int K, const double* gram_bordered, const double* w0, double min_pivot,
                              double* w_hat, double* cov, double* quad_profiled, double* logdet_gram, int* status) {
  if (nprob < 0 || K < 1 || K > CLR_MAX_MEAN_BASIS || (nprob > 0 && !gram_bordered)) return CLR_INVALID_ARGUMENT;
  if (!std::isfinite(min_pivot) || min_pivot < 0.0 || min_pivot >= 1.0) return CLR_INVALID_ARGUMENT;
  const size_t k = (size_t)K, k1 = k + 1;
  std::vector<double> work((size_t)clr::gram_solve_work(K)), w(k), c(k * k), zero(k, 0.0);
  for (size_t p = 0; p < (size_t)nprob; ++p) {
    double q, ld;
    const int st = clr::gram_solve(K, gram_bordered + p * k1 * k1, w0 ? w0 + p * k : zero.data(), min_pivot, w.data(), c.data(),
                                   &q, &ld, work.data());
    if (w_hat) std::copy(w.begin(), w.end(), w_hat + p * k);
    if (cov) std::copy(c.begin(), c.end(), cov + p * k * k);
    if (quad_profiled) quad_profiled[p] = q;
    if (logdet_gram) logdet_gram[p] = ld;
    if (status) status[p] = st;
  }
  return CLR_OK;
}
