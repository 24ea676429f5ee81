// celerite_amd/csrc/clr_gram_solve.h
//
// The small solve of a linear mean's generalised-least-squares fit (clr_batch_fit_mean_weights): from the bordered Gram
// matrix of one problem,
//     S = [[G, d], [d^T, q]] ,  G = Phi^T K^-1 Phi ,  d = Phi^T K^-1 r ,  q = r^T K^-1 r   (r at the weights w0 in force),
// the weights w = w0 + G^-1 d, their covariance G^-1, log det G and the profiled quadratic form q - d^T G^-1 d.
//
// The profiled quadratic form is what is left of q once the basis has taken its share -- d^T G^-1 d is most of q when
// the model fits, 1 - 1e-6 of it on a series the basis explains -- so q - d^T delta in working precision would lose to
// cancellation what the small solve got right.  It is evaluated as the quadratic it is the minimum of,
//     q - 2 d^T delta + delta^T G delta = q - d^T delta - delta^T (d - G delta) ,
// whose error is of SECOND order in delta's, with the dot products accumulated in twice the working precision
// (error-free products through fma, error-free sums): the result is good to the rounding of the entries of S.
//
// ONE routine for the device (one thread per problem: mean_kernels.hip) and the host (clr_gram_solve: gram_solve.cpp),
// written so that the two return the same bits: plain products, sums, quotients and square roots, each rounded on its
// own (both units are compiled with contraction off), and a logarithm made of such operations instead of the two
// platforms' library functions.
//
// G is scaled to unit diagonal first, G_s = D^-1/2 G D^-1/2 -- a basis mixes a constant with a template of any
// amplitude, and the scaling takes that out of the pivots -- then factored by an unpivoted Cholesky.  A problem is
// refused (CLR_GRAM_REFUSED: the status CLR_NOT_POSITIVE_DEFINITE) when a diagonal entry of G is not positive and
// finite, or a pivot of G_s is not above zero or lies below min_pivot: w = w0, the other outputs NaN.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CLR_GRAM_HD __host__ __device__
#else
#define CLR_GRAM_HD
#endif

namespace clr {

constexpr int CLR_GRAM_REFUSED = 2;  // CLR_NOT_POSITIVE_DEFINITE of celerite_hip.h

// doubles of `work` gram_solve needs
CLR_GRAM_HD inline long gram_solve_work(int K) { return (long)K * K + 2L * K; }

// log x for a positive finite x: x = 2^e m with m in (sqrt(1/2), sqrt(2)], log m = 2 atanh(s), s = (m - 1) / (m + 1),
// |s| <= 0.1716: the series in s^2 to the term s^24 / 25 (the next is below 2^-62); e log 2 in two parts, the high one
// exact for |e| < 2^11.  A few ulp of max(|log m|, ulp(e log 2)).
CLR_GRAM_HD inline double gram_log(double x) {
  long long bits;
  __builtin_memcpy(&bits, &x, sizeof(bits));
  int e = (int)((bits >> 52) & 0x7ff);
  if (e == 0) {  // subnormal
    x = x * 18014398509481984.0;  // 2^54
    __builtin_memcpy(&bits, &x, sizeof(bits));
    e = (int)((bits >> 52) & 0x7ff) - 54;
  }
  e -= 1023;
  bits = (bits & 0x000fffffffffffffLL) | 0x3ff0000000000000LL;
  double m;
  __builtin_memcpy(&m, &bits, sizeof(m));
  if (m > 1.4142135623730951) {
    m = m * 0.5;
    e += 1;
  }
  const double s = (m - 1.0) / (m + 1.0), z = s * s;
  double p = 1.0 / 25.0;
  p = p * z + 1.0 / 23.0;
  p = p * z + 1.0 / 21.0;
  p = p * z + 1.0 / 19.0;
  p = p * z + 1.0 / 17.0;
  p = p * z + 1.0 / 15.0;
  p = p * z + 1.0 / 13.0;
  p = p * z + 1.0 / 11.0;
  p = p * z + 1.0 / 9.0;
  p = p * z + 1.0 / 7.0;
  p = p * z + 1.0 / 5.0;
  p = p * z + 1.0 / 3.0;
  p = p * z;  // log m = 2 s (1 + p)
  const double two_s = 2.0 * s;
  const double lm = two_s + two_s * p;
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
  const double de = (double)e;
  return de * ln2_hi + (lm + de * ln2_lo);
}

// (hi, lo) += a * b, the product and the sum without error (Ogita, Rump, Oishi: Dot2)
CLR_GRAM_HD inline void gram_dot2(double a, double b, double* hi, double* lo) {
  const double p = a * b, pe = __builtin_fma(a, b, -p);
  const double t = *hi + p, z = t - *hi;
  const double te = (*hi - (t - z)) + (p - z);
  *hi = t;
  *lo = *lo + (te + pe);
}

CLR_GRAM_HD inline double gram_sqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return ::sqrt(x);
#else
  return __builtin_sqrt(x);
#endif
}

// S: the bordered Gram matrix, (K + 1) x (K + 1) row-major (the lower triangle and the border row K are read);
// w0: [K]; outputs w_hat [K], cov [K][K], *quad, *logdet (none null); work: gram_solve_work(K) doubles.
// Returns 0, or CLR_GRAM_REFUSED.
CLR_GRAM_HD inline int gram_solve(int K, const double* S, const double* w0, double min_pivot, double* w_hat, double* cov,
                                  double* quad, double* logdet, double* work) {
  const int K1 = K + 1;
  double* L = work;           // [K][K] the factor of G_s, then its inverse (lower triangles)
  double* s = work + (long)K * K;  // [K] D^-1/2
  double* v = s + K;          // [K] the right-hand side on its way to G_s^-1 D^-1/2 d
  const double nan = __builtin_nan("");
  bool ok = true;
  for (int i = 0; i < K; ++i) {
    const double g = S[i * K1 + i];
    if (!(g > 0.0) || !(g < __builtin_inf())) ok = false;
  }
  double ld = 0.0;
  if (ok) {
    for (int i = 0; i < K; ++i) {
      const double g = S[i * K1 + i];
      s[i] = 1.0 / gram_sqrt(g);
      ld = ld + gram_log(g);
    }
    for (int j = 0; j < K && ok; ++j) {
      double p = 1.0;  // (the scaled diagonal)
      for (int k = 0; k < j; ++k) p = p - L[j * K + k] * L[j * K + k];
      if (!(p > 0.0) || !(p >= min_pivot)) {
        ok = false;
        break;
      }
      const double ljj = gram_sqrt(p);
      L[j * K + j] = ljj;
      ld = ld + 2.0 * gram_log(ljj);
      for (int i = j + 1; i < K; ++i) {
        double a = (S[i * K1 + j] * s[i]) * s[j];
        for (int k = 0; k < j; ++k) a = a - L[i * K + k] * L[j * K + k];
        L[i * K + j] = a / ljj;
      }
    }
  }
  if (!ok) {
    for (int i = 0; i < K; ++i) w_hat[i] = w0[i];
    for (int i = 0; i < K * K; ++i) cov[i] = nan;
    *quad = nan;
    *logdet = nan;
    return CLR_GRAM_REFUSED;
  }
  // L u = D^-1/2 d, L^T v = u, delta = D^-1/2 v
  for (int i = 0; i < K; ++i) {
    double a = S[K * K1 + i] * s[i];
    for (int k = 0; k < i; ++k) a = a - L[i * K + k] * v[k];
    v[i] = a / L[i * K + i];
  }
  for (int i = K - 1; i >= 0; --i) {
    double a = v[i];
    for (int k = i + 1; k < K; ++k) a = a - L[k * K + i] * v[k];
    v[i] = a / L[i * K + i];
  }
  for (int i = 0; i < K; ++i) {
    v[i] = v[i] * s[i];
    w_hat[i] = w0[i] + v[i];
  }
  // q - d^T delta - delta^T rho with rho = d - G delta (see above); (hi, lo) is minus the running value
  double hi = -S[K * K1 + K], lo = 0.0;
  for (int i = 0; i < K; ++i) {
    double gh = 0.0, gl = 0.0;
    for (int j = 0; j < K; ++j) gram_dot2(j <= i ? S[i * K1 + j] : S[j * K1 + i], v[j], &gh, &gl);
    const double d = S[K * K1 + i];
    const double t = d - gh, z = t - d;
    const double rho = t + (((d - (t - z)) + (-gh - z)) - gl);
    gram_dot2(d, v[i], &hi, &lo);
    lo = lo + v[i] * rho;
  }
  *quad = -(hi + lo);
  *logdet = ld;
  // L <- L^-1 in place, column by column (column j needs the later columns and diagonals, still untouched)
  for (int j = 0; j < K; ++j) {
    const double inv = 1.0 / L[j * K + j];
    for (int i = j + 1; i < K; ++i) {
      double a = L[i * K + j] * inv;
      for (int k = j + 1; k < i; ++k) a = a + L[i * K + k] * L[k * K + j];
      L[i * K + j] = -a / L[i * K + i];
    }
    L[j * K + j] = inv;
  }
  // cov = D^-1/2 L^-T L^-1 D^-1/2, the upper triangle mirrored: exactly symmetric
  for (int i = 0; i < K; ++i)
    for (int j = i; j < K; ++j) {
      double a = 0.0;
      for (int k = j; k < K; ++k) a = a + L[k * K + i] * L[k * K + j];
      a = (a * s[i]) * s[j];
      cov[i * K + j] = a;
      cov[j * K + i] = a;
    }
  return 0;
}

}  // namespace clr
