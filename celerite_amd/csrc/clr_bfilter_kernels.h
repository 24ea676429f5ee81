// celerite_amd/csrc/clr_bfilter_kernels.h -- the causal half of a plan's materialised factor: the one-step-ahead residuals
// (innovations) z = L^-1 r of every problem, and the mean and variance of the process at a point x given only the samples
// strictly before x, in O((N + M) J^2).
//
// Slot notation of clr_bsolve_kernels.h / clr_bpredvar_rec_kernels.h (slot n: phi[n] the decay n -> n+1, u[n], W[n], D[n];
// u(x) the reference's feature row at a point x, c the rows' decay rates).  Two forward recurrences the code already runs:
//     z_n = r_n - u[n] . g_n ,  g+_n = g_n + W[n] z_n ,  g_{n+1} = phi[n] o g+_n ,  g_0 = 0   (the solve's forward sweep,
//                                                                                             before its division by D)
//     S+_n = S_n + D_n W_n W_n^T ,  S_{n+1} = Phi_n S+_n Phi_n ,  S_0 = 0                     (the factorisation's state)
// One step ahead, at the samples: E[y_n | y_<n] = y_n - z_n with variance D_n.  At a point x with m = #{n : t_n < x}:
//     psi = exp(-c (x - t_{m-1})) ,  w = psi o u(x)
//     mean(x) = w^T g+_{m-1} ,  var(x) = k(0) - w^T S+_{m-1} w                               (m = 0: mean 0, var k(0))
// -- w^T S+ w is the term `left` of the recurrence variance, the share of k(0) the past explains; the mean is the same
// projection of the solve's forward state.  Strict <: a point at x = t_n reproduces the one-step-ahead prediction of
// sample n.  Passes:
//   0. bfilter_features_kernel       u(x) of every point of the tile (the only trigonometry of the points);
//   1. bsolve_summarize_kernel, bsolve_prefix_kernel<false> (unchanged): the chunks' start states of g -- they depend on
//      the right-hand side and are formed by every call; the chunk maps beside them once per factor;
//   2. bpvrec_forward_kernel<false>, bpvrec_walk_kernel (unchanged, VAR only): the chunks' start states of S, once per factor;
//   3. bfilter_forward_kernel        per chunk from its start state(s), carrying g (and S): z of every sample, mean and
//                                    var of every point the lane owns.
// Lane = (problem, chunk).  The tile's points are sorted per problem; chunk c owns the points with
// t_{lo_c} < x <= t_{lo_{c+1}} -- the gaps m in (lo_c, lo_{c+1}] --, chunk 0 also everything up to t_0 (m = 0), the last
// chunk everything beyond its first sample.  A lane finds its range by binary search of its two boundary times in the
// sorted points and moves a cursor as it walks: no atomics.  A point's result is a function of its gap's g+, S+, the gap's
// time and the point: its exponentials are the library's, so it does not depend on the tile, the batch or the sharding.
#pragma once

namespace clr {

struct BFilterParams {
  int nrhs;             // right-hand sides of the call (grid.z of the forward kernel)
  int lean;             // the factor holds W, D only
  int have_M, have_S;   // the chunk maps / the chunks' forward start states of S of this factor are formed
  int have_g;           // the chunks' start states of g of this call's right-hand sides are formed (an earlier tile)
  const double* xT;     // [B][nrhs][L][nchunk] right-hand sides
  double* zT;           // the innovations, laid out like xT (may be xT itself); null: not written
  double* M;            // [B][nchunk][J*J]
  double* off;          // [B][nrhs][nchunk][J] forward chunk offsets
  double* starts;       // [B][nrhs][nchunk][J] forward chunk start states of g
  double* S;            // [B][nchunk][J (J + 1) / 2] forward chunk start states of S (VAR)
  const double* t;      // the plan's times, row-major [problem][n] (the S walk's chunk boundaries)
  long t_stride;
  int npts;             // points of this tile (POINTS)
  const double* xs;     // the tile's points, ascending: point r of problem b at xs[b * xs_stride + r] (xs_stride 0: shared)
  long xs_stride;
  double* ux;           // [B][npts][J] u(x)
  double* mean;         // point r of problem b -> mean[b * out_stride + r]; null: not asked for
  double* var;          // ... var[b * out_stride + r] (VAR)
  long out_stride;
};

// first index r in [0, n) with !(x[r] <= T) (NaN points count as +inf: they sort last)
__device__ __forceinline__ int bfilter_upper_bound(const double* x, int n, double T) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (x[mid] <= T) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// 0. one thread per (problem, point)
template <int JR, int JC, bool FAST>
__global__ void __launch_bounds__(256) bfilter_features_kernel(const BatchParams P, const BFilterParams S) {
  constexpr int J = JR + 2 * JC;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)P.B * S.npts) return;
  const int b = (int)(idx / S.npts), r = (int)(idx % S.npts);
  Problem<JR, JC> p;
  load_problem<JR, JC>(P, b, p);
  double uu[J], vv[J];
  features_uv<JR, JC, FAST>(p, S.xs[(long)b * S.xs_stride + r], uu, vv);
#pragma unroll
  for (int j = 0; j < J; ++j) S.ux[idx * J + j] = uu[j];
}

// 3. the forward recurrence per chunk from its start state(s); right-hand side blockIdx.z
template <int JR, int JC, bool LEAN, bool FAST, bool POINTS, bool VAR>
__global__ void __launch_bounds__(64) bfilter_forward_kernel(const BatchParams P, const BFilterParams S) {
  constexpr int J = JR + 2 * JC, NS = J * (J + 1) / 2;
  const int b = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.z;
  if (c >= P.nchunk) return;
  const auto F = make_slots<JR, JC, LEAN, FAST>(P, b, c);
  const long cells = (long)P.L * P.nchunk;
  const double* x = S.xT + ((long)b * S.nrhs + r) * cells + c;
  double* z = S.zT ? S.zT + ((long)b * S.nrhs + r) * cells + c : nullptr;
  const double* st = S.starts + (((long)b * S.nrhs + r) * P.nchunk + c) * J;
  double g[J], Sm[VAR ? NS : 1];
#pragma unroll
  for (int j = 0; j < J; ++j) g[j] = st[j];
  if (VAR) {
    const double* ss = S.S + ((long)b * P.nchunk + c) * NS;
#pragma unroll
    for (int k = 0; k < NS; ++k) Sm[k] = ss[k];
  }
  const int n0 = c * P.L;
  const int last = (P.N - n0 < P.L) ? P.N - n0 : P.L;  // samples of this chunk inside the series
  // the lane's points [cur, end)
  DirectSeries ts;
  Problem<JR, JC> p;
  const double* xp = nullptr;
  long row = 0;
  double k0 = 0.0;
  int cur = 0, end = 0;
  if (POINTS) {
    ts = bpvrec_times(P, b, c);
    load_problem<JR, JC>(P, b, p);
    k0 = p.sum_ar + p.sum_ac;
    xp = S.xs + (long)b * S.xs_stride;
    row = (long)b * S.npts;
    cur = (c == 0) ? 0 : bfilter_upper_bound(xp, S.npts, ts.t(0));
    end = (c == P.nchunk - 1) ? S.npts : bfilter_upper_bound(xp, S.npts, ts.t(P.L));
    if (c == 0) {  // no sample before the point: the prior
      const double t0 = ts.t(0);
      while (cur < end && xp[cur] <= t0) {
        if (S.mean) S.mean[(long)b * S.out_stride + cur] = 0.0;
        if (VAR) S.var[(long)b * S.out_stride + cur] = k0;
        ++cur;
      }
    }
  }
  double nph[J], nuu[J], nww[J], nd, nb;
  F.get(0, nph, nuu, nww, &nd);
  nb = x[0];
  for (int i = 0; i < last; ++i) {
    const int n = n0 + i;
    double ph[J], uu[J], ww[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { ph[j] = nph[j]; uu[j] = nuu[j]; ww[j] = nww[j]; }
    const double d = nd, bn = nb;
    if (i + 1 < last) {  // (the next step's slot, one step ahead)
      F.get(i + 1, nph, nuu, nww, &nd);
      nb = x[(long)(i + 1) * P.nchunk];
    }
    double ug = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) ug = fma(uu[j], g[j], ug);
    const double zn = bn - ug;
    if (z) z[(long)i * P.nchunk] = zn;
    // g+ = g + W z ;  S+ = S + D W W^T
#pragma unroll
    for (int j = 0; j < J; ++j) g[j] = fma(ww[j], zn, g[j]);
    if (VAR) {
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const double dw = d * ww[j];
#pragma unroll
        for (int k = j; k < J; ++k) Sm[sym_index<J>(j, k)] = fma(dw, ww[k], Sm[sym_index<J>(j, k)]);
      }
    }
    const bool tail = (n == P.N - 1);  // the last sample: no successor, its gap reaches to +inf
    if (POINTS) {
      const double tn = ts.t(i);
      const double tnext = tail ? 0.0 : ts.t(i + 1);
      while (cur < end && (tail || xp[cur] <= tnext)) {
        double psi[J], w[J];
        bpvrec_decay<JR, JC>(p, xp[cur] - tn, psi);
        const double* up = S.ux + (row + cur) * J;
#pragma unroll
        for (int j = 0; j < J; ++j) w[j] = psi[j] * up[j];
        if (S.mean) {
          double mu = 0.0;
#pragma unroll
          for (int j = 0; j < J; ++j) mu = fma(w[j], g[j], mu);
          S.mean[(long)b * S.out_stride + cur] = mu;
        }
        if (VAR) {
          double lf = 0.0;
#pragma unroll
          for (int j = 0; j < J; ++j) {
            double sw = 0.0;
#pragma unroll
            for (int k = 0; k < J; ++k) sw = fma(Sm[sym_at<J>(j, k)], w[k], sw);
            lf = fma(w[j], sw, lf);
          }
          S.var[(long)b * S.out_stride + cur] = k0 - lf;
        }
        ++cur;
      }
    }
    if (tail) break;
#pragma unroll
    for (int j = 0; j < J; ++j) g[j] = ph[j] * g[j];
    if (VAR) {
#pragma unroll
      for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int k = j; k < J; ++k) Sm[sym_index<J>(j, k)] = (ph[j] * ph[k]) * Sm[sym_index<J>(j, k)];
      }
    }
  }
}

}  // namespace clr
