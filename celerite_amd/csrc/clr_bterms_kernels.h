// celerite_amd/csrc/clr_bterms_kernels.h -- component separation on a plan's materialised factor: the posterior mean and
// variance of the process of a GROUP of kernel terms, E[f_g(x) | y] = k_g*^T K^-1 r and
// Var[f_g(x) | y] = k_g(0) - k_g*^T K^-1 k_g*, for every problem, any number of groups and M points each in
// O((N + G M) J^2): one forward and one backward pass over the series whatever the number of groups.
//
// Slot notation of clr_bpredvar_rec_kernels.h (slot n: phi[n] the decay n -> n+1, u[n], W[n], D[n]; u(x), v(x) the feature
// rows at a point, c the rows' decay rates, m = #{n : t_n <= x}).  A group g is a 0/1 vector over the coefficient terms
// (real terms first, then the complex ones), mask_g that vector spread over the rows -- a complex term owns its cos and
// its sin row --, u_g = mask_g o u(x), v_g = mask_g o v(x), k_g(0) = sum_{j in g} a_j.  The cross-covariance of the group
// with the samples is k_g(x - t_n) = (psi o u_g(x)) . v(t_n) below the point and (psi' o v_g(x)) . u(t_n) above it, so
// the group enters through the point's own rows alone and the states over the series are those of the full kernel:
//     S+_n, Q_n                                               the factor's (clr_bpredvar_rec_kernels.h; pv_S, loo_Q)
//     p+_n = phi_{n-1} o p+_{n-1} + v(t_n) alpha_n            forward,  alpha = K^-1 r
//     b_n  = phi_n o b_{n+1} + u(t_n) alpha_n ,  b_N = 0      backward
// and with psi = exp(-c (x - t_{m-1})), psi' = exp(-c (t_m - x)), w = psi o u_g(x):
//     mean_g = w^T p+_{m-1} + (psi' o v_g(x))^T b_m                          (m = 0: first term 0; m = N: second term 0)
//     left   = w^T S+_{m-1} w ,  e = v_g(x) - psi o (S+_{m-1} w) ,  e' = psi' o e
//     var_g  = k_g(0) - left - e'^T Q_m e'                                   (m = 0: left = 0, e = v_g; m = N: last term 0)
// p and b are the two diagonal recurrences of K z (clr_bdot_kernels.h: its PASS 1 state is phi o p+, its PASS 0 state is
// b) run on z = alpha: their chunk offsets and walks ARE bdot_kernel<.., false> and bdot_prefix_kernel, unchanged.  They
// need nothing of the factor -- v(t_n), u(t_n) and phi are regenerated from the times and the coefficients as that file
// does -- so the mean has replays of its own (J doubles of state, no factor traffic) and the variance replays carry S or
// Q alone, at the register count of the recurrence variance: no instantiation carries p beside S.  Passes per tile:
//   0. bpvrec_features_kernel (unchanged)   u(x), v(x) of every point: the only trigonometry of the points, once per
//                                           point whatever the number of groups;
//   1. bdot_kernel<0 / 1, false>, bdot_prefix_kernel<0 / 1> (unchanged; the first tile of a call): start states of b, p;
//   2. bterms_mean_forward_kernel           per chunk carrying p+: the forward half of every (point, group)'s mean; points
//                                           from t_{N-1} on are finished here;
//      bterms_mean_backward_kernel          per chunk carrying b: adds the backward half;
//   3. the start states of S and Q by the passes of clr_bpredvar_rec_kernels.h / clr_binvdiag_kernels.h, unless formed;
//   4. bterms_var_forward_kernel            per chunk carrying S: left and e' of every (point, group) -- it knows both
//                                           times of the gap, so the backward kernel evaluates no exponential;
//      bterms_var_backward_kernel           per chunk carrying Q: the variances.
// Lane = (problem, chunk); the ownership of the sorted points, the binary searches and the cursors are those of
// bpvrec_forward_kernel / bpvrec_backward_kernel: no atomics.  The masks are applied after the features, by selection:
// the empty group gives exactly 0.  The exponentials of the points are the library's, so a point's bits depend on
// neither the tile, the batch nor the sharding.
#pragma once

namespace clr {

struct BTermsParams {
  int npts;                 // points of this tile
  int G;                    // groups
  int lean;                 // the factor holds W, D only
  int have_pb;              // the chunks' start states of p and b of this call are formed (an earlier tile)
  int have_S, have_Q;       // the chunks' start states of S / start matrices Q of this factor are formed
  const double* xs;         // the tile's points, ascending: point r of problem b at xs[b * xs_stride + r] (xs_stride 0: shared)
  long xs_stride;
  const unsigned* rowmask;  // [G] bit j: row j belongs to the group
  const double* aT;         // [B][L][nchunk] alpha = K^-1 r, chunk-interleaved
  BDotParams pb;            // pass 1: zT = aT, the decay products and offsets; pb.starts is overwritten per pass
  double* pstart;           // [B][nchunk][J] phi o p+ entering every chunk
  double* bstart;           // [B][nchunk][J] b entering every chunk from above
  const double* t;          // the plan's times, row-major [problem][n] (the S walk's chunk boundaries)
  long t_stride;
  double* S;                // [B][nchunk][J (J + 1) / 2] forward chunk start states of S
  BInvDiagParams Q;         // pass 3: Q.Q the backward start matrices
  double* ux;               // [B][npts][J] u(x)
  double* vx;               // [B][npts][J] v(x)
  double* e;                // [B][npts][G][J] e' = psi' o e
  double* left;             // [B][npts][G]
  double* mean;             // point r of group g of problem b -> mean[(b * G + g) * out_stride + r]; null: not asked for
  double* var;              // ... var[(b * G + g) * out_stride + r]; null: not asked for
  long out_stride;
};

// k_g(0): the amplitudes of the group's terms, in coefficient order
template <int JR, int JC>
__device__ __forceinline__ double bterms_k0(const Problem<JR, JC>& p, unsigned m) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < JR; ++j) s += ((m >> j) & 1u) ? p.ar[j] : 0.0;
#pragma unroll
  for (int j = 0; j < JC; ++j) s += ((m >> (JR + 2 * j)) & 1u) ? p.ac[j] : 0.0;
  return s;
}

// sum_{j in g} a_j b_j, rows ascending
template <int J>
__device__ __forceinline__ double bterms_masked_dot(unsigned m, const double* a, const double* b) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < J; ++j) s = ((m >> j) & 1u) ? fma(a[j], b[j], s) : s;
  return s;
}

// pass 2, forward: the state of bdot_kernel<.., 1, ..> on alpha, the points of every gap served on the way up
template <int JR, int JC, bool FAST>
__global__ void __launch_bounds__(64) bterms_mean_forward_kernel(const BatchParams P, const BTermsParams S) {
  constexpr int J = JR + 2 * JC;
  const int b = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x;
  if (c >= P.nchunk) return;
  Problem<JR, JC> p;
  load_problem<JR, JC>(P, b, p);
  const DirectSeries ts = bpvrec_times(P, b, c);
  const double* al = S.aT + (long)b * P.L * P.nchunk + c;
  const double* st = S.pstart + ((long)b * P.nchunk + c) * J;
  double g[J];
#pragma unroll
  for (int j = 0; j < J; ++j) g[j] = st[j];
  const int n0 = c * P.L;
  const int last = (P.N - n0 < P.L) ? P.N - n0 : P.L;  // samples of this chunk inside the series (>= 1)
  // the lane's points [cur, end)
  const double* xp = S.xs + (long)b * S.xs_stride;
  const long row = (long)b * S.npts;
  double* out = S.mean + (long)b * S.G * S.out_stride;
  int cur = (c == 0) ? 0 : bpvrec_lower_bound(xp, S.npts, ts.t(0));
  const int end = (c == P.nchunk - 1) ? S.npts : bpvrec_lower_bound(xp, S.npts, ts.t(P.L));
  if (c == 0) {  // before the first sample: no forward half
    const double t0 = ts.t(0);
    while (cur < end && xp[cur] < t0) {
      for (int q = 0; q < S.G; ++q) out[q * S.out_stride + cur] = 0.0;
      ++cur;
    }
  }
  for (int i = 0; i < last; ++i) {
    const int n = n0 + i;
    const double tn = ts.t(i), an = al[(long)i * P.nchunk];
    double uu[J], vv[J];
    features_uv<JR, JC, FAST>(p, tn, uu, vv);
#pragma unroll
    for (int j = 0; j < J; ++j) g[j] = fma(vv[j], an, g[j]);  // p+_n
    const bool tail = (n == P.N - 1);  // the last sample: no successor, its gap reaches to +inf
    const double tnext = tail ? 0.0 : ts.t(i + 1);
    while (cur < end && (tail || xp[cur] < tnext)) {
      double psi[J], w[J];
      bpvrec_decay<JR, JC>(p, xp[cur] - tn, psi);
      const double* up = S.ux + (row + cur) * J;
#pragma unroll
      for (int j = 0; j < J; ++j) w[j] = psi[j] * up[j];
      for (int q = 0; q < S.G; ++q) out[q * S.out_stride + cur] = bterms_masked_dot<J>(S.rowmask[q], w, g);
      ++cur;
    }
    if (tail) break;
    double phid[nz(JR + JC)];
    features_phi_distinct<JR, JC>(p, tnext - tn, phid);
#pragma unroll
    for (int j = 0; j < J; ++j) g[j] = phid[phi_index<JR>(j)] * g[j];
  }
}

// pass 2, backward: the state of bdot_kernel<.., 0, ..> on alpha, the points of every gap served on the way down
template <int JR, int JC, bool FAST>
__global__ void __launch_bounds__(64) bterms_mean_backward_kernel(const BatchParams P, const BTermsParams S) {
  constexpr int J = JR + 2 * JC;
  const int b = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x;
  if (c >= P.nchunk) return;
  Problem<JR, JC> p;
  load_problem<JR, JC>(P, b, p);
  const DirectSeries ts = bpvrec_times(P, b, c);
  const double* al = S.aT + (long)b * P.L * P.nchunk + c;
  const double* st = S.bstart + ((long)b * P.nchunk + c) * J;
  double k[J];
#pragma unroll
  for (int j = 0; j < J; ++j) k[j] = st[j];
  const int n0 = c * P.L;
  const int last = (P.N - n0 < P.L) ? P.N - n0 : P.L;
  const double* xp = S.xs + (long)b * S.xs_stride;
  const long row = (long)b * S.npts;
  double* out = S.mean + (long)b * S.G * S.out_stride;
  const int lo = (c == 0) ? 0 : bpvrec_lower_bound(xp, S.npts, ts.t(0));
  int cur = (c == P.nchunk - 1) ? S.npts : bpvrec_lower_bound(xp, S.npts, ts.t(P.L));
  // the backward half of point r in the gap below the sample at time tm, k = b_m
  auto serve = [&](int r, double tm) {
    double dec[J], w[J];
    bpvrec_decay<JR, JC>(p, tm - xp[r], dec);
    const double* vp = S.vx + (row + r) * J;
#pragma unroll
    for (int j = 0; j < J; ++j) w[j] = dec[j] * vp[j];
    for (int q = 0; q < S.G; ++q) out[q * S.out_stride + r] += bterms_masked_dot<J>(S.rowmask[q], w, k);
  };
  for (int i = last - 1; i >= 0; --i) {
    const int n = n0 + i;
    const double tn = ts.t(i), an = al[(long)i * P.nchunk];
    double uu[J], vv[J];
    features_uv<JR, JC, FAST>(p, tn, uu, vv);
    if (n == P.N - 1) {  // the last sample: the gap above it is the forward kernel's; b_{N-1} = u alpha
      while (cur > lo && !(xp[cur - 1] < tn)) --cur;
#pragma unroll
      for (int j = 0; j < J; ++j) k[j] = uu[j] * an;
      continue;
    }
    const double tm = ts.t(i + 1);
    while (cur > lo && !(xp[cur - 1] < tn)) { --cur; serve(cur, tm); }  // the gap m = n + 1: k = b_{n+1}
    double phid[nz(JR + JC)];
    features_phi_distinct<JR, JC>(p, tm - tn, phid);
#pragma unroll
    for (int j = 0; j < J; ++j) k[j] = fma(uu[j], an, phid[phi_index<JR>(j)] * k[j]);
  }
  if (c == 0) {  // before the first sample: m = 0, k = b_0
    const double t0 = ts.t(0);
    while (cur > 0) { --cur; serve(cur, t0); }
  }
}

// pass 4, forward: bpvrec_forward_kernel<.., true> with the groups' masks on the point's rows
template <int JR, int JC, bool LEAN, bool FAST>
__global__ void __launch_bounds__(64) bterms_var_forward_kernel(const BatchParams P, const BTermsParams S) {
  constexpr int J = JR + 2 * JC, NS = J * (J + 1) / 2;
  const int b = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x;
  if (c >= P.nchunk) return;
  const auto F = make_slots<JR, JC, LEAN, FAST>(P, b, c);
  const DirectSeries ts = bpvrec_times(P, b, c);
  Problem<JR, JC> p;
  load_problem<JR, JC>(P, b, p);
  const double* ss = S.S + ((long)b * P.nchunk + c) * NS;
  double Sm[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) Sm[k] = ss[k];
  const int n0 = c * P.L;
  const int last = (P.N - n0 < P.L) ? P.N - n0 : P.L;  // samples of this chunk inside the series
  // the lane's points [cur, end)
  const double* xp = S.xs + (long)b * S.xs_stride;
  const long row = (long)b * S.npts;
  double* out = S.var + (long)b * S.G * S.out_stride;
  int cur = (c == 0) ? 0 : bpvrec_lower_bound(xp, S.npts, ts.t(0));
  const int end = (c == P.nchunk - 1) ? S.npts : bpvrec_lower_bound(xp, S.npts, ts.t(P.L));
  if (c == 0) {  // before the first sample: left = 0, e = v_g(x), the gap's upper sample is t_0
    const double t0 = ts.t(0);
    while (cur < end && xp[cur] < t0) {
      double psip[J];
      bpvrec_decay<JR, JC>(p, t0 - xp[cur], psip);
      const double* vp = S.vx + (row + cur) * J;
      for (int q = 0; q < S.G; ++q) {
        const unsigned m = S.rowmask[q];
        double* ep = S.e + ((row + cur) * S.G + q) * J;
#pragma unroll
        for (int j = 0; j < J; ++j) ep[j] = ((m >> j) & 1u) ? psip[j] * vp[j] : 0.0;
        S.left[(row + cur) * S.G + q] = 0.0;
      }
      ++cur;
    }
  }
  double nph[J], nuu[J], nww[J], nd;
  F.get(0, nph, nuu, nww, &nd);
  for (int i = 0; i < last; ++i) {
    const int n = n0 + i;
    double ph[J], ww[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { ph[j] = nph[j]; ww[j] = nww[j]; }
    const double d = nd;
    if (i + 1 < last) F.get(i + 1, nph, nuu, nww, &nd);  // (the next step's slot, one step ahead)
    // S+ = S + D W W^T
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const double dw = d * ww[j];
#pragma unroll
      for (int k = j; k < J; ++k) Sm[sym_index<J>(j, k)] = fma(dw, ww[k], Sm[sym_index<J>(j, k)]);
    }
    const bool tail = (n == P.N - 1);  // the last sample: no successor, its gap reaches to +inf
    const double tn = ts.t(i);
    const double tnext = tail ? 0.0 : ts.t(i + 1);
    while (cur < end && (tail || xp[cur] < tnext)) {
      double psi[J], psip[J];
      bpvrec_decay<JR, JC>(p, xp[cur] - tn, psi);
      if (!tail) bpvrec_decay<JR, JC>(p, tnext - xp[cur], psip);  // (tail: finished here, e' is never read)
      const double* up = S.ux + (row + cur) * J;
      const double* vp = S.vx + (row + cur) * J;
      for (int q = 0; q < S.G; ++q) {
        const unsigned m = S.rowmask[q];
        double w[J], ee[J], lf = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) w[j] = ((m >> j) & 1u) ? psi[j] * up[j] : 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) {
          double sw = 0.0;
#pragma unroll
          for (int k = 0; k < J; ++k) sw = fma(Sm[sym_at<J>(j, k)], w[k], sw);
          lf = fma(w[j], sw, lf);
          ee[j] = (((m >> j) & 1u) ? vp[j] : 0.0) - psi[j] * sw;
        }
        if (tail) { out[q * S.out_stride + cur] = bterms_k0<JR, JC>(p, m) - lf; continue; }
        double* ep = S.e + ((row + cur) * S.G + q) * J;
#pragma unroll
        for (int j = 0; j < J; ++j) ep[j] = psip[j] * ee[j];
        S.left[(row + cur) * S.G + q] = lf;
      }
      ++cur;
    }
    if (tail) break;
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
      for (int k = j; k < J; ++k) Sm[sym_index<J>(j, k)] = (ph[j] * ph[k]) * Sm[sym_index<J>(j, k)];
    }
  }
}

// pass 4, backward: bpvrec_backward_kernel with one e' per (point, group), already decayed, and the group's own k(0)
template <int JR, int JC, bool LEAN, bool FAST>
__global__ void __launch_bounds__(64) bterms_var_backward_kernel(const BatchParams P, const BTermsParams S) {
  constexpr int J = JR + 2 * JC, NS = J * (J + 1) / 2;
  const int b = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x;
  if (c >= P.nchunk) return;
  const auto F = make_slots<JR, JC, LEAN, FAST>(P, b, c);
  const DirectSeries ts = bpvrec_times(P, b, c);
  Problem<JR, JC> p;
  load_problem<JR, JC>(P, b, p);
  const double* qs = S.Q.Q + ((long)b * P.nchunk + c) * NS;
  double Q[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) Q[k] = qs[k];
  const int n0 = c * P.L;
  const int last = (P.N - n0 < P.L) ? P.N - n0 : P.L;
  const double* xp = S.xs + (long)b * S.xs_stride;
  const long row = (long)b * S.npts;
  double* out = S.var + (long)b * S.G * S.out_stride;
  const int lo = (c == 0) ? 0 : bpvrec_lower_bound(xp, S.npts, ts.t(0));
  int cur = (c == P.nchunk - 1) ? S.npts : bpvrec_lower_bound(xp, S.npts, ts.t(P.L));
  // the variances of point r in the gap below sample m, Q = Q_m (e' as the forward kernel left it)
  auto serve = [&](int r) {
    for (int q = 0; q < S.G; ++q) {
      double ep[J], quad = 0.0;
      const double* ee = S.e + ((row + r) * S.G + q) * J;
#pragma unroll
      for (int j = 0; j < J; ++j) ep[j] = ee[j];
#pragma unroll
      for (int j = 0; j < J; ++j) {
        double qe = 0.0;
#pragma unroll
        for (int k = 0; k < J; ++k) qe = fma(Q[sym_at<J>(j, k)], ep[k], qe);
        quad = fma(ep[j], qe, quad);
      }
      out[q * S.out_stride + r] = (bterms_k0<JR, JC>(p, S.rowmask[q]) - S.left[(row + r) * S.G + q]) - quad;
    }
  };
  double nph[J], nuu[J], nww[J], nd;
  F.get(last - 1, nph, nuu, nww, &nd);
  for (int i = last - 1; i >= 0; --i) {
    const int n = n0 + i;
    double ph[J], uu[J], ww[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { ph[j] = nph[j]; uu[j] = nuu[j]; ww[j] = nww[j]; }
    const double rd = 1.0 / nd;
    if (i > 0) F.get(i - 1, nph, nuu, nww, &nd);  // (the previous sample's slot, one step ahead)
    const double tn = ts.t(i);
    if (n == P.N - 1) {  // the last sample: the gap above it is the forward kernel's; its transition is 0
      while (cur > lo && !(xp[cur - 1] < tn)) --cur;
#pragma unroll
      for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int k = j; k < J; ++k) Q[sym_index<J>(j, k)] = rd * uu[j] * uu[k];
      }
      continue;
    }
    while (cur > lo && !(xp[cur - 1] < tn)) { --cur; serve(cur); }  // the gap m = n + 1: t_n <= x < t_{n+1}, Q = Q_{n+1}
    double g[J], v[J], s = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) g[j] = ph[j] * ww[j];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      double qg = 0.0;
#pragma unroll
      for (int k = 0; k < J; ++k) qg = fma(Q[sym_at<J>(j, k)], g[k], qg);
      s = fma(g[j], qg, s);
      v[j] = ph[j] * qg;
    }
    const double cn = rd + s;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const double cu = cn * uu[j];
#pragma unroll
      for (int k = j; k < J; ++k) {
        const double pq = (ph[j] * ph[k]) * Q[sym_index<J>(j, k)];
        Q[sym_index<J>(j, k)] = fma(cu, uu[k], pq - fma(uu[j], v[k], v[j] * uu[k]));
      }
    }
  }
  if (c == 0) {  // before the first sample: m = 0, Q = Q_0
    while (cur > 0) { --cur; serve(cur); }
  }
}

}  // namespace clr
