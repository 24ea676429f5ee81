// celerite_amd/csrc/clr_bpredvar_rec_kernels.h -- the conditional variance of GP.predict for every problem of a plan from
// its materialised factor in O((N + M) J^2): one forward and one backward pass over the series plus O(J^2) per point,
// instead of one forward substitution per point (clr_bpredvar_kernels.h, O(M N J)).
//
// Slot notation of clr_bsolve_kernels.h / clr_binvdiag_kernels.h (slot n: phi[n] the decay n -> n+1, u[n], W[n], D[n]);
// v(x) = (1.., cos d x, sin d x), u(x) the reference's feature rows at a point x, c the rows' decay rates.  For a point x
// let m be the number of samples with t_n <= x.  With
//     S+_n = S_n + D_n W_n W_n^T ,  S_{n+1} = Phi_n S+_n Phi_n ,  S_0 = 0      (the factorisation's own state, from W, D)
//     Q_n  = u_n u_n^T / D_n + F_n^T Q_{n+1} F_n ,  Q_N = 0                     (clr_binvdiag_kernels.h)
// the forward substitution z = L^-1 k* has z_n = D_n W_n^T Phi(t_n -> x) u(x) for n < m, and for n >= m the state
// h_n = Phi(x -> t_n) v(x) - g_n obeys the homogeneous h_{n+1} = F_n h_n, z_n = u_n^T h_n.  So
//     psi = exp(-c (x - t_{m-1})) ,  w = psi o u(x) ,  left = w^T S+_{m-1} w            (m = 0: 0)
//     e   = v(x) - psi o (S+_{m-1} w) ,  e' = exp(-c (t_m - x)) o e
//     var(x) = k(0) - left - e'^T Q_m e'                                                 (m = N: the last term is 0)
// The map S -> Phi (S + D W W^T) Phi is a diagonal congruence plus a constant: over a chunk lo .. hi-1,
// S_hi = Psi_c S_lo Psi_c + C_c with Psi_c = exp(-c (t_hi - t_lo)) -- no matrix products in the walk.  Passes:
//   0. bpvrec_features_kernel          u(x), v(x) of every point of the tile (the only trigonometry of the points);
//   1. bpvrec_forward_kernel<false>    per chunk from S = 0: the offset C_c;
//      bpvrec_walk_kernel              one lane per problem over the chunks: start[c] (overwrites C_c);
//   2. binvdiag_kernel<false>, binvdiag_walk_kernel (unchanged): start[c] = Q_{hi_c};
//   3. bpvrec_forward_kernel<true>     per chunk from its start state, carrying S: left and e of every point it owns;
//   4. bpvrec_backward_kernel          per chunk down from Q_{hi_c}, carrying Q: var of every point it owns.
// Passes 1 and 2 depend on the factor only and are skipped while their results are valid (have_S, have_Q).
// Lane = (problem, chunk).  The tile's points are sorted per problem; chunk c owns the points with
// t_{lo_c} <= x < t_{lo_{c+1}} -- the gaps m in (lo_c, lo_{c+1}] --, chunk 0 also everything before t_0 (m = 0, Q_0), the
// last chunk everything from t_{N-1} on (m = N: var = k(0) - left, written by pass 3).  A lane finds its range by binary
// search of its two boundary times in the sorted points and moves a cursor as it walks: no atomics.  A point's result is a
// function of its gap's S+, Q, the gap's two times and the point: the exponentials of the points are the library's (no
// wave-uniform choice of a polynomial), so it does not depend on the tile, the batch or the sharding.
#pragma once

namespace clr {

struct BPredVarRecParams {
  int npts;             // points of this tile
  int lean;             // the factor holds W, D only
  int have_S, have_Q;   // the chunks' forward start states / backward start matrices of this factor are formed
  const double* xs;     // the tile's points, ascending: point r of problem b at xs[b * xs_stride + r] (xs_stride 0: shared)
  long xs_stride;
  const double* t;      // the plan's times, row-major [problem][n] (the walk's chunk boundaries)
  long t_stride;
  double* S;            // [B][nchunk][J (J + 1) / 2] forward chunk offsets C_c, then the chunks' start states
  double* ux;           // [B][npts][J] u(x)
  double* e;            // [B][npts][J] v(x), then e
  double* left;         // [B][npts]
  double* var;          // point r of problem b -> var[b * var_stride + r]
  long var_stride;
  BInvDiagParams Q;     // pass 2: Q.Q the backward start matrices (Q.cT: only read beside, by the solve's summarize)
};

// the lane's times: sample i of chunk c at t(i), i <= L (the next chunk's first sample)
__device__ __forceinline__ DirectSeries bpvrec_times(const BatchParams& P, int b, int c) {
  return DirectSeries{P.t + b * P.t_stride + c * P.lane_cs, nullptr, nullptr, P.lane_is, P.lane_cs, P.L, (long)P.N - (long)c * P.L};
}

// first index r in [0, n) with !(x[r] < T) (NaN points count as +inf: they sort last)
__device__ __forceinline__ int bpvrec_lower_bound(const double* x, int n, double T) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (x[mid] < T) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// exp(-c_j dt) for the J rows (one library exp per distinct rate)
template <int JR, int JC>
__device__ __forceinline__ void bpvrec_decay(const Problem<JR, JC>& p, double dt, double* out) {
#pragma unroll
  for (int j = 0; j < JR; ++j) out[j] = exp(-p.cr[j] * dt);
#pragma unroll
  for (int j = 0; j < JC; ++j) out[JR + 2 * j] = out[JR + 2 * j + 1] = exp(-p.cc[j] * dt);
}

// 0. one thread per (problem, point)
template <int JR, int JC, bool FAST>
__global__ void __launch_bounds__(256) bpvrec_features_kernel(const BatchParams P, const BPredVarRecParams S) {
  constexpr int J = JR + 2 * JC;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)P.B * S.npts) return;
  const int b = (int)(idx / S.npts), r = (int)(idx % S.npts);
  Problem<JR, JC> p;
  load_problem<JR, JC>(P, b, p);
  double uu[J], vv[J];
  features_uv<JR, JC, FAST>(p, S.xs[(long)b * S.xs_stride + r], uu, vv);
#pragma unroll
  for (int j = 0; j < J; ++j) { S.ux[idx * J + j] = uu[j]; S.e[idx * J + j] = vv[j]; }
}

// passes 1 (REPLAY = false) and 3
template <int JR, int JC, bool LEAN, bool FAST, bool REPLAY>
__global__ void __launch_bounds__(64) bpvrec_forward_kernel(const BatchParams P, const BPredVarRecParams S) {
  constexpr int J = JR + 2 * JC, NS = J * (J + 1) / 2;
  const int b = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x;
  if (c >= P.nchunk) return;
  const auto F = make_slots<JR, JC, LEAN, FAST>(P, b, c);
  const DirectSeries ts = bpvrec_times(P, b, c);
  Problem<JR, JC> p;
  load_problem<JR, JC>(P, b, p);
  double* ss = S.S + ((long)b * P.nchunk + c) * NS;
  double Sm[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) Sm[k] = REPLAY ? ss[k] : 0.0;
  const int n0 = c * P.L;
  const int last = (P.N - n0 < P.L) ? P.N - n0 : P.L;  // samples of this chunk inside the series
  const double k0 = p.sum_ar + p.sum_ac;
  // the lane's points [cur, end)
  const double* xp = S.xs + (long)b * S.xs_stride;
  const long row = (long)b * S.npts;
  int cur = 0, end = 0;
  if (REPLAY) {
    cur = (c == 0) ? 0 : bpvrec_lower_bound(xp, S.npts, ts.t(0));
    end = (c == P.nchunk - 1) ? S.npts : bpvrec_lower_bound(xp, S.npts, ts.t(P.L));
    if (c == 0) {  // before the first sample: S^x = 0, e = v(x) as the features kernel left it
      const double t0 = ts.t(0);
      while (cur < end && xp[cur] < t0) { S.left[row + cur] = 0.0; ++cur; }
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
    if (REPLAY) {
      const double tn = ts.t(i);
      const double tnext = tail ? 0.0 : ts.t(i + 1);
      while (cur < end && (tail || xp[cur] < tnext)) {
        double psi[J], w[J], ee[J], lf = 0.0;
        bpvrec_decay<JR, JC>(p, xp[cur] - tn, psi);
        const double* up = S.ux + (row + cur) * J;
        double* ep = S.e + (row + cur) * J;
#pragma unroll
        for (int j = 0; j < J; ++j) w[j] = psi[j] * up[j];
#pragma unroll
        for (int j = 0; j < J; ++j) {
          double sw = 0.0;
#pragma unroll
          for (int k = 0; k < J; ++k) sw = fma(Sm[sym_at<J>(j, k)], w[k], sw);
          lf = fma(w[j], sw, lf);
          ee[j] = ep[j] - psi[j] * sw;
        }
#pragma unroll
        for (int j = 0; j < J; ++j) ep[j] = ee[j];
        S.left[row + cur] = lf;
        if (tail) S.var[(long)b * S.var_stride + cur] = k0 - lf;
        ++cur;
      }
    }
    if (tail) break;
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
      for (int k = j; k < J; ++k) Sm[sym_index<J>(j, k)] = (ph[j] * ph[k]) * Sm[sym_index<J>(j, k)];
    }
  }
  if (!REPLAY) {
#pragma unroll
    for (int k = 0; k < NS; ++k) ss[k] = Sm[k];
  }
}

// pass 1b: start[c] = S ; S <- Psi_c S Psi_c + C_c, c ascending; one lane per problem
template <int JR, int JC>
__global__ void __launch_bounds__(64) bpvrec_walk_kernel(const BatchParams P, const BPredVarRecParams S) {
  constexpr int J = JR + 2 * JC, NS = J * (J + 1) / 2;
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  if (b >= P.B) return;
  Problem<JR, JC> p;
  load_problem<JR, JC>(P, (int)b, p);
  const double* tb = S.t + b * S.t_stride;
  double Sm[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) Sm[k] = 0.0;
  for (int c = 0; c < P.nchunk; ++c) {
    double* ss = S.S + (b * P.nchunk + c) * NS;
    double C[NS], psi[J];
#pragma unroll
    for (int k = 0; k < NS; ++k) { C[k] = ss[k]; ss[k] = Sm[k]; }
    if (c + 1 == P.nchunk) break;
    bpvrec_decay<JR, JC>(p, tb[(long)(c + 1) * P.L] - tb[(long)c * P.L], psi);
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
      for (int k = j; k < J; ++k) Sm[sym_index<J>(j, k)] = fma(psi[j] * psi[k], Sm[sym_index<J>(j, k)], C[sym_index<J>(j, k)]);
    }
  }
}

// pass 4: the recurrence of binvdiag_kernel from start[c], the points of every gap served on the way down
template <int JR, int JC, bool LEAN, bool FAST>
__global__ void __launch_bounds__(64) bpvrec_backward_kernel(const BatchParams P, const BPredVarRecParams S) {
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
  const double k0 = p.sum_ar + p.sum_ac;
  const double* xp = S.xs + (long)b * S.xs_stride;
  const long row = (long)b * S.npts;
  const int lo = (c == 0) ? 0 : bpvrec_lower_bound(xp, S.npts, ts.t(0));
  int cur = (c == P.nchunk - 1) ? S.npts : bpvrec_lower_bound(xp, S.npts, ts.t(P.L));
  // var of point r in the gap below the sample at time tm, Q = Q_m
  auto serve = [&](int r, double tm) {
    double dec[J], ep[J], quad = 0.0;
    bpvrec_decay<JR, JC>(p, tm - xp[r], dec);
    const double* ee = S.e + (row + r) * J;
#pragma unroll
    for (int j = 0; j < J; ++j) ep[j] = dec[j] * ee[j];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      double qe = 0.0;
#pragma unroll
      for (int k = 0; k < J; ++k) qe = fma(Q[sym_at<J>(j, k)], ep[k], qe);
      quad = fma(ep[j], qe, quad);
    }
    S.var[(long)b * S.var_stride + r] = (k0 - S.left[row + r]) - quad;
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
    if (n == P.N - 1) {  // the last sample: the gap above it is pass 3's; its transition is 0
      while (cur > lo && !(xp[cur - 1] < tn)) --cur;
#pragma unroll
      for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int k = j; k < J; ++k) Q[sym_index<J>(j, k)] = rd * uu[j] * uu[k];
      }
      continue;
    }
    {  // the gap m = n + 1: t_n <= x < t_{n+1}, Q = Q_{n+1}
      const double tm = ts.t(i + 1);
      while (cur > lo && !(xp[cur - 1] < tn)) { --cur; serve(cur, tm); }
    }
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
    const double t0 = ts.t(0);
    while (cur > 0) { --cur; serve(cur, t0); }
  }
}

}  // namespace clr
