// celerite_amd/csrc/clr_bcond_kernels.h -- the joint posterior of the latent process at M sorted points per problem from a
// plan's materialised factor: the covariance between the points (clr_batch_predict_cov) and joint draws
// (clr_batch_sample_conditional) in linear time -- no N x M block, no M x M factorisation.
//
// Slot notation of clr_bpredvar_rec_kernels.h (slot n: phi[n] the decay n -> n+1, u[n], W[n], D[n]; u(x), v(x) the feature
// rows at a point, c the rows' decay rates, S+_n and Q_n the factor's two matrix recurrences, F_n = Phi_n (I - W_n u_n^T)).
// Points ascending, m_j = #{n : t_n <= x_j} (m below).  Per point, with e_j of the recurrence variance's forward replay:
//     r_j = u(x_j) - exp(-c (t_m - x_j)) o (Q_m e'_j)                                     (m = N: r_j = u(x_j))
// and between consecutive points the J x J transport of the forward substitution's homogeneous state from x_j to x_{j+1}
//     T_j = decay to x_{j+1} . prod_{n = m_j}^{m_{j+1} - 1} (I - W_n u_n^T) (decay to t_n)                (decays only)
// the posterior covariance is C_ij = r_j^T T_{j-1} ... T_i e_i (i <= j), C_jj = r_j^T e_j, and C + reg I = L diag(d) L^T
// with L_ji = r_j^T T_{j-1} ... T_i omega_i follows from the celerite recurrence with T in place of the diagonal decay:
//     d_j = r_j^T e_j + reg - r_j^T G_j r_j ,  omega_j = (e_j - G_j r_j) / d_j ,  G_{j+1} = T_j (G_j + d_j omega_j omega_j^T) T_j^T
//     a draw: z_j = sqrt(d_j) n_j ,  f_j = z_j + r_j^T gamma_j ,  gamma_{j+1} = T_j (gamma_j + omega_j z_j)
// Passes, per tile of PROBLEMS (a problem needs all its points at once):
//   0. bpvrec_features_kernel, bpvrec_forward_kernel<true> (clr_bpredvar_rec_kernels.h, unchanged): u(x), e of every point;
//   1. bcond_backward_kernel       bpvrec_backward_kernel storing the vector r_j over u(x) instead of the quadratic form;
//   2. bcond_transport_kernel      lane = (problem, chunk), carrying T alone: per owned point the transport from the
//                                  previous owned point (or the chunk's start), and the transport from the last owned point
//                                  (or the start) to the chunk's end; a chunk that owns no point IS the solve's chunk map
//                                  (bs_M) and is left to it where that is formed -- the steps without a point are the
//                                  solve's summarize's, the same bits either way;
//      bcond_stitch_kernel         one wave per problem, lane = entry of the J x J state: multiplies across chunk boundaries
//                                  and across chunks that own no point, T[j] = transport x_{j-1} -> x_j;
//   3. bcond_pair_kernel           lane = (problem, source i): h <- T_j h from e_i, r_j^T h into both triangles;
//   4. bcond_factor_kernel         one wave per problem, the J x J state over the lanes through LDS, sequential in j;
//      bcond_draw_kernel           lane = (problem, draw), sequential in j.
// Ownership of points and cursors as bpvrec_forward_kernel; no atomics; a problem's result is a function of its factor, its
// chunking and its points alone.
#pragma once

namespace clr {

struct BCondParams {
  int npts;             // points per problem
  int lean;
  int have_M;           // the solve's chunk maps of this factor are formed (read only)
  int size;             // draws per problem
  const double* xs;     // ascending: point r of problem b at xs[b * xs_stride + r] (xs_stride 0: shared)
  long xs_stride;
  const double* t;      // the plan's times, row-major (the chunk boundaries)
  long t_stride;
  const double* Q;      // [B][nchunk][J (J + 1) / 2] the backward start matrices (loo_Q)
  const double* M;      // [B][nchunk][J * J] the solve's chunk maps (bs_M)
  double* r;            // [B][npts][J] u(x), then r
  const double* e;      // [B][npts][J] e
  double* T;            // [B][npts][J * J] entry j: the transport into x_j (entry 0 is not used)
  double* E;            // [B][nchunk][J * J] the chunks' transports to their ends
  int* own;             // [B][nchunk] points a chunk owns
  double* cov;          // [B][npts][npts]
  double regularize, min_pivot;
  double* sd;           // [B][npts] sqrt(d), 0 at a degenerate pivot
  double* omega;        // [B][npts][J]
  int* status;          // [B] 0 or CLR_NOT_POSITIVE_DEFINITE's value
  const double* normals;  // [B][size][npts]
  double* draws;          // [B][size][npts]
};

// 1. the recurrence of bpvrec_backward_kernel from start[c]; r of every point served on the way down (points from t_{N-1}
// on keep u(x))
template <int JR, int JC, bool LEAN, bool FAST>
__global__ void __launch_bounds__(64) bcond_backward_kernel(const BatchParams P, const BCondParams S) {
  constexpr int J = JR + 2 * JC, NS = J * (J + 1) / 2;
  const int b = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x;
  if (c >= P.nchunk) return;
  const auto F = make_slots<JR, JC, LEAN, FAST>(P, b, c);
  const DirectSeries ts = bpvrec_times(P, b, c);
  Problem<JR, JC> p;
  load_problem<JR, JC>(P, b, p);
  const double* qs = S.Q + ((long)b * P.nchunk + c) * NS;
  double Q[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) Q[k] = qs[k];
  const int n0 = c * P.L;
  const int last = (P.N - n0 < P.L) ? P.N - n0 : P.L;
  const double* xp = S.xs + (long)b * S.xs_stride;
  const long row = (long)b * S.npts;
  const int lo = (c == 0) ? 0 : bpvrec_lower_bound(xp, S.npts, ts.t(0));
  int cur = (c == P.nchunk - 1) ? S.npts : bpvrec_lower_bound(xp, S.npts, ts.t(P.L));
  // r of point q in the gap below the sample at time tm, Q = Q_m
  auto serve = [&](int q, double tm) {
    double dec[J], ep[J];
    bpvrec_decay<JR, JC>(p, tm - xp[q], dec);
    const double* ee = S.e + (row + q) * J;
    double* rp = S.r + (row + q) * J;
#pragma unroll
    for (int j = 0; j < J; ++j) ep[j] = dec[j] * ee[j];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      double qe = 0.0;
#pragma unroll
      for (int k = 0; k < J; ++k) qe = fma(Q[sym_at<J>(j, k)], ep[k], qe);
      rp[j] = rp[j] - dec[j] * qe;
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
    if (i > 0) F.get(i - 1, nph, nuu, nww, &nd);
    const double tn = ts.t(i);
    if (n == P.N - 1) {  // the last sample: the points above it keep r = u(x); its transition is 0
      while (cur > lo && !(xp[cur - 1] < tn)) --cur;
#pragma unroll
      for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int k = j; k < J; ++k) Q[sym_index<J>(j, k)] = rd * uu[j] * uu[k];
      }
      continue;
    }
    {
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

// 2. the transports of one chunk.  T is the transport from the last emitted position (an owned point, or the chunk's
// start: at t_lo, before sample lo's update) to the walk's position; a step without a point is the step of
// bsolve_summarize_kernel's chunk map, expression for expression.
template <int JR, int JC, bool LEAN, bool FAST>
__global__ void __launch_bounds__(64) bcond_transport_kernel(const BatchParams P, const BCondParams S) {
  constexpr int J = JR + 2 * JC;
  const int b = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x;
  if (c >= P.nchunk) return;
  const auto F = make_slots<JR, JC, LEAN, FAST>(P, b, c);
  const DirectSeries ts = bpvrec_times(P, b, c);
  Problem<JR, JC> p;
  load_problem<JR, JC>(P, b, p);
  const bool last_chunk = c == P.nchunk - 1;
  const double* xp = S.xs + (long)b * S.xs_stride;
  const long row = (long)b * S.npts;
  int cur = (c == 0) ? 0 : bpvrec_lower_bound(xp, S.npts, ts.t(0));
  const int end = last_chunk ? S.npts : bpvrec_lower_bound(xp, S.npts, ts.t(P.L));
  S.own[(long)b * P.nchunk + c] = end - cur;
  if (cur == end && (last_chunk || S.have_M)) return;  // (the stitch reads the solve's chunk map; the last chunk's end is never read)
  double T[J * J];
#pragma unroll
  for (int k = 0; k < J * J; ++k) T[k] = (k / J == k % J) ? 1.0 : 0.0;
  // point `cur` at decay `psi` from the walk's position: T[cur] = diag(psi) T, and the walk starts anew at the point
  auto emit = [&](const double* psi) {
    double* o = S.T + (row + cur) * (J * J);
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
      for (int k = 0; k < J; ++k) { o[j * J + k] = psi[j] * T[j * J + k]; T[j * J + k] = (j == k) ? 1.0 : 0.0; }
    }
  };
  auto decay_to = [&](const double* psi) {
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
      for (int k = 0; k < J; ++k) T[j * J + k] = psi[j] * T[j * J + k];
    }
  };
  const int n0 = c * P.L;
  const int last = (P.N - n0 < P.L) ? P.N - n0 : P.L;
  if (c == 0) {  // before the first sample: pure decays
    const double t0 = ts.t(0);
    double at = 0.0, psi[J];
    bool any = false;
    while (cur < end && xp[cur] < t0) {
      bpvrec_decay<JR, JC>(p, any ? xp[cur] - at : 0.0, psi);
      emit(psi);
      at = xp[cur]; any = true;
      ++cur;
    }
    if (any) { bpvrec_decay<JR, JC>(p, t0 - at, psi); decay_to(psi); }
  }
  double nph[J], nuu[J], nww[J], nd;
  F.get(0, nph, nuu, nww, &nd);
  for (int i = 0; i < last; ++i) {
    const int n = n0 + i;
    double ph[J], uu[J], ww[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { ph[j] = nph[j]; uu[j] = nuu[j]; ww[j] = nww[j]; }
    if (i + 1 < last) F.get(i + 1, nph, nuu, nww, &nd);  // (the next step's slot, one step ahead)
    const bool tail = (n == P.N - 1);
    const double tnext = tail ? 0.0 : ts.t(i + 1);
    if (!(cur < end && (tail || xp[cur] < tnext))) {  // no point in this gap: T <- Phi (T - W (u^T T))
      if (tail) break;
      double pw[J];
#pragma unroll
      for (int j = 0; j < J; ++j) pw[j] = ph[j] * ww[j];
#pragma unroll
      for (int k = 0; k < J; ++k) {
        double r = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) r = fma(uu[j], T[j * J + k], r);
#pragma unroll
        for (int j = 0; j < J; ++j) T[j * J + k] = fma(-pw[j], r, ph[j] * T[j * J + k]);
      }
      continue;
    }
    // T <- T - W (u^T T), the points of the gap, the decay to the next sample
#pragma unroll
    for (int k = 0; k < J; ++k) {
      double r = 0.0;
#pragma unroll
      for (int j = 0; j < J; ++j) r = fma(uu[j], T[j * J + k], r);
#pragma unroll
      for (int j = 0; j < J; ++j) T[j * J + k] = fma(-ww[j], r, T[j * J + k]);
    }
    double at = ts.t(i), psi[J];
    while (cur < end && (tail || xp[cur] < tnext)) {
      bpvrec_decay<JR, JC>(p, xp[cur] - at, psi);
      emit(psi);
      at = xp[cur];
      ++cur;
    }
    if (tail) break;
    bpvrec_decay<JR, JC>(p, tnext - at, psi);
    decay_to(psi);
  }
  if (!last_chunk) {
    double* o = S.E + ((long)b * P.nchunk + c) * (J * J);
#pragma unroll
    for (int k = 0; k < J * J; ++k) o[k] = T[k];
  }
}

// 2b. one wave per problem over the chunks, lane (j, k) = entry of the J x J carry X: the transport from the last point
// seen to the start of the chunk at hand.  A chunk's first owned point takes T <- T X; then X <- its transport to its
// end; a chunk that owns no point multiplies X <- E X (E: the solve's chunk map where that is formed).
template <int J>
__global__ void __launch_bounds__(64) bcond_stitch_kernel(const BatchParams P, const BCondParams S) {
  __shared__ double Xs[J * J], Es[J * J];
  const int b = blockIdx.x, lane = threadIdx.x;
  const bool live = lane < J * J;
  const int j = live ? lane / J : 0, k = live ? lane % J : 0;
  const int* own = S.own + (long)b * P.nchunk;
  const long row = (long)b * S.npts;
  bool seen = false;
  int cur = 0;
  for (int c = 0; c < P.nchunk; ++c) {
    const int cnt = own[c];
    const bool last_chunk = c == P.nchunk - 1;
    if (cnt > 0 && seen) {  // T[cur] <- T[cur] X
      double* tp = S.T + (row + cur) * (J * J);
      if (live) Es[lane] = tp[lane];
      __syncthreads();
      double a = 0.0;
#pragma unroll
      for (int i = 0; i < J; ++i) a = fma(Es[j * J + i], Xs[i * J + k], a);
      if (live) tp[lane] = a;
      __syncthreads();
    }
    if (!last_chunk) {
      const double* src = ((cnt == 0 && S.have_M) ? S.M : S.E) + ((long)b * P.nchunk + c) * (J * J);
      if (cnt > 0 || !seen) {  // X <- E (before the first point the carry is not read)
        __syncthreads();
        if (live) Xs[lane] = src[lane];
        __syncthreads();
      } else {  // X <- E X
        if (live) Es[lane] = src[lane];
        __syncthreads();
        double a = 0.0;
#pragma unroll
        for (int i = 0; i < J; ++i) a = fma(Es[j * J + i], Xs[i * J + k], a);
        __syncthreads();
        if (live) Xs[lane] = a;
        __syncthreads();
      }
    }
    if (cnt > 0) seen = true;
    cur += cnt;
  }
}

// 3. lane = (problem, source i): C_ii = r_i^T e_i; h <- T_j h from e_i, C_ij = C_ji = r_j^T h.  The lanes of a wave read
// the same T_j and r_j.
template <int J>
__global__ void __launch_bounds__(64) bcond_pair_kernel(const BatchParams P, const BCondParams S) {
  const int b = blockIdx.y, i0 = blockIdx.x * 64, i = i0 + threadIdx.x;
  const long row = (long)b * S.npts, Mm = S.npts;
  const bool live = i < S.npts;
  double* cov = S.cov + (long)b * Mm * Mm;
  double h[J];
  {
    const double* ee = S.e + (row + (live ? i : 0)) * J;
    const double* rr = S.r + (row + (live ? i : 0)) * J;
    double v = 0.0;
#pragma unroll
    for (int a = 0; a < J; ++a) { h[a] = ee[a]; v = fma(rr[a], h[a], v); }
    if (live) cov[i * Mm + i] = v;
  }
  for (int j = i0 + 1; j < S.npts; ++j) {
    const double* Tj = S.T + (row + j) * (J * J);
    const double* rj = S.r + (row + j) * J;
    if (!(live && j > i)) continue;
    double nh[J], v = 0.0;
#pragma unroll
    for (int a = 0; a < J; ++a) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < J; ++q) s = fma(Tj[a * J + q], h[q], s);
      nh[a] = s;
    }
#pragma unroll
    for (int a = 0; a < J; ++a) { h[a] = nh[a]; v = fma(rj[a], h[a], v); }
    cov[i * Mm + j] = v;
    cov[j * Mm + i] = v;
  }
}

// 4. one wave per problem, sequential in j; lane (a, q) = entry of the J x J state G, the vectors in LDS.  Every lane forms
// the pivot itself, in one order.  One lane per problem would hold G, T and a product, 3 J^2 doubles (384 VGPRs at width 8),
// and leave all but B / 64 waves idle; this mapping takes 18..56 VGPRs and B waves (it was not A/B-timed).
template <int JR, int JC>
__global__ void __launch_bounds__(64) bcond_factor_kernel(const BatchParams P, const BCondParams S) {
  constexpr int J = JR + 2 * JC;
  __shared__ double G[J * J], H[J * J], X[J * J], Tm[J * J], rr[J], ee[J], gr[J], om[J];
  const int b = blockIdx.x, lane = threadIdx.x;
  const bool live = lane < J * J, vec = lane < J;
  const int a = live ? lane / J : 0, q = live ? lane % J : 0;
  Problem<JR, JC> p;
  load_problem<JR, JC>(P, b, p);
  const double tol = S.min_pivot * (p.sum_ar + p.sum_ac);
  const long row = (long)b * S.npts;
  if (live) G[lane] = 0.0;
  int status = 0;
  for (int j = 0; j < S.npts; ++j) {
    if (vec) { rr[lane] = S.r[(row + j) * J + lane]; ee[lane] = S.e[(row + j) * J + lane]; }
    if (live && j + 1 < S.npts) Tm[lane] = S.T[(row + j + 1) * (J * J) + lane];
    __syncthreads();
    if (vec) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < J; ++i) s = fma(G[lane * J + i], rr[i], s);
      gr[lane] = s;
    }
    __syncthreads();
    double re = 0.0, rg = 0.0;
#pragma unroll
    for (int i = 0; i < J; ++i) { re = fma(rr[i], ee[i], re); rg = fma(rr[i], gr[i], rg); }
    const double d = (re + S.regularize) - rg;
    if (!(d >= -tol) || !(d <= 1.79769313486231570815e+308)) { status = 2; break; }  // (below the bar, or not finite)
    const bool degenerate = fabs(d) <= tol;
    const double dd = degenerate ? 0.0 : d;
    if (vec) {
      const double w = degenerate ? 0.0 : (ee[lane] - gr[lane]) / d;
      om[lane] = w;
      S.omega[(row + j) * J + lane] = w;
    }
    if (lane == 0) S.sd[row + j] = sqrt(dd);
    if (j + 1 == S.npts) break;
    __syncthreads();
    if (live) H[lane] = fma(dd * om[a], om[q], G[lane]);
    __syncthreads();
    if (live) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < J; ++i) s = fma(Tm[a * J + i], H[i * J + q], s);
      X[lane] = s;
    }
    __syncthreads();
    if (live) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < J; ++i) s = fma(X[a * J + i], Tm[q * J + i], s);
      G[lane] = s;
    }
    __syncthreads();
  }
  if (lane == 0) S.status[b] = status;
}

// 4b. lane = (problem, draw), sequential in j
template <int J>
__global__ void __launch_bounds__(64) bcond_draw_kernel(const BatchParams P, const BCondParams S) {
  const int b = blockIdx.y, s = blockIdx.x * 64 + threadIdx.x;
  if (s >= S.size) return;
  const long row = (long)b * S.npts;
  const double* nn = S.normals + ((long)b * S.size + s) * S.npts;
  double* out = S.draws + ((long)b * S.size + s) * S.npts;
  double g[J];
#pragma unroll
  for (int a = 0; a < J; ++a) g[a] = 0.0;
  for (int j = 0; j < S.npts; ++j) {
    const double* rj = S.r + (row + j) * J;
    const double* oj = S.omega + (row + j) * J;
    const double z = S.sd[row + j] * nn[j];
    double f = 0.0;
#pragma unroll
    for (int a = 0; a < J; ++a) f = fma(rj[a], g[a], f);
    out[j] = z + f;
    if (j + 1 == S.npts) break;
    const double* Tn = S.T + (row + j + 1) * (J * J);
    double w[J], ng[J];
#pragma unroll
    for (int a = 0; a < J; ++a) w[a] = fma(oj[a], z, g[a]);
#pragma unroll
    for (int a = 0; a < J; ++a) {
      double t = 0.0;
#pragma unroll
      for (int i = 0; i < J; ++i) t = fma(Tn[a * J + i], w[i], t);
      ng[a] = t;
    }
#pragma unroll
    for (int a = 0; a < J; ++a) g[a] = ng[a];
  }
}

}  // namespace clr
