// celerite_amd/csrc/clr_bpredvar_kernels.h -- the conditional variance of GP.predict (celerite.py:465-470) for every
// problem of a plan from its materialised factor, parallel in n:
//     var_p(x*) = k_p(0) - k*^T K_p^-1 k* ,   k*_n = k_p(x* - t_{p,n}) ,   k_p(0) = sum a_real + sum a_comp
// With K = L D L^T the quadratic form is sum_n z_n^2 / D_n for z = L^-1 k* (dot_solve, cholesky.h:343-357): the FORWARD
// half of the batched solve (clr_bsolve_kernels.h) and nothing else -- no backward sweep, nothing written per sample.
// The right-hand sides are a function of what the plan holds on the device (times, coefficients) and of the prediction
// points, so they are formed there, a TILE of points at a time (BPredVarParams::nrhs of them: device scratch is bounded
// whatever M is).  Passes over one tile, lane = (problem, chunk), the right-hand side on grid.z:
//   1. bpredvar_cross_kernel     k_p(x*_m - t_{p,n}) straight into the chunk-interleaved layout [problem][rhs][i][chunk]:
//                                tau first, then exp(-c |tau|), cos(d tau), sin(d |tau|) per entry (a running product
//                                along n underflows on sparse series and cannot recover);
//   2. bsolve_summarize_kernel   the forward offsets of every chunk from the zero state (and, once per factor, the chunk
//      bsolve_prefix_kernel      maps M the batched solve shares), then the walk over the chunks;
//   3. bpredvar_forward_kernel   the forward recurrence from the true start states, accumulating x_n^2 / D_n per
//                                (problem, rhs, chunk); one lane carries RPL right-hand sides of its (problem, chunk) in
//                                registers, so that a step's factor slot -- and, on the lean layout, the regenerated
//                                phi, u -- is fetched once and serves all of them;
//   4. bpredvar_finish_kernel    var = k_p(0) - the chunk partials summed in chunk order.
// Every right-hand side is independent of the others and of the tile it rides in: a point's result does not depend on
// the tile size.  Padded samples n >= N are skipped (their cross-covariance is written as 0).
#pragma once

namespace clr {

struct BPredVarParams {
  int nrhs;             // points of this tile
  int lean;             // the factor holds W, D only
  int have_M;           // the chunk maps of this factor are already in M (an earlier solve or tile formed them)
  int cross_fast;       // host-verified: max|d_comp| * max|x* - t| < CLR_FAST_TRIG_LIMIT (the cross-covariances' phases)
  const double* xs;     // the tile's points: point r of problem b at xs[b * xs_stride + r] (xs_stride 0: shared)
  long xs_stride;
  const double* t;      // the plan's times, row-major [problem][n]
  long t_stride;
  double* xT;           // [B][nrhs][L][nchunk] the cross-covariances
  double* M;            // [B][nchunk][J*J]
  double* off;          // [B][nrhs][nchunk][J] chunk offsets of the forward sweep
  double* starts;       // [B][nrhs][nchunk][J] chunk start states
  double* part;         // [B][nrhs][nchunk] sum x^2 / D of every chunk (may alias off: the walk has consumed the offsets)
  double* var;          // point r of problem b -> var[b * var_stride + r]
  long var_stride;
};

// right-hand sides one lane of bpredvar_forward_kernel carries: states RPL x J, the current and the prefetched slot
// 2 (3 J + 1), values 2 RPL and sums RPL doubles -- 8 at widths <= 4 (<= 106 doubles), 4 above (<= 94 at width 8), inside
// the 512 VGPRs of a wave that has its SIMD to itself (__launch_bounds__(64))
constexpr int bpredvar_rhs_per_lane(int J) { return J <= 4 ? 8 : 4; }

// k(tau) of celerite terms (terms.py: RealTerm / ComplexTerm get_value), every factor evaluated at |tau| directly
template <bool FAST>
__device__ __forceinline__ double cross_covariance(const double* ar, const double* cr, int JR, const double* ac,
                                                   const double* bc, const double* cc, const double* dc, int JC, double tau) {
  const double at = fabs(tau);
  double k = 0.0;
  for (int j = 0; j < JR; ++j) k = fma(ar[j], exp(-cr[j] * at), k);
  for (int j = 0; j < JC; ++j) {
    double sd, cd;
    sincos_phase<FAST>(dc[j] * at, &sd, &cd);  // cos(d tau) = cos(d |tau|)
    k = fma(exp(-cc[j] * at), fma(ac[j], cd, bc[j] * sd), k);
  }
  return k;
}

// 1. one thread per cell (i, chunk) of right-hand side blockIdx.z of problem blockIdx.y
template <int JR, int JC, bool FAST>
__global__ void __launch_bounds__(256) bpredvar_cross_kernel(const BatchParams P, const BPredVarParams S) {
  const int b = blockIdx.y, r = blockIdx.z;
  const long cells = (long)P.L * P.nchunk;
  const long cell = (long)blockIdx.x * 256 + threadIdx.x;
  if (cell >= cells) return;
  const int i = (int)(cell / P.nchunk), c = (int)(cell % P.nchunk);
  const long n = (long)c * P.L + i;
  double v = 0.0;
  if (n < P.N) {
    const double x = S.xs[(long)b * S.xs_stride + r];
    v = cross_covariance<FAST>(P.a_real + (long)b * JR, P.c_real + (long)b * JR, JR, P.a_comp + (long)b * JC, P.b_comp + (long)b * JC,
                               P.c_comp + (long)b * JC, P.d_comp + (long)b * JC, JC, x - S.t[(long)b * S.t_stride + n]);
  }
  S.xT[((long)b * S.nrhs + r) * cells + cell] = v;
}

// 3. forward recurrence per chunk from its start state for RPL right-hand sides at once: sum x^2 / D per (rhs, chunk)
template <int JR, int JC, bool LEAN, bool FAST, int RPL>
__global__ void __launch_bounds__(64) bpredvar_forward_kernel(const BatchParams P, const BPredVarParams S) {
  constexpr int J = JR + 2 * JC;
  const int b = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x, r0 = blockIdx.z * RPL;
  if (c >= P.nchunk) return;
  const auto F = make_slots<JR, JC, LEAN, FAST>(P, b, c);
  const long cells = (long)P.L * P.nchunk;
  // (a ragged last group -- a tile of one point is one: the spare slots are skipped, a branch the whole grid.z slice
  //  takes alike, so a right-hand side costs the same arithmetic and the same bits whichever slot it rides in)
  const int nk = S.nrhs - r0 < RPL ? S.nrhs - r0 : RPL;
  long ro[RPL];
  double g[RPL][J], q[RPL], nb[RPL];
#pragma unroll
  for (int k = 0; k < RPL; ++k) {
    const long row = (long)b * S.nrhs + r0 + (k < nk ? k : 0);
    ro[k] = row * cells + c;
    q[k] = 0.0;
    nb[k] = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) g[k][j] = 0.0;
    if (k < nk) {
      const double* st = S.starts + (row * P.nchunk + c) * J;
#pragma unroll
      for (int j = 0; j < J; ++j) g[k][j] = st[j];
    }
  }
  const int n0 = c * P.L;
  // (the slot of step i + 1 and its right-hand sides one step ahead of the arithmetic, as in the batched solve)
  double nph[J], nuu[J], nww[J], nd;
  F.get(0, nph, nuu, nww, &nd);
#pragma unroll
  for (int k = 0; k < RPL; ++k)
    if (k < nk) nb[k] = S.xT[ro[k]];
  for (int i = 0; i < P.L; ++i) {
    const int n = n0 + i;
    if (n >= P.N) break;  // (padding: only the last chunk's lanes)
    double ph[J], uu[J], ww[J], bn[RPL];
#pragma unroll
    for (int j = 0; j < J; ++j) { ph[j] = nph[j]; uu[j] = nuu[j]; ww[j] = nww[j]; }
#pragma unroll
    for (int k = 0; k < RPL; ++k) bn[k] = nb[k];
    const double rd = 1.0 / nd;
    if (i + 1 < P.L && n + 1 < P.N) {
      F.get(i + 1, nph, nuu, nww, &nd);
#pragma unroll
      for (int k = 0; k < RPL; ++k)
        if (k < nk) nb[k] = S.xT[ro[k] + (long)(i + 1) * P.nchunk];
    }
#pragma unroll
    for (int k = 0; k < RPL; ++k) {
      if (k >= nk) break;
      double ug = 0.0;
#pragma unroll
      for (int j = 0; j < J; ++j) ug = fma(uu[j], g[k][j], ug);
      const double xn = bn[k] - ug;
      q[k] = fma(xn * xn, rd, q[k]);
#pragma unroll
      for (int j = 0; j < J; ++j) g[k][j] = ph[j] * fma(ww[j], xn, g[k][j]);
    }
  }
#pragma unroll
  for (int k = 0; k < RPL; ++k)
    if (k < nk) S.part[((long)b * S.nrhs + r0 + k) * P.nchunk + c] = q[k];
}

// 4. one lane per (problem, point): k(0) less the chunk partials in chunk order
template <int JR, int JC>
__global__ void __launch_bounds__(64) bpredvar_finish_kernel(const BatchParams P, const BPredVarParams S) {
  const long idx = (long)blockIdx.x * 64 + threadIdx.x;
  if (idx >= (long)P.B * S.nrhs) return;
  const int b = (int)(idx / S.nrhs), r = (int)(idx % S.nrhs);
  Problem<JR, JC> p;
  load_problem<JR, JC>(P, b, p);
  const double* part = S.part + idx * P.nchunk;
  double s = 0.0;
  for (int c = 0; c < P.nchunk; ++c) s += part[c];
  S.var[(long)b * S.var_stride + r] = (p.sum_ar + p.sum_ac) - s;
}

}  // namespace clr
