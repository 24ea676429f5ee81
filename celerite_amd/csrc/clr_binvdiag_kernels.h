// celerite_amd/csrc/clr_binvdiag_kernels.h -- diag(K^-1) for every problem of a plan from its materialised factor in
// O(N J^2): what the leave-one-out predictive distribution needs (y_n - mu_-n = alpha_n / c_n, sigma^2_-n = 1 / c_n with
// c_n = (K^-1)_nn, alpha = K^-1 r).
//
// In the solve's slot notation (clr_bsolve_kernels.h: slot n holds phi[n], u[n], W[n], D[n]; F_n = Phi_n (I - W_n u_n^T),
// the last sample's transition is 0) column n of L^-1 is x_n = 1, g = phi[n] o W[n], then x_m = -u[m] . g, g <- F_m g for
// m > n, and c_n = sum_m x_m^2 / D_m.  So with the symmetric J x J matrix
//     Q_n = u[n] u[n]^T / D_n + F_n^T Q_{n+1} F_n ,   Q_N = 0
//     c_n = 1 / D_n + g_n^T Q_{n+1} g_n ,             g_n = phi[n] o W[n]
// one backward matrix recurrence gives all N entries.  One matrix-vector product serves the output and the update: with
// P = Phi_n Q_{n+1} Phi_n, v = P W[n] = phi[n] o (Q_{n+1} g_n), s = g_n^T Q_{n+1} g_n:
//     c_n = 1 / D_n + s ,   Q_n = P - u v^T - v u^T + c_n u u^T                    (about 5 J^2 flops per sample)
// The map Q -> C + M^T Q M composes: over a chunk lo .. hi-1, Q_lo = C_c + M_c^T Q_hi M_c with M_c = F_{hi-1} ... F_lo,
// exactly the chunk map of the batched solve (bs_M, formed by ITS bsolve_summarize_kernel when no solve has yet).  Passes:
//   1. binvdiag_kernel<.., false>  per chunk from Q = 0: the chunk's offset C_c;
//   2. binvdiag_walk_kernel        one lane per problem over the chunks, descending: start[c] = Q ; Q <- C_c + M_c^T Q M_c
//                                  (start[c] overwrites C_c: one buffer);
//   3. binvdiag_kernel<.., true>   the same recurrence per chunk from start[c]: c_n into [problem][i][chunk].
// Lane = (problem, chunk).  Q is kept as its upper triangle, J (J + 1) / 2 doubles, in registers.
// Conventions at the end of the series are the solve's: padded samples n >= N are skipped; sample N-1 (transition 0)
// gives c_{N-1} = 1 / D_{N-1} and Q_{N-1} = u u^T / D_{N-1}.
#pragma once

namespace clr {

struct BInvDiagParams {
  int lean;        // the factor holds W, D only
  int have_M;      // the chunk maps of this factor are already in M (clr_batch_solve's validity rule)
  double* cT;      // [B][L][nchunk] diag(K^-1), chunk-interleaved
  double* M;       // [B][nchunk][J*J] the batched solve's chunk maps
  double* Q;       // [B][nchunk][J (J + 1) / 2] chunk offsets C_c, then the chunks' start matrices
  double* off;     // [B][nchunk][J] scratch of the solve's summarize when it forms the chunk maps here
};

// entry (j, k), j <= k, of a symmetric J x J matrix kept as its upper triangle, row after row
template <int J>
__device__ __forceinline__ constexpr int sym_index(int j, int k) { return j * J - (j * (j - 1)) / 2 + (k - j); }
template <int J>
__device__ __forceinline__ constexpr int sym_at(int j, int k) { return j <= k ? sym_index<J>(j, k) : sym_index<J>(k, j); }

// passes 1 and 3
template <int JR, int JC, bool LEAN, bool FAST, bool REPLAY>
__global__ void __launch_bounds__(64) binvdiag_kernel(const BatchParams P, const BInvDiagParams S) {
  constexpr int J = JR + 2 * JC, NS = J * (J + 1) / 2;
  const int b = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x;
  if (c >= P.nchunk) return;
  const auto F = make_slots<JR, JC, LEAN, FAST>(P, b, c);
  const long cells = (long)P.L * P.nchunk;
  double* out = S.cT + (long)b * cells + c;
  double* qs = S.Q + ((long)b * P.nchunk + c) * NS;
  double Q[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) Q[k] = REPLAY ? qs[k] : 0.0;
  const int n0 = c * P.L;
  const int last = (P.N - n0 < P.L) ? P.N - n0 : P.L;  // samples of this chunk inside the series
  double nph[J], nuu[J], nww[J], nd;
  F.get(last - 1, nph, nuu, nww, &nd);
  for (int i = last - 1; i >= 0; --i) {
    const int n = n0 + i;
    double ph[J], uu[J], ww[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { ph[j] = nph[j]; uu[j] = nuu[j]; ww[j] = nww[j]; }
    const double rd = 1.0 / nd;
    if (i > 0) F.get(i - 1, nph, nuu, nww, &nd);  // (the previous sample's slot, one step ahead)
    if (n == P.N - 1) {  // the last sample: its transition is 0
      if (REPLAY) out[(long)i * P.nchunk] = rd;
#pragma unroll
      for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int k = j; k < J; ++k) Q[sym_index<J>(j, k)] = rd * uu[j] * uu[k];
      }
      continue;
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
    if (REPLAY) out[(long)i * P.nchunk] = cn;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const double cu = cn * uu[j];
#pragma unroll
      for (int k = j; k < J; ++k) {
        const double p = (ph[j] * ph[k]) * Q[sym_index<J>(j, k)];
        Q[sym_index<J>(j, k)] = fma(cu, uu[k], p - fma(uu[j], v[k], v[j] * uu[k]));
      }
    }
  }
  if (!REPLAY) {
#pragma unroll
    for (int k = 0; k < NS; ++k) qs[k] = Q[k];
  }
}

// pass 2: start[c] = Q ; Q <- C_c + M_c^T Q M_c, c descending; one lane per problem
template <int J>
__global__ void __launch_bounds__(64) binvdiag_walk_kernel(const BatchParams P, const BInvDiagParams S) {
  constexpr int NS = J * (J + 1) / 2;
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  if (b >= P.B) return;
  double Q[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) Q[k] = 0.0;
  for (int c = P.nchunk - 1; c >= 0; --c) {
    const double* Mc = S.M + (b * P.nchunk + c) * (J * J);
    double* qs = S.Q + (b * P.nchunk + c) * NS;
    double M[J * J], nx[NS];
#pragma unroll
    for (int k = 0; k < J * J; ++k) M[k] = Mc[k];
#pragma unroll
    for (int k = 0; k < NS; ++k) { nx[k] = qs[k]; qs[k] = Q[k]; }
    // column k of T = Q M, then entries (j, k), j <= k, of M^T T
#pragma unroll
    for (int k = 0; k < J; ++k) {
      double T[J];
#pragma unroll
      for (int i = 0; i < J; ++i) {
        double a = 0.0;
#pragma unroll
        for (int l = 0; l < J; ++l) a = fma(Q[sym_at<J>(i, l)], M[l * J + k], a);
        T[i] = a;
      }
#pragma unroll
      for (int j = 0; j <= k; ++j) {
        double a = nx[sym_index<J>(j, k)];
#pragma unroll
        for (int i = 0; i < J; ++i) a = fma(M[i * J + j], T[i], a);
        nx[sym_index<J>(j, k)] = a;
      }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) Q[k] = nx[k];
  }
}

}  // namespace clr
