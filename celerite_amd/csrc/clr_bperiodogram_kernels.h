// celerite_amd/csrc/clr_bperiodogram_kernels.h -- the periodogram under a plan's covariance: at every trial frequency w
// the generalised-least-squares fit of A cos w tau + B sin w tau (tau = t - t_ref) to the residual in force with K^-1 as
// the metric, for every problem of the plan, from its materialised factor.
//
// With K = L diag(D) L^T and z_x = L^-1 x every inner product is x^T K^-1 y = sum_n z_x[n] z_y[n] / D_n, and z_x is the
// forward recurrence of clr_bsolve_kernels.h / clr_bfilter_kernels.h (slot n: phi[n], u[n], W[n], D[n]):
//     z_n = x_n - u[n] . g_n ,  g+_n = g_n + W[n] z_n ,  g_{n+1} = phi[n] o g+_n ,  g_0 = 0 .
// The columns c_n = cos(w tau_n), s_n = sin(w tau_n) are formed on the fly from the resident times -- one subtraction, one
// product, the library's sincos -- whitened by that recurrence and folded into running sums: no right-hand side is
// written to memory.  The whitened residual z_r (and z_1 of the constant column, with the offset) do not depend on the
// frequency; the caller forms them once per call with the forward pass of clr_batch_one_step_ahead and the walks read
// them per step.  Passes, lane = (problem, chunk), a block of FB frequencies per lane on grid.z:
//   1. bperiodogram_walk_kernel<.., false>  the chunk from a zero start: the 2 FB end offsets of g, J doubles each;
//   2. bsolve_prefix_kernel<J, false>       (unchanged) the chunks' start states, the 2 nf columns as right-hand sides,
//                                           with the factor's own chunk maps;
//   3. bperiodogram_walk_kernel<.., true>   the same walk from the start states: the sums cc, cs, ss, cr, sr (and c1, s1)
//                                           of z_x z_y / D in registers, one partial per (problem, frequency, chunk).
// The reduction over the chunks, in chunk order, and the small solve are mean_kernels.hip's (launch_periodogram_reduce):
// they do not depend on the width.  A frequency's arithmetic is the same sequence of operations in every slot of a block
// and a slot past the tile's end recomputes the tile's last frequency without writing: a (problem, frequency)'s bits depend
// on the plan's chunking and on nothing else.
#pragma once

namespace clr {

// frequencies per lane: 2 FB forward states of J doubles beside one slot in flight (tools/kernel_resources.py: no scratch)
constexpr int bperiodogram_block(int J) { return J <= 2 ? 8 : (J <= 4 ? 4 : 2); }

constexpr int BPG_SUMS = 7;  // cc, cs, ss, cr, sr, c1, s1 (the last two with the offset only)

struct BPeriodogramParams {
  int lean;             // the factor holds W, D only
  int nf;               // frequencies of this tile
  int offset;           // the columns are (1, c, s): zT holds z_1 behind z_r
  const double* omega;  // frequency f of the tile for problem b at omega[b * omega_stride + f] (omega_stride 0: shared)
  long omega_stride;
  double t_ref;
  const double* zT;     // [B][1 + offset][L][nchunk] z_r (, z_1), chunk-interleaved
  double* M;            // [B][nchunk][J*J] the factor's chunk maps (formed)
  double* off;          // [B][2 nf][nchunk][J] forward chunk offsets; right-hand side 2 f: cos, 2 f + 1: sin
  double* starts;       // [B][2 nf][nchunk][J] forward chunk start states
  double* part;         // [B][nf][nchunk][BPG_SUMS] the chunks' sums
};

template <int JR, int JC, bool LEAN, bool FAST, int FB, bool SUMS>
__global__ void __launch_bounds__(64) bperiodogram_walk_kernel(const BatchParams P, const BPeriodogramParams S) {
  constexpr int J = JR + 2 * JC;
  const int b = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x, f0 = blockIdx.z * FB;
  if (c >= P.nchunk) return;
  const auto F = make_slots<JR, JC, LEAN, FAST>(P, b, c);
  const DirectSeries ts = bpvrec_times(P, b, c);
  const int nz = 1 + S.offset;
  const long cells = (long)P.L * P.nchunk;
  const double* zr = S.zT + (long)b * nz * cells + c;
  const double* z1 = zr + cells;  // (read with the offset only)
  const long rhs0 = (long)b * 2 * S.nf;
  double om[FB], gc[FB][J], gs[FB][J], acc[SUMS ? FB : 1][BPG_SUMS];
#pragma unroll
  for (int k = 0; k < FB; ++k) {
    const int f = (f0 + k < S.nf) ? f0 + k : S.nf - 1;  // (past the tile's end: the last frequency again, never written)
    om[k] = S.omega[(long)b * S.omega_stride + f];
    if (SUMS) {
      const double* sc = S.starts + ((rhs0 + 2 * f) * P.nchunk + c) * J;
      const double* ss = S.starts + ((rhs0 + 2 * f + 1) * P.nchunk + c) * J;
#pragma unroll
      for (int j = 0; j < J; ++j) { gc[k][j] = sc[j]; gs[k][j] = ss[j]; }
#pragma unroll
      for (int i = 0; i < BPG_SUMS; ++i) acc[k][i] = 0.0;
    } else {
#pragma unroll
      for (int j = 0; j < J; ++j) { gc[k][j] = 0.0; gs[k][j] = 0.0; }
    }
  }
  const int n0 = c * P.L;
  const int last = (P.N - n0 < P.L) ? P.N - n0 : P.L;  // samples of this chunk inside the series
  double nph[J], nuu[J], nww[J], nd, nt, nzr = 0.0, nz1 = 0.0;
  F.get(0, nph, nuu, nww, &nd);
  nt = ts.t(0);
  if (SUMS) {
    nzr = zr[0];
    if (S.offset) nz1 = z1[0];
  }
  for (int i = 0; i < last; ++i) {
    const int n = n0 + i;
    double ph[J], uu[J], ww[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { ph[j] = nph[j]; uu[j] = nuu[j]; ww[j] = nww[j]; }
    const double d = nd, tn = nt, zrn = nzr, z1n = nz1;
    if (i + 1 < last) {  // (the next step's slot, one step ahead)
      F.get(i + 1, nph, nuu, nww, &nd);
      nt = ts.t(i + 1);
      if (SUMS) {
        nzr = zr[(long)(i + 1) * P.nchunk];
        if (S.offset) nz1 = z1[(long)(i + 1) * P.nchunk];
      }
    }
    const double tau = tn - S.t_ref;
    const double id = SUMS ? 1.0 / d : 0.0;
    const bool tail = (n == P.N - 1);  // the last sample: no successor, the state it would produce is never read
#pragma unroll
    for (int k = 0; k < FB; ++k) {
      double sn, cs;
      sincos(om[k] * tau, &sn, &cs);
      double ugc = 0.0, ugs = 0.0;
#pragma unroll
      for (int j = 0; j < J; ++j) { ugc = fma(uu[j], gc[k][j], ugc); ugs = fma(uu[j], gs[k][j], ugs); }
      const double zc = cs - ugc, zs = sn - ugs;
      if (SUMS) {
        const double cw = zc * id, sw = zs * id;
        acc[k][0] = fma(cw, zc, acc[k][0]);
        acc[k][1] = fma(cw, zs, acc[k][1]);
        acc[k][2] = fma(sw, zs, acc[k][2]);
        acc[k][3] = fma(cw, zrn, acc[k][3]);
        acc[k][4] = fma(sw, zrn, acc[k][4]);
        if (S.offset) {
          acc[k][5] = fma(cw, z1n, acc[k][5]);
          acc[k][6] = fma(sw, z1n, acc[k][6]);
        }
      }
      if (tail) {
#pragma unroll
        for (int j = 0; j < J; ++j) { gc[k][j] = 0.0; gs[k][j] = 0.0; }
      } else {
#pragma unroll
        for (int j = 0; j < J; ++j) {
          gc[k][j] = ph[j] * fma(ww[j], zc, gc[k][j]);
          gs[k][j] = ph[j] * fma(ww[j], zs, gs[k][j]);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < FB; ++k) {
    const int f = f0 + k;
    if (f >= S.nf) break;
    if (SUMS) {
      double* o = S.part + (((long)b * S.nf + f) * P.nchunk + c) * BPG_SUMS;
#pragma unroll
      for (int i = 0; i < BPG_SUMS; ++i) o[i] = acc[k][i];
    } else {
      double* oc = S.off + ((rhs0 + 2 * f) * P.nchunk + c) * J;
      double* os = S.off + ((rhs0 + 2 * f + 1) * P.nchunk + c) * J;
#pragma unroll
      for (int j = 0; j < J; ++j) { oc[j] = gc[k][j]; os[j] = gs[k][j]; }
    }
  }
}

}  // namespace clr
