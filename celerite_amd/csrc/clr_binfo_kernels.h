// celerite_amd/csrc/clr_binfo_kernels.h -- the information matrix of every problem of a narrow plan (clr_batch_information).
// Included from the middle of clr_batch_kernels.h, behind clr_grad_kernels.h (BatchParams, grad_series, grad_group in scope).
//
// With z = L^-1 r the one-step-ahead innovations and D their variances, loglike = -1/2 sum_n (log D_n + z_n^2 / D_n + log 2 pi),
// and for two directions i, j (the columns of clr_batch_grad, then the constant mean)
//     I[i][j] = sum_n  1/2 (d_i D_n / D_n)(d_j D_n / D_n) + (d_i z_n)(d_j z_n) / D_n            (scoring, Harvey 1989, 3.4)
// a Gram matrix of two numbers per sample and direction -- d_i D_n / (sqrt 2 D_n) and d_i z_n / sqrt D_n -- which the
// forward-mode tangent recurrence of clr_grad_core.h already carries (dD, dx of grad_chunk).  No second-order recurrence.
//
// After an evaluation by the scan (start state of every chunk in P.starts, route per problem in P.need_exact) and the
// riders of every gradient chunk (grad_riders_kernel):
//   info_chunk_kernel, pass 0   lane = chunk, blockIdx.z = direction group: the base recurrence and the group's two tangents
//                               from ZERO tangent states; the tangent state at the chunk's end        -> tan [B][chunk][M][TAN]
//   info_walk_kernel            thread = (problem, direction): walks the chunks as grad_combine does and leaves the TRUE
//                               tangent start state of every chunk in place of its record             -> tan
//   info_chunk_kernel, pass 1   the same lanes again from the true (S, f, dS, df): the two numbers of every sample and
//                               direction, chunk-interleaved (a wave's 64 lanes store 512 contiguous bytes per
//                               number and step); steps at or past the problem's length store zeros   -> rows [tile][M][2][C]
//   info_chunk_kernel, pass 2   the sequential form: problems the scan sent to the sequential recurrence (or every problem:
//                               seq_all) as ONE chunk of the row-major series from the zero state     -> rows
//   info_gram_kernel            workgroup = (slab of CLR_INFO_SLAB cells, problem): R R^T of the slab through LDS tiles, one
//                               thread per entry of the upper triangle, the cells in order            -> part [tile][slab][NP]
//   info_gram_finish_kernel     the slabs in order, both triangles from the one sum                    -> out [tile][M][M]
// The mean's direction (group GROUPS, kind 4) has dD = dS = 0 and d r = -1: dx_n = -1 - u_n . df_n.
// No atomics; the shape of every sum follows the chunking and the problem's own route alone, so a problem's bits depend on
// neither the batch, the tile nor a sharding.
#pragma once

#include "clr_grad_kernels.h"

namespace clr {

constexpr int CLR_INFO_SLAB = 8192;  // cells of a problem's 2 C per workgroup of info_gram_kernel (fixed: see above)
constexpr int CLR_INFO_TILE = 128;   // ... staged through LDS at a time
constexpr int CLR_INFO_MAX_M = 18;   // 1 + 2 J_real + 4 J_comp <= 17 directions at width 8, and the mean

struct BInfoParams {
  int M;             // directions: 1 + 2 J_real + 4 J_comp (+ 1 with the mean, the last one)
  int mean;          // 1: the mean's direction is carried
  int b0, nb;        // the tile: problems b0 .. b0 + nb - 1 (passes 1, 2 and the Gram kernels)
  int seq_all;       // every problem takes the sequential form
  double* tan;       // [B][g_nchunk][M][TAN]
  double* rows;      // [nb][M][2][C]
  long C;            // cells per number and direction: g_nchunk * g_m * L (chunked and sequential form alike)
  double* part;      // [nb][nslab][NP]
  double* out;       // [nb][M][M]
  int nslab;
  // the row-major series (the sequential form reads them whatever the chunked passes read)
  const double *rm_t, *rm_diag, *rm_y;
  long rm_t_stride, rm_diag_stride, rm_y_stride;
};

// One chunk, one group (grad_chunk with the tangent states handed in and out and the per-sample numbers stored):
// tin0 / tin1: the two directions' tangent start states (dS[SZ] df[J], the problem's row order; null: zero);
// tout0 / tout1 (may be null): their states after the chunk; r0 / r1 (may be null): where local step i stores
// dD / (sqrt 2 D) at [i * rstep] and dx / sqrt D at [half + i * rstep].
template <int JR, int JC, bool FAST, class Src>
__device__ __forceinline__ void info_chunk(const double* a_real, const double* c_real, const double* a_comp,
                                           const double* b_comp, const double* c_comp, const double* d_comp, double jitter,
                                           Src& src, int L, int N, int n0, const double* start, int group, const double* tin0,
                                           const double* tin1, double* tout0, double* tout1, double* r0, double* r1,
                                           long rstep, long half) {
  using Sh = GradShape<JR, JC>;
  constexpr int J = Sh::J, SZ = Sh::SZ, M = JR + JC;
  constexpr int RR = JR > 0 ? JR - 1 : 0;
  constexpr int CR = JC > 0 ? J - 2 : 0;
  constexpr int CB = JC > 0 ? J - 1 : 0;
  int kind, term, q0, q1;
  if (group < Sh::GROUPS) grad_group<JR, JC>(group, &kind, &term, &q0, &q1);
  else { kind = 4; term = 0; q0 = Sh::NG; q1 = -1; }

  Problem<JR, JC> p;
  int perm[J];
  {
    const int sr = kind == 1 ? term : JR - 1, sc = (kind == 2 || kind == 3) ? term : JC - 1;
    p.sum_ar = 0.0;
    p.sum_ac = 0.0;
    CLR_UNROLL
    for (int j = 0; j < JR; ++j) {
      const int o = j == JR - 1 ? sr : (j == sr ? JR - 1 : j);
      p.ar[j] = a_real[o];
      p.cr[j] = c_real[o];
      perm[j] = o;
    }
    CLR_UNROLL
    for (int j = 0; j < JC; ++j) {
      const int o = j == JC - 1 ? sc : (j == sc ? JC - 1 : j);
      p.ac[j] = a_comp[o];
      p.bc[j] = b_comp[o];
      p.cc[j] = c_comp[o];
      p.dc[j] = d_comp[o];
      perm[JR + 2 * j] = JR + 2 * o;
      perm[JR + 2 * j + 1] = JR + 2 * o + 1;
    }
    CLR_UNROLL
    for (int j = 0; j < JR; ++j) p.sum_ar += a_real[j];
    CLR_UNROLL
    for (int j = 0; j < JC; ++j) p.sum_ac += a_comp[j];
    p.jitter = jitter;
  }

  double S[SZ], f[J], dS[2][SZ], df[2][J];
  CLR_UNROLL
  for (int j = 0; j < J; ++j) {
    CLR_UNROLL
    for (int k = 0; k <= j; ++k) {
      const int a = perm[k], b = perm[j];
      const int at = a <= b ? a + b * (b + 1) / 2 : b + a * (a + 1) / 2;
      S[tri(k, j)] = start ? start[at] : 0.0;
      dS[0][tri(k, j)] = tin0 ? tin0[at] : 0.0;
      dS[1][tri(k, j)] = tin1 ? tin1[at] : 0.0;
    }
    f[j] = start ? start[SZ + perm[j]] : 0.0;
    df[0][j] = tin0 ? tin0[SZ + perm[j]] : 0.0;
    df[1][j] = tin1 ? tin1[SZ + perm[j]] : 0.0;
  }

  src.prologue();
  double tn = src.t(0);
  double t_next = src.t(1);
  double diag_n = src.diag(0), y_n = src.y(0);
  for (int i = 0; i < L; ++i) {
    src.step_begin(i);
    const bool valid = n0 + i < N;
    const double t_cur_next = t_next, diag_cur = diag_n, y_cur = y_n;
    if (i + 1 < L) {
      t_next = src.t(i + 2);
      diag_n = src.diag(i + 1);
      y_n = src.y(i + 1);
    }
    const double dt = t_cur_next - tn;

    // ---- base step up to w, x ----
    double u[J], v[J];
    features_uv<JR, JC, FAST>(p, tn, u, v);
    double q[J];
    CLR_UNROLL
    for (int j = 0; j < J; ++j) {
      double acc = 0.0;
      CLR_UNROLL
      for (int k = 0; k < J; ++k) acc += S[sym(k, j)] * u[k];
      q[j] = acc;
    }
    double s = 0.0, uf = 0.0;
    CLR_UNROLL
    for (int j = 0; j < J; ++j) { s += u[j] * q[j]; uf += u[j] * f[j]; }
    const double D = p.diagonal(diag_cur) - s;
    const double invD = 1.0 / D;
    const double x = y_cur - uf;
    double z[J], w[J];
    CLR_UNROLL
    for (int j = 0; j < J; ++j) {
      z[j] = v[j] - q[j];
      w[j] = z[j] * invD;
    }
    double phid[nz(M)], pp[nz(M * (M + 1) / 2)];
    features_phi_distinct<JR, JC>(p, dt, phid);
    CLR_UNROLL
    for (int b = 0; b < M; ++b) {
      CLR_UNROLL
      for (int a = 0; a <= b; ++a) pp[tri(a, b)] = phid[a] * phid[b];
    }
    // (formed as (dD / D) / sqrt 2 and dx / sqrt D, never through D^2: a padded tail's D = 1e300 must not overflow)
    const double sa = 0.70710678118654752440 * invD, sb = sqrt(invD);

    // ---- the two tangents: everything that reads the state BEFORE this step ----
    CLR_UNROLL
    for (int e = 0; e < 2; ++e) {
      double da = 0.0, duA = 0.0, duB = 0.0, dvA = 0.0, dvB = 0.0, dy = 0.0;
      if (kind == 0) {
        da = 1.0;
      } else if (kind == 1) {
        if (e == 0) { da = 1.0; duA = 1.0; }
      } else if (kind == 2) {
        if (e == 0) { da = 1.0; duA = v[CR]; duB = v[CB]; }
        else { duA = v[CB]; duB = -v[CR]; }
      } else if (kind == 3) {
        if (e == 1) {
          duA = -tn * u[CB]; duB = tn * u[CR];
          dvA = -tn * v[CB]; dvB = tn * v[CR];
        }
      } else if (e == 0) {
        dy = -1.0;  // the constant mean: r = y - mu
      }
      double dq[J];
      CLR_UNROLL
      for (int j = 0; j < J; ++j) {
        double acc = 0.0;
        CLR_UNROLL
        for (int k = 0; k < J; ++k) acc += dS[e][sym(k, j)] * u[k];
        dq[j] = acc;
      }
      double duq = 0.0, duf = 0.0;
      if (kind == 1) {
        if (JR > 0) { grad_add_col<J, RR>(S, duA, dq); duq = duA * q[RR]; duf = duA * f[RR]; }
      } else if (kind == 2 || kind == 3) {
        if (JC > 0) {
          grad_add_col<J, CR>(S, duA, dq);
          grad_add_col<J, CB>(S, duB, dq);
          duq = duA * q[CR] + duB * q[CB];
          duf = duA * f[CR] + duB * f[CB];
        }
      }
      double ds = duq, dx = duf;
      CLR_UNROLL
      for (int j = 0; j < J; ++j) { ds += u[j] * dq[j]; dx += u[j] * df[e][j]; }
      dx = dy - dx;
      const double dD = da - ds;
      double* r = e == 0 ? r0 : r1;
      if (r) {
        r[(long)i * rstep] = valid ? dD * sa : 0.0;
        r[half + (long)i * rstep] = valid ? dx * sb : 0.0;
      }
      double dz[J], dw[J];
      CLR_UNROLL
      for (int j = 0; j < J; ++j) dz[j] = -dq[j];
      if (kind == 3 && JC > 0) { dz[CR] += dvA; dz[CB] += dvB; }
      CLR_UNROLL
      for (int j = 0; j < J; ++j) dw[j] = (dz[j] - w[j] * dD) * invD;
      CLR_UNROLL
      for (int j = 0; j < J; ++j) {
        CLR_UNROLL
        for (int k = 0; k <= j; ++k)
          dS[e][tri(k, j)] = pp[tri(phi_index<JR>(k), phi_index<JR>(j))] *
                             fma(dz[k], w[j], fma(z[k], dw[j], dS[e][tri(k, j)]));
        df[e][j] = phid[phi_index<JR>(j)] * (df[e][j] + fma(dw[j], x, w[j] * dx));
      }
    }

    // ---- base update ----
    CLR_UNROLL
    for (int j = 0; j < J; ++j) f[j] = phid[phi_index<JR>(j)] * (f[j] + w[j] * x);
    CLR_UNROLL
    for (int j = 0; j < J; ++j) {
      CLR_UNROLL
      for (int k = 0; k <= j; ++k)
        S[tri(k, j)] = pp[tri(phi_index<JR>(k), phi_index<JR>(j))] * fma(z[k], w[j], S[tri(k, j)]);
    }

    // ---- d Phi (grad_chunk): d phi / dc = -dt phi on the term's rows ----
    if (kind == 1) {
      if (JR > 0) {
        CLR_UNROLL
        for (int k = 0; k < J; ++k) dS[1][sym(RR, k)] = fma(k == RR ? -2.0 * dt : -dt, S[sym(RR, k)], dS[1][sym(RR, k)]);
        df[1][RR] = fma(-dt, f[RR], df[1][RR]);
      }
    } else if (kind == 3) {
      if (JC > 0) {
        CLR_UNROLL
        for (int k = 0; k < CR; ++k) {
          dS[0][sym(CR, k)] = fma(-dt, S[sym(CR, k)], dS[0][sym(CR, k)]);
          dS[0][sym(CB, k)] = fma(-dt, S[sym(CB, k)], dS[0][sym(CB, k)]);
        }
        dS[0][tri(CR, CR)] = fma(-2.0 * dt, S[tri(CR, CR)], dS[0][tri(CR, CR)]);
        dS[0][tri(CR, CB)] = fma(-2.0 * dt, S[tri(CR, CB)], dS[0][tri(CR, CB)]);
        dS[0][tri(CB, CB)] = fma(-2.0 * dt, S[tri(CB, CB)], dS[0][tri(CB, CB)]);
        df[0][CR] = fma(-dt, f[CR], df[0][CR]);
        df[0][CB] = fma(-dt, f[CB], df[0][CB]);
      }
    }
    tn = t_cur_next;
    src.step_end(i);
  }

  CLR_UNROLL
  for (int e = 0; e < 2; ++e) {
    double* o = e == 0 ? tout0 : tout1;
    if (!o) continue;
    CLR_UNROLL
    for (int j = 0; j < J; ++j) {
      CLR_UNROLL
      for (int k = 0; k <= j; ++k) {
        const int a = perm[k], b = perm[j];
        o[a <= b ? a + b * (b + 1) / 2 : b + a * (a + 1) / 2] = dS[e][tri(k, j)];
      }
      o[SZ + perm[j]] = df[e][j];
    }
  }
}

// pass 0: zero tangent starts -> tangent states at the chunks' ends; pass 1: true tangent starts -> rows (chunked route);
// pass 2: rows of the sequential form (lane 0 of a one-wave grid row: the whole row-major series as one chunk).
template <int JR, int JC, bool FAST>
__global__ void __launch_bounds__(64) info_chunk_kernel(const BatchParams P, const BInfoParams I, int pass) {
  using Wd = Widths<JR, JC>;
  using Sh = GradShape<JR, JC>;
  constexpr int TAN = Sh::SZ + Sh::J;
  const int bl = blockIdx.y, b = (pass == 0 ? 0 : I.b0) + bl;
  const bool seq = I.seq_all || P.need_exact[b] >= 2;  // (wave-uniform)
  if (seq != (pass == 2)) return;
  const int group = blockIdx.z;
  int q0, q1;
  if (group < Sh::GROUPS) { int kind, term; grad_group<JR, JC>(group, &kind, &term, &q0, &q1); }
  else { q0 = Sh::NG; q1 = -1; }
  const double *ar = P.a_real + (long)b * JR, *cr = P.c_real + (long)b * JR, *ac = P.a_comp + (long)b * JC,
               *bc = P.b_comp + (long)b * JC, *cc = P.c_comp + (long)b * JC, *dc = P.d_comp + (long)b * JC;
  double* rows = I.rows + (long)bl * I.M * 2 * I.C;
  if (pass == 2) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    DirectSeries src{I.rm_t + b * I.rm_t_stride, I.rm_diag + b * I.rm_diag_stride, I.rm_y + b * I.rm_y_stride,
                     1, (long)I.C, (int)I.C, (long)P.N};
    // (C >= N steps: those past the series store the zeros the Gram pass reads there)
    info_chunk<JR, JC, FAST>(ar, cr, ac, bc, cc, dc, P.jitter[b], src, (int)I.C, series_len(P, b), 0, nullptr, group,
                             nullptr, nullptr, nullptr, nullptr, rows + (long)q0 * 2 * I.C,
                             q1 >= 0 ? rows + (long)q1 * 2 * I.C : nullptr, 1, I.C);
    return;
  }
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= P.g_nchunk) return;
  DirectSeries src = grad_series(P, b, c);
  double* tan = I.tan + ((long)b * P.g_nchunk + c) * I.M * TAN;
  double *t0 = tan + (long)q0 * TAN, *t1 = q1 >= 0 ? tan + (long)q1 * TAN : nullptr;
  const double* start = c > 0 ? P.starts + ((long)b * P.nchunk + (long)c * P.g_m) * Wd::START : nullptr;
  if (pass == 0)
    info_chunk<JR, JC, FAST>(ar, cr, ac, bc, cc, dc, P.jitter[b], src, P.g_m * P.L, series_len(P, b), c * P.g_m * P.L, start,
                             group, nullptr, nullptr, t0, t1, nullptr, nullptr, 0, 0);
  else
    info_chunk<JR, JC, FAST>(ar, cr, ac, bc, cc, dc, P.jitter[b], src, P.g_m * P.L, series_len(P, b), c * P.g_m * P.L, start,
                             group, t0, t1, nullptr, nullptr, rows + (long)q0 * 2 * I.C + c,
                             q1 >= 0 ? rows + (long)q1 * 2 * I.C + c : nullptr, P.g_nchunk, I.C);
}

// One (problem, direction): walk the chunks (grad_combine's update) and overwrite every chunk's zero-start record with the
// tangent state the chunk truly starts from.
template <int J>
__global__ void __launch_bounds__(64) info_walk_kernel(const BatchParams P, const BInfoParams I) {
  constexpr int SZ = J * (J + 1) / 2, RID = J * J + J + SZ, TAN = SZ + J;
  const long idx = (long)blockIdx.x * 64 + threadIdx.x;
  if (idx >= (long)P.B * I.M) return;
  const int b = (int)(idx / I.M), q = (int)(idx % I.M);
  if (I.seq_all || P.need_exact[b] >= 2) return;
  double dS[SZ], df[J];
#pragma unroll
  for (int i = 0; i < SZ; ++i) dS[i] = 0.0;
#pragma unroll
  for (int i = 0; i < J; ++i) df[i] = 0.0;
  for (int c = 0; c < P.g_nchunk; ++c) {
    const double* R = P.g_riders + ((long)b * P.g_nchunk + c) * RID;
    double* G = I.tan + (((long)b * P.g_nchunk + c) * I.M + q) * TAN;
    const double *AA = R, *eta = R + J * J;
    double g[TAN];
#pragma unroll
    for (int i = 0; i < TAN; ++i) { g[i] = G[i]; G[i] = i < SZ ? dS[i] : df[i - SZ]; }
    if (c + 1 == P.g_nchunk) break;
    double h[J], T[J * J];
#pragma unroll
    for (int i = 0; i < J; ++i) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < J; ++k) a = fma(dS[sym(i, k)], eta[k], a);
      h[i] = df[i] - a;
    }
#pragma unroll
    for (int i = 0; i < J; ++i) {
      double a = g[SZ + i];
#pragma unroll
      for (int k = 0; k < J; ++k) a = fma(AA[i * J + k], h[k], a);
      df[i] = a;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < J; ++k) s = fma(AA[i * J + k], dS[sym(k, j)], s);
        T[i * J + j] = s;
      }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
      for (int i = 0; i <= j; ++i) {
        double s = g[tri(i, j)];
#pragma unroll
        for (int k = 0; k < J; ++k) s = fma(T[i * J + k], AA[j * J + k], s);
        dS[tri(i, j)] = s;
      }
    }
  }
}

// information_kernels.hip: R R^T of the tile's rows, slab by slab, then the slabs in order
void launch_info_gram(const BInfoParams& I, hipStream_t s);

}  // namespace clr
