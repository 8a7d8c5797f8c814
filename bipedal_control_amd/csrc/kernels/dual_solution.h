// The dual solution of the QP a sweep has solved (include/bpmpc.h "Dual solution"; restatement: tests/dual_solution_reference.py): the costates
// lambda_k = s_k + S_k dx_k and the minimum-norm multipliers of the state-input equality rows, with the two residuals that certify them (HIP only).
// Everything is read behind a value sweep: the materialised model, K, dx, du, S, s and the closed-loop [Acl | bcl] of the value function's terms
// table.  No sweep: one wave per node.
//   dual_node (one wave per node), on the FP64 matrix cores, the vectors as column nx as in value_function.h:
//       Ma = S+ [Acl | bcl] + [0 | s+]          G = [Hux | g0] = [P | r] + R [K | kappa] + B'Ma          g_u(dx) = Hux dx + g0
//   then the rank-deficient solve  [N | nu0] = -pinv(D') G  through the Gram matrix M = D D' (at most 16 x 16):
//       a diagonally pivoted Cholesky M = L L' that stops where the pivot falls below 1e-12 of the largest diagonal entry (L: nc x rank),
//       pinv(M) = L (L'L)^-2 L' with L'L factored by an unpivoted Cholesky, applied to D G, and one step of residual refinement
//       X <- X - pinv(M) D (G + D'X), which takes the squared condition number of the Gram route out of the result.
//   The solution lies in range(L) = range(D): the component of every column in null(D') is zero, which is what makes it the minimum-norm one.
// The padding of nx = 22 / 24 to the 32-wide tiles selects zeros in the wave; rows of D at and beyond nc are zeros selected in the wave too.
#pragma once
#include <hip/hip_runtime.h>

#include "../dual_kernels.h"
#include "value_function.h"      // value_masked, value_aug, kValueKS, value_terms_stride, LdsSwz, lds1, lds_wave_sync, time_segment

namespace bpmpc {

constexpr double kDualEigenvalueFloor = 1e-12;      // eigenvalues of D D' below this fraction of the largest count as zero (singular values: 1e-6)

template <int NJ>
struct DualNodeLds {
  using LS = LdsSwz<2>;
  static constexpr int KR = 4 * kValueKS, LD = 33;
  union {
    alignas(16) double Ka[LS::size(KR)];    // [K | kappa], zero beyond row nu and beyond column nx (in registers once the products begin)
    double Y[kDualRows][LD];                // later: the solve's intermediate vectors, a column per right-hand side
  };
  union {
    alignas(16) double Ma[LS::size(KR)];    // S+ [Acl | bcl] + [0 | s+]
    double Rho[KR][LD];                     // later: G + D'X of the refinement step
  };
  double G[KR][LD];                         // [Hux | g0], zero beyond row nu and beyond column nx
  double Dm[kDualRows][KR + 1];             // D, rows >= nc zero
  double M[kDualRows][kDualRows + 1];       // D D'
  double L[kDualRows][kDualRows + 1];       // its pivoted Cholesky factor, columns >= rank zero
  double T[kDualRows][kDualRows + 1];       // L'L
  double Tc[kDualRows][kDualRows + 1];      // its Cholesky factor (lower), the identity beyond rank
  double Tinv[kDualRows];                   // 1 / diagonal of Tc
  double W[kDualRows][LD];                  // D times the right-hand sides
  double X[kDualRows][LD];                  // [N | nu0]
  double dx[32], gu[32], nu[kDualRows];
};
static_assert(LdsSwz<2>::size(4 * kValueKS) == 4 * kValueKS * 33, "Rho lies over Ma");

__device__ __forceinline__ double dual_wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
  return v;
}

// One node (b, k) on one wave.  Nodes beyond the problem's grid, problems the sweep skipped and problems whose sweep failed are not touched.
template <int NJ>
__device__ __forceinline__ void dual_node(DualNodeLds<NJ>& w, const DualArgs& a, int b, int k) {
  constexpr int NX = 12 + NJ, NU = 12 + NJ, KS = kValueKS, KR = 4 * KS, TS = value_terms_stride(NX), NR = kDualRows, NC = NX + 1;
  using LS = LdsSwz<2>;
  static_assert(NX == NU && NC <= 32 && NX <= KR && NC <= kWave, "two block rows / columns, six k-steps, a lane per right-hand side");
  const int l = threadIdx.x, li = l & 15, lk = l >> 4;
  const size_t s = (size_t)b * a.N + k;
  const int info = a.n_info[s];
  if (!a.active[b] || info == 0) return;
  if (a.summary[(size_t)b * 4 + 3] != 0.0) return;      // the sweep failed: no policy, the rows stay (k_dual_summary sets status 2)
  const int n = a.g_nodes[a.p_grid[b]];
  const size_t xs = ((size_t)b * (a.N + 1) + k) * NX;
  const bool last = k + 1 == n;
  // ---- lambda_k = s_k + S_k dx_k (the terminal costate rides with the last node)
  const double dxl = value_masked(a.dx + xs, l < NX, l);
  if (l < 32) w.dx[l] = dxl;
  lds_wave_sync();
  {
    const double* Sk = a.S + xs * NX;
    double lam = value_masked(a.s + xs, l < NX, l);
    for (int c = 0; c < NX; ++c) lam += value_masked(Sk, l < NX, l * NX + c) * w.dx[c];
    if (l < NX) a.lambda[xs + l] = lam;
    if (last && l < NX) a.lambda[xs + NX + l] = 0.0;
  }
  double* oN = a.nu_gain + s * NR * NX;
  if (info & 1) {      // event node: no input, no rows
    for (int idx = l; idx < NR * NX; idx += kWave) oN[idx] = 0.0;
    if (l < NR) { a.nu0[s * NR + l] = 0.0; a.nu[s * NR + l] = 0.0; }
    if (l == 0) { a.residual[s] = 0.0; a.gain_residual[s] = 0.0; a.aux[2 * s] = 0.0; a.aux[2 * s + 1] = 0.0; a.rows[s] = 0; }
    return;
  }
  const double *B = a.B + s * NX * NU, *R = a.R + s * NU * NU, *P = a.P + s * NU * NX, *rv = a.r + s * NU, *K = a.K + s * NU * NX, *du = a.du + s * NU;
  const double *T = a.terms + s * TS, *tA = T, *tb = T + 2 * NX * NX;
  const double *Sn = a.S + (xs + NX) * NX, *sn = a.s + xs + NX;
  int nc = a.nc[s];
  nc = nc < 0 ? 0 : (nc > NR ? NR : nc);
  // ---- Ka = [K | kappa] to LDS, zero padded (as value_terms_node forms it); D to LDS, rows >= nc zero
  constexpr int KIT = (NU * NX + kWave - 1) / kWave, DIT = (NR * NU + kWave - 1) / kWave;
  double kv[KIT], dv[DIT];
#pragma unroll
  for (int it = 0; it < KIT; ++it) kv[it] = value_masked(K, l + it * kWave < NU * NX, l + it * kWave);
#pragma unroll
  for (int it = 0; it < DIT; ++it) {
    const int idx = l + it * kWave;
    dv[it] = value_masked(a.D + s * NR * NU, idx < NR * NU && idx / NU < nc, idx);
  }
  const double dul = value_masked(du, l < NU, l);
  for (int idx = l; idx < LS::size(KR); idx += kWave) w.Ka[idx] = 0.0;
  for (int idx = l; idx < NR * (KR + 1); idx += kWave) (&w.Dm[0][0])[idx] = 0.0;
  lds_wave_sync();
#pragma unroll
  for (int it = 0; it < KIT; ++it) {
    const int idx = l + it * kWave;
    if (idx < NU * NX) w.Ka[LS::ix(idx / NX, idx % NX)] = kv[it];
  }
#pragma unroll
  for (int it = 0; it < DIT; ++it) {
    const int idx = l + it * kWave;
    if (idx < NR * NU) w.Dm[idx / NU][idx % NU] = dv[it];
  }
  lds_wave_sync();
  if (l < NU) {
    double kap = dul;
    for (int j = 0; j < NX; ++j) kap -= w.Ka[LS::ix(l, j)] * w.dx[j];
    w.Ka[LS::ix(l, NX)] = kap;
  }
  lds_wave_sync();
  double kb[2][KS];      // Ka(4 ks + lk, 16 blk + li): the B operand of R Ka
#pragma unroll
  for (int blk = 0; blk < 2; ++blk)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) kb[blk][ks] = lds1(w.Ka[LS::ix(4 * ks + lk, 16 * blk + li)]);
  // ---- Ma = S+ [Acl | bcl] + [0 | s+]: S+ straight from memory into the A-operand registers, [Acl | bcl] from the terms table into the B operand
#pragma unroll
  for (int bi = 0; bi < 2; ++bi) {
    double aS[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int row = 16 * bi + li, kk = 4 * ks + lk;
      aS[ks] = value_masked(Sn, row < NX && kk < NX, row * NX + kk);
    }
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      v4d acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = 16 * bi + lk + 4 * r;
        acc[r] = value_masked(sn, rr < NX && 16 * bj + li == NX, rr);
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aS[ks], value_aug<NX>(tA, tb, 4 * ks + lk, 16 * bj + li), acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = 16 * bi + lk + 4 * r;
        if (rr < KR) w.Ma[LS::ix(rr, 16 * bj + li)] = acc[r];
      }
    }
  }
  lds_wave_sync();
  // ---- G = [P | r] + R Ka + B'Ma (row 16 bi + li of B' is column 16 bi + li of B)
#pragma unroll
  for (int bi = 0; bi < 2; ++bi) {
    double aR[KS], aB[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int row = 16 * bi + li, kk = 4 * ks + lk;
      aR[ks] = value_masked(R, row < NU && kk < NU, row * NU + kk);
      aB[ks] = value_masked(B, row < NU && kk < NX, kk * NU + row);
    }
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      v4d acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = value_aug<NX>(P, rv, 16 * bi + lk + 4 * r, 16 * bj + li);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aR[ks], kb[bj][ks], acc, 0, 0, 0);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aB[ks], lds1(w.Ma[LS::ix(4 * ks + lk, 16 * bj + li)]), acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = 16 * bi + lk + 4 * r;
        if (rr < KR) w.G[rr][16 * bj + li] = acc[r];
      }
    }
  }
  lds_wave_sync();
  // ---- g_u(dx_k) = Hux dx_k + g0; the Gram matrix M = D D'
  {
    const int u = l < NU ? l : 0;
    double g = w.G[u][NX];
    for (int c = 0; c < NX; ++c) g += w.G[u][c] * w.dx[c];
    if (l < 32) w.gu[l] = l < NU ? g : 0.0;
  }
  for (int idx = l; idx < NR * NR; idx += kWave) {
    const int i = idx >> 4, j = idx & 15;
    double acc = 0.0;
    for (int c = 0; c < NU; ++c) acc += w.Dm[i][c] * w.Dm[j][c];
    w.M[i][j] = acc;
    w.L[i][j] = 0.0;
    w.Tc[i][j] = i == j ? 1.0 : 0.0;
  }
  if (l < NR) w.Tinv[l] = 1.0;
  lds_wave_sync();
  // ---- diagonally pivoted Cholesky of M, lane i < 16 owns row i; stops at the threshold: rank = the number of steps taken
  int rank = 0;
  {
    double d = l < NR ? w.M[l & 15][l & 15] : -1.0;
    bool done = l >= NR;
    const double floor_ = kDualEigenvalueFloor * dual_wave_max(d);
    for (int j = 0; j < NR; ++j) {
      const double cand = done ? -1.0 : d;
      const double piv = dual_wave_max(cand);
      if (!(piv > floor_) || !(piv > 0.0)) break;      // (the same value in every lane)
      const unsigned long long hit = __ballot(!done && cand == piv);
      const int p = __ffsll((long long)hit) - 1;
      const double root = sqrt(piv);
      if (l < NR) {
        double v = w.M[l][p];
        for (int t = 0; t < j; ++t) v -= w.L[l][t] * w.L[p][t];
        const double lv = done ? 0.0 : (l == p ? root : v / root);
        w.L[l][j] = lv;
        d -= lv * lv;
        if (l == p) done = true;
      }
      ++rank;
      lds_wave_sync();
    }
  }
  // ---- T = L'L and its Cholesky factor (rank x rank, positive definite: no pivoting)
  for (int idx = l; idx < NR * NR; idx += kWave) {
    const int i = idx >> 4, j = idx & 15;
    double acc = 0.0;
    for (int c = 0; c < NR; ++c) acc += w.L[c][i] * w.L[c][j];
    w.T[i][j] = acc;
  }
  lds_wave_sync();
  for (int j = 0; j < rank; ++j) {
    double dj = w.T[j][j];
    for (int t = 0; t < j; ++t) dj -= w.Tc[j][t] * w.Tc[j][t];
    const double root = sqrt(dj);
    lds_wave_sync();                                     // every lane has read row j before its diagonal entry is written
    if (l >= j && l < rank) {
      double v = w.T[l][j];
      for (int t = 0; t < j; ++t) v -= w.Tc[l][t] * w.Tc[j][t];
      w.Tc[l][j] = l == j ? root : v / root;
      if (l == j) w.Tinv[j] = 1.0 / root;
    }
    lds_wave_sync();
  }
  // ---- X = -pinv(M) D G, then one refinement step with Rho = G + D'X: lane c <= nx owns right-hand side c
  for (int rep = 0; rep < 2; ++rep) {
    const double* rhs = rep == 0 ? &w.G[0][0] : &w.Rho[0][0];
    for (int idx = l; idx < NR * NC; idx += kWave) {
      const int i = idx / NC, c = idx % NC;
      double acc = 0.0;
      for (int u = 0; u < NU; ++u) acc += w.Dm[i][u] * rhs[u * DualNodeLds<NJ>::LD + c];
      w.W[i][c] = acc;
    }
    lds_wave_sync();
    if (l < NC) {      // the lane's column of Y holds z; loops of run-time length over LDS: nothing indexed in registers
#pragma nounroll
      for (int p = 0; p < rank; ++p) {
        double acc = 0.0;
#pragma nounroll
        for (int i = 0; i < NR; ++i) acc += w.L[i][p] * w.W[i][l];
        w.Y[p][l] = acc;
      }
#pragma nounroll
      for (int pass = 0; pass < 2; ++pass) {
#pragma nounroll
        for (int p = 0; p < rank; ++p) {                 // Tc z' = z
          double v = w.Y[p][l];
#pragma nounroll
          for (int t = 0; t < p; ++t) v -= w.Tc[p][t] * w.Y[t][l];
          w.Y[p][l] = v * w.Tinv[p];
        }
#pragma nounroll
        for (int p = rank - 1; p >= 0; --p) {            // Tc'z'' = z'
          double v = w.Y[p][l];
#pragma nounroll
          for (int t = p + 1; t < rank; ++t) v -= w.Tc[t][p] * w.Y[t][l];
          w.Y[p][l] = v * w.Tinv[p];
        }
      }
#pragma nounroll
      for (int i = 0; i < NR; ++i) {
        double acc = 0.0;
#pragma nounroll
        for (int p = 0; p < rank; ++p) acc += w.L[i][p] * w.Y[p][l];
        w.X[i][l] = (rep == 0 ? 0.0 : w.X[i][l]) - acc;
      }
    }
    lds_wave_sync();
    // Rho = G + D'X: after the first pass the right-hand side of the refinement, after the second the stationarity residual of the gain form
    for (int idx = l; idx < NU * NC; idx += kWave) {
      const int u = idx / NC, c = idx % NC;
      double acc = w.G[u][c];
      for (int i = 0; i < NR; ++i) acc += w.Dm[i][u] * w.X[i][c];
      w.Rho[u][c] = acc;
    }
    lds_wave_sync();
  }
  // ---- the multiplier at the solution, the two residuals and the node's maxima
  if (l < NR) {
    double v = w.X[l][NX];
    for (int c = 0; c < NX; ++c) v += w.X[l][c] * w.dx[c];
    w.nu[l] = l < nc ? v : 0.0;
  }
  lds_wave_sync();
  double res = 0.0, gnorm = 0.0, gres = 0.0, hux = 0.0;
  if (l < NU) {
    double v = w.gu[l];
    gnorm = fabs(v);
    for (int i = 0; i < NR; ++i) v += w.Dm[i][l] * w.nu[i];
    res = fabs(v);
  }
  for (int idx = l; idx < NU * NX; idx += kWave) {
    const int u = idx / NX, c = idx % NX;
    gres = fmax(gres, fabs(w.Rho[u][c]));
    hux = fmax(hux, fabs(w.G[u][c]));
  }
  res = dual_wave_max(res); gnorm = dual_wave_max(gnorm); gres = dual_wave_max(gres); hux = dual_wave_max(hux);
  for (int idx = l; idx < NR * NX; idx += kWave) {
    const int i = idx / NX, c = idx % NX;
    oN[idx] = i < nc ? w.X[i][c] : 0.0;
  }
  if (l < NR) {
    a.nu0[s * NR + l] = l < nc ? w.X[l][NX] : 0.0;
    a.nu[s * NR + l] = w.nu[l];
  }
  if (l == 0) { a.residual[s] = res; a.gain_residual[s] = gres; a.aux[2 * s] = gnorm; a.aux[2 * s + 1] = hux; a.rows[s] = nc; }
}

// The six maxima of a problem over its nodes, on one wave; status as the value function's.
template <int NJ>
__device__ __forceinline__ void dual_summary_problem(const DualArgs& a, int b) {
  constexpr int NX = 12 + NJ, NR = kDualRows;
  const int l = threadIdx.x;
  if (!a.active[b]) return;                                        // skipped by the sweep: rows, summary and status stay
  if (a.summary[(size_t)b * 4 + 3] != 0.0) {
    if (l == 0) a.status[b] = 2;
    return;
  }
  const int n = a.g_nodes[a.p_grid[b]];
  const size_t s0 = (size_t)b * a.N;
  double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = l; k < n; k += kWave) {
    m[0] = fmax(m[0], a.residual[s0 + k]);
    m[1] = fmax(m[1], a.aux[2 * (s0 + k)]);
    m[2] = fmax(m[2], a.gain_residual[s0 + k]);
    m[3] = fmax(m[3], a.aux[2 * (s0 + k) + 1]);
  }
  for (int idx = l; idx < n * NR; idx += kWave) m[4] = fmax(m[4], fabs(a.nu[s0 * NR + idx]));
  for (int idx = l; idx < (n + 1) * NX; idx += kWave) m[5] = fmax(m[5], fabs(a.lambda[(size_t)b * (a.N + 1) * NX + idx]));
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double v = dual_wave_max(m[i]);
    if (l == 0) a.summary_out[(size_t)b * 6 + i] = v;
  }
  if (l == 0) a.status[b] = 1;
}

// One query on one wave: the multipliers of problem b at (t, x) and the costate there (the value query's dfdx, the same arithmetic).
template <int NJ>
__device__ __forceinline__ void dual_query_wave(double* lds /* 32 doubles */, const DualQueryArgs& a, int b) {
  constexpr int NX = 12 + NJ, NR = kDualRows;
  const int l = threadIdx.x;
  const int N = a.N, grid = a.p_grid[b], n = a.g_nodes[grid];
  const double* tp = a.g_time + (size_t)grid * (N + 1);
  int j;
  double al;
  time_segment(tp, n + 1, a.t[b], &j, &al);
  const double be = 1.0 - al;
  const size_t n0 = (size_t)b * (N + 1) + j;
  const double *S0 = a.S + n0 * NX * NX, *S1 = S0 + NX * NX, *s0 = a.s + n0 * NX, *s1 = s0 + NX, *x0 = a.x_lin + n0 * NX, *x1 = x0 + NX;
  double* delta = lds;
  if (l < NX) delta[l] = a.x[(size_t)b * NX + l] - (al * x0[l] + be * x1[l]);
  lds_wave_sync();
  if (l < NX) {
    double Sd = 0.0;
    for (int c = 0; c < NX; ++c) Sd += (al * S0[l * NX + c] + be * S1[l * NX + c]) * delta[c];
    const double sl = al * s0[l] + be * s1[l];
    a.lambda[(size_t)b * NX + l] = sl + Sd;
  }
  const size_t node = (size_t)b * N + j;
  if (l < NR) {
    const double* Nn = a.nu_gain + (node * NR + l) * NX;
    double v = a.nu0[node * NR + l];
    for (int c = 0; c < NX; ++c) v += Nn[c] * delta[c];
    a.nu[(size_t)b * NR + l] = v;
  }
  if (l == 0) a.rows[b] = a.node_rows[node];
}

}  // namespace bpmpc
