// The value function of the QP a sweep has solved (include/bpmpc.h "Value function"; restatement: tests/value_function_reference.py), on the FP64
// matrix cores (HIP only).  Under the sweep's policy du = K dx + kappa, kappa = du - K dx from the stored K, dx, du, the QP of a node is the
// closed-loop model
//     Acl = A + B K    bcl = b + B kappa    Qcl = Q + K'(R K + P) + P'K    qcl = q + K'(r + R kappa) + P'kappa    ccl = c + r'kappa + kappa'R kappa / 2
// and the cost-to-go V_k(dx) = v_k + s_k'dx + dx'S_k dx / 2 follows backward from V_n = 0:
//     S_k = Qcl + Acl'S+ Acl    s_k = qcl + Acl'(s+ + S+ bcl)    v_k = ccl + v+ + s+'bcl + bcl'S+ bcl / 2.
// The vectors ride along as an extra column, as in project_mfma.h and riccati_mfma.h:
//   value_terms_node (one wave per node)          Ka = [K | kappa]  (nu x (nx + 1))
//       [Acl | bcl] = [A | b] + B Ka       RK = [P | r] + R Ka       [Qcl | qcl ; . | g] = [Q | q ; 0] + Ka'RK + [P'Ka ; 0],   g = kappa'(R kappa + r)
//   value_sweep_problem (four waves per problem, one 16x16 block of the 32x32 tile each)          Aa = [Acl | bcl]  (nx x (nx + 1))
//       Ma = S+ Aa + [0 | s+]              [S | s ; . | g] = [Qcl | qcl ; 0] + Aa'Ma,               g = bcl'(S+ bcl + s+)
// nx = 22 / 24 is neither a multiple of 4 nor of 16: the contraction runs over 24 = 6 k-steps and the tiles are 32 wide; whatever lies beyond nx (nx + 1
// with the vector column) is a zero selected in the wave when the operand is formed, never a value read from memory.  No sparsity of Q, R or P is
// assumed.  LDS matrices are in the LdsSwz<2> layout (riccati_mfma.h), which serves the X Y and the X'Y operand patterns without bank conflicts.
#pragma once
#include <hip/hip_runtime.h>

#include "../value_kernels.h"
#include "riccati_mfma.h"   // v4d, LdsSwz, lds1, lds_barrier, lds_wave_sync
#include "rollout.h"        // time_segment

namespace bpmpc {

constexpr int kValueKS = 6;      // k-steps of 4: the contraction length nx <= 24

template <int NJ>
struct ValueTermsLds {
  using LS = LdsSwz<2>;
  alignas(16) double Ka[LS::size(4 * kValueKS)];   // [K | kappa], zero beyond row nu and beyond column nx
  alignas(16) double RK[LS::size(4 * kValueKS)];   // [R K + P | R kappa + r]
  double dx[32];
  double rk[32];                                   // r_i kappa_i
};

// value `p[idx]` where `ok`, an exact zero elsewhere; the load itself is unconditional (element 0 of the same array) - no branch around it
__device__ __forceinline__ double value_masked(const double* p, bool ok, int idx) {
  const double v = p[ok ? idx : 0];
  return ok ? v : 0.0;
}
// element (rr, col) of an [M | m] block in the accumulator layout: M [nx][nx] for col < nx, the vector m in column nx, zero beyond
template <int NX>
__device__ __forceinline__ double value_aug(const double* M, const double* m, int rr, int col) {
  const bool in_m = rr < NX && col < NX, in_v = rr < NX && col == NX;
  const double v = *(in_m ? M + rr * NX + col : (in_v ? m + rr : M));
  return (in_m || in_v) ? v : 0.0;
}

// One node (b, k) on one wave.  Nodes beyond the problem's grid and problems the sweep skipped are not touched.
template <int NJ>
__device__ __forceinline__ void value_terms_node(ValueTermsLds<NJ>& w, const ValueArgs& a, int b, int k) {
  constexpr int NX = 12 + NJ, NU = 12 + NJ, KS = kValueKS, KR = 4 * KS, TS = value_terms_stride(NX);
  using LS = LdsSwz<2>;
  static_assert(NX == NU && NX + 1 <= 32 && NX <= KR, "two block rows / columns, six k-steps");
  const int l = threadIdx.x, li = l & 15, lk = l >> 4;
  const size_t s = (size_t)b * a.N + k;
  const int info = a.n_info[s];
  if (!a.active[b] || info == 0) return;
  const int n = a.g_nodes[a.p_grid[b]];
  const size_t xs = ((size_t)b * (a.N + 1) + k) * NX;
  // the expansion point: the iterate before the line search of this iteration moves it (the terminal node rides with the last one).  Requested
  // here, stored behind everything else: a store in front of the node's loads would stand in their way (the memory counter retires in order)
  const bool last = k + 1 == n;
  const double x_here = value_masked(a.x + xs, l < NX, l), x_next = value_masked(a.x + xs + NX, last && l < NX, l);
  auto store_x_lin = [&]() {
    if (l < NX) a.x_lin[xs + l] = x_here;
    if (last && l < NX) a.x_lin[xs + NX + l] = x_next;
  };
  double* T = a.terms + s * TS;
  double *oA = T, *oQ = T + NX * NX, *ob = T + 2 * NX * NX, *oq = ob + NX, *oc = oq + NX;
  if (info & 1) {      // event node: identity jump with the stored b, no cost
    const double bl = value_masked(a.b + s * NX, l < NX, l);
    for (int idx = l; idx < NX * NX; idx += kWave) { oA[idx] = (idx / NX == idx % NX) ? 1.0 : 0.0; oQ[idx] = 0.0; }
    if (l < NX) { ob[l] = bl; oq[l] = 0.0; }
    if (l == 0) oc[0] = 0.0;
    store_x_lin();
    return;
  }
  const double *A = a.A + s * NX * NX, *B = a.B + s * NX * NU, *bv = a.b + s * NX, *Q = a.Q + s * NX * NX, *R = a.R + s * NU * NU, *P = a.P + s * NU * NX;
  const double *qv = a.q + s * NX, *rv = a.r + s * NU, *K = a.K + s * NU * NX, *du = a.du + s * NU;
  // ---- Ka = [K | kappa] to LDS, zero padded.  K, dx, du and r are requested in one go (one memory round trip for the eight pieces of K, not one
  //      each) and go to LDS when they are there
  constexpr int KIT = (NU * NX + kWave - 1) / kWave;
  double kv[KIT];
#pragma unroll
  for (int it = 0; it < KIT; ++it) kv[it] = value_masked(K, l + it * kWave < NU * NX, l + it * kWave);
  const double dxl = value_masked(a.dx + xs, l < NX, l), dul = value_masked(du, l < NU, l), rl = value_masked(rv, l < NU, l);
  for (int idx = l; idx < LS::size(KR); idx += kWave) w.Ka[idx] = 0.0;
  if (l < 32) w.dx[l] = dxl;
  lds_wave_sync();
#pragma unroll
  for (int it = 0; it < KIT; ++it) {
    const int idx = l + it * kWave;
    if (idx < NU * NX) w.Ka[LS::ix(idx / NX, idx % NX)] = kv[it];
  }
  lds_wave_sync();
  if (l < NU) {
    double kap = dul;
    for (int j = 0; j < NX; ++j) kap -= w.Ka[LS::ix(l, j)] * w.dx[j];
    w.Ka[LS::ix(l, NX)] = kap;
    w.rk[l] = rl * kap;
  }
  lds_wave_sync();
  // operand element Ka(4 ks + lk, 16 blk + li): the B operand of X Ka and the A operand of Ka'Y alike
  double kb[2][KS];
#pragma unroll
  for (int blk = 0; blk < 2; ++blk)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) kb[blk][ks] = lds1(w.Ka[LS::ix(4 * ks + lk, 16 * blk + li)]);
  // ---- [Acl | bcl] = [A | b] + B Ka: B straight from memory into the A-operand registers (row 16 bi + li, k = 4 ks + lk)
#pragma unroll
  for (int bi = 0; bi < 2; ++bi) {
    double aB[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int row = 16 * bi + li, kk = 4 * ks + lk;
      aB[ks] = value_masked(B, row < NX && kk < NU, row * NU + kk);
    }
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      v4d acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = value_aug<NX>(A, bv, 16 * bi + lk + 4 * r, 16 * bj + li);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aB[ks], kb[bj][ks], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = 16 * bi + lk + 4 * r, col = 16 * bj + li;
        if (rr < NX && col < NX) oA[rr * NX + col] = acc[r];
        if (rr < NX && col == NX) ob[rr] = acc[r];
      }
    }
  }
  // ---- RK = [P | r] + R Ka -> LDS (rows >= nu are exact zeros)
#pragma unroll
  for (int bi = 0; bi < 2; ++bi) {
    double aR[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int row = 16 * bi + li, kk = 4 * ks + lk;
      aR[ks] = value_masked(R, row < NU && kk < NU, row * NU + kk);
    }
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      v4d acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = value_aug<NX>(P, rv, 16 * bi + lk + 4 * r, 16 * bj + li);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aR[ks], kb[bj][ks], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = 16 * bi + lk + 4 * r;
        if (rr < KR) w.RK[LS::ix(rr, 16 * bj + li)] = acc[r];
      }
    }
  }
  lds_wave_sync();
  // r'kappa, summed in index order by every lane (the same value in all of them)
  double rkap = 0.0;
  for (int i = 0; i < NU; ++i) rkap += w.rk[i];
  const double c0 = a.c[s];
  // ---- [Qcl | qcl ; . | g] = [Q | q ; 0] + Ka'RK + [P'Ka ; 0]: P' straight from memory (row 16 bi + li of P' is column 16 bi + li of P)
#pragma unroll
  for (int bi = 0; bi < 2; ++bi) {
    double aP[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int row = 16 * bi + li, kk = 4 * ks + lk;
      aP[ks] = value_masked(P, row < NX && kk < NU, kk * NX + row);
    }
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      v4d acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = value_aug<NX>(Q, qv, 16 * bi + lk + 4 * r, 16 * bj + li);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(kb[bi][ks], lds1(w.RK[LS::ix(4 * ks + lk, 16 * bj + li)]), acc, 0, 0, 0);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aP[ks], kb[bj][ks], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = 16 * bi + lk + 4 * r, col = 16 * bj + li;
        if (rr < NX && col < NX) oQ[rr * NX + col] = acc[r];
        if (rr < NX && col == NX) oq[rr] = acc[r];
        if (rr == NX && col == NX) oc[0] = c0 + 0.5 * (acc[r] + rkap);      // c + r'kappa + kappa'R kappa / 2 from g = kappa'R kappa + kappa'r
      }
    }
  }
  store_x_lin();
}

template <int NJ>
struct ValueSweepLds {
  using LS = LdsSwz<2>;
  alignas(16) double Sp[LS::size(32)];             // S+, zero beyond nx
  alignas(16) double Ma[LS::size(4 * kValueKS)];   // [S+ Acl | S+ bcl + s+]
  alignas(16) double T[LS::size(32)];              // the stage's result before the symmetrisation
  alignas(16) double sv[32];                       // s+, zero beyond nx
};

// what a wave holds of a stage: its two operand slices of Aa = [Acl | bcl], its block of [Qcl | qcl ; 0], ccl
struct ValueStage {
  double aB[kValueKS], aA[kValueKS];
  v4d cQ;
  double ccl;
};
template <int NX>
__device__ __forceinline__ ValueStage value_load_stage(const double* T, int bi, int bj, int li, int lk) {
  const double *tA = T, *tQ = T + NX * NX, *tb = T + 2 * NX * NX, *tq = tb + NX;
  ValueStage st;
#pragma unroll
  for (int ks = 0; ks < kValueKS; ++ks) {
    const int kk = 4 * ks + lk;      // Aa(kk, col): the B operand of S+ Aa (col in block column bj), the A operand of Aa'Ma (col in block row bi)
    st.aB[ks] = value_aug<NX>(tA, tb, kk, 16 * bj + li);
    st.aA[ks] = value_aug<NX>(tA, tb, kk, 16 * bi + li);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) st.cQ[r] = value_aug<NX>(tQ, tq, 16 * bi + lk + 4 * r, 16 * bj + li);
  st.ccl = tq[NX];
  return st;
}

// One problem on four waves, backward from its own last node.  Wave w owns block (w / 2, w % 2) of the 32x32 tile.
template <int NJ>
__device__ __forceinline__ void value_sweep_problem(ValueSweepLds<NJ>& w, const ValueArgs& a, int b) {
  constexpr int NX = 12 + NJ, KS = kValueKS, KR = 4 * KS, TS = value_terms_stride(NX);
  using LS = LdsSwz<2>;
  const int tid = threadIdx.x, wv = tid >> 6, bi = wv >> 1, bj = wv & 1, l = tid & 63, li = l & 15, lk = l >> 4;
  if (!a.active[b]) return;                                        // skipped by the sweep: rows and status stay
  if (a.summary[(size_t)b * 4 + 3] != 0.0) {                       // the sweep failed: its gains describe no policy; the rows stay
    if (tid == 0) a.status[b] = 2;
    return;
  }
  const int n = a.g_nodes[a.p_grid[b]];
  const double* terms = a.terms + (size_t)b * a.N * TS;
  double* oS = a.S + (size_t)b * (a.N + 1) * NX * NX;
  double* os = a.s + (size_t)b * (a.N + 1) * NX;
  double* ov = a.v + (size_t)b * (a.N + 1);
  ValueStage cur = value_load_stage<NX>(terms + (size_t)(n > 0 ? n - 1 : 0) * TS, bi, bj, li, lk);
  for (int idx = tid; idx < LS::size(32); idx += 256) { w.Sp[idx] = 0.0; w.T[idx] = 0.0; }
  for (int idx = tid; idx < LS::size(KR); idx += 256) w.Ma[idx] = 0.0;
  if (tid < 32) w.sv[tid] = 0.0;
  // V_n = 0
  const double2 zz = make_double2(0.0, 0.0);
  for (int idx = tid; idx < NX * NX / 2; idx += 256) reinterpret_cast<double2*>(oS + (size_t)n * NX * NX)[idx] = zz;
  if (tid < NX / 2) reinterpret_cast<double2*>(os + (size_t)n * NX)[tid] = zz;
  if (tid == 0) ov[n] = 0.0;
  double v = 0.0;                                                  // v+ (followed by the one lane that owns element (nx, nx))
  lds_barrier();
  for (int k = n - 1; k >= 0; --k) {
    // the next stage's operands do not depend on S: requested now, they travel under the two dependent products of this stage
    const ValueStage nxt = value_load_stage<NX>(terms + (size_t)(k > 0 ? k - 1 : 0) * TS, bi, bj, li, lk);
    const int col = 16 * bj + li;
    // ---- Ma = S+ Aa + [0 | s+]
    v4d m0, m1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = 16 * bi + lk + 4 * r;
      const double sp = w.sv[rr];
      m0[r] = col == NX ? sp : 0.0;                                // (sv is zero beyond nx)
    }
#pragma unroll
    for (int ks = 0; ks < KS; ks += 2) {                           // two accumulators: two half as long chains of dependent instructions
      m0 = __builtin_amdgcn_mfma_f64_16x16x4f64(lds1(w.Sp[LS::ix(16 * bi + li, 4 * ks + lk)]), cur.aB[ks], m0, 0, 0, 0);
      m1 = __builtin_amdgcn_mfma_f64_16x16x4f64(lds1(w.Sp[LS::ix(16 * bi + li, 4 * ks + 4 + lk)]), cur.aB[ks + 1], m1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = 16 * bi + lk + 4 * r;
      if (rr < KR) w.Ma[LS::ix(rr, col)] = m0[r] + m1[r];
    }
    // s+'bcl: the lanes of column nx hold bcl(4 ks + lk) as their B operand; the four partial sums meet in index order
    double dot = 0.0;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) dot += w.sv[4 * ks + lk] * cur.aB[ks];
    {
      const int src = (NX - 16) & 15;
      const double d0 = __shfl(dot, src), d1 = __shfl(dot, src + 16), d2 = __shfl(dot, src + 32), d3 = __shfl(dot, src + 48);
      dot = (d0 + d1) + (d2 + d3);
    }
    lds_barrier();
    // ---- [S | s ; . | g] = [Qcl | qcl ; 0] + Aa'Ma
    v4d t0 = cur.cQ, t1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < KS; ks += 2) {
      t0 = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.aA[ks], lds1(w.Ma[LS::ix(4 * ks + lk, col)]), t0, 0, 0, 0);
      t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.aA[ks + 1], lds1(w.Ma[LS::ix(4 * ks + 4 + lk, col)]), t1, 0, 0, 0);
    }
    const v4d t = t0 + t1;
#pragma unroll
    for (int r = 0; r < 4; ++r) w.T[LS::ix(16 * bi + lk + 4 * r, col)] = t[r];
    lds_barrier();
    // ---- S_k = (S + S') / 2 as computed, so that rounding cannot build up an asymmetry over the stages; s_k; v_k
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = 16 * bi + lk + 4 * r;
      if (rr < NX && col < NX) w.Sp[LS::ix(rr, col)] = 0.5 * (t[r] + w.T[LS::ix(col, rr)]);
      if (rr < NX && col == NX) w.sv[rr] = t[r];
      if (rr == NX && col == NX) {                                 // g = bcl'S+ bcl + bcl's+
        v = cur.ccl + v + 0.5 * (t[r] + dot);
        ov[k] = v;
      }
    }
    lds_barrier();
    // ---- 16-byte stores of the stage's rows from LDS (column pairs of a row are neighbours in the swizzled layout too)
    for (int idx = tid; idx < NX * NX / 2; idx += 256) {
      const int row = (2 * idx) / NX, c2 = (2 * idx) % NX;
      reinterpret_cast<double2*>(oS + (size_t)k * NX * NX)[idx] = *reinterpret_cast<const double2*>(&w.Sp[LS::ix(row, c2)]);
    }
    if (tid < NX / 2) reinterpret_cast<double2*>(os + (size_t)k * NX)[tid] = *reinterpret_cast<const double2*>(&w.sv[2 * tid]);
    cur = nxt;
  }
  if (tid == 0) a.status[b] = 1;
}

// One query on one wave: V(t, x) of problem b, its gradient and (dfdxx != nullptr) its Hessian.  t is clamped to the solution's span by the
// segment rule itself (time_segment: alpha = 1 before the first node, 0 behind the last one).
template <int NJ>
__device__ __forceinline__ void value_query_wave(double* lds /* 2 * 32 doubles */, const ValueQueryArgs& a, int b) {
  constexpr int NX = 12 + NJ;
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
  double* part = lds + 32;
  if (l < NX) delta[l] = a.x[(size_t)b * NX + l] - (al * x0[l] + be * x1[l]);
  lds_wave_sync();
  if (l < NX) {
    double Sd = 0.0;
    for (int c = 0; c < NX; ++c) Sd += (al * S0[l * NX + c] + be * S1[l * NX + c]) * delta[c];
    const double sl = al * s0[l] + be * s1[l];
    a.dfdx[(size_t)b * NX + l] = sl + Sd;
    part[l] = sl * delta[l] + 0.5 * delta[l] * Sd;
  }
  lds_wave_sync();
  if (l == 0) {
    double f = al * a.v[n0] + be * a.v[n0 + 1];
    for (int i = 0; i < NX; ++i) f += part[i];
    a.f[b] = f;
  }
  if (a.dfdxx)
    for (int idx = l; idx < NX * NX; idx += kWave) a.dfdxx[(size_t)b * NX * NX + idx] = al * S0[idx] + be * S1[idx];
}

}  // namespace bpmpc
