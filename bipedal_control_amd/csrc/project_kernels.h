// The change of variables behind its (problem, node) mapping (kernels/project_mfma.h), shared by k_project.hip and its per-problem-weight
// twins of k_weights.hip: the kernels differ in where the constant part of Q / R comes from.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "launch.h"
#include "kernels/project_mfma.h"

namespace bpmpc {

// QD: Q as its diagonal Qd (Launch::weights_q_diagonal; kernel k_project_fast_qd), else the dense Qc; Rc: the dense R.  Problem b reads them
// w_stride (Qc, Rc) / qd_stride (Qd) doubles further on: 0 for the model's weights, the row strides of the weight table (SolverWeights, solver.h)
template <int NJ, bool PK, bool WJ, bool QD>
__device__ __forceinline__ void project_fast_node(ProjectMfmaWorkspace<NJ, PK>& ws, const Launch& L, const double* Qc, const double* Qd, const double* Rc,
                                                  size_t w_stride, size_t qd_stride) {
  constexpr int NX = 12 + NJ, NU = 12 + NJ;
  const int b = blockIdx.x / L.klen, k = L.k0 + blockIdx.x % L.klen;
  if (!L.buf.active[b]) return;
  const int g = L.buf.p_grid[b];
  if (k >= L.buf.g_nodes[g]) return;
  const size_t s = (size_t)b * L.N + k;
  ProjectIn in;
  in.kind = L.buf.g_kind[(size_t)g * L.N + k];
  in.nc = L.buf.nc[s];
  in.C = L.buf.C + s * kMaxEqRows * NX; in.D = L.buf.D + s * kMaxEqRows * NU; in.e = L.buf.e + s * kMaxEqRows;
  in.A = L.buf.A + s * NX * NX; in.B = L.buf.B + s * NX * NU; in.b = L.buf.b + s * NX;
  in.Q = L.buf.Q + s * NX * NX; in.R = L.buf.R + s * NU * NU; in.P = L.buf.P + s * NU * NX; in.q = L.buf.q + s * NX; in.r = L.buf.r + s * NU;
  ProjectOut out;
  out.Px = L.buf.Px + s * NU * NX; out.Pu = L.buf.Pu + s * NU * NU; out.Pe = L.buf.Pe + s * NU; out.nut = L.buf.nut + s;
  out.At = L.buf.At + s * NX * NX; out.Bt = L.buf.Bt + s * NX * NU; out.bt = L.buf.bt + s * NX;
  out.Qt = L.buf.Qt + s * NX * NX; out.Rt = L.buf.Rt + s * NU * NU; out.Pt = L.buf.Pt + s * NU * NX; out.qt = L.buf.qt + s * NX;
  out.rt = L.buf.rt + s * NU;
  in.qrd = L.buf.qrd + s * kQrdStride;
  in.r_shift_at = L.ilqr ? kQrdRShift : 0;
  const double dt = L.buf.g_dt[(size_t)g * L.N + k];
  out.Wt = L.buf.Wt + s * PackedLq<NJ>::W_SIZE; out.Qp = L.buf.Qp + s * PackedLq<NJ>::Q_SIZE; out.Mt = L.buf.Mt + s * PackedLq<NJ>::M_SIZE;
  if constexpr (PK) { in.zero = L.buf.zero_page; in.Vt = L.buf.Vt + s * NJ * PackedLq<NJ>::WP; in.mode = L.buf.g_mode[(size_t)g * L.N + k] & 3; }   // written by the structured elimination
  else out.Vt = L.buf.Vt + s * NJ * PackedLq<NJ>::WP;   // FullPivLU elimination (Px, Pu, Pe): this kernel packs the joint rows for the sweep's loaders
  project_apply_mfma<NJ, PK, WJ, QD>(ws, in, out, dt, dt * (1.0 / L.model->robot_mass), Qc + b * w_stride, Qd + b * qd_stride, Rc + b * w_stride, L.reg_prim);   // as written by linearize_fast
}
}  // namespace bpmpc
