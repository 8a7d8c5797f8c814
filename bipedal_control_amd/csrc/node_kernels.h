// The per-node kernels of k_weights.hip (per-problem cost weights and cone parameters, bpmpc_solver_set_weights / bpmpc_solver_set_cone_params)
// behind their (problem, node) mappings, and the workgroup shapes they share with k_node.hip.  The three bodies restate what k_linearize_fast,
// k_trial_fast and k_ls_tail of k_node.hip do behind their mappings, with the cost weights and the cone parameters from the problem's rows
// instead of the model: linearize_fast.h's bodies do the work in both.  They are NOT shared
// with those kernels on purpose.  Routed through these functions with a null row, the kernels of k_node.hip computed the same but no longer
// compiled to the same instructions (21 of 150 functions moved; a kernel's bits follow the text of its translation unit, DESIGN.md "plant_stick"),
// and an untouched handle has to launch the parent's machine code: profiles/solver_weights_isa_check.txt.  A change to one side belongs on the other.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "launch.h"

namespace bpmpc {

constexpr int kTrialWaves = 4; // same for the value-only trial kernel (smaller per-node LDS: four waves, 8 waves per CU)
// wavefronts per workgroup of the linearisation kernel: they share one copy of the model block in LDS.  Four: 74.3 KB at nx = 22, 79.1 KB
// at nx = 24 (a wave serves four nodes of 4.2 KB each, packed lanes, LinFastCfg) - two workgroups, eight waves per CU
template <int NJ> constexpr int lin_waves() { return 4; }      // (five - ten waves per CU - was measured: 0.302 against 0.223 ms at batch 256; the kernel is not short of waves, experiments/LOG.md)
// the stage-one columns wait in LDS when two workgroups per CU (eight waves: the registers allow no more) still fit, else in HBM scratch
template <int NJ, bool CHAIN>
struct LinKernelLds {
  using C = LinFastCfg<NJ, true, CHAIN>;
  static constexpr bool PARK = sizeof(LinFastNodeLds<NJ, true, CHAIN, true>) * (lin_waves<NJ>() * C::NPW) + sizeof(LinFastShared<NJ>) <= 80 * 1024;
  using NL = LinFastNodeLds<NJ, true, CHAIN, PARK>;
};
constexpr int kTailThreads = 512;

// The lineariser behind its slot mapping: node slot `sub` of the workgroup holds node k of problem b (`valid`: it holds one; event_wg: the
// workgroup holds nothing but event nodes and needs no model block).  stage() fills `shared`; every thread of the workgroup calls.
// tl0: the workgroup's start (BPMPC_LIN_TIMELINE).
template <int NJ, bool MAT, bool CHAIN, bool ILQR, class NL, class Stage>
__device__ __forceinline__ void linearize_fast_slot(const Launch& L, LinFastShared<NJ>& shared, NL& lds, bool valid, int b, int k, bool event_wg, int g,
                                                    long long tl0, Stage&& stage) {
  using C = LinFastCfg<NJ, true, CHAIN>;
  // The memory round trips of a workgroup's start overlap: (1) the problem's flags and grid, the node's word (valid | mode | kind, written
  // by k_prepare) and the lane's entries of the iterate - addresses that only depend on the slot, loaded before anything is known about
  // the node - are in flight while (2) the model block is staged; (3) what hangs on the grid (dt, swing references) follows.
  const int act = L.buf.active[b];
  const size_t s0 = (size_t)b * L.N + k;
  const int info = L.buf.n_info[s0];
  constexpr int NXc = 12 + NJ;
  const double* xk = L.buf.x + ((size_t)b * (L.N + 1) + k) * NXc;
  // round 6: dt and the swing references come from the node record (n_aux, written by k_prepare), not from the grid tables behind p_grid[b]:
  // nothing a workgroup waits for before its barrier is more than one memory round trip away
  const LinFastPre pre = linearize_preload<C>(xk, xk + NXc, L.buf.u + s0 * NXc, L.buf.xref + s0 * NXc, g, L.buf.n_aux + s0 * kNodeAux);
  if (!event_wg) stage();
  NodeInputs in;
  in.kind = info & 1; in.mode = (info >> 1) & 3;                  // (the same facts as the grid tables hold, one hop earlier)
  in.dt = 0.0;                                                    // (the node record carries it: LinFastPre::aux)
  in.x = xk; in.xnext = xk + NXc; in.u = L.buf.u + s0 * NXc; in.xref = L.buf.xref + s0 * NXc; in.zref = nullptr; in.zdref = nullptr;
  __syncthreads();
#ifdef BPMPC_LIN_TIMELINE
  const long long tl1 = wall_clock64();
#endif
  valid = valid && act != 0 && info != 0;
  const size_t s = valid ? (size_t)b * L.N + k : 0;
  LinFastOut out;
  out.A = L.buf.A; out.B = L.buf.B; out.b = L.buf.b; out.Q = L.buf.Q; out.R = L.buf.R; out.q = L.buf.q; out.r = L.buf.r; out.c = L.buf.c;
  out.C = L.buf.C; out.D = L.buf.D; out.e = L.buf.e; out.perf = L.buf.perf; out.nc = L.buf.nc;
  out.park = L.buf.lin_park;
  out.dump = L.buf.lin_dump;
  out.qrd = L.buf.qrd;
  out.s = s;
  out.ilqr_shift = L.ilqr_shift;
#ifndef BPMPC_LIN_PROF_PROBLEM
#define BPMPC_LIN_PROF_PROBLEM 0     // the problem whose first 64 nodes report their phase cycles (-DBPMPC_LINFAST_PROFILE): 0 runs on an empty chip, batch / 2 in steady state
#endif
  out.prof = (valid && b == BPMPC_LIN_PROF_PROBLEM && k < 64) ? L.buf.rprof + 8 * k : nullptr;
  linearize_fast<NJ, MAT, C, NL, ILQR>(*L.model, shared, lds, valid, in, pre, out, g);      // g: lane inside the node's group
#ifdef BPMPC_LIN_TIMELINE
  if (threadIdx.x % kWave == 0 && blockIdx.x < 2048) {      // every wave: the workgroup's end is the latest of its waves
    double* t = L.buf.rprof + 16 * blockIdx.x + 4 * (threadIdx.x / kWave);
    unsigned hw; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    unsigned xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    t[0] = (double)tl0; t[1] = (double)tl1; t[2] = (double)wall_clock64(); t[3] = (double)(hw | ((unsigned long long)(xcc & 15) << 32));
  }
#else
  (void)tl0;
#endif
}

// The model block of ONE problem: the scalar and kinematic prefix from the model image, except the six cone scalars of LinFastScalars - three
// 16-byte pieces, from the problem's cone row `cone` (bpmpc_solver_set_cone_params) - and, COST, the tail - Q then R, the layout of a weight row's
// used part - from `row`.  All of it through the one flat 16-byte copy of load_shared_model: a piece picks its source ADDRESS, so every request is
// in flight before the first LDS store and the rows cost no round trip of their own.
template <int NT, int NJ, bool COST>
__device__ __forceinline__ void load_shared_model_rows(const DeviceModel& md, const double* cone, const double* row, LinFastShared<NJ, COST>& sh, int tid) {
  using S = LinFastShared<NJ, true>;
  static_assert(offsetof(S, Q) % 16 == 0 && offsetof(S, R) == offsetof(S, Q) + sizeof(S::Q) && sizeof(S) == offsetof(S, R) + sizeof(S::R),
                "the weights are the tail of the block, Q then R without a gap: the used part of a weight row");
  static_assert(sizeof(S::Q) + sizeof(S::R) <= kWeightRowStride * sizeof(double), "the tail fits a weight row");
  constexpr size_t kCone = offsetof(S, sc) + offsetof(LinFastScalars, friction);
  static_assert(kCone % 16 == 0 && kConeRowUsed % 2 == 0 && offsetof(LinFastScalars, cone_reg) == offsetof(LinFastScalars, friction) + 8 &&
                offsetof(LinFastScalars, cone_grip) == offsetof(LinFastScalars, friction) + 16 && offsetof(LinFastScalars, cone_shift) == offsetof(LinFastScalars, friction) + 24 &&
                offsetof(LinFastScalars, barrier_mu) == offsetof(LinFastScalars, friction) + 32 && offsetof(LinFastScalars, barrier_delta) == offsetof(LinFastScalars, friction) + 40,
                "the cone scalars are whole 16-byte pieces of the block in the order of a cone row");
  using S0 = LinFastShared<NJ, false>;
  static_assert(offsetof(S, sc) == offsetof(S0, sc), "one place in both blocks");
  constexpr int N16 = sizeof(LinFastShared<NJ, COST>) / 16, P16 = COST ? offsetof(S, Q) / 16 : N16, C16 = kCone / 16, CN = kConeRowUsed / 2, K = (N16 + NT - 1) / NT;
  static_assert(C16 + CN <= P16, "the cone scalars lie in the prefix");
  const uint4* img = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(&md) + kLinImageOffset);
  const uint4* w = reinterpret_cast<const uint4*>(row);
  const uint4* c = reinterpret_cast<const uint4*>(cone);
  uint4* dst = reinterpret_cast<uint4*>(&sh);
  uint4 v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int i = tid + k * NT, ii = i < N16 ? i : 0;
    const uint4* src = (COST && ii >= P16) ? w + (ii - P16) : img + ii;
    if (k * NT < C16 + CN) src = (ii >= C16 && ii < C16 + CN) ? c + (ii - C16) : src;      // (the first pass only, known when compiled)
    v[k] = *src;
  }
#pragma unroll
  for (int k = 0; k < K; ++k) asm volatile("" : "+v"(v[k].x), "+v"(v[k].y), "+v"(v[k].z), "+v"(v[k].w));   // all of them in flight before the first store
#pragma unroll
  for (int k = 0; k < K; ++k) { const int i = tid + k * NT; if (i < N16) dst[i] = v[k]; }
}

// The per-node tables of the trial kernel with the slot's own cone parameters behind them: the workgroups of that kernel run in launch order and
// straddle problems, so the shared model block is NOT one problem's and cone_terms reads the slot's copy instead (trial_fast, NL::kCone) - from
// LDS, as broadcasts at the one place the cone is evaluated, not from registers held across the evaluation (the kernel lives at three waves per
// SIMD without scratch).  pos_gain and robot_mass stay the model's.
template <int NJ, bool CHAIN>
struct TrialConeNodeLds : LinFastNodeLds<NJ, false, CHAIN> {
  static constexpr bool kCone = true;
  ConeScalars cone_sc;
};

// The value-only trial of one workgroup (k_trial_fast): its node slots in the launch-index mapping.  W: the weight table (the slot's lane
// group sums over the row of ITS problem, dense, from global memory as the model's dense weights).  Cone: the cone table; lane l of a slot
// requests entry l % 8 of its problem's row (entries 6 and 7 are zeros) together with its entries of the iterate.
template <int NJ, bool CHAIN, class NL>
__device__ __forceinline__ void trial_fast_rows_workgroup(const Launch& L, LinFastShared<NJ, false>& shared, NL* lds, const double* W, const double* Cone) {
  static_assert(NL::kCone, "the slots carry their cone parameters");
  using C = LinFastCfg<NJ, true, CHAIN>;
  constexpr int NX = 12 + NJ, NU = 12 + NJ, LPN = C::LPN, NPW = C::NPW;
  const int sub = threadIdx.x / LPN, g = threadIdx.x % LPN;
  const int widx = blockIdx.x * (kTrialWaves * NPW) + sub;
  {   // a workgroup whose problems have all finished their line search has nothing to evaluate (the second round: all but a few workgroups)
    const int total = L.batch * L.klen, w0 = blockIdx.x * (kTrialWaves * NPW), w1 = (w0 + kTrialWaves * NPW < total ? w0 + kTrialWaves * NPW : total) - 1;
    bool any = false;
    for (int pb = w0 / L.klen; pb <= w1 / L.klen; ++pb) any = any || L.buf.done[pb] == 0;
    if (!any) return;
  }
  bool valid = widx < L.batch * L.klen;
  const int b = valid ? widx / L.klen : 0, k = valid ? L.k0 + widx % L.klen : 0;
  const double* dx = L.buf.dx + ((size_t)b * (L.N + 1) + k) * NX;
  {
    // the node's facts and the lane's entries of iterate and step are requested before the model block is staged, as in k_linearize_fast
    // (line search 0.099 -> 0.096 ms at batch 256, 1.049 -> 0.975 at 4096)
    const int fin = L.buf.done[b];
    const double alpha = L.buf.alpha[b];
    const int info = L.buf.n_info[(size_t)b * L.N + k];
    const size_t s0 = (size_t)b * L.N + k;
    const double* xk = L.buf.x + ((size_t)b * (L.N + 1) + k) * NX;
    const TrialPre pre = trial_preload<C>(xk, xk + NX, L.buf.u + s0 * NU, L.buf.xref + s0 * NX, dx, dx + NX, L.buf.du + s0 * NU, g, L.buf.n_aux + s0 * kNodeAux);
    const double cone_pre = Cone[(size_t)b * kConeRowStride + g % kConeRowStride];
    load_shared_model<kTrialWaves * kWave>(*L.model, shared, threadIdx.x);
    NodeInputs in;                      // dt and the swing references come with the node record (TrialPre::x.aux)
    in.kind = info & 1; in.mode = (info >> 1) & 3; in.dt = 0.0;
    in.x = xk; in.xnext = xk + NX; in.u = L.buf.u + s0 * NU; in.xref = L.buf.xref + s0 * NX; in.zref = nullptr; in.zdref = nullptr;
    __syncthreads();
    valid = valid && fin == 0 && info != 0;
    const size_t s = valid ? s0 : 0;
    trial_fast<NJ, C, false, NL, false, true>(*L.model, shared, lds[sub], valid, in, alpha, dx, L.buf.du + s * NU, dx + NX, L.buf.trial_perf + s * 3, g, nullptr, &pre,
                                              W + (size_t)b * kWeightRowStride, cone_pre);
  }
}

// Back-tracking rounds after the first one of one problem (k_ls_tail).  W: as trial_fast_rows_workgroup.  Cone: the cone table; the workgroup
// serves one problem, whose row is overlaid on the model block as in the lineariser.
template <int NJ, bool CHAIN, class NL>
__device__ __forceinline__ void ls_tail_rows_problem(const Launch& L, int first_round, int max_trials, int pending, LinFastShared<NJ, false>& shared, NL* lds,
                                                double* partial, const double* W, const double* Cone) {
  using C = LinFastCfg<NJ, true, CHAIN>;
  constexpr int NX = 12 + NJ, NU = 12 + NJ, LPN = C::LPN, NPW = C::NPW, CHUNK = (kTailThreads / kWave) * NPW;
  const int b = blockIdx.x;
  if (L.buf.done[b]) return;
  volatile const int* done = L.buf.done + b;
  volatile const double* alpha = L.buf.alpha + b;
  if (pending) {
    // the trial of the last round that ran as a launch over all nodes has not been judged yet: that decision here, in the workgroup that would go on
    // with the problem anyway, instead of a launch of k_ls_decide in which all but a few workgroups only read a flag
    int bb = b;
    asm volatile("" : "+s"(bb));
    linesearch_decide<NJ, kTailThreads, true>(partial, problem_ls<NJ>(L, bb), L.ls);
    __threadfence();
    __syncthreads();
    if (*done) return;
  }
  load_shared_model_rows<kTailThreads, NJ, false>(*L.model, Cone + (size_t)b * kConeRowStride, nullptr, shared, threadIdx.x);
  __syncthreads();
  const int sub = threadIdx.x / LPN, g = threadIdx.x % LPN;
  const int n = L.buf.g_nodes[L.buf.p_grid[b]];
  for (int round = first_round; round < max_trials; ++round) {
    const double al = *alpha;
    for (int k0 = 0; k0 < n; k0 += CHUNK) {
      const int k = k0 + sub;
      const bool valid = k < n;
      const int kk = valid ? k : 0;
      const size_t s = (size_t)b * L.N + kk;
      const NodeInputs in = node_inputs<NJ>(L, b, kk);
      const double* dx = L.buf.dx + ((size_t)b * (L.N + 1) + kk) * NX;
      // the model block through an offset the compiler cannot see through: its scalar constants (LinFastScalars) are loop invariant, and hoisted
      // out of the round loop they lived in registers across the whole evaluation (256 registers + 20 .. 28 B of scratch)
      unsigned opaque = 0;
      asm volatile("" : "+v"(opaque));
      const auto& sh = *reinterpret_cast<const LinFastShared<NJ, false>*>(reinterpret_cast<const char*>(&shared) + opaque);
      // the problem's weight row likewise formed here, from scalars: a loop-invariant pointer kept in vector registers across the evaluation sent
      // the table-walk variant at nx = 24 (256 registers) to scratch memory
      int bw = b;
      asm volatile("" : "+s"(bw));
      const double* row = W + (size_t)bw * kWeightRowStride;
      trial_fast<NJ, C, false, NL, false, true>(*L.model, sh, lds[sub], valid, in, al, dx, L.buf.du + s * NU, dx + NX, L.buf.trial_perf + s * 3, g, nullptr, nullptr, row);
    }
    __threadfence();
    __syncthreads();
    // the problem's pointers are formed HERE, from an index the compiler cannot see through: hoisted out of the round loop they lived across the trial
    // evaluation, and at nx = 24 (256 registers) three of them went to scratch memory
    int bb = b;
    asm volatile("" : "+s"(bb));
    const ProblemLS p = problem_ls<NJ>(L, bb);
    linesearch_decide<NJ, kTailThreads, false>(partial, p, L.ls);
    __threadfence();
    __syncthreads();
    if (*done) break;
  }
}

}  // namespace bpmpc
