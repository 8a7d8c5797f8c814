// Device-resident gait schedules (bpmpc_gait_batch, include/bpmpc.h): one GaitSchedule per robot kept in HBM between setups, advanced
// by bpmpc_solver_setup_gaits with the semantics of SolverBase::preRun [OCS2-upstream, recalled] - the reference manager first
// (SwitchedModelReferenceManager.cpp:62-69: getModeSchedule(t0 - H, t0 + 2 H), GaitSchedule.cpp:78-137), then the synchronized
// GaitReceiver (GaitReceiver.cpp:49-59: a received template inserted at (t0 + H, H), GaitSchedule.cpp:46-73).  The window feeds the
// same grid / node-table code as k_reference_grids, so the tables are bit-identical to what the host path builds from the same schedule.
#pragma once
#include <hip/hip_runtime.h>

#include "reference_device.h"

namespace bpmpc {

#define EXACT_FP_BODY _Pragma("clang fp contract(off)")   // first statement of a body: no fused multiply-add, as on the host

constexpr int kGaitMeta = 3;   // per state slot: number of events, number of modes, template index (getModeSchedule tiles with it)

struct GaitAdvanceArgs {
  ReferenceGenArgs ref;        // library, grid settings and node-table outputs; ref.t0 per group
  int n_advance;               // groups [0, n_advance) advance and lay a grid; the groups behind them carry their state over unchanged
  const int* src;              // per group: slot of its state in the front buffer, < 0 = the state after create / reset
  const int* insert_gait;      // per group: pending insertModeSequenceTemplate (< 0: none)
  const double* insert_start;
  const double* insert_final;
  const int* command;          // per group: pending GaitReceiver command (< 0: none)
  const double* ev_in;         // front buffer [slot][kRefMaxEvents]
  const int* ms_in;            //              [slot][kRefMaxEvents + 1]
  const int* meta_in;          //              [slot][kGaitMeta]
  double* ev_out;              // back buffer, slot = group
  int* ms_out;
  int* meta_out;
};

__global__ __launch_bounds__(64) void k_gait_advance(GaitAdvanceArgs a) {
  EXACT_FP_BODY
  __shared__ RefGenLds w;
  __shared__ int tmpl;
  const int g = blockIdx.x, l = threadIdx.x;
  const GaitLibraryView& lib = a.ref.lib;
  const int src = a.src[g];
  if (src < 0) {               // GaitSchedule(initialModeSchedule, defaultModeSequenceTemplate, phaseTransitionStanceTime)
    if (l == 0) {
      DevSchedule s{w.ev, w.ms, 0, 0, kRefMaxEvents, kRefOk, 0.0};
      for (int i = 0; i < lib.init_n_events; ++i) ref_push_ev(s, lib.init_events[i]);
      for (int i = 0; i <= lib.init_n_events; ++i) ref_push_ms(s, lib.init_modes[i]);
      w.ne = s.ne; w.nm = s.nm; w.status = s.status; tmpl = lib.n_templates - 1;
    }
  } else {
    const int* meta = a.meta_in + (size_t)src * kGaitMeta;
    const int ne = meta[0], nm = meta[1];
    for (int i = l; i < ne; i += 64) w.ev[i] = a.ev_in[(size_t)src * kRefMaxEvents + i];
    for (int i = l; i < nm; i += 64) w.ms[i] = a.ms_in[(size_t)src * (kRefMaxEvents + 1) + i];
    if (l == 0) { w.ne = ne; w.nm = nm; w.status = kRefOk; tmpl = meta[2]; }
  }
  if (l == 0) w.base = 0;
  __syncthreads();
  if (g < a.n_advance) {
    const double t0 = a.ref.t0[g], horizon = a.ref.horizon, lower = t0 - horizon, upper = t0 + 2 * horizon;
    if (l == 0) {
      w.rows = 12;
      w.vrows = 4;
      // a pending insert first: tiling from a start far in the past only fits with the compaction bound t0 - H of this setup
      DevSchedule s{w.ev, w.ms, w.ne, w.nm, kRefMaxEvents, w.status, lower};
      if (a.insert_gait[g] >= 0) { tmpl = a.insert_gait[g]; ref_insert(s, lib, tmpl, a.insert_start[g], a.insert_final[g]); }
      int base = 0;
      if (s.status == kRefOk) base = ref_window(s, lib, tmpl, lower, upper);
      if (s.status == kRefOk) ref_check_swings(s);
      w.base = base; w.ne = s.ne; w.nm = s.nm; w.status = s.status;
      ref_lay_grid(w, a.ref, t0);
    }
    __syncthreads();
    ref_fill_tables(w, a.ref, g, l);
    __syncthreads();
    if (l == 0) {
      // GaitReceiver::preSolverRun behind the reference manager: the command shapes the NEXT window, from t0 + H on
      // (insertModeSequenceTemplate(receivedGait_, finalTime, timeHorizon) with finalTime = t0 + H, timeHorizon = H)
      if (w.status == kRefOk && a.command[g] >= 0) {
        DevSchedule s{w.ev + w.base, w.ms + w.base, w.ne, w.nm, kRefMaxEvents - w.base, kRefOk, lower};
        tmpl = a.command[g];
        ref_insert(s, lib, tmpl, t0 + horizon, horizon);
        w.ne = s.ne; w.nm = s.nm; w.status = s.status;
      }
      a.ref.nodes[g] = w.n_grid; a.ref.status[g] = w.status; a.ref.rows[g] = w.rows | (w.vrows << 8);
    }
    __syncthreads();
  }
  const double* ev = w.ev + w.base;
  const int* ms = w.ms + w.base;
  for (int i = l; i < w.ne; i += 64) a.ev_out[(size_t)g * kRefMaxEvents + i] = ev[i];
  for (int i = l; i < w.nm; i += 64) a.ms_out[(size_t)g * (kRefMaxEvents + 1) + i] = ms[i];
  if (l == 0) {
    int* meta = a.meta_out + (size_t)g * kGaitMeta;
    meta[0] = w.ne; meta[1] = w.nm; meta[2] = tmpl;
  }
}

// GaitReceiver::mpcModeSequenceCallback for a batch: gait[b] >= 0 becomes robot b's pending template (the latest command wins)
__global__ __launch_bounds__(256) void k_gait_command(int batch, const int* gait, int* pending) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < batch && gait[b] >= 0) pending[b] = gait[b];
}

#undef EXACT_FP_BODY

}  // namespace bpmpc
