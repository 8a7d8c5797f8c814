// Tracking telemetry on the device (DebugPublisher::update, bipedal_controllers/src/debug/DebugPublisher.cpp, called from
// BipedalController.cpp:270; msg/TrackingError.msg) for a batch of robots: forward kinematics of the configuration the policy asks for,
// q_des = x*[6:12 + nj], and of the measured one, q_meas = [rbd[3:6], rbd[0:3], rbd[6:6 + nj]]; base pose, the four contact points and the joint
// positions of both in one sample per robot and update; the tracking errors of the sample accumulated into a statistics row; the sample stored
// into a per-robot ring that freezes when the robot falls (include/bpmpc.h "Tracking telemetry" has the layouts and the rules).
//
// Mapping: the tick's (kernels/tick.h) - lane g of a robot carries generalised coordinate g, 16 lanes per robot at nj = 10, 32 at nj = 12, four
// or two robots per wavefront.  Joint lanes write the joint-local rotations Rfix E(q) of both configurations to LDS; lane 4 p + i (p = 0 desired,
// 1 measured) composes them along the chain of contact i and places the point; lane i takes lane 4 + i's point by a DPP row shift.  The squared
// errors of the base position, the base angles and the joints are summed over the robot's lanes by DPP rotations.  Sample and statistics row are
// staged in LDS and stored as runs of consecutive doubles.  The kinematic tree, the contact points and their order are those of the WBC's
// rigid-body pass (kernels/wbc.h) and of oracle/wbc_py.py fk / contact_points.
//
// The error norms are formed without multiply-add contraction and in a stated order, so that a restatement (tests/telemetry_reference.py) gives
// their bits: the contact errors as sqrt((dx dx + dy dy) + dz dz); the three lane sums as row16_allreduce_add leaves them in lane 0 (position),
// lane 1 (angles) and lane 6 (joints), the 32-lane robots adding the upper row's sum to the lower's.
#pragma once
#include "tick.h"

namespace bpmpc {

constexpr int kTelStatsStride = 40;
constexpr int kTelGroups = 7;                       // base position, base angles, four contact points, joints
constexpr int kTelSamples = 3 * kTelGroups;         // entry of the statistics row: number of samples accumulated
constexpr int kTelFirstUnsafe = kTelSamples + 1;    // n of the first sample that was unsafe or not finite, -1: none
constexpr int kTelJointMax = kTelSamples + 2;       // 12 entries: largest |joint error| per joint
__host__ __device__ constexpr int telemetry_sample_stride(int nj) { return 40 + 2 * nj; }

struct TelemetryArgs {
  int batch, ring_len, every, freeze;
  const double* t;                    // [batch], nullable
  const double *x_opt, *rbd;          // [batch][12 + NJ], [batch][2 (6 + NJ)]
  const int *safe, *mode;             // [batch], nullable
  double *sample, *stats, *ring;      // [max_batch][stride], [max_batch][40], [max_batch][ring_len][stride]
  int *frozen, *count;                // [max_batch], [max_batch][2]: n, samples recorded into the ring
};

template <int NJ>
struct TelemetryLds {
  using C = LinFastCfg<NJ>;
  double T[C::NPW][2][NJ][9];         // joint-local rotations of the desired and the measured configuration
  double smp[C::NPW][telemetry_sample_stride(NJ)];
  double row[C::NPW][kTelStatsStride];
};

template <int NJ>
__device__ __forceinline__ void telemetry_robot(const DeviceModel& md, TelemetryLds<NJ>& w, const TelemetryArgs& a) {
#pragma clang fp contract(off)
  using C = LinFastCfg<NJ>;
  constexpr int G = C::G, NX = C::NX, LPN = C::LPN, NPW = C::NPW, S = telemetry_sample_stride(NJ);
  static_assert(C::G0 == 0 && NJ <= 12, "one lane per coordinate; twelve joint_max entries");
  const int sub = threadIdx.x / LPN, g = threadIdx.x % LPN;
  const int bq = blockIdx.x * NPW + sub;
  const bool valid = bq < a.batch;
  const int b = valid ? bq : 0;            // lane groups beyond the batch compute robot 0 and write nothing (the DPP reductions need every lane)
  const bool live = valid && a.frozen[b] == 0;
  if (__ballot(live) == 0) return;         // one wavefront per workgroup: nothing but the flag test for frozen robots
  double* smp = w.smp[sub];
  double* row = w.row[sub];
  const int n = a.count[2 * b], rec = a.count[2 * b + 1];
  const int safe = a.safe ? a.safe[b] : 1;

  // ---- this lane's coordinate of both configurations; base pose and joints of the sample; the robot's statistics row
  const double* xo = a.x_opt + (size_t)b * NX;
  const double* rb = a.rbd + (size_t)b * 2 * G;
  double qd = 0.0, qm = 0.0;
  if (g < G) {
    qd = xo[6 + g];
    qm = g < 3 ? rb[3 + g] : (g < 6 ? rb[g - 3] : rb[g]);
    if (g < 6) { smp[g] = qd; smp[6 + g] = qm; }
    else { smp[36 + g - 6] = qd; smp[36 + NJ + g - 6] = qm; }
  }
  if (g == 0) {
    smp[36 + 2 * NJ] = a.t ? a.t[b] : 0.0;
    smp[36 + 2 * NJ + 1] = a.safe ? (double)safe : 0.0;
    smp[36 + 2 * NJ + 2] = a.mode ? (double)a.mode[b] : 0.0;
    smp[36 + 2 * NJ + 3] = (double)n;
  }
  for (int c = g; c < kTelStatsStride; c += LPN) row[c] = a.stats[(size_t)b * kTelStatsStride + c];
  if (g >= 6 && g < G) {
    const int body = g - 5;
    const double* ax = md.axis[body];
    for (int p = 0; p < 2; ++p) {
      double sg, cg;
      sincos(p == 0 ? qd : qm, &sg, &cg);
      double rot[9], E[9];
      exact::axis_angle(ax, sg, cg, rot);             // the literals are rounded product by product, the matrix products below are fused:
      fused::mat3_mul(md.Rfix[body], rot, E);         // the bits this kernel has always produced ("Kinematic primitives")
      for (int i = 0; i < 9; ++i) w.T[sub][p][body - 1][i] = E[i];
    }
  }
  lds_wave_sync();

  // ---- contact points: lane 4 p + i walks the chain of contact i in configuration p (wbc_py.fk: o_j = o_parent + R_parent pfix_j,
  // R_j = R_parent Rfix_j E(q_j); contact_points: o_body + R_body contact_off)
  double pt[3] = {0.0, 0.0, 0.0};
  const bool is_contact = g < 2 * kNumContacts;
  if (is_contact) {
    const int p = g / kNumContacts, i = g % kNumContacts;
    const double* base = smp + 6 * p;
    double sy, cy, sp, cp, sr, cr;
    sincos(base[3], &sy, &cy);
    sincos(base[4], &sp, &cp);
    sincos(base[5], &sr, &cr);
    double R[9], o[3] = {base[0], base[1], base[2]};
    exact::rot_zyx(sy, cy, sp, cp, sr, cr, R);
    const int body = md.contact_body[i], depth = md.depth[body];
    for (int d = 0; d < depth; ++d) {
      const int j = md.path[body][d];
      double E[9];
      for (int k = 0; k < 9; ++k) E[k] = w.T[sub][p][j - 1][k];
      fused::chain_step(R, o, md.pfix[j], E);
    }
    fused::point_on_body(R, o, md.contact_off[i], pt);
    for (int k = 0; k < 3; ++k) smp[12 + 3 * g + k] = pt[k];
  }

  // ---- errors.  Lane i < 4: contact i, against the measured point of lane 4 + i; the lane sums of the squared coordinate errors
  const double mx = dpp_row_f64<kDppRowShl + kNumContacts>(pt[0]), my = dpp_row_f64<kDppRowShl + kNumContacts>(pt[1]),
               mz = dpp_row_f64<kDppRowShl + kNumContacts>(pt[2]);
  const double cx = pt[0] - mx, cy_ = pt[1] - my, cz = pt[2] - mz;
  const double e_contact = sqrt((cx * cx + cy_ * cy_) + cz * cz);
  double dq = qd - qm;
  if (g >= 3 && g < 6) dq = tick_normalize_angle(dq);
  const double aq = fabs(dq), sq = dq * dq;
  const double s_pos = node_allreduce_add<LPN>(g < 3 ? sq : 0.0);
  const double s_ang = node_allreduce_add<LPN>(g >= 3 && g < 6 ? sq : 0.0);
  const double s_jnt = node_allreduce_add<LPN>(g >= 6 && g < G ? sq : 0.0);
  // lane k < 7 holds the error of group k: contact i of lane i moves to lane 2 + i
  const double e_shifted = dpp_row_f64<kDppRowShr + 2>(e_contact);
  const double e = g == 0 ? sqrt(s_pos) : (g == 1 ? sqrt(s_ang) : (g < 6 ? e_shifted : sqrt(s_jnt)));
  const bool entry_bad = (g < G && !(isfinite(qd) && isfinite(qm))) || (is_contact && !(isfinite(pt[0]) && isfinite(pt[1]) && isfinite(pt[2])));
  const bool error_bad = g < kTelGroups && !isfinite(e);
  const bool not_finite = node_allreduce_add<LPN>(entry_bad ? 1.0 : 0.0) > 0.0;
  const bool errors_finite = !(node_allreduce_add<LPN>(error_bad ? 1.0 : 0.0) > 0.0);

  // ---- the record
  const bool trigger = (a.safe && safe == 0) || not_finite;
  const bool freezing = a.freeze != 0 && trigger;
  const bool record = a.ring_len > 0 && (freezing || n % a.every == 0);
  if (errors_finite) {
    if (g < kTelGroups) {
      row[3 * g] += e * e;
      if (e > row[3 * g + 1]) { row[3 * g + 1] = e; row[3 * g + 2] = (double)n; }
    }
    if (g >= 6 && g < G) row[kTelJointMax + g - 6] = fmax(row[kTelJointMax + g - 6], aq);
    if (g == 0) row[kTelSamples] += 1.0;
  }
  if (g == 0 && trigger && row[kTelFirstUnsafe] < 0.0) row[kTelFirstUnsafe] = (double)n;
  lds_wave_sync();
  if (!live) return;
  for (int c = g; c < kTelStatsStride; c += LPN) a.stats[(size_t)b * kTelStatsStride + c] = row[c];
  double* last = a.sample + (size_t)b * S;
  for (int c = g; c < S; c += LPN) last[c] = smp[c];
  if (record) {
    double* slot = a.ring + ((size_t)b * a.ring_len + rec % a.ring_len) * S;
    for (int c = g; c < S; c += LPN) slot[c] = smp[c];
  }
  if (g == 0) {
    a.count[2 * b] = n + 1;
    if (record) a.count[2 * b + 1] = rec + 1;
    if (freezing) a.frozen[b] = 1;
  }
}

}  // namespace bpmpc
