// Batched rigid-body plant on the device (include/bpmpc.h "Plant"): joint commands of a batch of robots -> their next rigid-body states and the
// sensors of bpmpc_sensor_inputs.  This engine's own model, specified in include/bpmpc.h: the rigid-body dynamics of kernels/wbc.h with
// q = [position, zyx, joints], v = dq/dt, penalty contacts at the four contact points (explicit spring, linearly implicit normal and regularised
// Coulomb damping), a joint PD whose kd term is implicit, and a semi-implicit Euler step.  It imitates no other simulator.
//
// One wavefront per robot, every substep of a control step inside one launch; q and v live in LDS (WbcRbd::q / v) between the substeps and meet
// HBM at entry and exit only.  One substep of length h:
//   rigid-body pass   wbc_rbd_pass at (q, v) with gravity, as it is; M, nle and the contact Jacobian are assembled from it as wbc_robot does
//   contacts          lanes 0..3: penetration, spring force, the diagonal damping D_i of the point
//   system            lane l owns row l of A = M + h J'DJ + h diag(0, kd) (lower triangle; J'DJ by three rank-one updates per closed contact) and
//                     entry l of the right-hand side M v + h (S'(tau + kd velDes) - nle + J'f + w_ext)
//   solve             Cholesky without pivoting in LDS, lane per row, the forward substitution folded into the factorisation; back substitution
//   integrate         v+ = the solution, q+ = q + h v+
// The sensors are formed from (q+, v+) of the last substep.  The arithmetic of one robot depends on nothing but that robot's data.
//
// Stick-slip contacts (STICK; k_plant_stick_step): a robot with kt > 0 carries an anchor and a flag per contact point.  They are loaded once per
// launch, live in LDS beside q and v over the substeps and meet HBM at entry and exit only.  Lanes 0..3 own the law: anchor a fresh contact, clamp
// the spring at the Coulomb cap (slip), give the damper the friction the spring has not used, make the sticking spring linearly implicit.  kt is
// wave-uniform; a robot with kt = 0 takes the branch that is the plant without stiction, operation for operation, and touches no anchor.  The
// handle launches the instantiation without STICK until stiction is first set on it.  The two instantiations are compiled in translation units of
// their own (plant.hip, plant_stick.hip): each then has one call site of the rigid-body pass, and the compiler inlines and contracts k_plant_step
// as it did before the plant had stiction - the same bits at the same speed.
//
// Joint model (JOINT; k_plant_joint_step, plant_joint.hip, a third translation unit for the same reason): a joint row per robot (armature, damping,
// friction loss, end stops; include/bpmpc.h "joints").  Lanes 6..NV-1 load their joint's five constants once per launch and keep them in registers
// over the substeps; the three scalars of the row are wave-uniform and parked in LDS.  Whether the row is neutral is one ballot per launch: a robot
// with the neutral row takes the branch that is k_plant_stick_step, operation for operation.  Everything the model adds is lane-local: the
// armature and the damping go onto the diagonal entry the lane owns, the end-stop torque into the lane's generalised force.
//
// Bodies (BODY; k_plant_body_step, plant_body.hip, a fourth translation unit for the same reason): a body row per robot (mass, centre of mass and
// inertia of every body; include/bpmpc.h "bodies").  Lanes 0..NJ load their body's ten numbers once per launch - entry-major rows, so consecutive
// lanes read consecutive words - into LDS (PlantBodyLds::body), not into registers: the joint kernel has none to spare.  The rigid-body pass then
// takes the three inertial constants of a body from there (wbc_rbd_pass on a PlantBodyModel, kernels/wbc.h) where it takes them from the model, each
// lane its own body's, and everything else - geometry, axes, contact offsets, gravity - from the model as before.  Nothing else changes: there
// is no branch on whether a row is the model's.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../device_model.h"
#include "wbc.h"   // wbc_rbd_pass, wbc_on_chain, wbc_contact_jac_col, kinematics.h, lds_wave_sync, kWave

namespace bpmpc {

constexpr int kPlantParamStride = 8;      // BPMPC_PLANT_PARAM_STRIDE
constexpr double kPlantGravity = 9.81;
constexpr int kPlantJointParamStride = 64;      // BPMPC_PLANT_JOINT_PARAM_STRIDE
constexpr int kPlantJointSlots = 12;            // joints a row has room for
// A joint row: five blocks of kPlantJointSlots (armature, damping, friction_loss, lower, upper), then k_limit, c_limit, w_eps, reserved
enum PlantJointEntry { kJointArmature = 0, kJointDamping = 12, kJointFriction = 24, kJointLower = 36, kJointUpper = 48, kJointKLimit = 60, kJointCLimit = 61,
                       kJointWEps = 62, kJointParamUsed = 63 };
constexpr double kPlantJointKLimit = 1e4, kPlantJointCLimit = 1e2, kPlantJointWEps = 0.01;      // the scalars of the neutral row
static_assert(kMaxJoints <= kPlantJointSlots, "a joint row holds every joint");
constexpr int kPlantBodyParamStride = 160;      // BPMPC_PLANT_BODY_PARAM_STRIDE
constexpr int kPlantBodySlots = 16;             // bodies a block of a body row has room for
// A body row: ten blocks of kPlantBodySlots, body b at slot b of each (mass; com x, y, z; inertia xx, xy, xz, yy, yz, zz)
enum PlantBodyEntry { kBodyMass = 0, kBodyCom = 16, kBodyInertia = 64 };
static_assert(kMaxBodies <= kPlantBodySlots, "a body row holds every body");

// A parameter row
struct PlantSettings {
  double kn, cn, d0, mu, v_eps, contact_threshold, reserved[2];
};
static_assert(sizeof(PlantSettings) == kPlantParamStride * sizeof(double), "PlantSettings is a parameter row");

// The sections of the output block, in doubles per robot: the members of bpmpc_sensor_inputs the plant writes (contact: four ints), the ground-truth
// rbd in the layout of bpmpc_controller_tick, the contact forces
enum PlantOut { kPlantJointPos, kPlantJointVel, kPlantQuat, kPlantAngLocal, kPlantAccLocal, kPlantFeetHeights, kPlantOdomPos, kPlantOdomQuat, kPlantOdomLin,
                kPlantOdomAng, kPlantRbd, kPlantContactForce, kPlantContact, kPlantOutEnd };
__host__ __device__ constexpr int plant_out_width(int s, int nj) {
  return s == kPlantJointPos || s == kPlantJointVel ? nj
         : s == kPlantQuat || s == kPlantOdomQuat || s == kPlantFeetHeights ? 4
         : s == kPlantRbd ? 2 * (6 + nj)
         : s == kPlantContactForce ? 12
         : s == kPlantContact ? 2
                              : 3;
}
__host__ __device__ constexpr int plant_out_offset(int s, int nj) {
  int o = 0;
  for (int i = 0; i < s; ++i) o += plant_out_width(i, nj);
  return o;
}

struct PlantArgs {
  int batch, substeps;
  int cmd_stride;                                   // doubles between the robots' rows of pos_des / vel_des / tau_ff (NJ, or 3 NJ for a tick's joint_cmd)
  double h;                                         // substep length
  const double* params;                             // [max_batch][kPlantParamStride]
  double* state;                                    // [max_batch][2 (6 + NJ)]: q, v; read and updated
  const double *pos_des, *vel_des, *tau_ff;         // [batch] rows of NJ, cmd_stride apart
  const double *kp, *kd;                            // [batch][NJ]
  const double *base_force, *ground;                // [batch][3], [batch][4]; nullable: 0
  double torque_limits[kMaxJoints / 2];             // per leg joint; <= 0: no limit
  // outputs, written after the last substep: one block, section s ([max_batch][plant_out_width(s)]) at out + max_batch plant_out_offset(s)
  double* out;
  int max_batch;
};

// Stick-slip contacts: what the STICK instantiation takes beside PlantArgs
struct PlantStickArgs {
  const double* kt;                                 // [max_batch] tangential stiffness; 0: none
  double* anchor;                                   // [max_batch][4][2] world xy of the anchors; read and updated for a robot with kt > 0
  int* anchored;                                    // [max_batch][4]
};

// The joint model: what the JOINT instantiation takes beside PlantArgs and PlantStickArgs
struct PlantJointArgs {
  const double* rows;                               // [max_batch][kPlantJointParamStride]
};

// Bodies: what the BODY instantiation takes beside the three above
struct PlantBodyArgs {
  const double* rows;                               // [max_batch][kPlantBodyParamStride]
};

template <int NJ>
struct PlantLds {
  static constexpr int NV = 6 + NJ;
  WbcRbd<NJ> rbd;
  double A[NV][NV + 1];                  // M, then the system matrix (lower triangle), then its Cholesky factor below the diagonal; column NV: right-hand side
  double dg[NV];                         // diagonal of the factor
  double J[3 * kNumContacts][NV];
  double D[3 * kNumContacts];            // damping of the contact rows (ct, ct, cn per point; 0 for an open point)
  double fz[kNumContacts], nrm[kNumContacts];      // spring force, start-of-step normal force
  int closed[kNumContacts];
  double par[kPlantParamStride];
  double *state, *out;                   // this robot's state row and the output block: parked here over the substeps, not in scalar registers
  size_t out_stride;                     // max_batch
  double h;
};

// Stick-slip contacts in LDS, behind the members above: the robot's kt; for kt > 0 the tangential spring forces, the anchors and the flags over
// the substeps
template <int NJ>
struct PlantStickLds : PlantLds<NJ> {
  double ft[kNumContacts][2], anchor[kNumContacts][2];
  int anchored[kNumContacts];
  double kt;
  double* anchor_row;                    // this robot's anchors and flags in HBM: parked here over the substeps as state and out are
  int* anchored_row;
};

// The joint model in LDS, behind the members above: the three scalars of the robot's joint row, parked here over the substeps as h is
template <int NJ>
struct PlantJointLds : PlantStickLds<NJ> {
  double k_limit, c_limit, w_eps;
};

// The inertial constants of a robot's bodies as the rigid-body pass reads them (the members of DeviceModel it takes them from otherwise)
template <int NJ>
struct PlantBodyConstants {
  double mass[NJ + 1], com[NJ + 1][3];
  double inertia[NJ + 1][6];             // xx, xy, xz, yy, yz, zz about the com, body frame
};

// The model the rigid-body pass sees in the BODY instantiation: the handle's model with the inertial constants of one robot's row
template <int NJ>
struct PlantBodyModel {
  const DeviceModel& md;
  const PlantBodyConstants<NJ>& body;
};
template <int NJ>
__device__ __forceinline__ const DeviceModel& wbc_geometry(const PlantBodyModel<NJ>& m) { return m.md; }
template <int NJ>
__device__ __forceinline__ const PlantBodyConstants<NJ>& wbc_inertial(const PlantBodyModel<NJ>& m) { return m.body; }

// Bodies in LDS, behind the members above: the robot's body row, body-major, over the substeps
template <int NJ>
struct PlantBodyLds : PlantJointLds<NJ> {
  PlantBodyConstants<NJ> body;
};

template <int NJ, bool STICK, bool JOINT, bool BODY = false>
using PlantLdsOf = std::conditional_t<BODY, PlantBodyLds<NJ>, std::conditional_t<JOINT, PlantJointLds<NJ>, std::conditional_t<STICK, PlantStickLds<NJ>, PlantLds<NJ>>>>;

template <int NJ, bool STICK, bool JOINT = false, bool BODY = false>
__device__ void plant_robot(const DeviceModel& md, PlantLdsOf<NJ, STICK, JOINT, BODY>& w, const PlantArgs& a, const PlantStickArgs& sa, int b, int l,
                            const PlantJointArgs& ja = PlantJointArgs{}, const PlantBodyArgs& ba = PlantBodyArgs{}) {
  static_assert(STICK || !JOINT, "the joint model is compiled with stick-slip contacts");
  static_assert(JOINT || !BODY, "the body rows are compiled with the joint model");
  constexpr int NV = 6 + NJ, NC = kNumContacts;
  WbcRbd<NJ>& r = w.rbd;
  if (l < kPlantParamStride) {      // these lanes all park the same pointers: one predicate for the prologue
    w.par[l] = a.params[(size_t)b * kPlantParamStride + l];
    w.state = a.state + (size_t)b * 2 * NV; w.out = a.out; w.out_stride = (size_t)a.max_batch; w.h = a.h;
  }
  static_assert(kPlantParamStride <= kWave && NV <= kWave, "one lane per row entry and per coordinate");
  if (l < NV) { const double* state = a.state + (size_t)b * 2 * NV; r.q[l] = state[l]; r.v[l] = state[NV + l]; }
  // this lane's share of the command: constant over the substeps
  double pd = 0.0, vd = 0.0, tf = 0.0, kp = 0.0, kd = 0.0, lim = HUGE_VAL, wext = 0.0, ground = 0.0;
  if (l >= 6 && l < NV) {
    const int j = l - 6;
    const size_t c = (size_t)b * a.cmd_stride + j;
    pd = a.pos_des[c]; vd = a.vel_des[c]; tf = a.tau_ff[c];
    kp = a.kp[(size_t)b * NJ + j]; kd = a.kd[(size_t)b * NJ + j];
    lim = a.torque_limits[j % (NJ / 2)];
    if (!(lim > 0.0)) lim = HUGE_VAL;      // no limit
  }
  if (l < 3 && a.base_force) wext = a.base_force[(size_t)b * 3 + l];
  if (l < NC && a.ground) ground = a.ground[(size_t)b * NC + l];
  if constexpr (STICK) {
    const double kt = sa.kt[b];
    if (l == 0) { w.kt = kt; w.anchor_row = sa.anchor + (size_t)b * NC * 2; w.anchored_row = sa.anchored + (size_t)b * NC; }
    if (l < NC && kt > 0.0) {
      w.anchor[l][0] = sa.anchor[((size_t)b * NC + l) * 2]; w.anchor[l][1] = sa.anchor[((size_t)b * NC + l) * 2 + 1];
      w.anchored[l] = sa.anchored[(size_t)b * NC + l];
    }
  }
  // this lane's joint: constant over the substeps.  The base lanes carry the neutral values, under which every term below is exactly 0
  double arm = 0.0, damp = 0.0, fric = 0.0, lower = -HUGE_VAL, upper = HUGE_VAL;
  bool joints = false;      // wave-uniform: the robot's row is not neutral
  if constexpr (JOINT) {
    const double* row = ja.rows + (size_t)b * kPlantJointParamStride;
    if (l >= 6 && l < NV) {
      const int j = l - 6;
      arm = row[kJointArmature + j]; damp = row[kJointDamping + j]; fric = row[kJointFriction + j];
      lower = row[kJointLower + j]; upper = row[kJointUpper + j];
    }
    if (l == 0) {
      double weps = row[kJointWEps];
      if (!(weps > 0.0)) weps = kPlantJointWEps;
      w.k_limit = row[kJointKLimit]; w.c_limit = row[kJointCLimit]; w.w_eps = weps;
    }
    joints = __any(arm != 0.0 || damp != 0.0 || fric != 0.0 || lower != -HUGE_VAL || upper != HUGE_VAL) != 0;
  }
  // this lane's body: into LDS, read by the rigid-body pass behind its first barrier
  if constexpr (BODY) {
    static_assert(NJ + 1 <= kPlantBodySlots && NJ + 1 <= kWave, "one lane per body of the row");
    if (l < NJ + 1) {
      const double* row = ba.rows + (size_t)b * kPlantBodyParamStride + l;
      w.body.mass[l] = row[kBodyMass];
      for (int k = 0; k < 3; ++k) w.body.com[l][k] = row[kBodyCom + k * kPlantBodySlots];
      for (int k = 0; k < 6; ++k) w.body.inertia[l][k] = row[kBodyInertia + k * kPlantBodySlots];
    }
  }
  double acc = 0.0;      // lanes 0..2: (v+ - v) / h of the last substep

#pragma unroll 1
  for (int step = 0; step < a.substeps; ++step) {
    int lp = l;
    asm volatile("" : "+v"(lp));      // the lane, opaque: the pass's lane predicates are formed in each substep and not held in scalar registers over the loop
    if constexpr (BODY) wbc_rbd_pass<NJ>(PlantBodyModel<NJ>{md, w.body}, r, true, lp);      // the robot's own masses, centres of mass and inertias
    else
    wbc_rbd_pass<NJ>(md, r, true, lp);      // synchronises at entry and exit
    // ---- mass matrix, nonlinear effects, contact Jacobian (the assembly of wbc_robot)
#pragma unroll 1
    for (int idx = l; idx < NV * NV; idx += kWave) {
      const int hh = idx / NV, g = idx % NV;
      double val = 0.0;
      if (wbc_on_chain(md, hh, g)) val = fused::dot3(r.S[hh], r.fc[g]) + fused::dot3(r.S[hh] + 3, r.fc[g] + 3);
      else if (wbc_on_chain(md, g, hh)) val = fused::dot3(r.S[g], r.fc[hh]) + fused::dot3(r.S[g] + 3, r.fc[hh] + 3);
      w.A[hh][g] = val;
    }
    double nle = 0.0;
    if (l < NV) nle = fused::dot3(r.S[l], r.ws[l]) + fused::dot3(r.S[l] + 3, r.ws[l] + 3);
#pragma unroll 1
    for (int idx = l; idx < NC * NV; idx += kWave) {
      const int i = idx / NV, g = idx % NV;
      double col[3];
      wbc_contact_jac_col<NJ>(md, r, i, g, col);
      for (int k = 0; k < 3; ++k) w.J[3 * i + k][g] = col[k];
    }
    // ---- contact law of point l
    if (l < NC) {
      const double kn = w.par[0], cn = w.par[1], d0 = w.par[2], mu = w.par[3], veps = w.par[4];
      const double d = ground - r.cp[l][2];
      const bool closed = d > 0.0;
      double f = 0.0, cni = 0.0, n = 0.0, ct = 0.0;
      if (closed) {
        f = kn * d;
        cni = cn * fmin(1.0, d / d0);
        n = fmax(0.0, kn * d - cni * r.cv[l][2]);
        ct = mu * n / sqrt(r.cv[l][0] * r.cv[l][0] + r.cv[l][1] * r.cv[l][1] + veps * veps);
      }
      if constexpr (STICK) {
        const double kt = w.kt;
        if (kt > 0.0) {
          double fx = 0.0, fy = 0.0;
          int anchored = 0;
          if (closed) {
            const double px = r.cp[l][0], py = r.cp[l][1];
            double ax = px, ay = py;      // a point that closes anchors where it is
            if (w.anchored[l]) { ax = w.anchor[l][0]; ay = w.anchor[l][1]; }
            double sx = ax - px, sy = ay - py;
            const double phi = kt * sqrt(sx * sx + sy * sy), cap = mu * n;
            double room = cap - phi, imp = w.h * kt;
            if (phi > cap) {      // slip: the anchor follows at the cap, the damper has nothing left and the spring is explicit
              const double scale = cap / phi;
              ax = cap > 0.0 ? px + sx * scale : px; ay = cap > 0.0 ? py + sy * scale : py;
              sx = ax - px; sy = ay - py;
              room = 0.0; imp = 0.0;
            }
            fx = kt * sx; fy = kt * sy;
            ct = room / sqrt(r.cv[l][0] * r.cv[l][0] + r.cv[l][1] * r.cv[l][1] + veps * veps) + imp;
            w.anchor[l][0] = ax; w.anchor[l][1] = ay;
            anchored = 1;
          }
          w.anchored[l] = anchored;
          w.ft[l][0] = fx; w.ft[l][1] = fy;
        }
      }
      w.closed[l] = closed ? 1 : 0;
      w.fz[l] = f; w.nrm[l] = n;
      w.D[3 * l] = ct; w.D[3 * l + 1] = ct; w.D[3 * l + 2] = cni;
    }
    lds_wave_sync();
    const double h = w.h;
    // ---- row l of the system and entry l of the right-hand side
    const double v_old = l < NV ? r.v[l] : 0.0;
    if (l < NV) {
      if constexpr (JOINT) {
        if (joints) w.A[l][l] += arm;      // the M of both sides
      }
      double mv = 0.0;
#pragma unroll 1
      for (int g = 0; g < NV; ++g) mv += w.A[l][g] * r.v[g];
      double gen = -nle;
      for (int i = 0; i < NC; ++i) gen += w.J[3 * i + 2][l] * w.fz[i];
      if constexpr (STICK) {
        if (w.kt > 0.0) {
          double tang = 0.0;
          for (int i = 0; i < NC; ++i) tang += w.J[3 * i][l] * w.ft[i][0] + w.J[3 * i + 1][l] * w.ft[i][1];
          gen += tang;
        }
      }
      // base lanes carry kp = kd = tf = 0 and the other lanes wext = 0: no branch on the lane's kind
      const double tau = fmin(lim, fmax(-lim, kp * (pd - r.q[l]) + tf));
      gen += wext + tau + kd * vd;
      double cj = 0.0;      // passive damping of this lane's joint
      if constexpr (JOINT) {
        if (joints) {
          const double ql = r.q[l], weps = w.w_eps;
          const double pen_up = fmax(ql - upper, 0.0), pen_lo = fmax(lower - ql, 0.0);
          gen += w.k_limit * (pen_lo - pen_up);      // outside the clamp: the end stop is not the actuator
          cj = damp + fric / sqrt(v_old * v_old + weps * weps);
          if (pen_up > 0.0 || pen_lo > 0.0) cj += w.c_limit;
        }
      }
#pragma unroll 1
      for (int i = 0; i < NC; ++i)
        if (w.closed[i])
          for (int k = 0; k < 3; ++k) {
            const double* jr = w.J[3 * i + k];
            const double c = h * w.D[3 * i + k] * jr[l];
            for (int g = 0; g <= l; ++g) w.A[l][g] += c * jr[g];
          }
      if constexpr (JOINT) {
        if (joints) w.A[l][l] += h * (kd + cj);
        else w.A[l][l] += h * kd;
      } else {
        w.A[l][l] += h * kd;
      }
      w.A[l][NV] = mv + h * gen;
    }
    // ---- Cholesky A = L L' (row l below the diagonal), y = L^-1 rhs in column NV
#pragma unroll 1
    for (int k = 0; k < NV; ++k) {
      lds_wave_sync();
      const double d = sqrt(w.A[k][k]);
      if (l == k) { w.dg[k] = d; w.A[k][NV] = w.A[k][NV] / d; }
      double lk = 0.0;
      if (l > k && l < NV) { lk = w.A[l][k] / d; w.A[l][k] = lk; }
      lds_wave_sync();
      if (l > k && l < NV) {
        for (int j = k + 1; j <= l; ++j) w.A[l][j] -= lk * w.A[j][k];
        w.A[l][NV] -= lk * w.A[k][NV];
      }
    }
    // ---- L' x = y
    double vplus = 0.0;
#pragma unroll 1
    for (int k = NV - 1; k >= 0; --k) {
      lds_wave_sync();
      const double xk = w.A[k][NV] / w.dg[k];
      if (l < k) w.A[l][NV] -= w.A[k][l] * xk;
      if (l == k) vplus = xk;
    }
    // ---- integrate
    if (l < NV) {
      acc = (vplus - v_old) / h;
      r.v[l] = vplus;
      r.q[l] += h * vplus;
    }
  }
  lds_wave_sync();

  // ============================================================ state, contact forces and sensors from (q+, v+)
  asm volatile("" : "+v"(l));      // opaque as above: the predicates below are formed here, not kept over the substeps
  double* const state = w.state;
  double* const out_base = w.out;
  const size_t out_stride = w.out_stride;
  auto out = [&](int section) { return out_base + out_stride * plant_out_offset(section, NJ); };
  if (l < NV) { state[l] = r.q[l]; state[NV + l] = r.v[l]; }
  if (l < 3 * NC) {
    const int i = l / 3;
    double f = 0.0;
    if (w.closed[i]) {
      double jv = 0.0;
      for (int g = 0; g < NV; ++g) jv += w.J[l][g] * r.v[g];
      double spring = l % 3 == 2 ? w.fz[i] : 0.0;
      if constexpr (STICK) {
        if (l % 3 != 2 && w.kt > 0.0) spring = w.ft[i][l % 3];
      }
      f = spring - w.D[l] * jv;
    }
    out(kPlantContactForce)[(size_t)b * 3 * NC + l] = f;
  }
  if constexpr (STICK) {
    if (l < NC && w.kt > 0.0) {
      double* const anchor_row = w.anchor_row;
      anchor_row[2 * l] = w.anchor[l][0]; anchor_row[2 * l + 1] = w.anchor[l][1];
      w.anchored_row[l] = w.anchored[l];
    }
  }
  if (l < NC) {
    reinterpret_cast<int*>(out(kPlantContact))[(size_t)b * NC + l] = w.nrm[l] > w.par[5] ? 1 : 0;
    out(kPlantFeetHeights)[(size_t)b * NC + l] = ground;
  }
  // wave-uniform: orientation, Euler rates, angular velocity
  const double z = r.q[3], y = r.q[4], x = r.q[5];
  const double sz = sin(z), cz = cos(z), sy = sin(y), cy = cos(y), sx = sin(x), cx = cos(x);
  double Rb[9];
  fused::rot_zyx(sz, cz, sy, cy, sx, cx, Rb);
  const double r0 = r.v[3], r1 = r.v[4], r2 = r.v[5];
  const double wg[3] = {-sz * r1 + cy * cz * r2, cz * r1 + cy * sz * r2, r0 - sy * r2};      // E(zyx) thetadot
  const double hz = 0.5 * z, hy = 0.5 * y, hx = 0.5 * x;
  const double shz = sin(hz), chz = cos(hz), shy = sin(hy), chy = cos(hy), shx = sin(hx), chx = cos(hx);
  const double qt[4] = {chz * chy * shx - shz * shy * chx, chz * shy * chx + shz * chy * shx, shz * chy * chx - chz * shy * shx, chz * chy * chx + shz * shy * shx};
  // linear acceleration of the base origin (lanes 0..2 hold it) seen by every lane
  const double ax = __shfl(acc, 0), ay = __shfl(acc, 1), az = __shfl(acc, 2) + kPlantGravity;
  if (l < 3) {
    // R' w and R' (a + g e_z): column l of R
    const double c0 = l == 0 ? Rb[0] : (l == 1 ? Rb[1] : Rb[2]), c1 = l == 0 ? Rb[3] : (l == 1 ? Rb[4] : Rb[5]), c2 = l == 0 ? Rb[6] : (l == 1 ? Rb[7] : Rb[8]);
    out(kPlantAngLocal)[(size_t)b * 3 + l] = c0 * wg[0] + c1 * wg[1] + c2 * wg[2];
    out(kPlantAccLocal)[(size_t)b * 3 + l] = c0 * ax + c1 * ay + c2 * az;
    const double wl = l == 0 ? wg[0] : (l == 1 ? wg[1] : wg[2]);
    out(kPlantOdomPos)[(size_t)b * 3 + l] = r.q[l];
    out(kPlantOdomLin)[(size_t)b * 3 + l] = r.v[l];
    out(kPlantOdomAng)[(size_t)b * 3 + l] = wl;
    double* rbd = out(kPlantRbd) + (size_t)b * 2 * NV;
    rbd[l] = r.q[3 + l]; rbd[3 + l] = r.q[l];
    rbd[NV + l] = wl; rbd[NV + 3 + l] = r.v[l];
  }
  if (l < 4) {
    const double ql = l == 0 ? qt[0] : (l == 1 ? qt[1] : (l == 2 ? qt[2] : qt[3]));
    out(kPlantQuat)[(size_t)b * 4 + l] = ql;
    out(kPlantOdomQuat)[(size_t)b * 4 + l] = ql;
  }
  if (l >= 6 && l < NV) {
    double* rbd = out(kPlantRbd) + (size_t)b * 2 * NV;
    out(kPlantJointPos)[(size_t)b * NJ + l - 6] = r.q[l];
    out(kPlantJointVel)[(size_t)b * NJ + l - 6] = r.v[l];
    rbd[l] = r.q[l]; rbd[NV + l] = r.v[l];
  }
}

}  // namespace bpmpc
