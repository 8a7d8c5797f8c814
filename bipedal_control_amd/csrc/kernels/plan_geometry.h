// Plan geometry on the device (BipedalControllerVisualizer::update, bipedal_controllers/src/BipedalControllerVisualizer.cpp:73-87, and its twin
// ocs2_bipedal_robot_ros/src/visualization/BipedalRobotVisualizer.cpp) for a batch of robots: forward kinematics of EVERY node of a plan - the
// base path, the paths of the four contact points, the centre of pressure - the future footholds and a summary row per robot (include/bpmpc.h
// "Plan geometry" has the layouts and the rules).
//
// The per-item arithmetic is written once, as __host__ __device__ functions (the first half of this file): the joint-local rotation, the chain
// walk of one contact, the row tail with the centre of pressure, the foothold predicate and the summary updates.  The kernels (the second half)
// and bpmpc_plan_rows_host (plan_geometry.hip) are compiled from that text.  Every sum of products that the header states an order for is formed
// without multiply-add contraction.
//
// Mapping.  A wavefront takes a TILE of 16 consecutive nodes of one robot and one block (optimized: the states x, desired: the references xref):
//   load   the tile's states, 16 (12 + NJ) consecutive doubles, into LDS; a lane that meets an entry that is not finite flags its node; beside
//          them what the chain walks read of the model (PlanChains)
//   A      lanes over (node, joint) pairs: the joint-local rotation Rfix E(q) into LDS; behind them (node, base angle) pairs: sine and cosine.
//          Four passes of the wave, one sincos per lane and pass, and only one pass mixes the two kinds of pair
//   B      lane 4 n + i walks the chain of contact i of node n: all 64 lanes carry a chain (the telemetry's mapping, 16 lanes per configuration
//          with 4 of them walking, would leave three quarters of the wave idle here)
//   C      lane n < 16 completes row n: base position, centre of pressure, time, mode, kind, sum_z, contact mask, flag
//   store  the tile's rows, 16 x 24 consecutive doubles, as runs of consecutive doubles
// Footholds and summary need the rows of a whole robot: plan_reduce, one wavefront per robot with nodes on lanes.  The landing flags of 64 nodes
// are four ballots (one per contact point), the slot of an entry is the running count plus the number of set bits below it, carried from one
// chunk of 64 nodes to the next.
//
// Two ways to launch them (plan_geometry.hip chooses; tools/plan_geometry_probe.py measures both):
//   one launch    k_plan_fused: a workgroup of four wavefronts owns a robot, its waves share the tiles, wave 0 reduces behind a barrier
//   two launches  k_plan_nodes, one wavefront per tile, then k_plan_reduce, one wavefront per robot
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../device_model.h"
#include "kinematics.h"        // the exact:: flavour: the host twin must give the kernels' bits
#include "riccati_fast.h"      // lds_wave_sync, readlane_f64

namespace bpmpc {

constexpr int kPlanNodeStride = 24, kPlanMaxFootholds = 16, kPlanFootholdStride = 6, kPlanSummaryStride = 16;
constexpr int kPlanTile = 16;                     // nodes of a tile: 4 lanes per node
constexpr int kPlanFusedWaves = 4;
// entries of a node row
constexpr int kPgBase = 0, kPgContact = 3, kPgCop = 15, kPgTime = 18, kPgMode = 19, kPgKind = 20, kPgSumZ = 21, kPgMask = 22, kPgBad = 23;
// entries of a summary row
constexpr int kPsNodes = 0, kPsFootholds = 1, kPsPath = 2, kPsApex = 3, kPsDrift = 7, kPsMinSumZ = 11, kPsBad = 12;

#define PG_HD __host__ __device__ __forceinline__

// ------------------------------------------------------------------------------------------------ the per-item arithmetic, host and device

// the contact points of a mode as a bit mask; the last node's mode -1 has no contact
PG_HD int plan_contact_mask(int mode) {
  int m = 0;
  for (int i = 0; i < kNumContacts; ++i) m |= exact::stance_flag(mode, i) ? 1 << i : 0;
  return m;
}

// E = Rfix[body] E(q): the joint-local rotation of joint `body` (1 .. nj) at the angle q (wbc_py.fk: Rfix_j axis_angle(axis_j, q_j))
PG_HD void plan_joint_rotation(const DeviceModel& md, int body, double q, double* E) {
  double sg, cg;
  sincos(q, &sg, &cg);
  exact::joint_rotation(md.Rfix[body], md.axis[body], sg, cg, E);
}

// What the chain walks read of a model, gathered once (per wavefront into LDS; on the host into a local): a walk that fetched path, pfix and
// offset from the device model would wait for two dependent loads from global memory per joint of the chain
struct PlanChains {
  double pfix[kMaxJoints][3];             // of joint j (1 .. nj) at j - 1
  double off[kNumContacts][3];            // contact_off
  unsigned char path[kNumContacts][kMaxJoints];      // the bodies on the way base -> contact body of point i (at most kMaxBodies)
  int depth[kNumContacts];
};
constexpr int kPlanChainEntries = 3 * kMaxJoints + 3 * kNumContacts + kNumContacts * kMaxJoints + kNumContacts;
PG_HD void plan_chains_fill(const DeviceModel& md, PlanChains& c, int e) {      // entry e of kPlanChainEntries
  if (e < 3 * kMaxJoints) { c.pfix[e / 3][e % 3] = md.pfix[1 + e / 3][e % 3]; return; }
  e -= 3 * kMaxJoints;
  if (e < 3 * kNumContacts) { c.off[e / 3][e % 3] = md.contact_off[e / 3][e % 3]; return; }
  e -= 3 * kNumContacts;
  if (e < kNumContacts * kMaxJoints) { c.path[e / kMaxJoints][e % kMaxJoints] = (unsigned char)md.path[md.contact_body[e / kMaxJoints]][e % kMaxJoints]; return; }
  e -= kNumContacts * kMaxJoints;
  c.depth[e] = md.depth[md.contact_body[e]];
}

// sine and cosine of one base angle: the four walks of a node share them
PG_HD void plan_base_sincos(double angle, double* sc) { sincos(angle, sc, sc + 1); }

// The chain walk of contact i: pos the base position, sc the sines and cosines of the zyx angles (sin yaw, cos yaw, sin pitch, ..), T the
// joint-local rotations of the configuration, joint j (1 .. nj) at T + 9 (j - 1).  wbc_py.fk / contact_points: o_j = o_parent + R_parent pfix_j,
// R_j = R_parent Rfix_j E(q_j); point = o_body + R_body contact_off_i
PG_HD void plan_chain_point(const PlanChains& ch, int i, const double* pos, const double* sc, const double* T, double* pt) {
  double R[9], o[3] = {pos[0], pos[1], pos[2]};
  exact::rot_zyx(sc[0], sc[1], sc[2], sc[3], sc[4], sc[5], R);
  const int depth = ch.depth[i];
  for (int d = 0; d < depth; ++d) {
    const int j = ch.path[i][d];
    exact::chain_step(R, o, ch.pfix[j - 1], T + 9 * (j - 1));
  }
  exact::point_on_body(R, o, ch.off[i], pt);
}

// Centre of pressure of four points p [4][3] under the normal forces fz [4]: sum_z = ((fz0 + fz1) + fz2) + fz3; with sum_z > 0
// cop = ((w0 p0 + w1 p1) + w2 p2) + w3 p3 per component, w_i = fz_i / sum_z; else 0.  Returns sum_z.
PG_HD double plan_cop(const double* fz, const double* p, double* cop) {
#pragma clang fp contract(off)
  const double sum_z = ((fz[0] + fz[1]) + fz[2]) + fz[3];
  cop[0] = cop[1] = cop[2] = 0.0;
  if (sum_z > 0.0) {
    const double w0 = fz[0] / sum_z, w1 = fz[1] / sum_z, w2 = fz[2] / sum_z, w3 = fz[3] / sum_z;
    for (int c = 0; c < 3; ++c) cop[c] = ((w0 * p[c] + w1 * p[3 + c]) + w2 * p[6 + c]) + w3 * p[9 + c];
  }
  return sum_z;
}

// Everything of a row but its contact points (entries 3..14, which the chain walks have written): x the node's state or reference, u the node's
// input (NULL: the last node, the desired block, a plan without inputs), mode and kind -1 for the last node
PG_HD void plan_row_tail(double* row, const double* x, const double* u, double t, int mode, int kind, bool not_finite) {
  for (int c = 0; c < 3; ++c) row[kPgBase + c] = x[6 + c];
  double sum_z = 0.0;
  row[kPgCop] = row[kPgCop + 1] = row[kPgCop + 2] = 0.0;
  if (u) {
    const double fz[4] = {u[2], u[5], u[8], u[11]};
    sum_z = plan_cop(fz, row + kPgContact, row + kPgCop);
  }
  row[kPgTime] = t;
  row[kPgMode] = (double)mode;
  row[kPgKind] = (double)kind;
  row[kPgSumZ] = sum_z;
  row[kPgMask] = (double)plan_contact_mask(mode);
  row[kPgBad] = not_finite ? 1.0 : 0.0;
}

// The foothold predicate on the rows [n + 1][24] of a robot: the contact points that land at node k, as a bit mask.  k is a pre-event node
// strictly inside the horizon; `pre` is the mode of the nearest intermediate node before it, `post` of the nearest one after it (among the nodes
// 0 .. n - 1; without either there is no foothold); point i lands when !flag(pre, i) && flag(post, i).
PG_HD int plan_landing_mask(const double* rows, int k, int n) {
  const double* r = rows + (size_t)k * kPlanNodeStride;
  if (r[kPgKind] != 1.0) return 0;
  const double t = r[kPgTime];
  if (!(rows[kPgTime] < t && t < rows[(size_t)n * kPlanNodeStride + kPgTime])) return 0;
  int pre = -1, post = -1;
  for (int j = k - 1; j >= 0 && pre < 0; --j)
    if (rows[(size_t)j * kPlanNodeStride + kPgKind] == 0.0) pre = (int)rows[(size_t)j * kPlanNodeStride + kPgMode];
  for (int j = k + 1; j < n && post < 0; ++j)
    if (rows[(size_t)j * kPlanNodeStride + kPgKind] == 0.0) post = (int)rows[(size_t)j * kPlanNodeStride + kPgMode];
  if (pre < 0 || post < 0) return 0;
  return ~plan_contact_mask(pre) & plan_contact_mask(post);
}

// One foothold entry: contact point i that lands at the pre-event node k is taken from the row of the post-event node k + 1
PG_HD void plan_foothold_entry(const double* rows, int k, int i, double* entry) {
  const double* r = rows + (size_t)(k + 1) * kPlanNodeStride;
  entry[0] = r[kPgTime];
  entry[1] = (double)i;
  for (int c = 0; c < 3; ++c) entry[2 + c] = r[kPgContact + 3 * i + c];
  entry[5] = (double)(k + 1);
}

// The summary of a robot is accumulated in 64 accumulators: node k updates accumulator k mod 64 (a lane of the reducing wavefront), with k
// ascending; then the accumulators are merged.  A row that is flagged not finite is counted and takes part in nothing else.
struct PlanAcc {
  double path, apex[kNumContacts], drift[kNumContacts], min_sum_z;
  int bad;
};
PG_HD void plan_acc_init(PlanAcc& a) {
  a.path = 0.0; a.min_sum_z = HUGE_VAL; a.bad = 0;
  for (int i = 0; i < kNumContacts; ++i) { a.apex[i] = -HUGE_VAL; a.drift[i] = 0.0; }
}
// node k of the rows [n + 1][24]: the apexes, the smallest sum_z; with its successor k + 1 the path segment sqrt((dx dx + dy dy) + dz dz) and the
// stance drift sqrt(dx dx + dy dy) of every point that both modes hold in contact.  Comparisons are `>` and `<`: a NaN changes nothing.
PG_HD void plan_acc_node(PlanAcc& a, const double* rows, int k, int n) {
#pragma clang fp contract(off)
  const double* r = rows + (size_t)k * kPlanNodeStride;
  if (r[kPgBad] != 0.0) { a.bad += 1; return; }
  for (int i = 0; i < kNumContacts; ++i)
    if (r[kPgContact + 3 * i + 2] > a.apex[i]) a.apex[i] = r[kPgContact + 3 * i + 2];
  if (r[kPgKind] == 0.0 && r[kPgMask] != 0.0 && r[kPgSumZ] < a.min_sum_z) a.min_sum_z = r[kPgSumZ];
  if (k >= n) return;
  const double* s = r + kPlanNodeStride;
  if (s[kPgBad] != 0.0) return;
  const double dx = s[0] - r[0], dy = s[1] - r[1], dz = s[2] - r[2];
  a.path += sqrt((dx * dx + dy * dy) + dz * dz);
  const int both = (int)r[kPgMask] & (int)s[kPgMask];
  for (int i = 0; i < kNumContacts; ++i) {
    if (!((both >> i) & 1)) continue;
    const double ex = s[kPgContact + 3 * i] - r[kPgContact + 3 * i], ey = s[kPgContact + 3 * i + 1] - r[kPgContact + 3 * i + 1];
    const double d = sqrt(ex * ex + ey * ey);
    if (d > a.drift[i]) a.drift[i] = d;
  }
}
// the maxima, the minimum and the count of `b` into `a` (exact in any order); the path lengths are added by the caller, accumulator 0, 1, .. 63
PG_HD void plan_acc_merge(PlanAcc& a, const PlanAcc& b) {
  for (int i = 0; i < kNumContacts; ++i) {
    if (b.apex[i] > a.apex[i]) a.apex[i] = b.apex[i];
    if (b.drift[i] > a.drift[i]) a.drift[i] = b.drift[i];
  }
  if (b.min_sum_z < a.min_sum_z) a.min_sum_z = b.min_sum_z;
  a.bad += b.bad;
}
// the merged accumulator, its path length the sum over the 64 accumulators in ascending order, as a summary row; an apex or a smallest sum_z
// that no row contributed to is 0
PG_HD void plan_summary_row(const PlanAcc& a, int n, int footholds, double* row) {
  row[kPsNodes] = (double)n;
  row[kPsFootholds] = (double)footholds;
  row[kPsPath] = a.path;
  for (int i = 0; i < kNumContacts; ++i) { row[kPsApex + i] = a.apex[i] == -HUGE_VAL ? 0.0 : a.apex[i]; row[kPsDrift + i] = a.drift[i]; }
  row[kPsMinSumZ] = a.min_sum_z == HUGE_VAL ? 0.0 : a.min_sum_z;
  row[kPsBad] = (double)a.bad;
  for (int c = kPsBad + 1; c < kPlanSummaryStride; ++c) row[c] = 0.0;
}

// ------------------------------------------------------------------------------------------------ the kernels' bodies

// One description of a plan for the three sources (the solver's iterate, a policy slot, stand-alone arrays): the grid tables one row per GRID,
// p_grid the grid of a robot (NULL: robot b reads row b).  in_N is the node stride of the source, N that of the outputs.
struct PlanArgs {
  int batch, N, in_N, tiles, blocks;      // tiles: of 16 nodes, enough for the longest plan; blocks: 1 optimized only, 2 with the desired block
  const double *x, *u, *xref;             // [batch][in_N + 1][NX], [batch][in_N][NU] nullable, [batch][in_N][NX] (blocks == 2)
  const double* g_time;                   // [grids][in_N + 1]
  const int *g_kind, *g_mode, *g_nodes, *p_grid;      // [grids][in_N], [grids][in_N], [grids], [batch] nullable
  double *optimized, *desired;            // [max_batch][N + 1][24]
  double *footholds, *summary;            // [max_batch][16][6], [max_batch][16]
  int* count;                             // [max_batch]
};

template <int NJ>
struct PlanTileLds {
  double xs[kPlanTile][12 + NJ];          // the tile's states
  double T[kPlanTile][NJ][9];             // joint-local rotations
  double sc[kPlanTile][6];                // sines and cosines of the base angles
  double rows[kPlanTile][kPlanNodeStride];
  PlanChains chains;
  int bad[kPlanTile];
};

// a device n_nodes is clamped: to what the source holds and to what the outputs hold
__device__ __forceinline__ int plan_nodes_of(const PlanArgs& a, int g) {
  const int n = a.g_nodes[g], cap = a.in_N < a.N ? a.in_N : a.N;
  return n < 0 ? 0 : (n > cap ? cap : n);
}

// Tile `tile` of block `which` (0 optimized, 1 desired) of robot b on one wavefront.  Nodes beyond the block's last node (n_nodes for the
// optimized block; n_nodes - 1 for the desired one: the last node has no reference) are neither computed nor written.
template <int NJ>
__device__ __forceinline__ void plan_tile(const DeviceModel& md, PlanTileLds<NJ>& w, const PlanArgs& a, int b, int which, int tile, int lane) {
  constexpr int NX = 12 + NJ, NU = 12 + NJ;
  const int g = a.p_grid ? a.p_grid[b] : b;
  const int n = plan_nodes_of(a, g);
  const int k0 = tile * kPlanTile, last = which == 0 ? n : n - 1;
  if (k0 > last) return;                                      // the whole wavefront
  const int cnt = last - k0 + 1 < kPlanTile ? last - k0 + 1 : kPlanTile;
  const double* src = which == 0 ? a.x + ((size_t)b * (a.in_N + 1) + k0) * NX : a.xref + ((size_t)b * a.in_N + k0) * NX;
  double* xs = &w.xs[0][0];
  if (lane < kPlanTile) w.bad[lane] = 0;
  for (int e = lane; e < kPlanChainEntries; e += kWave) plan_chains_fill(md, w.chains, e);
  lds_wave_sync();
  for (int c = lane; c < cnt * NX; c += kWave) {
    const double v = src[c];
    xs[c] = v;
    if (!isfinite(v)) w.bad[c / NX] = 1;
  }
  lds_wave_sync();
  for (int p = lane; p < cnt * (NJ + 3); p += kWave) {         // A: every (node, joint) pair, then every (node, base angle) pair
    if (p < cnt * NJ) plan_joint_rotation(md, p % NJ + 1, w.xs[p / NJ][12 + p % NJ], w.T[p / NJ][p % NJ]);
    else { const int q = p - cnt * NJ; plan_base_sincos(w.xs[q / 3][9 + q % 3], &w.sc[q / 3][2 * (q % 3)]); }
  }
  lds_wave_sync();
  {                                                            // B
    const int nd = lane / kNumContacts, i = lane % kNumContacts;
    if (nd < cnt) plan_chain_point(w.chains, i, &w.xs[nd][6], w.sc[nd], &w.T[nd][0][0], &w.rows[nd][kPgContact + 3 * i]);
  }
  lds_wave_sync();
  if (lane < cnt) {                                            // C
    const int k = k0 + lane;
    const bool is_last = k == n;
    const int mode = is_last ? -1 : a.g_mode[(size_t)g * a.in_N + k], kind = is_last ? -1 : a.g_kind[(size_t)g * a.in_N + k];
    const double* u = (which == 0 && a.u && !is_last) ? a.u + ((size_t)b * a.in_N + k) * NU : nullptr;
    plan_row_tail(w.rows[lane], w.xs[lane], u, a.g_time[(size_t)g * (a.in_N + 1) + k], mode, kind, w.bad[lane] != 0);
  }
  lds_wave_sync();
  double* dst = (which == 0 ? a.optimized : a.desired) + ((size_t)b * (a.N + 1) + k0) * kPlanNodeStride;
  const double* rows = &w.rows[0][0];
  for (int c = lane; c < cnt * kPlanNodeStride; c += kWave) dst[c] = rows[c];
  lds_wave_sync();                                             // the next tile of this wavefront reuses the workspace
}

// Footholds and summary of robot b from its optimized rows, on one wavefront: node k of a chunk of 64 on lane k mod 64
__device__ __forceinline__ void plan_reduce(const PlanArgs& a, int b, int lane) {
  const int g = a.p_grid ? a.p_grid[b] : b;
  const int n = plan_nodes_of(a, g);
  const double* rows = a.optimized + (size_t)b * (a.N + 1) * kPlanNodeStride;
  double* entries = a.footholds + (size_t)b * kPlanMaxFootholds * kPlanFootholdStride;
  const unsigned long long below = (1ull << lane) - 1ull;
  PlanAcc acc;
  plan_acc_init(acc);
  int total = 0;
  for (int c0 = 0; c0 <= n; c0 += kWave) {
    const int k = c0 + lane;
    int landing = 0;
    if (k <= n) {
      plan_acc_node(acc, rows, k, n);
      landing = plan_landing_mask(rows, k, n);
    }
    int before = 0, chunk = 0;                                 // entries of lower lanes, entries of the chunk
    for (int i = 0; i < kNumContacts; ++i) {
      const unsigned long long bal = __ballot((landing >> i) & 1);
      before += __popcll(bal & below);
      chunk += __popcll(bal);
    }
    for (int i = 0, slot = total + before; i < kNumContacts; ++i) {
      if (!((landing >> i) & 1)) continue;
      if (slot < kPlanMaxFootholds) plan_foothold_entry(rows, k, i, entries + slot * kPlanFootholdStride);
      ++slot;
    }
    total += chunk;
  }
  for (int s = 1; s < kWave; s <<= 1) {                        // maxima, minimum and count: a butterfly, every lane ends with all of them
    PlanAcc o;
    for (int i = 0; i < kNumContacts; ++i) { o.apex[i] = __shfl_xor(acc.apex[i], s); o.drift[i] = __shfl_xor(acc.drift[i], s); }
    o.min_sum_z = __shfl_xor(acc.min_sum_z, s);
    o.bad = __shfl_xor(acc.bad, s);
    plan_acc_merge(acc, o);
  }
  double path = 0.0;                                           // the path lengths of the lanes in ascending order
  const double mine = acc.path;
  for (int l = 0; l < kWave; ++l) path += readlane_f64(mine, l);
  acc.path = path;
  if (lane == 0) {
    plan_summary_row(acc, n, total, a.summary + (size_t)b * kPlanSummaryStride);
    a.count[b] = total;
  }
}

}  // namespace bpmpc
