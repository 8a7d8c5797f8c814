// Host-only part of the C ABI (include/bpmpc.h): model ingest, the reference-manager pre-pass and the error model (capi_internal.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "cone_params.h"
#include "estimator.h"
#include "info_tree.h"
#include "plant.h"
#include "reference_gen.h"

struct bpmpc_model { bpmpc::RobotModel rm; };
struct bpmpc_gait { std::unique_ptr<bpmpc::GaitSchedule> schedule; };

namespace bpmpc {
namespace {
thread_local std::string g_last_error;
}
void set_last_error(const std::string& message) { g_last_error = message; }
const RobotModel& model_of(const bpmpc_model* handle) { return handle->rm; }

int translate(const std::exception& e, int fallback) {
  set_last_error(e.what());
  if (dynamic_cast<const DeviceError*>(&e)) return BPMPC_ERR_DEVICE;
  if (dynamic_cast<const Unsupported*>(&e)) return BPMPC_ERR_UNSUPPORTED;
  if (dynamic_cast<const std::invalid_argument*>(&e)) return BPMPC_ERR_INVALID_ARGUMENT;
  if (dynamic_cast<const std::length_error*>(&e)) return BPMPC_ERR_CAPACITY;
  return fallback;
}

namespace {
const char* const kEstParamNames[] = {"footRadius", "imuProcessNoisePosition", "imuProcessNoiseVelocity", "footProcessNoisePosition",
                                      "footSensorNoisePosition", "footSensorNoiseVelocity", "footHeightSensorNoise"};
}

void estimator_check_param_row(const char* who, const double* row, int r) {
  for (int e = 0; e < kEstParamStride - 1; ++e) {
    const bool positive = e >= 4;
    if (!std::isfinite(row[e]) || row[e] < 0.0 || (positive && row[e] == 0.0))
      throw std::invalid_argument(std::string(who) + ": row " + std::to_string(r) + ", entry " + std::to_string(e) + " (" + kEstParamNames[e] + ") is " +
                                  (!std::isfinite(row[e]) ? "not finite" : row[e] < 0.0 ? "negative" : "zero"));
  }
}

EstSettings estimator_load_settings(const char* task_info_path) {
  EstSettings s{0.02, 0.02, 0.02, 0.002, 0.005, 0.1, 0.01, 0.0};      // LinearKalmanFilter.h:45-51
  if (task_info_path) {
    // [OCS2-upstream] loadData::loadPtreeValue keeps the member's initial value when the key is absent
    const auto t = read_info_file(task_info_path);
    double* v = &s.foot_radius;
    for (int e = 0; e < kEstParamStride - 1; ++e) (void)t->get(std::string("kalmanFilter.") + kEstParamNames[e], v + e);
    estimator_check_param_row("kalmanFilter settings", v, 0);
  }
  return s;
}

namespace {
const char* const kPlantParamNames[] = {"kn", "cn", "d0", "mu", "v_eps", "contact_threshold"};
constexpr int kPlantParamUsed = 6;
}

void plant_check_param_row(const char* who, const double* row, int r) {
  for (int e = 0; e < kPlantParamUsed; ++e) {
    const bool positive = e == 0 || e == 2 || e == 4;
    if (!std::isfinite(row[e]) || row[e] < 0.0 || (positive && row[e] == 0.0))
      throw std::invalid_argument(std::string(who) + ": row " + std::to_string(r) + ", entry " + std::to_string(e) + " (" + kPlantParamNames[e] + ") is " +
                                  (!std::isfinite(row[e]) ? "not finite" : row[e] < 0.0 ? "negative" : "zero"));
  }
}

PlantSettings plant_load_settings(const char* task_info_path) {
  PlantSettings s{5e4, 5e2, 1e-3, 0.7, 0.01, 1.0, {0.0, 0.0}};      // include/bpmpc.h "Plant"
  if (task_info_path) {
    const auto t = read_info_file(task_info_path);
    double* v = &s.kn;
    for (int e = 0; e < kPlantParamUsed; ++e) (void)t->get(std::string("plant.") + kPlantParamNames[e], v + e);
    plant_check_param_row("plant settings", v, 0);
  }
  return s;
}

double plant_load_stiction(const char* task_info_path) {
  double kt = 0.0;
  if (task_info_path) {
    const auto t = read_info_file(task_info_path);
    (void)t->get("plant.kt", &kt);
    if (!std::isfinite(kt) || kt < 0.0) throw std::invalid_argument(std::string("plant settings: kt is ") + (!std::isfinite(kt) ? "not finite" : "negative"));
  }
  return kt;
}

namespace {
const char* const kSensorParamNames[] = {"gyro_noise", "gyro_bias_walk", "gyro_bias_init", "accel_noise", "accel_bias_walk", "accel_bias_init", "orientation_noise",
                                         "joint_pos_noise", "joint_pos_resolution", "joint_vel_noise", "contact_dropout", "delay_steps"};
static_assert(sizeof(kSensorParamNames) / sizeof(kSensorParamNames[0]) == kSensorParamUsed, "a name per used entry of a sensor row");
}

void plant_check_sensor_row(const char* who, const double* row, int r) {
  for (int e = 0; e < kSensorParamStride; ++e) {
    const char* name = e < kSensorParamUsed ? kSensorParamNames[e] : "reserved";
    const char* why = !std::isfinite(row[e])                                            ? "not finite"
                      : row[e] < 0.0                                                    ? "negative"
                      : e == kSensContactDropout && row[e] > 1.0                        ? "above 1"
                      : e == kSensDelaySteps && row[e] != std::floor(row[e])            ? "not an integer"
                      : e == kSensDelaySteps && row[e] > (double)kSensorMaxDelay        ? "above 8"
                      : e >= kSensorParamUsed && row[e] != 0.0                          ? "not zero"
                                                                                        : nullptr;
    if (why) throw std::invalid_argument(std::string(who) + ": row " + std::to_string(r) + ", entry " + std::to_string(e) + " (" + name + ") is " + why);
  }
}

void plant_load_sensor_settings(const char* task_info_path, double* row, long* seed) {
  double v[kSensorParamStride] = {};
  double s = 0.0;
  if (task_info_path) {
    const auto t = read_info_file(task_info_path);
    for (int e = 0; e < kSensorParamUsed; ++e) (void)t->get(std::string("plantSensors.") + kSensorParamNames[e], v + e);
    plant_check_sensor_row("plantSensors settings", v, 0);
    (void)t->get("plantSensors.seed", &s);
    if (!std::isfinite(s) || s != std::floor(s) || std::fabs(s) > 9007199254740992.0)
      throw std::invalid_argument("plantSensors settings: seed is not an integer a double holds exactly");
  }
  std::copy(v, v + kSensorParamStride, row);
  if (seed) *seed = (long)s;
}

namespace {
const char* const kInputParamNames[] = {"delay", "dropout", "push_force", "push_interval", "push_duration"};
static_assert(sizeof(kInputParamNames) / sizeof(kInputParamNames[0]) == kInputParamUsed, "a name per used entry of an input row");
}

void plant_check_input_row(const char* who, const double* row, int r) {
  for (int e = 0; e < kInputParamStride; ++e) {
    const char* name = e < kInputParamUsed ? kInputParamNames[e] : "reserved";
    const char* why = !std::isfinite(row[e])                       ? "not finite"
                      : row[e] < 0.0                               ? "negative"
                      : e == kInDropout && row[e] > 1.0            ? "above 1"
                      : e >= kInputParamUsed && row[e] != 0.0      ? "not zero"
                                                                   : nullptr;
    if (why) throw std::invalid_argument(std::string(who) + ": row " + std::to_string(r) + ", entry " + std::to_string(e) + " (" + name + ") is " + why);
  }
}

void plant_load_input_settings(const char* task_info_path, double* row, long* seed) {
  double v[kInputParamStride] = {};
  double s = 0.0;
  if (task_info_path) {
    const auto t = read_info_file(task_info_path);
    for (int e = 0; e < kInputParamUsed; ++e) (void)t->get(std::string("plantInputs.") + kInputParamNames[e], v + e);
    plant_check_input_row("plantInputs settings", v, 0);
    (void)t->get("plantInputs.seed", &s);
    if (!std::isfinite(s) || s != std::floor(s) || std::fabs(s) > 9007199254740992.0)
      throw std::invalid_argument("plantInputs settings: seed is not an integer a double holds exactly");
  }
  std::copy(v, v + kInputParamStride, row);
  if (seed) *seed = (long)s;
}

namespace {
const char* const kJointBlockNames[] = {"armature", "damping", "friction_loss", "lower", "upper"};
}

void plant_check_joint_row(const char* who, const double* row, int r, int nj) {
  auto refuse = [&](int e, const std::string& name, const char* why) {
    throw std::invalid_argument(std::string(who) + ": row " + std::to_string(r) + ", entry " + std::to_string(e) + " (" + name + ") is " + why);
  };
  for (int block = 0; block < 5; ++block)
    for (int j = 0; j < nj; ++j) {
      const int e = block * kPlantJointSlots + j;
      const std::string name = std::string(kJointBlockNames[block]) + "[" + std::to_string(j) + "]";
      const double x = row[e];
      if (std::isnan(x)) refuse(e, name, "not a number");
      if (block < 3 && !std::isfinite(x)) refuse(e, name, "not finite");
      if (block < 3 && x < 0.0) refuse(e, name, "negative");
      if (block == 3 && x == HUGE_VAL) refuse(e, name, "+inf");
      if (block == 4 && x == -HUGE_VAL) refuse(e, name, "-inf");
      if (block == 4 && !(row[kJointLower + j] < x)) refuse(e, name, "not above lower");
    }
  const char* const scalars[] = {"k_limit", "c_limit", "w_eps"};
  for (int e = kJointKLimit; e <= kJointWEps; ++e) {
    const double x = row[e];
    if (!std::isfinite(x)) refuse(e, scalars[e - kJointKLimit], "not finite");
    if (x < 0.0) refuse(e, scalars[e - kJointKLimit], "negative");
    if (e == kJointWEps && x == 0.0) refuse(e, scalars[e - kJointKLimit], "zero");
  }
  if (row[kJointParamUsed] != 0.0) refuse(kJointParamUsed, "reserved", "not zero");
}

bool plant_joint_row_neutral(const double* row, int nj) {
  for (int j = 0; j < nj; ++j)
    if (row[kJointArmature + j] != 0.0 || row[kJointDamping + j] != 0.0 || row[kJointFriction + j] != 0.0 || row[kJointLower + j] != -HUGE_VAL ||
        row[kJointUpper + j] != HUGE_VAL)
      return false;
  return true;
}

void plant_load_joint_settings(const RobotModel& rm, const char* task_info_path, double* row) {
  double v[kPlantJointParamStride] = {};
  for (int j = 0; j < kPlantJointSlots; ++j) { v[kJointLower + j] = -HUGE_VAL; v[kJointUpper + j] = HUGE_VAL; }
  v[kJointKLimit] = kPlantJointKLimit; v[kJointCLimit] = kPlantJointCLimit; v[kJointWEps] = kPlantJointWEps;
  if (task_info_path) {
    const auto t = read_info_file(task_info_path);
    double from_urdf = 0.0;
    (void)t->get("plantJoints.fromUrdf", &from_urdf);
    if (from_urdf != 0.0)
      for (int j = 0; j < rm.nj; ++j) {
        v[kJointLower + j] = rm.joint_lower[1 + j]; v[kJointUpper + j] = rm.joint_upper[1 + j];
        v[kJointDamping + j] = rm.joint_damping[1 + j]; v[kJointFriction + j] = rm.joint_friction[1 + j];
      }
    const char* const per_joint[] = {"armature", "damping", "frictionLoss"};
    for (int block = 0; block < 3; ++block) {
      double x = 0.0;
      if (t->get(std::string("plantJoints.") + per_joint[block], &x))
        for (int j = 0; j < rm.nj; ++j) v[block * kPlantJointSlots + j] = x;
    }
    (void)t->get("plantJoints.kLimit", v + kJointKLimit);
    (void)t->get("plantJoints.cLimit", v + kJointCLimit);
    (void)t->get("plantJoints.wEps", v + kJointWEps);
    plant_check_joint_row("plantJoints settings", v, 0, rm.nj);
  }
  std::copy(v, v + kPlantJointParamStride, row);
}

namespace {
const char* const kBodyBlockNames[] = {"mass", "com_x", "com_y", "com_z", "ixx", "ixy", "ixz", "iyy", "iyz", "izz"};

// The eigenvalues of the symmetric 3 x 3 (xx, xy, xz, yy, yz, zz) by cyclic Jacobi rotations, ascending
void sym3_eigenvalues(const double* s, double* ev) {
  double a[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
  for (int sweep = 0; sweep < 32; ++sweep) {
    const double off = std::fabs(a[0][1]) + std::fabs(a[0][2]) + std::fabs(a[1][2]);
    if (off == 0.0) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (a[p][q] == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < 3; ++k) { const double akp = a[k][p], akq = a[k][q]; a[k][p] = c * akp - sn * akq; a[k][q] = sn * akp + c * akq; }
        for (int k = 0; k < 3; ++k) { const double apk = a[p][k], aqk = a[q][k]; a[p][k] = c * apk - sn * aqk; a[q][k] = sn * apk + c * aqk; }
        a[p][q] = a[q][p] = 0.0;
      }
  }
  ev[0] = a[0][0]; ev[1] = a[1][1]; ev[2] = a[2][2];
  std::sort(ev, ev + 3);
}
}  // namespace

void plant_body_model_row(const RobotModel& rm, double* row) {
  std::fill(row, row + kPlantBodyParamStride, 0.0);
  for (int b = 0; b <= rm.nj; ++b) {
    row[kBodyMass + b] = rm.mass[b];
    for (int k = 0; k < 3; ++k) row[kBodyCom + k * kPlantBodySlots + b] = rm.com[b][k];
    const double* I = rm.inertia[b];      // 3 x 3, row major: the entries of its upper triangle
    const double six[6] = {I[0], I[1], I[2], I[4], I[5], I[8]};
    for (int k = 0; k < 6; ++k) row[kBodyInertia + k * kPlantBodySlots + b] = six[k];
  }
}

void plant_check_body_row(const char* who, const double* row, int r, int nj) {
  auto refuse = [&](int e, const std::string& name, const char* why) {
    throw std::invalid_argument(std::string(who) + ": row " + std::to_string(r) + ", entry " + std::to_string(e) + " (" + name + ") is " + why);
  };
  for (int b = 0; b <= nj; ++b) {
    const std::string at = "[" + std::to_string(b) + "]";
    for (int block = 0; block < 10; ++block) {
      const int e = block * kPlantBodySlots + b;
      const double x = row[e];
      if (std::isnan(x)) refuse(e, kBodyBlockNames[block] + at, "not a number");
      if (!std::isfinite(x)) refuse(e, kBodyBlockNames[block] + at, "not finite");
      if (block == 0 && x < 0.0) refuse(e, kBodyBlockNames[block] + at, "negative");
      if (block == 0 && x == 0.0) refuse(e, kBodyBlockNames[block] + at, "zero");
    }
    double s[6], ev[3];
    for (int k = 0; k < 6; ++k) s[k] = row[kBodyInertia + k * kPlantBodySlots + b];
    sym3_eigenvalues(s, ev);
    if (!(ev[0] > 0.0)) refuse(kBodyInertia + b, "inertia" + at, "not positive definite");
    // no mass distribution has a principal moment above the sum of the other two; 1e-9: the rounding of a rod's or a point's row, not a licence
    if (ev[2] > (ev[0] + ev[1]) * (1.0 + 1e-9)) refuse(kBodyInertia + b, "inertia" + at, "against the triangle inequality of its principal moments");
  }
}

void plant_compose_body_row(const char* who, const double* row_in, int nj, int body, double mass_scale, const double* com_shift, double payload_mass,
                            const double* payload_pos, double* row_out) {
  const std::string w(who);
  if (body < -1 || body > nj) throw std::invalid_argument(w + ": body must be -1 or 0.." + std::to_string(nj));
  if (!std::isfinite(mass_scale) || mass_scale <= 0.0) throw std::invalid_argument(w + ": mass_scale must be finite and positive");
  if (!std::isfinite(payload_mass) || payload_mass < 0.0) throw std::invalid_argument(w + ": payload_mass must be finite and not negative");
  for (int k = 0; k < 3; ++k) {
    if (com_shift && !std::isfinite(com_shift[k])) throw std::invalid_argument(w + ": com_shift is not finite");
    if (payload_pos && !std::isfinite(payload_pos[k])) throw std::invalid_argument(w + ": payload_pos is not finite");
  }
  if (body >= 0 && payload_mass > 0.0 && !payload_pos) throw std::invalid_argument(w + ": a payload needs payload_pos");
  double v[kPlantBodyParamStride];
  std::copy(row_in, row_in + kPlantBodyParamStride, v);
  auto scale = [&](int b) {
    v[kBodyMass + b] *= mass_scale;
    for (int k = 0; k < 6; ++k) v[kBodyInertia + k * kPlantBodySlots + b] *= mass_scale;
  };
  if (body < 0) {
    for (int b = 0; b <= nj; ++b) scale(b);
  } else {
    scale(body);
    double c[3], I[6];
    for (int k = 0; k < 3; ++k) c[k] = v[kBodyCom + k * kPlantBodySlots + body] + (com_shift ? com_shift[k] : 0.0);
    for (int k = 0; k < 6; ++k) I[k] = v[kBodyInertia + k * kPlantBodySlots + body];
    double m = v[kBodyMass + body];
    if (payload_mass > 0.0) {
      const double total = m + payload_mass;
      double cn[3];
      for (int k = 0; k < 3; ++k) cn[k] = (m * c[k] + payload_mass * payload_pos[k]) / total;
      // parallel axes: each part's inertia about the common centre of mass gains mass (|d|^2 E - d d')
      auto shift = [&](double mass, const double* from) {
        const double d[3] = {from[0] - cn[0], from[1] - cn[1], from[2] - cn[2]};
        const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        I[0] += mass * (dd - d[0] * d[0]); I[1] -= mass * d[0] * d[1]; I[2] -= mass * d[0] * d[2];
        I[3] += mass * (dd - d[1] * d[1]); I[4] -= mass * d[1] * d[2]; I[5] += mass * (dd - d[2] * d[2]);
      };
      shift(m, c);
      shift(payload_mass, payload_pos);
      m = total;
      for (int k = 0; k < 3; ++k) c[k] = cn[k];
    }
    v[kBodyMass + body] = m;
    for (int k = 0; k < 3; ++k) v[kBodyCom + k * kPlantBodySlots + body] = c[k];
    for (int k = 0; k < 6; ++k) v[kBodyInertia + k * kPlantBodySlots + body] = I[k];
  }
  for (int block = 0; block < 10; ++block)
    for (int b = nj + 1; b < kPlantBodySlots; ++b) v[block * kPlantBodySlots + b] = 0.0;
  std::copy(v, v + kPlantBodyParamStride, row_out);
}

bool plant_body_rows_equal(const double* a, const double* b, int nj) {
  for (int block = 0; block < 10; ++block)
    if (std::memcmp(a + block * kPlantBodySlots, b + block * kPlantBodySlots, (size_t)(nj + 1) * sizeof(double)) != 0) return false;
  return true;
}

void plant_load_body_settings(const RobotModel& rm, const char* task_info_path, double* row) {
  double v[kPlantBodyParamStride];
  plant_body_model_row(rm, v);
  if (task_info_path) {
    const auto t = read_info_file(task_info_path);
    double scale = 1.0, payload = 0.0;
    int body = 0;
    const bool scaled = t->get("plantBodies.massScale", &scale);
    const bool loaded = t->get("plantBodies.payloadMass", &payload);
    (void)t->get("plantBodies.payloadBody", &body);
    if (scaled && scale != 1.0) plant_compose_body_row("plantBodies settings (massScale)", v, rm.nj, -1, scale, nullptr, 0.0, nullptr, v);
    if (loaded && payload != 0.0) {
      double pos[3] = {0.0, 0.0, 0.0};
      if (t->find("plantBodies.payloadOffset")) {
        const std::vector<double> off = load_matrix(*t, "plantBodies.payloadOffset", 3, 1);
        for (int k = 0; k < 3; ++k) pos[k] = off[k];
      }
      plant_compose_body_row("plantBodies settings (payload)", v, rm.nj, body, 1.0, nullptr, payload, pos, v);
    }
    if (scaled || loaded) plant_check_body_row("plantBodies settings", v, 0, rm.nj);
  }
  std::copy(v, v + kPlantBodyParamStride, row);
}
}  // namespace bpmpc

using namespace bpmpc;

namespace {
int fail(int code, const std::string& why) { set_last_error(why); return code; }

int copy_out(const double* src, size_t n, double* out, int capacity) {
  if ((size_t)capacity < n) throw std::length_error("output capacity too small");
  std::copy(src, src + n, out);
  return (int)n;
}

// A bpmpc_*_load_*params call behind its null check: load(v) fills a row of STRIDE doubles, which is copied out only when nothing was thrown
template <int STRIDE, typename Load>
int load_into_row(double* row, Load&& load) {
  return guarded(BPMPC_ERR_IO, [&] {
    double v[STRIDE];
    load(v);
    std::copy(v, v + STRIDE, row);
  });
}

// A bpmpc_*_check_*params call behind its refusals: check(row, r) for each of the n_rows rows of `stride` doubles
template <typename Check>
int check_n_rows(const double* rows, int n_rows, int stride, Check&& check) {
  return guarded(BPMPC_ERR_IO, [&] {
    for (int r = 0; r < n_rows; ++r) check(rows + (size_t)r * stride, r);
  });
}
}  // namespace

extern "C" {

const char* bpmpc_last_error(void) { return g_last_error.c_str(); }
const char* bpmpc_version(void) { return "bpmpc 0.1 (gfx950, fp64)"; }

int bpmpc_model_create(const char* urdf, const char* task, const char* reference, bpmpc_model** out) {
  if (!urdf || !task || !reference || !out) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_model_create: null argument");
  *out = nullptr;
  return guarded(BPMPC_ERR_IO, [&] {
    auto m = std::make_unique<bpmpc_model>();
    m->rm = load_robot_model(urdf, task, reference);
    *out = m.release();
    return (int)BPMPC_OK;
  });
}
int bpmpc_model_create_ex(const char* urdf, const char* task, const char* reference, int use_hard_friction_cone, bpmpc_model** out) {
  const int rc = bpmpc_model_create(urdf, task, reference, out);
  if (rc == BPMPC_OK) (*out)->rm.hard_friction_cone = use_hard_friction_cone != 0;
  return rc;
}
void bpmpc_model_destroy(bpmpc_model* m) { delete m; }

int bpmpc_model_dims(const bpmpc_model* m, int* nx, int* nu, int* n_contacts, int* n_joints) {
  if (!m) return fail(BPMPC_ERR_INVALID_ARGUMENT, "null model");
  if (nx) *nx = m->rm.nx;
  if (nu) *nu = m->rm.nu;
  if (n_contacts) *n_contacts = kNumContacts;
  if (n_joints) *n_joints = m->rm.nj;
  return BPMPC_OK;
}

int bpmpc_model_get(const bpmpc_model* m, const char* name, double* out, int capacity) {
  if (!m || !name || !out) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_model_get: null argument");
  return guarded(BPMPC_ERR_IO, [&]() -> int {
    const RobotModel& r = m->rm;
    const std::string n(name);
    const int nj = r.nj, nb = nj + 1;
    auto scalar = [&](double v) { return copy_out(&v, 1, out, capacity); };
    auto list = [&](std::initializer_list<double> v) { std::vector<double> t(v); return copy_out(t.data(), t.size(), out, capacity); };
    if (n == "initial_state") return copy_out(r.initial_state.data(), r.initial_state.size(), out, capacity);
    if (n == "default_joint_state") return copy_out(r.default_joint_state.data(), r.default_joint_state.size(), out, capacity);
    if (n == "Q") return copy_out(r.Q.data(), r.Q.size(), out, capacity);
    if (n == "R") return copy_out(r.R.data(), r.R.size(), out, capacity);
    if (n == "robot_mass") return scalar(r.robot_mass);
    if (n == "com_height") return scalar(r.com_height);
    if (n == "time_horizon") return scalar(r.time_horizon);
    if (n == "position_error_gain") return scalar(r.position_error_gain);
    if (n == "phase_transition_stance_time") return scalar(r.phase_transition_stance_time);
    if (n == "body_mass") return copy_out(r.mass, nb, out, capacity);
    if (n == "body_com") return copy_out(&r.com[0][0], 3 * nb, out, capacity);
    if (n == "body_inertia") return copy_out(&r.inertia[0][0], 9 * nb, out, capacity);
    if (n == "joint_rotation") return copy_out(&r.Rfix[1][0], 9 * nj, out, capacity);
    if (n == "joint_offset") return copy_out(&r.pfix[1][0], 3 * nj, out, capacity);
    if (n == "joint_axis") return copy_out(&r.axis[1][0], 3 * nj, out, capacity);
    if (n == "joint_lower") return copy_out(&r.joint_lower[1], nj, out, capacity);
    if (n == "joint_upper") return copy_out(&r.joint_upper[1], nj, out, capacity);
    if (n == "joint_damping") return copy_out(&r.joint_damping[1], nj, out, capacity);
    if (n == "joint_friction") return copy_out(&r.joint_friction[1], nj, out, capacity);
    if (n == "contact_offset") return copy_out(&r.contact_off[0][0], 3 * kNumContacts, out, capacity);
    if (n == "joint_parent") { std::vector<double> t(nj); for (int j = 0; j < nj; ++j) t[j] = r.parent[j + 1]; return copy_out(t.data(), nj, out, capacity); }
    if (n == "contact_body") { std::vector<double> t(kNumContacts); for (int c = 0; c < kNumContacts; ++c) t[c] = r.contact_body[c]; return copy_out(t.data(), t.size(), out, capacity); }
    if (n == "cone") return list({r.friction_coefficient, r.cone_regularization, r.cone_gripper_force, r.cone_hessian_shift, r.barrier_mu, r.barrier_delta});
    if (n == "hard_cone") return list({r.hard_friction_cone ? 1.0 : 0.0, r.sqp_inequality_mu, r.sqp_inequality_delta});
    if (n == "swing") return list({r.swing.lift_off_velocity, r.swing.touch_down_velocity, r.swing.swing_height, r.swing.swing_time_scale});
    if (n == "rollout") return list({r.rollout.abs_tol, r.rollout.rel_tol, r.rollout.time_step, (double)r.rollout.max_steps_per_second, r.mrt_frequency, r.mpc_frequency});
    if (n == "sqp") return list({r.sqp.dt, (double)r.sqp.sqp_iteration, r.sqp.delta_tol, r.sqp.g_max, r.sqp.g_min, (double)r.sqp.use_feedback_policy,
                                 1.0 /* projectStateInputEqualityConstraints */, 0.0 /* integratorType: 0 = RK2 */,
                                 r.sqp.alpha_decay, r.sqp.alpha_min, r.sqp.gamma_c, r.sqp.armijo_factor, r.sqp.cost_tol});
    // settings blocks the reference loads beside sqp (BipedalRobotInterface.cpp:98-100); field order documented in include/bpmpc.h
    if (n == "ipm") {
      const IpmConfig& p = r.ipm;
      return list({p.dt, (double)p.ipm_iteration, p.delta_tol, p.g_max, p.g_min, (double)p.compute_lagrange_multipliers, (double)p.use_feedback_policy,
                   p.initial_barrier_parameter, p.target_barrier_parameter, p.barrier_linear_decrease_factor, p.barrier_superlinear_decrease_power,
                   p.barrier_reduction_cost_tol, p.barrier_reduction_constraint_tol, p.fraction_to_boundary_margin, (double)p.use_primal_step_size_for_dual,
                   p.initial_slack_lower_bound, p.initial_dual_lower_bound, p.initial_slack_margin_rate, p.initial_dual_margin_rate,
                   (double)p.n_threads, (double)p.thread_priority});
    }
    if (n == "ddp") {
      const DdpConfig& d = r.ddp;
      return list({(double)d.algorithm, (double)d.max_num_iterations, d.min_rel_cost, d.constraint_tolerance, d.abs_tol_ode, d.rel_tol_ode, d.time_step,
                   (double)d.max_num_steps_per_second, (double)d.backward_pass_integrator, d.constraint_penalty_initial_value, d.constraint_penalty_increase_rate,
                   (double)d.pre_compute_riccati_terms, (double)d.use_feedback_policy, (double)d.strategy, d.ls_min_step_length, d.ls_max_step_length,
                   (double)d.ls_hessian_correction_strategy, d.ls_hessian_correction_multiple, (double)d.n_threads, (double)d.thread_priority});
    }
    throw std::invalid_argument("bpmpc_model_get: unknown name " + n);
  });
}

int bpmpc_model_compose_weights(const bpmpc_model* m, const double* Q_task, const double* R_task, double* row_out) {
  if (!m || !Q_task || !R_task || !row_out) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_model_compose_weights: null argument");
  return guarded(BPMPC_ERR_IO, [&] {
    const RobotModel& r = m->rm;
    const std::vector<double> R = compose_input_weight(r, R_task);      // what load_robot_model runs on the R of task.info
    std::fill(row_out, row_out + BPMPC_SOLVER_WEIGHT_STRIDE, 0.0);
    std::copy(Q_task, Q_task + r.nx * r.nx, row_out);
    std::copy(R.begin(), R.end(), row_out + r.nx * r.nx);
  });
}

int bpmpc_model_check_cone_params(const bpmpc_model* m, const double* row) {
  if (!m || !row) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_model_check_cone_params: null model handle or row");
  return guarded(BPMPC_ERR_IO, [&] {
    const std::string why = check_cone_row(row, m->rm.hard_friction_cone);
    if (!why.empty()) throw std::invalid_argument("bpmpc_model_check_cone_params: " + why);
  });
}

int bpmpc_model_joint_name(const bpmpc_model* m, int j, char* out, int capacity) {
  if (!m || !out || j < 0 || j >= m->rm.nj) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_model_joint_name: bad argument");
  const std::string& s = m->rm.joint_names[j];
  if ((int)s.size() + 1 > capacity) return fail(BPMPC_ERR_CAPACITY, "name buffer too small");
  std::memcpy(out, s.c_str(), s.size() + 1);
  return (int)s.size();
}

int bpmpc_estimator_load_params(const char* task_info_path, double* row) {
  if (!row) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_estimator_load_params: null row");
  return load_into_row<kEstParamStride>(row, [&](double* v) {
    const EstSettings s = estimator_load_settings(task_info_path);
    std::copy(&s.foot_radius, &s.foot_radius + kEstParamStride, v);
  });
}

int bpmpc_estimator_check_params(const double* rows, int n_rows) {
  if (!rows) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_estimator_check_params: null rows");
  return check_n_rows(rows, n_rows, kEstParamStride, [](const double* row, int r) { estimator_check_param_row("bpmpc_estimator_check_params", row, r); });
}

int bpmpc_plant_load_params(const char* task_info_path, double* row) {
  if (!row) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_load_params: null row");
  return load_into_row<kPlantParamStride>(row, [&](double* v) {
    const PlantSettings s = plant_load_settings(task_info_path);
    std::copy(&s.kn, &s.kn + kPlantParamStride, v);
  });
}

int bpmpc_plant_load_stiction(const char* task_info_path, double* kt) {
  if (!kt) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_load_stiction: null kt");
  return guarded(BPMPC_ERR_IO, [&] {
    *kt = plant_load_stiction(task_info_path);
    return (int)BPMPC_OK;
  });
}

int bpmpc_plant_check_params(const double* rows, int n_rows) {
  if (!rows) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_check_params: null rows");
  return check_n_rows(rows, n_rows, kPlantParamStride, [](const double* row, int r) { plant_check_param_row("bpmpc_plant_check_params", row, r); });
}

int bpmpc_plant_load_sensor_params(const char* task_info_path, double* row) {
  if (!row) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_load_sensor_params: null row");
  return load_into_row<kSensorParamStride>(row, [&](double* v) { plant_load_sensor_settings(task_info_path, v, nullptr); });      // (the seed is validated with the row)
}

int bpmpc_plant_check_sensor_params(const double* rows, int n_rows) {
  if (!rows) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_check_sensor_params: null rows");
  return check_n_rows(rows, n_rows, kSensorParamStride, [](const double* row, int r) { plant_check_sensor_row("bpmpc_plant_check_sensor_params", row, r); });
}

int bpmpc_plant_sensor_draw(long seed, int robot, long tick, double* z, double* u) {
  if (!z || !u) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_sensor_draw: null z or u");
  if (robot < 0 || tick < -1) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_sensor_draw: robot must not be negative and tick must be -1 (the turn-on draw) or not negative");
  const unsigned long long s = (unsigned long long)seed, t = tick < 0 ? kSensorTurnOnTick : (unsigned long long)tick;
  const unsigned k0 = (unsigned)s, k1 = (unsigned)(s >> 32);
  for (int g = 0; g < kSensorGaussians; ++g) z[g] = sensor_gaussian(t, (unsigned)robot, k0, k1, g);
  const Philox4 block = sensor_block(t, (unsigned)robot, kSensorUniformBlock, k0, k1);
  for (int i = 0; i < kSensorUniforms; ++i) u[i] = sensor_uniform(block.w[i]);
  return BPMPC_OK;
}

int bpmpc_plant_load_input_params(const char* task_info_path, double* row) {
  if (!row) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_load_input_params: null row");
  return load_into_row<kInputParamStride>(row, [&](double* v) { plant_load_input_settings(task_info_path, v, nullptr); });      // (the seed is validated with the row)
}

int bpmpc_plant_check_input_params(const double* rows, int n_rows) {
  if (!rows) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_check_input_params: null rows");
  return check_n_rows(rows, n_rows, kInputParamStride, [](const double* row, int r) { plant_check_input_row("bpmpc_plant_check_input_params", row, r); });
}

int bpmpc_plant_input_draw(long seed, int robot, long counter, double u[3]) {
  if (!u) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_input_draw: null u");
  if (robot < 0 || counter < 0) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_input_draw: robot and counter must not be negative");
  const unsigned long long s = (unsigned long long)seed;
  const unsigned k0 = (unsigned)s, k1 = (unsigned)(s >> 32);
  u[0] = input_loss_draw((unsigned long long)counter, (unsigned)robot, k0, k1);
  input_push_draw((unsigned long long)counter, (unsigned)robot, k0, k1, u + 1, u + 2);
  return BPMPC_OK;
}

int bpmpc_plant_load_joint_params(const bpmpc_model* model, const char* task_info_path, double* row) {
  if (!model || !row) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_load_joint_params: null model or row");
  return load_into_row<kPlantJointParamStride>(row, [&](double* v) { plant_load_joint_settings(model->rm, task_info_path, v); });
}

int bpmpc_plant_check_joint_params(const double* rows, int n_rows, int nj) {
  if (!rows) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_check_joint_params: null rows");
  if (nj < 1 || nj > kMaxJoints) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_check_joint_params: nj must be 1.." + std::to_string(kMaxJoints));
  return check_n_rows(rows, n_rows, kPlantJointParamStride, [&](const double* row, int r) { plant_check_joint_row("bpmpc_plant_check_joint_params", row, r, nj); });
}

int bpmpc_plant_load_body_params(const bpmpc_model* model, const char* task_info_path, double* row) {
  if (!model || !row) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_load_body_params: null model or row");
  return load_into_row<kPlantBodyParamStride>(row, [&](double* v) { plant_load_body_settings(model->rm, task_info_path, v); });
}

int bpmpc_plant_check_body_params(const double* rows, int n_rows, int nj) {
  if (!rows) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_check_body_params: null rows");
  if (nj < 1 || nj > kMaxJoints) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_check_body_params: nj must be 1.." + std::to_string(kMaxJoints));
  return check_n_rows(rows, n_rows, kPlantBodyParamStride, [&](const double* row, int r) { plant_check_body_row("bpmpc_plant_check_body_params", row, r, nj); });
}

int bpmpc_plant_compose_body_row(const bpmpc_model* model, const double* row_in, int body, double mass_scale, const double* com_shift, double payload_mass,
                                 const double* payload_pos, double* row_out) {
  if (!model || !row_out) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_plant_compose_body_row: null model or row_out");
  return guarded(BPMPC_ERR_IO, [&] {
    double start[kPlantBodyParamStride];
    if (!row_in) plant_body_model_row(model->rm, start);
    plant_compose_body_row("bpmpc_plant_compose_body_row", row_in ? row_in : start, model->rm.nj, body, mass_scale, com_shift, payload_mass, payload_pos, row_out);
    return (int)BPMPC_OK;
  });
}

int bpmpc_gait_create(const bpmpc_model* m, bpmpc_gait** out) {
  if (!m || !out) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_gait_create: null argument");
  return guarded(BPMPC_ERR_IO, [&] {
    auto g = std::make_unique<bpmpc_gait>();
    g->schedule = std::make_unique<GaitSchedule>(m->rm.initial_mode_schedule, m->rm.default_template, m->rm.phase_transition_stance_time);
    *out = g.release();
    return (int)BPMPC_OK;
  });
}
void bpmpc_gait_destroy(bpmpc_gait* g) { delete g; }

int bpmpc_gait_load_template(const char* path, const char* name, double* switching_times, int* modes, int capacity, int* n_modes) {
  if (!path || !name || !switching_times || !modes || !n_modes) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_gait_load_template: null argument");
  return guarded(BPMPC_ERR_IO, [&] {
    const ModeTemplate t = load_mode_template(path, name);
    if (t.switching_times.size() != t.modes.size() + 1) throw std::runtime_error("gait template needs one more switching time than modes");
    if ((int)t.modes.size() + 1 > capacity) throw std::length_error("gait template capacity too small");
    std::copy(t.switching_times.begin(), t.switching_times.end(), switching_times);
    std::copy(t.modes.begin(), t.modes.end(), modes);
    *n_modes = (int)t.modes.size();
    return (int)BPMPC_OK;
  });
}

int bpmpc_gait_insert_template(bpmpc_gait* g, const double* switching_times, const int* modes, int n_modes, double start_time, double final_time) {
  if (!g || !switching_times || !modes || n_modes < 0) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_gait_insert_template: bad argument");
  return guarded(BPMPC_ERR_IO, [&] {
    ModeTemplate t;
    t.switching_times.assign(switching_times, switching_times + n_modes + 1);
    t.modes.assign(modes, modes + n_modes);
    g->schedule->insert_template(t, start_time, final_time);
    return (int)BPMPC_OK;
  });
}

int bpmpc_gait_mode_schedule(bpmpc_gait* g, double lower, double upper, double* event_times, int* modes, int capacity, int* n_events) {
  if (!g || !event_times || !modes || !n_events) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_gait_mode_schedule: null argument");
  return guarded(BPMPC_ERR_IO, [&] {
    const ModeSchedule& s = g->schedule->mode_schedule(lower, upper);
    if ((int)s.modes.size() > capacity) throw std::length_error("mode schedule capacity too small");
    std::copy(s.event_times.begin(), s.event_times.end(), event_times);
    std::copy(s.modes.begin(), s.modes.end(), modes);
    *n_events = (int)s.event_times.size();
    return (int)BPMPC_OK;
  });
}

int bpmpc_swing_reference(const bpmpc_model* m, const double* event_times, const int* modes, int n_events, const double* t, int n_t, double* z,
                          double* zdot) {
  if (!m || !modes || !t || !z || !zdot || n_events < 0 || (n_events > 0 && !event_times)) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_swing_reference: bad argument");
  return guarded(BPMPC_ERR_IO, [&] {
    ModeSchedule s;
    s.event_times.assign(event_times, event_times + n_events);
    s.modes.assign(modes, modes + n_events + 1);
    SwingPlanner planner(m->rm.swing);
    planner.update(s);
    for (int i = 0; i < n_t; ++i)
      for (int c = 0; c < kNumContacts; ++c) {
        z[4 * i + c] = planner.z_position(c, t[i]);
        zdot[4 * i + c] = planner.z_velocity(c, t[i]);
      }
    return (int)BPMPC_OK;
  });
}

int bpmpc_time_grid(double t0, double tf, double dt, const double* event_times, int n_events, double* node_times, int* node_events, int capacity,
                    int* n_nodes) {
  if (!node_times || !node_events || !n_nodes || n_events < 0 || (n_events > 0 && !event_times)) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_time_grid: bad argument");
  return guarded(BPMPC_ERR_IO, [&] {
    const std::vector<double> ev(event_times, event_times + n_events);
    const std::vector<GridNode> grid = shooting_grid(t0, tf, dt, ev);
    if ((int)grid.size() > capacity) throw std::length_error("time grid capacity too small");
    for (size_t i = 0; i < grid.size(); ++i) { node_times[i] = grid[i].time; node_events[i] = grid[i].event; }
    *n_nodes = (int)grid.size();
    return (int)BPMPC_OK;
  });
}

int bpmpc_cmd_vel_to_targets(const bpmpc_model* m, const double cmd_vel[4], double t_now, const double* x_now, double time_to_target, double* times,
                             double* states) {
  if (!m || !cmd_vel || !x_now || !times || !states) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_cmd_vel_to_targets: null argument");
  return guarded(BPMPC_ERR_IO, [&] { cmd_vel_to_targets(m->rm, cmd_vel, t_now, x_now, time_to_target, times, states); return (int)BPMPC_OK; });
}
int bpmpc_goal_to_targets(const bpmpc_model* m, const double goal[4], double t_now, const double* x_now, double* times, double* states) {
  if (!m || !goal || !x_now || !times || !states) return fail(BPMPC_ERR_INVALID_ARGUMENT, "bpmpc_goal_to_targets: null argument");
  return guarded(BPMPC_ERR_IO, [&] { goal_to_targets(m->rm, goal, t_now, x_now, times, states); return (int)BPMPC_OK; });
}

}  // extern "C"
