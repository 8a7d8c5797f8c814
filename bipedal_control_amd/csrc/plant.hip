// Host side of the batched rigid-body plant (kernels/plant.h): settings ingest, device buffers, the C ABI (include/bpmpc.h "Plant").  The plant
// stands where the reference has MuJoCo or Gazebo (bipedal_mujoco, bipedal_gazebo/src/BipedalHWSim.cpp) and imitates neither: the model is the one
// specified in include/bpmpc.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "estimator.h"
#include "info_tree.h"
#include "kernel_launchers.h"
#include "plant.h"
#include "supervisor.h"

namespace bpmpc {

template <int NJ>
__global__ __launch_bounds__(kWave) void k_plant_step(const DeviceModel* model, PlantArgs a) {
  __shared__ PlantLds<NJ> w;
  const int b = blockIdx.x;
  if (b >= a.batch) return;
  plant_robot<NJ, false>(*model, w, a, PlantStickArgs{}, b, threadIdx.x);
}

// bpmpc_plant_set_stiction for the robots of `mask` (NULL: every robot below `batch`): kt[b] = src[b] (n_rows == batch) or src[0]; a robot whose
// kt changes loses its anchors.  One thread per robot.
__global__ __launch_bounds__(256) void k_plant_set_stiction(int batch, const int* mask, const double* src, int n_rows, double* kt, double* anchor, int* anchored) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch || (mask && !mask[b])) return;
  const double val = src[n_rows == 1 ? 0 : b];
  if (val == kt[b]) return;
  kt[b] = val;
  for (int i = 0; i < kNumContacts; ++i) { anchored[b * kNumContacts + i] = 0; anchor[(b * kNumContacts + i) * 2] = 0.0; anchor[(b * kNumContacts + i) * 2 + 1] = 0.0; }
}

// bpmpc_plant_set_state for the robots of `mask` (NULL: every robot below `batch`): q, v from rbd_in[b] (the Euler rates from the world angular
// velocity as WbcBase::updateMeasured forms them) and the robot's row of the rbd output; the robot's anchors are cleared.  One thread per entry of
// [q | v].
__global__ __launch_bounds__(256) void k_plant_set_state(int batch, int nv, const int* mask, const double* rbd_in, double* state, double* rbd_out, double* anchor,
                                                         int* anchored) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= batch * 2 * nv) return;
  const int b = i / (2 * nv), e = i % (2 * nv);
  if (mask && !mask[b]) return;
  if (e < kNumContacts) { anchored[b * kNumContacts + e] = 0; anchor[(b * kNumContacts + e) * 2] = 0.0; anchor[(b * kNumContacts + e) * 2 + 1] = 0.0; }
  const double* rb = rbd_in + (size_t)b * 2 * nv;
  rbd_out[i] = rb[e];
  double val;
  if (e < 3) val = rb[3 + e];
  else if (e < 6) val = rb[e - 3];
  else if (e < nv) val = rb[e];
  else if (e < nv + 3) val = rb[e + 3];
  else if (e < nv + 6) {
    double rates[3];
    const double cy = cos(rb[0]), sy = sin(rb[0]), cp = cos(rb[1]), sp = sin(rb[1]);
    fused::euler_rates_from_world_omega(sy, cy, sp, cp, rb + nv, rates);
    val = e == nv + 3 ? rates[0] : (e == nv + 4 ? rates[1] : rates[2]);
  } else val = rb[e];
  state[i] = val;
}

}  // namespace bpmpc

using namespace bpmpc;

namespace {

// every robot's kt becomes the handle's start value and every anchor is cleared
void write_default_stiction(bpmpc_plant* p) {
  const size_t B = p->max_batch;
  std::vector<double> kt(B, p->kt_start);
  HIP_CHECK(hipMemcpyAsync(p->d_kt, kt.data(), B * sizeof(double), hipMemcpyHostToDevice, p->hs.stream));
  HIP_CHECK(hipMemsetAsync(p->d_anchor, 0, B * kNumContacts * 2 * sizeof(double), p->hs.stream));
  HIP_CHECK(hipMemsetAsync(p->d_anchored, 0, B * kNumContacts * sizeof(int), p->hs.stream));
  HIP_CHECK(hipStreamSynchronize(p->hs.stream));      // kt lives on this frame
  p->stick = p->kt_start > 0.0;
}

// every joint row becomes the start row, and the start row decides which kernel steps launch
void write_start_joint_params(bpmpc_plant* p) {
  p->joints.fill_from_start(p->hs.stream, p->max_batch);
  p->joint = !plant_joint_row_neutral(p->joint_start, p->nj);
}

// every body row becomes the start row, and the start row decides which kernel steps launch
void write_start_body_params(bpmpc_plant* p) {
  p->bodies.fill_from_start(p->hs.stream, p->max_batch);
  double model_row[kPlantBodyParamStride];
  plant_body_model_row(p->rm, model_row);
  p->body = !plant_body_rows_equal(p->body_start, model_row, p->nj);
}

void check_batch(const bpmpc_plant* p, int batch, const char* who) {
  if (batch < 1) throw std::invalid_argument(std::string(who) + ": batch must be positive");
  if (batch > p->max_batch) throw std::length_error(std::string(who) + ": batch exceeds max_batch");
}

// the refusals of a step behind its null checks
void check_step(const bpmpc_plant* p, int batch, double period, int substeps, const char* who) {
  if (substeps < 1) throw std::invalid_argument(std::string(who) + ": substeps must be at least 1");
  if (!std::isfinite(period) || period <= 0.0) throw std::invalid_argument(std::string(who) + ": period must be finite and positive");
  check_batch(p, batch, who);
  if (batch != p->last_batch)
    throw std::invalid_argument(std::string(who) + ": batch " + std::to_string(batch) + " differs from the batch of the last set_state (" + std::to_string(p->last_batch) +
                                "): the other robots have no state");
}

// what every step passes its kernel, the command apart: base_force and feet_heights (nullable) are staged as the step's other host inputs are
PlantArgs step_args(const bpmpc_plant* p, int batch, double period, int substeps, const double* base_force, const double* feet_heights, bool on_device) {
  PlantArgs a{};
  a.batch = batch; a.substeps = substeps; a.h = period / substeps; a.params = p->params.d_params; a.state = p->d_state;
  for (int i = 0; i < kMaxJoints / 2; ++i) a.torque_limits[i] = p->torque_limits[i];
  a.out = p->d_out; a.max_batch = p->max_batch;
  a.base_force = staged(base_force, p->d_force, (size_t)batch * 3, on_device, p->hs.stream);
  a.ground = staged(feet_heights, p->d_ground, (size_t)batch * 4, on_device, p->hs.stream);
  return a;
}

// On a handle whose input model is switched: k_plant_input in front of the step kernel, which then consumes the applied rows and force
void launch_input(bpmpc_plant* p, PlantArgs& a, double period) {
  p->last_ground = a.ground;
  if (!p->input) return;
  const size_t rows = (size_t)p->max_batch * p->nj;
  const PlantInputArgs ia{a.batch, p->max_batch, input_period_ns(period), p->inputs.d_params, p->d_ikey, p->d_iticks, p->d_iring, a.pos_des, a.vel_des, a.tau_ff, a.kp, a.kd,
                          a.cmd_stride, a.base_force, p->d_applied, p->d_applied_force, p->d_iflags};
  launch_plant_input(p->nj, p->hs.stream, ia);
  a.cmd_stride = p->nj;
  a.pos_des = p->d_applied; a.vel_des = p->d_applied + rows; a.tau_ff = p->d_applied + 2 * rows; a.kp = p->d_applied + 3 * rows; a.kd = p->d_applied + 4 * rows;
  a.base_force = p->d_applied_force;
  p->applied_valid = true;
}

// the step kernel, on a switched handle the input model in front of it and the sensor model behind it: `period` is the control step's
void launch_step(bpmpc_plant* p, PlantArgs a, double period) {
  launch_input(p, a, period);
  const PlantStickArgs sa{p->d_kt, p->d_anchor, p->d_anchored};
  const PlantJointArgs ja{p->joints.d_params};
  if (p->body) launch_plant_body_step(p->nj, p->hs.stream, p->d_model, a, sa, ja, PlantBodyArgs{p->bodies.d_params});      // body rows, the joint model and stick-slip contacts
  else if (p->joint) launch_plant_joint_step(p->nj, p->hs.stream, p->d_model, a, sa, ja);      // the joint model and stick-slip contacts
  else if (p->stick) launch_plant_stick_step(p->nj, p->hs.stream, p->d_model, a, sa);
  else KL_NJ(p->nj, hipLaunchKernelGGL(k_plant_step<NJ>, dim3(a.batch), dim3(kWave), 0, p->hs.stream, p->d_model, a));
  HIP_CHECK(hipGetLastError());
  if (p->sense) {
    const PlantSenseArgs se{a.batch, p->max_batch, std::sqrt(period), p->sensors.d_params, p->d_skey, p->d_sticks, p->d_sbias, p->d_sring, p->d_out, p->d_sensed};
    launch_plant_sense(p->nj, p->hs.stream, se);
    p->sensed_valid = true;
  }
}

// the handle leaves the untouched state: from now on every step measures, and the sensed block holds nothing until one has
void switch_sensors(bpmpc_plant* p) {
  if (!p->sense) p->sensed_valid = false;
  p->sense = true;
}

// every sensor row zero, every bias and counter zero, every key the start key: the handle is untouched
void write_untouched_sensors(bpmpc_plant* p) {
  const size_t B = p->max_batch;
  hipStream_t st = p->hs.stream;
  HIP_CHECK(hipMemsetAsync(p->sensors.d_params, 0, B * kSensorParamStride * sizeof(double), st));
  launch_plant_seed_sensors(st, p->max_batch, nullptr, p->sensor_seed, p->sensors.d_params, p->d_skey, p->d_sticks, p->d_sbias);      // keys and counters
  HIP_CHECK(hipMemsetAsync(p->d_sbias, 0, B * 6 * sizeof(double), st));
  HIP_CHECK(hipStreamSynchronize(st));
  p->sense = false; p->sensed_valid = false;
}

// the handle leaves the untouched state: from now on every step runs the input model, and the applied block holds nothing until one has
void switch_inputs(bpmpc_plant* p) {
  if (!p->input) p->applied_valid = false;
  p->input = true;
}

// every input row zero, every counter zero, every key the start key: the handle is untouched
void write_untouched_inputs(bpmpc_plant* p) {
  const size_t B = p->max_batch;
  hipStream_t st = p->hs.stream;
  HIP_CHECK(hipMemsetAsync(p->inputs.d_params, 0, B * kInputParamStride * sizeof(double), st));
  HIP_CHECK(hipMemsetAsync(p->d_iflags, 0, B * 3 * sizeof(int), st));
  launch_plant_seed_inputs(st, p->max_batch, nullptr, p->input_seed, p->d_ikey, p->d_iticks);
  HIP_CHECK(hipStreamSynchronize(st));
  p->input = false; p->applied_valid = false;
}

// The pieces of bpmpc_plant_create, in its order.  Each allocates its zero-filled buffers before its table: the fills run on the null stream, and
// the upload of a start row (ParamTable::create) waits for them before anything is enqueued on the handle's stream.

// the state, the mask and the device copies of host inputs
void create_state_and_staging(bpmpc_plant* p) {
  const size_t B = p->max_batch, nj = p->nj, nv = p->nv;
  DeviceBuffers& m = p->mem;
  p->d_state = m.alloc<double>(B * 2 * nv, true);
  p->d_mask = m.alloc<int>(B);
  p->d_rbd_in = m.alloc<double>(B * 2 * nv);
  p->d_pd = m.alloc<double>(B * nj); p->d_vd = m.alloc<double>(B * nj); p->d_tf = m.alloc<double>(B * nj); p->d_kp = m.alloc<double>(B * nj); p->d_kd = m.alloc<double>(B * nj);
  p->d_force = m.alloc<double>(B * 3); p->d_ground = m.alloc<double>(B * 4);
}

// the output block and its section pointers
void create_outputs(bpmpc_plant* p) {
  const size_t B = p->max_batch;
  p->d_out = p->mem.alloc<double>(B * plant_out_offset(kPlantOutEnd, p->nj), true);
  auto section = [&](int sec) { return p->d_out + B * plant_out_offset(sec, p->nj); };
  bpmpc_sensor_inputs& s = p->out.sensors;
  s.joint_pos = section(kPlantJointPos); s.joint_vel = section(kPlantJointVel); s.quat = section(kPlantQuat);
  s.angular_vel_local = section(kPlantAngLocal); s.linear_accel_local = section(kPlantAccLocal);
  s.contact = reinterpret_cast<int*>(section(kPlantContact)); s.mode = nullptr;
  s.feet_heights = section(kPlantFeetHeights); s.odom_pos = section(kPlantOdomPos); s.odom_quat = section(kPlantOdomQuat);
  s.odom_lin_vel = section(kPlantOdomLin); s.odom_ang_vel = section(kPlantOdomAng);
  p->out.rbd = section(kPlantRbd); p->out.contact_force = section(kPlantContactForce);
}

// contact parameters and stick-slip contacts: `defaults` and kt_start are loaded
void create_contacts(bpmpc_plant* p) {
  const size_t B = p->max_batch;
  DeviceBuffers& m = p->mem;
  p->d_kt = m.alloc<double>(B); p->d_kt_in = m.alloc<double>(B);
  p->d_anchor = m.alloc<double>(B * kNumContacts * 2); p->d_anchored = m.alloc<int>(B * kNumContacts);
  p->params.create(m, p->max_batch, kPlantParamStride, kPlantParamStride - 2, &p->defaults.kn);
  p->params.fill_from_start(p->hs.stream, p->max_batch);
  write_default_stiction(p);
}

void create_joints(bpmpc_plant* p, const char* task_info_path) {
  plant_load_joint_settings(p->rm, task_info_path, p->joint_start);
  p->joints.create(p->mem, p->max_batch, kPlantJointParamStride, kJointParamUsed, p->joint_start);
  write_start_joint_params(p);
}

void create_bodies(bpmpc_plant* p, const char* task_info_path) {
  plant_load_body_settings(p->rm, task_info_path, p->body_start);
  p->bodies.create(p->mem, p->max_batch, kPlantBodyParamStride, kPlantBodyParamStride, p->body_start);
  write_start_body_params(p);
}

// A task file with settings for the sensor or the input model (a non-zero used entry of the start row): its row for every robot; true: the handle
// is to be switched
bool fill_if_configured(bpmpc_plant* p, ParamTable& table, const double* start_row) {
  if (std::all_of(start_row, start_row + table.used, [](double v) { return v == 0.0; })) return false;
  table.fill_from_start(p->hs.stream, p->max_batch);
  return true;
}

// sensor model: the members it measures live in the sensed block, the others are the truth's
void create_sensors(bpmpc_plant* p, const char* task_info_path) {
  plant_load_sensor_settings(task_info_path, p->sensor_start, &p->sensor_seed);
  const size_t B = p->max_batch;
  DeviceBuffers& m = p->mem;
  p->d_skey = m.alloc<unsigned>(B * 2); p->d_sticks = m.alloc<unsigned long long>(B * 2); p->d_sbias = m.alloc<double>(B * 6);
  p->d_sring = m.alloc<double>(B * kSensorRing * sensor_sample_width(p->nj), true);
  p->d_sensed = m.alloc<double>(B * sensor_sensed_offset(kSensedEnd, p->nj), true);
  auto measured = [&](int sec) { return p->d_sensed + B * sensor_sensed_offset(sec, p->nj); };
  p->sensed = p->out.sensors;
  p->sensed.joint_pos = measured(kSensedJointPos); p->sensed.joint_vel = measured(kSensedJointVel); p->sensed.quat = measured(kSensedQuat);
  p->sensed.angular_vel_local = measured(kSensedAngLocal); p->sensed.linear_accel_local = measured(kSensedAccLocal);
  p->sensed.contact = reinterpret_cast<int*>(measured(kSensedContact));
  p->sensors.create(m, p->max_batch, kSensorParamStride, kSensorParamUsed, p->sensor_start);
  write_untouched_sensors(p);
  if (fill_if_configured(p, p->sensors, p->sensor_start)) {      // turned on under the start key
    launch_plant_seed_sensors(p->hs.stream, p->max_batch, nullptr, p->sensor_seed, p->sensors.d_params, p->d_skey, p->d_sticks, p->d_sbias);
    switch_sensors(p);
  }
}

// input model: the step kernels consume the applied block on a switched handle, the caller's pointers otherwise
void create_inputs(bpmpc_plant* p, const char* task_info_path) {
  plant_load_input_settings(task_info_path, p->input_start, &p->input_seed);
  const size_t B = p->max_batch, nj = p->nj;
  DeviceBuffers& m = p->mem;
  p->d_ikey = m.alloc<unsigned>(B * 2); p->d_iticks = m.alloc<unsigned long long>(B * 2);
  p->d_iring = m.alloc<double>(B * kInputRing * kInputRows * nj, true);
  p->d_applied = m.alloc<double>(kInputRows * B * nj, true); p->d_applied_force = m.alloc<double>(B * 3, true); p->d_iflags = m.alloc<int>(B * 3, true);
  p->inputs.create(m, p->max_batch, kInputParamStride, kInputParamUsed, p->input_start);
  write_untouched_inputs(p);
  if (fill_if_configured(p, p->inputs, p->input_start)) switch_inputs(p);      // under the start key, which write_untouched_inputs has set
}

}  // namespace

extern "C" {

int bpmpc_plant_create(const bpmpc_model* model, const char* task_info_path, int device, int max_batch, bpmpc_plant** out) {
  if (!model || !out) { set_last_error("bpmpc_plant_create: null model or output"); return BPMPC_ERR_INVALID_ARGUMENT; }
  *out = nullptr;
  if (max_batch < 1) { set_last_error("bpmpc_plant_create: max_batch must be positive"); return BPMPC_ERR_INVALID_ARGUMENT; }
  std::unique_ptr<bpmpc_plant> p(new bpmpc_plant);
  const int rc = guarded(BPMPC_ERR_IO, [&]() -> int {
    if (const int refused = open_side_handle("bpmpc_plant_create", p.get(), model, device, max_batch)) return refused;
    p->defaults = plant_load_settings(task_info_path);
    p->kt_start = plant_load_stiction(task_info_path);
    p->nj = p->rm.nj; p->nv = 6 + p->rm.nj;
    if (task_info_path) {
      const auto t = read_info_file(task_info_path);
      const std::vector<double> lim = load_matrix(*t, "torqueLimitsTask", p->nj / 2, 1);
      for (int i = 0; i < p->nj / 2; ++i) p->torque_limits[i] = lim[i];
    }
    create_state_and_staging(p.get());
    create_outputs(p.get());
    create_contacts(p.get());
    create_joints(p.get(), task_info_path);
    create_bodies(p.get(), task_info_path);
    create_sensors(p.get(), task_info_path);
    create_inputs(p.get(), task_info_path);
    HIP_CHECK(hipStreamSynchronize(p->hs.stream));
    return BPMPC_OK;
  });
  if (rc != BPMPC_OK) { bpmpc_plant_destroy(p.release()); return rc; }
  *out = p.release();
  return BPMPC_OK;
}

void bpmpc_plant_destroy(bpmpc_plant* p) {
  if (!p) return;
  if (p->hs.stream) { (void)hipSetDevice(p->device); (void)hipStreamSynchronize(p->hs.stream); }
  if (p->ev_tick) (void)hipEventDestroy(p->ev_tick);
  if (p->ev_step) (void)hipEventDestroy(p->ev_step);
  close_side_handle(p);
}

int bpmpc_plant_set_state(bpmpc_plant* p, int batch, const int* mask, const double* rbd, int inputs_on_device) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_set_state: null handle or rbd", rbd != nullptr, [&] {
    check_batch(p, batch, "bpmpc_plant_set_state");
    const size_t B = batch, E = 2 * p->nv;
    if (!inputs_on_device)
      for (size_t i = 0; i < B * E; ++i)
        if (!mask || mask[i / E]) if (!std::isfinite(rbd[i])) throw std::invalid_argument("bpmpc_plant_set_state: rbd of robot " + std::to_string(i / E) + " is not finite");
    hipStream_t st = p->hs.stream;
    const int* dmask = staged(mask, p->d_mask, B, inputs_on_device, st);
    const double* drbd = staged(rbd, p->d_rbd_in, B * E, inputs_on_device, st);
    hipLaunchKernelGGL(k_plant_set_state, dim3((batch * (int)E + 255) / 256), dim3(256), 0, st, batch, p->nv, dmask, drbd, p->d_state, p->out.rbd,
                       p->d_anchor, p->d_anchored);
    HIP_CHECK(hipGetLastError());
    if (p->sense) launch_plant_forget_samples(st, batch, dmask, p->d_sticks);      // n = 0: the robots' sample history is forgotten
    if (p->input) launch_plant_forget_commands(st, batch, dmask, p->d_iticks);     // n = 0: the robots' buffered commands are forgotten
    p->last_batch = batch;
    p->hs.finish(inputs_on_device);
  });
}

int bpmpc_plant_get_state(bpmpc_plant* p, int batch, double* host_rbd) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_get_state: null handle or rbd", host_rbd != nullptr, [&] {
    check_batch(p, batch, "bpmpc_plant_get_state");
    HIP_CHECK(hipMemcpyAsync(host_rbd, p->out.rbd, (size_t)batch * 2 * p->nv * sizeof(double), hipMemcpyDeviceToHost, p->hs.stream));
    p->hs.synchronise_own();
  });
}

int bpmpc_plant_step(bpmpc_plant* p, int batch, const bpmpc_joint_command* c, int inputs_on_device, double period, int substeps) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_step: null handle or command", c && c->pos_des && c->vel_des && c->tau_ff && c->kp && c->kd, [&] {
    check_step(p, batch, period, substeps, "bpmpc_plant_step");
    PlantArgs a = step_args(p, batch, period, substeps, c->base_force, c->feet_heights, inputs_on_device);
    auto input = [&](const double* src, double* staging) { return staged(src, staging, (size_t)batch * p->nj, inputs_on_device, p->hs.stream); };
    a.cmd_stride = p->nj;
    a.pos_des = input(c->pos_des, p->d_pd); a.vel_des = input(c->vel_des, p->d_vd); a.tau_ff = input(c->tau_ff, p->d_tf);
    a.kp = input(c->kp, p->d_kp); a.kd = input(c->kd, p->d_kd);
    launch_step(p, a, period);
    p->hs.finish(inputs_on_device);
  });
}

int bpmpc_plant_device_outputs(bpmpc_plant* p, bpmpc_plant_outputs* o) {
  if (!p || !o) { set_last_error("bpmpc_plant_device_outputs: null argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  *o = p->out;
  return BPMPC_OK;
}

// One step on the commands of the controller's last tick, read where the tick wrote them: the plant's stream waits for the tick on the solver's
// stream, and the solver's stream waits for the step before the next tick overwrites joint_cmd
int bpmpc_plant_step_controlled(bpmpc_plant* p, bpmpc_controller* controller, int batch, double period, int substeps, const double* base_force,
                                const double* feet_heights, int inputs_on_device) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_step_controlled: null plant or controller", controller != nullptr, [&] {
    const ControllerCommands cc = controller_commands(controller);
    if (cc.nj != p->nj) throw std::invalid_argument("bpmpc_plant_step_controlled: the plant and the controller are built for different robots");
    if (cc.device != p->device) throw std::invalid_argument("bpmpc_plant_step_controlled: the plant and the controller live on different devices");
    check_step(p, batch, period, substeps, "bpmpc_plant_step_controlled");
    if (cc.last_tick_batch == 0) throw std::invalid_argument("bpmpc_plant_step_controlled: the controller has not ticked yet: there are no joint commands");
    if (batch != cc.last_tick_batch)
      throw std::invalid_argument("bpmpc_plant_step_controlled: batch " + std::to_string(batch) + " differs from the batch of the controller's last tick (" +
                                  std::to_string(cc.last_tick_batch) + ")");
    hipStream_t st = p->hs.stream;
    PlantArgs a = step_args(p, batch, period, substeps, base_force, feet_heights, inputs_on_device);
    a.cmd_stride = 3 * p->nj;
    a.pos_des = cc.joint_cmd; a.vel_des = cc.joint_cmd + p->nj; a.tau_ff = cc.joint_cmd + 2 * p->nj;
    a.kp = cc.kp; a.kd = cc.kd;
    StreamHandshake::record(&p->ev_tick, cc.stream);
    HIP_CHECK(hipStreamWaitEvent(st, p->ev_tick, 0));
    launch_step(p, a, period);
    StreamHandshake::record(&p->ev_step, st);
    HIP_CHECK(hipStreamWaitEvent(cc.stream, p->ev_step, 0));
    p->hs.finish(inputs_on_device || !(base_force || feet_heights));      // waited for only when a host array of the caller's was staged
  });
}

// One step on the commands of a supervisor's last update, read where the update wrote them (stride nj): bpmpc_plant_step_controlled with the
// supervisor's five arrays and its stream in the two waits.  The plant's stream waits for an update that was only enqueued, and the supervisor's
// stream for the step before the next update overwrites the commands; the step kernels are those of every other step
int bpmpc_plant_step_supervised(bpmpc_plant* p, bpmpc_supervisor* sup, int batch, double period, int substeps, const double* base_force,
                                const double* feet_heights, int inputs_on_device) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_step_supervised: null plant or supervisor", sup != nullptr, [&] {
    if (sup->nj != p->nj) throw std::invalid_argument("bpmpc_plant_step_supervised: the plant and the supervisor are built for different robots");
    if (sup->device != p->device) throw std::invalid_argument("bpmpc_plant_step_supervised: the plant and the supervisor live on different devices");
    check_step(p, batch, period, substeps, "bpmpc_plant_step_supervised");
    if (batch > sup->max_batch) throw std::length_error("bpmpc_plant_step_supervised: batch exceeds the supervisor's max_batch");
    hipStream_t st = p->hs.stream;
    PlantArgs a = step_args(p, batch, period, substeps, base_force, feet_heights, inputs_on_device);
    a.cmd_stride = p->nj;
    a.pos_des = sup->d_cmd[0]; a.vel_des = sup->d_cmd[1]; a.tau_ff = sup->d_cmd[2]; a.kp = sup->d_cmd[3]; a.kd = sup->d_cmd[4];
    sup->hs.before_foreign(st);
    launch_step(p, a, period);
    sup->hs.after_foreign(st);
    p->hs.finish(inputs_on_device || !(base_force || feet_heights));      // waited for only when a host array of the caller's was staged
  });
}

// bpmpc_estimator_update on the plant's device outputs: the estimator's stream waits for a step that was only enqueued, and the plant's stream for
// this update before its next step overwrites the outputs
int bpmpc_estimator_update_from_plant(bpmpc_estimator* e, bpmpc_plant* p, int batch, double period, double* host_rbd) {
  if (!e) { set_last_error("bpmpc_estimator_update_from_plant: null estimator"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(p, BPMPC_ERR_IO, "bpmpc_estimator_update_from_plant: null plant", [&]() -> int {
    if (e->nj != p->nj) throw std::invalid_argument("bpmpc_estimator_update_from_plant: the estimator and the plant are built for different robots");
    if (e->device != p->device) throw std::invalid_argument("bpmpc_estimator_update_from_plant: the estimator and the plant live on different devices");
    if (batch != p->last_batch) throw std::invalid_argument("bpmpc_estimator_update_from_plant: batch differs from the batch of the plant's last set_state");
    if (p->sense && !p->sensed_valid)
      throw std::invalid_argument("bpmpc_estimator_update_from_plant: the plant's sensor model has been switched on and no step has run since: there is no measurement");
    p->hs.before_foreign(e->hs.stream);
    const int rc = bpmpc_estimator_update(e, batch, p->sense ? &p->sensed : &p->out.sensors, 1, period, host_rbd);
    p->hs.after_foreign(e->hs.stream);
    return rc;
  });
}

int bpmpc_plant_get_params(const bpmpc_plant* p, int robot, double* row) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_get_params: null handle or row", row != nullptr, [&] {
    p->params.get("bpmpc_plant_get_params", p->hs.stream, p->max_batch, robot, row);
  });
}

int bpmpc_plant_set_params(bpmpc_plant* p, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_set_params: null handle or rows", rows != nullptr, [&] {
    check_batch(p, batch, "bpmpc_plant_set_params");
    p->params.set("bpmpc_plant_set_params", p->hs.stream, batch, mask, p->d_mask, rows, n_rows, inputs_on_device,
                  [](const double* row, int r) { plant_check_param_row("bpmpc_plant_set_params", row, r); });
    p->hs.finish(inputs_on_device);      // device rows are only enqueued on the handle's stream: the next step runs behind them
  });
}

int bpmpc_plant_reset_params(bpmpc_plant* p) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_reset_params: null handle", [&] {
    p->params.fill_from_start(p->hs.stream, p->max_batch);
    p->hs.synchronise_own();
  });
}

int bpmpc_plant_get_joint_params(const bpmpc_plant* p, int robot, double* row) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_get_joint_params: null handle or row", row != nullptr, [&] {
    p->joints.get("bpmpc_plant_get_joint_params", p->hs.stream, p->max_batch, robot, row);
  });
}

int bpmpc_plant_set_joint_params(bpmpc_plant* p, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_set_joint_params: null handle or rows", rows != nullptr, [&] {
    check_batch(p, batch, "bpmpc_plant_set_joint_params");
    p->joints.set("bpmpc_plant_set_joint_params", p->hs.stream, batch, mask, p->d_mask, rows, n_rows, inputs_on_device,
                  [&](const double* row, int r) { plant_check_joint_row("bpmpc_plant_set_joint_params", row, r, p->nj); });
    p->joint = true;      // from here on every robot of the handle steps in k_plant_joint_step
    p->hs.finish(inputs_on_device);      // device rows are only enqueued on the handle's stream: the next step runs behind them
  });
}

int bpmpc_plant_reset_joint_params(bpmpc_plant* p) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_reset_joint_params: null handle", [&] {
    write_start_joint_params(p);
    p->hs.synchronise_own();
  });
}

int bpmpc_plant_get_body_params(const bpmpc_plant* p, int robot, double* row) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_get_body_params: null handle or row", row != nullptr, [&] {
    double got[kPlantBodyParamStride];
    p->bodies.get("bpmpc_plant_get_body_params", p->hs.stream, p->max_batch, robot, got);
    for (int e = 0; e < kPlantBodyParamStride; ++e) row[e] = e % kPlantBodySlots <= p->nj ? got[e] : 0.0;      // slots of bodies the robot does not have
  });
}

int bpmpc_plant_set_body_params(bpmpc_plant* p, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_set_body_params: null handle or rows", rows != nullptr, [&] {
    check_batch(p, batch, "bpmpc_plant_set_body_params");
    p->bodies.set("bpmpc_plant_set_body_params", p->hs.stream, batch, mask, p->d_mask, rows, n_rows, inputs_on_device,
                  [&](const double* row, int r) { plant_check_body_row("bpmpc_plant_set_body_params", row, r, p->nj); });
    p->body = true;      // from here on every robot of the handle steps in k_plant_body_step
    p->hs.finish(inputs_on_device);      // device rows are only enqueued on the handle's stream: the next step runs behind them
  });
}

int bpmpc_plant_reset_body_params(bpmpc_plant* p) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_reset_body_params: null handle", [&] {
    write_start_body_params(p);
    p->hs.synchronise_own();
  });
}

int bpmpc_plant_set_stiction(bpmpc_plant* p, int batch, const int* mask, const double* kt, int n_rows, int inputs_on_device) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_set_stiction: null handle or kt", kt != nullptr, [&] {
    check_batch(p, batch, "bpmpc_plant_set_stiction");
    if (n_rows != 1 && n_rows != batch) throw std::invalid_argument("bpmpc_plant_set_stiction: n_rows must be 1 or batch");
    if (!inputs_on_device)
      for (int r = 0; r < n_rows; ++r)
        if ((n_rows == 1 || !mask || mask[r]) && (!std::isfinite(kt[r]) || kt[r] < 0.0))
          throw std::invalid_argument("bpmpc_plant_set_stiction: entry " + std::to_string(r) + " (kt) is " + (!std::isfinite(kt[r]) ? "not finite" : "negative"));
    hipStream_t st = p->hs.stream;
    const int* dmask = staged(mask, p->d_mask, (size_t)batch, inputs_on_device, st);
    const double* dkt = staged(kt, p->d_kt_in, (size_t)n_rows, inputs_on_device, st);
    hipLaunchKernelGGL(k_plant_set_stiction, dim3((batch + 255) / 256), dim3(256), 0, st, batch, dmask, dkt, n_rows, p->d_kt, p->d_anchor, p->d_anchored);
    HIP_CHECK(hipGetLastError());
    p->stick = true;
    p->hs.finish(inputs_on_device);
  });
}

int bpmpc_plant_get_stiction(const bpmpc_plant* p, int robot, double* kt) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_get_stiction: null handle or kt", kt != nullptr, [&] {
    if (robot >= p->max_batch) throw std::length_error("bpmpc_plant_get_stiction: robot exceeds max_batch");
    if (robot < 0) { *kt = p->kt_start; return; }
    HIP_CHECK(hipMemcpyAsync(kt, p->d_kt + robot, sizeof(double), hipMemcpyDeviceToHost, p->hs.stream));
    HIP_CHECK(hipStreamSynchronize(p->hs.stream));
  });
}

int bpmpc_plant_reset_stiction(bpmpc_plant* p) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_reset_stiction: null handle", [&] { write_default_stiction(p); });
}

int bpmpc_plant_get_anchors(bpmpc_plant* p, int batch, double* host_anchor, int* host_anchored) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_get_anchors: null handle, anchor or anchored", host_anchor && host_anchored, [&] {
    check_batch(p, batch, "bpmpc_plant_get_anchors");
    HIP_CHECK(hipMemcpyAsync(host_anchor, p->d_anchor, (size_t)batch * kNumContacts * 2 * sizeof(double), hipMemcpyDeviceToHost, p->hs.stream));
    HIP_CHECK(hipMemcpyAsync(host_anchored, p->d_anchored, (size_t)batch * kNumContacts * sizeof(int), hipMemcpyDeviceToHost, p->hs.stream));
    p->hs.synchronise_own();
  });
}

int bpmpc_plant_get_sensor_params(const bpmpc_plant* p, int robot, double* row) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_get_sensor_params: null handle or row", row != nullptr, [&] {
    p->sensors.get("bpmpc_plant_get_sensor_params", p->hs.stream, p->max_batch, robot, row);
  });
}

int bpmpc_plant_set_sensor_params(bpmpc_plant* p, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_set_sensor_params: null handle or rows", rows != nullptr, [&] {
    check_batch(p, batch, "bpmpc_plant_set_sensor_params");
    p->sensors.set("bpmpc_plant_set_sensor_params", p->hs.stream, batch, mask, p->d_mask, rows, n_rows, inputs_on_device,
                   [](const double* row, int r) { plant_check_sensor_row("bpmpc_plant_set_sensor_params", row, r); });
    switch_sensors(p);
    p->hs.finish(inputs_on_device);
  });
}

int bpmpc_plant_reset_sensor_params(bpmpc_plant* p) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_reset_sensor_params: null handle", [&] { write_untouched_sensors(p); });
}

int bpmpc_plant_seed_sensors(bpmpc_plant* p, int batch, const int* mask, long seed, int inputs_on_device) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_seed_sensors: null handle", [&] {
    check_batch(p, batch, "bpmpc_plant_seed_sensors");
    hipStream_t st = p->hs.stream;
    const int* dmask = staged(mask, p->d_mask, (size_t)batch, inputs_on_device, st);
    launch_plant_seed_sensors(st, batch, dmask, seed, p->sensors.d_params, p->d_skey, p->d_sticks, p->d_sbias);
    switch_sensors(p);
    p->hs.finish(inputs_on_device);
  });
}

int bpmpc_plant_get_sensor_state(bpmpc_plant* p, int batch, double* gyro_bias, double* accel_bias, double* ticks) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_get_sensor_state: null handle", [&] {
    check_batch(p, batch, "bpmpc_plant_get_sensor_state");
    const size_t B = batch;
    std::vector<double> bias(B * 6);
    std::vector<unsigned long long> counters(B * 2);
    HIP_CHECK(hipMemcpyAsync(bias.data(), p->d_sbias, B * 6 * sizeof(double), hipMemcpyDeviceToHost, p->hs.stream));
    HIP_CHECK(hipMemcpyAsync(counters.data(), p->d_sticks, B * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, p->hs.stream));
    p->hs.synchronise_own();
    for (size_t b = 0; b < B; ++b)
      for (int i = 0; i < 3; ++i) {
        if (gyro_bias) gyro_bias[b * 3 + i] = bias[b * 6 + i];
        if (accel_bias) accel_bias[b * 3 + i] = bias[b * 6 + 3 + i];
      }
    if (ticks) for (size_t i = 0; i < B * 2; ++i) ticks[i] = (double)counters[i];
  });
}

int bpmpc_plant_sensed_outputs(bpmpc_plant* p, bpmpc_sensor_inputs* o) {
  if (!p || !o) { set_last_error("bpmpc_plant_sensed_outputs: null argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  *o = p->sensed;
  return BPMPC_OK;
}

int bpmpc_plant_get_input_params(const bpmpc_plant* p, int robot, double* row) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_get_input_params: null handle or row", row != nullptr, [&] {
    p->inputs.get("bpmpc_plant_get_input_params", p->hs.stream, p->max_batch, robot, row);
  });
}

int bpmpc_plant_set_input_params(bpmpc_plant* p, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_set_input_params: null handle or rows", rows != nullptr, [&] {
    check_batch(p, batch, "bpmpc_plant_set_input_params");
    p->inputs.set("bpmpc_plant_set_input_params", p->hs.stream, batch, mask, p->d_mask, rows, n_rows, inputs_on_device,
                  [](const double* row, int r) { plant_check_input_row("bpmpc_plant_set_input_params", row, r); });
    switch_inputs(p);
    p->hs.finish(inputs_on_device);
  });
}

int bpmpc_plant_reset_input_params(bpmpc_plant* p) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_reset_input_params: null handle", [&] { write_untouched_inputs(p); });
}

int bpmpc_plant_seed_inputs(bpmpc_plant* p, int batch, const int* mask, long seed, int inputs_on_device) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_seed_inputs: null handle", [&] {
    check_batch(p, batch, "bpmpc_plant_seed_inputs");
    hipStream_t st = p->hs.stream;
    const int* dmask = staged(mask, p->d_mask, (size_t)batch, inputs_on_device, st);
    launch_plant_seed_inputs(st, batch, dmask, seed, p->d_ikey, p->d_iticks);
    switch_inputs(p);
    p->hs.finish(inputs_on_device);
  });
}

int bpmpc_plant_get_input_state(bpmpc_plant* p, int batch, double* ticks, int* delay_steps, int* lost, int* pushing) {
  return guarded(p, BPMPC_ERR_IO, "bpmpc_plant_get_input_state: null handle", [&] {
    check_batch(p, batch, "bpmpc_plant_get_input_state");
    const size_t B = batch, MB = p->max_batch;
    std::vector<unsigned long long> counters(B * 2);
    hipStream_t st = p->hs.stream;
    HIP_CHECK(hipMemcpyAsync(counters.data(), p->d_iticks, B * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (delay_steps) HIP_CHECK(hipMemcpyAsync(delay_steps, p->d_iflags, B * sizeof(int), hipMemcpyDeviceToHost, st));
    if (lost) HIP_CHECK(hipMemcpyAsync(lost, p->d_iflags + MB, B * sizeof(int), hipMemcpyDeviceToHost, st));
    if (pushing) HIP_CHECK(hipMemcpyAsync(pushing, p->d_iflags + 2 * MB, B * sizeof(int), hipMemcpyDeviceToHost, st));
    p->hs.synchronise_own();
    if (ticks) for (size_t i = 0; i < B * 2; ++i) ticks[i] = (double)counters[i];
  });
}

int bpmpc_plant_applied_command(bpmpc_plant* p, bpmpc_joint_command* o) {
  if (!p || !o) { set_last_error("bpmpc_plant_applied_command: null argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  if (!p->input) { set_last_error("bpmpc_plant_applied_command: the plant's input model is untouched: the step kernel consumes the caller's command"); return BPMPC_ERR_INVALID_ARGUMENT; }
  if (!p->applied_valid) {
    set_last_error("bpmpc_plant_applied_command: the plant's input model has been switched on and no step has run since: there is no applied command");
    return BPMPC_ERR_INVALID_ARGUMENT;
  }
  const size_t rows = (size_t)p->max_batch * p->nj;
  o->pos_des = p->d_applied; o->vel_des = p->d_applied + rows; o->tau_ff = p->d_applied + 2 * rows; o->kp = p->d_applied + 3 * rows; o->kd = p->d_applied + 4 * rows;
  o->base_force = p->d_applied_force;
  o->feet_heights = p->last_ground;
  return BPMPC_OK;
}

}  // extern "C"
