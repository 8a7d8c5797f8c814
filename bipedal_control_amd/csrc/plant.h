// The handle of the batched rigid-body plant (include/bpmpc.h: bpmpc_plant, plant.hip) and what it needs of a controller's last tick
// (controller.cpp).  The model itself is kernels/plant.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/bpmpc.h"
#include "device_handle.h"
#include "robot_model.h"
#include "kernels/plant.h"
#include "kernels/plant_input.h"
#include "kernels/sensor_noise.h"

struct bpmpc_plant {
  bpmpc::RobotModel rm;
  bpmpc::DeviceModel dm;
  bpmpc::DeviceModel* d_model = nullptr;
  bpmpc::PlantSettings defaults{};      // the keys plant.<name> of task.info over the defaults of include/bpmpc.h: every row after create / reset_params
  double torque_limits[bpmpc::kMaxJoints / 2] = {};      // torqueLimitsTask of task.info (the WBC's key); 0 without a task.info: no limit
  int device = 0, max_batch = 0, nj = 0, nv = 0;
  int last_batch = 0;                   // batch of the last set_state: the rows of d_state that hold a state (0 before the first)
  bpmpc::DeviceBuffers mem;             // every d_* below
  bpmpc::StreamHandshake hs;            // the handle's stream; foreign launches: an estimator update on the estimator's stream that reads the outputs
  hipEvent_t ev_tick = nullptr, ev_step = nullptr;      // step_controlled: the tick on the solver's stream, the step on the plant's
  double* d_state = nullptr;            // [max_batch][2 nv]: q, v
  // the per-robot row tables; each start row is the host member named beside it
  bpmpc::ParamTable params;             // contact parameters (kernels/plant.h PlantSettings): `defaults`
  bpmpc::ParamTable joints;             // joint rows: joint_start
  bpmpc::ParamTable bodies;             // body rows: body_start
  bpmpc::ParamTable sensors;            // sensor rows: sensor_start
  bpmpc::ParamTable inputs;             // input rows: input_start
  int* d_mask = nullptr;                // [max_batch] device copy of a host mask
  // device copies of host inputs
  double *d_rbd_in = nullptr, *d_pd = nullptr, *d_vd = nullptr, *d_tf = nullptr, *d_kp = nullptr, *d_kd = nullptr, *d_force = nullptr, *d_ground = nullptr;
  // stick-slip contacts (include/bpmpc.h "Plant"): per-robot tangential stiffness, anchors and flags
  double kt_start = 0.0;                // the key plant.kt of task.info (absent: 0): every robot's kt after create / reset_stiction
  bool stick = false;                   // steps launch k_plant_stick_step: kt_start > 0, or stiction has been set since create / reset_stiction
  double* d_kt = nullptr;               // [max_batch]
  double* d_kt_in = nullptr;            // [max_batch] device copy of host values
  double* d_anchor = nullptr;           // [max_batch][4][2]
  int* d_anchored = nullptr;            // [max_batch][4]
  // joint model (include/bpmpc.h "Plant", joints): per-robot joint rows
  double joint_start[bpmpc::kPlantJointParamStride] = {};      // the start row: the neutral row under the keys plantJoints.<name> of task.info
  bool joint = false;                   // steps launch k_plant_joint_step: the start row is not neutral, or rows have been set since create / reset_joint_params
  // bodies (include/bpmpc.h "Plant", bodies): per-robot body rows
  double body_start[bpmpc::kPlantBodyParamStride] = {};      // the start row: the model row under the keys plantBodies.<name> of task.info
  bool body = false;                    // steps launch k_plant_body_step: the start row is not the model row, or rows have been set since create / reset_body_params
  double* d_out = nullptr;              // the output block of k_plant_step (kernels/plant.h PlantOut)
  bpmpc_plant_outputs out{};            // its sections (leading dimension max_batch)
  // sensor model (include/bpmpc.h "Plant", sensors): per-robot rows, generator state, biases, the ring of measured samples, the sensed block
  double sensor_start[bpmpc::kSensorParamStride] = {};      // the keys plantSensors.<name> of task.info (absent: 0): every row after create
  long sensor_seed = 0;                 // the key plantSensors.seed (absent: 0): every robot's key after create / reset_sensor_params
  bool sense = false;                   // steps launch k_plant_sense behind the step kernel: the handle is switched (not untouched)
  bool sensed_valid = false;            // a step has run since the switch: the sensed block holds measurements
  unsigned* d_skey = nullptr;           // [max_batch][2]
  unsigned long long* d_sticks = nullptr;      // [max_batch][2]: tick t, samples n since the last (re)start
  double* d_sbias = nullptr;            // [max_batch][6]: gyro bias, accelerometer bias
  double* d_sring = nullptr;            // [max_batch][kSensorRing][sensor_sample_width(nj)]
  double* d_sensed = nullptr;           // the sensed block: the sections of sensor_sensed_offset, leading dimension max_batch
  bpmpc_sensor_inputs sensed{};         // its members; what the sensor model leaves alone points into `out`
  // input model (include/bpmpc.h "Plant", inputs): per-robot rows, generator state, the ring of arrived commands, the applied command
  double input_start[bpmpc::kInputParamStride] = {};      // the keys plantInputs.<name> of task.info (absent: 0): every row after create
  long input_seed = 0;                  // the key plantInputs.seed (absent: 0): every robot's key after create / reset_input_params
  bool input = false;                   // steps launch k_plant_input in front of the step kernel: the handle is switched (not untouched)
  bool applied_valid = false;           // a step has run since the switch: the applied block holds a command
  const double* last_ground = nullptr;  // feet_heights as the last step consumed them: what bpmpc_plant_applied_command reports
  unsigned* d_ikey = nullptr;           // [max_batch][2]
  unsigned long long* d_iticks = nullptr;      // [max_batch][2]: tick t, steps n since the last (re)start
  double* d_iring = nullptr;            // [max_batch][kInputRing][5 nj]
  double* d_applied = nullptr;          // [5][max_batch][nj]: the applied pos_des, vel_des, tau_ff, kp, kd
  double* d_applied_force = nullptr;    // [max_batch][3]
  int* d_iflags = nullptr;              // [3][max_batch]: delay_steps, lost, pushing of the last step
};

static_assert(bpmpc::kPlantParamStride == BPMPC_PLANT_PARAM_STRIDE, "PlantSettings follows the row layout of include/bpmpc.h");
static_assert(bpmpc::kInputParamStride == BPMPC_PLANT_INPUT_PARAM_STRIDE, "an input row follows the layout of include/bpmpc.h");
static_assert(bpmpc::kPlantJointParamStride == BPMPC_PLANT_JOINT_PARAM_STRIDE, "a joint row follows the layout of include/bpmpc.h");
static_assert(bpmpc::kPlantBodyParamStride == BPMPC_PLANT_BODY_PARAM_STRIDE, "a body row follows the layout of include/bpmpc.h");

namespace bpmpc {
// The keys plant.<name> of task.info over the defaults (NULL: the defaults); host only (capi.cpp), also behind bpmpc_plant_load_params
PlantSettings plant_load_settings(const char* task_info_path);
// A host row before it is accepted: every entry finite, kn, d0 and v_eps positive, the others not negative; throws std::invalid_argument naming the entry
void plant_check_param_row(const char* who, const double* row, int r);
// The key plant.kt of task.info (absent, or a NULL path: 0); throws std::invalid_argument naming kt when it is negative or not finite
double plant_load_stiction(const char* task_info_path);

// plant_stick.hip: one launch of k_plant_stick_step<nj> for a.batch robots on `stream`
void launch_plant_stick_step(int nj, hipStream_t stream, const DeviceModel* model, const PlantArgs& a, const PlantStickArgs& sa);

// plant_joint.hip: one launch of k_plant_joint_step<nj> for a.batch robots on `stream`
void launch_plant_joint_step(int nj, hipStream_t stream, const DeviceModel* model, const PlantArgs& a, const PlantStickArgs& sa, const PlantJointArgs& ja);
// The start row of a handle: the neutral row, the URDF's limits and <dynamics> under plantJoints.fromUrdf 1, the scalar keys plantJoints.<name> of
// task.info over both (NULL: the neutral row); host only (capi.cpp), also behind bpmpc_plant_load_joint_params
void plant_load_joint_settings(const RobotModel& rm, const char* task_info_path, double* row);
// A host row of a robot with nj joints before it is accepted (include/bpmpc.h "joints"); throws std::invalid_argument naming the entry
void plant_check_joint_row(const char* who, const double* row, int r, int nj);
// Whether a row is the neutral one as far as a robot with nj joints reads it: no armature, damping or friction, no finite limit
bool plant_joint_row_neutral(const double* row, int nj);

// plant_body.hip: one launch of k_plant_body_step<nj> for a.batch robots on `stream`
void launch_plant_body_step(int nj, hipStream_t stream, const DeviceModel* model, const PlantArgs& a, const PlantStickArgs& sa, const PlantJointArgs& ja,
                            const PlantBodyArgs& ba);
// The model row: what bpmpc_model_get returns for "body_mass", "body_com" and "body_inertia", in the layout of a body row; slots b > nj are 0
void plant_body_model_row(const RobotModel& rm, double* row);
// The start row of a handle: the model row, then the keys plantBodies.<name> of task.info (NULL: the model row); host only (capi.cpp), also behind
// bpmpc_plant_load_body_params
void plant_load_body_settings(const RobotModel& rm, const char* task_info_path, double* row);
// A host row of a robot with nj joints before it is accepted (include/bpmpc.h "bodies"); throws std::invalid_argument naming the entry
void plant_check_body_row(const char* who, const double* row, int r, int nj);
// bpmpc_plant_compose_body_row behind its null checks: row_out from row_in (both [kPlantBodyParamStride]; they may be the same array)
void plant_compose_body_row(const char* who, const double* row_in, int nj, int body, double mass_scale, const double* com_shift, double payload_mass,
                            const double* payload_pos, double* row_out);
// Whether two rows are the same as far as a robot with nj joints reads them, bit for bit
bool plant_body_rows_equal(const double* a, const double* b, int nj);

// A measured sample, in doubles: joint_pos[nj], joint_vel[nj], quat[4], angular_vel_local[3], linear_accel_local[3], contact[4] (0.0 or 1.0): one
// slot of the ring.  The sensed block holds the same members as sections of leading dimension max_batch, the contacts as four ints (2 doubles).
__host__ __device__ constexpr int sensor_sample_width(int nj) { return 2 * nj + 14; }
enum SensorSection { kSensedJointPos, kSensedJointVel, kSensedQuat, kSensedAngLocal, kSensedAccLocal, kSensedContact, kSensedEnd };
__host__ __device__ constexpr int sensor_sensed_offset(int s, int nj) {
  return s == kSensedJointPos ? 0 : s == kSensedJointVel ? nj : s == kSensedQuat ? 2 * nj : s == kSensedAngLocal ? 2 * nj + 4 : s == kSensedAccLocal ? 2 * nj + 7
         : s == kSensedContact ? 2 * nj + 10 : 2 * nj + 12;
}

struct PlantSenseArgs {
  int batch, max_batch;
  double sqrt_period;                               // sqrt of the step's period: the scale of the bias walks
  const double* params;                             // [max_batch][kSensorParamStride]
  const unsigned* key;                              // [max_batch][2]
  unsigned long long* ticks;                        // [max_batch][2]: t, n; read and advanced
  double* bias;                                     // [max_batch][6]; read and walked
  double* ring;                                     // [max_batch][kSensorRing][sensor_sample_width(nj)]
  const double* truth;                              // the output block of the step kernel (PlantArgs::out)
  double* sensed;                                   // the sensed block
};

// plant_sense.hip: one launch of k_plant_sense<nj> for a.batch robots on `stream`, behind the step kernel
void launch_plant_sense(int nj, hipStream_t stream, const PlantSenseArgs& a);
// bpmpc_plant_seed_sensors for the robots of `mask` (device; NULL: every robot below `batch`): key, t = n = 0, the turn-on biases under the robot's row
void launch_plant_seed_sensors(hipStream_t stream, int batch, const int* mask, long seed, const double* params, unsigned* key, unsigned long long* ticks, double* bias);
// n = 0 for the robots of `mask`: what bpmpc_plant_set_state does to the sensor model
void launch_plant_forget_samples(hipStream_t stream, int batch, const int* mask, unsigned long long* ticks);

struct PlantInputArgs {
  int batch, max_batch;
  long long period_ns;                              // P = input_period_ns(period) of the step
  const double* params;                             // [max_batch][kInputParamStride]
  const unsigned* key;                              // [max_batch][2]
  unsigned long long* ticks;                        // [max_batch][2]: t, n; read and advanced
  double* ring;                                     // [max_batch][kInputRing][5 nj]
  const double *pos_des, *vel_des, *tau_ff;         // the incoming command: [batch] rows of nj, cmd_stride apart (PlantArgs)
  const double *kp, *kd;                            // [batch][nj]
  int cmd_stride;
  const double* base_force;                         // [batch][3]; nullable: 0
  double* applied;                                  // [5][max_batch][nj]
  double* force;                                    // [max_batch][3]
  int* flags;                                       // [3][max_batch]: delay_steps, lost, pushing
};

// plant_input.hip: one launch of k_plant_input<nj> for a.batch robots on `stream`, in front of the step kernel
void launch_plant_input(int nj, hipStream_t stream, const PlantInputArgs& a);
// bpmpc_plant_seed_inputs for the robots of `mask` (device; NULL: every robot below `batch`): key, t = n = 0
void launch_plant_seed_inputs(hipStream_t stream, int batch, const int* mask, long seed, unsigned* key, unsigned long long* ticks);
// n = 0 for the robots of `mask`: what bpmpc_plant_set_state does to the input model
void launch_plant_forget_commands(hipStream_t stream, int batch, const int* mask, unsigned long long* ticks);

// The keys plantInputs.<name> of task.info over zeros (NULL: zeros) and the key plantInputs.seed; host only (capi.cpp)
void plant_load_input_settings(const char* task_info_path, double* row, long* seed);
// A host row before it is accepted: every entry finite and not negative, dropout <= 1, the reserved entries 0; throws std::invalid_argument naming
// the entry
void plant_check_input_row(const char* who, const double* row, int r);

// The keys plantSensors.<name> of task.info over zeros (NULL: zeros) and the key plantSensors.seed; host only (capi.cpp)
void plant_load_sensor_settings(const char* task_info_path, double* row, long* seed);
// A host row before it is accepted: every entry finite and not negative, contact_dropout <= 1, delay_steps an integer <= 8, the reserved entries 0;
// throws std::invalid_argument naming the entry
void plant_check_sensor_row(const char* who, const double* row, int r);

// What bpmpc_plant_step_controlled reads of a controller (controller.cpp): the last tick's joint_cmd ([batch][3][nj]) and the joint gains where they
// live, the stream they are written on, the batch of the last tick (0: none yet)
struct ControllerCommands {
  hipStream_t stream;
  const double *joint_cmd, *kp, *kd;
  int nj, device, max_batch, last_tick_batch;
};
ControllerCommands controller_commands(const bpmpc_controller* c);
}  // namespace bpmpc
