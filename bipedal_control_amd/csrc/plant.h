// The handle of the batched rigid-body plant (include/bpmpc.h: bpmpc_plant, plant.hip) and what it needs of a controller's last tick
// (controller.cpp).  The model itself is kernels/plant.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/bpmpc.h"
#include "device_handle.h"
#include "robot_model.h"
#include "kernels/plant.h"

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
  double* d_params = nullptr;           // [max_batch][kPlantParamStride]
  double* d_rows = nullptr;             // [max_batch + 1][kPlantParamStride] device copy of host rows; the last row holds `defaults`
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
  double* d_out = nullptr;              // the output block of k_plant_step (kernels/plant.h PlantOut)
  bpmpc_plant_outputs out{};            // its sections (leading dimension max_batch)
};

static_assert(bpmpc::kPlantParamStride == BPMPC_PLANT_PARAM_STRIDE, "PlantSettings follows the row layout of include/bpmpc.h");

namespace bpmpc {
// The keys plant.<name> of task.info over the defaults (NULL: the defaults); host only (capi.cpp), also behind bpmpc_plant_load_params
PlantSettings plant_load_settings(const char* task_info_path);
// A host row before it is accepted: every entry finite, kn, d0 and v_eps positive, the others not negative; throws std::invalid_argument naming the entry
void plant_check_param_row(const char* who, const double* row, int r);
// The key plant.kt of task.info (absent, or a NULL path: 0); throws std::invalid_argument naming kt when it is negative or not finite
double plant_load_stiction(const char* task_info_path);

// plant_stick.hip: one launch of k_plant_stick_step<nj> for a.batch robots on `stream`
void launch_plant_stick_step(int nj, hipStream_t stream, const DeviceModel* model, const PlantArgs& a, const PlantStickArgs& sa);

// What bpmpc_plant_step_controlled reads of a controller (controller.cpp): the last tick's joint_cmd ([batch][3][nj]) and the joint gains where they
// live, the stream they are written on, the batch of the last tick (0: none yet)
struct ControllerCommands {
  hipStream_t stream;
  const double *joint_cmd, *kp, *kd;
  int nj, device, max_batch, last_tick_batch;
};
ControllerCommands controller_commands(const bpmpc_controller* c);
}  // namespace bpmpc
