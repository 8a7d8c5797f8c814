/* bpmpc - C ABI of the MI355X-native batched NMPC engine (libbpmpc.so).
 *
 * Drop-in boundary for the OCS2 SQP hot path of zitongbai/bipedal_control.  Every entry point
 * names the reference interface it replaces (paths relative to the reference tree).  Plain C: pointers, sizes,
 * ints and doubles only; row-major contiguous host arrays owned by the caller unless a function says "device";
 * every call returns 0 on success or a negative bpmpc_status (never throws across the ABI); a textual reason is
 * available from bpmpc_last_error() (thread local).  A solver handle is not re-entrant (one calling thread per
 * handle, like the reference's single MPC thread, bipedal_controllers/src/BipedalController.cpp:332-351);
 * different handles are independent.  There is NO CPU fallback: creating a solver without a HIP device fails.
 *
 * State / input layout (ocs2_centroidal_model convention used by the reference, task.info:181-210,247-278):
 *   x = [h_lin/m (3), h_ang/m (3), base position (3), yaw, pitch, roll, leg joints (nj)]          nx = 12 + nj
 *   u = [F_0, F_1, F_2, F_3 (world frame, 3 each), leg joint velocities (nj)]                      nu = 12 + nj
 * Mode ids: FLY 0, LF 1, RF 2, STANCE 3 (ocs2_bipedal_robot/include/ocs2_bipedal_robot/gait/MotionPhaseDefinition.h:47-52).
 */
#ifndef BPMPC_H
#define BPMPC_H

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  BPMPC_OK = 0,
  BPMPC_ERR_INVALID_ARGUMENT = -1,
  BPMPC_ERR_IO = -2,            /* file missing / malformed (the reference throws std::invalid_argument / runtime_error) */
  BPMPC_ERR_UNSUPPORTED = -3,
  BPMPC_ERR_NO_DEVICE = -4,     /* no usable HIP device: the engine has no CPU path */
  BPMPC_ERR_DEVICE = -5,        /* HIP runtime error */
  BPMPC_ERR_CAPACITY = -6,      /* caller buffer or solver capacity too small */
  BPMPC_ERR_NUMERICAL = -7      /* non positive-definite stage Hessian etc. */
} bpmpc_status;

const char* bpmpc_last_error(void);
const char* bpmpc_version(void);

/* ---------------------------------------------------------------------------------------------------------------
 * Model = what BipedalRobotInterface builds at construction
 *   ocs2_bipedal_robot/src/BipedalRobotInterface.cpp:67-204 (constructor + setupOptimalConrolProblem),
 *   :239-291 (input-cost matrix), :298-315 (friction-cone settings), src/common/ModelSettings.cpp:40-67.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct bpmpc_model bpmpc_model;

int bpmpc_model_create(const char* urdf_path, const char* task_info_path, const char* reference_info_path, bpmpc_model** out);
/* The same with the fourth constructor argument of the reference, useHardFrictionConeConstraint (BipedalRobotInterface.h:66-69, default
 * false; BipedalRobotInterface.cpp:181-182): the friction cone of every stance contact is an INEQUALITY constraint of the problem instead of
 * a soft constraint.  The SQP solver handles it as [OCS2-upstream, recalled] ocs2_sqp does: the relaxed barrier of task.info's
 * sqp.inequalityConstraintMu / sqp.inequalityConstraintDelta (:74-75) on the LINEAR approximation of the constraint, times dt, added to the
 * stage cost before the projection (value, gradient p'(h) dh/du, Gauss-Newton Hessian p''(h) dh dh'; neither the cone's own second
 * derivative nor its hessianDiagonalShift).  Mu = 0 (the upstream default when the key is absent) means no penalty at all. */
int bpmpc_model_create_ex(const char* urdf_path, const char* task_info_path, const char* reference_info_path, int use_hard_friction_cone,
                          bpmpc_model** out);
void bpmpc_model_destroy(bpmpc_model* model);
/* CentroidalModelInfo.stateDim / inputDim / numThreeDofContacts / actuatedDofNum */
int bpmpc_model_dims(const bpmpc_model* model, int* nx, int* nu, int* n_contacts, int* n_joints);
/* Named constant blocks, copied into out[0..capacity); returns the element count or a negative status.
 * Names: "initial_state" (BipedalRobotInterface::getInitialState), "default_joint_state", "Q", "R", "robot_mass",
 * "com_height", "body_mass", "body_com", "body_inertia", "joint_parent", "joint_rotation", "joint_offset", "joint_axis",
 * "joint_lower", "joint_upper" (<limit lower= upper=> of the URDF's revolute joints, urdf::Joint::limits; -inf / +inf without the tag),
 * "joint_damping", "joint_friction" (<dynamics damping= friction=> of the URDF's revolute joints, urdf::Joint::dynamics; 0 without the tag or
 * the attribute),
 * "contact_body", "contact_offset", "cone" (mu, regularization, gripper force, hessian shift, barrier mu, barrier delta),
 * "swing" (liftOffVelocity, touchDownVelocity, swingHeight, swingTimeScale), "sqp" (dt, sqpIteration, deltaTol, g_max, g_min,
 * useFeedbackPolicy, projectStateInputEqualityConstraints (always 1), integratorType (always 0 = RK2): bpmpc_model_create returns
 * BPMPC_ERR_UNSUPPORTED with the key in bpmpc_last_error() for a task.info that sets the latter two otherwise; then the filter line
 * search's alpha_decay, alpha_min, gamma_c, armijoFactor, costTol (optional keys, upstream's defaults 0.5, 1e-4, 1e-6, 1e-4, 1e-4; refused
 * with BPMPC_ERR_UNSUPPORTED: alpha_decay outside (0, 1), alpha_min outside (0, 1], gamma_c outside [0, 1], armijoFactor outside [0, 1),
 * a negative costTol, and any pair for which 1, alpha_decay, alpha_decay^2, .. >= alpha_min has more than 64 terms)),
 * "time_horizon", "position_error_gain", "phase_transition_stance_time", "hard_cone" (flag, sqp.inequalityConstraintMu, Delta),
 * "rollout" (AbsTolODE, RelTolODE, timeStep, maxNumStepsPerSecond, mrt frequency, mpc frequency).
 * The other two solver-settings blocks the reference loads beside `sqp` (src/BipedalRobotInterface.cpp:98-100; accessors ddpSettings(),
 * ipmSettings(), include/ocs2_bipedal_robot/BipedalRobotInterface.h:78-80) are loaded and exposed.  The ipm block has no consumer (the
 * reference constructs no IPM solver either); the ddp block is what bpmpc_settings.solver = BPMPC_SOLVER_DDP runs on (the reference's DDP
 * solver lives in one stand-alone node, BipedalRobotDdpMpcNode.cpp:70-74):
 *   "ipm": dt, ipmIteration, deltaTol, g_max, g_min, computeLagrangeMultipliers, useFeedbackPolicy, initialBarrierParameter,
 *          targetBarrierParameter, barrierLinearDecreaseFactor, barrierSuperlinearDecreasePower, barrierReductionCostTol,
 *          barrierReductionConstraintTol, fractionToBoundaryMargin, usePrimalStepSizeForDual, initialSlackLowerBound,
 *          initialDualLowerBound, initialSlackMarginRate, initialDualMarginRate, nThreads, threadPriority          (booleans as 0 / 1)
 *   "ddp": algorithm (0 SLQ, 1 ILQR), maxNumIterations, minRelCost, constraintTolerance, AbsTolODE, RelTolODE, timeStep,
 *          maxNumStepsPerSecond, backwardPassIntegratorType (0 ODE45, 1 EULER, 2 ODE45_OCS2, 3 ADAMS_BASHFORTH, 4 BULIRSCH_STOER,
 *          5 MODIFIED_MIDPOINT, 6 RK4, 7 RK5_VARIABLE, 8 ADAMS_BASHFORTH_MOULTON), constraintPenaltyInitialValue,
 *          constraintPenaltyIncreaseRate, preComputeRiccatiTerms, useFeedbackPolicy, strategy (0 LINE_SEARCH, 1 LEVENBERG_MARQUARDT),
 *          lineSearch.minStepLength, lineSearch.maxStepLength, lineSearch.hessianCorrectionStrategy (0 DIAGONAL_SHIFT,
 *          1 CHOLESKY_MODIFICATION, 2 EIGENVALUE_MODIFICATION, 3 GERSHGORIN_MODIFICATION), lineSearch.hessianCorrectionMultiple,
 *          nThreads, threadPriority */
int bpmpc_model_get(const bpmpc_model* model, const char* name, double* out, int capacity);
/* joint name j (DFS order = state order); returns length or negative status */
int bpmpc_model_joint_name(const bpmpc_model* model, int j, char* out, int capacity);

/* ---------------------------------------------------------------------------------------------------------------
 * Host pre-pass of a solve = SolverBase::preRun hooks of the reference:
 *   GaitSchedule                          ocs2_bipedal_robot/src/gait/GaitSchedule.cpp:40-137
 *   loadModeSequenceTemplate              ocs2_bipedal_robot/src/gait/ModeSequenceTemplate.cpp:50-71
 *   SwitchedModelReferenceManager         ocs2_bipedal_robot/src/reference_manager/SwitchedModelReferenceManager.cpp:55-69
 *   SwingTrajectoryPlanner                ocs2_bipedal_robot/src/foot_planner/SwingTrajectoryPlanner.cpp:50-219
 *   cmdVel / goal -> TargetTrajectories   bipedal_controllers/src/TargetTrajectoriesPublisher.cpp:30-99
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct bpmpc_gait bpmpc_gait;

/* GaitSchedule(initialModeSchedule, defaultModeSequenceTemplate, phaseTransitionStanceTime) from reference.info */
int bpmpc_gait_create(const bpmpc_model* model, bpmpc_gait** out);
void bpmpc_gait_destroy(bpmpc_gait* gait);
/* loadModeSequenceTemplate(gait.info, name): switching_times[n_modes+1], modes[n_modes] */
int bpmpc_gait_load_template(const char* gait_info_path, const char* name, double* switching_times, int* modes, int capacity, int* n_modes);
/* GaitSchedule::insertModeSequenceTemplate */
int bpmpc_gait_insert_template(bpmpc_gait* gait, const double* switching_times, const int* modes, int n_modes, double start_time,
                               double final_time);
/* GaitSchedule::getModeSchedule(lower, upper) (mutating, like the reference): event_times[n_events], modes[n_events+1] */
int bpmpc_gait_mode_schedule(bpmpc_gait* gait, double lower, double upper, double* event_times, int* modes, int capacity, int* n_events);
/* SwingTrajectoryPlanner::update(schedule, terrain 0) then getZpositionConstraint / getZvelocityConstraint at n_t times:
 * z[n_t*4], zdot[n_t*4] */
int bpmpc_swing_reference(const bpmpc_model* model, const double* event_times, const int* modes, int n_events, const double* t, int n_t,
                          double* z, double* zdot);
/* [OCS2-upstream] timeDiscretizationWithEvents(t0, tf, dt, eventTimes): node_times[n], node_events[n] (0 none, 1 pre, 2 post) */
int bpmpc_time_grid(double t0, double tf, double dt, const double* event_times, int n_events, double* node_times, int* node_events,
                    int capacity, int* n_nodes);
/* cmdVelToTargetTrajectories / goalToTargetTrajectories: two-point trajectory times[2], states[2*nx] */
int bpmpc_cmd_vel_to_targets(const bpmpc_model* model, const double cmd_vel[4], double t_now, const double* x_now, double time_to_target,
                             double* times, double* states);
int bpmpc_goal_to_targets(const bpmpc_model* model, const double goal[4], double t_now, const double* x_now, double* times, double* states);

/* ---------------------------------------------------------------------------------------------------------------
 * Solver = SqpMpc / SqpSolver::runImpl for a BATCH of independent MPC problems on one MI355X
 *   construction sites replaced: bipedal_controllers/src/BipedalController.cpp:303-306,
 *                                ocs2_bipedal_robot_ros/src/BipedalRobotSqpMpcNode.cpp:70
 *   run site replaced:           MPC_MRT_Interface::advanceMpc(), BipedalController.cpp:339
 *   settings:                    task.info:66-83 (sqp), :169-179 (mpc)
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct bpmpc_solver bpmpc_solver;

typedef struct {
  int device;           /* HIP device ordinal */
  int max_batch;        /* capacity in problems */
  int max_nodes;        /* capacity in shooting intervals per problem (event nodes included) */
  int sqp_iterations;   /* <= 0: sqp.sqpIteration of task.info */
  double dt;            /* <= 0: sqp.dt of task.info */
  int return_gains;     /* allocate and compute the feedback gains K (sqp.useFeedbackPolicy) */
  int profile;          /* HIP-event timing (bpmpc_solver_kernel_time): 0 off, 1 every kernel class, 2 the linearisation kernel only */
  void* stream;         /* hipStream_t to run on; NULL = a stream owned by the solver */
  int reference_kernels; /* != 0: run the lane-emulation-verified reference kernel bodies instead of the fast variants (debugging) */
  int pipeline_chunks;  /* > 1: sweep the horizon in that many chunks, the Riccati sweep of one chunk overlapping with the
                           linearisation/projection of the earlier stages (fast kernels only, results are bit-identical).
                           0 or 1 = one launch per stage.  Measured on MI355X: no gain (both sides are bound by LDS
                           bandwidth), so it is off by default; see DESIGN.md. */
  int materialize_lq;   /* 0 (default): "fused" solve - the lineariser leaves in HBM only what the rest of the solve reads (rows 3..11
                           of A and B, b, q, r, the active rows of C, D, e, a 320-byte record of the node-dependent part of Q and R);
                           "A", "B", "Q", "R", "c", "C", "D", "e" of bpmpc_solver_read are then incomplete.
                           != 0: the complete per-node LQ approximation of the reference ([OCS2-upstream] LinearQuadraticApproximator
                           output: A, B, b, Q, R, q, r, c, C, D, e) is written - what the parity stages read and what the roofline
                           unit of bench.py is defined on.  The solution (x, u, K) is the same bits in both modes. */
  double reg_prim;      /* [OCS2-upstream] HPIPM's reg_prim (hpipm_catkin sets 1e-12): added to the diagonal of every stage Hessian
                           [R~ P~'; P~ Q~] of the projected QP, terminal stage included, before the Riccati factorisation.  0 (default) =
                           exact recursion; 1e-12 moves the H1 input step by ~5e-9 relative (tests/test_recalled_behaviours.py). */
  int solver;           /* BPMPC_SOLVER_SQP (0, default): SqpMpc, the solver of BipedalController.cpp:303-306 / BipedalRobotSqpMpcNode.cpp:70.
                           BPMPC_SOLVER_DDP (1): GaussNewtonDDP_MPC of ocs2_bipedal_robot_ros/src/BipedalRobotDdpMpcNode.cpp:70-71 with the ddp block of
                           task.info:115-156 - ONE ILQR iteration per run (ddp.algorithm ILQR, maxNumIterations 1, strategy LINE_SEARCH, hessian
                           correction DIAGONAL_SHIFT, at most 15 step lengths maxStepLength, / 2, .. >= minStepLength; anything else: BPMPC_ERR_UNSUPPORTED):
                           Euler-discretised LQ model on the time grid of the
                           nominal trajectories, equality-constrained Riccati recursion, line search over TimeTriggeredRollout roll-outs of the
                           policy (rollout block of task.info).  The solution is the accepted roll-out ON ITS OWN TIME POINTS: bpmpc_solver_fetch
                           returns them in out_t, stats.n_nodes = points - 1 (at most max_nodes), stats.step_size = the accepted step length,
                           merit_before / merit_after = performance index of the baseline / accepted roll-out; the controller is a
                           FeedforwardController (ddp.useFeedbackPolicy false) - out_K of a DDP solve holds the gains of the policy on the
                           nominal grid, for inspection.  The backward pass runs on the kernels of the SQP path (reference_kernels = 1: the
                           lane-emulated bodies), all step lengths of the line search are rolled out in one launch.  A DDP solution is NOT on the
                           shooting grid: bpmpc_solver_rollout, bpmpc_solver_constraint_values and a second bpmpc_solver_run without a new setup /
                           reset return BPMPC_ERR_UNSUPPORTED.  SLQ, later iterations on the roll-out's grid and the continuous-time backward pass
                           are not implemented. */
  int feedback_policy;  /* 0 (default): sqp.useFeedbackPolicy of task.info decides for the warm start, the policy rollout AND the controller a caller
                           builds from the solution; 1: LinearController, 2: FeedforwardController - one value for all three, as the single
                           sqp::Settings of the reference */
} bpmpc_settings;
#define BPMPC_SOLVER_SQP 0
#define BPMPC_SOLVER_DDP 1

typedef struct {
  int n_events;
  const double* event_times;  /* [n_events] */
  const int* modes;           /* [n_events + 1] */
} bpmpc_mode_schedule;

typedef struct {
  int n_points;
  const double* times;        /* [n_points] */
  const double* states;       /* [n_points * nx] */
} bpmpc_target;

typedef struct {
  int n_nodes;                /* shooting intervals of this problem */
  int iterations;             /* SQP iterations performed */
  int status;                 /* 0 ok, 1 line search took no step, 2 numerical failure (non-positive pivot in the Riccati sweep), 3 (DDP solver) the baseline
                                 roll-out failed or recorded more time points than max_nodes + 1: the nominal trajectories stay */
  int reserved;
  double merit_before, dynamics_sse_before, equality_sse_before;   /* PerformanceIndex of the last linearisation */
  double merit_after, dynamics_sse_after, equality_sse_after;      /* after the accepted step */
  double step_size;           /* alpha of the last iteration (0 = rejected) */
  double armijo_descent;
  double dx_norm, du_norm;
} bpmpc_stats;

int bpmpc_solver_create(const bpmpc_model* model, const bpmpc_settings* settings, bpmpc_solver** out);
void bpmpc_solver_destroy(bpmpc_solver* solver);

/* One call = host pre-pass + upload + SQP iteration(s) + download, for `batch` problems with horizon [t0, t0 + horizon].
 *   t0[batch], x0[batch*nx] (measured state)
 *   schedules: n_schedules == 1 (shared; all t0 must be equal) or == batch
 *   targets[batch]
 *   warm_x[batch*(max_nodes+1)*nx], warm_u[batch*max_nodes*nu]: initial iterate on this solve's grid, or NULL for the
 *     cold start of BipedalRobotInitializer::compute (src/initialization/BipedalRobotInitializer.cpp:56-63)
 * outputs (strides use max_nodes; entries beyond n_nodes are untouched):
 *   out_t[batch*(max_nodes+1)], out_x[batch*(max_nodes+1)*nx], out_u[batch*max_nodes*nu],
 *   out_K[batch*max_nodes*nu*nx] (nullable; needs return_gains), stats[batch] */
int bpmpc_solve_batch(bpmpc_solver* solver, int batch, double horizon, const double* t0, const double* x0,
                      const bpmpc_mode_schedule* schedules, int n_schedules, const bpmpc_target* targets, const double* warm_x,
                      const double* warm_u, double* out_t, double* out_x, double* out_u, double* out_K, bpmpc_stats* stats);

/* The same work split into stages so that a caller can keep everything resident in HBM between solves
 * (bench.py times bpmpc_solver_run only; inputs are already on the device when the timed region starts). */
int bpmpc_solver_setup(bpmpc_solver* solver, int batch, double horizon, const double* t0, const double* x0,
                       const bpmpc_mode_schedule* schedules, int n_schedules, const bpmpc_target* targets, const double* warm_x,
                       const double* warm_u);
/* Receding-horizon step: like bpmpc_solver_setup, but the initial iterate is taken from the previous solve of this handle
 * (same batch), entirely on the device: inside the time span of the previous solution u_k = uff(t_k) + K(t_k) x_k and x_{k+1} is
 * interpolated, beyond it the initializer guess is used ([OCS2-upstream] SqpSolver::initializeStateInputTrajectories with
 * mpc.coldStart false, task.info:173, and sqp.useFeedbackPolicy true, task.info:80 - the MPC loop of
 * bipedal_controllers/src/BipedalController.cpp:332-350).  Needs a completed bpmpc_solver_run on the handle. */
int bpmpc_solver_setup_from_previous(bpmpc_solver* solver, int batch, double horizon, const double* t0, const double* x0,
                                     const bpmpc_mode_schedule* schedules, int n_schedules, const bpmpc_target* targets);
/* Device-side reference generation: the whole pre-pass of a solve on the GPU.  Problem b follows
 * gait template gaits[gait_of_problem[b]] (a ModeSequenceTemplate of gait.info; < 0 or n_gaits == 0: the initial schedule of
 * reference.info only), inserted at gait_start[b] into GaitSchedule(initialModeSchedule, defaultModeSequenceTemplate) and asked for
 * [t0 - horizon, t0 + 2 horizon] (GaitSchedule.cpp:40-137 as called from SwitchedModelReferenceManager.cpp:55-69); swing-height
 * splines, shooting grid and node tables are derived from it per distinct (t0, gait, start), and the target trajectory is
 * cmdVelToTargetTrajectories(cmd_vel[b], t0[b], x0[b]) reaching time_to_target (<= 0: horizon) ahead
 * (TargetTrajectoriesPublisher.cpp:40-62); with command_kind = 1 the four numbers are a goal pose (x, y, unused, yaw) and the
 * target is goalToTargetTrajectories (TargetTrajectoriesPublisher.cpp:64-99, reach time from targetDisplacementVelocity /
 * targetRotationVelocity of reference.info).  Tables are bit-identical to those bpmpc_solver_setup builds on the host from the same
 * schedule; errors (undefined take-off / touch-down, grid longer than max_nodes) are reported the same way.
 * x0 == NULL: the end states of the last bpmpc_solver_rollout on this handle (closed loop without leaving the device).
 * from_previous != 0: initial iterate shifted from the previous solve as in bpmpc_solver_setup_from_previous, else cold start. */
typedef struct {
  int n_modes;
  const double* switching_times; /* n_modes + 1 */
  const int* modes;              /* n_modes */
} bpmpc_gait_template;
int bpmpc_solver_setup_commands(bpmpc_solver* solver, int batch, double horizon, const double* t0, const double* x0,
                                const bpmpc_gait_template* gaits, int n_gaits, const int* gait_of_problem, const double* gait_start,
                                const double* cmd_vel /* [batch][4]: vx, vy, vz, yaw rate */, int command_kind, double time_to_target,
                                int from_previous);
/* Device-resident gait schedules: one GaitSchedule per robot kept on the device between setups, changed at run time by gait
 * commands with the semantics of GaitReceiver (ocs2_bipedal_robot/src/gait/GaitReceiver.cpp:49-59), so that every robot runs on
 * its own gait clock and its schedule is the result of its whole command history (GaitSchedule.cpp:46-137, owned by
 * SwitchedModelReferenceManager.cpp:62-69 and shared with the GaitReceiver).  Per robot b, horizon H:
 *   create / reset   GaitSchedule(initialModeSchedule, defaultModeSequenceTemplate, phaseTransitionStanceTime) of reference.info
 *                    (what bpmpc_gait_create builds); nothing pending.  The template library gaits[0 .. n_gaits) is uploaded once.
 *   insert           insertModeSequenceTemplate(gaits[g], start, final), recorded per robot (a second insert before the setup
 *                    replaces the first; g < 0 leaves the robot's pending insert as it is) and applied by the next setup BEFORE its
 *                    getModeSchedule: tiling from a start far in the past (a phase offset) only fits the event capacity once the
 *                    compaction bound t0 - H of that setup is known.
 *   command          GaitReceiver::mpcModeSequenceCallback: g >= 0 becomes the robot's pending template (the latest command before a
 *                    setup wins), g < 0 leaves the robot's pending command as it is.  gait may be a device array (inputs_on_device:
 *                    ordered on the solver's stream; its template indices are checked by the next setup).
 *   setup at t0[b]   SolverBase::preRun [OCS2-upstream, recalled]: the reference manager first, then the synchronized modules -
 *                    1. getModeSchedule(t0 - H, t0 + 2 H) (mutating): its window feeds this setup's grid, swing references, node tables;
 *                    2. a pending command: insertModeSequenceTemplate(gaits[g], t0 + H, H) - GaitReceiver's literal (finalTime,
 *                       timeHorizon) - and the command is no longer pending.
 *                    A command therefore shapes the NEXT setup's window, from t0 + H on, behind a phaseTransitionStanceTime STANCE
 *                    phase unless the last phase already is STANCE.
 *   rejected setup   (tiling order, event capacity, grid longer than max_nodes, undefined take-off / touch-down; the statuses and
 *                    messages of bpmpc_solver_setup_commands) changes no robot's schedule nor pending insert / command: the schedules
 *                    are double-buffered and the new ones are kept only when every robot was accepted.
 *   capacity         the per-robot event capacity and compaction of bpmpc_solver_setup_commands (only what getModeSchedule would erase
 *                    is dropped), so t0 may jump arbitrarily far ahead.
 * Robots with one history (create / reset, inserts, commands and the t0 of every setup alike) share a grid; a fleet that never
 * diverged keeps a single grid.  Robots behind `batch` keep their schedules.  Destroy the gait batch before its solver.
 * bpmpc_solver_setup_gaits is bpmpc_solver_setup_commands with the schedules taken from the gait batch (x0 = NULL, from_previous,
 * command kinds, errors alike); bpmpc_gait_batch_mode_schedule reports robot's schedule after the last setup (not mutating; it
 * synchronises).  Invalid handles, a handle of another solver, batch > max_batch, an unknown template index or robot, NULL
 * pointers: BPMPC_ERR_INVALID_ARGUMENT. */
typedef struct bpmpc_gait_batch bpmpc_gait_batch;
int bpmpc_gait_batch_create(bpmpc_solver* solver, const bpmpc_gait_template* gaits, int n_gaits, bpmpc_gait_batch** out);
void bpmpc_gait_batch_destroy(bpmpc_gait_batch* gaits);
int bpmpc_gait_batch_reset(bpmpc_gait_batch* gaits);
int bpmpc_gait_batch_insert(bpmpc_gait_batch* gaits, int batch, const int* gait, const double* start_time, const double* final_time);
int bpmpc_gait_batch_command(bpmpc_gait_batch* gaits, int batch, const int* gait, int inputs_on_device);
int bpmpc_gait_batch_mode_schedule(bpmpc_gait_batch* gaits, int robot, double* event_times, int* modes, int capacity, int* n_events);
int bpmpc_solver_setup_gaits(bpmpc_solver* solver, bpmpc_gait_batch* gaits, int batch, double horizon, const double* t0, const double* x0,
                             const double* cmd_vel /* [batch][4] */, int command_kind, double time_to_target, int from_previous);
/* Device-resident target trajectories: one TargetTrajectories per robot kept on the device between setups, the other half of the reference
 * manager beside the gait batch.  The reference changes a robot's target only when a command arrives - BipedalController::starting sets the
 * single point at the current observation (BipedalController.cpp:145,153), TargetTrajectoriesPublisher turns a /cmd_vel or goal message into a
 * two-point trajectory from the observation AT THE TIME OF THE MESSAGE (TargetTrajectoriesPublisher.h:48-87, .cpp:30-99) - and every MPC solve in
 * between interpolates that same trajectory [OCS2-upstream, recalled: ReferenceManager::setTargetTrajectories / preSolverRun].  Per robot b:
 *   storage          n points (n <= max_points, given at create, 2 .. 64), times[max_points], states[max_points][nx], and the status row
 *                    status[b][4] = (messages applied, messages dropped, source of the stored target, n) with the sources 0 none, 1 start,
 *                    2 velocity, 3 goal, 4 trajectory.  Robots at or beyond `batch` and robots with mask[b] == 0 (mask == NULL: every robot
 *                    below batch) keep every bit of theirs.
 *   create / reset   no target (n = 0), counters and source 0.
 *   start            starting(): the target becomes the single point (t_obs[b], x_obs[b]).
 *   cmd_vel          cmdVelToTargetTrajectories(cmd[b] = (vx, vy, vz, yaw rate), observation), reaching time_to_target ahead; <= 0 means
 *                    mpc.timeHorizon of task.info, the reference's TIME_TO_TARGET.
 *   goal             goalToTargetTrajectories(goal[b] = (x, y, unused, yaw), observation): the reach time t_obs + max(|dyaw| /
 *                    targetRotationVelocity, distance / targetDisplacementVelocity) is fixed by this call.
 *                    Both are computed ONCE, from the observation passed to the call, with the arithmetic of bpmpc_solver_setup_commands' targets;
 *                    the stored points stay until the next call that touches the robot.  The reference's quirk is kept: a robot whose t_obs
 *                    equals 0.0 ignores a velocity or goal message (TargetTrajectoriesPublisher.h:49,75) and its dropped counter goes up;
 *                    start and set_targets are not messages and ignore nothing.
 *   set_targets      an arbitrary TargetTrajectories (a waypoint route): the first n_points[b] entries of times[b] and states[b].
 *   x_obs == NULL    the observations already on the device, what bpmpc_solver_setup_commands(x0 = NULL) starts from: the observations of the
 *                    last controller tick, otherwise the end states of the last rollout.  Without such a source, or with another batch:
 *                    BPMPC_ERR_INVALID_ARGUMENT.  t_obs is always given.
 *   inputs_on_device != 0: mask, the command rows, t_obs, x_obs, n_points, times and states are device pointers, ordered on the solver's
 *                    stream; nothing is validated (a count outside 0 .. max_points is held inside it) and the call only enqueues.  Host arrays
 *                    are validated - every used entry finite, n_points in 1 .. max_points, times not decreasing; a bad value names the robot
 *                    and the entry in bpmpc_last_error(), changes nothing and returns BPMPC_ERR_INVALID_ARGUMENT - and the call returns when
 *                    they have been read.
 *   get_targets      robot's stored trajectory: *n_points, then its times and states when n <= capacity (else BPMPC_ERR_CAPACITY); get_status
 *                    the status rows of robots 0 .. batch - 1.  Both synchronise.
 *   attach           bpmpc_solver_attach_commands(solver, commands): while attached, bpmpc_solver_setup_commands and bpmpc_solver_setup_gaits
 *                    ignore cmd_vel (may be NULL), command_kind and time_to_target and take every robot's target from the command batch: the
 *                    points the host path bpmpc_solver_setup keeps of a TargetTrajectories - the last one at or before t0, the ones inside
 *                    [t0, t0 + horizon], the first one behind - so the references equal those of bpmpc_solver_setup given the stored trajectory.
 *                    More than 8 such points, or a robot without a target, rejects the setup with the host path's message and the robot's
 *                    number (BPMPC_ERR_INVALID_ARGUMENT).  A setup only reads the command batch: a rejected one leaves it bit for bit as it
 *                    was.  NULL detaches; a detached solver runs what a solver that never had a command batch runs.  SQP and DDP alike.
 * The handle is created on a solver, enqueues on its stream, and is destroyed before it.  Null handles, a handle of another solver, batch >
 * max_batch, max_points outside 2 .. 64, a robot out of range, NULL pointers: BPMPC_ERR_INVALID_ARGUMENT. */
typedef struct bpmpc_command_batch bpmpc_command_batch;
int bpmpc_command_batch_create(bpmpc_solver* solver, int max_points, bpmpc_command_batch** out);
void bpmpc_command_batch_destroy(bpmpc_command_batch* commands);
int bpmpc_command_batch_reset(bpmpc_command_batch* commands);
int bpmpc_command_batch_start(bpmpc_command_batch* commands, int batch, const int* mask, const double* t_obs, const double* x_obs, int inputs_on_device);
int bpmpc_command_batch_cmd_vel(bpmpc_command_batch* commands, int batch, const int* mask, const double* cmd /* [batch][4] */, const double* t_obs,
                                const double* x_obs, double time_to_target, int inputs_on_device);
int bpmpc_command_batch_goal(bpmpc_command_batch* commands, int batch, const int* mask, const double* goal /* [batch][4]: x, y, unused, yaw */,
                             const double* t_obs, const double* x_obs, int inputs_on_device);
int bpmpc_command_batch_set_targets(bpmpc_command_batch* commands, int batch, const int* mask, const int* n_points /* [batch] */,
                                    const double* times /* [batch][max_points] */, const double* states /* [batch][max_points][nx] */,
                                    int inputs_on_device);
int bpmpc_command_batch_get_targets(bpmpc_command_batch* commands, int robot, double* times, double* states, int capacity, int* n_points);
int bpmpc_command_batch_get_status(bpmpc_command_batch* commands, int batch, int* status /* [batch][4] */);
int bpmpc_solver_attach_commands(bpmpc_solver* solver, bpmpc_command_batch* commands);
/* MRT side: MRT_BASE::rolloutPolicy for every problem of the batch - TimeTriggeredRollout::run from
 * (t_start[b], x_start[b]) over `duration` under the LinearController of the last solve (u = uff(t) + K(t) x), ODE45 with the
 * rollout block of task.info (AbsTolODE, RelTolODE, timeStep, maxNumStepsPerSecond), restarted at the mode-schedule events inside
 * the window; what MRT_ROS_Dummy_Loop (ocs2_bipedal_robot_ros/src/BipedalRobotDummyNode.cpp:72-86) and BipedalController.cpp:322
 * obtain through initRollout.  t_start / x_start NULL: initial time / measured state of the last solve.  Outputs (nullable):
 * x_end[batch*nx], u_end[batch*nu] (the policy at the end point), steps[batch*2] (accepted, rejected integrator steps).  The end
 * states also stay on the device: bpmpc_solver_setup_commands(x0 = NULL) starts the next solve from them; with all three outputs
 * NULL the call only enqueues and integrator failures are reported by that next setup. */
int bpmpc_solver_rollout(bpmpc_solver* solver, const double* t_start, const double* x_start, double duration, double* x_end,
                         double* u_end, int* steps);
int bpmpc_solver_reset(bpmpc_solver* solver);   /* restore the initial iterate of the last setup (device-side copy, async) */
int bpmpc_solver_run(bpmpc_solver* solver);     /* enqueue the SQP iteration(s) on the solver's stream */
int bpmpc_solver_sync(bpmpc_solver* solver);
int bpmpc_solver_fetch(bpmpc_solver* solver, double* out_t, double* out_x, double* out_u, double* out_K, bpmpc_stats* stats);
/* Run one stage of an iteration on the current iterate (parity tests, roofline measurement):
 * "linearize", "project", "riccati", "linesearch"; "value" with the value function enabled ("Value function" below); "dual" with the dual
 * solution enabled ("Dual solution" below; behind "value"). */
int bpmpc_solver_stage(bpmpc_solver* solver, const char* stage);
/* Copy a named device buffer to the host (tests): "x","u","xref","A","B","b","Q","R","P","q","r","c","C","D","e","nc","perf",
 * "Px","Pu","Pe","nut","dx","du","K","Acl","summary","stats","g_kind","g_mode","g_nodes","g_dt","g_start","g_zref","g_zdref","g_time",
 * "p_grid","x0".  The projected LQ model depends on the kernel set:
 *   settings.reference_kernels = 1:  plain matrices "At","Bt","bt","Qt","Rt","Pt","qt","rt" and the gain scratch "Kt","kt";
 *   fast kernels (default):          the packed layout "Wt" = [At | bt | Bt] (nx rows of WP columns; on the default structured path only
 *                                    its rows 0..11 are written: the JOINT rows 12..nx-1 read as zeros or as the leftovers of an earlier
 *                                    run - they are [I | b | 0] + dt * "Vt" (row j of Vt = joint row 12 + j of [Px | Pe | Pu], dt = g_dt of
 *                                    the node) and every sweep completes them itself; they are written with BPMPC_WT_JOINT_ROWS=1,
 *                                    BPMPC_DENSE_PROJECT=1 or reference_kernels), "Qp" = [Qt | qt] (nx rows of 32
 *                                    columns), "Mt" = [Pt | rt | Rt] (nu rows of WP columns), WP = 16 * ceil((nx + 1 + nu) / 16); block
 *                                    columns beyond nx + 1 + nut and rows >= nut of Mt are not written (kernels/project_node.h PackedLq);
 *                                    the plain names return "unknown buffer".
 * The elimination outputs depend on the path as well: on the default fast path (structured elimination, input weight without force /
 * joint-velocity cross terms) only "Vt" (the joint rows of [Px | Pe | Pu], nj rows of WP columns; columns at and beyond
 * 16 * ceil((nx + 1 + nut) / 16) are not written and hold whatever an earlier, wider node left there), "Pe" and "nut" are written -
 * "Px" and "Pu" are NOT (they read as zeros or as the leftovers of an earlier run on another path); they are written with
 * BPMPC_DENSE_PROJECT=1 (environment, read when the solver is created) and by the reference kernels.
 * Integer buffers are converted to double.  Returns the element count or a negative status; out == NULL only queries the element
 * count. */
int bpmpc_solver_read(bpmpc_solver* solver, const char* name, double* out, long capacity);
/* Device pointers of the iterate, for zero-copy hand-off (e.g. an RCCL gather through torch.distributed):
 * x: batch*(max_nodes+1)*nx doubles, u: batch*max_nodes*nu doubles.  Valid until the next setup with a warm start from the previous
 * solve (the solution buffers then trade places with the kept copy); query again after such a setup. */
int bpmpc_solver_device_trajectories(bpmpc_solver* solver, double** x_dev, double** u_dev);
/* Asynchronous device-to-device copy of the iterate into caller-owned device buffers (same shapes as above) on the
 * solver's stream - e.g. torch tensors that are then all-gathered over RCCL. */
int bpmpc_solver_export_trajectories(bpmpc_solver* solver, double* x_dst_dev, double* u_dst_dev);
/* Solution metrics for solver observers (the reference adds SolverObserver::ConstraintTermObserver on "<foot>_zeroVelocity",
 * ocs2_bipedal_robot_ros/src/BipedalRobotSqpMpcNode.cpp:74-86): the values of the active state-input equality rows at the CURRENT iterate
 * (after a solve: the solution) of every intermediate node, values[b][k][0..rows[b][k]) in registration order per contact i = 0..3:
 * zeroForce_i (3 rows, swing), zeroVelocity_i (3 rows, stance), normalVelocity_i (1 row, swing) (BipedalRobotInterface.cpp:187-191).
 * values: [batch][max_nodes][16]; rows, modes (optional): [batch][max_nodes], 0 / -1 for event nodes and beyond the grid; mode bit 0 =
 * left foot in stance, bit 1 = right foot (MotionPhaseDefinition.h:57-76).  A debugging path: synchronises. */
int bpmpc_solver_constraint_values(bpmpc_solver* solver, double* values, int* rows, int* modes);
/* Change settings.materialize_lq of a live solver. */
int bpmpc_solver_set_materialize(bpmpc_solver* solver, int materialize_lq);
/* Change settings.profile of a live solver (0 / 1 / 2 as above). */
int bpmpc_solver_set_profile(bpmpc_solver* solver, int level);
/* Accumulated HIP-event time of one kernel class since the last call with reset != 0 (needs settings.profile):
 * "prepare","linearize","project","riccati","linesearch". */
int bpmpc_solver_kernel_time(bpmpc_solver* solver, const char* kernel, int reset, double* total_ms, int* launches);
/* Sizes chosen by the last setup: nodes per problem (max over the batch) and number of distinct grids. */
int bpmpc_solver_layout(const bpmpc_solver* solver, int* batch, int* n_nodes_max, int* n_grids, int* nx, int* nu);

/* ---------------------------------------------------------------------------------------------------------------
 * Whole-body controller = WeightedWbc for a BATCH of robots (first slice)
 *   construction replaced:  bipedal_controllers/src/BipedalController.cpp:97-100 (WeightedWbc + loadTasksSetting(taskFile))
 *   update site replaced:   bipedal_controllers/src/BipedalController.cpp:229   wbc_->update(optimizedState, optimizedInput, measuredRbdState_, plannedMode, period)
 *   tasks:                  bipedal_wbc/src/WbcBase.cpp:162-403, QP: bipedal_wbc/src/WeightedWbc.cpp:20-84 (qpOASES, nWSR 20)
 * Decision vector per robot: [generalised accelerations (6 + nj), contact forces (12), joint torques (nj)].
 * rbd_state_measured per robot: [ZYX Euler (3), base position (3), joints (nj), world angular velocity (3), linear velocity (3), joint velocities (nj)]
 * (CentroidalModelRbdConversions layout, WbcBase.cpp:58-77).  A QP that is not solved leaves the robot's previous solution in place - lastQpSol_,
 * WeightedWbc.cpp:68-81 - and sets status 1.  Status 1 means "not solved by this active-set iteration within 20 working-set changes (or it met a
 * singular working set), or the equalities are inconsistent"; it does not mean that the QP is infeasible.  The handle keeps the last solutions
 * between calls (zero after creation / bpmpc_wbc_reset).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct bpmpc_wbc bpmpc_wbc;
int bpmpc_wbc_create(const bpmpc_model* model, const char* task_info_path, int device, int max_batch, bpmpc_wbc** out);
void bpmpc_wbc_destroy(bpmpc_wbc* wbc);
int bpmpc_wbc_dims(const bpmpc_wbc* wbc, int* n_decision_variables, int* n_generalized_coordinates);
/* state_desired[batch*nx], input_desired[batch*nu], rbd_state_measured[batch*2*(6+nj)], mode[batch] -> solution[batch*n], status[batch] (nullable);
 * debug (nullable, tests): batch*1024 doubles - M, nle, J, Jdot v, base-task right-hand side, rank / iterations / working-set size, why the
 * iteration ended (0 solved, 1 equalities inconsistent, 2 singular KKT system, 3 change budget exhausted, 4 working set too large), the smallest
 * KKT pivot accepted and the one rejected (or 0), the working set */
int bpmpc_wbc_update(bpmpc_wbc* wbc, int batch, const double* state_desired, const double* input_desired, const double* rbd_state_measured,
                     const int* mode, double period, double* solution, int* status, double* debug);
int bpmpc_wbc_reset(bpmpc_wbc* wbc);

/* ---------------------------------------------------------------------------------------------------------------
 * Controller tick = BipedalController::update for a BATCH of robots, on the device (bipedal_controllers/src/BipedalController.cpp:186-262)
 *   observation   :397-403  computeCentroidalStateFromRbdModel(measured rbd state) + yaw unwrap: from rbd[b] (the layout of
 *                           bpmpc_wbc_update) q = [base position, zyx, joints], v = [linear velocity, E(zyx)^-1 angular velocity, joint
 *                           velocities], x_obs = [A(q) v / m, q] (A: centroidal momentum matrix in Euler-rate base coordinates, m: robot mass),
 *                           then x_obs[9] = yaw_last + shortest_angular_distance(yaw_last, x_obs[9]) (distance in (-pi, pi]); yaw_last is kept
 *                           per robot on the handle, 0 after create / reset (BipedalController::starting)
 *   policy        :199      evaluatePolicy(t, x_obs) of the last completed bpmpc_solver_run, see bpmpc_solver_evaluate_policy
 *   WBC           :229      the WBC handle's WeightedWbc::update(x*, u*, rbd, planned mode): the same kernel and the same per-robot last QP
 *                           solutions as bpmpc_wbc_update (the fallback of WeightedWbc.cpp:68-81 is the same whichever entry point ran)
 *   safety        SafetyChecker::check (SafetyChecker.h:39-52): safe = 0 when |x_obs[10]| > pi/3 or |x_obs[11]| > pi/3 (the limit passes)
 *   commands      :237-252  joint_cmd[b] = [posDes = x*[12:], velDes = u*[12:], torque = last nj entries of the WBC solution] ([3][nj];
 *                           the joint gains kp / kd of the five-tuple are per-robot data of the controller, see "Run-time parameters" below,
 *                           and so is the torque the hardware layer forms from the five-tuple)
 * Everything runs on the solver's stream (three launches: k_tick_observe_policy, k_wbc, k_tick_commands).  The observations also close the
 * loop: bpmpc_solver_setup_commands(x0 = NULL) starts from the states of the last rollout OR the last tick, whichever ran last on the solver.
 * ------------------------------------------------------------------------------------------------------------- */
/* MRT_BASE::evaluatePolicy for every problem of the last completed bpmpc_solver_run (host in / out; synchronises): t[batch], x[batch*nx] ->
 * x_opt[batch*nx] = LinearInterpolation of the solution's states at t (clamped before the first and after the last node),
 * u_opt[batch*nu] = uff(t) + K(t) x with the feedback policy (the input and gain of a pre-event node and of the terminal node repeat the
 * previous one, uff_j = u_j - K_j x_j: multiple_shooting::toPrimalSolution [OCS2-upstream, recalled]) or u(t) without it, planned_mode[batch]
 * = ModeSchedule::modeAtTime(t) (a time exactly on an event belongs to the earlier mode; before the first / after the last node the mode of
 * the first / last interval of the solution - a clamp to its time span).  batch must equal the batch of the last setup.
 * BPMPC_ERR_INVALID_ARGUMENT: no completed run since the last setup, batch mismatch; BPMPC_ERR_UNSUPPORTED: the DDP solver. */
int bpmpc_solver_evaluate_policy(bpmpc_solver* solver, int batch, const double* t, const double* x, double* x_opt, double* u_opt, int* planned_mode);

typedef struct bpmpc_controller bpmpc_controller;
/* Per-robot outputs of a tick (row-major, strides of the WBC's max_batch do not apply: [batch] leading):
 * x_obs[batch*nx], x_opt[batch*nx], u_opt[batch*nu], joint_cmd[batch*3*nj], wbc_solution[batch*n] (bpmpc_wbc_dims), planned_mode[batch],
 * wbc_status[batch], safe[batch]. */
typedef struct {
  double *x_obs, *x_opt, *u_opt, *joint_cmd, *wbc_solution;
  int *planned_mode, *wbc_status, *safe;
} bpmpc_tick_outputs;
/* Solver and WBC of the same robot on the same device; the handles must outlive the controller. */
int bpmpc_controller_create(bpmpc_solver* solver, bpmpc_wbc* wbc, bpmpc_controller** out);
void bpmpc_controller_destroy(bpmpc_controller* controller);
int bpmpc_controller_reset(bpmpc_controller* controller);   /* yaw_last = 0 for every robot */
/* One tick for `batch` robots: t[batch] (policy time), rbd[batch*2*(6+nj)] measured rigid-body state.  inputs_on_device != 0: t and rbd are
 * device pointers (e.g. the tensors of a GPU simulator).  host_out NULL: nothing is copied back or synchronised (read the results through
 * bpmpc_controller_device_outputs); otherwise every non-NULL member receives its block and the call synchronises.  batch must equal the
 * batch of the solver's last setup (else BPMPC_ERR_INVALID_ARGUMENT) and be at most the WBC's max_batch (else BPMPC_ERR_CAPACITY); a tick
 * needs a completed bpmpc_solver_run since that setup (BPMPC_ERR_INVALID_ARGUMENT) and an SQP solver (DDP: BPMPC_ERR_UNSUPPORTED).
 * period: as in bpmpc_wbc_update (unused by the reference). */
int bpmpc_controller_tick(bpmpc_controller* controller, int batch, const double* t, const double* rbd, int inputs_on_device, double period,
                          const bpmpc_tick_outputs* host_out);
/* Device pointers of the outputs of the last tick (same shapes as above, leading dimension the WBC's max_batch).  wbc_solution / wbc_status
 * are the WBC handle's own buffers: a later bpmpc_wbc_update overwrites them. */
int bpmpc_controller_device_outputs(bpmpc_controller* controller, bpmpc_tick_outputs* dev_out);

/* ---------------------------------------------------------------------------------------------------------------
 * Per-robot restarts: BipedalController::starting (bipedal_controllers/src/BipedalController.cpp:123-179) for the robots of a mask, while
 * every other robot of the batch goes on untouched (not a single bit of its state changes).  mask[batch]: non-zero = restart this robot.
 * inputs_on_device != 0: mask and the state arrays are device pointers (e.g. (safe == 0) of bpmpc_controller_device_outputs) and the call only
 * enqueues work; with host arrays the call synchronises.  Restarts recorded before one setup accumulate: the masks are OR-ed and the latest
 * state given for a robot wins.  Null handles or masks: BPMPC_ERR_INVALID_ARGUMENT.
 *   solver      bpmpc_solver_restart = MPC_BASE::reset per problem [OCS2-upstream, recalled] (:147-148).  batch must equal the batch of the last
 *               setup (before any setup or otherwise: BPMPC_ERR_INVALID_ARGUMENT); the DDP solver: BPMPC_ERR_UNSUPPORTED.  x_new (nullable,
 *               [batch*nx]): its rows of masked problems replace those of the closed-loop start that setup_commands / setup_gaits(x0 = NULL)
 *               read (the end states of the last rollout or the observations of the last tick, whichever ran last).  The next accepted setup of
 *               any kind consumes the restart: with a shifted warm start (setup_from_previous, from_previous != 0) the masked problems keep the
 *               initializer's guess of a cold setup and the others are shifted as before; a cold setup or the caller's warm arrays win for
 *               everyone.  A rejected setup leaves the restart pending.  From the restart to the first completed bpmpc_solver_run after that
 *               setup, bpmpc_solver_evaluate_policy, bpmpc_controller_tick and bpmpc_solver_rollout return BPMPC_ERR_INVALID_ARGUMENT (the state
 *               of a fresh handle before its first run: the controller waits for the first policy of the new episode, :154).
 *   WBC         bpmpc_wbc_restart = clearLastQpSol (:179): the masked robots' last solutions and statuses become 0.  Enqueued on the WBC handle's
 *               stream; a later controller tick on another stream waits for it.  batch > max_batch: BPMPC_ERR_CAPACITY.
 *   gait batch  bpmpc_gait_batch_restart: the masked robots go back to their state after create / reset; their pending insert and command are
 *               dropped.  The next accepted bpmpc_solver_setup_gaits applies the restart first, so an insert or command recorded after the
 *               restart applies to the new episode; a rejected setup leaves it pending; robots restarted together share one grid again.  A
 *               device mask is read back by that setup (which synchronises anyway).  Separate from the controller restart on purpose: starting()
 *               leaves the gait schedule alone, whether a new episode starts a new gait clock is the caller's choice.
 *   controller  bpmpc_controller_restart, on the solver's stream: k_restart_observe (the tick's observation of rbd[b] with the yaw unwrapped
 *               against 0, :126-127, so wrapped to (-pi, pi]) writes x_obs[b] and yaw_last[b] of the masked robots; then bpmpc_solver_restart
 *               with those observations as x_new and bpmpc_wbc_restart.  batch: the solver's last setup, at most the WBC's max_batch.
 * The loop after a fall: restart -> bpmpc_solver_setup_gaits(x0 = NULL, from_previous = 1) -> run -> tick.  Not reproduced: the one-point target
 * of :145 (the batched setups take their targets from the commands: cmd_vel = 0 holds the pose), the DDP solver, the stop request itself.
 * ------------------------------------------------------------------------------------------------------------- */
int bpmpc_solver_restart(bpmpc_solver* solver, int batch, const int* mask, const double* x_new, int inputs_on_device);
int bpmpc_wbc_restart(bpmpc_wbc* wbc, int batch, const int* mask, int inputs_on_device);
int bpmpc_gait_batch_restart(bpmpc_gait_batch* gaits, int batch, const int* mask, int inputs_on_device);
/* rbd[batch*2*(6+nj)]: the measured rigid-body states the restarted robots start from (layout of bpmpc_controller_tick). */
int bpmpc_controller_restart(bpmpc_controller* controller, int batch, const int* mask, const double* rbd, int inputs_on_device);

/* ---------------------------------------------------------------------------------------------------------------
 * Run-time parameters: BipedalController::dynamicReconfigCallback (bipedal_controllers/src/BipedalController.cpp:407-478), the reference's only
 * run-time tuning interface, for every robot of a batch separately.  It sets the base-task PD gains (WbcBase::setBasePDGains, WbcBase.h:66-69),
 * the swing-leg PD gains (setSwingLegPDGains, WbcBase.h:55-58), the three task weights (WeightedWbc::setWeights, WeightedWbc.h:48-52) and the
 * joint-level kp / kd that update() hands to HybridJointHandle::setCommand (:250-254).
 *   WBC         every robot of a WBC handle has a parameter row of BPMPC_WBC_PARAM_STRIDE doubles on the device; k_wbc reads robot b's row:
 *                 [0..5]   base kp: position x, y, z, orientation x, y, z (the order of baseAccelPDTask.baseKp)      setBasePDGains
 *                 [6..11]  base kd, same order                                                                     setBasePDGains
 *                 [12,13]  swing-leg kp, kd                                                                        setSwingLegPDGains
 *                 [14..16] weights: swing leg, base acceleration, contact force                                    setWeights
 *                 [17]     friction coefficient of the WBC's pyramid             loadTasksSetting only: per robot is this engine's extension
 *                 [18]     noContactMotionTask.tolerance                         likewise
 *                 [19..24] torque limits per leg joint; nj / 2 entries are used  likewise
 *                 [25..31] reserved, written as 0
 *               Every row starts as what loadTasksSetting reads from task.info (the reference's dynamic_reconfigure server additionally calls the
 *               callback once at start-up with the defaults of its .cfg, which then override task.info from the first tick; this engine
 *               keeps task.info until the caller sets a row - the Python mirror offers those defaults as a preset).  The working-set budget (nWSR 20)
 *               stays a constant of the handle.
 *               bpmpc_wbc_get_params: row[32] = the task.info values (robot < 0) or the robot's current row; synchronises.
 *               bpmpc_wbc_set_params: the rows of the robots with mask[b] != 0 (mask NULL: every robot below `batch`) are replaced by rows[b]
 *               (n_rows == batch) or by rows[0] (n_rows == 1); robots outside the mask and at or beyond `batch` keep theirs.  Host arrays are
 *               validated - every used entry finite; gains, weights, friction and limits not negative (the tolerance may have any sign) - and a
 *               bad value returns BPMPC_ERR_INVALID_ARGUMENT, names the entry in bpmpc_last_error() and changes nothing; the call synchronises.
 *               inputs_on_device != 0: mask and rows are device pointers (e.g. a [batch, 32] tensor), nothing is validated and the call only
 *               enqueues on the WBC handle's stream, ordered like bpmpc_wbc_restart: a later controller tick on another stream waits for it.
 *               bpmpc_wbc_reset_params: every row back to the task.info values.
 *               batch > max_batch: BPMPC_ERR_CAPACITY.  A restart keeps the parameters, as starting() does: bpmpc_wbc_reset, bpmpc_wbc_restart and
 *               bpmpc_controller_restart do not touch the rows.
 *   controller  joint gains kp[nj], kd[nj] per robot (0 after create; restarts and bpmpc_controller_reset keep them), set by
 *               bpmpc_controller_set_joint_gains (kp, kd: [n_rows][nj]; mask, n_rows, host / device as bpmpc_wbc_set_params; host values must be
 *               finite and not negative; on the solver's stream).  k_tick_commands additionally forms the torque with which the reference's
 *               hardware layer consumes the five-tuple (bipedal_gazebo/src/BipedalHWSim.cpp:174-175),
 *                 joint_torque[b][j] = kp_j (posDes_j - q_j) + kd_j (velDes_j - v_j) + tau_j     (q, v: the joint entries of the tick's rbd)
 *               which with zero gains is the WBC torque bit for bit.  bpmpc_controller_joint_outputs: every argument nullable; host_*
 *               [batch*nj] receive the last tick's joint_torque and the current gains and make the call synchronise; dev_* receive the handle's
 *               buffers (leading dimension the WBC's max_batch, like bpmpc_controller_device_outputs).
 * Not reproduced: per-robot MPC cost weights, UpperJointController (the MPC models carry no upper-body joints).  (The reference's server has no
 * MPC weights to reproduce; per-problem weights of the solver handle are this engine's own extension, "Per-problem cost weights" below, and no
 * part of this interface.)  The SafetyChecker limits and
 * InitialJointController are the supervisor's ("Supervisor" below).
 * ------------------------------------------------------------------------------------------------------------- */
#define BPMPC_WBC_PARAM_STRIDE 32
#define BPMPC_WBC_PARAM_BASE_KP 0
#define BPMPC_WBC_PARAM_BASE_KD 6
#define BPMPC_WBC_PARAM_SWING_KP 12
#define BPMPC_WBC_PARAM_SWING_KD 13
#define BPMPC_WBC_PARAM_WEIGHT_SWING_LEG 14
#define BPMPC_WBC_PARAM_WEIGHT_BASE_ACCEL 15
#define BPMPC_WBC_PARAM_WEIGHT_CONTACT_FORCE 16
#define BPMPC_WBC_PARAM_FRICTION 17
#define BPMPC_WBC_PARAM_CONTACT_TOLERANCE 18
#define BPMPC_WBC_PARAM_TORQUE_LIMITS 19
#define BPMPC_WBC_PARAM_RESERVED 25
int bpmpc_wbc_get_params(const bpmpc_wbc* wbc, int robot, double* row);
int bpmpc_wbc_set_params(bpmpc_wbc* wbc, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device);
int bpmpc_wbc_reset_params(bpmpc_wbc* wbc);
int bpmpc_controller_set_joint_gains(bpmpc_controller* controller, int batch, const int* mask, const double* kp, const double* kd, int n_rows,
                                     int inputs_on_device);
int bpmpc_controller_joint_outputs(bpmpc_controller* controller, int batch, double* host_torque, double* host_kp, double* host_kd,
                                   double** dev_torque, double** dev_kp, double** dev_kd);

/* ---------------------------------------------------------------------------------------------------------------
 * Per-problem cost weights: every problem of an SQP solver handle solves under a weight row of its own, settable at run time like the rows above
 * (this engine's extension: the reference fixes Q and R when BipedalRobotInterface reads task.info).  One handle, one setup and one run then
 * cover a sweep of Q / R candidates or a fleet whose robots weigh tracking differently.
 *   row         BPMPC_SOLVER_WEIGHT_STRIDE = 2 * 24 * 24 doubles, dense and row major: Q (nx x nx, stride nx) followed by R (nu x nu, stride nu) -
 *               the blocks bpmpc_model_get "Q" / "R" return; nx*nx + nu*nu entries are used, the rest reads 0.  The start row is the model's Q, R.
 *   set         bpmpc_solver_set_weights: the rows of the problems with mask[b] != 0 (mask NULL: every problem) become rows[b] (n_rows == batch) or
 *               rows[0] (n_rows == 1); batch must equal the batch of the last setup.  Every bpmpc_solver_run enqueued after the call solves under
 *               the new rows; no new setup is needed (the weights enter neither the grids nor the references).  With host arrays the call
 *               synchronises; inputs_on_device != 0: mask and rows are device pointers and the call only enqueues on the solver's stream (the
 *               first set on a handle also allocates the table: 2 * max_batch rows).  From the first set on, the handle launches the
 *               per-problem kernels for EVERY problem of the batch (lineariser, line-search trials, change of variables: k_weights.hip; kernel
 *               classes "linearize_w", "linesearch_w", "project_w" of bpmpc_solver_kernel_time), also for rows equal to the model's.
 *   check       a host row is refused with BPMPC_ERR_INVALID_ARGUMENT - the entry and the reason in bpmpc_last_error(), nothing written, nothing
 *               enqueued, the kernels unchanged - when an entry is not finite; when Q or R is not symmetric (relative 1e-9); when it has a non-zero
 *               where the model's Q or R has a structural zero (the PATTERN rule: the hot kernels and the solver's choice of kernels are built on
 *               the model's pattern - non-zero lists, a diagonal Q, R without force / joint-velocity cross terms - and stay valid for every row
 *               this way; zeroing an entry the model has is allowed); when a diagonal Q has a negative entry (a model whose Q is not diagonal: when
 *               Q is not positive semidefinite); when R is not positive definite (pivoted Cholesky on the host; a model whose own R is only positive
 *               semidefinite - six joints per leg: J^T R_v J has rank 10 - asks its rows for semidefiniteness).  bpmpc_solver_check_weights runs this
 *               check alone.  Device rows are NOT checked: a device row outside these rules gives undefined results for its own problem only.
 *   get / reset bpmpc_solver_get_weights: row[BPMPC_SOLVER_WEIGHT_STRIDE] = the start row (robot < 0) or the problem's current row; synchronises.
 *               bpmpc_solver_reset_weights: every row back to the start row, and the handle back to the kernels it launched before any row was
 *               set.  bpmpc_solver_reset and the restarts keep the rows.
 *   compose     bpmpc_model_compose_weights (host only, no device): a row from the two matrices as task.info spells them - Q_task nx x nx as
 *               given, R_task 24 x 24 (contact forces, then contact-point velocities) mapped as R = blkdiag(R_F, J^T R_v J) with the contact
 *               Jacobians at initialState, by the function the model's own R is built with (BipedalRobotInterface.cpp:239-271): the Q and R of
 *               the task file reproduce bpmpc_model_get "Q" / "R" bit for bit.
 * BPMPC_ERR_UNSUPPORTED: the DDP solver (its cost of recorded points and its ILQR lineariser stay on the model's weights) and
 * settings.reference_kernels (the lane-emulation bodies read the model's Q and R), like reg_prim and bpmpc_solver_restart on those paths.
 * Not per problem: the kinematic and inertial constants of the MPC model.  (The cone parameters are: "Per-problem cone parameters" below.)
 * ------------------------------------------------------------------------------------------------------------- */
#define BPMPC_SOLVER_WEIGHT_STRIDE (2 * 24 * 24)
int bpmpc_solver_set_weights(bpmpc_solver* solver, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device);
int bpmpc_solver_get_weights(bpmpc_solver* solver, int robot, double* row);
int bpmpc_solver_reset_weights(bpmpc_solver* solver);
int bpmpc_solver_check_weights(const bpmpc_solver* solver, const double* row);
int bpmpc_model_compose_weights(const bpmpc_model* model, const double* Q_task, const double* R_task, double* row_out);

/* ---------------------------------------------------------------------------------------------------------------
 * Per-problem cone parameters: every problem of an SQP solver handle solves under friction-cone parameters of its own, settable at run time like
 * the weight rows above (this engine's extension: the reference fixes them when BipedalRobotInterface reads task.info).  One handle, one setup
 * and one run then cover a fleet that stands on different ground, or a sweep of the barrier's mu / delta next to one of Q / R.
 *   row         BPMPC_SOLVER_CONE_STRIDE = 8 doubles: the six values of bpmpc_model_get "cone" in that order (BPMPC_SOLVER_CONE_*: friction
 *               coefficient, regularisation, gripper force, Hessian diagonal shift, barrier mu, barrier delta), then two entries that must be 0.
 *               The start row is what the solver's kernels read of the model: for a model created with the hard friction cone
 *               (bpmpc_model_create_ex) entries 4 and 5 are sqp.inequalityConstraintMu / Delta and entry 3 is 0.
 *   set         bpmpc_solver_set_cone_params: the contract of bpmpc_solver_set_weights - the rows of the problems with mask[b] != 0 (mask NULL:
 *               every problem) become rows[b] (n_rows == batch) or rows[0] (n_rows == 1); batch must equal the batch of the last setup.  Every
 *               bpmpc_solver_run enqueued after the call solves under the new rows; no new setup is needed.  With host arrays the call
 *               synchronises; inputs_on_device != 0: mask and rows are device pointers and the call only enqueues on the solver's stream.  Host
 *               rows are checked before anything is allocated or enqueued; device rows are NOT checked.
 *   kernels     ONE per-problem kernel family serves the weight rows and the cone rows (k_weights.hip; kernel classes "linearize_w",
 *               "linesearch_w", "project_w").  The handle launches it for every problem from the first bpmpc_solver_set_weights OR
 *               bpmpc_solver_set_cone_params on, and returns to the default kernels when neither table has had a row set since its own reset.
 *               The first set of either allocates BOTH tables (2 * max_batch rows each); the one that was never set holds the model's row.
 *   check       bpmpc_model_check_cone_params (host only, no device): the check of a host row.  BPMPC_ERR_INVALID_ARGUMENT, the entry and the
 *               reason in bpmpc_last_error(), for: an entry that is not finite; friction <= 0; regularisation <= 0 (sqrt(Fx^2 + Fy^2 +
 *               regularisation) is a divisor at zero force); gripper force < 0; shift < 0; shift != 0 on a hard-cone model; mu <= 0; delta <= 0;
 *               entry 6 or 7 != 0.  A refused set writes nothing, enqueues nothing and leaves the kernels unchanged.
 *   get / reset bpmpc_solver_get_cone_params: row[BPMPC_SOLVER_CONE_STRIDE] = the start row (robot < 0, or a handle that never had a row set) or
 *               the problem's current row; synchronises.  bpmpc_solver_reset_cone_params: every row back to the start row.
 *               bpmpc_solver_reset and the restarts keep the rows.
 * BPMPC_ERR_UNSUPPORTED: the DDP solver and settings.reference_kernels, for the reasons of the weight rows.
 * Not per problem: pos_gain and the robot's mass (the model's in every kernel), the WBC's and the plant's friction (rows of their own handles).
 * ------------------------------------------------------------------------------------------------------------- */
#define BPMPC_SOLVER_CONE_STRIDE 8
#define BPMPC_SOLVER_CONE_FRICTION 0
#define BPMPC_SOLVER_CONE_REGULARIZATION 1
#define BPMPC_SOLVER_CONE_GRIPPER_FORCE 2
#define BPMPC_SOLVER_CONE_HESSIAN_SHIFT 3
#define BPMPC_SOLVER_CONE_BARRIER_MU 4
#define BPMPC_SOLVER_CONE_BARRIER_DELTA 5
#define BPMPC_SOLVER_CONE_RESERVED 6
int bpmpc_solver_set_cone_params(bpmpc_solver* solver, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device);
int bpmpc_solver_get_cone_params(bpmpc_solver* solver, int robot, double* row);
int bpmpc_solver_reset_cone_params(bpmpc_solver* solver);
int bpmpc_model_check_cone_params(const bpmpc_model* model, const double* row);

/* ---------------------------------------------------------------------------------------------------------------
 * Value function: the cost-to-go of the QP an SQP solver handle has just solved, per node of every problem and on query (this engine's
 * extension; what SolverBase::getValueFunction asks for, and the one SolverBase query a multiple-shooting SQP can answer exactly).
 *   definition  Take the QP of the LAST SWEPT SQP iteration of problem b in the unprojected LQ model - A, B, b, Q, R, P, q, r, c per node as
 *               bpmpc_solver_read names them, the cost already times dt, event nodes identity jumps (the stored b) without cost.  The sweep's
 *               optimal feasible policy is du = K_k dx + kappa_k with kappa_k = du_k - K_k dx_k from the stored K, dx, du; the equality
 *               constraints live inside K, so the cost-to-go of that policy is the QP's value function for EVERY dx, not only on the optimal
 *               trajectory:
 *                   V_k(dx) = v_k + s_k' dx + dx' S_k dx / 2        k = 0 .. n_nodes[b],   V_n = 0 (there is no final cost)
 *                   Acl = A + B K     bcl = b + B kappa     Qcl = Q + K'(R K + P) + P'K     qcl = q + K'r + (P' + K'R) kappa
 *                   ccl = c + r'kappa + kappa'R kappa / 2
 *                   S_k = Qcl + Acl' S+ Acl     s_k = qcl + Acl'(s+ + S+ bcl)     v_k = ccl + v+ + s+'bcl + bcl' S+ bcl / 2
 *               S_k is stored symmetrised as computed, (S + S') / 2.  dx is measured from the EXPANSION POINT x_lin,k: the iterate the model was
 *               linearised at, i.e. x before the line search of that iteration moved it; the handle keeps its own copy.  Nothing is assumed of
 *               the sparsity of Q, R or P: the kernels read what the lineariser wrote (hard-cone model, per-problem weights included).
 *   enable      bpmpc_solver_enable_value_function(on != 0) allocates the buffers (once, at the first such call) and from then on every
 *               bpmpc_solver_run computes the value function behind the backward pass of every iteration (behind the last chunk with
 *               pipeline_chunks > 1) and before that iteration's line search touches x: two kernels on the solver's stream (k_value.hip; kernel
 *               classes "value_terms", "value_sweep" of bpmpc_solver_kernel_time), nothing read back or waited for.  Such a handle linearises in
 *               MATERIALISED form: a handle created with materialize_lq = 0 switches as bpmpc_solver_set_materialize(solver, 1) would - the
 *               solution stays the same bits, which is the contract of the two modes - and a bpmpc_solver_set_materialize while the feature is
 *               on is remembered, not applied.  on == 0 stops the launches, puts the handle's own materialise setting back and keeps the
 *               buffers (they describe the last run that computed them).  A problem the sweep skipped (converged earlier) keeps the value
 *               function of its last sweep.  A handle that never enables the feature launches and allocates nothing for it.
 *               BPMPC_ERR_UNSUPPORTED: the DDP solver.  BPMPC_ERR_INVALID_ARGUMENT: settings.reference_kernels without return_gains.
 *   fetch       bpmpc_solver_value_function (synchronises; every pointer nullable): S[batch][max_nodes+1][nx*nx] full storage, row major;
 *               s[batch][max_nodes+1][nx]; v[batch][max_nodes+1]; x_lin[batch][max_nodes+1][nx]; status[batch]: 0 = no value function yet,
 *               1 = valid, 2 = the sweep of that problem failed (bpmpc_stats.status == 2) and its rows are left as they were.  Entries beyond
 *               n_nodes[b] are never written.  bpmpc_solver_device_value_function: the device pointers of the same arrays, same layouts, no
 *               synchronisation (valid for the handle's life once enabled).
 *   query       bpmpc_solver_evaluate_value: t[batch], x[batch][nx] -> f[batch], dfdx[batch][nx], dfdxx[batch][nx*nx] (nullable).  Per problem t
 *               is clamped to the solution's time span, (i, a) = LinearInterpolation::timeSegment as bpmpc_solver_evaluate_policy uses it for
 *               the states (an event time, stored twice, belongs to the interval that ends there); S, s, v, x_lin are interpolated with a and
 *               re-centred with delta = x - x_lin(t): f = v + s'delta + delta'S delta / 2, dfdx = s + S delta, dfdxx = S.  inputs_on_device != 0:
 *               all five are device pointers and the call only enqueues on the solver's stream; otherwise it synchronises.  The rows are
 *               evaluated as they are: look at status for a problem whose sweep failed.  BPMPC_ERR_INVALID_ARGUMENT: the feature not enabled, no
 *               completed run since the last setup, a batch other than that setup's; BPMPC_ERR_UNSUPPORTED: the DDP solver.
 *   stage       bpmpc_solver_stage(solver, "value") runs the two kernels on the current buffers (stage-wise parity tests).
 * setup_from_previous, the restarts, the policy buffer and sharding are not involved: the buffers describe the last run until the next one.
 * ------------------------------------------------------------------------------------------------------------- */
int bpmpc_solver_enable_value_function(bpmpc_solver* solver, int on);
int bpmpc_solver_value_function(bpmpc_solver* solver, double* S, double* s, double* v, double* x_lin, int* status);
int bpmpc_solver_device_value_function(bpmpc_solver* solver, double** S_dev, double** s_dev, double** v_dev, double** x_lin_dev, int** status_dev);
int bpmpc_solver_evaluate_value(bpmpc_solver* solver, int batch, const double* t, const double* x, int inputs_on_device, double* f, double* dfdx,
                                double* dfdxx);

/* ---------------------------------------------------------------------------------------------------------------
 * Dual solution: the costates of the dynamics and the Lagrange multipliers of the state-input equality rows of the QP an SQP solver handle has just
 * solved, per node of every problem and on query, with two residuals that certify the step and the gains without any oracle (this engine's
 * extension; what SolverBase::getStateInputEqualityConstraintLagrangian asks for).
 *   definition  The QP of the LAST SWEPT SQP iteration of problem b in the unprojected LQ model, as "Value function" above takes it.  Lagrangian:
 *                   cost + sum_k lambda_{k+1}'(A dx_k + B du_k + b - dx_{k+1}) + sum_k nu_k'(C dx_k + D du_k + e)
 *               with the rows of C, D, e as bpmpc_solver_read returns them: nc[k] rows in registration order (zero force, zero velocity, normal
 *               velocity per contact point), 16 slots.  With S, s of the value function, and + for node k + 1:
 *                   lambda_k = s_k + S_k dx_k        k = 0 .. n_nodes[b],   lambda_n = 0
 *               and per intermediate node, event nodes excepted, under the sweep's policy du = K dx + kappa:
 *                   Hux = P + R K + B'S+ Acl     g0 = r + R kappa + B'(s+ + S+ bcl)     g_u(dx) = Hux dx + g0
 *               (the input gradient of the Hamiltonian as a function of dx), and
 *                   [N | nu0] = -pinv(D') [Hux | g0]        nu_k = nu0 + N dx_k
 *               D is NEVER of full row rank while a foot stands: the two contact points of a rigid foot cannot move along the line between them
 *               (single stance: 14 rows of rank 13, double stance: 12 of rank 10; only a flight node's 16 rows have rank 16).  nu is therefore
 *               not unique, and this is the MINIMUM-NORM solution, which is: the component of every column of [N | nu0] in null(D') is zero.
 *               Singular values of D below 1e-6 of the largest count as zero - equivalently eigenvalues of D D' below 1e-12 of the largest; on
 *               these robots the smallest kept singular value is above 0.05 of the largest and the dropped ones are rounding noise.
 *               nu belongs to the QP, whose cost is already times dt (divide by the node's dt for a multiplier of the continuous-time cost).
 *               With the hard-cone model the cone inequalities are in the cost, as the SQP treats them: they have no multiplier here.
 *               Certificates: residual_k = |g_u(dx_k) + D'nu_k|_inf is zero exactly when the step (dx, du) the sweep returned is stationary in
 *               du on the constraint set - the Riccati sweep, the constraint elimination and the change of variables together returned the QP's
 *               minimiser; gain_residual_k = max |Hux + D'N| says the same of the gains K for every dx.
 *               CAVEAT, stationarity in x: lambda_k = q + Q dx + P'du + A'lambda+ + C'nu holds at nodes where D has full row rank only.  At a
 *               rank-deficient node off convergence the linearised redundant row is inconsistent in its state part, the elimination drops it,
 *               and the QP that was solved does not contain it; what always holds is lambda_k = q + Q dx + P'du + A'lambda+ + K'g_u(dx_k).
 *   enable      bpmpc_solver_enable_dual_solution(on != 0) allocates the buffers (once, at the first such call), turns the value function on as
 *               bpmpc_solver_enable_value_function(solver, 1) would and keeps it on while this is on (a bpmpc_solver_enable_value_function(solver,
 *               0) in between is remembered and applies once this is off).  From then on two more kernels follow the value function's behind
 *               every backward pass (k_dual.hip: k_dual_node, one wave per node - kernel class "dual" of bpmpc_solver_kernel_time -, and
 *               k_dual_summary).  on == 0 stops the launches and keeps the buffers.  A problem the sweep skipped keeps its rows.  A handle that
 *               never enables the feature launches and allocates nothing for it.  Memory: per node 16 nx doubles of nu_gain (at max_batch 4096,
 *               max_nodes 100, nx = 22: 1.2 GB) and about 37 + nx more.  BPMPC_ERR_UNSUPPORTED: the DDP solver.
 *   fetch       bpmpc_solver_dual_solution (synchronises; every pointer nullable): lambda[batch][max_nodes+1][nx]; nu, nu0[batch][max_nodes][16];
 *               nu_gain[batch][max_nodes][16][nx]; residual, gain_residual[batch][max_nodes]; summary[batch][6]: the maxima over the problem's
 *               nodes of residual, |g_u(dx_k)|_inf, gain_residual, |Hux|, |nu|, |lambda|; status[batch] as the value function's: 0 none yet,
 *               1 valid, 2 the sweep of that problem failed and its rows are left as they were.  Rows at and beyond nc[k] are exact zeros; at an
 *               event node nu, nu0 and nu_gain are zero.  Nodes beyond n_nodes[b] are never written.  bpmpc_solver_device_dual_solution: the
 *               device pointers of the same arrays, no synchronisation.
 *   query       bpmpc_solver_evaluate_dual: t[batch], x[batch][nx] -> lambda[batch][nx], nu[batch][16], rows[batch].  (i, a) of the time segment
 *               as bpmpc_solver_evaluate_value; multipliers belong to intervals: the rows of node i are taken (an event time belongs to the
 *               interval that ends there; behind the last node: node n - 1), nu = nu0_i + N_i delta with delta = x - x_lin(t) interpolated as
 *               in the value query, rows = nc_i, and lambda is that query's dfdx.  inputs_on_device, refusals: as bpmpc_solver_evaluate_value.
 *   stage       bpmpc_solver_stage(solver, "dual") runs the two kernels on the current buffers, behind a "value" stage.
 * ------------------------------------------------------------------------------------------------------------- */
int bpmpc_solver_enable_dual_solution(bpmpc_solver* solver, int on);
int bpmpc_solver_dual_solution(bpmpc_solver* solver, double* lambda, double* nu, double* nu0, double* nu_gain, double* residual, double* gain_residual,
                               double* summary, int* status);
int bpmpc_solver_device_dual_solution(bpmpc_solver* solver, double** lambda_dev, double** nu_dev, double** nu0_dev, double** nu_gain_dev,
                                      double** residual_dev, double** gain_residual_dev, double** summary_dev, int** status_dev);
int bpmpc_solver_evaluate_dual(bpmpc_solver* solver, int batch, const double* t, const double* x, int inputs_on_device, double* lambda, double* nu,
                               int* rows);

/* ---------------------------------------------------------------------------------------------------------------
 * State estimation = BipedalController::updateStateEstimation (bipedal_controllers/src/BipedalController.cpp:188, :360-405) for a BATCH of robots:
 * what a simulator or a robot delivers - IMU quaternion, body-frame angular velocity and linear acceleration, joint encoders, contact flags -
 * becomes the rbd of bpmpc_controller_tick, [zyx, position, joints, angular velocity (world), linear velocity, joint velocities], on the device.
 *   front end, both kinds (bipedal_estimation/src/StateEstimateBase.cpp:34-63, StateEstimateBase.h:70-79): the joints go into their slots unchanged;
 *     zyx = quatToZyx(quat) with its one-sided clamp asin(min(-2 (x z - w y), .99999)); angular velocity (world) = E(zyx) thetadot, thetadot the
 *     ZYX Euler rates of the local angular velocity (R(zyx) w_local = E(zyx) thetadot).  zyxOffset_ is zero in the reference and is not reproduced.
 *   BPMPC_ESTIMATOR_FROM_TOPIC (FromTopicEstimate.cpp:28-47, the estimator the reference constructs, :354-358): zyx = quatToZyx(odom_quat), angular
 *     velocity = odom_ang_vel as given, position = odom_pos, linear velocity = odom_lin_vel; the IMU pointers may be NULL.
 *   BPMPC_ESTIMATOR_KALMAN: KalmanFilterEstimate.  The reference DECLARES it (LinearKalmanFilter.h: seven noise settings, a_, b_, c_, q_, p_, r_,
 *     xHat_, ps_, vs_) and does not implement it: src/LinearKalmanFilter.cpp is an empty file.  What runs here is the linear Kalman filter of the
 *     project that header cites (qiayuanl/legged_control), recalled and unpinned; this comment is its specification.
 *     Sizes: 4 contact points, state n = 18: x_hat = [p (3), v (3), foot positions (12)], observations m = 28.  After create / reset x_hat = 0, P = 100 I.
 *     C (28 x 18), contact i: rows 3i..3i+2 = [I3 at columns 0..2, -I3 at columns 6+3i..], rows 12+3i.. = [I3 at columns 3..5], row 24+i = a single 1
 *     at column 6+3i+2.  One update with dt = period:
 *       1. A = I with A[0:3,3:6] = dt I; B (18 x 3): rows 0..2 = dt^2/2 I, rows 3..5 = dt I
 *       2. Q diagonal: dt/20 imuProcessNoisePosition (0..2), dt 9.81/20 imuProcessNoiseVelocity (3..5), dt footProcessNoisePosition (6..17); the foot
 *          block of a contact whose flag is 0 is multiplied by 100
 *       3. R diagonal: footSensorNoisePosition (0..11), footSensorNoiseVelocity (12..23), footHeightSensorNoise (24..27); the velocity block and the
 *          height entry of a contact whose flag is 0 are multiplied by 100, the position block never
 *       4. kinematics with the base at the origin, q = [0, zyx, joints], v = [0, thetadot, joint_vel]: contact positions p_i and velocities v_i;
 *          ps_i = -p_i with footRadius added to its z, vs_i = -v_i, y = [ps, vs, feet_heights]
 *       5. accel = R(zyx) linear_accel_local + (0, 0, -9.81); x- = A x_hat + B accel; P- = A P A' + Q
 *       6. S = C P- C' + R; x_hat = x- + P- C' S^-1 (y - C x-); P = (I - P- C' S^-1 C) P-; P = (P + P') / 2
 *       7. if det P[0:2,0:2] > 1e-6: P[0:2,2:] = 0, P[2:,0:2] = 0, P[0:2,0:2] /= 10, reported as xy_reset[b] = 1 (else 0)
 *       8. rbd position = x_hat[0:3], linear velocity = x_hat[3:6]
 *     S is symmetric positive definite (R > 0); k_estimate solves with a Gauss-Jordan elimination without pivoting.
 *     Not reproduced: the odometry / tf publishing and updateFromTopic of the cited filter; getMode() (stanceLeg2ModeNumber).
 *   contact flags (Kalman kind): exactly one of `contact` ([batch*4], non-zero = closed) and `mode` ([batch], mode number 0..3 expanded by
 *     modeNumber2StanceLeg, MotionPhaseDefinition.h:57-76; e.g. the planned_mode device output of the last tick, which is what the reference passes
 *     today, :377) is non-NULL, otherwise BPMPC_ERR_INVALID_ARGUMENT.  Host modes outside 0..3 are refused (BPMPC_ERR_INVALID_ARGUMENT); device
 *     modes cannot be looked at without a synchronisation and are not: a device value outside 0..3 counts as mode 0, all four contacts open.
 *   settings: a parameter row of BPMPC_EST_PARAM_STRIDE doubles per robot, [footRadius, imuProcessNoisePosition, imuProcessNoiseVelocity,
 *     footProcessNoisePosition, footSensorNoisePosition, footSensorNoiseVelocity, footHeightSensorNoise, reserved 0].  Every row starts as the keys
 *     kalmanFilter.<name> of task_info_path; an absent key keeps the default of LinearKalmanFilter.h:45-51 (0.02, 0.02, 0.02, 0.002, 0.005, 0.1,
 *     0.01: loadPtreeValue semantics), a NULL path gives the defaults.  bpmpc_estimator_get_params / set_params / reset_params have the shapes, masks,
 *     n_rows and host / device semantics of bpmpc_wbc_get_params / set_params / reset_params; host rows are validated - every entry finite and not
 *     negative, the three sensor noises strictly positive - and a bad entry is named in bpmpc_last_error() and changes nothing.
 *   streams: the handle has its own stream.  inputs_on_device != 0: every non-NULL member of bpmpc_sensor_inputs (masks, rows, states likewise) is
 *     a device pointer and the call only enqueues; host arrays are copied first.  bpmpc_estimator_update with host_rbd receives rbd[batch*2*(6+nj)]
 *     and synchronises; with NULL it is only enqueued.  bpmpc_controller_tick_estimated is bpmpc_controller_tick with rbd = the estimator's device
 *     buffer (t: host or device by inputs_on_device): the solver's stream first waits for the estimator's pending update and the estimator's stream
 *     then waits for the tick, so a caller with device inputs never synchronises by hand.  Its outputs are the bits of bpmpc_estimator_update
 *     followed by bpmpc_controller_tick(rbd = dev_out.rbd, inputs_on_device = 1).  Its batch must be the batch of the estimator's last update
 *     (else BPMPC_ERR_INVALID_ARGUMENT, also before the first update: the other rows of rbd hold no estimate), besides what bpmpc_controller_tick
 *     asks of it; its period is accepted and not used, as that of bpmpc_controller_tick (the filter's dt is the period of the update).
 *   state: bpmpc_estimator_reset puts the robots of mask (NULL: every robot below batch) back to x_hat = 0, P = 100 I; bpmpc_estimator_set_state
 *     writes x_hat[batch*18] and, unless NULL, cov[batch*18*18] of the robots of mask (NULL: all; host values must be finite);
 *     bpmpc_estimator_get_state copies them to the host (either pointer nullable; synchronises).  Robots outside a mask do not change by one
 *     bit.  bpmpc_controller_restart does not touch the estimator.  bpmpc_estimator_device_outputs: rbd, x_hat, cov, xy_reset where they live
 *     (leading dimension max_batch).
 * Null handles and required pointers: BPMPC_ERR_INVALID_ARGUMENT ("null" in bpmpc_last_error()); batch > max_batch: BPMPC_ERR_CAPACITY.
 * ------------------------------------------------------------------------------------------------------------- */
enum { BPMPC_ESTIMATOR_FROM_TOPIC = 0, BPMPC_ESTIMATOR_KALMAN = 1 };
#define BPMPC_EST_PARAM_STRIDE 8
typedef struct bpmpc_estimator bpmpc_estimator;
typedef struct {
  const double *joint_pos, *joint_vel;                  /* [batch*nj] */
  const double *quat;                                   /* [batch*4] x y z w (the order of imuSensorHandle_.getOrientation(), :379-381) */
  const double *angular_vel_local, *linear_accel_local; /* [batch*3] IMU frame = base frame */
  const int *contact;                                   /* [batch*4] nullable: contact flags of the four contact points */
  const int *mode;                                      /* [batch] nullable: mode number 0..3 */
  const double *feet_heights;                           /* [batch*4] nullable: 0 (flat ground) */
  const double *odom_pos, *odom_quat, *odom_lin_vel, *odom_ang_vel;   /* FROM_TOPIC only: [batch*3], [batch*4] x y z w, [batch*3], [batch*3] */
} bpmpc_sensor_inputs;
typedef struct { double *rbd, *x_hat, *cov; int *xy_reset; } bpmpc_estimator_outputs;
int bpmpc_estimator_create(const bpmpc_model* model, const char* task_info_path, int kind, int device, int max_batch, bpmpc_estimator** out);
void bpmpc_estimator_destroy(bpmpc_estimator* estimator);
int bpmpc_estimator_update(bpmpc_estimator* estimator, int batch, const bpmpc_sensor_inputs* inputs, int inputs_on_device, double period,
                           double* host_rbd);
int bpmpc_estimator_device_outputs(bpmpc_estimator* estimator, bpmpc_estimator_outputs* dev_out);
int bpmpc_estimator_reset(bpmpc_estimator* estimator, int batch, const int* mask, int inputs_on_device);
int bpmpc_estimator_get_state(bpmpc_estimator* estimator, int batch, double* x_hat, double* cov);
int bpmpc_estimator_set_state(bpmpc_estimator* estimator, int batch, const int* mask, const double* x_hat, const double* cov, int inputs_on_device);
int bpmpc_estimator_get_params(const bpmpc_estimator* estimator, int robot, double* row);
int bpmpc_estimator_set_params(bpmpc_estimator* estimator, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device);
int bpmpc_estimator_reset_params(bpmpc_estimator* estimator);
/* Two helpers beside the handle, host only: they are the settings ingest of bpmpc_estimator_create and the row validation of
 * bpmpc_estimator_set_params as functions of their own, so that a configuration can be checked - and both are tested - on a machine without a
 * device, where no handle can be created.  load_params: row[8] = what every row of a handle created with this task_info_path (nullable) starts
 * as.  check_params: rows[n_rows*8] as set_params validates host rows; BPMPC_ERR_INVALID_ARGUMENT names the entry. */
int bpmpc_estimator_load_params(const char* task_info_path, double* row);
int bpmpc_estimator_check_params(const double* rows, int n_rows);
int bpmpc_controller_tick_estimated(bpmpc_controller* controller, bpmpc_estimator* estimator, int batch, const double* t, int inputs_on_device,
                                    double period, const bpmpc_tick_outputs* host_out);

/* ---------------------------------------------------------------------------------------------------------------
 * Plant = a rigid-body simulation of a BATCH of robots on the device: joint commands in, the sensors of bpmpc_sensor_inputs out, so that the
 * loop sensors -> bpmpc_estimator_update -> bpmpc_controller_tick_estimated -> joint commands closes without leaving the device.  The reference
 * closes its loop with MuJoCo or Gazebo (bipedal_mujoco, bipedal_gazebo/src/BipedalHWSim.cpp).  This plant imitates neither: it is this engine's own
 * model, this comment is its specification, and it is nowhere pinned against the reference's simulators.  Its joints are ideal until a joint
 * row says otherwise (see "joints": armature, damping, friction and end stops per robot).  It has no
 * self-collision and no torsional friction about the contact normal.  Its contacts stick and slip (a tangential anchor spring with a Coulomb cap)
 * for the robots whose tangential stiffness kt is set above 0; with kt = 0, the default, friction is the regularised Coulomb damper alone, under
 * which a loaded foot creeps.
 *   state per robot: q[6+nj] = [position, zyx, joints], v[6+nj] = dq/dt (Euler rates, not angular velocity: the coordinates of the WBC), so
 *     integrating q is a plain sum.  One control step of length `period` is `substeps` equal substeps of h = period / substeps.  One substep:
 *       1. rigid-body pass at (q, v) with gravity: M, nle (as the WBC's), the four contact points p_i, the stacked contact Jacobian J (12 x nv),
 *          the point velocities c_i = J_i v
 *       2. contact point i with ground height g_i (feet_heights, NULL: 0) and penetration d_i = g_i - p_i,z: open unless d_i > 0.  Closed:
 *          spring force f_i = (0, 0, kn d_i); normal damping cn_i = cn min(1, d_i / d0); start-of-step normal force
 *          n_i = max(0, kn d_i - cn_i c_i,z); tangential damping ct_i = mu n_i / sqrt(c_i,x^2 + c_i,y^2 + v_eps^2) (a regularised Coulomb law);
 *          D_i = diag(ct_i, ct_i, cn_i).  Open: f_i = 0, D_i = 0, n_i = 0.
 *          Stick-slip, for a robot with kt > 0 (a robot with kt = 0 runs the arithmetic above and nothing else; its flags stay 0).  Each point
 *          carries an anchor a_i (world x, y) and a flag anchored_i; p is the point's xy at the start-of-substep q.  Closed point:
 *            a. not anchored: a_i = p, anchored_i = 1
 *            b. s = a_i - p, phi = kt |s|, cap = mu n_i
 *            c. phi > cap: the point slips: a_i = p + s (cap / phi) (a_i = p when cap = 0), s = a_i - p again, stick = 0; otherwise stick = 1
 *            d. the spring force gains its tangential part: f_i = (kt s_x, kt s_y, kn d_i)
 *            e. the Coulomb damper gets the friction the spring has not used: ct_i = (cap - kt |s|) / sqrt(c_i,x^2 + c_i,y^2 + v_eps^2) when
 *               sticking, exactly 0 when slipping
 *            f. the spring is linearly implicit while sticking: D_i = diag(ct_i + stick h kt, ct_i + stick h kt, cn_i)
 *          Open point: anchored_i = 0.  At the start-of-step linearisation the tangential force never exceeds mu n_i.  Anchors are evaluated at
 *          the start of each substep only; after a step they hold what its last substep left.
 *       3. joint torque tau_j = kp_j (posDes_j - q_j) + tau_ff,j, clamped to +- the torque limit of its leg joint when that limit is > 0; the
 *          kd term kd_j (velDes_j - v+_j) is implicit and not clamped
 *       4. v+ solves (M + h J'DJ + h diag(0_6, kd)) v+ = M v + h (S'(tau + kd velDes) - nle + J'f + w_ext); S selects the joints, w_ext is the
 *          external force base_force (world frame, NULL: 0) on the base origin, acting on coordinates 0..2.  The matrix is symmetric positive
 *          definite; k_plant_step factors it by a Cholesky factorisation without pivoting.
 *       5. q+ = q + h v+
 *     All damping is linearly implicit, the normal contact spring is explicit, the tangential spring is linearly implicit while it sticks.
 *   outputs, written after the last substep from (q+, v+), in the layouts of bpmpc_sensor_inputs: joint_pos, joint_vel; quat (x y z w) of R(zyx);
 *     angular_vel_local = R' E(zyx) thetadot; linear_accel_local = R' (a + (0, 0, 9.81)) with a = (v+ - v)[0:3] / h of the last substep (what step 5
 *     of the Kalman filter inverts); contact[4] = (n_i > contact_threshold), n_i of the last substep; feet_heights = the ground heights given (0);
 *     mode = NULL (the plant reports contact flags); the ground truth for BPMPC_ESTIMATOR_FROM_TOPIC, odom_pos, odom_quat, odom_lin_vel and
 *     odom_ang_vel = E(zyx) thetadot (world); rbd[2*(6+nj)], the ground truth in the layout of bpmpc_controller_tick; contact_force[12], the force
 *     the ground applied to each point over the last substep, f_i - D_i J_i v+ (0 for an open point).  bpmpc_plant_device_outputs: these buffers where
 *     they live, leading dimension max_batch; &outputs.sensors is an argument of bpmpc_estimator_update (inputs_on_device = 1) as it stands.
 *   state: bpmpc_plant_set_state sets q, v of the robots of mask (NULL: every robot below batch) from rbd[batch*2*(6+nj)] (thetadot = E^-1 angular
 *     velocity) and their rows of the rbd output; the other outputs keep the values of the last step.  Robots outside the mask do not change by one
 *     bit.  The anchors of the robots of mask are cleared, and of no other robot.  Host values must be finite.  bpmpc_plant_get_state: host copy of the rbd output (synchronises).  A step needs a state for every robot of
 *     its batch: its batch must be that of the last set_state.
 *   bpmpc_plant_step: one control step.  The command holds pos_des, vel_des, tau_ff, kp, kd ([batch*nj] each), base_force ([batch*3], nullable) and
 *     feet_heights ([batch*4], nullable).  inputs_on_device != 0: device pointers, the call only enqueues on the plant's stream; host arrays are
 *     copied first and the call synchronises.  BPMPC_ERR_INVALID_ARGUMENT: substeps < 1, period not finite or <= 0, a null handle or required
 *     pointer, a batch other than that of the last set_state; batch > max_batch: BPMPC_ERR_CAPACITY.
 *   bpmpc_plant_step_controlled: one step on the controller's last tick, gathered on the device: posDes / velDes / tau from the tick's joint_cmd,
 *     kp / kd from the controller's joint gains (bpmpc_controller_joint_outputs).  The plant's stream waits for the tick and the solver's stream
 *     waits for the step, so no caller synchronises by hand.  base_force / feet_heights: host or device by inputs_on_device.  Before the first tick,
 *     or with a batch other than the last tick's: BPMPC_ERR_INVALID_ARGUMENT.
 *   bpmpc_estimator_update_from_plant: bpmpc_estimator_update(inputs = the plant's device outputs, inputs_on_device = 1) with the estimator's stream
 *     waiting for a step that was only enqueued and the plant's stream waiting for the update before the next step overwrites the outputs.  The loop
 *     step_controlled -> update_from_plant -> bpmpc_controller_tick_estimated -> every k ticks setup_commands(x0 = NULL) + run synchronises nowhere.
 *     A caller who passes the output pointers to bpmpc_estimator_update itself orders the two streams itself (bpmpc_plant_get_state synchronises).
 *   settings: a parameter row of BPMPC_PLANT_PARAM_STRIDE doubles per robot, [kn, cn, d0, mu, v_eps, contact_threshold, reserved 0, reserved 0].
 *     Every row starts as the keys plant.<name> of task_info_path; an absent key or a NULL path gives the defaults 5e4 N/m, 5e2 N s/m, 1e-3 m,
 *     0.7, 0.01 m/s, 1 N.  bpmpc_plant_get_params / set_params / reset_params have the shapes, masks, n_rows and host / device semantics of
 *     bpmpc_estimator_get_params / set_params / reset_params; host rows are validated - every entry finite, kn, d0 and v_eps positive, the others not
 *     negative - and a bad entry is named in bpmpc_last_error() and changes nothing.  bpmpc_plant_load_params / check_params: the settings ingest
 *     and the row validation as host-only functions, as the estimator's.  The torque limits are the WBC's key torqueLimitsTask of task_info_path,
 *     per handle (a NULL path: no limits).
 *   stiction: kt >= 0 [N/m] per robot, beside the parameter row (whose layout and reserved entries it leaves alone).  Every robot starts with the key
 *     plant.kt of task_info_path; an absent key or a NULL path gives 0.  bpmpc_plant_set_stiction(kt[n_rows], n_rows = 1 or batch): masks and host /
 *     device semantics of bpmpc_plant_set_params; host values must be finite and not negative, else BPMPC_ERR_INVALID_ARGUMENT names the entry in
 *     bpmpc_last_error() and nothing changes.  A robot whose kt changes loses its anchors.  bpmpc_plant_get_stiction: kt of `robot`, or with
 *     robot < 0 the start value.  bpmpc_plant_reset_stiction: every robot back to the start value, every anchor cleared.
 *     bpmpc_plant_load_stiction: the ingest as a host-only function.  bpmpc_plant_get_anchors: host copies of the anchors [batch*4*2] and the
 *     flags [batch*4] (synchronises).  A handle on which stiction was never set - start value 0, no set_stiction since create or
 *     reset_stiction - launches the kernel without stick-slip contacts, k_plant_step; any other launches k_plant_stick_step, in which a robot with
 *     kt = 0 computes the same bits.
 *   sensors: a sensor model behind the step kernels, per robot: noise, bias, quantisation, latency and contact dropout on what the IMU, the joint
 *     encoders and the contact switches report.  The step kernels and their outputs (the truth) are not changed by it; it writes a second block,
 *     the sensed block.  It is off until it is used (see "switching").
 *     random numbers: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85) with counter = (tick low word, tick
 *       high word, robot index in the batch, block) and key = (seed low word, seed high word): every draw is a function of (seed, robot, tick) and
 *       of nothing else.  A word w gives the uniform (w + 0.5) 2^-32.  The Gaussian z[g], g = 0..63, comes from block g >> 1, words (0, 1) for even
 *       g and (2, 3) for odd g: z = sqrt(-2 ln u1) cos(2 pi u2), so |z| <= 6.76.  The contact uniforms u[0..3] are the four words of block 32.  The
 *       turn-on draw is the same table at the tick with all 64 bits set.
 *     state per robot: key (2 words), tick t (64 bit), samples n since the last (re)start, gyro bias bg[3], accelerometer bias ba[3], a ring of 9
 *       measured samples; one sample is joint_pos[nj], joint_vel[nj], quat[4], angular_vel_local[3], linear_accel_local[3], contact[4].
 *     settings: a row of BPMPC_PLANT_SENSOR_PARAM_STRIDE doubles per robot, [gyro_noise rad/s, gyro_bias_walk rad/s/sqrt(s), gyro_bias_init rad/s,
 *       accel_noise m/s^2, accel_bias_walk m/s^2/sqrt(s), accel_bias_init m/s^2, orientation_noise rad, joint_pos_noise rad, joint_pos_resolution rad
 *       (0: not quantised), joint_vel_noise rad/s, contact_dropout (probability 0..1), delay_steps (integer valued, 0..8), reserved 0 x 4].  Every
 *       row starts as the keys plantSensors.<name> of task_info_path, an absent key or a NULL path gives 0; the key plantSensors.seed (absent: 0) is
 *       every robot's start key.  Host rows are validated - every entry finite and not negative, contact_dropout <= 1, delay_steps an integer <= 8,
 *       the reserved entries 0 - and a bad entry is named in bpmpc_last_error() and changes nothing.  A device row cannot be looked at: the kernel
 *       clamps its delay_steps to 0..8 (the integer part; not a number: 0).
 *     one measurement per control step of length period, by k_plant_sense behind the step kernel on the plant's stream:
 *       1. the draws z[0..63], u[0..3] at (t, robot, key)
 *       2. bias walk: bg += gyro_bias_walk sqrt(period) z[3..5]; ba += accel_bias_walk sqrt(period) z[9..11]
 *       3. the measured sample: angular_vel_local + bg + gyro_noise z[0..2]; linear_accel_local + ba + accel_noise z[6..8]; with
 *          orientation_noise > 0 quat (x) dq, normalised, where delta = orientation_noise z[12..14] and dq = (delta sin(|delta| / 2) / |delta|,
 *          cos(|delta| / 2)) (x y z w, Hamilton product: a rotation by delta in the body frame), else quat as it is; joint_pos_j + joint_pos_noise
 *          z[16 + j], then rint(. / D) D when D = joint_pos_resolution > 0 (ties to even); joint_vel_j + joint_vel_noise z[32 + j];
 *          contact_i = truth_i and not (u[i] < contact_dropout)
 *       4. the sample goes into ring slot n mod 9; the sensed block receives the sample with index max(n - delay_steps, 0)
 *       5. t += 1, n += 1
 *       feet_heights, odom_pos, odom_quat, odom_lin_vel, odom_ang_vel, rbd and contact_force stay the truth: the sensed block shares those pointers,
 *       and its mode is NULL.  A robot whose row is all zero (and whose biases are zero) reads the truth, equal as numbers.
 *     calls: bpmpc_plant_get_sensor_params / set_sensor_params have the shapes, masks, n_rows and host / device semantics of bpmpc_plant_get_params
 *       / set_params (robot < 0: the row of the task file).  bpmpc_plant_seed_sensors, for the robots of mask (NULL: every robot below batch; host
 *       or device by inputs_on_device): key = seed reinterpreted as unsigned, t = 0, n = 0, bg = gyro_bias_init z0[0..2], ba = accel_bias_init
 *       z0[3..5] with z0 the turn-on draw under the new key and the robot's current row; robots outside the mask do not change by one bit.
 *       bpmpc_plant_get_sensor_state: host copies of bg [batch*3], ba [batch*3] and ticks [batch*2] = (t, n) per robot as doubles (exact below
 *       2^53); each pointer nullable; synchronises.  bpmpc_plant_sensed_outputs: the sensed block where it lives (leading dimension max_batch), an
 *       argument of bpmpc_estimator_update (inputs_on_device = 1) as it stands.  bpmpc_plant_load_sensor_params / check_sensor_params: the ingest
 *       (row[16]; a bad plantSensors.seed is refused there too) and the row validation as host-only functions.  bpmpc_plant_sensor_draw: z[64] and
 *       u[4] of (seed, robot, tick) from the text the kernels compile, on the host; tick = -1 is the turn-on draw.
 *     switching: a handle is untouched when its task file has no non-zero plantSensors.<name> key and it has had no set_sensor_params or
 *       seed_sensors since create or reset_sensor_params.  An untouched handle launches nothing beside its step kernel, and
 *       bpmpc_estimator_update_from_plant reads the truth.  Any other handle is switched: every step launches k_plant_sense behind the step kernel,
 *       bpmpc_estimator_update_from_plant reads the sensed block behind it, and until a step has run since the switch it returns
 *       BPMPC_ERR_INVALID_ARGUMENT (there is no measurement yet).  A handle whose task file has a non-zero key is created switched, every row the
 *       file's, turned on as by seed_sensors(plantSensors.seed).  bpmpc_plant_set_state sets n = 0 for the robots of its mask - their history is
 *       forgotten, the next sample is the first of a new one - and touches neither bias, key nor t, and does not write the sensed block.
 *       bpmpc_plant_reset_sensor_params zeroes every row, bias, t and n, restores the start key and returns the handle to untouched.
 *   inputs: an input model in front of the step kernels, per robot: command latency, packet loss and pushes on the base.  It turns the command
 *     and base force a step was called with into the command and base force the step kernel consumes; the step kernels are not changed by it.  It
 *     is off until it is used (see "switching" below).  The latency is that of the reference's simulated hardware layer, which buffers every joint
 *     command and applies the oldest one that is not older than gazebo/delay (BipedalHWSim::writeSim, bipedal_gazebo/src/BipedalHWSim.cpp:160-176:
 *     entries are dropped from the back of cmdBuffer_ while stamp + delay < time, and the back is used); the shipped configurations set 9 ms (H1,
 *     Hunter, the bipedal_gazebo default) and 2 ms (OpenLoong).  Packet loss and pushes have no counterpart in the reference.
 *     state per robot: key (2 words), tick t (64 bit): steps since the last seeding, n (64 bit): steps since the robot's last (re)start, a ring of
 *       R = 16 arrived commands; one slot is the five rows pos_des, vel_des, tau_ff, kp, kd, 5 nj doubles.
 *     settings: a row of BPMPC_PLANT_INPUT_PARAM_STRIDE doubles per robot, [delay s, dropout (probability 0..1), push_force N, push_interval s,
 *       push_duration s, reserved 0 x 3].  Every row starts as the keys plantInputs.<name> of task_info_path, an absent key or a NULL path gives 0;
 *       the key plantInputs.seed (absent: 0) is every robot's start key.  Host rows are validated - every entry finite and not negative,
 *       dropout <= 1, the reserved entries 0 - and a bad entry is named in bpmpc_last_error() and changes nothing.  A device row cannot be looked
 *       at: the kernel counts an entry that is not a number or is negative as 0, dropout above 1 as 1, a time of 2^62 ns or more as 2^62 ns.
 *     random numbers: the generator and the uniform of the sensors (Philox4x32-10, counter = (low word, high word, robot, block), key = seed words,
 *       uniform (w + 0.5) 2^-32) with two blocks of their own, so that a handle seeded alike for sensors and inputs shares no word: block 64 at
 *       counter t, whose word 0 is the loss draw u_drop; block 65 at counter w (a push window, below), whose words 0 and 1 are u_s and u_dir.
 *     one control step, by k_plant_input in front of the step kernel on the plant's stream, with the incoming command c, the caller's base force f
 *       (NULL: 0) and the call's period.  ns(x) = llrint(x 1e9): integer nanoseconds, as ros::Time / ros::Duration compare them in the reference
 *       (that ros::Duration(double) rounds to the nearest nanosecond is recalled behaviour, not read from a source).  P = max(1, ns(period)).
 *       1. loss: lost = (n > 0) and (u_drop < dropout); arrived = lost ? ring[(n - 1) mod R] : c; ring[n mod R] = arrived.  A lost packet leaves
 *          the joint on what arrived last; consecutive losses keep holding it.
 *       2. delay: k = min(R - 1, ns(delay) / P) (integer division); applied = ring[max(n - k, 0) mod R]: the oldest command whose age is at most
 *          delay, and until the history is long enough the first one.  With k = 0 and no loss applied is c, bit for bit.
 *       3. push, off unless push_force > 0 and ns(push_interval) > 0: W = max(1, ns(push_interval) / P), D = min(W, max(1, ns(push_duration) / P)),
 *          w = t / W, o = t mod W, s = min(W - D, floor(u_s (W - D + 1))), pushing = (s <= o < s + D); force = f + push_force (cos 2 pi u_dir,
 *          sin 2 pi u_dir, 0) in the world frame while pushing, else f bit for bit: exactly one push of D steps per window of W steps.
 *       4. the applied rows (stride nj, leading dimension max_batch), the applied force [3] and the ints lost, pushing, delay_steps = k are written;
 *          t += 1, n += 1.  The step kernel then runs on the applied rows and force.
 *     calls: bpmpc_plant_get_input_params / set_input_params / reset_input_params have the shapes, masks, n_rows and host / device semantics of
 *       bpmpc_plant_get_sensor_params / set_sensor_params / reset_sensor_params (robot < 0: the row of the task file).  bpmpc_plant_seed_inputs, for
 *       the robots of mask (NULL: every robot below batch; host or device by inputs_on_device): key = seed reinterpreted as unsigned, t = 0, n = 0;
 *       robots outside the mask do not change by one bit.  bpmpc_plant_get_input_state: host copies of ticks [batch*2] = (t, n) per robot as doubles
 *       (exact below 2^53) and of delay_steps, lost and pushing [batch] of the last step; each pointer nullable; synchronises.
 *       bpmpc_plant_applied_command: the applied rows and force where they live (leading dimension max_batch); feet_heights is the device pointer
 *       the last step consumed (the caller's, or the handle's copy of a host array; NULL when none was given); BPMPC_ERR_INVALID_ARGUMENT on an
 *       untouched handle or before the first step since the switch.  bpmpc_plant_load_input_params / check_input_params: the ingest (row[8]; a bad
 *       plantInputs.seed is refused there too) and the row validation as host-only functions.  bpmpc_plant_input_draw: u[3] = (u_drop of block 64,
 *       u_s and u_dir of block 65) of (seed, robot) at that counter, from the text the kernel compiles, on the host.
 *     switching: a handle is untouched when its task file has no non-zero plantInputs.<name> key and it has had no set_input_params or seed_inputs
 *       since create or reset_input_params.  An untouched handle launches nothing new and hands the step kernel the caller's pointers.  Any other
 *       handle is switched: bpmpc_plant_step, bpmpc_plant_step_controlled and bpmpc_plant_step_supervised launch k_plant_input in front of the step
 *       kernel - in the latter two inside the waits that bracket the step, so the tick's or supervisor's buffers are read in the window in which the
 *       step kernel reads them on an untouched handle.  A switched robot whose row is all zero receives its command and force bit for bit.
 *       bpmpc_plant_set_state sets n = 0 for the robots of its mask - their buffered commands are forgotten (writeSim's "Simulation reset":
 *       buffer.clear()) - and touches neither key nor t.  bpmpc_plant_reset_input_params zeroes every row, t and n, restores the start key and
 *       returns the handle to untouched.
 *   joints: a joint model inside the step, per robot: rotor inertia (armature), viscous damping, Coulomb friction and end stops.  It is this
 *     engine's own model like the rest of the plant; it imitates neither MuJoCo's constraint solver nor Gazebo's and is pinned against neither.  It
 *     is off until it is used (see "switching" below).
 *     settings: a joint row of BPMPC_PLANT_JOINT_PARAM_STRIDE = 64 doubles per robot, beside the parameter row (whose layout and reserved entries it
 *       leaves alone):
 *          0..11  armature[j]       kg m^2       >= 0, added to the diagonal of M at coordinate 6 + j
 *         12..23  damping[j]        N m s/rad    >= 0, viscous, linearly implicit
 *         24..35  friction_loss[j]  N m          >= 0, regularised Coulomb, linearly implicit
 *         36..47  lower[j]          rad          may be -inf
 *         48..59  upper[j]          rad          may be +inf; lower < upper
 *         60      k_limit           N m/rad      >= 0, end-stop spring, explicit
 *         61      c_limit           N m s/rad    >= 0, end-stop damper, implicit, acts only beyond a limit
 *         62      w_eps             rad/s        > 0, regularisation of the friction law
 *         63      reserved                       written as 0
 *       Entries j >= nj are ignored.  The neutral row is armature = damping = friction_loss = 0, lower = -inf, upper = +inf, k_limit = 1e4,
 *       c_limit = 1e2, w_eps = 0.01.  The three scalar defaults are this engine's choice; nobody has measured them on a robot.  The end-stop spring
 *       is explicit, so it is stable only while h^2 k_limit < 4 (I_jj + armature_j + h (kd_j + c_j)) with I_jj the joint's diagonal entry of M: at
 *       h = 0.5 ms and k_limit = 1e4 the left side is 2.5e-3 kg m^2, which a joint with no armature, no damping and no kd can fall below.
 *     one substep for a robot whose row is not neutral, joint j, coordinate l = 6 + j, start-of-substep (q, v), in terms of steps 3 and 4 above:
 *       a. M_ll += armature_j: the M of both sides, the system matrix and M v
 *       b. end stop: pen_up = max(q_l - upper_j, 0), pen_lo = max(lower_j - q_l, 0), tau_lim = k_limit (pen_lo - pen_up), added to the
 *          generalised force outside the torque clamp of step 3 (the clamp models the actuator, the end stop does not);
 *          beyond = pen_up > 0 or pen_lo > 0
 *       c. implicit joint damping c_j = damping_j + friction_loss_j / sqrt(v_l^2 + w_eps^2) + (beyond ? c_limit : 0)
 *       d. the system matrix gets h (kd_j + c_j) on its diagonal where it gets h kd_j in step 4; nothing is added to the right-hand side (there is
 *          no velDes for passive damping)
 *       The matrix stays symmetric positive definite and is factored as before.  A robot with the neutral row (every armature, damping and
 *       friction_loss of a joint j < nj zero, every limit infinite) runs the arithmetic of k_plant_stick_step and nothing else.
 *     Every row starts as the start row of task_info_path: the neutral row, then the optional scalar keys plantJoints.armature, .damping,
 *       .frictionLoss (each applied to every joint), .kLimit, .cLimit, .wEps; plantJoints.fromUrdf 1 takes lower / upper from the model's <limit>
 *       and damping / friction_loss from its <dynamics damping friction> (bpmpc_model_get "joint_lower", "joint_upper", "joint_damping",
 *       "joint_friction"), and the scalar keys override the URDF values where both are given.  An absent block or a NULL path gives the neutral row.
 *     calls: bpmpc_plant_get_joint_params / set_joint_params / reset_joint_params have the shapes (row[64]), masks, n_rows, host / device semantics,
 *       error codes and stream ordering of bpmpc_plant_get_params / set_params / reset_params (robot < 0: the start row).  Host rows are validated -
 *       every used entry finite, except that lower may be -inf and upper +inf; armature, damping, friction_loss, k_limit and c_limit not negative;
 *       lower < upper; w_eps > 0; reserved 0 - and a bad entry is named in bpmpc_last_error() and changes nothing.  A device row cannot be looked
 *       at: the kernel takes a w_eps that is not > 0 as 0.01.  The state of robots outside the mask does not change by one bit, given that the same
 *       kernel is launched.  bpmpc_plant_set_state and a restart keep the rows, as they keep the parameter rows.  bpmpc_plant_load_joint_params /
 *       check_joint_params: the ingest (row[64], from the model and task_info_path) and the row validation (rows[n_rows*64] of a robot with nj
 *       joints) as host-only functions.
 *     switching: a handle whose start row is neutral (in the sense above: what a robot with nj joints reads of it) and that has had no set_joint_params since create or reset_joint_params launches
 *       exactly what it launched before the plant had a joint model (k_plant_step or k_plant_stick_step).  Any other handle launches
 *       k_plant_joint_step, which holds stick-slip contacts and the joint model, from bpmpc_plant_step, bpmpc_plant_step_controlled and
 *       bpmpc_plant_step_supervised alike.  The first set_joint_params on a handle therefore changes which kernel runs for EVERY robot of it, also
 *       those outside its mask and those whose row stays neutral: such a robot agrees with the other kernels to rounding (1e-9 relative is
 *       asserted; on the device it returned k_plant_stick_step's bits for H1 and G1, which the tests print and nothing promises).  bpmpc_plant_reset_joint_params writes the start row into every row and returns the handle
 *       to the kernel that start row selects.
 *   bodies: the rigid bodies themselves, per robot: mass, centre of mass and inertia of every body.  Without a body row every robot of a batch is
 *     simulated with exactly the inertial constants its controller plans with (the model's); with one the plant can be heavier, lighter, carry a
 *     payload or have a shifted centre of mass while the WBC and the MPC keep the model's: the mismatch is the point.  The controller side is not
 *     touched.  It is off until it is used (see "switching" below).
 *     settings: a body row of BPMPC_PLANT_BODY_PARAM_STRIDE = 160 doubles per robot: ten blocks of 16 slots, body b (0 = base, b = 1..nj the link
 *       moved by joint b) at slot b of each block.  Entry-major, so the lanes of consecutive bodies read consecutive words:
 *           0..15   mass[b]                              kg                          > 0
 *          16..63   com_x[b], com_y[b], com_z[b]         m, body frame               finite
 *          64..159  ixx, ixy, ixz, iyy, iyz, izz[b]      kg m^2, about the com,      symmetric positive definite, principal moments obey the
 *                                                        body frame                  triangle inequality (none above the sum of the other two)
 *       Slots b > nj are ignored on input and written as 0 by the getters.  The model row is what bpmpc_model_get returns for "body_mass",
 *       "body_com" and "body_inertia" (of the 3 x 3 its upper triangle), bit for bit.
 *     one substep for a robot with a body row is the substep above as it stands, with the three constants of every body - m_b, c_b, I_b in the
 *       rigid-body quantities of step 1 - taken from the robot's row.  Everything else still comes from the model: geometry, axes, contact
 *       offsets and gravity.
 *     Every row starts as the start row of task_info_path: the model row, then the optional keys plantBodies.massScale (every body's mass and
 *       inertia times it), plantBodies.payloadMass [kg], plantBodies.payloadBody (default 0, the base) and plantBodies.payloadOffset (a 3 x 1
 *       block "(0,0) x (1,0) y (2,0) z", body frame, default 0 0 0): a point mass merged into that body as bpmpc_plant_compose_body_row does.  An
 *       absent block or a NULL path gives the model row.
 *     calls: bpmpc_plant_get_body_params / set_body_params / reset_body_params have the shapes (row[160]), masks, n_rows, host / device semantics,
 *       error codes and stream ordering of bpmpc_plant_get_joint_params / set_joint_params / reset_joint_params (robot < 0: the start row).  Host
 *       rows are validated against the rules of the table - the principal moments by a Jacobi eigen-solve of the 3 x 3, the triangle inequality to
 *       1e-9 relative - and a bad entry is named in bpmpc_last_error() and changes nothing.  Device rows are not looked at: a row that breaks
 *       the rules gives a mass matrix that need not be positive definite, and the state of that robot, and of that robot only, is then anything.
 *       bpmpc_plant_set_state and a restart keep the rows.  bpmpc_plant_load_body_params / check_body_params: the ingest (row[160], from the model
 *       and task_info_path) and the row validation (rows[n_rows*160] of a robot with nj joints) as host-only functions.
 *       bpmpc_plant_compose_body_row(model, row_in, body, mass_scale, com_shift, payload_mass, payload_pos, row_out), host only, builds a row from
 *       row_in (NULL: the model row), in this order: mass and inertia of `body` times mass_scale (> 0; uniform density); its com moved by
 *       com_shift[3] (NULL: 0; the inertia about the new com unchanged); a point mass payload_mass (>= 0) at payload_pos[3] (body frame) merged
 *       into the body: new mass, new com, and the new inertia about the new com by the parallel-axis theorem.  body = -1 applies mass_scale to
 *       every body and takes no shift or payload.  row_out may be row_in.
 *     switching: a handle whose start row is the model row (what a robot with nj joints reads of it, bit for bit) and that has had no
 *       set_body_params since create or reset_body_params launches exactly what it launches without body rows (k_plant_step, k_plant_stick_step
 *       or k_plant_joint_step).  Any other handle launches k_plant_body_step, which holds stick-slip contacts, the joint model and the body rows,
 *       from bpmpc_plant_step, bpmpc_plant_step_controlled and bpmpc_plant_step_supervised alike, for every robot of it, also those outside the
 *       mask and those whose row is the model row: such a robot agrees with the other kernels to rounding (1e-9 relative is asserted; whether
 *       the bits are equal the tests print and nothing promises).  bpmpc_plant_reset_body_params writes the start row into every row and returns
 *       the handle to the kernel that start row selects.  The sensor and input kernels in front of and behind the step are unaffected.
 * ------------------------------------------------------------------------------------------------------------- */
#define BPMPC_PLANT_PARAM_STRIDE 8
#define BPMPC_PLANT_JOINT_PARAM_STRIDE 64
#define BPMPC_PLANT_BODY_PARAM_STRIDE 160
#define BPMPC_PLANT_SENSOR_PARAM_STRIDE 16
#define BPMPC_PLANT_INPUT_PARAM_STRIDE 8
typedef struct bpmpc_plant bpmpc_plant;
typedef struct {
  const double *pos_des, *vel_des, *tau_ff, *kp, *kd;   /* [batch*nj] */
  const double *base_force;                             /* [batch*3] nullable: world-frame force on the base origin */
  const double *feet_heights;                           /* [batch*4] nullable: ground height under each contact point */
} bpmpc_joint_command;
typedef struct {
  bpmpc_sensor_inputs sensors;
  double *rbd, *contact_force;                          /* [batch*2*(6+nj)], [batch*12] */
} bpmpc_plant_outputs;
int bpmpc_plant_create(const bpmpc_model* model, const char* task_info_path, int device, int max_batch, bpmpc_plant** out);
void bpmpc_plant_destroy(bpmpc_plant* plant);
int bpmpc_plant_set_state(bpmpc_plant* plant, int batch, const int* mask, const double* rbd, int inputs_on_device);
int bpmpc_plant_get_state(bpmpc_plant* plant, int batch, double* host_rbd);
int bpmpc_plant_step(bpmpc_plant* plant, int batch, const bpmpc_joint_command* command, int inputs_on_device, double period, int substeps);
int bpmpc_plant_device_outputs(bpmpc_plant* plant, bpmpc_plant_outputs* dev_out);
int bpmpc_plant_step_controlled(bpmpc_plant* plant, bpmpc_controller* controller, int batch, double period, int substeps, const double* base_force,
                                const double* feet_heights, int inputs_on_device);
int bpmpc_estimator_update_from_plant(bpmpc_estimator* estimator, bpmpc_plant* plant, int batch, double period, double* host_rbd);
int bpmpc_plant_get_params(const bpmpc_plant* plant, int robot, double* row);
int bpmpc_plant_set_params(bpmpc_plant* plant, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device);
int bpmpc_plant_reset_params(bpmpc_plant* plant);
int bpmpc_plant_load_params(const char* task_info_path, double* row);
int bpmpc_plant_check_params(const double* rows, int n_rows);
int bpmpc_plant_set_stiction(bpmpc_plant* plant, int batch, const int* mask, const double* kt, int n_rows, int inputs_on_device);
int bpmpc_plant_get_stiction(const bpmpc_plant* plant, int robot, double* kt);
int bpmpc_plant_reset_stiction(bpmpc_plant* plant);
int bpmpc_plant_load_stiction(const char* task_info_path, double* kt);
int bpmpc_plant_get_anchors(bpmpc_plant* plant, int batch, double* host_anchor, int* host_anchored);
int bpmpc_plant_get_sensor_params(const bpmpc_plant* plant, int robot, double* row);
int bpmpc_plant_set_sensor_params(bpmpc_plant* plant, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device);
int bpmpc_plant_reset_sensor_params(bpmpc_plant* plant);
int bpmpc_plant_load_sensor_params(const char* task_info_path, double* row);
int bpmpc_plant_check_sensor_params(const double* rows, int n_rows);
int bpmpc_plant_seed_sensors(bpmpc_plant* plant, int batch, const int* mask, long seed, int inputs_on_device);
int bpmpc_plant_get_sensor_state(bpmpc_plant* plant, int batch, double* gyro_bias, double* accel_bias, double* ticks);
int bpmpc_plant_sensed_outputs(bpmpc_plant* plant, bpmpc_sensor_inputs* dev_out);
int bpmpc_plant_sensor_draw(long seed, int robot, long tick, double* z, double* u);
int bpmpc_plant_get_input_params(const bpmpc_plant* plant, int robot, double* row);
int bpmpc_plant_set_input_params(bpmpc_plant* plant, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device);
int bpmpc_plant_reset_input_params(bpmpc_plant* plant);
int bpmpc_plant_load_input_params(const char* task_info_path, double row[8]);
int bpmpc_plant_check_input_params(const double* rows, int n_rows);
int bpmpc_plant_seed_inputs(bpmpc_plant* plant, int batch, const int* mask, long seed, int inputs_on_device);
int bpmpc_plant_get_input_state(bpmpc_plant* plant, int batch, double* ticks, int* delay_steps, int* lost, int* pushing);
int bpmpc_plant_applied_command(bpmpc_plant* plant, bpmpc_joint_command* dev_out);
int bpmpc_plant_input_draw(long seed, int robot, long counter, double u[3]);
int bpmpc_plant_get_joint_params(const bpmpc_plant* plant, int robot, double* row);
int bpmpc_plant_set_joint_params(bpmpc_plant* plant, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device);
int bpmpc_plant_reset_joint_params(bpmpc_plant* plant);
int bpmpc_plant_load_joint_params(const bpmpc_model* model, const char* task_info_path, double* row);
int bpmpc_plant_check_joint_params(const double* rows, int n_rows, int nj);
int bpmpc_plant_get_body_params(const bpmpc_plant* plant, int robot, double* row);
int bpmpc_plant_set_body_params(bpmpc_plant* plant, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device);
int bpmpc_plant_reset_body_params(bpmpc_plant* plant);
int bpmpc_plant_load_body_params(const bpmpc_model* model, const char* task_info_path, double* row);
int bpmpc_plant_check_body_params(const double* rows, int n_rows, int nj);
int bpmpc_plant_compose_body_row(const bpmpc_model* model, const double* row_in, int body, double mass_scale, const double* com_shift, double payload_mass,
                                 const double* payload_pos, double* row_out);

/* ---------------------------------------------------------------------------------------------------------------
 * Policy buffer = MPC_MRT_Interface between the solve and the control tick for a BATCH of robots, on the device.  In the reference a thread calls
 * advanceMpc() at mpcDesiredFrequency (bipedal_controllers/src/BipedalController.cpp:332-350) while update() calls updatePolicy() and
 * evaluatePolicy() at the control rate on whatever policy was finished last (:191-200): a tick never waits for a solve, and a solve that is still
 * running changes nothing for the ticks that happen meanwhile.  Without a buffer a tick reads the solver's working arrays on the solver's stream:
 * it queues behind the solve, the policy is gone from bpmpc_solver_setup_commands to the end of bpmpc_solver_run, and a failed solve hands its
 * iterate to the next tick.
 *   layout: two slots.  A slot holds per robot, with nothing shared between robots, the grid row the solver keeps per grid (node times, node kinds,
 *     modes, node count), x[N+1][nx], u[N][nu] and, when the solver's feedback policy is on, K[N][nu][nx]; N is the solver's max_nodes.  Ticks read
 *     the FRONT slot, publishes write the BACK slot.  Beside the slots, per robot: pending, generation (0 after create), t0 (the time of node 0 of
 *     the robot's policy) and status (the solve status it was published with).  The handle owns a stream: the buffer's stream.
 *   bpmpc_policy_create: for an SQP solver; a DDP solver is refused with BPMPC_ERR_UNSUPPORTED (its solution lives on the time points of its own
 *     roll-out, as for bpmpc_controller_tick).  max_batch above the solver's: BPMPC_ERR_CAPACITY.  The solver must outlive the buffer; detach the
 *     buffer from every controller before it is destroyed.
 *   bpmpc_policy_publish: enqueued on the SOLVER's stream, behind the run it publishes; with inputs_on_device != 0 or mask == NULL it never
 *     synchronises (a host mask is copied first and the call waits for the solver's stream).  Robot b is taken when mask[b] != 0 (NULL: every
 *     robot) and, with skip_failed != 0, the status of its last run is not 2; the status is read from the statistics on the device, not from the
 *     host.  A taken robot's live nodes (its grid's node count, plus one for x and the times) are copied from the solver's solution and grid row
 *     into the back slot, its pending flag is set and t0 and status are noted for the adoption.  A robot that is not taken keeps the policy,
 *     generation, t0 and status it has; the first publish after an adoption copies its front row into the back slot, so that the adoption can turn
 *     the slots over for the whole batch with one set of pointers for the tick kernel.  The refusals are those of a tick without a buffer - a
 *     completed bpmpc_solver_run since the last setup, no restart waiting, the batch of that setup - BPMPC_ERR_CAPACITY above max_batch, and a publish
 *     whose batch differs from the last publish's must take every robot (mask == NULL, skip_failed == 0).  Before it writes, the solver's stream
 *     waits for the last adoption: ticks enqueued before that adoption may still be reading what is now the back slot.  A second publish before an
 *     adoption overwrites the pending data of the robots it takes, and only theirs.
 *   bpmpc_policy_update = updatePolicy.  With no publish outstanding *adopted = 0 and nothing happens.  wait != 0: the buffer's stream waits for the
 *     last publish, then the adoption: the slots change roles and every pending robot takes generation + 1, its new t0 and status; nothing blocks on
 *     the host (simulations and tests: the policy takes effect at a known tick).  wait == 0: the reference's behaviour; if the last publish has
 *     not completed yet nothing is enqueued and *adopted = 0.  *adopted = 1 says that an adoption was enqueued, also when every robot of the
 *     publish was skipped.
 *   bpmpc_policy_info: host copies of generation, t0 and status [batch], each nullable; synchronises the buffer's stream.  They describe the
 *     policies of the front slot as of the last adoption.
 *   bpmpc_controller_attach_policy (NULL detaches): while attached, bpmpc_controller_tick, bpmpc_controller_tick_estimated,
 *     bpmpc_controller_set_joint_gains and the observation and WBC part of bpmpc_controller_restart run on the BUFFER's stream and the tick
 *     evaluates the front slot; the tick kernels are the same.  Detached, every call does exactly what it does without a buffer, on the solver's
 *     stream.  The call drains both streams once; afterwards events order them: bpmpc_solver_setup_commands(x0 = NULL) waits for the last tick
 *     (whose observations it starts from) and the next tick waits for that read, a restart's solver part waits for its observation,
 *     bpmpc_plant_step_controlled waits for the tick on the buffer's stream.  BPMPC_ERR_INVALID_ARGUMENT when the buffer was created for another
 *     solver or device.  A buffered tick is refused with BPMPC_ERR_INVALID_ARGUMENT until one publish with mask == NULL and skip_failed == 0 has
 *     been adopted (the reference's "waiting for the initial policy"), with a batch other than the published one, and after a
 *     bpmpc_controller_restart until the next adoption.  That adoption's publish must take the restarted robots: the buffer does not check it, it
 *     is the caller's job (a restarted robot that a masked or skip_failed publish leaves out keeps ticking on the policy of its previous episode).
 *   the loop, M ticks per MPC period, the policy D ticks old when it takes effect:
 *       every tick:        bpmpc_plant_step_controlled -> bpmpc_estimator_update_from_plant -> bpmpc_controller_tick_estimated
 *       tick k, k % M == 0: bpmpc_solver_setup_commands(x0 = NULL); bpmpc_solver_run; bpmpc_policy_publish(skip_failed = 1)
 *       tick k, k % M == D: bpmpc_policy_update(wait = 1)
 *     Four streams carry its work: the solver's, the buffer's, the estimator's and the plant's; the handles create six (the solver's producer
 *     stream and the WBC's own are idle in it), against the four hardware queues a process opens by default.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct bpmpc_policy bpmpc_policy;
int bpmpc_policy_create(bpmpc_solver* solver, int max_batch, bpmpc_policy** out);
void bpmpc_policy_destroy(bpmpc_policy* policy);
int bpmpc_policy_publish(bpmpc_policy* policy, int batch, const int* mask, int inputs_on_device, int skip_failed);
int bpmpc_policy_update(bpmpc_policy* policy, int wait, int* adopted);
int bpmpc_policy_info(bpmpc_policy* policy, int batch, int* generation, double* t0, int* status);
int bpmpc_controller_attach_policy(bpmpc_controller* controller, bpmpc_policy* policy);

/* ---------------------------------------------------------------------------------------------------------------
 * Tracking telemetry = DebugPublisher::update (bipedal_controllers/src/debug/DebugPublisher.cpp, called from BipedalController.cpp:270;
 * msg/TrackingError.msg) for a BATCH of robots, kept on the device: per update and robot one SAMPLE of what the policy asks for beside what was
 * measured, error STATISTICS accumulated over an episode, and a RING of the last samples that freezes when the robot falls.  Nothing reaches the
 * host unless it is asked for.  The handle is off until it is attached: a controller without one launches and changes nothing of this.
 *   sample, BPMPC_TELEMETRY_SAMPLE_STRIDE(nj) = 40 + 2 nj doubles (60 at nj = 10, 64 at nj = 12):
 *       0..2, 3..5         base_pos_desired, base_zyx_desired     x*[6:9], x*[9:12] (the yaw as the policy has it, unwrapped)
 *       6..8, 9..11        base_pos_measured, base_zyx_measured   rbd[3:6], rbd[0:3]
 *       12..23             contact_pos_desired[4][3]              world positions of the model's four contact points at q_des = x*[6:12 + nj]
 *       24..35             contact_pos_measured[4][3]             the same at q_meas = [rbd[3:6], rbd[0:3], rbd[6:6 + nj]]
 *       36.., 36 + nj..    joint_pos_desired[nj], joint_pos_measured[nj]      x*[12:], rbd[6:6 + nj]
 *       36 + 2 nj .. + 3   t, safe, planned_mode, n               as doubles; 0 where the caller gave none; n: the robot's update counter at the sample
 *     The contact points, their order and the kinematic tree are the WBC's (the contact frames of the model, in its order).  The desired
 *     velocities that the reference computes and never publishes are not part of it.
 *   errors of a sample, Euclidean norms: e0 = |base_pos_desired - base_pos_measured|, e1 = |normalize_angle(base_zyx_desired - base_zyx_measured)|
 *     (per component, onto (-pi, pi]: a desired yaw of 3.1 against a measured yaw of -3.1 is an error of 0.083), e2..e5 = |contact_pos_desired_i -
 *     contact_pos_measured_i|, e6 = |joint_pos_desired - joint_pos_measured|; beside them |joint error| of every joint.
 *   state per robot:
 *     n             updates since the robot's last reset.
 *     statistics    BPMPC_TELEMETRY_STATS_STRIDE = 40 doubles: for group k = 0..6 at 3 k the sum of e_k^2, the largest e_k and the n at which it
 *                   occurred (the first, among equals); 21 the number of samples accumulated; 22 first_unsafe_n (-1: none); 23..34 the largest
 *                   |joint error| per joint (unused ones 0); 35..39 reserved, 0.
 *     ring          ring_len samples (fixed at create; 0: no ring) in device memory, [robot][slot][stride].  With n mod every == 0 the sample is
 *                   recorded into slot r mod ring_len, r the number of samples the robot has recorded since its reset (n / every while `every`
 *                   has not changed since).
 *     frozen        with freeze_on_unsafe (the default) a robot freezes at the first sample whose `safe` is given and 0 or that holds a measured or
 *                   desired entry (0 .. 35 + 2 nj) that is not finite.  That sample is recorded into the ring whatever `every` says, sets
 *                   first_unsafe_n, and is accumulated only if all its errors are finite.  Afterwards the robot's ring, statistics, last sample and n
 *                   do not change until it is reset: the ring holds the last ring_len recorded samples up to and including the fall.  A frozen
 *                   robot costs its wavefront the flag test.  With freeze_on_unsafe off nothing freezes: a sample that is not finite is recorded
 *                   and not accumulated, first_unsafe_n is still set once.
 *   bpmpc_telemetry_create: ring_len < 0 or max_batch < 1: BPMPC_ERR_INVALID_ARGUMENT; BPMPC_ERR_NO_DEVICE without a GPU.  The ring takes
 *     max_batch * ring_len * stride * 8 bytes.  Every robot starts reset.  The handle owns a stream.
 *   bpmpc_telemetry_update: the stand-alone entry, as bpmpc_wbc_update is for the WBC.  x_opt [batch][12 + nj], rbd [batch][2 (6 + nj)]; t [batch],
 *     safe [batch] and planned_mode [batch] are nullable.  Host arrays (inputs_on_device == 0) are copied first and the call synchronises; device
 *     pointers are only enqueued on the handle's stream.  BPMPC_ERR_CAPACITY above max_batch.
 *   bpmpc_telemetry_configure: every >= 1 (else BPMPC_ERR_INVALID_ARGUMENT) and freeze_on_unsafe, from the next update on; 1 and on after create.
 *   bpmpc_telemetry_reset: for the robots with mask[b] != 0 (NULL: every robot below batch) n = 0, not frozen, the statistics and the last sample
 *     cleared, the ring empty; the other robots do not change by one bit.  With a device mask the call only enqueues: the (safe == 0) mask of
 *     bpmpc_controller_restart restarts the robot and its record.
 *   bpmpc_telemetry_device_outputs: where the last sample [max_batch][stride], the statistics [max_batch][40] and the frozen flags [max_batch] live.
 *   bpmpc_telemetry_get_stats: host copies for the first `batch` robots, each nullable; synchronises the handle's stream.
 *   bpmpc_telemetry_fetch_ring: for robots[0 .. n_robots) (NULL: the robots 0 .. batch - 1, n_robots ignored) host_counts[r] <= ring_len samples
 *     into host_samples [n_robots][ring_len][stride] (nullable), oldest first, the slots behind the count untouched; synchronises.  A robot index
 *     outside [0, batch): BPMPC_ERR_INVALID_ARGUMENT.
 *   bpmpc_controller_attach_telemetry (NULL detaches): while attached, every bpmpc_controller_tick and bpmpc_controller_tick_estimated enqueues
 *     the telemetry's kernel behind the tick's commands on the controller's stream (the solver's, or the attached policy buffer's), on the tick's
 *     own device buffers: t, x_opt, the measured rbd the tick ran on, safe and planned_mode.  It adds no synchronise and copies nothing to the
 *     host; the tick's outputs are bit for bit those of a detached tick.  The handle's stream and the controller's are ordered by events, so a
 *     stand-alone update, a reset or a read may follow a tick without a synchronise.  BPMPC_ERR_INVALID_ARGUMENT for a handle of another robot or
 *     on another device, BPMPC_ERR_CAPACITY for a tick whose batch exceeds the handle's max_batch.  Detach before the handle is destroyed.
 *   the loop, with the record restarted beside the robot:
 *       bpmpc_plant_step_controlled -> bpmpc_estimator_update_from_plant -> bpmpc_controller_tick_estimated (the sample is taken here)
 *       on a fall: bpmpc_controller_restart(mask = (safe == 0)); read bpmpc_telemetry_fetch_ring of the fallen robots; bpmpc_telemetry_reset(mask)
 * ------------------------------------------------------------------------------------------------------------- */
#define BPMPC_TELEMETRY_SAMPLE_STRIDE(nj) (40 + 2 * (nj))
#define BPMPC_TELEMETRY_STATS_STRIDE 40
typedef struct bpmpc_telemetry bpmpc_telemetry;
int bpmpc_telemetry_create(const bpmpc_model* model, int device, int max_batch, int ring_len, bpmpc_telemetry** out);
void bpmpc_telemetry_destroy(bpmpc_telemetry* telemetry);
int bpmpc_telemetry_dims(const bpmpc_telemetry* telemetry, int* sample_stride, int* stats_stride, int* ring_len);
int bpmpc_telemetry_update(bpmpc_telemetry* telemetry, int batch, const double* t, const double* x_opt, const double* rbd, const int* safe,
                           const int* planned_mode, int inputs_on_device);
int bpmpc_telemetry_configure(bpmpc_telemetry* telemetry, int every, int freeze_on_unsafe);
int bpmpc_telemetry_reset(bpmpc_telemetry* telemetry, int batch, const int* mask, int inputs_on_device);
int bpmpc_telemetry_device_outputs(bpmpc_telemetry* telemetry, double** sample, double** stats, int** frozen);
int bpmpc_telemetry_get_stats(bpmpc_telemetry* telemetry, int batch, double* host_stats, int* host_frozen);
int bpmpc_telemetry_fetch_ring(bpmpc_telemetry* telemetry, int batch, const int* robots, int n_robots, double* host_samples, int* host_counts);
int bpmpc_controller_attach_telemetry(bpmpc_controller* controller, bpmpc_telemetry* telemetry);

/* ---------------------------------------------------------------------------------------------------------------
 * Plan geometry = BipedalControllerVisualizer::update (bipedal_controllers/src/BipedalControllerVisualizer.cpp:73-87, and its twin
 * ocs2_bipedal_robot_ros/src/visualization/BipedalRobotVisualizer.cpp) for a BATCH of robots, kept on the device: a plan - the centroidal states
 * and inputs on a shooting grid - turned into task-space quantities for EVERY node: the base path, the paths of the four contact points, the
 * centre of pressure, the contact forces' sum; where the plan puts the feet down next (FUTURE FOOTHOLDS); and a SUMMARY row per robot, so that a
 * fleet can be watched without moving node rows.  Nothing reaches the host unless it is asked for.  A process that never creates the handle
 * launches nothing of this.  N = max_nodes of the handle; every output has the leading dimension max_batch.
 *   node rows, two blocks [max_batch][N + 1][BPMPC_PLAN_NODE_STRIDE = 24] doubles, OPTIMIZED (from the states x) and DESIRED (from the node
 *   references xref).  Row of robot b, node k <= n_nodes[b]:
 *       0..2      base position x_k[6:9]
 *       3..14     world positions of the model's four contact points at q = x_k[6:12 + nj]; tree, contact frames and order are the WBC's, as in
 *                 the tracking telemetry
 *       15..17    centre of pressure: sum_z = ((fz_0 + fz_1) + fz_2) + fz_3 with fz_i = u_k[3 i + 2]; with sum_z > 0 per component
 *                 ((w_0 p_0 + w_1 p_1) + w_2 p_2) + w_3 p_3, w_i = fz_i / sum_z, over all four points; else 0.  This is getCenterOfPressureMarker
 *                 of VisualizationHelpers.h as recalled ([OCS2-upstream], unpinned: the file is not part of the reference tree)
 *       18        t_k
 *       19        mode of node k (the entry of the grid's mode table; -1 for the last node, which has none)
 *       20        kind of node k (0 intermediate, 1 pre-event; -1 for the last node)
 *       21        sum_z
 *       22        the contact flags of the mode as a bit mask, bit i for contact point i (points 0, 1 the left foot, 2, 3 the right foot: modes
 *                 FLY 0, LF 3, RF 12, STANCE 15; 0 for the last node)
 *       23        1 when an entry of the node's state (any of its 12 + nj) is not finite, else 0.  The entries 0..17 of such a row are unspecified
 *     The last node has no input: its entries 15..17 and 21 are 0, as are those of a plan without inputs (u == NULL).  Rows beyond n_nodes[b] and
 *     robots beyond the batch are not written.  Sums of products are formed without multiply-add contraction.
 *     The desired block is publishDesiredTrajectory (:170-228) evaluated at the SHOOTING NODES instead of at the points of the target trajectories:
 *     the same row with xref in the place of x, entries 15..17 and 21 zero.  A reference exists for the nodes that carry a cost, 0 .. n_nodes - 1;
 *     the desired row of node n_nodes is not written.  A source without references (a policy slot, xref == NULL) leaves the block as it is.
 *   future footholds, [max_batch][BPMPC_PLAN_MAX_FOOTHOLDS = 16][6] doubles (t, contact point i, x, y, z, node index) and count[max_batch]:
 *     publishOptimizedStateTrajectory (:277-309) on the grid tables.  Every node k with kind 1 and t_0 < t_k < t_{n_nodes} (strict, as tStart <
 *     eventTimes[event] < tEnd) is an event inside the horizon.  pre = the mode of the nearest intermediate node (kind 0) before k, post = that of the
 *     nearest intermediate node after k, both among the nodes 0 .. n_nodes - 1; without either there is no foothold.  Every contact point with
 *     !flag(pre, i) && flag(post, i) gives one entry, taken from the optimized row of node k + 1, the POST-EVENT node: its time, i, its contact
 *     point i, k + 1.  (The reference interpolates its time trajectory at the event time, where two entries share one time; here the post-event
 *     node is taken.)  Entries are ordered by (k, i).  count is the true number; only the first 16 entries are stored, and slots behind the count
 *     keep what they held.
 *   summary, [max_batch][BPMPC_PLAN_SUMMARY_STRIDE = 16] doubles from the optimized rows of the nodes 0 .. n_nodes:
 *       0         n_nodes (a device n_nodes as clamped)
 *       1         the foothold count
 *       2         base path length, the sum of sqrt((dx dx + dy dy) + dz dz) over consecutive nodes k, k + 1
 *       3..6      apex of each contact point: the largest z over the nodes
 *       7..10     stance drift of each contact point: the largest sqrt(dx dx + dy dy) between two consecutive nodes whose modes both hold the
 *                 point in contact (the masks of entry 22; 0 when there are none)
 *       11        the smallest sum_z over the intermediate nodes whose mode has a contact (0 when there are none)
 *       12        the number of rows flagged not finite
 *       13..15    reserved, 0
 *     A flagged row is counted in entry 12 and takes part in nothing else, nor does a path segment or a drift with a flagged end.  Comparisons
 *     are > and <: a sum_z that is not a number changes nothing.  Order: 64 accumulators; node k, k ascending, updates accumulator k mod 64 (its
 *     segment and drift are those to node k + 1); the path length is the sum of the accumulators' path lengths, accumulator 0, 1, .. 63; maxima,
 *     minimum and count are exact in any order.  An apex or minimum that nothing contributed to is 0.
 *   sources of a plan.  All describe it alike: x [.][in_N + 1][nx], u [.][in_N][nu], node times [.][in_N + 1], kinds and modes [.][in_N], a node
 *   count, and a grid index per robot.
 *     bpmpc_plan_update_from_solver: the current iterate of the solver's last setup (after a run: the solution), its grid tables through the
 *       robots' grid indices, and its node references.  Enqueued on the SOLVER's stream behind what is there; the handle's stream and the solver's
 *       are ordered by events, so a read may follow without a synchronise; nothing is copied to the host and nothing synchronises.  The solver's
 *       arrays do not change.  BPMPC_ERR_INVALID_ARGUMENT: no setup yet, a solver of another robot or on another device; BPMPC_ERR_CAPACITY: the
 *       batch of the setup above max_batch, the solver's max_nodes above N; BPMPC_ERR_UNSUPPORTED: the DDP solver (its solution lives on the time
 *       points of its own roll-out).
 *     bpmpc_plan_update_from_policy: the FRONT slot of a policy buffer, what the ticks run on, on the BUFFER's stream, ordered the same way; the
 *       grid index is the identity.  A slot holds no references: the desired block is not written.  BPMPC_ERR_INVALID_ARGUMENT until the buffer
 *       holds an adopted policy for every robot (as a buffered tick) and for another robot or device; BPMPC_ERR_CAPACITY as above.
 *     bpmpc_plan_update: the stand-alone entry, as bpmpc_telemetry_update.  One row per robot with the HANDLE's strides: n_nodes [batch],
 *       t [batch][N + 1], x [batch][N + 1][nx], u [batch][N][nu] nullable, mode and kind [batch][N], xref [batch][N][nx] nullable.  Host arrays
 *       (inputs_on_device == 0) are copied first and the call synchronises; device pointers are only enqueued on the handle's stream.  A host
 *       n_nodes outside 1 .. N is refused (BPMPC_ERR_INVALID_ARGUMENT, "n_nodes[b]" in bpmpc_last_error()) before anything is enqueued; a device
 *       n_nodes is clamped into 0 .. N by the kernel.  BPMPC_ERR_CAPACITY above max_batch.
 *   bpmpc_plan_create: max_batch < 1 or max_nodes < 1: BPMPC_ERR_INVALID_ARGUMENT, before a device is looked for; BPMPC_ERR_NO_DEVICE without a
 *     GPU.  The outputs start as zeros.  The handle owns a stream.  Destroy it before the solvers and buffers it was updated from.
 *   bpmpc_plan_dims: max_batch, N and the three strides, each nullable.
 *   bpmpc_plan_configure: how an update is launched - 1: one kernel, a workgroup per robot; 2: a kernel over the node tiles and a second one for
 *     footholds and summary; 0 (after create): the handle chooses.  The outputs do not depend on it.
 *   bpmpc_plan_device_outputs: where the outputs live.
 *   bpmpc_plan_get_nodes (which: 0 optimized, 1 desired; [batch][N + 1][24]), bpmpc_plan_get_footholds ([batch][16][6], [batch]) and
 *     bpmpc_plan_get_summary ([batch][16]): host copies for the first `batch` robots, each pointer nullable; they synchronise the handle's stream.
 *   bpmpc_plan_rows_host: host only, no device: rows [n_nodes + 1][24], footholds [16][6], count [1] and summary [16] (each nullable) of ONE robot
 *     from t [n_nodes + 1], x [n_nodes + 1][nx], u [n_nodes][nu] (nullable), mode and kind [n_nodes], compiled from the text the kernels are
 *     compiled from; the sines and cosines are the host library's.
 *   Null handles and required pointers: BPMPC_ERR_INVALID_ARGUMENT ("null" and the function's name in bpmpc_last_error()).
 *   Not reproduced: the tf broadcast and joint states (:133-162 publishes the observation; node 0 of a plan that starts at the observation holds
 *     its base and contact points), marker colours and scales, the support-polygon message, the rate limit of maxUpdateFrequency.
 * ------------------------------------------------------------------------------------------------------------- */
#define BPMPC_PLAN_NODE_STRIDE 24
#define BPMPC_PLAN_MAX_FOOTHOLDS 16
#define BPMPC_PLAN_SUMMARY_STRIDE 16
typedef struct bpmpc_plan bpmpc_plan;
typedef struct {
  double* optimized;      /* [max_batch][N + 1][24] */
  double* desired;        /* [max_batch][N + 1][24] */
  double* footholds;      /* [max_batch][16][6] */
  double* summary;        /* [max_batch][16] */
  int* foothold_count;    /* [max_batch] */
} bpmpc_plan_outputs;
int bpmpc_plan_create(const bpmpc_model* model, int device, int max_batch, int max_nodes, bpmpc_plan** out);
void bpmpc_plan_destroy(bpmpc_plan* plan);
int bpmpc_plan_dims(const bpmpc_plan* plan, int* max_batch, int* max_nodes, int* node_stride, int* max_footholds, int* summary_stride);
int bpmpc_plan_configure(bpmpc_plan* plan, int launches);
int bpmpc_plan_update_from_solver(bpmpc_plan* plan, bpmpc_solver* solver);
int bpmpc_plan_update_from_policy(bpmpc_plan* plan, bpmpc_policy* policy);
int bpmpc_plan_update(bpmpc_plan* plan, int batch, const int* n_nodes, const double* t, const double* x, const double* u, const int* mode,
                      const int* kind, const double* xref, int inputs_on_device);
int bpmpc_plan_device_outputs(bpmpc_plan* plan, bpmpc_plan_outputs* out);
int bpmpc_plan_get_nodes(bpmpc_plan* plan, int batch, int which, double* host_rows);
int bpmpc_plan_get_footholds(bpmpc_plan* plan, int batch, double* host_entries, int* host_counts);
int bpmpc_plan_get_summary(bpmpc_plan* plan, int batch, double* host_rows);
int bpmpc_plan_rows_host(const bpmpc_model* model, int n_nodes, const double* t, const double* x, const double* u, const int* mode, const int* kind,
                         double* rows, double* footholds, int* count, double* summary);

/* ---------------------------------------------------------------------------------------------------------------
 * Supervisor = which controller drives which robot of a BATCH, decided on the device.  The reference has three pieces for it:
 *   InitialJointPositionController::update  bipedal_controllers/src/InitialJointController.cpp:110-141: holds the robot at defaultJointState,
 *                                           clamped to the URDF limits, with its own joint gains                              -> state INIT
 *   SafetyChecker::check + stopRequest      SafetyChecker.h:39-52, BipedalController.cpp:232-236: stops a robot that tilts    -> RUN to STOPPED
 *   switch_joint_init_pos_controller.py     bipedal_controllers/script: the operator hands a settled robot to the MPC         -> bpmpc_supervisor_request
 * A handle of its own (bpmpc_supervisor) with one kernel, k_supervise; a loop without it keeps its bits and its call time.
 *   state per robot (leading dimension max_batch):
 *     state[b]    BPMPC_SUP_INIT 0, BPMPC_SUP_RUN 1, BPMPC_SUP_STOPPED 2; after create every robot is in INIT
 *     elapsed[b]  seconds in the current state: the sum of the `period`s of its updates
 *     settled[b]  seconds the settle test has held without a break
 *     cause[b]    why the robot was stopped, a bit mask: 1 |roll| above the limit, 2 |pitch| above the limit, 4 base below the height limit,
 *                 8 a measurement that is not finite, 16 a RUN command that is not finite or is missing, 64 stop asked for by the caller
 *     unsafe[b]   the same bits as the last update evaluated them, in every state
 *     ready[b]    0 or 1
 *     q_latch[b][nj] and a latch-pending flag: the measured joints at the first update after entering INIT
 *     counts[8]   robots in INIT, in RUN, in STOPPED, with ready, with unsafe != 0 among the `batch` robots of the last update; the rest 0
 *   parameter row, BPMPC_SUP_PARAM_STRIDE doubles per robot, every row starting from the keys supervisor.<name> of the task file (an absent key
 *   or a NULL path: the default):
 *     [0] tilt_limit       pi/3 (SafetyChecker.h:41)  unsafe if |zyx[2]| > limit (bit 1) or |zyx[1]| > limit (bit 2); strict, as the reference
 *     [1] min_base_height  0    bit 4 if > 0 and position z < it                                          (this engine's extension)
 *     [2] ramp_time        0    seconds over which INIT moves from the latched joints to the target       (extension; 0: the reference's jump)
 *     [3] settle_pos_tol   0    rad        [4] settle_vel_tol  0  rad/s        [5] settle_time  0  s       (extension: the operator's judgement)
 *     [6] stop_kd          0    damping gain of a stopped robot                                           (extension)
 *     [7] reserved, written as 0
 *   five joint rows per robot, nj entries each (`which`): 0 q_init (default: the model's default_joint_state), 1 kp_init and 2 kd_init (default:
 *     the start-up values of the reference's reconfigure server for this controller, cfg/InitialJointControllerParams.cfg: 80 / 5 per leg motor,
 *     kd 3 for the sixth motor of a 12-joint robot), 3 lower and 4 upper (default: the URDF limits, bpmpc_model_get "joint_lower" / "joint_upper").
 *   bpmpc_supervisor_get_params / set_params / reset_params and set_joint_rows / get_joint_rows: masks, n_rows and host / device semantics are
 *     exactly those of bpmpc_wbc_get_params / set_params / reset_params (robot < 0: the start values).  Host rows are validated and a bad entry
 *     is named in bpmpc_last_error(): every used entry finite; limits, tolerances, times and gains not negative; tilt_limit > 0; lower <= upper
 *     against the robot's other limit, +-infinity allowed for these two rows only.  Device rows are not validated.  bpmpc_supervisor_load_params
 *     (row[8]) / check_params: the ingest and the row validation as host-only functions.
 *   bpmpc_supervisor_request: one masked launch on the supervisor's stream, enqueued at once like a restart (mask NULL: every robot below batch).
 *     Target INIT or STOPPED applies to every robot of the mask.  Target RUN applies only to robots that are in INIT, and with only_ready != 0
 *     only to those with ready == 1; the others are left unchanged bit for bit.  Entering any state sets elapsed = settled = 0 and ready = 0;
 *     entering INIT or RUN sets cause = 0; entering INIT sets latch-pending; entering STOPPED by request sets cause = 64.
 *   bpmpc_supervisor_update: counts zeroed on the stream, then one launch of k_supervise; per robot b < batch and in this order:
 *     1. the measurement rbd = [zyx, position, joints, angular velocity, linear velocity, joint velocities] gives `unsafe`: bits 1, 2, 4 as in the
 *        table; bit 8 if any of the 2 (6 + nj) entries is not finite; bit 16 if the robot is in RUN and run_cmd is NULL or any of its five
 *        entries of any joint is not finite.  The reference's comparisons let a NaN pass; bit 8 is this engine's addition.
 *     2. RUN and unsafe != 0: the robot goes to STOPPED with cause = unsafe, elapsed = settled = 0.  This is stopRequest.  The reference still
 *        sends that tick's command and stops at the next cycle; here the stop command goes out in the same update.  Nothing else moves by itself.
 *     3. elapsed += period.
 *     4. the command (pos_des, vel_des, tau_ff, kp, kd per joint):
 *        RUN      the five entries of run_cmd, bit for bit.
 *        INIT     if latch-pending, q_latch = the measured joints (a non-finite entry becomes q_init) and the flag is cleared.
 *                 s = 1 if ramp_time == 0 or elapsed >= ramp_time, else elapsed / ramp_time.  target_j = q_init_j if s == 1 (selected, not
 *                 computed), else q_latch_j + s (q_init_j - q_latch_j), each operation rounded once.  pos_des_j = target_j clamped in the
 *                 reference's order: above upper -> upper, else below lower -> lower.  vel_des = 0, kp = kp_init, kd = kd_init, tau_ff = 0
 *                 (InitialJointController.cpp:114-124).  The settle test: s == 1, unsafe == 0, every |q_j - pos_des_j| <= settle_pos_tol and
 *                 every |v_j| <= settle_vel_tol.  If it holds, settled += period, else settled = 0; ready = (settled >= settle_time) while the
 *                 test holds, else 0.
 *        STOPPED  pos_des_j = the measured q_j (0 if not finite), vel_des = 0, kp = 0, kd = stop_kd, tau_ff = 0; ready = 0.
 *     5. counts.  Robots at or beyond `batch` do not change by one bit.
 *     run_cmd (nullable) has the layout of bpmpc_plant_step's command ([batch*nj] each; base_force and feet_heights are not read).  Host arrays
 *     (inputs_on_device == 0) make the call synchronise; device arrays only enqueue.  period must be finite and positive.
 *   bpmpc_supervisor_update_controlled: run_cmd is the controller's last tick where the tick wrote it (joint_cmd [b][3][nj], the joint gains
 *     [b][nj]), rbd the estimator's device buffer or, with estimator NULL, rbd_dev.  The supervisor's stream waits for the tick and for the
 *     estimator's pending update; the controller's stream and the estimator's wait for the update before they overwrite what it read.  batch must
 *     be the batch of the controller's last tick.  Nothing synchronises.
 *   bpmpc_plant_step_supervised: bpmpc_plant_step_controlled with the supervisor's five command arrays and its stream in the two waits; the plant
 *     kernels are those of every other step.
 *   bpmpc_supervisor_device_outputs: the buffers where they live, and the supervisor's stream.  bpmpc_supervisor_get_state / get_commands: host copies for the first `batch`
 *     robots (counts: 8 ints), every pointer nullable; they synchronise the supervisor's stream.  Nothing else synchronises unless a host
 *     pointer asks for it.
 *   bpmpc_supervisor_rows_host: host only, no device: one update of ONE robot from the text the kernel is compiled from.  params [8]; joint_rows
 *     [5][nj] in the order of `which`; rbd [2 (6 + nj)]; run_cmd nullable, [nj] per member; flags [5] = state, cause, unsafe, ready,
 *     latch-pending and clocks [2] = elapsed, settled and q_latch [nj] are read and updated; command [5][nj] = pos_des, vel_des, tau_ff, kp, kd.
 *   batch > max_batch: BPMPC_ERR_CAPACITY.  Null handles: BPMPC_ERR_INVALID_ARGUMENT ("null" in bpmpc_last_error()).
 *   The settle-then-start loop:
 *     request(INIT)                                                        (after create this is already so)
 *     loop: step_supervised -> update(rbd = plant rbd, run_cmd = NULL)     until counts[3] == B   (a 32-byte fetch every n ticks)
 *     controller_restart(mask = ready, on device) -> setup_commands(x0 = NULL) -> run -> tick_estimated
 *     request(mask = NULL, RUN, only_ready = 1)
 *     loop: step_supervised -> update_from_plant -> tick_estimated -> update_controlled      (a robot that tilts is STOPPED on the device)
 *   Not reproduced: UpperJointController; the tick's own `safe` flag is unchanged.  The plant has end stops of its own since its joint model
 *     (bpmpc_plant_set_joint_params); the clamp here is unchanged by them and clamps the command, not the joint.
 * ------------------------------------------------------------------------------------------------------------- */
#define BPMPC_SUP_PARAM_STRIDE 8
#define BPMPC_SUP_INIT 0
#define BPMPC_SUP_RUN 1
#define BPMPC_SUP_STOPPED 2
typedef struct bpmpc_supervisor bpmpc_supervisor;
typedef struct {
  double *pos_des, *vel_des, *tau_ff, *kp, *kd;       /* [max_batch][nj] each: the layout of bpmpc_joint_command */
  int *state, *cause, *unsafe, *ready;                /* [max_batch] */
  int *counts;                                        /* [8] */
  double *elapsed;                                    /* [max_batch] */
  void *stream;                                       /* the supervisor's stream (a hipStream_t): what a caller orders or times its own work against */
} bpmpc_supervisor_outputs;
int bpmpc_supervisor_create(const bpmpc_model* model, const char* task_info_path, int device, int max_batch, bpmpc_supervisor** out);
void bpmpc_supervisor_destroy(bpmpc_supervisor* supervisor);
int bpmpc_supervisor_get_params(const bpmpc_supervisor* supervisor, int robot, double* row);
int bpmpc_supervisor_set_params(bpmpc_supervisor* supervisor, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device);
int bpmpc_supervisor_reset_params(bpmpc_supervisor* supervisor);
int bpmpc_supervisor_load_params(const char* task_info_path, double* row);
int bpmpc_supervisor_check_params(const double* rows, int n_rows);
int bpmpc_supervisor_set_joint_rows(bpmpc_supervisor* supervisor, int batch, const int* mask, int which, const double* rows, int n_rows,
                                    int inputs_on_device);
int bpmpc_supervisor_get_joint_rows(const bpmpc_supervisor* supervisor, int robot, int which, double* row);
int bpmpc_supervisor_request(bpmpc_supervisor* supervisor, int batch, const int* mask, int target, int only_ready, int inputs_on_device);
int bpmpc_supervisor_update(bpmpc_supervisor* supervisor, int batch, const double* rbd, const bpmpc_joint_command* run_cmd, int inputs_on_device,
                            double period);
int bpmpc_supervisor_update_controlled(bpmpc_supervisor* supervisor, bpmpc_controller* controller, bpmpc_estimator* estimator, const double* rbd_dev,
                                       int batch, double period);
int bpmpc_supervisor_device_outputs(bpmpc_supervisor* supervisor, bpmpc_supervisor_outputs* dev_out);
int bpmpc_supervisor_get_state(bpmpc_supervisor* supervisor, int batch, int* state, int* cause, int* unsafe, int* ready, double* elapsed, int* counts);
int bpmpc_supervisor_get_commands(bpmpc_supervisor* supervisor, int batch, double* pos_des, double* vel_des, double* tau_ff, double* kp, double* kd);
int bpmpc_supervisor_rows_host(const bpmpc_model* model, const double* params, const double* joint_rows, const double* rbd,
                               const bpmpc_joint_command* run_cmd, double period, int* flags, double* clocks, double* q_latch, double* command);
int bpmpc_plant_step_supervised(bpmpc_plant* plant, bpmpc_supervisor* supervisor, int batch, double period, int substeps, const double* base_force,
                                const double* feet_heights, int inputs_on_device);

#ifdef __cplusplus
}
#endif
#endif /* BPMPC_H */
