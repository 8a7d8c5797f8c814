// Executes HipSqpSolver::getStateInputEqualityConstraintLagrangian against libbpmpc.so with the stand-ins of integration/mock_ocs2 in place of OCS2
// (see mock_ocs2/README.md: this checks the ADAPTOR'S logic, it pins nothing about OCS2).  References as in mock_value.cpp.  One solve with
// Settings::createDualSolution, then the query at three times - a node time, between two nodes, behind the horizon - and a state off the plan, beside
// bpmpc_solver_evaluate_dual on the same handle: one line per query, "query <i> rows <adaptor> <abi> nu <largest difference> norm <largest |nu|>".
// Last line: what a solver created WITHOUT the setting says, "off <message>".  tests/test_gpu_adaptor_dual.py reads them.
//   build: g++ -std=c++17 -I include -I integration -I integration/mock_ocs2 integration/mock_dual.cpp -L bipedal_control_amd -lbpmpc -Wl,-rpath,... -o mock_dual
//   run:   ./mock_dual assets/h1 h1_mpc.urdf
#include <cmath>
#include <cstdio>
#include <string>

#include "HipSqpSolver.h"

namespace {
struct FixedReferences final : ocs2::ReferenceManagerInterface {
  ocs2::ModeSchedule ms;
  ocs2::TargetTrajectories tt;
  const ocs2::ModeSchedule& getModeSchedule() const override { return ms; }
  const ocs2::TargetTrajectories& getTargetTrajectories() const override { return tt; }
};
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: mock_dual <asset dir> <urdf file name>\n"); return 2; }
  const std::string dir = argv[1];
  const std::string urdf = dir + "/" + argv[2], task = dir + "/task.info", reference = dir + "/reference.info", gaitfile = dir + "/gait.info";
  try {
    bpmpc_model* model = nullptr;
    if (bpmpc_model_create(urdf.c_str(), task.c_str(), reference.c_str(), &model) != 0) throw std::runtime_error(bpmpc_last_error());
    int nx = 0, nu = 0;
    bpmpc_model_dims(model, &nx, &nu, nullptr, nullptr);
    ocs2::vector_t x0(nx);
    bpmpc_model_get(model, "initial_state", x0.data(), nx);
    const double horizon = 0.3;                                // 20 intervals of 0.015 s and the gait events inside them
    auto refs = std::make_shared<FixedReferences>();
    {
      bpmpc_gait* gait = nullptr;
      bpmpc_gait_create(model, &gait);
      double sw[16]; int modes[16], n_modes = 0;
      if (bpmpc_gait_load_template(gaitfile.c_str(), "trot", sw, modes, 16, &n_modes) != 0) throw std::runtime_error(bpmpc_last_error());
      bpmpc_gait_insert_template(gait, sw, modes, n_modes, -1.225, 3 * horizon);
      double ev[512]; int md[513], n_ev = 0;
      if (bpmpc_gait_mode_schedule(gait, -horizon, 3 * horizon, ev, md, 512, &n_ev) != 0) throw std::runtime_error(bpmpc_last_error());
      refs->ms.eventTimes.assign(ev, ev + n_ev);
      refs->ms.modeSequence.assign(md, md + n_ev + 1);
      bpmpc_gait_destroy(gait);
    }
    const double cmd[4] = {0.3, 0.0, 0.0, 0.0};
    double tt[2];
    std::vector<double> xs(2 * nx);
    if (bpmpc_cmd_vel_to_targets(model, cmd, 0.0, x0.data(), horizon, tt, xs.data()) != 0) throw std::runtime_error(bpmpc_last_error());
    refs->tt.timeTrajectory.assign(tt, tt + 2);
    for (int p = 0; p < 2; ++p) refs->tt.stateTrajectory.emplace_back(Eigen::Map<const ocs2::vector_t>(&xs[p * nx], nx));
    ocs2::OptimalControlProblem ocp;
    ocs2::bipedal_robot::HipSqpSolver::Settings ss;
    ss.maxNodes = 32;
    ss.createDualSolution = true;
    {
      ocs2::bipedal_robot::HipSqpSolver solver(task, urdf, reference, ocp, ss);
      solver.setReferenceManager(refs);
      solver.run(0.0, x0, horizon);
      ocs2::PrimalSolution primal;
      solver.getPrimalSolution(horizon, &primal);
      const size_t n = primal.timeTrajectory_.size();
      if (n < 8) throw std::runtime_error("too few time points");
      const double times[3] = {primal.timeTrajectory_[4], 0.5 * (primal.timeTrajectory_[6] + primal.timeTrajectory_[7]), horizon + 0.05};
      for (int i = 0; i < 3; ++i) {
        ocs2::vector_t x(primal.stateTrajectory_[5]);
        for (int c = 0; c < nx; ++c) x.data()[c] += 0.01 * ((c + i) % 3 - 1);
        const ocs2::vector_t got = solver.getStateInputEqualityConstraintLagrangian(times[i], x);
        std::vector<double> costate(nx);
        double nu_abi[16];
        int rows = -1;
        if (bpmpc_solver_evaluate_dual(solver.engineHandle(), 1, &times[i], x.data(), 0, costate.data(), nu_abi, &rows) != 0) throw std::runtime_error(bpmpc_last_error());
        double diff = 0, norm = 0;
        for (int r = 0; r < rows && r < static_cast<int>(got.size()); ++r) {
          diff = std::fmax(diff, std::fabs(got.data()[r] - nu_abi[r]));
          norm = std::fmax(norm, std::fabs(got.data()[r]));
        }
        std::printf("query %d rows %d %d nu %.17g norm %.17g\n", i, static_cast<int>(got.size()), rows, diff, norm);
      }
    }
    ss.createDualSolution = false;
    {
      ocs2::bipedal_robot::HipSqpSolver solver(task, urdf, reference, ocp, ss);
      solver.setReferenceManager(refs);
      solver.run(0.0, x0, horizon);
      try {
        solver.getStateInputEqualityConstraintLagrangian(0.0, x0);
        std::printf("off answered\n");
      } catch (const std::runtime_error& e) {
        std::printf("off %s\n", e.what());
      }
    }
    bpmpc_model_destroy(model);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "mock_dual: %s\n", e.what());
    return 1;
  }
  return 0;
}
