// TEST-ONLY: the filter line search's decision code (kernels/linesearch.h) under the lane emulation, on caller-supplied numbers.  Included by hostemu.cpp
// (the library the Python tests load) and by linesearch_driver.cpp (a stand-alone program that can be built with -fsanitize=address,undefined).
#pragma once
#include <cstddef>
#include <vector>

#include "../../bipedal_control_amd/csrc/kernels/linesearch.h"

using namespace bpmpc;

// The filter line search of one problem on caller-supplied numbers: linesearch_begin, then linesearch_decide once per trial table until the
// problem is done or the tables run out.  NL = lanes of the deciding workgroup (64: the reference kernels; 256: k_ls_decide; 512: k_ls_tail).
template <int NJ, int NL>
static int run_linesearch(const ProblemLS& p0, const LineSearchSettings& st, int n_rounds, const double* trial_tables) {
  std::vector<double> partial(3 * (NL > kWave ? NL : kWave) + 5, 0.0);
  ProblemLS p = p0;
  linesearch_begin<NJ>(partial.data(), p);
  int rounds = 0;
  while (rounds < n_rounds && !p.done[0]) {
    p.trial_perf = trial_tables + (size_t)rounds * p.n_nodes * 3;
    linesearch_decide<NJ, NL>(partial.data(), p, st);
    ++rounds;
  }
  return rounds;
}

extern "C" {

// settings[9]: g_max, g_min, alpha_decay, alpha_min, gamma_c, armijo_factor, delta_tol, cost_tol, max_iterations.
// state[4] in / out: done, active, iterations, remaining.  out[4]: alpha, base[3].  stats[kStatsStride] is written where the kernel writes it.
// Returns the number of decide rounds that ran (the caller reads state[0] to see whether the search ended), -1 for an unknown nj / lanes.
int emu_linesearch(int nj, int lanes, int n_nodes, int n_rounds, const double* node_perf, const double* trial_tables, const double* x0, double* x,
                   double* u, const double* dx, const double* du, const double* summary, const double* settings, int* state, double* stats,
                   double* out) {
  const LineSearchSettings st{settings[0], settings[1], settings[2], settings[3], settings[4], settings[5], settings[6], settings[7], (int)settings[8]};
  ProblemLS p{n_nodes, node_perf, nullptr, x0, x, u, dx, du, summary, out + 1, out, state, state + 1, state + 2, stats, state + 3};
#define BPMPC_EMU_LS(NJ_, NL_) if (nj == NJ_ && lanes == NL_) return run_linesearch<NJ_, NL_>(p, st, n_rounds, trial_tables)
  BPMPC_EMU_LS(10, 64); BPMPC_EMU_LS(10, 256); BPMPC_EMU_LS(10, 512);
  BPMPC_EMU_LS(12, 64); BPMPC_EMU_LS(12, 256); BPMPC_EMU_LS(12, 512);
#undef BPMPC_EMU_LS
  return -1;
}

}  // extern "C"
