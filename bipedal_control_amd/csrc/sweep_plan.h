// Which kernels a solver handle launches, as plain C++: the eight environment switches (read once, when the handle is created) and the Riccati sweep
// of a batch.  Host-only on purpose - no HIP header, no kernel header - so that tests/test_sweep_plan.py compiles it alone and walks the table.
// A new switch or a new regime goes HERE; solver.hip only maps a Sweep to its launcher.
#pragma once
#include <cstdlib>

namespace bpmpc {

// Riccati sweep by regime: eight waves with fixed roles while every problem has a CU to itself; four-wave workgroups up to two problems per CU;
// beyond that one wavefront per problem (riccati_wave.h at one wave per SIMD up to four problems per CU, riccati_wave2.h at two beyond).
enum class Sweep { EightWave, FourWave, WavePerSimd, TwoWavesPerSimd };

// BPMPC_RICCATI_WAVE: 0 never a wave per problem; 1 (default) as described; 2 riccati_wave.h at every batch size, 4 riccati_wave2.h at every
// batch size (tests); 3 riccati_wave2.h whenever a wave per problem is used
enum class RiccatiWave { Never, Auto, AlwaysOnePerSimd, AutoTwoPerSimd, AlwaysTwoPerSimd };

struct Switches {
  RiccatiWave riccati_wave = RiccatiWave::Auto;           // BPMPC_RICCATI_WAVE
  int r8_rounds = 0;                                       // BPMPC_R8_ROUNDS: rounds of the eight-wave sweep; 0: by the robot, as measured
  int ls_wide_rounds = 2;                                  // BPMPC_LS_WIDE_ROUNDS: line-search rounds that run as launches over all nodes (>= 1)
  bool wt_joint_rows = false;                              // BPMPC_WT_JOINT_ROWS=1: the change of variables always writes the joint rows of Wt (A/B of the byte cut)
  bool lin_tables = false;                                 // BPMPC_LIN_TABLES=1: the table walks also on a robot of two serial legs (tests)
  bool lin_compact = true;                                 // BPMPC_LIN_COMPACT=0: the lineariser keeps the event nodes in line (A/B, tests)
  bool dense_project = false;                              // BPMPC_DENSE_PROJECT=1: the general elimination also where the input weight allows the structured one
  bool dense_weights = false;                              // BPMPC_DENSE_WEIGHTS=1: the cost weights as dense matrices also where their non-zero lists exist (weight_structure.h; A/B, tests)
};

// `get` has the shape of std::getenv (a test passes its own)
inline Switches read_switches(const char* (*get)(const char*)) {
  const auto is = [&](const char* name, char c) { const char* e = get(name); return e && e[0] == c; };
  Switches sw;
  {
    const char* e = get("BPMPC_RICCATI_WAVE");
    const int v = e ? std::atoi(e) : 1;
    sw.riccati_wave = v == 1 ? RiccatiWave::Auto : v == 2 ? RiccatiWave::AlwaysOnePerSimd : v == 3 ? RiccatiWave::AutoTwoPerSimd
                    : v == 4 ? RiccatiWave::AlwaysTwoPerSimd : RiccatiWave::Never;
  }
  { const char* e = get("BPMPC_R8_ROUNDS"); const int v = e ? std::atoi(e) : 0; sw.r8_rounds = v > 0 ? v : 0; }
  { const char* e = get("BPMPC_LS_WIDE_ROUNDS"); const int v = e ? std::atoi(e) : 2; sw.ls_wide_rounds = v < 1 ? 1 : v; }
  sw.wt_joint_rows = is("BPMPC_WT_JOINT_ROWS", '1');
  sw.lin_tables = is("BPMPC_LIN_TABLES", '1');
  sw.lin_compact = !is("BPMPC_LIN_COMPACT", '0');
  sw.dense_project = is("BPMPC_DENSE_PROJECT", '1');
  sw.dense_weights = is("BPMPC_DENSE_WEIGHTS", '1');
  return sw;
}

// The eight-wave sweep holds a CU per problem; a larger batch runs it in ROUNDS (the dispatcher starts a workgroup as a CU becomes free, so the roll-outs
// behind the sweeps no longer stream at the same time).  Since its roll-out goes through the ring (round 6) two and three rounds of it beat what those batch
// sizes ran before on the 22-state robots - batch 512: 0.5447 against 0.5837 ms on the four-wave workgroups, 768: 0.807 against 0.878 on a wave per problem;
// 1024 in four rounds: 1.075 against 0.917, so from there on the wave sweeps - and lose on nx = 24 (G1 / 512: 0.8545 against 0.7682 on the four-wave
// workgroups), whose eight-wave stage is 55 % longer (`experiments/LOG.md`).  BPMPC_R8_ROUNDS overrides (1: the regimes of rounds 3 to 5; tests).
constexpr int kEightWaveRounds10Joints = 3, kEightWaveRoundsOtherwise = 1;
// up to two problems per CU the four-wave workgroups finish in one round (0.61 against 0.91 ms at batch 512); beyond that a wave per
// problem, four per CU, wins (G1 / 1024: 1.30 against 1.54 ms; 4096: 4.07 against 4.53 ms)
constexpr int kFourWaveProblemsPerCu = 2;
// two waves per SIMD (riccati_wave2.h) need eight problems per CU to fill the chip - the dispatcher packs a CU before it opens the next
// one, 1024 problems would occupy half of the CUs - and win from the first batch that takes riccati_wave.h a second round: beyond four
// problems per CU (batch 1024: 0.98 against 1.27 ms; 4096: 3.75 against 3.22 ms)
constexpr int kWavePerSimdProblemsPerCu = 4;

// The sweep that runs `batch` problems of a robot with `nj` joints on `num_cus` compute units.  The eight-wave test comes first: with three rounds
// (10 joints, default) the four-wave workgroups are never chosen.
inline Sweep choose_sweep(int nj, int batch, int num_cus, const Switches& sw) {
  if (sw.riccati_wave == RiccatiWave::AlwaysOnePerSimd) return Sweep::WavePerSimd;
  if (sw.riccati_wave == RiccatiWave::AlwaysTwoPerSimd) return Sweep::TwoWavesPerSimd;
  const int rounds = sw.r8_rounds > 0 ? sw.r8_rounds : (nj == 10 ? kEightWaveRounds10Joints : kEightWaveRoundsOtherwise);
  if (batch <= rounds * num_cus) return Sweep::EightWave;
  if (sw.riccati_wave == RiccatiWave::Never || batch <= kFourWaveProblemsPerCu * num_cus) return Sweep::FourWave;
  if (sw.riccati_wave == RiccatiWave::AutoTwoPerSimd) return Sweep::TwoWavesPerSimd;
  return batch <= kWavePerSimdProblemsPerCu * num_cus ? Sweep::WavePerSimd : Sweep::TwoWavesPerSimd;
}

}  // namespace bpmpc
