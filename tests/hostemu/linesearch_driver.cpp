// TEST-ONLY: stand-alone driver of emu_linesearch (linesearch_emu.h) for builds with -fsanitize=address,undefined: nothing sanitised is loaded into Python.
// Reads problems from the text file argv[1] and prints one result line per problem (tests/test_hostemu_linesearch.py writes the file and reads the lines).
//   per problem:  nj lanes n_nodes n_rounds active iterations remaining, then the arrays node_perf [3 n], trial tables [n_rounds 3 n], x0 [nx],
//                 x [(n + 1) nx], u [n nx], dx, du, summary [4], settings [9]
//   result line:  rounds done active iterations remaining alpha base[3] stats[16] x.. u..      (%.17g: doubles survive the round trip)
#include <cstdio>
#include <fstream>
#include <string>

#include "linesearch_emu.h"

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: linesearch_driver <cases.txt>\n"); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  auto read = [&in](size_t n) {
    std::vector<double> v(n);
    for (double& d : v) { std::string tok; in >> tok; d = std::stod(tok); }     // stod reads "nan" and "inf", operator>> does not
    return v;
  };
  int nj, lanes, n, rounds, active, iterations, remaining;
  while (in >> nj >> lanes >> n >> rounds >> active >> iterations >> remaining) {
    const int nx = 12 + nj;
    const std::vector<double> node_perf = read(3 * n), tables = read((size_t)rounds * 3 * n), x0 = read(nx);
    std::vector<double> x = read((size_t)(n + 1) * nx), u = read((size_t)n * nx);
    const std::vector<double> dx = read((size_t)(n + 1) * nx), du = read((size_t)n * nx), summary = read(4), settings = read(9);
    int state[4] = {-5, active, iterations, remaining};
    std::vector<double> stats(kStatsStride, -777.0), out(4, 0.0);
    const int ran = emu_linesearch(nj, lanes, n, rounds, node_perf.data(), tables.data(), x0.data(), x.data(), u.data(), dx.data(), du.data(), summary.data(),
                                   settings.data(), state, stats.data(), out.data());
    if (ran < 0 || !in) { std::fprintf(stderr, "bad problem\n"); return 3; }
    std::printf("%d %d %d %d %d", ran, state[0], state[1], state[2], state[3]);
    for (double v : out) std::printf(" %.17g", v);
    for (double v : stats) std::printf(" %.17g", v);
    for (double v : x) std::printf(" %.17g", v);
    for (double v : u) std::printf(" %.17g", v);
    std::printf("\n");
  }
  return 0;
}
