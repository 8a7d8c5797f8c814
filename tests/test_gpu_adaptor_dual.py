"""HipSqpSolver::getStateInputEqualityConstraintLagrangian EXECUTED: integration/mock_dual.cpp links integration/HipSqpSolver.h against libbpmpc.so with
the labelled stand-ins of integration/mock_ocs2 in place of OCS2, runs one solve with Settings::createDualSolution and asks for the multipliers at a
node time, between two nodes and behind the horizon.  What the adaptor hands back must be the first `rows` entries of what
bpmpc_solver_evaluate_dual returns on the same handle, bit for bit (the adaptor only re-packs it); with the setting off the call throws what it threw
before.  This checks the adaptor's logic; it pins nothing about OCS2 (mock_ocs2/README.md)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adaptor_lagrangian_is_the_abis_and_off_still_throws(tmp_path):
    exe = str(tmp_path / "mock_dual")
    lib = os.path.join(ROOT, "bipedal_control_amd")
    inc = [os.path.join(ROOT, d) for d in ("include", "integration", os.path.join("integration", "mock_ocs2"))]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + [a for i in inc for a in ("-I", i)] + [os.path.join(ROOT, "integration", "mock_dual.cpp"),
                   "-L", lib, "-lbpmpc", "-Wl,-rpath," + lib, "-o", exe], check=True)
    out = subprocess.run([exe, os.path.join(ROOT, "assets", "h1"), "h1_mpc.urdf"], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(out) == 4
    for i, line in enumerate(out[:3]):
        w = line.split()
        assert w[0] == "query" and int(w[1]) == i
        rows_adaptor, rows_abi, diff, norm = int(w[3]), int(w[4]), float(w[6]), float(w[8])
        assert rows_adaptor == rows_abi and rows_abi in (12, 14, 16), line      # an intermediate node of a trot: single or double stance, or flight
        assert diff == 0.0 and norm > 0.0, line
    assert out[3] == "off [HipSqpSolver] getStateInputEqualityConstraintLagrangian() not available yet."
