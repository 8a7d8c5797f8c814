"""HipSqpSolver::getValueFunction EXECUTED: integration/mock_value.cpp links integration/HipSqpSolver.h against libbpmpc.so with the labelled stand-ins
of integration/mock_ocs2 in place of OCS2, runs one solve with Settings::createValueFunction and asks for the value function at a node time, between
two nodes and behind the horizon.  What the adaptor hands back - f, dfdx, dfdxx - must be what bpmpc_solver_evaluate_value returns on the same handle,
bit for bit (the adaptor only re-packs it); with the setting off the call throws what it threw before.  This checks the adaptor's logic; it pins
nothing about OCS2 (mock_ocs2/README.md)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adaptor_value_function_is_the_abis_and_off_still_throws(tmp_path):
    exe = str(tmp_path / "mock_value")
    lib = os.path.join(ROOT, "bipedal_control_amd")
    inc = [os.path.join(ROOT, d) for d in ("include", "integration", os.path.join("integration", "mock_ocs2"))]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + [a for i in inc for a in ("-I", i)] + [os.path.join(ROOT, "integration", "mock_value.cpp"),
                   "-L", lib, "-lbpmpc", "-Wl,-rpath," + lib, "-o", exe], check=True)
    out = subprocess.run([exe, os.path.join(ROOT, "assets", "h1"), "h1_mpc.urdf"], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(out) == 4
    for i, line in enumerate(out[:3]):
        w = line.split()
        assert w[0] == "query" and int(w[1]) == i
        f_adaptor, f_abi, grad, hess, asym = float(w[3]), float(w[4]), float(w[6]), float(w[8]), float(w[10])
        assert f_adaptor == f_abi and grad == 0.0 and hess == 0.0 and asym == 0.0, line
        if i < 2:
            assert f_adaptor > 0.0, line               # inside the horizon: a cost-to-go
        else:
            assert f_adaptor == 0.0, line              # behind it: V_n = 0, there is no final cost
    assert out[3] == "off [HipSqpSolver] getValueFunction() not available yet."
