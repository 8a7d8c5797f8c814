#!/usr/bin/env python3
"""Generate tests/golden/kinematics_parent_bits.npz ON AN MI355X: the outputs of the WBC, the estimator, the controller tick, the telemetry and the plan
geometry (both launch modes and its host twin) as they stood before their forward kinematics moved into csrc/kernels/kinematics.h (commit 70b3099), for
the cases of tests/test_gpu_kinematics_parent_bits.py.  The file pins the bits those kernels must go on producing; it is regenerated only from a
checkout of that commit (with this script and that test module copied in), never from a later one.
Run from the repo root: python tests/golden/make_kinematics_parent_bits.py [output directory]"""
import os
import sys
import tempfile

import numpy as np
import torch  # noqa: F401  (before the library's runtime initialises, as in tests/test_gpu_plant.py)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    from tests import test_gpu_kinematics_parent_bits as tk
    out = {}
    with tempfile.TemporaryDirectory() as directory:
        for robot, what in tk.CASES:
            got = tk.record_stock(robot, what) if robot in tk.STOCK else tk.record_tree(robot, what, directory)
            for k, v in got.items():
                out["%s_%s" % (robot, k)] = np.asarray(v)
            print(robot, what, sorted(got), flush=True)
    dest = sys.argv[1] if len(sys.argv) > 1 else HERE
    os.makedirs(dest, exist_ok=True)
    np.savez_compressed(os.path.join(dest, "kinematics_parent_bits.npz"), **out)
    print("written", os.path.join(dest, "kinematics_parent_bits.npz"), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
