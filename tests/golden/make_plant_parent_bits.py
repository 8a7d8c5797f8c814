#!/usr/bin/env python3
"""Generate tests/golden/plant_parent_bits.npz ON AN MI355X: the outputs of k_plant_step as it stood before the plant had stick-slip contacts
(commit a414698), for the five robots of tests/test_gpu_plant.py::_cases after one launch of 20 substeps, H1 and G1.  The file pins the bits a plant
with kt = 0 must go on producing (tests/test_gpu_plant_stiction.py::test_parent_bits); it is regenerated only from a checkout of that commit, never
from a later one.
Run from the repo root: python tests/golden/make_plant_parent_bits.py [output directory]"""
import os
import sys

import numpy as np
import torch  # noqa: F401  (before the library's runtime initialises, as in tests/test_gpu_plant.py)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    from tests import test_gpu_plant as tp
    out = {}
    for robot in ("h1", "g1"):
        plant = tp._plant(robot, tp.B5)
        o = tp._set_and_step(plant, robot, tp.PERIOD, tp.SUBSTEPS)
        out[robot + "_state"] = plant.get_state()
        for k in tp.SENSORS:
            out[robot + "_" + k] = o[k]
    dest = sys.argv[1] if len(sys.argv) > 1 else HERE
    os.makedirs(dest, exist_ok=True)
    np.savez_compressed(os.path.join(dest, "plant_parent_bits.npz"), **out)
    print("written", os.path.join(dest, "plant_parent_bits.npz"), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
