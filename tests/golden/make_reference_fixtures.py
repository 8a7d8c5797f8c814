#!/usr/bin/env python3
"""Copy the reference's robot data files that the CPU tests compare the reduced assets against into tests/golden/reference/
(same relative paths), and record the function names its OCS2 headers declare (ocs2_interfaces.json) for
tests/test_ocs2_dump.py.  Data only: URDF descriptions and INFO settings, no program text.
Run from the repo root:  python tests/golden/make_reference_fixtures.py <checkout of zitongbai/bipedal_control>"""
import json
import os
import re
import shutil
import sys

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference")
DATA = ["bipedal_robot_example/unitree_h1/h1_description/urdf/h1_with_sole.urdf",
        "bipedal_robot_example/unitree_h1/h1_ocs2_config/config/task/task.info",
        "bipedal_robot_example/unitree_h1/h1_ocs2_config/config/command/reference.info",
        "bipedal_robot_example/unitree_h1/h1_ocs2_config/config/command/gait.info",
        "bipedal_robot_example/hunter/legged_hunter_description/urdf/hunter.urdf",
        "bipedal_robot_example/hunter/legged_hunter_config/config/task/task.info",
        "bipedal_robot_example/hunter/legged_hunter_config/config/command/reference.info",
        "bipedal_robot_example/unitree_g1/g1_description/g1.urdf"]
HEADERS = ["ocs2_bipedal_robot/include/ocs2_bipedal_robot/BipedalRobotInterface.h",
           "ocs2_bipedal_robot/include/ocs2_bipedal_robot/gait/ModeSequenceTemplate.h",
           "ocs2_bipedal_robot/include/ocs2_bipedal_robot/gait/GaitSchedule.h"]


def main(ref):
    for rel in DATA:
        dst = os.path.join(HERE, rel)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        shutil.copyfile(os.path.join(ref, rel), dst)
    names = {}
    for rel in HEADERS:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ref, rel)).read(), flags=re.S)      # the licence block
        names[rel] = sorted(set(re.findall(r"\b([A-Za-z_]\w*)\s*\(", text)))
    with open(os.path.join(HERE, "ocs2_interfaces.json"), "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
