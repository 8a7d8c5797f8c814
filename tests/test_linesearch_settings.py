"""The five keys of the sqp block that steer the filter line search ([OCS2-upstream] sqp::loadSettings: alpha_decay, alpha_min, gamma_c, armijoFactor,
costTol): loaded by both ingests and handed out, and values for which the back-tracking sequence 1, alpha_decay, alpha_decay^2, .. >= alpha_min would
not end (or would be longer than 64 trials) refused at model load instead of hanging the solver's trial-counting loop."""
import os

import pytest

import bipedal_control_amd as bp
from bipedal_control_amd import scenarios as sc
from oracle import ingest
from tests import linesearch_cases as lc

UPSTREAM = dict(alpha_decay=0.5, alpha_min=1e-4, gamma_c=1e-6, armijoFactor=1e-4, costTol=1e-4)


@pytest.mark.parametrize("robot", ["h1", "hunter", "openloong", "g1"])
def test_the_shipped_task_files_keep_upstreams_defaults(robot):
    s = sc.interface(robot).sqpSettings()
    assert {k: s[k] for k in UPSTREAM} == UPSTREAM
    files = sc.ROBOTS[robot]
    m = ingest.build_model(files["urdf"], files["task"], files["reference"])
    assert {k: m["sqp"][k] for k in UPSTREAM} == UPSTREAM


def test_accepted_values_round_trip_through_both_ingests(tmp_path):
    want = dict(alpha_decay=0.7, alpha_min=0.05, gamma_c=1.0, armijoFactor=0.9, costTol=0.0, g_max=-1.0, deltaTol=0.0)
    itf = lc.interface("h1", want, tmp_path)
    s = itf.sqpSettings()
    assert {k: s[k] for k in want} == want
    v = itf.get("sqp")
    assert len(v) == 13 and list(v[8:13]) == [0.7, 0.05, 1.0, 0.9, 0.0]          # appended: positions 0 .. 7 keep their meaning
    assert v[0] == 0.015 and v[2] == 0.0 and v[3] == -1.0 and v[6] == 1.0 and v[7] == 0.0
    files = sc.ROBOTS["h1"]
    m = ingest.build_model(files["urdf"], lc.write_task("h1", want, tmp_path), files["reference"])
    assert {k: m["sqp"][k] for k in want} == want
    # the edges of the accepted ranges
    for edge in (dict(alpha_min=1.0), dict(gamma_c=0.0), dict(armijoFactor=0.0), dict(alpha_decay=0.8, alpha_min=0.8 ** 63)):
        s = lc.interface("h1", edge, tmp_path).sqpSettings()
        assert all(s[k] == v for k, v in edge.items())


@pytest.mark.parametrize("settings,named", [
    (dict(alpha_decay=0.0), "alpha_decay"), (dict(alpha_decay=1.0), "alpha_decay"), (dict(alpha_decay=1.5), "alpha_decay"), (dict(alpha_decay=-0.5), "alpha_decay"),
    (dict(alpha_min=0.0), "alpha_min"), (dict(alpha_min=-1e-4), "alpha_min"), (dict(alpha_min=1.5), "alpha_min"),
    (dict(gamma_c=-1e-6), "gamma_c"), (dict(gamma_c=1.5), "gamma_c"),
    (dict(armijoFactor=-1e-4), "armijoFactor"), (dict(armijoFactor=1.0), "armijoFactor"),
    (dict(costTol=-1e-4), "costTol"),
    (dict(alpha_decay=0.8, alpha_min=0.8 ** 64), "alpha_min"),           # 65 trials
    (dict(alpha_decay=0.999), "alpha_decay"), (dict(alpha_min=1e-300), "alpha_min")])
def test_nonsense_is_refused_at_model_load(settings, named, tmp_path):
    with pytest.raises(bp.BpmpcError) as e:
        lc.interface("h1", settings, tmp_path)
    assert e.value.status == -3                      # BPMPC_ERR_UNSUPPORTED (include/bpmpc.h)
    assert "sqp." + named in str(e.value)


def test_write_task_edits_the_sqp_block_only(tmp_path):
    """The helper the device cases rest on: keys the file has are replaced in place, the others are added inside the block, nothing else moves."""
    path = lc.write_task("h1", dict(g_max=1e9, gamma_c=1.0), tmp_path)
    old, new = open(sc.ROBOTS["h1"]["task"]).read().split("\n"), open(path).read().split("\n")
    changed = [(a, b) for a, b in zip(old, [line for line in new if "gamma_c" not in line]) if a != b]
    assert len(new) == len(old) + 1 and len(changed) == 1 and "g_max" in changed[0][0] and "1000000000.0" in changed[0][1]
    assert os.path.dirname(path) == str(tmp_path)
    s = lc.interface("h1", dict(g_max=1e9, gamma_c=1.0), tmp_path).sqpSettings()
    assert s["g_max"] == 1e9 and s["gamma_c"] == 1.0 and s["g_min"] == 1e-6
    assert bp.BipedalRobotInterface(path, sc.ROBOTS["h1"]["urdf"], sc.ROBOTS["h1"]["reference"]).ipmSettings()["g_max"] == 10.0
