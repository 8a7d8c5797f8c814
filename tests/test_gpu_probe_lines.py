"""The measurement probes under tools/ keep the fields of their JSON lines: profiles/*.jsonl are appended to across commits and compared by
field.

One case per probe at the smallest shape (H1, batch 1; 2 timed samples, 1 warm-up, 1 repeat; no --parent-lib, no --profile): the probe runs as
a child process under `timeout -k 10`, must end with status 0 and must print one line per expected variant, and the set of field names of each
line must be the one in tests/golden/probe_fields.json[probe][variant].  That file was recorded once from the probes as they stood before they
moved onto tools/probekit.py, with the arguments below; it is not rewritten from the tree under test.  No timing is asserted.

Not here, because their run is a long simulation that the command line cannot skip: plant_stand_probe, supervisor_settle_probe, the sweep of
plant_body_probe (--no-sweep below) and --estimate of plant_sensor_probe.  wbc_params_probe and policy_buffer_probe are not here either: one
process that builds four to five fleets per batch and needs three repeats for its spread, tens of seconds at their smallest.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 120
SMALL = ["--shapes", "h1:1", "--warmup", "1"]
BLOCKS = SMALL + ["--samples", "2", "--block", "2", "--repeats", "1"]
CASES = {
    "plant_probe": SMALL + ["--ticks", "2"],
    "plant_sensor_probe": SMALL + ["--ticks", "2", "--repeats", "1"],
    "plant_input_probe": BLOCKS,
    "plant_joint_probe": BLOCKS,
    "plant_body_probe": BLOCKS + ["--no-sweep"],
    "supervisor_probe": ["--batches", "1", "--calls", "2", "--block", "2"],
    "telemetry_probe": SMALL + ["--ticks", "2", "--repeats", "1"],
    "plan_geometry_probe": ["--batches", "1", "--calls", "2", "--runs", "2"],
    "controller_tick_probe": SMALL + ["--ticks", "2"],
    "estimator_probe": SMALL + ["--ticks", "2", "--repeats", "1"],
}


def label(line):
    """what tells the lines of one probe apart: its variant, the way plan_geometry_probe launches, or nothing (one line)"""
    return str(line.get("variant", line.get("launches", "line")))


def run_probe(tools, probe, args=None, limit=LIMIT):
    """(exit status, the JSON lines on stdout) of tools/<probe>.py with the case's arguments"""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(tools, probe + ".py")] + (CASES[probe] if args is None else args)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
    return r.returncode, [json.loads(t) for t in r.stdout.splitlines() if t.startswith("{")]


@pytest.mark.parametrize("probe", sorted(CASES))
def test_probe_line_fields(probe):
    with open(os.path.join(ROOT, "tests", "golden", "probe_fields.json")) as f:
        golden = json.load(f)[probe]
    status, lines = run_probe(os.path.join(ROOT, "tools"), probe)
    assert status == 0
    assert sorted(label(line) for line in lines) == sorted(golden)
    for line in lines:
        assert sorted(line) == golden[label(line)], label(line)
