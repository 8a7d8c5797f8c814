"""Cost of the device-resident gait schedules: bpmpc_solver_setup_gaits against bpmpc_solver_setup_commands, and the solve behind each,
for one shared history (batch 1, 256, 4096), for a distinct history per robot (batch 256, 4096: one grid per robot, whose node kinds and
times are read back) and per tick of a 256-robot closed loop with gait switches.  Writes profiles/gait_batch_probe.jsonl.
Usage: python tools/gait_batch_probe.py [reps]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bipedal_control_amd as bp  # noqa: E402
from bipedal_control_amd import scenarios as sc  # noqa: E402
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
NI, TICK = 67, 0.02
H = NI * sc.DT
itf = sc.h1_interface()
lib = [bp.loadModeSequenceTemplate(sc.H1["gait"], g) for g in ("stance", "trot", "standing_trot", "flying_trot")]


def median_ms(fn):
    fn()                                                                       # first call: pinned arenas, code objects
    out = []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t))
    return float(np.median(out))


def case(batch, distinct):
    x0 = sc.perturbed_initial_states(itf, batch)
    cmd = np.tile([0.3, 0.0, 0.0, 0.1], (batch, 1))
    gop = np.ones(batch, np.int32)
    start = sc.GAIT_START + (np.arange(batch) * 1e-4 if distinct else np.zeros(batch))
    mpc = bp.BatchedSqpMpc(itf, max_batch=batch, max_nodes=sc.max_nodes_for(NI, H))
    gs = bp.BatchedGaitSchedule(mpc, lib)
    gs.insertModeSequenceTemplate(gop, start, 2 * H)
    state = {"k": 0}

    def commands():
        state["k"] += 1
        mpc.setup_commands(state["k"] * TICK, x0, lib, gop, start, cmd, horizon=H)
        mpc.synchronize()

    def gaits():
        state["k"] += 1
        mpc.setup_gaits(gs, state["k"] * TICK, x0, cmd, horizon=H)
        mpc.synchronize()

    def solve():                                                               # the initial iterate of the setup again, then one run
        mpc.reset()
        mpc.enqueue()
        mpc.synchronize()

    r = dict(case="shared" if not distinct else "distinct", batch=batch)
    r["setup_commands_ms"] = median_ms(commands)
    r["solve_after_commands_ms"] = median_ms(solve)
    r["n_grids_commands"] = mpc.layout()["n_grids"]
    r["setup_gaits_ms"] = median_ms(gaits)
    r["solve_after_gaits_ms"] = median_ms(solve)
    r["n_grids_gaits"] = mpc.layout()["n_grids"]
    return r


def closed_loop(batch=256, ticks=100):
    x0 = sc.perturbed_initial_states(itf, batch)
    cmd = np.tile([0.3, 0.0, 0.0, 0.1], (batch, 1))
    mpc = bp.BatchedSqpMpc(itf, max_batch=batch, max_nodes=sc.max_nodes_for(NI, H), return_gains=True)
    gs = bp.BatchedGaitSchedule(mpc, lib)
    gs.insertModeSequenceTemplate(1, sc.GAIT_START, 2 * H)
    mpc.setup_gaits(gs, 0.0, x0, cmd, horizon=H)
    mpc.enqueue()
    rng = np.random.default_rng(5)
    per_tick = []
    for k in range(1, ticks + 1):
        c = np.where(rng.random(batch) < 0.02, rng.integers(1, 4, batch), -1).astype(np.int32)   # ~5 robots switch per tick
        t = time.perf_counter()
        gs.command(c)
        mpc.rollout(TICK, fetch=False)
        mpc.setup_gaits(gs, k * TICK, None, cmd, horizon=H, from_previous=True)
        mpc.enqueue()
        mpc.synchronize()
        per_tick.append(1e3 * (time.perf_counter() - t))
    lay = mpc.layout()
    return dict(case="closed_loop_switches", batch=batch, ticks=ticks, tick_ms_median=float(np.median(per_tick[5:])),
                tick_ms_p90=float(np.percentile(per_tick[5:], 90)), n_grids_final=lay["n_grids"])


if __name__ == "__main__":
    rows = [case(1, False), case(256, False), case(4096, False), case(256, True), case(4096, True), closed_loop()]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "gait_batch_probe.jsonl"), "w") as f:
        for r in rows:
            r.update(horizon_s=H, n_intervals=NI, reps=REPS)
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))
