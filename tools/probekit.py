"""What the probes under tools/ share: plain functions, nothing to subclass.

  the driver     every measurement of a probe runs in a child process of its own (`<probe> --child <job> <the probe's options>`) under
                 `timeout -k 10 <limit>`, strictly one after the other; the first child that ends with a status other than 0 - a fault, an
                 abort, the time limit - ends the probe, so nothing more is started on the GPU, and only then are the lines published
                 (run_jobs, forwarded, driver_options, child_line)
  libraries      the parent commit's library beside or in place of this tree's (parent_library, use_parent_library, library)
  clocks         step (a watchdog for a step of a one-process probe), host_stats, steps (the plant's drained block of enqueued steps)
  kernel times   kernel_split: a `rocprofv3 --kernel-trace --stats` run of a child of its own, no counters; kernel_stats reads its database;
                 run_child_profiled puts the two together for a probe whose lines carry a `kernels` entry
  scenarios      tick_fleet (a solved batch and its controller), standing / standing_plant (the plant at rest on its soles), IMU_GRADE
torch and the library are imported inside the functions that need them, so that `--help` of a probe needs neither.
"""
import argparse
import faulthandler
import glob
import json
import os
import re
import sqlite3
import subprocess
import sys
import tempfile
import time
from contextlib import contextmanager

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_FORWARDED = ("child", "out", "shapes")
TICK_NI = 40
IMU_GRADE = dict(gyro_noise=2e-3, accel_noise=2e-2, joint_pos_noise=1e-4, delay_steps=1.0)
PERIOD, SUBSTEPS = 0.002, 4      # the closed loops in the plant: 2 ms ticks of 4 substeps
RAMP_TIME, POS_TOL, VEL_TOL, SETTLE_TIME = 0.1, 0.05, 0.5, 0.2      # the supervisor's rows of the settle phase


# ---- the driver

def driver_options(ap, limit):
    """the options every child-per-measurement probe has; `limit`: the probe's own default"""
    ap.add_argument("--commit", help="the commit the library was built from, recorded in every line")
    ap.add_argument("--limit", type=int, default=limit, help="time limit of one child process [s]")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--out")


def forwarded(a):
    """The command line that hands a child every option of the parsed namespace `a` but --child, --out and --shapes: an option that is added
    to a probe reaches its children without being named again.  A flag that is set is passed, an option without a value is left out."""
    args = []
    for dest, value in vars(a).items():
        if dest in NOT_FORWARDED or value is None or value is False:
            continue
        args.append("--" + dest.replace("_", "-"))
        if value is not True:
            args.append(repr(value) if isinstance(value, float) else str(value))
    return args


def run_child(script, job, args, limit):
    """(exit status, last line of stdout) of one child of `script` under its time limit"""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(script), "--child", job] + list(args)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    return r.returncode, (r.stdout.strip().splitlines() or [""])[-1]


def run_jobs(script, jobs, args, limit, out, run=run_child):
    """One child of `script` per job, in sequence; stops at the first that fails or prints no line.  The lines of the jobs before it are
    echoed as they come and appended to `out` at the end.  0 only if every job gave a line.  `run(script, job, args, limit)` -> (status, line)
    replaces the plain child for a probe with jobs of another kind (a profiler run)."""
    name = os.path.splitext(os.path.basename(script))[0]
    lines = []
    for job in jobs:
        status, text = run(script, job, args, limit)
        if status != 0 or not text:      # a fault, an abort or the time limit: nothing more is started on the GPU
            print("%s: %s ended with status %d%s; stopping" % (name, job, status, "" if text else " and no line"), file=sys.stderr)
            break
        print(text, flush=True)
        lines.append(text)
    if out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            for text in lines:
                f.write(text + "\n")
    return 0 if len(lines) == len(jobs) else 1


def child_line(a, line):
    """the child's side: the commit is stamped into the line its measurement returned, and the line is printed"""
    if getattr(a, "commit", None):
        line["commit"] = a.commit
    print(json.dumps(line), flush=True)
    return 0


# ---- libraries

def parent_library(path):
    """an earlier commit's libbpmpc.so, bound without insisting on what it lacks"""
    import ctypes as C
    import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before a library's runtime initialises)
    from bipedal_control_amd import abi
    return abi.bind(C.CDLL(os.path.abspath(path)), strict=False)


def use_parent_library(path):
    """this process calls the parent commit's library from here on"""
    from bipedal_control_amd import api
    api._LIB = parent_library(path)


@contextmanager
def library(api, lib):
    """the Python mirror calls `lib` (a ctypes library with the C ABI) inside: a handle is created, used and destroyed by one library only"""
    mine = api._LIB
    api._LIB = lib
    try:
        yield
    finally:
        api._LIB = mine


# ---- clocks

@contextmanager
def step(name, seconds):
    """a step under its own time limit: past it the traceback of every thread is dumped and the process ends"""
    print("# step %s (limit %d s)" % (name, seconds), file=sys.stderr, flush=True)
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def host_stats(prefix, samples, unit):
    """<prefix>_<unit>_median, _min, _p05 and _p95 of the samples"""
    import numpy as np
    p05, p95 = (float(x) for x in np.percentile(samples, [5, 95]))
    key = "%s_%s_" % (prefix, unit)
    return {key + "median": float(np.median(samples)), key + "min": float(np.min(samples)), key + "p05": p05, key + "p95": p95}


STEPS_CLOCK = "host clock around a drained block of enqueued steps, per step"


def steps(plant, r_dev, cmd, samples, warmup, block, substeps, period):
    """us per bpmpc_plant_step: `block` steps that are only enqueued, a host clock around them and the one-robot get_state that drains the
    plant's stream; the state is set back before every block"""
    import numpy as np
    out = []
    for k in range(warmup + samples):
        plant.set_state(r_dev)
        plant.get_state(1)
        t0 = time.perf_counter()
        for _ in range(block):
            plant.step(*cmd, period=period, substeps=substeps)
        plant.get_state(1)
        dt = time.perf_counter() - t0
        if k >= warmup:
            out.append(1e6 * dt / block)
    return np.array(out)


# ---- kernel times

def kernel_stats(db_path, kernels):
    """({kernel: calls, avg_us, min_us}, every name launched) from the `kernels` table of a rocprofv3 database.  A row belongs to kernel k if
    k stands in its name as a whole word - `k<...>`, `void bpmpc::k<...>(...)`, `...::k<...>` or bare - and the instantiations of one kernel
    are merged: the call-weighted mean and the overall minimum."""
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, count(*), avg(duration), min(duration) from kernels group by name").fetchall()
    db.close()
    split = {}
    for name, calls, avg, mn in rows:
        for k in kernels:
            if re.search(r"(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])" % re.escape(k), name):
                e = split.setdefault(k, dict(calls=0, avg_us=0.0, min_us=float("inf")))
                e["avg_us"] = (e["avg_us"] * e["calls"] + avg / 1e3 * calls) / (e["calls"] + calls)
                e["calls"] += int(calls)
                e["min_us"] = min(e["min_us"], mn / 1e3)
    return split, sorted({n.split("(")[0] for n, *_ in rows})


def kernel_split(script, child_args, kernels, limit):
    """(status, per-kernel averages, names launched) of `python <script> <child_args>` under rocprofv3 --kernel-trace --stats: a run of its
    own with no counters, the time limit in front of the profiler and the program after `--`.  A status other than 0 is a failed job."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--",
               sys.executable, os.path.abspath(script)] + list(child_args)
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            print("rocprofv3 exit %d: %s" % (r.returncode, r.stderr[-400:]), file=sys.stderr)
            return r.returncode or 1, None, None
        return (0,) + kernel_stats(dbs[0], kernels)


def run_child_profiled(kernels, ratio):
    """A `run` for run_jobs: the plain child's line and, where --profile is among the options, the per-kernel averages of one more child of the
    same job under the profiler (at most 20 ticks, 2 of warm-up) as its `kernels`, with avg_us of `ratio[1]` over that of `ratio[2]` as
    `ratio[0]`.  A failed profiler run fails the job."""
    def run(script, job, args, limit):
        status, text = run_child(script, job, args, limit)
        if status != 0 or not text or "--profile" not in args:
            return status, text
        ticks = min(int(args[args.index("--ticks") + 1]), 20)
        status, split, _ = kernel_split(script, ["--child", job, "--ticks", str(ticks), "--warmup", "2"], kernels, limit)
        if status != 0:
            return status, ""
        name, above, below = ratio
        if above in split and below in split:
            split[name] = split[above]["avg_us"] / split[below]["avg_us"]
        return 0, json.dumps(dict(json.loads(text), kernels=split))
    return run


# ---- scenarios

def tick_fleet(robot, B, stream):
    """(solver, controller, rbd): a batch solved once on `stream` (a trot, 40 intervals) and the measurement at rest at the planned
    configuration, where every QP of the tick is solved"""
    import numpy as np
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    itf = sc.interface(robot)
    horizon = TICK_NI * sc.DT
    tm = [bp.loadModeSequenceTemplate(itf.gaitFile, "trot")]
    x0 = sc.perturbed_initial_states(itf, B)
    cmd = np.tile(np.array([0.2, 0.0, 0.0, 0.0]), (B, 1))
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=sc.max_nodes_for(TICK_NI, horizon), return_gains=True, stream=stream)
    mpc.setup_commands(0.0, x0, tm, np.zeros(B, np.int32), sc.GAIT_START, cmd, horizon=horizon)
    mpc.enqueue()
    mpc.synchronize()
    ctrl = bp.BatchedController(mpc, bp.WeightedWbc(itf, max_batch=B))
    nj = itf.actuatedDofNum
    q = x0[:, 6:]
    rbd = np.concatenate([q[:, 3:6], q[:, 0:3], q[:, 6:], np.zeros((B, 6 + nj))], axis=1)
    return mpc, ctrl, rbd


def standing(robot, B):
    """(interface, rbd [B, 2 nv] at rest at the planned configuration with the soles 2.5 mm in the ground, the holding command)"""
    import numpy as np
    from bipedal_control_amd import scenarios as sc
    itf = sc.interface(robot)
    nj = itf.actuatedDofNum
    q = sc.perturbed_initial_states(itf, B)[:, 6:]
    rbd = np.concatenate([q[:, 3:6], q[:, 0:3], q[:, 6:], np.zeros((B, 6 + nj))], axis=1)
    rbd[:, 5] -= 0.0025
    cmd = [rbd[:, 6:6 + nj].copy(), np.zeros((B, nj)), np.zeros((B, nj)), np.full((B, nj), 1000.0), np.full((B, nj), 20.0)]
    return itf, rbd, cmd


def standing_plant(robot, B):
    """(interface, plant, r_dev, cmd): a plant set to `standing` and the state and the holding command as device tensors"""
    import torch
    import bipedal_control_amd as bp
    itf, rbd, cmd = standing(robot, B)
    plant = bp.BatchedPlant(itf, max_batch=B)
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")      # noqa: E731
    r_dev, cmd = dev(rbd), [dev(a) for a in cmd]
    torch.cuda.synchronize()
    plant.set_state(r_dev)
    return itf, plant, r_dev, cmd
