#!/usr/bin/env python3
"""Cost of the per-robot parameter rows and joint gains in the controller tick (include/bpmpc.h "Run-time parameters").

One process; H1 at batch 1, 256 and 4096; the dispatch-event method of tools/controller_tick_probe.py (torch events on the solver's stream around
each tick, device inputs, no host outputs).  Per batch three fleets are timed in interleaved repeats, so that drift hits them alike:
  a  the tick of a library built from the parent commit (--parent-lib: its libbpmpc.so, loaded beside this tree's)
  b  the tick of this tree, no row set
  c  the tick of this tree with a distinct row per robot (every used entry scaled by its own factor in 0.8 .. 1.2) and non-zero joint gains
  c0 as c, but every robot's row holds the task.info values: the same QPs as a and b, so what is left is the cost of the mechanism (the table
     and gain reads) without the different work that different parameters give the QPs
  c1 as c, but every robot carries the row that robot 0 has in c: whether the time follows the parameter values rather than their being distinct
(qp_iterations_*: the active-set iterations of b and c on the tick's own WBC inputs, from the debug block of bpmpc_wbc_update)
and, once, bpmpc_wbc_set_params for the full batch from device rows (host clock: enqueue, and enqueue + the synchronising get_params).
The spread of (a) is max - min of its per-repeat medians.  Acceptance: median(b) <= max(a); median(c) - median(a) <= spread + the time of reading
one 256-byte row per robot at the device-to-device copy bandwidth measured here (c0 likewise).  The fleets of this tree must also reproduce the parent's
wbc_solution bit for bit while no row is set.
Every step runs under its own time limit (a watchdog that ends the process even inside a blocked HIP call); the first failure ends the run.
One JSON line per batch and a summary line on stdout and in --out (default profiles/wbc_params_probe.jsonl).
usage (GPU box, repository root): python tools/wbc_params_probe.py --parent-lib /path/to/parent/libbpmpc.so [--batches 1,256,4096] [--ticks 40] [--repeats 5]
"""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.probekit import library, step      # noqa: E402

NI = 40


def fleet(B, stream, lib):
    import numpy as np
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    itf = sc.interface("h1")
    horizon = NI * sc.DT
    tm = [bp.loadModeSequenceTemplate(itf.gaitFile, "trot")]
    x0 = sc.perturbed_initial_states(itf, B)
    cmd = np.tile(np.array([0.2, 0.0, 0.0, 0.0]), (B, 1))
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=sc.max_nodes_for(NI, horizon), return_gains=True, stream=stream)
    mpc.setup_commands(0.0, x0, tm, np.zeros(B, np.int32), sc.GAIT_START, cmd, horizon=horizon)
    mpc.enqueue()
    mpc.synchronize()
    wbc = bp.WeightedWbc(itf, max_batch=B)
    ctrl = bp.BatchedController(mpc, wbc)
    nj = itf.actuatedDofNum
    q = x0[:, 6:]
    rbd = np.concatenate([q[:, 3:6], q[:, 0:3], q[:, 6:], np.zeros((B, 6 + nj))], axis=1)     # at rest at the planned configuration: every QP is solved
    return dict(itf=itf, mpc=mpc, wbc=wbc, ctrl=ctrl, rbd=rbd, nj=nj, lib=lib)


def copy_bandwidth(torch, stream, nbytes=1 << 28, repeats=5):
    src = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    best = None
    with torch.cuda.stream(stream):
        for _ in range(repeats + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            dst.copy_(src)
            b.record(stream)
            b.synchronize()
            ms = a.elapsed_time(b)
            best = ms if best is None else min(best, ms)
    return nbytes / (best * 1e-3)          # bytes read per second (as many are written beside them)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libbpmpc.so built from the parent commit; without it (a) and the acceptance are left out")
    ap.add_argument("--batches", default="1,256,4096")
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wbc_params_probe.jsonl"))
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("the spread of (a) needs at least three repeats")
    import numpy as np
    import torch
    from bipedal_control_amd import abi, api
    mine = api.load_library()
    parent = None
    if args.parent_lib:
        with step("load parent library", 60):
            parent = abi.bind(C.CDLL(os.path.abspath(args.parent_lib)), strict=False)      # the parent exports less than the header declares
            if hasattr(parent, "bpmpc_wbc_set_params"):
                raise SystemExit("--parent-lib already has bpmpc_wbc_set_params: not the parent commit's library")
    stream = torch.cuda.Stream()
    with step("copy bandwidth", 60):
        bw = copy_bandwidth(torch, stream)
    lines = []
    for B in [int(b) for b in args.batches.split(",")]:
        rec = dict(robot="h1", batch=B, ticks=args.ticks, repeats=args.repeats, copy_bandwidth_GBps=bw / 1e9)
        with step("setup batch %d" % B, args.step_limit):
            fleets = {}
            for k, lib in (("a", parent), ("b", mine), ("c", mine), ("c0", mine), ("c1", mine)):
                if lib is not None:
                    with library(api, lib):
                        fleets[k] = fleet(B, stream.cuda_stream, lib)
            t_dev = torch.full((B,), 0.0025, dtype=torch.float64, device="cuda")
            r_dev = torch.tensor(fleets["b"]["rbd"], dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()

        def ticks(f, n, timed):
            ms = []
            with library(api, f["lib"]):
                for _ in range(n):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    f["ctrl"].tick(t_dev, r_dev, fetch=False)
                    b.record(stream)
                    f["mpc"].synchronize()
                    if timed:
                        ms.append(a.elapsed_time(b))
            return ms

        with step("bit identity at batch %d" % B, args.step_limit):
            ticks(fleets["b"], 1, False)
            ticks(fleets["c"], 1, False)
            sol = {k: fleets[k]["ctrl"].device_outputs()["wbc_solution"].torch().clone() for k in ("b", "c")}
            rec["unsolved"] = int(fleets["b"]["ctrl"].device_outputs()["wbc_status"].torch().sum().item())
            if "a" in fleets:
                ticks(fleets["a"], 1, False)
                with library(api, parent):          # the parent's ABI ends before bpmpc_controller_joint_outputs: read its buffer through its own call
                    o = api._TickOutputs()
                    api._check(parent.bpmpc_controller_device_outputs(fleets["a"]["ctrl"]._h, C.byref(o)))
                view = api.DeviceArray(C.cast(o.wbc_solution, C.c_void_p).value, (B, fleets["a"]["wbc"].numDecisionVars), "<f8").torch()
                rec["same_bits_as_parent"] = bool(torch.equal(view, sol["b"]) and torch.equal(view, sol["c"]))
        with step("rows and gains at batch %d" % B, args.step_limit):
            f = fleets["c"]
            rng = np.random.default_rng(2)
            rows = np.tile(f["wbc"].getParams(-1), (B, 1))
            rows[:, :19 + f["nj"] // 2] *= rng.uniform(0.8, 1.2, (B, 19 + f["nj"] // 2))        # a distinct row per robot
            rows_d = torch.tensor(rows, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            enq, full = [], []
            for _ in range(20):
                t0 = time.perf_counter()
                f["wbc"].setParams(rows_d)
                t1 = time.perf_counter()
                f["wbc"].getParams(0)
                t2 = time.perf_counter()
                enq.append(1e6 * (t1 - t0))
                full.append(1e6 * (t2 - t0))
            rec["set_params_device_rows_enqueue_us"] = float(np.median(enq))
            rec["set_params_device_rows_enqueue_and_sync_us"] = float(np.median(full))
            same = torch.tensor(np.tile(f["wbc"].getParams(-1), (B, 1)), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            fleets["c0"]["wbc"].setParams(same)
            fleets["c0"]["wbc"].getParams(0)          # synchronises: `same` may go
            fleets["c1"]["wbc"].setParams(rows[0])
            for k in ("c", "c0", "c1"):
                fleets[k]["ctrl"].setLegMotorGains(np.full(f["nj"] // 2, 80.0), np.full(f["nj"] // 2, 5.0))
            # the work of the active-set iteration with and without the distinct rows, on the tick's own WBC inputs (the debug block of bpmpc_wbc_update)
            o = fleets["b"]["ctrl"].device_outputs()
            xo, uo, md = (o[k].torch().cpu().numpy() for k in ("x_opt", "u_opt", "planned_mode"))
            nv = 6 + f["nj"]
            for k in ("b", "c"):
                dbg = fleets[k]["wbc"].update(xo, uo, fleets[k]["rbd"], md, debug=True)[2]
                it = dbg[:, nv * nv + nv + 12 * nv + 19]
                rec["qp_iterations_" + k] = dict(mean=float(it.mean()), max=float(it.max()))
        med = {k: [] for k in fleets}
        with step("warm-up at batch %d" % B, args.step_limit):
            for f in fleets.values():
                ticks(f, args.warmup, False)
        for r in range(args.repeats):
            for k, f in fleets.items():
                with step("repeat %d of %s at batch %d" % (r, k, B), args.step_limit):
                    med[k].append(float(np.median(ticks(f, args.ticks, True))))
        rec["unsolved_with_rows"] = int(fleets["c"]["ctrl"].device_outputs()["wbc_status"].torch().sum().item())
        if rec["unsolved"] or rec["unsolved_with_rows"]:          # the fallback leaves k_wbc early: not the work this probe is about
            raise SystemExit("batch %d: %d / %d QPs not solved" % (B, rec["unsolved"], rec["unsolved_with_rows"]))
        for k in med:
            rec[k + "_us_repeat_medians"] = [1e3 * x for x in med[k]]
            rec[k + "_us"] = 1e3 * float(np.median(med[k]))
        rec["row_read_us"] = 1e6 * B * 256 / bw
        if "a" in med:
            rec["a_spread_us"] = 1e3 * (max(med["a"]) - min(med["a"]))
            rec["b_within_spread_of_a"] = bool(rec["b_us"] <= 1e3 * max(med["a"]))
            rec["c_within_allowance"] = bool(rec["c_us"] - rec["a_us"] <= rec["a_spread_us"] + rec["row_read_us"])
            rec["c0_within_allowance"] = bool(rec["c0_us"] - rec["a_us"] <= rec["a_spread_us"] + rec["row_read_us"])
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del rows_d, same, f
        for k in list(fleets):                      # destroyed by the library that created them, the controller first
            with library(api, fleets[k]["lib"]):
                fleets.pop(k).clear()
                gc.collect()
    summary = dict(summary=True, accepted=all(r.get("b_within_spread_of_a") and r.get("c_within_allowance") and r.get("same_bits_as_parent") for r in lines)
                   if parent is not None else None,
                   mechanism_accepted=all(r.get("b_within_spread_of_a") and r.get("c0_within_allowance") and r.get("same_bits_as_parent") for r in lines)
                   if parent is not None else None, device=torch.cuda.get_device_name(0))
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for rec in lines + [summary]:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
