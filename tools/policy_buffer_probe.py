#!/usr/bin/env python3
"""What the policy buffer (include/bpmpc.h "Policy buffer") costs and what it buys.  One process, one box; H1, horizon 100, batch 256 and 4096.

  (a) publish   k_policy_publish between events attached to its own dispatch (bpmpc_solver_kernel_time("policy_publish") under profile 1), with
                feedback and without, against a device-to-device copy of the same byte count in the same process (torch events around
                Tensor.copy_, which also bracket the event packets; `empty_launch_us` is that pair around a one-element fill).  Acceptance:
                publish <= copy + the copy's own spread (max - min over the repeats) + one empty launch.  Bytes are the live nodes of every robot,
                counted once (as many are read as written).
  (b) the loop  step_controlled -> update_from_plant -> tick_estimated every tick, setup_commands(x0 = NULL) + run (+ publish(skip_failed = 1))
                every M ticks, update(wait = 1) D ticks later, for D = 0 and D = M / 2, against the same calls without a buffer on a library built
                from the parent commit (--parent-lib).  The tick fetches its outputs, which waits for the controller's stream only: the host
                time from the step to the outputs is what a robot would see.  Mean and worst over `periods` MPC periods, the re-arming call
                (setup_commands + run + publish, host time) beside them, and where in its period the worst tick falls (0: right behind the
                re-arming call).  No ratio is asked for; the streams the loop holds are counted.
  (c) detached  the tick of a controller of this tree that has no buffer attached against the parent's tick: torch events on the solver's
                stream, interleaved repeats, spread = max - min of the parent's repeat medians; the wbc_solution must agree bit for bit.
Every step runs under its own time limit (a watchdog that ends the process even inside a blocked HIP call); the first failure ends the run.
One JSON line per measurement and a summary line on stdout and in --out (default profiles/policy_buffer_probe.jsonl).
usage (GPU box, repository root): python tools/policy_buffer_probe.py --parent-lib /path/to/parent/libbpmpc.so [--batches 256,4096]
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

NI = 100


class Fleet:
    """solver, WBC, controller, estimator and plant of B robots standing at the initial state; `buffered`: a PolicyBuffer attached"""

    def __init__(self, B, lib, buffered=False, feedback=None, stream=None, loop=True):
        import numpy as np
        import bipedal_control_amd as bp
        from bipedal_control_amd import scenarios as sc
        self.np, self.lib, self.B = np, lib, B
        self.itf = itf = sc.interface("h1")
        self.H = NI * sc.DT
        self.gaits = [bp.loadModeSequenceTemplate(itf.gaitFile, "stance")]
        self.mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=sc.max_nodes_for(NI, self.H), return_gains=True, feedback_policy=feedback, stream=stream)
        self.nj = nj = itf.actuatedDofNum
        self.wbc = bp.WeightedWbc(itf, max_batch=B)
        self.ctrl = bp.BatchedController(self.mpc, self.wbc)
        self.pol = None
        if buffered:
            self.pol = bp.PolicyBuffer(self.mpc, B)
            self.ctrl.attachPolicy(self.pol)
        if loop:
            self.est = bp.BatchedStateEstimate(itf, kind="from_topic", max_batch=B)
            self.plant = bp.BatchedPlant(itf, max_batch=B)
        if loop:        # the standing robots of the loop of tests/test_gpu_plant.py
            from oracle import wbc_py as wp
            from tests import oracle_bridge as ob
            from tests.test_plant_reference import standing_state
            m = ob.model("h1")
            q, v, _ = standing_state(m, depth=0.0025)
            rng = np.random.default_rng(5)
            noise = 0.002 * rng.standard_normal((B, len(q))) * np.r_[np.zeros(6), np.ones(len(q) - 6)]
            self.rbd0 = np.array([wp.rbd_from(m, q + noise[b], v) for b in range(B)])
            self.x0 = np.tile(itf.getInitialState(), (B, 1))
            self.x0[:, 6:] = np.c_[self.rbd0[:, 3:6], self.rbd0[:, 0:3], self.rbd0[:, 6:6 + nj]]
            self.ctrl.setJointGains(np.full(nj, bp.WbcParams.RECONFIGURE_MOTOR_KP), np.full(nj, bp.WbcParams.RECONFIGURE_MOTOR_KD))
        else:
            self.x0 = sc.perturbed_initial_states(itf, B)
            q = self.x0[:, 6:]
            self.rbd0 = np.concatenate([q[:, 3:6], q[:, 0:3], q[:, 6:], np.zeros((B, 6 + nj))], axis=1)

    def arm(self, t, first):
        self.mpc.setup_commands(t, self.x0 if first else None, self.gaits, -1, 0.0, self.np.zeros(4), horizon=self.H, from_previous=not first)
        self.mpc.enqueue()

    def close(self):
        for k in ("pol", "ctrl", "plant", "est", "wbc", "mpc"):      # the controller detaches before the buffer goes, the solver last
            if k == "pol" and self.pol is not None:
                self.ctrl.attachPolicy(None)
            if hasattr(self, k):
                delattr(self, k)
                gc.collect()


def live_bytes(f, feedback):
    """bytes a full publish moves each way: the live nodes of every robot"""
    nx = f.mpc.nx
    n = f.np.array([s.n_nodes for s in f.mpc.fetch()[4]], dtype=f.np.int64)
    per = ((n + 1) * nx + n * nx + (n * nx * nx if feedback else 0)) * 8 + (n + 1) * 8 + 2 * n * 4 + 4
    return int(per.sum())


def event_pair_us(torch, stream, work, repeats):
    out = []
    with torch.cuda.stream(stream):
        for _ in range(repeats + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            work()
            b.record(stream)
            b.synchronize()
            out.append(1e3 * a.elapsed_time(b))
    return out[1:]


def probe_publish(args, api, torch, B, feedback):
    import numpy as np
    rec = dict(part="a", robot="h1", horizon=NI, batch=B, feedback=bool(feedback), repeats=args.repeats)
    with step("publish fleet, batch %d" % B, args.step_limit):
        f = Fleet(B, api.load_library(), buffered=True, feedback=feedback, loop=False)
        f.arm(0.0, True)
        f.mpc.synchronize()
        rec["bytes_each_way"] = nbytes = live_bytes(f, feedback)
    with step("publish kernel, batch %d" % B, args.step_limit):
        us = []
        for r in range(args.repeats + 2):
            f.mpc.set_profile(1)
            f.pol.publish()
            f.mpc.set_profile(0)
            ms, n = f.mpc.kernel_time("policy_publish")
            assert n == 1, n
            f.pol.update()
            if r >= 2:
                us.append(1e3 * ms)
        rec["publish_us"], rec["publish_us_min"], rec["publish_us_max"] = float(np.median(us)), min(us), max(us)
        rec["publish_GBps_each_way"] = nbytes / (rec["publish_us"] * 1e-6) / 1e9
    with step("copy of the same bytes, batch %d" % B, args.step_limit):
        stream = torch.cuda.Stream()
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").random_()
        dst = torch.empty_like(src)
        one = torch.zeros(1, device="cuda")
        torch.cuda.synchronize()
        cp = event_pair_us(torch, stream, lambda: dst.copy_(src), args.repeats)
        empty = event_pair_us(torch, stream, lambda: one.fill_(1.0), args.repeats)
        rec["copy_us"], rec["copy_spread_us"], rec["empty_launch_us"] = float(np.median(cp)), max(cp) - min(cp), float(np.median(empty))
        rec["copy_GBps_each_way"] = nbytes / (rec["copy_us"] * 1e-6) / 1e9
        rec["publish_minus_copy_us"] = rec["publish_us"] - rec["copy_us"]
        rec["within_allowance"] = bool(rec["publish_minus_copy_us"] <= rec["copy_spread_us"] + rec["empty_launch_us"])
        del src, dst
    f.close()
    return rec


def run_loop(f, api, torch, periods, M, D):
    """host time from the step to the fetched tick outputs, per tick; the re-arming calls beside them"""
    import numpy as np
    buffered = f.pol is not None
    with library(api, f.lib):
        f.plant.set_state(f.rbd0)
        f.arm(0.0, True)
        if buffered:
            f.pol.publish()
            f.pol.update()
        out = f.ctrl.tick(np.zeros(f.B), f.plant.get_state(), period=0.002)
        tick_us, arm_us, armed = [], [], None
        for k in range(periods * M):
            t0 = time.perf_counter()
            f.plant.step_controlled(f.ctrl, period=0.002, substeps=4)
            f.est.update_from_plant(f.plant, period=0.002, fetch=False)
            out = f.ctrl.tick_estimated(np.full(f.B, 0.002 * (k + 1)), f.est, period=0.002)
            t1 = time.perf_counter()
            tick_us.append(1e6 * (t1 - t0))
            if k % M == M - 1:
                f.arm(0.002 * (k + 1), False)
                if buffered:
                    f.pol.publish(skip_failed=True)
                    armed = k
                arm_us.append(1e6 * (time.perf_counter() - t1))
            if buffered and armed is not None and k == armed + D:
                f.pol.update()
                armed = None
        f.mpc.synchronize()
    tick_us = tick_us[M:]                              # the first period warms everything up
    worst_after_arm = [int(np.argmax(tick_us[i:i + M])) for i in range(0, len(tick_us), M)]      # 0: the tick right behind the re-arming call
    return dict(worst_tick_of_period=worst_after_arm, ticks_after_arm_mean_us=float(np.mean(tick_us[0::M])),
                other_ticks_mean_us=float(np.mean([x for i, x in enumerate(tick_us) if i % M])), tick_mean_us=float(np.mean(tick_us)), tick_worst_us=float(np.max(tick_us)), tick_median_us=float(np.median(tick_us)),
                arm_mean_us=float(np.mean(arm_us[1:])), safe_robots=int(out["safe"].sum()), unsolved_qps=int(out["wbc_status"].sum()))


def probe_loop(args, api, torch, parent, B):
    recs = []
    mine = api.load_library()
    cases = ([("parent, no buffer", parent, False, 0)] if parent is not None else []) + [("this tree, no buffer", mine, False, 0), ("buffer, D = 0", mine, True, 0),
                                                                                         ("buffer, D = M / 2", mine, True, args.m // 2)]
    for name, lib, buffered, D in cases:
        with step("loop '%s', batch %d" % (name, B), args.step_limit):
            with library(api, lib):
                f = Fleet(B, lib, buffered=buffered)
            rec = dict(part="b", robot="h1", horizon=NI, batch=B, loop=name, M=args.m, D=D, periods=args.periods)
            rec.update(run_loop(f, api, torch, args.periods + 1, args.m, D))
            # created: the solver's and its producer stream (idle unless pipeline_chunks > 1), the WBC's (idle in this loop), the estimator's, the
            # plant's, and the buffer's; carrying work: the solver's, the estimator's, the plant's, the buffer's.  Against 4 hardware queues by default
            rec["streams_created"], rec["streams_working"] = (6, 4) if buffered else (5, 3)
            with library(api, lib):
                f.close()
            recs.append(rec)
            print(json.dumps(rec), flush=True)
    return recs


def probe_detached(args, api, torch, parent, B):
    import numpy as np
    rec = dict(part="c", robot="h1", horizon=NI, batch=B, ticks=args.ticks, repeats=args.repeats)
    stream = torch.cuda.Stream()
    fleets = {}
    with step("detached fleets, batch %d" % B, args.step_limit):
        for k, lib in (("parent", parent), ("detached", api.load_library())):
            with library(api, lib):
                f = fleets[k] = Fleet(B, lib, stream=stream.cuda_stream, loop=False)
                f.arm(0.0, True)
                f.mpc.synchronize()
        pol = None
        with library(api, api.load_library()):      # a buffer that was attached once and is gone again: the path a user takes back
            import bipedal_control_amd as bp
            pol = bp.PolicyBuffer(fleets["detached"].mpc, B)
            fleets["detached"].ctrl.attachPolicy(pol)
            fleets["detached"].ctrl.attachPolicy(None)
        t_dev = torch.full((B,), 0.0025, dtype=torch.float64, device="cuda")
        r_dev = torch.tensor(fleets["detached"].rbd0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

    def ticks(f, n):
        ms = []
        with library(api, f.lib):
            for _ in range(n):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                f.ctrl.tick(t_dev, r_dev, fetch=False)
                b.record(stream)
                f.mpc.synchronize()
                ms.append(a.elapsed_time(b))
        return ms

    with step("bit identity, batch %d" % B, args.step_limit):
        sols = {}
        for k, f in fleets.items():
            ticks(f, 1)
            with library(api, f.lib):
                o = api._TickOutputs()
                api._check(f.lib.bpmpc_controller_device_outputs(f.ctrl._h, C.byref(o)))
            sols[k] = api.DeviceArray(C.cast(o.wbc_solution, C.c_void_p).value, (B, f.wbc.numDecisionVars), "<f8").torch().clone()
        rec["same_bits_as_parent"] = bool(torch.equal(sols["parent"], sols["detached"]))
    med = {k: [] for k in fleets}
    with step("timing, batch %d" % B, args.step_limit):
        for f in fleets.values():
            ticks(f, 5)
        for _ in range(args.repeats):
            for k, f in fleets.items():
                med[k].append(1e3 * float(np.median(ticks(f, args.ticks))))
    for k in med:
        rec[k + "_us_repeat_medians"] = med[k]
        rec[k + "_us"] = float(np.median(med[k]))
    rec["parent_spread_us"] = max(med["parent"]) - min(med["parent"])
    rec["detached_within_spread_of_parent"] = bool(rec["detached_us"] <= max(med["parent"]))
    del pol
    gc.collect()
    for k in list(fleets):
        with library(api, fleets[k].lib):
            fleets.pop(k).close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libbpmpc.so built from the parent commit; without it the parent's loop of (b) and all of (c) are left out")
    ap.add_argument("--batches", default="256,4096")
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--m", type=int, default=10, help="ticks per MPC period")
    ap.add_argument("--periods", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_buffer_probe.jsonl"))
    args = ap.parse_args()
    import torch
    from bipedal_control_amd import abi, api
    api.load_library()
    parent = None
    if args.parent_lib:
        with step("load parent library", 60):
            parent = abi.bind(C.CDLL(os.path.abspath(args.parent_lib)), strict=False)      # the parent exports less than the header declares
            if hasattr(parent, "bpmpc_policy_create"):
                raise SystemExit("--parent-lib already has bpmpc_policy_create: not the parent commit's library")
    lines = []
    for B in [int(b) for b in args.batches.split(",")]:
        if "a" in args.parts:
            for feedback in (True, False):
                lines.append(probe_publish(args, api, torch, B, feedback))
                print(json.dumps(lines[-1]), flush=True)
        if "b" in args.parts:
            lines += probe_loop(args, api, torch, parent, B)
        if "c" in args.parts and parent is not None:
            lines.append(probe_detached(args, api, torch, parent, B))
            print(json.dumps(lines[-1]), flush=True)
    summary = dict(summary=True, device=torch.cuda.get_device_name(0), parts=args.parts, parent=parent is not None,
                   publish_within_allowance=[r["within_allowance"] for r in lines if r["part"] == "a"],
                   detached_within_spread_of_parent=[r["detached_within_spread_of_parent"] for r in lines if r["part"] == "c"],
                   same_bits_as_parent=[r["same_bits_as_parent"] for r in lines if r["part"] == "c"])
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for rec in lines + [summary]:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
