#!/usr/bin/env python3
"""What the supervisor costs, one child process per batch on one box (H1, batch 1 / 256 / 4096).

Per batch a child
  (a) times `--calls` bpmpc_supervisor_update from device arrays between two events on the supervisor's stream each - the 32-byte memset of the
      counters and k_supervise - once with every robot in INIT (no command) and once with every robot in RUN (a command passed through): the
      median, the minimum, the 95th percentile; and, between the same events on the same stream, a device-to-device copy that moves as many
      bytes as the RUN update reads and writes (the measurement, the five command rows, the parameter row and the per-robot scalars in; the five
      command rows and the scalars out) as the yardstick of a kernel that only streams;
  (b) times the closed loop's host time per tick - the calls of one tick and a device synchronise behind them - with
      step_controlled -> update_from_plant -> tick_estimated against step_supervised -> update_from_plant -> tick_estimated ->
      update_controlled, alternating in blocks of `--block` ticks in one process on the same handles; every block starts from the same plant
      state with every robot in RUN, the policy is evaluated at one fixed time.
A number of (a) is the time between two events on an otherwise idle stream, so it holds the launch gaps.  Nothing of this is a pass condition
of anything, and no ratio is promised.
One JSON line per batch on stdout; --out appends them to a file (profiles/supervisor_probe.jsonl is where the published one belongs).
Every child runs under a time limit; the first that fails or runs out of time ends the probe.
usage (GPU box, repository root): python tools/supervisor_probe.py [--batches 1,256,4096] [--calls 200] [--commit ID] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probekit as pk      # noqa: E402

PERIOD, SUBSTEPS = 0.002, 4


def measure(B, calls, block):
    import numpy as np
    import torch
    import bipedal_control_amd as bp
    stream = torch.cuda.Stream()
    mpc, ctrl, rbd = pk.tick_fleet("h1", B, stream.cuda_stream)
    itf = mpc.interface
    nj = itf.actuatedDofNum
    sup = bp.BatchedSupervisor(itf, B)
    own = torch.cuda.ExternalStream(sup.stream())
    r_dev = torch.tensor(rbd, dtype=torch.float64, device="cuda")
    cmd = [torch.zeros((B, nj), dtype=torch.float64, device="cuda") for _ in range(5)]
    torch.cuda.synchronize()

    def timed(body, count):
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(count)]
        for e0, e1 in pairs:
            e0.record(own)
            body()
            e1.record(own)
        own.synchronize()
        return np.array([1e3 * e0.elapsed_time(e1) for e0, e1 in pairs])      # us

    pct = lambda v, q: float(np.percentile(v, q))      # noqa: E731
    line = dict(probe="supervisor", robot="h1", batch=B, calls=calls)
    # (a)
    timed(lambda: sup.update(r_dev, None, PERIOD), 20)
    each = timed(lambda: sup.update(r_dev, None, PERIOD), calls)
    line.update(init_update_us_median=float(np.median(each)), init_update_us_min=float(each.min()), init_update_us_p95=pct(each, 95),
                init_counts=sup.state(B)["counts"])
    sup.request(sup.RUN)
    timed(lambda: sup.update(r_dev, cmd, PERIOD), 20)
    each = timed(lambda: sup.update(r_dev, cmd, PERIOD), calls)
    line.update(run_update_us_median=float(np.median(each)), run_update_us_min=float(each.min()), run_update_us_p95=pct(each, 95),
                run_counts=sup.state(B)["counts"])
    scalars = 5 * 4 + 2 * 8
    bytes_read = B * (8 * 2 * (6 + nj) + 5 * 8 * nj + 8 * bp.SupervisorParams.STRIDE + scalars)
    bytes_written = B * (5 * 8 * nj + scalars) + 32
    words = max(1, (bytes_read + bytes_written) // 16)
    src, dst = torch.zeros(words, dtype=torch.float64, device="cuda"), torch.zeros(words, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def copy():
        with torch.cuda.stream(own):
            dst.copy_(src)

    timed(copy, 20)
    each = timed(copy, calls)
    line.update(bytes_read=int(bytes_read), bytes_written=int(bytes_written), copy_bytes_each_way=int(8 * words), copy_us_median=float(np.median(each)),
                copy_us_min=float(each.min()), copy_us_p95=pct(each, 95))
    # (b)
    plant = bp.BatchedPlant(itf, max_batch=B)
    est = bp.BatchedStateEstimate(itf, kind="from_topic", max_batch=B)
    ctrl.setJointGains(np.full(nj, bp.WbcParams.RECONFIGURE_MOTOR_KP), np.full(nj, bp.WbcParams.RECONFIGURE_MOTOR_KD))
    t_dev = torch.full((B,), 0.0025, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    times = {"controlled": [], "supervised": []}

    def start_block(supervised):
        plant.set_state(r_dev)
        ctrl.tick(t_dev, r_dev, period=PERIOD, fetch=False)
        if supervised:
            sup.request(sup.INIT)      # a robot that was stopped in the last block starts over
            sup.request(sup.RUN)
            sup.update_controlled(ctrl, rbd=r_dev, period=PERIOD)
        torch.cuda.synchronize()

    def tick(supervised):
        t0 = time.perf_counter()
        if supervised:
            plant.step_supervised(sup, period=PERIOD, substeps=SUBSTEPS)
        else:
            plant.step_controlled(ctrl, period=PERIOD, substeps=SUBSTEPS)
        est.update_from_plant(plant, period=PERIOD, fetch=False)
        ctrl.tick_estimated(t_dev, est, period=PERIOD, fetch=False)
        if supervised:
            sup.update_controlled(ctrl, est, period=PERIOD)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for supervised in (False, True):      # warm-up
        start_block(supervised)
        for _ in range(block):
            tick(supervised)
    blocks =2 * ((calls + block - 1) // block)
    stopped = 0
    for r in range(blocks):
        supervised = r % 2 == 1
        start_block(supervised)
        for _ in range(block):
            times["supervised" if supervised else "controlled"].append(tick(supervised))
        if supervised:
            stopped = max(stopped, sup.state(B)["counts"]["stopped"])
    for k, v in times.items():
        line.update({"loop_%s_host_ms_median" % k: float(np.median(v)), "loop_%s_host_ms_min" % k: float(np.min(v)), "loop_%s_host_ms_p95" % k: pct(v, 95)})
    line.update(loop_ticks_each=len(times["controlled"]), loop_block=block, loop_most_stopped_in_a_block=int(stopped),
                plant_state_finite=bool(np.isfinite(plant.get_state()).all()))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,256,4096")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--block", type=int, default=20, help="ticks of one variant of the closed loop before the other takes over")
    pk.driver_options(ap, limit=240)
    a = ap.parse_args()
    if a.child:      # one batch, in this process
        return pk.child_line(a, measure(int(a.child), a.calls, a.block))
    return pk.run_jobs(__file__, a.batches.split(","), pk.forwarded(a), a.limit, a.out)


if __name__ == "__main__":
    sys.exit(main())
