#!/usr/bin/env python3
"""What the plan geometry costs, one child process per measurement on one box.

Per shape (H1, a trot, 100 intervals, batch 1 / 256 / 4096) and per way to launch (1: k_plan_fused; 2: k_plan_nodes + k_plan_reduce) a child
  solves the batch once on a stream of its own,
  times `--calls` bpmpc_plan_update_from_solver between two events on that stream each (the median, the minimum, the 95th percentile) and once
    more as one burst of `--calls` between two events (the average with the launches back to back),
  times, between the same events, a device-to-device copy that moves as many bytes as the update reads and writes - the states, inputs and
    references of the live nodes in; both blocks of rows, the footholds and the summary out - as the yardstick of a kernel that only streams,
  and times `--runs` solver runs (setup + run between events) alternately with and without an update behind them.
A number here is the time between two events on the solver's stream, so it holds the launch gaps of a stream that is otherwise idle.  Nothing of
this is a pass condition of anything.
One JSON line per measurement on stdout; --out appends them to a file (profiles/plan_geometry_probe.jsonl is where the published one belongs).
Every child runs under a time limit; the first that fails or runs out of time ends the probe.
usage (GPU box, repository root): python tools/plan_geometry_probe.py [--batches 1,256,4096] [--calls 200] [--commit ID] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probekit as pk      # noqa: E402

NI = 100


def measure(B, launches, calls, runs):
    import numpy as np
    import torch
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    itf = sc.interface("h1")
    prob = sc.trot_problem(itf, B, NI)
    N = NI + 16
    stream = torch.cuda.Stream()
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=N, stream=stream.cuda_stream)

    def setup():
        mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])

    setup()
    mpc.enqueue()
    mpc.synchronize()
    n = int(mpc.fetch()[4][0].n_nodes)
    plan = bp.PlanGeometry(itf, B, N)
    plan.configure(launches)

    def timed(body, count):
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(count)]
        with torch.cuda.stream(stream):
            for e0, e1 in pairs:
                e0.record(stream)
                body()
                e1.record(stream)
        stream.synchronize()
        return np.array([1e3 * e0.elapsed_time(e1) for e0, e1 in pairs])      # us

    timed(lambda: plan.update(mpc), 20)
    each = timed(lambda: plan.update(mpc), calls)
    burst = timed(lambda: [plan.update(mpc) for _ in range(calls)], 1)[0] / calls
    nx = 22
    bytes_read = 8 * B * ((n + 1) * nx + 2 * n * nx + (n + 1) + n)
    bytes_written = 8 * B * ((2 * n + 1) * bp.PlanNode.STRIDE + bp.PlanNode.MAX_FOOTHOLDS * bp.PlanNode.FOOTHOLD_STRIDE + bp.PlanNode.SUMMARY_STRIDE)
    words = (bytes_read + bytes_written) // 16
    src, dst = torch.zeros(words, dtype=torch.float64, device="cuda"), torch.zeros(words, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    timed(lambda: dst.copy_(src), 20)
    copy = timed(lambda: dst.copy_(src), calls)
    with_update, without = [], []
    for r in range(2 * runs + 2):
        setup()
        behind = r % 2 == 1
        dt = timed((lambda: (mpc.enqueue(), plan.update(mpc))) if behind else mpc.enqueue, 1)[0] / 1e3
        if r >= 2:
            (with_update if behind else without).append(dt)
    summ = plan.summary()
    entries, count = plan.footholds()
    pct = lambda v, q: float(np.percentile(v, q))      # noqa: E731
    return dict(probe="plan_geometry", robot="h1", batch=B, n_nodes=n, launches=launches, calls=calls, update_us_median=float(np.median(each)),
                update_us_min=float(each.min()), update_us_p95=pct(each, 95), update_us_burst_avg=float(burst), bytes_read=int(bytes_read),
                bytes_written=int(bytes_written), copy_bytes_each_way=int(8 * words), copy_us_median=float(np.median(copy)), copy_us_min=float(copy.min()),
                run_ms_median=float(np.median(without)), run_ms_with_update_median=float(np.median(with_update)), runs=runs,
                footholds_min=int(count.min()), footholds_max=int(count.max()), summary_finite=bool(np.isfinite(summ).all()),
                base_path_length_mean=float(summ[:, 2].mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,256,4096")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--runs", type=int, default=10)
    pk.driver_options(ap, limit=240)
    a = ap.parse_args()
    if a.child:      # one measurement, in this process
        B, launches = (int(v) for v in a.child.split(":"))
        return pk.child_line(a, measure(B, launches, a.calls, a.runs))
    jobs = ["%s:%d" % (B, launches) for B in a.batches.split(",") for launches in (1, 2)]
    return pk.run_jobs(__file__, jobs, pk.forwarded(a), a.limit, a.out)


if __name__ == "__main__":
    sys.exit(main())
