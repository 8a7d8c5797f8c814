"""What the dual solution of the solve (bpmpc_solver_enable_dual_solution) costs, beside the value function's kernels it runs behind.

Every line is one process of its own: H1, trot tiled from t = 0, `--intervals` shooting intervals (100: the headline grid), one SQP iteration per
run from the same cold setup, `--steps` runs after `--warmup`.
  kernels:B   a handle with the feature on, profile level 1: k_dual_node between events attached to its dispatch (kernel class "dual"), beside
              k_value_terms of the same runs - the yardstick: the same order of bytes and products per node, plus the small rank-deficient solve.
              node_over_terms = the ratio.  node_GBs = the algorithmic bytes of k_dual_node - per intermediate node 7 nx^2 + 22 nx + 16 nx doubles
              read (S_k, S+, Acl, B, R, P, K; the vectors; D), 16 (nx + 2) + nx + 5 written - over its time, beside the write roof of this box
              (tools/probes/write_roof.hip, as bench.py runs it).  The certificates of the last run ride along: the largest residual / |g_u| and
              gain residual / |Hux| over the batch.
  onoff:B     ONE handle with the value function on; its runs alternate between the dual solution off and on, and a host clock stands around enqueue
              + wait of every run: median and spread per state, on_minus_off.

usage (GPU box, repository root): python tools/dual_solution_probe.py [--shapes 1,256,4096] [--commit ID] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probekit as pk      # noqa: E402

SHAPES = "1,256,4096"
STATES = ("value_only", "dual_on")


def _handle(B, intervals, profile):
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    itf = sc.h1_interface()
    horizon = intervals * sc.DT
    prob = sc.trot_problem(itf, batch=B, n_intervals=intervals, gait_start=0.0)
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=sc.max_nodes_for(intervals, horizon), sqp_iterations=1, profile=profile, return_gains=True)
    return itf, prob, mpc


def _run(mpc, prob):
    mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    t0 = time.perf_counter()
    mpc.enqueue()
    mpc.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _base(B, itf, intervals, steps, warmup, mpc):
    return dict(probe="dual_solution", robot="h1", batch=B, intervals=intervals, nodes=mpc.layout()["n_nodes_max"], steps=steps, warmup=warmup, nx=itf.stateDim)


def kernels(B, intervals, steps, warmup):
    import bench
    itf, prob, mpc = _handle(B, intervals, True)
    mpc.enableDualSolution()
    classes = ("dual", "value_terms", "value_sweep", "riccati")
    for k in range(warmup + steps):
        if k == warmup:
            for c in classes:
                mpc.kernel_time(c, reset=True)
        _run(mpc, prob)
    line = _base(B, itf, intervals, steps, warmup, mpc)
    line["job"] = "kernels"
    line["clock"] = "dual (k_dual_node), value_terms, value_sweep: events attached to the dispatch; riccati: events recorded around its launches; per run"
    for c in classes:
        ms, n = mpc.kernel_time(c)
        line[c + "_ms"], line[c + "_launches"] = ms / steps, n
    line["node_over_terms"] = line["dual_ms"] / line["value_terms_ms"]
    kind = mpc.read("g_kind").astype(int)[:line["nodes"]]
    inter, nx = int((kind == 0).sum()), itf.stateDim
    read_d, write_d = 7 * nx * nx + 22 * nx + 16 * nx, 16 * (nx + 2) + nx + 5
    line["intermediate_nodes"], line["node_read_doubles_per_node"], line["node_written_doubles_per_node"] = inter, read_d, write_d
    line["node_bytes"] = 8 * B * inter * (read_d + write_d)
    line["node_GBs"] = line["node_bytes"] / (1e6 * line["dual_ms"])
    line["write_roof"] = bench.write_roof(B, inter, nx, line["node_GBs"])
    d = mpc.dualSolution()
    line["status_all_valid"] = bool((d.status == 1).all())
    line["residual_over_gu_max"] = float((d.summary[:, 0] / d.summary[:, 1]).max())
    line["gain_residual_over_hux_max"] = float((d.summary[:, 2] / d.summary[:, 3]).max())
    return line


def onoff(B, intervals, steps, warmup):
    itf, prob, mpc = _handle(B, intervals, False)
    mpc.enableValueFunction()
    host = {s: [] for s in STATES}
    for k in range(warmup + steps):
        for state in STATES:                       # the two states alternate inside every step
            mpc.enableDualSolution(state == "dual_on")
            ms = _run(mpc, prob)
            if k >= warmup:
                host[state].append(ms)
    line = _base(B, itf, intervals, steps, warmup, mpc)
    line["job"] = "onoff"
    line["clock"] = "host clock around enqueue and the wait for the stream, one handle with the value function on, the states alternating run by run"
    for state in STATES:
        line.update(pk.host_stats(state, host[state], "ms"))
    line["on_minus_off_ms"] = line["dual_on_ms_median"] - line["value_only_ms_median"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="batch sizes")
    ap.add_argument("--intervals", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--jobs", default="kernels,onoff", help="which kinds of lines")
    pk.driver_options(ap, limit=180)
    a = ap.parse_args()
    if a.child:      # one measurement, in this process
        job, arg = a.child.split(":")
        return pk.child_line(a, (kernels if job == "kernels" else onoff)(int(arg), a.intervals, a.steps, a.warmup))
    kinds = a.jobs.split(",")
    jobs = ["%s:%s" % (j, shape) for shape in a.shapes.split(",") for j in ("kernels", "onoff") if j in kinds]
    return pk.run_jobs(__file__, jobs, pk.forwarded(a), a.limit, a.out)


if __name__ == "__main__":
    sys.exit(main())
