"""What the value function of the solve (bpmpc_solver_enable_value_function) costs, and how close its kernels lie to the numpy restatement.

Every line is one process of its own: H1, trot tiled from t = 0, `--intervals` shooting intervals (100: the headline grid), one SQP iteration per
run from the same cold setup, `--steps` runs after `--warmup`.
  kernels:B   a handle created fused with the feature on, profile level 1: k_value_terms and k_value_sweep between events attached to their
              dispatches, the Riccati sweep of the same runs between the events of its kernel class.  sweep_over_riccati = the value sweep's time
              over the Riccati sweep's (the yardstick: a backward chain of two nx^3 products per stage and no factorisation has no reason to exceed
              it).  terms_GBs = the algorithmic bytes of k_value_terms - per intermediate node 6 nx^2 + 4 nx + 1 doubles of model, gain and step
              read, 2 nx^2 + 3 nx + 1 written - over its time, beside the write roof of this box (tools/probes/write_roof.hip, as bench.py runs it).
  onoff:B     ONE handle created fused; its runs alternate between three states - off and fused, off and materialised
              (bpmpc_solver_set_materialize), on - and a host clock stands around enqueue + wait of every run: median and spread per state;
              on_minus_off and the share of it that materialising alone costs (a fused handle pays both).
  rounding:S  scene S of tests/test_gpu_value_function.py (h1, g1, two_grids): the restatement in double from the same text in np.longdouble (r)
              and the device from the extended result, per quantity.

usage (GPU box, repository root): python tools/value_function_probe.py [--shapes 1,256,4096] [--commit ID] [--out FILE]
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
STATES = ("off_fused", "off_materialised", "on")


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
    return dict(probe="value_function", robot="h1", batch=B, intervals=intervals, nodes=mpc.layout()["n_nodes_max"], steps=steps, warmup=warmup, nx=itf.stateDim)


def kernels(B, intervals, steps, warmup):
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    itf, prob, mpc = _handle(B, intervals, True)
    mpc.enableValueFunction()
    classes = ("value_terms", "value_sweep", "riccati")
    for k in range(warmup + steps):
        if k == warmup:
            for c in classes:
                mpc.kernel_time(c, reset=True)
        _run(mpc, prob)
    line = _base(B, itf, intervals, steps, warmup, mpc)
    line["job"] = "kernels"
    line["clock"] = "value_terms, value_sweep: events attached to the dispatch; riccati: events recorded around its launches; per run"
    for c in classes:
        ms, n = mpc.kernel_time(c)
        line[c + "_ms"], line[c + "_launches"] = ms / steps, n
    line["sweep_over_riccati"] = line["value_sweep_ms"] / line["riccati_ms"]
    kind = mpc.read("g_kind").astype(int)[:line["nodes"]]
    inter, nx = int((kind == 0).sum()), itf.stateDim
    read_d, write_d = 6 * nx * nx + 4 * nx + 1, 2 * nx * nx + 3 * nx + 1
    line["intermediate_nodes"], line["terms_read_doubles_per_node"], line["terms_written_doubles_per_node"] = inter, read_d, write_d
    line["terms_bytes"] = 8 * B * inter * (read_d + write_d)
    line["terms_GBs"] = line["terms_bytes"] / (1e6 * line["value_terms_ms"])
    line["terms_frac_of_8TBs"] = line["terms_GBs"] / 8000.0
    line["write_roof"] = bench.write_roof(B, inter, nx, line["terms_GBs"])
    S, s, v, x_lin, status = mpc.valueFunction()
    line["status_all_valid"] = bool((status == 1).all())
    line["v0_median"] = float(np.median(v[:, 0]))
    return line


def onoff(B, intervals, steps, warmup):
    itf, prob, mpc = _handle(B, intervals, False)
    host = {s: [] for s in STATES}
    for k in range(warmup + steps):
        for state in STATES:                       # the three states alternate inside every step
            mpc.enableValueFunction(state == "on")
            mpc.set_materialize(state == "off_materialised")
            ms = _run(mpc, prob)
            if k >= warmup:
                host[state].append(ms)
    line = _base(B, itf, intervals, steps, warmup, mpc)
    line["job"] = "onoff"
    line["clock"] = "host clock around enqueue and the wait for the stream, one handle, the states alternating run by run"
    for state in STATES:
        line.update(pk.host_stats(state, host[state], "ms"))
    off, mat, on = (line["%s_ms_median" % s] for s in STATES)
    line["on_minus_off_ms"] = on - off
    line["materialise_share_of_difference"] = (mat - off) / (on - off) if on != off else None
    return line


def rounding(scene):
    from tests import test_gpu_value_function as t
    from tests import value_function_reference as vf
    c = t.Staged(scene)
    dev = (c.S, c.s, c.v)
    line = dict(probe="value_function", job="rounding", scene=scene, batch=c.B, nx=c.nx, nodes=[int(n) for n in c.n],
                measure="largest per-node distance relative to the node's largest entry; r: restatement in double from np.longdouble; device: from np.longdouble")
    for q, name in enumerate(("S", "s", "v")):
        line["r_" + name] = c.r[q]
        line["device_" + name] = max(vf.relative_distance(dev[q][b, :c.n[b] + 1], c.ext[b][q]) for b in range(c.B))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="batch sizes")
    ap.add_argument("--intervals", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--jobs", default="kernels,onoff,rounding", help="which kinds of lines")
    pk.driver_options(ap, limit=180)
    a = ap.parse_args()
    if a.child:      # one measurement, in this process
        job, arg = a.child.split(":")
        if job == "rounding":
            return pk.child_line(a, rounding(arg))
        return pk.child_line(a, (kernels if job == "kernels" else onoff)(int(arg), a.intervals, a.steps, a.warmup))
    kinds = a.jobs.split(",")
    jobs = ["%s:%s" % (j, shape) for shape in a.shapes.split(",") for j in ("kernels", "onoff") if j in kinds]
    jobs += ["rounding:%s" % s for s in ("h1", "g1", "two_grids") if "rounding" in kinds]
    return pk.run_jobs(__file__, jobs, pk.forwarded(a), a.limit, a.out)


if __name__ == "__main__":
    sys.exit(main())
