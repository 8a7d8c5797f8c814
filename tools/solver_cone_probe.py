"""What per-problem cone parameters (bpmpc_solver_set_cone_params) cost a solve: the per-problem kernel family, which now takes the cone table as
its second operand, against the default kernels of the same tree, per kernel class; distinct cone rows against equal ones; and the family on a
weights-only handle, the line that a run of this same file on the parent commit's tree is compared with (what the second operand costs the users
of bpmpc_solver_set_weights).

Every line is one process of its own: H1, trot tiled from t = 0, `--intervals` shooting intervals (100: the headline grid, 103 intermediate nodes),
one SQP iteration per run from the same cold setup, `--steps` runs after `--warmup`, every kernel class between device events of the solver's own
timers (bpmpc_solver_kernel_time, profile level 1) and a host clock around enqueue + wait.
  default        no row set: k_linearize_fast, k_trial_fast / k_ls_tail, k_project_fast(_qd)
  weights_equal  every weight row the model's, set through bpmpc_solver_set_weights, no cone row set (runs on the parent commit as well)
  cone_equal     every cone row the start row, set through bpmpc_solver_set_cone_params: the per-problem kernels on the same numbers
  cone_distinct  a cone row per problem: friction coefficients from 0.3 to 0.7, barrier mu from 0.05 to 0.2, different in every problem
in materialised and in fused mode.  The variants of one (batch, mode) run in turn, --repeats times, so each variant's own spread stands beside
the differences.  The ratio of a line's kernel class over the `default` line of the same repeat is left to the reader of the file.

The comparison with the parent commit alternates two trees on one box through tools/ab.py, e.g. with the parent's tree (and this file) under P:
  python tools/ab.py --env "TREE=P" --env "TREE=." --rounds 3 --args "weights_equal:fused:256|weights_equal:fused:4096" -- sh -c 'cd $TREE && python tools/solver_cone_probe.py --child $0'

usage (GPU box, repository root): python tools/solver_cone_probe.py [--shapes 256,4096] [--commit ID] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probekit as pk      # noqa: E402

SHAPES = "256,4096"
CLASSES = ("linearize", "linesearch", "project")
VARIANTS = ("default", "weights_equal", "cone_equal", "cone_distinct")


def measure(variant, mode, B, intervals, steps, warmup):
    import numpy as np
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    itf = sc.h1_interface()
    horizon = intervals * sc.DT
    prob = sc.trot_problem(itf, batch=B, n_intervals=intervals, gait_start=0.0)
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=sc.max_nodes_for(intervals, horizon), sqp_iterations=1, profile=True,
                           materialize_lq=(mode == "materialised"))
    weights = cone = None
    if variant == "weights_equal":
        weights = bp.MpcWeights.from_model(itf).row
    elif variant == "cone_equal":
        cone = bp.ConeParams.from_model(itf).row
    elif variant == "cone_distinct":
        f = np.arange(B) / max(1, B - 1)
        start = bp.ConeParams.from_model(itf)
        cone = np.stack([start.replaced(frictionCoefficient=0.3 + 0.4 * f[b], mu=0.05 * 4.0 ** f[B - 1 - b]).row for b in range(B)])
    elif variant != "default":
        raise ValueError("unknown variant %s" % variant)
    suffix = "" if variant == "default" else "_w"
    host = []
    for k in range(warmup + steps):
        mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
        if k == 0 and weights is not None:
            mpc.setWeights(weights)                           # once: the rows outlive a setup
        if k == 0 and cone is not None:
            mpc.setConeParams(cone)
        if k == warmup:
            for c in CLASSES:
                mpc.kernel_time(c + suffix, reset=True)
        t0 = time.perf_counter()
        mpc.enqueue()
        mpc.synchronize()
        if k >= warmup:
            host.append(1e3 * (time.perf_counter() - t0))
    lay = mpc.layout()
    line = dict(probe="solver_cone", robot="h1", batch=B, mode=mode, variant=variant, intervals=intervals, nodes=lay["n_nodes_max"], steps=steps, warmup=warmup,
                clock="device events of the solver's kernel classes, per run; host clock around enqueue and the wait for the stream", cone_row_bytes=64)
    for c in CLASSES:
        ms, n = mpc.kernel_time(c + suffix)
        other = mpc.kernel_time(c + ("" if suffix else "_w"))[1]
        line[c + "_ms"] = ms / steps
        line[c + "_launches"] = n
        line[c + "_other_set_launches"] = other            # 0: only the kernel set of the variant ran
    line.update(pk.host_stats("solve", host, "ms"))
    st = mpc.fetch()[4]
    line["status_max"] = int(max(s.status for s in st))
    line["back_tracked"] = int(sum(1 for s in st if s.step_size < 1.0))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="batch sizes")
    ap.add_argument("--intervals", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=2)
    pk.driver_options(ap, limit=180)
    a = ap.parse_args()
    if a.child:      # one measurement, in this process
        variant, mode, B = a.child.split(":")
        return pk.child_line(a, measure(variant, mode, int(B), a.intervals, a.steps, a.warmup))
    jobs = ["%s:%s:%s" % (v, mode, shape) for shape in a.shapes.split(",") for mode in ("materialised", "fused") for _ in range(a.repeats) for v in VARIANTS]
    return pk.run_jobs(__file__, jobs, pk.forwarded(a), a.limit, a.out)


if __name__ == "__main__":
    sys.exit(main())
