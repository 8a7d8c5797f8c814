"""Eight-wave Riccati sweep: phase cycles (ricp1), own work per wave and phase (ricp2, ricp10..14) of a library built with
-DBPMPC_RICCATI_PROFILE=<v> (tools/mkvariant.sh ricp<v> k_riccati -DBPMPC_RICCATI_PROFILE=<v>).  One line for the library in the tree:
PYTHONPATH=. python tools/ab.py --lib ricp1=tools/probes/lib_ricp1.bin --lib ricp2=tools/probes/lib_ricp2.bin --rounds 1 -- python tools/probes/ric_prof_read.py
"""
import numpy as np
import bipedal_control_amd as bp
from bipedal_control_amd import scenarios

itf = scenarios.h1_interface()
prob = scenarios.trot_problem(itf, batch=256, n_intervals=100)
mpc = bp.BatchedSqpMpc(itf, 256, 116)
mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
for st in ("linearize", "project", "riccati"):
    mpc.stage(st)
mpc.synchronize()
mpc.stage("riccati")
mpc.synchronize()
r = mpc.read("rprof").reshape(-1, 8)[:256]
print("per stage:", (r.mean(axis=0) / 107).round(0).tolist(), " whole horizon: roll-out [5]", r[:, 5].mean().round(0), "its recurrence [6]", r[:, 6].mean().round(0))
