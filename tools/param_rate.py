#!/usr/bin/env python3
"""What per-instance physical parameters (rkfdBatchSetParam) cost on the headline world: config 4, 4096 instances, the launch shape
bench.py uses (world-specific kernel, tuned instances per wavefront, split 3, five steps per launch, 25-step rollouts from a
snapshot).  Three batches:
  (a) no table - the kernels every batch had before the feature
  (b) a table whose rows all equal the model - the table kernels, every instance reading the same values from its own row
  (c) randomised rows (tests/instance_params.py: randomised)
timed in interleaved rounds (a b c a b c ...); prints the series and one JSON line with the medians.
usage: python tools/param_rate.py [rounds] [rollouts per round]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
torch.cuda.init()      # torch's HIP runtime before the library's first call (as bench.py does)
import rkfd_pkg
import instance_params as ip
R = rkfd_pkg.load()
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100
B, H = 4096, 25
sc = R.scenarios.config4(batch=B)
w = sc["world"]


def make(params):
    b = R.Batch(w, B, max_rigid=sc["max_rigid"])
    if params is not None:
        for n in ip.NAMES:
            b.set_param(n, params[n])
    b.specialize()
    b.set_state(sc["dis"], sc["vel"]); b.set_split(3); b.set_steps_per_launch(5); b.update_init()
    ipw, ms = b.tune_instances_per_wave(8)
    b.snapshot()
    return b, ipw


def rate(b, n):
    b.status()
    t0 = time.time()
    for r in range(n):
        b.restore(); b.update(H)
    st = b.status()
    dt = time.time() - t0
    assert st == 0, st
    return B * H * n / dt


cases = {"a_no_table": None,
         "b_model_rows": {n: np.tile(ip.model_values(w, n), (B, 1)) for n in ip.NAMES},
         "c_randomised": ip.randomised(w, B, seed=0x5EED)}
batches = {k: make(v) for k, v in cases.items()}
for k, (b, ipw) in batches.items():
    rate(b, max(N // 5, 4))      # warm-up
series = {k: [] for k in cases}
for r in range(ROUNDS):
    for k, (b, ipw) in batches.items():
        series[k].append(rate(b, N))
        print("round %d %-14s %.3f M steps/s (instances per wavefront %d)" % (r, k, series[k][-1] / 1e6, ipw), flush=True)
med = {k: statistics.median(v) for k, v in series.items()}
print(json.dumps(dict(workload="config4", instances=B, horizon=H, rollouts_per_round=N, rounds=ROUNDS, split=3, steps_per_launch=5,
                      instances_per_wave={k: batches[k][1] for k in cases},
                      steps_per_s_series={k: [round(x) for x in v] for k, v in series.items()},
                      median_steps_per_s={k: round(v) for k, v in med.items()},
                      relative_to_a={k: round(v / med["a_no_table"], 4) for k, v in med.items()})))
