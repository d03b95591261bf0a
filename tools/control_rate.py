#!/usr/bin/env python3
"""Rate of MPC-style rollouts with per-step controls on the headline world (config 4, 4096 instances, the bench's launch setup:
world-specific kernel, split 3, rollouts of H steps from a snapshot).  Four ways to run a rollout:
  (a) update(H) with zero inputs - the headline path
  (b) update_controlled(u) with a random schedule on the host (copied per rollout)
  (c) update_controlled(u) with the schedule as a float64 torch tensor on the device
  (d) the fallback without schedules: set_motor_input(u[:, k]) + update(1) per step
Prints one JSON line (steps/s of each).  usage: python tools/control_rate.py [horizon] [rollouts]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.cuda.init()      # torch's HIP runtime before the library's first call (as bench.py does)
import rkfd_pkg
R = rkfd_pkg.load()
H = int(sys.argv[1]) if len(sys.argv) > 1 else 25
N = int(sys.argv[2]) if len(sys.argv) > 2 else 200
B = 4096
sc = R.scenarios.config4(batch=B)
b = R.Batch(sc["world"], B, max_rigid=sc["max_rigid"])
b.specialize()
b.set_state(sc["dis"], sc["vel"]); b.set_split(3); b.update_init()
b.snapshot()
rng = np.random.default_rng(1)
u = np.ascontiguousarray(rng.normal(0.0, 0.5, (B, H, b.nlink)))
zero = np.zeros((B, b.nlink))


def run(case, n):
    ut = torch.from_numpy(u).to("cuda:0") if case == "c" else None
    b.set_motor_input(zero)
    best = None
    for rep in range(2):                      # the first pass warms up
        torch.cuda.synchronize(); b.status()
        t0 = time.time()
        for r in range(n):
            b.restore()
            if case == "a":
                b.update(H)
            elif case == "b":
                b.update_controlled(u)
            elif case == "c":
                b.update_controlled(ut)
            else:
                for k in range(H):
                    b.set_motor_input(u[:, k, :])
                    b.update(1)
        st = b.status()
        dt = time.time() - t0
        assert st == 0, st
        best = dt if best is None or dt < best else best
    return B * H * n / best


rates = {}
for case, name in (("a", "update_zero_inputs"), ("b", "controlled_host"), ("c", "controlled_device"), ("d", "stepwise_fallback")):
    rates[name] = run(case, N if case != "d" else max(N // 10, 4))
    print("%-20s %.3f M steps/s" % (name, rates[name] / 1e6), file=sys.stderr, flush=True)
print(json.dumps(dict(workload="config4", instances=B, horizon=H, rollouts=N, split=3,
                      steps_per_s={k: round(v) for k, v in rates.items()},
                      relative_to_a={k: round(v / rates["update_zero_inputs"], 4) for k, v in rates.items()})))
