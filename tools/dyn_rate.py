#!/usr/bin/env python3
"""What the joint-space dynamics (rkfdBatchUpdateDynamics) cost on the headline world: config 4, 4096 instances, the launch shape
bench.py uses (world-specific kernel, split 3, five steps per launch, 25-step rollouts from a snapshot).  Reports, not asserts:
  - milliseconds per launch for MASS, BIAS, GRAVITY and all three, by HIP events around the launch (median, min, max over N launches
    after warm-up), and the bytes each launch writes over its time;
  - the 25-step rollout of the same batch, by HIP events, and the dynamics' share of it.
Prints the series' summaries and one JSON line, and writes them to profiles/r11_dyn_rate.txt (or the file named third).
usage: python tools/dyn_rate.py [launches per flag set, >= 30] [rollouts] [output file]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.cuda.init()      # torch's HIP runtime before the library's first call (as bench.py does)
import rkfd_pkg
R = rkfd_pkg.load()
N = max(int(sys.argv[1]) if len(sys.argv) > 1 else 50, 30)
NR = int(sys.argv[2]) if len(sys.argv) > 2 else 20
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r11_dyn_rate.txt")
B, H = 4096, 25
sc = R.scenarios.config4(batch=B)
b = R.Batch(sc["world"], B, max_rigid=sc["max_rigid"])
b.specialize()
b.set_state(sc["dis"], sc["vel"]); b.set_split(3); b.set_steps_per_launch(5); b.update_init()
b.snapshot()
b.update(H); assert b.status() == 0


def events(fn, n):
    """milliseconds of n calls of fn, each between two events on the null stream"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def summary(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), n=len(ms))


nd = b.ndof
lines = ["joint-space dynamics on config 4: %d instances, %d links, %d coordinates (tools/dyn_rate.py)" % (B, b.nlink, nd)]
NAMES = {1: "mass", 2: "bias", 4: "gravity", 7: "all"}
WRITES = {1: 8 * B * nd * nd, 2: 8 * B * nd, 4: 8 * B * nd, 7: 8 * B * nd * (nd + 2)}
out = {"world": "config4", "batch": B, "nlink": b.nlink, "ndof": nd, "dynamics": {}}
for flags in (1, 2, 4, 7):
    events(lambda: b.update_dynamics(flags), 10)      # warm-up (the first launch allocates the buffers)
    s = summary(events(lambda: b.update_dynamics(flags), N))
    s["bytes_written"] = WRITES[flags]
    s["written_GB_per_s"] = WRITES[flags] / (s["median_ms"] * 1e-3) / 1e9
    out["dynamics"][NAMES[flags]] = s
    lines.append("dynamics %-8s median %.4f ms  (min %.4f, max %.4f, %d launches)  writes %d bytes: %.1f GB/s" %
                 (NAMES[flags], s["median_ms"], s["min_ms"], s["max_ms"], N, WRITES[flags], s["written_GB_per_s"]))
    print(lines[-1], flush=True)
assert all(np.isfinite(v).all() for v in b.get_dynamics().values())


def rollout():
    b.restore(); b.update(H); b.join()


events(rollout, 3)
s = summary(events(rollout, NR))
out["rollout_25_steps"] = s
lines.append("rollout of %d steps  median %.4f ms  (min %.4f, max %.4f, %d rollouts)" % (H, s["median_ms"], s["min_ms"], s["max_ms"], NR))
print(lines[-1], flush=True)
out["share_of_rollout"] = {k: v["median_ms"] / s["median_ms"] for k, v in out["dynamics"].items()}
lines.append("share of the rollout: " + ", ".join("%s %.4f" % kv for kv in out["share_of_rollout"].items()))
print(lines[-1])
assert b.status() == 0
lines.append(json.dumps(out))
print(lines[-1])
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
