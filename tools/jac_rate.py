#!/usr/bin/env python3
"""What the task-space Jacobians (rkfdBatchUpdateJacobians) cost on the headline world: config 4, 4096 instances, the launch shape
bench.py uses (world-specific kernel, split 3, five steps per launch, 25-step rollouts from a snapshot), four sites - both soles
and both hands, or the nearest links the world has.  Reports, not asserts:
  - milliseconds per launch for SITES, COM and both, by HIP events around the launch (median, min, max over N launches after
    warm-up);
  - the 25-step rollout of the same batch, by HIP events, and the Jacobians' share of it.
Prints the series' summaries and one JSON line, and writes them to profiles/r10_jac_rate.txt (or the file named third).
usage: python tools/jac_rate.py [launches per flag set, >= 30] [rollouts] [output file]"""
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
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r10_jac_rate.txt")
B, H = 4096, 25
sc = R.scenarios.config4(batch=B)
m = sc["world"].model.contents


def four_sites(m):
    """both soles and both hands: the leaves of the humanoid's tree that hang deepest below the root (two legs, two arms); in a
    world with fewer than four leaves, the last links"""
    par = m.arr("parent", m.nlink)
    depth = np.zeros(m.nlink, dtype=int)
    for i in range(m.nlink):
        depth[i] = 0 if par[i] < 0 else depth[par[i]] + 1
    leaves = [i for i in range(m.nlink) if not (par == i).any()]
    leaves.sort(key=lambda i: -depth[i])
    pick = sorted(leaves[:4])
    return pick if len(pick) == 4 else list(range(max(0, m.nlink - 4), m.nlink))


sites = four_sites(m)
b = R.Batch(sc["world"], B, max_rigid=sc["max_rigid"])
b.specialize()
b.set_state(sc["dis"], sc["vel"]); b.set_split(3); b.set_steps_per_launch(5); b.update_init()
b.set_jacobian_sites(sites, np.tile([0.0, 0.0, -0.02], (len(sites), 1)))
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


lines = ["task-space Jacobians on config 4: %d instances, %d links, %d coordinates, %d chains, sites on links %s (tools/jac_rate.py)" % (B, b.nlink, b.ndof, b.nchain, sites)]
NAMES = {1: "sites", 2: "com", 3: "sites+com"}
out = {"world": "config4", "batch": B, "nlink": b.nlink, "ndof": b.ndof, "nchain": b.nchain, "sites": [int(s) for s in sites], "jacobians": {}}
for flags in (1, 2, 3):
    events(lambda: b.update_jacobians(flags), 10)      # warm-up (the first launch allocates the buffers)
    s = summary(events(lambda: b.update_jacobians(flags), N))
    out["jacobians"][NAMES[flags]] = s
    lines.append("jacobians %-10s median %.4f ms  (min %.4f, max %.4f, %d launches)" % (NAMES[flags], s["median_ms"], s["min_ms"], s["max_ms"], N))
    print(lines[-1], flush=True)


def rollout():
    b.restore(); b.update(H); b.join()


events(rollout, 3)
s = summary(events(rollout, NR))
out["rollout_25_steps"] = s
lines.append("rollout of %d steps   median %.4f ms  (min %.4f, max %.4f, %d rollouts)" % (H, s["median_ms"], s["min_ms"], s["max_ms"], NR))
print(lines[-1], flush=True)
out["share_of_rollout"] = {k: v["median_ms"] / s["median_ms"] for k, v in out["jacobians"].items()}
lines.append("share of the rollout: " + ", ".join("%s %.4f" % kv for kv in out["share_of_rollout"].items()))
print(lines[-1])
assert b.status() == 0
lines.append(json.dumps(out))
print(lines[-1])
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
