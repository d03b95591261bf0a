#!/usr/bin/env python3
"""What the task-space read-out (rkfdBatchUpdateLinks) costs on the headline world: config 4, 4096 instances, the launch shape
bench.py uses (world-specific kernel, split 3, five steps per launch, 25-step rollouts from a snapshot).  Reports, not asserts:
  - milliseconds per read-out for every flag combination, by HIP events around the launch (median, min, max over N launches
    after warm-up);
  - the 25-step rollout of the same batch, by HIP events, and the read-out's share of it;
  - what a caller had before: get_state over PCIe plus scenarios.link_frames on the host (wall clock; poses only).
Prints the series' summaries and one JSON line.
usage: python tools/links_rate.py [launches per flag set, >= 30] [rollouts]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.cuda.init()      # torch's HIP runtime before the library's first call (as bench.py does)
import rkfd_pkg
R = rkfd_pkg.load()
N = max(int(sys.argv[1]) if len(sys.argv) > 1 else 50, 30)
NR = int(sys.argv[2]) if len(sys.argv) > 2 else 20
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


NAMES = {1: "pose", 2: "vel", 3: "pose+vel", 4: "com", 5: "pose+com", 6: "vel+com", 7: "pose+vel+com"}
out = {"world": "config4", "batch": B, "nlink": b.nlink, "nchain": b.nchain, "readout": {}}
for flags in range(1, 8):
    events(lambda: b.update_links(flags), 10)      # warm-up (the first launch allocates the buffers)
    s = summary(events(lambda: b.update_links(flags), N))
    out["readout"][NAMES[flags]] = s
    print("read-out %-13s median %.4f ms  (min %.4f, max %.4f, %d launches)" % (NAMES[flags], s["median_ms"], s["min_ms"], s["max_ms"], N), flush=True)


def rollout():
    b.restore(); b.update(H); b.join()


events(rollout, 3)
s = summary(events(rollout, NR))
out["rollout_25_steps"] = s
print("rollout of %d steps    median %.4f ms  (min %.4f, max %.4f, %d rollouts)" % (H, s["median_ms"], s["min_ms"], s["max_ms"], NR), flush=True)
out["readout_share_of_rollout"] = out["readout"]["pose+vel+com"]["median_ms"] / s["median_ms"]
print("read-out (all) / rollout = %.4f" % out["readout_share_of_rollout"])
assert b.status() == 0

# the alternative: the joint state over PCIe, forward kinematics on the host (poses only: no velocities, no COM)
m = sc["world"].model.contents
t_copy, t_fk = [], []
for _ in range(5):
    t0 = time.perf_counter(); dis, vel, _ = b.get_state(); t1 = time.perf_counter()
    R.scenarios.link_frames(m, dis); t2 = time.perf_counter()
    t_copy.append(1e3 * (t1 - t0)); t_fk.append(1e3 * (t2 - t1))
out["host_alternative"] = dict(get_state_ms=statistics.median(t_copy), link_frames_ms=statistics.median(t_fk))
print("alternative: get_state %.3f ms + scenarios.link_frames on the host %.1f ms (poses only)" % (out["host_alternative"]["get_state_ms"], out["host_alternative"]["link_frames_ms"]))
t0 = time.perf_counter(); b.update_links(); g = b.get_links(); t1 = time.perf_counter()
out["update_links_plus_get_links_ms"] = 1e3 * (t1 - t0)
print("update_links + get_links (all five arrays to the host) %.3f ms" % out["update_links_plus_get_links_ms"])
print(json.dumps(out))
