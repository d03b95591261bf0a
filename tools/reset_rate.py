#!/usr/bin/env python3
"""What the per-instance reset (rkfdBatchReset) costs on the headline world: config 4, 4096 instances, the launch shape bench.py
uses (world-specific kernel, split 3, five steps per launch).  Reports, not asserts:
  - a reset with 0 %, 1 % and 100 % of the instances selected, slot values as a host array (staged and uploaded by the call) and as
    a device tensor (read in place);
  - rkfdBatchRestore in the same process, the same way;
  - one single-step launch;
  - the host route a caller had before: get_state / get_contact / get_pivot / get_broken of the whole batch, rows patched on the
    host, set_* of the whole batch (wall clock; it cannot put acc and the contact forces back).
Every device figure is the median over N groups of K calls, each group between two events on the null stream and ended by a join
of the batch's internal streams; the whole series is taken M times, Restore and the resets alternating, and the SPREAD of Restore's
own M medians (max - min) is the margin the 100 % reset is held against.
Writes the report to profiles/r09_reset_rate.txt (or the path given) and prints one JSON line.
usage: python tools/reset_rate.py [out file] [groups N >= 20] [calls per group K] [repeats M >= 5]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.cuda.init()      # torch's HIP runtime before the library's first call (as bench.py does)
import rkfd_pkg
R = rkfd_pkg.load()
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r09_reset_rate.txt")
N = max(int(sys.argv[2]) if len(sys.argv) > 2 else 30, 20)
K = max(int(sys.argv[3]) if len(sys.argv) > 3 else 20, 1)
M = max(int(sys.argv[4]) if len(sys.argv) > 4 else 7, 5)
B = 4096
sc = R.scenarios.config4(batch=B)
b = R.Batch(sc["world"], B, max_rigid=sc["max_rigid"])
b.specialize()
b.set_state(sc["dis"], sc["vel"]); b.set_split(3); b.set_steps_per_launch(5); b.update_init()
b.update(25); assert b.status() == 0
b.snapshot()
b.bank_reserve(B); b.bank_store(0, first=0, count=B)
KEEP = R.RESET_KEEP
host = {"0 %": np.full(B, KEEP, dtype=np.int32), "1 %": np.full(B, KEEP, dtype=np.int32), "100 %": np.arange(B, dtype=np.int32)}
host["1 %"][::100] = np.arange(0, B, 100, dtype=np.int32)
dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in host.items()}
selected = {k: int((v != KEEP).sum()) for k, v in host.items()}


def group_ms(fn):
    """milliseconds per call of N groups of K calls of fn; a group ends with a join of the batch's internal streams"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(N)]
    for e0, e1 in ev:
        e0.record()
        for _ in range(K):
            fn()
        b.join()
        e1.record()
    torch.cuda.synchronize()
    b.status()
    return [e0.elapsed_time(e1) / K for e0, e1 in ev]


series = [("restore", lambda: b.restore())]
for k in host:
    series.append(("reset %s host" % k, lambda k=k: b.reset(host[k])))
    series.append(("reset %s device" % k, lambda k=k: b.reset(dev[k])))
series.append(("reset 100 % snapshot value", lambda: b.reset(np.full(B, R.RESET_SNAPSHOT, dtype=np.int32))))
series.append(("one step", lambda: b.update(1)))
for _, fn in series:      # warm-up: code objects, the staging of the slot values
    group_ms(fn)
medians = {name: [] for name, _ in series}
for _ in range(M):
    for name, fn in series:
        medians[name].append(statistics.median(group_ms(fn)))
assert b.status() == 0

lines = ["per-instance reset, config 4, %d instances, world-specific kernel, split 3; milliseconds per call" % B,
         "median over %d groups of %d calls, the series repeated %d times: median of the medians  [min .. max of the medians]" % (N, K, M)]
out = {"world": "config4", "batch": B, "groups": N, "calls_per_group": K, "repeats": M, "ms": {}}
for name, _ in series:
    m = medians[name]
    out["ms"][name] = dict(median=statistics.median(m), min=min(m), max=max(m))
    lines.append("  %-28s %.5f  [%.5f .. %.5f]" % (name, statistics.median(m), min(m), max(m)))
rs = out["ms"]["restore"]
spread = rs["max"] - rs["min"]
step = out["ms"]["one step"]["median"]
lines.append("selected instances: " + ", ".join("%s = %d" % kv for kv in selected.items()))
lines.append("spread of Restore's own medians (max - min): %.5f ms - the margin" % spread)
for name in ("reset 100 % device", "reset 100 % host", "reset 100 % snapshot value"):
    d = out["ms"][name]["median"] - rs["median"]
    lines.append("%s - restore = %+.5f ms: %s" % (name, d, "within the margin" if abs(d) <= spread else ("MISS: slower than Restore by more than the margin" if d > 0 else "faster than Restore by more than the margin")))
for name in ("reset 0 % device", "reset 0 % host", "reset 1 % device", "reset 1 % host"):
    lines.append("%s / one step = %.4f" % (name, out["ms"][name]["median"] / step))
out["restore_spread_ms"] = spread

# the host route: the whole batch over PCIe and back for one percent of the rows (wall clock)
rows = np.arange(0, B, 100)
t_host = []
for _ in range(5):
    t0 = time.perf_counter()
    dis, vel, acc = b.get_state(); act, typ, ref, f = b.get_contact(); pt, pp = b.get_pivot(); br = b.get_broken()
    for a in (dis, vel, act, typ, ref, pt, pp, br):
        a[rows] = a[0]
    b.set_state(dis, vel); b.set_contact(act, typ, ref); b.set_pivot(pt, pp); b.set_broken(br)
    t_host.append(1e3 * (time.perf_counter() - t0))
out["host_route_ms"] = statistics.median(t_host)
lines.append("host route (get / patch 1 %% of the rows / set of the whole batch, acc and forces not put back): %.3f ms" % out["host_route_ms"])
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fp:
    fp.write(text)
print(json.dumps(out))
