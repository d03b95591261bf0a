#!/usr/bin/env python3
"""What the contact read-out (rkfdBatchUpdateContactForces) costs: 4096 instances of config 4 (32 candidates) and of the humanoid with
its shell (764 candidates), the launch shape bench.py uses (world-specific kernel, split 3, five steps per launch, 25-step rollouts
from a snapshot).  Reports, not asserts:
  - milliseconds per launch for POINT, WRENCH, GENF and all three, by HIP events around the launch (median, min, max over N launches
    after warm-up), on the forces the rollout left;
  - beside them, in the same process: the 25-step rollout and update_jacobians(JAC_COM), by HIP events, and the read-out's share;
  - the host route it replaces: get_contact() + get_state() of the whole batch by the wall clock, and the numpy bookkeeping
    (tests/cf_cases.numpy_sum: refmath's forward kinematics and the sum over the candidate tables) on 8 instances, per instance.
Prints the series' summaries and one JSON line per world, and writes them to profiles/r12_cf_rate.txt (or the file named third).
usage: python tools/cf_rate.py [launches per flag set, >= 30] [rollouts] [output file]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")):
    sys.path.insert(0, p)
import numpy as np
import torch
torch.cuda.init()      # torch's HIP runtime before the library's first call (as bench.py does)
import rkfd_pkg
import cf_cases as cc
R = rkfd_pkg.load()
N = max(int(sys.argv[1]) if len(sys.argv) > 1 else 50, 30)
NR = int(sys.argv[2]) if len(sys.argv) > 2 else 10
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r12_cf_rate.txt")
B, H = 4096, 25


def events(fn, n):
    """milliseconds of n calls of fn, each between two events on the null stream"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def summary(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), n=len(ms))


lines = []
NAMES = {1: "point", 2: "wrench", 4: "genf", 7: "all"}
for world, make in (("config4", R.scenarios.config4), ("humanoid30_shell", R.scenarios.config4_shell)):
    sc = make(batch=B)
    b = R.Batch(sc["world"], B, max_rigid=sc["max_rigid"])
    b.specialize()
    b.set_state(sc["dis"], sc["vel"]); b.set_split(3); b.set_steps_per_launch(5); b.update_init()
    b.snapshot()
    b.update(H); assert b.status() == 0
    nd, nl, nc = b.ndof, b.nlink, b.ncand
    lines.append("contact read-out on %s: %d instances, %d links, %d coordinates, %d candidates, %.1f active per instance (tools/cf_rate.py)" %
                 (world, B, nl, nd, nc, b.get_contact()[0].sum() / B))
    print(lines[-1], flush=True)
    WRITES = {1: 8 * B * nc * 3, 2: B * nl * (48 + 4), 4: 8 * B * nd}
    WRITES[7] = WRITES[1] + WRITES[2] + WRITES[4]
    out = {"world": world, "batch": B, "nlink": nl, "ndof": nd, "ncand": nc, "contact_forces": {}}
    for flags in (1, 2, 4, 7):
        events(lambda: b.update_contact_forces(flags), 10)      # warm-up (the first launch allocates the buffers)
        s = summary(events(lambda: b.update_contact_forces(flags), N))
        s["bytes_written"] = WRITES[flags]
        out["contact_forces"][NAMES[flags]] = s
        lines.append("contact forces %-7s median %.4f ms  (min %.4f, max %.4f, %d launches)  writes %d bytes" %
                     (NAMES[flags], s["median_ms"], s["min_ms"], s["max_ms"], N, WRITES[flags]))
        print(lines[-1], flush=True)
    assert all(np.isfinite(v).all() for v in b.get_contact_forces().values())
    events(lambda: b.update_jacobians(R.JAC_COM), 10)
    s = summary(events(lambda: b.update_jacobians(R.JAC_COM), N))
    out["jacobians_com"] = s
    lines.append("update_jacobians(JAC_COM) median %.4f ms  (min %.4f, max %.4f, %d launches)" % (s["median_ms"], s["min_ms"], s["max_ms"], N))
    print(lines[-1], flush=True)

    def rollout():
        b.restore(); b.update(H); b.join()
    events(rollout, 2)
    s = summary(events(rollout, NR))
    out["rollout_25_steps"] = s
    lines.append("rollout of %d steps  median %.4f ms  (min %.4f, max %.4f, %d rollouts)" % (H, s["median_ms"], s["min_ms"], s["max_ms"], NR))
    print(lines[-1], flush=True)
    out["share_of_rollout"] = {k: v["median_ms"] / s["median_ms"] for k, v in out["contact_forces"].items()}
    lines.append("share of the rollout: " + ", ".join("%s %.4f" % kv for kv in out["share_of_rollout"].items()))
    # the host route: the copies of the whole batch, and the bookkeeping on a few instances
    t = []
    for _ in range(5):
        t0 = time.perf_counter(); act, _, _, f = b.get_contact(); dis, _, _ = b.get_state(); t.append((time.perf_counter() - t0) * 1e3)
    out["host_copies_ms"] = statistics.median(t)
    cand = cc.model_cand(sc["world"])
    t0 = time.perf_counter(); cc.numpy_sum(sc["world"], cand, dis[:8], act[:8], f[:8]); per = (time.perf_counter() - t0) * 1e3 / 8
    out["host_numpy_ms_per_instance"] = per
    lines.append("host route: get_contact + get_state of %d instances %.3f ms (median of 5, wall clock); numpy bookkeeping %.3f ms per instance (8 instances; wrench only, no genf)" %
                 (B, out["host_copies_ms"], per))
    print(lines[-1], flush=True)
    assert b.status() == 0
    lines.append(json.dumps(out))
    print(lines[-1])
    b.close()
with open(OUT, "w") as fh:
    fh.write("\n".join(lines) + "\n")
