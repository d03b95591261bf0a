#!/usr/bin/env python3
"""Worst deviation of the task-space read-out from the comparison protocol's reference (tests/links_cases.py), per world, as
|delta|_inf / max( 1, |reference|_inf ) over R, p, v, com, comvel: under the lane emulator, on the GPU when there is one, and -
the control tools/parity_report.py uses - between the oracle's two builds (plain and fused multiply-add), which shows what
rounding alone does to the same formulas.  The tests assert 1e-12; anything above 1e-13 here wants an explanation.
usage: python tools/links_parity.py"""
import os, subprocess, sys, tempfile, pathlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")):
    sys.path.insert(0, p)
import numpy as np
import rkfd_pkg
import links_cases as lc
from oracle.pyoracle import Oracle
R = rkfd_pkg.load()
subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "all", "fma"], check=True, stdout=subprocess.DEVNULL)
LIB_FMA = os.path.join(ROOT, "oracle", "_build", "librkfd_oracle_fma.so")
gpu = R.lib().rkfdHipDeviceCount() > 0
cs = lc.cases(R)
cs.update(lc.random_tree_cases(R, pathlib.Path(tempfile.mkdtemp())))
print("%-18s %12s %12s %12s" % ("world", "emulator", "gpu", "oracle fma"))
worst = [0.0, 0.0, 0.0]
for name, c in cs.items():
    ref = lc.reference(R, Oracle, c["world"], c["dis"], c["vel"], c["broken"])
    fma = lc.reference(R, Oracle, c["world"], c["dis"], c["vel"], c["broken"], libpath=LIB_FMA)
    e = max(lc.deviations(lc.emu_links(c["world"], c["dis"], c["vel"]), ref).values())
    f = max(lc.deviations(fma, ref).values())
    g = float("nan")
    if gpu:
        b = R.Batch(c["world"], c["dis"].shape[0], max_rigid=0); b.set_state(c["dis"], c["vel"]); b.update_links()
        g = max(lc.deviations(b.get_links(), ref).values()); b.close()
    worst = [max(worst[0], e), max(worst[1], g) if gpu else float("nan"), max(worst[2], f)]
    print("%-18s %12.2e %12.2e %12.2e" % (name, e, g, f))
print("%-18s %12.2e %12.2e %12.2e" % ("worst", *worst))
