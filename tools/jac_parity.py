#!/usr/bin/env python3
"""Worst deviation of the task-space Jacobians from the reference of tests/jac_cases.py (the oracle's unit-rate columns), per world,
as |delta|_inf / max( 1, |reference|_inf ) over J and Jcom: under the lane emulator and, when there is one, on the GPU; beside them
the reference-only figure of the geometric cross-check - how far the textbook Jacobian (axis x lever arm on the oracle's composed
frames) sits from the oracle's unit-rate columns, the orthonormality defect of the files' frames - and the device against that
textbook Jacobian.  The tests assert 1e-12 against the reference and ten times the recorded textbook figure plus 1e-12 against the
textbook Jacobian; the last lines print the table tests/jac_cases.GEOM_RECORDED holds.
usage: python tools/jac_parity.py [output file, default profiles/r10_jac_parity.txt]"""
import os, sys, tempfile, pathlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")):
    sys.path.insert(0, p)
import numpy as np
import rkfd_pkg
import jac_cases as jc
import links_cases as lc
from oracle.pyoracle import Oracle
R = rkfd_pkg.load()
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10_jac_parity.txt")
gpu = R.lib().rkfdHipDeviceCount() > 0
tmp = pathlib.Path(tempfile.mkdtemp())
cs = jc.cases(R)
cs.update(jc.random_tree_cases(R, tmp))
cs.update(jc.limit_tree_cases(R, tmp))
lines = ["task-space Jacobians: |delta|_inf / max( 1, |reference|_inf ), worst of J and Jcom (tools/jac_parity.py)",
         "reference: the oracle's link velocities and comvel at unit rate vectors (tests/jac_cases.py); bound of the tests 1e-12",
         "textbook: axis x lever arm on the oracle's composed frames - against the oracle (reference only) and the emulator against it",
         "gpu: %s" % ("measured on this run" if gpu else "not run (no device)"),
         "%-18s %5s %5s %12s %12s %14s %14s" % ("world", "nlink", "ndof", "emulator", "gpu", "textbook/orac", "emu/textbook")]
worst = np.zeros(4)
rec = {}
for name, c in cs.items():
    m = c["world"].model.contents
    ref, fr = jc.reference(R, Oracle, c["world"], c["dis"], c["links"], c["points"], c["broken"], with_frames=True)
    got = jc.emu_jac(c["world"], c["dis"], c["links"], c["points"])
    tb = jc.textbook_batch(c["world"], fr, c["links"], c["points"])
    e = jc.worst(lc.deviations(got, ref, jc.KEYS))
    t = jc.worst(lc.deviations(tb, ref, jc.KEYS))
    et = jc.worst(lc.deviations(got, tb, jc.KEYS))
    g = float("nan")
    if gpu:
        b = R.Batch(c["world"], c["dis"].shape[0], max_rigid=0); b.set_state(c["dis"], np.zeros_like(c["dis"]))
        b.set_jacobian_sites(c["links"], c["points"]); b.update_jacobians()
        g = jc.worst(lc.deviations(b.get_jacobians(), ref, jc.KEYS)); b.close()
    worst = np.maximum(worst, [e, g if gpu else 0.0, t, et])
    rec[name] = t
    lines.append("%-18s %5d %5d %12.2e %12.2e %14.2e %14.2e" % (name, m.nlink, m.ndof, e, g, t, et))
lines.append("%-18s %5s %5s %12.2e %12.2e %14.2e %14.2e" % ("worst", "", "", worst[0], worst[1] if gpu else float("nan"), worst[2], worst[3]))
print("\n".join(lines))
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
print("GEOM_RECORDED = {")
for k, v in rec.items():
    print('    "%s": %.1e,' % (k, v))
print("}")
