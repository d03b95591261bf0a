#!/usr/bin/env python3
"""Worst deviation of the joint-space dynamics (rkfdBatchUpdateDynamics) from the two references of tests/dyn_cases.py, per world, as
|delta|_inf / max( 1, |reference|_inf ): reference A (M from the oracle's unit-rate twists) and reference B (M, h, g from refmath's
Newton-Euler) against each other - a figure of the references alone, the orthonormality defect of the files' frames -, the lane
emulator against each, and, when there is a device, the GPU against each.  The tests assert 1e-12 against A on every world and
against B on the worlds whose frames are orthonormal to rounding (the model files and the trees marked _on, their frames passed
through eom_cases._orthonormal_frames); the raw ten-digit trees are listed against B for the record only.
usage: python tools/dyn_parity.py [output file, default profiles/r11_dyn_parity.txt]"""
import os, sys, tempfile, pathlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")):
    sys.path.insert(0, p)
import numpy as np
import rkfd_pkg
import dyn_cases as dc
import links_cases as lc
from oracle.pyoracle import Oracle
R = rkfd_pkg.load()
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r11_dyn_parity.txt")
gpu = R.lib().rkfdHipDeviceCount() > 0
tmp = pathlib.Path(tempfile.mkdtemp())
cs = dc.cases(R)
for ortho in (False, True):
    tag = "_on" if ortho else ""
    cs.update({k + tag: c for k, c in dc.random_tree_cases(R, tmp, ortho).items()})
    cs.update({k + tag: c for k, c in dc.limit_tree_cases(R, tmp, ortho).items()})


def worst(got, ref, keys):
    d = lc.deviations(got, ref, keys)
    return max(d.values()) if d else 0.0


lines = ["joint-space dynamics: |delta|_inf / max( 1, |reference|_inf ) (tools/dyn_parity.py)",
         "A: M from the oracle's link twists at unit rate vectors; B: M, h, g of refmath's Newton-Euler (tests/dyn_cases.py); bound of the tests 1e-12",
         "A-B: the references against each other (M); the others: worst of M against A, worst of M, h, g against B",
         "asserted: A on every world, B on the worlds whose frames are orthonormal to rounding (yes in the column `B asserted`)",
         "gpu: %s" % ("measured on this run" if gpu else "not run (no device)"),
         "%-20s %5s %5s %10s %10s %10s %10s %10s %10s" % ("world", "nlink", "ndof", "A-B", "emu/A", "emu/B", "gpu/A", "gpu/B", "B asserted")]
top = np.zeros(5)
for name, c in cs.items():
    m = c["world"].model.contents
    A = dc.reference_a(R, Oracle, c["world"], c["dis"], c["broken"])
    Bq = dc.reference_b(c["world"], c["dis"], c["vel"])
    got = dc.emu_dyn(c["world"], c["dis"], c["vel"])
    row = [worst(A, Bq, ("M",)), worst(got, A, ("M",)), worst(got, Bq, dc.KEYS), float("nan"), float("nan")]
    if gpu:
        b = R.Batch(c["world"], c["dis"].shape[0], max_rigid=0); b.set_state(c["dis"], c["vel"]); b.update_dynamics()
        g = b.get_dynamics(); b.close()
        row[3], row[4] = worst(g, A, ("M",)), worst(g, Bq, dc.KEYS)
    if c["ortho"]:
        top = np.fmax(top, row)
    else:
        top[[1, 3]] = np.fmax(top[[1, 3]], [row[1], row[3]])
    lines.append("%-20s %5d %5d %10.2e %10.2e %10.2e %10.2e %10.2e %10s" % (name, m.nlink, m.ndof, *row, "yes" if c["ortho"] else "no"))
lines.append("%-20s %5s %5s %10.2e %10.2e %10.2e %10.2e %10.2e %10s" % ("worst of the asserted", "", "", *top, ""))
print("\n".join(lines))
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
