#!/usr/bin/env python3
"""Worst deviation of the contact read-out (rkfdBatchUpdateContactForces) from the references of tests/cf_cases.py, per world, as
|delta|_inf / max( 1, |reference|_inf ): point and wrench against the numpy sum over the candidate tables, genf against reference A
(the oracle's unit-rate Jacobians; A' on trees with raw ten-digit frames) and reference B (refmath's Newton-Euler, worlds with
orthonormal frames) - the lane emulator against each and, when there is a device, the GPU against each.  The trees carry synthetic
candidates, which only the emulator's harness takes: their GPU columns stay empty.  The tests assert 1e-12.
usage: python tools/cf_parity.py [output file, default profiles/r12_cf_parity.txt]"""
import os, sys, tempfile, pathlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")):
    sys.path.insert(0, p)
import numpy as np
import rkfd_pkg
import cf_cases as cc
import links_cases as lc
from oracle.pyoracle import Oracle
R = rkfd_pkg.load()
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r12_cf_parity.txt")
gpu = R.lib().rkfdHipDeviceCount() > 0
tmp = pathlib.Path(tempfile.mkdtemp())
cs = cc.cases(R, tmp)
for ortho in (False, True):
    cs.update({k + ("_on" if ortho else ""): c for k, c in cc.tree_cases(R, tmp, ortho).items()})


def worst(got, ref, keys):
    d = lc.deviations(got, ref, [k for k in keys if k in ref])
    return max(d.values()) if d else 0.0


lines = ["contact read-out: |delta|_inf / max( 1, |reference|_inf ) (tools/cf_parity.py)",
         "sum: point and wrench against the numpy sum over the candidate tables on refmath.fk (count is compared exactly); A: genf from the oracle's",
         "unit-rate site Jacobians (per link, A', on raw ten-digit frames); B: genf of refmath's Newton-Euler (orthonormal frames); bound of the tests 1e-12",
         "the trees carry synthetic candidates, which only the emulator's harness takes: no GPU figure there (nan)",
         "gpu: %s" % ("measured on this run" if gpu else "not run (no device)"),
         "%-20s %5s %5s %5s %10s %10s %10s %10s %10s %10s" % ("world", "nlink", "ndof", "ncand", "emu/sum", "emu/A", "emu/B", "gpu/sum", "gpu/A", "gpu/B")]
top = np.full(6, np.nan)
for name, c in cs.items():
    m = c["world"].model.contents
    w, cand, dis, act, f = c["world"], c["cand"], c["dis"], c["active"], c["f"]
    S = cc.numpy_sum(w, cand, dis, act, f)
    A = {"genf": cc.reference_a(R, Oracle, w, cand, dis, act, f, c["ortho"])}
    Bq = {"genf": cc.reference_b(w, cand, dis, act, f)} if c["ortho"] else None
    got = cc.emu_cf(w, dis, act, f, cand=cand if c["synthetic"] else None)
    assert np.array_equal(got["count"], S["count"])
    row = [worst(got, S, ("point", "wrench")), worst(got, A, ("genf",)), worst(got, Bq, ("genf",)) if Bq else np.nan, np.nan, np.nan, np.nan]
    if gpu and not c["synthetic"]:
        b = R.Batch(w, dis.shape[0], max_rigid=0); b.set_state(dis, np.zeros_like(dis))
        da, df = cc.DevArray(R, act), cc.DevArray(R, f)
        b.update_contact_forces(active=da, f=df); g = b.get_contact_forces()
        da.free(); df.free(); b.close()
        assert np.array_equal(g["count"], S["count"])
        row[3:] = [worst(g, S, ("point", "wrench")), worst(g, A, ("genf",)), worst(g, Bq, ("genf",)) if Bq else np.nan]
    top = np.fmax(top, row)
    lines.append("%-20s %5d %5d %5d %10.2e %10.2e %10.2e %10.2e %10.2e %10.2e" % (name, m.nlink, m.ndof, cand.n, *row))
lines.append("%-20s %5s %5s %5s %10.2e %10.2e %10.2e %10.2e %10.2e %10.2e" % ("worst", "", "", "", *top))
print("\n".join(lines))
with open(OUT, "w") as fh:
    fh.write("\n".join(lines) + "\n")
