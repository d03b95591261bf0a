#!/usr/bin/env python3
"""Deviation table of the tree-size limit cases (tests/tree_limits.py): per case the oracle-alone control (plain build against the
build with fused multiply-adds), the lane emulator and - when a GPU is visible - the generic kernel, the world-specific kernel, two instances per
wavefront and a batch with a parameter table, each against the oracle as
max over dis / vel / acc of |delta|_inf / max( 1, |ref|_inf ) after two steps, B = 4."""
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")]
import rkfd_pkg
import tree_limits as tl
from emu import EmuBatch
from oracle.pyoracle import Oracle

R = rkfd_pkg.load()
gpu = R.lib().rkfdHipDeviceCount() > 0
B = 4
tmp = pathlib.Path(tempfile.mkdtemp())


def run(make, w, dis, vel, mr, kernel="generic", params=None):
    b = make(w, B, max_rigid=mr)
    for n, v in (params or {}).items():
        b.set_param(n, v)
    if kernel == "ipw2":
        b.set_instances_per_wave(2)
    if kernel != "generic":
        b.specialize()
    b.set_state(dis, vel); b.update_init(); b.update(tl.NSTEPS)
    assert b.status() == 0
    st = b.get_state()
    if hasattr(b, "close"):
        b.close()
    return st


def table(w, dis, vel):
    """a batch with a randomised parameter table against the oracle on a model copy per instance"""
    import instance_params as ip
    P = ip.randomised(w, B, seed=0x64)
    ref = [tl.oracle_run(Oracle, ip.model_with(w, ip.of_instance(P, i)), dis[i:i + 1], vel[i:i + 1])[0] for i in range(B)]
    return tl.deviation(run(R.Batch, w, dis, vel, 0, params=P), ref)


def col(x):
    return "%10s" % "-" if x is None else "%10.2e" % x


print("%-24s %-16s %10s %10s %10s %10s %10s %10s" % ("case", "model/dev/coord", "control", "emulator", "gpu", "gpu spec", "gpu ipw2", "gpu table"))
rows = [(c, None) for c in tl.FREE] + [(c, s) for c in tl.CONTACT for s in ("mlcp", "vert")]
for case, solver in rows:
    if solver is None:
        w = tl.world(R, case, tmp); dis, vel = tl.states(w, B); mr = 0
    else:
        w, _, dis, vel = tl.seated_world(R, case, tmp, B, solver=R.SOLVER_MLCP if solver == "mlcp" else R.SOLVER_VERT); mr = 16
    ref = tl.oracle_run(Oracle, w, dis, vel)
    ctl = tl.control(Oracle, w, dis, vel, ref)
    emu = tl.deviation(run(EmuBatch, w, dis, vel, mr), ref)
    g = [None] * 4
    if gpu:
        g[0] = tl.deviation(run(R.Batch, w, dis, vel, mr), ref)
        if R.lib().rkfdLdsBytesFor(w.model, mr) <= 64 * 1024:          # (above: no world-specific kernel, rkfdBatchSpecialize refuses)
            g[1] = tl.deviation(run(R.Batch, w, dis, vel, mr, "spec"), ref)
        if case.ipw2:
            g[2] = tl.deviation(run(R.Batch, w, dis, vel, mr, "ipw2"), ref)
        if case.name in ("chain64_fixed32", "chain59f"):
            g[3] = table(w, dis, vel)
    print("%-24s %-16s %10.2e %10.2e %s" % (case.name + (" " + solver if solver else ""), "%d / %d / %d" % case.dims, ctl, emu, " ".join(col(x) for x in g)), flush=True)
