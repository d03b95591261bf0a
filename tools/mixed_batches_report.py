#!/usr/bin/env python3
"""The character lists of the mixed-batch tests (tests/mixed_batches.py) as the oracle sees them, and which ordered pairs of characters
share a wavefront under the launch shapes the tests use: the first part of profiles/r08_mixed_batches.txt.  CPU only.
usage: python tools/mixed_batches_report.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import rkfd_pkg
R = rkfd_pkg.load()
from oracle.pyoracle import Oracle
import mixed_batches as mb

NSTEPS = 12


def report(name, world, chars, breakable=False):
    print(f"{name}: {len(chars)} characters, contact counts of each alone on the oracle (rkFDUpdateInit, then {NSTEPS} steps)")
    for k, c in enumerate(chars):
        o, cnt = mb.oracle_run(Oracle, world, c, NSTEPS)
        tail = "   broken " + "".join(map(str, o.get_broken()[1:4])) if breakable else ""
        print(f"  {k} {c.label:<56s} {' '.join('%d' % n for n in cnt)}{tail}")
    idx, one, many = mb.arrangement(len(chars))
    print(f"  batch {len(idx)}; one launch: {len(one)} ordered pairs (all {len(chars) * (len(chars) - 1)}), instance {len(idx) - 1} beside the stand-in half")
    print(f"  set_split(3): parts {mb.parts(len(idx), 3)}, {len(many)} ordered pairs, {len(many - one)} of them not in the single launch"
          + (": " + " ".join("%d|%d" % p for p in sorted(many - one)) if many - one else ""))
    print()


w, _ = mb.box_world(R)
report("box on the rigid floor (config1_rigid world; capacity 8, and 2 for the overflow case)", w, mb.box_characters(R, w))
w, _, chars = mb.humanoid_characters(R)
report("humanoid, config 4", w, chars)
report("humanoid, config 4, a parameter row and a control schedule per character", w, mb.with_params_and_controls(w, chars, NSTEPS))
w, _, chars = mb.wall_characters(R)
report("wall_hit (breakable joints)", w, chars, breakable=True)
