"""Unlike instances side by side under the lane emulator (tests/mixed_batches.py): every ordered pair of a world's characters - an
airborne box beside a resting one, a wall that breaks beside one that holds - in one emulated wavefront (RKFD_W = 2) and in
neighbouring ones (RKFD_W = 1).  Every instance must be, bit for bit, what its character gives in an emulated batch of one, and
that batch of one must agree with the oracle.  The MI355X repeats this, with the humanoid, in tests/test_gpu_mixed.py - the
emulator's halves run on their own threads and cannot show what the execution mask does to a shared wavefront."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mixed_batches as mb
from emu import EmuBatch

NSTEPS = 8


class Case:
    """a world, its characters, the oracle's runs of them (the gate) and the emulated batches of one"""

    def __init__(self, R, oracle_cls, name, max_rigid=None):
        self.name = name
        if name == "box":
            self.world, self.max_rigid = mb.box_world(R)
            every = mb.box_characters(R, self.world)
            # the gate on the whole list and on the four the CPU tier has the time for
            mb.assert_gate([mb.oracle_run(oracle_cls, self.world, c, NSTEPS)[1] for c in every], mb.BOX_FULL)
            self.chars = [every[i] for i in mb.BOX_SHORT]
            self.breakable = False
        else:
            self.world, self.max_rigid, self.chars = mb.wall_characters(R)
            self.breakable = True
        if max_rigid is not None:
            self.max_rigid = max_rigid
        runs = [mb.oracle_run(oracle_cls, self.world, c, NSTEPS) for c in self.chars]
        self.oracles = [o for o, _ in runs]; self.counts = [c for _, c in runs]
        if name == "box":
            mb.assert_gate(self.counts, mb.BOX_FULL)
        else:
            mb.assert_wall_gate(self.counts, [o.get_broken()[1:4] for o in self.oracles])
        self.idx, self.pairs, _ = mb.arrangement(len(self.chars))
        self.status, self.want = [], []
        for c in self.chars:
            st, res = mb.run(EmuBatch(self.world, 1, max_rigid=self.max_rigid, ipw=1), [c], NSTEPS, self.breakable)
            self.status.append(st); self.want.append(res)

    def mixed(self, ipw):
        eb = EmuBatch(self.world, len(self.idx), max_rigid=self.max_rigid, ipw=ipw)
        return mb.run(eb, [self.chars[i] for i in self.idx], NSTEPS, self.breakable)


@pytest.fixture(scope="module")
def cases(R, oracle_cls):
    made = {}

    def get(name, max_rigid=None):
        if (name, max_rigid) not in made:
            made[name, max_rigid] = Case(R, oracle_cls, name, max_rigid)
        return made[name, max_rigid]
    return get


def _rel(x, y):
    return np.abs(x - y).max() / max(1.0, np.abs(y).max())


@pytest.mark.parametrize("name", ["box", "wall_hit"])
def test_batches_of_one_agree_with_the_oracle(cases, name):
    """the expected values of the mixed tests anchored outside the device code: 1e-9 relative on state and contact forces, equal
    contact sets (and broken flags), as tests/test_emu_parity.py asks of these worlds"""
    case = cases(name)
    for c, o, st, res in zip(case.chars, case.oracles, case.status, case.want):
        assert st == 0, c.label
        for x, y in zip(res[:3], o.get_state()):
            assert _rel(x[0], y) < 1e-9, c.label
        oact, otyp, oref, of = o.get_contact()
        assert (res[3][0] == oact).all(), c.label
        assert _rel(res[6][0], of * (oact[:, None] != 0)) < 1e-9, c.label
        if case.breakable:
            assert res[9][0].tolist() == o.get_broken().tolist(), c.label


@pytest.mark.parametrize("ipw", [1, 2])
@pytest.mark.parametrize("name", ["box", "wall_hit"])
def test_unlike_neighbours_equal_their_batches_of_one(cases, name, ipw):
    case = cases(name)
    st, got = case.mixed(ipw)
    assert st == 0
    bad = mb.differing(got, case.idx, case.want)
    print(f"{name} ipw {ipw}: batch {len(case.idx)}, {len(bad)} instances differ from their batch of one")
    assert not bad, bad


@pytest.mark.parametrize("ipw", [1, 2])
def test_overflowing_neighbours_equal_their_batches_of_one(cases, ipw):
    """capacity 2: the flat and the landing box overflow (status 2, the surplus vertices dropped), the corner and the airborne one
    do not; the mixed batch reports 2, and every instance still is its batch of one at that capacity"""
    case = cases("box", max_rigid=2)
    assert [st for st in case.status] == [0, 2, 0, 2]
    st, got = case.mixed(ipw)
    assert st == 2
    bad = mb.differing(got, case.idx, case.want)
    print(f"box at capacity 2, ipw {ipw}: batch {len(case.idx)}, {len(bad)} instances differ from their batch of one")
    assert not bad, bad


def test_poisoned_neighbour_leaves_the_others_alone(R, cases, tmp_path):
    """one character's state holds a NaN (emulator only - nothing that is not finite goes to a device): the run ends, and its
    partners in the wavefront and every other instance are their batches of one to the last bit.  In a child process with a
    time limit, so that a device loop the NaN does not let end fails the test instead of hanging it."""
    case = cases("box")
    out = str(tmp_path / "poisoned.npz")
    child = subprocess.run([sys.executable, os.path.abspath(mb.__file__), str(NSTEPS), out], timeout=300)
    assert child.returncode == 0
    z = np.load(out)
    got = tuple(z[n] for n in mb.RESULT_NAMES[:9])
    idx = case.idx
    assert {(i, j) for i, j in case.pairs if mb.POISONED in (i, j)}, "the poisoned character has no partner"
    clean = [p for p, c in enumerate(idx) if c != mb.POISONED]
    bad = [b for b in mb.differing(got, idx, case.want) if b[0] in clean]
    assert not bad, bad
    assert not np.isfinite(got[0][[p for p, c in enumerate(idx) if c == mb.POISONED]]).all()
