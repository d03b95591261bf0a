"""Helpers of the per-instance reset tests (tests/test_emu_reset.py, tests/test_gpu_reset.py): small worlds whose instances are
unlike each other, in the style of tests/mixed_batches.py, and the STORY every property is read from - one run of a batch (Batch or
emu_reset.EmuResetBatch: the same surface) with a store, a reset at once, a reset later, and the same batch run with no reset call.

Worlds and what each exists to carry:
  box    scenarios.config1_rigid's world, the box characters of mixed_batches: rigid anchors (cv_ref) and forces (cv_f)
  arm    scenarios.arm_press: friction pivots (piv_type, piv_prev)
  wall   scenarios.wall_hit: broken flags appear during the run (brk)
  c4     scenarios.config4 at a small batch: eligible for two instances per wavefront, forces on eight sole vertices

THE GATE (assert_gate) is a condition, not a measurement: at store time the stored row must hold that state, and every instance
about to be reset must differ from its slot in dis before the reset (assert_differs).  A case that fails it is the wrong case; the
gate stays.

Motor input is no state (as for Snapshot / Restore): an instance continues as its slot's source did only under the same motor
input, so every instance of the arm world gets the input of the scenario's first instance."""
import numpy as np

import mixed_batches as mb

KEEP, SNAPSHOT = -1, -2
N0, N1 = 20, 30                 # steps before the store; steps compared after a reset
WORLDS = ("box", "arm", "wall", "c4")
NAMES = mb.RESULT_NAMES
BOX_ORDER = (1, 6, 3, 2, 4, 5, 0)      # mixed_batches.box_characters: flat, landing, corner, edge, sliding, spinning, airborne
ARM_ORDER = (0, 6, 2, 3, 4, 5, 1)      # of scenarios.arm_press's seeded instances: the first two keep a friction pivot from step 4 on


class Case:
    """B unlike instances of one world: dis, vel (B, ndof), motor_in (B, nlink) or None"""

    def __init__(self, R, name, B):
        S = R.scenarios
        self.name, self.B, self.motor_in = name, B, None
        if name == "box":
            self.world, self.max_rigid = mb.box_world(R)
            ch = mb.box_characters(R, self.world)
            pick = [ch[BOX_ORDER[i % len(BOX_ORDER)]] for i in range(B)]
            self.dis = np.array([c.dis for c in pick]); self.vel = np.array([c.vel for c in pick])
            self.dis[:, 0] += 1.0e-3 * np.arange(B)        # (along the hard half of the floor: no two instances share a dis)
        else:
            n = max(B, len(ARM_ORDER))
            sc = {"arm": S.arm_press, "wall": S.wall_hit, "c4": S.config4}[name](batch=n)
            order = (list(ARM_ORDER) + list(range(len(ARM_ORDER), n))) if name == "arm" else list(range(n))
            self.world, self.max_rigid = sc["world"], sc["max_rigid"]
            self.dis = sc["dis"][order][:B].copy(); self.vel = sc["vel"][order][:B].copy()
            if name == "arm":
                self.motor_in = np.tile(sc["motor_in"][0], (B, 1))
        m = self.world.model.contents
        self.nlink, self.ndof, self.ncand = m.nlink, m.ndof, m.ncand

    def fill(self, b):
        """the instances into a batch, up to and including update_init"""
        b.set_state(self.dis, self.vel)
        if self.motor_in is not None:
            b.set_motor_input(self.motor_in)
        b.update_init()
        return b


def result(b):
    """dis, vel, acc, cv_active, cv_type, cv_ref, cv_f, piv_type, piv_prev, broken - copies"""
    return tuple(np.array(x) for x in mb.result(b, True))


def rows_equal(x, p, y, q):
    """name of the first array in which instance p of result x differs from instance q of result y, or None"""
    for k, n in enumerate(NAMES):
        if not np.array_equal(x[k][p], y[k][q]):
            return n
    return None


def assert_gate(name, res, j):
    """instance j of a result holds the state its world exists to carry"""
    act, f, piv, brk = res[3][j], res[6][j], res[7][j], res[9][j]
    if name in ("box", "c4"):
        assert (act != 0).any() and (f[act != 0] != 0).any(), (name, j, "no contact force")
    elif name == "arm":
        assert (piv != 0).any(), (name, j, "no friction pivot")
    else:
        assert (brk != 0).any(), (name, j, "nothing broken")


def assert_differs(res, targets, row):
    """every instance about to be reset differs in dis from the row (dis of one instance) it is reset to"""
    for t in targets:
        assert not np.array_equal(res[0][t], row), ("instance %d already equals its slot" % t)


def plan(B):
    """-> (source j, instance stored in the other slot, instances reset at once, instances reset later).  Under two instances per
    wavefront and B >= 5: 0 is reset beside 1 kept, 3 is reset beside 2 kept - both orders -, and an odd batch's last instance,
    reset later, has the stand-in half for a neighbour.  B = 1: the instance is reset, later, to its own earlier state."""
    j = 1 if B > 1 else 0
    now = [t for t in (0, 3) if t < B and t != j]
    late = [t for t in dict.fromkeys((2, B - 1)) if 0 <= t < B and t not in now and (t != j or B == 1)]
    return j, min(2, B - 1), now, late


SLOT, OTHER = 1, 0              # the row the story resets from, and a second row that holds another instance


class Story:
    """make() -> a fresh batch of case.B instances (configured by the caller, not filled).  The run:
         fill, N0 steps, bank_reserve(2), slot OTHER <- instance `other`, slot SLOT <- instance j        [self.stored: the result then]
         reset `now` from SLOT, n1 single steps                                                         [self.first[k]]
         reset `late` from SLOT (a new call: every other instance KEEP), n1 single steps                [self.second[k]]
       and the same batch with no reset call at all: N0 steps, 2 n1 single steps                        [self.plain[k]]
       status: what status() returned after each of the two reset calls and at the end."""

    def __init__(self, make, case, n0=N0, n1=N1):
        B = case.B
        self.case, self.n1 = case, n1
        self.j, self.other, self.now, self.late = plan(B)
        b = case.fill(make())
        b.update(n0)
        b.bank_reserve(2)
        assert b.bank_size() == 2
        b.bank_store(OTHER, first=self.other); b.bank_store(SLOT, first=self.j)
        self.stored = result(b)
        self.status = []
        self.first, self.second = [], []
        for targets, rec in ((self.now, self.first), (self.late, self.second)):
            before = result(b)
            slots = np.full(B, KEEP, dtype=np.int32); slots[targets] = SLOT
            self.before_second = before      # (after the loop: what the batch held before the second call)
            b.reset(slots)
            self.status.append(b.status())
            for _ in range(n1):
                b.update(1)
                rec.append(result(b))
        self.status.append(b.status())
        self.batch = b
        c = case.fill(make())
        c.update(n0)
        self.plain = []
        for _ in range(2 * n1):
            c.update(1)
            self.plain.append(result(c))
        self.plain_status = c.status()
        if hasattr(c, "close"):
            c.close()

    # ---- the properties ------------------------------------------------------------------------------------------------------
    def check_gate(self):
        assert_gate(self.case.name, self.stored, self.j)
        assert_differs(self.stored, self.now, self.stored[0][self.j])
        assert_differs(self.before_second, self.late, self.stored[0][self.j])
        # (no reset call of the story names a row that is not there; whatever else the run reports, the plain run reports too)
        assert 5 not in self.status and set(self.status) - {0} <= {self.plain_status}, (self.status, self.plain_status)

    def check_twin(self):
        """an instance reset at once equals the stored instance after every step"""
        assert self.now, "the batch is too small for a twin"
        for k, r in enumerate(self.first):
            for i in self.now:
                assert rows_equal(r, i, r, self.j) is None, (k, i, rows_equal(r, i, r, self.j))

    def check_late(self):
        """an instance reset later reproduces what the stored instance did after the store"""
        assert self.late
        for k, r in enumerate(self.second):
            for i in self.late:
                assert rows_equal(r, i, self.first[k], self.j) is None, (k, i, rows_equal(r, i, self.first[k], self.j))

    def check_untouched(self):
        """every instance a reset call keeps is what the batch run with no reset call holds: all but `now` in the first phase; in the
        second the instances never reset, and those of `now` - kept by the second call - are what the stored instance is by then"""
        B, n1 = self.case.B, self.n1
        for k in range(n1):
            for i in range(B):
                if i not in self.now:
                    assert rows_equal(self.first[k], i, self.plain[k], i) is None, (k, i)
                if i not in self.now and i not in self.late:
                    assert rows_equal(self.second[k], i, self.plain[n1 + k], i) is None, (k, i)
            for i in self.now:
                assert rows_equal(self.second[k], i, self.plain[n1 + k], self.j) is None, (k, i)


def masked(B):
    """a mask with both values next to each other in either order, its first and last instance selected when B allows"""
    m = np.zeros(B, dtype=bool)
    m[[i for i in (0, 3, B - 1) if 0 <= i < B]] = True
    return m
