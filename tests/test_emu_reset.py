"""The per-instance reset on the lane emulator (no GPU): the device code of roki-fd_amd/csrc/reset/rkfd_reset.h, driven by
tests/emu/rkfd_emu_reset.cpp over the emulator's state arrays and a bank of numpy arrays (tests/emu/emu_reset.py), with the step
kernels of the emulator in between - one and two instances per emulated wavefront.  Every comparison is np.array_equal over dis, vel,
acc, the contact state (active, type, ref, f), the pivots and the broken flags (tests/reset_cases.py).

The story (store, reset at once, reset later, the same batch with no reset call) runs on the box world, whose steps are cheap on the
emulator, with the step counts of reset_cases (20 before the store, 30 compared); the snapshot value and the bad values are checked
on every world of reset_cases after a few steps - what they need is a state worth copying, not a long run."""
import numpy as np
import pytest

import reset_cases as rc
from emu_reset import EmuResetBatch, FIELDS

B_STORY = {1: 3, 2: 5}           # batch of the story per instances per wavefront: five make the wavefronts (0, 1), (2, 3), (4, stand-in)
# steps before the snapshot at which the world's gate holds (arm: the first two instances keep a pivot from step 4 on; wall: the joints
# break within five steps; c4 stands on its soles from the start; the box characters carry forces by step 20)
SCENE_STEPS = {"box": 20, "arm": 6, "wall": 6, "c4": 4}


@pytest.fixture(scope="module")
def stories(R):
    made = {}

    def get(ipw):
        if ipw not in made:
            case = rc.Case(R, "box", B_STORY[ipw])
            made[ipw] = rc.Story(lambda: EmuResetBatch(case.world, case.B, max_rigid=case.max_rigid, ipw=ipw), case)
        return made[ipw]
    return get


@pytest.fixture(scope="module")
def scenes(R):
    """per (world, ipw): a batch of three after SCENE_STEPS steps, a snapshot, three more steps, and a bank of two rows"""
    made = {}

    def get(name, ipw):
        if (name, ipw) not in made:
            case = rc.Case(R, name, 3)
            b = case.fill(EmuResetBatch(case.world, 3, max_rigid=case.max_rigid, ipw=ipw))
            b.update(SCENE_STEPS[name])
            rc.assert_gate(name, rc.result(b), 0); rc.assert_gate(name, rc.result(b), 1)
            b.snapshot()
            b.bank_reserve(2); b.bank_store(0, first=0, count=2)
            b.update(3)
            assert b.status() == 0
            made[(name, ipw)] = b
        return made[(name, ipw)]
    return get


@pytest.mark.parametrize("ipw", [1, 2])
def test_gate_and_padding(stories, ipw):
    s = stories(ipw)
    s.check_gate()
    assert s.batch.pad_intact()


@pytest.mark.parametrize("ipw", [1, 2])
def test_twin(stories, ipw):
    stories(ipw).check_twin()


@pytest.mark.parametrize("ipw", [1, 2])
def test_late_reset(stories, ipw):
    stories(ipw).check_late()


@pytest.mark.parametrize("ipw", [1, 2])
def test_untouched(stories, ipw):
    stories(ipw).check_untouched()


def test_sharing_a_wavefront(stories):
    """with two instances per wavefront the wavefronts of a batch of five are (0, 1), (2, 3) and (4, stand-in): the first reset call
    resets 0 beside 1 kept and 3 beside 2 kept, the second resets 2 beside 3 kept and 4 beside the stand-in half; the twins and the
    late ones pass with the step kernel that pairs them"""
    s = stories(2)
    assert (s.j, s.now, s.late) == (1, [0, 3], [2, 4]) and s.case.B % 2 == 1
    assert s.batch.ipw == 2
    s.check_twin(); s.check_late(); s.check_untouched()


@pytest.mark.parametrize("ipw", [1, 2])
@pytest.mark.parametrize("name", rc.WORLDS)
def test_snapshot_value_is_a_masked_restore(scenes, name, ipw):
    b = scenes(name, ipw)
    mask = rc.masked(b.B)
    assert mask.any() and not mask.all()
    want_all, keep = b.clone(), rc.result(b)
    want_all.restore()
    want = rc.result(want_all)
    for slots in (mask, np.where(mask, rc.SNAPSHOT, rc.KEEP).astype(np.int32)):
        got_b = b.clone()
        got_b.reset(slots)
        got = rc.result(got_b)
        assert got_b.status() == 0 and got_b.pad_intact()
        for i in range(b.B):
            assert rc.rows_equal(got, i, want if mask[i] else keep, i) is None, (i, mask[i])
        assert rc.rows_equal(got, 0, keep, 0) is not None       # (the restore moved something)


@pytest.mark.parametrize("name", rc.WORLDS)
def test_bad_values_touch_nothing_and_set_status_5(scenes, name):
    src = scenes(name, 1)
    keep = rc.result(src)
    # beyond the bank, a negative value that is none of the two, and - without a snapshot - SNAPSHOT; with no bank, any row
    for slots, bank, snap in (([src.nslots, -3, rc.KEEP], True, True), ([rc.SNAPSHOT, rc.KEEP, rc.SNAPSHOT], True, False),
                              ([0, rc.KEEP, 1], False, True), ([2 ** 31 - 1, -2 ** 31, rc.KEEP], True, True)):
        b = src.clone(bank=bank, snap=snap)
        b.reset(np.array(slots, dtype=np.int32))
        got = rc.result(b)
        for i in range(b.B):
            assert rc.rows_equal(got, i, keep, i) is None, (slots, i)
        assert b.status() == 5 and b.status() == 0            # (reported once)
        assert b.pad_intact()
    # the other instances of the same call are reset
    b = src.clone()
    b.reset(np.array([1, src.nslots, rc.KEEP], dtype=np.int32))
    got = rc.result(b)
    bank = src.bank_rows()
    assert b.status() == 5
    assert np.array_equal(b.dis[0], bank["dis"][1]) and np.array_equal(b.acc[0], bank["acc"][1]) and np.array_equal(b.cv_f[0], bank["cv_f"][1])
    assert rc.rows_equal(got, 0, keep, 0) is not None
    for i in (1, 2):
        assert rc.rows_equal(got, i, keep, i) is None


def test_rows_are_copied_whole_and_from_the_right_slot(scenes):
    """every array of a row, raw (anchors and forces of candidates out of contact included), and nothing of the row beside it"""
    src = scenes("wall", 1)
    b = src.clone()
    b.reset(np.array([rc.KEEP, 0, 1], dtype=np.int32))
    bank = src.bank_rows()
    for k in FIELDS:
        assert np.array_equal(getattr(b, k)[1], bank[k][0]) and np.array_equal(getattr(b, k)[2], bank[k][1]), k
        assert np.array_equal(getattr(b, k)[0], getattr(src, k)[0]), k
    assert not np.array_equal(bank["dis"][0], bank["dis"][1]) and b.pad_intact()


def test_parts_of_a_split_launch(scenes):
    """a launch per part over [lo, hi), as under rkfdBatchSetSplit: each touches its own instances only, together they give the
    whole; the last workgroup of every launch is partial"""
    src = scenes("box", 1)
    slots = np.array([1, 0, rc.SNAPSHOT], dtype=np.int32)
    whole = src.clone(); whole.reset(slots)
    parts = src.clone()
    parts.reset(slots, 0, 1)
    for k in FIELDS:
        assert np.array_equal(getattr(parts, k)[1:], getattr(src, k)[1:]), k
    parts.reset(slots, 1, 3)
    for k in FIELDS:
        assert np.array_equal(getattr(parts, k), getattr(whole, k)), k
    assert parts.pad_intact() and parts.status() == 0
