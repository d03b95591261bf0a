"""The per-instance reset on the MI355X (rkfdBatchBankReserve / BankStore / Reset / ResetDev, rkfd_reset_kernel): the properties of
tests/test_emu_reset.py on the real kernel, for every world of tests/reset_cases.py and batches of 1, 3 and 130 (130 ends in a
partial workgroup whatever the workgroup holds), the three forms of the slot values, stream order on a stream made with
hipStreamNonBlocking at both split settings, two instances per wavefront, a parameter table, the tuning, and the node level.
Every comparison is np.array_equal over dis, vel, acc, the contact state, the pivots and the broken flags."""
import os
import subprocess
import sys

import numpy as np
import pytest

import instance_params as ip
import reset_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 3, 130)


def _make(R, case, configure=None):
    def make():
        b = R.Batch(case.world, case.B, device=0, max_rigid=case.max_rigid)
        if configure:
            configure(b)
        return b
    return make


@pytest.fixture(scope="module")
def cases(R):
    made = {}

    def get(name, B):
        if (name, B) not in made:
            made[(name, B)] = rc.Case(R, name, B)
        return made[(name, B)]
    return get


@pytest.fixture(scope="module")
def stories(R, cases):
    made = {}

    def get(name, B):
        if (name, B) not in made:
            case = cases(name, B)
            made[(name, B)] = rc.Story(_make(R, case), case)
        return made[(name, B)]
    return get


# ---- properties 1 - 4 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", rc.WORLDS)
def test_store_reset_and_run_on(stories, name, B):
    """gate; twin (B > 1): reset at once, equal to the stored instance after every one of 30 steps; late reset: reproduces what the
    stored instance did after the store; untouched: every kept instance equals the batch run with no reset call.  B = 1: the
    instance is reset, later, to its own earlier state."""
    s = stories(name, B)
    s.check_gate()
    if B > 1:
        s.check_twin()
    s.check_late()
    s.check_untouched()


# ---- properties 5 and 6 ----------------------------------------------------------------------------------------------------------
def _scene(R, case):
    """a batch after N0 steps, a snapshot, a bank of two rows (instances 0 and min(1, B-1)) and three more steps"""
    b = case.fill(R.Batch(case.world, case.B, device=0, max_rigid=case.max_rigid))
    b.update(rc.N0)
    b.snapshot()
    b.bank_reserve(2); b.bank_store(0, first=0); b.bank_store(1, first=min(1, case.B - 1))
    b.update(3)
    return b


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", rc.WORLDS)
def test_snapshot_value_is_a_masked_restore(R, cases, name, B):
    case = cases(name, B)
    mask = rc.masked(B)
    a, c = _scene(R, case), _scene(R, case)
    keep = rc.result(a)
    a.reset(np.where(mask, rc.SNAPSHOT, rc.KEEP).astype(np.int32))
    c.restore()
    got, want = rc.result(a), rc.result(c)
    assert a.status() == 0 and c.status() == 0
    for i in range(B):
        assert rc.rows_equal(got, i, want if mask[i] else keep, i) is None, (i, mask[i])
    assert rc.rows_equal(got, 0, keep, 0) is not None
    a.close(); c.close()


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", rc.WORLDS)
def test_bad_values_touch_nothing_and_status_5_is_reported_once(R, cases, name, B):
    case = cases(name, B)
    b = _scene(R, case)
    keep = rc.result(b)
    assert b.status() == 0
    last = B - 1
    for bad in (2, -3, 2 ** 31 - 1, -2 ** 31):
        slots = np.full(B, rc.KEEP, dtype=np.int32); slots[last] = bad
        b.reset(slots)
        assert b.status() == 5 and b.status() == 0
        got = rc.result(b)
        for i in range(B):
            assert rc.rows_equal(got, i, keep, i) is None, (bad, i)
    # without a bank every row is a bad value; the snapshot value still works, and the others of the same call are reset
    b.bank_reserve(0)
    assert b.bank_size() == 0
    slots = np.full(B, rc.KEEP, dtype=np.int32); slots[last] = 0
    if B > 1:
        slots[0] = rc.SNAPSHOT
    b.reset(slots)
    assert b.status() == 5 and b.status() == 0
    got = rc.result(b)
    assert rc.rows_equal(got, last, keep, last) is None
    if B > 1:
        c = _scene(R, case); c.restore()
        assert rc.rows_equal(got, 0, rc.result(c), 0) is None and rc.rows_equal(got, 0, keep, 0) is not None
        c.close()
    b.close()
    # SNAPSHOT without a snapshot
    b = case.fill(R.Batch(case.world, B, device=0, max_rigid=case.max_rigid))
    b.update(2)
    keep = rc.result(b)
    b.reset(np.ones(B, dtype=bool))
    assert b.status() == 5 and b.status() == 0
    got = rc.result(b)
    for i in range(B):
        assert rc.rows_equal(got, i, keep, i) is None
    b.close()


# ---- the emulator's reset code on the same state ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.WORLDS)
def test_bank_rows_and_post_reset_state_equal_the_emulators(R, cases, name):
    """the device's state after N0 steps goes into the emulator's arrays as the accessors report it; the same store and the same
    reset - a row of the bank, the other row, the snapshot value, a bad value - on both: the post-reset state, which holds the
    bank's rows, is the same bit for bit, and so is the status"""
    from emu_reset import EmuResetBatch
    case = cases(name, 5)
    b = case.fill(R.Batch(case.world, 5, device=0, max_rigid=case.max_rigid))
    b.update(rc.N0)
    rc.assert_gate(name, rc.result(b), 1)
    e = EmuResetBatch(case.world, 5, max_rigid=case.max_rigid)

    def load():
        d, v, a = b.get_state(); act, typ, ref, f = b.get_contact(); pt, pp = b.get_pivot()
        e.dis[...] = d; e.vel[...] = v; e.acc[...] = a
        e.cv_active[...] = act; e.cv_type[...] = typ; e.cv_ref[...] = ref; e.cv_f[...] = f
        e.piv_type[...] = pt; e.piv_prev[...] = pp; e.brk[...] = b.get_broken()
    load()
    for x in (b, e):
        x.snapshot(); x.bank_reserve(3); x.bank_store(1, first=1, count=2)
    b.update(2)
    load()
    slots = np.array([1, rc.KEEP, rc.SNAPSHOT, 2, 3], dtype=np.int32)
    b.reset(slots); e.reset(slots)
    got, want = rc.result(b), rc.result(e)
    for i in range(5):
        assert rc.rows_equal(got, i, want, i) is None, (i, rc.rows_equal(got, i, want, i))
    assert rc.rows_equal(got, 0, got, 3) is not None and e.pad_intact()
    assert b.status() == 5 and e.status() == 5
    b.close()


# ---- the forms of the slot values (a child process: torch's HIP runtime comes up before the library's) -----------------------------
_FORMS_CHILD = r"""
import sys
sys.path[:0] = [ROOT, ROOT + "/tests"]
import numpy as np
import torch
torch.cuda.init()
import rkfd_pkg
import reset_cases as rc
R = rkfd_pkg.load()
B = 130
case = rc.Case(R, "c4", B)
b = case.fill(R.Batch(case.world, B, device=0, max_rigid=case.max_rigid))
b.update(5)
b.snapshot()
b.bank_reserve(B + 2)
b.bank_store(0, first=1); b.bank_store(1, first=7)
b.update(3)
b.bank_store(2, first=0, count=B)                 # the state every form starts from
back = np.arange(2, B + 2, dtype=np.int32)
start = rc.result(b)
rng = np.random.default_rng(5)
slots = rng.integers(-2, 2, B).astype(np.int32)   # SNAPSHOT, KEEP, row 0, row 1
mask = slots == rc.SNAPSHOT
got = {}
for form, arg in (("host", slots), ("tensor", torch.from_numpy(slots).to("cuda:0")),
                  ("mask", mask), ("explicit", np.where(mask, rc.SNAPSHOT, rc.KEEP).astype(np.int32)),
                  ("mask tensor", torch.from_numpy(np.where(mask, rc.SNAPSHOT, rc.KEEP).astype(np.int32)).to("cuda:0"))):
    b.reset(back)
    assert all(np.array_equal(x, y) for x, y in zip(rc.result(b), start)), form
    b.reset(arg)
    del arg                                       # the batch keeps a tensor until its launch is waited for
    b.update(2)
    got[form] = rc.result(b)
    assert b.status() == 0
for p, q in (("host", "tensor"), ("mask", "explicit"), ("mask", "mask tensor")):
    assert all(np.array_equal(x, y) for x, y in zip(got[p], got[q])), (p, q)
assert not all(np.array_equal(x, y) for x, y in zip(got["host"], got["mask"]))
for bad in (torch.zeros(B, dtype=torch.int64, device="cuda:0"), torch.zeros(B, dtype=torch.int32), torch.zeros(B + 1, dtype=torch.int32, device="cuda:0"),
            torch.zeros((B, 2), dtype=torch.int32, device="cuda:0")[:, 0], np.zeros(B, dtype=np.int64), np.zeros(B + 1, dtype=np.int32)):
    try:
        b.reset(bad)
    except (TypeError, ValueError):
        continue
    raise AssertionError("accepted slot values of the wrong dtype / device / shape / layout")
b.close()
print("FORMS_OK")
"""


def test_host_slots_tensor_and_mask_give_the_same_bits(R):
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + _FORMS_CHILD], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "FORMS_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- stream order ------------------------------------------------------------------------------------------------------------------
class _NonBlockingStream:
    """a stream made with hipStreamNonBlocking by the HIP runtime the library is linked to (tests/test_gpu_stream_order.py)"""

    def __init__(self, L):
        import ctypes
        self._L = L
        h = ctypes.c_void_p()
        assert L.hipStreamCreateWithFlags(ctypes.byref(h), 1) == 0 and h.value
        self.cuda_stream = h.value

    def close(self):
        import ctypes
        assert self._L.hipStreamDestroy(ctypes.c_void_p(self.cuda_stream)) == 0


@pytest.mark.parametrize("split", [1, 3])
def test_update_reset_update_in_stream_order(R, cases, split):
    """update -> reset -> update on a hipStreamNonBlocking stream with no host wait in between, one launch and three parts with two
    steps per launch: the same bits as the sequence with status() after every call"""
    case = cases("c4", 130)
    s = _NonBlockingStream(R.lib())
    slots = np.full(130, rc.KEEP, dtype=np.int32)
    slots[[0, 42, 43, 44, 87, 129]] = [1, 0, 1, rc.SNAPSHOT, 0, 1]      # (the parts of three: [0, 43), [43, 86), [86, 130))
    out = []
    for wait in (False, True):
        b = R.Batch(case.world, 130, device=0, max_rigid=case.max_rigid)
        if split > 1:
            b.set_split(split); b.set_steps_per_launch(2)
        b.set_state(case.dis, case.vel)
        b.update_init(s.cuda_stream)
        b.update(4, s.cuda_stream)
        b.snapshot()
        b.bank_reserve(2); b.bank_store(0, first=5, count=2)
        seq = [lambda: b.update(5, s.cuda_stream), lambda: b.reset(slots, s.cuda_stream), lambda: b.update(5, s.cuda_stream),
               lambda: b.reset(slots[::-1].copy(), s.cuda_stream), lambda: b.update(3, s.cuda_stream)]
        for call in seq:
            call()
            if wait:
                assert b.status(s.cuda_stream) == 0
        assert b.status(s.cuda_stream) == 0
        out.append(rc.result(b))
        b.close()
    s.close()
    for k, (x, y) in enumerate(zip(*out)):
        assert np.array_equal(x, y), rc.NAMES[k]


# ---- two instances per wavefront, parameters, tuning ---------------------------------------------------------------------------------
def test_two_instances_per_wavefront_batch_5(R, cases):
    """config 4 specialised with two instances per wavefront, batch 5: reset beside kept, kept beside reset, and the instance beside
    the stand-in half, on the real kernel"""
    case = cases("c4", 5)

    def configure(b):
        b.set_instances_per_wave(2); b.specialize()
        assert b.instances_per_wave() == 2
    s = rc.Story(_make(R, case, configure), case)
    assert (s.j, s.now, s.late) == (1, [0, 3], [2, 4])
    s.check_gate(); s.check_twin(); s.check_late(); s.check_untouched()
    # and the same bits as the generic kernel's story
    g = rc.Story(_make(R, case), case)
    for k in range(rc.N1):
        for x, y in zip(s.second[k], g.second[k]):
            assert np.array_equal(x, y), k


def test_with_a_parameter_table(R, cases):
    """two instances with equal rows pass the twin property (parameters are no state: the reset leaves the table alone)"""
    case = cases("c4", 5)
    P = ip.randomised(case.world, 5, 0x5E7)
    for n in ip.NAMES:
        P[n][[0, 3]] = P[n][1]      # the instances reset at once carry the row of the stored one; 2 and 4, reset later, rows of their own

    def configure(b):
        for n in ip.NAMES:
            b.set_param(n, P[n])
        assert b.has_params()
    s = rc.Story(_make(R, case, configure), case)
    s.check_gate(); s.check_twin(); s.check_untouched()
    # (an instance with another row does NOT continue as the stored one did: parameters are no state, the reset leaves them alone)
    assert rc.rows_equal(s.second[-1], 2, s.first[-1], 1) is not None and rc.rows_equal(s.second[-1], 4, s.first[-1], 1) is not None
    assert s.batch.has_params()
    for n in ip.NAMES:
        assert np.array_equal(s.batch.get_param(n), P[n]), n
    # the table matters: the same story on the model's parameters goes another way
    plain = rc.Story(_make(R, case), case, n1=2)
    assert not np.array_equal(plain.first[1][0], s.first[1][0])


def test_tuning_leaves_the_bank_alone(R, cases):
    case = cases("c4", 5)
    b = case.fill(R.Batch(case.world, 5, device=0, max_rigid=case.max_rigid))
    b.specialize()
    b.update(rc.N0)
    b.bank_reserve(1); b.bank_store(0, first=1)
    Y = []
    for _ in range(10):
        b.update(1); Y.append(rc.result(b))
    before = rc.result(b)
    chosen, _ = b.tune_instances_per_wave(4)
    assert chosen in (1, 2) and b.bank_size() == 1
    for x, y in zip(rc.result(b), before):
        assert np.array_equal(x, y)
    slots = np.full(5, rc.KEEP, dtype=np.int32); slots[[0, 4]] = 0
    b.reset(slots)
    for k in range(10):
        b.update(1)
        r = rc.result(b)
        for i in (0, 4):
            assert rc.rows_equal(r, i, Y[k], 1) is None, (k, i)
    assert b.status() == 0
    b.close()


# ---- the node level ----------------------------------------------------------------------------------------------------------------
def test_node_equals_one_batch(R, cases):
    """three shards (on one device when there is only one): bank rows taken with global indices from the last shard, slot values
    that cross the shard boundaries; the result equals a single Batch doing the same"""
    B = 11
    case = cases("c4", B)
    ndev = R.lib().rkfdHipDeviceCount()
    n = R.Node(case.world, B, max_rigid=case.max_rigid, devices=[k % ndev for k in range(3)])
    shards = n.shards()
    assert len(shards) == 3 and shards[-1][2] == B
    last_lo = shards[-1][1]
    b = R.Batch(case.world, B, device=0, max_rigid=case.max_rigid)
    slots = np.full(B, rc.KEEP, dtype=np.int32)
    slots[[0, shards[0][2] - 1, shards[0][2], shards[1][2], B - 1]] = [1, 0, 1, rc.SNAPSHOT, 0]
    for x in (n, b):
        x.set_state(case.dis, case.vel)
        x.update_init(); x.update(6)
        x.snapshot()
        x.bank_reserve(2)
        x.bank_store(0, first=last_lo - 1, count=2)      # (one row from the shard before the last, one from the last)
        x.update(3)
        x.reset(slots)
        x.update(4)
        assert x.status() == 0
    for p, q in zip(n.get_state(), b.get_state()):
        assert np.array_equal(p, q)
    want = rc.result(b)
    for k, (_, lo, hi) in enumerate(shards):
        got = rc.result(n.batch(k))
        for i in range(lo, hi):
            assert rc.rows_equal(got, i - lo, want, i) is None, i
    # a bad value on one shard: status 5 from the node, the others of the call reset
    slots[:] = rc.KEEP; slots[0] = 2
    n.reset(slots)
    assert n.status() == 5 and n.status() == 0
    with pytest.raises(R.RkfdError, match="not within"):
        n.bank_store(1, first=B - 1, count=2)
    n.close(); b.close()
