"""Control schedules (rkfdBatchUpdateControlled) under the lane emulator, without a GPU: the device code reads motor input k of a
schedule at the start of step k.  A schedule run in rounds of launches, its pointer advanced as the C ABI does, gives the bits of
stepping one step at a time with the inputs set in between and agrees with the oracle stepped the same way.
tests/emu/rkfd_emu_ctrl.cpp is the harness; tests/test_gpu_control.py repeats this on the GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from emu import EmuBatch, DevState, ROOT, HERE

RTOL = 1e-9
_libs = {}


def _lib(ipw):
    if ipw not in _libs:
        path = os.path.join(HERE, "librkfd_emu_ctrl%s.so" % ("_w2" if ipw == 2 else ""))
        if not os.path.exists(path):
            subprocess.run(["make", "-C", ROOT, "emu"], check=True, stdout=subprocess.DEVNULL)
        L = C.CDLL(path)
        L.rkfd_emu_run_ctrl.argtypes = [C.c_void_p, C.c_int, C.POINTER(DevState), C.c_int, C.c_void_p, C.c_int]
        _libs[ipw] = L
    return _libs[ipw]


class CtrlEmuBatch(EmuBatch):
    def update_controlled_round(self, u, first, nsteps):
        """one launch of rkfdBatchUpdateControlled: steps [first, first + nsteps) of schedule u [B, H, nlink]"""
        u = np.ascontiguousarray(u, dtype=np.float64)
        H = u.shape[1]
        st = DevState()
        for k in ("dis", "vel", "acc", "motor_in", "piv_type", "piv_prev", "cv_active", "cv_type", "cv_ref", "cv_f", "brk", "dbg"):
            setattr(st, k, getattr(self, k).ctypes.data)
        st.dbg_stride = 18 * self.nlink
        st.batch = self.B
        ptr = u.ctypes.data + 8 * first * self.nlink          # ctrl + r*per*nlink
        self.err = _lib(self.ipw).rkfd_emu_run_ctrl(C.cast(self.world.model, C.c_void_p), self.max_rigid, C.byref(st), nsteps,
                                                   C.c_void_p(ptr), H * self.nlink)
        if self.err < 0:
            raise RuntimeError("emulator: device model build failed")


def schedule(sc, B, H, seed):
    """random per-step inputs around the scenario's own, on every link; a third of the rows far beyond any motor's limits
    (a DC motor saturates its voltage, a torque motor takes them as they are)"""
    m = sc["world"].model.contents
    rng = np.random.default_rng(seed)
    base = np.asarray(sc.get("motor_in", np.zeros((B, m.nlink))))[:B]
    u = base[:, None, :] + rng.normal(0.0, 1.0, (B, H, m.nlink))
    sat = rng.random((B, H)) < 0.35
    u[sat] *= 40.0
    return u


def _close(x, y):
    return np.abs(x - y).max() / max(1.0, np.abs(y).max())


CASES = [("arm_press", 2, 1), ("arm_press", 2, 2), ("config3", 2, 1), ("config3", 2, 2)]


def _scenario(R, name, B):
    if name == "arm_press":
        return R.scenarios.arm_press(batch=B, root="fixed", with_box=True)
    return R.scenarios.config3(batch=B)


@pytest.mark.parametrize("name,B,ipw", CASES)
def test_schedule_in_rounds_equals_stepwise_and_oracle(R, oracle_cls, name, B, ipw):
    H = 6
    sc = _scenario(R, name, B)
    u = schedule(sc, B, H, seed=0xC0DE + ipw)

    # rounds of 2 + 4 steps, the pointer advanced by the C ABI's rule
    a = CtrlEmuBatch(sc["world"], B, max_rigid=sc["max_rigid"], ipw=ipw)
    a.set_state(sc["dis"], sc["vel"]); a.update_init()
    a.update_controlled_round(u, 0, 2)
    assert a.status() == 0
    a.update_controlled_round(u, 2, 4)
    assert a.status() == 0

    # six single steps with the input set in between
    s = EmuBatch(sc["world"], B, max_rigid=sc["max_rigid"], ipw=ipw)
    s.set_state(sc["dis"], sc["vel"]); s.update_init()
    for k in range(H):
        s.set_motor_input(u[:, k, :])
        s.update(1)
        assert s.status() == 0

    for x, y in zip(a.get_state(), s.get_state()):
        assert np.array_equal(x, y)
    for x, y in zip(a.get_contact(), s.get_contact()):
        assert np.array_equal(x, y)
    for x, y in zip(a.get_pivot(), s.get_pivot()):
        assert np.array_equal(x, y)
    dis, vel, acc = a.get_state()
    # the last row stays the motor input (the kernel stores it): a plain step afterwards continues with it, in both
    a.update(1); s.update(1)
    for x, y in zip(a.get_state(), s.get_state()):
        assert np.array_equal(x, y)

    # the oracle stepped with per-step inputs
    for i in range(B):
        o = oracle_cls(sc["world"].model)
        o.set_state(sc["dis"][i], sc["vel"][i]); o.update_init()
        for k in range(H):
            o.set_motor_input(u[i, k]); o.update()
        od, ov, oa = o.get_state()
        for x, y in ((dis[i], od), (vel[i], ov), (acc[i], oa)):
            assert _close(x, y) < RTOL


def test_schedule_changes_the_result(R):
    """the schedule is read: a different input in the last step changes the arm's state (the test above would pass with the inputs ignored
    only if stepwise ignored them too)"""
    B, H = 1, 2
    sc = _scenario(R, "arm_press", B)
    u = schedule(sc, B, H, seed=7)
    out = []
    for scale in (1.0, -1.0):
        v = u.copy(); v[:, 1, :] *= scale
        a = CtrlEmuBatch(sc["world"], B, max_rigid=sc["max_rigid"])
        a.set_state(sc["dis"], sc["vel"]); a.update_init()
        a.update_controlled_round(v, 0, H)
        out.append(a.get_state()[1])
    assert not np.array_equal(out[0], out[1])
