"""Per-instance physical parameters under the lane emulator, without a GPU: the device code built with RKFD_PARAMS = 1 reads every
instance's masses, centres of mass, inertias, joint friction and contact-info constants at the instance's row of the table
(tests/emu/rkfd_emu_par.cpp makes the table and binds the model to it exactly as the C ABI's launch does).
  - instance i of the table run equals, bit for bit, a single-model run on model_with(P_i);
  - two instances per wavefront equal one, bit for bit;
  - a table whose rows equal the model equals the run without a table, bit for bit;
  - every instance agrees with the unchanged oracle on model_with(P_i) to 1e-9 (the tolerance of tests/test_emu_control.py).
tests/test_gpu_params.py repeats this on the GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from emu import EmuBatch, DevState, ROOT, HERE
import instance_params as ip

RTOL = 1e-9
B, H = 4, 6
_libs = {}


def _lib(ipw):
    if ipw not in _libs:
        path = os.path.join(HERE, "librkfd_emu_par%s.so" % ("_w2" if ipw == 2 else ""))
        if not os.path.exists(path):
            subprocess.run(["make", "-C", ROOT, "emu"], check=True, stdout=subprocess.DEVNULL)
        L = C.CDLL(path)
        L.rkfd_emu_run_par.argtypes = [C.c_void_p, C.c_int, C.POINTER(DevState), C.c_int, C.c_int, C.c_void_p]
        _libs[ipw] = L
    return _libs[ipw]


class ParEmuBatch(EmuBatch):
    """EmuBatch whose launches carry a table of per-instance parameters (params: {name: (B, width)}; missing names: the model's)"""

    def __init__(self, world, batch, max_rigid=8, ipw=1, params=None):
        super().__init__(world, batch, max_rigid=max_rigid, ipw=ipw)
        self.params = None
        if params is not None:
            m = world.model.contents
            self.params = [np.ascontiguousarray(params[n] if n in params else np.tile(ip.model_values(world, n), (batch, 1)),
                                                dtype=np.float64).reshape(batch, ip.width(m, n)).copy() for n in ip.NAMES]

    def _run(self, mode, nsteps):
        st = DevState()
        for k in ("dis", "vel", "acc", "motor_in", "piv_type", "piv_prev", "cv_active", "cv_type", "cv_ref", "cv_f", "brk", "dbg"):
            setattr(st, k, getattr(self, k).ctypes.data)
        st.dbg_stride = 18 * self.nlink
        st.batch = self.B
        par = None
        if self.params is not None:
            par = (C.c_void_p * 13)(*[a.ctypes.data for a in self.params])
        self.err = _lib(self.ipw).rkfd_emu_run_par(C.cast(self.world.model, C.c_void_p), self.max_rigid, C.byref(st), mode, nsteps,
                                                  C.cast(par, C.c_void_p) if par is not None else None)
        if self.err < 0:
            raise RuntimeError("emulator: device model build failed")


def _scenario(R, name):
    if name == "arm_press":
        return R.scenarios.arm_press(batch=B, root="fixed", with_box=True)
    return R.scenarios.config3(batch=B)


def _run(b, sc, lo=0, hi=None):
    hi = b.B + lo if hi is None else hi
    b.set_state(sc["dis"][lo:hi], sc["vel"][lo:hi])
    if "motor_in" in sc:
        b.set_motor_input(np.asarray(sc["motor_in"])[lo:hi])
    b.update_init()
    assert b.status() == 0
    b.update(H)
    assert b.status() == 0
    return tuple(b.get_state()) + tuple(b.get_contact()) + tuple(b.get_pivot())


def _close(x, y):
    return np.abs(x - y).max() / max(1.0, np.abs(y).max())


@pytest.fixture(scope="module", params=["arm_press", "config3"])
def case(R, request):
    sc = _scenario(R, request.param)
    P = ip.randomised(sc["world"], B, seed=0xD0 + len(request.param))
    t1 = _run(ParEmuBatch(sc["world"], B, max_rigid=sc["max_rigid"], ipw=1, params=P), sc)
    return request.param, sc, P, t1


def test_instance_equals_single_model_run(R, case):
    name, sc, P, t1 = case
    m = sc["world"].model.contents
    assert any(ip.of_instance(P, 0)["mass"][i] != ip.model_values(sc["world"], "mass")[i] for i in range(m.nlink))
    for i in range(B):
        mc = ip.model_with(sc["world"], ip.of_instance(P, i))
        one = _run(EmuBatch(mc, 1, max_rigid=sc["max_rigid"]), sc, i, i + 1)
        for k, (x, y) in enumerate(zip(t1, one)):
            assert np.array_equal(x[i], y[0]), (name, i, k)
    # ... and the parameters matter: the instances started alike do not end alike
    plain = _run(EmuBatch(sc["world"], B, max_rigid=sc["max_rigid"]), sc)
    assert not np.array_equal(plain[0], t1[0])


def test_two_instances_per_wavefront_equal_one(R, case):
    name, sc, P, t1 = case
    t2 = _run(ParEmuBatch(sc["world"], B, max_rigid=sc["max_rigid"], ipw=2, params=P), sc)
    for k, (x, y) in enumerate(zip(t1, t2)):
        assert np.array_equal(x, y), (name, k)


@pytest.mark.parametrize("ipw", [1, 2])
def test_table_of_model_rows_equals_no_table(R, case, ipw):
    name, sc, P, t1 = case
    plain = _run(EmuBatch(sc["world"], B, max_rigid=sc["max_rigid"], ipw=ipw), sc)
    same = _run(ParEmuBatch(sc["world"], B, max_rigid=sc["max_rigid"], ipw=ipw, params={}), sc)
    none = _run(ParEmuBatch(sc["world"], B, max_rigid=sc["max_rigid"], ipw=ipw, params=None), sc)
    for k, (x, y, z) in enumerate(zip(plain, same, none)):
        assert np.array_equal(x, y) and np.array_equal(x, z), (name, k)


def test_instances_agree_with_the_oracle_on_the_model_copy(R, oracle_cls, case):
    name, sc, P, t1 = case
    dis, vel, acc, act, typ, ref, f = t1[:7]
    for i in range(B):
        mc = ip.model_with(sc["world"], ip.of_instance(P, i))
        o = oracle_cls(mc.model)
        o.set_state(sc["dis"][i], sc["vel"][i])
        if "motor_in" in sc:
            o.set_motor_input(np.asarray(sc["motor_in"])[i])
        o.update_init()
        for _ in range(H):
            o.update()
        od, ov, oa = o.get_state()
        errs = {"dis": _close(dis[i], od), "vel": _close(vel[i], ov), "acc": _close(acc[i], oa)}
        print(name, i, errs)
        assert max(errs.values()) < RTOL, (name, i, errs)
        oact, otyp, oref, of = o.get_contact()[:4]
        assert np.array_equal(act[i], oact), (name, i)
        assert _close(f[i], of) < RTOL, (name, i)
