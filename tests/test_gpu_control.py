"""Control schedules on the MI355X (rkfdBatchUpdateControlled, ...Dev, rkfdNodeUpdateControlled): H x (rkJointMotorSetInput;
rkFDUpdate) in the fused / split launches of rkfdBatchUpdate gives the bits of H x (set_motor_input; update(1)), under every launch
configuration, and agrees with the oracle stepped with per-step inputs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-9


def schedule(sc, B, H, seed, scale=0.5, saturate=False):
    m = sc["world"].model.contents
    rng = np.random.default_rng(seed)
    base = np.asarray(sc.get("motor_in", np.zeros((B, m.nlink))))[:B]
    u = base[:, None, :] + rng.normal(0.0, scale, (B, H, m.nlink))
    if saturate:
        u[rng.random((B, H)) < 0.35] *= 40.0
    return u


def _batch(R, sc, B, split=1, spl=None, kernel="generic"):
    b = R.Batch(sc["world"], B, device=0, max_rigid=sc["max_rigid"])
    if kernel == "ipw2":
        b.set_instances_per_wave(2)
    if kernel in ("spec", "ipw2"):
        b.specialize()
    if split > 1:
        b.set_split(split)
    if spl:
        b.set_steps_per_launch(spl)
    b.set_state(sc["dis"], sc["vel"])
    if "motor_in" in sc:
        b.set_motor_input(sc["motor_in"])
    b.update_init()
    return b


def _stepwise(b, u):
    for k in range(u.shape[1]):
        b.set_motor_input(u[:, k, :])
        b.update(1)


def _result(b):
    st = b.status()
    return (st,) + tuple(b.get_state()) + tuple(b.get_contact()) + tuple(b.get_pivot())


def _same(x, y):
    assert x[0] == y[0]
    for p, q in zip(x[1:], y[1:]):
        assert np.array_equal(p, q)


@pytest.fixture(scope="module")
def c4(R):
    B, H = 40, 7
    sc = R.scenarios.config4(batch=B)
    u = schedule(sc, B, H, seed=41)
    ref = _batch(R, sc, B)
    _stepwise(ref, u)
    want = _result(ref)
    # ... and one plain step more with the last row as the input
    ref.update(1)
    want_next = _result(ref)
    ref.close()
    return sc, B, H, u, want, want_next


@pytest.mark.parametrize("kernel", ["generic", "spec", "ipw2"])
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("spl", [1, 5, 7])
def test_config4_controlled_equals_stepwise(R, c4, kernel, split, spl):
    sc, B, H, u, want, want_next = c4
    b = _batch(R, sc, B, split=split, spl=spl, kernel=kernel)
    if kernel == "ipw2":
        assert b.instances_per_wave() == 2
    b.update_controlled(u)
    _same(_result(b), want)
    # the batch's motor input is the last row now: a plain update continues as the stepwise run does
    b.update(1)
    _same(_result(b), want_next)
    b.close()


@pytest.mark.parametrize("name", ["arm_press", "config3"])
def test_controlled_matches_oracle(R, oracle_cls, name):
    B, H = 4, 6
    sc = R.scenarios.arm_press(batch=B) if name == "arm_press" else R.scenarios.config3(batch=B)
    u = schedule(sc, B, H, seed=5, scale=1.0, saturate=True)
    b = _batch(R, sc, B, split=2, spl=4)
    b.update_controlled(u)
    assert b.status() == 0
    dis, vel, acc = b.get_state()
    for i in range(B):
        o = oracle_cls(sc["world"].model)
        o.set_state(sc["dis"][i], sc["vel"][i])
        if "motor_in" in sc:
            o.set_motor_input(sc["motor_in"][i])
        o.update_init()
        for k in range(H):
            o.set_motor_input(u[i, k]); o.update()
        od, ov, oa = o.get_state()
        for x, y in ((dis[i], od), (vel[i], ov), (acc[i], oa)):
            assert np.abs(x - y).max() / max(1.0, np.abs(y).max()) < RTOL


@pytest.mark.parametrize("cfg", ["config4_vert", "config4_volume"])
def test_plugin_worlds_controlled_equals_stepwise(R, cfg):
    """the Vert plugin's worlds keep one fused launch per part; the Volume plugin's kernel variant"""
    B, H = 8, 6
    sc = R.scenarios.config4_vert(batch=B) if cfg == "config4_vert" else R.scenarios.config4_volume(batch=B)
    u = schedule(sc, B, H, seed=9)
    for split in (1, 3):
        a = _batch(R, sc, B, split=split); a.update_controlled(u)
        s = _batch(R, sc, B, split=split); _stepwise(s, u)
        _same(_result(a), _result(s))
        a.close(); s.close()


def test_mpc_loop_and_back_to_back_calls(R):
    """snapshot, then K schedules each from restore(); and two controlled calls issued back to back without a host sync under split
    launches (the second must not overwrite the first's schedule while its steps still read it)"""
    B, H, K = 48, 25, 3
    sc = R.scenarios.config4(batch=B)
    b = _batch(R, sc, B, split=3, kernel="spec")
    b.snapshot()
    us = [schedule(sc, B, H, seed=100 + k) for k in range(K)]
    outs = []
    for u in us:
        b.restore()
        b.update_controlled(u)
        outs.append(_result(b))
    for u, got in zip(us, outs):
        s = _batch(R, sc, B, split=3, kernel="spec")
        _stepwise(s, u)
        _same(got, _result(s))
        s.close()
    # back to back, no sync in between: u1 then u2
    b.restore()
    b.update_controlled(us[0])
    b.update_controlled(us[1])
    got = _result(b)
    s = _batch(R, sc, B, split=3, kernel="spec")
    _stepwise(s, us[0]); _stepwise(s, us[1])
    _same(got, _result(s))
    b.close(); s.close()


_DEV_CHILD = r"""
import sys
sys.path[:0] = [ROOT, ROOT + "/tests"]
import numpy as np
import torch
torch.cuda.init()      # torch's HIP runtime before the library's first call (as bench.py does)
import rkfd_pkg
from test_gpu_control import schedule, _batch, _result, _same
R = rkfd_pkg.load()
B, H = 32, 10
sc = R.scenarios.config4(batch=B)
u = schedule(sc, B, H, seed=77)
for split in (1, 3):
    a = _batch(R, sc, B, split=split, kernel="spec")
    a.update_controlled(u)
    d = _batch(R, sc, B, split=split, kernel="spec")
    ut = torch.from_numpy(u).to("cuda:0")
    d.update_controlled(ut)
    del ut      # the batch keeps the tensor until its steps are waited for
    _same(_result(a), _result(d))
    a.close(); d.close()
b = _batch(R, sc, B)
for bad in (torch.zeros((B, H, b.nlink), dtype=torch.float32, device="cuda:0"), torch.from_numpy(u), np.zeros((B, H, b.nlink + 1))):
    try:
        b.update_controlled(bad)
    except (TypeError, ValueError):
        continue
    raise AssertionError("accepted a schedule of the wrong dtype / device / shape")
b.close()
print("DEV_OK")
"""


def test_device_schedule_equals_host(R):
    """a float64 torch tensor on the device (the zero-copy path) gives the bits of the host schedule; a fresh child process, so that
    torch's HIP runtime comes up before the library's"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % root + _DEV_CHILD], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DEV_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_node_equals_one_batch(R):
    B, H = 30, 8
    sc = R.scenarios.config4(batch=B)
    u = schedule(sc, B, H, seed=3)
    n = R.Node(sc["world"], B, max_rigid=sc["max_rigid"], devices=[0, 0, 0])
    n.set_state(sc["dis"], sc["vel"])
    n.update_init()
    assert n.status() == 0
    n.update_controlled(u)
    n.update(1)      # continues with the last row
    assert n.status() == 0
    nd, nv, na = n.get_state()
    n.close()
    b = _batch(R, sc, B)
    b.update_controlled(u)
    b.update(1)
    assert b.status() == 0
    for x, y in zip((nd, nv, na), b.get_state()):
        assert np.array_equal(x, y)
    b.close()
