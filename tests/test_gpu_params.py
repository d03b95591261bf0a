"""Per-instance physical parameters on the MI355X (rkfdBatchSetParam, rkfdNodeSetParam): instance i of a batch that carries parameters
P_i gives, bit for bit, what a plain batch built on a copy of the model holding P_i gives - under the generic and the world-specific
kernels, one and two instances per wavefront (odd batch: the stand-in half), split launches and fused steps - and agrees with the
unchanged oracle on that copy within the tolerances of tests/test_gpu_solver_paths.py."""
import numpy as np
import pytest

import instance_params as ip

pytestmark = pytest.mark.gpu

STATE_TOL, FORCE_TOL = 1e-9, 1e-8


def _batch(R, world, sc, B, lo=0, split=1, spl=None, kernel="generic", params=None, init=True):
    b = R.Batch(world, B, device=0, max_rigid=sc["max_rigid"])
    if params is not None:
        for n, v in params.items():
            b.set_param(n, v)
    if kernel == "ipw2":
        b.set_instances_per_wave(2)
    if kernel in ("spec", "ipw2"):
        b.specialize()
    if split > 1:
        b.set_split(split)
    if spl:
        b.set_steps_per_launch(spl)
    b.set_state(sc["dis"][lo:lo + B], sc["vel"][lo:lo + B])
    if "motor_in" in sc:
        b.set_motor_input(np.asarray(sc["motor_in"])[lo:lo + B])
    if init:
        b.update_init()
    return b


def _result(b):
    st = b.status()
    return (st,) + tuple(b.get_state()) + tuple(b.get_contact()) + tuple(b.get_pivot())


def _same(x, y):
    assert x[0] == y[0]
    for k, (p, q) in enumerate(zip(x[1:], y[1:])):
        assert np.array_equal(p, q), k


def _same_instance(x, i, y):
    """instance i of result x against the single instance of result y"""
    assert x[0] == y[0]
    for k, (p, q) in enumerate(zip(x[1:], y[1:])):
        assert np.array_equal(p[i], q[0]), (i, k)


def _singles(R, sc, P, picks, H, kernel="generic"):
    """plain batches of one instance built on model_with(P_i), from that instance's start state"""
    out = {}
    for i in picks:
        mc = ip.model_with(sc["world"], ip.of_instance(P, i))
        b = _batch(R, mc, sc, 1, lo=i, kernel=kernel)
        assert not b.has_params()
        b.update(H)
        out[i] = _result(b)
        b.close()
    return out


C4_B, C4_H, C4_PICKS = 41, 7, (0, 1, 20, 39, 40)


@pytest.fixture(scope="module")
def c4(R):
    sc = R.scenarios.config4(batch=C4_B)
    P = ip.randomised(sc["world"], C4_B, seed=0xC4)
    plain = _batch(R, sc["world"], sc, C4_B); plain.update(C4_H); plain_result = _result(plain); plain.close()
    return sc, P, _singles(R, sc, P, C4_PICKS, C4_H), plain_result


@pytest.mark.parametrize("kernel", ["generic", "spec", "ipw2"])
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("spl", [1, 5])
def test_config4_instances_equal_batches_on_model_copies(R, c4, kernel, split, spl):
    sc, P, want, plain = c4
    b = _batch(R, sc["world"], sc, C4_B, split=split, spl=spl, kernel=kernel, params=P)
    assert b.has_params()
    if kernel == "ipw2":
        assert b.instances_per_wave() == 2
    b.update(C4_H)
    got = _result(b)
    for i in C4_PICKS:
        _same_instance(got, i, want[i])
    # the parameters matter: no compared instance ends where the same instance of a plain batch ends
    for i in C4_PICKS:
        assert not np.array_equal(got[2][i], plain[2][i]), i
    b.close()


@pytest.mark.parametrize("kernel", ["spec", "ipw2"])
@pytest.mark.parametrize("split", [1, 3])
def test_config4_table_set_after_specialize(R, c4, kernel, split):
    """specialize first, set_param afterwards: the batch swaps its world-specific kernel for the one built for batches with a
    table (and back on clear_params), keeps the instances per wavefront, and gives the same bits"""
    sc, P, want, plain = c4
    b = _batch(R, sc["world"], sc, C4_B, split=split, spl=5, kernel=kernel, init=False)
    assert not b.has_params()
    for n, v in P.items():
        b.set_param(n, v)
    assert b.has_params() and b.instances_per_wave() == (2 if kernel == "ipw2" else 1)
    b.update_init(); b.update(C4_H)
    got = _result(b)
    for i in C4_PICKS:
        _same_instance(got, i, want[i])
    b.close()
    # ... and a table that goes again after the kernel for it was built
    c = _batch(R, sc["world"], sc, C4_B, split=split, spl=5, kernel=kernel, init=False)
    c.set_param("mass", P["mass"])
    c.clear_params()
    assert c.instances_per_wave() == (2 if kernel == "ipw2" else 1)
    c.update_init(); c.update(C4_H)
    _same(_result(c), plain)
    c.close()


@pytest.mark.parametrize("name", ["config4_vert", "config4_volume"])
@pytest.mark.parametrize("kernel", ["generic", "spec"])
def test_vert_and_volume_instances_equal_batches_on_model_copies(R, name, kernel):
    B, H, picks = 5, 4, (0, 2, 4)
    sc = getattr(R.scenarios, name)(batch=B)
    P = ip.randomised(sc["world"], B, seed=0xB0 + len(name))
    want = _singles(R, sc, P, picks, H, kernel=kernel)
    b = _batch(R, sc["world"], sc, B, kernel=kernel, params=P)
    b.update(H)
    got = _result(b)
    for i in picks:
        _same_instance(got, i, want[i])
    b.close()


def _close(x, y):
    return np.abs(x - y).max() / max(1.0, np.abs(y).max())


@pytest.mark.parametrize("name", ["config4", "config3", "arm_press"])
def test_instances_agree_with_the_oracle_on_model_copies(R, oracle_cls, name):
    B, H = 4, 6
    sc = R.scenarios.arm_press(batch=B) if name == "arm_press" else getattr(R.scenarios, name)(batch=B)
    P = ip.randomised(sc["world"], B, seed=0x0A + len(name))
    b = _batch(R, sc["world"], sc, B, params=P)
    first = _result(b)
    b.update(H)
    last = _result(b)
    b.close()
    for i in range(B):
        mc = ip.model_with(sc["world"], ip.of_instance(P, i))
        o = oracle_cls(mc.model)
        o.set_state(sc["dis"][i], sc["vel"][i])
        if "motor_in" in sc:
            o.set_motor_input(np.asarray(sc["motor_in"])[i])
        o.update_init()
        for stage, got in (("first evaluation", first), ("six steps", last)):
            if stage == "six steps":
                for _ in range(H):
                    o.update()
            od, ov, oa = o.get_state()
            oact, otyp, oref, of = o.get_contact()[:4]
            errs = dict(dis=_close(got[1][i], od), vel=_close(got[2][i], ov), acc=_close(got[3][i], oa), f=_close(got[7][i], of))
            print(name, i, stage, errs)
            assert got[0] == 0
            assert np.array_equal(got[4][i], oact), (name, i, stage)
            assert errs["dis"] < STATE_TOL and errs["vel"] < STATE_TOL, (name, i, stage, errs)
            assert errs["acc"] < FORCE_TOL and errs["f"] < FORCE_TOL, (name, i, stage, errs)


@pytest.mark.parametrize("kernel", ["generic", "ipw2"])
def test_control_schedule_with_a_table_equals_stepwise(R, kernel):
    B, H = 9, 6
    sc = R.scenarios.config4(batch=B)
    P = ip.randomised(sc["world"], B, seed=0xC7)
    m = sc["world"].model.contents
    u = np.random.default_rng(3).normal(0.0, 0.5, (B, H, m.nlink))
    a = _batch(R, sc["world"], sc, B, split=3, spl=5, kernel=kernel, params=P)
    a.update_controlled(u)
    s = _batch(R, sc["world"], sc, B, kernel=kernel, params=P)
    for k in range(H):
        s.set_motor_input(u[:, k, :]); s.update(1)
    _same(_result(a), _result(s))
    a.close(); s.close()


def test_lifecycle(R):
    B, H = 7, 5
    sc = R.scenarios.config4(batch=B)
    w = sc["world"]
    P = ip.randomised(w, B, seed=0x1F)
    plain = _batch(R, w, sc, B); plain.update(H); want_plain = _result(plain); plain.close()
    tab = _batch(R, w, sc, B, params=P); tab.update(H); want_tab = _result(tab); tab.close()
    assert not np.array_equal(want_plain[1], want_tab[1])

    b = _batch(R, w, sc, B, kernel="spec", params=P)
    # get_param returns what was set; a key never set reads as the model's
    for n in ip.NAMES:
        assert np.array_equal(b.get_param(n), P[n]), n
    b.snapshot()
    b.update(H)
    _same(_result(b), want_tab)
    # snapshot / restore leave the parameters in place ...
    b.restore(); b.update(H)
    _same(_result(b), want_tab)
    # ... and so does the tuning of the instances per wavefront, which also puts the state back
    b.restore(); b.join(); b.status()
    before = _result(b)
    assert b.tune_instances_per_wave(4)[0] in (1, 2)
    assert b.has_params()
    _same(_result(b), before)
    b.update(H)
    _same(_result(b), want_tab)
    b.close()
    # one key back to the model, then all of them: the bits of a batch that never had a table (fresh batches: the state an
    # update_init leaves - friction pivots, contact forces - depends on the parameters it ran with)
    for how in ("none", "clear"):
        c = _batch(R, w, sc, B, kernel="spec", params=P, init=False)
        c.set_param("mass", None)
        assert np.array_equal(c.get_param("mass"), np.tile(ip.model_values(w, "mass"), (B, 1)))
        assert np.array_equal(c.get_param("com"), P["com"])
        if how == "none":
            for n in ip.NAMES:
                c.set_param(n, None)
            assert c.has_params()
        else:
            c.clear_params()
            assert not c.has_params()
        assert np.array_equal(c.get_param("ci_kf"), np.tile(ip.model_values(w, "ci_kf"), (B, 1)))
        c.update_init(); c.update(H)
        _same(_result(c), want_plain)
        c.close()


def test_refusals_leave_the_table_as_it_was(R):
    B, H = 4, 3
    sc = R.scenarios.config4(batch=B)
    w = sc["world"]
    P = ip.randomised(w, B, seed=0x2F)
    ref = _batch(R, w, sc, B, params=P); ref.update(H); want = _result(ref); ref.close()
    b = _batch(R, w, sc, B, params=P)
    massive = int(np.argmax(ip.model_values(w, "mass") > 0))
    bad = {}
    x = P["visc"].copy(); x[2, 3] = np.nan; bad["NaN"] = ("visc", x)
    x = P["ci_k"].copy(); x[1, 0] = np.inf; bad["inf"] = ("ci_k", x)
    x = P["mass"].copy(); x[3, massive] = -1.0; bad["negative mass"] = ("mass", x)
    x = P["mass"].copy(); x[0, massive] = 0.0; bad["zero mass on a massive link"] = ("mass", x)
    for what, (n, v) in bad.items():
        with pytest.raises(R.RkfdError) as e:
            b.set_param(n, v)
        assert str(e.value).startswith("rkfdBatchSetParam:"), (what, str(e.value))
        assert np.array_equal(b.get_param(n), P[n]), what
    with pytest.raises(R.RkfdError) as e:
        b.set_param(13, P["mass"])
    assert "unknown parameter key" in str(e.value)
    with pytest.raises(R.RkfdError):
        b.set_param(-1, None)
    with pytest.raises(ValueError):
        b.set_param("weight", P["mass"])
    b.update(H)
    _same(_result(b), want)
    b.close()
    # a refused first Set leaves the batch without a table
    c = _batch(R, w, sc, B)
    with pytest.raises(R.RkfdError):
        c.set_param("mass", bad["negative mass"][1])
    assert not c.has_params()
    c.close()


def test_node_set_param_equals_one_batch(R):
    total, H = 13, 5
    sc = R.scenarios.config4(batch=total)
    w = sc["world"]
    P = ip.randomised(w, total, seed=0x3F)
    one = _batch(R, w, sc, total, params=P); one.update(H); want = one.get_state(); assert one.status() == 0; one.close()
    n = R.Node(w, total, max_rigid=sc["max_rigid"])
    for name, v in P.items():
        n.set_param(name, v)
    with pytest.raises(R.RkfdError):
        n.set_param("mass", -P["mass"])
    n.set_state(sc["dis"], sc["vel"])
    n.update_init(); n.update(H)
    assert n.status() == 0
    got = n.get_state()
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    n.close()
    n = R.Node(w, total, max_rigid=sc["max_rigid"])
    n.set_param("mass", P["mass"])
    n.clear_params()
    n.set_state(sc["dis"], sc["vel"]); n.update_init(); n.update(H)
    assert n.status() == 0
    plain = _batch(R, w, sc, total); plain.update(H)
    for x, y in zip(n.get_state(), plain.get_state()):
        assert np.array_equal(x, y)
    plain.close(); n.close()
