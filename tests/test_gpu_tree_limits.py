"""The tree-size limits of the one-wavefront mapping on the MI355X (tests/tree_limits.py; the emulated twin is
tests/test_emu_tree_limits.py): the sixth pointer-jumping round, all 64 lanes carrying a link, 64 joint coordinates, 96 model
links read out of 64 lanes, 63 spherical pseudo-links, contacts on links of depth 59 and the 32 / 32 edge of two instances per
wavefront - under the generic kernel, the world-specific kernel (hipRTC), two instances per wavefront, a table of per-instance
parameters and a control schedule.  Step state against the oracle within 1e-8 max( 1, |ref|_inf ) after two steps (the bound of
tests/test_random_trees.py for trees on the GPU; the oracle-alone control that carries it is asserted in the emulated twin), the
task-space read-out within its 1e-12; everything that compares device code with device code is bit for bit."""
import numpy as np
import pytest

import instance_params as ip
import links_cases as lc
import tree_limits as tl

pytestmark = pytest.mark.gpu

B = 4
KERNELS = ["generic", "spec"]


def _batch(R, w, dis, vel, max_rigid, kernel="generic", params=None, motor_in=None):
    b = R.Batch(w, dis.shape[0], device=0, max_rigid=max_rigid)
    if params is not None:
        for n, v in params.items():
            b.set_param(n, v)
    if kernel == "ipw2":
        b.set_instances_per_wave(2)
    if kernel in ("spec", "ipw2"):
        b.specialize()
        assert b.instances_per_wave() == (2 if kernel == "ipw2" else 1)
    b.set_state(dis, vel)
    if motor_in is not None:
        b.set_motor_input(motor_in)
    b.update_init()
    return b


def _result(b):
    assert b.status() == 0
    return tuple(b.get_state()) + tuple(b.get_pivot())


def _same(x, y, what):
    for k, (p, q) in enumerate(zip(x, y)):
        assert np.array_equal(p, q), (what, k)


@pytest.fixture(scope="module")
def free(R, oracle_cls, tmp_path_factory):
    """case name -> (world, dis, vel, the oracle's states after the steps): made once, shared, never changed"""
    tmp, made = tmp_path_factory.mktemp("tree_limits"), {}

    def get(case):
        if case.name not in made:
            w = tl.world(R, case, tmp)
            dis, vel = tl.states(w, B)
            made[case.name] = (w, dis, vel, tl.oracle_run(oracle_cls, w, dis, vel))
        return made[case.name]
    return get


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case", tl.FREE, ids=repr)
def test_free_motion_at_the_limits(R, oracle_cls, free, case, kernel):
    w, dis, vel, ref = free(case)
    b = _batch(R, w, dis, vel, 0, kernel)
    b.update(tl.NSTEPS)
    got = _result(b)
    dev = tl.deviation(got[:3], ref)
    print(f"{case.name} {kernel}: gpu {dev:.2e}")
    assert dev < tl.STEP_TOL, (case.name, kernel, dev)
    # the read-out at the stepped state: every model link, also those merged into a lane's body
    b.update_links()
    links = b.get_links()
    lc.check(links, lc.reference(R, oracle_cls, w, got[0], got[1]), f"{case.name} {kernel}")
    lc.check_positions_second_fk(R, w, got[0], links, case.name)
    if case.ipw2 and kernel == "spec":
        b2 = _batch(R, w, dis, vel, 0, "ipw2")
        b2.update(tl.NSTEPS)
        _same(_result(b2), got, case.name + " two instances per wavefront")
        b2.update_links()
        l2 = b2.get_links()
        for k in lc.KEYS:
            assert np.array_equal(l2[k], links[k]), (case.name, k)
        b2.close()
    b.close()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("solver", ["mlcp", "vert"])
@pytest.mark.parametrize("case", tl.CONTACT, ids=repr)
def test_contacts_on_deep_links(R, oracle_cls, tmp_path, case, solver, kernel):
    w, h, dis, vel = tl.seated_world(R, case, tmp_path, B, solver=R.SOLVER_MLCP if solver == "mlcp" else R.SOLVER_VERT)
    m = w.model.contents
    assert m.ndof == case.dims[2] and m.ncand == 16 * len(case.boxes)
    if kernel == "spec" and R.lib().rkfdLdsBytesFor(w.model, 16) > 64 * 1024:
        # (64 coordinates AND a contact solve of 16 vertices: the library keeps such a world on the generic kernel, and says so)
        with pytest.raises(R.RkfdError, match="above 64 KiB of LDS per instance keep the generic kernel"):
            _batch(R, w, dis, vel, 16, kernel)
        return
    b = _batch(R, w, dis, vel, 16, kernel)
    for nsteps in (1, tl.NSTEPS):
        ref = tl.oracle_run(oracle_cls, w, dis, vel, nsteps=nsteps)
        b.update(1)
        assert b.status() == 0
        act, typ, _, f = b.get_contact()
        for i, (_, (oact, otyp, _, of)) in enumerate(ref):
            assert len(tl.rigid_links_in_contact(m, oact, h)) >= 2, (case.name, i)
            assert (act[i] == oact).all() and (typ[i] == otyp * (oact != 0)).all(), (case.name, i)
            assert tl.relerr(f[i], of) < tl.STEP_TOL, (case.name, i)
    dev = tl.deviation(b.get_state(), ref)
    print(f"{case.name} {solver} {kernel}: gpu {dev:.2e}")
    assert dev < tl.STEP_TOL, (case.name, solver, kernel, dev)
    b.update_links()
    d1, v1, _ = b.get_state()
    lc.check(b.get_links(), lc.reference(R, oracle_cls, w, d1, v1), f"{case.name} {solver} {kernel}")
    b.close()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["chain64_fixed32", "chain59f"])
def test_parameter_table_equals_batches_on_model_copies(R, free, name, kernel):
    w, dis, vel, _ = free(tl.BY_NAME[name])
    P = ip.randomised(w, B, seed=0x64)
    b = _batch(R, w, dis, vel, 0, kernel, params=P)
    assert b.has_params()
    b.update(tl.NSTEPS)
    got = _result(b)
    b.close()
    plain = _batch(R, w, dis, vel, 0, kernel)
    plain.update(tl.NSTEPS)
    unchanged = _result(plain)
    plain.close()
    for i in range(B):
        one = _batch(R, ip.model_with(w, ip.of_instance(P, i)), dis[i:i + 1], vel[i:i + 1], 0, kernel)
        assert not one.has_params()
        one.update(tl.NSTEPS)
        want = _result(one)
        one.close()
        for k, (p, q) in enumerate(zip(got, want)):
            assert np.array_equal(p[i], q[0]), (name, i, k)
        assert not np.array_equal(got[1][i], unchanged[1][i]), (name, i)      # (the parameters matter)


@pytest.mark.parametrize("kernel", KERNELS)
def test_control_schedule_on_96_model_links(R, oracle_cls, free, kernel):
    """DC and torque motors on the joints of chain64_fixed32, inputs strided by its 96 model links while 64 lanes step: a schedule
    through update_controlled against the same inputs set step by step, bit for bit - and the stepwise run against the oracle"""
    H = 3
    case = tl.BY_NAME["chain64_fixed32"]
    w, dis, vel, _ = free(case)
    m = w.model.contents
    u = np.random.default_rng(96).normal(0.0, 0.5, (B, H, m.nlink))
    a = _batch(R, w, dis, vel, 0, kernel, motor_in=u[:, 0])
    a.update_controlled(u)
    s = _batch(R, w, dis, vel, 0, kernel, motor_in=u[:, 0])
    for k in range(H):
        s.set_motor_input(u[:, k]); s.update(1)
    got = _result(s)
    _same(_result(a), got, "update_controlled")
    idle = _batch(R, w, dis, vel, 0, kernel)
    idle.update(H)
    assert not np.array_equal(_result(idle)[1], got[1])                     # (the inputs drive something)
    for i in range(B):
        o = oracle_cls(w.model)
        o.set_state(dis[i], vel[i]); o.set_motor_input(u[i, 0]); o.update_init()
        for k in range(H):
            o.set_motor_input(u[i, k])
            assert o.update() == 0
        for x, y in zip(got[:3], o.get_state()):
            assert tl.relerr(x[i], y) < tl.STEP_TOL, (i, tl.relerr(x[i], y))
        o.close()
    a.close(); s.close(); idle.close()
