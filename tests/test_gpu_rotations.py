"""Large rotations on the GPU: every quadrant of d_sincos, multi-turn joints, the x < 0 branch of d_atan2_ypos, d_to_aa beyond a quarter
turn and the orientation update through the half turn - with the constants in __constant__ memory, fp contraction and (world-specific
kernels) hipRTC, none of which the lane emulator has.  The cases of tests/test_emu_rotations.py (tests/rot_cases.py) on the generic,
the world-specific, the two-per-wavefront and the parameter-table kernels, and the four read-outs; every batch has 8 instances or
fewer.

Bounds: the read-outs at links_cases.TOL = 1e-12 max( 1, |value|_inf ) against the references of their case modules and against
the emulator on every instance (as tests/test_gpu_links.py, test_gpu_jac.py, test_gpu_dyn.py, test_gpu_cf.py); free-motion rollouts
against the oracle at 1e-8 (tests/test_random_trees.py: test_gpu_on_random_trees), angle-axis blocks compared as rotation matrices;
the kernel variants bit for bit against the generic kernel, as tests/test_gpu_edge.py and tests/test_gpu_params.py promise; one link's
frame against a long double forward kinematics at 2e-15 (one frame product of three terms on values good to 2^-52 each); one step
at zero velocity against the oracle's at max( 1e-12, 1e-14 / ( pi - theta ) ) (tests/test_rot_primitives.py).
Measured: profiles/r13_rot_parity.txt (tools/rot_parity.py)."""
import numpy as np
import pytest

import instance_params as ip
import rot_cases as rc
import solver_paths as sp

pytestmark = pytest.mark.gpu
B = 8
TOL_FREE = 1e-8          # free motion on the GPU against the oracle: the bound of test_gpu_on_random_trees
TOL_PROBE = 2e-15
VARIANTS = ["generic", "specialized", "two_per_wave", "table"]


@pytest.fixture(scope="module")
def cases(R, tmp_path_factory):
    return rc.readout_cases(R, tmp_path_factory.mktemp("rot_trees"), B)


@pytest.mark.parametrize("name", rc.READOUT_WORLDS)
def test_readouts_at_large_rotations(R, oracle_cls, cases, name):
    c = cases[name]
    got = rc.gpu_readouts(R, c)
    dev = rc.check_readouts(R, oracle_cls, c, got, name)
    demu = rc.check_against_emulator(got, rc.emu_readouts(c), name)
    print(name, "references", {k: "%.2e" % v for k, v in dev.items()}, "emulator", {k: "%.2e" % v for k, v in demu.items()})


def test_readouts_at_large_rotations_with_a_parameter_table(R, oracle_cls, cases):
    c = cases["humanoid30"]
    P = ip.randomised(c["world"], B, seed=0x2071)
    got = rc.gpu_readouts(R, c, par=P)
    plain = rc.gpu_readouts(R, c)
    assert np.abs(got["links"]["com"] - plain["links"]["com"]).max() > 1e-5 and np.array_equal(got["links"]["R"], plain["links"]["R"])
    dev = rc.check_readouts(R, oracle_cls, c, got, "humanoid30 + table", par=P)
    demu = rc.check_against_emulator(got, rc.emu_readouts(c, par=P), "humanoid30 + table")
    print("humanoid30 + table: references", {k: "%.2e" % v for k, v in dev.items()}, "emulator", {k: "%.2e" % v for k, v in demu.items()})


# ---- direct probes: one link, one primitive ---------------------------------------------------------------------------------------------
def test_first_joint_of_chain30_isolates_sincos(R):
    """the frame of the link on chain30's first joint (link 1, behind the fixed base) is org_R Rz( q0 ): d_sincos through the links
    kernel, over a sweep of q0 through every quadrant on both signs, every multiple of pi/2 up to 4 pi and up to 1e5 rad"""
    w, dis = rc.sincos_probe_states(R)
    k = np.rint(dis[:, 0] * (2 / np.pi)).astype(np.int64)
    assert {int(q) for q in k[k > 0] & 3} == {int(q) for q in k[k < 0] & 3} == {0, 1, 2, 3}
    e = rc.probe_error(R, w, dis)
    print(f"first joint of chain30 over q0: {e:.2e}")
    assert e <= TOL_PROBE, e


def test_base_link_of_a_box_isolates_from_aa(R):
    """the base link's frame is org_R R( aa ), org_p + org_R t: d_from_aa through the links kernel for theta = 0 ... 7 rad"""
    w, dis = rc.from_aa_probe_states(R)
    e = rc.probe_error(R, w, dis)
    print(f"base link of a free box over theta: {e:.2e}")
    assert e <= TOL_PROBE, e


@pytest.mark.parametrize("specialized", [False, True])
def test_one_step_at_rest_isolates_to_aa(R, oracle_cls, specialized):
    e_or, e_start, bound = rc.to_aa_probe(R, oracle_cls, specialized)
    print("one step at rest: against the oracle", e_or, "against the start", e_start, "bound", bound)
    assert (e_or <= bound).all() and (e_start <= bound).all(), (e_or, e_start, bound)


# ---- rollouts -------------------------------------------------------------------------------------------------------------------------
ROLLOUTS = {"chain30": (rc.chain30_rollout, 3, 1), "humanoid": (rc.humanoid_rollout, 5, 1), "tumbling_box": (rc.tumbling_box, 5, 4)}


@pytest.fixture(scope="module")
def rollouts(R, oracle_cls):
    """name -> (scene, the oracle's trajectory, the generic kernel's final state): computed once per scene, never written to"""
    cache = {}

    def get(name):
        if name not in cache:
            make, n, chunks = ROLLOUTS[name]
            sc = make(R, n)
            cache[name] = (sc, rc.oracle_trajectory(oracle_cls, sc), rc.run_variant(R, sc, "generic", chunks))
        return cache[name]
    return get


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(ROLLOUTS))
def test_free_rollouts_at_large_angles(R, rollouts, name, variant):
    """chain30 at +-40 rad, the airborne humanoid with its base at theta = 2.2 and 3.1 turning at 15 rad/s, the box tumbling through
    the half turn (400 steps as four launches of 100; the gates on the oracle's trajectory as in tests/test_emu_rotations.py)"""
    sc, tr, generic = rollouts(name)
    assert tr["ncontact"] == 0
    if name == "tumbling_box":
        rc.assert_tumble_gates(tr["dis"])
    got = generic if variant == "generic" else rc.run_variant(R, sc, variant, ROLLOUTS[name][2])
    d = rc.state_dev(R, sc["world"].model.contents, got, tuple(tr[k][:, -1] for k in ("dis", "vel", "acc")))
    print(f"{sc['name']} {variant}: {d:.2e}")
    assert d < TOL_FREE, d
    for k, (x, y) in enumerate(zip(got, generic)):
        assert np.array_equal(x, y), (name, variant, k)


@pytest.mark.parametrize("specialized", [False, True])
def test_upside_down_box_on_the_floor(R, specialized):
    """|aa| = 3.06, 3.11 and 2.42 with contacts (MLCP): after update_init and after 6 steps through solver_paths.compare"""
    sc = rc.upside_down_box(R)
    ors = sp.oracles(sc["world"], sc["dis"], sc["vel"])
    b = R.Batch(sc["world"], 3, device=0, max_rigid=sc["max_rigid"])
    if specialized:
        b.specialize()
    b.set_state(sc["dis"], sc["vel"]); b.update_init()
    assert sum(int((o.get_contact()[0] != 0).sum()) for o in ors) > 0
    w0 = sp.compare(b, ors, "upside-down box, init")
    b.update(6)
    assert b.status() == 0
    for o in ors:
        o.update_n(6)
    assert sum(int((o.get_contact()[0] != 0).sum()) for o in ors) > 0
    w6 = sp.compare(b, ors, "upside-down box, 6 steps")
    print(f"upside-down box specialized={specialized}: init {w0:.2e}, 6 steps {w6:.2e}")
    b.close()


@pytest.mark.parametrize("specialized", [False, True])
def test_half_turn_is_written_back_as_the_identity(R, oracle_cls, specialized):
    """PINS A KNOWN DEVIATION (DEVIATIONS.md, "A half turn is written back as the identity"), as
    tests/test_emu_rotations.py::test_emulated_half_turn_is_written_back_as_the_identity does under the emulator: a free box at aa =
    ( pi, 0, 0 ) at rest, and one at pi - 1e-6 turning at 1e-3 rad/s about its axis, have aa exactly 0 after one step, on the device
    and in the oracle, and go on from the identity; one at pi - 1e-3 does not collapse.  A fix of d_to_aa must change this test with it."""
    w = rc.free_box_world(R)
    dis, vel = rc.half_turn_states()
    got, ref = [], []
    for steps in (1, 2):
        b = R.Batch(w, dis.shape[0], device=0, max_rigid=0)
        if specialized:
            b.specialize()
        b.set_state(dis, vel); b.update_init(); b.update(steps)
        assert b.status() == 0
        got.append(b.get_state()[0]); b.close()
        od = []
        for i in range(dis.shape[0]):
            o = oracle_cls(w.model); o.set_state(dis[i], vel[i]); o.update_init(); o.update_n(steps)
            od.append(o.get_state()[0]); o.close()
        ref.append(np.stack(od))
    rc.check_half_turn(got[0], got[1], ref[0], ref[1])


def test_free_flight_keeps_the_angular_momentum(R, oracle_cls):
    """gravity has no moment about the centre of mass: R ( I w ) of the tumbling box is constant but for the integrator's error, which
    the oracle has as well - the device may drift twice as far as the oracle plus 1e-12, per instance, over the 400 steps"""
    sc = rc.tumbling_box(R, 5)
    tr = rc.oracle_trajectory(oracle_cls, sc, frames=True)
    rc.assert_tumble_gates(tr["dis"])
    m = sc["world"].model.contents
    dor = rc.drift(rc.angular_momentum(m, tr["R"], tr["v"]))
    dgpu = rc.device_momentum_drift(R, sc)
    print("angular momentum drift over 400 steps: device", dgpu, "oracle", dor)
    assert (dor > 0).all() and (dor < 1e-3).all()          # a drift there is, and momentum is what is being conserved
    assert (dgpu <= 2 * dor + 1e-12).all(), (dgpu, dor)
