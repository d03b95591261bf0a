"""Known-answer tests pinning the CPU oracle (the reference ships none: SURVEY.md 8c).
Independent mechanics: tests/refmath.py (classical Newton-Euler inverse dynamics)."""
import os
import tempfile

import numpy as np
import pytest

import refmath as rm

G = 9.80665


def _world(R, files, ci=None, solver=None, **kw):
    w = R.World(solver=R.SOLVER_MLCP if solver is None else solver, **kw)
    if ci:
        w.contact_info(os.path.join(R.scenarios.MODELS, ci))
    ids = [w.reg_file(f if os.path.isabs(f) else os.path.join(R.scenarios.MODELS, f)) for f in files]
    return w, ids


def test_free_fall_box(R, oracle_cls):
    """(1) float box in free fall: qdd = (0,0,-g,0,0,0) whatever the attitude / spin-free velocity"""
    w, _ = _world(R, ["box.ztk", "floor.ztk"], "contactinfo.ztk")
    o = oracle_cls(w.model)
    dis = np.array([0.3, -0.2, 1.0, 0.3, -0.2, 0.5]); vel = np.array([0.1, 0.2, 0.3, 0, 0, 0])
    o.set_state(dis, vel); o.update_init()
    acc = o.get_state()[2]
    assert np.allclose(acc, [0, 0, -G, 0, 0, 0], atol=1e-12)


def test_aba_vs_newton_euler_chain30(R, oracle_cls):
    """(2) joint accelerations of the articulated-body sweeps satisfy the independent inverse dynamics"""
    sc = R.scenarios.config2(batch=4)
    md = rm.model_arrays(sc["world"].model.contents)
    o = oracle_cls(sc["world"].model)
    for b in range(4):
        o.set_state(sc["dis"][b], sc["vel"][b]); assert o.eval(False) == 0
        qdd = o.get_state()[2]
        tau = rm.rnea(md, sc["dis"][b], sc["vel"][b], qdd)
        assert np.abs(tau).max() < 1e-10 * max(1.0, np.abs(qdd).max())


@pytest.fixture(scope="module")
def humanoid_nomotor(R):
    txt = open(os.path.join(R.scenarios.MODELS, "humanoid30.ztk")).read()
    txt = "\n".join(l for l in txt.splitlines() if not l.strip().startswith("motor:"))
    d = tempfile.mkdtemp()
    p = os.path.join(d, "h30_nomotor.ztk")
    open(p, "w").write(txt)
    return p


def test_aba_vs_newton_euler_float_humanoid(R, oracle_cls, humanoid_nomotor):
    """(2) same on the 30-DoF floating-base tree (float joint bias terms, branches)"""
    w, _ = _world(R, [humanoid_nomotor], solver=R.SOLVER_VERT)
    md = rm.model_arrays(w.model.contents)
    o = oracle_cls(w.model)
    rng = np.random.default_rng(7)
    for _ in range(4):
        q = rng.uniform(-1, 1, 30); qd = rng.uniform(-2, 2, 30)
        o.set_state(q, qd); assert o.eval(False) == 0
        qdd = o.get_state()[2]
        assert np.abs(rm.rnea(md, q, qd, qdd)).max() < 1e-10 * max(1.0, np.abs(qdd).max())


def test_aba_vs_newton_euler_float_humanoid_with_motors(R, oracle_cls):
    """(2) the same with the humanoid's DC motors driven (inputs beyond the +-24 V limits too): input torque, back-EMF torque and
    the rotor inertia reflected through the gear (refmath.actuator_torque, [UNVERIFIED-DEP] DEVIATIONS.md item 5).  A DC-motor
    joint with joint friction carries a friction torque nobody reports: on its coordinate the balance is held to the limit the
    reference's rule leaves for the pivot state (src/rkfd_util.c:345-352), every other coordinate must close"""
    w, _ = _world(R, ["humanoid30.ztk"], solver=R.SOLVER_VERT)
    m = w.model.contents
    md = rm.model_arrays(m)
    o = oracle_cls(w.model)
    rng = np.random.default_rng(8)
    closed = 0
    for _ in range(4):
        q = rng.uniform(-1, 1, 30); qd = rng.uniform(-2, 2, 30); inp = rng.uniform(-30, 30, m.nlink)
        o.set_state(q, qd); o.set_motor_input(inp); assert o.eval(False) == 0
        qdd = o.get_state()[2]; piv = o.get_pivot()[0]
        r = rm.rnea(md, q, qd, qdd) - rm.actuator_torque(md, qd, qdd, inp)
        tol = 1e-10 * max(1.0, np.abs(qdd).max())
        for l in range(m.nlink):
            for k in range(md["dofoff"][l], md["dofoff"][l] + (6 if md["jtype"][l] == rm.FLOAT else int(md["jtype"][l] in (rm.REVOL, rm.PRISM)))):
                if md["mtype"][l] == rm.MOTOR_DC and (md["stiff"][l] or md["visc"][l] or md["coulomb"][l] or md["sfric"][l]):
                    fmax = md["sfric"][l] if piv[l] == 0 else abs(md["stiff"][l] * q[k] + md["visc"][l] * qd[k] + md["coulomb"][l] * np.sign(qd[k]))
                    assert abs(r[k]) <= abs(fmax) + tol, (l, r[k], fmax)
                else:
                    assert abs(r[k]) < tol, (l, r[k]); closed += 1
    assert closed >= 24 and (md["mtype"] == rm.MOTOR_DC).any()


def test_probed_matrix_is_J_Minv_JT(R, oracle_cls, humanoid_nomotor):
    """(3) the column-by-column probed contact matrix equals J M^-1 J' + L, symmetric PSD"""
    w, (h, f) = _world(R, [humanoid_nomotor, "floor.ztk"], "contact_rigid.ztk")
    m = w.model.contents
    md = rm.model_arrays(m)
    o = oracle_cls(w.model)
    q = np.zeros(30); q[2] = 0.3667 - 0.002   # soles 2 mm into the floor
    o.set_state(q, np.zeros(30)); assert o.eval(False) == 0
    nc, a, b, fv = o.mlcp()
    assert nc >= 4
    assert np.abs(a - a.T).max() < 1e-9 * np.abs(a).max()
    act, typ, ref, fw = o.get_contact()
    Rw, pw = o.link_frames()
    # rebuild J' columns with the independent inverse dynamics
    cand_pair = m.arr("cand_pair", m.ncand); cand_side = m.arr("cand_side", m.ncand); cand_vert = m.arr("cand_vert", m.ncand)
    pair_shape = m.arr("pair_shape", 2 * m.npair).reshape(-1, 2); shape_link = m.arr("shape_link", m.nshape)
    verts = m.arr("verts", 3 * (m.arr("shape_voff", m.nshape + 1)[-1])).reshape(-1, 3)
    M = rm.mass_matrix(md, q)
    cols = []
    for j in np.nonzero(act)[0]:
        la = shape_link[pair_shape[cand_pair[j], cand_side[j]]]
        x = pw[la] + Rw[la] @ verts[cand_vert[j]]
        n = np.array([0, 0, 1.0]); t1 = np.array([1.0, 0, 0]); t2 = np.array([0, 1.0, 0])
        cols.append(rm.point_jacobian_T(md, q, la, x, [n, t1, t2]))
    JT = np.concatenate(cols, axis=1)
    a_ref = JT.T @ np.linalg.solve(M, JT) + 1e-4 * np.eye(3 * nc)
    assert np.abs(a - a_ref).max() < 1e-8 * np.abs(a_ref).max()
    assert np.linalg.eigvalsh((a + a.T) / 2).min() > 0


def test_box_rests_on_rigid_floor(R, oracle_cls):
    """(4) box on the rigid floor (K=1000, L=1e-4): it neither sinks nor bounces away, all four
    bottom vertices stay in contact, the normal force of the committing evaluation stays of the
    order of m g (0.5..2 m g) and there is no net tangential force.  (The velocity-level LCP with
    relaxation, re-solved at every Runge-Kutta stage, settles into a micrometre-scale 4-step limit
    cycle; the committing evaluation samples it, so equality with m g is not expected.)"""
    w, _ = _world(R, ["box.ztk", "floor.ztk"], "contactinfo.ztk")
    o = oracle_cls(w.model)
    o.set_state(np.array([0, 0, 0.0499, 0, 0, 0.0]), np.zeros(6)); o.update_init()
    fz = []
    for k in range(1500):
        assert o.update() == 0
        if k >= 1000:
            fz.append(o.get_contact()[3][:, 2].sum())
    act, typ, ref, f = o.get_contact()
    dis, vel, _ = o.get_state()
    assert act.sum() == 4
    assert 0.5 * 0.5 * G < min(fz) and max(fz) < 2.0 * 0.5 * G
    assert np.abs(f[:, :2].sum(0)).max() < 1e-6
    assert abs(dis[2] - 0.05) < 1e-5 and np.abs(vel).max() < 5e-3


def test_pgs_fixed_iteration_iterate(R, oracle_cls):
    """(5) the MLCP force is the 10-sweep projected Gauss-Seidel iterate (not the fixed point):
    re-run the reference's loop (reference src/rkfd_mlcp.c:190-249) in Python on the oracle's a, b"""
    sc = R.scenarios.config4(batch=1)
    o = oracle_cls(sc["world"].model)
    m = sc["world"].model.contents
    o.set_state(sc["dis"][0], sc["vel"][0])
    o.eval(False)                      # creates the contacts (all sticking)
    act0, typ0, ref0, _ = o.get_contact()
    o.eval(False)
    nc, a, b, f = o.mlcp()
    mu = [0.5 if t == 0 else 0.3 for t in typ0[act0 > 0]]
    TOL = 1e-12
    x = np.zeros(3 * nc)
    for _ in range(m.max_iter):
        for c in range(nc):
            k = 3 * c
            ff = -(b[k] + a[k] @ x - a[k, k] * x[k]) / a[k, k]
            x[k] = 0.0 if ff < TOL else ff
        for c in range(nc):
            k = 3 * c
            ff = [0.0 if abs(a[k + i, k + i]) < TOL else -(b[k + i] + a[k + i] @ x - a[k + i, k + i] * x[k + i]) / a[k + i, k + i] for i in (1, 2)]
            fn = ff[0] ** 2 + ff[1] ** 2; fs = (mu[c] * x[k]) ** 2
            if fn < TOL or fs < TOL:
                x[k + 1] = x[k + 2] = 0.0
            elif fn > fs:
                x[k + 1], x[k + 2] = ff[0] * fs / fn, ff[1] * fs / fn
            else:
                x[k + 1], x[k + 2] = ff
    assert np.allclose(x / m.dt, f, rtol=1e-12, atol=1e-12 * np.abs(f).max())


def test_penalty_single_vertex(R, oracle_cls):
    """(6) penalty force of one vertex, hand-computed: f = -E d - (V + E dt) v_rel (reference
    src/rkfd_penalty.c:23-24) with E=100, V=1, dt=1e-3 ('soft body', contactinfo.ztk)"""
    sc = R.scenarios.config1(batch=1)
    o = oracle_cls(sc["world"].model)
    dis = np.array([0, -1.0, 0.05 - 0.004, 0, 0, 0]); vel = np.array([0.0, 0, -0.2, 0, 0, 0])
    o.set_state(dis, vel); o.eval(False)
    act, typ, ref, f = o.get_contact()
    idx = np.nonzero(act)[0]
    assert len(idx) == 4
    E, V, dt = 100.0, 1.0, 1e-3
    expect = -E * (-0.004) - (V + E * dt) * (-0.2)
    assert np.allclose(f[idx, 2], expect, rtol=1e-12)
    assert np.allclose(f[idx, :2], 0, atol=1e-14)
    # leaving contact fast enough flips the sign of the force: no adhesion (the vertex is skipped)
    o2 = oracle_cls(sc["world"].model)
    o2.set_state(dis, np.array([0.0, 0, 1.0, 0, 0, 0])); o2.eval(False)
    assert np.abs(o2.get_contact()[3]).max() == 0.0


def test_rkg_is_fourth_order(R, oracle_cls):
    """(7) frictionless pendulum (first link of chain30 moving, others locked by symmetry is not
    possible) -> use the 2-step error ratio on the full chain: halving dt divides the error by ~16"""
    errs = []
    sc = R.scenarios.config2(batch=1)
    q0, v0 = sc["dis"][0] * 0.3, sc["vel"][0] * 0.3

    def run(dt, n):
        w = R.World(solver=R.SOLVER_VERT, dt=dt)
        w.reg_file(os.path.join(R.scenarios.MODELS, "chain30.ztk"))
        o = oracle_cls(w.model)
        o.set_state(q0, v0); o.update_init()
        for _ in range(n):
            o.update()
        return o.get_state()[0]
    ref = run(1.25e-4, 160)
    for dt, n in ((2e-3, 10), (1e-3, 20)):
        errs.append(np.abs(run(dt, n) - ref).max())
    assert 10.0 < errs[0] / errs[1] < 24.0


def test_dc_motor_friction_truth_table(R, oracle_cls):
    """(8) joint friction of a DC-motor joint (reference src/rkfd_util.c:330-364): at rest with zero
    input the static friction holds the arm against gravity (|needed| < staticfriction) and the
    pivot stays SF; a large input voltage breaks away and the committing evaluation flips it to KF"""
    w, (h, f) = _world(R, ["humanoid30.ztk", "floor.ztk"], "contact_elastic.ztk", solver=R.SOLVER_VERT)
    o = oracle_cls(w.model)
    dis = np.zeros(30); dis[:6] = w.init_dis(h)[:6]; dis[2] = 1.0   # in the air
    o.set_state(dis, np.zeros(30)); o.update_init()
    typ, prev = o.get_pivot()
    m = w.model.contents
    jt = m.arr("jtype", m.nlink)
    assert (typ[jt == 1] == 0).all()
    acc = o.get_state()[2]
    assert np.abs(acc[6:]).max() < 1e-9        # every joint sticks
    inp = np.zeros(m.nlink); inp[1] = 24.0
    o.set_motor_input(inp); o.eval(True)
    typ2, _ = o.get_pivot()
    assert typ2[1] == 1 and abs(o.get_state()[2][6]) > 1.0


def test_flop_counting_build_matches_the_plain_oracle(R):
    """oracle/flopcount.cpp compiles the oracle source with a counting number type: same results bit for
    bit, and a flop count per step of the order SURVEY 8d estimates (~0.1 Mflop for one ABA-only step)"""
    import ctypes as C
    import os
    import subprocess
    import oracle.pyoracle as po
    root = os.path.join(os.path.dirname(__file__), "..")
    subprocess.run(["make", "-C", os.path.join(root, "oracle"), "count"], check=True, stdout=subprocess.DEVNULL)
    sc = R.scenarios.config4(batch=1)
    plain = po.Oracle(sc["world"].model)
    plain.set_state(sc["dis"][0], sc["vel"][0]); plain.update_init(); plain.update_n(5)
    Lc = C.CDLL(os.path.join(root, "oracle", "_build", "librkfd_oracle_count.so"))
    vp = C.c_void_p
    Lc.rkfdOracleCreate.argtypes = [vp]; Lc.rkfdOracleCreate.restype = vp
    Lc.rkfdOracleSetState.argtypes = [vp, vp, vp]; Lc.rkfdOracleGetState.argtypes = [vp, vp, vp, vp]
    Lc.rkfdOracleUpdateInit.argtypes = [vp]; Lc.rkfdOracleUpdateN.argtypes = [vp, C.c_int]; Lc.rkfdOracleDestroy.argtypes = [vp]
    Lc.rkfdOracleFlops.restype = C.c_ulonglong
    o = Lc.rkfdOracleCreate(C.cast(sc["world"].model, vp))
    d = np.ascontiguousarray(sc["dis"][0]); v = np.ascontiguousarray(sc["vel"][0])
    Lc.rkfdOracleSetState(o, d.ctypes.data, v.ctypes.data); Lc.rkfdOracleUpdateInit(o)
    Lc.rkfdOracleFlopsReset(); Lc.rkfdOracleUpdateN(o, 5)
    flops = Lc.rkfdOracleFlops() / 5
    acc = np.empty_like(d); dis = np.empty_like(d); vel = np.empty_like(d)
    Lc.rkfdOracleGetState(o, dis.ctypes.data, vel.ctypes.data, acc.ctypes.data); Lc.rkfdOracleDestroy(o)
    pd, pv, pa = plain.get_state()
    assert np.array_equal(dis, pd) and np.array_equal(acc, pa)
    assert 1e5 < flops < 2e6


def test_spherical_joint_conserves_energy(R, oracle_cls):
    """the oracle's spherical joint (3x3 joint-space inertia, angle-axis coordinates composed as rotations): three links
    with off-axis centres of mass and full inertia tensors swinging freely at ~2 rad/s - total energy (13 J) is conserved
    to 4e-7 J over 0.2 s, and the drift falls 4x when the step is halved: stage states are formed as x (+) h sum c_i k_i
    with rotations COMPOSED (rkChainCatJointDisAll, reference src/rkfd_sim.c:306-320), which is second order on the
    rotation group (the revolute chain, where (+) is plain addition, shows the scheme's 4th order: test above)"""
    import os
    drift = []
    for dt in (2e-3, 1e-3):
        w = R.World(solver=R.SOLVER_MLCP, dt=dt); w.reg_file(os.path.join(R.scenarios.MODELS, "arm_spher.ztk"))
        m = w.model.contents
        mass = m.arr("mass", m.nlink); com = m.arr("com", 3 * m.nlink).reshape(-1, 3); I = m.arr("inertia", 9 * m.nlink).reshape(-1, 3, 3)
        rng = np.random.default_rng(5)
        dis = rng.uniform(-0.6, 0.6, m.ndof); vel = rng.uniform(-2, 2, m.ndof)

        def energy(o):
            Rw, pw = o.link_frames(); v, _ = o.link_vel_acc()
            e = 0.0
            for i in range(m.nlink):
                vc = v[i, :3] + np.cross(v[i, 3:], com[i])
                e += 0.5 * mass[i] * vc @ vc + 0.5 * v[i, 3:] @ I[i] @ v[i, 3:] + mass[i] * 9.80665 * (pw[i] + Rw[i] @ com[i])[2]
            return e
        o = oracle_cls(w.model); o.set_state(dis, vel); o.update_init()
        e0 = energy(o)
        o.update_n(int(round(0.2 / dt)))
        drift.append(abs(energy(o) - e0))
    assert drift[1] < 1e-6 and 3.0 < drift[0] / drift[1] < 32.0, drift


def _wall_world(R, tmp_path, nbrick, thresholds, upright):
    """a row of bricks on breakable float joints (models/gen_models.py: wall) over the floor, MLCP plugin"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_models", os.path.join(R.scenarios.MODELS, "gen_models.py"))
    gm = importlib.util.module_from_spec(spec); spec.loader.exec_module(gm)
    f = tmp_path / "w.ztk"
    f.write_text(gm.wall("w", nbrick, thresholds, upright=upright))
    w = R.World(solver=R.SOLVER_MLCP)
    w.contact_info(os.path.join(R.scenarios.MODELS, "contactinfo.ztk"))
    w.reg_file(str(f)); w.reg_file(os.path.join(R.scenarios.MODELS, "floor.ztk"))
    return w


def test_breakable_float_joint_carries_the_weight_above_it(R, oracle_cls, tmp_path):
    """BREAKABLE FLOAT JOINT, known answers (RoKi's rk_joint_brfloat is not here [UNVERIFIED-DEP]; this pins the restatement
    to mechanics).  A column of three 0.25 kg bricks: the joint of brick k transmits the weight of the bricks from k up -
    3 m g = 7.355 N, 2 m g = 4.903 N, m g = 2.452 N - and no torque (the centres of mass lie on the column's axis).
    Thresholds just above leave everything at rest with zero accelerations; brick 2's threshold just below 2 m g breaks
    THAT joint at the first committing evaluation (rkFDUpdateInit): from the next evaluation on bricks 2 + 3 (brick 3 still
    rigidly attached to brick 2) fall freely, brick 1 stays where it is, and brick 3's joint, which now transmits nothing,
    never breaks."""
    g, ms = 9.80665, 0.25
    w = _wall_world(R, tmp_path, 3, [(3 * ms * g + 0.01, 1.0), (2 * ms * g + 0.01, 1.0), (ms * g + 0.01, 1.0)], True)
    m = w.model.contents
    assert (m.arr("jtype", m.nlink)[:4] == [0, 5, 5, 5]).all() and m.ndof == 18
    o = oracle_cls(w.model); o.set_state(np.zeros(18), np.zeros(18)); o.update_init()
    o.update_n(5)
    assert o.get_broken().sum() == 0 and np.abs(o.get_state()[0]).max() == 0 and np.abs(o.get_state()[2]).max() == 0
    w = _wall_world(R, tmp_path, 3, [(3 * ms * g + 0.01, 1.0), (2 * ms * g - 0.01, 1.0), (ms * g + 0.01, 1.0)], True)
    o = oracle_cls(w.model); o.set_state(np.zeros(18), np.zeros(18)); o.update_init()
    assert o.get_broken().tolist() == [0, 0, 1, 0, 0]               # base, brick 1, brick 2 (broken), brick 3, floor
    assert np.abs(o.get_state()[2]).max() == 0                      # ... from the NEXT evaluation on
    o.update()
    d, v, a = o.get_state()
    # brick 2's six coordinates live in its joint-origin frame, whose x axis points up: falling = -g along x
    assert np.allclose(a[6:12], [-g, 0, 0, 0, 0, 0], atol=1e-12) and np.abs(a[:6]).max() == 0 and np.abs(a[12:]).max() == 0
    assert abs(d[6] + 0.5 * g * 1e-6) < 1e-15 and np.abs(d[:6]).max() == 0 and np.abs(d[12:]).max() == 0
    o.update_n(20)
    assert o.get_broken().tolist() == [0, 0, 1, 0, 0]               # broken for good; brick 3 rides on brick 2 in free fall


def test_breakable_float_joint_torque_threshold(R, oracle_cls, tmp_path):
    """a cantilever of two bricks: the first joint carries the shear force 2 m g = 4.903 N and the bending moment
    m g ( 0.05 + 0.15 ) = 0.4903 N m about the link origin; only the TORQUE threshold decides here"""
    g, ms = 9.80665, 0.25
    tq = ms * g * 0.2
    for thr, want in ((tq + 1e-3, 0), (tq - 1e-3, 1)):
        w = _wall_world(R, tmp_path, 2, [(100.0, thr), (100.0, 100.0)], False)
        o = oracle_cls(w.model); o.set_state(np.zeros(12), np.zeros(12)); o.update_init()
        assert o.get_broken()[1] == want and o.get_broken()[2] == 0
        o.update()
        a = o.get_state()[2]
        if want:      # the two bricks, still rigidly attached to each other, fall without turning: gravity acts at their common centre of mass
            assert np.allclose(a[:6], [0, 0, -g, 0, 0, 0], atol=1e-12) and np.abs(a[6:]).max() == 0
        else:
            assert np.abs(a).max() == 0
