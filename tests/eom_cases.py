"""The residual of the equation of motion: what a batch reports after an evaluation, checked against independent mechanics.

After rkfdBatchEval at a state (q, qd) a batch holds the accelerations qdd, the contact force of every candidate vertex and
the motor inputs.  tests/refmath.py - a world-frame Newton-Euler inverse dynamics that shares nothing with the oracle or the
device code - must then find

    rnea( q, qd, qdd; external forces = the reported contact forces ) - actuator torques = 0

on every joint coordinate.  The check is algebraic (no integrator, no linear solve), needs no oracle, and covers in one number
the articulated-body sweeps, every joint kind, the contact Jacobian, action and reaction of a pair, the motor model and what a
table of per-instance parameters changes.  tests/test_emu_eom.py runs the cases below under the lane emulator and on the
oracle, tests/test_gpu_eom.py on the GPU.

Conventions.  The force of candidate j acts on the link that owns the vertex (cand_side), at the vertex's world position from
refmath's own forward kinematics; its negative acts on the other link of the pair at the same point.  Coordinates of DC-motor
joints with joint friction (any of stiff, visc, coulomb, sfric non-zero) carry a friction torque the ABI does not report: there
the residual IS the friction torque, and what is asserted is the bound of the reference's rule (src/rkfd_util.c:330-364: the
torque is clamped to +-fmax, fmax = |static friction| while the pivot is RK_CONTACT_SF and |kinetic friction| =
|stiff q + visc qd + coulomb sgn(qd)| (DEVIATIONS.md item 5) while it is RK_CONTACT_KF; 1-DoF joints without a DC motor and
all other joints get no friction, :378-384 with DEVIATIONS.md item 12).  Every other coordinate gets equality.

Volume-plugin worlds are left out: the ABI reports no per-pair wrench under that plugin, so there is nothing to feed the
inverse dynamics with.

Tolerance.  scale s = max(1, largest |term| of the balance) per instance; the oracle's own worst relative residual is measured
per case family (profiles/r07_eom_residuals.txt records the figures), and a batch is allowed 10x that, not less than 1e-12:
the device's world-frame formulation rounds differently from the oracle's link-frame one (tests/test_random_trees.py)."""
import os

import numpy as np

import instance_params as ip
import refmath as rm
from randtree import random_tree_ztk

B = 3                   # odd: with two instances per wavefront the last wavefront's second half is a stand-in
TOL_FLOOR = 1e-12
TOL_FACTOR = 10.0
ORACLE_LIMIT = 1e-8     # an oracle residual beyond this is a finding, not a tolerance
G, BRICK_MASS = 9.80665, 0.25


# ------------------------------------------------------------------------------------------------------------------ worlds
class Setup:
    """a world, B start states and how to reach the state the residual is taken at"""

    def __init__(self, world, dis, vel, max_rigid, nsteps, motor_in=None, params=None, min_active=0, brk=None):
        self.world, self.max_rigid, self.nsteps, self.params, self.min_active, self.brk = world, max_rigid, nsteps, params, min_active, brk
        self.dis = np.ascontiguousarray(dis, dtype=np.float64); self.vel = np.ascontiguousarray(vel, dtype=np.float64)
        self.motor_in = None if motor_in is None else np.ascontiguousarray(motor_in, dtype=np.float64)
        assert self.dis.shape[0] == B
        assert all(not np.array_equal(self.dis[0], self.dis[i]) or not np.array_equal(self.vel[0], self.vel[i]) for i in range(1, B))


def _m(R, name):
    return os.path.join(R.scenarios.MODELS, name)


def _scenario(sc, nsteps, min_active=0, params=None):
    return Setup(sc["world"], sc["dis"], sc["vel"], sc["max_rigid"], nsteps, motor_in=sc.get("motor_in"), params=params, min_active=min_active)


def _orthonormal_frames(txt):
    """random_tree_ztk prints its link frames with ten decimals: rotations that are orthonormal to 1e-10 only.  The oracle and
    the device invert a frame by transposing it, refmath applies it as given, and on such a frame the two differ by the
    defect times the terms of the balance (measured: residuals of 1e-9 relative on these trees where every other world gives
    1e-16) - an artefact of the input, not of the mechanics.  Here every frame is replaced by the nearest rotation (polar
    decomposition), printed with 17 significant digits."""
    out = []; rows = None
    for l in txt.splitlines():
        if l.startswith("frame : {"):
            rows = []
        elif rows is not None and l.startswith("}"):
            A = np.array(rows)
            U, _, Vt = np.linalg.svd(A[:, :3])
            Q = U @ Vt
            out.append("frame : {")
            out.extend(" " + ", ".join(repr(float(x)) for x in list(Q[r]) + [A[r, 3]]) for r in range(3))
            out.append("}")
            rows = None
        elif rows is not None:
            rows.append([float(x) for x in l.split(",")])
        else:
            out.append(l)
    return "\n".join(out) + "\n"


def _tree(R, tmp, seed, nlink, root, nsteps, friction=True, params=False):
    txt = _orthonormal_frames(random_tree_ztk(seed, nlink, root=root, motors=True))
    if not friction:
        txt = "\n".join(l for l in txt.splitlines() if l.split(":")[0].strip() not in ("stiffness", "viscosity", "coulomb", "staticfriction")) + "\n"
    f = tmp / f"eom_tree{seed}.ztk"
    f.write_text(txt)
    w = R.World(solver=R.SOLVER_MLCP)
    w.reg_file(str(f))
    m = w.model.contents
    rng = np.random.default_rng(seed + 4000)
    dis = rng.uniform(-0.8, 0.8, (B, m.ndof)); vel = 0.3 * rng.uniform(-1.0, 1.0, (B, m.ndof))
    inp = rng.uniform(-30.0, 30.0, (B, m.nlink))          # beyond the +-24 V and +-5 N m limits too
    P = None
    if params:
        P = {k: v for k, v in ip.randomised(w, B, seed=seed).items() if k in ("mass", "com", "inertia")}
    return Setup(w, dis, vel, 0, nsteps, motor_in=inp, params=P)


def _config1(R, tmp):
    sc = R.scenarios.config1(batch=B)
    m = sc["world"].model.contents
    dis = sc["dis"].copy(); vel = sc["vel"].copy()
    dis[:, 3:6] *= np.array([1.0, 0.6, 0.2])[:, None]
    for i in range(B):                                    # lowest vertex 2 mm inside the soft floor, sinking and sliding
        dis[i, 2] -= R.scenarios.lowest_vertex_z(m, dis[i], 0) + 0.002
    vel[:, 2] = -0.05; vel[:, 0] = (0.0, 0.1, 0.2)
    return Setup(sc["world"], dis, vel, 0, 3, min_active=1)


def _seam(R, tmp):
    """the world of test_elastic_and_rigid_contacts_in_one_evaluation"""
    w = R.World(solver=R.SOLVER_MLCP); w.contact_info(_m(R, "contactinfo.ztk"))
    w.reg_file(_m(R, "box.ztk")); w.reg_file(_m(R, "floor_hardsoft.ztk"))
    m = w.model.contents
    dis = np.zeros((B, m.ndof)); vel = np.zeros((B, m.ndof))
    dis[:, 2] = 0.05 - 0.0005; dis[:, 5] = np.linspace(0.0, 0.6, B)
    vel[:, 0] = 0.3; vel[:, 5] = 1.0
    return Setup(w, dis, vel, 8, 1, min_active=4)


def _stack(R, tmp):
    """the world of test_stacked_boxes"""
    w = R.World(solver=R.SOLVER_MLCP); w.contact_info(_m(R, "contactinfo.ztk"))
    for f in ("box.ztk", "box_small.ztk", "box_small.ztk", "floor.ztk"):
        w.reg_file(_m(R, f))
    m = w.model.contents
    dis = np.zeros((B, m.ndof)); vel = np.zeros((B, m.ndof))
    dis[:, 0:3] = (0, 0, 0.05 - 0.0005)
    dis[:, 6:9] = (0.01, 0.0, 0.1 + 0.025 - 0.001); dis[:, 9:12] = (0, 0, 0.3)
    dis[:, 12:15] = (-0.02, 0.01, 0.15 + 0.025 - 0.0015); dis[:, 15:18] = (0.1, 0, 0)
    vel[:, 6] = np.linspace(0.0, 0.5, B)
    return Setup(w, dis, vel, 24, 1, min_active=6)


def _vert_box(R, tmp):
    """the world of test_vert_plugin_rigid_qp_box: flat, tilted, tilted and spinning"""
    w = R.World(solver=R.SOLVER_VERT); w.contact_info(_m(R, "contactinfo.ztk"))
    w.reg_file(_m(R, "box.ztk")); w.reg_file(_m(R, "floor.ztk"))
    m = w.model.contents
    dis = np.zeros((B, 6)); vel = np.zeros((B, 6))
    dis[:, 2] = 0.0499
    dis[1:, 3:6] = np.random.default_rng(1).uniform(-0.3, 0.3, (B - 1, 3))
    vel[:, 0] = np.linspace(0.0, 0.4, B); vel[2:, 3:6] = np.random.default_rng(2).uniform(-1, 1, (B - 2, 3))
    for i in range(1, B):
        dis[i, 2] -= R.scenarios.lowest_vertex_z(m, dis[i], 0) + 0.0001
    return Setup(w, dis, vel, 8, 1, min_active=1)


def _wall(R, tmp, nbrick, upright, below):
    """test_oracle_kat.py's _wall_world: bricks on breakable float joints, every threshold that decides just above or just
    below the load the joint carries at rest: the weight of the bricks from it up (column), m g x 0.2 m of bending moment on
    the first joint (cantilever of two).  The instances differ by how far the last brick is lifted (along gravity: the loads stay)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_models", _m(R, "gen_models.py"))
    gm = importlib.util.module_from_spec(spec); spec.loader.exec_module(gm)
    d = -0.01 if below else 0.01
    mg = BRICK_MASS * G
    if upright:
        thr = [((nbrick - k) * mg + d, 1.0) for k in range(nbrick)]
        load = dict(force=[(nbrick - k) * mg for k in range(nbrick)], torque=[0.0] * nbrick)
    else:
        thr = [(100.0, mg * 0.2 + 0.1 * d), (100.0, 100.0)]
        load = dict(force=[2 * mg, mg], torque=[mg * 0.2, mg * 0.05])
    f = tmp / f"eom_wall_{nbrick}_{int(upright)}_{int(below)}.ztk"
    f.write_text(gm.wall("w", nbrick, thr, upright=upright))
    w = R.World(solver=R.SOLVER_MLCP)
    w.contact_info(_m(R, "contactinfo.ztk"))
    w.reg_file(str(f)); w.reg_file(_m(R, "floor.ztk"))
    m = w.model.contents
    dis = np.zeros((B, m.ndof)); vel = np.zeros((B, m.ndof))
    dis[:, 6 * (nbrick - 1) + (0 if upright else 2)] = 0.002 * np.arange(B)
    return Setup(w, dis, vel, 8, 1 if below else 2, brk=dict(below=below, load=load, first=1, nbrick=nbrick))


class Case:
    def __init__(self, name, family, build, contacts=False):
        self.name, self.family, self.build, self.contacts = name, family, build, contacts

    def __repr__(self):
        return self.name


CASES = [
    # free motion, every joint kind
    Case("free_arm_spher", "free", lambda R, t: _scenario(R.scenarios.arm_spher(batch=B, contact=False), 3)),
    Case("free_tree_float8", "free", lambda R, t: _tree(R, t, 11, 8, "float", 0)),
    Case("free_tree_fixed12", "free", lambda R, t: _tree(R, t, 12, 12, "fixed", 2)),
    Case("free_tree_float20", "free", lambda R, t: _tree(R, t, 13, 20, "float", 3)),
    Case("free_tree_revolute9", "free", lambda R, t: _tree(R, t, 14, 9, "revolute", 4)),
    Case("free_tree_fixed16_nofriction", "free", lambda R, t: _tree(R, t, 15, 16, "fixed", 2, friction=False)),
    Case("free_tree_revolute14", "free", lambda R, t: _tree(R, t, 16, 14, "revolute", 1)),
    # rigid contacts, MLCP
    Case("mlcp_config4", "mlcp", lambda R, t: _scenario(R.scenarios.config4(batch=B), 1, min_active=8), contacts=True),
    Case("mlcp_config5", "mlcp", lambda R, t: _scenario(R.scenarios.config5(batch=B), 0, min_active=24), contacts=True),
    Case("mlcp_arm_press_fixed", "mlcp", lambda R, t: _scenario(R.scenarios.arm_press(batch=B, root="fixed", with_box=True), 2, min_active=3), contacts=True),
    Case("mlcp_arm_press_revolute", "mlcp", lambda R, t: _scenario(R.scenarios.arm_press(batch=B, root="revolute", with_box=True), 3, min_active=2), contacts=True),
    Case("mlcp_stacked_boxes", "mlcp", _stack, contacts=True),
    # Vert plugin
    Case("vert_config4", "vert", lambda R, t: _scenario(R.scenarios.config4_vert(batch=B), 1, min_active=8), contacts=True),
    Case("vert_box", "vert", _vert_box, contacts=True),
    # penalty contacts
    Case("penalty_config1", "penalty", _config1, contacts=True),
    Case("penalty_seam_elastic_and_rigid", "penalty", _seam, contacts=True),
    # self-collision
    Case("self_arm_fold", "self", lambda R, t: _scenario(R.scenarios.arm_fold(batch=B), 1, min_active=2), contacts=True),
    # spherical joints in contact
    Case("spher_contact", "spher_contact", lambda R, t: _scenario(R.scenarios.arm_spher(batch=B, contact=True), 2, min_active=3), contacts=True),
    # breakable float joints
    Case("brfloat_column_holds", "brfloat", lambda R, t: _wall(R, t, 3, True, False)),
    Case("brfloat_column_breaks", "brfloat", lambda R, t: _wall(R, t, 3, True, True)),
    Case("brfloat_cantilever_holds", "brfloat", lambda R, t: _wall(R, t, 2, False, False)),
    Case("brfloat_cantilever_breaks", "brfloat", lambda R, t: _wall(R, t, 2, False, True)),
    # parameter table
    Case("params_config4", "params", lambda R, t: _scenario(R.scenarios.config4(batch=B), 1, min_active=8,
                                                              params={k: v for k, v in ip.randomised(R.scenarios.config4(batch=B)["world"], B, seed=0xE0).items() if k in ("mass", "com", "inertia")}), contacts=True),
    Case("params_tree_float20", "params", lambda R, t: _tree(R, t, 13, 20, "float", 2, params=True)),
]
CASE_IDS = [c.name for c in CASES]
FAMILIES = sorted({c.family for c in CASES})
TOOTH_CASES = ("mlcp_config4", "mlcp_arm_press_fixed")
# the launch sequences are short (0 .. 4 steps): every state is set in or next to the configuration of interest, and the lane
# emulator, which runs 64 host threads per instance, takes about a second per evaluation of the humanoid


def case(name):
    return CASES[CASE_IDS.index(name)]


# ------------------------------------------------------------------------------------------------------------- backends
class OracleBatch:
    """B oracles behind the surface of a batch (instance i on the model copy with instance i's parameters)"""

    def __init__(self, oracle_cls, world, batch, max_rigid=0, params=None):
        self.B = batch
        self._keep = [world if params is None else ip.model_with(world, ip.of_instance(params, i)) for i in range(batch)]
        self.o = [oracle_cls(k.model) for k in self._keep]

    def set_state(self, dis, vel):
        for i, o in enumerate(self.o):
            o.set_state(dis[i], vel[i])

    def set_motor_input(self, inp):
        for i, o in enumerate(self.o):
            o.set_motor_input(inp[i])

    def update_init(self):
        for o in self.o:
            o.update_init()

    def update(self, n=1):
        for o in self.o:
            o.update_n(n)

    def eval(self, do_up_ref=False):
        for o in self.o:
            assert o.eval(do_up_ref) == 0

    def status(self):
        return 0

    def get_state(self):
        return tuple(np.array(x) for x in zip(*[o.get_state() for o in self.o]))

    def get_contact(self):
        """like rkfdBatchGetContact: a candidate out of contact has no state (the oracle keeps its last force)"""
        act, typ, ref, f = (np.array(x) for x in zip(*[o.get_contact() for o in self.o]))
        on = act != 0
        return act, typ * on, ref * on[:, :, None], f * on[:, :, None]

    def get_pivot(self):
        return tuple(np.array(x) for x in zip(*[o.get_pivot() for o in self.o]))

    def get_broken(self):
        return np.array([o.get_broken() for o in self.o])


def read_out(b):
    dis, vel, acc = b.get_state(); act, typ, ref, f = b.get_contact()
    return dict(dis=np.array(dis), vel=np.array(vel), acc=np.array(acc), act=np.array(act), f=np.array(f),
                piv=np.array(b.get_pivot()[0]), broken=np.array(b.get_broken()))


def run(su, b):
    """the launch sequence of every case: set_state (+ set_motor_input), update_init, update(n), eval(False), read.
    -> (what the batch holds after the evaluation, what it held after update_init)"""
    b.set_state(su.dis, su.vel)
    if su.motor_in is not None:
        b.set_motor_input(su.motor_in)
    b.update_init()
    assert b.status() == 0
    first = read_out(b)
    if su.nsteps:
        b.update(su.nsteps)
        assert b.status() == 0
    b.eval(False)
    assert b.status() == 0
    return read_out(b), first


# ------------------------------------------------------------------------------------------------------------ the check
class Tables:
    """the index bookkeeping of the candidate contact vertices (as tests/test_oracle_kat.py::test_probed_matrix_is_J_Minv_JT)"""

    def __init__(self, m):
        self.m = m
        nc = m.ncand
        cand_pair = m.arr("cand_pair", nc); cand_side = m.arr("cand_side", nc); cand_vert = m.arr("cand_vert", nc)
        pair_shape = m.arr("pair_shape", 2 * m.npair).reshape(-1, 2); shape_link = m.arr("shape_link", m.nshape)
        nv = m.arr("shape_voff", m.nshape + 1)[-1] if m.nshape else 0
        verts = m.arr("verts", 3 * nv).reshape(-1, 3)
        pair_ci = m.arr("pair_ci", m.npair)
        self.own = np.array([shape_link[pair_shape[cand_pair[j], cand_side[j]]] for j in range(nc)], dtype=int)
        self.other = np.array([shape_link[pair_shape[cand_pair[j], 1 - cand_side[j]]] for j in range(nc)], dtype=int)
        self.vert = np.array([verts[cand_vert[j]] for j in range(nc)]).reshape(nc, 3)
        self.mu = np.array([max(m.arr("ci_sf", m.nci)[pair_ci[cand_pair[j]]], m.arr("ci_kf", m.nci)[pair_ci[cand_pair[j]]]) for j in range(nc)])
        chain = m.arr("chain", m.nlink)
        self.floor = chain == m.nchain - 1            # every world here registers its floor last
        self.jtype = m.arr("jtype", m.nlink); self.mtype = m.arr("mtype", m.nlink); self.dofoff = m.arr("dofoff", m.nlink)


def model_of_instance(su, i):
    m = su.world.model.contents
    P = {} if su.params is None else ip.of_instance(su.params, i)
    return rm.model_arrays(m, mass=P.get("mass"), com=P.get("com"), inertia=P.get("inertia"))


def contact_forces(md, tb, q, act, f, drop_reaction=None):
    """fext of refmath.rnea from the reported forces: f_j on the vertex's owner at the vertex, -f_j on the other link there"""
    R, p, _ = rm.fk(md, q)
    fext = {}
    for j in np.nonzero(act)[0]:
        x = p[tb.own[j]] + R[tb.own[j]] @ tb.vert[j]
        fext.setdefault(int(tb.own[j]), []).append((x, f[j]))
        if drop_reaction != j:
            fext.setdefault(int(tb.other[j]), []).append((x, -f[j]))
    return fext


def residual(su, tb, i, out, rotor=True, drop_reaction=None):
    """-> dict: r [ndof] the balance, s its scale, W the joint wrenches; instance i of the read-out `out`"""
    md = model_of_instance(su, i)
    q, qd, qdd = out["dis"][i], out["vel"][i], out["acc"][i]
    brk = out["broken"][i]
    fext = contact_forces(md, tb, q, out["act"][i], out["f"][i], drop_reaction)
    t_dyn = rm.rnea(md, q, qd, qdd, broken=brk)
    t_all, W = rm.rnea(md, q, qd, qdd, fext=fext, broken=brk, wrench=True)
    inp = np.zeros(md["nlink"]) if su.motor_in is None else su.motor_in[i]
    t_act = rm.actuator_torque(md, qd, qdd, inp, rotor=rotor)
    s = max(1.0, np.abs(t_dyn).max(initial=0.0), np.abs(t_all - t_dyn).max(initial=0.0), np.abs(t_act).max(initial=0.0))
    return dict(r=t_all - t_act, s=s, W=W, md=md)


def friction_bounds(md, tb, q, qd, piv):
    """per joint coordinate: None where the balance must close, else the largest friction torque the reference's rule
    (src/rkfd_util.c:330-364) leaves on it with the pivot in the reported state"""
    bound = [None] * md["ndof"]
    for l in range(md["nlink"]):
        if tb.jtype[l] not in (rm.REVOL, rm.PRISM) or tb.mtype[l] != rm.MOTOR_DC:
            continue
        if not (md["stiff"][l] or md["visc"][l] or md["coulomb"][l] or md["sfric"][l]):
            continue
        k = tb.dofoff[l]
        if piv[l] == 0:       # RK_CONTACT_SF
            bound[k] = abs(md["sfric"][l])
        else:
            bound[k] = abs(md["stiff"][l] * q[k] + md["visc"][l] * qd[k] + md["coulomb"][l] * np.sign(qd[k]))
    return bound


def check_instance(su, tb, i, out, tol, exact_zeros=True, **perturb):
    """every assertion on one instance; -> its relative residual (over the coordinates that must close)"""
    res = residual(su, tb, i, out, **perturb)
    r, s, md = res["r"], res["s"], res["md"]
    q, qd, qdd = out["dis"][i], out["vel"][i], out["acc"][i]
    bound = friction_bounds(md, tb, q, qd, out["piv"][i])
    worst = 0.0
    for k in range(md["ndof"]):
        if bound[k] is None:
            worst = max(worst, abs(r[k]) / s)
            assert abs(r[k]) <= tol * s, f"instance {i} coordinate {k}: residual {r[k]:.3e}, scale {s:.3e}, allowed {tol:.1e} relative"
        else:
            assert abs(r[k]) <= bound[k] + tol * s, f"instance {i} coordinate {k}: friction torque {r[k]:.6e} beyond {bound[k]:.6e}"
    # intact breakable joints: accelerations exactly zero
    for l in range(md["nlink"]):
        if tb.jtype[l] == rm.BRFLOAT and not out["broken"][i][l]:
            assert (qdd[tb.dofoff[l]:tb.dofoff[l] + 6] == 0.0).all(), f"instance {i}: intact breakable joint {l} accelerates"
    # admissibility of the reported forces
    act, f = out["act"][i], out["f"][i]
    if exact_zeros:
        assert (f[act == 0] == 0.0).all(), f"instance {i}: a candidate out of contact reports a force"
    for j in np.nonzero(act)[0]:
        if tb.floor[tb.other[j]] or tb.floor[tb.own[j]]:
            g = f[j] if tb.floor[tb.other[j]] else -f[j]          # the force on the body that lies on the floor
            assert g[2] >= 0.0, f"instance {i} candidate {j}: the floor pulls ({g[2]:.3e})"
            assert np.hypot(g[0], g[1]) <= tb.mu[j] * g[2] + 1e-9 * max(1.0, np.abs(g).max()), f"instance {i} candidate {j}: {g} outside the friction cone (mu {tb.mu[j]})"
    return worst, res


def check_breakable(su, tb, out, first, tol):
    """the breakable-joint cases: refmath's joint wrenches at the state of rkFDUpdateInit against the known loads and the
    thresholds, and the flags the batch reports against what those wrenches predict"""
    info = su.brk
    for i in range(B):
        none = np.zeros_like(first["broken"][i])
        res = residual(su, tb, i, dict(first, broken=np.tile(none, (B, 1))))
        md = res["md"]
        predict = none.copy()
        for k in range(info["nbrick"]):
            l = info["first"] + k
            assert tb.jtype[l] == rm.BRFLOAT
            fn, tn = np.linalg.norm(res["W"][l][0]), np.linalg.norm(res["W"][l][1])
            assert abs(fn - info["load"]["force"][k]) < 1e-9 and abs(tn - info["load"]["torque"][k]) < 1e-9, (i, k, fn, tn)
            predict[l] = int(fn > md["brk_f"][l] or tn > md["brk_t"][l])
        assert (first["acc"][i] == 0.0).all()          # the evaluation of rkFDUpdateInit still ran with every joint intact
        assert np.array_equal(first["broken"][i], predict), (i, first["broken"][i], predict)
        if info["below"]:
            assert predict.sum() >= 1
        else:
            assert predict.sum() == 0 and out["broken"][i].sum() == 0 and (out["acc"][i] == 0.0).all()


def check(su, out, first, tol, exact_zeros=True):
    """every assertion of a case on the read-out of a batch; -> (worst relative residual, active contacts)"""
    tb = Tables(su.world.model.contents)
    worst = 0.0
    for i in range(B):
        w, _ = check_instance(su, tb, i, out, tol, exact_zeros=exact_zeros)
        worst = max(worst, w)
        assert int(out["act"][i].sum()) >= su.min_active, f"instance {i}: {int(out['act'][i].sum())} active contacts, expected at least {su.min_active}"
    if su.brk is not None:
        check_breakable(su, tb, out, first, tol)
    return worst, int(out["act"].sum())


# ---------------------------------------------------------------------------------------------------------- tolerances
_oracle_residuals = {}


def oracle_residuals(R, oracle_cls, tmp):
    """the oracle's worst relative residual of every case, measured once per session: {case name: value}.  Every property
    of check() is asserted on the oracle on the way, with ORACLE_LIMIT as its tolerance."""
    if not _oracle_residuals:
        for c in CASES:
            su = c.build(R, tmp)
            out, first = run(su, OracleBatch(oracle_cls, su.world, B, su.max_rigid, su.params))
            _oracle_residuals[c.name] = check(su, out, first, ORACLE_LIMIT)[0]
    return _oracle_residuals


def family_tolerance(R, oracle_cls, tmp, family):
    """what a batch is allowed in `family`: 10x the oracle's worst relative residual there, at least 1e-12"""
    res = oracle_residuals(R, oracle_cls, tmp)
    return max(TOL_FLOOR, TOL_FACTOR * max(res[c.name] for c in CASES if c.family == family))


def apply_params(b, su):
    if su.params is not None:
        for n, v in su.params.items():
            b.set_param(n, v)
