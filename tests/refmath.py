"""Independent numpy mechanics used to pin the oracle (known-answer tests) and, through the residual of the equation
of motion (tests/eom_cases.py), the device code.

A classical (non-spatial) recursive Newton-Euler inverse dynamics in world coordinates,
written from the textbook vector equations; it shares no code and no formulation with
oracle/rkfd_oracle.c (link-frame articulated-body algorithm) or the device code
(world-frame spatial ABA).  Joint conventions are those of include/rkfd_model.h.

Joint kinds: fixed, revolute, prismatic, float, spherical (three coordinates: the rotational half of the float joint's
convention) and the breakable float joint.  A breakable float joint is kinematically a float joint - the link sits where
its six coordinates put it.  Intact, it is rigid with its parent: its six accelerations are zero, there is no joint
equation, and what the recursion finds on its six coordinates is the wrench the joint transmits.  Broken, it is a float
joint.  Actuators of 1-DoF joints: actuator_torque() [UNVERIFIED-DEP: RoKi's motors are not here; DEVIATIONS.md item 5].
"""
import numpy as np

G = 9.80665
FIXED, REVOL, PRISM, FLOAT, SPHER, BRFLOAT = 0, 1, 2, 3, 4, 5
MOTOR_NONE, MOTOR_TRQ, MOTOR_DC = 0, 1, 2


def rot_aa(aa):
    th = np.linalg.norm(aa)
    if th < 1e-12:
        return np.eye(3)
    k = aa / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def model_arrays(m, mass=None, com=None, inertia=None):
    """numpy views of the ctypes RkfdModel.  mass [nlink] / com [nlink*3] / inertia [nlink*9]: the values of ONE instance
    of a batch that carries a parameter table, in place of the model's"""
    nl = m.nlink
    d = dict(nlink=nl, ndof=m.ndof,
             parent=m.arr("parent", nl), jtype=m.arr("jtype", nl), dofoff=m.arr("dofoff", nl),
             org=m.arr("org", 12 * nl).reshape(nl, 12), mass=m.arr("mass", nl),
             com=m.arr("com", 3 * nl).reshape(nl, 3), inertia=m.arr("inertia", 9 * nl).reshape(nl, 3, 3),
             mtype=m.arr("mtype", nl), mot_gear=m.arr("mot_gear", nl), mot_inertia=m.arr("mot_inertia", nl),
             mot_k=m.arr("mot_k", nl), mot_admit=m.arr("mot_admit", nl),
             mot_vmax=m.arr("mot_vmax", nl), mot_vmin=m.arr("mot_vmin", nl),
             stiff=m.arr("stiff", nl), visc=m.arr("visc", nl), coulomb=m.arr("coulomb", nl), sfric=m.arr("sfric", nl),
             brk_f=m.arr("brk_f", nl), brk_t=m.arr("brk_t", nl))
    if mass is not None:
        d["mass"] = np.asarray(mass, dtype=float).reshape(nl)
    if com is not None:
        d["com"] = np.asarray(com, dtype=float).reshape(nl, 3)
    if inertia is not None:
        d["inertia"] = np.asarray(inertia, dtype=float).reshape(nl, 3, 3)
    return d


def fk(md, q):
    """world frames (R, p) of every link and the world orientation of each joint-origin frame"""
    nl = md["nlink"]
    R = np.zeros((nl, 3, 3)); p = np.zeros((nl, 3)); Row = np.zeros((nl, 3, 3))
    for i in range(nl):
        Ro = md["org"][i, :9].reshape(3, 3); po = md["org"][i, 9:]
        par = md["parent"][i]
        Rp, pp = (np.eye(3), np.zeros(3)) if par < 0 else (R[par], p[par])
        off = md["dofoff"][i]; jt = md["jtype"][i]
        Row[i] = Rp @ Ro
        if jt == REVOL:
            c, s = np.cos(q[off]), np.sin(q[off])
            R[i] = Rp @ Ro @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]); p[i] = pp + Rp @ po
        elif jt == PRISM:
            R[i] = Rp @ Ro; p[i] = pp + Rp @ (po + Ro[:, 2] * q[off])
        elif jt in (FLOAT, BRFLOAT):
            R[i] = Rp @ Ro @ rot_aa(q[off + 3:off + 6]); p[i] = pp + Rp @ (po + Ro @ q[off:off + 3])
        elif jt == SPHER:
            R[i] = Rp @ Ro @ rot_aa(q[off:off + 3]); p[i] = pp + Rp @ po
        else:
            R[i] = Rp @ Ro; p[i] = pp + Rp @ po
    return R, p, Row


def rnea(md, q, qd, qdd, fext=None, gravity=G, broken=None, wrench=False):
    """generalized forces that produce qdd at (q, qd).  fext: dict link -> list of (point_w, force_w).
    Float joints return (force, moment about the link origin) projected on the joint-origin axes, spherical joints the
    moment on those axes.

    broken [nlink] (needed when the model has breakable float joints): an INTACT breakable joint is rigid with its parent -
    whatever qdd holds on its six coordinates is taken as zero, and its six entries of the result are zero (there is no
    joint equation); a broken one is a float joint.  wrench=True: returns (tau, W) with W[i] = (force, moment about the
    link origin) that joint i transmits to its link, world frame - for an intact breakable joint the constraint wrench
    its thresholds are compared with (include/rkfd_model.h: norm of the force, norm of the torque about the link origin)."""
    nl = md["nlink"]
    R, p, Row = fk(md, q)
    q = np.asarray(q, dtype=float); qd = np.asarray(qd, dtype=float); qdd = np.array(qdd, dtype=float)
    intact = np.zeros(nl, dtype=bool)
    for i in range(nl):
        if md["jtype"][i] == BRFLOAT:
            assert broken is not None, "a model with breakable float joints needs the broken flags"
            intact[i] = not broken[i]
            if intact[i]:
                qdd[md["dofoff"][i]:md["dofoff"][i] + 6] = 0.0
    w = np.zeros((nl, 3)); al = np.zeros((nl, 3)); a = np.zeros((nl, 3))
    for i in range(nl):
        par = md["parent"][i]; off = md["dofoff"][i]; jt = md["jtype"][i]
        if par < 0:
            wp = np.zeros(3); alp = np.zeros(3); ap = np.zeros(3); pp = np.zeros(3)
        else:
            wp, alp, ap, pp = w[par], al[par], a[par], p[par]
        r = p[i] - pp
        a[i] = ap + np.cross(alp, r) + np.cross(wp, np.cross(wp, r))
        w[i] = wp; al[i] = alp
        z = R[i][:, 2]
        if jt == REVOL:
            w[i] = wp + z * qd[off]
            al[i] = alp + z * qdd[off] + np.cross(wp, z * qd[off])
        elif jt == PRISM:
            a[i] += 2 * np.cross(wp, z * qd[off]) + z * qdd[off]
        elif jt in (FLOAT, BRFLOAT):
            vj = Row[i] @ qd[off:off + 3]; wj = Row[i] @ qd[off + 3:off + 6]
            w[i] = wp + wj
            al[i] = alp + Row[i] @ qdd[off + 3:off + 6] + np.cross(wp, wj)
            a[i] += 2 * np.cross(wp, vj) + Row[i] @ qdd[off:off + 3]
        elif jt == SPHER:
            wj = Row[i] @ qd[off:off + 3]
            w[i] = wp + wj
            al[i] = alp + Row[i] @ qdd[off:off + 3] + np.cross(wp, wj)
    f = np.zeros((nl, 3)); n = np.zeros((nl, 3))   # force / moment about the link origin, world frame
    for i in range(nl):
        cw = R[i] @ md["com"][i]
        Iw = R[i] @ md["inertia"][i] @ R[i].T
        ac = a[i] + np.cross(al[i], cw) + np.cross(w[i], np.cross(w[i], cw))
        F = md["mass"][i] * (ac - np.array([0, 0, -gravity]))
        N = Iw @ al[i] + np.cross(w[i], Iw @ w[i])
        f[i] = F; n[i] = N + np.cross(cw, F)
        if fext and i in fext:
            for (x, fw) in fext[i]:
                f[i] -= fw; n[i] -= np.cross(np.asarray(x) - p[i], fw)
    tau = np.zeros(md["ndof"])
    for i in range(nl - 1, -1, -1):
        par = md["parent"][i]; off = md["dofoff"][i]; jt = md["jtype"][i]
        z = R[i][:, 2]
        if jt == REVOL:
            tau[off] = z @ n[i]
        elif jt == PRISM:
            tau[off] = z @ f[i]
        elif jt == FLOAT or (jt == BRFLOAT and not intact[i]):
            tau[off:off + 3] = Row[i].T @ f[i]; tau[off + 3:off + 6] = Row[i].T @ n[i]
        elif jt == SPHER:
            tau[off:off + 3] = Row[i].T @ n[i]
        if par >= 0:
            f[par] += f[i]; n[par] += n[i] + np.cross(p[i] - p[par], f[i])
    if wrench:
        return tau, [(f[i].copy(), n[i].copy()) for i in range(nl)]
    return tau


def actuator_torque(md, qd, qdd, inp, rotor=True):
    """what the actuators put on the joint coordinates, [ndof]; inp [nlink] are the motor inputs (rkJointMotorSetInput).
    Torque motor: the input clamped to [min, max].  DC motor: admit gear k clamp(V) - admit (gear k)^2 qd (input torque minus
    the back-EMF 'resistance' torque), and the rotor and gear inertia reflected through the gear, gear^2 (J_rotor + J_gear)
    (mot_inertia holds the sum), resists the joint's acceleration: - gear^2 J qdd (rotor=False leaves that term out).
    [UNVERIFIED-DEP] this is DEVIATIONS.md item 5's statement of RoKi's motor, which is not available to check against."""
    tau = np.zeros(md["ndof"])
    for i in range(md["nlink"]):
        if md["jtype"][i] not in (REVOL, PRISM):
            continue
        off = md["dofoff"][i]
        if md["mtype"][i] == MOTOR_TRQ:
            tau[off] = min(max(inp[i], md["mot_vmin"][i]), md["mot_vmax"][i])
        elif md["mtype"][i] == MOTOR_DC:
            gk = md["mot_gear"][i] * md["mot_k"][i]
            v = min(max(inp[i], md["mot_vmin"][i]), md["mot_vmax"][i])
            tau[off] = md["mot_admit"][i] * gk * v - md["mot_admit"][i] * gk * gk * qd[off] \
                - (md["mot_gear"][i] ** 2 * md["mot_inertia"][i] * qdd[off] if rotor else 0.0)
    return tau


def mass_matrix(md, q):
    n = md["ndof"]
    z = np.zeros(n)
    h0 = rnea(md, q, z, z, gravity=0.0)
    M = np.zeros((n, n))
    for k in range(n):
        e = np.zeros(n); e[k] = 1
        M[:, k] = rnea(md, q, z, e, gravity=0.0) - h0
    return M


def point_jacobian_T(md, q, link, x, dirs):
    """columns J' d for world directions d of a force applied at world point x on `link`
    (generalized force of the external force), via inverse dynamics"""
    n = md["ndof"]
    z = np.zeros(n)
    h0 = rnea(md, q, z, z, gravity=0.0)
    cols = []
    for d in dirs:
        h = rnea(md, q, z, z, fext={link: [(x, np.asarray(d, dtype=float))]}, gravity=0.0)
        cols.append(h0 - h)
    return np.array(cols).T
