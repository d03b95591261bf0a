"""Worlds at the tree-size limits of the one-wavefront mapping (tests/test_emu_tree_limits.py, tools/tree_limits_report.py): 64 device links (one per lane), 64 joint coordinates, six pointer-jumping rounds (more than 32
levels), more model links than lanes after fixed-link merging, 63 pseudo-links of spherical joints, the 32 / 32 edge of two
instances per wavefront - and the worlds just beyond, which the builder refuses.

A world is an EXPLICIT topology (parent list, joint list, optional boxes on named links) written as ZTK text, with seeded
frames, masses and inertias drawn as tests/randtree.py draws them (frame offsets within +-0.05 m, so that a chain of 64 links
stays within a few metres).  States: dis uniform +-0.3, vel uniform +-1, seed 5.

Bound of the step state against the oracle: 1e-8 max( 1, |ref|_inf ), the bound of tests/test_random_trees.py for random trees
on the GPU.  It is a condition on the INPUTS: for every case the plain oracle build and its build with fused multiply-adds (two
roundings of one algorithm) must agree below CONTROL_TOL = 1e-9, or the world itself is too sensitive to carry the bound."""
import functools
import os
import subprocess

import numpy as np

from randtree import _rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TOL = 1e-8
CONTROL_TOL = 1e-9
NSTEPS = 2
SEED = 5

_MOTORS = ("[roki::motor]\nname : dcm\ntype: dc\nmotorconstant : 2.53e-2\nadmittance : 0.045872\nmaxvoltage : 24.0\nminvoltage : -24.0\n"
           "gearratio : 100.0\nrotorinertia : 2.97e-7\ngearinertia : 3.0e-7\n\n"
           "[roki::motor]\nname : trqm\ntype: trq\nmax : 5.0\nmin : -5.0\n\n")


def tree_ztk(name, parents, joints, seed, boxes=None, motors=False):
    """ZTK text of the tree parents[i] (None / -1 for the root) with joint kinds joints[i] in fixed / revolute / prismatic /
    float / spherical; boxes: {link index: centre of a 6 x 5 x 4 cm box in the link's frame}; motors: DC and torque motors (and
    joint friction under the DC motors) on revolute and prismatic joints, as tests/randtree.py writes them"""
    rng = np.random.default_rng(seed)
    boxes = boxes or {}
    s = f"[roki::chain]\nname : {name}\n\n"
    if motors:
        s += _MOTORS
    for i, c in sorted(boxes.items()):
        s += f"[zeo::shape]\ntype : box\nname : sh{i}\ncenter : {c[0]:.12f}, {c[1]:.12f}, {c[2]:.12f}\ndepth : 0.06\nwidth : 0.05\nheight : 0.04\n\n"
    for i, (par, jt) in enumerate(zip(parents, joints)):
        R = _rot(rng); p = rng.uniform(-0.05, 0.05, 3)
        if i == 0:
            p = np.array([0.0, 0.0, 0.5]); R = np.eye(3)
        A = rng.normal(size=(3, 3)); I = (A @ A.T) * 1e-3 + np.eye(3) * 2e-3
        com = rng.uniform(-0.03, 0.03, 3)
        mk = rng.choice(["dcm", "trqm", ""])
        fr = (rng.uniform(0, 0.5), rng.uniform(0, 0.2), rng.uniform(0.1, 1.0), rng.uniform(1.0, 1.5))
        s += f"[roki::link]\nname : l{i}\njointtype : {jt}\nmass : {rng.uniform(0.3, 2.0):.6f}\nstuff : body\n"
        s += f"COM : {{ {com[0]:.6f}, {com[1]:.6f}, {com[2]:.6f} }}\n"
        s += "inertia : {\n" + "".join(f" {I[r,0]:.8f}, {I[r,1]:.8f}, {I[r,2]:.8f}\n" for r in range(3)) + "}\n"
        s += "frame : {\n" + "".join(f" {R[r,0]:.10f}, {R[r,1]:.10f}, {R[r,2]:.10f}, {p[r]:.6f}\n" for r in range(3)) + "}\n"
        if motors and jt in ("revolute", "prismatic") and mk:
            s += f"motor : {mk}\n"
            if mk == "dcm":
                s += f"stiffness: {fr[0]:.4f}\nviscosity: {fr[1]:.4f}\ncoulomb: {fr[2]:.4f}\nstaticfriction: {fr[3]:.4f}\n"
        if par is not None and par >= 0:
            s += f"parent : l{par}\n"
        if i in boxes:
            s += f"shape : sh{i}\n"
        s += "\n"
    return s


# ---- topologies: (parents, joints) ------------------------------------------------------------------------------------------------
def chain(n, root="revolute", joint="revolute"):
    return [None] + list(range(n - 1)), [root] + [joint] * (n - 1)


def star(n, root):
    return [None] + [0] * (n - 1), [root] + ["revolute"] * (n - 1)


def comb(nspine):
    """a spine with one tooth on every spine link: a parent that gathers two children on every level"""
    par, jt = [], []
    for k in range(nspine):
        par.append(None if k == 0 else 2 * (k - 1)); jt.append("revolute")      # spine link 2k
        par.append(2 * k); jt.append("revolute")                                 # its tooth 2k + 1
    return par, jt


def binary(n):
    return [None] + [(i - 1) // 2 for i in range(1, n)], ["revolute"] * n


def chain_fixed(nmove, every, root="revolute"):
    """a chain of nmove moving links with a fixed link IN the chain after every `every`-th of them: the device merges each fixed
    link into the link above it, and the links below hang on the merged body"""
    par, jt = [], []
    for k in range(nmove):
        par.append(len(par) - 1 if par else None); jt.append(root if k == 0 else "revolute")
        if (k + 1) % every == 0:
            par.append(len(par) - 1); jt.append("fixed")
    return par, jt


def fork(nbranch, root="float"):
    """two chains of nbranch links below one root"""
    par, jt = [None], [root]
    for _ in range(2):
        for k in range(nbranch):
            par.append(0 if k == 0 else len(par) - 1); jt.append("revolute")
    return par, jt


def spher_chain(nspher, root="fixed"):
    return [None] + list(range(nspher)), [root] + ["spherical"] * nspher


def spher_star(nspher, root="float"):
    return [None] + [0] * nspher, [root] + ["spherical"] * nspher


class Case:
    def __init__(self, name, topo, dims, what, motors=False, boxes=(), ipw2=False):
        self.name, self.topo, self.dims, self.what = name, topo, dims, what      # dims: (model links, device links, coordinates)
        self.motors, self.boxes, self.ipw2 = motors, tuple(boxes), ipw2
        self.seed = 7000 + sum(ord(c) for c in name)

    def __repr__(self):
        return self.name


# every accepted case of free motion: name -> Case
FREE = [
    Case("chain33", chain(33), (33, 33, 33), "the first world with six pointer-jumping rounds"),
    Case("chain34", chain(34), (34, 34, 34), "six rounds, an even depth"),
    Case("chain64", chain(64), (64, 64, 64), "every lane a link, depth 64"),
    Case("chain59f", chain(59, root="float"), (59, 59, 64), "64 coordinates with a float joint"),
    Case("star59f", star(59, "float"), (59, 59, 64), "one level of 58 links: sweep schedule and Ia pool at their widest"),
    Case("star64", star(64, "revolute"), (64, 64, 64), "one level of 63 links"),
    Case("comb32", comb(32), (64, 64, 64), "a gathering parent at every level"),
    Case("binary64", binary(64), (64, 64, 64), "a complete binary tree"),
    Case("chain64_fixed32", chain_fixed(64, 2), (96, 64, 64), "more model links than lanes", motors=True),
    Case("spher22", spher_chain(21), (22, 64, 63), "63 pseudo-links in a chain"),
    Case("spherstar", spher_star(19), (20, 58, 63), "57 pseudo-links on one level, float root"),
    Case("chain32", chain(32), (32, 32, 32), "the two-instance edge: 32 links, 32 coordinates", ipw2=True),
    Case("chain27f", chain(27, root="float"), (27, 27, 32), "the two-instance edge with a float root: 32 coordinates", ipw2=True),
]
# contact cases: boxes on deep links, seated on the floor (seated_world)
CONTACT = [
    Case("chain59f_boxes", chain(59, root="float"), (59, 59, 64), "probe walks of depth 59", boxes=(58, 45, 30, 10)),
    Case("fork29x2_boxes", fork(29), (59, 59, 64), "contacts on two deep branches", boxes=(29, 58)),
]
# refused at build: (Case, instances per wavefront, the builder's message)
MSG_DOF = r"ndof %d exceeds the per-wave limit 64"
MSG_LINK = r"nlink %d \(after merging fixed links\) exceeds the per-wave limit 64"
MSG_IPW2 = r"two instances per wavefront need a world of at most 32 links, 32 joint coordinates"
REFUSED = [
    (Case("chain65", chain(65), (65, 65, 65), ""), 1, MSG_DOF % 65),
    (Case("chain60f", chain(60, root="float"), (60, 60, 65), ""), 1, MSG_DOF % 65),
    (Case("spher23", spher_chain(22), (23, 67, 66), ""), 1, MSG_DOF % 66),
    (Case("chain100_fixed33", chain_fixed(67, 2), (100, 67, 67), ""), 1, MSG_DOF % 67),
    (Case("chain64_fixedroot", chain(65, root="fixed"), (65, 65, 64), ""), 1, MSG_LINK % 65),
    (Case("chain33", chain(33), (33, 33, 33), ""), 2, MSG_IPW2),
]
BY_NAME = {c.name: c for c in FREE + CONTACT}


def write(case, tmp_path, boxes=None, tag=""):
    f = tmp_path / f"{case.name}{tag}.ztk"
    par, jt = case.topo
    f.write_text(tree_ztk(case.name, par, jt, case.seed, boxes=boxes, motors=case.motors))
    return str(f)


def world(R, case, tmp_path):
    """the world of a free-motion case; its model dimensions are those the case names"""
    w = R.World(solver=R.SOLVER_MLCP)
    w.reg_file(write(case, tmp_path))
    m = w.model.contents
    assert (m.nlink, m.ndof) == (case.dims[0], case.dims[2]), (case.name, m.nlink, m.ndof)
    return w


def states(w, B, seed=SEED, vel_scale=1.0):
    m = w.model.contents
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.3, 0.3, (B, m.ndof)), rng.uniform(-1.0, 1.0, (B, m.ndof)) * vel_scale


def seated_world(R, case, tmp_path, B, solver=None):
    """a contact case: (world, chain, dis, vel).  The joint coordinates are ONE seeded draw shared by the instances (root position
    in x / y and all velocities differ); the centre of every box is placed in its link's frame so that, at those coordinates, the
    lowest vertex of EVERY box lies scenarios.SEAT_DEPTH inside the floor: every boxed link is in rigid contact at once.
    Velocities are +-1e-3: a vertex moves ~1e-6 m in a step, so the seated contacts last over the compared steps."""
    S = R.scenarios

    def reg(boxes, tag):
        w = R.World(solver=R.SOLVER_MLCP if solver is None else solver)
        w.contact_info(os.path.join(S.MODELS, "contactinfo.ztk"))
        h = w.reg_file(write(case, tmp_path, boxes=boxes, tag=tag))
        w.pair_chain_unreg(h)          # (the tree's own pairs go, as in tests/test_random_trees.py: this is about the floor)
        w.reg_file(os.path.join(S.MODELS, "floor.ztk"))
        return w, h
    w0, h = reg({i: np.zeros(3) for i in case.boxes}, "_pass1")
    m = w0.model.contents
    dis, vel = states(w0, B, vel_scale=1e-3)
    dis[:, 2:] = dis[0, 2:]
    Rl, pl = S.link_frames(m, dis[:1])
    half = np.array([0.03, 0.025, 0.02])
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * half
    low = {i: (pl[0, i, 2] + (corners @ Rl[0, i].T)[:, 2]).min() for i in case.boxes}
    z0 = min(low.values())
    # shift every box along the world's z, expressed in its link's frame, down to the level of the lowest one
    boxes = {i: Rl[0, i].T @ np.array([0.0, 0.0, z0 - low[i]]) for i in case.boxes}
    w, h = reg(boxes, "")
    m = w.model.contents
    dis[:, 2] -= S.lowest_vertex_z(m, dis[0], h) + S.SEAT_DEPTH
    return w, h, dis, vel


def rigid_links_in_contact(m, act, chain):
    """model links of `chain` in a pair with an active contact vertex whose contact info is RIGID (act: [ncand] of one instance)"""
    pair = m.arr("cand_pair", m.ncand)
    pshape = m.arr("pair_shape", 2 * m.npair).reshape(-1, 2)
    rigid = m.arr("ci_type", m.nci)[m.arr("pair_ci", m.npair)] == 0      # CONTACT_RIGID
    slink, ch = m.arr("shape_link", m.nshape), m.arr("chain", m.nlink)
    out = set()
    for c in np.flatnonzero((np.asarray(act) != 0) & rigid[pair]):
        for s in (0, 1):
            l = slink[pshape[pair[c], s]]
            if ch[l] == chain:
                out.add(int(l))
    return out


def relerr(x, y):
    return float(np.abs(x - y).max() / max(1.0, np.abs(y).max()))


def oracle_run(oracle_cls, w, dis, vel, nsteps=NSTEPS, libpath=None, motor_in=None):
    """per instance: ((dis, vel, acc), (act, typ, ref, f) or None) after update_init and nsteps steps"""
    out = []
    m = w.model.contents
    for i in range(dis.shape[0]):
        o = oracle_cls(w.model, libpath) if libpath else oracle_cls(w.model)
        o.set_state(dis[i], vel[i])
        if motor_in is not None:
            o.set_motor_input(motor_in[i])
        o.update_init(); o.update_n(nsteps)
        out.append((o.get_state(), o.get_contact() if m.ncand else None))
        o.close()
    return out


def deviation(state, ref):
    """worst relerr over dis, vel, acc and the instances; state: (dis, vel, acc) [B, ndof], ref: oracle_run's list"""
    return max(relerr(x[i], y) for i, (st, _) in enumerate(ref) for x, y in zip(state, st))


@functools.lru_cache(maxsize=None)
def fma_oracle_lib():
    """the rounding control: the oracle source built with fused multiply-adds (make -C oracle fma), built once per process"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "fma"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "oracle", "_build", "librkfd_oracle_fma.so")


def control(oracle_cls, w, dis, vel, ref, motor_in=None):
    """the oracle built with fused multiply-adds against the plain build `ref` (oracle_run): the sensitivity of the world itself"""
    fma = oracle_run(oracle_cls, w, dis, vel, libpath=fma_oracle_lib(), motor_in=motor_in)
    return max(relerr(x, y) for (sf, _), (sr, _) in zip(fma, ref) for x, y in zip(sf, sr))
