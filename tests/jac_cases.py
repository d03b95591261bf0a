"""Helpers of the task-space Jacobian tests (rkfdBatchUpdateJacobians; tests/test_emu_jac.py, tests/test_gpu_jac.py,
tools/jac_parity.py): the worlds and their sites, the reference, the textbook cross-check and the bound.

Reference - no code under test in it: for a state dis and every coordinate c, the oracle's link velocities and the numpy comvel of
tests/links_cases.reference at ( dis, vel = e_c ) are column c:
  J[s][:, c] = ( R_l ( v_l + w_l x point ), R_l w_l ),  Jcom[ch][:, c] = comvel[ch]
Bound: links_cases.TOL = 1e-12 max( 1, |value|_inf ), the bound the read-out is asserted at for the very quantities a column
consists of (a column is a read-out at a unit rate vector: the same depth x a few ulp on both sides).

The textbook Jacobian (axis x lever arm on the oracle's composed world frames) is a guard on conventions, not the acceptance bound:
it equals the recursion only for exactly orthonormal frames.  GEOM_RECORDED holds, per world, how far it sits from the oracle's
unit-rate columns (a reference-only figure, the orthonormality defect of the files' frames; profiles/r10_jac_parity.txt,
tools/jac_parity.py); the device is asserted against the textbook Jacobian to ten times that figure plus TOL."""
import ctypes as C
import os
import subprocess

import numpy as np

from emu import ROOT, HERE
import links_cases as lc
import instance_params as ip
import tree_limits as tl

SITES, COM, ALL = 1, 2, 3
TOL = lc.TOL
KEYS = ("J", "Jcom")
WORLDS = ["arm_revroot", "arm_spher", "humanoid30", "humanoid30_shell", "wall_cantilever", "config5"]
LIMIT_TREES = ["chain59f", "chain64_fixed32", "spherstar"]      # 64 coordinates with a float root; 96 model links; 63 coordinates of spherical joints
_emu = None

# |textbook - oracle unit-rate columns|_inf / max( 1, |oracle|_inf ) over J and Jcom, per world at the states of cases():
# profiles/r10_jac_parity.txt (tools/jac_parity.py writes both)
GEOM_RECORDED = {
    "arm_revroot": 1.1e-16, "arm_spher": 4.4e-16, "humanoid30": 5.6e-16, "humanoid30_shell": 8.9e-16, "wall_cantilever": 3.3e-16, "config5": 8.9e-16,
    # frames written with ten digits (tests/randtree.py, tests/tree_limits.py): the defect the recursion's exact map does not have
    "rand300": 2.0e-10, "rand301": 1.5e-10, "rand302": 2.0e-10, "rand303": 5.2e-10, "rand304": 1.6e-10, "rand305": 3.2e-10, "rand306": 1.6e-10,
    "rand307": 2.4e-10, "rand308": 4.1e-10, "rand309": 4.7e-10, "chain59f": 5.7e-10, "chain64_fixed32": 1.1e-09, "spherstar": 1.2e-10,
}


def emu_lib():
    global _emu
    if _emu is None:
        path = os.path.join(HERE, "librkfd_emu_jac.so")
        if not os.path.exists(path):
            subprocess.run(["make", "-C", ROOT, "emu"], check=True, stdout=subprocess.DEVNULL)
        L = C.CDLL(path)
        L.rkfd_emu_jac.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
        _emu = L
    return _emu


def emu_jac(world, dis, links, points=None, flags=ALL, par=None):
    """the Jacobians' device code under the lane emulator: dict as Batch.get_jacobians(); par = (mass [B, nl], com [B, 3 nl])"""
    m = world.model.contents
    B = dis.shape[0]
    dis = np.ascontiguousarray(dis, dtype=np.float64)
    links = np.ascontiguousarray(links, dtype=np.int32)
    pts = None if points is None else np.ascontiguousarray(points, dtype=np.float64)
    shapes = {"J": (B, links.size, 6, m.ndof), "Jcom": (B, m.nchain, 3, m.ndof)}
    need = {"J": SITES, "Jcom": COM}
    out = {k: np.full(shapes[k], np.nan) for k in KEYS if flags & need[k]}
    pm = pc = None
    if par is not None:
        pm = np.ascontiguousarray(par[0], dtype=np.float64); pc = np.ascontiguousarray(par[1], dtype=np.float64)
    p = lambda a: None if a is None else a.ctypes.data
    r = emu_lib().rkfd_emu_jac(C.cast(world.model, C.c_void_p), B, p(dis), flags, links.size, p(links), p(pts), p(pm), p(pc), *[p(out.get(k)) for k in KEYS])
    assert r == 0, r
    return out


def unit_rate_readout(R, oracle_cls, world, dis_i, broken_i=None, mass_i=None, com_i=None):
    """links_cases.reference of ONE state at the ndof unit rate vectors: dict with R, p, v [ndof, nl, ..], comvel [ndof, nc, 3]"""
    nd = world.model.contents.ndof
    rep = lambda a: None if a is None else np.repeat(np.asarray(a)[None], nd, axis=0)
    return lc.reference(R, oracle_cls, world, rep(dis_i), np.eye(nd), rep(broken_i), rep(mass_i), rep(com_i))


def from_unit_rates(u, links, points):
    """(J [nsite, 6, ndof], Jcom [nc, 3, ndof]) of one state from unit_rate_readout's dict"""
    nd = u["v"].shape[0]
    pts = np.zeros((len(links), 3)) if points is None else np.asarray(points, dtype=np.float64)
    J = np.zeros((len(links), 6, nd))
    for s, l in enumerate(links):
        Rl, v, w = u["R"][:, l], u["v"][:, l, :3], u["v"][:, l, 3:]
        J[s, :3] = np.einsum("cij,cj->ic", Rl, v + np.cross(w, pts[s]))
        J[s, 3:] = np.einsum("cij,cj->ic", Rl, w)
    return J, np.transpose(u["comvel"], (1, 2, 0)).copy()


def reference(R, oracle_cls, world, dis, links, points=None, broken=None, mass=None, com=None, with_frames=False):
    """the reference of the states dis [B, ndof]: dict as Batch.get_jacobians(); with_frames: also the oracle's R, p [B, nl, ..]"""
    m = world.model.contents
    B = dis.shape[0]
    out = {"J": np.zeros((B, len(links), 6, m.ndof)), "Jcom": np.zeros((B, m.nchain, 3, m.ndof))}
    fr = {"R": np.zeros((B, m.nlink, 3, 3)), "p": np.zeros((B, m.nlink, 3))}
    for i in range(B):
        pick = lambda a: None if a is None else a[i]
        u = unit_rate_readout(R, oracle_cls, world, dis[i], pick(broken), pick(mass), pick(com))
        out["J"][i], out["Jcom"][i] = from_unit_rates(u, links, points)
        fr["R"][i], fr["p"][i] = u["R"][0], u["p"][0]
    return (out, fr) if with_frames else out


def check(got, ref, what, keys=KEYS):
    return lc.check(got, ref, what, keys=[k for k in keys if k in got])


# ---- the model's tree, for the zero pattern and the textbook Jacobian ---------------------------------------------------------------
def coordinate_owner(m):
    jt, off = m.arr("jtype", m.nlink), m.arr("dofoff", m.nlink)
    dof = {0: 0, 1: 1, 2: 1, 3: 6, 4: 3, 5: 6}
    own = np.full(m.ndof, -1)
    for i in range(m.nlink):
        own[off[i]:off[i] + dof[int(jt[i])]] = i
    return own


def moves(m):
    """[nlink, ndof] bool: coordinate c belongs to link l's joint or to an ancestor's"""
    par, own = m.arr("parent", m.nlink), coordinate_owner(m)
    out = np.zeros((m.nlink, m.ndof), dtype=bool)
    for l in range(m.nlink):
        k = l
        while k >= 0:
            out[l] |= own == k
            k = par[k]
    return out


def chain_moves(m):
    """[nchain, ndof] bool: coordinate c belongs to a link of the chain"""
    ch, own = m.arr("chain", m.nlink), coordinate_owner(m)
    return np.stack([ch[own] == c for c in range(m.nchain)]) if m.ndof else np.zeros((m.nchain, 0), dtype=bool)


def textbook(world, Rw, pw, links, points=None, mass=None, com=None):
    """the geometric Jacobian of ONE state on composed world frames Rw [nl, 3, 3], pw [nl, 3] (the oracle's): axis x ( p_site -
    p_joint ) for rotations about the link origin, the axis itself for translations; the axes of float and spherical rates are
    those of the joint-origin frame, R_parent org_R"""
    m = world.model.contents
    nl, nd = m.nlink, m.ndof
    par, jt, off = m.arr("parent", nl), m.arr("jtype", nl), m.arr("dofoff", nl)
    org = m.arr("org", 12 * nl).reshape(nl, 12)
    mv = moves(m)
    pts = np.zeros((len(links), 3)) if points is None else np.asarray(points, dtype=np.float64)

    def columns(l, pt):
        J = np.zeros((6, nd))
        ps = pw[l] + Rw[l] @ pt
        for k in range(nl):
            if jt[k] == 0 or not mv[l, off[k]]:
                continue
            Ro = org[k, :9].reshape(3, 3)
            Rjo = Ro if par[k] < 0 else Rw[par[k]] @ Ro
            arm = ps - pw[k]
            if jt[k] == 1:
                J[:3, off[k]] = np.cross(Rw[k][:, 2], arm); J[3:, off[k]] = Rw[k][:, 2]
            elif jt[k] == 2:
                J[:3, off[k]] = Rw[k][:, 2]
            else:
                rot0 = off[k] + (3 if jt[k] in (3, 5) else 0)
                for a in range(3):
                    if jt[k] in (3, 5):
                        J[:3, off[k] + a] = Rjo[:, a]
                    J[:3, rot0 + a] = np.cross(Rjo[:, a], arm); J[3:, rot0 + a] = Rjo[:, a]
        return J
    J = np.stack([columns(l, pts[s]) for s, l in enumerate(links)]) if len(links) else np.zeros((0, 6, nd))
    ms = m.arr("mass", nl) if mass is None else np.asarray(mass)
    cm = (m.arr("com", 3 * nl) if com is None else np.asarray(com)).reshape(nl, 3)
    chain = m.arr("chain", nl)
    Jc = np.zeros((m.nchain, 3, nd))
    for c in range(m.nchain):
        sel = np.flatnonzero(chain == c)
        M = ms[sel].sum()
        if M > 0:
            Jc[c] = sum(ms[i] * columns(i, cm[i])[:3] for i in sel if ms[i] != 0) / M
    return {"J": J, "Jcom": Jc}


def textbook_batch(world, fr, links, points=None):
    t = [textbook(world, fr["R"][i], fr["p"][i], links, points) for i in range(fr["R"].shape[0])]
    return {k: np.stack([x[k] for x in t]) for k in KEYS}


def worst(dev):
    return max(dev.values()) if dev else 0.0


# ---- the worlds and their sites -------------------------------------------------------------------------------------------------
def sites_for(world, seed, n_random=3):
    """sites of a world: the last link of every chain (at most six chains), every merged link (at most four) and seeded random
    links, each with a seeded non-zero point within +-0.2 m; the first site sits at its link's origin"""
    m = world.model.contents
    rng = np.random.default_rng(0x1AC0 + seed)
    chain = m.arr("chain", m.nlink)
    links = [int(np.flatnonzero(chain == c)[-1]) for c in range(min(m.nchain, 6))]
    links += ip.merged_links(world)[-4:]
    links += [int(x) for x in rng.integers(0, m.nlink, n_random)]
    pts = rng.uniform(-0.2, 0.2, (len(links), 3))
    pts[0] = 0.0
    return np.array(links, dtype=np.int32), pts


def cases(R):
    """name -> dict(world, dis, broken or None, links, points): the worlds of WORLDS at the seeded states of links_cases.cases"""
    lcs = lc.cases(R)
    w = R.World(solver=R.SOLVER_MLCP); w.reg_file(os.path.join(R.scenarios.MODELS, "arm_revroot.ztk"))
    d, v = lc.states(w, 3, 0x11AC + 9)
    lcs["arm_revroot"] = dict(world=w, dis=d, vel=v, broken=None)
    out = {}
    for k, name in enumerate(WORLDS):
        c = lcs[name]
        links, pts = sites_for(c["world"], k)
        out[name] = dict(world=c["world"], dis=c["dis"], vel=c["vel"], broken=c["broken"], links=links, points=pts)
    m = out["humanoid30_shell"]["world"].model.contents
    assert set(ip.merged_links(out["humanoid30_shell"]["world"])) & set(out["humanoid30_shell"]["links"].tolist())      # sites ON merged links
    m = out["config5"]["world"].model.contents
    assert len(set(m.arr("chain", m.nlink)[out["config5"]["links"]].tolist())) >= 5          # a site on the humanoid and on the boxes
    return out


def limit_tree_cases(R, tmp_path):
    out = {}
    for k, name in enumerate(LIMIT_TREES):
        w = tl.world(R, tl.BY_NAME[name], tmp_path)
        dis, vel = tl.states(w, 2)
        links, pts = sites_for(w, 40 + k)
        out[name] = dict(world=w, dis=dis, vel=vel, broken=None, links=links, points=pts)
    return out


def random_tree_cases(R, tmp_path):
    out = lc.random_tree_cases(R, tmp_path)
    for k, (name, c) in enumerate(out.items()):
        c["links"], c["points"] = sites_for(c["world"], 60 + k)
    return out


def tile(c, B, seed=0x6AC):
    """B states of a case: its seeded ones, then further seeded draws (broken flags repeated)"""
    n = c["dis"].shape[0]
    d2, _ = lc.states(c["world"], B, seed + B)
    d2[:min(n, B)] = c["dis"][:B]
    br = None if c["broken"] is None else np.stack([c["broken"][i % n] for i in range(B)])
    return d2, br
