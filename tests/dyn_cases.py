"""Helpers of the joint-space dynamics tests (rkfdBatchUpdateDynamics; tests/test_emu_dyn.py, tests/test_gpu_dyn.py,
tools/dyn_parity.py): the worlds, two references and the bound.  No device code in here.

Reference A - the model's own recursion.  The oracle's link-frame twists at the ndof unit rate vectors (jac_cases.unit_rate_readout,
v [ndof, nlink, 6]) are the columns ( V_i, W_i ) of every link's Jacobian in its own frame, and the kinetic energy
sum_i 0.5 m_i | v_i + w_i x c_i |^2 + 0.5 w_i' I_i w_i of those twists is 0.5 vel' M vel with
  M_A = sum_i m_i ( V_i + W_i x c_i )' ( V_i + W_i x c_i ) + W_i' I_i W_i
It holds whatever the frames of the file are (frames written with ten digits are orthonormal to 1e-10 only), and gives M alone.

Reference B - independent mechanics (tests/refmath.py, a world-frame Newton-Euler that shares nothing with the oracle or the device):
  M[:, k] = rnea( q, 0, e_k, gravity = 0 ),  h = rnea( q, qd, 0 ),  g = rnea( q, 0, 0 ),  every breakable joint taken as broken
(a breakable float joint is a float joint here, broken or not).  refmath applies a frame as given where the model's recursion
transposes it, so B is asserted on worlds whose frames are orthonormal to rounding only: the model files, and the random and limit
trees with their text passed through eom_cases._orthonormal_frames before it is written.  The raw ten-digit trees are asserted against
A alone.

Bound: links_cases.TOL = 1e-12 max( 1, |ref|_inf ), for both references: an entry of M is a sum over at most 96 links of products of
two read-out columns, each good to depth x a few ulp (links_cases), and h, g are one sweep down and one up the same tree."""
import ctypes as C
import os
import subprocess

import numpy as np

from emu import ROOT, HERE
import eom_cases as ec
import instance_params as ip
import jac_cases as jc
import links_cases as lc
import refmath as rm
import tree_limits as tl
from randtree import random_tree_ztk

MASS, BIAS, GRAVITY, ROTOR = 1, 2, 4, 8
ALL = 7
TOL = lc.TOL
KEYS = ("M", "h", "g")
NEED = {"M": MASS, "h": BIAS, "g": GRAVITY}
WORLDS = jc.WORLDS
LIMIT_TREES = jc.LIMIT_TREES
_emu = None


def emu_lib():
    global _emu
    if _emu is None:
        path = os.path.join(HERE, "librkfd_emu_dyn.so")
        if not os.path.exists(path):
            subprocess.run(["make", "-C", ROOT, "emu"], check=True, stdout=subprocess.DEVNULL)
        L = C.CDLL(path)
        L.rkfd_emu_dyn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6
        _emu = L
    return _emu


def emu_dyn(world, dis, vel, flags=ALL, par=None, waves=None):
    """the dynamics' device code under the lane emulator: ALL three arrays, NaN-prefilled, so that what the flags do not select can be
    seen untouched; par = dict with mass [B, nl], com [B, 3 nl], inertia [B, 9 nl]; waves: a list that receives the instances per
    workgroup the C ABI would launch with"""
    m = world.model.contents
    B = dis.shape[0]
    dis = np.ascontiguousarray(dis, dtype=np.float64); vel = np.ascontiguousarray(vel, dtype=np.float64)
    out = {"M": np.full((B, m.ndof, m.ndof), np.nan), "h": np.full((B, m.ndof), np.nan), "g": np.full((B, m.ndof), np.nan)}
    pp = [None, None, None]
    if par is not None:
        pp = [np.ascontiguousarray(par[k], dtype=np.float64) for k in ("mass", "com", "inertia")]
    p = lambda a: None if a is None else a.ctypes.data
    r = emu_lib().rkfd_emu_dyn(C.cast(world.model, C.c_void_p), B, p(dis), p(vel), flags, *[p(x) for x in pp], *[p(out[k]) for k in KEYS])
    assert r >= 0, r
    if waves is not None:
        waves.append(r)
    return out


def params_of(world, par, i):
    """(mass [nl], com [nl, 3], inertia [nl, 3, 3]) of instance i: the table's, else the model's"""
    m = world.model.contents
    nl = m.nlink
    get = lambda k, w: (m.arr(k, w * nl) if par is None else np.asarray(par[k][i], dtype=np.float64))
    return get("mass", 1).reshape(nl), get("com", 3).reshape(nl, 3), get("inertia", 9).reshape(nl, 3, 3)


def reference_a(R, oracle_cls, world, dis, broken=None, par=None):
    """M_A [B, ndof, ndof] of the states dis"""
    m = world.model.contents
    B, nd = dis.shape[0], m.ndof
    out = np.zeros((B, nd, nd))
    for i in range(B):
        u = jc.unit_rate_readout(R, oracle_cls, world, dis[i], None if broken is None else broken[i])
        ms, cm, In = params_of(world, par, i)
        V, W = u["v"][:, :, :3], u["v"][:, :, 3:]                 # [ndof, nl, 3]
        P = V + np.cross(W, cm[None])
        out[i] = np.einsum("l,alk,clk->ac", ms, P, P) + np.einsum("alj,ljk,clk->ac", W, In, W)
    return {"M": out}


def reference_b(world, dis, vel, par=None):
    """M, h, g [B, ..] of refmath"""
    m = world.model.contents
    B, nd = dis.shape[0], m.ndof
    out = {"M": np.zeros((B, nd, nd)), "h": np.zeros((B, nd)), "g": np.zeros((B, nd))}
    ones, z = np.ones(m.nlink, dtype=int), np.zeros(nd)
    for i in range(B):
        ms, cm, In = params_of(world, par, i)
        md = rm.model_arrays(m, ms, cm, In)
        for k in range(nd):
            e = np.zeros(nd); e[k] = 1.0
            out["M"][i][:, k] = rm.rnea(md, dis[i], z, e, gravity=0.0, broken=ones)
        out["h"][i] = rm.rnea(md, dis[i], vel[i], z, broken=ones)
        out["g"][i] = rm.rnea(md, dis[i], z, z, broken=ones)
    return out


def check(got, ref, what, keys=KEYS):
    return lc.check(got, ref, what, keys=[k for k in keys if k in got and k in ref])


def related(m):
    """[ndof, ndof] bool: the owner of one coordinate is the other's owner or an ancestor of it - where M may be non-zero"""
    own, mv = jc.coordinate_owner(m), jc.moves(m)
    A = mv[own] if m.ndof else np.zeros((0, 0), dtype=bool)          # A[c, a]: a belongs to own(c) or above
    return A | A.T


def check_structure(world, M, what):
    """exact symmetry, the exact zero pattern, positive definite on the coordinates of chains with mass"""
    m = world.model.contents
    assert np.array_equal(M, M.transpose(0, 2, 1)), what
    rel = related(m)
    assert (M[:, ~rel] == 0.0).all(), what
    cmv = jc.chain_moves(m)
    for c in range(m.nchain):
        for a in range(c + 1, m.nchain):
            assert (M[:, cmv[c]][:, :, cmv[a]] == 0.0).all(), (what, c, a)
    ms, chain = m.arr("mass", m.nlink), m.arr("chain", m.nlink)
    for c in range(m.nchain):
        if cmv[c].any() and ms[chain == c].sum() > 0:
            for i in range(M.shape[0]):
                assert np.linalg.eigvalsh(M[i][np.ix_(cmv[c], cmv[c])]).min() > 0, (what, c, i)


def rotor_diagonal(m):
    """[ndof]: gear^2 x mot_inertia on the coordinates of DC-motor joints, 0 elsewhere"""
    nl = m.nlink
    jt, off, mt = m.arr("jtype", nl), m.arr("dofoff", nl), m.arr("mtype", nl)
    gear, J = m.arr("mot_gear", nl), m.arr("mot_inertia", nl)
    out = np.zeros(m.ndof)
    for i in range(nl):
        if jt[i] in (rm.REVOL, rm.PRISM) and mt[i] == rm.MOTOR_DC:
            out[off[i]] = gear[i] ** 2 * J[i]
    return out


# ---- the worlds ---------------------------------------------------------------------------------------------------------------------
def cases(R):
    """the model files: jac_cases.WORLDS (revolute, spherical, float, merged links, breakable, five chains), frames orthonormal to
    rounding, both references"""
    return {k: dict(c, ortho=True) for k, c in jc.cases(R).items()}


def _reg_text(R, tmp_path, name, txt):
    f = tmp_path / f"{name}.ztk"
    f.write_text(txt)
    w = R.World(solver=R.SOLVER_MLCP); w.reg_file(str(f))
    return w


def limit_tree_cases(R, tmp_path, ortho):
    """the three limit trees (64 coordinates, 96 model links, 63 spherical coordinates): raw, or with orthonormalised frames"""
    out = {}
    for name in LIMIT_TREES:
        c = tl.BY_NAME[name]
        par, jt = c.topo
        txt = tl.tree_ztk(c.name, par, jt, c.seed, motors=c.motors)
        w = _reg_text(R, tmp_path, name + ("_on" if ortho else ""), ec._orthonormal_frames(txt) if ortho else txt)
        m = w.model.contents
        assert (m.nlink, m.ndof) == (c.dims[0], c.dims[2])
        dis, vel = tl.states(w, 2)
        out[name] = dict(world=w, dis=dis, vel=vel, broken=None, ortho=ortho)
    return out


def random_tree_cases(R, tmp_path, ortho, n=10):
    """the ten random trees of links_cases.random_tree_cases: raw, or with orthonormalised frames"""
    out = {}
    for k in range(n):
        seed = 300 + k
        txt = random_tree_ztk(seed, 4 + 5 * k, root=["float", "fixed", "revolute"][k % 3])
        w = _reg_text(R, tmp_path, f"rand{seed}" + ("_on" if ortho else ""), ec._orthonormal_frames(txt) if ortho else txt)
        if w.model.contents.ndof > 64:
            continue
        dis, vel = lc.states(w, 2, seed)
        out[f"rand{seed}"] = dict(world=w, dis=dis, vel=vel, broken=None, ortho=ortho)
    return out


def fixed_star(R, tmp_path, nfixed):
    """a revolute root with nfixed fixed links on it (frames orthonormalised): one device link, 51 ( nfixed + 1 ) + 6 doubles of LDS
    per instance - 420 of them are more than the 160 KiB a workgroup can have even with one instance"""
    txt = tl.tree_ztk("fixedstar", [None] + [0] * nfixed, ["revolute"] + ["fixed"] * nfixed, 7000 + nfixed)
    return _reg_text(R, tmp_path, f"fixedstar{nfixed}", ec._orthonormal_frames(txt))


def tile(c, B, seed=0xD71):
    """B states ( dis, vel, broken or None ) of a case: its seeded ones, then further seeded draws (broken flags repeated)"""
    n = c["dis"].shape[0]
    d2, v2 = lc.states(c["world"], B, seed + B)
    d2[:min(n, B)] = c["dis"][:B]; v2[:min(n, B)] = c["vel"][:B]
    br = None if c.get("broken") is None else np.stack([c["broken"][i % n] for i in range(B)])
    return d2, v2, br


def check_world(R, oracle_cls, c, got, what, idx=None, par=None):
    """M against A; on worlds with orthonormal frames M, h, g against B; the structure.  idx: the instances the references are
    evaluated on (all when None) - the structure is checked on every instance"""
    sel = np.arange(c["dis"].shape[0]) if idx is None else np.asarray(idx)
    pick = lambda a: None if a is None else np.asarray(a)[sel]
    sub = {k: v[sel] for k, v in got.items()}
    ppar = None if par is None else {k: pick(v) for k, v in par.items()}
    dev = {"A": check(sub, reference_a(R, oracle_cls, c["world"], c["dis"][sel], pick(c.get("broken")), ppar), what + " [A]", keys=("M",))}
    if c["ortho"]:
        dev["B"] = check(sub, reference_b(c["world"], c["dis"][sel], c["vel"][sel], ppar), what + " [B]")
    if "M" in got:
        check_structure(c["world"], got["M"], what)
    return dev
