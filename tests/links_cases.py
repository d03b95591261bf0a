"""Helpers of the task-space read-out tests (rkfdBatchUpdateLinks; tests/test_emu_links.py, tests/test_gpu_links.py): the worlds,
seeded states, the reference of the comparison protocol and the bound.

Protocol: a state (dis, vel, broken) goes into the oracle with set_state / set_broken, rkfdOracleEval( o, 0 ), then link_frames()
and link_vel_acc()[0] are the reference of R, p and v; com / comvel are numpy sums over those frames and velocities with the
model's (or the instance's) masses and centres of mass; positions are compared with scenarios.link_frames as well.
Bound: both sides compose at most 64 rigid transforms in fp64 from identical inputs, so they differ by depth x a few ulp,
~1e-14 x the scene's extent; asserted is |delta| <= 1e-12 max( 1, |value|_inf of that array )."""
import ctypes as C
import os
import subprocess

import numpy as np

from emu import ROOT, HERE
import instance_params as ip
from randtree import random_tree_ztk

POSE, VEL, COM = 1, 2, 4
ALL = 7
TOL = 1e-12
KEYS = ("R", "p", "v", "com", "comvel")
_emu = None


def emu_lib():
    global _emu
    if _emu is None:
        path = os.path.join(HERE, "librkfd_emu_links.so")
        if not os.path.exists(path):
            subprocess.run(["make", "-C", ROOT, "emu"], check=True, stdout=subprocess.DEVNULL)
        L = C.CDLL(path)
        L.rkfd_emu_links.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 7
        _emu = L
    return _emu


def emu_links(world, dis, vel, flags=ALL, par=None):
    """the read-out's device code under the lane emulator: dict as Batch.get_links(); par = (mass [B, nl], com [B, 3 nl])"""
    m = world.model.contents
    B = dis.shape[0]
    dis = np.ascontiguousarray(dis, dtype=np.float64); vel = np.ascontiguousarray(vel, dtype=np.float64)
    shapes = {"R": (B, m.nlink, 3, 3), "p": (B, m.nlink, 3), "v": (B, m.nlink, 6), "com": (B, m.nchain, 3), "comvel": (B, m.nchain, 3)}
    need = {"R": POSE, "p": POSE, "v": VEL, "com": COM, "comvel": COM}
    out = {k: np.full(shapes[k], np.nan) for k in KEYS if flags & need[k]}
    pm = pc = None
    if par is not None:
        pm = np.ascontiguousarray(par[0], dtype=np.float64); pc = np.ascontiguousarray(par[1], dtype=np.float64)
    p = lambda a: None if a is None else a.ctypes.data
    r = emu_lib().rkfd_emu_links(C.cast(world.model, C.c_void_p), B, p(dis), p(vel), flags, p(pm), p(pc), *[p(out.get(k)) for k in KEYS])
    assert r == 0
    return out


def states(world, B, seed, scale=0.8):
    m = world.model.contents
    rng = np.random.default_rng(seed)
    return rng.uniform(-scale, scale, (B, m.ndof)), rng.uniform(-1.0, 1.0, (B, m.ndof))


def reference(R, oracle_cls, world, dis, vel, broken=None, mass=None, com=None, libpath=None):
    """the protocol's reference for the states dis / vel [B, ndof] (broken [B, nl] or None; mass [B, nl] / com [B, 3 nl]: the
    instances' own, else the model's): dict as Batch.get_links()"""
    m = world.model.contents
    B, nl, nc = dis.shape[0], m.nlink, m.nchain
    chain = m.arr("chain", nl)
    out = {"R": np.zeros((B, nl, 3, 3)), "p": np.zeros((B, nl, 3)), "v": np.zeros((B, nl, 6)), "com": np.zeros((B, nc, 3)), "comvel": np.zeros((B, nc, 3))}
    o = oracle_cls(world.model, libpath) if libpath else oracle_cls(world.model)
    for i in range(B):
        o.set_state(dis[i], vel[i])
        o.set_broken(np.zeros(nl, dtype=np.int32) if broken is None else broken[i])
        o.eval(False)
        Ri, pi = o.link_frames(); vi = o.link_vel_acc()[0]
        out["R"][i], out["p"][i], out["v"][i] = Ri, pi, vi
        ms = m.arr("mass", nl) if mass is None else np.asarray(mass[i])
        cm = (m.arr("com", 3 * nl) if com is None else np.asarray(com[i])).reshape(nl, 3)
        cw = pi + np.einsum("lij,lj->li", Ri, cm)
        vc = np.einsum("lij,lj->li", Ri, vi[:, :3] + np.cross(vi[:, 3:], cm))
        for c in range(nc):
            sel = chain == c
            M = ms[sel].sum()
            if M > 0:
                out["com"][i, c] = (ms[sel, None] * cw[sel]).sum(0) / M
                out["comvel"][i, c] = (ms[sel, None] * vc[sel]).sum(0) / M
    o.close()
    return out


def deviations(got, ref, keys=KEYS):
    """{name: |delta|_inf / max( 1, |ref|_inf )} - the figure the bound TOL is about"""
    return {k: float(np.abs(got[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())) if ref[k].size else 0.0 for k in keys if k in got}


def check(got, ref, what, keys=KEYS):
    d = deviations(got, ref, keys)
    print(what, {k: "%.2e" % x for k, x in d.items()})
    for k, x in d.items():
        assert np.isfinite(got[k]).all(), (what, k)
        assert x <= TOL, (what, k, x)
    return d


def check_positions_second_fk(R, world, dis, got, what):
    """positions (and orientations) against scenarios.link_frames, the second, independent forward kinematics"""
    R2, p2 = R.scenarios.link_frames(world.model.contents, dis)
    check({"R": got["R"], "p": got["p"]}, {"R": R2, "p": p2}, what + " [scenarios.link_frames]", keys=("R", "p"))


# ---- the worlds: each a place where the read-out can go wrong -------------------------------------------------------------------
def _reg(R, files, solver=None, ci=True):
    M = R.scenarios.MODELS
    w = R.World(solver=R.SOLVER_MLCP if solver is None else solver)
    if ci:
        w.contact_info(os.path.join(M, "contactinfo.ztk"))
    for f in files:
        w.reg_file(os.path.join(M, f))
    return w


def aa_edge_states(world, B, seed):
    """states of arm_spher whose first joint's angle-axis vector is exactly zero, below the identity threshold, and within 1e-9 of
    |aa| = pi; the other joints random"""
    dis, vel = states(world, B, seed)
    ax = np.array([0.6, -0.48, 0.64])
    edge = [np.zeros(3), 3e-13 * ax, 1e-7 * ax, (np.pi - 1e-9) * ax, (np.pi + 1e-9) * ax]
    for i in range(B):
        dis[i, 0:3] = edge[i % len(edge)]
    return dis, vel


def cases(R, tmp_path=None):
    """name -> dict(world, dis, vel, broken or None): the worlds of the issue at seeded states (B = 3 each, arm_spher 5)"""
    S = R.scenarios
    out = {}

    def add(name, world, B=3, seed=0, broken=None, st=None):
        dis, vel = st if st is not None else states(world, B, 0x11AC + seed)
        out[name] = dict(world=world, dis=dis, vel=vel, broken=broken)
    add("chain30", S.config2(batch=1)["world"], seed=1)                    # depth 30: five pointer-jumping rounds
    add("humanoid30_shell", S.config4_shell(batch=1)["world"], seed=2)      # float base, fixed joints merged: model links != device links
    add("humanoid30", S.config4(batch=1)["world"], seed=3)
    w = S.arm_spher(batch=1)["world"]
    add("arm_spher", w, B=5, st=aa_edge_states(w, 5, 0x11AC + 4))           # spherical joints as three pseudo-links
    for nm, files in (("wall_cantilever", ["wall_cantilever.ztk", "floor.ztk"]), ("wall", ["wall.ztk", "box.ztk", "floor.ztk"])):
        w = _reg(R, files)
        m = w.model.contents
        brf = (m.arr("jtype", m.nlink) == 5).astype(np.int32)
        some = brf.copy(); some[np.flatnonzero(brf)[::2]] = 0
        add(nm, w, seed=5, broken=np.stack([0 * brf, some, brf]))            # breakable float joints: none, some, all broken
    sc = S.config5(batch=1)                                                # several chains, a static floor chain - made massless here
    m = sc["world"].model.contents
    ms = m.arr("mass", m.nlink); ms[m.arr("chain", m.nlink) == m.nchain - 1] = 0.0
    add("config5", ip.model_with(sc["world"], {"mass": ms}), seed=6)
    return out


def wall_after_steps(R, make_batch, nsteps):
    """scenarios.wall_hit's two instances whose joints break in stages (tests/test_emu_parity.py), stepped nsteps by the batch
    make_batch( world, B, max_rigid ) returns: (dis, vel, broken, world) as the steps left them; some joints must have broken in
    the run and some must have held"""
    sc = R.scenarios.wall_hit(batch=10)
    pick = [2, 9]
    b = make_batch(sc["world"], 2, sc["max_rigid"])
    b.set_state(sc["dis"][pick], sc["vel"][pick]); b.update_init()
    br0 = np.array(b.get_broken()).copy()
    b.update(nsteps)
    assert b.status() == 0
    dis, vel, _ = b.get_state()
    br = np.array(b.get_broken())
    assert br.sum() > br0.sum() and (br.sum(axis=1) < (sc["world"].model.contents.arr("jtype", br.shape[1]) == 5).sum()).all()
    assert np.abs(vel).max() > 0.05
    return dis, vel, br, sc["world"]


def random_tree_cases(R, tmp_path, n=10):
    """ten seeded trees of tests/randtree.py: prismatic joints, which no model file has"""
    out = {}
    for k in range(n):
        seed = 300 + k
        nlink = 4 + 5 * k
        f = tmp_path / f"rand{seed}.ztk"
        f.write_text(random_tree_ztk(seed, nlink, root=["float", "fixed", "revolute"][k % 3]))
        w = R.World(solver=R.SOLVER_MLCP); w.reg_file(str(f))
        m = w.model.contents
        if m.ndof > 64:
            continue
        dis, vel = states(w, 2, seed)
        out[f"rand{seed}"] = dict(world=w, dis=dis, vel=vel, broken=None)
    return out
