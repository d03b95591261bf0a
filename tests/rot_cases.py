"""Helpers of the large-rotation tests (tests/test_rot_primitives.py, tests/test_emu_rotations.py, tests/test_gpu_rotations.py,
tools/rot_parity.py): the rotation primitives of roki-fd_amd/csrc/device/rkfd_dev_base.h against long double, seeded states beyond
the first quadrant, the case table of the four read-outs at those states, the rollouts, and the comparison of states in
rotation-matrix space.  No device code in here.

Every other random state of the suite sits within +-0.8 rad (links_cases.states) and base attitudes within +-0.3: d_sincos never
leaves its k = 0 quadrant there, d_atan2_ypos never sees x < 0 and d_to_aa nothing beyond a quarter turn.  big_states draws
revolute coordinates from +-3.2 and +-40 rad and gives every float / spherical / broken breakable-float block a rotation of
2.2, 3.0, pi - 1e-3 or 4.0 rad about a random axis.

References and bounds are those of the case modules this one reuses (links_cases, jac_cases, dyn_cases, cf_cases: 1e-12 max( 1,
|value|_inf )); the primitives are compared with np.longdouble (64-bit mantissa: eps 1.1e-19, asserted by the test)."""
import ctypes as C
import os
import subprocess

import numpy as np

from emu import ROOT, HERE
import cf_cases as cc
import dyn_cases as dc
import instance_params as ip
import jac_cases as jc
import links_cases as lc

LD = np.longdouble
EPS = 2.0 ** -52
PI_LD = LD(np.pi) + LD(1.2246467991473532e-16)          # pi to ~1e-32, good to long double's 1.1e-19
FIXED, REVOL, PRISM, FLOAT, SPHER, BRFLOAT = 0, 1, 2, 3, 4, 5
THETAS = (2.2, 3.0, np.pi - 1e-3, 4.0)                  # the last one, beyond pi, is for read-outs only
REV_SCALES = (3.2, 40.0)
_prim = None


# ---- the primitives under the emulator build ------------------------------------------------------------------------------------------
def prim_lib():
    global _prim
    if _prim is None:
        path = os.path.join(HERE, "librkfd_emu_prim.so")
        if not os.path.exists(path):
            subprocess.run(["make", "-C", ROOT, "emu"], check=True, stdout=subprocess.DEVNULL)
        L = C.CDLL(path)
        L.rkfd_emu_prim_sincos.argtypes = [C.c_int] + [C.c_void_p] * 3
        L.rkfd_emu_prim_atan2_ypos.argtypes = [C.c_int] + [C.c_void_p] * 3
        L.rkfd_emu_prim_from_aa.argtypes = [C.c_int] + [C.c_void_p] * 2
        L.rkfd_emu_prim_to_aa.argtypes = [C.c_int] + [C.c_void_p] * 2
        for f in (L.rkfd_emu_prim_sincos, L.rkfd_emu_prim_atan2_ypos, L.rkfd_emu_prim_from_aa, L.rkfd_emu_prim_to_aa):
            f.restype = None
        _prim = L
    return _prim


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def d_sincos(x):
    x = _f64(x).ravel()
    s, c = np.full(x.size, np.nan), np.full(x.size, np.nan)
    prim_lib().rkfd_emu_prim_sincos(x.size, x.ctypes.data, s.ctypes.data, c.ctypes.data)
    return s, c


def d_atan2_ypos(y, x):
    y, x = _f64(y).ravel(), _f64(x).ravel()
    assert y.size == x.size and (y >= 0).all()
    r = np.full(x.size, np.nan)
    prim_lib().rkfd_emu_prim_atan2_ypos(x.size, y.ctypes.data, x.ctypes.data, r.ctypes.data)
    return r


def d_from_aa(aa):
    aa = _f64(aa).reshape(-1, 3)
    m = np.full((aa.shape[0], 3, 3), np.nan)
    prim_lib().rkfd_emu_prim_from_aa(aa.shape[0], aa.ctypes.data, m.ctypes.data)
    return m


def d_to_aa(m):
    m = _f64(m).reshape(-1, 3, 3)
    aa = np.full((m.shape[0], 3), np.nan)
    prim_lib().rkfd_emu_prim_to_aa(m.shape[0], m.ctypes.data, aa.ctypes.data)
    return aa


# ---- inputs of the primitives ---------------------------------------------------------------------------------------------------------
SINCOS_RANGES = (0.8, 3.2, 100.0, 1e3, 1e4, 1e5)


def _ulps(x, n):
    for _ in range(abs(n)):
        x = np.nextafter(x, np.inf if n > 0 else -np.inf)
    return x


def sincos_inputs(ndraw=50000, seed=0x51C0):
    """name -> inputs: seeded uniform draws per range; every k pi/2, |k| <= 64, with its +-1 ulp, +-2 ulp and +-1e-9 neighbours;
    the midpoints ( k + 0.5 ) pi/2, where rint( x 2/pi ) ties"""
    rng = np.random.default_rng(seed)
    out = {"uniform +-%g" % r: rng.uniform(-r, r, ndraw) for r in SINCOS_RANGES}
    k = np.arange(-64, 65, dtype=np.float64)
    m = k * (np.pi / 2)
    out["k pi/2 and neighbours"] = np.concatenate([m, _ulps(m, 1), _ulps(m, -1), _ulps(m, 2), _ulps(m, -2), m + 1e-9, m - 1e-9])
    out["midpoints"] = (k + 0.5) * (np.pi / 2)
    return out


def sincos_errors(x):
    """(max |s - sin|, max |c - cos|, max |s^2 + c^2 - 1|) against long double"""
    s, c = d_sincos(x)
    xl = _f64(x).ravel().astype(LD)
    sl, cl = s.astype(LD), c.astype(LD)
    return float(np.abs(sl - np.sin(xl)).max()), float(np.abs(cl - np.cos(xl)).max()), float(np.abs(sl * sl + cl * cl - LD(1)).max())


ATAN_BOUNDARIES = (0.4375, 0.6875, 1.1875, 2.4375)


def atan2_inputs(ndraw=50000, seed=0xA7A2):
    """name -> (y, x), y >= 0, no negative zero: seeded draws (normal, and ratios spread over twelve decades); the four interval
    boundaries of d_atan_pos +-1 ulp on both signs of x and at three scales; x = +0.0; y = 0, 1e-300, 1e300"""
    rng = np.random.default_rng(seed)
    out = {"normal": (np.abs(rng.normal(size=ndraw)), rng.normal(size=ndraw))}
    xr = rng.choice([-1.0, 1.0], ndraw) * 10.0 ** rng.uniform(-3, 3, ndraw)
    out["log-uniform ratio"] = (10.0 ** rng.uniform(-6, 6, ndraw) * np.abs(xr), xr)
    b = np.array(ATAN_BOUNDARIES)
    r = np.concatenate([b, _ulps(b, 1), _ulps(b, -1)])
    ys, xs = [], []
    for sc in (1.0, 0.25, 8.0):          # powers of two: y / |x| is exactly r
        for sg in (1.0, -1.0):
            ys.append(r * sc); xs.append(np.full(r.size, sg * sc))
    out["interval boundaries"] = (np.concatenate(ys), np.concatenate(xs))
    out["x = +0"] = (np.array([1.0, 1e-300, 1e300, 0.0]), np.zeros(4))
    xe = np.array([1.0, -1.0, 1e-300, -1e-300, 1e300, -1e300, 3.0, -3.0])
    out["y = 0"] = (np.zeros(xe.size), xe)
    out["y = 1e-300"] = (np.full(xe.size, 1e-300), xe)
    out["y = 1e300"] = (np.full(xe.size, 1e300), xe)
    return out


def atan2_error(y, x):
    r = d_atan2_ypos(y, x)
    ref = np.arctan2(_f64(y).ravel().astype(LD), _f64(x).ravel().astype(LD))
    return float(np.abs(r.astype(LD) - ref).max())


def _axes(rng, n):
    a = rng.normal(size=(n, 3))
    return a / np.linalg.norm(a, axis=1)[:, None]


def aa_inputs(ndraw=5000, seed=0xAA01):
    """angle-axis vectors [n, 3]: theta = 0, 3e-13 (below the identity threshold RKFD_TOL = 1e-12), 1e-7, then ndraw draws from each
    of ( 0, pi/2 ), ( pi/2, pi ), ( pi, 2 pi ), then theta = 2 pi and 7; random axes"""
    rng = np.random.default_rng(seed)
    th = np.concatenate([[0.0, 3e-13, 1e-7], rng.uniform(0, np.pi / 2, ndraw), rng.uniform(np.pi / 2, np.pi, ndraw),
                         rng.uniform(np.pi, 2 * np.pi, ndraw), [2 * np.pi, 7.0]])
    return th[:, None] * _axes(rng, th.size)


def rodrigues_ld(aa):
    """(R [n, 3, 3], theta [n], axis [n, 3]) in long double of the fp64 vectors aa"""
    a = _f64(aa).reshape(-1, 3).astype(LD)
    th = np.sqrt((a * a).sum(axis=1))
    n = a / np.where(th > 0, th, LD(1))[:, None]
    s, c = np.sin(th), np.cos(th)
    K = np.zeros((a.shape[0], 3, 3), dtype=LD)
    K[:, 0, 1] = -n[:, 2]; K[:, 0, 2] = n[:, 1]; K[:, 1, 0] = n[:, 2]
    K[:, 1, 2] = -n[:, 0]; K[:, 2, 0] = -n[:, 1]; K[:, 2, 1] = n[:, 0]
    eye = np.eye(3, dtype=LD)[None]
    R = c[:, None, None] * eye + (1 - c)[:, None, None] * (n[:, :, None] * n[:, None, :]) + s[:, None, None] * K
    return R, th, n


IDENT_TOL = 1e-12          # RKFD_TOL (include/rkfd_model.h): d_from_aa returns the identity below it, by definition


def from_aa_errors(aa):
    """(max |R - Rodrigues| over theta >= RKFD_TOL; orthonormality: the largest of | |r| - 1 | over rows and columns and |r . r'| over
    distinct rows and distinct columns; max |R' R - 1|, for the record; the R).
    The formula's own defect is delta ( s^2 1 + k^2 n n' ) in R' R, delta = |n|^2 - 1 of the rounded unit axis and k = 1 - cos: at
    a half turn 4 delta n_i^2 on the diagonal, twice what it does to the length of that column"""
    Rd = d_from_aa(aa)
    Rl, th, _ = rodrigues_ld(aa)
    big = np.asarray(th >= IDENT_TOL)
    e = float(np.abs(Rd.astype(LD) - Rl)[big].max())
    Rq = Rd.astype(LD)
    eye = np.eye(3, dtype=LD)[None]
    orth = 0.0
    for G in (np.einsum("nki,nkj->nij", Rq, Rq), np.einsum("nik,njk->nij", Rq, Rq)):
        d = np.sqrt(np.einsum("nii->ni", G)) - 1
        orth = max(orth, float(np.abs(d).max()), float(np.abs(G * (1 - eye)).max()))
    gram = float(np.abs(np.einsum("nki,nkj->nij", Rq, Rq) - eye).max())
    return e, orth, gram, Rd


def wrapped_ld(aa):
    """the equivalent rotation vector with angle in ( -pi, pi ] of fp64 vectors aa, in long double: (vector [n, 3], pi - |angle| [n])"""
    _, th, n = rodrigues_ld(aa)
    w = th - 2 * PI_LD * np.round(th / (2 * PI_LD))
    return w[:, None] * n, PI_LD - np.abs(w)


def roundtrip_errors(aa):
    """d_to_aa( d_from_aa( aa ) ): (|result - equivalent rotation vector|_inf [n], its bound max( 1e-12, 1e-14 / ( pi - theta ) ) [n])"""
    back = d_to_aa(d_from_aa(aa))
    want, gap = wrapped_ld(aa)
    err = np.abs(back.astype(LD) - want).max(axis=1).astype(np.float64)
    bound = np.maximum(1e-12, 1e-14 / np.maximum(gap.astype(np.float64), 1e-300))
    return err, bound


# ---- states beyond the first quadrant -------------------------------------------------------------------------------------------------
def rot_blocks(m):
    """offsets of the angle-axis blocks in dis: [(offset, link)] of float, spherical and breakable-float joints"""
    jt, off = m.arr("jtype", m.nlink), m.arr("dofoff", m.nlink)
    return [(int(off[i]) + (0 if jt[i] == SPHER else 3), i) for i in range(m.nlink) if jt[i] in (FLOAT, SPHER, BRFLOAT)]


def big_states(world, B, seed, broken=None, thetas=THETAS):
    """(dis, vel) [B, ndof]: revolute coordinates uniform in +-3.2 or +-40 rad by instance, prismatic ones in +-0.8 m, translations
    of float joints in +-0.8 m; every float, spherical and BROKEN breakable-float block a rotation about a random axis by
    thetas[i % len] (an unbroken breakable joint keeps a draw from +-0.8); rates uniform in +-1.  B = 8 holds every pair of scale
    and theta"""
    m = world.model.contents
    rng = np.random.default_rng(0xB160 + seed)
    jt, off = m.arr("jtype", m.nlink), m.arr("dofoff", m.nlink)
    dis = rng.uniform(-0.8, 0.8, (B, m.ndof)); vel = rng.uniform(-1.0, 1.0, (B, m.ndof))
    for i in range(B):
        sc = REV_SCALES[(i + i // 4) % 2]
        for l in range(m.nlink):
            if jt[l] == REVOL:
                dis[i, off[l]] = rng.uniform(-sc, sc)
        for o, l in rot_blocks(m):
            ax = _axes(rng, 1)[0]
            if jt[l] == BRFLOAT and (broken is None or not broken[i][l]):
                continue
            dis[i, o:o + 3] = thetas[i % len(thetas)] * ax
    return dis, vel


def rot_dev(R, m, got, ref):
    """largest |R( got block ) - R( ref block )| over the angle-axis blocks of dis [B, ndof]: device and oracle may come out on
    opposite sides of pi, and those are equal rotations"""
    w = 0.0
    for o, _ in rot_blocks(m):
        w = max(w, float(np.abs(R.scenarios._rot_aa_batch(got[:, o:o + 3]) - R.scenarios._rot_aa_batch(ref[:, o:o + 3])).max()))
    return w


def state_dev(R, m, got, ref):
    """worst deviation of ( dis, vel, acc ) [B, ndof] each from the oracle's: angle-axis blocks of dis in rotation-matrix space, all
    other coordinates per instance as |delta|_inf / max( 1, |oracle|_inf ) (tests/test_random_trees.py)"""
    gd, rd = got[0].copy(), ref[0].copy()
    w = rot_dev(R, m, gd, rd)
    for o, _ in rot_blocks(m):
        gd[:, o:o + 3] = 0.0; rd[:, o:o + 3] = 0.0
    for x, y in ((gd, rd), (got[1], ref[1]), (got[2], ref[2])):
        for i in range(x.shape[0]):
            w = max(w, float(np.abs(x[i] - y[i]).max() / max(1.0, np.abs(y[i]).max())))
    return w


# ---- the read-out cases ---------------------------------------------------------------------------------------------------------------
READOUT_WORLDS = ["chain30", "humanoid30", "arm_spher", "wall", "rand303_on", "rand305_on"]


def readout_cases(R, tmp_path, B):
    """name -> one dict that serves links_cases, jac_cases, dyn_cases and cf_cases: world, dis, vel, broken, links, points, ortho, cand,
    active, f, synthetic.  The worlds are those modules' own; the states are big_states.  The wall has some joints broken on every
    instance; the two random trees (frames orthonormalised: both references of dyn_cases / cf_cases apply) have prismatic joints and
    carry synthetic candidates, which only the emulator's harness takes"""
    lcs = lc.cases(R)
    trees = dc.random_tree_cases(R, tmp_path, ortho=True)
    out = {}
    for k, name in enumerate(READOUT_WORLDS):
        tree = name.startswith("rand")
        w = trees[name[:-3]]["world"] if tree else lcs[name]["world"]
        m = w.model.contents
        br = None
        if name == "wall":
            some = lcs[name]["broken"][1]
            assert some.any() and not (some == (m.arr("jtype", m.nlink) == BRFLOAT)).all()
            br = np.tile(some, (B, 1))
        dis, vel = big_states(w, B, k, broken=br)
        links, pts = jc.sites_for(w, 80 + k)
        cand = cc.synthetic_cand(w, 40, 80 + k) if tree else cc.model_cand(w)
        act, f = cc.random_inputs(B, cand.n, 80 + k)
        out[name] = dict(world=w, dis=dis, vel=vel, broken=br, links=links, points=pts, ortho=True, cand=cand, active=act, f=f, synthetic=tree)
    for name in ("rand303_on", "rand305_on"):
        m = out[name]["world"].model.contents
        assert (m.arr("jtype", m.nlink) == PRISM).any(), name
    return out


def emu_readouts(c, par=None):
    """the four read-outs of a case under the lane emulator: {"links": .., "jac": .., "dyn": .., "cf": ..}; par: a parameter table as
    instance_params.randomised gives it (mass, com, inertia are what the read-outs take)"""
    w = c["world"]
    mc = None if par is None else (par["mass"], par["com"])
    return {"links": lc.emu_links(w, c["dis"], c["vel"], par=mc),
            "jac": jc.emu_jac(w, c["dis"], c["links"], c["points"], par=mc),
            "dyn": dc.emu_dyn(w, c["dis"], c["vel"], par=par),
            "cf": cc.emu_cf(w, c["dis"], c["active"], c["f"], cand=c["cand"] if c["synthetic"] else None)}


def check_readouts(R, oracle_cls, c, got, what, idx=None, par=None):
    """every read-out in `got` against the references its own case module uses, at that module's bound (links_cases.TOL); idx: the
    instances (all when None); par: the parameter table the read-outs ran with.  -> {read-out: worst deviation}"""
    sel = np.arange(c["dis"].shape[0]) if idx is None else np.asarray(idx)
    pick = lambda a: None if a is None else np.asarray(a)[sel]
    sub = lambda g: {k: v[sel] for k, v in g.items()}
    w = c["world"]
    mass, com = (None, None) if par is None else (par["mass"][sel], par["com"][sel])
    dev = {}
    if "links" in got:
        g = sub(got["links"])
        d = lc.check(g, lc.reference(R, oracle_cls, w, c["dis"][sel], c["vel"][sel], pick(c["broken"]), mass=mass, com=com), what + " links")
        lc.check_positions_second_fk(R, w, c["dis"][sel], g, what + " links")
        dev["links"] = max(d.values())
    if "jac" in got:
        ref = jc.reference(R, oracle_cls, w, c["dis"][sel], c["links"], c["points"], pick(c["broken"]), mass=mass, com=com)
        dev["jac"] = max(jc.check(sub(got["jac"]), ref, what + " jac").values())
    if "dyn" in got:
        d = dc.check_world(R, oracle_cls, c, got["dyn"], what + " dyn", idx=sel, par=par)
        dev["dyn"] = max(max(x.values()) for x in d.values())
    if "cf" in got:
        d = cc.check_world(R, oracle_cls, c, got["cf"], what + " cf", idx=sel)
        dev["cf"] = max([max(x.values()) for x in d.values() if x] + [0.0])
    return dev


def check_against_emulator(got, emu, what):
    """the GPU's read-outs against the emulator's on every instance, at the same bound.  -> {read-out: worst deviation}"""
    dev = {}
    for k, chk in (("links", lc.check), ("jac", jc.check), ("dyn", dc.check), ("cf", cc.check)):
        if k in got:
            d = chk(got[k], emu[k], f"{what} {k} [emulator, every instance]")
            dev[k] = max(list(d.values()) + [0.0])
    return dev


# ---- the rollouts ---------------------------------------------------------------------------------------------------------------------
def free_box_world(R):
    """models/box.ztk alone: one float link, nothing to touch"""
    return lc._reg(R, ["box.ztk"], ci=False)


NROLL = 8          # the generators below draw eight instances and hand out the first B: instance i is the same whatever B


def chain30_rollout(R, B=3):
    """chain30 at +-40 rad and +-8 rad/s, 20 steps"""
    w = R.scenarios.config2(batch=1)["world"]
    rng = np.random.default_rng(0xC430)
    nd = w.model.contents.ndof
    dis, vel = rng.uniform(-40.0, 40.0, (NROLL, nd)), rng.uniform(-8.0, 8.0, (NROLL, nd))
    return dict(name="chain30 +-40 rad", world=w, dis=dis[:B].copy(), vel=vel[:B].copy(), steps=20, max_rigid=0)


def humanoid_rollout(R, B=4):
    """humanoid30 three metres above the floor, joints in +-3.2 rad at +-1 rad/s, the base at theta = 2.2 and 3.1 about random axes,
    turning at 15 rad/s about random axes; 40 steps.  Its own pairs are unregistered: at such angles its shapes sit inside each
    other, which is not what this is about (tests/test_random_trees.py does the same)"""
    M = R.scenarios.MODELS
    w = R.World(solver=R.SOLVER_MLCP)
    w.contact_info(os.path.join(M, "contactinfo.ztk"))
    h = w.reg_file(os.path.join(M, "humanoid30.ztk"))
    w.pair_chain_unreg(h)
    w.reg_file(os.path.join(M, "floor.ztk"))
    m = w.model.contents
    rng = np.random.default_rng(0x4830)
    dis = rng.uniform(-3.2, 3.2, (NROLL, m.ndof)); vel = rng.uniform(-1.0, 1.0, (NROLL, m.ndof))
    assert [o for o, _ in rot_blocks(m)] == [3]
    dis[:, 0:2] = 0.0; dis[:, 2] = 3.0
    dis[:, 3:6] = np.array([2.2, 3.1])[np.arange(NROLL) % 2][:, None] * _axes(rng, NROLL)
    vel[:, 0:3] = rng.uniform(-0.5, 0.5, (NROLL, 3)); vel[:, 3:6] = 15.0 * _axes(rng, NROLL)
    return dict(name="airborne humanoid30", world=w, dis=dis[:B].copy(), vel=vel[:B].copy(), steps=40, max_rigid=8)


def tumbling_box(R, B=4):
    """a free box turning at 20 - 25 rad/s about random axes from random attitudes, 400 steps of 1 ms: 8 - 10 rad, through the half
    turn at least once (assert_tumble_gates asserts that on the oracle's trajectory).  models/box.ztk is a cube, whose angular
    velocity would simply stay: the principal inertias are set to 0.6 : 1.0 : 1.4 of the cube's, so that the body precesses"""
    w = free_box_world(R)
    I = w.model.contents.arr("inertia", 9).reshape(3, 3) * np.diag([0.6, 1.0, 1.4])
    w = ip.model_with(w, {"inertia": I.ravel()})
    rng = np.random.default_rng(0x7B0D)          # (seed 0x7B0C brings one instance within 1.4e-5 of pi: outside the gate)
    dis = np.zeros((NROLL, 6)); vel = np.zeros((NROLL, 6))
    dis[:, 3:6] = rng.uniform(0.5, 2.5, NROLL)[:, None] * _axes(rng, NROLL)
    vel[:, 0:3] = rng.uniform(-0.5, 0.5, (NROLL, 3))
    vel[:, 3:6] = rng.uniform(20.0, 25.0, NROLL)[:, None] * _axes(rng, NROLL)
    return dict(name="tumbling box", world=w, dis=dis[:B].copy(), vel=vel[:B].copy(), steps=400, max_rigid=0)


def oracle_trajectory(oracle_cls, sc, frames=False):
    """the oracle's states after update_init and after every step: dis, vel, acc [B, steps + 1, ndof]; frames: also the link frames
    and link velocities of link 0 (R [B, steps + 1, 3, 3], v [B, steps + 1, 6])"""
    B, nd, n = sc["dis"].shape[0], sc["dis"].shape[1], sc["steps"]
    out = {k: np.zeros((B, n + 1, nd)) for k in ("dis", "vel", "acc")}
    out["R"] = np.zeros((B, n + 1, 3, 3)); out["v"] = np.zeros((B, n + 1, 6)); out["ncontact"] = 0
    for i in range(B):
        o = oracle_cls(sc["world"].model)
        o.set_state(sc["dis"][i], sc["vel"][i]); o.update_init()
        for t in range(n + 1):
            if t:
                o.update()
            out["dis"][i, t], out["vel"][i, t], out["acc"][i, t] = o.get_state()
            if frames:
                out["R"][i, t] = o.link_frames()[0][0]; out["v"][i, t] = o.link_vel_acc()[0][0]
            out["ncontact"] += int((o.get_contact()[0] != 0).sum()) if sc["world"].model.contents.ncand else 0
        o.close()
    return out


def tumble_gates(traj_dis):
    """(half-turn crossings [B], closest approach pi - |aa| [B]) of the oracle's trajectory dis [B, T, 6]: a crossing shows as the
    angle-axis vector jumping to the opposite axis, consecutive vectors with a negative dot product"""
    aa = traj_dis[:, :, 3:6]
    crossings = ((aa[:, 1:] * aa[:, :-1]).sum(axis=2) < 0).sum(axis=1)
    closest = (np.pi - np.linalg.norm(aa, axis=2)).min(axis=1)
    return crossings, closest


def assert_tumble_gates(traj_dis):
    crossings, closest = tumble_gates(traj_dis)
    assert (crossings >= 1).all(), crossings
    assert (closest >= 1e-4).all(), closest
    return crossings, closest


def upside_down_box(R):
    """a box nearly upside down, |aa| = 3.06, 3.11 and 2.42 about axes near x, its lowest vertex 1e-5 m inside the rigid floor (MLCP)
    and moving down at 0.05 m/s with some spin: in contact at the first evaluation, contacts made and broken in the first six
    steps (the oracle's counts per step: 1111001.., 1112111.., 1111001..) and held from then on; 30 steps"""
    M = R.scenarios.MODELS
    w = R.World(solver=R.SOLVER_MLCP)
    w.contact_info(os.path.join(M, "contactinfo.ztk"))
    c = w.reg_file(os.path.join(M, "box.ztk"))
    w.reg_file(os.path.join(M, "floor.ztk"))
    m = w.model.contents
    ax = np.array([[1.0, 0.05, 0.02], [0.98, -0.1, 0.15], [0.9, 0.3, -0.2]])
    ax /= np.linalg.norm(ax, axis=1)[:, None]
    dis = np.zeros((3, m.ndof)); vel = np.zeros((3, m.ndof))
    o = w.dof_offset(c)
    dis[:, o + 3:o + 6] = np.array([3.06, 3.11, 2.42])[:, None] * ax
    dis[:, o + 2] = 0.2
    for i in range(3):
        dis[i, o + 2] -= R.scenarios.lowest_vertex_z(m, dis[i], c) + 1e-5
    vel[:, o + 2] = -0.05
    vel[:, o + 3:o + 6] = np.array([[0.4, -0.3, 0.2], [-0.5, 0.2, 0.3], [0.3, 0.3, -0.4]])
    return dict(name="upside-down box on the floor", world=w, dis=dis, vel=vel, steps=30, max_rigid=8)


# the half turn: DEVIATIONS.md, "A half turn is written back as the identity"
def half_turn_cases():
    """(name, angle about x, spin about x [rad/s], collapses)"""
    return [("at rest at pi", np.pi, 0.0, True), ("pi - 1e-6 turning at 1e-3 rad/s", np.pi - 1e-6, 1e-3, True),
            ("pi - 1e-3 turning at 1e-3 rad/s", np.pi - 1e-3, 1e-3, False)]


def half_turn_states():
    cs = half_turn_cases()
    dis = np.zeros((len(cs), 6)); vel = np.zeros((len(cs), 6))
    for i, (_, th, spin, _) in enumerate(cs):
        dis[i, 3] = th; vel[i, 3] = spin
    return dis, vel


def check_half_turn(one, two, odis1, odis2):
    """dis [3, 6] of half_turn_states after one and after two steps, the batch's and the oracle's.  With a step of 1 ms the second case
    reaches the half turn in its FIRST step and is written back as zero there; its second step starts from the identity"""
    for i, (name, th, spin, collapses) in enumerate(half_turn_cases()):
        for d1, d2 in ((one, two), (odis1, odis2)):
            a1, a2 = d1[i, 3:6], d2[i, 3:6]
            if collapses:
                assert (a1 == 0.0).all(), (name, a1)
                assert (a2[1:] == 0.0).all() and abs(a2[0] - 1e-3 * spin) <= 1e-15, (name, a2)          # the half turn is gone for good
            else:
                assert (a1[1:] == 0.0).all() and abs(a1[0] - (th + 1e-3 * spin)) < 1e-12, (name, a1)
                assert (a2[1:] == 0.0).all() and abs(a2[0] - (th + 2e-3 * spin)) < 1e-12, (name, a2)


# ---- long double forward kinematics of ONE link (the direct probes of tests/test_gpu_rotations.py) --------------------------------------
def probe_link(m):
    """the first link with a joint coordinate, all of whose ancestors are fixed (chain30: link 1 behind the fixed base; a float-root
    box: link 0)"""
    jt, par = m.arr("jtype", m.nlink), m.arr("parent", m.nlink)
    l = int(np.flatnonzero(jt != FIXED)[0])
    k = par[l]
    while k >= 0:
        assert jt[k] == FIXED
        k = par[k]
    return l


def probe_frame_ld(m, dis):
    """world frame of probe_link( m ) in long double: (R [B, 3, 3], p [B, 3]).  The fixed ancestors' frames composed, then revolute:
    org_R Rz( q ); float: org_R R( aa ), org_p + org_R t.  One frame product of three terms on values good to 2^-52 each: 2e-15 is
    asserted"""
    l = probe_link(m)
    jt = int(m.arr("jtype", m.nlink)[l]); off = int(m.arr("dofoff", m.nlink)[l])
    par = m.arr("parent", m.nlink)
    org = m.arr("org", 12 * m.nlink).reshape(m.nlink, 12).astype(LD)
    Rp, pp = np.eye(3, dtype=LD), np.zeros(3, dtype=LD)
    path = []
    k = par[l]
    while k >= 0:
        path.append(int(k)); k = par[k]
    for k in reversed(path):
        pp = pp + Rp @ org[k, 9:]; Rp = Rp @ org[k, :9].reshape(3, 3)
    Ro, po = org[l, :9].reshape(3, 3), org[l, 9:]
    B = dis.shape[0]
    if jt == REVOL:
        q = _f64(dis[:, off]).astype(LD)
        Rj = np.zeros((B, 3, 3), dtype=LD)
        Rj[:, 0, 0] = np.cos(q); Rj[:, 0, 1] = -np.sin(q); Rj[:, 1, 0] = np.sin(q); Rj[:, 1, 1] = np.cos(q); Rj[:, 2, 2] = 1
        pj = np.tile(po, (B, 1))
    else:
        assert jt == FLOAT
        Rj, th, _ = rodrigues_ld(dis[:, off + 3:off + 6])
        Rj[np.asarray(th < IDENT_TOL)] = np.eye(3, dtype=LD)
        pj = po[None] + np.einsum("ij,bj->bi", Ro, _f64(dis[:, off:off + 3]).astype(LD))
    return np.einsum("ij,bjk->bik", Rp @ Ro, Rj), pp[None] + np.einsum("ij,bj->bi", Rp, pj)


SINCOS_SWEEP = np.concatenate([np.linspace(-40.0, 40.0, 41), np.arange(-8, 9) * (np.pi / 2), [0.8, -0.8, 2.5, -2.5, 1e3, -1e4, 1e5]])
AA_SWEEP_THETAS = np.array([0.0, 3e-13, 1e-7, 0.5, 1.5, 2.2, 3.0, np.pi - 1e-3, np.pi - 1e-9, np.pi, 4.0, 5.5, 2 * np.pi, 7.0])
TO_AA_THETAS = np.array([0.5, 2.0, 3.0, np.pi - 1e-3, 4.0])


def to_aa_bound(theta):
    """the round-trip bound of the issue for a rotation by theta: max( 1e-12, 1e-14 / ( pi - |theta wrapped| ) )"""
    w = np.abs(np.asarray(theta) - 2 * np.pi * np.round(np.asarray(theta) / (2 * np.pi)))
    return np.maximum(1e-12, 1e-14 / np.maximum(np.pi - w, 1e-300))


# ---- the free-flight invariant ----------------------------------------------------------------------------------------------------------
def angular_momentum(m, Rw, v):
    """world angular momentum about the centre of mass of link 0, R ( I w ), from its world attitude Rw [.., 3, 3] and link-frame
    twist v [.., 6] (linear, angular); gravity has no moment about the centre of mass: constant in free flight"""
    I = m.arr("inertia", 9 * m.nlink).reshape(m.nlink, 3, 3)[0]
    return np.einsum("...ij,...j->...i", Rw, np.einsum("ij,...j->...i", I, v[..., 3:]))


def drift(L):
    """largest |L(t) - L(0)|_inf / |L(0)|_inf over the samples L [B, T, 3], per instance [B]"""
    return np.abs(L - L[:, :1]).max(axis=(1, 2)) / np.abs(L[:, 0]).max(axis=1)


# ---- on the GPU: what tests/test_gpu_rotations.py and tools/rot_parity.py both run --------------------------------------------------------
def gpu_readouts(R, c, par=None):
    """the four read-outs of a case from one batch (the trees' synthetic candidates exist in the emulator's harness only: no contact
    read-out there)"""
    b = R.Batch(c["world"], c["dis"].shape[0], device=0, max_rigid=0)
    b.set_state(c["dis"], c["vel"])
    if c["broken"] is not None:
        b.set_broken(c["broken"])
    if par is not None:
        for k in ("mass", "com", "inertia"):
            b.set_param(k, par[k])
    got = {}
    b.update_links(); got["links"] = b.get_links()
    b.set_jacobian_sites(c["links"], c["points"]); b.update_jacobians(); got["jac"] = b.get_jacobians()
    b.update_dynamics(); got["dyn"] = b.get_dynamics()
    if not c["synthetic"]:
        da, df = cc.DevArray(R, c["active"]), cc.DevArray(R, c["f"])
        b.update_contact_forces(active=da, f=df); got["cf"] = b.get_contact_forces()
        da.free(); df.free()
    assert b.status() == 0
    b.close()
    return got


def probe_sweep(R, world, dis_all):
    """(R, p) of rot_cases.probe_link for the states dis_all [n, ndof], eight at a time through one batch's read-out"""
    n = dis_all.shape[0]
    l = probe_link(world.model.contents)
    b = R.Batch(world, 8, device=0, max_rigid=0)
    Rs, ps = [], []
    for k in range(0, n, 8):
        d = np.zeros((8, dis_all.shape[1])); d[:min(8, n - k)] = dis_all[k:k + 8]
        b.set_state(d, np.zeros_like(d)); b.update_links(lc.POSE)
        g = b.get_links()
        Rs.append(g["R"][:, l].copy()); ps.append(g["p"][:, l].copy())
    assert b.status() == 0
    b.close()
    return np.concatenate(Rs)[:n], np.concatenate(ps)[:n]


def probe_error(R, world, dis_all):
    """|frame of the probe link on the device - long double forward kinematics of that link|_inf over R and p"""
    Rg, pg = probe_sweep(R, world, dis_all)
    Rl, pl = probe_frame_ld(world.model.contents, dis_all)
    return max(float(np.abs(Rg.astype(LD) - Rl).max()), float(np.abs(pg.astype(LD) - pl).max()))


def sincos_probe_states(R):
    w = R.scenarios.config2(batch=1)["world"]
    dis = np.zeros((SINCOS_SWEEP.size, w.model.contents.ndof)); dis[:, 0] = SINCOS_SWEEP
    return w, dis


def from_aa_probe_states(R):
    w = free_box_world(R)
    rng = np.random.default_rng(0xF0AA)
    dis = np.zeros((AA_SWEEP_THETAS.size, 6))
    dis[:, 0:3] = rng.uniform(-0.8, 0.8, dis[:, 0:3].shape)
    dis[:, 3:6] = AA_SWEEP_THETAS[:, None] * _axes(rng, dis.shape[0])
    return w, dis


def to_aa_probe(R, oracle_cls, specialized=False):
    """one step of a free box at rest from theta in TO_AA_THETAS: R( aa ) goes through d_from_aa, a product with the identity and
    d_to_aa.  -> (|R( device ) - R( oracle )| per instance, |R( device ) - R( start )| per instance, the bound per instance)"""
    w = free_box_world(R)
    rng = np.random.default_rng(0x70AA)
    n = TO_AA_THETAS.size
    dis = np.zeros((n, 6)); dis[:, 3:6] = TO_AA_THETAS[:, None] * _axes(rng, n)
    b = R.Batch(w, n, device=0, max_rigid=0)
    if specialized:
        b.specialize()
    b.set_state(dis, np.zeros_like(dis)); b.update_init(); b.update(1)
    assert b.status() == 0
    got = b.get_state()[0]
    b.close()
    ref = np.zeros_like(got)
    for i in range(n):
        o = oracle_cls(w.model); o.set_state(dis[i], np.zeros(6)); o.update_init(); o.update()
        ref[i] = o.get_state()[0]; o.close()
    rot = R.scenarios._rot_aa_batch
    assert (np.linalg.norm(got[:, 3:6], axis=1) <= np.pi).all()          # theta = 4.0 comes back as 2 pi - 4.0 on the opposite axis
    assert (got[-1, 3:6] * dis[-1, 3:6]).sum() < 0 and abs(np.linalg.norm(got[-1, 3:6]) - (2 * np.pi - 4.0)) < 1e-12
    return (np.abs(rot(got[:, 3:6]) - rot(ref[:, 3:6])).max(axis=(1, 2)), np.abs(rot(got[:, 3:6]) - rot(dis[:, 3:6])).max(axis=(1, 2)),
            to_aa_bound(TO_AA_THETAS))


def run_variant(R, sc, variant, chunks=1, each=None):
    """update_init and sc["steps"] steps in `chunks` launches under a kernel variant; each( b ) after every launch.  -> get_state()"""
    n = sc["dis"].shape[0]
    b = R.Batch(sc["world"], n, device=0, max_rigid=sc["max_rigid"])
    if variant == "table":          # a table whose rows are the model's own values: bit for bit what no table gives
        for k in ip.PER_LINK:
            b.set_param(k, np.tile(ip.model_values(sc["world"], k), (n, 1)))
        assert b.has_params()
    if variant == "two_per_wave":
        b.set_instances_per_wave(2)
    if variant in ("specialized", "two_per_wave"):
        b.specialize()
        assert b.instances_per_wave() == (2 if variant == "two_per_wave" else 1)
    b.set_state(sc["dis"], sc["vel"]); b.update_init()
    for _ in range(chunks):
        b.update(sc["steps"] // chunks)
        if each is not None:
            each(b)
    assert b.status() == 0
    out = b.get_state()
    b.close()
    return out


def device_momentum_drift(R, sc):
    """the drift of the world angular momentum R ( I w ) of the tumbling box over its steps, read after every step through
    update_links (attitude and link-frame twist of link 0), per instance"""
    m = sc["world"].model.contents
    n = sc["dis"].shape[0]
    b = R.Batch(sc["world"], n, device=0, max_rigid=0)
    b.set_state(sc["dis"], sc["vel"]); b.update_init()
    L = np.zeros((n, sc["steps"] + 1, 3))
    for t in range(sc["steps"] + 1):
        if t:
            b.update(1)
        b.update_links(lc.POSE | lc.VEL)
        g = b.get_links()
        L[:, t] = angular_momentum(m, g["R"][:, 0], g["v"][:, 0])
    assert b.status() == 0
    b.close()
    return drift(L)
