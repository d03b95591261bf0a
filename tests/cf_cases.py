"""Helpers of the contact read-out tests (rkfdBatchUpdateContactForces; tests/test_emu_cf.py, tests/test_gpu_cf.py,
tools/cf_parity.py): the worlds, the random inputs, the references and the bound.  No device code in here.

point, wrench, count - a plain numpy sum over eom_cases.Tables (cand_pair -> pair_shape -> shape_link, cand_side, cand_vert -> verts)
and refmath.fk: x_j = p_own + R_own v_j; an active candidate gives ( +f_j, ( x_j - p_own ) x f_j ) to the owner and
( -f_j, ( x_j - p_other ) x -f_j ) to the other link of its pair (the convention of eom_cases.contact_forces).

genf, reference A - the oracle's unit-rate columns (jac_cases.reference): sum_j J( own_j, v_j )' f_j - J( other_j, x_j in the other's
frame )' f_j over the active candidates, with J the linear rows of the site Jacobians.  x_j in the other's frame is R_o' ( x_j - p_o )
on the oracle's frames, which is that point only for orthonormal frames; on frames written with ten digits (the raw random and limit
trees) the device's definition is compared instead, reference A': sum_l J_l[0:3]' F_l + J_l[3:6]' N_l with J_l the oracle's unit-rate
site Jacobian of ( link l, its origin ) and ( F_l, N_l ) the numpy wrench - the text of include/rkfd_hip.h.
genf, reference B - independent mechanics: refmath.rnea( q, 0, 0 ) - refmath.rnea( q, 0, 0, fext ) with eom_cases.contact_forces, every
breakable joint taken as broken (a breakable float joint gets its six entries like any float joint); worlds with orthonormal frames.

Random inputs of the device form: forces uniform in +-100 N, about half the candidates active, the entries of the inactive ones NaN.

Bound: links_cases.TOL = 1e-12 max( 1, |value|_inf of the array ).  A wrench entry is a sum over at most ncand (764) products of a
position good to depth x a few ulp and a force; genf one more sum over at most 96 links of such entries times Jacobian columns good
to the same: n eps relative to the largest entry, 1e-13 at most."""
import ctypes as C
import os
import subprocess

import numpy as np

from emu import ROOT, HERE
import dyn_cases as dc
import eom_cases as ec
import jac_cases as jc
import links_cases as lc
import refmath as rm

POINT, WRENCH, GENF = 1, 2, 4
ALL = 7
TOL = lc.TOL
KEYS = ("point", "wrench", "count", "genf")
NEED = {"point": POINT, "wrench": WRENCH, "count": WRENCH, "genf": GENF}
WORLDS = ["config4", "config5", "humanoid30_shell", "arm_fold", "arm_spher_contact", "stacked_boxes", "wall", "no_candidates"]
LIMIT_TREES = jc.LIMIT_TREES
_emu = None


def emu_lib():
    global _emu
    if _emu is None:
        path = os.path.join(HERE, "librkfd_emu_cf.so")
        if not os.path.exists(path):
            subprocess.run(["make", "-C", ROOT, "emu"], check=True, stdout=subprocess.DEVNULL)
        L = C.CDLL(path)
        L.rkfd_emu_cf.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
        _emu = L
    return _emu


class Cand:
    """the candidate tables in model space: own, other [nc], vert [nc, 3]"""

    def __init__(self, own, other, vert):
        self.own = np.ascontiguousarray(own, dtype=np.int32); self.other = np.ascontiguousarray(other, dtype=np.int32)
        self.vert = np.ascontiguousarray(vert, dtype=np.float64).reshape(-1, 3)
        self.n = self.own.size


def model_cand(world):
    tb = ec.Tables(world.model.contents)
    return Cand(tb.own, tb.other, tb.vert)


def synthetic_cand(world, n, seed):
    """n seeded candidates on any two different links of the world, vertices within +-0.2 m"""
    m = world.model.contents
    rng = np.random.default_rng(0xCF00 + seed)
    own = rng.integers(0, m.nlink, n)
    other = (own + rng.integers(1, m.nlink, n)) % m.nlink
    return Cand(own, other, rng.uniform(-0.2, 0.2, (n, 3)))


def emu_cf(world, dis, active, f, flags=ALL, cand=None, waves=None):
    """the contact read-out's device code under the lane emulator: ALL four arrays, NaN-prefilled (count: -1), so that what the flags
    do not select can be seen untouched; cand: explicit candidate tables (None: the model's); waves: a list that receives the
    instances per workgroup the C ABI would launch with"""
    m = world.model.contents
    B = dis.shape[0]
    nc = m.ncand if cand is None else cand.n
    dis = np.ascontiguousarray(dis, dtype=np.float64)
    active = np.ascontiguousarray(active, dtype=np.int32).reshape(B, nc); f = np.ascontiguousarray(f, dtype=np.float64).reshape(B, nc, 3)
    out = {"point": np.full((B, nc, 3), np.nan), "wrench": np.full((B, m.nlink, 6), np.nan), "count": np.full((B, m.nlink), -1, dtype=np.int32),
           "genf": np.full((B, m.ndof), np.nan)}
    p = lambda a: None if a is None else a.ctypes.data
    tabs = [0, None, None, None] if cand is None else [cand.n, p(cand.own), p(cand.other), p(cand.vert)]
    r = emu_lib().rkfd_emu_cf(C.cast(world.model, C.c_void_p), B, p(dis), p(active), p(f), flags, *tabs, *[p(out[k]) for k in KEYS])
    assert r >= 0, r
    if waves is not None:
        waves.append(r)
    return out


def random_inputs(B, nc, seed):
    """(active [B, nc] int32, f [B, nc, 3]): forces uniform in +-100 N, about half the candidates active, inactive entries NaN"""
    rng = np.random.default_rng(0xCF10 + seed)
    active = (rng.uniform(size=(B, nc)) < 0.5).astype(np.int32)
    f = rng.uniform(-100.0, 100.0, (B, nc, 3))
    f[active == 0] = np.nan
    return active, f


# ---- references ---------------------------------------------------------------------------------------------------------------------
def numpy_sum(world, cand, dis, active, f):
    """point, wrench, count [B, ..] by a plain sum over the candidate tables on refmath's forward kinematics"""
    m = world.model.contents
    md = rm.model_arrays(m)
    B = dis.shape[0]
    out = {"point": np.zeros((B, cand.n, 3)), "wrench": np.zeros((B, m.nlink, 6)), "count": np.zeros((B, m.nlink), dtype=np.int32)}
    for i in range(B):
        Rw, pw, _ = rm.fk(md, dis[i])
        for j in range(cand.n):
            o, t = cand.own[j], cand.other[j]
            x = pw[o] + Rw[o] @ cand.vert[j]
            out["point"][i, j] = x
            if active[i, j]:
                fj = f[i, j]
                out["wrench"][i, o, :3] += fj; out["wrench"][i, o, 3:] += np.cross(x - pw[o], fj)
                out["wrench"][i, t, :3] -= fj; out["wrench"][i, t, 3:] -= np.cross(x - pw[t], fj)
                out["count"][i, o] += 1; out["count"][i, t] += 1
    return out


def reference_a(R, oracle_cls, world, cand, dis, active, f, ortho):
    """genf [B, ndof] from the oracle's unit-rate site Jacobians: per candidate on orthonormal frames, else per link (A')"""
    m = world.model.contents
    B = dis.shape[0]
    out = np.zeros((B, m.ndof))
    ones = np.ones((1, m.nlink), dtype=np.int32)          # the columns of a breakable float joint, broken or not
    for i in range(B):
        on = np.flatnonzero(active[i])
        if on.size == 0:
            continue
        if ortho:
            _, fr = jc.reference(R, oracle_cls, world, dis[i:i + 1], [0], None, broken=ones, with_frames=True)
            Ro, po = fr["R"][0], fr["p"][0]
            x = po[cand.own[on]] + np.einsum("jab,jb->ja", Ro[cand.own[on]], cand.vert[on])
            xo = np.einsum("jba,jb->ja", Ro[cand.other[on]], x - po[cand.other[on]])
            links = np.concatenate([cand.own[on], cand.other[on]]); pts = np.concatenate([cand.vert[on], xo])
            J = jc.reference(R, oracle_cls, world, dis[i:i + 1], links, pts, broken=ones)["J"][0]
            ff = np.concatenate([f[i, on], -f[i, on]])
            out[i] = np.einsum("skc,sk->c", J[:, :3], ff)
        else:
            W = numpy_sum(world, cand, dis[i:i + 1], active[i:i + 1], f[i:i + 1])
            links = np.flatnonzero(W["count"][0])
            J = jc.reference(R, oracle_cls, world, dis[i:i + 1], links, None, broken=ones)["J"][0]
            out[i] = np.einsum("skc,sk->c", J, W["wrench"][0][links])
    return out


def reference_b(world, cand, dis, active, f):
    """genf [B, ndof] = rnea( q, 0, 0 ) - rnea( q, 0, 0, fext )"""
    m = world.model.contents
    md = rm.model_arrays(m)
    ones, z = np.ones(m.nlink, dtype=int), np.zeros(m.ndof)
    out = np.zeros((dis.shape[0], m.ndof))
    for i in range(dis.shape[0]):
        fext = ec.contact_forces(md, cand, dis[i], active[i], np.nan_to_num(f[i]))
        out[i] = rm.rnea(md, dis[i], z, z, broken=ones) - rm.rnea(md, dis[i], z, z, fext=fext, broken=ones)
    return out


def check(got, ref, what, keys=KEYS):
    keys = [k for k in keys if k in got and k in ref]
    if "count" in keys:
        assert np.array_equal(got["count"], ref["count"]), what
    return lc.check(got, ref, what, keys=[k for k in keys if k != "count"])


def check_properties(world, cand, dis, active, f, got, rerun, what):
    """on every instance: finite despite the NaN poison; wrench and genf exactly linear in a rescaling of f by 2; exact zeros where no
    ancestor is touched; action and reaction cancel.  rerun( f2 ) -> the read-out of the same inputs with the forces f2"""
    m = world.model.contents
    for k in ("point", "wrench", "genf"):
        assert np.isfinite(got[k]).all(), (what, k)
    twice = rerun(2.0 * f)
    assert np.array_equal(twice["wrench"], 2.0 * got["wrench"]) and np.array_equal(twice["genf"], 2.0 * got["genf"]), what
    assert np.array_equal(twice["count"], got["count"]) and np.array_equal(twice["point"], got["point"]), what
    mv = jc.moves(m)
    md = rm.model_arrays(m)
    for i in range(dis.shape[0]):
        touched = got["count"][i] > 0
        may = mv[touched].any(axis=0) if touched.any() else np.zeros(m.ndof, dtype=bool)
        assert (got["genf"][i][~may] == 0.0).all(), (what, i)
        assert (got["wrench"][i][~touched] == 0.0).all(), (what, i)
        _, pw, _ = rm.fk(md, dis[i])
        F, N = got["wrench"][i][:, :3], got["wrench"][i][:, 3:]
        N0 = N + np.cross(pw, F)
        assert np.abs(F.sum(axis=0)).max() <= TOL * max(1.0, np.abs(F).max()), (what, i, F.sum(axis=0))
        assert np.abs(N0.sum(axis=0)).max() <= TOL * max(1.0, np.abs(N0).max()), (what, i, N0.sum(axis=0))


def check_world(R, oracle_cls, c, got, what, idx=None):
    """point / wrench / count against the numpy sum, genf against A (A' on raw frames) and - orthonormal frames - B, on the instances
    idx (all when None).  -> the deviations"""
    sel = np.arange(c["dis"].shape[0]) if idx is None else np.asarray(idx)
    sub = {k: v[sel] for k, v in got.items()}
    w, cand, dis, act, f = c["world"], c["cand"], c["dis"][sel], c["active"][sel], c["f"][sel]
    dev = {"sum": check(sub, numpy_sum(w, cand, dis, act, f), what + " [numpy sum]")}
    dev["A"] = check(sub, {"genf": reference_a(R, oracle_cls, w, cand, dis, act, f, c["ortho"])}, what + (" [A]" if c["ortho"] else " [A']"))
    if c["ortho"]:
        dev["B"] = check(sub, {"genf": reference_b(w, cand, dis, act, f)}, what + " [B]")
    return dev


# ---- the worlds ---------------------------------------------------------------------------------------------------------------------
def _case(world, B, seed, cand=None, ortho=True):
    synthetic = cand is not None
    cand = cand if synthetic else model_cand(world)
    dis, _ = lc.states(world, B, 0xCF20 + seed)
    act, f = random_inputs(B, cand.n, seed)
    return dict(world=world, dis=dis, cand=cand, active=act, f=f, ortho=ortho, synthetic=synthetic)


def cases(R, tmp_path, B=3):
    """the model-file worlds of WORLDS with the model's own candidates, seeded states and the random inputs"""
    S = R.scenarios
    M = S.MODELS
    out = {}
    out["config4"] = _case(S.config4(batch=1)["world"], B, 1)                   # 32 candidates: fewer than a wavefront
    out["config5"] = _case(S.config5(batch=1)["world"], B, 2)                   # five chains, body on body
    out["humanoid30_shell"] = _case(S.config4_shell(batch=1)["world"], B, 3)    # 764 candidates: eleven rounds of 64 and a remainder of 60
    out["arm_fold"] = _case(S.arm_fold(batch=1)["world"], B, 4)                 # owner and other link in the same chain
    out["arm_spher_contact"] = _case(S.arm_spher(batch=1, contact=True)["world"], B, 5)
    out["stacked_boxes"] = _case(ec._stack(R, tmp_path).world, B, 6)
    out["wall"] = _case(lc._reg(R, ["wall.ztk", "box.ztk", "floor.ztk"]), B, 7)  # breakable float joints
    w = R.World(solver=R.SOLVER_MLCP); w.reg_file(os.path.join(M, "arm_revroot.ztk"))
    out["no_candidates"] = _case(w, B, 8)
    return out


def tree_cases(R, tmp_path, ortho, ncand=40):
    """synthetic candidates on the limit trees and the ten random trees: raw frames (A') or orthonormalised (A and B)"""
    out = {}
    src = dict(dc.limit_tree_cases(R, tmp_path, ortho)); src.update(dc.random_tree_cases(R, tmp_path, ortho))
    for k, (name, c) in enumerate(src.items()):
        w = c["world"]
        if w.model.contents.nlink < 2:
            continue
        out[name] = _case(w, 2, 20 + k, cand=synthetic_cand(w, ncand, k), ortho=ortho)
    return out


def tile(c, B, seed=0xCF3):
    """B instances of a case: its seeded ones, then further seeded draws"""
    n = c["dis"].shape[0]
    d2, _ = lc.states(c["world"], B, seed + B)
    a2, f2 = random_inputs(B, c["cand"].n, seed + B)
    k = min(n, B)
    d2[:k] = c["dis"][:k]; a2[:k] = c["active"][:k]; f2[:k] = c["f"][:k]
    return dict(c, dis=d2, active=a2, f=f2)


class DevArray:
    """a numpy array copied to device memory of the library's own HIP runtime (hipMalloc through the library's handle), handed to
    Batch.update_contact_forces through __cuda_array_interface__: the tests' process keeps torch's runtime out (tests/test_gpu_dyn.py)"""

    def __init__(self, R, a):
        self._L = R.lib()
        a = np.ascontiguousarray(a)
        self._p = C.c_void_p()
        self._L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self._L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self._L.hipFree.argtypes = [C.c_void_p]
        assert self._L.hipMalloc(C.byref(self._p), max(a.nbytes, 8)) == 0
        if a.nbytes:
            assert self._L.hipMemcpy(self._p, a.ctypes.data, a.nbytes, 1) == 0          # hipMemcpyHostToDevice
        self.__cuda_array_interface__ = dict(shape=a.shape, typestr=a.dtype.str, data=(self._p.value, False), version=2, strides=None)

    def free(self):
        if self._p:
            self._L.hipFree(self._p); self._p = C.c_void_p()
