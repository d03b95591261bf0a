"""Helpers of the per-instance physical parameter tests (rkfdBatchSetParam; tests/test_param_abi.py, test_emu_params.py,
test_gpu_params.py): a copy of a world's model with some arrays replaced, and randomised parameters for a batch.

The tests' yardstick is the MODEL COPY: instance i of a batch that carries parameters P_i must give, bit for bit, what a plain
batch built on model_with(world, P_i) gives, and the unchanged oracle runs on that copy."""
import ctypes as C

import numpy as np

# key order of include/rkfd_hip.h (RKFD_PAR_*); the names are the binding's
NAMES = ("mass", "com", "inertia", "stiff", "visc", "coulomb", "sfric", "ci_sf", "ci_kf", "ci_k", "ci_l", "ci_e", "ci_v")
PER_LINK = {"mass": 1, "com": 3, "inertia": 9, "stiff": 1, "visc": 1, "coulomb": 1, "sfric": 1}


def width(model, name):
    """doubles per instance of a parameter, model space"""
    return model.nlink * PER_LINK[name] if name in PER_LINK else model.nci


def model_values(world, name):
    m = world.model.contents
    return m.arr(name, width(m, name))


class ModelCopy:
    """what Batch, EmuBatch and the oracle take for a world: an object with .model (a pointer to an RkfdModel).  The structure is
    a copy of the world's; the overridden arrays point at numpy buffers this object keeps alive, everything else at the
    world's own arrays (so the world is kept alive too)."""

    def __init__(self, world, overrides):
        self.world = world
        src = world.model.contents
        self._struct = type(src)()
        C.memmove(C.byref(self._struct), C.byref(src), C.sizeof(src))
        self._keep = {}
        for name, val in overrides.items():
            assert name in NAMES, name
            a = np.ascontiguousarray(val, dtype=np.float64).reshape(width(src, name)).copy()
            self._keep[name] = a
            setattr(self._struct, name, a.ctypes.data_as(C.POINTER(C.c_double)))
        self.model = C.pointer(self._struct)


def model_with(world, overrides):
    return ModelCopy(world, overrides)


def randomised(world, B, seed):
    """per-instance parameters {name: (B, width)} for every key: masses x U(0.7, 1.3) with the inertia scaled along, centres of mass
    shifted by up to 5 mm per axis, joint friction (stiff, visc, coulomb, sfric) and contact-info values x U(0.5, 1.5) - the two
    friction coefficients of a contact info by ONE factor, so that kinetic friction stays below static friction as in every
    contact-info file.  EVERY link and contact info is randomised, the contact infos in contact among them.  The links the device
    merges into their parents (fixed joints: the soles and hands of the humanoid) are massless in the shipped models, and a factor
    leaves them so: each of them gets a payload of its own instead, a mass U(0.1, 0.3) kg with a diagonal inertia U(1, 3)e-4 kg m^2
    at its shifted centre of mass, so that the composite body of the foot differs from instance to instance through the merge.
    (mass 0 -> positive is allowed; positive -> 0 is what rkfdBatchSetParam refuses.)"""
    m = world.model.contents
    rng = np.random.default_rng(seed)
    NL, nci = m.nlink, m.nci
    out = {}
    s = rng.uniform(0.7, 1.3, (B, NL))
    out["mass"] = model_values(world, "mass")[None, :] * s
    out["inertia"] = (model_values(world, "inertia").reshape(1, NL, 9) * s[:, :, None]).reshape(B, 9 * NL)
    inertia = out["inertia"].reshape(B, NL, 9)
    for i in merged_links(world):
        if model_values(world, "mass")[i] == 0.0:
            out["mass"][:, i] = rng.uniform(0.1, 0.3, B)
            inertia[:, i, :] = 0.0
            for d in (0, 4, 8):
                inertia[:, i, d] = rng.uniform(1e-4, 3e-4, B)
    out["inertia"] = inertia.reshape(B, 9 * NL)
    out["com"] = model_values(world, "com")[None, :] + rng.uniform(-0.005, 0.005, (B, 3 * NL))
    for name in ("stiff", "visc", "coulomb", "sfric"):
        out[name] = model_values(world, name)[None, :] * rng.uniform(0.5, 1.5, (B, NL))
    f = rng.uniform(0.5, 1.5, (B, nci))
    out["ci_sf"] = model_values(world, "ci_sf")[None, :] * f
    out["ci_kf"] = model_values(world, "ci_kf")[None, :] * f
    for name in ("ci_k", "ci_l", "ci_e", "ci_v"):
        out[name] = model_values(world, name)[None, :] * rng.uniform(0.5, 1.5, (B, nci))
    return out


def of_instance(params, i):
    return {k: v[i] for k, v in params.items()}


def merged_links(world):
    """model links the device folds into a parent: fixed joints below a parent (rkfd_devmodel.cpp)"""
    m = world.model.contents
    par, jt = m.arr("parent", m.nlink), m.arr("jtype", m.nlink)
    return [i for i in range(m.nlink) if jt[i] == 0 and par[i] >= 0]
