"""ctypes binding of librkfd_amd.so (include/rkfd_hip.h, include/roki_fd_amd.h)."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librkfd_amd.so")

JOINT_FIXED, JOINT_REVOL, JOINT_PRISM, JOINT_FLOAT = 0, 1, 2, 3
JOINT_SPHER, JOINT_BRFLOAT = 4, 5
SOLVER_VERT, SOLVER_MLCP, SOLVER_VOLUME = 0, 1, 2
CONTACT_RIGID, CONTACT_ELASTIC = 0, 1
SF, KF = 0, 1

_pi = C.POINTER(C.c_int)
_pd = C.POINTER(C.c_double)


class RkfdError(RuntimeError):
    pass


class RkfdModel(C.Structure):
    """Mirror of rkfdModel (include/rkfd_model.h); field order must match."""
    _fields_ = [
        ("nlink", C.c_int), ("ndof", C.c_int), ("nchain", C.c_int),
        ("parent", _pi), ("jtype", _pi), ("dofoff", _pi), ("chain", _pi),
        ("org", _pd), ("mass", _pd), ("com", _pd), ("inertia", _pd),
        ("stiff", _pd), ("visc", _pd), ("coulomb", _pd), ("sfric", _pd),
        ("mtype", _pi),
        ("mot_k", _pd), ("mot_admit", _pd), ("mot_vmax", _pd), ("mot_vmin", _pd), ("mot_gear", _pd), ("mot_inertia", _pd),
        ("nshape", C.c_int),
        ("shape_link", _pi), ("shape_voff", _pi), ("shape_foff", _pi),
        ("verts", _pd), ("planes", _pd),
        ("shape_slide_mode", _pi), ("shape_slide_vel", _pd), ("shape_slide_axis", _pd),
        ("npair", C.c_int),
        ("pair_shape", _pi), ("pair_ci", _pi),
        ("nci", C.c_int),
        ("ci_type", _pi),
        ("ci_sf", _pd), ("ci_kf", _pd), ("ci_k", _pd), ("ci_l", _pd), ("ci_e", _pd), ("ci_v", _pd),
        ("ncand", C.c_int),
        ("cand_pair", _pi), ("cand_side", _pi), ("cand_vert", _pi),
        ("dt", C.c_double), ("friction_weight", C.c_double),
        ("max_iter", C.c_int), ("solver", C.c_int), ("pyramid", C.c_int),
        ("brk_f", _pd), ("brk_t", _pd),
    ]

    def arr(self, name, n, dtype=None):
        p = getattr(self, name)
        if n == 0:
            return np.zeros(0, dtype=dtype or (np.int32 if isinstance(p, _pi) else np.float64))
        return np.ctypeslib.as_array(p, shape=(n,)).copy()


_lib = None


def lib():
    """Loads librkfd_amd.so; raises when it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RkfdError(f"{LIB_PATH} is missing: run `make` (or __graft_entry__.build()) first")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.rkfdWorldCreate.restype = vp
    L.rkfdWorldFree.argtypes = [vp]
    L.rkfdWorldRegFile.argtypes = [vp, C.c_char_p]
    L.rkfdWorldSetContactInfo.argtypes = [vp, C.c_char_p]
    L.rkfdWorldPairChainUnreg.argtypes = [vp, C.c_int]
    L.rkfdWorldSetPrp.argtypes = [vp, C.c_double, C.c_double, C.c_int, C.c_int]
    L.rkfdWorldSetPyramid.argtypes = [vp, C.c_int]
    L.rkfdWorldSetSlide.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, vp]; L.rkfdWorldSetSlide.restype = C.c_int
    L.rkfdWorldModel.argtypes = [vp]
    L.rkfdWorldModel.restype = C.POINTER(RkfdModel)
    L.rkfdWorldChainDofOffset.argtypes = [vp, C.c_int]
    L.rkfdWorldChainLinkOffset.argtypes = [vp, C.c_int]
    L.rkfdWorldChainInitDis.argtypes = [vp, C.c_int, _pd]
    L.rkfdWorldWriteZTK.argtypes = [vp, C.c_int, C.c_char_p, _pd]
    L.rkfdHipLastError.restype = C.c_char_p
    L.rkfdBatchCreate.argtypes = [C.POINTER(RkfdModel), C.c_int, C.c_int, C.c_int]
    L.rkfdBatchCreate.restype = vp
    L.rkfdBatchDestroy.argtypes = [vp]
    L.rkfdSpecializeCompile.argtypes = [C.POINTER(RkfdModel), C.c_int]
    for f in ("rkfdBatchSize", "rkfdBatchDof", "rkfdBatchLdsBytes", "rkfdBatchResidency", "rkfdBatchSpecialize"):
        getattr(L, f).argtypes = [vp]
    L.rkfdBatchSetState.argtypes = [vp, vp, vp]
    L.rkfdBatchGetState.argtypes = [vp, vp, vp, vp]
    L.rkfdBatchSetMotorInput.argtypes = [vp, vp]
    L.rkfdBatchGetContact.argtypes = [vp, vp, vp, vp, vp]
    L.rkfdBatchSetContact.argtypes = [vp, vp, vp, vp]
    L.rkfdBatchGetPivot.argtypes = [vp, vp, vp]
    L.rkfdBatchSetPivot.argtypes = [vp, vp, vp]
    L.rkfdBatchGetBroken.argtypes = [vp, vp]; L.rkfdBatchSetBroken.argtypes = [vp, vp]
    L.rkfdBatchSetInstancesPerWave.argtypes = [vp, C.c_int]; L.rkfdBatchInstancesPerWave.argtypes = [vp]
    L.rkfdBatchSetStepsPerLaunch.argtypes = [vp, C.c_int]
    L.rkfdBatchTuneInstancesPerWave.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
    L.rkfdSpecializeCompileW.argtypes = [C.POINTER(RkfdModel), C.c_int, C.c_int]
    L.rkfdSpecializeCompileP.argtypes = [C.POINTER(RkfdModel), C.c_int, C.c_int, C.c_int]
    L.rkfdBatchUpdateInit.argtypes = [vp, vp]
    L.rkfdBatchUpdate.argtypes = [vp, C.c_int, vp]
    L.rkfdBatchEval.argtypes = [vp, C.c_int, vp]
    L.rkfdBatchUpdateControlled.argtypes = [vp, C.c_int, vp, vp]; L.rkfdBatchUpdateControlledDev.argtypes = [vp, C.c_int, vp, vp]
    L.rkfdNodeUpdateControlled.argtypes = [vp, C.c_int, vp]
    L.rkfdLdsBytesFor.argtypes = [C.POINTER(RkfdModel), C.c_int]
    L.rkfdBatchParamWidth.argtypes = [vp, C.c_int]; L.rkfdBatchSetParam.argtypes = [vp, C.c_int, vp]; L.rkfdBatchGetParam.argtypes = [vp, C.c_int, vp]
    L.rkfdBatchClearParams.argtypes = [vp]; L.rkfdBatchHasParams.argtypes = [vp]
    L.rkfdNodeSetParam.argtypes = [vp, C.c_int, vp]; L.rkfdNodeClearParams.argtypes = [vp]
    L.rkfdBatchStatus.argtypes = [vp, vp]
    L.rkfdBatchContactStats.argtypes = [vp, C.c_int, _pd, _pd, C.POINTER(C.c_longlong)]
    L.rkfdBatchSnapshot.argtypes = [vp]; L.rkfdBatchRestore.argtypes = [vp, vp]
    L.rkfdBatchBankReserve.argtypes = [vp, C.c_int]; L.rkfdBatchBankSize.argtypes = [vp]
    L.rkfdBatchBankStore.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.rkfdBatchReset.argtypes = [vp, vp, vp]; L.rkfdBatchResetDev.argtypes = [vp, vp, vp]
    L.rkfdNodeBankReserve.argtypes = [vp, C.c_int]; L.rkfdNodeBankStore.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.rkfdNodeReset.argtypes = [vp, vp]
    L.rkfdBatchProfile.argtypes = [vp, C.c_int, vp]
    L.rkfdBatchSetSplit.argtypes = [vp, C.c_int]; L.rkfdBatchJoin.argtypes = [vp, vp]
    L.rkfdBatchTimeLaunches.argtypes = [vp, C.c_int]; L.rkfdBatchLaunchTiming.argtypes = [vp, vp, vp]
    for f in ("rkfdBatchDevDis", "rkfdBatchDevVel", "rkfdBatchDevAcc"):
        getattr(L, f).argtypes = [vp]
        getattr(L, f).restype = vp
    L.rkfdBatchLinkNum.argtypes = [vp]; L.rkfdBatchChainNum.argtypes = [vp]
    L.rkfdBatchUpdateLinks.argtypes = [vp, C.c_int, vp]; L.rkfdBatchGetLinks.argtypes = [vp, vp, vp, vp, vp, vp]
    L.rkfdNodeGetLinks.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    for f in ("rkfdBatchDevLinkAtt", "rkfdBatchDevLinkPos", "rkfdBatchDevLinkVel", "rkfdBatchDevCom", "rkfdBatchDevComVel"):
        getattr(L, f).argtypes = [vp]
        getattr(L, f).restype = vp
    L.rkfdBatchSetJacobianSites.argtypes = [vp, C.c_int, vp, vp]; L.rkfdBatchJacobianSiteNum.argtypes = [vp]
    L.rkfdBatchUpdateJacobians.argtypes = [vp, C.c_int, vp]; L.rkfdBatchGetJacobians.argtypes = [vp, vp, vp]
    L.rkfdNodeSetJacobianSites.argtypes = [vp, C.c_int, vp, vp]; L.rkfdNodeGetJacobians.argtypes = [vp, C.c_int, vp, vp]
    for f in ("rkfdBatchDevJacobian", "rkfdBatchDevComJacobian"):
        getattr(L, f).argtypes = [vp]
        getattr(L, f).restype = vp
    L.rkfdBatchUpdateDynamics.argtypes = [vp, C.c_int, vp]; L.rkfdBatchGetDynamics.argtypes = [vp, vp, vp, vp]
    L.rkfdNodeGetDynamics.argtypes = [vp, C.c_int, vp, vp, vp]
    for f in ("rkfdBatchDevMassMatrix", "rkfdBatchDevBias", "rkfdBatchDevGravity"):
        getattr(L, f).argtypes = [vp]
        getattr(L, f).restype = vp
    L.rkfdBatchUpdateContactForces.argtypes = [vp, C.c_int, vp]; L.rkfdBatchUpdateContactForcesDev.argtypes = [vp, C.c_int, vp, vp, vp]
    L.rkfdBatchGetContactForces.argtypes = [vp, vp, vp, vp, vp]; L.rkfdNodeGetContactForces.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    for f in _CF_DEV:
        getattr(L, f).argtypes = [vp]
        getattr(L, f).restype = vp
    L.rkfdNodeCreate.argtypes = [C.POINTER(RkfdModel), C.c_int, C.c_int, C.c_int, vp]; L.rkfdNodeCreate.restype = vp
    L.rkfdNodeDestroy.argtypes = [vp]
    for f in ("rkfdNodeDevices", "rkfdNodeSize", "rkfdNodeSpecialize", "rkfdNodeUpdateInit", "rkfdNodeSnapshot", "rkfdNodeRestore", "rkfdNodeStatus"):
        getattr(L, f).argtypes = [vp]
    L.rkfdNodeShard.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.rkfdNodeBatch.argtypes = [vp, C.c_int]; L.rkfdNodeBatch.restype = vp
    L.rkfdNodeSetState.argtypes = [vp, vp, vp]; L.rkfdNodeSetMotorInput.argtypes = [vp, vp]
    L.rkfdNodeGetState.argtypes = [vp, vp, vp, vp]
    L.rkfdNodeSetSplit.argtypes = [vp, C.c_int]; L.rkfdNodeUpdate.argtypes = [vp, C.c_int]
    L.rkfdNodeSetStepsPerLaunch.argtypes = [vp, C.c_int]; L.rkfdNodeTuneInstancesPerWave.argtypes = [vp, C.c_int]
    L.rkfdNodeGather.argtypes = [vp, vp, vp]
    L.rkfdNodeGatherDev.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]; L.rkfdNodeGatherDev.restype = vp
    _lib = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class World:
    """The rkFD world builder: chains registered from ZTK files + contact-info table.
    Mirrors rkFDCreate / rkFDChainRegFile / rkFDContactInfoScanFile / rkFDSetSolver /
    rkFDPrpSet* (reference src/rkfd_sim.c:32-54,224-273; include/roki_fd/rkfd_sim.h:89-93)."""

    def __init__(self, solver=SOLVER_VERT, dt=0.001, friction_weight=100.0, max_iter=10):
        self._L = lib()
        self._w = self._L.rkfdWorldCreate()
        if not self._w:
            raise RkfdError("rkfdWorldCreate failed")
        self.nchain = 0
        self.set_prp(dt, friction_weight, max_iter, solver)

    def close(self):
        if self._w:
            self._L.rkfdWorldFree(self._w)
            self._w = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_slide(self, chain, shape, mode, vel=0.0, axis=(0.0, 1.0, 0.0)):
        """rkFDCDCellSetSlideMode / Vel / Axis on shape number `shape` of a chain (its order in the ZTK file)"""
        ax = (C.c_double * 3)(*axis)
        if self._L.rkfdWorldSetSlide(self._w, int(chain), int(shape), int(bool(mode)), float(vel), ax) != 0:
            raise RkfdError("no such chain / shape")

    def set_pyramid(self, pyramid):
        """rkFDPrpSetPyramid: faces of the Vert plugin's friction pyramid (default 8)"""
        self._L.rkfdWorldSetPyramid(self._w, int(pyramid))

    def set_prp(self, dt, friction_weight, max_iter, solver):
        self._L.rkfdWorldSetPrp(self._w, dt, friction_weight, max_iter, solver)

    def reg_file(self, path):
        cid = self._L.rkfdWorldRegFile(self._w, os.fspath(path).encode())
        if cid < 0:
            raise RkfdError(f"cannot register chain from {path}")
        self.nchain = cid + 1
        return cid

    def contact_info(self, path):
        if self._L.rkfdWorldSetContactInfo(self._w, os.fspath(path).encode()) != 0:
            raise RkfdError(f"cannot read contact info from {path}")

    def pair_chain_unreg(self, chain):
        self._L.rkfdWorldPairChainUnreg(self._w, chain)

    @property
    def model(self):
        p = self._L.rkfdWorldModel(self._w)
        if not p:
            raise RkfdError("rkfdWorldModel failed")
        return p

    def dof_offset(self, chain):
        return self._L.rkfdWorldChainDofOffset(self._w, chain)

    def link_offset(self, chain):
        return self._L.rkfdWorldChainLinkOffset(self._w, chain)

    def init_dis(self, chain):
        buf = np.zeros(64, dtype=np.float64)
        n = self._L.rkfdWorldChainInitDis(self._w, chain, buf.ctypes.data_as(_pd))
        return buf[:n].copy()


# task-space read-out (include/rkfd_hip.h: RKFD_LINKS_*): what update_links computes and get_links returns
LINKS_POSE, LINKS_VEL, LINKS_COM = 1, 2, 4
LINKS_ALL = LINKS_POSE | LINKS_VEL | LINKS_COM
_LINKS_KEYS = (("R", LINKS_POSE), ("p", LINKS_POSE), ("v", LINKS_VEL), ("com", LINKS_COM), ("comvel", LINKS_COM))


def _links_arrays(n, nl, nc, flags):
    """host arrays of a read-out over n instances: {name: array} of the quantities `flags` selects"""
    shapes = {"R": (n, nl, 3, 3), "p": (n, nl, 3), "v": (n, nl, 6), "com": (n, nc, 3), "comvel": (n, nc, 3)}
    return {k: np.empty(shapes[k]) for k, f in _LINKS_KEYS if flags & f}


# task-space Jacobians (include/rkfd_hip.h: RKFD_JAC_*): what update_jacobians computes and get_jacobians returns
JAC_SITES, JAC_COM = 1, 2
JAC_ALL = JAC_SITES | JAC_COM
_JAC_KEYS = (("J", JAC_SITES), ("Jcom", JAC_COM))


def _jac_sites(links, points):
    """(nsite, int32 links, float64 points (nsite, 3) or None) of a list of sites, shapes checked before any library call"""
    links = np.ascontiguousarray(np.asarray(links, dtype=np.int32).reshape(-1))
    if points is not None:
        points = np.ascontiguousarray(points, dtype=np.float64)
        if points.shape != (links.size, 3):
            raise ValueError(f"site points of shape {points.shape}: expected ({links.size}, 3)")
    return links.size, links, points


def _jac_arrays(n, ns, nc, nd, flags):
    """host arrays of the Jacobians over n instances: {name: array} of the quantities `flags` selects"""
    shapes = {"J": (n, ns, 6, nd), "Jcom": (n, nc, 3, nd)}
    return {k: np.empty(shapes[k]) for k, f in _JAC_KEYS if flags & f}


# joint-space dynamics (include/rkfd_hip.h: RKFD_DYN_*): what update_dynamics computes and get_dynamics returns
DYN_MASS, DYN_BIAS, DYN_GRAVITY, DYN_ROTOR = 1, 2, 4, 8
DYN_ALL = DYN_MASS | DYN_BIAS | DYN_GRAVITY
_DYN_KEYS = (("M", DYN_MASS), ("h", DYN_BIAS), ("g", DYN_GRAVITY))


def _dyn_arrays(n, nd, flags):
    """host arrays of the dynamics over n instances: {name: array} of the quantities `flags` selects"""
    shapes = {"M": (n, nd, nd), "h": (n, nd), "g": (n, nd)}
    return {k: np.empty(shapes[k]) for k, f in _DYN_KEYS if flags & f}


# contact read-out (include/rkfd_hip.h: RKFD_CF_*): what update_contact_forces computes and get_contact_forces returns
CF_POINT, CF_WRENCH, CF_GENF = 1, 2, 4
CF_ALL = CF_POINT | CF_WRENCH | CF_GENF
_CF_KEYS = (("point", CF_POINT), ("wrench", CF_WRENCH), ("count", CF_WRENCH), ("genf", CF_GENF))
_CF_DEV = ("rkfdBatchDevContactPoint", "rkfdBatchDevContactWrench", "rkfdBatchDevContactCount", "rkfdBatchDevContactGenForce")


def _cf_shapes(n, nc, nl, nd):
    return {"point": (n, nc, 3), "wrench": (n, nl, 6), "count": (n, nl), "genf": (n, nd)}


def _cf_arrays(n, nc, nl, nd, flags):
    """host arrays of the contact read-out over n instances: {name: array} of the quantities `flags` selects (count: int32)"""
    shapes = _cf_shapes(n, nc, nl, nd)
    return {k: np.empty(shapes[k], dtype=np.int32 if k == "count" else np.float64) for k, f in _CF_KEYS if flags & f}


def _cf_dev_ptr(name, t, typestr, shapes, device):
    """device address of an argument of update_contact_forces, checked before any library call: a contiguous torch tensor on
    cuda:`device`, or any object with a __cuda_array_interface__ (contiguous; its device is the caller's word)"""
    if type(t).__module__.split(".")[0] == "torch":
        import torch
        want = {"<i4": torch.int32, "<f8": torch.float64}[typestr]
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"update_contact_forces: {name} of type {type(t).__name__}: expected a torch tensor")
        if tuple(t.shape) not in shapes:
            raise ValueError(f"update_contact_forces: {name} of shape {tuple(t.shape)}: expected {shapes[0]}")
        if t.dtype != want:
            raise TypeError(f"update_contact_forces: {name} of dtype {t.dtype}: expected {want}")
        if t.device.type != "cuda" or t.device.index != device:
            raise ValueError(f"update_contact_forces: {name} on {t.device}: expected cuda:{device}")
        if not t.is_contiguous():
            raise ValueError(f"update_contact_forces: {name} must be contiguous")
        return t.data_ptr()
    cai = getattr(t, "__cuda_array_interface__", None)
    if cai is None:
        raise TypeError(f"update_contact_forces: {name} of type {type(t).__name__}: expected a torch tensor on the device (or an object with a __cuda_array_interface__)")
    if tuple(cai["shape"]) not in shapes:
        raise ValueError(f"update_contact_forces: {name} of shape {tuple(cai['shape'])}: expected {shapes[0]}")
    if cai["typestr"] != typestr:
        raise TypeError(f"update_contact_forces: {name} of type {cai['typestr']}: expected {typestr}")
    if cai.get("strides") is not None:
        raise ValueError(f"update_contact_forces: {name} must be contiguous")
    return int(cai["data"][0])


# per-instance reset (include/rkfd_hip.h: RKFD_RESET_*): slot values besides the rows 0 .. nslots-1 of the bank
RESET_KEEP, RESET_SNAPSHOT = -1, -2


def reset_slots(slots, n, device=None):
    """the slot values of a reset over n instances, checked before any library call -> ("host", int32 array (n,)) or ("dev",
    tensor).  A numpy int32 array (n,) is taken as it is; a numpy bool mask (n,) stands for RESET_SNAPSHOT where True and
    RESET_KEEP where False; a contiguous torch int32 tensor (n,) on cuda:`device` is read in place (device=None: host forms only)."""
    if isinstance(slots, np.ndarray):
        if slots.shape != (n,):
            raise ValueError(f"reset slots of shape {slots.shape}: expected ({n},)")
        if slots.dtype == np.bool_:
            return "host", np.where(slots, RESET_SNAPSHOT, RESET_KEEP).astype(np.int32)
        if slots.dtype != np.int32:
            raise TypeError(f"reset slots of dtype {slots.dtype}: expected int32 (slot values) or bool (a mask: True = RESET_SNAPSHOT)")
        return "host", np.ascontiguousarray(slots)
    if type(slots).__module__.split(".")[0] != "torch" or device is None:
        raise TypeError(f"reset slots of type {type(slots).__name__}: expected a numpy int32 or bool array"
                        + ("" if device is None else " or a torch int32 tensor"))
    import torch
    if not isinstance(slots, torch.Tensor):
        raise TypeError(f"reset slots of type {type(slots).__name__}: expected a numpy int32 or bool array or a torch int32 tensor")
    if tuple(slots.shape) != (n,):
        raise ValueError(f"reset slots of shape {tuple(slots.shape)}: expected ({n},)")
    if slots.dtype != torch.int32:
        raise TypeError(f"reset slots of dtype {slots.dtype}: expected torch.int32")
    if slots.device.type != "cuda" or slots.device.index != device:
        raise ValueError(f"reset slots on {slots.device}: expected cuda:{device}")
    if not slots.is_contiguous():
        raise ValueError("reset slots: the tensor must be contiguous")
    return "dev", slots


# per-instance physical parameters (include/rkfd_hip.h: RKFD_PAR_*): the key of a name is its place here
PARAM_NAMES = ("mass", "com", "inertia", "stiff", "visc", "coulomb", "sfric", "ci_sf", "ci_kf", "ci_k", "ci_l", "ci_e", "ci_v")


def param_key(name_or_key):
    """key of a parameter given by name ("mass", "ci_kf", ...) or by key; an unknown NAME is a ValueError, an unknown integer
    key goes to the library, which refuses it with a message"""
    if isinstance(name_or_key, str):
        if name_or_key not in PARAM_NAMES:
            raise ValueError(f"unknown parameter {name_or_key!r}: one of {', '.join(PARAM_NAMES)}")
        return PARAM_NAMES.index(name_or_key)
    return int(name_or_key)


class Batch:
    """B instances of one world on one GPU (include/rkfd_hip.h).  All arrays are
    instance-major numpy arrays [B, ...]."""

    def __init__(self, world, batch, device=0, max_rigid=8, _handle=None):
        """_handle: an rkfdBatch that someone else owns (Node.batch) - close() then only forgets it"""
        self._L = lib()
        self.world = world
        m = world.model.contents
        self.B, self.ndof, self.nlink, self.ncand = batch, m.ndof, m.nlink, m.ncand
        self.nchain = m.nchain
        self._links_flags = 0          # what the last update_links() computed
        self._jac_flags = 0            # what the last update_jacobians() computed, of the present sites
        self._dyn_flags = 0            # what the last update_dynamics() computed
        self._cf_flags = 0             # what the last update_contact_forces() computed
        self.device = device
        self._ctrl_keep = []           # device schedules of update_controlled() the launches issued since the last join / sync read
        self._owned = _handle is None
        self._b = self._L.rkfdBatchCreate(world.model, batch, device, max_rigid) if self._owned else _handle
        if not self._b:
            raise RkfdError(self._L.rkfdHipLastError().decode())

    def close(self):
        if getattr(self, "_b", None):
            if self._owned:
                self._L.rkfdBatchDestroy(self._b)
            self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r):
        if r < 0:
            raise RkfdError(self._L.rkfdHipLastError().decode())

    def _synced(self, r):
        """after a call that waited for the batch's launches: the device schedules they read may go"""
        self._chk(r)
        self._ctrl_keep.clear()

    def set_state(self, dis, vel):
        dis = np.ascontiguousarray(dis, dtype=np.float64).reshape(self.B, self.ndof)
        vel = np.ascontiguousarray(vel, dtype=np.float64).reshape(self.B, self.ndof)
        self._synced(self._L.rkfdBatchSetState(self._b, _ptr(dis), _ptr(vel)))

    def get_state(self):
        dis = np.empty((self.B, self.ndof)); vel = np.empty_like(dis); acc = np.empty_like(dis)
        self._synced(self._L.rkfdBatchGetState(self._b, _ptr(dis), _ptr(vel), _ptr(acc)))
        return dis, vel, acc

    def set_motor_input(self, inp):
        inp = np.ascontiguousarray(inp, dtype=np.float64).reshape(self.B, self.nlink)
        self._synced(self._L.rkfdBatchSetMotorInput(self._b, _ptr(inp)))

    def get_contact(self):
        act = np.empty((self.B, self.ncand), dtype=np.int32); typ = np.empty_like(act)
        ref = np.empty((self.B, self.ncand, 3)); f = np.empty_like(ref)
        self._synced(self._L.rkfdBatchGetContact(self._b, _ptr(act), _ptr(typ), _ptr(ref), _ptr(f)))
        return act, typ, ref, f

    def set_contact(self, act, typ, ref):
        act = np.ascontiguousarray(act, dtype=np.int32); typ = np.ascontiguousarray(typ, dtype=np.int32)
        ref = np.ascontiguousarray(ref, dtype=np.float64)
        self._synced(self._L.rkfdBatchSetContact(self._b, _ptr(act), _ptr(typ), _ptr(ref)))

    def get_pivot(self):
        typ = np.empty((self.B, self.nlink), dtype=np.int32); prev = np.empty((self.B, self.nlink))
        self._synced(self._L.rkfdBatchGetPivot(self._b, _ptr(typ), _ptr(prev)))
        return typ, prev

    def set_pivot(self, typ, prev):
        typ = np.ascontiguousarray(typ, dtype=np.int32); prev = np.ascontiguousarray(prev, dtype=np.float64)
        self._synced(self._L.rkfdBatchSetPivot(self._b, _ptr(typ), _ptr(prev)))

    def get_broken(self):
        """breakable float joints: 1 per link whose joint has broken, [B, nlink]"""
        br = np.empty((self.B, self.nlink), dtype=np.int32)
        self._synced(self._L.rkfdBatchGetBroken(self._b, _ptr(br)))
        return br

    def set_broken(self, broken):
        br = np.ascontiguousarray(broken, dtype=np.int32).reshape(self.B, self.nlink)
        self._synced(self._L.rkfdBatchSetBroken(self._b, _ptr(br)))

    def param_width(self, name_or_key):
        """doubles per instance of a parameter: nlink * {1, 3, 9} or nci (model space)"""
        w = self._L.rkfdBatchParamWidth(self._b, param_key(name_or_key))
        if w < 0:
            raise RkfdError(f"unknown parameter key {name_or_key!r}")
        return w

    def set_param(self, name_or_key, values):
        """per-instance physical parameters (rkfdBatchSetParam): values (B, width) in MODEL space - the links / contact infos of
        the world the batch was made from -, None: this parameter back to the model's value.  Synchronous; takes effect from the
        next launch; touches no state."""
        k = param_key(name_or_key)
        if values is None:
            self._synced(self._L.rkfdBatchSetParam(self._b, k, None))
            return
        w = self._L.rkfdBatchParamWidth(self._b, k)
        if w >= 0:
            values = np.ascontiguousarray(values, dtype=np.float64).reshape(self.B, w)
        else:
            values = np.ascontiguousarray(values, dtype=np.float64)      # (the library refuses the key with its message)
        self._synced(self._L.rkfdBatchSetParam(self._b, k, _ptr(values)))

    def get_param(self, name_or_key):
        """what the next launch will use, (B, width): the model's values where the parameter was never set"""
        k = param_key(name_or_key)
        out = np.empty((self.B, self.param_width(k)))
        self._chk(self._L.rkfdBatchGetParam(self._b, k, _ptr(out)))
        return out

    def clear_params(self):
        self._synced(self._L.rkfdBatchClearParams(self._b))

    def has_params(self):
        return bool(self._L.rkfdBatchHasParams(self._b))

    def update_init(self, stream=None):
        self._chk(self._L.rkfdBatchUpdateInit(self._b, stream))

    def update(self, nsteps=1, stream=None):
        self._chk(self._L.rkfdBatchUpdate(self._b, nsteps, stream))

    def update_controlled(self, u, stream=None):
        """H x (set the motor inputs u[:, k, :]; rkFDUpdate) for a control schedule u of shape (B, H, nlink), float64: the same bits as
        H x (set_motor_input(u[:, k]); update(1)), in the launches update() makes; afterwards the motor input is u[:, H-1, :].
        A numpy array is copied before the call returns.  A torch tensor on the batch's device is read in place, in order after
        `stream` (default: torch.cuda.current_stream()); the batch keeps a reference to it until join() or a synchronous accessor."""
        if isinstance(u, np.ndarray):
            if u.ndim != 3 or u.shape[0] != self.B or u.shape[2] != self.nlink or u.shape[1] < 1:
                raise ValueError(f"control schedule of shape {u.shape}: expected ({self.B}, H, {self.nlink})")
            if u.dtype != np.float64:
                raise TypeError(f"control schedule of dtype {u.dtype}: expected float64")
            u = np.ascontiguousarray(u)
            self._chk(self._L.rkfdBatchUpdateControlled(self._b, u.shape[1], _ptr(u), stream))
            return
        import torch
        if not isinstance(u, torch.Tensor):
            raise TypeError(f"control schedule of type {type(u).__name__}: expected a numpy array or a torch tensor")
        if u.dim() != 3 or u.shape[0] != self.B or u.shape[2] != self.nlink or u.shape[1] < 1:
            raise ValueError(f"control schedule of shape {tuple(u.shape)}: expected ({self.B}, H, {self.nlink})")
        if u.dtype != torch.float64:
            raise TypeError(f"control schedule of dtype {u.dtype}: expected torch.float64")
        if u.device.type != "cuda" or u.device.index != self.device:
            raise ValueError(f"control schedule on {u.device}: expected cuda:{self.device}")
        if not u.is_contiguous():
            raise ValueError("control schedule: the tensor must be contiguous")
        if stream is None:
            stream = torch.cuda.current_stream(u.device).cuda_stream
        self._chk(self._L.rkfdBatchUpdateControlledDev(self._b, u.shape[1], C.c_void_p(u.data_ptr()), C.c_void_p(stream or 0)))
        self._ctrl_keep.append(u)      # read by launches that may still be queued on the internal streams

    def eval(self, do_up_ref=False, stream=None):
        self._chk(self._L.rkfdBatchEval(self._b, 1 if do_up_ref else 0, stream))

    def status(self, stream=None):
        r = self._L.rkfdBatchStatus(self._b, stream)
        self._synced(r)
        return r

    def contact_stats(self, reset=False):
        """(mean rigid, mean elastic contact vertices per instance-step, instance-steps counted) since the last reset"""
        rg = C.c_double(); el = C.c_double(); n = C.c_longlong()
        self._chk(self._L.rkfdBatchContactStats(self._b, int(bool(reset)), C.byref(rg), C.byref(el), C.byref(n)))
        return rg.value, el.value, n.value

    def snapshot(self):
        """keep a device-resident copy of the whole state (start of MPC-style rollouts)"""
        self._chk(self._L.rkfdBatchSnapshot(self._b))

    def restore(self, stream=None):
        """put the snapshot back, in stream order (no host traffic)"""
        self._chk(self._L.rkfdBatchRestore(self._b, C.c_void_p(stream or 0)))

    def bank_reserve(self, nslots):
        """rkfdBatchBankReserve: (re)allocate the bank of start states with nslots rows on the batch's device (contents undefined);
        0 frees it.  Synchronous."""
        self._synced(self._L.rkfdBatchBankReserve(self._b, int(nslots)))

    def bank_size(self):
        return self._L.rkfdBatchBankSize(self._b)

    def bank_store(self, slot, first=0, count=1):
        """rows slot .. slot+count-1 of the bank <- the live state of the instances first .. first+count-1 (after update_init, and
        any steps, the rows hold consistent accelerations, pivots, anchors and forces).  Synchronous."""
        self._synced(self._L.rkfdBatchBankStore(self._b, int(slot), int(first), int(count)))

    def reset(self, slots, stream=None):
        """per-instance reset ON THE DEVICE, in stream order (rkfdBatchReset): instance i gets bank row slots[i], keeps its state
        (RESET_KEEP) or gets its own row of snapshot() (RESET_SNAPSHOT); any other value leaves it as it is and status() reports 5.
        slots: a numpy int32 array (B,), copied before the call returns; a numpy bool mask (B,) - True: RESET_SNAPSHOT, False:
        RESET_KEEP; or a contiguous torch int32 tensor (B,) on the batch's device - read in place, in order after `stream`
        (default: torch.cuda.current_stream()), and kept referenced until join() or a synchronous accessor."""
        kind, s = reset_slots(slots, self.B, self.device)
        if kind == "host":
            self._chk(self._L.rkfdBatchReset(self._b, _ptr(s), C.c_void_p(stream or 0)))
            return
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(s.device).cuda_stream
        self._chk(self._L.rkfdBatchResetDev(self._b, C.c_void_p(s.data_ptr()), C.c_void_p(stream or 0)))
        self._ctrl_keep.append(s)      # read by a launch that may still be queued

    def set_split(self, nsplit):
        """rkfdBatchSetSplit: launch the batch as nsplit kernels on internal streams (tails overlap)"""
        self._chk(self._L.rkfdBatchSetSplit(self._b, int(nsplit)))

    def join(self, stream=None):
        """rkfdBatchJoin: make `stream` wait for the split launches (no host synchronisation)"""
        self._synced(self._L.rkfdBatchJoin(self._b, C.c_void_p(stream or 0)))

    def time_launches(self, on=True):
        self._chk(self._L.rkfdBatchTimeLaunches(self._b, int(bool(on))))

    def launch_timing(self):
        """(number of launches, their summed duration in ms) since time_launches(True); synchronises the device"""
        n = C.c_int(); ms = C.c_double()
        self._chk(self._L.rkfdBatchLaunchTiming(self._b, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def profile(self, nsteps=1):
        """diagnostic launch with in-kernel phase stamps: [B, 32] cycles (RKFD_NPROF)"""
        out = np.zeros((self.B, 32), dtype=np.uint64)
        self._chk(self._L.rkfdBatchProfile(self._b, nsteps, _ptr(out)))
        return out

    @property
    def lds_bytes(self):
        return self._L.rkfdBatchLdsBytes(self._b)

    def set_steps_per_launch(self, n):
        """under split launches: steps one launch carries (default 5)"""
        self._chk(self._L.rkfdBatchSetStepsPerLaunch(self._b, int(n)))

    def set_instances_per_wave(self, ipw):
        """1 (default) or 2 instances per wavefront in the world-specific kernel; call before specialize()"""
        self._chk(self._L.rkfdBatchSetInstancesPerWave(self._b, int(ipw)))

    def instances_per_wave(self):
        return self._L.rkfdBatchInstancesPerWave(self._b)

    def tune_instances_per_wave(self, nsteps=8):
        """measure both mappings on the present state (kept), keep the faster; -> (chosen, (ms with 1, ms with 2))"""
        ms = (C.c_double * 2)()
        r = self._L.rkfdBatchTuneInstancesPerWave(self._b, int(nsteps), ms)
        self._chk(r)
        return r, (ms[0], ms[1])

    def specialize(self):
        """compile the step kernel for this world (hipRTC): same results, its dimensions as literals"""
        self._chk(self._L.rkfdBatchSpecialize(self._b))

    def residency(self):
        """instances per compute unit the HIP runtime can keep resident (registers + LDS)"""
        return self._L.rkfdBatchResidency(self._b)

    def update_links(self, flags=LINKS_ALL, stream=None):
        """task-space read-out ON THE DEVICE from the live state: poses (LINKS_POSE) and velocities (LINKS_VEL) of every model
        link, centre of mass and its velocity of every chain (LINKS_COM).  One kernel launch in stream order after everything the
        batch has launched (no host wait, no state changed); get_links() / links_tensors() / dev_tensors(links=True) hand the results out."""
        self._chk(self._L.rkfdBatchUpdateLinks(self._b, int(flags), stream))
        self._links_flags = int(flags)

    def get_links(self):
        """host copies of the last update_links(): a dict with (of what its flags selected) R [B, nl, 3, 3] (row-major, link ->
        world), p [B, nl, 3] (world), v [B, nl, 6] ((linear, angular) of the link origin in the link's own frame), com and
        comvel [B, nc, 3] (world)"""
        if not self._links_flags:
            raise RkfdError("get_links: no read-out has been made (update_links)")
        out = _links_arrays(self.B, self.nlink, self.nchain, self._links_flags)
        self._chk(self._L.rkfdBatchGetLinks(self._b, *[_ptr(out.get(k)) for k, _ in _LINKS_KEYS]))
        return out

    def set_jacobian_sites(self, links, points=None):
        """the sites of the following update_jacobians(): model links (nsite,) and points (nsite, 3) in the links' frames (None:
        the link origins); an empty list clears them.  Synchronous; a refused list leaves the previous sites in place."""
        ns, links, points = _jac_sites(links, points)
        self._chk(self._L.rkfdBatchSetJacobianSites(self._b, ns, _ptr(links), _ptr(points)))
        self._jac_flags &= ~JAC_SITES

    @property
    def nsite(self):
        return self._L.rkfdBatchJacobianSiteNum(self._b)

    def update_jacobians(self, flags=JAC_ALL, stream=None):
        """task-space Jacobians ON THE DEVICE from the live state: J (JAC_SITES) maps the packed joint RATES to the world velocity
        of every site point and the world angular velocity of its link, Jcom (JAC_COM) to the velocity of every chain's centre of
        mass.  One kernel launch in stream order after everything the batch has launched (no host wait, no state changed);
        get_jacobians() / jacobian_tensors() hand the results out."""
        self._chk(self._L.rkfdBatchUpdateJacobians(self._b, int(flags), stream))
        self._jac_flags = int(flags)

    def get_jacobians(self):
        """host copies of the last update_jacobians(): a dict with (of what its flags selected) J [B, nsite, 6, ndof] and
        Jcom [B, nc, 3, ndof], world frame, columns in the order of the packed rate vector"""
        if not self._jac_flags:
            raise RkfdError("get_jacobians: no Jacobians have been computed (update_jacobians)")
        out = _jac_arrays(self.B, self.nsite, self.nchain, self.ndof, self._jac_flags)
        self._chk(self._L.rkfdBatchGetJacobians(self._b, *[_ptr(out.get(k)) for k, _ in _JAC_KEYS]))
        return out

    def jacobian_ptrs(self):
        """device addresses of J and Jcom (None for a buffer no update_jacobians() has needed yet; J's moves when nsite changes)"""
        return (self._L.rkfdBatchDevJacobian(self._b), self._L.rkfdBatchDevComJacobian(self._b))

    def jacobian_tensors(self):
        """the Jacobians' buffers as a dict of zero-copy float64 torch views, J [B, nsite, 6, ndof] and Jcom [B, nc, 3, ndof]
        (None where no update_jacobians() has needed the buffer yet)"""
        import torch

        class _View:
            def __init__(self, ptr, shape):
                self.__cuda_array_interface__ = dict(shape=shape, typestr="<f8", data=(int(ptr), False), version=2, strides=None)
        shapes = ((self.B, self.nsite, 6, self.ndof), (self.B, self.nchain, 3, self.ndof))
        return {k: torch.as_tensor(_View(p, sh), device="cuda") if p else None for (k, _), p, sh in zip(_JAC_KEYS, self.jacobian_ptrs(), shapes)}

    def update_dynamics(self, flags=DYN_ALL, stream=None):
        """joint-space dynamics ON THE DEVICE from the live state: the inertia matrix M (DYN_MASS) with respect to the packed joint
        RATES, the bias force h = rnea(q, qd, 0) (DYN_BIAS) and the gravity force g (DYN_GRAVITY), M qdd + h = generalised force;
        DYN_ROTOR adds the reflected rotor inertia of the DC-motor joints to M's diagonal.  One kernel launch in stream order after
        everything the batch has launched (no host wait, no state changed); get_dynamics() / dynamics_tensors() hand the results out."""
        self._chk(self._L.rkfdBatchUpdateDynamics(self._b, int(flags), stream))
        self._dyn_flags = int(flags)

    def get_dynamics(self):
        """host copies of the last update_dynamics(): a dict with (of what its flags selected) M [B, ndof, ndof], h and g [B, ndof],
        rows and columns in the order of the packed rate vector"""
        if not self._dyn_flags:
            raise RkfdError("get_dynamics: no dynamics have been computed (update_dynamics)")
        out = _dyn_arrays(self.B, self.ndof, self._dyn_flags)
        self._chk(self._L.rkfdBatchGetDynamics(self._b, *[_ptr(out.get(k)) for k, _ in _DYN_KEYS]))
        return out

    def dynamics_ptrs(self):
        """device addresses of M, h and g (None for a buffer no update_dynamics() has needed yet; stable once allocated)"""
        return tuple(getattr(self._L, f)(self._b) for f in ("rkfdBatchDevMassMatrix", "rkfdBatchDevBias", "rkfdBatchDevGravity"))

    def dynamics_tensors(self):
        """the dynamics' buffers as a dict of zero-copy float64 torch views, M [B, ndof, ndof], h and g [B, ndof] (None where no
        update_dynamics() has needed the buffer yet)"""
        import torch

        class _View:
            def __init__(self, ptr, shape):
                self.__cuda_array_interface__ = dict(shape=shape, typestr="<f8", data=(int(ptr), False), version=2, strides=None)
        shapes = ((self.B, self.ndof, self.ndof), (self.B, self.ndof), (self.B, self.ndof))
        return {k: torch.as_tensor(_View(p, sh), device="cuda") if p else None for (k, _), p, sh in zip(_DYN_KEYS, self.dynamics_ptrs(), shapes)}

    def update_contact_forces(self, flags=CF_ALL, stream=None, active=None, f=None):
        """contact read-out ON THE DEVICE from the live joint coordinates and the force of every candidate contact vertex: the world
        position of every candidate vertex (CF_POINT), the net contact wrench and the number of active candidates of every model
        link (CF_WRENCH) and the generalised contact force J_c' f on the packed joint rates (CF_GENF).  One kernel launch in stream
        order after everything the batch has launched (no host wait, no state changed).  active / f: the caller's own flags and
        forces in place of the batch's, contiguous int32 (B, ncand) and float64 (B, ncand, 3) torch tensors on the batch's device
        (or other objects with a __cuda_array_interface__ of those shapes and types), read in place in order after `stream`
        (default for tensors: torch.cuda.current_stream()); the batch keeps a reference to them until join() or a synchronous
        accessor.  get_contact_forces() / contact_force_tensors() hand the results out."""
        if active is None and f is None:
            self._chk(self._L.rkfdBatchUpdateContactForces(self._b, int(flags), stream))
            self._cf_flags = int(flags)
            return
        if active is None or f is None:
            raise ValueError("update_contact_forces: active and f are given together (%s is missing)" % ("active" if active is None else "f"))
        pa = _cf_dev_ptr("active", active, "<i4", ((self.B, self.ncand),), self.device)
        pf = _cf_dev_ptr("f", f, "<f8", ((self.B, self.ncand, 3), (self.B, self.ncand * 3)), self.device)
        if stream is None and type(f).__module__.split(".")[0] == "torch":
            import torch
            stream = torch.cuda.current_stream(f.device).cuda_stream
        self._chk(self._L.rkfdBatchUpdateContactForcesDev(self._b, int(flags), C.c_void_p(pa), C.c_void_p(pf), C.c_void_p(stream or 0)))
        self._cf_flags = int(flags)
        self._ctrl_keep.append((active, f))      # read by a launch that may still be queued

    def get_contact_forces(self):
        """host copies of the last update_contact_forces(): a dict with (of what its flags selected) point [B, ncand, 3] (world),
        wrench [B, nlink, 6] (world axes: force, moment about the link origin), count [B, nlink] (int32) and genf [B, ndof]"""
        if not self._cf_flags:
            raise RkfdError("get_contact_forces: no contact forces have been computed (update_contact_forces)")
        out = _cf_arrays(self.B, self.ncand, self.nlink, self.ndof, self._cf_flags)
        self._chk(self._L.rkfdBatchGetContactForces(self._b, *[_ptr(out.get(k)) for k, _ in _CF_KEYS]))
        return out

    def contact_force_ptrs(self):
        """device addresses of point, wrench, count and genf (None for a buffer no update_contact_forces() has needed yet; stable
        once allocated)"""
        return tuple(getattr(self._L, f)(self._b) for f in _CF_DEV)

    def contact_force_tensors(self):
        """the contact read-out's buffers as a dict of zero-copy torch views, point [B, ncand, 3], wrench [B, nlink, 6] and genf
        [B, ndof] float64, count [B, nlink] int32 (None where no update_contact_forces() has needed the buffer yet, or it is empty)"""
        import torch

        class _View:
            def __init__(self, ptr, shape, typestr):
                self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(int(ptr), False), version=2, strides=None)
        shapes = _cf_shapes(self.B, self.ncand, self.nlink, self.ndof)
        return {k: torch.as_tensor(_View(p, shapes[k], "<i4" if k == "count" else "<f8"), device="cuda") if p and np.prod(shapes[k]) else None
                for (k, _), p in zip(_CF_KEYS, self.contact_force_ptrs())}

    def dev_tensors(self, links=False):
        """torch tensors ALIASING the live device state [B, ndof] (dis, vel, acc): zero-copy views
        for consumers on the device, e.g. the RCCL all-gather of final states.  links=True: the buffers of the task-space
        read-out follow, likewise zero-copy - R [B, nl, 3, 3], p [B, nl, 3], v [B, nl, 6], com, comvel [B, nc, 3], None where no
        update_links() has needed the buffer yet - always eight entries; without it always the three, whatever has been read out."""
        import torch

        class _View:
            def __init__(self, ptr, shape):
                self.__cuda_array_interface__ = dict(shape=shape, typestr="<f8", data=(int(ptr), False), version=2, strides=None)
        ptrs = self.dev_ptrs(links)
        nl, nc = self.nlink, self.nchain
        shapes = ((self.B, self.ndof),) * 3 + ((self.B, nl, 3, 3), (self.B, nl, 3), (self.B, nl, 6), (self.B, nc, 3), (self.B, nc, 3))
        return tuple(torch.as_tensor(_View(p, sh), device="cuda") if p else None for p, sh in zip(ptrs, shapes[:len(ptrs)]))

    def links_tensors(self):
        """the read-out's buffers alone, as a dict of zero-copy torch views (R, p, v, com, comvel; None where no update_links()
        has needed the buffer yet)"""
        return dict(zip([k for k, _ in _LINKS_KEYS], self.dev_tensors(links=True)[3:]))

    def dev_ptrs(self, links=False):
        """device addresses of dis, vel, acc; links=True: followed by those of the read-out's R, p, v, com, comvel (None for a
        buffer no update_links() has needed yet; stable once allocated)"""
        st = (self._L.rkfdBatchDevDis(self._b), self._L.rkfdBatchDevVel(self._b), self._L.rkfdBatchDevAcc(self._b))
        if not links:
            return st
        return st + tuple(getattr(self._L, f)(self._b) for f in ("rkfdBatchDevLinkAtt", "rkfdBatchDevLinkPos", "rkfdBatchDevLinkVel", "rkfdBatchDevCom", "rkfdBatchDevComVel"))


class Node:
    """`total` instances of one world over the GPUs of one node from ONE process (include/rkfd_hip.h: rkfdNode*): device k
    simulates its contiguous shard with its own host thread and stream inside the library, no per-step communication; the
    only collective is gather(): one RCCL all-gather of the final {dis, vel}."""

    def __init__(self, world, total, max_rigid=8, ndev=0, devices=None):
        self._L = lib()
        self.world = world
        m = world.model.contents
        self.total, self.ndof, self.nlink, self.nchain = total, m.ndof, m.nlink, m.nchain
        self.ncand = m.ncand
        dv = None
        if devices is not None:
            dv = (C.c_int * len(devices))(*devices); ndev = len(devices)
        self._n = self._L.rkfdNodeCreate(world.model, total, max_rigid, ndev, C.cast(dv, C.c_void_p) if dv is not None else None)
        if not self._n:
            raise RkfdError(self._L.rkfdHipLastError().decode())
        self.ndev = self._L.rkfdNodeDevices(self._n)

    def close(self):
        if getattr(self, "_n", None):
            self._L.rkfdNodeDestroy(self._n)
            self._n = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r):
        if r < 0:
            raise RkfdError(self._L.rkfdHipLastError().decode())
        return r

    def shards(self):
        out = []
        for k in range(self.ndev):
            d, lo, hi = C.c_int(), C.c_int(), C.c_int()
            self._chk(self._L.rkfdNodeShard(self._n, k, C.byref(d), C.byref(lo), C.byref(hi)))
            out.append((d.value, lo.value, hi.value))
        return out

    def batch(self, k):
        """the Batch behind shard k (rkfdNodeBatch), for the per-batch accessors: a view - the node keeps owning it, and it must
        not be used after the node is closed"""
        if not 0 <= k < self.ndev:
            raise RkfdError(f"no shard {k} (the node has {self.ndev})")
        dev, lo, hi = self.shards()[k]
        return Batch(self.world, hi - lo, device=dev, _handle=self._L.rkfdNodeBatch(self._n, k))

    def set_state(self, dis, vel):
        dis = np.ascontiguousarray(dis, dtype=np.float64).reshape(self.total, self.ndof)
        vel = np.ascontiguousarray(vel, dtype=np.float64).reshape(self.total, self.ndof)
        self._chk(self._L.rkfdNodeSetState(self._n, _ptr(dis), _ptr(vel)))

    def set_motor_input(self, inp):
        inp = np.ascontiguousarray(inp, dtype=np.float64).reshape(self.total, self.nlink)
        self._chk(self._L.rkfdNodeSetMotorInput(self._n, _ptr(inp)))

    def set_param(self, name_or_key, values):
        """Batch.set_param over all instances: values (total, width), sharded like set_state; None: back to the model's value"""
        k = param_key(name_or_key)
        if values is not None:
            values = np.ascontiguousarray(values, dtype=np.float64).reshape(self.total, -1)
        self._chk(self._L.rkfdNodeSetParam(self._n, k, _ptr(values) if values is not None else None))

    def clear_params(self):
        self._chk(self._L.rkfdNodeClearParams(self._n))

    def update_controlled(self, u):
        """Batch.update_controlled on every device: u is the host schedule of all instances, (total, H, nlink) float64"""
        if not isinstance(u, np.ndarray) or u.ndim != 3 or u.shape[0] != self.total or u.shape[2] != self.nlink or u.shape[1] < 1:
            raise ValueError(f"control schedule of shape {getattr(u, 'shape', None)}: expected a numpy array ({self.total}, H, {self.nlink})")
        if u.dtype != np.float64:
            raise TypeError(f"control schedule of dtype {u.dtype}: expected float64")
        u = np.ascontiguousarray(u)
        self._chk(self._L.rkfdNodeUpdateControlled(self._n, u.shape[1], _ptr(u)))

    def get_state(self):
        dis = np.empty((self.total, self.ndof)); vel = np.empty_like(dis); acc = np.empty_like(dis)
        self._chk(self._L.rkfdNodeGetState(self._n, _ptr(dis), _ptr(vel), _ptr(acc)))
        return dis, vel, acc

    def specialize(self):
        self._chk(self._L.rkfdNodeSpecialize(self._n))

    def set_split(self, nsplit):
        self._chk(self._L.rkfdNodeSetSplit(self._n, nsplit))

    def set_steps_per_launch(self, n):
        self._chk(self._L.rkfdNodeSetStepsPerLaunch(self._n, int(n)))

    def tune_instances_per_wave(self, nsteps=8):
        self._chk(self._L.rkfdNodeTuneInstancesPerWave(self._n, int(nsteps)))

    def update_init(self):
        self._chk(self._L.rkfdNodeUpdateInit(self._n))

    def update(self, nsteps=1):
        self._chk(self._L.rkfdNodeUpdate(self._n, nsteps))

    def snapshot(self):
        self._chk(self._L.rkfdNodeSnapshot(self._n))

    def restore(self):
        self._chk(self._L.rkfdNodeRestore(self._n))

    def status(self):
        return self._chk(self._L.rkfdNodeStatus(self._n))

    def bank_reserve(self, nslots):
        """Batch.bank_reserve on every device: the bank is replicated, like the model"""
        self._chk(self._L.rkfdNodeBankReserve(self._n, int(nslots)))

    def bank_store(self, slot, first=0, count=1):
        """rows slot .. of EVERY device's bank <- the live state of the instances first .. first+count-1, GLOBAL indices"""
        self._chk(self._L.rkfdNodeBankStore(self._n, int(slot), int(first), int(count)))

    def reset(self, slots):
        """Batch.reset over all instances: slots is a numpy int32 array or bool mask (total,), sharded like set_state"""
        _, s = reset_slots(slots, self.total)
        self._chk(self._L.rkfdNodeReset(self._n, _ptr(s)))

    def get_links(self, flags=LINKS_ALL):
        """Batch.update_links(flags) on every device's own thread and stream, then the results of ALL instances in instance
        order, as Batch.get_links() returns them"""
        out = _links_arrays(self.total, self.nlink, self.nchain, int(flags))
        self._chk(self._L.rkfdNodeGetLinks(self._n, int(flags), *[_ptr(out.get(k)) for k, _ in _LINKS_KEYS]))
        return out

    def set_jacobian_sites(self, links, points=None):
        """Batch.set_jacobian_sites on every device: the sites are replicated, like the model"""
        ns, links, points = _jac_sites(links, points)
        self._chk(self._L.rkfdNodeSetJacobianSites(self._n, ns, _ptr(links), _ptr(points)))

    def get_jacobians(self, flags=JAC_ALL):
        """Batch.update_jacobians(flags) on every device's own thread and stream, then the results of ALL instances in instance
        order, as Batch.get_jacobians() returns them"""
        ns = max(self._L.rkfdBatchJacobianSiteNum(self._L.rkfdNodeBatch(self._n, 0)), 0)
        out = _jac_arrays(self.total, ns, self.nchain, self.ndof, int(flags))
        self._chk(self._L.rkfdNodeGetJacobians(self._n, int(flags), *[_ptr(out.get(k)) for k, _ in _JAC_KEYS]))
        return out

    def get_contact_forces(self, flags=CF_ALL):
        """Batch.update_contact_forces(flags) on every device's own thread and stream, then the results of ALL instances in
        instance order, as Batch.get_contact_forces() returns them"""
        out = _cf_arrays(self.total, self.ncand, self.nlink, self.ndof, int(flags))
        self._chk(self._L.rkfdNodeGetContactForces(self._n, int(flags), *[_ptr(out.get(k)) for k, _ in _CF_KEYS]))
        return out

    def get_dynamics(self, flags=DYN_ALL):
        """Batch.update_dynamics(flags) on every device's own thread and stream, then the results of ALL instances in instance
        order, as Batch.get_dynamics() returns them"""
        out = _dyn_arrays(self.total, self.ndof, int(flags))
        self._chk(self._L.rkfdNodeGetDynamics(self._n, int(flags), *[_ptr(out.get(k)) for k, _ in _DYN_KEYS]))
        return out

    def gather(self):
        """one RCCL all-gather of the final {dis, vel}; returns them on the host, [total, ndof] each"""
        dis = np.empty((self.total, self.ndof)); vel = np.empty_like(dis)
        self._chk(self._L.rkfdNodeGather(self._n, _ptr(dis), _ptr(vel)))
        return dis, vel
