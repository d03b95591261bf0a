"""Which rigid-contact solve a step kernel runs, stated as plain Python, and scenes that reach each one.

The MLCP plugin's Gauss-Seidel and the Vert plugin's QP are sets of size-dependent paths picked inside the step kernel.  The
functions below restate those picks, each next to the device or host line it mirrors, so that a test can name the path a
world reaches and fail when the device no longer takes it.  tests/test_solver_paths.py checks the rules against the choices
the device-model builder reports (storage, Vert variant, LDS); tests/test_emu_solver_paths.py and
tests/test_gpu_solver_paths.py compare every path with the oracle."""
import ctypes as C
import os

import numpy as np

# ---------------------------------------------------------------------------------------------------------------- dispatch rules
PGS_NC = 4              # RKFD_PGS_NC        (roki-fd_amd/csrc/device/rkfd_dev_mlcp.h:11)
PGS_DPP_MAX = 16        # RKFD_PGS_DPP_MAX   (rkfd_dev_mlcp.h:84)
SW_MAXLEN = 8           # RKFD_SW_MAXLEN     (rkfd_dev_mlcp.h, sweep-order storage)
SW_DOUBLES = 8 * 9 * 32  # RKFD_SW_DOUBLES
QP_NQ_MAX = 24          # RKFD_QP_NQ_MAX     (unknowns whose QP factor lives in registers)
WAVE = 64
LDS_LIMIT = 160 * 1024  # rkfdBatchCreate refuses more per instance (rkfd_capi.hip)


def vert_variant(pyramid, max_rigid):
    """rkfdDevModel.vert_rigid of a Vert-plugin world with rigid contacts (rkfd_devmodel.cpp:617-627):
    2 - at most 24 unknowns, the QP's factor in registers; 3 - more unknowns or more pyramid faces than lanes, the wide form;
    1 - between, the factor in LDS"""
    v = 1
    if 3 * max_rigid <= QP_NQ_MAX:
        v = 2
    if 3 * max_rigid > WAVE or pyramid * max_rigid > WAVE:
        v = 3
    return v


def packing_considered(plugin, ipw, max_rigid):
    """whether the device-model builder weighs a packed lower triangle against full rows at all (rkfd_devmodel.cpp:722-728):
    PGS worlds only, and with one instance per wavefront only above 16 contacts (below, the DPP Gauss-Seidel exists for full
    rows only).  Where it is weighed, the triangle is taken when it lets one more instance share a CU."""
    return plugin == "mlcp" and max_rigid > 0 and not (ipw == 1 and max_rigid <= PGS_DPP_MAX)


def row_fills(comp_sizes):
    """rkfd_pgs_group_layout (rkfd_dev_mlcp.h:288-312): the connected components, largest first (equal sizes in the order
    found), each to the emptiest of four rows of 16.  -> the four row fills, or None where a component or a row would
    exceed 16 (fits = false)"""
    if any(s > PGS_DPP_MAX for s in comp_sizes):
        return None                                      # :288  BALLOT( mysize > 16 ) -> fits = false
    rows = [0, 0, 0, 0]
    for sz in range(PGS_DPP_MAX, 0, -1):                 # :289  for sz = 16 .. 1
        for s in comp_sizes:
            if s != sz:
                continue
            r = min(range(4), key=lambda i: rows[i])     # :295-298 the emptiest row, the first of equals
            if rows[r] + sz > PGS_DPP_MAX:               # :299
                return None
            rows[r] += sz
    return rows


def mlcp_path(nc, max_rigid, storage, ipw, comp_sizes, debug_variants=0):
    """the Gauss-Seidel a PGS evaluation with nc rigid contacts runs (rkfd_dev_mlcp.h:643-654 and :899-908).
    storage: "full" or "packed" (rkfdDevModel.ma_packed); comp_sizes: contacts per connected component (trees joined by
    contacts between moving links).  -> (path, detail) with detail the row fills of a grouped solve, else None"""
    assert sum(comp_sizes) == nc
    pk = storage == "packed"
    ma_size = 3 * max_rigid * (3 * max_rigid + 1) // 2 if pk else 9 * max_rigid * max_rigid
    fills = None
    # :644  grouped layout only above 16 contacts, for a capacity above 16, unless switched off (rkfdDebugVariants(8))
    if max_rigid > PGS_DPP_MAX and nc > PGS_DPP_MAX and not debug_variants & 8:
        fills = row_fills(comp_sizes)
    # :654  sweep-order storage: rows of at most 8 contacts, unless switched off (rkfdDebugVariants(32))
    sw = fills is not None and max(fills) <= SW_MAXLEN and ma_size >= SW_DOUBLES and not debug_variants & 32
    if nc <= PGS_NC:                                     # :899
        return "registers", None
    if nc == 8:                                          # :900
        return "dpp8", None
    if (not pk or ipw == 2) and nc <= PGS_DPP_MAX:       # :901
        return ("dpp_packed" if pk else "dpp_full"), None
    if fills is not None:                                # :902-906
        return ("grouped_sw" if sw else "grouped_packed" if pk else "grouped_full"), tuple(fills)
    return ("general_packed" if pk else "general_full"), None     # :908


def probe_passes(nc, ipw=1):
    """probe columns go 64 at a time (32 with two instances per wavefront): M = 3 nc columns (rkfd_dev_mlcp.h:660)"""
    wl = WAVE // ipw
    return -(-3 * nc // wl)


def row_stride(nc, max_rigid, vert=False):
    """ld of the full-row matrix: odd (M+1) unless every contact slot is taken (rkfd_dev_mlcp.h:583)"""
    M = 3 * nc
    return M + 1 if (vert or nc < max_rigid) else M


def vert_mfma_tiles(nc, pyramid, max_rigid, mfma=True):
    """the MFMA Gram product of the Vert QP (rkfd_dev_vertqp.h:180-223, called at :269 from the narrow QP, variants 1 and
    2): n = 3 nc <= 32; tile c00 alone for n <= 16, c01 / c11 as well for n 17 - 32.  -> the tiles, () where it is not used"""
    n = 3 * nc
    if not mfma or vert_variant(pyramid, max_rigid) == 3 or n > 32 or n == 0:
        return ()
    return ("c00",) if n <= 16 else ("c00", "c01", "c11")


# ------------------------------------------------------------------------------------------- what the device-model builder picks
def devmodel_layout(model, max_rigid, ipw=1):
    """(vert_rigid, ma_packed, ma_size, lds_bytes, lds_shared) the device-model builder picks for a world, read through the
    lane emulator's harness, which links the same builder (tests/emu/rkfd_emu.cpp: rkfd_emu_layout).  None when it refuses."""
    import emu
    L = emu.lib()
    L.rkfd_emu_layout.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    out = (C.c_int * 5)()
    if L.rkfd_emu_layout(C.cast(model, C.c_void_p), int(max_rigid), 8 // ipw, out) < 0:
        return None
    return tuple(out)


# -------------------------------------------------------------------------------------------------------------------- scenes
SEAT_DEPTH = 1.0e-5     # as roki-fd_amd/scenarios.py: resting vertices are seated this deep, so that bodies stay down


def _aa(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    return a / np.linalg.norm(a) * angle


# the poses a box may take on the floor, and the contact vertices each gives
POSES = {
    "flat": (None, 4),
    "edge": (_aa((1.0, 0.0, 0.0), 0.3), 2),             # rolled about x: one bottom edge down
    "vertex": (_aa((1.0, 1.0, 0.0), 0.35), 1),          # tipped about the diagonal: one corner down
}


def wide_box_ztk(width=0.6, depth=0.6, height=0.05, mass=2.0):
    """a wide flat box (one float link, stuff 'body'): a table for small boxes"""
    ix = mass * (width ** 2 + height ** 2) / 12.0
    iy = mass * (depth ** 2 + height ** 2) / 12.0
    iz = mass * (width ** 2 + depth ** 2) / 12.0
    return f"""[roki::chain]
name : wide_box

[zeo::shape]
type : box
name : shape
depth : {depth}
width : {width}
height : {height}

[roki::link]
name : link#00
jointtype : float
mass : {mass}
stuff : body
inertia : {{
 {ix}, 0, 0
 0, {iy}, 0
 0, 0, {iz}
}}
shape : shape
"""


def _seat(R, m, dis, chain, off, base):
    """lower chain `chain` (dofs at off) so that its lowest vertex is SEAT_DEPTH below `base`"""
    dis[off + 2] += base - SEAT_DEPTH - R.scenarios.lowest_vertex_z(m, dis, chain)


def box_scene(R, poses, solver="mlcp", pyramid=None, spacing=0.3):
    """boxes (box.ztk) on the floor, one per entry of `poses` ("flat" / "edge" / "vertex"), in a row-major grid of
    `spacing`: every box is a component of its own.  -> (world, dis [ndof], vel [ndof], expected contacts per component)"""
    M = R.scenarios.MODELS
    w = R.World(solver=R.SOLVER_MLCP if solver == "mlcp" else R.SOLVER_VERT)
    w.contact_info(os.path.join(M, "contactinfo.ztk"))
    if pyramid is not None:
        w.set_pyramid(pyramid)
    ch = [w.reg_file(os.path.join(M, "box.ztk")) for _ in poses]
    w.reg_file(os.path.join(M, "floor.ztk"))
    m = w.model.contents
    dis = np.zeros(m.ndof)
    ncol = int(np.ceil(np.sqrt(len(poses))))
    for k, (c, p) in enumerate(zip(ch, poses)):
        o = w.dof_offset(c)
        dis[o:o + 2] = ((k % ncol) - (ncol - 1) / 2) * spacing, ((k // ncol) - (ncol - 1) / 2) * spacing
        aa = POSES[p][0]
        if aa is not None:
            dis[o + 3:o + 6] = aa
        dis[o + 2] = 0.05
        _seat(R, m, dis, c, o, 0.0)
    return w, dis, np.zeros(m.ndof), [POSES[p][1] for p in poses]


def table_scene(R, tmp_path, nsmall, loose=(), solver="mlcp"):
    """a wide flat box on the floor with `nsmall` box_small.ztk resting on it (one component of 4 + 4 nsmall contacts: the
    small boxes touch the table, the table the floor), and boxes on the floor beside it (`loose`: their poses)"""
    M = R.scenarios.MODELS
    f = tmp_path / "wide_box.ztk"
    f.write_text(wide_box_ztk())
    w = R.World(solver=R.SOLVER_MLCP if solver == "mlcp" else R.SOLVER_VERT)
    w.contact_info(os.path.join(M, "contactinfo.ztk"))
    t = w.reg_file(f)
    sm = [w.reg_file(os.path.join(M, "box_small.ztk")) for _ in range(nsmall)]
    lo = [w.reg_file(os.path.join(M, "box.ztk")) for _ in loose]
    w.reg_file(os.path.join(M, "floor.ztk"))
    m = w.model.contents
    dis = np.zeros(m.ndof)
    to = w.dof_offset(t)
    dis[to + 2] = 0.05
    _seat(R, m, dis, t, to, 0.0)
    top = R.scenarios.chain_vertices(m, dis, t)[:, 2].max()
    # small boxes on a grid inside the 0.6 x 0.6 table top, 0.15 apart
    for k, c in enumerate(sm):
        o = w.dof_offset(c)
        dis[o:o + 2] = ((k % 3) - 1) * 0.18, ((k // 3) - 1) * 0.18
        dis[o + 2] = top + 0.05
        _seat(R, m, dis, c, o, top)
    for k, (c, p) in enumerate(zip(lo, loose)):
        o = w.dof_offset(c)
        dis[o:o + 2] = 0.6 + 0.3 * k, 0.0
        aa = POSES[p][0]
        if aa is not None:
            dis[o + 3:o + 6] = aa
        dis[o + 2] = 0.05
        _seat(R, m, dis, c, o, 0.0)
    return w, dis, np.zeros(m.ndof), [4 + 4 * nsmall] + [POSES[p][1] for p in loose]


# ------------------------------------------------------------------------------------------- contacts of an oracle evaluation
def contact_components(model, active):
    """contacts per connected component of an evaluation: `active` the candidates in rigid contact (oracle get_contact),
    a component the chains joined by contacts between two moving chains; a chain all of whose joints are fixed is static.
    Sizes in the order of the components' first contacts."""
    m = model.contents
    nl = m.nlink
    chain = m.arr("chain", nl); jtype = m.arr("jtype", nl)
    pair_shape = m.arr("pair_shape", 2 * m.npair).reshape(-1, 2)
    shape_link = m.arr("shape_link", m.nshape)
    cand_pair = m.arr("cand_pair", m.ncand)
    static = {c for c in set(chain.tolist()) if all(jtype[chain == c] == 0)}
    par = {}

    def find(x):
        while par.setdefault(x, x) != x:
            x = par[x]
        return x
    owner = []
    for j in np.flatnonzero(np.asarray(active) != 0):
        a, b = (int(chain[shape_link[s]]) for s in pair_shape[cand_pair[j]])
        mv = [c for c in (a, b) if c not in static]
        for c in mv[1:]:
            par[find(c)] = find(mv[0])
        owner.append(mv[0])
    sizes = {}
    for c in owner:
        r = find(c)
        sizes[r] = sizes.get(r, 0) + 1
    return list(sizes.values())


# ---------------------------------------------------------------------------------------------------------------------- cases
# one world per path: (scene, its arguments, plugin, pyramid, max_rigid, instances per wavefront, the path, contacts).
# scene "boxes": box_scene(poses); "table": table_scene(small boxes on the table, poses of the boxes beside it).
# Vert cases name the variant ("vert1" / "vert2" / "vert3") and the MFMA tiles of the Gram product.
class Case:
    def __init__(self, name, scene, arg, plugin, cap, path, nc, ipw=1, pyramid=None, rows=None, tiles=None):
        self.name, self.scene, self.arg, self.plugin, self.cap, self.path, self.nc = name, scene, arg, plugin, cap, path, nc
        self.ipw, self.pyramid, self.rows, self.tiles = ipw, pyramid, rows, tiles

    def __repr__(self):
        return self.name

    def build(self, R, tmp_path):
        if self.scene == "boxes":
            return box_scene(R, self.arg, solver=self.plugin, pyramid=self.pyramid)
        return table_scene(R, tmp_path, self.arg[0], loose=self.arg[1], solver=self.plugin)


F, E, V = "flat", "edge", "vertex"
CASES = [
    Case("mlcp_registers_nc4", "boxes", [F], "mlcp", 4, "registers", 4),
    Case("mlcp_dpp8_nc8", "boxes", [F, F], "mlcp", 8, "dpp8", 8),
    Case("mlcp_dpp_full_nc5", "boxes", [F, V], "mlcp", 8, "dpp_full", 5),
    Case("mlcp_dpp_full_nc7", "boxes", [F, E, V], "mlcp", 8, "dpp_full", 7),
    Case("mlcp_dpp_full_nc9", "boxes", [F, F, V], "mlcp", 16, "dpp_full", 9),
    Case("mlcp_dpp_full_nc12_even_stride", "boxes", [F, F, F], "mlcp", 12, "dpp_full", 12),
    Case("mlcp_dpp_full_nc16_even_stride", "boxes", [F, F, F, F], "mlcp", 16, "dpp_full", 16),
    Case("mlcp_dpp_packed_ipw2_nc5", "boxes", [F, V], "mlcp", 5, "dpp_packed", 5, ipw=2),
    Case("mlcp_dpp_packed_ipw2_nc7", "boxes", [F, E, V], "mlcp", 7, "dpp_packed", 7, ipw=2),
    Case("mlcp_dpp_packed_ipw2_nc9", "boxes", [F, F, V], "mlcp", 9, "dpp_packed", 9, ipw=2),
    Case("mlcp_dpp_packed_ipw2_nc12", "boxes", [F, F, F], "mlcp", 12, "dpp_packed", 12, ipw=2),
    Case("mlcp_dpp_packed_ipw2_nc16", "boxes", [F, F, F, F], "mlcp", 16, "dpp_packed", 16, ipw=2),
    Case("mlcp_general_packed_nc5", "boxes", [F, V], "mlcp", 24, "general_packed", 5),
    Case("mlcp_general_packed_nc9", "boxes", [F, F, V], "mlcp", 24, "general_packed", 9),
    Case("mlcp_general_packed_nc12", "boxes", [F, F, F], "mlcp", 24, "general_packed", 12),
    Case("mlcp_grouped_sw_4rows_nc32", "boxes", [F] * 8, "mlcp", 32, "grouped_sw", 32, rows=(8, 8, 8, 8)),
    Case("mlcp_grouped_packed_row12_nc20", "table", (2, (F, F)), "mlcp", 24, "grouped_packed", 20, rows=(12, 4, 4, 0)),
    Case("mlcp_grouped_full_nc40_even_stride", "boxes", [F] * 10, "mlcp", 40, "grouped_full", 40, rows=(12, 12, 8, 8)),
    Case("mlcp_grouped_full_nc40_lds_edge", "boxes", [F] * 10, "mlcp", 42, "grouped_full", 40, rows=(12, 12, 8, 8)),
    Case("mlcp_general_packed_one_component_nc20", "table", (4, ()), "mlcp", 20, "general_packed", 20),
    Case("mlcp_general_packed_one_component_nc36", "table", (8, ()), "mlcp", 36, "general_packed", 36),
    Case("mlcp_general_full_one_component_nc24", "table", (5, ()), "mlcp", 42, "general_full", 24),
    Case("vert2_mfma_c00_n15", "boxes", [F, V], "vert", 8, "vert2", 5, tiles=("c00",)),
    Case("vert2_mfma_c11_n18", "boxes", [F, E], "vert", 8, "vert2", 6, tiles=("c00", "c01", "c11")),
    Case("vert1_pyr4_mfma_n27", "boxes", [F, F, V], "vert", 9, "vert1", 9, pyramid=4, tiles=("c00", "c01", "c11")),
    Case("vert1_pyr6_mfma_n30", "boxes", [F, F, E], "vert", 10, "vert1", 10, pyramid=6, tiles=("c00", "c01", "c11")),
    Case("vert1_pyr4_nc12", "boxes", [F, F, F], "vert", 16, "vert1", 12, pyramid=4, tiles=()),
    Case("vert3_wide_nc6", "boxes", [F, E], "vert", 24, "vert3", 6, tiles=()),
]
CASE_IDS = [c.name for c in CASES]


def observed_path(R, case, world, comps, nc, debug_variants=0):
    """the path the helper names for what the builder picked and the oracle's contacts"""
    vr, packed, _, _, _ = devmodel_layout(world.model, case.cap, case.ipw)
    if case.plugin == "vert":
        return "vert%d" % vr
    return mlcp_path(nc, case.cap, "packed" if packed else "full", case.ipw, comps, debug_variants)[0]


# ---------------------------------------------------------------------------------------------------------- oracle comparison
TOL_STATE = 1e-9        # dis / vel, relative to max(1, |oracle|)
TOL_ACC = 1e-8          # acc and contact forces


def rel(x, y):
    return float(np.abs(x - y).max() / max(1.0, np.abs(y).max()))


def states(dis, vel, B):
    """B instances of a scene's state: instance i slides its first body along x at 2 i mm/s (same contacts, other forces)"""
    d = np.tile(dis, (B, 1)); v = np.tile(vel, (B, 1))
    v[:, 0] += 0.002 * np.arange(B)
    return d, v


def oracles(world, dis, vel):
    """one oracle per instance, after its first evaluation (rkFDUpdateInit)"""
    from oracle.pyoracle import Oracle
    out = []
    for i in range(dis.shape[0]):
        o = Oracle(world.model)
        o.set_state(dis[i], vel[i])
        o.update_init()
        out.append(o)
    return out


def compare(batch, ors, what):
    """the batch's state and contacts against one oracle per instance, at the suite's tolerances; -> the largest relative
    error seen (dis, vel, acc, forces)"""
    dis, vel, acc = batch.get_state()
    act, typ, ref, f = batch.get_contact()
    worst = 0.0
    for i, o in enumerate(ors):
        od, ov, oa = o.get_state()
        oact, otyp, _, of = o.get_contact()
        on = oact != 0
        assert (act[i] == oact).all(), f"{what}: instance {i}: contact set differs from the oracle"
        assert (typ[i] == otyp * on).all(), f"{what}: instance {i}: stick / slip set differs from the oracle"
        e = (rel(dis[i], od), rel(vel[i], ov), rel(acc[i], oa), rel(f[i], of * on[:, None]))
        assert e[0] < TOL_STATE and e[1] < TOL_STATE, f"{what}: instance {i}: dis / vel differ from the oracle by {e[:2]}"
        assert e[2] < TOL_ACC and e[3] < TOL_ACC, f"{what}: instance {i}: acc / forces differ from the oracle by {e[2:]}"
        worst = max(worst, *e)
    return worst


def check_path(R, case, world, oracle, debug_variants=0):
    """the oracle's first evaluation holds case.nc rigid contacts and the helper names case.path for them: a world that
    reaches another path fails here, not silently elsewhere.  -> contacts per component"""
    act = oracle.get_contact()[0]
    comps = contact_components(world.model, act)
    nc = int((act != 0).sum())
    assert nc == case.nc, f"{case.name}: {nc} contacts, expected {case.nc}"
    if case.plugin == "mlcp":
        assert oracle.mlcp()[0] == nc
    assert observed_path(R, case, world, comps, nc, debug_variants) == case.path
    if case.rows is not None:
        assert mlcp_path(nc, case.cap, "full", case.ipw, comps)[1] == case.rows
    if case.tiles is not None:
        assert vert_mfma_tiles(nc, case.pyramid or 8, case.cap) == case.tiles
    return comps
