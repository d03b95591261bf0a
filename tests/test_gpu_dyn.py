"""The joint-space dynamics on the GPU (rkfdBatchUpdateDynamics, rkfd_dyn_kernel): the worlds of tests/test_emu_dyn.py at batch sizes
1, 3 and 130 against the two references of tests/dyn_cases.py on the first three and the last instance and against the emulator's
device code on every instance, to 1e-12 max( 1, |value|_inf ); symmetry and the zero pattern on every instance; closure of
M acc + h against the step's own accelerations; the kinetic energy against the read-out; stream order without a host wait;
determinism; that the launch changes no state; flags and refusals; zero-copy views; the node level.
Measured worst deviations on the GPU: profiles/r11_dyn_parity.txt."""
import os
import subprocess

import numpy as np
import pytest

import dyn_cases as dc
import eom_cases as ec
import instance_params as ip
import refmath as rm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def worlds(R, tmp_path_factory):
    """name -> case; the trees twice: raw (reference A) and with orthonormal frames (both references)"""
    tmp = tmp_path_factory.mktemp("dyn_trees")
    cs = dc.cases(R)
    for ortho in (False, True):
        tag = "_on" if ortho else ""
        cs.update({k + tag: c for k, c in dc.limit_tree_cases(R, tmp, ortho).items()})
        cs.update({k + tag: c for k, c in dc.random_tree_cases(R, tmp, ortho).items()})
    return cs


TREES = dc.LIMIT_TREES + [f"rand{300 + k}" for k in range(10)]
NAMES = dc.WORLDS + TREES + [t + "_on" for t in TREES]


def _dynamics(R, c, dis, vel, flags=dc.ALL, broken=None):
    b = R.Batch(c["world"], dis.shape[0], device=0, max_rigid=0)
    b.set_state(dis, vel)
    if broken is not None:
        b.set_broken(broken)
    b.update_dynamics(flags)
    return b, b.get_dynamics()


@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("name", NAMES)
def test_dynamics_match_the_references(R, oracle_cls, worlds, name, B):
    """130 leaves a partial last workgroup at four instances per workgroup (32 full ones and one of two) and fills the last one at
    two (65 workgroups); B = 1 and 3 are a partial workgroup alone.  Nothing is written past `batch`: the buffers hold exactly `batch`
    instances, and the last instance is compared like every other"""
    c = worlds[name]
    dis, vel, br = dc.tile(c, B)
    b, got = _dynamics(R, c, dis, vel, broken=br)
    assert got["M"].shape == (B, b.ndof, b.ndof) and got["h"].shape == got["g"].shape == (B, b.ndof)
    pick = sorted(set(list(range(min(B, 3))) + [B - 1]))
    cc = dict(c, dis=dis, vel=vel, broken=br)
    dc.check_world(R, oracle_cls, cc, got, f"{name} B={B}", idx=pick)
    dc.check(got, dc.emu_dyn(c["world"], dis, vel), f"{name} B={B} [emulator, every instance]")
    b.close()


def test_closure_against_the_step(R, oracle_cls, tmp_path_factory):
    """after set_state, set_motor_input, update_init, update(n), eval(False): M acc + h - actuator torques (less the rotor term, which
    RKFD_DYN_ROTOR put into M) is zero on every coordinate without joint friction and within the friction bound elsewhere"""
    tmp = tmp_path_factory.mktemp("dyn_eom")
    tol = ec.family_tolerance(R, oracle_cls, tmp, "free")
    n = 0
    for case in ec.CASES:
        if not case.name.startswith("free_"):
            continue
        su = case.build(R, tmp)
        b = R.Batch(su.world, ec.B, device=0, max_rigid=su.max_rigid)
        out, _ = ec.run(su, b)
        b.update_dynamics(dc.MASS | dc.BIAS | dc.ROTOR)
        d = b.get_dynamics()
        b.close()
        tb = ec.Tables(su.world.model.contents)
        worst = 0.0
        for i in range(ec.B):
            md = ec.model_of_instance(su, i)
            q, qd, qdd = out["dis"][i], out["vel"][i], out["acc"][i]
            inp = np.zeros(md["nlink"]) if su.motor_in is None else su.motor_in[i]
            t_act = rm.actuator_torque(md, qd, qdd, inp, rotor=False)
            t_dyn = d["M"][i] @ qdd + d["h"][i]
            r = t_dyn - t_act
            s = max(1.0, np.abs(t_dyn).max(initial=0.0), np.abs(t_act).max(initial=0.0))
            bound = ec.friction_bounds(md, tb, q, qd, out["piv"][i])
            for k in range(md["ndof"]):
                if bound[k] is None:
                    worst = max(worst, abs(r[k]) / s)
                    assert abs(r[k]) <= tol * s, (case.name, i, k, r[k], s, tol)
                else:
                    assert abs(r[k]) <= bound[k] + tol * s, (case.name, i, k, r[k], bound[k])
        print(f"closure {case.name:32s} worst {worst:.2e} allowed {tol:.2e}")
        n += 1
    assert n == 7


def test_energy_identity_against_the_readout(R, worlds):
    """0.5 vel' M vel equals sum 0.5 m | v + w x c |^2 + 0.5 w' I w of the read-out's link velocities at the same state"""
    c = worlds["humanoid30"]
    dis, vel, _ = dc.tile(c, 5)
    b, got = _dynamics(R, c, dis, vel, dc.MASS)
    b.update_links(R.LINKS_VEL)
    v = b.get_links()["v"]
    b.close()
    ms, cm, In = dc.params_of(c["world"], None, 0)
    vc = v[:, :, :3] + np.cross(v[:, :, 3:], cm[None])
    T = 0.5 * np.einsum("l,blk,blk->b", ms, vc, vc) + 0.5 * np.einsum("blj,ljk,blk->b", v[:, :, 3:], In, v[:, :, 3:])
    TM = 0.5 * np.einsum("ba,bac,bc->b", vel, got["M"], vel)
    assert T.min() > 0.1
    assert np.abs(T - TM).max() <= dc.TOL * max(1.0, np.abs(T).max()), np.abs(T - TM).max()


def test_stream_order_without_a_host_wait(R, oracle_cls):
    """update(5) under set_split(3), update_dynamics, get_dynamics - no status() / join in between - equals a second batch that waited"""
    B = 130
    sc = R.scenarios.config4(batch=B)
    out = []
    for wait in (False, True):
        b = R.Batch(sc["world"], B, device=0, max_rigid=sc["max_rigid"])
        b.set_split(3)
        b.set_state(sc["dis"], sc["vel"]); b.update_init(); b.update(5)
        if wait:
            assert b.status() == 0
        b.update_dynamics()
        out.append((b, b.get_dynamics()))
    for k in dc.KEYS:
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
    b = out[0][0]
    assert b.status() == 0
    dis, vel, _ = b.get_state()
    assert np.abs(dis - sc["dis"]).max() > 1e-6          # the steps were seen
    pick = [0, 1, 64, B - 1]
    dc.check({k: v[pick] for k, v in out[0][1].items()}, dc.reference_b(sc["world"], dis[pick], vel[pick]), "config4 after 5 steps")
    for x, _ in out:
        x.close()


def test_two_launches_are_bit_identical(R, worlds):
    for name in ("humanoid30", "chain64_fixed32"):
        c = worlds[name]
        dis, vel, _ = dc.tile(c, 130)
        b, first = _dynamics(R, c, dis, vel)
        ptrs = b.dynamics_ptrs()
        b.update_dynamics(); second = b.get_dynamics()
        assert b.dynamics_ptrs() == ptrs and all(ptrs)          # the buffers are stable
        for k in dc.KEYS:
            assert np.array_equal(first[k], second[k]), (name, k)
        b.close()


def _final(b):
    return tuple(b.get_state()) + tuple(b.get_contact()) + tuple(b.get_pivot())


@pytest.mark.parametrize("variant", ["generic", "specialized", "two_per_wave", "table"])
def test_dynamics_change_nothing(R, variant):
    """update(5); update_dynamics(); update(5) leaves, bit for bit, what update(10) leaves"""
    B = 9
    sc = R.scenarios.config3(batch=B) if variant == "two_per_wave" else R.scenarios.config4(batch=B)
    res = []
    for read in (False, True):
        b = R.Batch(sc["world"], B, device=0, max_rigid=sc["max_rigid"])
        if variant == "table":
            P = ip.randomised(sc["world"], B, seed=0xD713)
            for k in ("mass", "com", "inertia"):
                b.set_param(k, P[k])
        if variant == "two_per_wave":
            b.set_instances_per_wave(2)
        if variant in ("specialized", "two_per_wave"):
            b.specialize()
            assert b.instances_per_wave() == (2 if variant == "two_per_wave" else 1)
        b.set_state(sc["dis"], sc["vel"]); b.update_init()
        if read:
            b.update(5); b.update_dynamics(dc.ALL | dc.ROTOR); b.update(5)
            assert all(np.isfinite(v).all() for v in b.get_dynamics().values())
        else:
            b.update(10)
        assert b.status() == 0
        res.append(_final(b)); b.close()
    for k, (x, y) in enumerate(zip(*res)):
        assert np.array_equal(x, y), (variant, k)


def test_dynamics_with_a_parameter_table(R, oracle_cls, worlds):
    c = worlds["humanoid30"]
    dis, vel, _ = dc.tile(c, 5)
    P = {k: v for k, v in ip.randomised(c["world"], 5, seed=0xD712).items() if k in ("mass", "com", "inertia")}
    b, plain = _dynamics(R, c, dis, vel)
    for k in P:
        b.set_param(k, P[k])
    b.update_dynamics(); got = b.get_dynamics()
    cc = dict(c, dis=dis, vel=vel, broken=None)
    dc.check_world(R, oracle_cls, cc, got, "humanoid30 + table", par=P)
    dc.check(got, dc.emu_dyn(c["world"], dis, vel, par=P), "humanoid30 + table [emulator]")
    for k in dc.KEYS:
        assert np.abs(got[k] - plain[k]).max() > 1e-5, k
    P2 = dict(P, inertia=P["inertia"] * 1.5)                         # a later change of the table reaches the next launch
    b.set_param("inertia", P2["inertia"])
    b.update_dynamics(dc.MASS); again = b.get_dynamics()
    dc.check(again, dc.reference_b(c["world"], dis, vel, P2), "table changed", keys=("M",))
    b.clear_params(); b.update_dynamics(); back = b.get_dynamics()
    for k in dc.KEYS:
        assert np.array_equal(back[k], plain[k]), k
    b.close()


def test_flags_and_refusals(R, worlds, tmp_path):
    c = worlds["humanoid30"]
    m = c["world"].model.contents
    L = R.lib()
    err = lambda: L.rkfdHipLastError().decode()
    n = c["dis"].shape[0]
    b = R.Batch(c["world"], n, device=0, max_rigid=0)
    b.set_state(c["dis"], c["vel"])
    # a batch that never asked holds nothing
    assert b.dynamics_ptrs() == (None, None, None)
    assert L.rkfdBatchGetDynamics(b._b, np.zeros(1).ctypes.data, None, None) == -1 and "no dynamics have been computed" in err()
    with pytest.raises(R.RkfdError, match="no dynamics have been computed"):
        b.get_dynamics()
    for flags in (0, 16, 23, -1):
        assert L.rkfdBatchUpdateDynamics(b._b, flags, None) == -1 and "RKFD_DYN_MASS, RKFD_DYN_BIAS, RKFD_DYN_GRAVITY and RKFD_DYN_ROTOR" in err(), flags
    for flags in (dc.ROTOR, dc.ROTOR | dc.BIAS, dc.ROTOR | dc.BIAS | dc.GRAVITY):
        assert L.rkfdBatchUpdateDynamics(b._b, flags, None) == -1 and "RKFD_DYN_ROTOR without RKFD_DYN_MASS" in err(), flags
    assert b.dynamics_ptrs() == (None, None, None)
    b.update_dynamics(dc.GRAVITY)
    only = b.get_dynamics()
    assert set(only) == {"g"} and b.dynamics_ptrs()[0] is None and b.dynamics_ptrs()[1] is None and b.dynamics_ptrs()[2]
    Mbuf = np.zeros((n, m.ndof, m.ndof)); hbuf = np.zeros((n, m.ndof))
    assert L.rkfdBatchGetDynamics(b._b, Mbuf.ctypes.data, None, None) == -1 and "RKFD_DYN_MASS" in err()
    assert L.rkfdBatchGetDynamics(b._b, None, hbuf.ctypes.data, None) == -1 and "RKFD_DYN_BIAS" in err()
    assert L.rkfdBatchGetDynamics(b._b, None, None, None) == 0
    b.update_dynamics(); full = b.get_dynamics()
    pg = b.dynamics_ptrs()
    assert all(pg) and np.array_equal(full["g"], only["g"])
    b.update_dynamics(dc.MASS | dc.ROTOR); rot = b.get_dynamics()
    assert set(rot) == {"M"} and b.dynamics_ptrs() == pg
    assert L.rkfdBatchGetDynamics(b._b, None, None, hbuf.ctypes.data) == -1 and "RKFD_DYN_GRAVITY" in err()      # not part of the LAST launch
    diag = dc.rotor_diagonal(m)
    assert diag.max() > 0 and np.array_equal(rot["M"], full["M"] + np.diag(diag)[None])
    # snapshot / restore / reset leave the results alone
    b.update_dynamics(); b.snapshot()
    b.set_state(c["dis"][::-1].copy(), c["vel"][::-1].copy()); b.restore()
    b.bank_reserve(1); b.bank_store(0, 0, 1); b.reset(np.zeros(n, dtype=np.int32))
    after = b.get_dynamics()
    for k in dc.KEYS:
        assert np.array_equal(after[k], full[k]), k
    b.close()
    # (more than 64 joint coordinates: no batch can be built of such a world, so that refusal cannot be reached through a batch; the
    # emulator's harness applies the same rule, tests/test_emu_dyn.py)
    # a world whose single instance does not fit the LDS of a workgroup: refused at the first call, the message names the bytes
    w = dc.fixed_star(R, tmp_path, 420)
    m = w.model.contents
    b = R.Batch(w, 2, device=0, max_rigid=0)
    with pytest.raises(R.RkfdError, match=r"421 links and 1 joint coordinates needs %d bytes of LDS for one instance" % (8 * (51 * 421 + 6))):
        b.update_dynamics()
    assert b.dynamics_ptrs() == (None, None, None)
    b.close()
    # between: 150 and 300 fixed links run two and one instance per workgroup
    for nfixed in (150, 300):
        w2 = dc.fixed_star(R, tmp_path, nfixed)
        dis, vel = np.full((5, 1), 0.3), np.full((5, 1), 1.0)
        dis[:, 0] += 0.1 * np.arange(5)
        b2 = R.Batch(w2, 5, device=0, max_rigid=0)
        b2.set_state(dis, vel); b2.update_dynamics()
        dc.check(b2.get_dynamics(), dc.reference_b(w2, dis, vel), f"{nfixed} fixed links")
        b2.close()


_ZERO_COPY = r"""
import sys
ROOT = sys.argv[1]
sys.path[:0] = [ROOT, ROOT + "/tests", ROOT + "/tests/emu"]
import numpy as np
import torch
torch.cuda.init()      # torch's HIP runtime before the library's first call (as bench.py does)
import rkfd_pkg
import dyn_cases as dc
import jac_cases as jc
import links_cases as lc
R = rkfd_pkg.load()
c = jc.cases(R)["humanoid30"]
dis, vel = lc.states(c["world"], 130, 0x2D)
b = R.Batch(c["world"], 130, device=0, max_rigid=0)
assert b.dynamics_tensors() == {"M": None, "h": None, "g": None}
b.set_state(dis, vel); b.set_jacobian_sites(c["links"], c["points"]); b.update_jacobians(); b.update_dynamics()
got = b.get_dynamics(); J = b.get_jacobians()["J"]
# the other views keep their shapes
assert len(b.dev_tensors()) == 3 and len(b.dev_tensors(links=True)) == 8 and set(b.links_tensors()) == {"R", "p", "v", "com", "comvel"}
assert tuple(b.jacobian_tensors()["J"].shape) == J.shape
t = b.dynamics_tensors()
L = R.lib()
assert t["M"].data_ptr() == L.rkfdBatchDevMassMatrix(b._b) == b.dynamics_ptrs()[0]
assert t["h"].data_ptr() == L.rkfdBatchDevBias(b._b) == b.dynamics_ptrs()[1]
assert t["g"].data_ptr() == L.rkfdBatchDevGravity(b._b) == b.dynamics_ptrs()[2]
for k in dc.KEYS:
    assert t[k].dtype == torch.float64 and tuple(t[k].shape) == got[k].shape and np.array_equal(t[k].cpu().numpy(), got[k]), k
# forward dynamics of one instance on the device: qdd = M^-1 ( J' f - h ) for a force and moment on the first site
i = 7
f = np.array([3.0, -2.0, 40.0, 0.5, -0.25, 1.0])
Jt = b.jacobian_tensors()["J"]
rhs = torch.einsum("rc,r->c", Jt[i, 0], torch.as_tensor(f, device="cuda")) - t["h"][i]
dev = torch.linalg.solve(t["M"][i], rhs).cpu().numpy()
host = np.linalg.solve(got["M"][i], J[i, 0].T @ f - got["h"][i])
assert np.abs(dev - host).max() <= 1e-10 * max(1.0, np.abs(host).max()), np.abs(dev - host).max()
ptrs = b.dynamics_ptrs()
b.update_dynamics()
assert b.dynamics_ptrs() == ptrs      # stable
# the views alias the live buffers: the dynamics of another state show through them
b.set_state(dis[::-1].copy(), vel[::-1].copy()); b.update_dynamics(); g2 = b.get_dynamics()
assert np.array_equal(t["M"].cpu().numpy(), g2["M"]) and not np.array_equal(g2["M"], got["M"])
print("zero-copy ok")
"""


def test_zero_copy_views(R, tmp_path):
    """the torch views of dynamics_tensors() equal get_dynamics(), their pointers the C ones, and M^-1 ( J' f - h ) solved on them on
    the GPU equals the host value; in a process of its own, because torch's HIP runtime has to come up before the library's first call"""
    import sys
    f = tmp_path / "zero_copy_dyn.py"
    f.write_text(_ZERO_COPY)
    r = subprocess.run([sys.executable, str(f), ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "zero-copy ok" in r.stdout, r.stdout + r.stderr


def test_node_get_dynamics(R, worlds):
    c = worlds["humanoid30"]
    dis, vel, _ = dc.tile(c, 19)
    n = R.Node(c["world"], 19, max_rigid=0, devices=[0])
    n.set_state(dis, vel)
    got = n.get_dynamics()
    b, ref = _dynamics(R, c, dis, vel)
    for k in dc.KEYS:
        assert np.array_equal(got[k], ref[k]), k
    only = n.get_dynamics(dc.BIAS)
    assert set(only) == {"h"} and np.array_equal(only["h"], ref["h"])
    with pytest.raises(R.RkfdError, match="RKFD_DYN_ROTOR without RKFD_DYN_MASS"):
        n.get_dynamics(dc.ROTOR | dc.BIAS)
    b.close(); n.close()
