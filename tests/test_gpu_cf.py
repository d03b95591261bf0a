"""The contact read-out on the GPU (rkfdBatchUpdateContactForces[Dev], rkfd_cf_kernel): the worlds of tests/test_emu_cf.py at batch
sizes 1, 3 and 130 through update_contact_forces(active=, f=) against the references of tests/cf_cases.py on the first three and the
last instance and against the emulator's device code on every instance, to 1e-12 max( 1, |value|_inf ); closure of the equation of
motion M acc + h - genf - actuator torques on every eom_cases case with contacts; the batch's own forces against the numpy sum over
get_contact() and get_links(); stream order without a host wait; determinism; that the launch changes no state; flags and refusals;
zero-copy views; the node level.  Measured worst deviations on the GPU: profiles/r12_cf_parity.txt."""
import os
import subprocess

import numpy as np
import pytest

import cf_cases as cc
import dyn_cases as dc
import eom_cases as ec
import instance_params as ip
import refmath as rm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def worlds(R, tmp_path_factory):
    return cc.cases(R, tmp_path_factory.mktemp("cf_worlds"))


def _read_out(R, c, flags=cc.ALL, f=None):
    """a batch at the case's states, one launch on the case's (or the given) forces handed over on the device -> (batch, results)"""
    B = c["dis"].shape[0]
    b = R.Batch(c["world"], B, device=0, max_rigid=0)
    b.set_state(c["dis"], np.zeros_like(c["dis"]))
    da, df = cc.DevArray(R, c["active"]), cc.DevArray(R, c["f"] if f is None else f)
    b.update_contact_forces(flags, active=da, f=df)
    got = b.get_contact_forces()
    da.free(); df.free()
    return b, got


@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("name", cc.WORLDS)
def test_contact_forces_match_the_references(R, oracle_cls, worlds, name, B):
    """130 leaves a partial last workgroup at four instances per workgroup (32 full ones and one of two); B = 1 and 3 are a partial
    workgroup alone.  The buffers hold exactly `batch` instances, and the last instance is compared like every other"""
    c = cc.tile(worlds[name], B)
    b, got = _read_out(R, c)
    m = c["world"].model.contents
    assert got["point"].shape == (B, m.ncand, 3) and got["wrench"].shape == (B, m.nlink, 6) and got["count"].shape == (B, m.nlink) and got["genf"].shape == (B, m.ndof)
    assert got["count"].dtype == np.int32
    pick = sorted(set(list(range(min(B, 3))) + [B - 1]))
    cc.check_world(R, oracle_cls, c, got, f"{name} B={B}", idx=pick)
    cc.check(got, cc.emu_cf(c["world"], c["dis"], c["active"], c["f"]), f"{name} B={B} [emulator, every instance]")

    def rerun(f2):
        b2, g2 = _read_out(R, c, f=f2)
        b2.close()
        return g2
    cc.check_properties(c["world"], c["cand"], c["dis"], c["active"], c["f"], got, rerun, f"{name} B={B}")
    b.close()


@pytest.mark.parametrize("case", [c for c in ec.CASES if c.contacts], ids=lambda c: c.name)
def test_closure_of_the_equation_of_motion(R, oracle_cls, tmp_path_factory, case):
    """after ec.run: M acc + h - genf - actuator torques (less the rotor term, which RKFD_DYN_ROTOR put into M), with genf from the
    batch's own contact forces, is zero on every coordinate without joint friction and within the friction bound elsewhere"""
    tmp = tmp_path_factory.mktemp("cf_eom")
    tol = ec.family_tolerance(R, oracle_cls, tmp, case.family)
    su = case.build(R, tmp)
    b = R.Batch(su.world, ec.B, device=0, max_rigid=su.max_rigid)
    ec.apply_params(b, su)
    out, _ = ec.run(su, b)
    b.update_dynamics(dc.MASS | dc.BIAS | dc.ROTOR)
    b.update_contact_forces(cc.GENF)
    d = b.get_dynamics(); genf = b.get_contact_forces()["genf"]
    b.close()
    tb = ec.Tables(su.world.model.contents)
    worst = 0.0
    for i in range(ec.B):
        assert int(out["act"][i].sum()) >= su.min_active, f"instance {i}: {int(out['act'][i].sum())} active contacts, expected at least {su.min_active}"
        md = ec.model_of_instance(su, i)
        q, qd, qdd = out["dis"][i], out["vel"][i], out["acc"][i]
        inp = np.zeros(md["nlink"]) if su.motor_in is None else su.motor_in[i]
        t_act = rm.actuator_torque(md, qd, qdd, inp, rotor=False)
        t_dyn = d["M"][i] @ qdd + d["h"][i]
        r = t_dyn - genf[i] - t_act
        s = max(1.0, np.abs(t_dyn).max(initial=0.0), np.abs(genf[i]).max(initial=0.0), np.abs(t_act).max(initial=0.0))
        bound = ec.friction_bounds(md, tb, q, qd, out["piv"][i])
        for k in range(md["ndof"]):
            if bound[k] is None:
                worst = max(worst, abs(r[k]) / s)
                assert abs(r[k]) <= tol * s, (case.name, i, k, r[k], s, tol)
            else:
                assert abs(r[k]) <= bound[k] + tol * s, (case.name, i, k, r[k], bound[k])
    assert np.abs(genf).max() > 0.0
    print(f"closure {case.name:32s} worst {worst:.2e} allowed {tol:.2e}")


@pytest.mark.parametrize("name", ["config4", "stacked_boxes"])
def test_the_batchs_own_forces(R, tmp_path, name):
    """after update(n): get_contact_forces() equals the numpy sum over get_contact() and get_links()"""
    if name == "config4":
        sc = R.scenarios.config4(batch=3); w, dis, vel, mr, n = sc["world"], sc["dis"], sc["vel"], sc["max_rigid"], 3
    else:
        su = ec._stack(R, tmp_path); w, dis, vel, mr, n = su.world, su.dis, su.vel, su.max_rigid, 2
    b = R.Batch(w, 3, device=0, max_rigid=mr)
    b.set_state(dis, vel); b.update_init(); b.update(n)
    b.update_contact_forces(); b.update_links(R.LINKS_POSE)
    got = b.get_contact_forces()
    assert b.status() == 0
    act, _, _, f = b.get_contact(); lk = b.get_links()
    assert act.sum() >= 8
    cand = cc.model_cand(w)
    m = w.model.contents
    ref = {"point": np.zeros((3, cand.n, 3)), "wrench": np.zeros((3, m.nlink, 6)), "count": np.zeros((3, m.nlink), dtype=np.int32)}
    for i in range(3):
        for j in range(cand.n):
            o, t = cand.own[j], cand.other[j]
            x = lk["p"][i, o] + lk["R"][i, o] @ cand.vert[j]
            ref["point"][i, j] = x
            if act[i, j]:
                ref["wrench"][i, o, :3] += f[i, j]; ref["wrench"][i, o, 3:] += np.cross(x - lk["p"][i, o], f[i, j])
                ref["wrench"][i, t, :3] -= f[i, j]; ref["wrench"][i, t, 3:] -= np.cross(x - lk["p"][i, t], f[i, j])
                ref["count"][i, o] += 1; ref["count"][i, t] += 1
    cc.check(got, ref, f"{name} own forces")
    dis2, _, _ = b.get_state()
    cc.check(got, {"genf": cc.reference_b(w, cand, dis2, act, f)}, f"{name} own forces [B]")
    assert np.abs(got["genf"]).max() > 1.0
    b.close()


def test_stream_order_without_a_host_wait(R):
    """update(5) under set_split(3), update_contact_forces, get_contact_forces - no status() / join in between - equals a second batch
    that waited"""
    B = 130
    sc = R.scenarios.config4(batch=B)
    out = []
    for wait in (False, True):
        b = R.Batch(sc["world"], B, device=0, max_rigid=sc["max_rigid"])
        b.set_split(3)
        b.set_state(sc["dis"], sc["vel"]); b.update_init(); b.update(5)
        if wait:
            assert b.status() == 0
        b.update_contact_forces()
        out.append((b, b.get_contact_forces()))
    for k in cc.KEYS:
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
    b = out[0][0]
    assert b.status() == 0
    dis, _, _ = b.get_state()
    act, _, _, f = b.get_contact()
    assert np.abs(dis - sc["dis"]).max() > 1e-6 and act.sum() >= 8 * B          # the steps were seen
    pick = [0, 1, 64, B - 1]
    cand = cc.model_cand(sc["world"])
    cc.check({k: v[pick] for k, v in out[0][1].items()}, cc.numpy_sum(sc["world"], cand, dis[pick], act[pick], f[pick]), "config4 after 5 steps")
    for x, _ in out:
        x.close()


@pytest.mark.parametrize("split", [1, 3])
def test_a_writer_after_the_launch_waits_for_its_stream(R, split):
    """the launch on a stream made with hipStreamNonBlocking, which the null stream of the accessors' copies is not ordered against:
    set_state right behind it must wait for the launch (it is the batch's last launch), so the read-out is that of the stepped state"""
    import ctypes
    L = R.lib()
    h = ctypes.c_void_p()
    assert L.hipStreamCreateWithFlags(ctypes.byref(h), 1) == 0 and h.value      # (1: hipStreamNonBlocking)
    s = h.value
    B = 130
    sc = R.scenarios.config4(batch=B)
    out = []
    for wait in (False, True):
        b = R.Batch(sc["world"], B, device=0, max_rigid=sc["max_rigid"])
        b.set_split(split)
        b.set_state(sc["dis"], sc["vel"]); b.update_init(s); b.update(5, s)
        b.update_contact_forces(stream=s)
        if wait:
            assert b.status(s) == 0
        b.set_state(sc["dis"][::-1].copy() + 0.01, sc["vel"])
        out.append(b.get_contact_forces())
        assert b.status(s) == 0
        b.close()
    for k in cc.KEYS:
        assert np.array_equal(out[0][k], out[1][k]), k
    assert np.abs(out[0]["genf"]).max() > 1.0
    assert L.hipStreamDestroy(ctypes.c_void_p(s)) == 0


def test_two_launches_are_bit_identical(R, worlds):
    for name in ("humanoid30_shell", "config5"):
        c = cc.tile(worlds[name], 130)
        b, first = _read_out(R, c)
        ptrs = b.contact_force_ptrs()
        da, df = cc.DevArray(R, c["active"]), cc.DevArray(R, c["f"])
        b.update_contact_forces(active=da, f=df); second = b.get_contact_forces()
        da.free(); df.free()
        assert b.contact_force_ptrs() == ptrs and all(ptrs)          # the buffers are stable
        for k in cc.KEYS:
            assert np.array_equal(first[k], second[k]), (name, k)
        b.close()


def _final(b):
    return tuple(b.get_state()) + tuple(b.get_contact()) + tuple(b.get_pivot())


@pytest.mark.parametrize("variant", ["generic", "specialized", "two_per_wave", "table"])
def test_contact_forces_change_nothing(R, variant):
    """update(5); update_contact_forces(); update(5) leaves, bit for bit, what update(10) leaves"""
    B = 9
    sc = R.scenarios.config3(batch=B) if variant == "two_per_wave" else R.scenarios.config4(batch=B)
    res = []
    for read in (False, True):
        b = R.Batch(sc["world"], B, device=0, max_rigid=sc["max_rigid"])
        if variant == "table":
            P = ip.randomised(sc["world"], B, seed=0xCF13)
            for k in ("mass", "com", "inertia"):
                b.set_param(k, P[k])
        if variant == "two_per_wave":
            b.set_instances_per_wave(2)
        if variant in ("specialized", "two_per_wave"):
            b.specialize()
            assert b.instances_per_wave() == (2 if variant == "two_per_wave" else 1)
        b.set_state(sc["dis"], sc["vel"]); b.update_init()
        if read:
            b.update(5); b.update_contact_forces(); b.update(5)
            assert all(np.isfinite(v).all() for v in b.get_contact_forces().values())
        else:
            b.update(10)
        assert b.status() == 0
        res.append(_final(b)); b.close()
    for k, (x, y) in enumerate(zip(*res)):
        assert np.array_equal(x, y), (variant, k)


def test_flags_and_refusals(R, worlds):
    c = worlds["config5"]
    m = c["world"].model.contents
    L = R.lib()
    err = lambda: L.rkfdHipLastError().decode()
    n = c["dis"].shape[0]
    b = R.Batch(c["world"], n, device=0, max_rigid=0)
    b.set_state(c["dis"], np.zeros_like(c["dis"]))
    # a batch that never asked holds nothing
    assert b.contact_force_ptrs() == (None, None, None, None)
    assert L.rkfdBatchGetContactForces(b._b, np.zeros(1).ctypes.data, None, None, None) == -1 and "no contact forces have been computed" in err()
    with pytest.raises(R.RkfdError, match="no contact forces have been computed"):
        b.get_contact_forces()
    da, df = cc.DevArray(R, c["active"]), cc.DevArray(R, c["f"])
    pa, pf = da.__cuda_array_interface__["data"][0], df.__cuda_array_interface__["data"][0]
    for flags in (0, 8, 15, -1):
        assert L.rkfdBatchUpdateContactForces(b._b, flags, None) == -1 and "RKFD_CF_POINT, RKFD_CF_WRENCH and RKFD_CF_GENF" in err(), flags
        assert L.rkfdBatchUpdateContactForcesDev(b._b, flags, pa, pf, None) == -1 and "RKFD_CF_POINT, RKFD_CF_WRENCH and RKFD_CF_GENF" in err(), flags
    assert L.rkfdBatchUpdateContactForcesDev(b._b, 7, pa, None, None) == -1 and "null f_dev" in err()
    assert L.rkfdBatchUpdateContactForcesDev(b._b, 7, None, pf, None) == -1 and "null active_dev" in err()
    with pytest.raises(ValueError, match="f is missing"):
        b.update_contact_forces(active=da)
    with pytest.raises(ValueError, match="active is missing"):
        b.update_contact_forces(f=df)
    with pytest.raises(TypeError):
        b.update_contact_forces(active=c["active"], f=c["f"])          # host arrays are no device arrays
    assert b.contact_force_ptrs() == (None, None, None, None)
    b.update_contact_forces(cc.GENF, active=da, f=df)
    only = b.get_contact_forces()
    p = b.contact_force_ptrs()
    assert set(only) == {"genf"} and p[:3] == (None, None, None) and p[3]
    pbuf = np.zeros((n, m.ncand, 3)); wbuf = np.zeros((n, m.nlink, 6)); cbuf = np.zeros((n, m.nlink), dtype=np.int32); gbuf = np.zeros((n, m.ndof))
    assert L.rkfdBatchGetContactForces(b._b, pbuf.ctypes.data, None, None, None) == -1 and "RKFD_CF_POINT" in err()
    assert L.rkfdBatchGetContactForces(b._b, None, wbuf.ctypes.data, None, None) == -1 and "RKFD_CF_WRENCH" in err()
    assert L.rkfdBatchGetContactForces(b._b, None, None, cbuf.ctypes.data, None) == -1 and "RKFD_CF_WRENCH" in err()
    assert L.rkfdBatchGetContactForces(b._b, None, None, None, None) == 0
    b.update_contact_forces(active=da, f=df); full = b.get_contact_forces()
    pg = b.contact_force_ptrs()
    assert all(pg) and pg[3] == p[3] and np.array_equal(full["genf"], only["genf"])
    b.update_contact_forces(cc.POINT | cc.WRENCH, active=da, f=df); pw = b.get_contact_forces()
    assert set(pw) == {"point", "wrench", "count"} and b.contact_force_ptrs() == pg
    assert all(np.array_equal(pw[k], full[k]) for k in pw)
    assert L.rkfdBatchGetContactForces(b._b, None, None, None, gbuf.ctypes.data) == -1 and "RKFD_CF_GENF" in err()      # not part of the LAST launch
    # snapshot / restore / reset leave the results alone
    b.update_contact_forces(active=da, f=df); b.snapshot()
    b.set_state(c["dis"][::-1].copy(), np.zeros_like(c["dis"])); b.restore()
    b.bank_reserve(1); b.bank_store(0, 0, 1); b.reset(np.zeros(n, dtype=np.int32))
    after = b.get_contact_forces()
    for k in cc.KEYS:
        assert np.array_equal(after[k], full[k]), k
    da.free(); df.free()
    b.close()
    # a world under the Volume plugin: refused at the first call, nothing allocated
    w = R.World(solver=R.SOLVER_VOLUME); w.contact_info(os.path.join(R.scenarios.MODELS, "contactinfo.ztk"))
    w.reg_file(os.path.join(R.scenarios.MODELS, "box.ztk")); w.reg_file(os.path.join(R.scenarios.MODELS, "floor.ztk"))
    bv = R.Batch(w, 2, device=0, max_rigid=2)
    with pytest.raises(R.RkfdError, match="Volume plugin produces no per-vertex contact forces"):
        bv.update_contact_forces()
    assert bv.contact_force_ptrs() == (None, None, None, None)
    bv.close()


_ZERO_COPY = r"""
import sys
ROOT = sys.argv[1]
sys.path[:0] = [ROOT, ROOT + "/tests", ROOT + "/tests/emu"]
import numpy as np
import torch
torch.cuda.init()      # torch's HIP runtime before the library's first call (as bench.py does)
import rkfd_pkg
import cf_cases as cc
R = rkfd_pkg.load()
sc = R.scenarios.config4(batch=130)
w = sc["world"]
m = w.model.contents
b = R.Batch(w, 130, device=0, max_rigid=sc["max_rigid"])
assert b.contact_force_tensors() == {"point": None, "wrench": None, "count": None, "genf": None}
b.set_state(sc["dis"], sc["vel"]); b.update_init(); b.update(3)
b.update_dynamics(R.DYN_MASS | R.DYN_BIAS); b.update_contact_forces()
got = b.get_contact_forces(); dyn = b.get_dynamics()
assert b.status() == 0 and np.abs(got["genf"]).max() > 1.0
# the other views keep their shapes
assert len(b.dev_tensors()) == 3 and len(b.dev_tensors(links=True)) == 8 and set(b.dynamics_tensors()) == {"M", "h", "g"}
t = b.contact_force_tensors()
L = R.lib()
for k, fn in zip(cc.KEYS, ("rkfdBatchDevContactPoint", "rkfdBatchDevContactWrench", "rkfdBatchDevContactCount", "rkfdBatchDevContactGenForce")):
    assert t[k].data_ptr() == getattr(L, fn)(b._b) == b.contact_force_ptrs()[cc.KEYS.index(k)], k
    assert t[k].dtype == (torch.int32 if k == "count" else torch.float64) and tuple(t[k].shape) == got[k].shape, k
    assert np.array_equal(t[k].cpu().numpy(), got[k]), k
# the passive acceleration of one instance on the device: M^-1 ( genf - h )
i = 7
td = b.dynamics_tensors()
dev = torch.linalg.solve(td["M"][i], t["genf"][i] - td["h"][i]).cpu().numpy()
host = np.linalg.solve(dyn["M"][i], got["genf"][i] - dyn["h"][i])
assert np.abs(dev - host).max() <= 1e-10 * max(1.0, np.abs(host).max()), np.abs(dev - host).max()
# the device form on torch tensors: the batch's own flags and forces handed back in give the same bits
act, _, _, f = b.get_contact()
ta = torch.as_tensor(act.astype(np.int32), device="cuda"); tf = torch.as_tensor(f, device="cuda")
tf[ta == 0] = float("nan")
ptrs = b.contact_force_ptrs()
b.update_contact_forces(active=ta, f=tf)
torch.cuda.synchronize()
again = b.get_contact_forces()
assert b.contact_force_ptrs() == ptrs      # stable
for k in cc.KEYS:
    assert np.array_equal(again[k], got[k]), k
# the views alias the live buffers: other forces show through them
b.update_contact_forces(active=ta, f=2.0 * tf); g2 = b.get_contact_forces()
assert np.array_equal(t["genf"].cpu().numpy(), g2["genf"]) and np.array_equal(g2["genf"], 2.0 * got["genf"])
for bad in (ta.to(torch.int64), ta[:, :-1], ta.cpu()):
    try:
        b.update_contact_forces(active=bad, f=tf)
    except (TypeError, ValueError):
        pass
    else:
        raise AssertionError("a bad tensor was accepted")
print("zero-copy ok")
"""


def test_zero_copy_views(R, tmp_path):
    """the torch views of contact_force_tensors() equal get_contact_forces(), their pointers the C ones, and M^-1 ( genf - h ) solved
    on them on the GPU equals the host value; the device form on torch tensors; in a process of its own, because torch's HIP runtime
    has to come up before the library's first call"""
    import sys
    f = tmp_path / "zero_copy_cf.py"
    f.write_text(_ZERO_COPY)
    r = subprocess.run([sys.executable, str(f), ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "zero-copy ok" in r.stdout, r.stdout + r.stderr


def test_node_get_contact_forces(R):
    sc = R.scenarios.config4(batch=19)
    res = []
    n = R.Node(sc["world"], 19, max_rigid=sc["max_rigid"], devices=[0])
    n.set_state(sc["dis"], sc["vel"]); n.update_init(); n.update(3)
    got = n.get_contact_forces()
    assert n.status() == 0
    b = R.Batch(sc["world"], 19, device=0, max_rigid=sc["max_rigid"])
    b.set_state(sc["dis"], sc["vel"]); b.update_init(); b.update(3); b.update_contact_forces()
    ref = b.get_contact_forces()
    assert ref["count"].sum() >= 2 * 8 * 19
    for k in cc.KEYS:
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k
    only = n.get_contact_forces(cc.WRENCH)
    assert set(only) == {"wrench", "count"} and np.array_equal(only["wrench"], ref["wrench"])
    with pytest.raises(R.RkfdError, match="RKFD_CF_POINT, RKFD_CF_WRENCH and RKFD_CF_GENF"):
        n.get_contact_forces(8)
    b.close(); n.close()
