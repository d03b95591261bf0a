"""The task-space read-out on the GPU (rkfdBatchUpdateLinks, rkfd_links_kernel): the worlds of tests/test_emu_links.py at batch
sizes 1, 3 and 130 against the comparison protocol of tests/links_cases.py (oracle frames and velocities at the same state, numpy
sums for the centres of mass, scenarios.link_frames) to 1e-12 max( 1, |value|_inf ); stream order without a host wait; that the
read-out changes no state; flags; zero-copy views; the node level; the reference-named C accessors.
Measured worst deviations on the GPU: profiles/r06_links_parity.txt."""
import os
import subprocess

import numpy as np
import pytest

import instance_params as ip
import links_cases as lc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS = ["chain30", "humanoid30_shell", "humanoid30", "arm_spher", "wall_cantilever", "wall", "config5"]


@pytest.fixture(scope="module")
def worlds(R):
    return lc.cases(R)


def _tile(c, B):
    """B states of a case: its seeded ones, then further seeded draws"""
    n = c["dis"].shape[0]
    d2, v2 = lc.states(c["world"], B, 0x6AB + B)
    d2[:min(n, B)] = c["dis"][:B]; v2[:min(n, B)] = c["vel"][:B]
    br = None if c["broken"] is None else np.stack([c["broken"][i % n] for i in range(B)])
    return d2, v2, br


def _readout(R, world, dis, vel, broken=None, max_rigid=0, flags=lc.ALL):
    b = R.Batch(world, dis.shape[0], device=0, max_rigid=max_rigid)
    b.set_state(dis, vel)
    if broken is not None:
        b.set_broken(broken)
    b.update_links(flags)
    return b, b.get_links()


@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("name", WORLDS)
def test_readout_matches_the_oracle(R, oracle_cls, worlds, name, B):
    """130 = 32 workgroups of four instances and a last one of two: the partial workgroup, and nothing written past `batch` -
    the buffers hold exactly `batch` instances, and the last instance is compared like every other"""
    c = worlds[name]
    dis, vel, br = _tile(c, B)
    b, got = _readout(R, c["world"], dis, vel, br)
    # the oracle for the case's own states and the batch's last instances; every instance against the emulator's device code
    pick = sorted(set(list(range(min(B, 3))) + [B - 1]))
    ref = lc.reference(R, oracle_cls, c["world"], dis[pick], vel[pick], None if br is None else br[pick])
    lc.check({k: v[pick] for k, v in got.items()}, ref, f"{name} B={B}")
    lc.check_positions_second_fk(R, c["world"], dis, got, f"{name} B={B}")
    emu = lc.emu_links(c["world"], dis, vel)
    lc.check(got, emu, f"{name} B={B} [emulator, every instance]")
    b.close()


def test_readout_on_random_trees(R, oracle_cls, tmp_path):
    for name, c in lc.random_tree_cases(R, tmp_path).items():
        b, got = _readout(R, c["world"], c["dis"], c["vel"])
        lc.check(got, lc.reference(R, oracle_cls, c["world"], c["dis"], c["vel"]), name)
        b.close()


def test_readout_with_a_parameter_table(R, oracle_cls, worlds):
    c = worlds["humanoid30"]
    dis, vel, _ = _tile(c, 5)
    P = ip.randomised(c["world"], 5, seed=0x11AD)
    b, plain = _readout(R, c["world"], dis, vel)
    b.set_param("mass", P["mass"]); b.set_param("com", P["com"])
    b.update_links(); got = b.get_links()
    for k in ("R", "p", "v"):
        assert np.array_equal(got[k], plain[k]), k
    lc.check(got, lc.reference(R, oracle_cls, c["world"], dis, vel, mass=P["mass"], com=P["com"]), "humanoid30 + table")
    b.set_param("mass", P["mass"] * 1.5)                     # a later change of the table reaches the next read-out
    b.update_links(lc.COM); again = b.get_links()
    lc.check(again, lc.reference(R, oracle_cls, c["world"], dis, vel, mass=P["mass"] * 1.5, com=P["com"]), "table changed", keys=("com", "comvel"))
    b.clear_params(); b.update_links(); back = b.get_links()
    assert np.array_equal(back["com"], plain["com"])
    b.close()


def test_readout_after_joints_broke_in_a_run(R, oracle_cls):
    """the wall hit by the box, stepped on the GPU until joints have broken during the run: the read-out of the live state,
    without a host wait in between, against the oracle at the batch's get_state() and get_broken()"""
    sc = R.scenarios.wall_hit(batch=10)
    b = R.Batch(sc["world"], 2, device=0, max_rigid=sc["max_rigid"])
    b.set_state(sc["dis"][[2, 9]], sc["vel"][[2, 9]]); b.update_init(); b.update(18)
    b.update_links(); got = b.get_links()
    assert b.status() == 0
    dis, vel, _ = b.get_state(); br = np.array(b.get_broken())
    assert br.sum() >= 3 and np.abs(vel).max() > 0.05          # joints broke in the run, bricks move
    lc.check(got, lc.reference(R, oracle_cls, sc["world"], dis, vel, br), "wall after 18 steps")
    b.close()


def _config4(R, B):
    sc = R.scenarios.config4(batch=B)
    return sc


def test_stream_order_without_a_host_wait(R, oracle_cls):
    """update(5) under set_split(3), update_links, get_links - no status() / join in between - equals a second batch that waited"""
    B = 130
    sc = _config4(R, B)
    out = []
    for wait in (False, True):
        b = R.Batch(sc["world"], B, device=0, max_rigid=sc["max_rigid"])
        b.set_split(3)
        b.set_state(sc["dis"], sc["vel"]); b.update_init(); b.update(5)
        if wait:
            assert b.status() == 0
        b.update_links()
        out.append((b, b.get_links()))
    for k in lc.KEYS:
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
    b = out[0][0]
    assert b.status() == 0
    dis, vel, _ = b.get_state()
    pick = [0, 1, 64, B - 1]
    lc.check({k: v[pick] for k, v in out[0][1].items()}, lc.reference(R, oracle_cls, sc["world"], dis[pick], vel[pick]), "config4 after 5 steps")
    for x, _ in out:
        x.close()


def _final(b):
    return tuple(b.get_state()) + tuple(b.get_contact()) + tuple(b.get_pivot())


@pytest.mark.parametrize("variant", ["generic", "specialized", "two_per_wave", "table"])
def test_readout_changes_nothing(R, variant):
    """update(5); update_links(); update(5) leaves, bit for bit, what update(10) leaves"""
    B = 9
    sc = R.scenarios.config3(batch=B) if variant == "two_per_wave" else _config4(R, B)
    res = []
    for read in (False, True):
        b = R.Batch(sc["world"], B, device=0, max_rigid=sc["max_rigid"])
        if variant == "table":
            P = ip.randomised(sc["world"], B, seed=0x11AE)
            for k in ("mass", "com", "inertia"):
                b.set_param(k, P[k])
        if variant == "two_per_wave":
            b.set_instances_per_wave(2)
        if variant in ("specialized", "two_per_wave"):
            b.specialize()
            assert b.instances_per_wave() == (2 if variant == "two_per_wave" else 1)
        b.set_state(sc["dis"], sc["vel"]); b.update_init()
        if read:
            b.update(5); b.update_links(); b.update(5); b.get_links()
        else:
            b.update(10)
        assert b.status() == 0
        res.append(_final(b)); b.close()
    for k, (x, y) in enumerate(zip(*res)):
        assert np.array_equal(x, y), (variant, k)


def test_flags(R, worlds):
    c = worlds["humanoid30"]
    b, full = _readout(R, c["world"], c["dis"], c["vel"])
    b2, only = _readout(R, c["world"], c["dis"], c["vel"], flags=lc.COM)
    assert set(only) == {"com", "comvel"}
    assert np.array_equal(only["com"], full["com"]) and np.array_equal(only["comvel"], full["comvel"])
    n = c["dis"].shape[0]
    Rbuf = np.zeros((n, b2.nlink, 3, 3))
    L = R.lib()
    assert L.rkfdBatchGetLinks(b2._b, Rbuf.ctypes.data, None, None, None, None) == -1
    assert b"RKFD_LINKS_POSE" in L.rkfdHipLastError()
    b3 = R.Batch(c["world"], n, device=0, max_rigid=0)
    assert L.rkfdBatchGetLinks(b3._b, Rbuf.ctypes.data, None, None, None, None) == -1 and b"no read-out" in L.rkfdHipLastError()
    assert b3.dev_ptrs(links=True)[3:] == (None,) * 5 and L.rkfdBatchDevLinkPos(b3._b) is None          # a batch that never asked holds nothing
    assert L.rkfdBatchUpdateLinks(b3._b, 8, None) == -1 and L.rkfdBatchUpdateLinks(b3._b, 0, None) == -1
    for x in (b, b2, b3):
        x.close()


_ZERO_COPY = r"""
import sys
ROOT = sys.argv[1]
sys.path[:0] = [ROOT, ROOT + "/tests", ROOT + "/tests/emu"]
import numpy as np
import torch
torch.cuda.init()      # torch's HIP runtime before the library's first call (as bench.py does)
import rkfd_pkg
import links_cases as lc
R = rkfd_pkg.load()
c = lc.cases(R)["humanoid30"]
dis, vel = lc.states(c["world"], 130, 0x2C)
b = R.Batch(c["world"], 130, device=0, max_rigid=0)
assert len(b.dev_tensors()) == 3 and b.dev_tensors(links=True)[3:] == (None,) * 5
b.set_state(dis, vel); b.update_links()
got = b.get_links()
d_dis, d_vel, d_acc = b.dev_tensors()      # the state views keep their shape of three after a read-out
assert np.array_equal(d_dis.cpu().numpy(), dis)
t = b.dev_tensors(links=True)
assert len(t) == 8 and set(b.links_tensors()) == set(lc.KEYS)
for x, k in zip(t[3:], lc.KEYS):
    assert x.data_ptr() == b.dev_ptrs(links=True)[3 + lc.KEYS.index(k)] == b.links_tensors()[k].data_ptr(), k
    assert tuple(x.shape) == got[k].shape and np.array_equal(x.cpu().numpy(), got[k]), k
# a cost evaluated on the device: the mean base height
dev = float(t[4][:, 0, 2].mean().cpu()); host = float(got["p"][:, 0, 2].mean())
assert abs(dev - host) <= 1e-13 * max(1.0, abs(host)), (dev, host)
ptrs = b.dev_ptrs(links=True)
b.update_links()
assert b.dev_ptrs(links=True) == ptrs      # stable
# the views alias the live buffers: a read-out of another state shows through them
b.set_state(dis[::-1].copy(), vel[::-1].copy()); b.update_links(); g2 = b.get_links()
assert np.array_equal(t[4].cpu().numpy(), g2["p"]) and not np.array_equal(g2["p"], got["p"])
print("zero-copy ok")
"""


def test_zero_copy_views(R, tmp_path):
    """the torch views of dev_tensors() equal get_links() and a cost evaluated on them on the GPU equals the host value; in a
    process of its own, because torch's HIP runtime has to come up before the library's first call (as in bench.py)"""
    import sys
    f = tmp_path / "zero_copy.py"
    f.write_text(_ZERO_COPY)
    r = subprocess.run([sys.executable, str(f), ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "zero-copy ok" in r.stdout, r.stdout + r.stderr


def test_node_get_links(R, worlds):
    c = worlds["humanoid30"]
    dis, vel, _ = _tile(c, 19)
    n = R.Node(c["world"], 19, max_rigid=0, devices=[0])
    n.set_state(dis, vel)
    got = n.get_links()
    b, ref = _readout(R, c["world"], dis, vel)
    for k in lc.KEYS:
        assert np.array_equal(got[k], ref[k]), k
    only = n.get_links(lc.POSE)
    assert set(only) == {"R", "p"} and np.array_equal(only["p"], ref["p"])
    b.close(); n.close()


def test_reference_named_accessors_from_c(R, oracle_cls, tmp_path):
    """tests/c/links_driver.c (gcc): the arm's tip after 100 steps through rkfdChainLinkWldPos, against the oracle at the state
    the driver prints"""
    exe = str(tmp_path / "links_driver")
    subprocess.run(["gcc", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "links_driver.c"),
                    "-L" + os.path.join(ROOT, "roki-fd_amd"), "-lrkfd_amd", "-Wl,-rpath," + os.path.join(ROOT, "roki-fd_amd"), "-o", exe], check=True)
    r = subprocess.run([exe, os.path.join(ROOT, "models"), "100"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {l.split()[0]: np.array([float(x) for x in l.split()[1:]]) for l in r.stdout.splitlines() if " " in l}
    assert r.stdout.splitlines()[-1] == "reused", r.stdout
    w = R.World(solver=R.SOLVER_MLCP); w.reg_file(os.path.join(R.scenarios.MODELS, "arm_revroot.ztk"))
    m = w.model.contents
    tip = int(rows["link"][0])
    assert tip == m.nlink - 1 and abs(rows["dis"][1] - 0.6) > 1e-3          # it moved
    ref = lc.reference(R, oracle_cls, w, rows["dis"][None], rows["vel"][None])
    got = {"p": rows["tip"], "R": rows["att"].reshape(3, 3), "com": rows["com"]}
    lc.check(got, {"p": ref["p"][0, tip], "R": ref["R"][0, tip], "com": ref["com"][0, 0]}, "arm tip after 100 steps", keys=("p", "R", "com"))
    d0 = np.zeros((1, m.ndof)); d0[0, 0] = 0.3; d0[0, 1] = 0.6
    ref0 = lc.reference(R, oracle_cls, w, d0, np.zeros_like(d0))
    assert np.abs(rows["tip0"] - ref0["p"][0, tip]).max() <= lc.TOL
