"""The task-space Jacobians on the GPU (rkfdBatchUpdateJacobians, rkfd_jac_kernel): the worlds of tests/test_emu_jac.py at batch
sizes 1, 3 and 130 against the reference of tests/jac_cases.py (the oracle's unit-rate columns) on the first and the last
instances and against the emulator's device code on every instance, to 1e-12 max( 1, |value|_inf ); stream order without a host
wait; that the launch changes no state; flags, sites and their refusals; zero-copy views; the node level.
Measured worst deviations on the GPU: profiles/r10_jac_parity.txt."""
import os
import subprocess

import numpy as np
import pytest

import instance_params as ip
import jac_cases as jc
import links_cases as lc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def worlds(R, tmp_path_factory):
    cs = jc.cases(R)
    cs.update(jc.limit_tree_cases(R, tmp_path_factory.mktemp("limit_trees")))
    return cs


def _jacobians(R, c, dis, flags=jc.ALL, broken=None):
    b = R.Batch(c["world"], dis.shape[0], device=0, max_rigid=0)
    b.set_state(dis, np.zeros_like(dis))
    if broken is not None:
        b.set_broken(broken)
    b.set_jacobian_sites(c["links"], c["points"])
    b.update_jacobians(flags)
    return b, b.get_jacobians()


def _against_oracle_and_emulator(R, oracle_cls, c, B, name):
    dis, br = jc.tile(c, B)
    b, got = _jacobians(R, c, dis, broken=br)
    assert got["J"].shape == (B, len(c["links"]), 6, b.ndof) and got["Jcom"].shape == (B, b.nchain, 3, b.ndof)
    pick = sorted(set(list(range(min(B, 3))) + [B - 1]))
    ref = jc.reference(R, oracle_cls, c["world"], dis[pick], c["links"], c["points"], None if br is None else br[pick])
    jc.check({k: v[pick] for k, v in got.items()}, ref, f"{name} B={B}")
    jc.check(got, jc.emu_jac(c["world"], dis, c["links"], c["points"]), f"{name} B={B} [emulator, every instance]")
    m = c["world"].model.contents
    mv = jc.moves(m)
    for s, l in enumerate(c["links"]):
        assert (got["J"][:, s][:, :, ~mv[l]] == 0.0).all(), (name, s)
    b.close()


@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("name", jc.WORLDS + jc.LIMIT_TREES)
def test_jacobians_match_the_oracle(R, oracle_cls, worlds, name, B):
    """130 = 32 workgroups of four instances and a last one of two: the partial workgroup, and nothing written past `batch` -
    the buffers hold exactly `batch` instances, and the last instance is compared like every other"""
    _against_oracle_and_emulator(R, oracle_cls, worlds[name], B, name)


@pytest.mark.parametrize("B", [1, 3, 130])
def test_jacobians_on_random_trees(R, oracle_cls, tmp_path, B):
    for name, c in jc.random_tree_cases(R, tmp_path).items():
        _against_oracle_and_emulator(R, oracle_cls, c, B, name)


def test_jacobians_with_a_parameter_table(R, oracle_cls, worlds):
    c = worlds["humanoid30"]
    dis, _ = jc.tile(c, 5)
    P = ip.randomised(c["world"], 5, seed=0x1AC2)
    b, plain = _jacobians(R, c, dis)
    b.set_param("mass", P["mass"]); b.set_param("com", P["com"])
    b.update_jacobians(); got = b.get_jacobians()
    assert np.array_equal(got["J"], plain["J"])
    assert np.abs(got["Jcom"] - plain["Jcom"]).max() > 1e-5
    jc.check(got, jc.reference(R, oracle_cls, c["world"], dis, c["links"], c["points"], mass=P["mass"], com=P["com"]), "humanoid30 + table")
    b.set_param("mass", P["mass"] * 1.5 + 0.1)                     # a later change of the table reaches the next launch
    b.update_jacobians(jc.COM); again = b.get_jacobians()
    jc.check(again, jc.reference(R, oracle_cls, c["world"], dis, c["links"], c["points"], mass=P["mass"] * 1.5 + 0.1, com=P["com"]), "table changed", keys=("Jcom",))
    b.clear_params(); b.update_jacobians(); back = b.get_jacobians()
    assert np.array_equal(back["Jcom"], plain["Jcom"])
    b.close()


def test_stream_order_without_a_host_wait(R, oracle_cls):
    """update(5) under set_split(3), update_jacobians, get_jacobians - no status() / join in between - equals a second batch that waited"""
    B = 130
    sc = R.scenarios.config4(batch=B)
    links, pts = jc.sites_for(sc["world"], 80)
    out = []
    for wait in (False, True):
        b = R.Batch(sc["world"], B, device=0, max_rigid=sc["max_rigid"])
        b.set_split(3)
        b.set_jacobian_sites(links, pts)
        b.set_state(sc["dis"], sc["vel"]); b.update_init(); b.update(5)
        if wait:
            assert b.status() == 0
        b.update_jacobians()
        out.append((b, b.get_jacobians()))
    for k in jc.KEYS:
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
    b = out[0][0]
    assert b.status() == 0
    dis, vel, _ = b.get_state()
    assert np.abs(dis - sc["dis"]).max() > 1e-6          # the steps were seen
    pick = [0, 1, 64, B - 1]
    jc.check({k: v[pick] for k, v in out[0][1].items()}, jc.reference(R, oracle_cls, sc["world"], dis[pick], links, pts), "config4 after 5 steps")
    for x, _ in out:
        x.close()


def _final(b):
    return tuple(b.get_state()) + tuple(b.get_contact()) + tuple(b.get_pivot())


@pytest.mark.parametrize("variant", ["generic", "specialized", "two_per_wave", "table"])
def test_jacobians_change_nothing(R, variant):
    """update(5); update_jacobians(); update(5) leaves, bit for bit, what update(10) leaves"""
    B = 9
    sc = R.scenarios.config3(batch=B) if variant == "two_per_wave" else R.scenarios.config4(batch=B)
    links, pts = jc.sites_for(sc["world"], 81)
    res = []
    for read in (False, True):
        b = R.Batch(sc["world"], B, device=0, max_rigid=sc["max_rigid"])
        if variant == "table":
            P = ip.randomised(sc["world"], B, seed=0x1AC3)
            for k in ("mass", "com", "inertia"):
                b.set_param(k, P[k])
        if variant == "two_per_wave":
            b.set_instances_per_wave(2)
        if variant in ("specialized", "two_per_wave"):
            b.specialize()
            assert b.instances_per_wave() == (2 if variant == "two_per_wave" else 1)
        b.set_state(sc["dis"], sc["vel"]); b.update_init()
        if read:
            b.set_jacobian_sites(links, pts)
            b.update(5); b.update_jacobians(); b.update(5)
            assert np.isfinite(b.get_jacobians()["J"]).all()
        else:
            b.update(10)
        assert b.status() == 0
        res.append(_final(b)); b.close()
    for k, (x, y) in enumerate(zip(*res)):
        assert np.array_equal(x, y), (variant, k)


def test_sites_and_flags(R, worlds):
    c = worlds["humanoid30"]
    m = c["world"].model.contents
    L = R.lib()
    err = lambda: L.rkfdHipLastError().decode()
    n = c["dis"].shape[0]
    b = R.Batch(c["world"], n, device=0, max_rigid=0)
    b.set_state(c["dis"], c["vel"])
    # a batch that never asked holds nothing
    assert b.jacobian_ptrs() == (None, None) and b.nsite == 0
    assert L.rkfdBatchGetJacobians(b._b, None, np.zeros(1).ctypes.data) == -1 and "no Jacobians have been computed" in err()
    # flags
    for flags in (0, 4, 7, -1):
        assert L.rkfdBatchUpdateJacobians(b._b, flags, None) == -1 and "RKFD_JAC_SITES and RKFD_JAC_COM" in err(), flags
    assert L.rkfdBatchUpdateJacobians(b._b, jc.SITES, None) == -1 and "without sites" in err()
    assert L.rkfdBatchUpdateJacobians(b._b, jc.ALL, None) == -1 and "without sites" in err()
    assert b.jacobian_ptrs() == (None, None)
    b.update_jacobians(jc.COM)                     # the centre of mass needs no sites
    only = b.get_jacobians()
    assert set(only) == {"Jcom"} and b.jacobian_ptrs()[0] is None and b.jacobian_ptrs()[1]
    Jbuf = np.zeros((n, 64, 6, m.ndof))
    assert L.rkfdBatchGetJacobians(b._b, Jbuf.ctypes.data, None) == -1 and "RKFD_JAC_SITES" in err()
    # sites, then their replacement between two launches
    b.set_jacobian_sites(c["links"], c["points"])
    assert b.nsite == len(c["links"])
    b.update_jacobians(); first = b.get_jacobians()
    assert np.array_equal(first["Jcom"], only["Jcom"])
    pJ = b.jacobian_ptrs()
    # refusals leave the previous sites in place
    for links, pts, msg in (([m.nlink], None, "is not within the model's"), ([-1], None, "is not within the model's"),
                            ([0, 1], [[0, 0, 0], [0, np.nan, 0]], "not finite"), ([0], [[np.inf, 0, 0]], "not finite"), ([0] * 65, None, "0 .. 64")):
        with pytest.raises(R.RkfdError, match=msg):
            b.set_jacobian_sites(links, None if pts is None else np.array(pts, dtype=float))
        assert b.nsite == len(c["links"])
    b.update_jacobians()
    assert np.array_equal(b.get_jacobians()["J"], first["J"]) and b.jacobian_ptrs() == pJ
    other = c["links"][::-1].copy()
    b.set_jacobian_sites(other, c["points"][::-1].copy())           # the same number: the buffer stays
    assert L.rkfdBatchGetJacobians(b._b, Jbuf.ctypes.data, None) == -1 and "present sites" in err()      # not computed for these sites yet
    b.update_jacobians(jc.SITES)
    assert b.jacobian_ptrs() == pJ
    assert np.array_equal(b.get_jacobians()["J"], first["J"][:, ::-1])
    # nsite changed
    b.set_jacobian_sites(c["links"][:2])                            # points None: the link origins
    assert b.nsite == 2 and b.jacobian_ptrs()[0] is None and b.jacobian_ptrs()[1] == pJ[1]
    b.update_jacobians(); two = b.get_jacobians()
    assert two["J"].shape == (n, 2, 6, m.ndof)
    jc.check(two, jc.emu_jac(c["world"], c["dis"], c["links"][:2], None), "two sites at the link origins")
    b.set_jacobian_sites([])                                          # cleared
    assert b.nsite == 0 and L.rkfdBatchUpdateJacobians(b._b, jc.SITES, None) == -1 and "without sites" in err()
    b.update_jacobians(jc.COM)
    assert np.array_equal(b.get_jacobians()["Jcom"], only["Jcom"])
    # snapshot / restore leave the results alone
    b.snapshot(); b.restore()
    assert np.array_equal(b.get_jacobians()["Jcom"], only["Jcom"])
    b.close()


_ZERO_COPY = r"""
import sys
ROOT = sys.argv[1]
sys.path[:0] = [ROOT, ROOT + "/tests", ROOT + "/tests/emu"]
import numpy as np
import torch
torch.cuda.init()      # torch's HIP runtime before the library's first call (as bench.py does)
import rkfd_pkg
import jac_cases as jc
import links_cases as lc
R = rkfd_pkg.load()
c = jc.cases(R)["humanoid30"]
dis, vel = lc.states(c["world"], 130, 0x2D)
b = R.Batch(c["world"], 130, device=0, max_rigid=0)
assert b.jacobian_tensors() == {"J": None, "Jcom": None}
b.set_state(dis, vel); b.set_jacobian_sites(c["links"], c["points"]); b.update_jacobians()
got = b.get_jacobians()
assert len(b.dev_tensors()) == 3 and len(b.dev_tensors(links=True)) == 8      # the state views keep their shapes
t = b.jacobian_tensors()
L = R.lib()
assert t["J"].data_ptr() == L.rkfdBatchDevJacobian(b._b) == b.jacobian_ptrs()[0]
assert t["Jcom"].data_ptr() == L.rkfdBatchDevComJacobian(b._b) == b.jacobian_ptrs()[1]
for k in jc.KEYS:
    assert t[k].dtype == torch.float64 and tuple(t[k].shape) == got[k].shape and np.array_equal(t[k].cpu().numpy(), got[k]), k
# Jcom' f on the device: a desired force on the centre of mass of chain 0 as joint forces
f = np.array([3.0, -2.0, 40.0])
dev = torch.einsum("brc,r->bc", t["Jcom"][:, 0], torch.as_tensor(f, device="cuda")).cpu().numpy()
host = np.einsum("brc,r->bc", got["Jcom"][:, 0], f)
assert np.abs(dev - host).max() <= 1e-13 * max(1.0, np.abs(host).max()), np.abs(dev - host).max()
ptrs = b.jacobian_ptrs()
b.update_jacobians()
assert b.jacobian_ptrs() == ptrs      # stable
# the views alias the live buffers: the Jacobians of another state show through them
b.set_state(dis[::-1].copy(), vel[::-1].copy()); b.update_jacobians(); g2 = b.get_jacobians()
assert np.array_equal(t["J"].cpu().numpy(), g2["J"]) and not np.array_equal(g2["J"], got["J"])
print("zero-copy ok")
"""


def test_zero_copy_views(R, tmp_path):
    """the torch views of jacobian_tensors() equal get_jacobians(), their pointers the C ones, and Jcom' f evaluated on them on the
    GPU equals the host value; in a process of its own, because torch's HIP runtime has to come up before the library's first call"""
    import sys
    f = tmp_path / "zero_copy_jac.py"
    f.write_text(_ZERO_COPY)
    r = subprocess.run([sys.executable, str(f), ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "zero-copy ok" in r.stdout, r.stdout + r.stderr


def test_node_get_jacobians(R, worlds):
    c = worlds["humanoid30"]
    dis, _ = jc.tile(c, 19)
    n = R.Node(c["world"], 19, max_rigid=0, devices=[0])
    n.set_state(dis, np.zeros_like(dis))
    n.set_jacobian_sites(c["links"], c["points"])
    got = n.get_jacobians()
    b, ref = _jacobians(R, c, dis)
    for k in jc.KEYS:
        assert np.array_equal(got[k], ref[k]), k
    only = n.get_jacobians(jc.COM)
    assert set(only) == {"Jcom"} and np.array_equal(only["Jcom"], ref["Jcom"])
    with pytest.raises(R.RkfdError, match="is not within the model's"):
        n.set_jacobian_sites([b.nlink])
    assert np.array_equal(n.get_jacobians(jc.SITES)["J"], ref["J"])          # the refused list changed nothing
    b.close(); n.close()
