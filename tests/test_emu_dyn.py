"""The joint-space dynamics (rkfdBatchUpdateDynamics) under the lane emulator, without a GPU: the device code of
roki-fd_amd/csrc/readout/rkfd_dyn.h on 64 host threads (tests/emu/rkfd_emu_dyn.cpp) against the two references of
tests/dyn_cases.py - A, the kinetic energy of the oracle's unit-rate twists (M, every world), and B, refmath's Newton-Euler (M, h, g,
worlds with orthonormal frames) - to 1e-12 max( 1, |value|_inf ); exact symmetry, the exact zero pattern, positive definiteness;
the flags; the rotor diagonal; the parameter table.  Measured worst deviations: profiles/r11_dyn_parity.txt.
tests/test_gpu_dyn.py repeats the worlds on the GPU."""
import numpy as np
import pytest

import dyn_cases as dc
import instance_params as ip


@pytest.fixture(scope="module")
def worlds(R):
    return dc.cases(R)


def _emulate(c, **kw):
    return dc.emu_dyn(c["world"], c["dis"], c["vel"], **kw)


@pytest.mark.parametrize("name", dc.WORLDS)
def test_emulated_dynamics_match_both_references(R, oracle_cls, worlds, name):
    c = worlds[name]
    assert c["dis"].shape[0] >= 3 and np.abs(c["vel"]).min(axis=1).max() > 0
    got = _emulate(c)
    dc.check_world(R, oracle_cls, c, got, name)
    assert np.abs(got["h"] - got["g"]).max() > 1e-3          # the velocities matter
    if name == "wall_cantilever":
        # breakable float joints are float joints here whether broken or not: the flags are not an input at all
        assert c["broken"] is not None and c["broken"].any() and not c["broken"].all()
    if name == "config5":
        m = c["world"].model.contents
        assert m.nchain >= 5 and not dc.related(m).all()


@pytest.mark.parametrize("ortho", [False, True], ids=["raw", "orthonormal"])
def test_emulated_dynamics_on_random_trees(R, oracle_cls, tmp_path, ortho):
    cs = dc.random_tree_cases(R, tmp_path, ortho)
    assert len(cs) == 10
    prism = 0
    for name, c in cs.items():
        m = c["world"].model.contents
        prism += int((m.arr("jtype", m.nlink) == 2).sum())
        dc.check_world(R, oracle_cls, c, _emulate(c), name)
    assert prism > 5


@pytest.mark.parametrize("ortho", [False, True], ids=["raw", "orthonormal"])
@pytest.mark.parametrize("name", dc.LIMIT_TREES)
def test_emulated_dynamics_at_the_tree_limits(R, oracle_cls, tmp_path, name, ortho):
    """64 coordinates behind a float root (every lane a column), 96 model links (two blocks of lanes, two instances per workgroup),
    63 coordinates of spherical joints"""
    c = dc.limit_tree_cases(R, tmp_path, ortho)[name]
    m = c["world"].model.contents
    assert m.ndof >= 63 or m.nlink > 64
    waves = []
    got = dc.emu_dyn(c["world"], c["dis"], c["vel"], waves=waves)
    dc.check_world(R, oracle_cls, c, got, name)
    # the instances per workgroup by the LDS need: the 96-link tree is not refused, it runs two per workgroup
    assert waves == [2 if m.nlink > 64 else 4]


def test_each_flag_alone_leaves_the_other_arrays_untouched(worlds):
    c = worlds["humanoid30"]
    full = _emulate(c)
    assert all(np.isfinite(full[k]).all() for k in dc.KEYS)
    for flags in (dc.MASS, dc.BIAS, dc.GRAVITY, dc.MASS | dc.GRAVITY, dc.BIAS | dc.GRAVITY):
        one = _emulate(c, flags=flags)
        for k in dc.KEYS:
            if flags & dc.NEED[k]:
                assert np.array_equal(one[k], full[k]), (flags, k)
            else:
                assert np.isnan(one[k]).all(), (flags, k)


def test_rotor_flag_adds_the_reflected_inertia_on_the_diagonal(R, tmp_path, worlds):
    hit = 0
    cs = dict(worlds)
    cs.update(dc.limit_tree_cases(R, tmp_path, True))
    for name in ("humanoid30", "arm_revroot", "chain64_fixed32"):
        c = cs[name]
        m = c["world"].model.contents
        rot = dc.rotor_diagonal(m)
        plain = _emulate(c, flags=dc.MASS)["M"]
        with_r = _emulate(c, flags=dc.MASS | dc.ROTOR)["M"]
        off = ~np.eye(m.ndof, dtype=bool)
        assert np.array_equal(with_r[:, off], plain[:, off]), name
        d0, d1 = np.einsum("bii->bi", plain), np.einsum("bii->bi", with_r)
        assert np.array_equal(d1[:, rot == 0], d0[:, rot == 0]), name
        assert np.array_equal(d1, d0 + rot[None]), name          # one rounded addition, as the model's numbers give it
        hit += int((rot > 0).sum())
    assert hit > 10


def test_emulated_dynamics_with_a_parameter_table(R, oracle_cls, worlds):
    """an instance's own masses, centres of mass AND inertias: the results follow refmath on the instance's model"""
    c = worlds["humanoid30"]
    B = c["dis"].shape[0]
    P = {k: v for k, v in ip.randomised(c["world"], B, seed=0xD711).items() if k in ("mass", "com", "inertia")}
    got = _emulate(c, par=P)
    plain = _emulate(c)
    dc.check_world(R, oracle_cls, c, got, "humanoid30 + table", par=P)
    for k in dc.KEYS:
        assert np.abs(got[k] - plain[k]).max() > 1e-5, k
    # the inertia alone moves M
    P2 = dict(P, mass=np.tile(ip.model_values(c["world"], "mass"), (B, 1)), com=np.tile(ip.model_values(c["world"], "com"), (B, 1)))
    assert np.abs(_emulate(c, par=P2)["M"] - plain["M"]).max() > 1e-5


def test_more_than_64_coordinates_are_refused(R, tmp_path):
    import ctypes as C
    import tree_limits as tl
    case = tl.REFUSED[0][0]
    w = R.World(solver=R.SOLVER_MLCP)
    w.reg_file(tl.write(case, tmp_path))
    m = w.model.contents
    assert m.ndof == 65
    z = np.zeros((1, m.ndof))
    assert dc.emu_lib().rkfd_emu_dyn(C.cast(w.model, C.c_void_p), 1, z.ctypes.data, z.ctypes.data, dc.ALL, None, None, None, None, None, None) == -1


def test_instances_per_workgroup_follow_the_lds_need(R, tmp_path, worlds):
    """4, else 2, else 1 instance per workgroup within 160 KiB; 0 - refused by the C ABI - when one instance does not fit"""
    waves = []
    c = worlds["humanoid30"]
    dc.emu_dyn(c["world"], c["dis"][:1], c["vel"][:1], waves=waves)
    w = dc.fixed_star(R, tmp_path, 420)
    m = w.model.contents
    assert m.nlink == 421 and 8 * (51 * m.nlink + 6 * m.ndof) > 160 * 1024
    z = np.zeros((1, m.ndof))
    got = dc.emu_dyn(w, z + 0.3, z + 1.0, waves=waves)
    assert waves == [4, 0]
    # (the emulator has no LDS limit: the result of the large world is still right)
    dc.check(got, dc.reference_b(w, z + 0.3, z + 1.0), "421 links on one joint")
    # between the two: 2 and 1
    for nfixed, want in ((150, 2), (300, 1)):
        w2 = dc.fixed_star(R, tmp_path, nfixed)
        ws = []
        dc.emu_dyn(w2, z, z, waves=ws)
        assert ws == [want], (nfixed, ws)
