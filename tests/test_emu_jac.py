"""The task-space Jacobians (rkfdBatchUpdateJacobians) under the lane emulator, without a GPU: the device code of
roki-fd_amd/csrc/readout/rkfd_jac.h on 64 host threads (tests/emu/rkfd_emu_jac.cpp) against the reference of tests/jac_cases.py -
the oracle's link velocities and the numpy comvel at unit rate vectors, column by column - to 1e-12 max( 1, |value|_inf ); J vel
against the emulated read-out; the exact zero pattern; the parameter table; the textbook Jacobian as a guard on conventions.
Measured worst deviations: profiles/r10_jac_parity.txt.  tests/test_gpu_jac.py repeats the worlds on the GPU."""
import numpy as np
import pytest

import instance_params as ip
import jac_cases as jc
import links_cases as lc


@pytest.fixture(scope="module")
def worlds(R):
    return jc.cases(R)


@pytest.fixture(scope="module")
def refs(R, oracle_cls, worlds):
    """name -> (reference, oracle frames): computed once, shared by the tests below, never written to"""
    return {name: jc.reference(R, oracle_cls, c["world"], c["dis"], c["links"], c["points"], c["broken"], with_frames=True) for name, c in worlds.items()}


def _zero_pattern(c, got):
    """columns of coordinates that do not move a site / belong to another chain are exactly 0.0"""
    m = c["world"].model.contents
    mv, cmv = jc.moves(m), jc.chain_moves(m)
    if "J" in got:
        for s, l in enumerate(c["links"]):
            assert (got["J"][:, s][:, :, ~mv[l]] == 0.0).all(), (s, l)
    if "Jcom" in got:
        for ch in range(m.nchain):
            assert (got["Jcom"][:, ch][:, :, ~cmv[ch]] == 0.0).all(), ch


def _both_flags(c, ref, name):
    got = jc.emu_jac(c["world"], c["dis"], c["links"], c["points"])
    jc.check(got, ref, name)
    _zero_pattern(c, got)
    for flags, key in ((jc.SITES, "J"), (jc.COM, "Jcom")):
        one = jc.emu_jac(c["world"], c["dis"], c["links"], c["points"], flags=flags)
        assert set(one) == {key} and np.array_equal(one[key], got[key]), (name, flags)
    return got


@pytest.mark.parametrize("name", jc.WORLDS)
def test_emulated_jacobians_match_the_oracle(worlds, refs, name):
    c = worlds[name]
    got = _both_flags(c, refs[name][0], name)
    m = c["world"].model.contents
    if name == "config5":
        # the static floor chain was made massless: zeros; a site on a box and one on the humanoid, the other chains' columns exact zeros
        assert not got["Jcom"][:, -1].any() and np.abs(got["Jcom"][:, 0]).max() > 0.1
        cmv = jc.chain_moves(m)
        ch = m.arr("chain", m.nlink)[c["links"]]
        for s in range(len(c["links"])):
            assert (got["J"][:, s][:, :, ~cmv[ch[s]]] == 0.0).all()
            assert np.abs(got["J"][:, s]).max() > 0.5 or not cmv[ch[s]].any()          # (the floor has no coordinates at all)
        assert sum(bool(cmv[x].any()) for x in set(ch.tolist())) >= 5
    if name == "wall_cantilever":
        # breakable float joints contribute their six columns whether broken or not: the flags are not an input at all
        assert c["broken"] is not None and c["broken"].any() and not c["broken"].all()
    if name == "humanoid30_shell":
        on_merged = [s for s, l in enumerate(c["links"]) if l in ip.merged_links(c["world"])]
        assert on_merged and np.abs(c["points"][on_merged]).min() > 0


def test_emulated_jacobians_on_random_trees(R, oracle_cls, tmp_path):
    cs = jc.random_tree_cases(R, tmp_path)
    assert len(cs) == 10
    prism = 0
    for name, c in cs.items():
        m = c["world"].model.contents
        prism += int((m.arr("jtype", m.nlink) == 2).sum())
        ref, fr = jc.reference(R, oracle_cls, c["world"], c["dis"], c["links"], c["points"], with_frames=True)
        _geometric(c, _both_flags(c, ref, name), ref, fr, name)
    assert prism > 5


@pytest.mark.parametrize("name", jc.LIMIT_TREES)
def test_emulated_jacobians_at_the_tree_limits(R, oracle_cls, tmp_path, name):
    """64 coordinates behind a float root (every lane a column), 96 model links (two blocks of lanes), 63 coordinates of spherical joints"""
    c = jc.limit_tree_cases(R, tmp_path)[name]
    m = c["world"].model.contents
    assert m.ndof >= 63 or m.nlink > 64
    ref, fr = jc.reference(R, oracle_cls, c["world"], c["dis"], c["links"], c["points"], with_frames=True)
    got = _both_flags(c, ref, name)
    _geometric(c, got, ref, fr, name)


def test_j_times_vel_is_the_readout(worlds):
    """J vel and Jcom vel against the emulator's own links read-out of a random vel, at TOL"""
    for name, c in worlds.items():
        got = jc.emu_jac(c["world"], c["dis"], c["links"], c["points"])
        ro = lc.emu_links(c["world"], c["dis"], c["vel"])
        Rl, v, w = ro["R"][:, c["links"]], ro["v"][:, c["links"], :3], ro["v"][:, c["links"], 3:]
        want = np.concatenate([np.einsum("bsij,bsj->bsi", Rl, v + np.cross(w, c["points"][None])), np.einsum("bsij,bsj->bsi", Rl, w)], axis=2)
        lc.check({"J vel": np.einsum("bsrc,bc->bsr", got["J"], c["vel"]), "Jcom vel": np.einsum("bkrc,bc->bkr", got["Jcom"], c["vel"])},
                 {"J vel": want, "Jcom vel": ro["comvel"]}, name, keys=("J vel", "Jcom vel"))


def test_null_points_are_the_link_origins(worlds):
    c = worlds["humanoid30"]
    a = jc.emu_jac(c["world"], c["dis"], c["links"], None, flags=jc.SITES)
    b = jc.emu_jac(c["world"], c["dis"], c["links"], np.zeros_like(c["points"]), flags=jc.SITES)
    assert np.array_equal(a["J"], b["J"])
    # the angular rows do not depend on the point
    assert np.array_equal(a["J"][:, :, 3:], jc.emu_jac(c["world"], c["dis"], c["links"], c["points"], flags=jc.SITES)["J"][:, :, 3:])


def test_emulated_jacobians_with_a_parameter_table(R, oracle_cls, worlds):
    """an instance's own masses and centres of mass move Jcom as they move the reference, and J not by a bit"""
    c = worlds["humanoid30"]
    B = c["dis"].shape[0]
    P = ip.randomised(c["world"], B, seed=0x1AC1)
    got = jc.emu_jac(c["world"], c["dis"], c["links"], c["points"], par=(P["mass"], P["com"]))
    plain = jc.emu_jac(c["world"], c["dis"], c["links"], c["points"])
    assert np.array_equal(got["J"], plain["J"])
    assert np.abs(got["Jcom"] - plain["Jcom"]).max() > 1e-5
    jc.check(got, jc.reference(R, oracle_cls, c["world"], c["dis"], c["links"], c["points"], mass=P["mass"], com=P["com"]), "humanoid30 + table")


def test_sites_are_checked(worlds):
    c = worlds["humanoid30"]
    m = c["world"].model.contents
    import ctypes as C
    L = jc.emu_lib()
    dis = np.ascontiguousarray(c["dis"][:1])
    J = np.zeros((1, 65, 6, m.ndof))
    for links, pts in (([m.nlink], None), ([-1], None), ([0], [[0.0, np.nan, 0.0]]), ([0], [[np.inf, 0.0, 0.0]]), ([0] * 65, None)):
        li = np.array(links, dtype=np.int32)
        pt = None if pts is None else np.array(pts)
        r = L.rkfd_emu_jac(C.cast(c["world"].model, C.c_void_p), 1, dis.ctypes.data, jc.SITES, li.size, li.ctypes.data,
                           None if pt is None else pt.ctypes.data, None, None, J.ctypes.data, None)
        assert r == -2, (links, pts)


def _geometric(c, got, ref, fr, name):
    tb = jc.textbook_batch(c["world"], fr, c["links"], c["points"])
    live = jc.worst(lc.deviations(tb, ref, jc.KEYS))
    dev = jc.worst(lc.deviations(got, tb, jc.KEYS))
    rec = jc.GEOM_RECORDED[name]
    print(f"{name}: textbook against the oracle {live:.2e} (recorded {rec:.2e}), device against the textbook {dev:.2e}")
    assert dev <= 10 * rec + jc.TOL, (name, dev, rec)


@pytest.mark.parametrize("name", jc.WORLDS)
def test_textbook_jacobian_guards_the_conventions(worlds, refs, name):
    c = worlds[name]
    ref, fr = refs[name]
    _geometric(c, jc.emu_jac(c["world"], c["dis"], c["links"], c["points"]), ref, fr, name)
