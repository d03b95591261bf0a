"""The contact read-out (rkfdBatchUpdateContactForces) under the lane emulator, without a GPU: the device code of
roki-fd_amd/csrc/readout/rkfd_cf.h on 64 host threads (tests/emu/rkfd_emu_cf.cpp) against the references of tests/cf_cases.py - the
numpy sum over the candidate tables (point, wrench, count), A, the oracle's unit-rate Jacobians, and B, refmath's Newton-Euler (genf) -
to 1e-12 max( 1, |value|_inf ); finite results despite NaN in the entries of inactive candidates, exact linearity in the forces, exact
zeros, action and reaction; the flags.  Measured worst deviations: profiles/r12_cf_parity.txt.  tests/test_gpu_cf.py repeats the
worlds on the GPU."""
import numpy as np
import pytest

import cf_cases as cc
import jac_cases as jc


@pytest.fixture(scope="module")
def worlds(R, tmp_path_factory):
    return cc.cases(R, tmp_path_factory.mktemp("cf_worlds"))


def _emulate(c, f=None, **kw):
    return cc.emu_cf(c["world"], c["dis"], c["active"], c["f"] if f is None else f, cand=c["cand"] if c.get("synthetic") else None, **kw)


def _check(R, oracle_cls, c, name):
    got = _emulate(c)
    dev = cc.check_world(R, oracle_cls, c, got, name)
    cc.check_properties(c["world"], c["cand"], c["dis"], c["active"], c["f"], got, lambda f2: _emulate(c, f=f2), name)
    return got, dev


@pytest.mark.parametrize("name", cc.WORLDS)
def test_emulated_contact_forces_match_the_references(R, oracle_cls, worlds, name):
    c = worlds[name]
    m = c["world"].model.contents
    assert c["cand"].n == m.ncand and np.isnan(c["f"][c["active"] == 0]).all()
    got, _ = _check(R, oracle_cls, c, name)
    if name == "no_candidates":
        assert m.ncand == 0 and got["point"].size == 0
        assert (got["wrench"] == 0.0).all() and (got["count"] == 0).all() and (got["genf"] == 0.0).all()
        return
    assert c["active"].sum() > 0 and (c["active"] == 0).sum() > 0 and np.abs(got["genf"]).max() > 1.0
    if name == "config4":
        assert 0 < m.ncand < 64          # fewer than a wavefront
    if name == "humanoid30_shell":
        assert m.ncand == 764 and m.ncand % 64 == 60
    if name == "config5":
        chain = m.arr("chain", m.nlink)
        assert m.nchain >= 5 and (chain[c["cand"].own] != m.nchain - 1).any() and ((chain[c["cand"].own] != m.nchain - 1) & (chain[c["cand"].other] != m.nchain - 1)).any()
    if name == "arm_fold":
        chain = m.arr("chain", m.nlink)
        assert (chain[c["cand"].own] == chain[c["cand"].other]).any()
    if name == "wall":
        assert (m.arr("jtype", m.nlink) == 5).sum() > 0
        # a breakable float joint gets its six entries like any float joint
        own = jc.coordinate_owner(m)
        brf = np.isin(own, np.flatnonzero(m.arr("jtype", m.nlink) == 5))
        assert np.abs(got["genf"][:, brf]).max() > 1.0


@pytest.mark.parametrize("ortho", [False, True], ids=["raw", "orthonormal"])
def test_emulated_contact_forces_on_trees_with_synthetic_candidates(R, oracle_cls, tmp_path, ortho):
    """the explicit-table entry: candidates on any two links of the three limit trees (64 coordinates, 96 model links, 63 spherical
    coordinates) and of ten random trees, without a contact solver"""
    cs = cc.tree_cases(R, tmp_path, ortho)
    assert set(cc.LIMIT_TREES) <= set(cs) and len(cs) == 13
    for name, c in cs.items():
        waves = []
        got = _emulate(c, waves=waves)
        cc.check_world(R, oracle_cls, c, got, name)
        cc.check_properties(c["world"], c["cand"], c["dis"], c["active"], c["f"], got, lambda f2: _emulate(c, f=f2), name)
        assert waves == [4]


def test_each_flag_alone_leaves_the_other_arrays_untouched(worlds):
    c = worlds["config5"]
    full = _emulate(c)
    for flags in (cc.POINT, cc.WRENCH, cc.GENF, cc.POINT | cc.GENF, cc.WRENCH | cc.GENF):
        one = _emulate(c, flags=flags)
        for k in cc.KEYS:
            if flags & cc.NEED[k]:
                assert np.array_equal(one[k], full[k]), (flags, k)
            else:
                assert (one[k] == -1).all() if k == "count" else np.isnan(one[k]).all(), (flags, k)


def test_an_inactive_candidate_contributes_nothing_whatever_its_entry_holds(worlds):
    c = worlds["humanoid30_shell"]
    a = _emulate(c)
    for fill in (0.0, np.inf, 1e300):
        f2 = c["f"].copy(); f2[c["active"] == 0] = fill
        b = _emulate(c, f=f2)
        for k in cc.KEYS:
            assert np.array_equal(a[k], b[k]), (fill, k)


def test_more_than_64_coordinates_and_bad_links_are_refused(R, tmp_path):
    import ctypes as C
    import tree_limits as tl
    w = R.World(solver=R.SOLVER_MLCP)
    w.reg_file(tl.write(tl.REFUSED[0][0], tmp_path))
    m = w.model.contents
    assert m.ndof == 65
    z = np.zeros((1, m.ndof))
    assert cc.emu_lib().rkfd_emu_cf(C.cast(w.model, C.c_void_p), 1, z.ctypes.data, None, None, cc.ALL, 0, None, None, None, None, None, None, None) == -1
    w2 = R.scenarios.config4(batch=1)["world"]
    bad = cc.Cand([0, w2.model.contents.nlink], [1, 0], np.zeros((2, 3)))
    z = np.zeros((1, w2.model.contents.ndof))
    assert cc.emu_lib().rkfd_emu_cf(C.cast(w2.model, C.c_void_p), 1, z.ctypes.data, None, None, cc.ALL, 2, bad.own.ctypes.data, bad.other.ctypes.data,
                                     bad.vert.ctypes.data, None, None, None, None) == -2
