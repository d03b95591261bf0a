"""The task-space read-out (rkfdBatchUpdateLinks) under the lane emulator, without a GPU: the device code of
roki-fd_amd/csrc/readout/rkfd_links.h on 64 host threads (tests/emu/rkfd_emu_links.cpp) against the comparison protocol of
tests/links_cases.py - the oracle's link frames and link velocities at the same state, numpy sums for the centres of mass,
scenarios.link_frames as a second forward kinematics - to 1e-12 max( 1, |value|_inf ).
Measured worst deviations under the emulator: profiles/r06_links_parity.txt (all below 1e-13).
tests/test_gpu_links.py repeats the worlds on the GPU."""
import numpy as np
import pytest

import instance_params as ip
import links_cases as lc

WORLDS = ["chain30", "humanoid30_shell", "humanoid30", "arm_spher", "wall_cantilever", "wall", "config5"]


@pytest.fixture(scope="module")
def worlds(R):
    return lc.cases(R)


@pytest.mark.parametrize("name", WORLDS)
def test_emulated_readout_matches_the_oracle(R, oracle_cls, worlds, name):
    c = worlds[name]
    got = lc.emu_links(c["world"], c["dis"], c["vel"])
    ref = lc.reference(R, oracle_cls, c["world"], c["dis"], c["vel"], c["broken"])
    lc.check(got, ref, name)
    lc.check_positions_second_fk(R, c["world"], c["dis"], got, name)
    m = c["world"].model.contents
    if name == "config5":
        # the static floor chain was made massless: it reports zeros, the others do not
        assert m.nchain == 6 and not got["com"][:, -1].any() and not got["comvel"][:, -1].any()
        assert np.abs(got["com"][:, :-1]).min(axis=2).max() > 0
    if name in ("humanoid30", "humanoid30_shell"):
        assert len(ip.merged_links(c["world"])) > 0          # model links != device links


def test_emulated_readout_on_random_trees(R, oracle_cls, tmp_path):
    cs = lc.random_tree_cases(R, tmp_path)
    assert len(cs) == 10
    prism = 0
    for name, c in cs.items():
        m = c["world"].model.contents
        prism += int((m.arr("jtype", m.nlink) == 2).sum())
        got = lc.emu_links(c["world"], c["dis"], c["vel"])
        lc.check(got, lc.reference(R, oracle_cls, c["world"], c["dis"], c["vel"]), name)
        lc.check_positions_second_fk(R, c["world"], c["dis"], got, name)
    assert prism > 5


def test_emulated_readout_with_a_parameter_table(R, oracle_cls, worlds):
    """an instance's own masses and centres of mass move com / comvel and nothing else"""
    c = worlds["humanoid30"]
    B = c["dis"].shape[0]
    P = ip.randomised(c["world"], B, seed=0x11AC)
    got = lc.emu_links(c["world"], c["dis"], c["vel"], par=(P["mass"], P["com"]))
    plain = lc.emu_links(c["world"], c["dis"], c["vel"])
    for k in ("R", "p", "v"):
        assert np.array_equal(got[k], plain[k]), k
    assert np.abs(got["com"] - plain["com"]).max() > 1e-5
    lc.check(got, lc.reference(R, oracle_cls, c["world"], c["dis"], c["vel"], mass=P["mass"], com=P["com"]), "humanoid30 + table")


def test_emulated_readout_after_joints_broke_in_a_run(R, oracle_cls):
    """a state the step leaves, not a draw: the wall hit by the box (tests/test_emu_parity.py), stepped under the emulator until
    joints have broken during the run; the read-out of that state against the oracle at the same state AND broken flags"""
    from emu import EmuBatch
    dis, vel, br, world = lc.wall_after_steps(R, lambda w, B, mr: EmuBatch(w, B, max_rigid=mr), 18)
    lc.check(lc.emu_links(world, dis, vel), lc.reference(R, oracle_cls, world, dis, vel, br), "wall after 18 steps")


def test_emulated_flags_select_what_is_written(R, worlds):
    c = worlds["humanoid30"]
    full = lc.emu_links(c["world"], c["dis"], c["vel"])
    for flags in (lc.POSE, lc.VEL, lc.COM, lc.POSE | lc.COM):
        got = lc.emu_links(c["world"], c["dis"], c["vel"], flags=flags)
        for k, x in got.items():
            assert np.array_equal(x, full[k]), (flags, k)
