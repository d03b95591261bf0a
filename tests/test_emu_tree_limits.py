"""The tree-size limits of the one-wavefront mapping under the lane emulator (tests/tree_limits.py): every accepted case against
the oracle - step state within 1e-8 max( 1, |ref|_inf ) after two steps, contact activity equal, the task-space read-out within its
1e-12 - with the oracle-alone control (plain build against the build with fused multiply-adds, below 1e-9) that makes the bound a
statement about the device code and not about the world; and the refusals just beyond the limits, with the builder's message."""
import numpy as np
import pytest

import links_cases as lc
import tree_limits as tl
from emu import EmuBatch

B = 2


def _emu_steps(w, dis, vel, max_rigid, ipw=1, nsteps=tl.NSTEPS):
    eb = EmuBatch(w, dis.shape[0], max_rigid=max_rigid, ipw=ipw)
    eb.set_state(dis, vel); eb.update_init(); eb.update(nsteps)
    assert eb.status() == 0
    return eb


@pytest.mark.parametrize("case", tl.FREE, ids=repr)
def test_free_motion_at_the_limits(R, oracle_cls, tmp_path, case):
    w = tl.world(R, case, tmp_path)
    dis, vel = tl.states(w, B)
    ref = tl.oracle_run(oracle_cls, w, dis, vel)
    ctl = tl.control(oracle_cls, w, dis, vel, ref)
    eb = _emu_steps(w, dis, vel, 0)
    dev = tl.deviation(eb.get_state(), ref)
    print(f"{case.name}: control {ctl:.2e} emulator {dev:.2e}")
    assert ctl < tl.CONTROL_TOL, (case.name, ctl)
    assert dev < tl.STEP_TOL, (case.name, dev)
    if case.ipw2:
        e2 = _emu_steps(w, dis, vel, 0, ipw=2)
        for x, y in zip(e2.get_state(), eb.get_state()):
            assert np.array_equal(x, y), case.name
    # the read-out at the stepped state (96 model links out of 64 lanes, poses through six rounds)
    d1, v1, _ = eb.get_state()
    lc.check(lc.emu_links(w, d1, v1), lc.reference(R, oracle_cls, w, d1, v1), case.name)
    lc.check_positions_second_fk(R, w, d1, lc.emu_links(w, d1, v1), case.name)


@pytest.mark.parametrize("solver", ["mlcp", "vert"])
@pytest.mark.parametrize("case", tl.CONTACT, ids=repr)
def test_contacts_on_deep_links(R, oracle_cls, tmp_path, case, solver):
    w, h, dis, vel = tl.seated_world(R, case, tmp_path, B, solver=R.SOLVER_MLCP if solver == "mlcp" else R.SOLVER_VERT)
    m = w.model.contents
    assert m.ndof == case.dims[2] and m.ncand == 16 * len(case.boxes)          # (8 vertices of each box and 8 of the floor per pair)
    ref1 = tl.oracle_run(oracle_cls, w, dis, vel, nsteps=1)
    ref = tl.oracle_run(oracle_cls, w, dis, vel)
    ctl = tl.control(oracle_cls, w, dis, vel, ref)
    eb1 = _emu_steps(w, dis, vel, 16, nsteps=1)
    eb = _emu_steps(w, dis, vel, 16)
    dev = tl.deviation(eb.get_state(), ref)
    print(f"{case.name} {solver}: control {ctl:.2e} emulator {dev:.2e}")
    for r, e in ((ref1, eb1), (ref, eb)):
        act, typ, _, f = e.get_contact()
        for i, (_, (oact, otyp, _, of)) in enumerate(r):
            # the deep probe walks run on more than one side: at least two links in rigid contact over the compared steps
            assert len(tl.rigid_links_in_contact(m, oact, h)) >= 2, (case.name, i)
            assert (act[i] == oact).all() and (typ[i] == otyp * (oact != 0)).all(), (case.name, i)
            assert tl.relerr(f[i], of) < tl.STEP_TOL, (case.name, i)
    assert ctl < tl.CONTROL_TOL, (case.name, ctl)
    # (the narrowest case: chain59f_boxes under MLCP measures 8.2e-9 here, profiles/r07_tree_limits.txt - the first to watch when
    #  the summation order of the contact solve changes)
    assert dev < tl.STEP_TOL, (case.name, dev)


@pytest.mark.parametrize("case,ipw,msg", tl.REFUSED, ids=lambda x: repr(x) if isinstance(x, (tl.Case, int)) else "msg")
def test_refused_beyond_the_limits(R, tmp_path, case, ipw, msg):
    """the host-only entry points that build the device model refuse with the builder's message; so does the emulator"""
    import re
    w = R.World(solver=R.SOLVER_MLCP)
    w.reg_file(tl.write(case, tmp_path))
    m = w.model.contents
    assert m.nlink == case.dims[0] and m.ndof == case.dims[2]
    L = R.lib()
    if ipw == 1:
        assert L.rkfdLdsBytesFor(w.model, 0) == -1
        with pytest.raises(RuntimeError, match="device model build failed"):
            EmuBatch(w, 1, max_rigid=0).update_init()
    else:
        assert L.rkfdLdsBytesFor(w.model, 0) > 0                    # one instance per wavefront takes it
        assert L.rkfdSpecializeCompileW(w.model, 0, 2) == -1        # (refused before any compiler is asked)
    assert re.search(msg, L.rkfdHipLastError().decode()), L.rkfdHipLastError()
