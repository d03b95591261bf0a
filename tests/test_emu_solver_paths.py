"""Every contact-solve path of the step kernel (tests/solver_paths.py) under the lane emulator against the oracle, without a
GPU: the first evaluation and two steps, one instance per wavefront (batch 1) or two (batch 2, the emulator's RKFD_W = 2
build).  The MFMA Gram product of the Vert QP is compiled out of the emulator: the GPU matrix
(tests/test_gpu_solver_paths.py) covers it."""
import pytest

import solver_paths as sp
from emu import EmuBatch

NSTEPS = 2


@pytest.mark.parametrize("case", sp.CASES, ids=sp.CASE_IDS)
def test_emulated_path_matches_oracle(R, tmp_path, case):
    w, dis, vel, _ = case.build(R, tmp_path)
    B = case.ipw
    d, v = sp.states(dis, vel, B)
    ors = sp.oracles(w, d, v)
    sp.check_path(R, case, w, ors[0])
    eb = EmuBatch(w, B, max_rigid=case.cap, ipw=case.ipw)
    eb.set_state(d, v)
    eb.update_init()
    assert eb.status() == 0
    sp.compare(eb, ors, f"{case.name}: first evaluation")
    eb.update(NSTEPS)
    assert eb.status() == 0
    for o in ors:
        o.update_n(NSTEPS)
    sp.compare(eb, ors, f"{case.name}: {NSTEPS} steps")
