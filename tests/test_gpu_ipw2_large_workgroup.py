"""Two instances per wavefront with a workgroup above 64 KiB of LDS: rkfdBatchSpecialize gives the module's kernel the
dynamic-LDS attribute there, and the launch must go through and give the bits of one instance per wavefront.  The workgroup
is pushed over 64 KiB with the diagnostic pad RKFD_LDS_PAD_BYTES (added to every workgroup, either mapping), kept small
enough that one instance per wavefront stays within the 64 KiB rkfdBatchSpecialize accepts."""
import numpy as np
import pytest

import solver_paths as sp

B = 5           # odd: the last wavefront of two carries a stand-in half
SPEC_LDS = 64 * 1024


@pytest.mark.gpu
def test_two_instances_above_64k_of_lds_match_one(R, monkeypatch):
    w, dis, vel, _ = sp.box_scene(R, ["flat", "vertex"])
    cap = 5
    lds1 = sp.devmodel_layout(w.model, cap, 1)[3]
    lds2 = sp.devmodel_layout(w.model, cap, 2)[3]
    pad = SPEC_LDS - lds1
    assert 2 * lds2 + pad > SPEC_LDS
    monkeypatch.setenv("RKFD_LDS_PAD_BYTES", str(pad))
    d, v = sp.states(dis, vel, B)
    out = []
    for ipw in (1, 2):
        b = R.Batch(w, B, device=0, max_rigid=cap)
        try:
            assert b.lds_bytes == SPEC_LDS
            if ipw == 2:
                b.set_instances_per_wave(2)
            b.specialize()
            assert b.instances_per_wave() == ipw
            b.set_state(d, v)
            b.update_init()
            b.update(6)
            assert b.status() == 0
            out.append(b.get_state() + b.get_contact())
        finally:
            b.close()
    for x, y in zip(*out):
        assert np.array_equal(x, y)
