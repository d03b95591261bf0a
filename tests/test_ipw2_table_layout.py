"""The LDS layouts after the world's static tables (candidate info, link info, child / pool table, face offsets, path table) left
the LDS of the kernel with two instances per wavefront: it reads them from the device model in global memory (rkfdDevModel.tabs).
The headline world then keeps full contact-matrix rows at two per wavefront and gains the sixth wavefront per CU; the one-instance
layouts do not move, and the box cases of the solver-path matrix keep the packed triangle.  CPU only (the device-model builder
through the lane emulator's harness, rkfd_emu_layout)."""
import re

import pytest

import solver_paths as sp

PIECE, PIECES_PER_CU = 1280, 128      # how the hardware hands out LDS (profiles/r01_lds_residency.txt)


def slots(workgroup_bytes):
    return PIECES_PER_CU // -(-workgroup_bytes // PIECE)


def test_config4_two_per_wavefront_keeps_full_rows_and_six_wavefronts(R):
    sc = R.scenarios.CONFIGS["config4"](batch=8)
    lay = sp.devmodel_layout(sc["world"].model, sc["max_rigid"], 2)
    assert lay == (0, 0, 576, 13280, 0)          # no Vert QP, full rows (9 x 8^2 doubles), 13 280 B, nothing shared in LDS
    assert slots(2 * lay[3]) == 6


@pytest.mark.parametrize("name, lds", [("config2", 13360), ("config3", 14416), ("config4", 13888), ("config4v", 18240), ("config5", 52608)])
def test_one_instance_layouts_do_not_move(R, name, lds):
    sc = R.scenarios.CONFIGS[name](batch=8)
    assert R.lib().rkfdLdsBytesFor(sc["world"].model, sc["max_rigid"]) == lds
    assert sp.devmodel_layout(sc["world"].model, sc["max_rigid"], 1)[3] == lds


# capacity -> workgroup bytes of the two-instance box cases with the packed triangle
BOX_WG = {5: 10336, 7: 15616, 9: 20128, 12: 28000, 16: 41920}


@pytest.mark.parametrize("case", [c for c in sp.CASES if c.ipw == 2], ids=lambda c: c.name)
def test_two_instance_box_cases_stay_packed(R, tmp_path, capfd, monkeypatch, case):
    """packed where it gains a wavefront per CU; the full-row bytes are the builder's own first pass (RKFD_DEVMODEL_DUMP)"""
    assert case.path == "dpp_packed" and case.cap in BOX_WG
    w, *_ = case.build(R, tmp_path)
    monkeypatch.setenv("RKFD_DEVMODEL_DUMP", "1")
    capfd.readouterr()
    vr, packed, ma_size, lds, _ = sp.devmodel_layout(w.model, case.cap, 2)
    passes = [int(n) for n in re.findall(r"-> (\d+) B of LDS", capfd.readouterr().err)]
    assert (vr, packed) == (0, 1)
    assert ma_size == 3 * case.cap * (3 * case.cap + 1) // 2
    assert len(passes) == 2 and passes[1] == lds          # full rows, then the packed triangle the builder kept
    assert 2 * lds == BOX_WG[case.cap]
    assert slots(2 * lds) > slots(2 * passes[0])
