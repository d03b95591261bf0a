"""The path helper (tests/solver_paths.py) against what the device-model builder picks: its Vert variants, the storage of the
contact matrix, the LDS an instance needs, and the contact counts and components of the path scenes.  CPU only: when the
dispatch changes, these fail before any GPU run."""
import re

import pytest

import solver_paths as sp


@pytest.mark.parametrize("case", sp.CASES, ids=sp.CASE_IDS)
def test_case_reaches_its_path(R, oracle_cls, tmp_path, case):
    """every case of the emulator / GPU matrices holds its contact count at the first evaluation and reaches its path"""
    w, dis, vel, exp = case.build(R, tmp_path)
    o = oracle_cls(w.model)
    o.set_state(dis, vel)
    o.update_init()
    comps = sp.check_path(R, case, w, o)
    assert sorted(comps) == sorted(exp)
    vr, packed, ma_size, lds, _ = sp.devmodel_layout(w.model, case.cap, case.ipw)
    if case.plugin == "vert":
        assert vr == sp.vert_variant(case.pyramid or 8, case.cap) and not packed
    else:
        assert vr == 0
        assert not packed or sp.packing_considered("mlcp", case.ipw, case.cap)
        assert ma_size == (3 * case.cap * (3 * case.cap + 1) // 2 if packed else 9 * case.cap * case.cap)
    assert lds <= sp.LDS_LIMIT


@pytest.mark.parametrize("pyramid", [4, 6, 8])
def test_vert_variant_rule_matches_the_builder(R, capfd, monkeypatch, pyramid):
    """vert_variant over every capacity the active set allows (pyramid x max_rigid <= 192, 3 max_rigid <= 128), against the
    builder's dump (RKFD_DEVMODEL_DUMP) and its layout"""
    w, *_ = sp.box_scene(R, ["flat"], solver="vert", pyramid=pyramid)
    monkeypatch.setenv("RKFD_DEVMODEL_DUMP", "1")
    seen = set()
    for cap in range(1, min(192 // pyramid, 128 // 3) + 1):
        capfd.readouterr()
        n = R.lib().rkfdLdsBytesFor(w.model, cap)
        err = capfd.readouterr().err
        got = [int(v) for v in re.findall(r" vert (\d+) ", err)]
        assert got and got[-1] == sp.vert_variant(pyramid, cap), (cap, err)
        lay = sp.devmodel_layout(w.model, cap)
        assert lay[0] == sp.vert_variant(pyramid, cap) and lay[3] == n
        seen.add(lay[0])
    assert seen == ({1, 2, 3} if pyramid < 8 else {2, 3})


def test_packing_rule_matches_the_builder(R):
    """full rows wherever the builder does not weigh the packed triangle (one instance per wavefront up to a capacity of 16);
    where it does, both storages occur over the capacities; rkfdLdsBytesFor reports the builder's bytes"""
    w, *_ = sp.box_scene(R, ["flat"] * 4)
    seen = set()
    for ipw in (1, 2):
        for cap in range(1, 43 if ipw == 1 else 17):
            vr, packed, ma_size, lds, shared = sp.devmodel_layout(w.model, cap, ipw)
            assert vr == 0
            if not sp.packing_considered("mlcp", ipw, cap):
                assert not packed and ma_size == 9 * cap * cap, (ipw, cap)
            else:
                seen.add(packed)
            if ipw == 1:
                assert R.lib().rkfdLdsBytesFor(w.model, cap) == lds
    assert seen == {0, 1}


def test_mlcp_path_rules():
    """the dispatch restated, at its edges"""
    P = sp.mlcp_path
    assert P(4, 4, "full", 1, [4])[0] == "registers" and P(4, 24, "packed", 1, [4])[0] == "registers"
    assert P(8, 24, "packed", 1, [4, 4])[0] == "dpp8"
    assert P(5, 24, "packed", 1, [4, 1])[0] == "general_packed" and P(5, 16, "packed", 2, [4, 1])[0] == "dpp_packed"
    assert P(16, 16, "full", 1, [16])[0] == "dpp_full"
    assert P(17, 24, "packed", 1, [4, 4, 4, 4, 1]) == ("grouped_sw", (5, 4, 4, 4))
    assert P(17, 24, "packed", 1, [17])[0] == "general_packed"               # one component of 17: fits = false
    assert P(32, 32, "packed", 1, [4] * 8) == ("grouped_sw", (8, 8, 8, 8))
    assert P(32, 32, "packed", 1, [4] * 8, debug_variants=32)[0] == "grouped_packed"
    assert P(32, 32, "packed", 1, [4] * 8, debug_variants=8)[0] == "general_packed"
    assert P(40, 40, "full", 1, [4] * 10) == ("grouped_full", (12, 12, 8, 8))
    assert P(36, 40, "full", 1, [16, 16, 4])[1] == (16, 16, 4, 0)
    assert sp.row_fills([12, 12, 12, 12, 12]) is None                     # a fifth 12 finds no row with room
    assert sp.probe_passes(21) == 1 and sp.probe_passes(22) == 2 and sp.probe_passes(42) == 2
    assert sp.row_stride(40, 40) == 120 and sp.row_stride(39, 40) == 118
    assert sp.vert_mfma_tiles(5, 8, 8) == ("c00",) and sp.vert_mfma_tiles(6, 8, 8) == ("c00", "c01", "c11")
    assert sp.vert_mfma_tiles(11, 4, 16) == () and sp.vert_mfma_tiles(5, 8, 24) == ()


def test_lds_limit_of_many_contacts(R):
    """ten boxes (60 joint coordinates, the most that fit a wavefront) at the largest capacity, 42 contacts (126 MLCP rows),
    need 163 536 bytes of LDS per instance: 304 below the 160 KiB rkfdBatchCreate allows, so the whole range of capacities
    is usable with full rows (case mlcp_grouped_full_nc40_lds_edge).  The Vert plugin's QP at a capacity of 32 needs more
    than 160 KiB, which rkfdBatchCreate refuses (tests/test_gpu_solver_paths.py)"""
    L = R.lib()
    w10, *_ = sp.box_scene(R, ["flat"] * 10)
    assert L.rkfdLdsBytesFor(w10.model, 40) <= L.rkfdLdsBytesFor(w10.model, 42) <= sp.LDS_LIMIT
    wv, *_ = sp.box_scene(R, ["flat"], solver="vert", pyramid=4)
    assert L.rkfdLdsBytesFor(wv.model, 24) <= sp.LDS_LIMIT < L.rkfdLdsBytesFor(wv.model, 32)
