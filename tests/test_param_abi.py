"""Per-instance physical parameters: what can be checked without a GPU - the library exports the calls and the header declares
them, the widths, the binding's surface, and the worlds the parameter tests randomise have what those tests claim to exercise."""
import os
import re

import numpy as np
import pytest

import instance_params as ip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["rkfdSpecializeCompileP", "rkfdBatchParamWidth", "rkfdBatchSetParam", "rkfdBatchGetParam", "rkfdBatchClearParams", "rkfdBatchHasParams",
        "rkfdNodeSetParam", "rkfdNodeClearParams"]


def test_library_exports_and_header_declares(R):
    L = R.lib()
    hdr = open(os.path.join(ROOT, "include", "rkfd_hip.h")).read()
    for s in SYMS:
        assert hasattr(L, s), s
        assert re.search(r"\b%s\s*\(" % s, hdr), s
    keys = re.search(r"enum \{ (RKFD_PAR_MASS.*?RKFD_PAR_COUNT) \}", hdr, re.S).group(1)
    names = re.findall(r"RKFD_PAR_(\w+)", keys)
    assert [n.lower() for n in names[:-1]] == list(ip.NAMES) and names[-1] == "COUNT"
    assert tuple(R.binding.PARAM_NAMES) == ip.NAMES


def test_width_of_a_null_batch_and_bad_keys(R):
    L = R.lib()
    assert L.rkfdBatchParamWidth(None, 0) == -1
    assert L.rkfdBatchHasParams(None) == 0
    assert L.rkfdBatchSetParam(None, 0, None) == -1 and L.rkfdHipLastError()
    with pytest.raises(ValueError):
        R.binding.param_key("weight")
    assert [R.binding.param_key(n) for n in ip.NAMES] == list(range(13))


def test_binding_methods_exist(R):
    for f in ("set_param", "get_param", "clear_params", "has_params", "param_width"):
        assert callable(getattr(R.Batch, f)), f
    for f in ("set_param", "clear_params"):
        assert callable(getattr(R.Node, f)), f


def test_helper_widths_match_the_documented_ones(R):
    sc = R.scenarios.config4(batch=1)
    m = sc["world"].model.contents
    for k, n in enumerate(ip.NAMES):
        want = m.nci if n.startswith("ci_") else m.nlink * {"com": 3, "inertia": 9}.get(n, 1)
        assert ip.width(m, n) == want


def test_randomised_worlds_have_a_merged_massive_link_and_model_copy_holds(R):
    """config 4 (the humanoid): the fixed soles the device merges into the feet are among the randomised links, with a mass;
    model_with leaves the world alone and the copy carries the override"""
    sc = R.scenarios.config4(batch=3)
    w = sc["world"]
    mass = ip.model_values(w, "mass")
    merged = ip.merged_links(w)
    assert merged, "no link on a fixed joint below a parent"
    P = ip.randomised(w, 3, seed=5)
    assert all((P["mass"][:, i] != mass[i]).all() and (P["mass"][:, i] > 0).all() for i in merged)
    assert set(P) == set(ip.NAMES)
    mc = ip.model_with(w, ip.of_instance(P, 1))
    got = mc.model.contents.arr("mass", w.model.contents.nlink)
    assert np.array_equal(got, P["mass"][1]) and np.array_equal(ip.model_values(w, "mass"), mass)
    assert mc.model.contents.nlink == w.model.contents.nlink and mc.model.contents.dt == w.model.contents.dt
    # the device-model builder accepts the copy and sizes it as the world (parameters change no layout)
    L = R.lib()
    assert L.rkfdLdsBytesFor(mc.model, sc["max_rigid"]) == L.rkfdLdsBytesFor(w.model, sc["max_rigid"]) > 0


@pytest.mark.parametrize("world,ipw", [("config4", 1), ("config4", 2), ("config5", 1)])
def test_table_kernels_are_ahead_of_time_and_within_budget(R, world, ipw):
    """`make spec` leaves the world-specific kernels for batches WITH a table in the store too (the first rkfdBatchSetParam on a
    specialised batch of a baseline world loads a file, no run-time compile), and they keep the budget of their plain
    counterparts (tests/test_build_resources.py): three waves per SIMD and no vector spills with one instance per wavefront, two
    waves with two."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("spec_resources", os.path.join(ROOT, "tools", "spec_resources.py"))
    sr = importlib.util.module_from_spec(spec); spec.loader.exec_module(sr)
    sc = sr.world(world)
    L = R.lib()
    assert L.rkfdSpecializeCompileP(sc["world"].model, sc["max_rigid"], ipw, 1) > 10000
    assert L.rkfdSpecializeLastFromStore() == 1
    r = sr.resources(sc, ipw, 1)
    print(world, ipw, r)
    assert r["vgpr"] <= (168 if ipw == 1 else 256) and r["vgpr_spill"] == 0 and r["scratch"] <= 64, r
