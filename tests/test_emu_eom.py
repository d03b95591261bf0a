"""The residual of the equation of motion (tests/eom_cases.py) under the lane emulator and on the oracle, without a GPU:
the accelerations, contact forces and motor inputs a batch reports after an evaluation must balance in tests/refmath.py's
independent Newton-Euler inverse dynamics, on every joint coordinate of every case - and a perturbed copy of the outputs must not.
The cases with a table of per-instance parameters run on the emulator class of tests/test_emu_params.py.
tests/test_gpu_eom.py repeats this on the GPU."""
import os

import numpy as np
import pytest

import eom_cases as ec
import refmath as rm
from emu import EmuBatch

PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r07_eom_residuals.txt")


@pytest.fixture(scope="module")
def shared_tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("eom")


_emu_runs = {}


def _emu_run(R, case, tmp):
    """(setup, read-out, read-out after update_init) of a case under the emulator, run once per session"""
    if case.name not in _emu_runs:
        su = case.build(R, tmp)
        _emu_runs[case.name] = (su,) + ec.run(su, _emu_batch(su))
    return _emu_runs[case.name]


def _emu_batch(su):
    if su.params is not None:
        from test_emu_params import ParEmuBatch
        return ParEmuBatch(su.world, ec.B, max_rigid=su.max_rigid, params=su.params)
    return EmuBatch(su.world, ec.B, max_rigid=su.max_rigid)


def test_oracle_residuals_are_rounding(R, oracle_cls, shared_tmp):
    """the oracle's own residual, per case: the yardstick of the tolerance.  Beyond 1e-8 it would be a finding to explain."""
    res = ec.oracle_residuals(R, oracle_cls, shared_tmp)
    for name, v in res.items():
        print(f"{name:36s} oracle {v:.2e}")
        assert v < ec.ORACLE_LIMIT, name
    for fam in ec.FAMILIES:
        print(f"family {fam:16s} allowed {ec.family_tolerance(R, oracle_cls, shared_tmp, fam):.2e}")


@pytest.mark.parametrize("case", ec.CASES, ids=ec.CASE_IDS)
def test_emulated_kernel_balances(R, oracle_cls, shared_tmp, case):
    tol = ec.family_tolerance(R, oracle_cls, shared_tmp, case.family)
    su, out, first = _emu_run(R, case, shared_tmp)
    worst, nact = ec.check(su, out, first, tol)
    print(f"{case.name:36s} oracle {ec.oracle_residuals(R, oracle_cls, shared_tmp)[case.name]:.2e} emulator {worst:.2e} allowed {tol:.2e} active {nact}")
    assert (nact > 0) == case.contacts


def test_cases_cover_every_joint_kind_and_motor_type(R, shared_tmp):
    """read from the models, so that a change to a generator cannot hollow the cases out: every joint kind of rkfd_model.h, each
    motor type, prismatic joints and merged fixed links in the random trees, a friction-free tree with DC motors, every family
    meant to have contacts marked so"""
    jt, mt = set(), set()
    tree_jt, tree_merged = set(), 0
    for c in ec.CASES:
        su = c.build(R, shared_tmp)
        m = su.world.model.contents
        j, t, par = m.arr("jtype", m.nlink), m.arr("mtype", m.nlink), m.arr("parent", m.nlink)
        jt |= {int(x) for x in j}; mt |= {int(x) for x in t[(j == rm.REVOL) | (j == rm.PRISM)]}
        if "tree" in c.name:
            tree_jt |= {int(x) for x in j}; tree_merged += int(((j == rm.FIXED) & (par >= 0)).sum())
            assert 8 <= m.nlink <= 20
        if c.name == "free_tree_fixed16_nofriction":
            md = rm.model_arrays(m)
            assert not any(np.abs(md[k]).max() for k in ("stiff", "visc", "coulomb", "sfric")) and (t == rm.MOTOR_DC).sum() >= 2
        if c.family in ("free", "params") and "tree" in c.name and c.name != "free_tree_fixed16_nofriction":
            md = rm.model_arrays(m)
            assert ((t == rm.MOTOR_DC) & (md["sfric"] > 0)).any(), c.name
    assert jt == {rm.FIXED, rm.REVOL, rm.PRISM, rm.FLOAT, rm.SPHER, rm.BRFLOAT}
    assert mt == {rm.MOTOR_NONE, rm.MOTOR_TRQ, rm.MOTOR_DC}
    assert {rm.FIXED, rm.REVOL, rm.PRISM, rm.FLOAT} <= tree_jt and tree_merged > 0
    for fam in ("mlcp", "vert", "penalty", "self", "spher_contact"):
        assert all(c.contacts for c in ec.CASES if c.family == fam)
    assert any(c.contacts for c in ec.CASES if c.family == "params")


def _perturbed(su, out, kind):
    """a copy of the outputs with one thing wrong; -> (out, keyword arguments of check_instance, instance)"""
    tb = ec.Tables(su.world.model.contents)
    o = {k: v.copy() for k, v in out.items()}
    i = 0
    res = ec.residual(su, tb, i, out)
    if kind == "force_negated":
        j = int(np.argmax(np.abs(out["f"][i]).sum(1)))          # the contact that carries the most
        assert np.abs(out["f"][i][j]).sum() > 0.1
        o["f"][i][j] *= -1.0
        return o, {}, i
    if kind == "reaction_dropped":
        j2 = [j for j in np.nonzero(out["act"][i])[0] if not tb.floor[tb.other[j]] and np.abs(out["f"][i][j]).sum() > 0.1]
        return o, dict(drop_reaction=int(j2[0])), i             # a reaction that lands on a moving link
    if kind == "qdd_shifted":
        bound = ec.friction_bounds(res["md"], tb, out["dis"][i], out["vel"][i], out["piv"][i])
        k = [k_ for k_ in range(len(bound)) if bound[k_] is None][0]
        o["acc"][i][k] += 1e-6 * res["s"]
        return o, {}, i
    if kind == "rotor_omitted":
        return o, dict(rotor=False), i
    raise KeyError(kind)


# config 4 and arm_press, each with the four perturbations - but for two that cannot show on config 4 whatever the check: the
# second body of every pair of config 4 is the floor, on which a dropped reaction does no work (it runs on the stacked
# boxes, whose pairs have two moving sides; the boxes of config 5 lie beside the feet, not under them), and every DC-motor joint of the humanoid carries joint friction, whose torque the ABI does
# not report, so its coordinates are held to a bound that a rotor term of gear^2 J qdd = 6e-3 kg m^2 x qdd stays inside (it
# runs on the friction-free random tree, whose DC-motor joints are checked by equality)
TEETH = [("mlcp_config4", "force_negated"), ("mlcp_stacked_boxes", "reaction_dropped"), ("mlcp_config4", "qdd_shifted"),
         ("free_tree_fixed16_nofriction", "rotor_omitted"),
         ("mlcp_arm_press_fixed", "force_negated"), ("mlcp_arm_press_fixed", "reaction_dropped"), ("mlcp_arm_press_fixed", "qdd_shifted"),
         ("mlcp_arm_press_fixed", "rotor_omitted")]


@pytest.mark.parametrize("name,kind", TEETH, ids=[f"{n}-{k}" for n, k in TEETH])
def test_a_perturbed_copy_fails(R, oracle_cls, shared_tmp, name, kind):
    """the check has teeth: one contact force negated, one reaction left out, one acceleration shifted by 1e-6 of the scale, the
    rotor inertia left out - each fails the assertion the unperturbed outputs pass"""
    case = ec.case(name)
    tol = ec.family_tolerance(R, oracle_cls, shared_tmp, case.family)
    su, out, first = _emu_run(R, case, shared_tmp)
    tb = ec.Tables(su.world.model.contents)
    ec.check_instance(su, tb, 0, out, tol)
    bad, kw, i = _perturbed(su, out, kind)
    with pytest.raises(AssertionError, match="residual|friction torque|floor pulls|friction cone"):
        ec.check_instance(su, tb, i, bad, tol, **kw)


def test_write_profile(R, oracle_cls, shared_tmp):
    """RKFD_EOM_PROFILE=1: (re)write the CPU columns of profiles/r07_eom_residuals.txt; otherwise only check it lists every case"""
    if os.environ.get("RKFD_EOM_PROFILE"):
        res = ec.oracle_residuals(R, oracle_cls, shared_tmp)
        lines = ["# worst relative residual of the equation of motion per case (tests/eom_cases.py): max |r| / s over the coordinates that",
                 "# must close and the 3 instances.  oracle, emulator: x86-64 host.  The GPU figures are printed by tests/test_gpu_eom.py",
                 "# (pytest -s, lines starting with EOM) and are not recorded here yet.  allowed = max(1e-12, 10 x the oracle's worst of the family).",
                 f"# {'case':34s} {'family':14s} {'oracle':>9s} {'emulator':>9s} {'allowed':>9s}"]
        for c in ec.CASES:
            su, out, first = _emu_run(R, c, shared_tmp)
            tol = ec.family_tolerance(R, oracle_cls, shared_tmp, c.family)
            lines.append(f"{c.name:36s} {c.family:14s} {res[c.name]:9.2e} {ec.check(su, out, first, tol)[0]:9.2e} {tol:9.2e}")
        open(PROFILE, "w").write("\n".join(lines) + "\n")
    txt = open(PROFILE).read()
    assert all(c.name in txt for c in ec.CASES)
