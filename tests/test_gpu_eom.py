"""The residual of the equation of motion (tests/eom_cases.py) on the MI355X: what a batch reports after rkfdBatchEval - the
accelerations, the contact force of every candidate vertex, the motor inputs - must balance in tests/refmath.py's independent
Newton-Euler inverse dynamics, in the generic kernel, the world-specific kernel, two instances per wavefront where the world
is eligible, and split launches.  No oracle output is compared; the oracle only sets the tolerance (10x its own residual per
case family, at least 1e-12).  tests/test_emu_eom.py is the same check without a GPU."""
import pytest

import eom_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shared_tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("eom")


def _batch(R, su, kernel):
    b = R.Batch(su.world, ec.B, device=0, max_rigid=su.max_rigid)
    try:
        if kernel == "ipw2":
            try:
                b.set_instances_per_wave(2)
            except R.RkfdError as e:
                assert "two instances per wavefront need" in str(e)
                pytest.skip("this world is not eligible for two instances per wavefront")
        if kernel in ("spec", "ipw2"):
            b.specialize()
            assert b.instances_per_wave() == (2 if kernel == "ipw2" else 1)
        if kernel == "split3":
            b.set_split(3)
        ec.apply_params(b, su)
        return b
    except BaseException:
        b.close()
        raise


def _check(R, oracle_cls, tmp, case, kernel):
    tol = ec.family_tolerance(R, oracle_cls, tmp, case.family)
    su = case.build(R, tmp)
    b = _batch(R, su, kernel)
    try:
        out, first = ec.run(su, b)
    finally:
        b.close()
    worst, nact = ec.check(su, out, first, tol)
    print(f"EOM {case.name:36s} {kernel:8s} gpu {worst:.2e} oracle {ec.oracle_residuals(R, oracle_cls, tmp)[case.name]:.2e} allowed {tol:.2e} active {nact}")
    assert (nact > 0) == case.contacts


@pytest.mark.parametrize("kernel", ["generic", "spec", "ipw2"])
@pytest.mark.parametrize("case", ec.CASES, ids=ec.CASE_IDS)
def test_gpu_balances(R, oracle_cls, shared_tmp, case, kernel):
    _check(R, oracle_cls, shared_tmp, case, kernel)


def test_gpu_balances_under_split_launches(R, oracle_cls, shared_tmp):
    """three instances as three launches on internal streams"""
    _check(R, oracle_cls, shared_tmp, ec.case("mlcp_arm_press_revolute"), "split3")
