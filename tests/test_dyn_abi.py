"""The joint-space dynamics' surface without a GPU: exports, declarations, loud failures, bindings, and the compiler's resource
report of the new kernel (roki-fd_amd/kernel_resources_dyn.txt) beside the untouched reports of the step kernels, the read-out, the
reset and the Jacobians - line for line what the build gave before the dynamics existed (tests/golden/kernel_reports_before_dyn/)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rkfdBatchUpdateDynamics", "rkfdBatchGetDynamics", "rkfdBatchDevMassMatrix", "rkfdBatchDevBias", "rkfdBatchDevGravity", "rkfdNodeGetDynamics")
OTHER_REPORTS = ("kernel_resources.txt", "kernel_resources_par.txt", "kernel_resources_links.txt", "kernel_resources_reset.txt", "kernel_resources_jac.txt")
UNCHANGED = ("kernel_resources.txt", "kernel_resources_links.txt", "kernel_resources_reset.txt", "kernel_resources_jac.txt")


def _report(name):
    out, cur = {}, None
    for line in open(os.path.join(ROOT, "roki-fd_amd", name)):
        m = re.match(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.match(r"\s*(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


def test_exports_and_header(R):
    L = C.CDLL(R.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "rkfd_hip.h")).read()
    for n in NEW:
        assert hasattr(L, n), n
        assert re.search(r"\b%s\s*\(" % n, hdr), n
    assert re.search(r"RKFD_DYN_MASS = 1, RKFD_DYN_BIAS = 2, RKFD_DYN_GRAVITY = 4, RKFD_DYN_ROTOR = 8", hdr)
    assert (R.DYN_MASS, R.DYN_BIAS, R.DYN_GRAVITY, R.DYN_ROTOR, R.DYN_ALL) == (1, 2, 4, 8, 7)
    # the accessors' ordering comment names the launch
    assert re.search(r"Restore / Reset\[Dev\] / UpdateLinks / UpdateJacobians / UpdateDynamics\)", hdr)


def test_null_fails_with_a_message(R):
    L = R.lib()
    buf = (C.c_double * 16)()
    assert L.rkfdBatchUpdateDynamics(None, 7, None) == -1 and b"rkfdBatchUpdateDynamics: null batch" in L.rkfdHipLastError()
    assert L.rkfdBatchGetDynamics(None, buf, None, None) == -1 and b"rkfdBatchGetDynamics: null batch" in L.rkfdHipLastError()
    assert L.rkfdNodeGetDynamics(None, 7, None, None, None) == -1 and b"rkfdNodeGetDynamics: null node" in L.rkfdHipLastError()
    assert L.rkfdBatchDevMassMatrix(None) is None and L.rkfdBatchDevBias(None) is None and L.rkfdBatchDevGravity(None) is None


def test_bindings_exist(R):
    for n in ("update_dynamics", "get_dynamics", "dynamics_tensors", "dynamics_ptrs"):
        assert callable(getattr(R.Batch, n))
    assert callable(R.Node.get_dynamics)
    a = R.binding._dyn_arrays(3, 5, R.DYN_MASS | R.DYN_GRAVITY)
    assert {k: v.shape for k, v in a.items()} == {"M": (3, 5, 5), "g": (3, 5)}


def test_dyn_kernel_report(R):
    k = _report("kernel_resources_dyn.txt")
    assert set(k) == {"rkfd_dyn_kernel"}
    assert k["rkfd_dyn_kernel"]["VGPRs Spill"] == 0 and k["rkfd_dyn_kernel"]["SGPRs Spill"] == 0 and k["rkfd_dyn_kernel"]["ScratchSize [bytes/lane]"] == 0, k


def test_dyn_kernel_is_in_no_other_report(R):
    for name in OTHER_REPORTS:
        assert "rkfd_dyn_kernel" not in open(os.path.join(ROOT, "roki-fd_amd", name)).read(), name


@pytest.mark.parametrize("name", UNCHANGED)
def test_other_reports_are_what_they_were(R, name):
    """a regression guard (it passes without the feature): the reports of the step kernels, the read-out, the reset and the
    Jacobians, line for line as the build wrote them before the dynamics' translation unit was added"""
    got = open(os.path.join(ROOT, "roki-fd_amd", name)).read().splitlines()
    want = open(os.path.join(ROOT, "tests", "golden", "kernel_reports_before_dyn", name)).read().splitlines()
    assert got == want, name
