"""The task-space Jacobians' surface without a GPU: exports, declarations, loud failures, bindings, and the compiler's resource
report of the new kernel (roki-fd_amd/kernel_resources_jac.txt) beside the untouched reports of the step kernels, the read-out and
the reset - line for line what the build gave before the Jacobians existed (tests/golden/kernel_reports_before_jac/)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rkfdBatchSetJacobianSites", "rkfdBatchJacobianSiteNum", "rkfdBatchUpdateJacobians", "rkfdBatchGetJacobians", "rkfdBatchDevJacobian",
       "rkfdBatchDevComJacobian", "rkfdNodeSetJacobianSites", "rkfdNodeGetJacobians")
OTHER_REPORTS = ("kernel_resources.txt", "kernel_resources_par.txt", "kernel_resources_links.txt", "kernel_resources_reset.txt")
UNCHANGED = ("kernel_resources.txt", "kernel_resources_links.txt", "kernel_resources_reset.txt")


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
    assert re.search(r"RKFD_JAC_SITES = 1, RKFD_JAC_COM = 2", hdr)
    assert (R.JAC_SITES, R.JAC_COM, R.JAC_ALL) == (1, 2, 3)


def test_null_fails_with_a_message(R):
    L = R.lib()
    buf = (C.c_double * 16)()
    link = (C.c_int * 1)(0)
    assert L.rkfdBatchSetJacobianSites(None, 1, link, None) == -1 and b"null batch" in L.rkfdHipLastError()
    assert L.rkfdBatchUpdateJacobians(None, 3, None) == -1 and b"null batch" in L.rkfdHipLastError()
    assert L.rkfdBatchGetJacobians(None, buf, None) == -1 and b"null batch" in L.rkfdHipLastError()
    assert L.rkfdNodeSetJacobianSites(None, 1, link, None) == -1 and b"null node" in L.rkfdHipLastError()
    assert L.rkfdNodeGetJacobians(None, 3, None, None) == -1 and b"null node" in L.rkfdHipLastError()
    assert L.rkfdBatchJacobianSiteNum(None) == -1
    assert L.rkfdBatchDevJacobian(None) is None and L.rkfdBatchDevComJacobian(None) is None


def test_bindings_exist(R):
    for n in ("set_jacobian_sites", "update_jacobians", "get_jacobians", "jacobian_tensors", "jacobian_ptrs"):
        assert callable(getattr(R.Batch, n))
    assert callable(R.Node.set_jacobian_sites) and callable(R.Node.get_jacobians)
    with pytest.raises(ValueError, match=r"expected \(2, 3\)"):
        R.binding._jac_sites([0, 1], [[0.0, 0.0, 0.0]])


def test_jac_kernel_report(R):
    k = _report("kernel_resources_jac.txt")
    assert set(k) == {"rkfd_jac_kernel"}
    assert k["rkfd_jac_kernel"]["VGPRs Spill"] == 0 and k["rkfd_jac_kernel"]["SGPRs Spill"] == 0 and k["rkfd_jac_kernel"]["ScratchSize [bytes/lane]"] == 0, k


def test_jac_kernel_is_in_no_other_report(R):
    for name in OTHER_REPORTS:
        assert "rkfd_jac_kernel" not in open(os.path.join(ROOT, "roki-fd_amd", name)).read(), name


@pytest.mark.parametrize("name", UNCHANGED)
def test_other_reports_are_what_they_were(R, name):
    """a regression guard (it passes without the feature): the reports of the step kernels, the read-out and the reset, line for
    line as the build wrote them before the Jacobians' translation unit was added"""
    got = open(os.path.join(ROOT, "roki-fd_amd", name)).read().splitlines()
    want = open(os.path.join(ROOT, "tests", "golden", "kernel_reports_before_jac", name)).read().splitlines()
    assert got == want, name
