"""The contact read-out's surface without a GPU: exports, declarations, loud failures, bindings, and the compiler's resource report
of the new kernel (roki-fd_amd/kernel_resources_cf.txt) beside the untouched reports of the step kernels, the read-out, the reset, the
Jacobians and the dynamics - line for line what the build gave before the contact read-out existed
(tests/golden/kernel_reports_before_cf/)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rkfdBatchUpdateContactForces", "rkfdBatchUpdateContactForcesDev", "rkfdBatchGetContactForces", "rkfdBatchDevContactPoint",
       "rkfdBatchDevContactWrench", "rkfdBatchDevContactCount", "rkfdBatchDevContactGenForce", "rkfdNodeGetContactForces")
OTHER_REPORTS = ("kernel_resources.txt", "kernel_resources_par.txt", "kernel_resources_links.txt", "kernel_resources_reset.txt",
                 "kernel_resources_jac.txt", "kernel_resources_dyn.txt")
UNCHANGED = ("kernel_resources.txt", "kernel_resources_links.txt", "kernel_resources_reset.txt", "kernel_resources_jac.txt", "kernel_resources_dyn.txt")


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
    assert re.search(r"enum \{ RKFD_CF_POINT = 1, RKFD_CF_WRENCH = 2, RKFD_CF_GENF = 4 \}", hdr)
    assert (R.CF_POINT, R.CF_WRENCH, R.CF_GENF, R.CF_ALL) == (1, 2, 4, 7)
    # the accessors' ordering comment keeps its list and names the new launches in a sentence after it
    at = re.search(r"Restore / Reset\[Dev\] / UpdateLinks / UpdateJacobians / UpdateDynamics\)", hdr)
    assert at
    rest = hdr[at.end():hdr.index("int rkfdBatchSetState")]
    assert "rkfdBatchUpdateContactForces" in rest and "rkfdBatchUpdateContactForcesDev" in rest


def test_null_fails_with_a_message(R):
    L = R.lib()
    buf = (C.c_double * 16)()
    assert L.rkfdBatchUpdateContactForces(None, 7, None) == -1 and b"rkfdBatchUpdateContactForces: null batch" in L.rkfdHipLastError()
    assert L.rkfdBatchUpdateContactForcesDev(None, 7, buf, buf, None) == -1 and b"rkfdBatchUpdateContactForcesDev: null batch" in L.rkfdHipLastError()
    assert L.rkfdBatchGetContactForces(None, buf, None, None, None) == -1 and b"rkfdBatchGetContactForces: null batch" in L.rkfdHipLastError()
    assert L.rkfdNodeGetContactForces(None, 7, None, None, None, None) == -1 and b"rkfdNodeGetContactForces: null node" in L.rkfdHipLastError()
    for n in NEW[3:7]:
        assert getattr(L, n)(None) is None, n


def test_bindings_exist(R):
    for n in ("update_contact_forces", "get_contact_forces", "contact_force_ptrs", "contact_force_tensors"):
        assert callable(getattr(R.Batch, n))
    assert callable(R.Node.get_contact_forces)
    a = R.binding._cf_arrays(3, 11, 4, 5, R.CF_WRENCH | R.CF_GENF)
    assert {k: v.shape for k, v in a.items()} == {"wrench": (3, 4, 6), "count": (3, 4), "genf": (3, 5)}
    assert a["count"].dtype == np.int32 and a["wrench"].dtype == np.float64
    assert set(R.binding._cf_arrays(1, 2, 3, 4, R.CF_ALL)) == {"point", "wrench", "count", "genf"}


def test_device_arguments_are_checked_before_any_library_call(R):
    """what update_contact_forces(active=, f=) takes: the shapes, the types and contiguity of a __cuda_array_interface__"""
    class Arr:
        def __init__(self, shape, typestr, strides=None):
            self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(4096, False), version=2, strides=strides)
    ptr = R.binding._cf_dev_ptr
    assert ptr("f", Arr((2, 5, 3), "<f8"), "<f8", ((2, 5, 3), (2, 15)), 0) == 4096
    assert ptr("f", Arr((2, 15), "<f8"), "<f8", ((2, 5, 3), (2, 15)), 0) == 4096
    with pytest.raises(ValueError, match="shape"):
        ptr("active", Arr((2, 4), "<i4"), "<i4", ((2, 5),), 0)
    with pytest.raises(TypeError, match="<i8"):
        ptr("active", Arr((2, 5), "<i8"), "<i4", ((2, 5),), 0)
    with pytest.raises(ValueError, match="contiguous"):
        ptr("active", Arr((2, 5), "<i4", strides=(40, 4)), "<i4", ((2, 5),), 0)
    with pytest.raises(TypeError, match="ndarray"):
        ptr("active", np.zeros((2, 5), dtype=np.int32), "<i4", ((2, 5),), 0)


def test_cf_kernel_report(R):
    k = _report("kernel_resources_cf.txt")
    assert set(k) == {"rkfd_cf_kernel"}
    assert k["rkfd_cf_kernel"]["VGPRs Spill"] == 0 and k["rkfd_cf_kernel"]["SGPRs Spill"] == 0 and k["rkfd_cf_kernel"]["ScratchSize [bytes/lane]"] == 0, k


def test_cf_kernel_is_in_no_other_report(R):
    for name in OTHER_REPORTS:
        assert "rkfd_cf_kernel" not in open(os.path.join(ROOT, "roki-fd_amd", name)).read(), name


@pytest.mark.parametrize("name", UNCHANGED)
def test_other_reports_are_what_they_were(R, name):
    """a regression guard (it passes without the feature): the reports of the step kernels, the read-out, the reset, the Jacobians and
    the dynamics, line for line as the build wrote them before the contact read-out's translation unit was added"""
    got = open(os.path.join(ROOT, "roki-fd_amd", name)).read().splitlines()
    want = open(os.path.join(ROOT, "tests", "golden", "kernel_reports_before_cf", name)).read().splitlines()
    assert got == want, name
