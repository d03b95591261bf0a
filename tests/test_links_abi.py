"""The task-space read-out's surface without a GPU: exports, loud failures, bindings, and the compiler's resource report of the
new kernel (roki-fd_amd/kernel_resources_links.txt) beside the untouched report of the step kernels."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rkfdBatchLinkNum", "rkfdBatchChainNum", "rkfdBatchUpdateLinks", "rkfdBatchGetLinks", "rkfdBatchDevLinkAtt", "rkfdBatchDevLinkPos",
       "rkfdBatchDevLinkVel", "rkfdBatchDevCom", "rkfdBatchDevComVel", "rkfdNodeGetLinks", "rkfdChainLinkWldPos", "rkfdChainLinkWldAtt", "rkfdChainWldCOM")


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
    hdr = open(os.path.join(ROOT, "include", "rkfd_hip.h")).read() + open(os.path.join(ROOT, "include", "roki_fd_amd.h")).read()
    for n in NEW:
        assert hasattr(L, n), n
        assert re.search(r"\b%s\s*\(" % n, hdr), n
    assert re.search(r"RKFD_LINKS_POSE = 1, RKFD_LINKS_VEL = 2, RKFD_LINKS_COM = 4", hdr)
    assert (R.LINKS_POSE, R.LINKS_VEL, R.LINKS_COM) == (1, 2, 4)


def test_null_and_no_gpu_fail_with_a_message(R):
    L = R.lib()
    buf = (C.c_double * 16)()
    assert L.rkfdBatchUpdateLinks(None, 7, None) == -1 and b"null batch" in L.rkfdHipLastError()
    assert L.rkfdBatchGetLinks(None, buf, None, None, None, None) == -1 and b"null batch" in L.rkfdHipLastError()
    assert L.rkfdNodeGetLinks(None, 7, None, None, None, None, None) == -1 and b"null node" in L.rkfdHipLastError()
    assert L.rkfdBatchLinkNum(None) == -1 and L.rkfdBatchChainNum(None) == -1
    for f in ("rkfdBatchDevLinkAtt", "rkfdBatchDevLinkPos", "rkfdBatchDevLinkVel", "rkfdBatchDevCom", "rkfdBatchDevComVel"):
        assert getattr(L, f)(None) is None
    # the reference-named accessors: no crash on NULL, zeros / the identity
    L.rkfdChainLinkWldPos.argtypes = [C.c_void_p, C.c_int, C.c_void_p]; L.rkfdChainLinkWldAtt.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.rkfdChainWldCOM.argtypes = [C.c_void_p, C.c_void_p]
    for k in range(16):
        buf[k] = 5.0
    L.rkfdChainLinkWldPos(None, 0, buf); assert list(buf[:3]) == [0, 0, 0]
    L.rkfdChainLinkWldAtt(None, 0, buf); assert list(buf[:9]) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    L.rkfdChainWldCOM(None, buf); assert list(buf[:3]) == [0, 0, 0]
    if L.rkfdHipDeviceCount() == 0:
        sc = R.scenarios.config2(batch=2)
        try:
            R.Batch(sc["world"], 2)
        except R.RkfdError as e:
            assert "HIP" in str(e)      # no batch, hence no read-out, without a GPU: there is no CPU fallback
        else:
            raise AssertionError("rkfdBatchCreate must fail without a GPU")


def test_bindings_exist(R):
    for n in ("update_links", "get_links", "dev_tensors", "dev_ptrs", "links_tensors"):
        assert callable(getattr(R.Batch, n))
    assert callable(R.Node.get_links)


def test_links_kernel_report(R):
    k = _report("kernel_resources_links.txt")
    assert set(k) == {"rkfd_links_kernel"}
    assert k["rkfd_links_kernel"]["VGPRs Spill"] == 0 and k["rkfd_links_kernel"]["ScratchSize [bytes/lane]"] == 0, k


# the step kernels' report as the compiler of this toolchain (ROCm 7.2) wrote it before the read-out existed: VGPRs, scratch bytes per
# lane, waves per SIMD, VGPR spills.  The read-out lives in a translation unit of its own, so none of these may move with it.
STEP_REPORT = {
    "rkfd_step_kernel": (168, 0, 3, 0), "rkfd_step_kernel_pk": (163, 0, 3, 0), "rkfd_step_kernel_vqp": (235, 0, 2, 0),
    "rkfd_step_kernel_prof": (168, 12, 3, 2), "rkfd_step_kernel_prof_pk": (162, 0, 3, 0), "rkfd_step_kernel_prof_vqp": (235, 0, 2, 0),
    "rkfd_step_kernel_vol": (256, 364, 2, 213), "rkfd_step_kernel_prof_vol": (256, 404, 2, 248), "rkfd_restore_kernel": (17, 0, 8, 0)}


def test_step_kernel_report_is_what_it_was(R):
    """a regression guard (it passes without the feature): the same nine kernels with the same registers, scratch, occupancy
    and spills as before the read-out was added"""
    k = _report("kernel_resources.txt")
    assert set(k) == set(STEP_REPORT)
    for name, want in STEP_REPORT.items():
        got = (k[name]["VGPRs"], k[name]["ScratchSize [bytes/lane]"], k[name]["Occupancy [waves/SIMD]"], k[name]["VGPRs Spill"])
        assert got == want, (name, got, want)
