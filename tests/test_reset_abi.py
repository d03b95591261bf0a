"""The per-instance reset's surface without a GPU: exports, header, loud failures, bindings, the argument checks of Batch.reset, the
plain-C driver (compiled here, run under the gpu mark) and the compiler's resource report of the new kernel
(roki-fd_amd/kernel_resources_reset.txt)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rkfdBatchBankReserve", "rkfdBatchBankSize", "rkfdBatchBankStore", "rkfdBatchReset", "rkfdBatchResetDev",
       "rkfdNodeBankReserve", "rkfdNodeBankStore", "rkfdNodeReset")


def test_exports_and_header(R):
    L = C.CDLL(R.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "rkfd_hip.h")).read()
    for n in NEW:
        assert hasattr(L, n), n
        assert re.search(r"\bint %s\s*\(" % n, hdr), n
    assert re.search(r"enum \{ RKFD_RESET_KEEP = -1, RKFD_RESET_SNAPSHOT = -2 \}", hdr)
    assert (R.RESET_KEEP, R.RESET_SNAPSHOT) == (-1, -2)
    assert (R.binding.RESET_KEEP, R.binding.RESET_SNAPSHOT) == (-1, -2)


def test_null_and_no_gpu_fail_with_a_message(R):
    L = R.lib()
    slots = (C.c_int * 4)(-1, -1, -1, -1)
    for call, what in ((lambda: L.rkfdBatchBankReserve(None, 2), b"null batch"), (lambda: L.rkfdBatchBankStore(None, 0, 0, 1), b"null batch"),
                       (lambda: L.rkfdBatchReset(None, slots, None), b"null batch"), (lambda: L.rkfdBatchResetDev(None, slots, None), b"null batch"),
                       (lambda: L.rkfdNodeBankReserve(None, 2), b"null node"), (lambda: L.rkfdNodeBankStore(None, 0, 0, 1), b"null node"),
                       (lambda: L.rkfdNodeReset(None, slots), b"null node")):
        assert call() == -1
        assert what in L.rkfdHipLastError(), L.rkfdHipLastError()
    assert L.rkfdBatchBankSize(None) == -1
    if L.rkfdHipDeviceCount() == 0:
        sc = R.scenarios.config2(batch=2)
        with pytest.raises(R.RkfdError, match="HIP"):       # no batch, hence no bank and no reset, without a GPU: there is no CPU fallback
            R.Batch(sc["world"], 2)
        with pytest.raises(R.RkfdError, match="HIP"):
            R.Node(sc["world"], 2)


def test_bindings_exist(R):
    for n in ("bank_reserve", "bank_size", "bank_store", "reset"):
        assert callable(getattr(R.Batch, n))
    for n in ("bank_reserve", "bank_store", "reset"):
        assert callable(getattr(R.Node, n))


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the argument was checked" % name)


def _batch_without_gpu(R, B=4, device=0):
    """a Batch that has no handle and whose library must not be reached: the checks of reset() come before any call"""
    b = R.Batch.__new__(R.Batch)
    b.B, b.device, b._b, b._L, b._ctrl_keep, b._owned = B, device, None, _NoLibrary(), [], False
    return b


def test_reset_refuses_a_wrong_argument_before_the_library_call(R):
    import torch
    b = _batch_without_gpu(R)
    n = R.Node.__new__(R.Node)
    n.total, n._n, n._L = 4, None, _NoLibrary()
    for obj in (b, n):
        with pytest.raises(TypeError, match="int32"):
            obj.reset(np.zeros(4, dtype=np.int64))
        with pytest.raises(TypeError, match="int32"):
            obj.reset(np.zeros(4, dtype=np.float64))
        with pytest.raises(ValueError, match=r"\(4,\)"):
            obj.reset(np.zeros(5, dtype=np.int32))
        with pytest.raises(ValueError, match=r"\(4,\)"):
            obj.reset(np.zeros((4, 1), dtype=bool))
        with pytest.raises(TypeError, match="numpy"):
            obj.reset([0, 1, 2, 3])
    with pytest.raises(ValueError, match="cuda:0"):
        b.reset(torch.zeros(4, dtype=torch.int32))                 # a tensor on the host
    with pytest.raises(TypeError, match="torch.int32"):
        b.reset(torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\(4,\)"):
        b.reset(torch.zeros(3, dtype=torch.int32))
    with pytest.raises(TypeError, match="numpy"):
        n.reset(torch.zeros(4, dtype=torch.int32))                 # the node level takes host arrays
    # what the checks hand on: a mask becomes SNAPSHOT / KEEP
    kind, s = R.reset_slots(np.array([True, False, False, True]), 4)
    assert kind == "host" and s.dtype == np.int32 and s.tolist() == [R.RESET_SNAPSHOT, R.RESET_KEEP, R.RESET_KEEP, R.RESET_SNAPSHOT]
    b._b = None      # (nothing to close)


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


def test_reset_kernel_report(R):
    k = _report("kernel_resources_reset.txt")
    assert set(k) == {"rkfd_reset_kernel"}
    r = k["rkfd_reset_kernel"]
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, r
    # and the step kernels' report does not know the new kernel
    assert "rkfd_reset_kernel" not in _report("kernel_resources.txt")


def _build_driver(tmp_path):
    exe = str(tmp_path / "reset_driver")
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "reset_driver.c"),
                    "-L" + os.path.join(ROOT, "roki-fd_amd"), "-lrkfd_amd", "-Wl,-rpath," + os.path.join(ROOT, "roki-fd_amd"), "-o", exe], check=True)
    return exe


def test_c_driver_compiles(R, tmp_path):
    """tests/c/reset_driver.c is plain C over the public headers: gcc builds and links it without a GPU"""
    assert os.path.exists(_build_driver(tmp_path))


@pytest.mark.gpu
def test_c_driver_runs(R, tmp_path):
    r = subprocess.run([_build_driver(tmp_path), os.path.join(ROOT, "models"), "6", "10"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["bank of a null batch -1", "bank before 0", "bank 2", "twin identical", "others identical", "reset instance moved",
                                     "status 5 then 0", "status 5", "after bad values untouched", "bank freed 0"], r.stdout
