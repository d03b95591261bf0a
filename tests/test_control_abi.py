"""The control-schedule entry points (rkfdBatchUpdateControlled, ...Dev, rkfdNodeUpdateControlled): exported, declared, and on a
machine without a GPU they refuse bad arguments with a message instead of crashing; the bindings expose them."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rkfdBatchUpdateControlled", "rkfdBatchUpdateControlledDev", "rkfdNodeUpdateControlled")


def test_exported_and_declared(R):
    L = C.CDLL(R.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "rkfd_hip.h")).read()
    for n in NAMES:
        assert hasattr(L, n), n
        assert ("int %s(" % n) in hdr, n


def test_bad_arguments_fail_with_a_message(R):
    L = R.lib()
    u = np.zeros(8)
    for call, what in ((lambda: L.rkfdBatchUpdateControlled(None, 1, u.ctypes.data, None), "null batch"),
                       (lambda: L.rkfdBatchUpdateControlledDev(None, 1, u.ctypes.data, None), "null batch"),
                       (lambda: L.rkfdNodeUpdateControlled(None, 1, u.ctypes.data), "null node")):
        assert call() == -1
        assert what in L.rkfdHipLastError().decode()


def test_no_gpu_no_batch(R):
    """without a GPU there is no batch to give a schedule to: creation fails loudly (no CPU fallback)"""
    if R.lib().rkfdHipDeviceCount() > 0:
        return      # on a GPU box the path is live: tests/test_gpu_control.py
    sc = R.scenarios.arm_press(batch=2)
    with pytest.raises(R.RkfdError):
        R.Batch(sc["world"], 2, max_rigid=sc["max_rigid"])


def test_bindings_expose_update_controlled(R):
    assert callable(getattr(R.Batch, "update_controlled", None))
    assert callable(getattr(R.Node, "update_controlled", None))
