"""EmuBatch with the per-instance reset: the device code of roki-fd_amd/csrc/reset/rkfd_reset.h (tests/emu/rkfd_emu_reset.cpp) over
the emulator's state arrays, a bank and a snapshot of numpy arrays - the surface of roki_fd_amd.Batch (bank_reserve, bank_size,
bank_store, snapshot, restore, reset, status).  Every array the reset code may write or read is followed by PAD rows of a sentinel:
pad_intact() tells whether anything was written past `batch` or `nslots`.  Development / test harness only."""
import ctypes as C
import os
import subprocess

import numpy as np

from emu import HERE, ROOT, DevState, EmuBatch

LIB_PATH = os.path.join(HERE, "librkfd_emu_reset.so")
FIELDS = ("dis", "vel", "acc", "piv_type", "piv_prev", "brk", "cv_active", "cv_type", "cv_ref", "cv_f")
PAD = 3
SENTINEL_F, SENTINEL_I = -7.25e77, 0x5A5A5A5A
RESET_KEEP, RESET_SNAPSHOT = -1, -2
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            subprocess.run(["make", "-C", ROOT, "emu"], check=True, stdout=subprocess.DEVNULL)
        L = C.CDLL(LIB_PATH)
        L.rkfd_emu_reset.argtypes = [C.POINTER(DevState), C.POINTER(DevState), C.c_int, C.POINTER(DevState), C.c_void_p] + [C.c_int] * 5
        _lib = L
    return _lib


def _padded(like, rows):
    """(rows + PAD, ...) of the sentinel, shaped and typed like the rows of `like`"""
    a = np.empty((rows + PAD,) + like.shape[1:], dtype=like.dtype)
    a[...] = SENTINEL_I if like.dtype == np.int32 else SENTINEL_F
    return a


def _devstate(arrays, n):
    st = DevState()
    for k in FIELDS:
        setattr(st, k, arrays[k].ctypes.data)
    st.batch = n
    return st


class EmuResetBatch(EmuBatch):
    def __init__(self, world, batch, max_rigid=8, ipw=1):
        super().__init__(world, batch, max_rigid=max_rigid, ipw=ipw)
        # the state arrays become the first B rows of padded ones (same address for the emulator's runs)
        self._full = {}
        for k in FIELDS:
            old = getattr(self, k)
            self._full[k] = _padded(old, batch)
            self._full[k][:batch] = old
            setattr(self, k, self._full[k][:batch])
        self._bank, self.nslots = None, 0
        self._snap = None
        self.reset_err = 0

    def bank_reserve(self, nslots):
        self.nslots = int(nslots)
        self._bank = {k: _padded(getattr(self, k), self.nslots) for k in FIELDS} if nslots else None

    def bank_size(self):
        return self.nslots

    def bank_store(self, slot, first=0, count=1):
        assert self._bank is not None and 0 <= slot and slot + count <= self.nslots and 0 <= first and first + count <= self.B
        for k in FIELDS:
            self._bank[k][slot:slot + count] = getattr(self, k)[first:first + count]

    def bank_rows(self):
        """the bank as the result tuple of mixed_batches.result lays a batch out (raw arrays)"""
        return {k: self._bank[k][:self.nslots].copy() for k in FIELDS}

    def snapshot(self):
        self._snap = {k: _padded(getattr(self, k), self.B) for k in FIELDS}
        for k in FIELDS:
            self._snap[k][:self.B] = getattr(self, k)

    def restore(self):
        assert self._snap is not None
        for k in FIELDS:
            getattr(self, k)[...] = self._snap[k][:self.B]

    def reset(self, slots, first=0, end=None):
        """the launch rkfdBatchReset makes over the instances [first, end) (default: all; a split launch makes one per part)"""
        slots = np.asarray(slots)
        if slots.dtype == np.bool_:
            slots = np.where(slots, RESET_SNAPSHOT, RESET_KEEP)
        s = _padded(np.zeros((1,), dtype=np.int32), self.B)
        s[:self.B] = slots
        st = _devstate(self._full, self.B)
        bank = _devstate(self._bank, self.nslots) if self._bank else None
        snap = _devstate(self._snap, self.B) if self._snap else None
        e = lib().rkfd_emu_reset(C.byref(st), C.byref(bank) if bank else None, self.nslots, C.byref(snap) if snap else None, s.ctypes.data,
                                 first, self.B if end is None else end, self.ndof, self.nlink, self.ncand)
        self.reset_err = self.reset_err or e

    def status(self):
        """the last run's status, or - once, like the device's flag - what a reset left"""
        e, self.reset_err = self.reset_err, 0
        return e or self.err

    def pad_intact(self):
        for d in (self._full, self._bank, self._snap):
            if d is None:
                continue
            n = {id(self._full): self.B, id(self._bank): self.nslots, id(self._snap): self.B}[id(d)]
            for k in FIELDS:
                if not (d[k][n:] == (SENTINEL_I if d[k].dtype == np.int32 else SENTINEL_F)).all():
                    return False
        return True

    def clone(self, bank=True, snap=True):
        """a second batch holding the same state (and bank, and snapshot): nothing is stepped"""
        c = EmuResetBatch(self.world, self.B, max_rigid=self.max_rigid, ipw=self.ipw)
        for k in FIELDS + ("motor_in",):
            getattr(c, k)[...] = getattr(self, k)
        if bank and self._bank is not None:
            c.bank_reserve(self.nslots)
            for k in FIELDS:
                c._bank[k][...] = self._bank[k]
        if snap and self._snap is not None:
            c._snap = {k: self._snap[k].copy() for k in FIELDS}
        return c
