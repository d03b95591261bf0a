"""Host calls that FOLLOW a launch are ordered after it - also when the launch went to a stream made with hipStreamNonBlocking
(PyTorch's streams, the node level's per-device streams), which the null stream of the accessors' blocking copies is not ordered
against, and at the default split, where the batch has no internal streams to wait for.

Protocol: every case runs one call sequence twice on fresh batches - once with NO host wait between the calls, once with
status() on the launch stream between every two calls - and the results must be bit-identical.  The waited run is the reference;
it is anchored to the oracle once (test_motor_input_loop_against_the_oracle).  The window: a fused launch of 25 steps of config 4
with 64 instances runs for about 4 ms (0.177 ms per step, profiles/r03_latency_vs_residency.txt), a host copy starts within
tens of microseconds, so a copy that is not ordered falls inside the launch."""
import numpy as np
import pytest

import links_cases as lc

pytestmark = pytest.mark.gpu

B, H, NLOOP = 64, 25, 10
NODE_B = 37
RTOL_STANDING = 1e-8          # config 4 in tests/test_gpu_parity.py


def scenario(R):
    s = R.scenarios.config4(batch=B)
    m = s["world"].model.contents
    rng = np.random.default_rng(0x57E)
    s["X"] = s["dis"] + rng.uniform(-1e-3, 1e-3, s["dis"].shape)
    s["V"] = s["vel"] + rng.uniform(-1e-2, 1e-2, s["vel"].shape)
    s["u"] = rng.normal(0.0, 0.5, (B, NLOOP, m.nlink))
    return s


@pytest.fixture(scope="module")
def sc(R):
    return scenario(R)


class _NonBlockingStream:
    """a stream made with hipStreamNonBlocking by the HIP runtime the library itself is linked to (its symbols are reached through
    the library's handle; a process may hold a second runtime, PyTorch's): the kind of stream PyTorch hands out and the node level
    makes.  PyTorch's own streams: test_torch_streams, in a process where torch comes up first."""

    def __init__(self, L):
        import ctypes
        self._L = L
        h = ctypes.c_void_p()
        assert L.hipStreamCreateWithFlags(ctypes.byref(h), 1) == 0 and h.value      # (1: hipStreamNonBlocking)
        self.cuda_stream = h.value

    def close(self):
        import ctypes
        assert self._L.hipStreamDestroy(ctypes.c_void_p(self.cuda_stream)) == 0


@pytest.fixture(params=["null", "nonblocking"])
def stream(R, request):
    """(the object that keeps the stream alive, its handle)"""
    if request.param == "null":
        yield None, None
        return
    s = _NonBlockingStream(R.lib())
    yield s, s.cuda_stream
    s.close()      # (every batch that launched on it has waited for it and is closed)


def _batch(R, sc, split, kernel, s, n=B):
    b = R.Batch(sc["world"], n, device=0, max_rigid=sc["max_rigid"])
    if kernel == "spec":
        b.specialize()
    if split > 1:
        b.set_split(split)
    b.set_state(sc["dis"][:n], sc["vel"][:n])
    b.update_init(s)
    assert b.status(s) == 0
    return b


def _result(b, s=None):
    assert b.status(s) == 0
    return tuple(b.get_state()) + tuple(b.get_contact()) + tuple(b.get_pivot()) + (b.get_broken(),)


def _same(x, y, what=""):
    assert len(x) == len(y)
    for k, (p, q) in enumerate(zip(x, y)):
        assert np.array_equal(p, q), (what, k)


def _twice(R, sc, split, kernel, s, seq):
    """seq( b, wait ) on a fresh batch without and with host waits; -> (result without, result with)"""
    out = []
    for waited in (False, True):
        b = _batch(R, sc, split, kernel, s)
        out.append(seq(b, (lambda b=b: b.status(s)) if waited else (lambda: 0)))
        b.close()
    return out


AXES = [(1, "generic"), (3, "generic"), (1, "spec"), (3, "spec")]
axes = pytest.mark.parametrize("split,kernel", AXES)


@axes
def test_set_state_after_a_launch_in_flight(R, sc, stream, split, kernel):
    keep, s = stream

    def seq(b, wait):
        b.update(H, s); wait()
        b.set_state(sc["X"], sc["V"]); wait()
        d, v, _ = b.get_state(); wait()
        b.update(1, s)
        return (d, v) + _result(b, s)
    got, want = _twice(R, sc, split, kernel, s, seq)
    assert np.array_equal(got[0], sc["X"]) and np.array_equal(got[1], sc["V"])      # (not what the launch left at its end)
    _same(got, want)


def _motor_loop(sc, s):
    def seq(b, wait):
        for t in range(NLOOP):
            b.set_motor_input(sc["u"][:b.B, t]); wait()
            b.update(1, s); wait()
        return _result(b, s)
    return seq


@axes
def test_motor_input_loop(R, sc, stream, split, kernel):
    """the reference drivers' loop and the MPC pattern: no input lands a step early"""
    keep, s = stream
    got, want = _twice(R, sc, split, kernel, s, _motor_loop(sc, s))
    _same(got, want)
    c = _batch(R, sc, split, kernel, s)
    c.update_controlled(sc["u"], s)
    _same(_result(c, s), want, "update_controlled")
    c.close()


def test_motor_input_loop_against_the_oracle(R, oracle_cls, sc):
    """the anchor of the waited runs: instances 0 and B-1 of the waited loop against the oracle stepping the same loop"""
    b = _batch(R, sc, 1, "generic", None)
    got = _motor_loop(sc, None)(b, b.status)
    b.close()
    for i in (0, B - 1):
        o = oracle_cls(sc["world"].model)
        o.set_state(sc["dis"][i], sc["vel"][i]); o.update_init()
        for t in range(NLOOP):
            o.set_motor_input(sc["u"][i, t])
            assert o.update() == 0
        for k, (x, y) in enumerate(zip(got[:3], o.get_state())):
            err = np.abs(x[i] - y).max() / max(1.0, np.abs(y).max())
            print(f"instance {i} {'dis vel acc'.split()[k]}: {err:.2e}")
            assert err < RTOL_STANDING, (i, k, err)
        assert np.array_equal(got[3][i], o.get_contact()[0])
        o.close()


READERS = ["get_state", "get_contact", "get_pivot", "get_broken"]
WRITERS = [("set_contact", "get_contact", slice(0, 3)), ("set_pivot", "get_pivot", slice(None)), ("set_broken", "get_broken", None)]


def _tup(x):
    return x if isinstance(x, tuple) else (x,)


@axes
@pytest.mark.parametrize("reader", READERS)
def test_reader_after_a_launch_in_flight(R, sc, stream, split, kernel, reader):
    keep, s = stream

    def seq(b, wait):
        b.update(H, s); wait()
        return _tup(getattr(b, reader)())
    got, want = _twice(R, sc, split, kernel, s, seq)
    _same(got, want, reader)


@axes
@pytest.mark.parametrize("writer,reader,part", WRITERS, ids=[w[0] for w in WRITERS])
def test_writer_after_a_launch_in_flight(R, sc, stream, split, kernel, writer, reader, part):
    """the values the waited run read back after the launch, written at once after the same launch: nothing of the launch may
    come after them, and the steps that follow start from them"""
    keep, s = stream
    vals = []

    def seq(b, wait):
        b.update(H, s); wait()
        if not vals:                              # (the waited run goes first and reads them)
            v = getattr(b, reader)()
            vals.append(_tup(v)[part] if part is not None else (v,))
        getattr(b, writer)(*vals[0]); wait()
        b.update(5, s)
        return _result(b, s)
    want = None
    for waited in (True, False):
        b = _batch(R, sc, split, kernel, s)
        r = seq(b, (lambda b=b: b.status(s)) if waited else (lambda: 0))
        b.close()
        if waited:
            want = r
        else:
            _same(r, want, writer)


@axes
def test_links_readout_after_steps(R, sc, stream, split, kernel):
    keep, s = stream

    def seq(b, wait):
        b.update(5, s); wait()
        b.update_links(stream=s); wait()
        out = b.get_links()
        return tuple(out[k] for k in lc.KEYS)
    got, want = _twice(R, sc, split, kernel, s, seq)
    _same(got, want)


_TORCH_CHILD = r"""
import sys
sys.path[:0] = [ROOT, ROOT + "/tests", ROOT + "/tests/emu"]
import torch
torch.cuda.init()      # torch's HIP runtime before the library's first call (as bench.py does)
import rkfd_pkg
import test_gpu_stream_order as t
R = rkfd_pkg.load()
sc = t.scenario(R)
s = torch.cuda.Stream()
assert s.cuda_stream != 0
st = (s, s.cuda_stream)
for split, kernel in t.AXES:
    t.test_set_state_after_a_launch_in_flight(R, sc, st, split, kernel)
    t.test_motor_input_loop(R, sc, st, split, kernel)
    for reader in t.READERS:
        t.test_reader_after_a_launch_in_flight(R, sc, st, split, kernel, reader)
    for w in t.WRITERS:
        t.test_writer_after_a_launch_in_flight(R, sc, st, split, kernel, *w)
    t.test_links_readout_after_steps(R, sc, st, split, kernel)
print("TORCH_OK")
"""


def test_torch_streams():
    """every batch-level case above with a torch.cuda.Stream() passed as .cuda_stream; a fresh child process, so that torch's HIP
    runtime comes up before the library's (as in tests/test_gpu_control.py)"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % root + _TORCH_CHILD], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- the node level: always a non-blocking stream per device, here at the DEFAULT split and with no status() before the calls ----
NODES = pytest.mark.parametrize("shards", [3, 1])


def _node(R, sc, shards):
    n = R.Node(sc["world"], NODE_B, max_rigid=sc["max_rigid"], **(dict(devices=[0, 0, 0]) if shards == 3 else dict(ndev=1)))
    assert n.ndev == shards
    n.set_state(sc["dis"][:NODE_B], sc["vel"][:NODE_B])
    n.update_init()
    return n


@NODES
def test_node_set_state_after_a_launch_in_flight(R, sc, shards):
    X, V = sc["X"][:NODE_B], sc["V"][:NODE_B]
    out = []
    for waited in (False, True):
        n = _node(R, sc, shards)
        wait = n.status if waited else (lambda: 0)
        n.update(H); wait()
        n.set_state(X, V); wait()
        d, v, _ = n.get_state(); wait()
        n.update(1)
        assert n.status() == 0
        out.append((d, v) + tuple(n.get_state()))
        n.close()
    assert np.array_equal(out[0][0], X) and np.array_equal(out[0][1], V)
    _same(out[0], out[1])


@NODES
def test_node_motor_input_loop(R, sc, shards):
    u = sc["u"][:NODE_B]
    b = _batch(R, sc, 1, "generic", None, n=NODE_B)
    want = _motor_loop(sc, None)(b, b.status)[:3]
    b.close()
    n = _node(R, sc, shards)
    for t in range(NLOOP):
        n.set_motor_input(u[:, t])
        n.update(1)
    assert n.status() == 0
    _same(n.get_state(), want, "loop")
    n.close()
    n = _node(R, sc, shards)
    n.update_controlled(np.ascontiguousarray(u))
    assert n.status() == 0
    _same(n.get_state(), want, "update_controlled")
    n.close()


@NODES
def test_node_shard_accessors_after_a_launch_in_flight(R, sc, shards):
    """every accessor of the per-shard batches (Node.batch: rkfdNodeBatch), each at once after a launch of its own, against one
    waited batch of all instances making the same calls"""
    b = _batch(R, sc, 1, "generic", None, n=NODE_B)
    n = _node(R, sc, shards)
    views = [(n.batch(k), lo, hi) for k, (_d, lo, hi) in enumerate(n.shards())]
    for reader in READERS:
        b.update(H); assert b.status() == 0
        want = _tup(getattr(b, reader)())
        n.update(H)
        for v, lo, hi in views:
            _same(_tup(getattr(v, reader)()), tuple(x[lo:hi] for x in want), reader)
    for writer, reader, part in WRITERS:
        b.update(H); assert b.status() == 0
        r = getattr(b, reader)()
        vals = _tup(r)[part] if part is not None else (r,)
        getattr(b, writer)(*vals)
        b.update(5)
        n.update(H)
        for v, lo, hi in views:
            getattr(v, writer)(*[x[lo:hi] for x in vals])
        n.update(5)
        want = _result(b)
        assert n.status() == 0
        _same(n.get_state(), want[:3], writer)
        for v, lo, hi in views:
            _same(_result(v), tuple(x[lo:hi] for x in want), writer)
    for v, _lo, _hi in views:
        v.close()
    n.close(); b.close()
