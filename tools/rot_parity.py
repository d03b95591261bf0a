#!/usr/bin/env python3
"""Worst deviations of the large-rotation cases of tests/rot_cases.py: the rotation primitives of device/rkfd_dev_base.h (emulator
build) against long double; the four read-outs at rot_cases.big_states against the references of their case modules; the direct
probes of d_sincos, d_from_aa and d_to_aa; the rollouts at large angles and through the half turn against the oracle (angle-axis
blocks compared as rotation matrices); the closest approach to pi of every tumbling instance; the drift of the angular momentum in
free flight - under the lane emulator and, when there is a device, on the GPU.  What a run does not measure is marked NOT measured.
The tests assert the bounds named per section (tests/test_rot_primitives.py, test_emu_rotations.py, test_gpu_rotations.py).
usage: python tools/rot_parity.py [output file, default profiles/r13_rot_parity.txt]"""
import os, sys, tempfile, pathlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")):
    sys.path.insert(0, p)
import numpy as np
import rkfd_pkg
import instance_params as ip
import links_cases as lc
import rot_cases as rc
import solver_paths as sp
from emu import EmuBatch
from oracle.pyoracle import Oracle
R = rkfd_pkg.load()
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r13_rot_parity.txt")
gpu = R.lib().rkfdHipDeviceCount() > 0
NOT = "NOT measured"
tmp = pathlib.Path(tempfile.mkdtemp())
EPS = 2.0 ** -52


class EmuR:
    """the package with Batch backed by the lane emulator: what rot_cases' GPU helpers take"""

    def __getattr__(self, k):
        return getattr(R, k)

    def Batch(self, world, batch, device=0, max_rigid=8):
        b = EmuBatch(world, batch, max_rigid=max_rigid)
        b.close = lambda: None
        b.update_links = lambda flags=lc.ALL: setattr(b, "_links", lc.emu_links(world, b.dis, b.vel, flags))
        b.get_links = lambda: b._links
        return b


fmt = lambda d: "  ".join("%s %.2e" % kv for kv in d.items())
vec = lambda a: " ".join("%.2e" % x for x in np.atleast_1d(a))
lines = ["large rotations (tools/rot_parity.py); gpu: %s" % ("measured on this run" if gpu else NOT + " (no device)"), ""]

# ---- primitives (emulator build against np.longdouble) ---------------------------------------------------------------------------------
lines += ["primitives, emulator build against np.longdouble (eps %.2e); the GPU build of the primitives is reached through the probes below" % np.finfo(np.longdouble).eps,
          "d_sincos: bound 2^-52 = %.3e on sin and cos, 4 x 2^-52 on |s^2 + c^2 - 1|" % EPS]
for name, x in rc.sincos_inputs().items():
    es, ec, eu = rc.sincos_errors(x)
    lines.append("  %-24s n %6d  sin %.3e  cos %.3e  |s^2+c^2-1| %.3e" % (name, x.size, es, ec, eu))
lines.append("d_atan2_ypos: bound 4 x 2^-52 = %.3e" % (4 * EPS))
for name, (y, x) in rc.atan2_inputs().items():
    lines.append("  %-24s n %6d  %.3e" % (name, x.size, rc.atan2_error(y, x)))
aa = rc.aa_inputs()
th = np.linalg.norm(aa, axis=1)
e, orth, gram, _ = rc.from_aa_errors(aa)
lines += ["d_from_aa: bound 8 x 2^-52 = %.3e" % (8 * EPS),
          "  n %d  |R - Rodrigues| %.3e  lengths and angles of rows and columns %.3e  (|R' R - 1| %.3e)" % (th.size, e, orth, gram),
          "d_to_aa( d_from_aa( aa ) ): bound max( 1e-12, 1e-14 / ( pi - theta ) )"]
err, bound = rc.roundtrip_errors(aa)
gap = np.abs(np.pi - th)
for lo, hi in ((0.0, 1.5), (1.5, 3.0), (3.0, np.pi - 1e-3), (np.pi - 1e-3, np.pi), (np.pi, np.pi + 1e-3), (np.pi + 1e-3, 2 * np.pi + 1e-9), (6.9, 7.1)):
    on = (th >= lo) & (th < hi)
    if on.any():
        lines.append("  theta in [%.4f, %.4f)  n %5d  |error| %.3e  |error| x |pi - theta| %.3e  closest to pi %.2e  worst error / bound %.3f"
                     % (lo, hi, on.sum(), err[on].max(), (err[on] * gap[on]).max(), gap[on].min(), (err[on] / bound[on]).max()))

# ---- read-outs --------------------------------------------------------------------------------------------------------------------------
lines += ["", "read-outs at rot_cases.big_states, B = 8: |delta|_inf / max( 1, |reference|_inf ), worst over the references of each case module; bound 1e-12",
          "(the trees carry synthetic contact candidates, which only the emulator's harness takes: no GPU figure for cf there)"]
cs = rc.readout_cases(R, tmp, 8)
for name, c in cs.items():
    emu = rc.emu_readouts(c)
    lines.append("  %-12s emulator / references  %s" % (name, fmt(rc.check_readouts(R, Oracle, c, emu, name))))
    if gpu:
        got = rc.gpu_readouts(R, c)
        lines.append("  %-12s gpu / references       %s" % (name, fmt(rc.check_readouts(R, Oracle, c, got, name))))
        lines.append("  %-12s gpu / emulator         %s" % (name, fmt(rc.check_against_emulator(got, emu, name))))
    else:
        lines.append("  %-12s gpu                    %s" % (name, NOT))
c = cs["humanoid30"]
P = ip.randomised(c["world"], 8, seed=0x2071)
emu = rc.emu_readouts(c, par=P)
lines.append("  %-12s emulator / references  %s" % ("humanoid30+table", fmt(rc.check_readouts(R, Oracle, c, emu, "table", par=P))))
if gpu:
    got = rc.gpu_readouts(R, c, par=P)
    lines.append("  %-12s gpu / references       %s" % ("humanoid30+table", fmt(rc.check_readouts(R, Oracle, c, got, "table", par=P))))
    lines.append("  %-12s gpu / emulator         %s" % ("humanoid30+table", fmt(rc.check_against_emulator(got, emu, "table"))))
else:
    lines.append("  %-12s gpu                    %s" % ("humanoid30+table", NOT))

# ---- direct probes ----------------------------------------------------------------------------------------------------------------------
lines += ["", "direct probes: one link's frame against a long double forward kinematics of that link, bound 2e-15; one step of a free box at rest against the oracle's step",
          "and against its start, as rotation matrices, bound max( 1e-12, 1e-14 / ( pi - theta ) ), theta = " + " ".join("%.6f" % x for x in rc.TO_AA_THETAS)]
for what, Rx in (("emulator", EmuR()), ("gpu", R if gpu else None)):
    if Rx is None:
        lines.append("  %-8s %s" % (what, NOT))
        continue
    w, dis = rc.sincos_probe_states(R)
    lines.append("  %-8s d_sincos  (first joint of chain30 over %d values of q0)   %.3e" % (what, dis.shape[0], rc.probe_error(Rx, w, dis)))
    w, dis = rc.from_aa_probe_states(R)
    lines.append("  %-8s d_from_aa (base link of a free box over %d values of theta) %.3e" % (what, dis.shape[0], rc.probe_error(Rx, w, dis)))
    for spec in ((False, True) if what == "gpu" else (False,)):
        e_or, e_st, bd = rc.to_aa_probe(Rx, Oracle, spec)
        lines.append("  %-8s d_to_aa   (%s kernel) against the oracle: %s   against the start: %s   bound: %s"
                     % (what, "world-specific" if spec else "generic", vec(e_or), vec(e_st), vec(bd)))

# ---- rollouts ---------------------------------------------------------------------------------------------------------------------------
lines += ["", "free-motion rollouts against the oracle: rot_cases.state_dev (angle-axis blocks as rotation matrices, the rest |delta|_inf / max( 1, |oracle|_inf ));",
          "bound 1e-9 under the emulator, 1e-8 on the GPU; the GPU's kernel variants are bit for bit the generic kernel's (asserted by the tests)"]
final = lambda tr: tuple(tr[k][:, -1] for k in ("dis", "vel", "acc"))
for key, make, nemu, ngpu, chunks in (("chain30", rc.chain30_rollout, 2, 3, 1), ("humanoid", rc.humanoid_rollout, 2, 5, 1), ("tumbling_box", rc.tumbling_box, 2, 5, 4)):
    sc = make(R, nemu)
    tr = rc.oracle_trajectory(Oracle, sc)
    m = sc["world"].model.contents
    row = []
    for ipw in (1, 2):
        b = EmuBatch(sc["world"], nemu, max_rigid=sc["max_rigid"], ipw=ipw)
        b.set_state(sc["dis"], sc["vel"]); b.update_init(); b.update(sc["steps"])
        row.append("emulator ipw=%d %.2e" % (ipw, rc.state_dev(R, m, b.get_state(), final(tr))))
    lines.append("  %-28s %d steps, %d instances:  %s" % (sc["name"], sc["steps"], nemu, "  ".join(row)))
    if gpu:
        sc = make(R, ngpu)
        tr = rc.oracle_trajectory(Oracle, sc)
        row = ["%s %.2e" % (v, rc.state_dev(R, m, rc.run_variant(R, sc, v, chunks), final(tr))) for v in ("generic", "specialized", "two_per_wave", "table")]
        lines.append("  %-28s %d steps, %d instances:  gpu  %s" % (sc["name"], sc["steps"], ngpu, "  ".join(row)))
    else:
        lines.append("  %-28s gpu %s" % (sc["name"], NOT))
sc = rc.tumbling_box(R, 5)
tr = rc.oracle_trajectory(Oracle, sc, frames=True)
crossings, closest = rc.tumble_gates(tr["dis"])
lines += ["tumbling box, the oracle's trajectory of the five instances (the gates: at least one crossing, no closer than 1e-4):",
          "  half-turn crossings %s   closest approach pi - |aa| %s" % (" ".join(map(str, crossings)), vec(closest))]
dor = rc.drift(rc.angular_momentum(sc["world"].model.contents, tr["R"], tr["v"]))
lines += ["angular momentum R ( I w ) of the tumbling box over its 400 steps, largest |L(t) - L(0)|_inf / |L(0)|_inf per instance; the device may drift 2 x the oracle + 1e-12",
          "  oracle   %s" % vec(dor), "  gpu      %s" % (vec(rc.device_momentum_drift(R, sc)) if gpu else NOT), "  emulator %s" % NOT]

# ---- the box on the floor ---------------------------------------------------------------------------------------------------------------
lines += ["", "box dropped nearly upside down (|aa| = 3.06, 3.11, 2.42) onto the rigid floor, MLCP: solver_paths.compare (worst relative error of dis, vel, acc, forces;",
          "bounds 1e-9 on dis / vel, 1e-8 on acc / forces) after update_init and after 6 steps"]
sc = rc.upside_down_box(R)
for what, mk in (("emulator ipw=1", lambda: EmuBatch(sc["world"], 3, max_rigid=sc["max_rigid"])), ("emulator ipw=2", lambda: EmuBatch(sc["world"], 3, max_rigid=sc["max_rigid"], ipw=2)),
                 ("gpu generic", (lambda: R.Batch(sc["world"], 3, device=0, max_rigid=sc["max_rigid"])) if gpu else None), ("gpu world-specific", "spec" if gpu else None)):
    if mk is None:
        lines.append("  %-20s %s" % (what, NOT))
        continue
    if mk == "spec":
        b = R.Batch(sc["world"], 3, device=0, max_rigid=sc["max_rigid"]); b.specialize()
    else:
        b = mk()
    ors = sp.oracles(sc["world"], sc["dis"], sc["vel"])
    b.set_state(sc["dis"], sc["vel"]); b.update_init()
    w0 = sp.compare(b, ors, what)
    b.update(6)
    for o in ors:
        o.update_n(6)
    n6 = sum(int((o.get_contact()[0] != 0).sum()) for o in ors)
    lines.append("  %-20s init %.2e   6 steps %.2e   (oracle contacts after 6 steps: %d)" % (what, w0, sp.compare(b, ors, what), n6))

print("\n".join(lines))
with open(OUT, "w") as fh:
    fh.write("\n".join(lines) + "\n")
