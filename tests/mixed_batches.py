"""Helpers of the mixed-batch tests (tests/test_emu_mixed.py, tests/test_gpu_mixed.py): batches whose neighbouring instances are
as UNLIKE each other as a world allows - an airborne body beside a standing one -, so that the two instances that share a wavefront
under RKFD_W = 2 take different branches, carry different contact counts and run loops of different length.

A CHARACTER is one instance's complete input: dis, vel and optionally motor input, broken flags, a parameter row and a control
schedule.  arrange(K) puts every ordered pair of K characters side by side; the yardstick of every instance is the batch of ONE
on the generic kernel (one instance per wavefront, no split), compared with np.array_equal.

The ORACLE GATE (oracle_run / assert_gate) keeps a character list honest: run alone on the oracle the characters must spread
over no contact, the world's nominal full contact and something strictly between, and at least one count must change during
the run.  A list that fails it is the wrong list; the condition stays."""
import numpy as np

import instance_params as ip

SEAT_IN = 1.0e-4        # depth at which the box characters are seated (deeper than scenarios.SEAT_DEPTH on purpose: the compensation
                        # term then throws the box off the floor, and the contact counts chatter between full and none)


class Character:
    def __init__(self, label, dis, vel, motor_in=None, broken=None, params=None, ctrl=None):
        self.label = label
        self.dis = np.array(dis, dtype=np.float64); self.vel = np.array(vel, dtype=np.float64)
        self.motor_in = None if motor_in is None else np.array(motor_in, dtype=np.float64)
        self.broken = None if broken is None else np.array(broken, dtype=np.int32)
        self.params = params            # {name: row} in model space (instance_params), or None
        self.ctrl = None if ctrl is None else np.array(ctrl, dtype=np.float64)      # (H, nlink), or None

    def but(self, label, **kw):
        d = dict(dis=self.dis, vel=self.vel, motor_in=self.motor_in, broken=self.broken, params=self.params, ctrl=self.ctrl)
        d.update(kw)
        return Character(label, **d)


# ---- arrangement ---------------------------------------------------------------------------------------------------------------
def arrange(K):
    """[i, j for every ordered pair i != j] + [0]: positions 2p and 2p+1 share a wavefront when the batch goes out in one part,
    the trailing instance has the stand-in half for a neighbour"""
    idx = []
    for i in range(K):
        for j in range(K):
            if i != j:
                idx += [i, j]
    return idx + [0]


def parts(n, nsplit):
    """the contiguous parts [lo, hi) rkfdBatchSetSplit makes of a batch of n"""
    out = [(n * k // nsplit, n * (k + 1) // nsplit) for k in range(nsplit)]
    return [(lo, hi) for lo, hi in out if hi > lo]


def wavefront_pairs(idx, nsplit=1):
    """the ordered pairs (character in the lower half, character in the upper half) of the wavefronts a batch arranged as idx
    forms when it goes out in nsplit parts, and the characters left alone beside a stand-in half"""
    pairs, alone = set(), set()
    for lo, hi in parts(len(idx), nsplit):
        for p in range(lo, hi, 2):
            if p + 1 < hi:
                pairs.add((idx[p], idx[p + 1]))
            else:
                alone.add(idx[p])
    return pairs, alone


def arrangement(K, nsplit=3):
    """arrange(K) with the check that every ordered pair of unlike characters shares a wavefront in the single launch or in the
    split one, and that some instance meets the stand-in half -> (idx, pairs of the single launch, pairs of the split launch)"""
    idx = arrange(K)
    assert len(idx) == 2 * K * (K - 1) + 1
    one, alone1 = wavefront_pairs(idx, 1)
    many, alonen = wavefront_pairs(idx, nsplit)
    want = {(i, j) for i in range(K) for j in range(K) if i != j}
    assert want <= (one | many), sorted(want - (one | many))
    assert alone1 and alonen
    return idx, one, many


# ---- batches -------------------------------------------------------------------------------------------------------------------
def fill(b, chars, nlink):
    """the characters' inputs into a batch (Batch or EmuBatch) of len(chars) instances, before update_init"""
    b.set_state(np.array([c.dis for c in chars]), np.array([c.vel for c in chars]))
    if any(c.motor_in is not None for c in chars):
        b.set_motor_input(np.array([np.zeros(nlink) if c.motor_in is None else c.motor_in for c in chars]))
    if any(c.broken is not None for c in chars):
        b.set_broken(np.array([np.zeros(nlink, dtype=np.int32) if c.broken is None else c.broken for c in chars]))


def param_table(world, chars):
    """{name: (len(chars), width)} of the characters' parameter rows; a character without a row carries the model's values"""
    if not any(c.params for c in chars):
        return None
    return {n: np.array([ip.model_values(world, n) if not c.params else c.params[n] for c in chars]) for n in ip.NAMES}


def schedule(chars):
    """(len(chars), H, nlink) of the characters' control schedules, or None"""
    return np.ascontiguousarray(np.array([c.ctrl for c in chars])) if chars[0].ctrl is not None else None


def result(b, breakable):
    """what a run leaves behind: get_state (dis, vel, acc), get_contact (four arrays), get_pivot (two), get_broken"""
    r = tuple(b.get_state()) + tuple(b.get_contact()) + tuple(b.get_pivot())
    return r + ((b.get_broken(),) if breakable else ())


def run(b, chars, nsteps, breakable):
    """the characters through a batch of len(chars): fill, update_init, nsteps steps -> (status, result)"""
    fill(b, chars, b.nlink)
    b.update_init()
    st = b.status()                 # (the emulator reports per call, the device keeps the flag: or-ed they agree)
    u = schedule(chars)
    if u is None:
        b.update(nsteps)
    else:
        assert u.shape[1] == nsteps
        b.update_controlled(u)
    return st | b.status(), result(b, breakable)


RESULT_NAMES = ("dis", "vel", "acc", "cv_active", "cv_type", "cv_ref", "cv_f", "piv_type", "piv_prev", "broken")


def differing(got, idx, want):
    """positions of the mixed batch whose result is not, bit for bit, the batch-of-one result of their character:
    [(position, character, name of the first array that differs)]"""
    bad = []
    for p, c in enumerate(idx):
        for k, (x, y) in enumerate(zip(got, want[c])):
            if not np.array_equal(x[p], y[0]):
                bad.append((p, c, RESULT_NAMES[k])); break
    return bad


# ---- the oracle gate -----------------------------------------------------------------------------------------------------------
def oracle_run(oracle_cls, world, ch, nsteps):
    """the character alone on the oracle -> (oracle after nsteps, rigid contact count after rkFDUpdateInit and after every step)"""
    mc = ip.model_with(world, ch.params) if ch.params else world
    o = oracle_cls(mc.model)
    o.model_owner = mc              # (the copy's arrays must outlive the oracle)
    o.set_state(ch.dis, ch.vel)
    if ch.motor_in is not None:
        o.set_motor_input(ch.motor_in)
    if ch.broken is not None:
        o.set_broken(ch.broken)
    o.update_init()
    counts = [int((o.get_contact()[0] != 0).sum())]
    for k in range(nsteps):
        if ch.ctrl is not None:
            o.set_motor_input(ch.ctrl[k])
        o.update()
        counts.append(int((o.get_contact()[0] != 0).sum()))
    return o, counts


def assert_gate(counts, full, at_least=False):
    """counts: per character the oracle's contact counts [first evaluation, step 1, ...].  One character starts with none, one
    with the world's nominal maximum `full` (at_least: or more), one strictly between, and one count changes during the run."""
    first = [c[0] for c in counts]
    assert 0 in first, first
    assert any(f >= full if at_least else f == full for f in first), first
    assert any(0 < f < full for f in first), first
    assert any(len(set(c)) > 1 for c in counts), counts


def assert_slides(o, ch, dof, counts):
    """a character launched with a tangential velocity is still in contact and has kept most of it on the oracle: its contacts are at
    the friction cone (the slide branch of the Gauss-Seidel sweeps), a sticking contact would have stopped it within a step"""
    assert min(counts[:3]) > 0 and ch.vel[dof] != 0.0
    assert o.get_state()[1][dof] / ch.vel[dof] > 0.5


# ---- worlds and characters -----------------------------------------------------------------------------------------------------
def box_characters(R, w):
    """the box (half height 0.05) of world w (box_world) over the rigid half of the floor in seven states:
    airborne, flat, on an edge, on a corner, flat and sliding, flat and spinning, 0.02 mm above the floor and falling"""
    S = R.scenarios
    m = w.model.contents
    at = np.zeros(6); at[1] = 1.0                     # over the hard half, no rotation

    def seated(aa):
        d = at.copy(); d[3:6] = aa; d[2] = 0.1
        d[2] -= S.lowest_vertex_z(m, d, 0) + SEAT_IN
        return d
    z6 = np.zeros(6)
    tilted = S.aa_from_rpy_deg(10.0, 20.0, 30.0)
    air = at.copy(); air[2] = 0.3; air[3:6] = tilted
    flat = seated(np.zeros(3))
    hover = at.copy(); hover[2] = 0.05 + 2e-5
    return [Character("airborne", air, z6),
            Character("flat", flat, z6),
            Character("edge", seated((0.2, 0.0, 0.0)), z6),
            Character("corner", seated(tilted), z6),
            Character("flat sliding", flat, (0.5, 0, 0, 0, 0, 0)),
            Character("flat spinning", flat, (0, 0, 0, 0, 0, 3.0)),
            Character("landing", hover, (0, 0, -0.02, 0, 0, 0))]


BOX_FULL = 4                    # a flat box stands on four vertices
BOX_SHORT = (0, 1, 3, 6)        # the four characters of the CPU tier: airborne, flat, corner, landing


def box_world(R, volume=False):
    sc = R.scenarios.config1_volume(batch=1) if volume else R.scenarios.config1_rigid(batch=1)
    return sc["world"], sc["max_rigid"]


def humanoid_characters(R, world_of=None):
    """config 4's humanoid: instances 0 and 1 as seeded, and from instance 0: lifted 0.3 m; lifted just clear of the floor and
    falling; standing with 0.3 m/s lateral base velocity (the contacts slide); the perturbed pose BEFORE seat_soles_flat levels
    the soles, lowered until its lowest vertex is seated - tilted soles, a few vertices.  -> (world, max_rigid, characters)"""
    S = R.scenarios
    sc = (S.config4 if world_of is None else world_of)(batch=2)
    w = sc["world"]; m = w.model.contents
    bo = w.dof_offset(0)
    d0, d1 = sc["dis"][0], sc["dis"][1]
    z = np.zeros(m.ndof)
    air = d0.copy(); air[bo + 2] += 0.3
    land = d0.copy(); land[bo + 2] -= S.lowest_vertex_z(m, land, 0) - 2e-5
    vland = z.copy(); vland[bo + 2] = -0.02
    vslide = z.copy(); vslide[bo + 1] = 0.3
    init = w.init_dis(0); n = init.shape[0]
    u = S.splitmix64_uniform(0x5EED0004, n - 6)
    tilt = d0.copy(); tilt[bo:bo + n] = init; tilt[bo + 6:bo + n] += (u - 0.5) * 0.1
    tilt[bo + 2] -= S.lowest_vertex_z(m, tilt, 0) + S.SEAT_DEPTH
    chars = [Character("standing 0", d0, z), Character("standing 1", d1, z), Character("airborne", air, z),
             Character("landing", land, vland), Character("standing, sliding", d0, vslide), Character("tilted soles", tilt, z)]
    return w, sc["max_rigid"], chars


HUMANOID_FULL = 7               # the standing humanoid: at least 7 of its 8 sole vertices


def with_params_and_controls(world, chars, nsteps, seed=0xC4A2):
    """every character with a parameter row of its own - the first the model's, the second light (masses and inertias x 0.7), the
    third heavy (x 1.3), the others from instance_params.randomised - and a control schedule of its own over the steps"""
    K = len(chars)
    P = ip.randomised(world, K, seed)
    m = world.model.contents
    rows = [ip.of_instance(P, i) for i in range(K)]
    rows[0] = {n: ip.model_values(world, n).copy() for n in ip.NAMES}
    for i, s in ((1, 0.7), (2, 1.3)):
        rows[i] = {n: ip.model_values(world, n).copy() for n in ip.NAMES}
        rows[i]["mass"] *= s; rows[i]["inertia"] *= s
    rng = np.random.default_rng(seed + 1)
    out = []
    for i, c in enumerate(chars):
        u = rng.normal(0.0, 0.5 * (1 + i), (nsteps, m.nlink))
        out.append(c.but(c.label + " +row +schedule", params=rows[i], ctrl=u))
    return out


WALL_PICK = 3                   # of scenarios.wall_hit(batch=10): at the seeded speed the two upper joints break at once, at three times all three


def wall_characters(R):
    """scenarios.wall_hit (bricks on breakable float joints, world tables in LDS under RKFD_W = 2): the box at rest 2 mm further
    from the bricks (it touches nothing, nothing breaks); the seeded speed (the two upper joints break); three times the speed
    (all three break); three times the speed with the two upper bricks broken off beforehand through set_broken (the lowest joint
    then holds).  -> (world, max_rigid, characters)"""
    sc = R.scenarios.wall_hit(batch=10)
    w = sc["world"]; m = w.model.contents
    d, v = sc["dis"][WALL_PICK], sc["vel"][WALL_PICK]
    jt = m.arr("jtype", m.nlink)
    bricks = [i for i in range(m.nlink) if jt[i] == R.JOINT_BRFLOAT]
    assert len(bricks) == 3
    br = np.zeros(m.nlink, dtype=np.int32); br[bricks[1:]] = 1
    back = d.copy(); back[w.dof_offset(1)] -= 0.002
    chars = [Character("box at rest", back, np.zeros_like(v)), Character("seeded speed", d, v), Character("three times the speed", d, 3.0 * v),
             Character("upper bricks broken beforehand, three times the speed", d, 3.0 * v, broken=br)]
    return w, sc["max_rigid"], chars


def assert_wall_gate(counts, broken, bricks=3):
    """counts as in assert_gate, broken: per character the oracle's final flags.  The wall has no nominal full contact: one character
    starts with no contact and the others with some, the largest count of the run differs between characters, one count changes;
    the final flags are of at least three kinds, nothing broken and everything broken among them."""
    first = [c[0] for c in counts]
    assert 0 in first and max(first) > 0, first
    assert len({max(c) for c in counts}) >= 3, counts
    assert any(len(set(c)) > 1 for c in counts), counts
    kinds = {tuple(b) for b in broken}
    assert len(kinds) >= 3 and 0 in {sum(k) for k in kinds} and bricks in {sum(k) for k in kinds}, kinds


# ---- the poisoned neighbour (emulator only; never on a device) -------------------------------------------------------------------
POISONED = 2                    # position in BOX_SHORT of the character that is replaced


def poisoned_box_characters(R, w):
    """the four box characters of the CPU tier with the corner one replaced by a flat box whose x coordinate is a NaN"""
    chars = [box_characters(R, w)[i] for i in BOX_SHORT]
    bad = chars[1].dis.copy(); bad[0] = np.nan
    chars[POISONED] = Character("flat, NaN in dis", bad, chars[1].vel)
    return chars


if __name__ == "__main__":
    # child process of tests/test_emu_mixed.py::test_poisoned_neighbour...: python mixed_batches.py <nsteps> <out.npz>
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), os.path.join(here, "emu")]
    import rkfd_pkg
    from emu import EmuBatch
    R_ = rkfd_pkg.load()
    w_, mr_ = box_world(R_)
    chars_ = poisoned_box_characters(R_, w_)
    idx_, _, _ = arrangement(len(chars_))
    eb_ = EmuBatch(w_, len(idx_), max_rigid=mr_, ipw=2)
    st_, res_ = run(eb_, [chars_[i] for i in idx_], int(sys.argv[1]), False)
    np.savez(sys.argv[2], status=st_, **{n: x for n, x in zip(RESULT_NAMES, res_)})
