"""Unlike instances in one wavefront on the MI355X (tests/mixed_batches.py).  The kernel behind the headline figure puts two instances
into a wavefront (RKFD_W = 2): ballots shifted to the half, broadcasts through ds_bpermute within the half, Gauss-Seidel increments
through DPP under a per-instance contact count, wave-wide ANY() branches a half runs because its neighbour voted for them, loops
with per-instance trip counts.  Every other test of that kernel pairs near-twins; here every ordered pair of a world's characters -
airborne beside standing, sliding beside resting, breaking beside whole, overflowing beside empty - shares a wavefront, and every
instance must be, bit for bit, what its character gives in a batch of ONE on the generic kernel.  The same arrangement runs on the
generic kernel and on the world-specific one with one instance per wavefront (neighbours in memory, not in the wavefront), and
under the Vert and Volume plugins, which refuse two per wavefront.  No state that is not finite goes to the device."""
import numpy as np
import pytest

import instance_params as ip
import mixed_batches as mb

pytestmark = pytest.mark.gpu

NSTEPS = 12
VARIANTS = ["generic", "spec", "ipw2", "ipw2_split"]


def _configure(b, variant):
    if variant.startswith("ipw2"):
        b.set_instances_per_wave(2)
    if variant != "generic":
        b.specialize()
    if variant.startswith("ipw2"):
        assert b.instances_per_wave() == 2
    if variant == "ipw2_split":
        b.set_split(3); b.set_steps_per_launch(5)


class Case:
    """a world, its characters, the oracle's runs of them (the gate) and the batches of one on the generic kernel"""

    def __init__(self, R, oracle_cls, name):
        self.R, self.name, self.breakable, self.expect_status = R, name, False, 0
        if name in ("box", "box_cap2", "box_volume"):
            self.world, self.max_rigid = mb.box_world(R, volume=name == "box_volume")
            if name == "box_cap2":
                self.max_rigid, self.expect_status = 2, 2
            self.chars = mb.box_characters(R, self.world)
            self.full, self.at_least = mb.BOX_FULL, False
        elif name in ("humanoid", "humanoid_par_ctrl", "humanoid_vert"):
            self.world, self.max_rigid, self.chars = mb.humanoid_characters(R, R.scenarios.config4_vert if name == "humanoid_vert" else None)
            if name == "humanoid_par_ctrl":
                self.chars = mb.with_params_and_controls(self.world, self.chars, NSTEPS)
            self.full, self.at_least = mb.HUMANOID_FULL, True
        else:
            self.world, self.max_rigid, self.chars = mb.wall_characters(R)
            self.breakable = True
        # the gate: alone on the oracle the characters are as unlike as the tests claim
        # (the box and the humanoid worlds under another plugin carry the characters of the MLCP world: gated there)
        self.oracles = None
        if name in ("box", "box_cap2", "humanoid", "humanoid_par_ctrl", "wall_hit"):
            runs = [mb.oracle_run(oracle_cls, self.world, c, NSTEPS) for c in self.chars]
            self.oracles = [o for o, _ in runs]; self.counts = [c for _, c in runs]
            if self.breakable:
                mb.assert_wall_gate(self.counts, [o.get_broken()[1:4] for o in self.oracles])
            else:
                mb.assert_gate(self.counts, self.full, self.at_least)
                for i, dof in ((4, 0), (5, 5)) if name.startswith("box") else ((4, self.world.dof_offset(0) + 1),):
                    mb.assert_slides(self.oracles[i], self.chars[i], dof, self.counts[i])
        self.idx, self.pairs, self.pairs_split = mb.arrangement(len(self.chars))
        self.status, self.want = [], []
        for c in self.chars:
            b = R.Batch(ip.model_with(self.world, c.params) if c.params else self.world, 1, device=0, max_rigid=self.max_rigid)
            st, res = mb.run(b, [c], NSTEPS, self.breakable)
            b.close()
            self.status.append(st); self.want.append(res)

    def mixed(self, variant):
        chars = [self.chars[i] for i in self.idx]
        b = self.R.Batch(self.world, len(chars), device=0, max_rigid=self.max_rigid)
        P = mb.param_table(self.world, chars)
        if P is not None:
            for n, v in P.items():
                b.set_param(n, v)
            assert b.has_params()
        _configure(b, variant)
        st, got = mb.run(b, chars, NSTEPS, self.breakable)
        b.close()
        return st, got


@pytest.fixture(scope="module")
def cases(R, oracle_cls):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(R, oracle_cls, name)
        return made[name]
    return get


def _check(case, variant):
    st, got = case.mixed(variant)
    bad = mb.differing(got, case.idx, case.want)
    print(f"{case.name} {variant}: batch {len(case.idx)}, status {st}, {len(bad)} instances differ from their batch of one")
    assert st == case.expect_status
    assert not bad, [(p, case.chars[c].label, what) for p, c, what in bad]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["box", "box_cap2", "humanoid", "wall_hit", "humanoid_par_ctrl"])
def test_unlike_neighbours_equal_their_batches_of_one(cases, name, variant):
    """box_cap2: capacity 2 - the flat and the landing boxes overflow (status 2), their surplus vertices dropped the same way alone
    and in company; the others do not.  humanoid_par_ctrl: every character with a parameter row (the model's, a light one, a heavy
    one, random ones) and a control schedule of its own, through update_controlled with the table in place; the batches of one
    run on a copy of the model holding the row.  wall_hit: breakable joints keep the world tables in LDS under RKFD_W = 2, the
    humanoid reads them from global memory."""
    case = cases(name)
    if name == "box_cap2":
        assert [case.status[i] for i in (0, 1, 2, 3)] == [0, 2, 0, 0] and 2 in case.status[4:]
    else:
        assert case.status == [0] * len(case.chars)
    _check(case, variant)


@pytest.mark.parametrize("variant", ["generic", "spec"])
@pytest.mark.parametrize("name", ["humanoid_vert", "box_volume"])
def test_unlike_neighbours_under_the_other_plugins(R, cases, name, variant):
    """the Vert QP (humanoid) and the Volume plugin (box): two per wavefront is refused; neighbours in memory with widely different
    active sets must not reach into each other's contact arrays"""
    case = cases(name)
    probe = R.Batch(case.world, 2, device=0, max_rigid=case.max_rigid)
    with pytest.raises(R.RkfdError, match="two instances per wavefront need"):
        probe.set_instances_per_wave(2)
    assert probe.instances_per_wave() == 1
    probe.close()
    assert case.status == [0] * len(case.chars)
    _check(case, variant)


def _rel(x, y):
    return np.abs(x - y).max() / max(1.0, np.abs(y).max())


def test_humanoid_characters_agree_with_the_oracle(cases):
    """the expected values anchored outside the device code: the batches of one against the oracle at the bound
    test_full_batch_sample_matches_oracle uses for config 4 (1e-8), equal contact sets"""
    case = cases("humanoid")
    for c, o, res in zip(case.chars, case.oracles, case.want):
        for x, y in zip(res[:3], o.get_state()):
            assert _rel(x[0], y) < 1e-8, c.label
        oact, otyp, oref, of = o.get_contact()
        assert (res[3][0] == oact).all(), c.label
        assert _rel(res[6][0], of * (oact[:, None] != 0)) < 1e-8, c.label
