"""The rotation primitives of roki-fd_amd/csrc/device/rkfd_dev_base.h - d_sincos, d_atan2_ypos, d_from_aa, d_to_aa - as the lane
emulator's build compiles them (tests/emu/rkfd_emu_prim.cpp), against np.longdouble, without a GPU.

Every random state of the older tests keeps d_sincos in its k = 0 quadrant and d_atan2_ypos at x > 0; here every quadrant, the
two-term reduction up to |x| = 1e5, the rint ties, all five intervals of d_atan_pos and both signs of x are asked for, and
d_to_aa( d_from_aa( aa ) ) for rotations up to and beyond the half turn.

Bounds (none of them comes from what the code gives):
  d_sincos        |error| <= 2^-52: the header claims under 1 ulp of a result of at most 1; |s^2 + c^2 - 1| <= 4 x 2^-52.  A quadrant
                  mix-up is an error of order 1.
  d_atan2_ypos    |error| <= 4 x 2^-52 against long double arctan2 (results up to pi: ulp 2^-51; fdlibm's atan is good to 1 ulp, the
                  quotient y / x adds half an ulp of the argument, pi - atan one more rounding).
  d_from_aa       8 x 2^-52 against a long double Rodrigues formula, orthonormality to the same bound: rows and columns of length 1
                  and distinct ones at right angles, each to 8 x 2^-52.  (The entries of R' R - 1 are another measure: its diagonal
                  is twice the defect of a length, and reaches 8.7 x 2^-52 next to a half turn, where the formula turns the defect
                  delta of the rounded unit axis into 4 delta n_i^2; rot_cases.from_aa_errors, printed here.)  Below the threshold RKFD_TOL
                  = 1e-12 the function returns the identity by definition (links_cases.aa_edge_states): theta = 3e-13 is asserted
                  to give exactly the identity, which is within theta of the true rotation.
  round trip      max( 1e-12, 1e-14 / ( pi - theta ) ): d_to_aa reads the antisymmetric part of the matrix, 2 sin( theta ) n, which
                  vanishes at the half turn - an error of 1.6e-16 / ( pi - theta ) measured, sixty times that asserted; for theta in
                  ( pi, 2 pi ) the result is the equivalent rotation -( 2 pi - theta ) n.
Measured values: profiles/r13_rot_parity.txt (tools/rot_parity.py).  Signed zeros are left out: d_atan2_ypos( 0, -0.0 ) returns 0
where libm gives pi, and no caller passes -0.0 there."""
import numpy as np
import pytest

import rot_cases as rc

EPS = 2.0 ** -52


@pytest.fixture(scope="module", autouse=True)
def long_double():
    if not np.finfo(np.longdouble).eps < 2e-19:
        pytest.skip("np.longdouble is no wider than double here: no reference")


SINCOS = list(rc.sincos_inputs(ndraw=1))


@pytest.mark.parametrize("name", SINCOS)
def test_sincos_against_long_double(name):
    x = rc.sincos_inputs()[name]
    es, ec, eu = rc.sincos_errors(x)
    print(f"d_sincos {name}: n = {x.size}, |sin error| {es:.3e}, |cos error| {ec:.3e}, |s^2 + c^2 - 1| {eu:.3e}")
    assert es <= EPS and ec <= EPS, (name, es, ec)
    assert eu <= 4 * EPS, (name, eu)


def test_sincos_inputs_reach_every_quadrant_and_both_reduction_terms():
    """what the inputs are for: all four values of q = k & 3 on both signs of k, and k large enough that the second term of the
    reduction matters (k x 6.08e-11 above an ulp of the reduced argument from k ~ 1e-5 on: every range above 0.8)"""
    ins = rc.sincos_inputs()
    k = np.concatenate([np.rint(x * (2 / np.pi)) for x in ins.values()])
    for sign in (1, -1):
        assert {int(q) for q in np.unique(k[k * sign > 0].astype(np.int64) & 3)} == {0, 1, 2, 3}
    assert np.abs(k).max() > 6e4 and (np.rint(ins["uniform +-0.8"] * (2 / np.pi)) != 0).sum() < ins["uniform +-0.8"].size * 0.02


ATAN2 = list(rc.atan2_inputs(ndraw=1))


@pytest.mark.parametrize("name", ATAN2)
def test_atan2_ypos_against_long_double(name):
    y, x = rc.atan2_inputs()[name]
    assert not np.signbit(x[x == 0]).any() and not np.signbit(y[y == 0]).any()
    e = rc.atan2_error(y, x)
    print(f"d_atan2_ypos {name}: n = {x.size}, |error| {e:.3e}")
    assert e <= 4 * EPS, (name, e)


def test_atan2_inputs_reach_every_interval_on_both_signs():
    ins = rc.atan2_inputs()
    y = np.concatenate([v[0] for v in ins.values()]); x = np.concatenate([v[1] for v in ins.values()])
    edges = (0.0,) + rc.ATAN_BOUNDARIES + (np.inf,)
    for sg in (1.0, -1.0):
        on = x * sg > 0
        with np.errstate(over="ignore"):          # (1e300 / 1e-300: the quotient the device forms, too)
            r = y[on] / np.abs(x[on])
        for lo, hi in zip(edges[:-1], edges[1:]):
            assert ((r >= lo) & (r < hi)).sum() > 100, (sg, lo, hi)
    yb, xb = ins["interval boundaries"]
    for b in rc.ATAN_BOUNDARIES:
        for sg in (1.0, -1.0):
            r = yb[xb * sg > 0] / np.abs(xb[xb * sg > 0])
            assert (r == b).any() and (r == np.nextafter(b, 0)).any() and (r == np.nextafter(b, 9)).any()
    assert ((x == 0) & (y > 0)).any() and ((x == 0) & (y == 0)).any()


def test_from_aa_against_long_double_rodrigues():
    aa = rc.aa_inputs()
    th = np.linalg.norm(aa, axis=1)
    assert th[0] == 0 and abs(th[1] - 3e-13) < 1e-27 and abs(th[-1] - 7.0) < 1e-14 and th.size == 15005
    e, orth, gram, Rd = rc.from_aa_errors(aa)
    print(f"d_from_aa: n = {th.size}, |R - Rodrigues| {e:.3e}, lengths and angles of rows and columns {orth:.3e}, |R' R - 1| {gram:.3e}")
    assert e <= 8 * EPS and orth <= 8 * EPS, (e, orth)
    below = th < rc.IDENT_TOL
    assert below.sum() == 2 and (Rd[below] == np.eye(3)).all()          # theta = 0 and 3e-13: the identity, exactly
    Rl, _, _ = rc.rodrigues_ld(aa[below])
    assert float(np.abs(Rd[below] - Rl).max()) <= th[below].max()


def test_to_aa_of_from_aa_returns_the_equivalent_rotation():
    aa = rc.aa_inputs()
    th = np.linalg.norm(aa, axis=1)
    err, bound = rc.roundtrip_errors(aa)
    for lo, hi in ((0.0, 1.5), (1.5, 3.0), (3.0, np.pi), (np.pi, 2 * np.pi + 1e-9), (6.9, 7.1)):
        on = (th >= lo) & (th < hi)
        print(f"d_to_aa( d_from_aa ) theta in [{lo:.3f}, {hi:.3f}): n = {on.sum()}, |error| {err[on].max():.3e}, "
              f"error x ( pi - theta ) {(err[on] * 1e-14 / np.where(bound[on] > 1e-12, bound[on], np.inf)).max():.3e}, closest to pi {np.abs(np.pi - th[on]).min():.2e}")
    assert (err <= bound).all(), (th[err > bound], err[err > bound], bound[err > bound])
    # beyond the half turn the vector comes back on the opposite axis, with |aa| in [0, pi]
    back = rc.d_to_aa(rc.d_from_aa(aa))
    assert (np.linalg.norm(back, axis=1) <= np.pi + 1e-15).all()
    beyond = (th > np.pi + 1e-3) & (th < 2 * np.pi - 1e-3)
    assert ((back[beyond] * aa[beyond]).sum(axis=1) < 0).all()
