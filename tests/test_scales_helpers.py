"""CPU: the scaled problems of tests/scales.py against the oracle alone (no GPU).

What tests/test_gpu_scales.py may demand of the library at scale 2^k depends on what the REFERENCE does there, and the reference
is not scale-free everywhere.  These tests pin, for the oracle (the literal restatement of the reference, oracle/spx_oracle.c):

  * the operators whose Float64 / Float32 evaluation is equivariant bit for bit, oracle(2^k P) == 2^k oracle(P), at every k of
    their set -- there the GPU comparison of y(2^k P) with 2^k y(P) may demand bits; a later change to the oracle that breaks
    this says so here first;
  * ShiftedGroupNormL2Binf is NOT equivariant: the upper end of its bracket is built from `ansatz = lmin + epsilon` with the
    absolute epsilon = 1 (src/shiftedGroupNormL2Binf.jl:81,97), and at k <= -10 the bracket of one group of scales.binf_regime()
    no longer encloses its root, `fl * fm > 0` (:102) fires and the reference writes zeros where it solves the group at k = 0;
    (the same happens to a third of the groups of 128 of scales.groups(128, 40, True): the regime depends on the weights, not on
    the group size);
  * psi(y) of ShiftedNormL1B2 is not either: IndBallL2 carries an absolute atol = eps, so a point far outside the ball at k = 0
    is feasible at k = -500;
  * the box objectives carry an absolute sqrt(eps) slack: a point outside [l, u] by 1e-9 * 2^k is inside it at k = -40 and
    outside at k = +40;
  * the range condition the scaled tests state about their own inputs (scales.assert_in_range)."""
import math

import numpy as np
import pytest

import scales

ALL_CASES = [(name, False) for name in scales.CPU_CASES] + [(name, True) for name in scales.CPU_CASES_F32]
EQUIVARIANT = [(n, f) for n, f in ALL_CASES if "binf_128" not in n]


@pytest.mark.parametrize("name,f32", EQUIVARIANT, ids=["%s%s" % (n, "_f32" if f else "") for n, f in EQUIVARIANT])
def test_oracle_is_bit_equivariant(orc, name, f32):
    """oracle(c q, c xk, c sj; c_lambda lambda, c Delta, c l, c u) == c oracle(q, xk, sj; ...), bit for bit, at every k"""
    P = (scales.CPU_CASES_F32 if f32 else scales.CPU_CASES)[name]()
    assert P.op in scales.BIT_EQUIVARIANT
    y0 = scales.oracle_y(orc, P)
    assert np.isfinite(y0).all() and np.count_nonzero(y0) > P.n // 2
    for k in (scales.K32 if f32 else scales.ALL_K64):
        scales.assert_in_range(P, k)
        yk = scales.oracle_y(orc, scales.scaled(P, k))
        assert yk.dtype == y0.dtype
        assert scales.same_bits(scales.unscale(yk, k), y0), (name, k, scales.ulps(scales.unscale(yk, k), y0))


def test_obj_plain_l1_is_bit_equivariant(orc):
    P = scales.CPU_CASES["prox_l1"]()
    for k in scales.ALL_K64:
        assert scales.obj_equivariance(orc, P, k) == 0.0, k


def test_every_bit_equivariant_operator_has_a_case():
    ops64 = {mk().op for mk in scales.CPU_CASES.values()}
    ops32 = {mk().op for mk in scales.CPU_CASES_F32.values()}
    assert set(scales.BIT_EQUIVARIANT) <= ops64 and set(scales.F32_OPS) == ops32


def test_the_binf_regime_really_occurs(orc):
    """groups of 8: at least one group is zeroed (y == -(xk + sj) exactly) at some k <= -10 and is not zeroed at k = 0; every
    group outside that set agrees with the scaled unit-scale answer to 1e-9"""
    P = scales.binf_regime()
    z0, y0 = scales.binf_zeroed(orc, P, 0)
    seen = np.zeros_like(z0)
    for k in (-500, -200, -40, -10):
        scales.assert_in_range(P, k)
        z, y = scales.binf_zeroed(orc, P, k)
        more = z & ~z0
        seen |= more
        assert not (z0 & ~z).any(), k                     # what the reference zeroes at k = 0 stays zeroed
        keep = np.repeat(~more, 8)
        bar = 1e-9 * np.maximum(np.abs(y0), np.abs(P.xk + P.sj))
        assert (np.abs(y - y0)[keep] <= bar[keep]).all(), (k, float(np.max(np.abs(y - y0)[keep])))
        # the zeroed group is a solved one at k = 0: far from zero there
        for g in np.flatnonzero(more):
            sl = slice(8 * g, 8 * g + 8)
            assert np.max(np.abs(y0[sl] + (P.xk + P.sj)[sl])) > 1e-3, (k, g)
    assert seen.sum() >= 1, "no group is zeroed at small scale only: the seed no longer shows the regime"
    for k in (40, 200, 500):                              # and at large scale the reference solves what it solves at k = 0
        z, y = scales.binf_zeroed(orc, P, k)
        assert np.array_equal(z, z0), k
        assert (np.abs(y - y0) <= 1e-9 * np.maximum(np.abs(y0), np.abs(P.xk + P.sj))).all(), k


def test_the_binf_regime_also_occurs_at_size_128(orc):
    """It is not a matter of the group size: on scales.groups(128, 40, True), whose weights are lambda_g = ||S_g|| {0.3, 0.8, 1.5} /
    sigma, the reference zeroes a third of the groups at k <= -10 that it solves at k >= -4 (on N(0, 1) weights U(0.2, 2), as in
    binf_regime, groups of 128 are equivariant).  That is why the case is left out of test_oracle_is_bit_equivariant; the
    groups outside that set agree with the scaled unit-scale answer to 1e-9, and the GPU is held to the oracle at each k."""
    P = scales.CPU_CASES["prox_group_l2_binf_128"]()
    z0, y0 = scales.binf_zeroed(orc, P, 0)
    bar = 1e-9 * np.maximum(np.abs(y0), np.abs(P.xk + P.sj))
    for k in scales.ALL_K64:
        scales.assert_in_range(P, k)
        z, y = scales.binf_zeroed(orc, P, k)
        more = z & ~z0
        assert not (z0 & ~z).any(), k
        assert (more.sum() >= 5) if k <= -10 else (more.sum() == 0), (k, np.flatnonzero(more).tolist())
        keep = np.repeat(~more, 128)
        assert (np.abs(y - y0)[keep] <= bar[keep]).all(), k


def test_obj_l1_b2_flips_with_the_absolute_eps(orc):
    y, x, sj, lam, delta = scales.b2_flip_point()
    assert orc.obj_l1_b2(y, x, sj, lam, delta) == math.inf
    c = lambda a, k: np.ldexp(a, k)
    v = orc.obj_l1_b2(c(y, -500), c(x, -500), c(sj, -500), math.ldexp(lam, -500), math.ldexp(delta, -500))
    assert np.isfinite(v) and v == math.ldexp(orc.obj_plain("l1", y, x, sj, lam), -1000)
    assert orc.obj_l1_b2(c(y, 500), c(x, 500), c(sj, 500), math.ldexp(lam, 500), math.ldexp(delta, 500)) == math.inf


@pytest.mark.parametrize("kind", ["l1", "l0", "lhalf"])
def test_the_box_slack_is_absolute(orc, kind):
    y, x, sj, l, u = scales.box_slack_point()
    lam_pow = scales.LAM_POW[kind]
    out = {}
    for k in (-40, 0, 40):
        c = lambda a: np.ldexp(a, k)
        out[k] = orc.obj_box(kind, c(y), c(x), c(sj), math.ldexp(scales.LAM, int(lam_pow * k)), math.ldexp(l, k), math.ldexp(u, k))
    assert np.isfinite(out[-40]) and np.isfinite(out[0]) and out[40] == math.inf, out
    assert out[-40] == math.ldexp(out[0], -80)            # psi scales by c^2 where it is finite


def test_the_range_condition_refuses_what_is_out_of_scope():
    P = scales.separable("prox_l1", 1001)
    for k in scales.ALL_K64:
        assert scales.assert_in_range(P, k)
    with pytest.raises(ValueError):
        scales.assert_in_range(P, 520)                    # squares overflow
    q = np.array(P.q)
    q[11] = 1e-8                                          # an unclamped element: its square is subnormal at 2^-500
    bad = scales.Problem(op="prox_l1", q=q, xk=np.array(P.xk), sj=np.array(P.sj), lam=scales.LAM, sigma=scales.SIGMA)
    assert scales.assert_in_range(bad, -200)
    with pytest.raises(ValueError):
        scales.assert_in_range(bad, -500)
    F = scales.separable("prox_l0", 1001, dtype=np.float32)
    for k in scales.K32:
        assert scales.assert_in_range(F, k)
    with pytest.raises(ValueError):
        scales.assert_in_range(F, 80)                     # lambda c^2 = 0.7 * 2^160 is no Float32


def test_scaled_problems_keep_their_zeros_and_their_floor():
    P = scales.groups(8, 40, True)
    assert not P.q[:8].any() and not P.xk[:8].any() and not P.sj[:8].any()      # the all-zero group
    assert (P.q[3::97] == 0).all()
    for a in (P.q, P.xk, P.sj, P.xk + P.sj, (P.q + P.xk) + P.sj):
        assert (np.abs(a[a != 0]) >= scales.FLOOR).all()
    Pk = scales.scaled(P, -500)
    assert Pk.k == -500 and Pk.sigma == P.sigma and Pk.delta == math.ldexp(P.delta, -500)
    assert np.array_equal(np.ldexp(Pk.q, 500), P.q) and np.array_equal(np.ldexp(Pk.lam, 500), P.lam)
    sq = Pk.xk[Pk.xk != 0] ** 2
    assert (sq >= 2.2250738585072014e-308).all()          # every nonzero square is a normal double
    H = scales.scaled(scales.separable("prox_lhalf", 33), -40)
    assert H.lam == math.ldexp(scales.LAM, -60)
    Z = scales.scaled(scales.separable("prox_l0_box", 33), 40)
    assert Z.lam == math.ldexp(scales.LAM, 80) and Z.l == math.ldexp(scales.LS, 40)
