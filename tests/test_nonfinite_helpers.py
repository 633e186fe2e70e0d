"""The CPU side of tests/nonfinite.py against the oracle alone: the class rules, the nan-aware bars (they accept the reference's own
result and refuse one that drops, adds or moves a NaN / Inf), and the input condition of check_sum -- sum |term| < 1e300 -- for
every plant set on the reference's own y.  The data, layouts and plant positions are the ones tests/test_gpu_nonfinite.py uses."""
import math

import numpy as np
import pytest

import arbiter
import nonfinite as nf

NAN, INF = np.nan, np.inf


def test_class_rules():
    a = np.array([0.0, -0.0, 5e-324, 1e308, INF, -INF, NAN, -NAN])
    assert nf.classes(a).tolist() == [0, 0, 0, 0, 1, 2, 3, 3]
    b = a.copy()
    assert nf.same_bits_or_both_nan(a, b).all()
    b[0], b[1] = -0.0, 0.0                                   # signed zeros are different bits
    assert nf.same_bits_or_both_nan(a, b).tolist() == [False, False] + [True] * 6
    assert nf.scalar_same(NAN, -NAN) and not nf.scalar_same(0.0, -0.0) and nf.scalar_same(INF, INF) and not nf.scalar_same(NAN, INF)
    assert nf.triple_same((1.0, NAN, INF), (1.0, NAN, INF)) and not nf.triple_same((1.0, NAN, INF), (1.0, 0.0, INF))
    assert nf.sum_class([1.0, 2.0]) == "finite" and nf.sum_class([1.0, INF]) == "+inf" and nf.sum_class([-INF, 3.0]) == "-inf"
    assert nf.sum_class([INF, -INF]) == "nan" and nf.sum_class([NAN, 1.0]) == "nan" and nf.sum_class([]) == "finite"
    # whatever the order, IEEE addition gives that class
    rng = np.random.default_rng(0)
    for terms in ([1.0, INF, 2.0], [INF, -INF, 1.0], [NAN, INF], [-INF, -1.0, -INF], [1e-300, -1.0]):
        for _ in range(5):
            acc = np.float64(0.0)
            with np.errstate(all="ignore"):
                for t in rng.permutation(terms):
                    acc = acc + t
            assert nf.scalar_class(acc) == nf.sum_class(terms)


def test_check_sum_accepts_and_refuses():
    t = np.array([1.0, -2.0, 3.5])
    assert nf.check_sum(2.5, t, "finite") == "finite"
    assert nf.check_sum(2.5 + 1e-13, t, "finite, inside the bar") == "finite"
    for got in (2.5 + 1e-10, NAN, INF):
        with pytest.raises(AssertionError):
            nf.check_sum(got, t, "finite, refused")
    assert nf.check_sum(1.4, np.array([1.0, 1.0]), "factor", factor=0.7, exact=True) == "finite"
    tn = np.array([1.0, NAN, 2.0])
    assert nf.check_sum(NAN, tn, "nan") == "nan"
    for got in (3.0, INF):                                   # a NaN dropped from the sum
        with pytest.raises(AssertionError):
            nf.check_sum(got, tn, "nan dropped")
    assert nf.check_sum(INF, np.array([1.0, INF]), "+inf") == "+inf"
    assert nf.check_sum(-INF, np.array([-INF, 5.0]), "-inf") == "-inf"
    assert nf.check_sum(NAN, np.array([-INF, INF]), "both") == "nan"
    for got, terms in ((NAN, [1.0, INF]), (-INF, [1.0, INF]), (INF, [INF, -INF]), (0.0, [INF, -INF])):
        with pytest.raises(AssertionError):
            nf.check_sum(got, np.array(terms), "refused")
    with pytest.raises(AssertionError):                      # the input condition
        nf.check_sum(2e300, np.array([1e300, 1e300]), "too large")


def test_plants():
    n = 11
    z = np.ones(n)
    pos = nf.positions(n, [5, 0, 7])
    assert pos == [0, 10, 5, 7]
    for name in nf.PLANTS_SEPARABLE:
        q, x, s = nf.plant(name, z, z, z, pos)
        touched = (q != 1.0) | (x != 1.0) | (s != 1.0)
        assert np.flatnonzero(touched).tolist() == ([] if name == "none" else sorted(pos)), name
        assert z.sum() == n                                   # the clean data stay as they were
    q, _, _ = nf.plant("pminf-q", z, z, z, pos)
    assert (q == INF).sum() == 2 and (q == -INF).sum() == 2
    q, x, s = nf.plant("tiny", z, z, z, pos)
    seen = {(float(v), bool(np.signbit(v))) for a in (q, x, s) for v in a[pos]}
    assert seen == {(float(v), bool(np.signbit(v))) for v in nf.TINY}
    q, x, s = nf.plant("huge", z, z, z, pos)
    assert sorted(x[pos].tolist()) == [-1e150, -1e150, 1e150, 1e150] and q.sum() == n and s.sum() == n
    q, x, s = nf.plant("large", z, z, z, pos)
    assert q[pos].tolist() == [1e148, 1.0, -1e148, 1.0] and s[pos].tolist() == [1.0, 1e148, 1.0, -1e148] and x.sum() == n


def _refuses(fn, y, pos):
    """the bar refuses y with the class at a planted position changed"""
    bad = y.copy()
    p = pos[-1]
    bad[p] = 0.25 if not np.isfinite(y[p]) else NAN
    with pytest.raises(AssertionError):
        fn(bad)


# ------------------------------------------------------------------ separable
@pytest.mark.parametrize("plant", nf.PLANTS_SEPARABLE)
@pytest.mark.parametrize("n", [3, 1537])
def test_separable_reference(orc, n, plant):
    x, sj, q, lo, up, selected = nf.separable_data(n, 7700 + n)
    pos = nf.positions(n, [n // 2])
    qp, xp, sp = nf.plant(plant, q, x, sj, pos)
    for kind, form in nf.SEP_OPS:
        what = "%s %s n %d %s" % (kind, form, n, plant)
        box = nf.sep_box(form, lo, up, selected, n)
        y = nf.sep_oracle(orc, kind, box, qp, xp, sp)
        nf.sep_check(orc, kind, box, y, y.copy(), qp, xp, sp, what)
        if plant.startswith("nan"):                          # a definite answer: NaN at the plants (a box may clamp it away), nowhere else
            nans = np.flatnonzero(np.isnan(y)).tolist()
            assert nans == sorted(pos) if (form == "plain" and plant == "nan-q") else set(nans) <= set(pos), what
            _refuses(lambda b: nf.sep_check(orc, kind, box, b, y, qp, xp, sp, what), y, pos)
        sel = nf.sep_selected(box, n)
        with np.errstate(all="ignore"):
            v = (xp + sp) + y
            terms = [qp * y, y * y, nf.h_terms(kind, v[sel])]
        for t in terms:                                      # the input condition of item 4
            assert nf.magnitude(t) < nf.MAG_LIMIT, (what, nf.magnitude(t))
        # the class of h by the rule is the class of the reference's own psi(y) on the selected indices
        exp = orc.obj_plain(kind, y[sel], xp[sel], sp[sel], nf.SEP_LAM)
        assert nf.scalar_class(exp) == nf.sum_class(terms[2]), (what, exp)
        if plant == "none":
            assert all(nf.sum_class(t) == "finite" for t in terms)
        if plant == "large" and form == "plain":              # a large y does travel through [1] and [2]
            assert nf.magnitude(terms[0]) > 1e290 and nf.magnitude(terms[1]) > 1e290, what


# ------------------------------------------------------------------ groups
LAYOUTS = [("uniform", g) for g in (3, 16, 128, 300, 1024, 5000)] + [("csr_bound", 0), ("csr_over", 0), ("one", 1000), ("one", 20_001)]


@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["%s%s" % (k, a or "") for k, a in LAYOUTS])
def test_group_reference(orc, layout, binf):
    D = nf.GroupData(layout, binf)
    y_clean = D.oracle(orc, D.q, D.x, D.sj, y0=-777.0)
    assert np.isfinite(y_clean).all()
    pos, gz, gsh = D.plant_positions(arbiter, y_clean)
    if D.ng > 1:                                             # one plant in a group the prox zeroes, one in a group it shrinks
        zp = arbiter.zero_pattern(y_clean, D.x, D.sj, D.csr)
        assert zp[gz] and not zp[gsh] and gsh != 0
        assert any(D.csr[gz] <= p < D.csr[gz + 1] for p in pos) and any(D.csr[gsh] <= p < D.csr[gsh + 1] for p in pos)
    for plant in nf.PLANTS:
        what = "%s binf %d %s" % (layout, binf, plant)
        qp, xp, sp = nf.plant(plant, D.q, D.x, D.sj, pos)
        y = D.oracle(orc, qp, xp, sp, y0=-777.0)
        if plant.startswith("nan") or plant == "tiny" or not binf:
            nf.check_group(orc, arbiter, y, y.copy(), qp, xp, sp, D.lam, D.sigma, D.csr, D.delta if binf else None, what)
        if plant == "nan-q":                                 # the whole group NaN, the other groups finite
            gid = np.searchsorted(D.csr, np.arange(D.n), side="right") - 1
            inside = (np.arange(D.n) >= D.csr[0]) & (np.arange(D.n) < D.csr[-1])
            hit = np.unique(gid[[p for p in pos if inside[p]]])
            assert np.array_equal(np.isnan(y), inside & np.isin(gid, hit)), what
            _refuses(lambda b: nf.check_group(orc, arbiter, b, y, qp, xp, sp, D.lam, D.sigma, D.csr, D.delta if binf else None,
                                              what), y, [p for p in pos if inside[p]])
        if plant == "pinf-q" and not binf and D.offsets is None:
            assert int(np.isinf(y).sum()) == len(pos) and not np.isnan(y).any(), what   # one Inf per plant
        with np.errstate(all="ignore"):
            v = (xp + sp) + y
            terms = [qp * y, y * y, nf.group_terms(v, D.lam, D.starts, D.sizes)]
        for t in terms:
            assert nf.magnitude(t) < nf.MAG_LIMIT, (what, nf.magnitude(t))
        kw = dict(offsets=D.offsets) if D.offsets is not None else dict(gsize=D.gsize)
        exp = orc.obj_group_l2(y, xp, sp, D.lam, **kw)
        assert nf.scalar_class(exp) == nf.sum_class(terms[2]), (what, exp, nf.sum_class(terms[2]))


# ------------------------------------------------------------------ B2
@pytest.mark.parametrize("delta", [1.0, 1e6], ids=["active", "inactive"])
@pytest.mark.parametrize("n", [3, 1_000, 20_001])
def test_b2_reference(orc, n, delta):
    x, sj, q = nf.b2_data(n)
    pos = nf.positions(n, [n // 2])
    for plant in nf.PLANTS:
        what = "b2 n %d delta %g %s" % (n, delta, plant)
        qp, xp, sp = nf.plant(plant, q, x, sj, pos)
        with np.errstate(all="ignore"):
            y = orc.prox_l1_b2(qp, xp, sp, 1.0, 1.0, delta, 1.0)
        nf.check_b2(y, y.copy(), xp, what)
        if plant == "nan-q":                                 # NaN at the plants, finite elsewhere
            assert np.flatnonzero(np.isnan(y)).tolist() == sorted(pos), what
            _refuses(lambda b: nf.check_b2(b, y, xp, what), y, pos)
        if plant == "none":
            moved = y.copy()
            moved[n // 2] += 1e-9 * max(1.0, nf.nan_norm(y))
            with pytest.raises(AssertionError):
                nf.check_b2(moved, y, xp, what)
        with np.errstate(all="ignore"):
            v = (xp + sp) + y
            terms = [qp * y, y * y, np.abs(v)]
        for t in terms:
            assert nf.magnitude(t) < nf.MAG_LIMIT, (what, nf.magnitude(t))
        exp = orc.obj_plain("l1", y, xp, sp, 1.0)
        assert nf.scalar_class(exp) == nf.sum_class(terms[2]), (what, exp)
