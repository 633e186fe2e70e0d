"""GPU parity: the HIP path (through the C ABI, via the host mirror of the reference API) against the CPU
oracle on the same seeded inputs, the committed golden fixtures, and the reference's own test shapes.

Bars (BASELINE.json north_star):
  * ShiftedNormL1(Box), ShiftedNormL0(Box), ShiftedIndBallL0(BInf): BIT-EXACT (np.array_equal incl. signed zeros)
  * ShiftedRootNormLhalf(Box), ShiftedGroupNormL2(Binf): <= 1e-12 relative (LHALF_TOL / GROUP_TOL below)
"""
import numpy as np
import pytest

import arbiter  # tests/arbiter.py: the 1e-12 bar, and the binary128 adjudication of whatever fails it

pytestmark = pytest.mark.gpu

LHALF_TOL = 1e-12   # |y_gpu - y_ref| <= LHALF_TOL * max(|y_ref|, |x + s|, |q|)   (y = val - (x+s): scale of the operands)
GROUP_TOL = 1e-12   # |y_gpu - y_ref| <= GROUP_TOL * max(|y_ref_i|, |xk_i + sj_i|, ||S_group||_2)  (arbiter.group_scale)
# No test below accepts a difference above these bars on a fixed looser tolerance: elements / groups that exceed them go
# to the binary128 arbiter and must satisfy |y_gpu - y_q| <= 1e-12 scale + |y_oracle64 - y_q| (arbiter.py).


@pytest.fixture(scope="module")
def s():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.build()


def _data(n, seed, quant=None):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=n)
    sj = rng.uniform(-0.5, 0.5, size=n)
    q = rng.normal(size=n)
    if quant:
        x, sj, q = (np.round(v * quant) / quant for v in (x, sj, q))
    return x, sj, q


def _dev(*arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrs]


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def _same_or_both_nan(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.int64) == b.view(np.int64))))


SIZES = [0, 1, 2, 3, 63, 255, 1024, 2049, 10_000, 1_000_003]


# ------------------------------------------------------------------ unboxed separable
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", ["l1", "l0", "lhalf"])
def test_unboxed(s, orc, op, n):
    x, sj, q = _data(n, 100 + n)
    lam, sigma = 0.7, 1.3
    h = {"l1": s.NormL1, "l0": s.NormL0, "lhalf": s.RootNormLhalf}[op](lam)
    xd, sd, qd = _dev(x, sj, q)
    psi = s.shifted(s.shifted(h, xd), sd)
    y = s.prox(psi, qd, sigma).cpu().numpy()
    ref = getattr(orc, "prox_" + op)(q, x, sj, lam, sigma)
    if op == "lhalf":
        arbiter.check_lhalf(orc, y, ref, q, x, sj, lam, sigma)
    else:
        assert _bits_equal(y, ref)
    # once-shifted (sj = 0) too
    psi1 = s.shifted(h, xd)
    y1 = s.prox(psi1, qd, sigma).cpu().numpy()
    ref1 = getattr(orc, "prox_" + op)(q, x, np.zeros(n), lam, sigma)
    if op == "lhalf":
        arbiter.check_lhalf(orc, y1, ref1, q, x, np.zeros(n), lam, sigma)
    else:
        assert _bits_equal(y1, ref1)


def test_config1_l1_n1e4_nu1(s, orc):
    # BASELINE config 1: ShiftedNormL1 prox! on n = 10^4 fp64 random q/x/s, nu = 1.0
    x, sj, q = _data(10_000, 20250613)
    xd, sd, qd = _dev(x, sj, q)
    y = s.prox(s.shifted(s.shifted(s.NormL1(1.0), xd), sd), qd, 1.0).cpu().numpy()
    assert _bits_equal(y, orc.prox_l1(q, x, sj, 1.0, 1.0))


# ------------------------------------------------------------------ boxed separable
BOX = {"l1_box": "NormL1", "l0_box": "NormL0", "lhalf_box": "RootNormLhalf"}


def _check_box(orc, op, y, ref, x, sj, q, lam, sigma, lo, up, mask=None):
    if op == "lhalf_box":
        arbiter.check_lhalf(orc, y, ref, q, x, sj, lam, sigma, box=(lo, up), mask=mask, what=op)
    else:
        assert _bits_equal(y, ref)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", list(BOX))
def test_box_scalar_bounds(s, orc, op, n):
    x, sj, q = _data(n, 200 + n)
    lam, sigma, delta = 1.0, 1.0, 1.0
    h = getattr(s, BOX[op])(lam)
    xd, sd, qd = _dev(x, sj, q)
    psi = s.shifted(s.shifted(h, xd, delta, s.NormLinf(1.0)), sd)
    y = s.prox(psi, qd, sigma).cpu().numpy()
    ref = getattr(orc, "prox_" + op)(q, x, sj, lam, sigma, -delta, delta)
    _check_box(orc, op, y, ref, x, sj, q, lam, sigma, -delta, delta)


@pytest.mark.parametrize("n", [1, 2, 5, 1000, 65_537])
@pytest.mark.parametrize("op", list(BOX))
@pytest.mark.parametrize("form", ["vec_vec", "vec_scalar", "scalar_vec"])
def test_box_vector_bounds_and_mask(s, orc, op, n, form):
    rng = np.random.default_rng(300 + n)
    x, sj, q = _data(n, 301 + n)
    lam, sigma = 0.9, 0.8
    l = -1.0 - 0.1 * rng.random(n)
    u = 1.0 + 0.1 * rng.random(n)
    lo = l if form in ("vec_vec", "vec_scalar") else -1.05
    uo = u if form in ("vec_vec", "scalar_vec") else 1.05
    h = getattr(s, BOX[op])(lam)
    xd, sd, qd = _dev(x, sj, q)
    ld = _dev(lo)[0] if not np.isscalar(lo) else lo
    ud = _dev(uo)[0] if not np.isscalar(uo) else uo
    # all selected
    psi = s.shifted(s.shifted(h, xd, ld, ud), sd)
    y = s.prox(psi, qd, sigma).cpu().numpy()
    _check_box(orc, op, y, getattr(orc, "prox_" + op)(q, x, sj, lam, sigma, lo, uo), x, sj, q, lam, sigma, lo, uo)
    # selected = every other index (test/partial_prox.jl: 1:2:n) and an unsorted duplicated vector (test_allocs.jl:111)
    for selected in (range(0, n, 2), list(rng.integers(0, n, size=max(1, n // 2)))):
        mask = orc.mask_from_selected([i + 1 for i in selected], n)
        psi = s.shifted(s.shifted(h, xd, ld, ud, selected), sd)
        y = s.prox(psi, qd, sigma).cpu().numpy()
        _check_box(orc, op, y, getattr(orc, "prox_" + op)(q, x, sj, lam, sigma, lo, uo, mask=mask), x, sj, q, lam, sigma, lo, uo, mask)


@pytest.mark.parametrize("op", list(BOX))
def test_box_golden_and_testsbox_through_gpu(s, kats, op):
    import torch
    name = {"l1_box": "ShiftedNormL1Box", "l0_box": "ShiftedNormL0Box", "lhalf_box": "ShiftedRootNormLhalfBox"}[op]
    k = kats["box_golden"]  # test/runtests.jl:449-494
    x, q = _dev(np.array(k["x"]), np.array(k["q"]))
    psi = s.shifted(getattr(s, BOX[op])(k["lambda"]), x, k["delta"], s.NormLinf(1.0))
    y = s.prox(psi, q, k["sigma"]).cpu().numpy()
    np.testing.assert_allclose(y, k["expected"][name], rtol=k["rtol"], atol=0)
    assert float(np.max(np.abs(y))) <= k["delta"]
    t = kats["testsbox"]  # test/testsbox.jl:13-97
    c = t[name]
    for qi, xi, lam, sol in zip(c["q"], c["x"], c["lambda"], c["sol"]):
        xd, qd, sd = _dev(np.array([xi]), np.array([qi]), np.array([t["s"]]))
        ld, ud = _dev(np.array([t["l"]]), np.array([t["u"]]))
        psi = s.shifted(getattr(s, BOX[op])(lam), xd, ld, ud)
        omega = s.shifted(psi, sd)
        s.prox(omega, qd, t["sigma"])
        assert abs(float(omega.sol[0]) - sol) <= t["atol"]


def test_box_constructor_errors(s):
    x = _dev(np.zeros(3))[0]
    l, u = _dev(np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.5, 1.0]))
    for H in (s.NormL1, s.NormL0):
        with pytest.raises(ValueError, match="lower bound is greater"):
            s.shifted(H(1.0), x, l, u)  # shiftedNormL1Box.jl:33-35
        with pytest.raises(ValueError):
            s.shifted(H(1.0), x, 1.0, -1.0)
    s.shifted(s.RootNormLhalf(1.0), x, l, u)  # no check in shiftedRootNormLhalfBox.jl:22-44


# ------------------------------------------------------------------ aliasing, views, state updates
def test_aliasing_and_views(s, orc):
    import torch
    n = 4099
    x, sj, q = _data(n, 7)
    for op, h in (("l1_box", s.NormL1(1.0)), ("l0_box", s.NormL0(1.0))):
        xd, sd, qd = _dev(x, sj, q)
        psi = s.shifted(s.shifted(h, xd, 1.0, s.NormLinf(1.0)), sd)
        ref = getattr(orc, "prox_" + op)(q, x, sj, 1.0, 1.0, -1.0, 1.0)
        out = s.prox_bang(qd, psi, qd, 1.0)  # y === q  (test/test_allocs.jl:108-113)
        assert out is qd and _bits_equal(qd.cpu().numpy(), ref)
    # ShiftedNormL1 with y === q reproduces the reference's two-pass body: -(xk) - sj
    xd, sd, qd = _dev(x, sj, q)
    psi = s.shifted(s.shifted(s.NormL1(1.0), xd), sd)
    s.prox_bang(qd, psi, qd, 1.0)
    assert _bits_equal(qd.cpu().numpy(), (-x) - sj)
    # 8-byte-aligned views (odd offset) take the scalar kernels
    big = _dev(np.concatenate([[0.0], x]), np.concatenate([[0.0], sj]), np.concatenate([[0.0], q]))
    xv, sv, qv = (b[1:] for b in big)
    psi = s.shifted(s.shifted(s.NormL1(1.0), xv, 1.0, s.NormLinf(1.0)), sv)
    y = torch.empty(n + 1, dtype=torch.float64, device="cuda:0")[1:]
    s.prox_bang(y, psi, qv, 1.0)
    assert _bits_equal(y.cpu().numpy(), orc.prox_l1_box(q, x, sj, 1.0, 1.0, -1.0, 1.0))
    for bad in (qv.float(), qv.cpu(), torch.stack([qv, qv], 1)[:, 0]):
        with pytest.raises(TypeError):
            s.prox_bang(y, psi, bad, 1.0)
    with pytest.raises(IndexError):
        s.prox_bang(y, psi, qv[:-1], 1.0)


def test_shift_and_bounds_updates(s, orc):
    n = 1000
    x, sj, q = _data(n, 8)
    x2, sj2, _ = _data(n, 9)
    xd, sd, qd, x2d, s2d = _dev(x, sj, q, x2, sj2)
    psi = s.shifted(s.NormL1(1.0), xd, 0.5, s.NormLinf(1.0))
    om = s.shifted(psi, sd)
    assert om.xk is psi.xk is xd and om.sj is sd and bool((psi.sj == 0).all())  # aliasing (runtests.jl:183-185)
    s.shift_bang(psi, x2d)  # writes INTO the caller's xd
    assert _bits_equal(xd.cpu().numpy(), x2)
    s.shift_bang(om, s2d)
    assert _bits_equal(sd.cpu().numpy(), sj2)
    s.set_radius_bang(om, 0.25)
    assert om.l == -0.25 and om.u == 0.25
    y = s.prox(om, qd, 0.5).cpu().numpy()
    assert _bits_equal(y, orc.prox_l1_box(q, x2, sj2, 1.0, 0.5, -0.25, 0.25))
    l, u = -np.abs(x) - 0.1, np.abs(sj) + 0.1
    ld, ud = _dev(l, u)
    s.set_bounds_bang(om, ld, ud)
    assert om.l is ld  # a vector replaces a stored scalar by reference
    y = s.prox(om, qd, 0.5).cpu().numpy()
    assert _bits_equal(y, orc.prox_l1_box(q, x2, sj2, 1.0, 0.5, l, u))
    l2d = _dev(l - 1.0)[0]
    s.set_bounds_bang(om, l2d, ud)
    assert om.l is ld and _bits_equal(ld.cpu().numpy(), l - 1.0)  # vector into vector: copied in place
    assert om.λ == 1.0
    bi = s.shifted(s.IndBallL0(3), xd, 0.5, s.NormLinf(1.0))
    s.set_radius_bang(bi, 2.0)
    assert bi.Δ == 2.0 and bi.r == 3


# ------------------------------------------------------------------ top-r selection
@pytest.mark.parametrize("n", [1, 2, 5, 64, 1000, 4097, 300_001])
@pytest.mark.parametrize("quant", [None, 8])
def test_indball_l0(s, orc, n, quant):
    x, sj, q = _data(n, 400 + n, quant)
    xd, sd, qd = _dev(x, sj, q)
    for r in sorted({1, 2, max(1, n // 100), max(1, n // 3), max(1, n - 1), n, n + 7}):
        psi = s.shifted(s.shifted(s.IndBallL0(r), xd), sd)
        y = s.prox(psi, qd, 1.0).cpu().numpy()
        assert _bits_equal(y, orc.prox_indball_l0(q, x, sj, r)), (n, r, quant)
        psi = s.shifted(s.shifted(s.IndBallL0(r), xd, 0.6, s.NormLinf(1.0)), sd)
        y = s.prox(psi, qd, 1.0).cpu().numpy()
        assert _bits_equal(y, orc.prox_indball_l0_binf(q, x, sj, r, 0.6)), (n, r, quant)


def test_indball_l0_small_n_both_kernels(s, orc):
    """n <= 8192 runs in one workgroup (k_sel_small); key 6 = 0 sends the same sizes through the kernel larger vectors use, the
    register-resident one-launch select -- and, with the resident grid capped at 2 workgroups (key 8), through the form that
    parks v in y.  All three must give the oracle's bits, ties and NaN included."""
    L = s._lib.load()
    rng = np.random.default_rng(6)
    try:
        for mode, coop in ((1, 0), (0, 0), (0, 2)):
            L.spx_ctx_set_tuning(s.context("cuda:0"), 6, mode)
            L.spx_ctx_set_tuning(s.context("cuda:0"), 8, coop)
            for n in (1, 2, 63, 1024, 1025, 5000, 8192, 8193, 65536):
                x, sj, q = _data(n, 700 + n, 8)
                if n >= 63:
                    q[rng.choice(n, size=3, replace=False)] = np.nan
                    q[rng.choice(n, size=2, replace=False)] = np.inf
                xd, sd, qd = _dev(x, sj, q)
                for r in sorted({1, 2, max(1, n // 7), max(1, n - 1), n, n + 3}):
                    with np.errstate(all="ignore"):
                        ref = orc.prox_indball_l0_binf(q, x, sj, r, 0.6)
                    y = s.prox(s.shifted(s.shifted(s.IndBallL0(r), xd, 0.6, s.NormLinf(1.0)), sd), qd, 1.0).cpu().numpy()
                    assert _same_or_both_nan(y, ref), (mode, n, r)
            # constant magnitude: the key span is zero, the index digits decide alone
            n = 3000
            q = np.where(np.arange(n) % 3 == 0, -2.5, 2.5); x = np.zeros(n); sj = np.zeros(n)
            xd, sd, qd = _dev(x, sj, q)
            for r in (1, 1500, 2999):
                y = s.prox(s.shifted(s.shifted(s.IndBallL0(r), xd), sd), qd, 1.0).cpu().numpy()
                assert _bits_equal(y, orc.prox_indball_l0(q, x, sj, r)), (mode, r)
    finally:
        L.spx_ctx_set_tuning(s.context("cuda:0"), 6, 1)
        L.spx_ctx_set_tuning(s.context("cuda:0"), 8, 0)


def test_indball_l0_ties_and_kats(s, orc, kats):
    T = kats["derived"]["tiebreak"]
    x, sj, q = (np.array(T[k]) for k in ("x", "s", "q"))
    xd, sd, qd = _dev(x, sj, q)
    for r in (2, 3, 4):
        y = s.prox(s.shifted(s.shifted(s.IndBallL0(r), xd), sd), qd, 1.0).cpu().numpy()
        assert _bits_equal(y, np.array(T["r%d" % r]))
    # all |v| equal: pure index tie-break over many index digits
    n = 70_001
    x, sj = np.zeros(n), np.zeros(n)
    q = np.where(np.arange(n) % 2 == 0, 1.5, -1.5)
    xd, sd, qd = _dev(x, sj, q)
    for r in (1, 4096, 4097, 33_333, n - 1):
        y = s.prox(s.shifted(s.shifted(s.IndBallL0(r), xd), sd), qd, 1.0).cpu().numpy()
        assert _bits_equal(y, orc.prox_indball_l0(q, x, sj, r))
        assert np.count_nonzero(y) == r and np.all(y[r:] == 0)
    # y === q is allowed (y is the reference's scratch too)
    x, sj, q = _data(5000, 11, 16)
    xd, sd, qd = _dev(x, sj, q)
    s.prox_bang(qd, s.shifted(s.shifted(s.IndBallL0(123), xd), sd), qd, 1.0)
    assert _bits_equal(qd.cpu().numpy(), orc.prox_indball_l0(q, x, sj, 123))


def test_indball_l0_nan_inf(s, orc):
    """Non-finite entries: the reference's sortperm compares with isless, so a NaN is the largest magnitude, all NaNs
    tie (ascending index decides) and +-Inf come next.  Kept-index set and values (NaN-aware) must match the oracle."""
    rng = np.random.default_rng(12)
    for n in (1000, (1 << 22) + 77):           # full-vector radix select / sample-predicted path
        x, sj, q = _data(n, 13)
        nan_at = rng.choice(n, size=9, replace=False)
        q[nan_at[:5]] = np.nan
        q[nan_at[5:7]] = -np.nan                # sign / payload must not matter
        x[nan_at[7:]] = np.nan
        inf_at = rng.choice(np.setdiff1d(np.arange(n), nan_at), size=6, replace=False)
        q[inf_at[:3]] = np.inf
        q[inf_at[3:]] = -np.inf
        xd, sd, qd = _dev(x, sj, q)
        with np.errstate(all="ignore"):
            top = orc.TopR(q, x, sj)
        L = s._lib.load(); ctx = s.context("cuda:0")
        try:
            for form in ((2, 1) if n > 1000 else (1,)):   # the pipeline (key 11 = 2 at this size since round 4) and the default form
                s._lib.check(L.spx_ctx_set_tuning(ctx, 11, form))
                for r in (1, 4, 9, 12, 15, 16, n // 7):
                    with np.errstate(all="ignore"):
                        ref = top.prox(r, 0.6)
                        ref0 = top.prox(r)
                    y = s.prox(s.shifted(s.shifted(s.IndBallL0(r), xd, 0.6, s.NormLinf(1.0)), sd), qd, 1.0).cpu().numpy()
                    assert _same_or_both_nan(y, ref), (n, r, form)
                    y0 = s.prox(s.shifted(s.shifted(s.IndBallL0(r), xd), sd), qd, 1.0).cpu().numpy()
                    assert _same_or_both_nan(y0, ref0), (n, r, form)
        finally:
            s._lib.check(L.spx_ctx_set_tuning(ctx, 11, 1))


@pytest.mark.parametrize("kind", ["scaled", "cauchy", "concentrated"])
def test_indball_l0_ranks_and_scales(s, orc, kind):
    """Sample-predicted path (n >= 2^20) over the whole range of r and over data whose r-th magnitude sits next to an
    exponent boundary, has heavy tails, or is packed into a 1e-9 relative range: the candidate digits follow the
    band's span (SelState::base), so none of these may change the kept set (tools/sweep_topr.py times them at n = 1e8)."""
    n = (1 << 22) + 4321
    rng = np.random.default_rng({"scaled": 1, "cauchy": 2, "concentrated": 3}[kind])
    x, sj = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n)
    if kind == "scaled":
        q = 1.37 * rng.normal(size=n)
    elif kind == "cauchy":
        q = rng.standard_cauchy(size=n)
    else:
        x, sj = np.zeros(n), np.zeros(n)
        q = (1.0 + 1e-9 * rng.normal(size=n)) * rng.choice([-1.0, 1.0], size=n)
    xd, sd, qd = _dev(x, sj, q)
    top = orc.TopR(q, x, sj)   # (the reference's sortperm once, every r from it)
    L = s._lib.load(); ctx = s.context("cuda:0")
    try:
        for form in (2, 1):   # the sample-predicted pipeline (the subject; key 11 = 2 at this size since round 4), the default form
            s._lib.check(L.spx_ctx_set_tuning(ctx, 11, form))
            for r in (1, 50, 5000, n // 100, n // 2, n - 5000):
                ref = top.prox(r, 0.9)
                y = s.prox(s.shifted(s.shifted(s.IndBallL0(r), xd, 0.9, s.NormLinf(1.0)), sd), qd, 1.0).cpu().numpy()
                assert _bits_equal(y, ref), (kind, r, form)
            r = n // 37  # aliased form (y === q)
            qa = qd.clone()
            s.prox_bang(qa, s.shifted(s.shifted(s.IndBallL0(r), xd), sd), qa, 1.0)
            assert _bits_equal(qa.cpu().numpy(), top.prox(r)), (kind, form)
    finally:
        s._lib.check(L.spx_ctx_set_tuning(ctx, 11, 1))


@pytest.mark.parametrize("n,lds", [((1 << 20) - 1, 1), (1 << 20, 1), ((1 << 20) + 1, 1), ((1 << 20) + 3001, 1), ((1 << 21) - 1, 1),
                                   (1 << 21, 0), ((1 << 21) + 1, 0), ((1 << 21) + 3001, 0), ((1 << 21) + 3001, 1),
                                   ((1 << 22) - 1, 1), (1 << 22, 1), ((1 << 22) + 1, 1), ((1 << 22) + 3001, 1),
                                   ((1 << 22) + 1, 2), ((1 << 22) + 3001, 2), (5_000_003, 1),
                                   (6 * (1 << 20) - 1, 1), (6 * (1 << 20), 1), (6 * (1 << 20) + 1, 1), (6 * (1 << 20) + 1, 2)])
def test_indball_l0_at_the_fast_path_threshold(s, orc, n, lds):
    """Either side of the sizes at which the forms hand over: v in registers -> v in LDS (k_sel_lds, above 2^20) -> 16 elements
    per lane in LDS + 8 in registers (k_sel_lds<.., REGX>, above 2^22 = what 256 resident workgroups hold in LDS; round 4) -> the
    sample-predicted pipeline (above 6 Mi); key 11 = 2 keeps the pipeline from 2^22 on; with the LDS forms switched off (tuning
    key 11 = 0) the pipeline takes over from the register form at 2^21 (SPX_SEL_REG_MAX_LOG2), as in round 2.  Lattice data
    (ties), all r regimes."""
    L = s._lib.load()
    ctx = s.context("cuda:0")
    rng = np.random.default_rng(n)
    x, sj = np.round(rng.normal(size=n) * 16) / 16, np.round(rng.uniform(-0.5, 0.5, size=n) * 16) / 16
    q = np.round(rng.normal(size=n) * 16) / 16
    xd, sd, qd = _dev(x, sj, q)
    s._lib.check(L.spx_ctx_set_tuning(ctx, 11, lds))
    try:
        top = orc.TopR(q, x, sj)   # (the reference's sortperm once per input, every r from it)
        for r in (1, 3, 777, n // 100, n // 3, n - 2):
            y = s.prox(s.shifted(s.shifted(s.IndBallL0(r), xd, 0.8, s.NormLinf(1.0)), sd), qd, 1.0).cpu().numpy()
            assert _bits_equal(y, top.prox(r, 0.8)), (n, r)
        if n > (1 << 22):   # y === xk: the form with register slots re-reads xk and sj in its storing phase
            xa = xd.clone()
            s.prox_bang(xa, s.shifted(s.shifted(s.IndBallL0(n // 7), xa, 0.8, s.NormLinf(1.0)), sd), qd, 1.0)
            assert _bits_equal(xa.cpu().numpy(), top.prox(n // 7, 0.8)), n
        s.prox_bang(qd, s.shifted(s.shifted(s.IndBallL0(n // 50), xd), sd), qd, 1.0)      # aliased form
        assert _bits_equal(qd.cpu().numpy(), top.prox(n // 50)), n
    finally:
        s._lib.check(L.spx_ctx_set_tuning(ctx, 11, 1))


def test_indball_l0_misaligned_views_fast_path(s, orc):
    """All four vectors 8 bytes off a 16-byte boundary (a view from an odd element on): the sample-predicted path
    runs on the aligned rest and element 0 rides with wave 0.  Element 0 as the largest / a tied / a dropped entry,
    odd and even n, disjoint and aliased y; a mixed alignment takes the full-vector path."""
    import torch
    for n in ((1 << 22) + 2, (1 << 22) + 5):
        rng = np.random.default_rng(n)
        x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), np.round(rng.normal(size=n) * 32) / 32
        for head in (100.0, 0.0, None):
            if head is not None:
                x[0], sj[0], q[0] = 0.0, 0.0, head
            else:
                x[0], sj[0], q[0] = x[7], sj[7], q[7]            # ties with element 7: the lower index wins
            mk = lambda a: torch.cat([torch.zeros(1, dtype=torch.float64), torch.from_numpy(a)]).cuda()[1:]
            xd, sd, qd = mk(x), mk(sj), mk(q)
            assert all(t.data_ptr() % 16 == 8 for t in (xd, sd, qd))
            top = orc.TopR(q, x, sj)   # (the reference's sortperm once per input, every r from it)
            for r in (1, n // 50, n - 3):
                ref = top.prox(r, 0.7)
                psi = s.shifted(s.shifted(s.IndBallL0(r), xd, 0.7, s.NormLinf(1.0)), sd)
                yv = mk(np.zeros(n))
                s.prox_bang(yv, psi, qd, 1.0)
                assert _bits_equal(yv.cpu().numpy(), ref), (n, head, r)
                ya = torch.from_numpy(np.zeros(n)).cuda()        # y aligned, inputs not: full-vector path
                s.prox_bang(ya, psi, qd, 1.0)
                assert _bits_equal(ya.cpu().numpy(), ref), (n, head, r)
            q2 = qd.clone()
            q2v = mk(q2.cpu().numpy())
            s.prox_bang(q2v, s.shifted(s.shifted(s.IndBallL0(n // 9), xd), sd), q2v, 1.0)   # aliased
            assert _bits_equal(q2v.cpu().numpy(), top.prox(n // 9)), (n, head)


# ------------------------------------------------------------------ groups
def _group_check(y, ref, q, x, sj, offsets):
    """The plain bar, no adjudication: every element within GROUP_TOL of the Float64 oracle."""
    scale = arbiter.group_scale(ref, q, x, sj, offsets)
    bad = np.abs(y - ref) > GROUP_TOL * np.maximum(scale, 1e-300)
    assert not bad.any(), (int(bad.sum()), float(np.max(np.abs(y - ref))))


def _binf_check(orc, y, ref, q, x, sj, lam, sigma, delta, offsets, what=""):
    """ShiftedGroupNormL2Binf in the regimes where the reference's formula is ill-conditioned (sigma*lambda >> ||S||, roots
    next to the pole of step(n), reversed brackets): the plain bar first, the binary128 arbiter for every group that fails
    it (arbiter.check_group).  Also: NaN patterns equal, and a group the oracle zeroes that the GPU does not (or vice
    versa) is a failure unless the arbiter sides with the GPU -- such a group fails the plain bar by construction."""
    assert np.array_equal(np.isnan(y), np.isnan(ref)), what
    fin = np.isfinite(ref)
    if not fin.all():   # non-finite results (overflowing data): compared as patterns only
        assert np.array_equal(np.isfinite(y), fin), what
        y, ref = np.where(fin, y, 0.0), np.where(fin, ref, 0.0)
    return arbiter.check_group(orc, y, ref, q, x, sj, lam, sigma, offsets, delta=delta, what=what)


@pytest.mark.parametrize("gsize", [64, 128, 256, 512, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 13, 16, 17, 33, 66, 100, 130, 250, 257,
                                   383, 386, 510, 511, 513, 1024, 2048, 2049, 3000, 4096, 4097, 8200,
                                   9, 32, 65, 129, 384, 385])  # (the last six: just above / at the tile tables' bounds)
@pytest.mark.parametrize("binf", [False, True])
@pytest.mark.parametrize("misaligned", [False, True])
def test_group_uniform(s, orc, gsize, binf, misaligned):
    # every tile of the register kernel (from one lane per group of two on), full and partly filled, even (16-byte pairs) and
    # odd (8-byte loads) sizes;
    # misaligned: all four vectors start 8 bytes off a 16-byte boundary
    if misaligned and gsize not in (2, 4, 10, 64, 100, 128, 386, 512, 3000):
        pytest.skip("misaligned views are checked on a subset")
    ng = 513 if gsize <= 513 else 19  # > 512: LDS-resident group per workgroup (<= 8192), general kernel above
    n = ng * gsize
    x, sj, q = _data(n, 500 + gsize)
    lam = np.random.default_rng(gsize).uniform(0.5, 1.5, size=ng)
    sigma, delta = 1.0, 1.0
    if misaligned:
        import torch
        xd, sd, qd = (torch.cat([torch.zeros(1, dtype=torch.float64), torch.from_numpy(a)]).cuda()[1:] for a in (x, sj, q))
        assert xd.data_ptr() % 16 == 8
    else:
        xd, sd, qd = _dev(x, sj, q)
    h = s.GroupNormL2.uniform(lam.tolist(), gsize) if gsize % 2 else \
        s.GroupNormL2(lam.tolist(), [range(i, i + gsize) for i in range(0, n, gsize)])
    if binf:
        psi = s.shifted(s.shifted(h, xd, delta, s.NormLinf(1.0)), sd)
        ref = orc.prox_group_l2_binf(q, x, sj, lam, sigma, delta, gsize=gsize)
    else:
        psi = s.shifted(s.shifted(h, xd), sd)
        ref = orc.prox_group_l2(q, x, sj, lam, sigma, gsize=gsize)
    y = s.prox(psi, qd, sigma).cpu().numpy()
    _group_check(y, ref, q, x, sj, list(range(0, n + 1, gsize)))


@pytest.mark.parametrize("binf", [False, True])
def test_group_ragged_and_single(s, orc, binf):
    rng = np.random.default_rng(77)
    sizes = [1, 5, 64, 129, 1000, 2, 4096, 33]
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    n = int(offsets[-1])
    x, sj, q = _data(n, 78)
    lam = rng.uniform(0.2, 2.0, size=len(sizes))
    xd, sd, qd = _dev(x, sj, q)
    groups = [range(int(a), int(b)) for a, b in zip(offsets[:-1], offsets[1:])]
    for sigma, delta in ((1.0, 1.0), (0.3, 0.2), (2.5, 5.0)):
        if binf:
            psi = s.shifted(s.shifted(s.GroupNormL2(lam.tolist(), groups), xd, delta, s.NormLinf(1.0)), sd)
            ref = orc.prox_group_l2_binf(q, x, sj, lam, sigma, delta, offsets=offsets)
        else:
            psi = s.shifted(s.shifted(s.GroupNormL2(lam.tolist(), groups), xd), sd)
            ref = orc.prox_group_l2(q, x, sj, lam, sigma, offsets=offsets)
        y = s.prox(psi, qd, sigma).cpu().numpy()
        _group_check(y, ref, q, x, sj, list(offsets))
    # NormL2 -> one group [:]  (shiftedGroupNormL2.jl:34-35)
    if binf:
        psi = s.shifted(s.NormL2(0.8), xd, 0.7, s.NormLinf(1.0))
        ref = orc.prox_group_l2_binf(q, x, np.zeros(n), [0.8], 1.1, 0.7, offsets=[0, n])
    else:
        psi = s.shifted(s.NormL2(0.8), xd)
        ref = orc.prox_group_l2(q, x, np.zeros(n), [0.8], 1.1, offsets=[0, n])
    y = s.prox(psi, qd, 1.1).cpu().numpy()
    _group_check(y, ref, q, x, np.zeros(n), [0, n])


@pytest.mark.parametrize("binf", [False, True])
@pytest.mark.parametrize("layout", ["interleaved", "permuted_big", "overlap_partial", "one_huge", "with_empty"])
def test_group_gather_index_sets(s, orc, binf, layout):
    """Groups as arbitrary index vectors (idx::Vector{Vector{Int}}, src/groupNormL2.jl:30-31): literal reference
    semantics incl. overlapping groups (last group wins) and indices in no group (y on entry survives)."""
    rng = np.random.default_rng({"interleaved": 1, "permuted_big": 2, "overlap_partial": 3, "one_huge": 4,
                                 "with_empty": 5}[layout])
    if layout == "interleaved":          # v = [[0, 2, 4, ...], [1, 3, 5, ...]]
        n = 2000
        groups = [list(range(0, n, 2)), list(range(1, n, 2))]
    elif layout == "permuted_big":       # a random partition into 3000 groups of mixed sizes
        n = 200_000
        perm = rng.permutation(n)
        cuts = np.sort(rng.choice(np.arange(1, n), size=2999, replace=False))
        groups = [g.tolist() for g in np.split(perm, cuts)]
    elif layout == "overlap_partial":    # overlapping groups, a repeated index, indices in no group
        n = 5000
        groups = [rng.choice(n // 2, size=300, replace=False).tolist() for _ in range(40)]
        groups[3] = groups[3] + groups[3][:5]
    elif layout == "one_huge":           # workgroup-per-group kernel
        n = 30_000
        groups = [rng.permutation(n)[:25_000].tolist(), [7, 3]]
    else:                                # an empty group among others
        n = 300
        groups = [list(range(0, 100)), [], list(range(299, 99, -1))]
    x, sj, q = _data(n, 600 + len(groups))
    lam = rng.uniform(0.3, 1.5, size=len(groups))
    y0 = rng.normal(size=n)
    sigma, delta = 0.9, 0.8
    xd, sd, qd, yd = _dev(x, sj, q, y0)
    h = s.GroupNormL2(lam.tolist(), groups)
    if binf:
        psi = s.shifted(s.shifted(h, xd, delta, s.NormLinf(1.0)), sd)
        ref = orc.prox_group_l2_idx(q, x, sj, lam, sigma, groups, delta=delta, y0=y0)
    else:
        psi = s.shifted(s.shifted(h, xd), sd)
        ref = orc.prox_group_l2_idx(q, x, sj, lam, sigma, groups, y0=y0)
    assert psi._layout.index is not None
    y = s.prox_bang(yd, psi, qd, sigma).cpu().numpy()
    S = (q + x) + sj
    scale = np.abs(ref).copy()
    for g in groups:
        if len(g):
            scale[g] = np.maximum(scale[g], np.linalg.norm(S[g]))
    covered = np.zeros(n, dtype=bool)
    for g in groups:
        covered[g] = True
    bad = np.abs(y - ref) > GROUP_TOL * np.maximum(scale, 1e-300)
    assert not bad.any(), (int(bad.sum()), float(np.max(np.abs(y - ref))))
    assert _bits_equal(y[~covered], ref[~covered])            # untouched / shift-only entries are exact
    # y === q
    q2 = qd.clone()
    s.prox_bang(q2, psi, q2, sigma)
    ref2 = orc.prox_group_l2_idx(q, x, sj, lam, sigma, groups, delta=delta if binf else None, y0=q)
    bad = np.abs(q2.cpu().numpy() - ref2) > GROUP_TOL * np.maximum(scale, 1e-300)
    assert not bad.any()
    # psi(y) on the same index sets
    val = psi(_dev(ref * 0.5)[0])
    exp = orc.obj_group_l2_idx(ref * 0.5, x, sj, lam, groups, delta=delta if binf else None)
    assert (val == exp) or abs(val - exp) <= 1e-12 * abs(exp)
    # host-pointer form: same kernels
    hy = y0.copy()
    psi_h = s.shifted(s.shifted(h, x, delta, s.NormLinf(1.0)), sj) if binf else s.shifted(s.shifted(h, x), sj)
    s.prox_bang(hy, psi_h, q, sigma)
    assert _bits_equal(hy, y)


def test_group_l2_csr_partial_cover(s, orc):
    """Consecutive ranges that do not span 0:n: ShiftedGroupNormL2 subtracts the shift at every index
    (src/shiftedGroupNormL2.jl:77), the Binf form only inside the groups (src/shiftedGroupNormL2Binf.jl:116)."""
    n = 1000
    x, sj, q = _data(n, 5)
    y0 = np.random.default_rng(6).normal(size=n)
    groups = [range(100, 300), range(300, 650), range(650, 900)]
    lam = [0.5, 1.0, 0.7]
    xd, sd, qd = _dev(x, sj, q)
    h = s.GroupNormL2(lam, groups)
    for binf in (False, True):
        psi = s.shifted(s.shifted(h, xd, 0.8, s.NormLinf(1.0)), sd) if binf else s.shifted(s.shifted(h, xd), sd)
        assert psi._layout.index is None and psi._layout.offsets is not None
        y = s.prox_bang(_dev(y0)[0], psi, qd, 0.9).cpu().numpy()
        ref = orc.prox_group_l2_idx(q, x, sj, lam, 0.9, [list(g) for g in groups], delta=0.8 if binf else None, y0=y0)
        np.testing.assert_allclose(y, ref, rtol=0, atol=1e-12)
        out = np.r_[0:100, 900:n]
        assert _bits_equal(y[out], ref[out])
        # objective: an infeasible entry OUTSIDE every group still makes the Binf value +Inf
        yy = np.zeros(n)
        yy[5] = 10.0
        val = psi(_dev(yy)[0])
        exp = orc.obj_group_l2_idx(yy, x, sj, lam, [list(g) for g in groups], delta=0.8 if binf else None)
        assert (val == exp) or abs(val - exp) <= 1e-12 * abs(exp)


@pytest.mark.parametrize("binf", [False, True])
@pytest.mark.parametrize("maxsize", [7, 32, 100, 128, 300, 512, 1500, 4096])
def test_group_ragged_bounded_sizes(s, orc, binf, maxsize):
    """Ragged consecutive groups with a size bound: CSR offsets + the bound select the register-tile kernels (bound <= 512:
    8-byte loads, per-group size) or the LDS-resident kernel (bound <= 2048 / 4096); a wrong (too small) bound still gives
    the right answer."""
    import ctypes
    import torch
    rng = np.random.default_rng(maxsize)
    sizes = rng.integers(1, maxsize + 1, size=700 if maxsize <= 512 else 60)
    sizes[:3] = (maxsize, 1, maxsize)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    n = int(offsets[-1])
    x, sj, q = _data(n, 9100 + maxsize)
    lam = rng.uniform(0.2, 2.0, size=sizes.size)
    xd, sd, qd = _dev(x, sj, q)
    groups = [range(int(a), int(b)) for a, b in zip(offsets[:-1], offsets[1:])]
    h = s.GroupNormL2(lam.tolist(), groups)
    sigma, delta = 0.8, 0.9
    if binf:
        psi = s.shifted(s.shifted(h, xd, delta, s.NormLinf(1.0)), sd)
        ref = orc.prox_group_l2_binf(q, x, sj, lam, sigma, delta, offsets=offsets)
    else:
        psi = s.shifted(s.shifted(h, xd), sd)
        ref = orc.prox_group_l2(q, x, sj, lam, sigma, offsets=offsets)
    assert psi._layout.offsets is not None and psi._layout.group_size == maxsize
    y = s.prox(psi, qd, sigma).cpu().numpy()
    _group_check(y, ref, q, x, sj, list(offsets))
    # y === q
    q2 = qd.clone()
    s.prox_bang(q2, psi, q2, sigma)
    _group_check(q2.cpu().numpy(), ref, q, x, sj, list(offsets))
    # a bound that is too small: the oversize groups are deferred to the general kernel, the result is the same
    L, ctx = s._lib.load(), s.context("cuda:0")
    lay = psi._layout
    yy = torch.full_like(qd, float("nan"))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    small = max(1, maxsize // 2)
    if binf:
        s._lib.check(L.spx_prox_group_l2_binf(ctx, p(yy), p(qd), p(xd), p(sd), n, p(lay.offsets), small, lay.ngroups,
                                              p(lay.lam), sigma, delta))
    else:
        s._lib.check(L.spx_prox_group_l2(ctx, p(yy), p(qd), p(xd), p(sd), n, p(lay.offsets), small, lay.ngroups, p(lay.lam),
                                         sigma))
    _group_check(yy.cpu().numpy(), ref, q, x, sj, list(offsets))


@pytest.mark.parametrize("binf", [False, True])
@pytest.mark.parametrize("maxsize", [40, 190, 512])
def test_group_ragged_many_groups(s, orc, binf, maxsize):
    """66 000 ragged groups with a size bound through the C entry points: the exact bound and one that is too small (a
    third of the groups then exceed their tile and go to the deferred list); offsets that start after 0 and end before n
    (plain form: the uncovered entries still get y - (xk + sj), Binf: untouched).
    (Tried on this layout: binning the groups by size class so that each runs on the smallest tile that holds it -- the
    extra launches and the lost streaming order cost more than the padding they save, 1.24 -> 1.56 ms at 1e6 groups of
    64..192; dropped.)"""
    import ctypes
    import torch
    rng = np.random.default_rng(1000 + maxsize)
    ng = 66_000
    sizes = rng.integers(0 if maxsize == 40 else 1, maxsize + 1, size=ng)      # (an empty group or two at maxsize 40)
    sizes[:3] = (maxsize, 1, maxsize)
    lead, trail = 5, 7
    offsets = lead + np.concatenate([[0], np.cumsum(sizes)])
    n = int(offsets[-1]) + trail
    x, sj, q = _data(n, 9300 + maxsize)
    lam = rng.uniform(0.2, 2.0, size=ng)
    xd, sd, qd = _dev(x, sj, q)
    offd = torch.from_numpy(offsets.astype(np.int64)).cuda()
    lamd = torch.from_numpy(lam).cuda()
    sigma, delta = 0.8, 0.9
    y0 = np.full(n, 123.0)
    if binf:
        ref = orc.prox_group_l2_binf(q, x, sj, lam, sigma, delta, offsets=offsets)
        ref[:lead] = y0[:lead]; ref[n - trail:] = y0[n - trail:]               # entries in no group keep y on entry
    else:
        ref = orc.prox_group_l2(q, x, sj, lam, sigma, offsets=offsets)
        ref[:lead] = y0[:lead] - (x[:lead] + sj[:lead]); ref[n - trail:] = y0[n - trail:] - (x[n - trail:] + sj[n - trail:])
    L, ctx = s._lib.load(), s.context("cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for bound in (maxsize, max(1, maxsize // 3)):
        yy = torch.from_numpy(y0.copy()).cuda()
        if binf:
            s._lib.check(L.spx_prox_group_l2_binf(ctx, p(yy), p(qd), p(xd), p(sd), n, p(offd), bound, ng, p(lamd), sigma, delta))
        else:
            s._lib.check(L.spx_prox_group_l2(ctx, p(yy), p(qd), p(xd), p(sd), n, p(offd), bound, ng, p(lamd), sigma))
        yh = yy.cpu().numpy()
        assert np.array_equal(yh[:lead], ref[:lead]) and np.array_equal(yh[n - trail:], ref[n - trail:]), bound
        _group_check(yh[lead:n - trail], ref[lead:n - trail], q[lead:n - trail], x[lead:n - trail], sj[lead:n - trail],
                     list(offsets - lead))


def test_group_binf_goldens_and_edge_branches(s, orc, kats):
    for name in ("group_l2_binf_single", "group_l2_binf_two"):  # test/runtests.jl:587-606, 658-705
        k = kats[name]
        x, q = _dev(np.array(k["x"]), np.array(k["q"]))
        off = k["offsets"]
        h = s.GroupNormL2(k["lambda"], [range(a, b) for a, b in zip(off[:-1], off[1:])])
        y = s.prox(s.shifted(h, x, k["delta"], s.NormLinf(1.0)), q, k["sigma"]).cpu().numpy()
        np.testing.assert_allclose(y, k["expected"], rtol=k["rtol"], atol=0)
        # explicit index vectors as in the reference test (`v = [collect(1:3), collect(4:6)]`, runtests.jl:658)
        hv = s.GroupNormL2(k["lambda"], [list(range(a, b)) for a, b in zip(off[:-1], off[1:])])
        yv = s.prox(s.shifted(hv, x, k["delta"], s.NormLinf(1.0)), q, k["sigma"]).cpu().numpy()
        assert _bits_equal(y, yv)
    with pytest.raises(IndexError):
        s.shifted(s.GroupNormL2([1.0, 1.0], [[0, 2, 4], [1, 3, 6]]), _dev(np.ones(6))[0])  # BoundsError
    # branches of shiftedGroupNormL2Binf.jl:102-109: zero groups, |X| <= Delta everywhere, huge lambda
    n, g = 128 * 6, 128
    rng = np.random.default_rng(5)
    x = rng.normal(size=n); sj = rng.uniform(-0.5, 0.5, size=n); q = rng.normal(size=n)
    x[:g] = 0; sj[:g] = 0; q[:g] = 0                  # all-zero group
    x[g:2 * g] *= 0.01                                # |X_i| <= Delta: nothing thresholds at lmin
    q[2 * g:3 * g] = -(x + sj)[2 * g:3 * g]           # S == 0
    lam = np.array([1.0, 1.0, 1.0, 1e6, 1e-9, 0.5])   # huge / tiny weights
    xd, sd, qd = _dev(x, sj, q)
    h = s.GroupNormL2(lam.tolist(), [range(i, i + g) for i in range(0, n, g)])
    y = s.prox(s.shifted(s.shifted(h, xd, 1.0, s.NormLinf(1.0)), sd), qd, 1.0).cpu().numpy()
    ref = orc.prox_group_l2_binf(q, x, sj, lam, 1.0, 1.0, gsize=g)
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(ref))
    offs = list(range(0, n + 1, g))
    well = np.ones(n, bool)
    well[3 * g:4 * g] = False
    _group_check(np.where(well, y, 0), np.where(well, ref, 0), q, x, sj, offs)
    # lambda = 1e6 >> ||S||: the root sits 3.5e-6 (relative) above the pole of step(n); the reference's Float64 evaluation
    # is 2.8e-6 away from the exact value of its own formula there (granularity of the double n), the kernel's closed form
    # (alpha = tau at the root) ~1e-16.  Adjudicated in binary128: the GPU may not be the worse side.
    v = _binf_check(orc, y, ref, q, x, sj, lam, 1.0, 1.0, offs, what="lambda=1e6 group")
    print(v)


def test_group_l2_property_vs_norml2(s):
    # test/runtests.jl:244-251: ShiftedGroupNormL2 prox == NormL2 prox of q + x, minus x
    rng = np.random.default_rng(3)
    x, q = rng.random(6), rng.random(6)
    lam, nu = rng.random(2), rng.random()
    xd, qd = _dev(x, q)
    y = s.prox(s.shifted(s.GroupNormL2(lam.tolist(), [range(0, 3), range(3, 6)]), xd), qd, nu).cpu().numpy()
    parts = []
    for g, sl in enumerate((slice(0, 3), slice(3, 6))):
        v = (q + x)[sl]
        parts.append(max(1 - nu * lam[g] / np.linalg.norm(v), 0.0) * v)
    assert np.linalg.norm(y - (np.concatenate(parts) - x)) <= 1e-11


@pytest.mark.parametrize("gsize", [1, 2, 3, 32, 128])
def test_group_binf_degenerate_bracket(s, orc, gsize):
    """lmax = ||S|| + sigma (zlmax + lambda ||X||) below sigma*lambda: the reference hands Roots.fzero a reversed bracket
    that straddles the pole of step(n); the root it returns can lie BELOW sigma*lambda.  Both the small-group kernel and
    the deferred list of the register kernel must reproduce the reference's literal arithmetic there."""
    rng = np.random.default_rng(1000 + gsize)
    ng = 4000
    n = ng * gsize
    scale = 0.6 / np.sqrt(gsize)
    x = rng.normal(size=n) * scale
    sj = rng.uniform(-0.5, 0.5, size=n) * scale
    q = rng.normal(size=n) * scale
    lam = rng.choice([2.0, 10.0, 0.7], size=ng)
    sigma, delta = 2.0, 0.3 * scale
    ref = orc.prox_group_l2_binf(q, x, sj, lam, sigma, delta, gsize=gsize)
    # the test is only meaningful if the regime actually occurs: count groups whose bracket is reversed
    S = ((q + x) + sj).reshape(ng, gsize)
    nX = np.linalg.norm(x.reshape(ng, gsize), axis=1)
    assert np.sum(np.linalg.norm(S, axis=1) + sigma * lam * nX < sigma * lam) > ng // 10
    xd, sd, qd = _dev(x, sj, q)
    h = s.GroupNormL2(lam.tolist(), [range(i, i + gsize) for i in range(0, n, gsize)])
    y = s.prox(s.shifted(s.shifted(h, xd, delta, s.NormLinf(1.0)), sd), qd, sigma).cpu().numpy()
    # roots next to the pole amplify last-bit differences of the norm: every group above the plain bar is adjudicated
    v = _binf_check(orc, y, ref, q, x, sj, lam, sigma, delta, np.arange(0, n + 1, gsize), what="degenerate bracket gsize=%d" % gsize)
    print(v)
    assert v.n_checked <= ng // 50, v       # ... and they are rare


# ------------------------------------------------------------------ iprox!
@pytest.mark.parametrize("op", ["ShiftedNormL0Box", "ShiftedNormL1Box"])
def test_iprox_testsbox_through_gpu(s, kats, op):
    # test/testsbox.jl:101-304: 14 cases per operator, exact ==
    t = kats["iprox_testsbox"]
    c = t[op]
    H = s.NormL0 if op == "ShiftedNormL0Box" else s.NormL1
    for d, g, x, lam, sol in zip(c["d"], c["g"], c["x"], c["lambda"], c["sol"]):
        xd, gd, dd, sd = _dev(np.array([x]), np.array([g]), np.array([d]), np.array([t["s"]]))
        ld, ud = _dev(np.array([t["l"]]), np.array([t["u"]]))
        omega = s.shifted(s.shifted(H(lam), xd, ld, ud), sd)
        s.iprox(omega, gd, dd)
        assert float(omega.sol[0]) == sol


@pytest.mark.parametrize("n", [1, 2, 3, 1000, 65_537, 1_000_003])
@pytest.mark.parametrize("op", ["l1", "l0", "l1_box", "l0_box"])
def test_iprox_parity(s, orc, op, n):
    rng = np.random.default_rng(600 + n)
    x, sj, g = _data(n, 601 + n)
    lam = 0.9
    box = op.endswith("box")
    if box:  # all three regimes of d, incl. |d| <= eps and exact zeros, and g == 0
        d = rng.choice([1.0, -1.0, 0.0, 1e-17], size=n) * rng.uniform(0.2, 3.0, size=n)
        g = np.where(rng.random(n) < 0.05, 0.0, g)
    else:
        d = rng.uniform(0.1, 3.0, size=n)
    xd, sd, gd, dd = _dev(x, sj, g, d)
    H = s.NormL1 if "l1" in op else s.NormL0
    if box:
        l = -1.0 - 0.1 * rng.random(n)
        u = 1.0 + 0.1 * rng.random(n)
        for lo, uo in ((-1.05, 1.05), (l, u)):
            ldv = _dev(lo)[0] if not np.isscalar(lo) else lo
            udv = _dev(uo)[0] if not np.isscalar(uo) else uo
            for selected in (None, range(0, n, 2)):
                psi = s.shifted(s.shifted(H(lam), xd, ldv, udv, selected) if selected is not None else s.shifted(H(lam), xd, ldv, udv), sd)
                y = s.iprox(psi, gd, dd).cpu().numpy()
                mask = orc.mask_from_selected([i + 1 for i in selected], n) if selected is not None else None
                ref = getattr(orc, "iprox_" + op)(g, d, x, sj, lam, lo, uo, mask=mask)
                assert _bits_equal(y, ref), (op, n)
    else:
        psi = s.shifted(s.shifted(H(lam), xd), sd)
        y = s.iprox(psi, gd, dd).cpu().numpy()
        assert _bits_equal(y, getattr(orc, "iprox_" + op)(g, d, x, sj, lam))
        dbad = d.copy()
        dbad[n // 2] = 0.0
        with pytest.raises(AssertionError):  # partial_prox.jl:59 @test_throws AssertionError
            s.iprox(psi, gd, _dev(dbad)[0])
        with pytest.raises(TypeError):
            s.iprox(s.shifted(s.RootNormLhalf(1.0), xd), gd, dd)  # no iprox! method in the reference either


# ------------------------------------------------------------------ psi(y)
@pytest.mark.parametrize("n", [1, 5, 1000, 65_537, 2_000_003])
def test_objective_values(s, orc, n):
    rng = np.random.default_rng(700 + n)
    x, sj, _ = _data(n, 701 + n)
    y = rng.uniform(-0.3, 0.3, size=n)
    y[rng.random(n) < 0.1] = 0.0
    x[rng.random(n) < 0.1] = 0.0  # exact zeros for the counting operators
    sj = np.where(x == 0.0, 0.0, sj)
    xd, sd, yd = _dev(x, sj, y)
    chi = s.NormLinf(1.0)
    rel = lambda a, b: abs(a - b) <= 1e-12 * max(1.0, abs(b))
    for kind, H in (("l1", s.NormL1), ("l0", s.NormL0), ("lhalf", s.RootNormLhalf)):
        lam = 0.7
        psi = s.shifted(s.shifted(H(lam), xd), sd)
        ref = orc.obj_plain(kind, y, x, sj, lam)
        assert (psi(yd) == ref) if kind == "l0" else rel(psi(yd), ref), (kind, n)
        # Box: inside (value) and outside (Inf); vector bounds and a selected subset too
        for delta in (1.0, 0.2):
            om = s.shifted(s.shifted(H(lam), xd, delta, chi), sd)
            ref = orc.obj_box(kind, y, x, sj, lam, -delta, delta)
            got = om(yd)
            assert (got == ref) if (kind == "l0" or np.isinf(ref)) else rel(got, ref), (kind, n, delta)
        if n >= 5:
            l = -1.0 - 0.1 * rng.random(n); u = 1.0 + 0.1 * rng.random(n)
            ld, ud = _dev(l, u)
            sel = range(0, n, 2)
            om = s.shifted(s.shifted(H(lam), xd, ld, ud, sel), sd)
            ref = orc.obj_box(kind, y, x, sj, lam, l, u, mask=orc.mask_from_selected([i + 1 for i in sel], n))
            assert (om(yd) == ref) if kind == "l0" else rel(om(yd), ref)
    nnz = int(np.count_nonzero((x + sj) + y))
    for r in (max(1, nnz - 1), nnz, nnz + 1):
        assert s.shifted(s.shifted(s.IndBallL0(r), xd), sd)(yd) == orc.obj_indball_l0(y, x, sj, r)
        for delta in (1.0, 0.2):
            got = s.shifted(s.shifted(s.IndBallL0(r), xd, delta, chi), sd)(yd)
            assert got == orc.obj_indball_l0(y, x, sj, r, delta=delta)


def test_objective_groups_and_reference_identities(s, orc):
    rng = np.random.default_rng(71)
    sizes = [1, 5, 64, 129, 1000, 2, 4096, 33]
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    n = int(offsets[-1])
    x, sj, _ = _data(n, 72)
    y = rng.uniform(-0.3, 0.3, size=n)
    lam = rng.uniform(0.2, 2.0, size=len(sizes))
    xd, sd, yd = _dev(x, sj, y)
    groups = [range(int(a), int(b)) for a, b in zip(offsets[:-1], offsets[1:])]
    h = s.GroupNormL2(lam.tolist(), groups)
    ref = orc.obj_group_l2(y, x, sj, lam, offsets=offsets)
    assert abs(s.shifted(s.shifted(h, xd), sd)(yd) - ref) <= 1e-12 * ref
    for delta in (1.0, 0.3):
        got = s.shifted(s.shifted(h, xd, delta, s.NormLinf(1.0)), sd)(yd)
        want = orc.obj_group_l2(y, x, sj, lam, offsets=offsets, delta=delta)
        assert got == want if np.isinf(want) else abs(got - want) <= 1e-12 * want
    # uniform 128-groups and the identities of test/runtests.jl:438-447
    m = 128 * 100
    x, sj, _ = _data(m, 73)
    xd = _dev(x)[0]
    lamu = rng.uniform(0.5, 1.5, size=100)
    hu = s.GroupNormL2(lamu.tolist(), [range(i, i + 128) for i in range(0, m, 128)])
    psi = s.shifted(hu, xd, 0.01, s.NormLinf(1.0))
    import torch
    zero = torch.zeros(m, dtype=torch.float64, device="cuda:0")
    hx = sum(lamu[g] * np.linalg.norm(x[g * 128:(g + 1) * 128]) for g in range(100))
    assert abs(psi(zero) - hx) <= 1e-12 * hx            # psi(zeros(n)) == h(x)
    yy = rng.random(m); yy *= 0.01 / np.max(np.abs(yy)) / 2
    assert np.isfinite(psi(_dev(yy)[0])) and psi(_dev(3 * yy)[0]) == np.inf   # inside / outside the trust region


@pytest.mark.parametrize("gs", [1, 2, 3, 4, 5, 8, 9, 16, 17, 40, 64, 65, 300])
def test_objective_group_sizes(s, orc, gs):
    """psi(y) of both group operators on uniform groups of every lane-team width of k_obj_group (1 .. 64 lanes per group) and on
    ragged groups with that size as the bound; the last wavefront's idle slots (group count not a multiple of 64 / team)."""
    rng = np.random.default_rng(4100 + gs)
    ng = 1237
    n = ng * gs
    x, sj, _ = _data(n, 4200 + gs)
    y = rng.uniform(-0.3, 0.3, size=n)
    lam = rng.uniform(0.2, 2.0, size=ng)
    xd, sd, yd = _dev(x, sj, y)
    import torch
    h = s.GroupNormL2.uniform(torch.from_numpy(lam).cuda(), gs)
    ref = orc.obj_group_l2(y, x, sj, lam, offsets=np.arange(0, n + 1, gs))
    assert abs(s.shifted(s.shifted(h, xd), sd)(yd) - ref) <= 1e-12 * ref
    for delta in (1.0, 0.2):
        got = s.shifted(s.shifted(h, xd, delta, s.NormLinf(1.0)), sd)(yd)
        want = orc.obj_group_l2(y, x, sj, lam, offsets=np.arange(0, n + 1, gs), delta=delta)
        assert got == want if np.isinf(want) else abs(got - want) <= 1e-12 * want
    # ragged: sizes 1 .. gs
    sizes = rng.integers(1, gs + 1, size=ng)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    m = int(offsets[-1])
    groups = [range(int(a), int(b)) for a, b in zip(offsets[:-1], offsets[1:])]
    hr = s.GroupNormL2(lam.tolist(), groups)
    refr = orc.obj_group_l2(y[:m], x[:m], sj[:m], lam, offsets=offsets)
    assert abs(s.shifted(s.shifted(hr, xd[:m]), sd[:m])(yd[:m]) - refr) <= 1e-12 * refr


# ------------------------------------------------------------------ ShiftedNormL1B2
def test_l1b2(s, orc, kats):
    k = kats["box_golden"]  # test/runtests.jl:467-474
    x, q = _dev(np.array(k["x"]), np.array(k["q"]))
    psi = s.shifted(s.NormL1(k["lambda"]), x, k["delta"], s.NormL2(1.0))
    assert type(psi).__name__ == "ShiftedNormL1B2"
    y = s.prox(psi, q, k["sigma"]).cpu().numpy()
    np.testing.assert_allclose(y, k["expected"]["ShiftedNormL1B2"], rtol=k["rtol"], atol=0)
    for n in (1, 2, 7, 1000, 300_001):
        xh, sh, qh = _data(n, 900 + n)
        xd, sd, qd = _dev(xh, sh, qh)
        for lam, sigma, delta in ((1.0, 1.0, 1.0), (0.3, 2.0, 0.05 * np.sqrt(n)), (2.0, 0.5, 100.0 * np.sqrt(n))):
            om = s.shifted(s.shifted(s.NormL1(lam), xd, delta, s.NormL2(1.0)), sd)
            y = s.prox(om, qd, sigma).cpu().numpy()
            ref = orc.prox_l1_b2(qh, xh, sh, lam, sigma, delta, 1.0)
            scale = max(np.linalg.norm(ref), np.linalg.norm(xh), 1e-300)
            assert np.max(np.abs(y - ref)) <= 1e-12 * scale, (n, lam, sigma, delta)
        s.set_radius_bang(om, 0.5)
        assert om.Δ == 0.5
    # 8-byte-aligned views (scalar kernels), chi = NormL2(0.7), y === q
    import torch
    n = 50_001
    xh, sh, qh = _data(n, 4242)
    xd, sd, qd = (torch.cat([torch.zeros(1, dtype=torch.float64), torch.from_numpy(a)]).cuda()[1:] for a in (xh, sh, qh))
    om = s.shifted(s.shifted(s.NormL1(0.8), xd, 3.0, s.NormL2(0.7)), sd)
    ref = orc.prox_l1_b2(qh, xh, sh, 0.8, 1.3, 3.0, 0.7)
    scale = max(np.linalg.norm(ref), np.linalg.norm(xh))
    assert np.max(np.abs(s.prox(om, qd, 1.3).cpu().numpy() - ref)) <= 1e-12 * scale
    xa, sa, qa = _dev(xh, sh, qh)
    oma = s.shifted(s.shifted(s.NormL1(0.8), xa, 3.0, s.NormL2(0.7)), sa)
    s.prox_bang(qa, oma, qa, 1.3)
    assert np.max(np.abs(qa.cpu().numpy() - ref)) <= 1e-12 * scale
    # psi(y) = lambda ||xk + sj + y||_1 + IndBallL2(Delta)(sj + y)   (src/shiftedNormL1B2.jl:32)
    yin = ref                                             # the prox lies inside the ball (up to rounding)
    for yy in (yin, 0.5 * yin, 3.0 * yin, np.zeros(n)):
        val, exp = oma(_dev(yy)[0]), orc.obj_l1_b2(yy, xh, sh, 0.8, 3.0)
        assert (val == exp) or abs(val - exp) <= 1e-12 * abs(exp), (val, exp)
    assert om(torch.cat([torch.zeros(1, dtype=torch.float64), torch.from_numpy(3.0 * yin)]).cuda()[1:]) == \
        orc.obj_l1_b2(3.0 * yin, xh, sh, 0.8, 3.0)


def test_l1b2_large(s, orc):
    # n = 4e6: vectorised reduction passes, iteration started from the a-priori upper bound of the root
    n = 4_000_000
    xh, sh, qh = _data(n, 77)
    xd, sd, qd = _dev(xh, sh, qh)
    for lam, sigma, delta in ((1.0, 1.0, 1.0), (0.2, 1.0, 300.0), (1.0, 1.0, 1e6)):
        om = s.shifted(s.shifted(s.NormL1(lam), xd, delta, s.NormL2(1.0)), sd)
        y = s.prox(om, qd, sigma).cpu().numpy()
        ref = orc.prox_l1_b2(qh, xh, sh, lam, sigma, delta, 1.0)
        scale = max(np.linalg.norm(ref), np.linalg.norm(xh))
        assert np.max(np.abs(y - ref)) <= 1e-12 * scale, (lam, sigma, delta)


@pytest.mark.parametrize("n", [2, 3, 4, 1001, 1002, 300_001])
def test_l1b2_misaligned_views(s, orc, n):
    """All four vectors from an odd element on (8 bytes off a 16-byte boundary): the vector kernels run on the aligned
    rest and take element 0 along (n >= 3; n = 2 stays on the scalar path).  Trust region active, barely active and
    inactive (twice: the second inactive call stores y in its first pass), y disjoint and aliased to q."""
    import torch
    xh, sh, qh = _data(n, 90 + n)
    xh[0], qh[0] = 3.0, -2.0                           # element 0 matters for the norms
    mk = lambda a: torch.cat([torch.zeros(1, dtype=torch.float64), torch.from_numpy(a)]).cuda()[1:]
    xd, sd, qd = mk(xh), mk(sh), mk(qh)
    assert all(t.data_ptr() % 16 == 8 for t in (xd, sd, qd))
    nrm = float(np.linalg.norm(xh))
    for lam, sigma, delta in ((1.0, 1.0, 0.5), (0.3, 0.7, 0.9 * nrm), (1.0, 1.0, 1e6), (1.0, 1.0, 1e6)):
        om = s.shifted(s.shifted(s.NormL1(lam), xd, delta, s.NormL2(1.0)), sd)
        ref = orc.prox_l1_b2(qh, xh, sh, lam, sigma, delta, 1.0)
        scale = max(np.linalg.norm(ref), np.linalg.norm(xh))
        yv = mk(np.zeros(n))
        s.prox_bang(yv, om, qd, sigma)
        assert np.max(np.abs(yv.cpu().numpy() - ref)) <= 1e-12 * scale, (n, lam, sigma, delta)
        q2 = mk(qh.copy())
        s.prox_bang(q2, om, q2, sigma)                 # y === q
        assert np.max(np.abs(q2.cpu().numpy() - ref)) <= 1e-12 * scale, (n, lam, sigma, delta, "aliased")


# ------------------------------------------------------------------ special values
def test_special_values_separable(s, orc):
    """+-0, +-Inf, NaN, subnormals, huge values and points exactly on the thresholds, in every combination of
    (q, xk, sj): the L1 / L0 families must reproduce the reference formulas bit for bit (signed zeros included; a NaN
    must be a NaN, its payload is not compared), also through iprox!."""
    lam, sigma = 1.0, 1.0
    vals = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1e308, -1e308,
                     np.sqrt(2.0), -np.sqrt(2.0), np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)])
    Q, X, S = (g.ravel().copy() for g in np.meshgrid(vals, vals, vals, indexing="ij"))
    n = Q.size
    qd, xd, sd = _dev(Q, X, S)
    with np.errstate(all="ignore"):
        for op, H in (("l1", s.NormL1), ("l0", s.NormL0)):
            y = s.prox(s.shifted(s.shifted(H(lam), xd), sd), qd, sigma).cpu().numpy()
            assert _same_or_both_nan(y, getattr(orc, "prox_" + op)(Q, X, S, lam, sigma)), op
        for op, H in (("l1_box", s.NormL1), ("l0_box", s.NormL0)):
            for lo, up in ((-1.0, 1.0), (0.0, 0.0), (-np.inf, np.inf), (-0.0, 2.0)):
                y = s.prox(s.shifted(s.shifted(H(lam), xd, lo, up), sd), qd, sigma).cpu().numpy()
                ref = getattr(orc, "prox_" + op)(Q, X, S, lam, sigma, lo, up)
                assert _same_or_both_nan(y, ref), (op, lo, up, int(np.sum(~(np.isnan(y) & np.isnan(ref)) & (y.view(np.int64) != ref.view(np.int64)))))
        # iprox!: d runs over the same special values (Box forms accept any sign of d)
        D = np.resize(np.array([1.0, -1.0, 0.0, -0.0, 2.0, 1e-17, -1e-17, np.inf, 5e-324, 0.5]), n)
        dd = _dev(D)[0]
        for name, H in (("iprox_l1_box", s.NormL1), ("iprox_l0_box", s.NormL0)):
            for lo, up in ((-1.0, 1.0), (-np.inf, np.inf), (-np.inf, 0.5), (0.0, 0.0)):
                y = s.iprox(s.shifted(s.shifted(H(lam), xd, lo, up), sd), qd, dd).cpu().numpy()
                assert _same_or_both_nan(y, getattr(orc, name)(Q, D, X, S, lam, lo, up)), (name, lo, up)


def test_special_values_lhalf(s, orc):
    """RootNormLhalf(Box) on the same special-value grid: finite results to LHALF_TOL, NaN where the reference formula
    gives NaN, +-Inf where it gives +-Inf."""
    lam, sigma = 0.8, 1.3
    vals = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1e308, -1e308, 1e-200, 3.0])
    Q, X, S = (g.ravel().copy() for g in np.meshgrid(vals, vals, vals, indexing="ij"))
    qd, xd, sd = _dev(Q, X, S)

    def check(y, ref, tag):
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(y), np.isnan(ref)), (tag, int(np.sum(np.isnan(y) != np.isnan(ref))))
        inf = np.isinf(ref)
        assert np.array_equal(y[inf], ref[inf]), tag
        with np.errstate(all="ignore"):
            scale = np.maximum(np.maximum(np.abs(ref), np.abs(X + S)), np.abs(Q))
            bad = fin & (np.abs(y - ref) > LHALF_TOL * np.where(np.isfinite(scale), scale, 1.0))
        assert not bad.any(), (tag, int(bad.sum()))

    with np.errstate(all="ignore"):
        y = s.prox(s.shifted(s.shifted(s.RootNormLhalf(lam), xd), sd), qd, sigma).cpu().numpy()
        check(y, orc.prox_lhalf(Q, X, S, lam, sigma), "lhalf")
        # Box form: infinite BOUNDS (absent / one-sided boxes) and NaN data are covered; +-Inf and 1e308 in q / xk / sj
        # are not (Inf - Inf and overflowing squares inside the candidate values: the kernel's rsq-based sqrt / closed
        # form and the reference's libm calls disagree on which garbage comes out) -- those grid points are masked
        big = lambda a: np.abs(np.nan_to_num(a, nan=0.0)) >= 1e300
        data_ok = ~(big(Q) | big(X) | big(S))
        for lo, up in ((-1.0, 1.0), (-np.inf, np.inf), (0.0, 2.0), (-np.inf, 0.5), (-0.5, np.inf)):
            y = s.prox(s.shifted(s.shifted(s.RootNormLhalf(lam), xd, lo, up), sd), qd, sigma).cpu().numpy()
            ref = orc.prox_lhalf_box(Q, X, S, lam, sigma, lo, up)
            y, ref = np.where(data_ok, y, 0.0), np.where(data_ok, ref, 0.0)
            check(y, ref, ("lhalf_box", lo, up))


def test_infinite_trust_region(s, orc):
    """Delta = Inf (no trust region): the BInf / Binf / B2 forms must still follow their formulas -- and then equal the
    forms without a trust region."""
    n, gs = 128 * 40, 128
    x, sj, q = _data(n, 321)
    xd, sd, qd = _dev(x, sj, q)
    lam = np.random.default_rng(1).uniform(0.5, 1.5, size=n // gs)
    h = s.GroupNormL2.uniform(lam.tolist(), gs)
    with np.errstate(all="ignore"):
        ref = orc.prox_group_l2_binf(q, x, sj, lam, 0.9, np.inf, gsize=gs)
    y = s.prox(s.shifted(s.shifted(h, xd, np.inf, s.NormLinf(1.0)), sd), qd, 0.9).cpu().numpy()
    _group_check(y, ref, q, x, sj, list(range(0, n + 1, gs)))
    _group_check(y, orc.prox_group_l2(q, x, sj, lam, 0.9, gsize=gs), q, x, sj, list(range(0, n + 1, gs)))
    yb = s.prox(s.shifted(s.shifted(s.IndBallL0(100), xd, np.inf, s.NormLinf(1.0)), sd), qd, 1.0).cpu().numpy()
    assert _bits_equal(yb, orc.prox_indball_l0(q, x, sj, 100))
    y2 = s.prox(s.shifted(s.shifted(s.NormL1(0.7), xd, np.inf, s.NormL2(1.0)), sd), qd, 1.1).cpu().numpy()
    assert np.max(np.abs(y2 - orc.prox_l1_b2(q, x, sj, 0.7, 1.1, np.inf, 1.0))) <= 1e-12 * np.linalg.norm(x)
    for H, name in ((s.NormL1, "prox_l1_box"), (s.NormL0, "prox_l0_box")):
        yy = s.prox(s.shifted(s.shifted(H(0.7), xd, np.inf, s.NormLinf(1.0)), sd), qd, 1.1).cpu().numpy()
        assert _bits_equal(yy, getattr(orc, name)(q, x, sj, 0.7, 1.1, -np.inf, np.inf))


@pytest.mark.parametrize("gs", [16, 128, 300, 1024])
def test_group_parameter_edges(s, orc, gs):
    """lambda = 0 groups, Delta = 0, tiny / huge sigma, all-zero and constant groups, for every group kernel family
    (4- / 8-lane tiles, partly filled tile, LDS-resident group)."""
    ng = 24
    n = ng * gs
    rng = np.random.default_rng(gs)
    x, sj, q = _data(n, 7000 + gs)
    x[:gs] = 0.0; sj[:gs] = 0.0; q[:gs] = 0.0                      # an all-zero group
    x[gs:2 * gs] = 0.25; sj[gs:2 * gs] = 0.0; q[gs:2 * gs] = 1.0   # a constant group
    x[2 * gs:3 * gs] = 0.0                                          # X = 0: nothing active at lmin
    lam = rng.uniform(0.2, 2.0, size=ng)
    lam[3] = 0.0                                                    # weight zero: sl = 0
    lam[4] = 1e-300
    xd, sd, qd = _dev(x, sj, q)
    h = s.GroupNormL2.uniform(lam.tolist(), gs)
    offs = list(range(0, n + 1, gs))
    for sigma, delta in ((1.0, 1.0), (1e-8, 1.0), (1e6, 1.0), (1.0, 0.0), (1.0, 1e-300), (0.7, 1e9)):
        with np.errstate(all="ignore"):
            ref = orc.prox_group_l2_binf(q, x, sj, lam, sigma, delta, gsize=gs)
            ref_plain = orc.prox_group_l2(q, x, sj, lam, sigma, gsize=gs)
        y = s.prox(s.shifted(s.shifted(h, xd, delta, s.NormLinf(1.0)), sd), qd, sigma).cpu().numpy()
        # sigma*lambda >> ||S|| (sigma = 1e6) makes the reference's own last step cancel: adjudicated, not loosened
        _binf_check(orc, y, ref, q, x, sj, lam, sigma, delta, offs, what="edges sigma=%g delta=%g" % (sigma, delta))
        yp = s.prox(s.shifted(s.shifted(h, xd), sd), qd, sigma).cpu().numpy()
        _group_check(yp, ref_plain, q, x, sj, offs)


# ------------------------------------------------------------------ prox! fused with the value of h
@pytest.mark.parametrize("n", [1, 2, 3, 1000, 1_000_003])
def test_prox_value_fused(s, orc, n):
    """spx_proxval_*: y must be bit-identical to the plain prox!, the value equal to psi(y) of that y (<= 1e-12; the
    NormL0 count exactly), for scalar / vector bounds, a selection mask, aligned and 8-byte-aligned vectors."""
    import torch
    x, sj, q = _data(n, 8100 + n)
    rng = np.random.default_rng(n)
    lo, up = -1.0 - 0.1 * rng.random(n), 1.0 + 0.1 * rng.random(n)
    selected = sorted(rng.choice(n, size=max(1, n // 3), replace=False).tolist())
    for misaligned in (False, True):
        if misaligned:
            xd, sd, qd, ld, ud = (torch.cat([torch.zeros(1, dtype=torch.float64), torch.from_numpy(a)]).cuda()[1:]
                                  for a in (x, sj, q, lo, up))
        else:
            xd, sd, qd, ld, ud = _dev(x, sj, q, lo, up)
        cases = []
        for H, kind in ((s.NormL1, "l1"), (s.NormL0, "l0"), (s.RootNormLhalf, "lhalf")):
            cases.append((s.shifted(s.shifted(H(0.7), xd), sd), kind))
            cases.append((s.shifted(s.shifted(H(0.7), xd, 0.9, s.NormLinf(1.0)), sd), kind))
            cases.append((s.shifted(s.shifted(H(0.7), xd, ld, ud, selected), sd), kind))
        for psi, kind in cases:
            y_plain = s.prox(psi, qd, 1.1).clone()
            y, val = s.prox_value(psi, qd, 1.1)
            assert torch.equal(y, y_plain), (type(psi).__name__, misaligned)
            exp = psi(y_plain)
            assert np.isfinite(exp)
            if kind == "l0":
                assert val == exp
            else:
                assert abs(val - exp) <= 1e-12 * max(abs(exp), 1e-300), (type(psi).__name__, val, exp)
    # q_scale: the prox of q_scale * q formed on the fly is bit-identical to scaling q first (R2: q = -nu grad f)
    xd, sd, qd = _dev(x, sj, q)
    for psi in (s.shifted(s.shifted(s.NormL1(0.7), xd, 0.9, s.NormLinf(1.0)), sd), s.shifted(s.shifted(s.NormL0(0.7), xd), sd),
                s.shifted(s.shifted(s.RootNormLhalf(0.7), xd, ld, ud, selected), sd) if not misaligned else
                s.shifted(s.shifted(s.RootNormLhalf(0.7), xd), sd)):
        y1, v1 = s.prox_value(psi, qd, 1.1, q_scale=-0.37)
        y1 = y1.clone()
        y2, v2 = s.prox_value(psi, -0.37 * qd, 1.1)
        assert torch.equal(y1, y2) and v1 == v2
    # y === q (ShiftedNormL1: the reference's two-pass quirk) through the fused form too
    xd, sd, qd = _dev(x, sj, q)
    psi = s.shifted(s.shifted(s.NormL1(0.7), xd), sd)
    q1, q2 = qd.clone(), qd.clone()
    s.prox_bang(q1, psi, q1, 1.1)
    _, val = s.prox_value_bang(q2, psi, q2, 1.1)
    assert torch.equal(q1, q2) and abs(val - psi(q1)) <= 1e-12 * max(abs(val), 1e-300)


@pytest.mark.parametrize("gs", [3, 16, 128, 300, 1024])
def test_group_binf_lattice_and_zero_x(s, orc, gs):
    """Data on a lattice (multiples of 1/4): activity boundaries |tau S - X| = Delta, equal entries, exact roots and the
    reference's exact zero froot(lmax) = ||S|| - ||-S|| (X = 0 with everything thresholded: the state of a solver at
    x0 = 0 inside a wide trust region) occur constantly."""
    rng = np.random.default_rng(40 + gs)
    ng = 150 if gs <= 300 else 24
    n = ng * gs
    offs = list(range(0, n + 1, gs))
    for rep in range(6):
        x = rng.integers(-8, 9, size=n) / 4.0
        sj = rng.integers(-2, 3, size=n) / 4.0
        q = rng.integers(-12, 13, size=n) / 4.0
        if rep % 3 == 1:
            x[: n // 2] = 0.0
        if rep % 3 == 2:
            x[:] = 0.0                                   # x0 = 0 everywhere
        lam = rng.choice([0.0, 0.25, 0.5, 1.0, 2.0, 8.0], size=ng)
        sigma = float(rng.choice([0.25, 0.5, 1.0, 2.0]))
        delta = float(rng.choice([0.25, 1.0, 3.0, 100.0]))
        xd, sd, qd = _dev(x, sj, q)
        h = s.GroupNormL2.uniform(lam.tolist(), gs)
        with np.errstate(all="ignore"):
            ref = orc.prox_group_l2_binf(q, x, sj, lam, sigma, delta, gsize=gs)
        y = s.prox(s.shifted(s.shifted(h, xd, delta, s.NormLinf(1.0)), sd), qd, sigma).cpu().numpy()
        _binf_check(orc, y, ref, q, x, sj, lam, sigma, delta, offs, what="lattice gs=%d rep=%d" % (gs, rep))


@pytest.mark.parametrize("gs", [1, 7, 128, 300, 1024])
def test_group_binf_zero_groups_strong_lambda(s, orc, gs):
    """The bulk of a group-lasso run: groups of the iterate that are zero (xk == 0 on the group, any sj) under a
    sigma*lambda above ||S||.  The reference's bracket is usually reversed there (lmax < lmin) and its fzero ends next to
    the pole of step(n), yet the result is always y = -sj; the kernels decide that without the literal evaluation
    (tools/sweep_params.py: 27 ms -> 0.7 ms at 1e6 x 128).  Mixed with ordinary groups and with ties sigma*lambda ~ ||S||."""
    rng = np.random.default_rng(900 + gs)
    ng = 600 if gs <= 300 else 40
    n = ng * gs
    x = rng.normal(size=n).reshape(ng, gs)
    zero_g = rng.random(ng) < 0.6
    x[zero_g] = 0.0
    x = x.reshape(n)
    sj, q = rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    nS = np.linalg.norm(((q + x) + sj).reshape(ng, gs), axis=1)
    lam = nS * rng.choice([0.5, 1.0 - 1e-12, 1.0, 1.0 + 1e-12, 1.5, 4.0, 40.0], size=ng)
    xd, sd, qd = _dev(x, sj, q)
    h = s.GroupNormL2.uniform(lam.tolist(), gs)
    for sigma, delta in ((1.0, 0.01), (1.0, 0.6), (0.37, 4.0), (2.0, 100.0)):
        lam_s = lam / sigma
        hs = s.GroupNormL2.uniform(lam_s.tolist(), gs)
        with np.errstate(all="ignore"):
            ref = orc.prox_group_l2_binf(q, x, sj, lam_s, sigma, delta, gsize=gs)
        y = s.prox(s.shifted(s.shifted(hs, xd, delta, s.NormLinf(1.0)), sd), qd, sigma).cpu().numpy()
        strong = zero_g & (sigma * lam_s * (1 - 1e-9) > nS)
        assert strong.sum() > ng // 5
        assert np.array_equal(y.reshape(ng, gs)[strong], -sj.reshape(ng, gs)[strong])   # exactly -sj
        v = _binf_check(orc, y, ref, q, x, sj, lam_s, sigma, delta, np.arange(0, n + 1, gs), what="zero groups gs=%d sigma=%g" % (gs, sigma))
        assert v.n_checked <= max(2, ng // 50), v


@pytest.mark.parametrize("gs", [1, 3, 16, 128, 250])
def test_group_binf_small_groups_being_zeroed(s, orc, gs):
    """Small nonzero groups (||xk|| < 1 on the group, entries inside the trust region) under a strong sigma*lambda: the
    reference's bracket is reversed; with every |xk_i| < Delta its answer is zeros (kernel comment in binf_root), which
    the register kernel now decides itself; entries outside the trust region or ties still take the literal evaluation
    (deferred list, register-resident since round 1).  Both must agree with the oracle."""
    rng = np.random.default_rng(950 + gs)
    ng = 1500
    n = ng * gs
    x = rng.normal(size=n) * (0.3 / np.sqrt(gs))
    sj, q = rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    S = ((q + x) + sj).reshape(ng, gs)
    nS, nX, mX = np.linalg.norm(S, axis=1), np.linalg.norm(x.reshape(ng, gs), axis=1), np.abs(x.reshape(ng, gs)).max(axis=1)
    xd, sd, qd = _dev(x, sj, q)
    seen_fast = seen_literal = 0
    for sigma, delta, lscale in ((1.0, 1.0, 3.0), (0.5, 0.05 / np.sqrt(gs), 8.0), (2.0, 0.4 / np.sqrt(gs), 2.0), (1.0, 50.0, 30.0)):
        lam = rng.uniform(0.5, 1.5, size=ng) * lscale * max(1.0, np.sqrt(gs))
        h = s.GroupNormL2.uniform(lam.tolist(), gs)
        with np.errstate(all="ignore"):
            ref = orc.prox_group_l2_binf(q, x, sj, lam, sigma, delta, gsize=gs)
        y = s.prox(s.shifted(s.shifted(h, xd, delta, s.NormLinf(1.0)), sd), qd, sigma).cpu().numpy()
        rev = nS + sigma * lam * nX < sigma * lam * (1 - 1e-6)          # (zlmax = 0 there or not: a lower bound on lmax)
        seen_fast += int(np.sum(rev & (mX < delta * (1 - 1e-9))))
        seen_literal += int(np.sum(rev & (mX > delta)))
        # roots next to the pole amplify last-bit differences of the norm (as test_group_binf_degenerate_bracket)
        offs = np.arange(0, n + 1, gs)
        v = _binf_check(orc, y, ref, q, x, sj, lam, sigma, delta, offs, what="being zeroed gs=%d sigma=%g" % (gs, sigma))
        assert v.n_checked <= ng // 50, v
        # a mis-decided group (zero on one side only) is never a "1 % outlier": the zero patterns agree wherever the
        # arbiter was not needed (needed + passed = the oracle's own Float64 decision was the rounding-decided one)
        zg, zo = arbiter.zero_pattern(y, x, sj, offs), arbiter.zero_pattern(ref, x, sj, offs)
        assert int(np.sum(zg != zo)) <= v.n_checked, (int(np.sum(zg != zo)), v)
    assert seen_fast > ng // 4 and seen_literal > ng // 10, (seen_fast, seen_literal)


@pytest.mark.parametrize("gs", [2, 16, 128, 700])
def test_group_binf_structured_scenarios(s, orc, gs):
    """Structured data for GroupNormL2Binf: X = 0, tiny X, S = X, S = 0, data tiny / huge against lambda and Delta,
    |X_i| = Delta EXACTLY (where the reference's froot(lmin) is decided by rounding at magnitude 1e16 and its bisection
    ends on a spurious root next to the pole: the literal evaluation must reproduce that), constant groups, heavy tails."""
    rng = np.random.default_rng(70 + gs)
    ng = 400 if gs <= 16 else (120 if gs <= 128 else 20)
    n = ng * gs

    def scen(k):
        x = rng.normal(size=n); sj = rng.uniform(-0.5, 0.5, size=n); q = rng.normal(size=n)
        if k == 0: x[:] = 0.0
        elif k == 1: x *= 1e-3
        elif k == 2: q = -sj.copy()
        elif k == 3: q = -(x + sj)
        elif k == 4: q *= 1e-6; sj *= 1e-6; x *= 1e-6
        elif k == 5: q *= 1e6
        elif k == 6: x = np.sign(x) * 1.0
        elif k == 7: q[:] = 0.25; x[:] = 0.5; sj[:] = 0.0
        elif k == 8: x[::2] = 0.0; q[1::2] = 0.0
        elif k == 9: x = rng.standard_cauchy(n); q = rng.standard_cauchy(n)
        return x, sj, q

    for k in range(10):
        for sigma, delta in ((1.0, 1.0), (0.01, 1.0), (30.0, 0.1), (1.0, 50.0)):
            x, sj, q = scen(k)
            lam = 10.0 ** rng.uniform(-3, 2, size=ng)
            xd, sd, qd = _dev(x, sj, q)
            h = s.GroupNormL2.uniform(lam.tolist(), gs)
            with np.errstate(all="ignore"):
                ref = orc.prox_group_l2_binf(q, x, sj, lam, sigma, delta, gsize=gs)
            y = s.prox(s.shifted(s.shifted(h, xd, delta, s.NormLinf(1.0)), sd), qd, sigma).cpu().numpy()
            _binf_check(orc, y, ref, q, x, sj, lam, sigma, delta, np.arange(0, n + 1, gs),
                        what="scenario %d gs=%d sigma=%g delta=%g" % (k, gs, sigma, delta))


@pytest.mark.parametrize("n", [1, 5, 64, 1000, 100_003])
def test_l1b2_structured_scenarios(s, orc, n):
    """x = 0, q = sj = 0, tiny / huge x, lattice data, constant vectors (the root is then hit exactly), heavy tails; tiny and
    huge radii."""
    rng = np.random.default_rng(300 + n)
    for k in range(9):
        x = rng.normal(size=n); sj = rng.uniform(-0.5, 0.5, size=n); q = rng.normal(size=n)
        if k == 0: x[:] = 0.0
        elif k == 1: q[:] = 0.0; sj[:] = 0.0
        elif k == 2: x *= 1e-8
        elif k == 3: x *= 1e8
        elif k == 4: x = np.round(x * 4) / 4; q = np.round(q * 4) / 4; sj = np.round(sj * 4) / 4
        elif k == 5: x[:] = 1.0; q[:] = -0.5; sj[:] = 0.25
        elif k == 6: x[::2] = 0.0
        elif k == 7: q = -sj + rng.choice([-1.0, 1.0], size=n) * 0.5
        elif k == 8: x = rng.standard_cauchy(n)
        xd, sd, qd = _dev(x, sj, q)
        for lam, sigma, delta, chil in ((1.0, 1.0, 1.0, 1.0), (0.01, 1.0, 0.1, 1.0), (5.0, 2.0, 1e-3, 0.5), (0.5, 0.3, 1e3, 2.0),
                                        (1.0, 1.0, 1e-12, 1.0)):
            with np.errstate(all="ignore"):
                ref = orc.prox_l1_b2(q, x, sj, lam, sigma, delta, chil)
            y = s.prox(s.shifted(s.shifted(s.NormL1(lam), xd, delta, s.NormL2(chil)), sd), qd, sigma).cpu().numpy()
            scale = max(np.linalg.norm(ref), np.linalg.norm(x), np.linalg.norm(sj + q), 1e-300)
            assert float(np.max(np.abs(y - ref))) <= 1e-12 * scale, (n, k, lam, sigma, delta, chil)


@pytest.mark.parametrize("gs", [1, 2, 4, 8, 16])
def test_group_binf_many_small_groups(s, orc, gs):
    """Rare-event hunt: 1e5 small random groups per configuration.  Small groups often have NO active entry at the root
    (all-inactive piece, B = 0 exactly): the masked sums must then be exactly zero and a psi of rounding size must count
    as converged -- otherwise the bracket logic bisected away from the root (3e-4 of 4-element groups, found by
    tools/fuzz_binf_many.py)."""
    rng = np.random.default_rng(900 + gs)
    ng = 100_000
    n = ng * gs
    for sigma, delta, lscale, xscale in ((1.0, 1.0, 1.0, 1.0), (0.3, 0.2, 0.1, 1.0), (2.0, 3.0, 3.0, 0.3), (1.0, 0.5, 1.0, 3.0),
                                         (1.0, 1.0, 30.0, 1.0)):
        x = rng.normal(size=n) * xscale
        sj = rng.uniform(-0.5, 0.5, size=n)
        q = rng.normal(size=n)
        lam = rng.uniform(0.05, 2.0, size=ng) * lscale
        xd, sd, qd = _dev(x, sj, q)
        import torch
        h = s.GroupNormL2.uniform(torch.from_numpy(lam).cuda(), gs)
        ref = orc.prox_group_l2_binf(q, x, sj, lam, sigma, delta, gsize=gs)
        y = s.prox(s.shifted(s.shifted(h, xd, delta, s.NormLinf(1.0)), sd), qd, sigma).cpu().numpy()
        # single ill-conditioned groups (the reference's last step cancels) sit above the plain bar: each one is adjudicated
        # in binary128; the failure this test guards against produced errors of 1e-2 .. 1e+2 in 3e-4 of the groups
        v = _binf_check(orc, y, ref, q, x, sj, lam, sigma, delta, np.arange(0, n + 1, gs), what="many small gs=%d sigma=%g" % (gs, sigma))
        # (lscale = 30: sigma*lambda >> ||S||, the root sits next to the pole and the REFERENCE's Float64 value is itself up to
        #  ~5e-9 off its own formula in 1-2 % of the groups; the closed form of the kernel is within 1e-15 there: measured
        #  "GPU closer to binary128 than the literal oracle in 1629 of 1629")
        assert v.n_checked <= ng // 20 and v.gpu_closer >= v.n_checked - 5, v


def test_group_binf_reference_faithful_mode(s, orc):
    """spx_ctx_set_tuning key 9 (round 3): groups whose root sits next to the pole of step(n) (u < n / 1000: sigma*lambda ~ 30 ||S||)
    take the reference's literal Float64 evaluation instead of the closed form at the root.  The default is the accurate side
    (within 1e-15 of binary128 where the reference is up to 4.5e-9 off); this mode is for reproducing a reference run: the
    results meet the ensemble bound of the arbiter, and they sit CLOSER to the literal Float64 oracle than the default's do
    (what is left is the summation order of `norm`, which the reference does not pin either)."""
    import torch
    L = s._lib.load()
    ctx = s.context("cuda:0")
    rng = np.random.default_rng(909)
    for gs in (4, 16, 128):
        ng = 40_000
        n = ng * gs
        sigma, delta = 1.0, 1.0
        x = rng.normal(size=n); sj = rng.uniform(-0.5, 0.5, size=n); q = rng.normal(size=n)
        lam = rng.uniform(0.05, 2.0, size=ng) * 30.0 * np.sqrt(gs / 4.0)
        xd, sd, qd = _dev(x, sj, q)
        h = s.GroupNormL2.uniform(torch.from_numpy(lam).cuda(), gs)
        ref = orc.prox_group_l2_binf(q, x, sj, lam, sigma, delta, gsize=gs)
        offs = np.arange(0, n + 1, gs)
        y0 = s.prox(s.shifted(s.shifted(h, xd, delta, s.NormLinf(1.0)), sd), qd, sigma).cpu().numpy()
        v0 = _binf_check(orc, y0, ref, q, x, sj, lam, sigma, delta, offs, what="default gs=%d" % gs)
        try:
            s._lib.check(L.spx_ctx_set_tuning(ctx, 9, 1))
            y1 = s.prox(s.shifted(s.shifted(h, xd, delta, s.NormLinf(1.0)), sd), qd, sigma).cpu().numpy()
        finally:
            s._lib.check(L.spx_ctx_set_tuning(ctx, 9, 0))
        v1 = _binf_check(orc, y1, ref, q, x, sj, lam, sigma, delta, offs, what="reference-faithful gs=%d" % gs)
        scale = np.maximum(arbiter.group_scale(ref, q, x, sj, offs), 1e-300)
        d0, d1 = np.max(np.abs(y0 - ref) / scale), np.max(np.abs(y1 - ref) / scale)
        assert v0.n_checked > 0, ("the regime (roots next to the pole) must occur", v0)
        assert d1 <= d0 and v1.n_checked <= v0.n_checked, (gs, d0, d1, v0, v1)


# ------------------------------------------------------------------ device-resident values (round 2)
def test_values_into_a_device_double(s, orc):
    """spx_ctx_set_value_target: psi(y) and the value of prox_value land in the caller's device double, the call returns
    NaN on the host and reads nothing back; the number is bit-identical to the synchronous one, for every operator family
    (separable, Box incl. the +Inf of an infeasible point, IndBallL0(BInf), groups, NormL1B2)."""
    import torch
    n = 50_000
    x, sj, q = _data(n, 31)
    xd, sd, qd = _dev(x, sj, q)
    yd = _dev(np.random.default_rng(2).uniform(-0.3, 0.3, size=n))[0]
    lam_g = np.random.default_rng(3).uniform(0.5, 1.5, size=n // 50)
    chi = s.NormLinf(1.0)
    psis = [s.shifted(s.shifted(s.NormL1(0.7), xd), sd), s.shifted(s.shifted(s.NormL0(0.7), xd), sd),
            s.shifted(s.shifted(s.RootNormLhalf(0.7), xd), sd), s.shifted(s.shifted(s.NormL1(0.7), xd, 0.9, chi), sd),
            s.shifted(s.shifted(s.NormL0(0.7), xd, 0.9, chi), sd), s.shifted(s.shifted(s.RootNormLhalf(0.7), xd, 0.9, chi), sd),
            s.shifted(s.shifted(s.IndBallL0(n // 3), xd), sd), s.shifted(s.shifted(s.IndBallL0(n // 3), xd, 0.9, chi), sd),
            s.shifted(s.shifted(s.GroupNormL2.uniform(lam_g.tolist(), 50), xd), sd),
            s.shifted(s.shifted(s.GroupNormL2.uniform(lam_g.tolist(), 50), xd, 0.9, chi), sd),
            s.shifted(s.shifted(s.NormL1(0.7), xd, 50.0, s.NormL2(1.0)), sd)]
    out = torch.full((1,), -1.0, dtype=torch.float64, device="cuda:0")
    for psi in psis:
        for yy in (yd, yd * 10.0):                     # the second one is outside every box / ball: +Inf
            want = psi(yy)
            with s.device_values(out):
                got_host = psi(yy)
            assert got_host != got_host                # NaN: the host value is not produced
            got = float(out.item())
            assert got == want or (np.isinf(got) and np.isinf(want)), (type(psi).__name__, got, want)
        assert psi(yd) == psi(yd)                      # back to the synchronous form
    for psi in psis[:6]:                               # prox fused with the value
        y1, v1 = s.prox_value(psi, qd, 1.1)
        y1 = y1.clone()
        with s.device_values(out):
            y2, v2 = s.prox_value(psi, qd, 1.1)
        assert torch.equal(y1, y2) and v2 != v2 and float(out.item()) == v1, type(psi).__name__


def test_indball_l0_front_sample_sizes(s, orc):
    """The sample-predicted pipeline draws 1, 2 or 4 samples per lane of its front kernel (n below 2^23, below 2^25, beyond:
    csrc/spx_select.hip k_s2_front<SPL>); the full-size tests cover 4, most others 1 -- this one the size class in between,
    on continuous and on lattice data (ties), at both ends and in the middle of r."""
    n = (1 << 23) + 3
    rng = np.random.default_rng(823)
    for quant in (None, 16):
        x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
        if quant:
            x, sj, q = (np.round(v * quant) / quant for v in (x, sj, q))
        xd, sd, qd = _dev(x, sj, q)
        top = orc.TopR(q, x, sj)
        for r in (5, n // 100, n // 2, n - 1000):
            y = s.prox(s.shifted(s.shifted(s.IndBallL0(r), xd, 0.8, s.NormLinf(1.0)), sd), qd, 1.0).cpu().numpy()
            assert _bits_equal(y, top.prox(r, 0.8)), (quant, r)
