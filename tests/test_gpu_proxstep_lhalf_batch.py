"""GPU: batched RootNormLhalf(Box) prox! + step statistics with the per-problem scalars on the device
(spx_proxstep_lhalf[_box]_batch, spx_lhalf_threshold_batch: include/spx_lhalf_batch.h; prox_step_lhalf_batch[_bang],
lhalf_threshold_batch).

The layout, the sizes and the bars are those of tests/test_gpu_proxstep_batch.py, whose Problems / Layout are reused (imported,
not edited): problem b is row b of the batch x n tensors, every row is held to the SINGLE call (spx_proxstep_lhalf[_box] through
the C ABI) on that row alone with host copies of the scalars -- y and xkn bit for bit, the three sums within 1e-12 of the sum of
the magnitudes of the terms (math.fsum of the stored values, np.sqrt(|xkn|) for plane 0) -- and to the CPU oracle at the
project's l-half bar (arbiter.check_lhalf).

What is new is the threshold of the unboxed operator.  The single call forms p = 54^(1/3) (2 sigma lambda)^(2/3) / 4 with the
host's pow, the batched kernel forms it on the device; the two agree to 4 ulps (test_threshold_sweep...), and an element whose
a = |q_scale q + (xk + sj)| lies between them has the other branch of the prox's jump (test_band...).  Every test that demands
bits of the unboxed operator first asserts ON THE HOST that no element of its rows has |a - p_host| <= 4 ulp(p_host): a condition
on the inputs, which holds for these seeds."""
import math

import numpy as np
import pytest

import test_gpu_proxstep_batch as tb
from test_gpu_proxstep_batch import POISON, R, TILE, _P, _check_stats, _same_sum

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 513, 3071, 3072, 3073, R, R + 1, R + 3073]
BATCHES = [1, 2, 3, 7]
TOL = 1e-12
INVALID = 1
LHALF, BOX, BOXMASK = ("lhalf", False, False), ("lhalf", True, False), ("lhalf", True, True)
OPS = [LHALF, BOX, BOXMASK]
OP_IDS = ["lhalf", "lhalf-box", "lhalf-box-mask"]
SEED = 8100


@pytest.fixture(scope="module")
def s():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.build()


def p_host(lam, sig):
    """the single call's threshold: Python's pow is glibc's, which libspx.so's host code (RowLhalf::make) calls"""
    nl = float(sig) * float(lam)
    return 54.0 ** (1 / 3) * (2 * nl) ** (2 / 3) / 4


def a_of(q, xk, sj, qs):
    """|sol| as the functor rounds it (WithStep, OpLhalf): q_scale * q, xk + sj, their sum -- one rounding each"""
    return np.abs(qs * q + (xk + sj))


def assert_clear_of_threshold(q, xk, sj, lam, sig, qs, what=""):
    """no element within 4 ulps of the host's threshold: then (a <= p_host) == (a <= p_dev) for every element"""
    p = p_host(lam, sig)
    a = a_of(q, xk, sj, qs)
    with np.errstate(invalid="ignore"):
        near = np.abs(a - p) <= 4 * np.spacing(p)
    assert not near.any(), "%s: an input sits on the threshold (draw another seed): %r" % (what, np.flatnonzero(near)[:5])


class Problems(tb.Problems):
    """tb.Problems for RootNormLhalf: the h terms are square roots, the rows are clear of the threshold, and every row's single
    call is held to the CPU oracle once"""
    _cache = {}

    def __init__(self, s, n, seed, rows):
        super().__init__(s, n, seed, rows)
        for r in range(rows):
            assert_clear_of_threshold(self.Q[r], self.X[r], self.SJ[r], self.lam[r], self.sig[r], self.qs[r], "n=%d row %d" % (n, r))

    def sum_refs(self, op, r, y, v, q=None, lam=None):
        q = self.Q[r] if q is None else q
        lam = self.lam[r] if lam is None else lam
        sel = self.mask.astype(bool) if op[2] else np.ones(y.size, dtype=bool)
        hm = math.fsum(np.sqrt(np.abs(v[sel])))
        qy = q * y
        return lam * hm, lam * hm, math.fsum(qy), math.fsum(np.abs(qy)), math.fsum(y * y)

    def ref(self, op):
        first = op not in self.refs
        out = super().ref(op)
        if first and self.n * self.rows <= 200000:      # (the many-row and long-reduce problems check sampled rows themselves)
            for r in range(self.rows):
                check_oracle(op, out[0][r].cpu().numpy(), self.Q[r], self.X[r], self.SJ[r], self.lam[r], self.sig[r], self.qs[r],
                             self.dl[r], self.mask, "oracle n=%d row %d %s" % (self.n, r, op))
        return out


def check_oracle(op, y, q, xk, sj, lam, sig, qs, dl, mask, what):
    import arbiter
    from oracle import oracle
    qq = qs * q
    with np.errstate(all="ignore"):
        if op[1]:
            m = mask if op[2] else None
            ref = oracle.prox_lhalf_box(qq, xk, sj, float(lam), float(sig), -float(dl), float(dl), mask=m)
            arbiter.check_lhalf(oracle, y, ref, qq, xk, sj, float(lam), float(sig), box=(-float(dl), float(dl)), mask=m, what=what)
        else:
            ref = oracle.prox_lhalf(qq, xk, sj, float(lam), float(sig))
            arbiter.check_lhalf(oracle, y, ref, qq, xk, sj, float(lam), float(sig), what=what)


class Layout(tb.Layout):
    def call(self, s, op, xkn=True):
        kind, box, msk = op
        return s.prox_step_lhalf_batch_bang(self.Y, self.Q, self.X, self.S, self.lam, self.sig, self.qs,
                                            l=-self.dl if box else None, u=self.dl if box else None,
                                            selected=self.prob.maskd if msk else None, xkn=self.K if xkn else None, out=self.out)


def stationary(q, lam, sig):
    """the oracle's formula for the stationary point at sol = q (oracle/spx_oracle.c, src/shiftedRootNormLhalf.jl:48,57)"""
    nl = sig * lam
    phi = np.arccos(nl / 4 * (np.abs(q) / 3) ** -1.5)
    return 2.0 / 3.0 * q * (1 + np.cos(2 * np.pi / 3 - 2.0 / 3.0 * phi))


# ------------------------------------------------------------------ the threshold
def threshold_sweep(s):
    """one spx_lhalf_threshold_batch call over sigma lambda = m 2^k, k = -500 .. 500 in steps of 20, three m in [1, 2) per k,
    sigma lambda split between lambda and sigma so that neither overflows: [(k, m, p_host, p_dev, gap in ulps of p_host)]"""
    import torch
    from oracle import oracle
    rng = np.random.default_rng(SEED)
    ks = [k for k in range(-500, 501, 20) for _ in range(3)]
    ms = [m for _ in range(-500, 501, 20) for m in (1.0, 1.0 + float(rng.random()), 2.0 - 2.0 ** -52)]
    lam = np.array([m * 2.0 ** (k // 2) for k, m in zip(ks, ms)])
    sig = np.array([2.0 ** (k - k // 2) for k in ks])
    assert all(float(s_ * l_) == m * 2.0 ** k for s_, l_, k, m in zip(sig, lam, ks, ms))
    ph = np.array([p_host(l_, s_) for l_, s_ in zip(lam, sig)])
    # p_host is the oracle's p: at xk = sj = 0 its prox is 0 at q = p and not at the next double
    zero = np.zeros(2)
    for l_, s_, p in zip(lam, sig, ph):
        with np.errstate(all="ignore"):
            y = oracle.prox_lhalf(np.array([p, np.nextafter(p, np.inf)]), zero, zero, float(l_), float(s_))
        assert y[0] == 0.0 and y[1] != 0.0, (l_, s_, p, y)
    pd = s.lhalf_threshold_batch(torch.from_numpy(lam).cuda(), torch.from_numpy(sig).cuda()).cpu().numpy()
    gap = np.abs(pd - ph) / np.spacing(ph)
    return [(k, m, float(a), float(b), float(g)) for k, m, a, b, g in zip(ks, ms, ph, pd, gap)]


def test_threshold_sweep_is_within_4_ulps_of_the_host(s):
    rows = threshold_sweep(s)
    assert len(rows) == 153
    worst = max(rows, key=lambda r: r[4])
    print("largest |p_dev - p_host| = %g ulp at sigma lambda = %r * 2^%d (p_host %r, p_dev %r)" % (worst[4], worst[1], worst[0], worst[2], worst[3]))
    for k, m, ph, pd, g in rows:
        assert g <= 4.0, (k, m, ph, pd, g)


def test_threshold_call_refusals_and_empty(s):
    import torch
    L, G, ctx = s._lib.load(), s._lib.load_lhalf_batch(), s.context("cuda:0")
    lam = torch.full((5,), 0.7, dtype=torch.float64, device="cuda:0")
    sig = torch.full((5,), 1.1, dtype=torch.float64, device="cuda:0")
    out = torch.full((5,), POISON, dtype=torch.float64, device="cuda:0")
    for what, f in (("lambda NULL", lambda: G.spx_lhalf_threshold_batch(ctx, None, _P(sig), 5, _P(out))),
                    ("sigma NULL", lambda: G.spx_lhalf_threshold_batch(ctx, _P(lam), None, 5, _P(out))),
                    ("p_dev NULL", lambda: G.spx_lhalf_threshold_batch(ctx, _P(lam), _P(sig), 5, None)),
                    ("batch < 0", lambda: G.spx_lhalf_threshold_batch(ctx, _P(lam), _P(sig), -1, _P(out)))):
        assert f() == INVALID, what
        assert L.spx_last_error(), what
    assert G.spx_lhalf_threshold_batch(ctx, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((out == POISON).all())
    assert G.spx_lhalf_threshold_batch(ctx, _P(lam), _P(sig), 5, _P(out)) == 0      # the next call is right
    p = p_host(0.7, 1.1)
    assert bool((torch.abs(out - p) <= 4 * float(np.spacing(p))).all())
    assert s.lhalf_threshold_batch(lam[:0], sig[:0]).numel() == 0


# ------------------------------------------------------------------ parity with the single call
@pytest.mark.parametrize("n", SIZES)
def test_lhalf_batch_rows_equal_the_single_call(s, n):
    prob = Problems.get(s, n, SEED + n)
    for op in OPS:
        for batch in BATCHES:
            for pad in (0, 1, 2, 3):
                for off in (0, 1):
                    lay = Layout(prob, range(batch), pad, off)
                    lay.call(s, op)
                    lay.check(s, op, "%s n=%d batch=%d pad=%d off=%d" % (op, n, batch, pad, off))


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
def test_lhalf_batch_without_xkn(s, op):
    """xkn = None: y and the sums as with it"""
    import torch
    for n in (3073, R + 3073):
        prob = Problems.get(s, n, SEED + n)
        lay = Layout(prob, range(3), 1, 0)
        lay.call(s, op, xkn=False)
        assert torch.equal(lay.Y, prob.ref(op)[0][:3]) and bool((lay.fk == POISON).all())
        got = lay.out.cpu().numpy()
        for b in range(3):
            _check_stats(op, got[b], prob.ref(op)[2][b], "no xkn n=%d row %d" % (n, b))


# ------------------------------------------------------------------ the band, planted
def _neighbours(p, k=6):
    out = [p]
    lo = hi = p
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


@pytest.mark.parametrize("n", [27, 3073, R + 3073])
def test_band_elements_take_the_branch_of_the_reported_threshold(s, n):
    """a row with xk = sj = 0 and q_scale = 1 among ordinary rows; its q carries +- the doubles from 6 below to 6 above p_host and
    p_dev (read back from the threshold call) at index 0, in the scalar tail and -- where there is one -- in the second tile:
    y == 0.0 exactly where |q| <= p_dev, elsewhere the stationary point to 1e-12 |q|.  (The branches are 0.67 p apart.)"""
    import torch
    prob = Problems.get(s, n, SEED + n)
    rng = np.random.default_rng(SEED + 50 + n)
    lam, sig = (float(v) for v in rng.uniform(0.3, 1.5, size=2))
    ph = p_host(lam, sig)
    pd = float(s.lhalf_threshold_batch(torch.tensor([lam], dtype=torch.float64, device="cuda:0"),
                                       torch.tensor([sig], dtype=torch.float64, device="cuda:0")).cpu()[0])
    assert abs(pd - ph) <= 4 * np.spacing(ph)
    vals = sorted(set(_neighbours(ph) + _neighbours(pd)))
    vals = np.array([v if i % 2 == 0 else -v for i, v in enumerate(vals)])
    m = len(vals)
    assert 13 <= m <= 17
    q = rng.normal(size=n)
    q[np.abs(np.abs(q) - ph) < 1e-6] = 0.25 * ph       # (the ordinary elements of the row stay away from the jump)
    if n == 27:
        q[n - 10:] = -vals[:10][::-1]                   # (n is odd: the last element is a row's scalar tail)
        q[:m] = vals
        planted = np.r_[0:m, n - 10:n]
    else:
        q[:m] = vals
        q[n - m:] = -vals
        planted = np.r_[0:m, n - m:n]                   # (n = 3073: the last planted elements ARE the second tile)
        if n > 2 * TILE:
            q[TILE + 5:TILE + 5 + m] = vals[::-1]
            planted = np.r_[planted, TILE + 5:TILE + 5 + m]
    for pad, off in ((1, 0), (0, 1), (2, 1)):
        lay = Layout(prob, range(3), pad, off)
        lay.Q[1].copy_(torch.from_numpy(q)); lay.X[1].zero_(); lay.S[1].zero_()
        lay.lam[1], lay.sig[1], lay.qs[1] = lam, sig, 1.0
        lay.call(s, LHALF)
        lay.padding_untouched()
        y = lay.Y[1].cpu().numpy()
        k = lay.K[1].cpu().numpy()
        zero = np.abs(q) <= pd
        assert zero[planted].any() and (~zero[planted]).any()
        assert np.all(y[zero] == 0.0), (n, pad, off, np.flatnonzero(zero & (y != 0.0))[:5])
        st = stationary(q[~zero], lam, sig)
        assert np.all(np.abs(y[~zero] - st) <= TOL * np.abs(q[~zero])), (n, pad, off)
        assert np.array_equal(k, y)                                   # xkn = (0 + 0) + y
        got = lay.out[1].cpu().numpy()                                # the sums are those of the stored y
        _check_stats(LHALF, got, (lam * math.fsum(np.sqrt(np.abs(k))), lam * math.fsum(np.sqrt(np.abs(k))), math.fsum(q * y),
                                  math.fsum(np.abs(q * y)), math.fsum(y * y)), "band row")
        for b in (0, 2):                                              # the ordinary rows keep the single call's bits
            assert torch.equal(lay.Y[b], prob.ref(LHALF)[0][b]) and torch.equal(lay.K[b], prob.ref(LHALF)[1][b]), (n, b)


# ------------------------------------------------------------------ padding and ends
@pytest.mark.parametrize("n", [3, 3073, R + 1])
def test_lhalf_batch_guard_bands_and_padding(s, n):
    """y and xkn between guard bands, poison everywhere: after the call the guard bands (and the inputs) are unchanged, every
    padding element still holds the poison and no row element does"""
    prob = Problems.get(s, n, SEED + n)
    for op in OPS:
        for batch, pad, off in ((1, 3, 1), (3, 0, 1), (3, 1, 0), (7, 3, 0)):
            lay = Layout(prob, range(batch), pad, off, guarded=True)
            lay.call(s, op)
            lay.zone.check()     # guard bands of y, xkn, q, xk, sj
            for g in lay.zone.bufs[2:]:   # q, xk, sj: read only
                assert bool((g.buf == g.snap).all()), g.name
            lay.check(s, op, "guarded %s n=%d batch=%d pad=%d off=%d" % (op, n, batch, pad, off))
    # the element-wise forms
    lay = Layout(prob, range(3), 1, 0, xkn_off=1, guarded=True)
    lay.call(s, BOXMASK)
    lay.zone.check()
    lay.check(s, BOXMASK, "guarded element-wise n=%d" % n)


# ------------------------------------------------------------------ placement independence, reproducibility
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("n", [513, 3073, R + 3073])
def test_lhalf_batch_bits_do_not_depend_on_placement(s, op, n):
    """the same problem at row 0 of batch 1, row 2 of batch 3, row 6 of batch 7 (rows of one parity, same ld, same bases): the
    same bits in y, xkn and the three sums"""
    import torch
    prob = Problems.get(s, n, SEED + n)
    for pad, off in ((1, 0), (2, 1)):
        seen = None
        for rows, at in (([4], 0), ([0, 1, 4], 2), ([0, 1, 2, 3, 5, 6, 4], 6)):
            lay = Layout(prob, rows, pad, off)
            lay.call(s, op)
            cur = (lay.Y[at].clone(), lay.K[at].clone(), lay.out[at].clone())
            if seen is not None:
                assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(seen, cur)), (op, n, pad, off, at)
            seen = cur


@pytest.mark.parametrize("n", [3073, R + 3073])
def test_lhalf_batch_sums_are_reproducible(s, n):
    import torch
    prob = Problems.get(s, n, SEED + n)
    for op in OPS:
        a, b = Layout(prob, range(7), 1, 1), Layout(prob, range(7), 1, 1)
        a.call(s, op); b.call(s, op); a.call(s, op)
        assert torch.equal(a.out.view(torch.int64), b.out.view(torch.int64)), (op, n)
        assert torch.equal(a.Y, b.Y) and torch.equal(a.K, b.K), (op, n)


# ------------------------------------------------------------------ more problems than CUs, more than 65535 rows
@pytest.mark.parametrize("batch,n", [(300, 5), (70001, 3)])
def test_lhalf_batch_many_rows(s, batch, n):
    import torch
    prob = Problems.get(s, n, SEED + 200 + batch, rows=batch)
    rng = np.random.default_rng(batch)
    rows = sorted({0, batch - 1} | set(rng.choice(batch, size=40, replace=False).tolist()))
    for op in (LHALF, BOXMASK):
        for pad, off in ((0, 0), (1, 1)):
            lay = Layout(prob, range(batch), pad, off)
            lay.call(s, op)
            lay.padding_untouched()
            got = lay.out.cpu().numpy()
            for r in rows:
                y, k, _ = prob.single(op, r)
                assert torch.equal(lay.Y[r], y) and torch.equal(lay.K[r], k), (op, batch, r)
                _check_stats(op, got[r], prob.sum_refs(op, r, y.cpu().numpy(), k.cpu().numpy()), "%s batch=%d row %d" % (op, batch, r))


def test_lhalf_batch_more_partials_than_one_pass_adds(s):
    """n = 2048 tiles + 1 element: the per-problem reduction takes its long loop (more than 2048 partials a plane)"""
    import torch
    n = 2048 * TILE + 1
    prob = Problems.get(s, n, SEED + 300, rows=2)
    op = BOX
    lay = Layout(prob, range(2), 1, 0)
    lay.call(s, op)
    lay.padding_untouched()
    got = lay.out.cpu().numpy()
    for r in range(2):
        y, k, st = prob.single(op, r)
        assert torch.equal(lay.Y[r], y) and torch.equal(lay.K[r], k), r
        if r == 1:
            _check_stats(op, got[r], prob.sum_refs(op, r, y.cpu().numpy(), k.cpu().numpy()), "long reduce row %d" % r)
    Problems._cache.pop((n, SEED + 300, 2))   # (a quarter of a gigabyte of rows)


# ------------------------------------------------------------------ mixed base alignment: the element-wise form
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("n", [3073, R + 3073])
def test_lhalf_batch_mixed_alignment_takes_the_elementwise_form(s, op, n):
    """xkn 8 bytes off while the others are aligned (and the reverse): the same y and xkn bits, the sums to the fsum bars"""
    prob = Problems.get(s, n, SEED + n)
    for off, xkn_off in ((0, 1), (1, 0)):
        for pad in (0, 1):
            lay = Layout(prob, range(3), pad, off, xkn_off=xkn_off)
            lay.call(s, op)
            lay.check(s, op, "mixed %s n=%d pad=%d off=%d/%d" % (op, n, pad, off, xkn_off))


# ------------------------------------------------------------------ isolation under non-finite data
def _equal_or_both_nan(a, b):
    import torch
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


@pytest.mark.parametrize("n", [3073, R + 3073])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), 1e150])
def test_lhalf_batch_nonfinite_row_is_isolated(s, n, value):
    """NaN, +Inf, 1e150 at element 0 and at the last element of ONE row's q in a batch of 3: that row is NaN where
    spx_proxstep_lhalf[_box] is NaN on it and equal elsewhere, the other rows keep the bits of the clean call"""
    import torch
    prob = Problems.get(s, n, SEED + n)
    for op in OPS:
        for pad, off in ((0, 0), (1, 1)):
            clean = Layout(prob, range(3), pad, off)
            clean.call(s, op)
            lay = Layout(prob, range(3), pad, off)
            lay.Q[1, 0] = value
            lay.Q[1, n - 1] = value
            lay.call(s, op)
            lay.padding_untouched()
            y, k, st = prob.single(op, 1, q=lay.Q[1].clone())
            what = (op, n, value, pad, off)
            assert _equal_or_both_nan(lay.Y[1], y) and _equal_or_both_nan(lay.K[1], k), what
            assert torch.equal(torch.isnan(lay.Y[1]), torch.isnan(y)), what
            got = lay.out[1].cpu().numpy()
            yh, kh, qh = y.cpu().numpy(), k.cpu().numpy(), lay.Q[1].cpu().numpy()
            sel = prob.mask.astype(bool) if op[2] else np.ones(n, dtype=bool)
            with np.errstate(all="ignore"):
                mags = (prob.lam[1] * np.sum(np.sqrt(np.abs(kh[sel]))), np.sum(np.abs(qh * yh)), np.sum(yh * yh))
            for j in range(3):
                assert _same_sum(float(got[j]), st[j], mags[j]), (what, j, got[j], st[j])
            for b in (0, 2):
                assert torch.equal(lay.Y[b], clean.Y[b]) and torch.equal(lay.K[b], clean.K[b]), what
                assert torch.equal(lay.out[b].view(torch.int64), clean.out[b].view(torch.int64)), what


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
def test_nan_lambda_touches_its_row_only(s, op):
    import torch
    n = 3073
    prob = Problems.get(s, n, SEED + n)
    clean = Layout(prob, range(3), 1, 0)
    clean.call(s, op)
    lay = Layout(prob, range(3), 1, 0)
    lay.lam[1] = float("nan")
    lay.call(s, op)
    lay.padding_untouched()
    assert math.isnan(float(lay.out[1, 0]))
    for b in (0, 2):
        assert torch.equal(lay.Y[b], clean.Y[b]) and torch.equal(lay.K[b], clean.K[b]), (op, b)
        assert torch.equal(lay.out[b].view(torch.int64), clean.out[b].view(torch.int64)), (op, b)


# ------------------------------------------------------------------ refusals and empties
def test_lhalf_batch_refusals_and_empties(s):
    import torch
    n, batch = 513, 3
    prob = Problems.get(s, n, SEED + n)
    L, B, ctx = s._lib.load(), s._lib.load_lhalf_batch(), s.context("cuda:0")
    lay = Layout(prob, range(batch), 1, 0)
    ld = lay.ld
    y, q, xk, sj, k = (_P(f) for f in (lay.fy, lay.fq, lay.fx, lay.fs, lay.fk))
    lam, sig, qs, lo, up, out = _P(lay.lam), _P(lay.sig), _P(lay.qs), _P(-lay.dl), _P(lay.dl), _P(lay.out)
    keep = (-lay.dl, lay.dl)
    Z = None

    def plain(y=y, q=q, xk=xk, sj=sj, n=n, batch=batch, ld=ld, lam=lam, sig=sig, qs=qs, k=k, out=out):
        return B.spx_proxstep_lhalf_batch(ctx, y, q, xk, sj, n, batch, ld, lam, sig, qs, k, out)

    def box(lo=lo, up=up, **kw):
        a = dict(y=y, q=q, xk=xk, sj=sj, n=n, batch=batch, ld=ld, lam=lam, sig=sig, qs=qs, k=k, out=out); a.update(kw)
        return B.spx_proxstep_lhalf_box_batch(ctx, a["y"], a["q"], a["xk"], a["sj"], a["n"], a["batch"], a["ld"], a["lam"], a["sig"], lo, up,
                                              _P(prob.maskd), a["qs"], a["k"], a["out"])

    def untouched():
        torch.cuda.synchronize()
        return bool((lay.fy == POISON).all()) and bool((lay.fk == POISON).all()) and bool((lay.out == POISON).all())

    def next_call_is_right():
        assert plain() == 0
        lay.check(s, LHALF, "after a refusal")
        lay.fy.fill_(POISON); lay.fk.fill_(POISON); lay.out.fill_(POISON)

    refusals = [
        ("y == q", lambda: plain(y=q)), ("xkn == y", lambda: plain(k=y)), ("xkn == q", lambda: plain(k=q)),
        ("xkn == xk", lambda: plain(k=xk)), ("xkn == sj", lambda: plain(k=sj)), ("ld < n", lambda: plain(ld=n - 1)),
        ("batch < 0", lambda: plain(batch=-1)), ("n < 0", lambda: plain(n=-1)), ("lambda NULL", lambda: plain(lam=Z)),
        ("sigma NULL", lambda: plain(sig=Z)), ("q_scale NULL", lambda: plain(qs=Z)), ("stats_dev NULL", lambda: plain(out=Z)),
        ("l NULL", lambda: box(lo=Z)), ("u NULL", lambda: box(up=Z)), ("box: y == q", lambda: box(y=q)),
        ("box: xkn == mask", lambda: box(k=_P(prob.maskd))),
        ("2^31 workgroups", lambda: plain(n=1, ld=1, batch=1 << 31)),
        ("2^31 workgroups, tiled", lambda: plain(n=R + 1, ld=R + 1, batch=((1 << 31) - 1) // 5 + 1)),
    ]
    for what, f in refusals:
        assert f() == INVALID, what
        assert L.spx_last_error(), what
        assert untouched(), what
        next_call_is_right()
    # empties: batch == 0 does nothing; n == 0 stores 3 * batch zeros (by a kernel)
    assert plain(batch=0) == 0 and box(batch=0) == 0 and untouched()
    assert plain(batch=0, lam=Z, out=Z) == 0 and untouched()
    next_call_is_right()
    assert plain(n=0, ld=0) == 0
    torch.cuda.synchronize()
    assert bool((lay.out == 0.0).all()) and bool((lay.fy == POISON).all()) and bool((lay.fk == POISON).all())
    lay.out.fill_(POISON)
    assert box(n=0, ld=5) == 0
    torch.cuda.synchronize()
    assert bool((lay.out == 0.0).all()) and bool((lay.fy == POISON).all())
    lay.out.fill_(POISON)
    next_call_is_right()
    # the mirror refuses what it can see
    with pytest.raises(TypeError):
        s.prox_step_lhalf_batch_bang(lay.Y, lay.Y, lay.X, lay.S, lay.lam, lay.sig, lay.qs)
    with pytest.raises(TypeError):
        s.prox_step_lhalf_batch_bang(lay.Y, lay.Q, lay.X, lay.S, lay.lam[:2], lay.sig, lay.qs)
    with pytest.raises(TypeError):
        s.prox_step_lhalf_batch_bang(lay.Y, lay.Q, lay.X, lay.S, lay.lam, lay.sig, lay.qs, l=keep[0])
    with pytest.raises(TypeError):
        s.prox_step_lhalf_batch_bang(lay.Y, lay.Q, lay.X, lay.S, lay.lam, lay.sig, lay.qs, selected=prob.maskd)
    with pytest.raises(TypeError):
        s.prox_step_lhalf_batch_bang(lay.Y, lay.Q.contiguous(), lay.X, lay.S, lay.lam, lay.sig, lay.qs)   # another row stride
    Yn, outn = s.prox_step_lhalf_batch(lay.Q, lay.X, lay.S, lay.lam, lay.sig, lay.qs)
    assert torch.equal(Yn, prob.ref(LHALF)[0][:batch]) and Yn.stride() == lay.Q.stride() and tuple(outn.shape) == (batch, 3)


# ------------------------------------------------------------------ the parameters follow the device
@pytest.mark.parametrize("n", [3073, R + 3073])
def test_captured_lhalf_batch_call_follows_the_device_parameters(s, n):
    """one batched call captured into a graph (side stream, warm-up first: the tiled form reserves its workspace there);
    between replays lambda, sigma and q_scale (and the box) are overwritten ON THE DEVICE: every replay's rows equal the single
    call with the NEW scalars, bit for bit"""
    import torch
    prob = Problems.get(s, n, SEED + n)
    rng = np.random.default_rng(SEED + 400 + n)
    for op in (LHALF, BOXMASK):
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            lay = Layout(prob, range(3), 1, 0)
            if op[1]:
                lay.lo, lay.up = -lay.dl, lay.dl.clone()

            def call():
                kind, box, msk = op
                s.prox_step_lhalf_batch_bang(lay.Y, lay.Q, lay.X, lay.S, lay.lam, lay.sig, lay.qs, l=lay.lo if box else None,
                                             u=lay.up if box else None, selected=prob.maskd if msk else None, xkn=lay.K, out=lay.out)
            call(); call()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call()
        for rep in range(3):
            lam, sig, qs, dl = (rng.uniform(0.3, 1.5, size=3) for _ in range(4))
            if not op[1]:
                for b in range(3):
                    assert_clear_of_threshold(prob.Q[b], prob.X[b], prob.SJ[b], lam[b], sig[b], qs[b], "replay %d row %d" % (rep, b))
            lay.lam.copy_(torch.from_numpy(lam)); lay.sig.copy_(torch.from_numpy(sig)); lay.qs.copy_(torch.from_numpy(qs))
            if op[1]:
                lay.lo.copy_(torch.from_numpy(-dl)); lay.up.copy_(torch.from_numpy(dl))
            lay.fy.fill_(POISON); lay.fk.fill_(POISON); lay.out.fill_(POISON)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            lay.padding_untouched()
            got = lay.out.cpu().numpy()
            for b in range(3):
                y, k, _ = prob.single(op, b, scal=(lam[b], sig[b], qs[b], dl[b]))
                what = (op, n, rep, b)
                assert torch.equal(lay.Y[b], y) and torch.equal(lay.K[b], k), what
                _check_stats(op, got[b], prob.sum_refs(op, b, y.cpu().numpy(), k.cpu().numpy(), lam=lam[b]), str(what))


# ------------------------------------------------------------------ scales
def test_lhalf_batch_rows_at_the_scales_of_the_family(s):
    """the RootNormLhalf(Box) problems of tests/scales.py (n = 1001; scalar bounds, with and without the mask) as the rows of ONE
    batched call, one row per exponent the file allows for the family (K64, all even): every row against the oracle on the scaled
    problem at the l-half bar; an element of the unboxed form in the band between the two thresholds may have the other branch"""
    import torch
    import arbiter
    import scales
    from oracle import oracle
    ks = [k for k in scales.K64 if k % 2 == 0]
    n = 1001
    for opname, masked in (("prox_lhalf", False), ("prox_lhalf_box", False), ("prox_lhalf_box", True)):
        P0 = scales.separable(opname, n, masked=masked)
        Ps = []
        for k in ks:
            scales.assert_in_range(P0, k)
            Ps.append(scales.scaled(P0, k))
        dev = lambda rows: torch.from_numpy(np.ascontiguousarray(np.stack(rows))).cuda()
        Q, X, S = dev([P.q for P in Ps]), dev([P.xk for P in Ps]), dev([P.sj for P in Ps])
        lam = dev([np.float64(P.lam) for P in Ps]); sig = dev([np.float64(P.sigma) for P in Ps])
        qs = torch.ones(len(Ps), dtype=torch.float64, device="cuda:0")
        box = opname.endswith("_box")
        kw = {}
        if box:
            kw = dict(l=dev([np.float64(P.l) for P in Ps]), u=dev([np.float64(P.u) for P in Ps]),
                      selected=torch.from_numpy(P0.mask.copy()).cuda() if masked else None)
        K = torch.empty_like(Q)
        Y, out = s.prox_step_lhalf_batch(Q, X, S, lam, sig, qs, xkn=K, **kw)
        pd = s.lhalf_threshold_batch(lam, sig).cpu().numpy()
        Yh, Kh, oh = Y.cpu().numpy(), K.cpu().numpy(), out.cpu().numpy()
        for b, (k, P) in enumerate(zip(ks, Ps)):
            what = "%s%s at 2^%d" % (opname, " masked" if masked else "", k)
            ref = scales.oracle_y(oracle, P)
            y = Yh[b].copy()
            if not box:
                ph = p_host(P.lam, P.sigma)
                assert abs(pd[b] - ph) <= 4 * np.spacing(ph), what
                a = a_of(P.q, P.xk, P.sj, 1.0)
                band = (a <= ph) != (a <= pd[b])
                xs = P.xk + P.sj
                for i in np.flatnonzero(band):       # the other branch, exactly or to the bar; then out of the comparison
                    if a[i] <= pd[b]:
                        assert y[i] == 0.0 - xs[i], (what, i)
                    else:
                        st = stationary(np.array([P.q[i] + xs[i]]), P.lam, P.sigma)[0] - xs[i]
                        assert abs(y[i] - st) <= TOL * max(abs(y[i]), abs(xs[i]), abs(P.q[i])), (what, i)
                    y[i] = ref[i]
            with np.errstate(all="ignore"):
                arbiter.check_lhalf(oracle, y, ref, P.q, P.xk, P.sj, P.lam, P.sigma, box=(P.l, P.u) if box else None, mask=P.mask, what=what)
            assert np.array_equal(Kh[b], (P.xk + P.sj) + Yh[b]), what
            sel = P.mask.astype(bool) if P.mask is not None else np.ones(n, dtype=bool)
            hm = float(P.lam) * math.fsum(np.sqrt(np.abs(Kh[b][sel])))
            qy = P.q * Yh[b]
            _check_stats(("lhalf", box, masked), oh[b], (hm, hm, math.fsum(qy), math.fsum(np.abs(qy)), math.fsum(Yh[b] * Yh[b])), what)
