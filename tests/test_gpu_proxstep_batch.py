"""GPU: batched prox! + step statistics with the per-problem scalars on the device (spx_proxstep_{l1,l0}[_box]_batch,
prox_step_batch / prox_step_batch_bang).

Problem b is row b of the batch x n tensors (row stride ld >= n); lambda_b, sigma_b, q_scale_b and the box [-Delta_b, Delta_b]
are read from device arrays by the kernel that stores y.  Every row is held to the SINGLE call (spx_proxstep_X through the C
ABI) on that row alone with the host copies of the scalars: y and xkn bit for bit (torch.equal), the three sums to the project's
bars for these blocked sums (test_gpu_proxstep.py: NormL0's [0] exactly lambda_b * count; else |got - ref| <= 1e-12 * sum of
the magnitudes of the terms, ref = math.fsum of the host's rounded terms -- the library is built without contraction).

Sizes sit at the edges of the kernels: a tile is 3072 elements (256 lanes x 6 pairs), one workgroup owns a problem up to
R = kBatchRowMax = 12288 elements (the row form), beyond it one workgroup takes one tile and a second launch adds the
partials (the tiled form).  A row is peeled by the parity of b * ld plus the bases' alignment: head of 0 / 1 elements, pairs,
tail of 0 / 1 -- so ld - n in {0, 1, 2, 3} and bases on / 8 bytes off a 16-byte boundary reach every combination.
The scalars are drawn from U(0.3, 1.5): every 2 lambda sigma is a non-trivial square-root argument, which is what holds the
device's Float64 sqrt (NormL0's threshold) to the host's."""
import ctypes
import math

import numpy as np
import pytest

import redzone

pytestmark = pytest.mark.gpu

R = 12288
TILE = 3072
SIZES = [1, 2, 3, 511, 512, 513, 3071, 3072, 3073, R - 1, R, R + 1, R + 3073]
BATCHES = [1, 2, 3, 7]
TOL = 1e-12
INVALID = 1
POISON = -777.25
# (kind, box, mask): the four operators, the box forms with and without a mask
OPS = [("l1", False, False), ("l0", False, False), ("l1", True, False), ("l1", True, True), ("l0", True, False), ("l0", True, True)]
OP_IDS = ["%s%s%s" % (k, "-box" if b else "", "-mask" if m else "") for k, b, m in OPS]


@pytest.fixture(scope="module")
def s():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.build()


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)


class Problems:
    """`rows` problems of n elements (data as _data of test_gpu_proxstep.py, one draw per row), their scalars, one shared mask,
    and -- computed once per operator, shared by every test that places these rows somewhere -- what the single call gives on
    each row: y, xkn (device, rows x n) and the reference sums."""
    _cache = {}

    @classmethod
    def get(cls, s, n, seed, rows=7):
        key = (n, seed, rows)
        if key not in cls._cache:
            cls._cache[key] = cls(s, n, seed, rows)
        return cls._cache[key]

    def __init__(self, s, n, seed, rows):
        import torch
        rng = np.random.default_rng(seed)
        self.s, self.n, self.rows = s, n, rows
        self.X = rng.normal(size=(rows, n))
        self.SJ = rng.uniform(-0.5, 0.5, size=(rows, n))
        self.Q = rng.normal(size=(rows, n))
        self.lam, self.sig, self.qs, self.dl = (rng.uniform(0.3, 1.5, size=rows) for _ in range(4))
        self.mask = np.zeros(n, dtype=np.uint8)
        self.mask[rng.choice(n, size=max(1, n // 3), replace=False)] = 1
        self.Xd, self.SJd, self.Qd = (torch.from_numpy(a).cuda() for a in (self.X, self.SJ, self.Q))
        self.maskd = torch.from_numpy(self.mask).cuda()
        self.refs = {}

    def single(self, op, r, q=None, xk=None, sj=None, scal=None):
        """spx_proxstep_X on row r alone (or on the given vectors / (lam, sig, qs, dl)): (y, xkn, [h, qy, yy])"""
        import torch
        s = self.s
        kind, box, msk = op
        L, ctx = s._lib.load(), s.context("cuda:0")
        q = self.Qd[r] if q is None else q
        xk = self.Xd[r] if xk is None else xk
        sj = self.SJd[r] if sj is None else sj
        lam, sig, qs, dl = scal if scal is not None else (self.lam[r], self.sig[r], self.qs[r], self.dl[r])
        n = q.numel()
        y, k = torch.full_like(q, POISON), torch.full_like(q, POISON)
        st = (ctypes.c_double * 3)()
        if box:
            rc = getattr(L, "spx_proxstep_%s_box" % kind)(ctx, _P(y), _P(q), _P(xk), _P(sj), n, float(lam), float(sig), None, None,
                                                          -float(dl), float(dl), _P(self.maskd) if msk else None, float(qs), _P(k), st, None)
        else:
            rc = getattr(L, "spx_proxstep_" + kind)(ctx, _P(y), _P(q), _P(xk), _P(sj), n, float(lam), float(sig), float(qs), _P(k), st, None)
        assert rc == 0, s._lib.load().spx_last_error()
        return y, k, [st[0], st[1], st[2]]

    def ref(self, op):
        """per operator: (Y rows x n, XKN rows x n on the device, [(h_ref, h_mag, qy_ref, qy_mag, yy_ref)] per row)"""
        import torch
        if op not in self.refs:
            ys, ks, sums = [], [], []
            for r in range(self.rows):
                y, k, _ = self.single(op, r)
                ys.append(y); ks.append(k)
                sums.append(self.sum_refs(op, r, y.cpu().numpy(), k.cpu().numpy()))
            self.refs[op] = (torch.stack(ys), torch.stack(ks), sums)
        return self.refs[op]

    def sum_refs(self, op, r, y, v, q=None, lam=None):
        """exactly rounded references from the host copies: v = (xk + sj) + y as stored"""
        kind, box, msk = op
        q = self.Q[r] if q is None else q
        lam = self.lam[r] if lam is None else lam
        sel = self.mask.astype(bool) if msk else np.ones(y.size, dtype=bool)
        if kind == "l0":
            h = lam * float(np.count_nonzero(v[sel]))
            hm = 0.0
        else:
            hm = math.fsum(np.abs(v[sel]))
            h = lam * hm
        qy = q * y
        return h, lam * hm, math.fsum(qy), math.fsum(np.abs(qy)), math.fsum(y * y)


def _check_stats(op, got, ref, what):
    h, hm, qy, mqy, yy = ref
    g0, g1, g2 = (float(v) for v in got)
    if op[0] == "l0":
        assert g0 == h, (what, g0, h)
    else:
        assert abs(g0 - h) <= TOL * max(hm, 1e-300), (what, g0, h)
    assert abs(g1 - qy) <= TOL * mqy, (what, g1, qy, mqy)
    assert abs(g2 - yy) <= TOL * yy, (what, g2, yy)


class Layout:
    """the five batch x n tensors of a call as views of flat poisoned buffers: row stride ld = n + pad, bases `off` (0 / 1)
    elements past a 256-byte boundary (xkn: xkn_off), rows = the problem rows placed at batch rows 0, 1, ..."""

    def __init__(self, prob, rows, pad, off, xkn_off=None, guarded=False):
        import torch
        self.prob, self.rows, self.n, self.batch = prob, list(rows), prob.n, len(rows)
        self.ld = ld = prob.n + pad
        xkn_off = off if xkn_off is None else xkn_off
        total = self.batch * ld
        self.zone = redzone.Zone() if guarded else None

        def flat(o, name):
            if guarded:   # [front guard | batch * ld elements | back guard], poison everywhere
                return self.zone.add(total, torch.float64, align_bytes=8 * o, role="inout", poison=POISON, name=name,
                                     data=torch.full((total,), POISON, dtype=torch.float64)).t
            return torch.full((total + 2,), POISON, dtype=torch.float64, device="cuda:0")[o:o + total]

        self.fy, self.fk = flat(off, "y"), flat(xkn_off, "xkn")
        self.fq, self.fx, self.fs = flat(off, "q"), flat(off, "xk"), flat(off, "sj")
        view = lambda f: f.as_strided((self.batch, self.n), (ld, 1))
        self.Y, self.K, self.Q, self.X, self.S = (view(f) for f in (self.fy, self.fk, self.fq, self.fx, self.fs))
        idx = torch.as_tensor(self.rows, device="cuda:0")
        self.Q.copy_(prob.Qd[idx]); self.X.copy_(prob.Xd[idx]); self.S.copy_(prob.SJd[idx])
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[self.rows])).cuda()
        self.lam, self.sig, self.qs, self.dl = dev(prob.lam), dev(prob.sig), dev(prob.qs), dev(prob.dl)
        self.out = torch.full((self.batch, 3), POISON, dtype=torch.float64, device="cuda:0")
        if guarded:
            for g in self.zone.bufs:
                g.snap = g.buf.clone()   # (the inputs were copied in after the snapshot was taken)

    def call(self, s, op, xkn=True):
        kind, box, msk = op
        return s.prox_step_batch_bang(self.Y, kind, self.Q, self.X, self.S, self.lam, self.sig, self.qs,
                                      l=-self.dl if box else None, u=self.dl if box else None,
                                      selected=self.prob.maskd if msk else None, xkn=self.K if xkn else None, out=self.out)

    def padding_untouched(self):
        """every element [b ld + n, (b + 1) ld) of y and xkn still holds the poison, and no row element does"""
        import torch
        for f, V in ((self.fy, self.Y), (self.fk, self.K)):
            whole = f.as_strided((self.batch, self.ld), (self.ld, 1))
            assert bool((whole[:, self.n:] == POISON).all()), "padding written"
            assert not bool((V == POISON).any()), "row element not written"

    def check(self, s, op, what, stats=True):
        import torch
        Yr, Kr, sums = self.prob.ref(op)
        idx = torch.as_tensor(self.rows, device="cuda:0")
        assert torch.equal(self.Y, Yr[idx]), what
        assert torch.equal(self.K, Kr[idx]), what
        self.padding_untouched()
        if stats:
            got = self.out.cpu().numpy()
            for b, r in enumerate(self.rows):
                _check_stats(op, got[b], sums[r], "%s row %d" % (what, b))


# ------------------------------------------------------------------ parity with the single call
@pytest.mark.parametrize("n", SIZES)
def test_batch_rows_equal_the_single_call(s, n):
    prob = Problems.get(s, n, 7100 + n)
    for op in OPS:
        for batch in BATCHES:
            for pad in (0, 1, 2, 3):
                for off in (0, 1):
                    lay = Layout(prob, range(batch), pad, off)
                    lay.call(s, op)
                    lay.check(s, op, "%s n=%d batch=%d pad=%d off=%d" % (op, n, batch, pad, off))


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
def test_batch_without_xkn(s, op):
    """xkn = None: y and the sums as with it"""
    import torch
    for n in (3073, R + 3073):
        prob = Problems.get(s, n, 7100 + n)
        lay = Layout(prob, range(3), 1, 0)
        lay.call(s, op, xkn=False)
        assert torch.equal(lay.Y, prob.ref(op)[0][:3]) and bool((lay.fk == POISON).all())
        got = lay.out.cpu().numpy()
        for b in range(3):
            _check_stats(op, got[b], prob.ref(op)[2][b], "no xkn n=%d row %d" % (n, b))


# ------------------------------------------------------------------ padding and ends
@pytest.mark.parametrize("n", [1, 3, 513, 3073, R + 1])
def test_batch_guard_bands_and_padding(s, n):
    """y and xkn between guard bands, poison everywhere: after the call the guard bands (and the inputs) are unchanged, every
    padding element still holds the poison and no row element does"""
    prob = Problems.get(s, n, 7100 + n)
    for op in (OPS[0], OPS[5], OPS[3]):
        for batch, pad, off in ((1, 0, 0), (1, 3, 1), (3, 0, 1), (3, 1, 0), (3, 1, 1), (3, 2, 1), (7, 3, 0)):
            lay = Layout(prob, range(batch), pad, off, guarded=True)
            lay.call(s, op)
            lay.zone.check()     # guard bands of y, xkn, q, xk, sj
            for g in lay.zone.bufs[2:]:   # q, xk, sj: read only
                assert bool((g.buf == g.snap).all()), g.name
            lay.check(s, op, "guarded %s n=%d batch=%d pad=%d off=%d" % (op, n, batch, pad, off))


# ------------------------------------------------------------------ placement independence
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("n", [513, 3073, R + 3073])
def test_batch_bits_do_not_depend_on_placement(s, op, n):
    """the same problem at row 0 of batch 1, row 2 of batch 3, row 6 of batch 7 (rows of one parity, same ld, same bases): the
    same bits in y, xkn and the three sums"""
    import torch
    prob = Problems.get(s, n, 7100 + n)
    for pad, off in ((1, 0), (2, 1)):
        seen = None
        for rows, at in (([4], 0), ([0, 1, 4], 2), ([0, 1, 2, 3, 5, 6, 4], 6)):
            lay = Layout(prob, rows, pad, off)
            lay.call(s, op)
            cur = (lay.Y[at].clone(), lay.K[at].clone(), lay.out[at].clone())
            if seen is not None:
                assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(seen, cur)), (op, n, pad, off, at)
            seen = cur


# ------------------------------------------------------------------ more problems than CUs, more than 65535 rows
@pytest.mark.parametrize("batch,n", [(300, 5), (70001, 3)])
def test_batch_many_rows(s, batch, n):
    import torch
    prob = Problems.get(s, n, 7300 + batch, rows=batch)
    rng = np.random.default_rng(batch)
    rows = sorted({0, batch - 1} | set(rng.choice(batch, size=50, replace=False).tolist()))
    for op in (OPS[1], OPS[3]):
        for pad, off in ((0, 0), (1, 1)):
            lay = Layout(prob, range(batch), pad, off)
            lay.call(s, op)
            lay.padding_untouched()
            got = lay.out.cpu().numpy()
            for r in rows:
                y, k, _ = prob.single(op, r)
                assert torch.equal(lay.Y[r], y) and torch.equal(lay.K[r], k), (op, batch, r)
                _check_stats(op, got[r], prob.sum_refs(op, r, y.cpu().numpy(), k.cpu().numpy()), "%s batch=%d row %d" % (op, batch, r))


def test_batch_more_partials_than_one_pass_adds(s):
    """n = 2048 tiles + 1 element: the per-problem reduction takes its long loop (more than 2048 partials a plane)"""
    import torch
    n = 2048 * TILE + 1
    prob = Problems.get(s, n, 7400, rows=2)
    op = OPS[2]
    lay = Layout(prob, range(2), 1, 0)
    lay.call(s, op)
    lay.padding_untouched()
    got = lay.out.cpu().numpy()
    for r in range(2):
        y, k, st = prob.single(op, r)
        assert torch.equal(lay.Y[r], y) and torch.equal(lay.K[r], k), r
        if r == 1:
            _check_stats(op, got[r], prob.sum_refs(op, r, y.cpu().numpy(), k.cpu().numpy()), "long reduce row %d" % r)
    Problems._cache.pop((n, 7400, 2))   # (half a gigabyte of rows)


# ------------------------------------------------------------------ mixed base alignment: the element-wise form
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("n", [3073, R + 3073])
def test_batch_mixed_alignment_takes_the_elementwise_form(s, op, n):
    """xkn 8 bytes off while the others are aligned (and the reverse): the same y and xkn bits, the sums to the fsum bars"""
    prob = Problems.get(s, n, 7100 + n)
    for off, xkn_off in ((0, 1), (1, 0)):
        for pad in (0, 1):
            lay = Layout(prob, range(3), pad, off, xkn_off=xkn_off)
            lay.call(s, op)
            lay.check(s, op, "mixed %s n=%d pad=%d off=%d/%d" % (op, n, pad, off, xkn_off))


# ------------------------------------------------------------------ isolation under non-finite data
def _same_sum(a, b, mag):
    """two sums of the same terms added in different orders (include/spx.h, non-finite data)"""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= 2 * TOL * mag     # (each within TOL * mag of the exact sum)


@pytest.mark.parametrize("n", [3073, R + 3073])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), 1e150])
def test_batch_nonfinite_row_is_isolated(s, n, value):
    """NaN, +Inf, 1e150 at element 0 and in the tail of ONE row of a batch of 3: that row behaves as spx_proxstep_X does on it,
    the other rows keep the bits of the clean call"""
    import torch
    prob = Problems.get(s, n, 7100 + n)
    for op in (OPS[0], OPS[3], OPS[5]):
        for pad, off in ((0, 0), (1, 1)):
            clean = Layout(prob, range(3), pad, off)
            clean.call(s, op)
            for where in ("q", "xk", "sj"):
                lay = Layout(prob, range(3), pad, off)
                t = {"q": lay.Q, "xk": lay.X, "sj": lay.S}[where]
                t[1, 0] = value
                t[1, n - 1] = value
                lay.call(s, op)
                lay.padding_untouched()
                y, k, st = prob.single(op, 1, q=lay.Q[1].clone(), xk=lay.X[1].clone(), sj=lay.S[1].clone())
                what = (op, n, value, where, pad, off)
                assert torch.equal(lay.Y[1].view(torch.int64), y.view(torch.int64)), what
                assert torch.equal(lay.K[1].view(torch.int64), k.view(torch.int64)), what
                got = lay.out[1].cpu().numpy()
                yh, kh, qh = y.cpu().numpy(), k.cpu().numpy(), lay.Q[1].cpu().numpy()
                sel = prob.mask.astype(bool) if op[2] else np.ones(n, dtype=bool)
                with np.errstate(all="ignore"):
                    mags = (prob.lam[1] * np.sum(np.abs(kh[sel])) if op[0] == "l1" else 0.0, np.sum(np.abs(qh * yh)), np.sum(yh * yh))
                for j in range(3):
                    if op[0] == "l0" and j == 0:
                        assert got[0] == st[0], what      # a count: always finite, exact
                    else:
                        assert _same_sum(float(got[j]), st[j], mags[j]), (what, j, got[j], st[j])
                for b in (0, 2):
                    assert torch.equal(lay.Y[b], clean.Y[b]) and torch.equal(lay.K[b], clean.K[b]), what
                    assert torch.equal(lay.out[b].view(torch.int64), clean.out[b].view(torch.int64)), what


# ------------------------------------------------------------------ refusals and empties
def test_batch_refusals_and_empties(s):
    import torch
    n, batch = 513, 3
    prob = Problems.get(s, n, 7100 + n)
    L, B, ctx = s._lib.load(), s._lib.load_batch(), s.context("cuda:0")
    lay = Layout(prob, range(batch), 1, 0)
    ld = lay.ld
    y, q, xk, sj, k = (_P(f) for f in (lay.fy, lay.fq, lay.fx, lay.fs, lay.fk))
    lam, sig, qs, lo, up, out = _P(lay.lam), _P(lay.sig), _P(lay.qs), _P(-lay.dl), _P(lay.dl), _P(lay.out)
    keep = (-lay.dl, lay.dl)
    Z = None

    def plain(y=y, q=q, xk=xk, sj=sj, n=n, batch=batch, ld=ld, lam=lam, sig=sig, qs=qs, k=k, out=out):
        return B.spx_proxstep_l1_batch(ctx, y, q, xk, sj, n, batch, ld, lam, sig, qs, k, out)

    def box(lo=lo, up=up, **kw):
        a = dict(y=y, q=q, xk=xk, sj=sj, n=n, batch=batch, ld=ld, lam=lam, sig=sig, qs=qs, k=k, out=out); a.update(kw)
        return B.spx_proxstep_l0_box_batch(ctx, a["y"], a["q"], a["xk"], a["sj"], a["n"], a["batch"], a["ld"], a["lam"], a["sig"], lo, up,
                                           _P(prob.maskd), a["qs"], a["k"], a["out"])

    def untouched():
        torch.cuda.synchronize()
        return bool((lay.fy == POISON).all()) and bool((lay.fk == POISON).all()) and bool((lay.out == POISON).all())

    def next_call_is_right():
        assert plain() == 0
        lay.check(s, OPS[0], "after a refusal")
        lay.fy.fill_(POISON); lay.fk.fill_(POISON); lay.out.fill_(POISON)

    refusals = [
        ("y == q", lambda: plain(y=q)), ("xkn == y", lambda: plain(k=y)), ("xkn == q", lambda: plain(k=q)),
        ("xkn == xk", lambda: plain(k=xk)), ("xkn == sj", lambda: plain(k=sj)), ("ld < n", lambda: plain(ld=n - 1)),
        ("batch < 0", lambda: plain(batch=-1)), ("n < 0", lambda: plain(n=-1)), ("lambda NULL", lambda: plain(lam=Z)),
        ("sigma NULL", lambda: plain(sig=Z)), ("q_scale NULL", lambda: plain(qs=Z)), ("stats_dev NULL", lambda: plain(out=Z)),
        ("l NULL", lambda: box(lo=Z)), ("u NULL", lambda: box(up=Z)), ("box: y == q", lambda: box(y=q)),
        ("box: xkn == mask", lambda: box(k=_P(prob.maskd))),
        # more than 2^31 - 1 workgroups: one per problem in the row form, five per problem at n = R + 1 (never launched: the
        # refusal comes before anything is touched)
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
        s.prox_step_batch_bang(lay.Y, "lhalf", lay.Q, lay.X, lay.S, lay.lam, lay.sig, lay.qs)
    with pytest.raises(TypeError):
        s.prox_step_batch_bang(lay.Y, "l1", lay.Y, lay.X, lay.S, lay.lam, lay.sig, lay.qs)
    with pytest.raises(TypeError):
        s.prox_step_batch_bang(lay.Y, "l1", lay.Q, lay.X, lay.S, lay.lam[:2], lay.sig, lay.qs)
    with pytest.raises(TypeError):
        s.prox_step_batch_bang(lay.Y, "l1", lay.Q, lay.X, lay.S, lay.lam, lay.sig, lay.qs, l=keep[0])
    with pytest.raises(TypeError):
        s.prox_step_batch_bang(lay.Y, "l1", lay.Q.contiguous(), lay.X, lay.S, lay.lam, lay.sig, lay.qs)   # another row stride
    Yn, outn = s.prox_step_batch("l1", lay.Q, lay.X, lay.S, lay.lam, lay.sig, lay.qs)
    assert torch.equal(Yn, prob.ref(OPS[0])[0][:batch]) and Yn.stride() == lay.Q.stride() and tuple(outn.shape) == (batch, 3)


# ------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("n", [3073, R + 3073])
def test_batch_sums_are_reproducible(s, n):
    import torch
    prob = Problems.get(s, n, 7100 + n)
    for op in OPS:
        a, b = Layout(prob, range(7), 1, 1), Layout(prob, range(7), 1, 1)
        a.call(s, op); b.call(s, op); a.call(s, op)
        assert torch.equal(a.out.view(torch.int64), b.out.view(torch.int64)), (op, n)


# ------------------------------------------------------------------ the parameters follow the device
@pytest.mark.parametrize("n", [3073, R + 3073])
def test_captured_batch_call_follows_the_device_parameters(s, n):
    """one batched call captured into a graph (side stream, warm-up first: the tiled form reserves its workspace there);
    between replays lambda, sigma and q_scale (and the box) are overwritten ON THE DEVICE: every replay's rows equal the single
    call with the NEW scalars, bit for bit"""
    import torch
    prob = Problems.get(s, n, 7100 + n)
    rng = np.random.default_rng(7500 + n)
    for op in (OPS[1], OPS[3]):
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            lay = Layout(prob, range(3), 1, 0)
            if op[1]:
                lay.lo, lay.up = -lay.dl, lay.dl.clone()

            def call():
                kind, box, msk = op
                s.prox_step_batch_bang(lay.Y, kind, lay.Q, lay.X, lay.S, lay.lam, lay.sig, lay.qs, l=lay.lo if box else None,
                                       u=lay.up if box else None, selected=prob.maskd if msk else None, xkn=lay.K, out=lay.out)
            call(); call()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call()
        for rep in range(3):
            lam, sig, qs, dl = (rng.uniform(0.3, 1.5, size=3) for _ in range(4))
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
