"""GPU: batched ShiftedNormL1B2 prox! + step statistics with the per-problem parameters on the device
(spx_proxstep_l1_b2_batch, prox_step_b2_batch / prox_step_b2_batch_bang; include/spx_b2_batch.h).

Problem b is row b of the batch x n tensors (row stride ld >= n); lambda_b, sigma_b, Delta_b and q_scale_b are read from device
arrays by the ONE workgroup that owns the row.  The reference of y is the CPU oracle (oracle.prox_l1_b2 at q_scale_b * q) at the
project's B2 bar, max |y - ref| <= 1e-12 max(||ref||, ||xk||) per row; bit identity with the single call is promised -- and
asserted -- on rows whose trust region is inactive only.  The sums: [0] within 1e-12 of lambda fsum|xkn|, [1] and [2] within
1e-12 * sum |terms| of math.fsum of the host's rounded products.

Shapes: n from {1, 2, 3, 7, 63, 64, 65}, on both sides of every bound of the plan's tile table (kB2BatchTiles: 64 x 4, 256 x 4,
256 x 16, 512 x 16 -- 256, 1024, 4096, 8192 elements), at kB2BatchRowMax - 1 / + 0 / + 1 / + 2 and 2 kB2BatchRowMax + 3 (the row
walk); batch 1, 2, 3, 7; ld = n, n + 1, n + 5 (an odd ld alternates the rows' parity); every base on a 16-byte boundary or 8
bytes off one.  Rows of one call mix active, barely active (Delta = 0.9 ||xk|| under a wide box) and inactive trust regions,
Gaussian and integer-lattice data; which class a row is in is decided from chi(ProjB(-xk)) on the host, with a margin."""
import ctypes
import math

import numpy as np
import pytest

import nonfinite
import redzone

pytestmark = pytest.mark.gpu

TOL = 1e-12
INVALID = 1
POISON = -777.25
ROW_MAX = 8192
N_MAX = 1 << 20
TILE_CAPS = [256, 1024, 4096, 8192]
SIZES = sorted({1, 2, 3, 7, 63, 64, 65} | {c + d for c in TILE_CAPS for d in (-1, 0, 1)} | {ROW_MAX + 2, 2 * ROW_MAX + 3})
BATCHES = [1, 2, 3, 7]
PADS = [0, 1, 5]
_D = ctypes.c_double
KINDS = ["active", "inactive", "barely", "active", "inactive", "lattice", "barely"]


@pytest.fixture(scope="module")
def s():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.build()


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)


def _bits(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _chi0(q, xk, sj, lam, sigma, qs):
    ls = lam * sigma
    sq = sj + qs * q
    with np.errstate(all="ignore"):
        return math.sqrt(math.fsum((np.minimum(np.maximum(-xk, sq - ls), sq + ls) ** 2).tolist()))


class Problems:
    """`rows` problems of n elements, their scalars, their oracle results and the class of each row's trust region (computed once
    per (n, rows, seed) and shared by every test that places these rows somewhere)"""
    _cache = {}

    @classmethod
    def get(cls, s, orc, n, rows=7, distinct=None):
        key = (n, rows, distinct)
        if key not in cls._cache:
            cls._cache[key] = cls(s, orc, n, rows, distinct)
        return cls._cache[key]

    def __init__(self, s, orc, n, rows, distinct):
        import torch
        self.s, self.orc, self.n, self.rows = s, orc, n, rows
        d = rows if distinct is None else distinct       # rows beyond `distinct` repeat the first ones (problem = row % distinct)
        rng = np.random.default_rng(5100 + 7 * n + d)
        X, SJ, Q = rng.normal(size=(d, n)), rng.uniform(-0.5, 0.5, size=(d, n)), rng.normal(size=(d, n))
        lam, sig, qs = rng.uniform(0.05, 0.6, size=d), rng.uniform(0.3, 1.5, size=d), rng.uniform(0.5, 1.5, size=d)
        dlt = np.empty(d)
        self.kind = []
        for r in range(d):
            kind = KINDS[r % len(KINDS)]
            if kind == "lattice":
                X[r], SJ[r], Q[r] = rng.integers(-8, 9, size=n) / 4.0, rng.integers(-2, 3, size=n) / 4.0, rng.integers(-12, 13, size=n) / 4.0
                if not X[r].any():
                    X[r, 0] = 0.75
                kind = "active"
            if kind == "barely":
                lam[r], sig[r] = 5.0, 1.0            # a wide box: ProjB(-xk) = -xk, chi = ||xk||
            c = _chi0(Q[r], X[r], SJ[r], lam[r], sig[r], qs[r])
            dlt[r] = {"active": 0.3 * c if c > 0 else 1.0, "inactive": 2.0 * c + 1.0, "barely": 0.9 * float(np.linalg.norm(X[r]))}[kind]
            # the class by the numbers, with a margin the sums' rounding cannot cross
            self.kind.append("active" if dlt[r] < c * (1 - 1e-9) else "inactive" if dlt[r] > c * (1 + 1e-9) else "edge")
        assert "edge" not in self.kind, self.kind
        pick = np.arange(rows) % d
        self.kind = [self.kind[k] for k in pick]
        self.X, self.SJ, self.Q = X[pick], SJ[pick], Q[pick]
        self.lam, self.sig, self.dlt, self.qs = lam[pick], sig[pick], dlt[pick], qs[pick]
        self.Xd, self.SJd, self.Qd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (self.X, self.SJ, self.Q))
        self._ref, self._single, self._ok = {}, {}, {}

    def ref(self, r):
        if r not in self._ref:
            self._ref[r] = self.orc.prox_l1_b2(self.qs[r] * self.Q[r], self.X[r], self.SJ[r], self.lam[r], self.sig[r], self.dlt[r])
        return self._ref[r]

    def single(self, r, q=None, xk=None, sj=None, scal=None):
        """spx_proxstep_l1_b2 on row r alone (or on the given vectors / (lambda, sigma, Delta, q_scale)): (y, xkn, [h, qy, yy])"""
        import torch
        L, ctx = self.s._lib.load(), self.s.context("cuda:0")
        q = (self.Qd[r] if q is None else q).clone()
        xk = (self.Xd[r] if xk is None else xk).clone()
        sj = (self.SJd[r] if sj is None else sj).clone()
        lam, sig, dlt, qs = scal if scal is not None else (self.lam[r], self.sig[r], self.dlt[r], self.qs[r])
        y, k = torch.full_like(q, POISON), torch.full_like(q, POISON)
        st = (_D * 3)()
        rc = L.spx_proxstep_l1_b2(ctx, _P(y), _P(q), _P(xk), _P(sj), self.n, float(lam), float(sig), float(dlt), 1.0, float(qs), _P(k),
                                  st, None)
        assert rc == 0, L.spx_last_error()
        return y, k, [st[0], st[1], st[2]]

    def single_cached(self, r):
        if r not in self._single:
            self._single[r] = self.single(r)
        return self._single[r]

    def check_row(self, r, y, k, out, what, stats=True):
        """row r's y (numpy), xkn and triple against the oracle, the host sums and -- by the row's class -- the single call's bits
        or the trust-region radius.  Results that are bit for bit ones already verified are not verified again."""
        key = (r, y.tobytes(), None if k is None else k.tobytes(), out.tobytes())
        if key in self._ok:
            return
        ref, x, sj, q = self.ref(r), self.X[r], self.SJ[r], self.Q[r]
        scale = max(float(np.linalg.norm(ref)), float(np.linalg.norm(x)))
        err = float(np.max(np.abs(y - ref))) if self.n else 0.0
        v = (x + sj) + y
        h = self.lam[r] * math.fsum(np.abs(v).tolist())
        qy = q * y
        mqy, sqy, syy = math.fsum(np.abs(qy).tolist()), math.fsum(qy.tolist()), math.fsum((y * y).tolist())
        print("%s row %d (%s): max |y - oracle| %.3e (bar %.3e) | h %.17g ref %.17g | qy %.17g ref %.17g (bar %.3g) | yy %.17g ref %.17g"
              % (what, r, self.kind[r], err, TOL * scale, out[0], h, out[1], sqy, TOL * mqy, out[2], syy))
        assert err <= TOL * scale, (what, r, err, scale)
        if k is not None:
            assert np.array_equal(k.view(np.int64), v.view(np.int64)), (what, r)          # xkn = (xk + sj) + y of the returned y
        if stats:
            assert abs(out[0] - h) <= TOL * h, (what, r, out[0], h)
            assert abs(out[1] - sqy) <= TOL * mqy, (what, r, out[1], sqy, mqy)
            assert abs(out[2] - syy) <= TOL * syy, (what, r, out[2], syy)
        if self.kind[r] == "inactive":
            ys, ks, _ = self.single_cached(r)
            assert np.array_equal(y, ref), (what, r)                                      # == the oracle
            assert np.array_equal(y.view(np.int64), ys.cpu().numpy().view(np.int64)), (what, r)   # the single call's bits
            if k is not None:
                assert np.array_equal(k.view(np.int64), ks.cpu().numpy().view(np.int64)), (what, r)
        else:
            nrm = math.sqrt(math.fsum(((sj + y) ** 2).tolist()))
            print("    ||sj + y|| %.17g Delta %.17g" % (nrm, self.dlt[r]))
            assert abs(nrm - self.dlt[r]) <= TOL * self.dlt[r], (what, r, nrm, self.dlt[r])
        self._ok[key] = True


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
        self.lam, self.sig, self.dlt, self.qs = dev(prob.lam), dev(prob.sig), dev(prob.dlt), dev(prob.qs)
        self.out = torch.full((self.batch, 3), POISON, dtype=torch.float64, device="cuda:0")
        ld_eff = ld if self.batch > 1 else self.n   # (the mirror hands ld = n to the library for a single row)
        self.pairs = self.n >= 2 and ld_eff % 2 == 0 and off == 0
        if guarded:
            for g in self.zone.bufs:
                g.snap = g.buf.clone()   # (the inputs were copied in after the snapshot was taken)

    def call(self, s, xkn=True):
        return s.prox_step_b2_batch_bang(self.Y, self.Q, self.X, self.S, self.lam, self.sig, self.dlt, self.qs,
                                         xkn=self.K if xkn else None, out=self.out)

    def padding_untouched(self, xkn=True):
        """every element [b ld + n, (b + 1) ld) of y and xkn still holds the poison, and no row element does"""
        for f, V in ((self.fy, self.Y), (self.fk, self.K))[:2 if xkn else 1]:
            whole = f.as_strided((self.batch, self.ld), (self.ld, 1))
            assert bool((whole[:, self.n:] == POISON).all()), "padding written"
            assert not bool((V == POISON).any()), "row element not written"
        if not xkn:
            assert bool((self.fk == POISON).all()), "xkn written"

    def check(self, what, xkn=True, stats=True):
        self.padding_untouched(xkn)
        Y, K, out = self.Y.cpu().numpy(), self.K.cpu().numpy(), self.out.cpu().numpy()
        for b, r in enumerate(self.rows):
            self.prob.check_row(r, np.ascontiguousarray(Y[b]), np.ascontiguousarray(K[b]) if xkn else None, out[b], what, stats)

    def triple(self):
        return self.Y.clone(), self.K.clone(), self.out.clone()


def _same(a, b):
    return all(_bits(x, z) for x, z in zip(a, b))


# ------------------------------------------------------------------ rows against the oracle (and what goes with each class)
@pytest.mark.parametrize("n", SIZES)
def test_b2_batch_rows_against_the_oracle(s, orc, n):
    prob = Problems.get(s, orc, n)
    assert {"active", "inactive"} <= set(prob.kind)
    for batch in BATCHES:
        for pad in PADS:
            for off in (0, 1):
                lay = Layout(prob, range(batch), pad, off)
                lay.call(s)
                lay.check("n=%d batch=%d pad=%d off=%d" % (n, batch, pad, off))
    # the rows in another order: an inactive row first, active ones behind it
    lay = Layout(prob, [4, 1, 6, 0, 5, 2, 3], 0, 0)
    lay.call(s)
    lay.check("n=%d reordered" % n)


# ------------------------------------------------------------------ the bits
@pytest.mark.parametrize("n", [2, 7, 65, 257, 1025, 4097, ROW_MAX, ROW_MAX + 1, 2 * ROW_MAX + 3])
def test_b2_batch_bits_do_not_depend_on_repeat_row_or_batch(s, orc, n):
    """a repeat; the same problem at row 0 of batch 1, row 2 of batch 3, row 6 of batch 7; every row of a batch of 7 against a
    batch-of-1 call on that row: the same bits in y, xkn and the three sums"""
    prob = Problems.get(s, orc, n)
    for pad, off in ((0, 0), (2, 0), (1, 0), (1, 1), (0, 1)):
        a, b = Layout(prob, range(7), pad, off), Layout(prob, range(7), pad, off)
        a.call(s); b.call(s); a.call(s)
        assert _same(a.triple(), b.triple()), (n, pad, off)
        # (with an odd ld the single row of batch 1 is handed ld = n and may fall into another class than the larger batches:
        #  it is left out there, the placements in batch 3 and batch 7 share their class and are compared)
        places = (([4], 0), ([0, 1, 4], 2), ([0, 1, 2, 3, 5, 6, 4], 6))
        seen = None
        for rows, at in places[1 if (pad % 2 and off == 0) else 0:]:
            lay = Layout(prob, rows, pad, off)
            lay.call(s)
            cur = (lay.Y[at].clone(), lay.K[at].clone(), lay.out[at].clone())
            assert seen is None or _same(seen, cur), (n, pad, off, at)
            seen = cur
        assert _same(seen, (a.Y[4], a.K[4], a.out[4])), (n, pad, off)
        if not (pad % 2 and off == 0):
            for r in range(7):   # a row moved from the batch of 7 into a batch of 1 keeps its bits
                one = Layout(prob, [r], pad, off)
                one.call(s)
                assert one.pairs == a.pairs
                assert _same((one.Y[0], one.K[0], one.out[0]), (a.Y[r], a.K[r], a.out[r])), (n, pad, off, r)


@pytest.mark.parametrize("n", [3, 64, 1000, ROW_MAX - 1, ROW_MAX + 2])
def test_b2_batch_xkn_absent_and_misaligned_alone(s, orc, n):
    """xkn = None, and xkn alone 8 bytes off (only its stores drop to 8 bytes): y and the sums keep their bits"""
    prob = Problems.get(s, orc, n)
    for pad, off in ((0, 0), (1, 0), (2, 0), (0, 1)):
        base = Layout(prob, range(3), pad, off)
        base.call(s)
        base.check("n=%d pad=%d off=%d" % (n, pad, off))
        lay = Layout(prob, range(3), pad, off)
        lay.call(s, xkn=False)
        lay.padding_untouched(xkn=False)
        assert _bits(lay.Y, base.Y) and _bits(lay.out, base.out), (n, pad, off)
        lay = Layout(prob, range(3), pad, off, xkn_off=1 - off)
        lay.call(s)
        lay.padding_untouched()
        assert _same(lay.triple(), base.triple()), (n, pad, off)


# ------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("n", [1, 2, 7, 65, 255, 257, 1025, 4097, ROW_MAX, ROW_MAX + 1, 2 * ROW_MAX + 3])
def test_b2_batch_guard_bands_and_padding(s, orc, n):
    """every vector between guard bands, poison everywhere: after the call the guard bands (and the inputs) are unchanged, every
    padding element still holds the poison and no row element does"""
    prob = Problems.get(s, orc, n)
    for batch, pad, off in ((1, 0, 0), (1, 5, 1), (3, 0, 1), (3, 1, 0), (3, 2, 0), (3, 5, 1), (7, 5, 0)):
        lay = Layout(prob, range(batch), pad, off, guarded=True)
        lay.call(s)
        lay.zone.check()
        for g in lay.zone.bufs[2:]:   # q, xk, sj: read only
            assert bool((g.buf == g.snap).all()), g.name
        lay.check("guarded n=%d batch=%d pad=%d off=%d" % (n, batch, pad, off))


# ------------------------------------------------------------------ more problems than CUs, more than 65535 rows
@pytest.mark.parametrize("batch,n", [(300, 15), (70001, 2)])
def test_b2_batch_many_rows(s, orc, batch, n):
    """the rows repeat three problems (problem = row % 3): a sample of rows against the oracle, ALL rows against the batch-of-1
    call on their problem"""
    import torch
    prob = Problems.get(s, orc, n, rows=batch, distinct=3)
    rng = np.random.default_rng(batch)
    rows = sorted({0, 1, 2, batch - 1} | set(rng.choice(batch, size=12, replace=False).tolist()))
    for pad, off in ((0, 0), (1, 1)):
        lay = Layout(prob, range(batch), pad, off)
        lay.call(s)
        lay.padding_untouched()
        Y, K, out = lay.Y.cpu().numpy(), lay.K.cpu().numpy(), lay.out.cpu().numpy()
        for r in rows:
            prob.check_row(r, np.ascontiguousarray(Y[r]), np.ascontiguousarray(K[r]), out[r], "batch=%d" % batch)
        for p in range(3):
            one = Layout(prob, [p], 0 if lay.pairs else pad, off)
            one.call(s)
            assert one.pairs == lay.pairs
            mine = torch.arange(p, batch, 3, device="cuda:0")
            for got, want in ((lay.Y, one.Y), (lay.K, one.K), (lay.out, one.out)):
                g = got[mine].contiguous().view(torch.int64)
                assert bool((g == want[0].contiguous().view(torch.int64)[None, :]).all()), (batch, p, pad, off)
    Problems._cache.pop((n, batch, 3))


def test_b2_batch_the_n_bound(s, orc):
    """n = 2^20 runs (the row walk, two rows) and meets the oracle; n = 2^20 + 1 is refused and the text names the single call"""
    import torch
    prob = Problems.get(s, orc, N_MAX, rows=2)
    lay = Layout(prob, range(2), 0, 0)
    lay.call(s)
    lay.check("n=2^20")
    Problems._cache.pop((N_MAX, 2, None))
    L, G, ctx = s._lib.load(), s._lib.load_b2_batch(), s.context("cuda:0")
    n = N_MAX + 1
    v = [torch.full((n,), POISON, dtype=torch.float64, device="cuda:0") for _ in range(5)]
    par = torch.ones(4, dtype=torch.float64, device="cuda:0")
    out = torch.full((3,), POISON, dtype=torch.float64, device="cuda:0")
    rc = G.spx_proxstep_l1_b2_batch(ctx, _P(v[0]), _P(v[1]), _P(v[2]), _P(v[3]), n, 1, n, _P(par[0:1]), _P(par[1:2]), _P(par[2:3]),
                                    _P(par[3:4]), 1.0, _P(v[4]), _P(out))
    assert rc == INVALID and b"spx_proxstep_l1_b2" in L.spx_last_error()
    torch.cuda.synchronize()
    assert bool((v[0] == POISON).all()) and bool((v[4] == POISON).all()) and bool((out == POISON).all())


# ------------------------------------------------------------------ isolation under non-finite data
@pytest.mark.parametrize("n", [65, 1025, ROW_MAX + 2])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf"), 1e150])
def test_b2_batch_nonfinite_row_is_isolated(s, orc, n, value):
    """NaN, +-Inf, 1e150 in one element of ONE row of a batch of 3 -- element 0, the middle, the tail -- of q, xk or sj, in the
    sequence clean / planted / clean: the planted row has the classes of spx_proxstep_l1_b2 on it and of the oracle, the other
    rows and the clean call behind keep the bits of the clean call in front"""
    prob = Problems.get(s, orc, n)
    for pad, off in ((0, 0), (1, 1)):
        clean = Layout(prob, range(3), pad, off)
        clean.call(s)
        for where in ("q", "xk", "sj"):
            for at in (0, n // 2, n - 1):
                lay = Layout(prob, range(3), pad, off)
                {"q": lay.Q, "xk": lay.X, "sj": lay.S}[where][0, at] = value     # row 0: an active trust region
                lay.call(s)
                lay.padding_untouched()
                what = "n=%d %r in %s[%d] pad=%d off=%d" % (n, value, where, at, pad, off)
                qh, xh, sh = lay.Q[0].cpu().numpy(), lay.X[0].cpu().numpy(), lay.S[0].cpu().numpy()
                y, k, st = prob.single(0, q=lay.Q[0], xk=lay.X[0], sj=lay.S[0])
                with np.errstate(all="ignore"):
                    ref = orc.prox_l1_b2(prob.qs[0] * qh, xh, sh, prob.lam[0], prob.sig[0], prob.dlt[0])
                got = lay.Y[0].cpu().numpy()
                print(what, "classes: batch", np.bincount(nonfinite.classes(got), minlength=4).tolist(), "single",
                      np.bincount(nonfinite.classes(y.cpu().numpy()), minlength=4).tolist(), "oracle",
                      np.bincount(nonfinite.classes(ref), minlength=4).tolist())
                nonfinite.check_classes(got, y.cpu().numpy(), what + " (single call)")
                nonfinite.check_classes(got, ref, what + " (oracle)")
                with np.errstate(all="ignore"):
                    assert nonfinite.same_bits_or_both_nan(lay.K[0].cpu().numpy(), (xh + sh) + got).all(), what
                for b in (1, 2):
                    assert _bits(lay.Y[b], clean.Y[b]) and _bits(lay.K[b], clean.K[b]) and _bits(lay.out[b], clean.out[b]), what
        after = Layout(prob, range(3), pad, off)
        after.call(s)
        assert _same(after.triple(), clean.triple()), (n, value, pad, off)


# ------------------------------------------------------------------ degenerate scalars
@pytest.mark.parametrize("n", [65, 1025, ROW_MAX + 2])
@pytest.mark.parametrize("delta", [0.0, -1.0, float("nan"), float("inf")])
def test_b2_batch_degenerate_radius_in_one_row(s, orc, n, delta):
    """Delta = 0, -1, NaN, +Inf in ONE row: the call returns, the other rows keep their bits, the guard bands are intact, and the
    +Inf row is an inactive row (exact)"""
    import torch
    prob = Problems.get(s, orc, n)
    clean = Layout(prob, range(3), 2, 0)
    clean.call(s)
    lay = Layout(prob, range(3), 2, 0, guarded=True)
    lay.dlt[0] = delta
    lay.call(s)
    torch.cuda.synchronize()
    lay.zone.check()
    whole = lay.fy.as_strided((3, lay.ld), (lay.ld, 1))
    assert bool((whole[:, n:] == POISON).all())
    for b in (1, 2):
        assert _bits(lay.Y[b], clean.Y[b]) and _bits(lay.K[b], clean.K[b]) and _bits(lay.out[b], clean.out[b]), (n, delta, b)
    if delta == float("inf"):
        y, k, _ = prob.single(0, scal=(prob.lam[0], prob.sig[0], delta, prob.qs[0]))
        ref = orc.prox_l1_b2(prob.qs[0] * prob.Q[0], prob.X[0], prob.SJ[0], prob.lam[0], prob.sig[0], delta)
        assert _bits(lay.Y[0], y) and _bits(lay.K[0], k)
        assert np.array_equal(lay.Y[0].cpu().numpy(), ref)


def test_b2_batch_q_scale(s, orc):
    """q_scale[b] = 0 in one row: the prox at q = 0, against the oracle; [1] sums q AS PASSED times y under any q_scale (a
    negative one included); the other rows keep their bits"""
    for n in (65, 1025, ROW_MAX + 2):
        prob = Problems.get(s, orc, n)
        clean = Layout(prob, range(4), 0, 0)
        clean.call(s)
        for qs in (0.0, -1.25):
            lay = Layout(prob, range(4), 0, 0)
            lay.qs[3] = qs
            lay.call(s)
            y, out = lay.Y[3].cpu().numpy(), lay.out[3].cpu().numpy()
            ref = orc.prox_l1_b2(qs * prob.Q[3], prob.X[3], prob.SJ[3], prob.lam[3], prob.sig[3], prob.dlt[3])
            scale = max(float(np.linalg.norm(ref)), float(np.linalg.norm(prob.X[3])))
            assert float(np.max(np.abs(y - ref))) <= TOL * scale, (n, qs)
            qy = prob.Q[3] * y                                    # q as passed
            assert abs(out[1] - math.fsum(qy.tolist())) <= TOL * math.fsum(np.abs(qy).tolist()), (n, qs, out[1])
            assert all(math.isfinite(v) for v in lay.out.cpu().numpy().ravel())
            for b in (0, 1, 2):
                assert _bits(lay.Y[b], clean.Y[b]) and _bits(lay.out[b], clean.out[b]), (n, qs, b)


# ------------------------------------------------------------------ refusals and empties
def test_b2_batch_refusals_and_empties(s, orc):
    import torch
    n, batch = 65, 3
    prob = Problems.get(s, orc, n)
    L, G, ctx = s._lib.load(), s._lib.load_b2_batch(), s.context("cuda:0")
    lay = Layout(prob, range(batch), 1, 0)
    ld = lay.ld
    y, q, xk, sj, k = (_P(f) for f in (lay.fy, lay.fq, lay.fx, lay.fs, lay.fk))
    lam, sig, dlt, qs, out = _P(lay.lam), _P(lay.sig), _P(lay.dlt), _P(lay.qs), _P(lay.out)
    Z = None

    def call(y=y, q=q, xk=xk, sj=sj, n=n, batch=batch, ld=ld, lam=lam, sig=sig, dlt=dlt, qs=qs, k=k, out=out):
        return G.spx_proxstep_l1_b2_batch(ctx, y, q, xk, sj, n, batch, ld, lam, sig, dlt, qs, 1.0, k, out)

    def untouched():
        torch.cuda.synchronize()
        return bool((lay.fy == POISON).all()) and bool((lay.fk == POISON).all()) and bool((lay.out == POISON).all())

    def next_call_is_right():
        assert call() == 0
        lay.check("after a refusal")
        lay.fy.fill_(POISON); lay.fk.fill_(POISON); lay.out.fill_(POISON)

    refusals = [
        ("y == q", lambda: call(y=q)), ("xkn == y", lambda: call(k=y)), ("xkn == q", lambda: call(k=q)),
        ("xkn == xk", lambda: call(k=xk)), ("xkn == sj", lambda: call(k=sj)), ("ld < n", lambda: call(ld=n - 1)),
        ("n < 0", lambda: call(n=-1)), ("batch < 0", lambda: call(batch=-1)),
        ("n > 2^20", lambda: call(n=N_MAX + 1, ld=N_MAX + 1)), ("batch > 2^31 - 1", lambda: call(batch=1 << 31)),
        ("lambda NULL", lambda: call(lam=Z)), ("sigma NULL", lambda: call(sig=Z)), ("delta NULL", lambda: call(dlt=Z)),
        ("q_scale NULL", lambda: call(qs=Z)), ("stats_dev NULL", lambda: call(out=Z)),
        ("lambda NULL, n == 0", lambda: call(n=0, lam=Z)), ("stats_dev NULL, n == 0", lambda: call(n=0, out=Z)),
    ]
    for what, f in refusals:
        assert f() == INVALID, what
        assert L.spx_last_error(), what
        assert untouched(), what
        next_call_is_right()
    # empties: batch == 0 does nothing; n == 0 stores 3 * batch zeros (by a kernel)
    assert call(batch=0) == 0 and call(batch=0, lam=Z, sig=Z, dlt=Z, qs=Z, out=Z) == 0 and untouched()
    next_call_is_right()
    for kw in (dict(n=0, ld=0), dict(n=0, ld=5), dict(n=0, ld=0, y=Z, q=Z, xk=Z, sj=Z, k=Z)):
        assert call(**kw) == 0, kw
        torch.cuda.synchronize()
        assert bool((lay.out == 0.0).all()) and bool((lay.fy == POISON).all()) and bool((lay.fk == POISON).all()), kw
        lay.out.fill_(POISON)
    next_call_is_right()
    # the mirror refuses what it can see
    with pytest.raises(TypeError):
        s.prox_step_b2_batch_bang(lay.Y, lay.Y, lay.X, lay.S, lay.lam, lay.sig, lay.dlt, lay.qs)
    with pytest.raises(TypeError):
        s.prox_step_b2_batch_bang(lay.Y, lay.Q, lay.X, lay.S, lay.lam, lay.sig, lay.dlt[:2], lay.qs)    # two radii
    with pytest.raises(TypeError):
        s.prox_step_b2_batch_bang(lay.Y, lay.Q, lay.X, lay.S, lay.lam, lay.sig, 0.3, lay.qs)            # a host radius
    with pytest.raises(TypeError):
        s.prox_step_b2_batch_bang(lay.Y, lay.Q, lay.X, lay.S, lay.lam, lay.sig, lay.dlt.cpu(), lay.qs)
    with pytest.raises(TypeError):
        s.prox_step_b2_batch_bang(lay.Y, lay.Q.contiguous(), lay.X, lay.S, lay.lam, lay.sig, lay.dlt, lay.qs)   # another row stride
    with pytest.raises(TypeError):
        s.prox_step_b2_batch_bang(lay.Y, lay.Q, lay.X, lay.S, lay.lam, lay.sig, lay.dlt, lay.qs, chi_lambda=lay.qs)
    Yn, outn = s.prox_step_b2_batch(lay.Q, lay.X, lay.S, lay.lam, lay.sig, lay.dlt, lay.qs)
    lay.call(s)
    assert _bits(Yn, lay.Y) and Yn.stride() == lay.Q.stride() and _bits(outn, lay.out)


# ------------------------------------------------------------------ the parameters follow the device
@pytest.mark.parametrize("n", [1000, 10000], ids=["row-resident", "row-walk"])
def test_captured_b2_batch_call_follows_the_device_parameters(s, orc, n):
    """one batched call captured into a graph on a side stream; between replays lambda, sigma, Delta and q_scale are overwritten
    ON THE DEVICE: every replay equals an eager call at the new values, bit for bit, and meets the oracle at them"""
    import torch
    rng = np.random.default_rng(5200 + n)
    prob = Problems.get(s, orc, n)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        lay = Layout(prob, range(3), 2, 0)
        lay.call(s)   # (the stream's context and the library's code object exist before the capture)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        lay.call(s)
    for rep in range(3):
        lam, sig, qs = rng.uniform(0.05, 0.6, size=3), rng.uniform(0.3, 1.5, size=3), rng.uniform(0.5, 1.5, size=3)
        dlt = prob.dlt[:3] * (1.0 if rep == 0 else rng.uniform(0.25, 4.0, size=3))
        if rep == 0:
            lam, sig, qs = prob.lam[:3], prob.sig[:3], prob.qs[:3]
        for t, a in ((lay.lam, lam), (lay.sig, sig), (lay.dlt, dlt), (lay.qs, qs)):
            t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        lay.fy.fill_(POISON); lay.fk.fill_(POISON); lay.out.fill_(POISON)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        lay.padding_untouched()
        if rep == 0:
            lay.check("captured n=%d, the problems' own scalars" % n)
        eager = Layout(prob, range(3), 2, 0)
        for t, a in ((eager.lam, lam), (eager.sig, sig), (eager.dlt, dlt), (eager.qs, qs)):
            t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        eager.call(s)
        assert _same(lay.triple(), eager.triple()), (n, rep)
        Y = lay.Y.cpu().numpy()
        for b in range(3):
            ref = orc.prox_l1_b2(qs[b] * prob.Q[b], prob.X[b], prob.SJ[b], lam[b], sig[b], dlt[b])
            scale = max(float(np.linalg.norm(ref)), float(np.linalg.norm(prob.X[b])))
            assert float(np.max(np.abs(Y[b] - ref))) <= TOL * scale, (n, rep, b)
