"""GPU: batched ShiftedIndBallL0 / ShiftedIndBallL0BInf prox! + step statistics with the per-problem parameters on the device
(spx_proxstep_indball_l0_batch, spx_proxstep_indball_l0_binf_batch, prox_step_topr_batch / prox_step_topr_batch_bang;
include/spx_topr_batch.h).

Problem b is row b of the batch x n tensors (row stride ld >= n); r_b, Delta_b and q_scale_b are read from device arrays by the
ONE workgroup that owns the row.  What is held, per row:
  1. y == bit for bit spx_prox_indball_l0[_binf] on that row with r_b (Delta_b) and a q multiplied by q_scale_b on the host, with
     tuning key 6 at 1 and at 0 where it applies (n <= 8192: the one-workgroup kernel / the resident grid); and == the oracle
     (oracle.TopR: orc_prox_indball_l0_perm, one sort per row reused over r);
  2. xkn == (xk + sj) + y;   3. [3b] == the exact count of nonzeros of xkn;
  4. [3b + 1], [3b + 2] within 1e-12 * sum |terms| of math.fsum of the host's rounded products (the project's bar for these sums);
  5. guard bands and padding untouched.

Shapes: n from {1, 2, 7, 63, 64, 65, 255, 257, 1025, 4097, 8191, 8192, 8193, 2 * 8192 + 3} -- both sides of the tile table's
bounds (64 x 4, 256 x 4, 256 x 16, 512 x 16) and of the row walk; batch 1 and 5; ld = n, n + 1, n + 6; every base on a 16-byte
boundary, every base 8 bytes off one, or mixed.  Every row has its own r from {0, 1, n/100, n/2, n - 1, n, n + 3, -2}, its own
Delta and its own q_scale; the eight rows of a size are Gaussian, a 1/4 lattice, a constant with alternating sign, all zeros and
values over 2^+-500."""
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
SIZES = [1, 2, 7, 63, 64, 65, 255, 257, 1025, 4097, 8191, 8192, 8193, 2 * ROW_MAX + 3]
BATCHES = [1, 5]
PADS = [0, 1, 6]
ALIGN = [0, 1, "mixed"]
KINDS = ["gauss", "gauss", "lattice", "const", "zeros", "wide", "gauss", "gauss"]


def r_choices(n):
    return [0, 1, n // 100, n // 2, n - 1, n, n + 3, -2]


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


def _same(a, b):
    return all(_bits(x, z) for x, z in zip(a, b))


def _i64(a):
    return np.ascontiguousarray(a).view(np.int64)


def make_row(kind, n, rng):
    """(q, xk, sj) of one row"""
    if kind == "lattice":
        return rng.integers(-12, 13, size=n) / 4.0, rng.integers(-8, 9, size=n) / 4.0, rng.integers(-2, 3, size=n) / 4.0
    if kind == "const":      # |v| = 0.75 everywhere, the sign alternates: only the index decides
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        return 0.25 * sign, 0.375 * sign, 0.125 * sign
    if kind == "zeros":
        return np.zeros(n), np.zeros(n), np.zeros(n)
    if kind == "wide":       # the whole exponent range
        e = rng.integers(-500, 501, size=n)
        return np.ldexp(rng.normal(size=n), e), np.ldexp(rng.normal(size=n), e - 3), np.ldexp(rng.normal(size=n), e - 5)
    return rng.normal(size=n), rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n)


class Problems:
    """`rows` problems of n elements with their parameters; the single call's and the oracle's results per (row, parameters),
    computed once and shared by every test that places these rows somewhere"""
    _cache = {}

    @classmethod
    def get(cls, s, orc, n, rows=8, distinct=None, kinds=KINDS, rot=0):
        key = (n, rows, distinct, tuple(kinds), rot)
        if key not in cls._cache:
            cls._cache[key] = cls(s, orc, n, rows, distinct, kinds, rot)
        return cls._cache[key]

    def __init__(self, s, orc, n, rows, distinct, kinds, rot):
        import torch
        self.s, self.orc, self.n, self.rows = s, orc, n, rows
        d = rows if distinct is None else distinct       # rows beyond `distinct` repeat the first ones (problem = row % distinct)
        rng = np.random.default_rng(6100 + 7 * n + d + 1000 * rot)
        Q, X, SJ = np.empty((d, n)), np.empty((d, n)), np.empty((d, n))
        for k in range(d):
            Q[k], X[k], SJ[k] = make_row(kinds[k % len(kinds)], n, rng)
        rs = r_choices(n)
        r = np.array([rs[(k + rot) % len(rs)] for k in range(d)], dtype=np.int64)
        qs = rng.uniform(0.5, 1.5, size=d)
        qs[kinds.index("const") % d if "const" in kinds else 0] = 1.0   # (the constant row stays constant)
        dlt = rng.uniform(0.3, 1.2, size=d)
        pick = np.arange(rows) % d
        self.kinds = [kinds[k % len(kinds)] for k in pick]
        self.Q, self.X, self.SJ, self.r, self.qs, self.dlt = Q[pick], X[pick], SJ[pick], r[pick], qs[pick], dlt[pick]
        self.Qd, self.Xd, self.SJd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (self.Q, self.X, self.SJ))
        self._single, self._topr, self._ok = {}, {}, {}

    def single(self, q, xk, sj, r, delta, small=1):
        """spx_prox_indball_l0[_binf] on device vectors (q already scaled), tuning key 6 = small: y"""
        import torch
        L, ctx = self.s._lib.load(), self.s.context("cuda:0")
        q, xk, sj = q.clone(), xk.clone(), sj.clone()
        y = torch.full_like(q, POISON)
        assert L.spx_ctx_set_tuning(ctx, 6, small) == 0
        try:
            if delta is None:
                rc = L.spx_prox_indball_l0(ctx, _P(y), _P(q), _P(xk), _P(sj), self.n, int(r))
            else:
                rc = L.spx_prox_indball_l0_binf(ctx, _P(y), _P(q), _P(xk), _P(sj), self.n, int(r), float(delta))
        finally:
            L.spx_ctx_set_tuning(ctx, 6, 1)
        assert rc == 0, L.spx_last_error()
        return y

    def single_row(self, row, r, qs, delta):
        """the single call's y on problem `row` at (r, q_scale, Delta), under both settings of tuning key 6 where it applies"""
        import torch
        key = (row, int(r), float(qs), None if delta is None else repr(float(delta)))
        if key not in self._single:
            qh = torch.from_numpy(qs * self.Q[row]).cuda()          # q multiplied on the host: one rounded multiply
            ys = [self.single(qh, self.Xd[row], self.SJd[row], r, delta, small).cpu().numpy()
                  for small in ((1, 0) if self.n <= ROW_MAX else (1,))]
            for y in ys[1:]:
                assert np.array_equal(_i64(y), _i64(ys[0])), ("the single call's two forms differ", self.n, row)
            self._single[key] = ys[0]
        return self._single[key]

    def oracle_row(self, row, r, qs, delta):
        key = (row, float(qs))
        if key not in self._topr:
            self._topr[key] = self.orc.TopR(qs * self.Q[row], self.X[row], self.SJ[row])     # one sort per row, reused over r
        with np.errstate(all="ignore"):
            return self._topr[key].prox(int(r), delta)

    def check_row(self, row, y, k, out, what, r=None, qs=None, delta=False, binf=True, q=None, finite=True):
        """row's y (numpy), xkn and triple against the single call, the oracle and the host sums.  Results that are bit for bit
        ones already verified are not verified again."""
        r = self.r[row] if r is None else r
        qs = self.qs[row] if qs is None else qs
        delta = (self.dlt[row] if binf else None) if delta is False else delta
        key = (row, int(r), float(qs), repr(delta), y.tobytes(), None if k is None else k.tobytes(), out.tobytes())
        if key in self._ok:
            return
        x, sj, q = self.X[row], self.SJ[row], self.Q[row]
        ys, yo = self.single_row(row, r, qs, delta), self.oracle_row(row, r, qs, delta)
        assert np.array_equal(_i64(y), _i64(ys)), (what, row, "single call", int(np.sum(_i64(y) != _i64(ys))))
        assert np.array_equal(_i64(y), _i64(yo)), (what, row, "oracle", int(np.sum(_i64(y) != _i64(yo))))
        with np.errstate(all="ignore"):
            v = (x + sj) + y
            qy, yy = q * y, y * y
        if k is not None:
            assert np.array_equal(_i64(k), _i64(v)), (what, row)            # xkn = (xk + sj) + y of the returned y
        count = int(np.count_nonzero(v != 0.0))
        mqy, sqy, syy = math.fsum(np.abs(qy).tolist()), math.fsum(qy.tolist()), math.fsum(yy.tolist())
        print("%s row %d (%s, r %d): nonzeros %r ref %d | qy %.17g ref %.17g (bar %.3g) | yy %.17g ref %.17g"
              % (what, row, self.kinds[row], r, out[0], count, out[1], sqy, TOL * mqy, out[2], syy))
        assert out[0] == float(count), (what, row, out[0], count)
        if delta is None:
            assert count <= max(int(r), 0), (what, row)                      # the plain form always lands in the ball
        assert abs(out[1] - sqy) <= TOL * mqy, (what, row, out[1], sqy, mqy)
        assert abs(out[2] - syy) <= TOL * syy, (what, row, out[2], syy)
        self._ok[key] = True


class Layout:
    """the five batch x n tensors of a call as views of flat poisoned buffers: row stride ld = n + pad, bases `off` elements past
    a 256-byte boundary (0, 1, or "mixed": y and xk one element off, q and sj on the boundary; xkn: xkn_off), rows = the problem
    rows placed at batch rows 0, 1, ..."""

    def __init__(self, prob, rows, pad, off, xkn_off=None, guarded=False, binf=True):
        import torch
        self.prob, self.rows, self.n, self.batch, self.binf = prob, list(rows), prob.n, len(rows), binf
        self.ld = ld = prob.n + pad
        offs = dict(y=1, q=0, xk=1, sj=0, xkn=0) if off == "mixed" else dict.fromkeys(("y", "q", "xk", "sj", "xkn"), off)
        if xkn_off is not None:
            offs["xkn"] = xkn_off
        total = self.batch * ld
        self.zone = redzone.Zone() if guarded else None

        def flat(name):
            o = offs[name]
            if guarded:   # [front guard | batch * ld elements | back guard], poison everywhere
                return self.zone.add(total, torch.float64, align_bytes=8 * o, role="inout", poison=POISON, name=name,
                                     data=torch.full((total,), POISON, dtype=torch.float64)).t
            return torch.full((total + 2,), POISON, dtype=torch.float64, device="cuda:0")[o:o + total]

        self.fy, self.fk = flat("y"), flat("xkn")
        self.fq, self.fx, self.fs = flat("q"), flat("xk"), flat("sj")
        view = lambda f: f.as_strided((self.batch, self.n), (ld, 1))
        self.Y, self.K, self.Q, self.X, self.S = (view(f) for f in (self.fy, self.fk, self.fq, self.fx, self.fs))
        idx = torch.as_tensor(self.rows, device="cuda:0")
        self.Q.copy_(prob.Qd[idx]); self.X.copy_(prob.Xd[idx]); self.S.copy_(prob.SJd[idx])
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[self.rows])).cuda()
        self.r, self.dlt, self.qs = dev(prob.r), dev(prob.dlt), dev(prob.qs)
        self.out = torch.full((self.batch, 3), POISON, dtype=torch.float64, device="cuda:0")
        ld_eff = ld if self.batch > 1 else self.n   # (the mirror hands ld = n to the library for a single row)
        self.pairs = self.n >= 2 and ld_eff % 2 == 0 and off == 0
        if guarded:
            for g in self.zone.bufs:
                g.snap = g.buf.clone()   # (the inputs were copied in after the snapshot was taken)

    def call(self, s, xkn=True):
        return s.prox_step_topr_batch_bang(self.Y, self.Q, self.X, self.S, self.r, self.qs, delta=self.dlt if self.binf else None,
                                           xkn=self.K if xkn else None, out=self.out)

    def padding_untouched(self, xkn=True):
        """every element [b ld + n, (b + 1) ld) of y and xkn still holds the poison, and no row element does"""
        for f, V in ((self.fy, self.Y), (self.fk, self.K))[:2 if xkn else 1]:
            whole = f.as_strided((self.batch, self.ld), (self.ld, 1))
            assert bool((whole[:, self.n:] == POISON).all()), "padding written"
            assert not bool((V == POISON).any()), "row element not written"
        if not xkn:
            assert bool((self.fk == POISON).all()), "xkn written"

    def check(self, what, xkn=True):
        self.padding_untouched(xkn)
        Y, K, out = self.Y.cpu().numpy(), self.K.cpu().numpy(), self.out.cpu().numpy()
        r, qs, dlt = self.r.cpu().numpy(), self.qs.cpu().numpy(), self.dlt.cpu().numpy()
        for b, row in enumerate(self.rows):
            self.prob.check_row(row, np.ascontiguousarray(Y[b]), np.ascontiguousarray(K[b]) if xkn else None, out[b], what,
                                r=int(r[b]), qs=float(qs[b]), delta=float(dlt[b]) if self.binf else None)

    def triple(self):
        return self.Y.clone(), self.K.clone(), self.out.clone()


# ------------------------------------------------------------------ rows against the single call and the oracle
@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("n", SIZES)
def test_topr_batch_rows_against_the_single_call_and_the_oracle(s, orc, n, binf):
    prob = Problems.get(s, orc, n)
    for batch in BATCHES:
        for pad in PADS:
            for off in ALIGN:
                rows = [3] if batch == 1 else ([0, 1, 2, 3, 4] if pad != 1 else [5, 6, 7, 2, 3])
                lay = Layout(prob, rows, pad, off, binf=binf)
                lay.call(s)
                lay.check("n=%d batch=%d pad=%d off=%s" % (n, batch, pad, off))
    # every row with the r of another one: each kind of data meets r = 1, n/100, n/2, n - 1
    for rot in (2, 5):
        other = Problems.get(s, orc, n, rot=rot)
        for rows in ([0, 1, 2, 3, 4], [5, 6, 7, 3, 4]):
            lay = Layout(other, rows, 0, 0, binf=binf)
            lay.call(s)
            lay.check("n=%d rot=%d" % (n, rot))


# ------------------------------------------------------------------ ties: the index decides
@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("kind", ["const", "lattice", "zeros", "wide"])
@pytest.mark.parametrize("n", [4097, ROW_MAX, ROW_MAX + 1, 2 * ROW_MAX + 3])
def test_topr_batch_tie_data_in_every_form(s, orc, n, kind, binf):
    """five rows of one kind of data with r in the middle of the row, next to both ends and at n/100: a constant |v| (icut decides:
    4097 and 8192 in the resident form, 8193 and 2 * 8192 + 3 -- two index digits -- in the row walk), a lattice, all zeros,
    values over 2^+-500"""
    prob = Problems.get(s, orc, n, rows=5, kinds=[kind], rot=1)       # r = 1, n/100, n/2, n - 1, n
    prob.qs[:] = 1.0
    assert n // 2 in prob.r.tolist()
    for pad, off in ((0, 0), (1, 0), (1, 1)):
        lay = Layout(prob, range(5), pad, off, binf=binf)
        lay.call(s)
        lay.check("%s n=%d pad=%d off=%s" % (kind, n, pad, off))
        if kind == "const":   # the kept entries are the first r
            kept = (lay.K != 0.0).sum(dim=1).cpu().numpy() if not binf else None
            if kept is not None:
                assert kept.tolist() == [min(max(int(r), 0), n) for r in prob.r], (kept, prob.r)
                assert bool((lay.K[2, :n // 2] != 0.0).all()) and bool((lay.K[2, n // 2:] == 0.0).all())


# ------------------------------------------------------------------ the bits
@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("n", [2, 7, 65, 257, 1025, 4097, ROW_MAX, ROW_MAX + 1, 2 * ROW_MAX + 3])
def test_topr_batch_bits_do_not_depend_on_repeat_row_or_batch(s, orc, n, binf):
    """a repeat; the same problem in rows 0 and 3 of a batch of 5 and as a batch of 1: the same bits in y, xkn and the three sums"""
    prob = Problems.get(s, orc, n)
    for pad, off in ((0, 0), (2, 0), (1, 0), (1, 1), (0, "mixed")):
        for p in (2, 3, 6):
            rows = [p, 0, 1, p, 5]
            a, b = Layout(prob, rows, pad, off, binf=binf), Layout(prob, rows, pad, off, binf=binf)
            a.call(s); b.call(s); a.call(s)
            assert _same(a.triple(), b.triple()), (n, pad, off)
            assert _same((a.Y[0], a.K[0], a.out[0]), (a.Y[3], a.K[3], a.out[3])), (n, pad, off, p)
            # (with an odd ld the single row of batch 1 is handed ld = n and may fall into another alignment class than the larger
            #  batch: y and xkn keep their bits there -- the selection is exact -- and the sums are compared within the class only)
            one = Layout(prob, [p], pad, off, binf=binf)
            one.call(s)
            assert _bits(one.Y[0], a.Y[0]) and _bits(one.K[0], a.K[0]), (n, pad, off, p)
            assert one.out[0, 0].item() == a.out[0, 0].item()
            if one.pairs == a.pairs:
                assert _bits(one.out[0], a.out[0]), (n, pad, off, p)


@pytest.mark.parametrize("n", [7, 64, 1000, ROW_MAX - 1, ROW_MAX + 2])
def test_topr_batch_xkn_absent_and_misaligned_alone(s, orc, n):
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
@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("n", [1, 2, 7, 65, 255, 257, 1025, 4097, ROW_MAX, ROW_MAX + 1, 2 * ROW_MAX + 3])
def test_topr_batch_guard_bands_and_padding(s, orc, n, binf):
    """every vector between guard bands, poison everywhere: after the call the guard bands (and the inputs) are unchanged, every
    padding element still holds the poison and no row element does"""
    prob = Problems.get(s, orc, n)
    for batch, pad, off in ((1, 0, 0), (1, 6, 1), (5, 0, 1), (5, 1, 0), (5, 6, 0), (5, 6, "mixed"), (5, 1, 1)):
        lay = Layout(prob, [3, 2, 7, 1, 4][:batch], pad, off, guarded=True, binf=binf)
        lay.call(s)
        lay.zone.check()
        for g in lay.zone.bufs[2:]:   # q, xk, sj: read only
            assert bool((g.buf == g.snap).all()), g.name
        lay.check("guarded n=%d batch=%d pad=%d off=%s" % (n, batch, pad, off))


# ------------------------------------------------------------------ more problems than CUs, more than 65535 rows
@pytest.mark.parametrize("batch,n", [(300, 15), (70001, 2)])
def test_topr_batch_many_rows(s, orc, batch, n):
    """the rows repeat three problems (problem = row % 3): a sample of rows against the single call and the oracle, ALL rows
    against the batch-of-1 call on their problem"""
    import torch
    prob = Problems.get(s, orc, n, rows=batch, distinct=3, rot=1)
    rng = np.random.default_rng(batch)
    rows = sorted({0, 1, 2, batch - 1} | set(rng.choice(batch, size=9, replace=False).tolist()))
    for pad, off in ((0, 0), (1, 1)):
        lay = Layout(prob, range(batch), pad, off)
        lay.call(s)
        lay.padding_untouched()
        Y, K, out = lay.Y.cpu().numpy(), lay.K.cpu().numpy(), lay.out.cpu().numpy()
        for r in rows:
            prob.check_row(r % 3, np.ascontiguousarray(Y[r]), np.ascontiguousarray(K[r]), out[r], "batch=%d" % batch)
        for p in range(3):
            one = Layout(prob, [p], 0 if lay.pairs else pad, off)
            one.call(s)
            assert one.pairs == lay.pairs
            mine = torch.arange(p, batch, 3, device="cuda:0")
            for got, want in ((lay.Y, one.Y), (lay.K, one.K), (lay.out, one.out)):
                g = got[mine].contiguous().view(torch.int64)
                assert bool((g == want[0].contiguous().view(torch.int64)[None, :]).all()), (batch, p, pad, off)
    Problems._cache.clear()


def test_topr_batch_the_n_bound(s, orc):
    """n = 2^20 with batch 1 runs (the row walk) and has the single call's bits; n = 2^20 + 1 is refused and the text names the
    single call"""
    import torch
    prob = Problems.get(s, orc, N_MAX, rows=1, kinds=["gauss"], rot=3)    # r = n / 2
    for binf in (False, True):
        lay = Layout(prob, [0], 0, 0, binf=binf)
        lay.call(s)
        lay.check("n=2^20")
    Problems._cache.clear()
    L, G, ctx = s._lib.load(), s._lib.load_topr_batch(), s.context("cuda:0")
    n = N_MAX + 1
    v = [torch.full((n,), POISON, dtype=torch.float64, device="cuda:0") for _ in range(5)]
    par = torch.ones(2, dtype=torch.float64, device="cuda:0")
    r = torch.ones(1, dtype=torch.int64, device="cuda:0")
    out = torch.full((3,), POISON, dtype=torch.float64, device="cuda:0")
    rc = G.spx_proxstep_indball_l0_batch(ctx, _P(v[0]), _P(v[1]), _P(v[2]), _P(v[3]), n, 1, n, _P(r), _P(par[0:1]), _P(v[4]), _P(out))
    assert rc == INVALID and b"spx_prox_indball_l0 " in L.spx_last_error()
    rc = G.spx_proxstep_indball_l0_binf_batch(ctx, _P(v[0]), _P(v[1]), _P(v[2]), _P(v[3]), n, 1, n, _P(r), _P(par[1:2]), _P(par[0:1]),
                                              _P(v[4]), _P(out))
    assert rc == INVALID and b"spx_prox_indball_l0_binf " in L.spx_last_error()
    torch.cuda.synchronize()
    assert bool((v[0] == POISON).all()) and bool((v[4] == POISON).all()) and bool((out == POISON).all())


# ------------------------------------------------------------------ isolation under non-finite data
@pytest.mark.parametrize("n", [65, 1025, ROW_MAX + 2])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf"), 1e150])
def test_topr_batch_nonfinite_row_is_isolated(s, orc, n, value):
    """NaN, +-Inf, 1e150 in one element of ONE row of a batch of 3 -- element 0, the scalar tail, another tile -- of q, xk or sj,
    in the sequence clean / planted / clean: the planted row has the single call's bits (a NaN for a NaN), the other rows and
    the clean call behind keep the bits of the clean call in front"""
    import torch
    prob = Problems.get(s, orc, n, rot=5)
    rows = [6, 2, 7]                                           # the planted row: Gaussian, r = n / 2
    assert prob.r[6] == n // 2 and prob.kinds[6] == "gauss"
    for pad, off in ((0, 0), (1, 1)):
        for binf in (False, True):
            clean = Layout(prob, rows, pad, off, binf=binf)
            clean.call(s)
            for where in ("q", "xk", "sj"):
                for at in (0, n - 1, (3 * n) // 4):
                    lay = Layout(prob, rows, pad, off, binf=binf)
                    {"q": lay.Q, "xk": lay.X, "sj": lay.S}[where][0, at] = value
                    lay.call(s)
                    lay.padding_untouched()
                    what = "n=%d %r in %s[%d] pad=%d off=%d" % (n, value, where, at, pad, off)
                    qh = torch.from_numpy(prob.qs[6] * lay.Q[0].cpu().numpy()).cuda()
                    y = prob.single(qh, lay.X[0], lay.S[0], prob.r[6], prob.dlt[6] if binf else None).cpu().numpy()
                    got = lay.Y[0].cpu().numpy()
                    assert nonfinite.same_bits_or_both_nan(got, y).all(), what
                    xh, sh = lay.X[0].cpu().numpy(), lay.S[0].cpu().numpy()
                    with np.errstate(all="ignore"):
                        w = (xh + sh) + got
                    assert nonfinite.same_bits_or_both_nan(lay.K[0].cpu().numpy(), w).all(), what
                    assert lay.out[0, 0].item() == float(np.count_nonzero(w != 0.0)), what       # NaN counts as nonzero
                    for b in (1, 2):
                        assert _bits(lay.Y[b], clean.Y[b]) and _bits(lay.K[b], clean.K[b]) and _bits(lay.out[b], clean.out[b]), what
            after = Layout(prob, rows, pad, off, binf=binf)
            after.call(s)
            assert _same(after.triple(), clean.triple()), (n, value, pad, off)


# ------------------------------------------------------------------ degenerate radius
@pytest.mark.parametrize("n", [65, 1025, ROW_MAX + 2])
@pytest.mark.parametrize("delta", [0.0, -1.0, float("nan"), float("inf")])
def test_topr_batch_degenerate_radius_in_one_row(s, orc, n, delta):
    """Delta = 0, -1, NaN, +Inf in ONE row: the call returns, the other rows keep their bits, the guard bands are intact, and
    that row's y is what the single call gives with the same Delta"""
    import torch
    prob = Problems.get(s, orc, n, rot=5)
    rows = [6, 2, 7]                                           # the degenerate row: Gaussian, r = n / 2
    clean = Layout(prob, rows, 2, 0)
    clean.call(s)
    lay = Layout(prob, rows, 2, 0, guarded=True)
    lay.dlt[0] = delta
    lay.call(s)
    torch.cuda.synchronize()
    lay.zone.check()
    whole = lay.fy.as_strided((3, lay.ld), (lay.ld, 1))
    assert bool((whole[:, n:] == POISON).all())
    for b in (1, 2):
        assert _bits(lay.Y[b], clean.Y[b]) and _bits(lay.K[b], clean.K[b]) and _bits(lay.out[b], clean.out[b]), (n, delta, b)
    qh = torch.from_numpy(prob.qs[6] * prob.Q[6]).cuda()
    y = prob.single(qh, prob.Xd[6], prob.SJd[6], prob.r[6], delta).cpu().numpy()
    assert nonfinite.same_bits_or_both_nan(lay.Y[0].cpu().numpy(), y).all(), (n, delta)


def test_topr_batch_q_scale(s, orc):
    """q_scale[b] = 0 and a negative one in one row: the prox at q_scale q against the single call and the oracle; [1] sums q AS
    PASSED times y; the other rows keep their bits"""
    for n in (65, 1025, ROW_MAX + 2):
        prob = Problems.get(s, orc, n)
        rows = [2, 3, 1, 6]
        clean = Layout(prob, rows, 0, 0)
        clean.call(s)
        for qs in (0.0, -1.25):
            lay = Layout(prob, rows, 0, 0)
            lay.qs[3] = qs
            lay.r[3] = n // 2
            lay.call(s)
            lay.check("n=%d q_scale=%g" % (n, qs))
            for b in (0, 1, 2):
                assert _bits(lay.Y[b], clean.Y[b]) and _bits(lay.out[b], clean.out[b]), (n, qs, b)


# ------------------------------------------------------------------ refusals and empties
@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
def test_topr_batch_refusals_and_empties(s, orc, binf):
    import torch
    n, batch = 65, 3
    prob = Problems.get(s, orc, n)
    L, G, ctx = s._lib.load(), s._lib.load_topr_batch(), s.context("cuda:0")
    lay = Layout(prob, range(batch), 1, 0, binf=binf)
    ld = lay.ld
    y, q, xk, sj, k = (_P(f) for f in (lay.fy, lay.fq, lay.fx, lay.fs, lay.fk))
    r, dlt, qs, out = _P(lay.r), _P(lay.dlt), _P(lay.qs), _P(lay.out)
    Z = None

    def call(y=y, q=q, xk=xk, sj=sj, n=n, batch=batch, ld=ld, r=r, dlt=dlt, qs=qs, k=k, out=out):
        if binf:
            return G.spx_proxstep_indball_l0_binf_batch(ctx, y, q, xk, sj, n, batch, ld, r, dlt, qs, k, out)
        return G.spx_proxstep_indball_l0_batch(ctx, y, q, xk, sj, n, batch, ld, r, qs, k, out)

    def untouched():
        torch.cuda.synchronize()
        return bool((lay.fy == POISON).all()) and bool((lay.fk == POISON).all()) and bool((lay.out == POISON).all())

    def next_call_is_right():
        assert call() == 0
        lay.check("after a refusal")
        lay.fy.fill_(POISON); lay.fk.fill_(POISON); lay.out.fill_(POISON)

    refusals = [
        ("y == q", lambda: call(y=q)), ("y == xk", lambda: call(y=xk)), ("y == sj", lambda: call(y=sj)),
        ("xkn == y", lambda: call(k=y)), ("xkn == q", lambda: call(k=q)),
        ("xkn == xk", lambda: call(k=xk)), ("xkn == sj", lambda: call(k=sj)), ("ld < n", lambda: call(ld=n - 1)),
        ("n < 0", lambda: call(n=-1)), ("batch < 0", lambda: call(batch=-1)),
        ("n > 2^20", lambda: call(n=N_MAX + 1, ld=N_MAX + 1)), ("batch > 2^31 - 1", lambda: call(batch=1 << 31)),
        ("r NULL", lambda: call(r=Z)), ("q_scale NULL", lambda: call(qs=Z)), ("stats_dev NULL", lambda: call(out=Z)),
        ("r NULL, n == 0", lambda: call(n=0, r=Z)), ("stats_dev NULL, n == 0", lambda: call(n=0, out=Z)),
    ]
    if binf:
        refusals.append(("delta NULL", lambda: call(dlt=Z)))
    for what, f in refusals:
        assert f() == INVALID, what
        assert L.spx_last_error(), what
        assert untouched(), what
        next_call_is_right()
    # empties: batch == 0 does nothing; n == 0 stores 3 * batch zeros (by a kernel)
    assert call(batch=0) == 0 and call(batch=0, r=Z, dlt=Z, qs=Z, out=Z) == 0 and untouched()
    next_call_is_right()
    for kw in (dict(n=0, ld=0), dict(n=0, ld=5), dict(n=0, ld=0, y=Z, q=Z, xk=Z, sj=Z, k=Z)):
        assert call(**kw) == 0, kw
        torch.cuda.synchronize()
        assert bool((lay.out == 0.0).all()) and bool((lay.fy == POISON).all()) and bool((lay.fk == POISON).all()), kw
        lay.out.fill_(POISON)
    next_call_is_right()
    # the mirror refuses what it can see
    d = dict(delta=lay.dlt) if binf else {}
    with pytest.raises(TypeError):
        s.prox_step_topr_batch_bang(lay.Y, lay.Y, lay.X, lay.S, lay.r, lay.qs, **d)
    with pytest.raises(TypeError):
        s.prox_step_topr_batch_bang(lay.Y, lay.Q, lay.Y, lay.S, lay.r, lay.qs, **d)
    with pytest.raises(TypeError):
        s.prox_step_topr_batch_bang(lay.Y, lay.Q, lay.X, lay.S, lay.r[:2], lay.qs, **d)                 # two r
    with pytest.raises(TypeError):
        s.prox_step_topr_batch_bang(lay.Y, lay.Q, lay.X, lay.S, lay.r.to(torch.float64), lay.qs, **d)   # r is not int64
    with pytest.raises(TypeError):
        s.prox_step_topr_batch_bang(lay.Y, lay.Q, lay.X, lay.S, 3, lay.qs, **d)                         # a host r
    with pytest.raises(TypeError):
        s.prox_step_topr_batch_bang(lay.Y, lay.Q, lay.X, lay.S, lay.r.cpu(), lay.qs, **d)
    with pytest.raises(TypeError):
        s.prox_step_topr_batch_bang(lay.Y, lay.Q, lay.X, lay.S, lay.r, lay.qs, delta=0.3)               # a host radius
    with pytest.raises(TypeError):
        s.prox_step_topr_batch_bang(lay.Y, lay.Q.contiguous(), lay.X, lay.S, lay.r, lay.qs, **d)        # another row stride
    Yn, outn = s.prox_step_topr_batch(lay.Q, lay.X, lay.S, lay.r, lay.qs, **d)
    lay.call(s)
    assert _bits(Yn, lay.Y) and Yn.stride() == lay.Q.stride() and _bits(outn, lay.out)


# ------------------------------------------------------------------ the parameters follow the device
@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("n", [1000, 10000], ids=["row-resident", "row-walk"])
def test_captured_topr_batch_call_follows_the_device_parameters(s, orc, n, binf):
    """one batched call captured COLD into a graph on a side stream (a single kernel node); between replays r, Delta and q_scale
    are overwritten ON THE DEVICE: every replay equals an eager call at the new values, bit for bit, and the single call"""
    import torch
    rng = np.random.default_rng(6200 + n)
    prob = Problems.get(s, orc, n)
    rows = [2, 3, 6]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        lay = Layout(prob, rows, 2, 0, binf=binf)
        s.context("cuda:0")   # the stream's context exists before the capture (creating one allocates) ...
        if not binf and n == 1000:
            lay.call(s)   # ... one of the four cases warm; the others are captured COLD: the call was never made on this context
    side.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, stream=side):
        lay.call(s)
    assert _graph_kernel_nodes(g) == (1, 1)                     # (nodes, kernel nodes): no memset node, no second kernel
    g.instantiate()
    for rep in range(3):
        r = np.array([prob.r[k] for k in rows]) if rep == 0 else rng.integers(1, n, size=3)
        qs = np.array([prob.qs[k] for k in rows]) if rep == 0 else rng.uniform(0.5, 1.5, size=3)
        dlt = np.array([prob.dlt[k] for k in rows]) * (1.0 if rep == 0 else rng.uniform(0.25, 4.0, size=3))
        for t, a in ((lay.r, r.astype(np.int64)), (lay.dlt, dlt), (lay.qs, qs)):
            t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        lay.fy.fill_(POISON); lay.fk.fill_(POISON); lay.out.fill_(POISON)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        lay.check("captured n=%d rep=%d" % (n, rep))
        eager = Layout(prob, rows, 2, 0, binf=binf)
        for t, a in ((eager.r, r.astype(np.int64)), (eager.dlt, dlt), (eager.qs, qs)):
            t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        eager.call(s)
        assert _same(lay.triple(), eager.triple()), (n, rep)


def _graph_kernel_nodes(g):
    """(nodes, kernel nodes) of a captured torch graph (keep_graph=True), asked of the HIP runtime the process already runs on"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert len(paths) == 1, paths                # one HIP runtime in the process: the graph handle is its own
    hip = ctypes.CDLL(paths[0])
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    handle = ctypes.c_void_p(g.raw_cuda_graph())
    count = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(handle, None, ctypes.byref(count)) == 0
    nodes = (ctypes.c_void_p * max(count.value, 1))()
    assert hip.hipGraphGetNodes(handle, nodes, ctypes.byref(count)) == 0
    kernels = 0
    for node in nodes[:count.value]:
        kind = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kind)) == 0
        kernels += kind.value == 0     # hipGraphNodeTypeKernel
    return count.value, kernels
