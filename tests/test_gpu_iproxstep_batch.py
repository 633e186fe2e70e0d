"""GPU: batched iprox! + step statistics with the per-problem scalars on the device (spx_iproxstep_{l1,l0}[_box]_batch,
iprox_step_batch / iprox_step_batch_bang).

Problem b is row b of the batch x n tensors (row stride ld >= n); lambda_b, the box [-Delta_b, Delta_b] and d_shift_b are read
from device arrays by the kernel that stores y, which sees deff = d + d_shift_b (one rounded add) in place of d.  Every row is held
to the SINGLE call (spx_iproxstep_X through the C ABI) on that row alone with the host copies of the scalars and the vector
torch.add(d_row, d_shift[b]) formed beforehand: y and xkn bit for bit (torch.equal), the four sums to the project's bars for
these blocked sums (test_gpu_iproxstep.py: NormL0's [0] exactly lambda_b * count; else |got - ref| <= 1e-12 * sum of the
magnitudes of the terms, ref = math.fsum of the host's rounded terms -- the library is built without contraction).

Sizes sit at the edges of the kernels: a tile is 3072 elements (256 lanes x 6 pairs), one workgroup owns a problem up to
R = kBatchRowMax = 12288 elements (the row form), beyond it one workgroup takes one tile and a second launch adds the
partials (the tiled form).  A row is peeled by the parity of b * ld plus the bases' alignment: head of 0 / 1 elements, pairs,
tail of 0 / 1 -- so ld - n in {0, 1, 2, 3} and bases on / 8 bytes off a 16-byte boundary reach every combination.
lambda ~ U(0.3, 1.5) per row.  Box forms: d has positive and negative entries and entries that are exactly -d_shift[b] (exactly 0
without d_shift), so that |deff| <= eps occurs; unboxed forms: deff > 0 (with d_shift, d itself is negative in places).  Every
case runs with and without d_shift."""
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
FLAG_POISON = 7
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
    """`rows` problems of n elements (one draw per row), their scalars, one shared mask, the four d matrices (box or not, to be
    shifted or not) and -- computed once per (operator, shifted), shared by every test that places these rows somewhere -- what
    the single call gives on each row: y, xkn (device, rows x n) and the reference sums."""
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
        self.G = rng.normal(size=(rows, n))
        self.lam, self.dl, self.shift = (rng.uniform(0.3, 1.5, size=rows) for _ in range(3))
        self.mask = np.zeros(n, dtype=np.uint8)
        self.mask[rng.choice(n, size=max(1, n // 3), replace=False)] = 1
        zero_at = rng.choice(n, size=max(1, n // 7), replace=False)   # where deff is exactly 0 in the box forms
        box = rng.normal(size=(rows, n))
        box_shifted = box.copy()
        box[:, zero_at] = 0.0
        box_shifted[:, zero_at] = -self.shift[:, None]
        # (box, shifted) -> d.  Unboxed: deff > 0 -- d in (0.1, 2) as it is, d in (-0.2, 2) under a shift >= 0.3
        self.D = {(True, False): box, (True, True): box_shifted,
                  (False, False): rng.uniform(0.1, 2.0, size=(rows, n)), (False, True): rng.uniform(-0.2, 2.0, size=(rows, n))}
        dev = lambda a: torch.from_numpy(a).cuda()
        self.Xd, self.SJd, self.Gd = dev(self.X), dev(self.SJ), dev(self.G)
        self.Dd = {k: dev(v) for k, v in self.D.items()}
        self.maskd = dev(self.mask)
        self.shiftd = dev(self.shift)
        self.refs = {}

    def deff(self, box, shifted, r, d=None, shift=None):
        """the vector the single call is given: torch.add(d_row, d_shift[b]) on the device, or d_row itself"""
        import torch
        d = self.Dd[(box, shifted)][r] if d is None else d
        if not shifted:
            return d
        return torch.add(d, float(self.shift[r] if shift is None else shift))

    def single(self, op, r, de, g=None, xk=None, sj=None, scal=None):
        """spx_iproxstep_X on row r alone (or on the given vectors / (lam, dl)) with d = de: (y, xkn, [h, gy, ydy, yy])"""
        import torch
        s = self.s
        kind, box, msk = op
        L, ctx = s._lib.load(), s.context("cuda:0")
        g = self.Gd[r] if g is None else g
        xk = self.Xd[r] if xk is None else xk
        sj = self.SJd[r] if sj is None else sj
        lam, dl = scal if scal is not None else (self.lam[r], self.dl[r])
        n = g.numel()
        y, k = torch.full_like(g, POISON), torch.full_like(g, POISON)
        st = (ctypes.c_double * 4)()
        if box:
            rc = getattr(L, "spx_iproxstep_%s_box" % kind)(ctx, _P(y), _P(g), _P(de), _P(xk), _P(sj), n, float(lam), None, None,
                                                           -float(dl), float(dl), _P(self.maskd) if msk else None, _P(k), st, None)
        else:
            rc = getattr(L, "spx_iproxstep_" + kind)(ctx, _P(y), _P(g), _P(de), _P(xk), _P(sj), n, float(lam), 0, _P(k), st, None)
        assert rc == 0, s._lib.load().spx_last_error()
        return y, k, [st[0], st[1], st[2], st[3]]

    def ref(self, op, shifted):
        """per (operator, shifted): (Y rows x n, XKN rows x n on the device, reference sums per row)"""
        import torch
        key = (op, shifted)
        if key not in self.refs:
            ys, ks, sums = [], [], []
            for r in range(self.rows):
                de = self.deff(op[1], shifted, r)
                y, k, _ = self.single(op, r, de)
                ys.append(y); ks.append(k)
                sums.append(self.sum_refs(op, r, y.cpu().numpy(), k.cpu().numpy(), de.cpu().numpy()))
            self.refs[key] = (torch.stack(ys), torch.stack(ks), sums)
        return self.refs[key]

    def sum_refs(self, op, r, y, v, de, g=None, lam=None):
        """exactly rounded references from the host copies: v = (xk + sj) + y as stored, de = deff as the single call saw it"""
        kind, box, msk = op
        g = self.G[r] if g is None else g
        lam = self.lam[r] if lam is None else lam
        sel = self.mask.astype(bool) if msk else np.ones(y.size, dtype=bool)
        if kind == "l0":
            h = lam * float(np.count_nonzero(v[sel]))
            hm = 0.0
        else:
            hm = math.fsum(np.abs(v[sel]))
            h = lam * hm
        gy, ydy = g * y, (de * y) * y
        return h, lam * hm, math.fsum(gy), math.fsum(np.abs(gy)), math.fsum(ydy), math.fsum(np.abs(ydy)), math.fsum(y * y)


def _check_stats(op, got, ref, what):
    h, hm, gy, mgy, ydy, mydy, yy = ref
    g0, g1, g2, g3 = (float(v) for v in got)
    if op[0] == "l0":
        assert g0 == h, (what, g0, h)
    else:
        assert abs(g0 - h) <= TOL * max(hm, 1e-300), (what, g0, h)
    assert abs(g1 - gy) <= TOL * mgy, (what, g1, gy, mgy)
    assert abs(g2 - ydy) <= TOL * mydy, (what, g2, ydy, mydy)
    assert abs(g3 - yy) <= TOL * yy, (what, g3, yy)


NAMES = ("y", "xkn", "g", "d", "xk", "sj")


class Layout:
    """the six batch x n tensors of a call as views of flat poisoned buffers: row stride ld = n + pad, bases `off` (0 / 1)
    elements past a 256-byte boundary (`odd`: the names of the vectors that sit at 1 - off instead), rows = the problem rows
    placed at batch rows 0, 1, ...; d is the matrix of (box, shifted)"""

    def __init__(self, prob, rows, pad, off, box, shifted, odd=(), guarded=False):
        import torch
        self.prob, self.rows, self.n, self.batch = prob, list(rows), prob.n, len(rows)
        self.box, self.shifted = box, shifted
        self.ld = ld = prob.n + pad
        total = self.batch * ld
        self.zone = redzone.Zone() if guarded else None

        def flat(name):
            o = 1 - off if name in odd else off
            if guarded:   # [front guard | batch * ld elements | back guard], poison everywhere
                return self.zone.add(total, torch.float64, align_bytes=8 * o, role="inout", poison=POISON, name=name,
                                     data=torch.full((total,), POISON, dtype=torch.float64)).t
            return torch.full((total + 2,), POISON, dtype=torch.float64, device="cuda:0")[o:o + total]

        self.fy, self.fk, self.fg, self.fd, self.fx, self.fs = (flat(nm) for nm in NAMES)
        view = lambda f: f.as_strided((self.batch, self.n), (ld, 1))
        self.Y, self.K, self.G, self.D, self.X, self.S = (view(f) for f in (self.fy, self.fk, self.fg, self.fd, self.fx, self.fs))
        idx = torch.as_tensor(self.rows, device="cuda:0")
        self.G.copy_(prob.Gd[idx]); self.X.copy_(prob.Xd[idx]); self.S.copy_(prob.SJd[idx]); self.D.copy_(prob.Dd[(box, shifted)][idx])
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[self.rows])).cuda()
        self.lam, self.dl, self.shift = dev(prob.lam), dev(prob.dl), dev(prob.shift)
        self.out = torch.full((self.batch, 4), POISON, dtype=torch.float64, device="cuda:0")
        self.flag = torch.full((self.batch,), FLAG_POISON, dtype=torch.int32, device="cuda:0")
        if guarded:
            for g in self.zone.bufs:
                g.snap = g.buf.clone()   # (the inputs were copied in after the snapshot was taken)

    def call(self, s, op, xkn=True):
        kind, box, msk = op
        assert box == self.box
        return s.iprox_step_batch_bang(self.Y, kind, self.G, self.D, self.X, self.S, self.lam,
                                       d_shift=self.shift if self.shifted else None,
                                       l=-self.dl if box else None, u=self.dl if box else None,
                                       selected=self.prob.maskd if msk else None, xkn=self.K if xkn else None, out=self.out,
                                       d_flag=None if box else self.flag)

    def padding_untouched(self):
        """every element [b ld + n, (b + 1) ld) of y and xkn still holds the poison, and no row element does"""
        for f, V in ((self.fy, self.Y), (self.fk, self.K)):
            whole = f.as_strided((self.batch, self.ld), (self.ld, 1))
            assert bool((whole[:, self.n:] == POISON).all()), "padding written"
            assert not bool((V == POISON).any()), "row element not written"

    def check(self, s, op, what, stats=True):
        import torch
        Yr, Kr, sums = self.prob.ref(op, self.shifted)
        idx = torch.as_tensor(self.rows, device="cuda:0")
        assert torch.equal(self.Y, Yr[idx]), what
        assert torch.equal(self.K, Kr[idx]), what
        self.padding_untouched()
        if not self.box:
            assert bool((self.flag == 0).all()), (what, self.flag.tolist())   # deff > 0 everywhere: every word cleared
        if stats:
            got = self.out.cpu().numpy()
            for b, r in enumerate(self.rows):
                _check_stats(op, got[b], sums[r], "%s row %d" % (what, b))


# ------------------------------------------------------------------ parity with the single call
@pytest.mark.parametrize("n", SIZES)
def test_ibatch_rows_equal_the_single_call(s, n):
    prob = Problems.get(s, n, 8100 + n)
    for op in OPS:
        for shifted in (False, True):
            for batch in BATCHES:
                for pad in (0, 1, 2, 3):
                    for off in (0, 1):
                        lay = Layout(prob, range(batch), pad, off, op[1], shifted)
                        lay.call(s, op)
                        lay.check(s, op, "%s shifted=%d n=%d batch=%d pad=%d off=%d" % (op, shifted, n, batch, pad, off))


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
def test_ibatch_without_xkn(s, op):
    """xkn = None: y and the sums as with it"""
    import torch
    for n in (3073, R + 3073):
        prob = Problems.get(s, n, 8100 + n)
        for shifted in (False, True):
            lay = Layout(prob, range(3), 1, 0, op[1], shifted)
            lay.call(s, op, xkn=False)
            assert torch.equal(lay.Y, prob.ref(op, shifted)[0][:3]) and bool((lay.fk == POISON).all())
            got = lay.out.cpu().numpy()
            for b in range(3):
                _check_stats(op, got[b], prob.ref(op, shifted)[2][b], "no xkn n=%d row %d" % (n, b))


# ------------------------------------------------------------------ padding and ends
@pytest.mark.parametrize("n", [1, 3, 513, 3073, R + 1])
def test_ibatch_guard_bands_and_padding(s, n):
    """all six vectors between guard bands, poison everywhere: after the call the guard bands (and the inputs) are unchanged,
    every padding element still holds the poison and no row element does"""
    prob = Problems.get(s, n, 8100 + n)
    for op in (OPS[0], OPS[1], OPS[5], OPS[3]):
        for shifted in (False, True):
            for batch, pad, off in ((1, 0, 0), (1, 3, 1), (3, 0, 1), (3, 1, 0), (3, 1, 1), (3, 2, 1), (7, 3, 0)):
                lay = Layout(prob, range(batch), pad, off, op[1], shifted, guarded=True)
                lay.call(s, op)
                lay.zone.check()     # guard bands of y, xkn, g, d, xk, sj
                for g in lay.zone.bufs[2:]:   # g, d, xk, sj: read only
                    assert bool((g.buf == g.snap).all()), g.name
                lay.check(s, op, "guarded %s shifted=%d n=%d batch=%d pad=%d off=%d" % (op, shifted, n, batch, pad, off))


# ------------------------------------------------------------------ placement independence
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("n", [513, 3073, R + 3073])
def test_ibatch_bits_do_not_depend_on_placement(s, op, n):
    """the same problem at row 0 of batch 1, row 2 of batch 3, row 6 of batch 7 (rows of one parity, same ld, same bases): the
    same bits in y, xkn and the four sums"""
    import torch
    prob = Problems.get(s, n, 8100 + n)
    for pad, off, shifted in ((1, 0, True), (2, 1, False)):
        seen = None
        for rows, at in (([4], 0), ([0, 1, 4], 2), ([0, 1, 2, 3, 5, 6, 4], 6)):
            lay = Layout(prob, rows, pad, off, op[1], shifted)
            lay.call(s, op)
            cur = (lay.Y[at].clone(), lay.K[at].clone(), lay.out[at].clone())
            if seen is not None:
                assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(seen, cur)), (op, n, pad, off, at)
            seen = cur


# ------------------------------------------------------------------ more problems than CUs, more than 65535 rows
@pytest.mark.parametrize("batch,n", [(300, 5), (70001, 3)])
def test_ibatch_many_rows(s, batch, n):
    import torch
    prob = Problems.get(s, n, 8300 + batch, rows=batch)
    rng = np.random.default_rng(batch)
    rows = sorted({0, batch - 1} | set(rng.choice(batch, size=50, replace=False).tolist()))
    for op, shifted in ((OPS[1], True), (OPS[3], False), (OPS[0], False), (OPS[5], True)):
        for pad, off in ((0, 0), (1, 1)):
            lay = Layout(prob, range(batch), pad, off, op[1], shifted)
            lay.call(s, op)
            lay.padding_untouched()
            if not op[1]:
                assert bool((lay.flag == 0).all())
            got = lay.out.cpu().numpy()
            for r in rows:
                de = prob.deff(op[1], shifted, r)
                y, k, _ = prob.single(op, r, de)
                assert torch.equal(lay.Y[r], y) and torch.equal(lay.K[r], k), (op, batch, r)
                _check_stats(op, got[r], prob.sum_refs(op, r, y.cpu().numpy(), k.cpu().numpy(), de.cpu().numpy()),
                             "%s batch=%d row %d" % (op, batch, r))


def test_ibatch_more_partials_than_one_pass_adds(s):
    """n = 2048 tiles + 1 element: the per-problem reduction takes its long loop (more than 2048 partials a plane)"""
    import torch
    n = 2048 * TILE + 1
    prob = Problems.get(s, n, 8400, rows=2)
    op = OPS[2]
    lay = Layout(prob, range(2), 1, 0, True, True)
    lay.call(s, op)
    lay.padding_untouched()
    got = lay.out.cpu().numpy()
    for r in range(2):
        de = prob.deff(True, True, r)
        y, k, st = prob.single(op, r, de)
        assert torch.equal(lay.Y[r], y) and torch.equal(lay.K[r], k), r
        if r == 1:
            _check_stats(op, got[r], prob.sum_refs(op, r, y.cpu().numpy(), k.cpu().numpy(), de.cpu().numpy()), "long reduce row %d" % r)
    Problems._cache.pop((n, 8400, 2))   # (most of a gigabyte of rows)


# ------------------------------------------------------------------ mixed base alignment: the element-wise form
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("n", [3073, R + 3073])
def test_ibatch_mixed_alignment_takes_the_elementwise_form(s, op, n):
    """xkn (or d alone) 8 bytes off while the others are aligned, and the reverse: the same y and xkn bits, the sums to the fsum
    bars"""
    prob = Problems.get(s, n, 8100 + n)
    for off, odd, shifted in ((0, ("xkn",), True), (1, ("xkn",), False), (0, ("d",), False), (1, ("d", "g"), True)):
        for pad in (0, 1):
            lay = Layout(prob, range(3), pad, off, op[1], shifted, odd=odd)
            lay.call(s, op)
            lay.check(s, op, "mixed %s n=%d pad=%d off=%d odd=%s" % (op, n, pad, off, odd))


# ------------------------------------------------------------------ d_flag: the reference's `@assert d[i] > 0`, per problem
@pytest.mark.parametrize("n", [R - 1, R + 3073], ids=["row-form", "tiled-form"])
@pytest.mark.parametrize("kind", ["l1", "l0"])
def test_ibatch_d_flag_names_the_row(s, n, kind):
    """a deff <= 0 or NaN planted at element 0, in the scalar tail, or in the third tile of ONE row raises that row's word only
    (the words held FLAG_POISON before: the call clears them); y keeps the single call's bits; a clean call afterwards on the
    same d_flag leaves all zeros.  Without d_shift a -0.0 is among the planted values: d enters as it is (a `+ 0.0` would make
    it +0.0 and flip the sign of -g / d)."""
    import torch
    prob = Problems.get(s, n, 8100 + n)
    op = (kind, False, False)
    pad, off = 1, 0          # ld even, n odd: every row starts on a pair and ends in a scalar tail
    for shifted in (False, True):
        Yr, Kr, _ = prob.ref(op, shifted)
        for where in (0, n - 1, 2 * TILE + 17):
            for kind_of in ("zero", "negative", "nan") + (() if shifted else ("minus-zero",)):
                lay = Layout(prob, range(3), pad, off, False, shifted)
                sh = float(prob.shift[1]) if shifted else 0.0
                value = {"zero": 0.0 - sh, "negative": -sh - 1.5, "nan": float("nan"), "minus-zero": -0.0}[kind_of]
                lay.D[1, where] = value
                lay.call(s, op)
                what = (kind, n, shifted, where, kind_of)
                assert lay.flag.tolist() == [0, 1, 0], (what, lay.flag.tolist())
                y, k, _ = prob.single(op, 1, prob.deff(False, shifted, 1, d=lay.D[1].clone()))
                assert torch.equal(lay.Y[1].view(torch.int64), y.view(torch.int64)), what
                assert torch.equal(lay.K[1].view(torch.int64), k.view(torch.int64)), what
                for b in (0, 2):
                    assert torch.equal(lay.Y[b], Yr[b]) and torch.equal(lay.K[b], Kr[b]), what
                lay.padding_untouched()
                # a clean call afterwards on the same d_flag leaves all zeros
                lay.D[1, where] = prob.Dd[(False, shifted)][1, where]
                lay.call(s, op)
                assert lay.flag.tolist() == [0, 0, 0], what
                assert torch.equal(lay.Y, Yr[:3]), what


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
def test_ibatch_nonfinite_row_is_isolated(s, n, value):
    """NaN, +Inf, 1e150 at element 0 and in the tail of ONE row of a batch of 3, in the sequence clean / planted / clean on one
    context: the planted row behaves as spx_iproxstep_X does on it, the other rows keep the bits of the clean call -- y, xkn, the
    sums and the flag -- and the clean call afterwards gives what the first gave"""
    import torch
    prob = Problems.get(s, n, 8100 + n)
    bits = lambda t: t.contiguous().view(torch.int64)
    for op in (OPS[0], OPS[3], OPS[5]):
        box = op[1]
        for pad, off, shifted in ((0, 0, True), (1, 1, False)):
            clean = Layout(prob, range(3), pad, off, box, shifted)
            clean.call(s, op)
            clean.check(s, op, "clean before")
            for where in ("g", "d", "xk", "sj"):
                lay = Layout(prob, range(3), pad, off, box, shifted)
                t = {"g": lay.G, "d": lay.D, "xk": lay.X, "sj": lay.S}[where]
                t[1, 0] = value
                t[1, n - 1] = value
                lay.call(s, op)
                lay.padding_untouched()
                de = prob.deff(box, shifted, 1, d=lay.D[1].clone())
                y, k, st = prob.single(op, 1, de, g=lay.G[1].clone(), xk=lay.X[1].clone(), sj=lay.S[1].clone())
                what = (op, n, value, where, pad, off)
                assert torch.equal(bits(lay.Y[1]), bits(y)), what
                assert torch.equal(bits(lay.K[1]), bits(k)), what
                got = lay.out[1].cpu().numpy()
                yh, kh, gh, dh = y.cpu().numpy(), k.cpu().numpy(), lay.G[1].cpu().numpy(), de.cpu().numpy()
                sel = prob.mask.astype(bool) if op[2] else np.ones(n, dtype=bool)
                with np.errstate(all="ignore"):
                    mags = (prob.lam[1] * np.sum(np.abs(kh[sel])) if op[0] == "l1" else 0.0, np.sum(np.abs(gh * yh)),
                            np.sum(np.abs((dh * yh) * yh)), np.sum(yh * yh))
                for j in range(4):
                    if op[0] == "l0" and j == 0:
                        assert got[0] == st[0], what      # a count: always finite, exact
                    else:
                        assert _same_sum(float(got[j]), st[j], mags[j]), (what, j, got[j], st[j])
                if not box:   # the flag: raised in the planted row exactly when a deff there is not > 0
                    assert lay.flag.tolist() == [0, int(not bool((de > 0).all())), 0], (what, lay.flag.tolist())
                for b in (0, 2):
                    assert torch.equal(lay.Y[b], clean.Y[b]) and torch.equal(lay.K[b], clean.K[b]), what
                    assert torch.equal(bits(lay.out[b]), bits(clean.out[b])), what
            after = Layout(prob, range(3), pad, off, box, shifted)
            after.call(s, op)
            assert torch.equal(bits(after.Y), bits(clean.Y)) and torch.equal(bits(after.K), bits(clean.K)), (op, n, value)
            assert torch.equal(bits(after.out), bits(clean.out)) and torch.equal(after.flag, clean.flag), (op, n, value)


# ------------------------------------------------------------------ refusals and empties
def test_ibatch_refusals_and_empties(s):
    import torch
    n, batch = 513, 3
    prob = Problems.get(s, n, 8100 + n)
    L, B, ctx = s._lib.load(), s._lib.load_ibatch(), s.context("cuda:0")
    lay = Layout(prob, range(batch), 1, 0, False, True)
    blay = Layout(prob, range(batch), 1, 0, True, True)
    ld = lay.ld
    y, g, d, xk, sj, k = (_P(f) for f in (lay.fy, lay.fg, lay.fd, lay.fx, lay.fs, lay.fk))
    keep = (-blay.dl, blay.dl.clone())
    lam, sh, lo, up, out, flag = _P(lay.lam), _P(lay.shift), _P(keep[0]), _P(keep[1]), _P(lay.out), _P(lay.flag)
    mask = _P(prob.maskd)
    Z = None

    def plain(y=y, g=g, d=d, xk=xk, sj=sj, n=n, batch=batch, ld=ld, lam=lam, sh=sh, flag=flag, k=k, out=out):
        return B.spx_iproxstep_l1_batch(ctx, y, g, d, xk, sj, n, batch, ld, lam, sh, flag, k, out)

    def box(**kw):
        a = dict(y=_P(blay.fy), g=_P(blay.fg), d=_P(blay.fd), xk=_P(blay.fx), sj=_P(blay.fs), n=n, batch=batch, ld=ld,
                 lam=_P(blay.lam), sh=_P(blay.shift), lo=lo, up=up, mask=mask, k=_P(blay.fk), out=_P(blay.out))
        a.update(kw)
        return B.spx_iproxstep_l0_box_batch(ctx, a["y"], a["g"], a["d"], a["xk"], a["sj"], a["n"], a["batch"], a["ld"], a["lam"],
                                            a["sh"], a["lo"], a["up"], a["mask"], a["k"], a["out"])

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == POISON).all()) for t in (lay.fy, lay.fk, lay.out, blay.fy, blay.fk, blay.out)) and \
            bool((lay.flag == FLAG_POISON).all())

    def next_call_is_right():
        assert plain() == 0
        lay.check(s, OPS[0], "after a refusal")
        lay.fy.fill_(POISON); lay.fk.fill_(POISON); lay.out.fill_(POISON); lay.flag.fill_(FLAG_POISON)

    refusals = [
        ("y == g", lambda: plain(y=g)), ("y == d", lambda: plain(y=d)), ("xkn == y", lambda: plain(k=y)),
        ("xkn == g", lambda: plain(k=g)), ("xkn == d", lambda: plain(k=d)), ("xkn == xk", lambda: plain(k=xk)),
        ("xkn == sj", lambda: plain(k=sj)), ("ld < n", lambda: plain(ld=n - 1)), ("batch < 0", lambda: plain(batch=-1)),
        ("n < 0", lambda: plain(n=-1)), ("lambda NULL", lambda: plain(lam=Z)), ("stats_dev NULL", lambda: plain(out=Z)),
        ("d_flag NULL", lambda: plain(flag=Z)),
        ("l NULL", lambda: box(lo=Z)), ("u NULL", lambda: box(up=Z)), ("box: lambda NULL", lambda: box(lam=Z)),
        ("box: stats_dev NULL", lambda: box(out=Z)), ("box: y == g", lambda: box(y=_P(blay.fg))),
        ("box: y == d", lambda: box(y=_P(blay.fd))), ("box: xkn == mask", lambda: box(k=mask)),
        ("box: ld < n", lambda: box(ld=n - 1)),
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
    # d_shift may be NULL: d enters as it is
    assert plain(sh=Z) == 0
    torch.cuda.synchronize()
    lay.fy.fill_(POISON); lay.fk.fill_(POISON); lay.out.fill_(POISON); lay.flag.fill_(FLAG_POISON)
    # empties: batch == 0 does nothing; n == 0 stores 4 * batch zeros (unboxed: and batch zero words) by a kernel
    assert plain(batch=0) == 0 and box(batch=0) == 0 and untouched()
    assert plain(batch=0, lam=Z, out=Z, flag=Z) == 0 and untouched()
    next_call_is_right()
    assert plain(n=0, ld=0) == 0
    torch.cuda.synchronize()
    assert bool((lay.out == 0.0).all()) and bool((lay.flag == 0).all())
    assert bool((lay.fy == POISON).all()) and bool((lay.fk == POISON).all())
    lay.out.fill_(POISON); lay.flag.fill_(FLAG_POISON)
    assert box(n=0, ld=5) == 0
    torch.cuda.synchronize()
    assert bool((blay.out == 0.0).all()) and bool((blay.fy == POISON).all())
    blay.out.fill_(POISON)
    next_call_is_right()
    # the box form is still right after all that
    blay.call(s, OPS[5])
    blay.check(s, OPS[5], "box after the refusals")
    # the mirror refuses what it can see
    with pytest.raises(TypeError):
        s.iprox_step_batch_bang(lay.Y, "lhalf", lay.G, lay.D, lay.X, lay.S, lay.lam)
    with pytest.raises(TypeError):
        s.iprox_step_batch_bang(lay.Y, "l1", lay.Y, lay.D, lay.X, lay.S, lay.lam)
    with pytest.raises(TypeError):
        s.iprox_step_batch_bang(lay.Y, "l1", lay.G, lay.Y, lay.X, lay.S, lay.lam)
    with pytest.raises(TypeError):
        s.iprox_step_batch_bang(lay.Y, "l1", lay.G, lay.D, lay.X, lay.S, lay.lam[:2])
    with pytest.raises(TypeError):
        s.iprox_step_batch_bang(lay.Y, "l1", lay.G, lay.D, lay.X, lay.S, lay.lam, d_shift=lay.shift[:2])
    with pytest.raises(TypeError):
        s.iprox_step_batch_bang(lay.Y, "l1", lay.G, lay.D, lay.X, lay.S, lay.lam, l=keep[0])
    with pytest.raises(TypeError):
        s.iprox_step_batch_bang(lay.Y, "l1", lay.G, lay.D, lay.X, lay.S, lay.lam, d_flag=lay.flag.to(torch.int64))
    with pytest.raises(TypeError):
        s.iprox_step_batch_bang(lay.Y, "l1", lay.G.contiguous(), lay.D, lay.X, lay.S, lay.lam)   # another row stride
    with pytest.raises(TypeError):
        s.iprox_step_batch_bang(lay.Y, "l1", lay.G, lay.D, lay.X, lay.S, lay.lam, out=torch.empty((batch, 3), dtype=torch.float64, device="cuda:0"))
    Yn, outn = s.iprox_step_batch("l1", lay.G, lay.D, lay.X, lay.S, lay.lam, d_shift=lay.shift)    # d_flag allocated by the mirror
    assert torch.equal(Yn, prob.ref(OPS[0], True)[0][:batch]) and Yn.stride() == lay.G.stride() and tuple(outn.shape) == (batch, 4)


# ------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("n", [3073, R + 3073])
def test_ibatch_sums_are_reproducible(s, n):
    import torch
    prob = Problems.get(s, n, 8100 + n)
    for op in OPS:
        for shifted in (False, True):
            a, b = Layout(prob, range(7), 1, 1, op[1], shifted), Layout(prob, range(7), 1, 1, op[1], shifted)
            a.call(s, op); b.call(s, op); a.call(s, op)
            assert torch.equal(a.out.view(torch.int64), b.out.view(torch.int64)), (op, n)
            assert torch.equal(a.Y.contiguous().view(torch.int64), b.Y.contiguous().view(torch.int64)), (op, n)


# ------------------------------------------------------------------ the parameters follow the device
@pytest.mark.parametrize("n", [3073, R + 3073])
def test_captured_ibatch_call_follows_the_device_parameters(s, n):
    """one batched call captured into a graph (one side stream, the same call made before: the tiled form reserves its workspace
    there); between replays lambda and d_shift (and the box) are overwritten ON THE DEVICE: every replay's rows equal the single
    call with the NEW scalars, bit for bit"""
    import torch
    prob = Problems.get(s, n, 8100 + n)
    rng = np.random.default_rng(8500 + n)
    for op in (OPS[1], OPS[3]):
        kind, box, msk = op
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            lay = Layout(prob, range(3), 1, 0, box, True)
            if box:
                lay.lo, lay.up = -lay.dl, lay.dl.clone()

            def call():
                s.iprox_step_batch_bang(lay.Y, kind, lay.G, lay.D, lay.X, lay.S, lay.lam, d_shift=lay.shift, l=lay.lo if box else None,
                                        u=lay.up if box else None, selected=prob.maskd if msk else None, xkn=lay.K, out=lay.out,
                                        d_flag=None if box else lay.flag)
            call(); call()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call()
        for rep in range(3):
            lam, dl = (rng.uniform(0.3, 1.5, size=3) for _ in range(2))
            # (unboxed: d > -0.2, so any shift >= 0.3 keeps deff > 0; the box forms take any shift)
            shift = rng.uniform(0.3, 1.5, size=3) if not box else rng.uniform(-1.0, 1.0, size=3)
            lay.lam.copy_(torch.from_numpy(lam)); lay.shift.copy_(torch.from_numpy(shift))
            if box:
                lay.lo.copy_(torch.from_numpy(-dl)); lay.up.copy_(torch.from_numpy(dl))
            lay.fy.fill_(POISON); lay.fk.fill_(POISON); lay.out.fill_(POISON); lay.flag.fill_(FLAG_POISON)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            lay.padding_untouched()
            if not box:
                assert lay.flag.tolist() == [0, 0, 0]
            got = lay.out.cpu().numpy()
            for b in range(3):
                de = prob.deff(box, True, b, shift=shift[b])
                y, k, _ = prob.single(op, b, de, scal=(lam[b], dl[b]))
                what = (op, n, rep, b)
                assert torch.equal(lay.Y[b], y) and torch.equal(lay.K[b], k), what
                _check_stats(op, got[b], prob.sum_refs(op, b, y.cpu().numpy(), k.cpu().numpy(), de.cpu().numpy(), lam=lam[b]), str(what))
