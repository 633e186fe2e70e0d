"""GPU: non-finite and extreme data through spx_iproxstep_* -- NaN, +-Inf, a subnormal and +-1e150 planted in g, xk, sj and d,
each at element 0, in the scalar tail (the last element of an odd n) and in another tile.

Every case runs the sequence clean / planted / clean / clean on one context A:
  status : every call returns 0, and spx_sync(A) is 0 afterwards;
  y      : the bits of spx_iprox_X on the same data (context B), NaN where that is NaN; xkn = (xk + sj) + y of that y;
  sums   : the IEEE class of their terms (tests/nonfinite.py: sum_class) -- the terms formed on the host from the y the device
           stored and the g, d that were passed; a finite sum to 1e-12 * sum |term| of math.fsum, the NormL0 count exactly (a
           NaN entry counts, the count is always finite).  The test's own condition: sum |term| < 1e307, so that no order of
           addition overflows (+-1e150 in g or sj gives |y| ~ 1e150 and terms up to 4e300, three of them);
  after  : the two clean calls behind the planted one give the bits a context created for the purpose gives on its first call.

n = 4099: with scalar bounds a tile is 2048 elements (element 2053 lies in the second), with vector bounds 1536; n is odd, so
the last element goes through the element-wise kernel.  The 8-bytes-off run peels element 0 into that kernel as well."""
import ctypes
import math

import numpy as np
import pytest

import nonfinite as nf

pytestmark = pytest.mark.gpu

_D = ctypes.c_double
N = 4099
POS = nf.positions(N, [2053])
LAM = 0.7
POISON = -777.25
MAG_LIMIT = 1e307
VALUES = (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf), ("subnormal", 5e-324), ("p1e150", 1e150), ("m1e150", -1e150))
VECTORS = ("g", "xk", "sj", "d")
FORMS = ["l1", "l0", "l1box", "l1vecbox+mask", "l0box", "l0vecbox+mask"]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    s = ge.build()
    L = s._lib.load()
    ctxs = []
    try:
        for _ in range(2):
            ctxs.append(_new_ctx(s, L))
        yield s, L, ctxs[0], ctxs[1]
    finally:
        torch.cuda.synchronize()
        for c in ctxs:
            L.spx_ctx_destroy(c)


def _new_ctx(s, L):
    import torch
    c = ctypes.c_void_p()
    s._lib.check(L.spx_ctx_create_on_stream(0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(c)))
    return c


def _dev(a, align8):
    """device copy; align8: the vector starts 8 bytes past a 16-byte boundary (the mask: 1 byte, it peels with the vectors)"""
    import torch
    t = torch.from_numpy(np.array(a))
    buf = torch.empty(t.numel() + 2, dtype=t.dtype, device="cuda:0")
    v = buf[1:1 + t.numel()] if align8 else buf[:t.numel()]
    v.copy_(t)
    return v


def _fill(align8, value=POISON):
    import torch
    buf = torch.full((N + 2,), value, dtype=torch.float64, device="cuda:0")
    return buf[1:1 + N] if align8 else buf[:N]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _same(a, b):
    import torch
    return bool(((a.view(torch.int64) == b.view(torch.int64)) | (a.isnan() & b.isnan())).all())


def _clean(form):
    rng = np.random.default_rng(7700 + FORMS.index(form))
    x, sj, g = rng.normal(size=N), rng.uniform(-0.5, 0.5, size=N), rng.normal(size=N)
    d = rng.uniform(0.5, 2.0, size=N)
    if "box" in form:
        r = rng.random(N)
        d = np.where(r < 0.15, 0.0, np.where(r < 0.30, -d, d))
    lo, up = -1.0 - 0.1 * rng.random(N), 1.0 + 0.1 * rng.random(N)
    mask = np.zeros(N, dtype=np.uint8)
    mask[rng.choice(N, size=N // 3, replace=False)] = 1
    mask[POS] = [1, 0, 1]        # a planted element inside the selected set and one outside it
    return dict(g=g, d=d, xk=x, sj=sj), lo, up, mask


class Problem:
    """one form on one set of host vectors: the fused call, the plain iprox!, the host terms"""

    def __init__(self, L, form, host, lo, up, mask, align8):
        self.L, self.form, self.host, self.align8 = L, form, host, align8
        self.kind = form[:2]
        self.dv = {k: _dev(v, align8) for k, v in host.items()}
        self.vec = form.endswith("vecbox+mask")
        self.box = "box" in form
        self.sel = np.flatnonzero(mask) if self.vec else np.arange(N)
        if self.vec:
            self.l, self.u, self.m = _dev(lo, align8), _dev(up, align8), _dev(mask, align8)

    def _head(self, ctx, y):
        v = self.dv
        return (ctx, _p(y), _p(v["g"]), _p(v["d"]), _p(v["xk"]), _p(v["sj"]), N, _D(LAM))

    def _bounds(self):
        if self.vec:
            return (_p(self.l), _p(self.u), _D(0.0), _D(0.0), _p(self.m))
        return (None, None, _D(-0.9), _D(0.9), None)

    def step(self, ctx, y, xkn):
        st = (ctypes.c_double * 4)()
        fn = getattr(self.L, "spx_iproxstep_" + self.kind + ("_box" if self.box else ""))
        mid = self._bounds() if self.box else (0,)
        return fn(*self._head(ctx, y), *mid, _p(xkn), st, None), list(st)

    def plain(self, ctx, y):
        fn = getattr(self.L, "spx_iprox_" + self.kind + ("_box" if self.box else ""))
        mid = self._bounds() if self.box else (0,)
        return fn(*self._head(ctx, y), *mid)


def _check_sum(got, terms, what, factor=1.0, exact=False):
    t = np.asarray(terms, dtype=np.float64)
    mag = nf.magnitude(t)
    assert mag < MAG_LIMIT, (what, mag)            # a condition on the test's own inputs
    cls = nf.sum_class(t)
    print("%s: got %r class %s sum |term| %.3g" % (what, got, cls, mag))
    if cls != "finite":
        assert nf.scalar_class(got) == cls, (what, got, cls)
        return
    ref = factor * math.fsum(t.tolist())
    assert math.isfinite(got), (what, got, ref)
    if exact:
        assert got == ref, (what, got, ref)
    else:
        assert abs(got - ref) <= nf.TOL * factor * mag, (what, got, ref, mag)


def _run(env, form, host, lo, up, mask, align8, what, finite):
    s, L, A, B = env
    pr = Problem(L, form, host, lo, up, mask, align8)
    ya, xkn, yb = _fill(align8), _fill(align8), _fill(align8)
    rc, st = pr.step(A, ya, xkn)
    assert rc == 0, (what, rc, L.spx_last_error())
    assert pr.plain(B, yb) == 0, what
    assert _same(ya, yb), what
    assert _same(xkn, (pr.dv["xk"] + pr.dv["sj"]) + ya), what
    yh = ya.cpu().numpy()
    if finite:
        assert np.isfinite(yh).all() and all(math.isfinite(t) for t in st), (what, st)
    g, d, x, sj = host["g"], host["d"], host["xk"], host["sj"]
    with np.errstate(all="ignore"):
        v = ((x + sj) + yh)[pr.sel]
        _check_sum(st[0], nf.h_terms(pr.kind, v), what + " [0]", factor=LAM, exact=pr.kind == "l0")
        _check_sum(st[1], g * yh, what + " [1]")
        _check_sum(st[2], (d * yh) * yh, what + " [2]")
        _check_sum(st[3], yh * yh, what + " [3]")
    if pr.kind == "l0":
        assert math.isfinite(st[0]), (what, st[0])
    return ya, xkn, st


@pytest.mark.parametrize("align8", [False, True])
@pytest.mark.parametrize("vector", VECTORS)
@pytest.mark.parametrize("form", FORMS)
def test_iprox_step_planted(env, form, vector, align8):
    import torch
    s, L, A, B = env
    clean, lo, up, mask = _clean(form)
    F = _new_ctx(s, L)           # the bits of a fresh context on the clean data
    try:
        pr = Problem(L, form, clean, lo, up, mask, align8)
        yf, kf = _fill(align8), _fill(align8)
        rc, fresh = pr.step(F, yf, kf)
        assert rc == 0 and L.spx_sync(F) == 0
    finally:
        torch.cuda.synchronize()
        L.spx_ctx_destroy(F)
    for vname, value in VALUES:
        planted = {k: a.copy() for k, a in clean.items()}
        planted[vector][POS] = value
        what = "%s %s=%s align8=%s" % (form, vector, vname, align8)
        for k, (name, host) in enumerate((("clean", clean), ("planted", planted), ("clean", clean), ("clean", clean))):
            ya, xkn, st = _run(env, form, host, lo, up, mask, align8, "%s call %d (%s)" % (what, k + 1, name), name == "clean")
            if name == "clean":
                assert torch.equal(ya, yf) and torch.equal(xkn, kf) and nf.triple_same(st, fresh), (what, k, st, fresh)
        assert L.spx_sync(A) == 0 and L.spx_sync(B) == 0, what
