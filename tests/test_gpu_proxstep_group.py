"""spx_proxstep_group_l2[_binf] / group_prox_step: prox! of ShiftedGroupNormL2(Binf) fused with the step statistics of a
trust-region iteration (csrc/spx_group.hip, include/spx.h "group forms" of spx_proxstep_*).

Bars, for a call with data (q, xk, sj, lambda):
  y    torch.equal with spx_prox_group_* on q_scale * q;
  xkn  torch.equal with (xd + sd) + y, on a buffer pre-filled with a poison value;
  [0]  == the value of spx_proxval_group_* on the same problem (same layout, route and alignment: the same bits);
  [1]  |got - fsum(q[i] * y[i])| <= 1e-12 * sum |q[i] * y[i]|, with the q that was passed (not q_scale * q);
  [2]  |got - fsum(y[i]^2)|      <= 1e-12 * sum y[i]^2
-- the bar and the reference of tests/test_gpu_proxstep.py::_check_sums, the project's bar for blocked Float64 sums; math.fsum
is exactly rounded and the host products are the rounded products the device forms (the library is built without contraction).

The Problem construction is that of tests/test_gpu_proxval_group.py (lattice data, zeroed and active groups, strong-lambda
groups; 301 / 61 / 13 groups by size: more than 8 workgroups on the 128-element tiles, so both ticket levels run)."""
import ctypes
import math
import zlib

import numpy as np
import pytest

import redzone

pytestmark = pytest.mark.gpu

_D = ctypes.c_double
TOL = 1e-12
INVALID = 1
POISON = -777.25
YFILL = -777.0


@pytest.fixture(scope="module")
def s():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.build()


def _dev(a, align8=False):
    """device copy; align8: the vector starts 8 bytes past a 16-byte boundary (the 8-byte load forms)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not align8:
        d = t.to("cuda:0")
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    buf[1:].copy_(t)
    return buf[1:]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


class Problem:
    """One layout with its data on the device, driven through the C ABI (the construction of tests/test_gpu_proxval_group.py)."""

    def __init__(self, s, layout, binf, align8=False, seed=0):
        import torch
        self.s, self.L, self.ctx, self.binf = s, s._lib.load(), s.context("cuda:0"), binf
        kind, arg = layout
        rng = np.random.default_rng(zlib.crc32(("%s%s%d%d" % (kind, arg, binf, seed)).encode()))
        self.offsets = None
        if kind == "uniform":
            gs = arg
            ng = 301 if gs <= 128 else 61 if gs <= 1024 else 13
            n, self.gsize, sizes = gs * ng, gs, np.full(ng, gs)
        elif kind == "one":
            n, ng, self.gsize, sizes = arg, 1, arg, np.array([arg])
        else:  # CSR: "csr_bound" (bound = largest size), "csr_nobound" (hint 0), "csr_over" (one group above the bound)
            ng = 700
            sizes = rng.integers(0, 61, size=ng)
            sizes[::97] = 0                      # empty groups
            if kind == "csr_over":
                sizes[ng // 2] = 777
            head = 5                             # offsets need not span 0:n
            off = head + np.concatenate([[0], np.cumsum(sizes)])
            n = int(off[-1]) + 9
            self.offsets = off.astype(np.int64)
            self.gsize = {"csr_bound": int(sizes.max()), "csr_nobound": 0, "csr_over": 60}[kind]
        self.n, self.ng = n, ng
        x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
        lat = n // 3
        x[:lat] = rng.integers(-8, 9, size=lat) / 4.0
        sj[:lat] = rng.integers(-2, 3, size=lat) / 4.0
        q[:lat] = rng.integers(-12, 13, size=lat) / 4.0
        x[: lat // 2] = 0.0
        if kind == "uniform":
            x[: self.gsize] = 0.0                # group 0: xk = 0 under a strong lambda (below) -- zeroed by both operators
        self.sigma, self.delta = 0.5, 1.0
        starts = self.offsets[:-1] if self.offsets is not None else np.arange(ng) * self.gsize
        S = (q + x) + sj
        nS = np.array([np.linalg.norm(S[a:a + m]) for a, m in zip(starts, sizes)])
        fac = rng.choice([0.0, 0.3, 0.7, 1.0, 1.5, 4.0, 40.0], size=ng)
        lam = np.where(nS > 0, nS, 1.0) * fac / self.sigma
        if kind != "one":
            lam[: ng // 3] = rng.choice([0.0, 0.25, 0.5, 1.0, 2.0, 8.0], size=ng // 3)   # (the lattice part: lattice weights)
        else:
            lam[:] = 0.6 * nS / self.sigma
        if kind == "uniform":                    # ... and group 1 active
            lam[0], lam[1] = 40.0 * nS[0] / self.sigma, 0.3 * nS[1] / self.sigma
        self.x, self.sj, self.q, self.lam = x, sj, q, lam
        self.xd, self.sd, self.qd = _dev(x, align8), _dev(sj, align8), _dev(q, align8)
        self.ld = _dev(lam)
        self.od = _dev(self.offsets) if self.offsets is not None else None
        self.align8 = align8
        self.torch = torch

    def new_y(self, fill=YFILL):
        return _dev(np.full(self.n, fill), self.align8)

    def new_xkn(self):
        return _dev(np.full(self.n, POISON), self.align8)

    def _tail(self):
        return (_D(self.delta),) if self.binf else ()

    def _head(self, y, q):
        return (self.ctx, _p(y), _p(self.qd if q is None else q), _p(self.xd), _p(self.sd), self.n, _p(self.od), self.gsize, self.ng,
                _p(self.ld), _D(self.sigma), *self._tail())

    def prox(self, y, q=None):
        fn = getattr(self.L, "spx_prox_group_l2" + ("_binf" if self.binf else ""))
        self.s._lib.check(fn(*self._head(y, q)))
        return y

    def proxval(self, y, q=None, q_scale=1.0):
        fn = getattr(self.L, "spx_proxval_group_l2" + ("_binf" if self.binf else ""))
        out = _D(-1.0)
        self.s._lib.check(fn(*self._head(y, q), _D(q_scale), ctypes.byref(out)))
        return y, out.value

    def step_rc(self, y, q=None, q_scale=1.0, xkn=None, host=True, dev=None):
        """the raw call: (rc, host triple or None)"""
        fn = getattr(self.L, "spx_proxstep_group_l2" + ("_binf" if self.binf else ""))
        st = (ctypes.c_double * 3)(-1.0, -2.0, -3.0) if host else None
        rc = fn(*self._head(y, q), _D(q_scale), _p(xkn), st, _p(dev))
        return rc, (tuple(st) if host else None)

    def step(self, y, q=None, q_scale=1.0, xkn=None, host=True, dev=None):
        rc, st = self.step_rc(y, q, q_scale, xkn, host, dev)
        self.s._lib.check(rc)
        return st


LAYOUTS = [("uniform", g) for g in (1, 2, 3, 8, 16, 17, 100, 128, 300, 512, 513, 1024, 5000)] + [
    ("csr_bound", 0), ("csr_nobound", 0), ("csr_over", 0), ("one", 1000), ("one", 1_000_003)]
_ids = ["%s%s" % (k, a or "") for k, a in LAYOUTS]


def _key9(s, v):
    s._lib.check(s._lib.load().spx_ctx_set_tuning(s.context("cuda:0"), 9, v))


def _check_sums(q, y, qy, yy, what):
    """q, y: host float64 arrays; the bar and reference of tests/test_gpu_proxstep.py::_check_sums.  Returns the references."""
    pq, py = q * y, y * y
    rqy, mqy, ryy = math.fsum(pq), math.fsum(np.abs(pq)), math.fsum(py)
    print("%s: qy %.17g ref %.17g (bar %.3g)  yy %.17g ref %.17g (bar %.3g)" % (what, qy, rqy, TOL * mqy, yy, ryy, TOL * ryy))
    assert abs(qy - rqy) <= TOL * mqy, (what, qy, rqy, mqy)
    assert abs(yy - ryy) <= TOL * ryy, (what, yy, ryy)
    return rqy, ryy


def _full_check(P, what, q_scale=1.0, fill=YFILL):
    """one step call against the plain prox at q_scale * q, the fused value and the fsum references; returns (y, xkn, triple)"""
    import torch
    qc = P.qd if q_scale == 1.0 else _dev((P.qd * q_scale).cpu().numpy(), P.align8)   # one rounded multiply per element
    y_plain = P.prox(P.new_y(fill), q=qc)
    _, v_pv = P.proxval(P.new_y(fill), q_scale=q_scale)
    y, xkn = P.new_y(fill), P.new_xkn()
    h, qy, yy = P.step(y, q_scale=q_scale, xkn=xkn)
    assert torch.equal(y, y_plain), what
    assert torch.equal(xkn, (P.xd + P.sd) + y), what
    print("%s: h %.17g proxval %.17g" % (what, h, v_pv))
    assert h == v_pv, (what, h, v_pv)
    refs = _check_sums(P.q, y.cpu().numpy(), qy, yy, what)
    return y, xkn, (h, qy, yy), refs


# ------------------------------------------------------------------ 1. every layout and route
@pytest.mark.parametrize("align8", [False, True], ids=["a16", "a8"])
@pytest.mark.parametrize("binf,key9", [(False, 0), (True, 0), (True, 1)], ids=["plain", "binf", "binf-key9"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
def test_every_layout(s, layout, binf, key9, align8):
    P = Problem(s, layout, binf, align8)
    try:
        _key9(s, key9)
        y, xkn, (h, qy, yy), (rqy, ryy) = _full_check(P, "layout %s binf %d key9 %d align8 %d" % (layout, binf, key9, align8))
    finally:
        _key9(s, 0)
    assert np.isfinite(h) and h > 0.0
    if P.offsets is not None:
        # the indices no group contains (5 in front, 9 behind) are part of xkn (checked over [0, n) above) and of both sums
        lo, hi = int(P.offsets[0]), int(P.offsets[-1])
        assert lo == 5 and P.n - hi == 9
        yh = y.cpu().numpy()
        out = np.r_[0:lo, hi:P.n]
        if binf:   # the Binf operator leaves y alone there: the known fill, which [2] must include
            assert np.all(yh[out] == YFILL)
        else:      # the plain operator subtracts the shift everywhere: the caller's y minus (xk + sj)
            assert np.array_equal(yh[out], YFILL - (P.x + P.sj)[out])
        part_yy = math.fsum(yh[out] * yh[out])
        part_qy = math.fsum(np.abs(P.q[out] * yh[out]))
        inner = math.fsum(yh[lo:hi] * yh[lo:hi])
        assert part_yy > 100 * TOL * ryy and abs(yy - inner) > 0.5 * part_yy, (part_yy, yy, inner)   # [2] without them misses the bar
        assert part_qy > 0.0


# ------------------------------------------------------------------ 2. groups on the deferred list
def test_groups_on_the_deferred_list_are_counted(s):
    """The data of test_groups_on_the_deferred_list_are_counted (tests/test_gpu_proxval_group.py): with tuning key 9 = 1 the
    groups whose root sits next to the pole are evaluated literally by the launch over the deferred list and by nothing else, so
    every group whose y differs between key 9 = 1 and key 9 = 0 was on the list.  Such groups occur; all three sums meet their
    bars, and a second call returns the same bits."""
    import torch
    gs = 16
    rng = np.random.default_rng(909 + gs)
    ng = 20_000
    n = ng * gs
    P = Problem.__new__(Problem)
    P.s, P.L, P.ctx, P.binf = s, s._lib.load(), s.context("cuda:0"), True
    P.n, P.ng, P.gsize, P.offsets, P.od, P.align8 = n, ng, gs, None, None, False
    P.sigma, P.delta = 1.0, 1.0
    P.x, P.sj, P.q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    nS = np.linalg.norm(((P.q + P.x) + P.sj).reshape(ng, gs), axis=1)
    P.lam = rng.uniform(1.0, 40.0, size=ng) * nS                      # sigma * lambda up to 40 ||S_g||: roots next to the pole
    P.lam[::2] = rng.uniform(0.1, 0.5, size=(ng + 1) // 2)            # every other group plainly active
    P.xd, P.sd, P.qd, P.ld = _dev(P.x), _dev(P.sj), _dev(P.q), _dev(P.lam)
    y0 = P.prox(P.new_y())
    try:
        _key9(s, 1)
        y1 = P.prox(P.new_y())
        y2, xkn, t2, _ = _full_check(P, "deferred list")
        y3, x3 = P.new_y(), P.new_xkn()
        t3 = P.step(y3, xkn=x3)
    finally:
        _key9(s, 0)
    assert torch.equal(y1, y2) and torch.equal(y2, y3) and torch.equal(xkn, x3)
    assert t2 == t3, (t2, t3)
    listed = (y1 != y0).view(ng, gs).any(dim=1).cpu().numpy()
    yh = y2.cpu().numpy()
    shares = [float(np.abs(t.reshape(ng, gs)).sum(axis=1)[listed].sum() / np.abs(t).sum()) for t in (P.q * yh, yh * yh)]
    print("%d groups on the list, their share of sum |q y| %.3e, of sum y^2 %.3e" % (int(listed.sum()), *shares))
    assert listed.sum() >= 10 and min(shares) > 1e-9, (int(listed.sum()), shares)   # (far above the bar: dropped terms would show)


# ------------------------------------------------------------------ 3. q_scale
@pytest.mark.parametrize("c", [-0.37, 0.0], ids=["c-0.37", "c0"])
@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("layout", [("uniform", 128), ("uniform", 8), ("uniform", 1024)], ids=["u128", "u8", "composed-u1024"])
def test_q_scale(s, layout, binf, c):
    """y is the plain prox on a pre-scaled q; [1] is taken with the UNSCALED q"""
    P = Problem(s, layout, binf, seed=3)
    y, xkn, (h, qy, yy), (rqy, ryy) = _full_check(P, "q_scale %g %s binf %d" % (c, layout, binf), q_scale=c)
    assert rqy != 0.0 and ryy > 0.0        # (at q_scale = 0 too: y = prox at 0 is not zero, so neither is <q, y>)
    if c != 0.0:                           # ... and the sum with the scaled q would miss the bar by far
        assert abs(c * rqy - rqy) > 1e6 * TOL * math.fsum(np.abs(P.q * y.cpu().numpy()))


# ------------------------------------------------------------------ 4. more partials than one trip of the class sum
def test_many_partials(s):
    """Plain groups of 8 sit on the 4-lane x 4-element tile: 16 groups per wavefront, 64 per workgroup.  64 * 16385 groups make
    16385 workgroups, 2049 per ticket class: the strided class sum (256 lanes x 8 loads) makes a second trip on all three planes."""
    import torch
    gs, ng = 8, 64 * 16385
    n = gs * ng
    assert n == 8_389_120
    rng = np.random.default_rng(4)
    x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    lam = rng.choice([0.3, 1.0, 3.0], size=ng) * math.sqrt(gs)
    xd, sd, qd, ld = _dev(x), _dev(sj), _dev(q), _dev(lam)
    L, ctx = s._lib.load(), s.context("cuda:0")
    head = lambda y: (ctx, _p(y), _p(qd), _p(xd), _p(sd), n, None, gs, ng, _p(ld), _D(0.5))
    y0 = torch.full((n,), YFILL, dtype=torch.float64, device="cuda:0")
    s._lib.check(L.spx_prox_group_l2(*head(y0)))
    v = _D(-1.0)
    y1 = torch.full((n,), YFILL, dtype=torch.float64, device="cuda:0")
    s._lib.check(L.spx_proxval_group_l2(*head(y1), _D(1.0), ctypes.byref(v)))
    y, xkn = torch.full((n,), YFILL, dtype=torch.float64, device="cuda:0"), torch.full((n,), POISON, dtype=torch.float64, device="cuda:0")
    st = (ctypes.c_double * 3)()
    s._lib.check(L.spx_proxstep_group_l2(*head(y), _D(1.0), _p(xkn), st, None))
    assert torch.equal(y, y0) and torch.equal(xkn, (xd + sd) + y)
    assert st[0] == v.value, (st[0], v.value)
    _check_sums(q, y.cpu().numpy(), st[1], st[2], "16385 workgroups")


# ------------------------------------------------------------------ 5. without xkn
@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("layout", [("uniform", 128), ("uniform", 17), ("uniform", 1024), ("csr_bound", 0)], ids=["u128", "u17", "u1024", "csr"])
def test_without_xkn(s, layout, binf):
    import torch
    P = Problem(s, layout, binf, seed=5)
    y1, xkn = P.new_y(), P.new_xkn()
    t1 = P.step(y1, xkn=xkn)
    spare = P.new_xkn()
    y2 = P.new_y()
    t2 = P.step(y2, xkn=None)
    assert torch.equal(y1, y2) and t1 == t2, (t1, t2)
    assert bool((spare == POISON).all())


# ------------------------------------------------------------------ 6. guard bands
REDZONE = [("1x8-binf", True, 8, 0), ("16x8-full", False, 128, 0), ("8x16-full-binf", True, 128, 0), ("64x6-padded", False, 300, 0),
           ("odd-8byte-loads", True, 17, 8), ("odd-8byte-loads-plain", False, 17, 8)]


@pytest.mark.parametrize("name,binf,gs,align", REDZONE, ids=[r[0] for r in REDZONE])
def test_guard_bands(s, name, binf, gs, align):
    """nothing is written outside [0, n) of y or xkn, every element of both is written, no input changes; a read past the end
    of an input would meet the poison and move y and the sums away from their references"""
    import torch
    ng = 1001
    n = gs * ng
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    nS = np.linalg.norm(((q + x) + sj).reshape(ng, gs), axis=1)
    sigma, delta = 0.9, 0.8
    lam = nS * rng.choice([0.3, 0.8, 1.5], size=ng) / sigma
    zone = redzone.Zone()
    f64 = torch.float64
    yb = zone.add(n, f64, align, role="out", name="y")
    vb = zone.add(n, f64, align, role="out", name="xkn")
    qb, xb, sb = (zone.add(n, f64, align, data=v, name=nm) for v, nm in ((q, "q"), (x, "xk"), (sj, "sj")))
    lb = zone.add(ng, f64, 0, data=lam, name="lambda")
    L, ctx = s._lib.load(), s.context("cuda:0")
    tail = (_D(delta),) if binf else ()
    sfx = "_binf" if binf else ""
    cp = lambda b: ctypes.c_void_p(b.ptr())
    head = lambda yp: (ctx, yp, cp(qb), cp(xb), cp(sb), n, None, gs, ng, cp(lb), _D(sigma), *tail)
    st = (ctypes.c_double * 3)()
    torch.cuda.synchronize()
    s._lib.check(getattr(L, "spx_proxstep_group_l2" + sfx)(*head(cp(yb)), _D(1.0), cp(vb), st, None))
    torch.cuda.synchronize()
    zone.check()
    y0 = torch.empty(n, dtype=f64, device="cuda:0")
    s._lib.check(getattr(L, "spx_prox_group_l2" + sfx)(*head(_p(y0))))
    v = _D(-1.0)
    y1 = torch.empty(n, dtype=f64, device="cuda:0")
    s._lib.check(getattr(L, "spx_proxval_group_l2" + sfx)(*head(_p(y1)), _D(1.0), ctypes.byref(v)))
    assert torch.equal(yb.t, y0) and torch.equal(vb.t, (xb.t + sb.t) + yb.t)
    if align == 0:
        assert st[0] == v.value, (st[0], v.value)       # (y1 is 16-byte aligned: the same route only when the zone's vectors are)
    else:
        assert abs(st[0] - v.value) <= TOL * v.value, (st[0], v.value)
    _check_sums(q, yb.t.cpu().numpy(), st[1], st[2], name)


# ------------------------------------------------------------------ 7. device results
@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("layout", [("uniform", 128), ("uniform", 16), ("uniform", 1024), ("csr_over", 0)], ids=["u128", "u16", "u1024", "csr-over"])
def test_device_results_have_the_host_bits(s, layout, binf):
    import torch
    P = Problem(s, layout, binf, seed=7)
    want = P.step(P.new_y())
    for host in (True, False):
        out = torch.full((5,), POISON, dtype=torch.float64, device="cuda:0")
        y = P.new_y()
        st = P.step(y, host=host, dev=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[0], got[1], got[2]) == want and got[3] == POISON and got[4] == POISON, (host, got, want)
        if host:
            assert st == want


# ------------------------------------------------------------------ 8. graph
def test_graph_replay(s):
    """The device-only form on 4096 x 128, plain and Binf, captured after one warm-up call and replayed twice on changed q: y, xkn
    and the triple equal the eager call's, bit for bit.  (Default queue count; no graph environment variable is touched.)"""
    import torch
    rng = np.random.default_rng(11)
    ng, gs = 4096, 128
    n = ng * gs
    x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    x[: n // 4] = np.round(x[: n // 4] * 4) / 4
    sj[: n // 4] = np.round(sj[: n // 4] * 4) / 4
    q[: n // 4] = np.round(q[: n // 4] * 4) / 4
    x[: n // 8] = 0.0
    nS = np.linalg.norm(((q + x) + sj).reshape(ng, gs), axis=1)
    lam = nS * rng.choice([0.3, 0.7, 1.0, 1.5, 4.0], size=ng)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xd, sd, qd = (torch.from_numpy(v).cuda() for v in (x, sj, q))
        h = s.GroupNormL2.uniform(torch.from_numpy(lam).cuda(), gs)
        psis = [s.shifted(s.shifted(h, xd), sd), s.shifted(s.shifted(h, xd, 1.0, s.NormLinf(1.0)), sd)]
        ys = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in psis]
        xkns = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in psis]
        outs = [torch.zeros(3, dtype=torch.float64, device="cuda") for _ in psis]

        def iteration():
            for psi, y, v, o in zip(psis, ys, xkns, outs):
                s.group_prox_step_bang(y, psi, qd, 1.0, q_scale=-0.5, xkn=v, out=o)

        iteration()                                  # the warm call
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        iteration()
    for rep in range(2):
        qd.copy_(torch.from_numpy(rng.normal(size=n) * (1.0 + rep)))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            iteration()
        side.synchronize()
        want = [(y.clone(), v.clone(), o.clone()) for y, v, o in zip(ys, xkns, outs)]
        for t in ys + xkns + outs:
            t.fill_(POISON)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for (y0, v0, o0), y, v, o in zip(want, ys, xkns, outs):
            assert torch.equal(y, y0) and torch.equal(v, v0), rep
            assert torch.equal(o.view(torch.int64), o0.view(torch.int64)), (rep, o, o0)
            assert float(o[0]) > 0.0
            _check_sums(qd.cpu().numpy(), y.cpu().numpy(), float(o[1]), float(o[2]), "replay %d" % rep)


# ------------------------------------------------------------------ 9. refusals
@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("layout", [("uniform", 16), ("uniform", 1024)], ids=["fused", "composed"])
def test_refusals(s, layout, binf):
    import torch
    P = Problem(s, layout, binf)
    y, spare = P.new_y(-9.0), P.new_xkn()
    inputs = [t.clone() for t in (P.qd, P.xd, P.sd)]
    out = torch.full((3,), POISON, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    rcs = [P.step_rc(y, xkn=t)[0] for t in (y, P.qd, P.xd, P.sd)]            # xkn is y / q / xk / sj
    rcs.append(P.step_rc(P.qd, xkn=spare, dev=out)[0])                        # y is q
    rcs.append(P.step_rc(y, xkn=spare, host=False, dev=None)[0])              # both results NULL
    P.ng += 1                                                                 # the argument errors of spx_prox_group_l2
    rcs.append(P.step_rc(y, xkn=spare, dev=out)[0])
    P.ng -= 1
    P.ng, keep = -1, P.ng
    rcs.append(P.step_rc(y, xkn=spare, dev=out)[0])
    P.ng = keep
    P.ld, keep = None, P.ld
    rcs.append(P.step_rc(y, xkn=spare, dev=out)[0])
    P.ld = keep
    P.gsize, keep = 0, P.gsize
    rcs.append(P.step_rc(y, xkn=spare, dev=out)[0])                           # group_size <= 0 with NULL offsets
    P.gsize = keep
    assert rcs == [INVALID] * len(rcs), rcs
    assert len(P.L.spx_last_error()) > 0
    torch.cuda.synchronize()
    assert bool((y == -9.0).all()) and bool((spare == POISON).all()) and bool((out == POISON).all())   # nothing was launched
    for t, t0 in zip((P.qd, P.xd, P.sd), inputs):
        assert torch.equal(t, t0)
    st = P.step(y, xkn=spare)                                                 # and the context is fine
    assert np.isfinite(st[0])


def test_refusals_of_the_mirror(s):
    import torch
    n, gs = 1024, 16
    rng = np.random.default_rng(1)
    x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    lam = [1.0] * (n // gs)
    chi = s.NormLinf(1.0)
    h = s.GroupNormL2.uniform(lam, gs)
    xd, sd, qd = _dev(x), _dev(sj), _dev(q)
    for binf in (False, True):
        tr = (1.0, chi) if binf else ()
        with pytest.raises(TypeError):               # Float32
            psi = s.shifted(s.shifted(h, xd.float(), *tr), sd.float())
            s.group_prox_step(psi, qd.float(), 1.0)
        with pytest.raises(TypeError):               # host
            psi = s.shifted(s.shifted(h, x.copy(), *tr), sj.copy())
            s.group_prox_step(psi, q.copy(), 1.0)
        with pytest.raises(TypeError):               # index sets (gather layout)
            perm = rng.permutation(n)
            hg = s.GroupNormL2(lam, [perm[i:i + gs].tolist() for i in range(0, n, gs)])
            psi = s.shifted(s.shifted(hg, xd, *tr), sd)
            assert psi._layout.index is not None
            s.group_prox_step(psi, qd, 1.0)
        psi = s.shifted(s.shifted(h, xd, *tr), sd)
        y = torch.full((n,), POISON, dtype=torch.float64, device="cuda:0")
        for bad in (qd, xd, sd):
            with pytest.raises(s.SpxError):
                s.group_prox_step_bang(y, psi, qd, 1.0, xkn=bad)
        with pytest.raises(TypeError):
            s.group_prox_step_bang(qd, psi, qd, 1.0)
        with pytest.raises(TypeError):
            s.group_prox_step(psi, qd, 1.0, out=torch.zeros(2, dtype=torch.float64, device="cuda:0"))
        torch.cuda.synchronize()
        assert bool((y == POISON).all())
        with pytest.raises(TypeError, match="ShiftedNormL1 / ShiftedNormL0 / ShiftedRootNormLhalf"):   # prox_step keeps refusing groups
            s.prox_step(psi, qd, 1.0)
        # the happy path of the mirror: the tuple form and the device form agree
        y1, hh, qy, yy = s.group_prox_step(psi, qd, 1.0)
        y1 = y1.clone()
        out = torch.zeros(3, dtype=torch.float64, device="cuda:0")
        y2, o = s.group_prox_step(psi, qd, 1.0, out=out)
        assert o is out and torch.equal(y1, y2) and tuple(out.cpu().tolist()) == (hh, qy, yy)
        assert hh == s.prox_value(psi, qd, 1.0)[1]
    for other in (s.shifted(s.shifted(s.NormL1(0.7), xd), sd), s.shifted(s.shifted(s.IndBallL0(3), xd), sd),
                  s.shifted(s.shifted(s.NormL1(1.0), xd, 1.0, s.NormL2(1.0)), sd)):
        with pytest.raises(TypeError):               # every non-group psi
            s.group_prox_step(other, qd, 1.0)


def test_host_valued_call_is_refused_under_capture(s):
    import torch
    ng, gs = 64, 128
    n = ng * gs
    rng = np.random.default_rng(2)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xd, sd, qd = (torch.from_numpy(rng.normal(size=n)).cuda() for _ in range(3))
        h = s.GroupNormL2.uniform([3.0] * ng, gs)
        psis = [s.shifted(s.shifted(h, xd), sd), s.shifted(s.shifted(h, xd, 1.0, s.NormLinf(1.0)), sd)]
        y = torch.full((n,), POISON, dtype=torch.float64, device="cuda")
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        for psi in psis:
            s.group_prox_step_bang(y, psi, qd, 1.1, out=out)
        y.fill_(POISON)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for psi in psis:
            with pytest.raises(s.SpxError) as e:
                s.group_prox_step_bang(y, psi, qd, 1.1)          # host-valued: refused, nothing recorded
            assert e.value.status == INVALID
        s.group_prox_step_bang(y, psis[0], qd, 1.1, out=out)     # (a capture must record something)
    torch.cuda.synchronize()
    assert bool((y == POISON).all())                             # no call has run


# ------------------------------------------------------------------ 10. empty
def test_empty(s):
    """n == 0 and ngroups == 0 are success cases: host zeros, and device zeros stored by a kernel"""
    import torch
    L, ctx = s._lib.load(), s.context("cuda:0")
    for binf in (False, True):
        fn = getattr(L, "spx_proxstep_group_l2" + ("_binf" if binf else ""))
        tail = (_D(1.0),) if binf else ()
        st = (ctypes.c_double * 3)(1.0, 2.0, 3.0)
        out = torch.full((3,), POISON, dtype=torch.float64, device="cuda:0")
        assert fn(ctx, None, None, None, None, 0, None, 16, 0, None, _D(0.5), *tail, _D(1.0), None, st, _p(out)) == 0
        assert list(st) == [0.0, 0.0, 0.0] and out.cpu().tolist() == [0.0, 0.0, 0.0]
        # ngroups == 0 on a vector of 40 (CSR offsets with no group): y as the plain operator leaves it
        n = 40
        rng = np.random.default_rng(3)
        xd, sd, qd = (_dev(rng.normal(size=n)) for _ in range(3))
        od = _dev(np.array([7], dtype=np.int64))
        y0 = torch.full((n,), YFILL, dtype=torch.float64, device="cuda:0")
        s._lib.check(getattr(L, "spx_prox_group_l2" + ("_binf" if binf else ""))(ctx, _p(y0), _p(qd), _p(xd), _p(sd), n, _p(od), 0, 0, None,
                                                                              _D(0.5), *tail))
        y = torch.full((n,), YFILL, dtype=torch.float64, device="cuda:0")
        st = (ctypes.c_double * 3)(1.0, 2.0, 3.0)
        out.fill_(POISON)
        assert fn(ctx, _p(y), _p(qd), _p(xd), _p(sd), n, _p(od), 0, 0, None, _D(0.5), *tail, _D(1.0), None, st, _p(out)) == 0
        assert list(st) == [0.0, 0.0, 0.0] and out.cpu().tolist() == [0.0, 0.0, 0.0]
        assert torch.equal(y, y0)
        out.fill_(POISON)
        assert fn(ctx, _p(y), _p(qd), _p(xd), _p(sd), n, _p(od), 0, 0, None, _D(0.5), *tail, _D(1.0), None, None, _p(out)) == 0
        assert out.cpu().tolist() == [0.0, 0.0, 0.0]


# ------------------------------------------------------------------ 11. the context afterwards
@pytest.mark.parametrize("layout", [("uniform", 128), ("uniform", 8), ("uniform", 1024), ("csr_over", 0)], ids=["u128", "u8", "u1024", "csr-over"])
def test_leaves_the_context_clean(s, layout):
    """after the new calls a plain spx_prox_group_*, a spx_proxval_group_* and a separable spx_proxstep_l1 give the bits they
    gave before: the ticket words have reset themselves and nothing of the workspace is taken for granted"""
    import torch
    Ps = [Problem(s, layout, False, seed=4), Problem(s, layout, True, seed=4)]
    n = Ps[0].n
    sep = s.shifted(s.shifted(s.NormL1(0.7), Ps[0].xd), Ps[0].sd)
    want = []
    for P in Ps:
        y0 = P.prox(P.new_y())
        y1, v1 = P.proxval(P.new_y())
        want.append((y0, y1, v1, P.step(P.new_y())))
    ys, hs, qys, yys = s.prox_step(sep, Ps[0].qd, 1.1)
    ys = ys.clone()
    for rep in range(3):                                 # (Binf calls alternate between the two count words)
        for P, (y0, y1, v1, st) in zip(Ps, want):
            xkn = P.new_xkn()
            assert P.step(P.new_y(), xkn=xkn) == st
            assert torch.equal(P.prox(P.new_y()), y0)
            assert P.step(P.new_y(), xkn=xkn) == st
            y, v = P.proxval(P.new_y())
            assert v == v1 and torch.equal(y, y1)
            assert P.step(P.new_y(), xkn=xkn) == st
            y, a, b, c = s.prox_step(sep, Ps[0].qd, 1.1)
            assert (a, b, c) == (hs, qys, yys) and torch.equal(y, ys)
    assert s._lib.load().spx_sync(s.context("cuda:0")) == 0
