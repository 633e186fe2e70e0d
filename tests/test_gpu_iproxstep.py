"""GPU: iprox! fused with the step statistics of a diagonal quasi-Newton iteration (spx_iproxstep_*, iprox_step /
iprox_step_bang).

One call stores y (bit-identical to the plain iprox!), xkn = (xk + sj) + y for every i, and four sums:
h = lambda * sum over the SELECTED indices of Term((xk + sj) + y), gy = sum over ALL i of g[i] y[i], ydy = sum over ALL i of
(d[i] y[i]) y[i], yy = sum over ALL i of y[i]^2.

Bars (those of tests/test_gpu_proxstep.py).  y and xkn: equal bits (torch.equal).  h against a host sum over the selected
indices of (xk + sj) + y: NormL0 exactly, NormL1 <= 1e-12 relative to lambda * math.fsum.  gy, ydy, yy against math.fsum
(exactly rounded) of the host products g[i] * y[i], (d[i] * y[i]) * y[i] and y[i] * y[i] -- the same rounded products the
device forms, the library is built without contraction: |got - ref| <= 1e-12 * sum |term|.  Key 17 = 0 and a repeated call
give the bits of the first call in all four sums.

Sizes (launch_vec's table).  ShiftedNormL1, NormL0 and NormL0Box with scalar bounds run the LDS-staged kernel at 4 KiB per wave
and vector: a workgroup covers 256 * 4 pairs = 2048 elements.  NormL0Box with vector bounds runs it at 3 KiB: 1536 elements.
ShiftedNormL1Box runs the register-staged kernel, 256 * 4 pairs = 2048 elements per tile, with either kind of bounds.  So the
edges are 1536 +- 1 and 2048 +- 1; the odd sizes also take the peeled head (8 bytes off) and the odd tail.  n = 1_000_003 is
652 workgroups with vector bounds and 489 without, plus the tail's slot: an odd n is never one launch, so the separate
four-plane reduction (k_value_reduce<4>) adds the planes there, in the order of the one-launch finish; its branch for lists of
more than 2048 slots is the three-plane kernel's, per plane, and is not reached below n = 3.1e6."""
import ctypes
import math

import numpy as np
import pytest

import redzone

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 1535, 1536, 1537, 2047, 2048, 2049, 1_000_003]
FORMS = ["l1", "l0", "l1box", "l1vecbox+mask", "l0box", "l0vecbox+mask"]
TOL = 1e-12
LAM = 0.7
INVALID = 1
ASSERT = 6
POISON = -777.25


@pytest.fixture(scope="module")
def s():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.build()


def _data(n, seed, boxed):
    """d: U(0.5, 2) for the unboxed forms; 70 % U(0.5, 2), 15 % exactly 0, 15 % U(-2, -0.5) for the Box forms"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=n)
    sj = rng.uniform(-0.5, 0.5, size=n)
    g = rng.normal(size=n)
    d = rng.uniform(0.5, 2.0, size=n)
    if boxed:
        r = rng.random(n)
        d = np.where(r < 0.15, 0.0, np.where(r < 0.30, -d, d))
    lo, up = -1.0 - 0.1 * rng.random(n), 1.0 + 0.1 * rng.random(n)
    selected = sorted(rng.choice(n, size=max(1, n // 3), replace=False).tolist())
    return x, sj, g, d, lo, up, selected


def _dev(arrs, misaligned=False):
    import torch
    if misaligned:  # every vector 8 bytes off a 16-byte boundary
        return [torch.cat([torch.zeros(1, dtype=torch.float64), torch.from_numpy(np.ascontiguousarray(a))]).cuda()[1:] for a in arrs]
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrs]


def _buf(n, misaligned=False, fill=POISON):
    import torch
    t = torch.full((n + 1,), fill, dtype=torch.float64, device="cuda:0")
    return t[1:] if misaligned else t[:n]


def _psi(s, form, xd, sd, ld, ud, selected):
    """(psi, kind, selected index array or None for all)"""
    H = s.NormL1 if form.startswith("l1") else s.NormL0
    if form in ("l1", "l0"):
        return s.shifted(s.shifted(H(LAM), xd), sd), form, None
    if form.endswith("vecbox+mask"):
        return s.shifted(s.shifted(H(LAM), xd, ld, ud, selected), sd), form[:2], np.asarray(selected)
    return s.shifted(s.shifted(H(LAM), xd, 0.9, s.NormLinf(1.0)), sd), form[:2], None


def _fsum(a):
    return math.fsum(a.tolist())


def _check_h(kind, h, x, sj, y, sel, what):
    v = (x + sj) + y
    if sel is not None:
        v = v[sel]
    if kind == "l0":
        exp = LAM * float(np.count_nonzero(v))
        print("%s: h %.17g ref %.17g (exact)" % (what, h, exp))
        assert h == exp, (what, h, exp)
    else:
        exp = LAM * _fsum(np.abs(v))
        print("%s: h %.17g ref %.17g (bar %.3g)" % (what, h, exp, TOL * abs(exp)))
        assert abs(h - exp) <= TOL * max(abs(exp), 1e-300), (what, h, exp)


def _check_sums(g, d, y, gy, ydy, yy, what):
    for name, got, t in (("gy", gy, g * y), ("ydy", ydy, (d * y) * y), ("yy", yy, y * y)):
        ref, mag = _fsum(t), _fsum(np.abs(t))
        print("%s: %s %.17g ref %.17g (bar %.3g)" % (what, name, got, ref, TOL * mag))
        assert abs(got - ref) <= TOL * mag, (what, name, got, ref, mag)


def _set(s, key, v):
    s._lib.check(s._lib.load().spx_ctx_set_tuning(s.context("cuda:0"), key, v))


def _full_check(s, psi, kind, sel, host, dev, ybuf, xkn, what):
    """one iprox_step_bang call into ybuf (aligned like the vectors, so that vectors 8 bytes off take the peeled head) against
    the plain iprox!, the host references, key 17 = 0 and a repeat; returns (y, four sums)"""
    import torch
    x, sj, g, d = host
    xd, sd, gd, dd = dev
    y_plain = s.iprox_bang(torch.full_like(gd, POISON), psi, gd, dd, check=False)
    xkn.fill_(POISON)
    ybuf.fill_(POISON)
    assert ybuf.data_ptr() % 16 == gd.data_ptr() % 16
    y, h, gy, ydy, yy = s.iprox_step_bang(ybuf, psi, gd, dd, xkn=xkn)
    assert torch.equal(y, y_plain), what
    assert torch.equal(xkn, (xd + sd) + y), what
    yh = y.cpu().numpy()
    _check_h(kind, h, x, sj, yh, sel, what)
    _check_sums(g, d, yh, gy, ydy, yy, what)
    first = [float(t).hex() for t in (h, gy, ydy, yy)]
    try:
        _set(s, 17, 0)
        y0, *st0 = s.iprox_step_bang(ybuf, psi, gd, dd, xkn=xkn)
        assert torch.equal(y0, y_plain) and torch.equal(xkn, (xd + sd) + y_plain), what
    finally:
        _set(s, 17, 1)
    assert [float(t).hex() for t in st0] == first, (what, "key 17", st0, first)
    _, *st1 = s.iprox_step_bang(ybuf, psi, gd, dd, xkn=xkn)
    assert [float(t).hex() for t in st1] == first, (what, "repeat", st1, first)
    return y, (h, gy, ydy, yy)


# ------------------------------------------------------------------ the six forms at the tile edges, both alignments
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_iprox_step_forms(s, n, form):
    boxed = "box" in form
    x, sj, g, d, lo, up, selected = _data(n, 9100 + n, boxed)
    if boxed and n > 1000:   # every branch of IproxL1Box / IproxL0Box is taken: d > eps, |d| <= eps, d < -eps
        assert (d > 0).sum() > n // 2 and (d == 0).sum() > n // 10 and (d < 0).sum() > n // 10
    for misaligned in (False, True):
        xd, sd, gd, dd, ld, ud = _dev((x, sj, g, d, lo, up), misaligned)
        psi, kind, sel = _psi(s, form, xd, sd, ld, ud, selected)
        _full_check(s, psi, kind, sel, (x, sj, g, d), (xd, sd, gd, dd), _buf(n, misaligned), _buf(n, misaligned), "%s n=%d mis=%s" % (form, n, misaligned))


def test_iprox_step_sums_run_over_the_right_index_sets(s):
    """gy, ydy and yy run over ALL elements, h over the SELECTED ones: the unselected elements carry y = iprox_zero(...) != 0,
    so a sum over the wrong index set lands far outside the bars"""
    n = 2049
    x, sj, g, d, lo, up, selected = _data(n, 9201, True)
    xd, sd, gd, dd, ld, ud = _dev((x, sj, g, d, lo, up))
    psi = s.shifted(s.shifted(s.NormL1(LAM), xd, ld, ud, selected), sd)
    y, h, gy, ydy, yy = s.iprox_step(psi, gd, dd, xkn=_buf(n))
    yh = y.cpu().numpy()
    sel = np.zeros(n, dtype=bool)
    sel[selected] = True
    assert np.count_nonzero(yh[~sel]) > n // 2              # the unselected elements do carry a step
    v = np.abs((x + sj) + yh)
    h_sel, h_all = LAM * _fsum(v[sel]), LAM * _fsum(v)
    assert abs(h - h_sel) <= TOL * h_sel and abs(h - h_all) > 1e-3 * h_all, (h, h_sel, h_all)
    _check_sums(g, d, yh, gy, ydy, yy, "index sets")
    for name, got, t in (("gy", gy, g * yh), ("ydy", ydy, (d * yh) * yh), ("yy", yy, yh * yh)):
        assert abs(got - _fsum(t[sel])) > 1e-3 * _fsum(np.abs(t)), (name, got)


def test_iprox_step_without_xkn(s):
    """xkn=None: y and the sums unchanged, a poisoned spare buffer stays untouched"""
    import torch
    n = 2049
    spare = _buf(n)
    for form in FORMS:
        x, sj, g, d, lo, up, selected = _data(n, 9300, "box" in form)
        xd, sd, gd, dd, ld, ud = _dev((x, sj, g, d, lo, up))
        psi, kind, sel = _psi(s, form, xd, sd, ld, ud, selected)
        y1, *st1 = s.iprox_step(psi, gd, dd, xkn=_buf(n))
        y1 = y1.clone()
        y2, *st2 = s.iprox_step(psi, gd, dd)
        assert torch.equal(y1, y2) and st1 == st2, form
    torch.cuda.synchronize()
    assert bool((spare == POISON).all())


def test_iprox_step_xkn_alone_misaligned(s):
    """every other vector 16-byte aligned and xkn 8 bytes off: the call takes the element-wise kernel, stores every element
    and nothing else"""
    import torch
    n = 2049
    for form in FORMS:
        x, sj, g, d, lo, up, selected = _data(n, 9350, "box" in form)
        xd, sd, gd, dd, ld, ud = _dev((x, sj, g, d, lo, up))
        full = torch.full((n + 3,), POISON, dtype=torch.float64, device="cuda:0")
        xkn = full[1:n + 1]
        assert xkn.data_ptr() % 16 == 8 and gd.data_ptr() % 16 == 0
        psi, kind, sel = _psi(s, form, xd, sd, ld, ud, selected)
        _full_check(s, psi, kind, sel, (x, sj, g, d), (xd, sd, gd, dd), _buf(n), xkn, form + " xkn 8 bytes off")
        assert bool((full[:1] == POISON).all()) and bool((full[n + 1:] == POISON).all())


# ------------------------------------------------------------------ device results, graph
def test_iprox_step_device_results_have_the_host_bits(s):
    import torch
    for n in (2048, 2049, 50_000):
        for form in FORMS:
            x, sj, g, d, lo, up, selected = _data(n, 9400 + n, "box" in form)
            xd, sd, gd, dd, ld, ud = _dev((x, sj, g, d, lo, up))
            psi, kind, sel = _psi(s, form, xd, sd, ld, ud, selected)
            xkn = _buf(n)
            y1, *host = s.iprox_step(psi, gd, dd, xkn=xkn)
            y1 = y1.clone()
            out = torch.full((6,), POISON, dtype=torch.float64, device="cuda:0")
            y2, o = s.iprox_step(psi, gd, dd, xkn=xkn, out=out)
            assert o is out and torch.equal(y1, y2)
            got = out.cpu().numpy()
            assert [float(t).hex() for t in got[:4]] == [float(t).hex() for t in host], (form, n)
            assert got[4] == POISON and got[5] == POISON


def _D(v):
    return ctypes.c_double(v)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def test_iprox_step_both_result_forms_agree(s):
    """stats and stats_dev given together (C ABI): the same bits in both"""
    import torch
    L, ctx = s._lib.load(), s.context("cuda:0")
    for n in (2048, 2049):
        x, sj, g, d, lo, up, selected = _data(n, 9450 + n, False)
        xd, sd, gd, dd = _dev((x, sj, g, d))
        y, xkn = _buf(n), _buf(n)
        st = (ctypes.c_double * 4)()
        out = torch.full((4,), POISON, dtype=torch.float64, device="cuda:0")
        for fn in (L.spx_iproxstep_l1, L.spx_iproxstep_l0):
            s._lib.check(fn(ctx, _p(y), _p(gd), _p(dd), _p(xd), _p(sd), n, _D(LAM), 1, _p(xkn), st, _p(out)))
            assert [float(t).hex() for t in out.cpu().numpy()] == [float(t).hex() for t in st], n


def test_iprox_step_in_a_graph(s):
    """one iprox_step_bang(..., xkn=, out=) run eagerly, then captured and replayed twice with g changed between the replays:
    y, xkn and out after each replay are the eager call's"""
    import torch
    n = 50_000
    rng = np.random.default_rng(9501)
    side = torch.cuda.Stream()
    for form in ("l0", "l1vecbox+mask"):
        x, sj, g, d, lo, up, selected = _data(n, 9500, "box" in form)
        with torch.cuda.stream(side):
            xd, sd, dd, ld, ud = _dev((x, sj, d, lo, up))
            gd = torch.from_numpy(g).cuda()
            psi, kind, sel = _psi(s, form, xd, sd, ld, ud, selected)
            y = torch.zeros(n, dtype=torch.float64, device="cuda")
            xkn = torch.zeros(n, dtype=torch.float64, device="cuda")
            out = torch.zeros(4, dtype=torch.float64, device="cuda")

            def step():
                s.iprox_step_bang(y, psi, gd, dd, xkn=xkn, out=out)

            step(); step()      # eager, on the capture stream: the workspace reaches its size
        side.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            step()
        for rep in range(2):
            gd.copy_(torch.from_numpy(rng.normal(size=n) * (1.0 + rep)))
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                step()
            side.synchronize()
            want = (y.clone(), xkn.clone(), out.clone())
            for t in (y, xkn, out):
                t.fill_(POISON)
            torch.cuda.synchronize()
            gr.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, want[0]) and torch.equal(xkn, want[1]), (form, rep)
            assert torch.equal(out.view(torch.int64), want[2].view(torch.int64)), (form, rep, out, want[2])
            o = out.cpu().numpy()
            _check_sums(gd.cpu().numpy(), d, y.cpu().numpy(), o[1], o[2], o[3], "%s replay %d" % (form, rep))


def test_iprox_step_host_valued_call_is_refused_under_capture(s):
    import torch
    n = 4096
    x, sj, g, d, lo, up, selected = _data(n, 9550, False)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xd, sd, gd, dd = _dev((x, sj, g, d))
        psi = s.shifted(s.shifted(s.NormL1(LAM), xd), sd)
        y = torch.full((n,), POISON, dtype=torch.float64, device="cuda")
        out = torch.zeros(4, dtype=torch.float64, device="cuda")
        s.iprox_step_bang(y, psi, gd, dd, out=out)
        y.fill_(POISON)
    side.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):
        with pytest.raises(s.SpxError) as e:
            s.iprox_step_bang(y, psi, gd, dd)          # host-valued: refused, nothing recorded
        assert e.value.status == INVALID
        s.iprox_step_bang(y, psi, gd, dd, out=out)     # (a capture must record something)
    torch.cuda.synchronize()
    assert bool((y == POISON).all())                   # neither call has run


# ------------------------------------------------------------------ errors
def test_iprox_step_errors(s):
    import torch
    L, ctx = s._lib.load(), s.context("cuda:0")
    n = 1000
    x, sj, g, d, lo, up, selected = _data(n, 9600, False)
    xd, sd, gd, dd, ld, ud = _dev((x, sj, g, d, lo, up))
    mask = torch.ones(n, dtype=torch.uint8, device="cuda:0")
    y = _buf(n)
    y0 = y.clone()
    st = (ctypes.c_double * 4)()
    spare = _buf(n)
    for fn in (L.spx_iproxstep_l1, L.spx_iproxstep_l0):
        head = (ctx, _p(y), _p(gd), _p(dd), _p(xd), _p(sd), n, _D(LAM))
        cases = [fn(*head, 0, _p(t), st, None) for t in (y, gd, dd, xd, sd)]                              # xkn is y / g / d / xk / sj
        cases.append(fn(ctx, _p(y), _p(y), _p(dd), _p(xd), _p(sd), n, _D(LAM), 0, _p(spare), st, None))   # y is g
        cases.append(fn(ctx, _p(y), _p(gd), _p(y), _p(xd), _p(sd), n, _D(LAM), 0, _p(spare), st, None))   # y is d
        cases.append(fn(*head, 0, _p(spare), None, None))                                                 # both results NULL
        out = torch.zeros(4, dtype=torch.float64, device="cuda:0")
        cases.append(fn(*head, 1, _p(spare), None, _p(out)))                                              # check_d, no host stats
        for k, rc in enumerate(cases):
            assert rc == INVALID, (k, rc)
        assert len(L.spx_last_error()) > 0
    for fn in (L.spx_iproxstep_l1_box, L.spx_iproxstep_l0_box):
        head = (ctx, _p(y), _p(gd), _p(dd), _p(xd), _p(sd), n, _D(LAM), _p(ld), _p(ud), _D(0.0), _D(0.0), _p(mask))
        cases = [fn(*head, _p(t), st, None) for t in (y, gd, dd, xd, sd, ld, ud)]                         # ... / l_vec / u_vec
        cases.append(fn(*head, ctypes.c_void_p(mask.data_ptr()), st, None))                               # xkn is the mask
        cases.append(fn(ctx, _p(y), _p(y), _p(dd), _p(xd), _p(sd), n, _D(LAM), None, None, _D(-1.0), _D(1.0), None, _p(spare), st, None))
        cases.append(fn(ctx, _p(y), _p(gd), _p(y), _p(xd), _p(sd), n, _D(LAM), None, None, _D(-1.0), _D(1.0), None, _p(spare), st, None))
        cases.append(fn(*head, _p(spare), None, None))
        for k, rc in enumerate(cases):
            assert rc == INVALID, (k, rc)
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and bool((spare == POISON).all())          # nothing was launched
    # the mirror: the same through SpxError / TypeError
    psi = s.shifted(s.shifted(s.NormL1(LAM), xd), sd)
    for bad in (gd, dd, xd, sd):
        with pytest.raises(s.SpxError):
            s.iprox_step_bang(y, psi, gd, dd, xkn=bad)
    with pytest.raises(TypeError):
        s.iprox_step_bang(gd, psi, gd, dd)
    with pytest.raises(TypeError):
        s.iprox_step_bang(dd, psi, gd, dd)
    with pytest.raises(TypeError):
        s.iprox_step(psi, gd, dd, out=torch.zeros(3, dtype=torch.float64, device="cuda:0"))
    with pytest.raises(TypeError):
        s.iprox_step(psi, gd, dd, check=True, out=torch.zeros(4, dtype=torch.float64, device="cuda:0"))
    lhalf = s.shifted(s.shifted(s.RootNormLhalf(LAM), xd), sd)
    grp = s.shifted(s.shifted(s.GroupNormL2.uniform([1.0] * (n // 100), 100), xd), sd)
    top = s.shifted(s.shifted(s.IndBallL0(10), xd), sd)
    b2 = s.shifted(s.shifted(s.NormL1(1.0), xd, 1.0, s.NormL2(1.0)), sd)
    f32 = s.shifted(s.shifted(s.NormL1(LAM), xd.float()), sd.float())
    host = s.shifted(s.shifted(s.NormL1(LAM), x.copy()), sj.copy())
    for psi_bad, gg, d2 in ((lhalf, gd, dd), (grp, gd, dd), (top, gd, dd), (b2, gd, dd), (f32, gd.float(), dd.float()), (host, g, d)):
        with pytest.raises(TypeError, match="ShiftedNormL1 / ShiftedNormL0 and their Box forms"):
            s.iprox_step(psi_bad, gg, d2)
    torch.cuda.synchronize()
    assert torch.equal(y, y0)


def test_iprox_step_check_d(s):
    """one non-positive d in an unboxed form: SPX_ERR_ASSERT (AssertionError through the mirror); the next call on the context
    returns 0 with the right bits -- the flag word is cleared per call and lies clear of the four results"""
    import torch
    L, ctx = s._lib.load(), s.context("cuda:0")
    for n in (2049, 50_000):
        x, sj, g, d, lo, up, selected = _data(n, 9700 + n, False)
        bad = d.copy()
        bad[n // 2] = 0.0
        xd, sd, gd, dd, bd = _dev((x, sj, g, d, bad))
        for fn, H in ((L.spx_iproxstep_l1, s.NormL1), (L.spx_iproxstep_l0, s.NormL0)):
            psi = s.shifted(s.shifted(H(LAM), xd), sd)
            y, xkn = _buf(n), _buf(n)
            st = (ctypes.c_double * 4)()
            assert fn(ctx, _p(y), _p(gd), _p(dd), _p(xd), _p(sd), n, _D(LAM), 1, _p(xkn), st, None) == 0
            want = [float(t).hex() for t in st]
            assert fn(ctx, _p(y), _p(gd), _p(bd), _p(xd), _p(sd), n, _D(LAM), 1, _p(xkn), st, None) == ASSERT
            assert fn(ctx, _p(y), _p(gd), _p(bd), _p(xd), _p(sd), n, _D(LAM), 0, _p(xkn), st, None) == 0      # unchecked: IEEE
            with pytest.raises(AssertionError):
                s.iprox_step(psi, gd, bd, check=True)
            assert fn(ctx, _p(y), _p(gd), _p(dd), _p(xd), _p(sd), n, _D(LAM), 1, _p(xkn), st, None) == 0
            assert [float(t).hex() for t in st] == want, (n, H.__name__)
            y_plain = s.iprox_bang(_buf(n), psi, gd, dd, check=False)
            assert torch.equal(y, y_plain) and torch.equal(xkn, (xd + sd) + y_plain)
            _check_sums(g, d, y.cpu().numpy(), st[1], st[2], st[3], "after the assertion n=%d" % n)


# ------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("mode", ["A", "B"])
@pytest.mark.parametrize("op", ["l1", "l0", "l1box", "l0vecbox+mask"])
@pytest.mark.parametrize("n", [1537, 2049])
def test_iprox_step_guard_bands(s, n, op, mode):
    """through the C ABI on guarded buffers: y and xkn are outputs (every element written, nothing outside them), the inputs are
    guarded against reads past the end (the poison would move y or a sum) and against writes"""
    import torch
    L, ctx = s._lib.load(), s.context("cuda:0")
    ay, ai = redzone.F64_MODES[mode]
    boxed = "box" in op
    x, sj, g, d, lo, up, selected = _data(n, 9800 + n, boxed)
    mask = np.zeros(n, dtype=np.uint8)
    mask[selected] = 1
    z = redzone.Zone()
    yb = z.add(n, torch.float64, ay, role="out", name="y")
    kb = z.add(n, torch.float64, ay, role="out", name="xkn")
    gb, db, xb, sb = (z.add(n, torch.float64, ai, data=a, name=nm) for a, nm in ((g, "g"), (d, "d"), (x, "xk"), (sj, "sj")))
    st = (ctypes.c_double * 4)()
    p = lambda b: ctypes.c_void_p(b.ptr())
    xd, sd, gd, dd, ld, ud = _dev((x, sj, g, d, lo, up))
    psi, kind, sel = _psi(s, op, xd, sd, ld, ud, selected)
    if op == "l0vecbox+mask":
        lb, ub = z.add(n, torch.float64, ai, data=lo, name="l"), z.add(n, torch.float64, ai, data=up, name="u")
        mb = z.add(n, torch.uint8, 1 if mode == "B" else 0, data=mask, name="mask")   # (mode B: the mask peels with the vectors)
        s._lib.check(L.spx_iproxstep_l0_box(ctx, p(yb), p(gb), p(db), p(xb), p(sb), n, _D(LAM), p(lb), p(ub), _D(0.0), _D(0.0), p(mb),
                                            p(kb), st, None))
    elif op == "l1box":
        s._lib.check(L.spx_iproxstep_l1_box(ctx, p(yb), p(gb), p(db), p(xb), p(sb), n, _D(LAM), None, None, _D(-0.9), _D(0.9), None,
                                            p(kb), st, None))
    else:
        fn = L.spx_iproxstep_l1 if op == "l1" else L.spx_iproxstep_l0
        s._lib.check(fn(ctx, p(yb), p(gb), p(db), p(xb), p(sb), n, _D(LAM), 1, p(kb), st, None))
    torch.cuda.synchronize()
    z.check()
    y_plain = s.iprox_bang(_buf(n), psi, gd, dd, check=False)
    assert torch.equal(yb.t, y_plain) and torch.equal(kb.t, (xd + sd) + y_plain)
    what = "guard bands %s n=%d mode=%s" % (op, n, mode)
    _check_h(kind, st[0], x, sj, y_plain.cpu().numpy(), sel, what)
    _check_sums(g, d, y_plain.cpu().numpy(), st[1], st[2], st[3], what)


def test_iprox_step_empty(s):
    """n == 0 is the success case: host zeros, and device zeros stored by a kernel"""
    import torch
    e = torch.zeros(0, dtype=torch.float64, device="cuda:0")
    psi = s.shifted(s.shifted(s.NormL1(LAM), e), e.clone())
    y, *st = s.iprox_step(psi, e.clone(), e.clone())
    assert st == [0.0, 0.0, 0.0, 0.0] and y.numel() == 0
    out = torch.full((4,), POISON, dtype=torch.float64, device="cuda:0")
    s.iprox_step(psi, e.clone(), e.clone(), out=out)
    assert out.cpu().tolist() == [0.0, 0.0, 0.0, 0.0]
    L, ctx = s._lib.load(), s.context("cuda:0")
    st = (ctypes.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    assert L.spx_iproxstep_l0_box(ctx, None, None, None, None, None, 0, _D(LAM), None, None, _D(-1.0), _D(1.0), None,
                                  None, st, None) == 0
    assert list(st) == [0.0, 0.0, 0.0, 0.0]


# ------------------------------------------------------------------ the context afterwards
def test_iprox_step_leaves_the_context_clean(s):
    """after an iprox_step call, psi(y), prox_value, prox_step and a checked iprox! on the same context give their usual bits:
    tickets, the flag word and the workspace are left clean"""
    import torch
    for n in (2048, 50_000):
        x, sj, g, d, lo, up, selected = _data(n, 9900 + n, False)
        xd, sd, gd, dd, ld, ud = _dev((x, sj, g, d, lo, up))
        psi = s.shifted(s.shifted(s.NormL1(LAM), xd, ld, ud, selected), sd)
        plain = s.shifted(s.shifted(s.NormL0(LAM), xd), sd)
        yd = _dev((np.random.default_rng(n).normal(size=n) * 0.1,))[0]
        want_obj = psi(yd)
        y_pv, want_pv = s.prox_value(psi, gd, 1.1)
        y_pv = y_pv.clone()
        _, *want_ps = s.prox_step(psi, gd, 1.1)
        want_ip = s.iprox_bang(_buf(n), plain, gd, dd, check=True).clone()
        xkn = _buf(n)
        for _ in range(2):
            s.iprox_step(psi, gd, dd, xkn=xkn)
            assert psi(yd) == want_obj
            s.iprox_step(plain, gd, dd, check=True, xkn=xkn)
            y2, v2 = s.prox_value(psi, gd, 1.1)
            assert v2 == want_pv and torch.equal(y2, y_pv)
            s.iprox_step(plain, gd, dd, xkn=xkn)
            assert list(s.prox_step(psi, gd, 1.1)[1:]) == want_ps
            s.iprox_step(psi, gd, dd, xkn=xkn)
            assert torch.equal(s.iprox_bang(_buf(n), plain, gd, dd, check=True), want_ip)
        assert s._lib.load().spx_sync(s.context("cuda:0")) == 0
