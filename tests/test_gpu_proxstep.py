"""GPU: prox! fused with the step statistics of a solver iteration (spx_proxstep_*, prox_step / prox_step_bang).

One call stores y (bit-identical to the plain prox!), xkn = (xk + sj) + y for every i, and three sums:
h = lambda * sum over the SELECTED indices of Term((xk + sj) + y), qy = sum over ALL i of q[i] y[i] with the unscaled q,
yy = sum over ALL i of y[i]^2.

Bars.  y and xkn: equal bits (torch.equal).  h against psi(y_plain): the bars of test_prox_value_fused (NormL0 exactly, else
<= 1e-12 relative); against prox_value of the same call: equal bits when both take the same kernel form.  qy and yy against
math.fsum (exactly rounded) of the host products q[i] * y[i] and y[i] * y[i] -- the same rounded products the device forms,
the library is built without contraction: |got - ref| <= 1e-12 * sum |q[i] y[i]| (the terms of qy change sign, so the bar is
on the sum of magnitudes) and likewise for yy.  1e-12 is the project's bar for these blocked sums at n = 1_000_003.

Sizes sit at the tile edges: a workgroup of the LDS-staged kernel covers 3072 elements with scalar bounds and 1536 with
vector bounds; one workgroup can finish at most 2048 partial slots (beyond: the separate three-sum reduction)."""
import ctypes
import math

import numpy as np
import pytest

import redzone

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 1000, 1535, 1536, 1537, 3071, 3072, 3073, 1_000_003]
TOL = 1e-12
INVALID = 1
POISON = -777.25


@pytest.fixture(scope="module")
def s():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.build()


def _data(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=n)
    sj = rng.uniform(-0.5, 0.5, size=n)
    q = rng.normal(size=n)
    lo, up = -1.0 - 0.1 * rng.random(n), 1.0 + 0.1 * rng.random(n)
    selected = sorted(rng.choice(n, size=max(1, n // 3), replace=False).tolist())
    return x, sj, q, lo, up, selected


def _dev(arrs, misaligned=False):
    import torch
    if misaligned:  # every vector 8 bytes off a 16-byte boundary
        return [torch.cat([torch.zeros(1, dtype=torch.float64), torch.from_numpy(np.ascontiguousarray(a))]).cuda()[1:] for a in arrs]
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrs]


def _buf(n, misaligned=False, fill=POISON):
    import torch
    t = torch.full((n + 1,), fill, dtype=torch.float64, device="cuda:0")
    return t[1:] if misaligned else t[:n]


def _nine(s, xd, sd, ld, ud, selected):
    """L1 / L0 / Lhalf, each unboxed, with a scalar box, and with vector bounds plus a selected third of the indices"""
    cases = []
    for H, kind in ((s.NormL1, "l1"), (s.NormL0, "l0"), (s.RootNormLhalf, "lhalf")):
        cases.append((s.shifted(s.shifted(H(0.7), xd), sd), kind, "plain"))
        cases.append((s.shifted(s.shifted(H(0.7), xd, 0.9, s.NormLinf(1.0)), sd), kind, "box"))
        cases.append((s.shifted(s.shifted(H(0.7), xd, ld, ud, selected), sd), kind, "vecbox+mask"))
    return cases


def _sum_refs(q, y):
    """(fsum of q*y, fsum of |q*y|, fsum of y*y) from host float64 arrays"""
    qy = q * y
    yy = y * y
    return math.fsum(qy), math.fsum(np.abs(qy)), math.fsum(yy)


def _check_sums(q, y, qy, yy, what):
    rqy, mqy, ryy = _sum_refs(q, y)
    print("%s: qy %.17g ref %.17g (bar %.3g)  yy %.17g ref %.17g (bar %.3g)" % (what, qy, rqy, TOL * mqy, yy, ryy, TOL * ryy))
    assert abs(qy - rqy) <= TOL * mqy, (what, qy, rqy, mqy)
    assert abs(yy - ryy) <= TOL * ryy, (what, yy, ryy)


def _check_h(kind, h, exp, what):
    assert np.isfinite(exp)
    if kind == "l0":
        assert h == exp, (what, h, exp)
    else:
        assert abs(h - exp) <= TOL * max(abs(exp), 1e-300), (what, h, exp)


def _full_check(s, psi, kind, q, qd, xd, sd, xkn, what, sigma=1.1, same_form=True):
    """one prox_step call against the plain prox, psi(y), prox_value and the fsum references; returns (y, h, qy, yy)"""
    import torch
    y_plain = s.prox(psi, qd, sigma).clone()
    exp = psi(y_plain)
    _, v_pv = s.prox_value(psi, qd, sigma)
    xkn.fill_(POISON)
    y, h, qy, yy = s.prox_step(psi, qd, sigma, xkn=xkn)
    assert torch.equal(y, y_plain), what
    assert torch.equal(xkn, (xd + sd) + y), what
    _check_h(kind, h, exp, what)
    if same_form:
        assert h == v_pv, (what, h, v_pv)   # the same skeleton under the same keys adds the same terms in the same order
    else:
        _check_h(kind, h, v_pv, what)
    _check_sums(q, y.cpu().numpy(), qy, yy, what)
    return y, h, qy, yy


# ------------------------------------------------------------------ the nine psi at the tile edges, both alignments
@pytest.mark.parametrize("n", SIZES)
def test_prox_step_nine_psi(s, n):
    x, sj, q, lo, up, selected = _data(n, 9100 + n)
    for misaligned in (False, True):
        xd, sd, qd, ld, ud = _dev((x, sj, q, lo, up), misaligned)
        xkn = _buf(n, misaligned)
        for psi, kind, form in _nine(s, xd, sd, ld, ud, selected):
            _full_check(s, psi, kind, q, qd, xd, sd, xkn, "%s %s n=%d mis=%s" % (kind, form, n, misaligned))


def test_prox_step_sums_run_over_the_right_index_sets(s):
    """qy and yy run over ALL elements, h over the SELECTED ones: the unselected elements carry y = clamp(q) != 0, so a sum
    over the wrong index set lands far outside the bars"""
    n = 3073
    x, sj, q, lo, up, selected = _data(n, 9201)
    xd, sd, qd, ld, ud = _dev((x, sj, q, lo, up))
    lam = 0.7
    psi = s.shifted(s.shifted(s.NormL1(lam), xd, ld, ud, selected), sd)
    xkn = _buf(n)
    y, h, qy, yy = s.prox_step(psi, qd, 1.1, xkn=xkn)
    yh = y.cpu().numpy()
    sel = np.zeros(n, dtype=bool)
    sel[selected] = True
    assert np.count_nonzero(yh[~sel]) > n // 2              # the unselected elements do carry a step
    v = np.abs((x + sj) + yh)
    h_sel, h_all = lam * math.fsum(v[sel]), lam * math.fsum(v)
    assert abs(h - h_sel) <= TOL * h_sel and abs(h - h_all) > 1e-3 * h_all, (h, h_sel, h_all)
    rqy, mqy, ryy = _sum_refs(q, yh)
    assert abs(qy - rqy) <= TOL * mqy and abs(yy - ryy) <= TOL * ryy
    qy_sel, yy_sel = math.fsum((q * yh)[sel]), math.fsum((yh * yh)[sel])
    assert abs(qy - qy_sel) > 1e-3 * mqy and abs(yy - yy_sel) > 1e-3 * ryy, (qy, qy_sel, yy, yy_sel)


@pytest.mark.parametrize("n", [3073, 1_000_003])
def test_prox_step_q_scale(s, n):
    """the prox at q_scale * q formed on the fly: y, xkn, h, yy have the bits of the call on the scaled vector; qy is taken
    with the UNSCALED q, so qy * q_scale is the other call's qy"""
    import torch
    x, sj, q, lo, up, selected = _data(n, 9300 + n)
    xd, sd, qd, ld, ud = _dev((x, sj, q, lo, up))
    qs = -0.37
    q2d = qs * qd
    for psi in (s.shifted(s.shifted(s.NormL1(0.7), xd, 0.9, s.NormLinf(1.0)), sd), s.shifted(s.shifted(s.NormL0(0.7), xd), sd),
                s.shifted(s.shifted(s.RootNormLhalf(0.7), xd, ld, ud, selected), sd)):
        k1, k2 = _buf(n), _buf(n)
        y1, h1, qy1, yy1 = s.prox_step(psi, qd, 1.1, q_scale=qs, xkn=k1)
        y1 = y1.clone()
        y2, h2, qy2, yy2 = s.prox_step(psi, q2d, 1.1, xkn=k2)
        assert torch.equal(y1, y2) and torch.equal(k1, k2), type(psi).__name__
        assert h1 == h2 and yy1 == yy2, (type(psi).__name__, h1, h2, yy1, yy2)
        mag = math.fsum(np.abs(q2d.cpu().numpy() * y2.cpu().numpy()))
        assert abs(qy1 * qs - qy2) <= TOL * mag, (type(psi).__name__, qy1 * qs, qy2, mag)
        _check_sums(q, y1.cpu().numpy(), qy1, yy1, "q_scale " + type(psi).__name__)


def test_prox_step_more_slots_than_one_workgroup_adds(s):
    """vector bounds at n = 3_200_001: 2084 workgroups > 2048, so the separate three-sum reduction and its long-list branch run"""
    n = 3_200_001
    x, sj, q, lo, up, selected = _data(n, 9400)
    xd, sd, qd, ld, ud = _dev((x, sj, q, lo, up))
    psi = s.shifted(s.shifted(s.NormL1(0.7), xd, ld, ud, selected), sd)
    _full_check(s, psi, "l1", q, qd, xd, sd, _buf(n), "2084 workgroups")


# ------------------------------------------------------------------ kernel forms
def _set(s, key, v):
    s._lib.check(s._lib.load().spx_ctx_set_tuning(s.context("cuda:0"), key, v))


FORMS = [  # (name, {key: value}) on top of the defaults key 0 = 0, key 1 = 1, key 3 = 1
    ("lds", {}),
    ("vec-nt", {3: 0}),
    ("vec-plain", {3: 0, 1: 0}),
    ("vec-gridstride", {3: 0, 0: 2}),
]


@pytest.mark.parametrize("n", [3073, 6144, 1_000_003])
def test_prox_step_kernel_forms(s, n):
    """LDS-staged, register-staged (non-temporal / plain / grid-stride) skeletons, each with key 17 at 1 and 0: y and xkn have
    equal bits across all of them, the three sums equal bits between key 17 = 0 and 1, and across skeletons they meet the
    bars.  (n = 6144 is even: one launch covers the vector, so key 17 = 1 takes the one-launch finish.)"""
    import torch
    x, sj, q, lo, up, selected = _data(n, 9500 + n)
    xd, sd, qd, ld, ud = _dev((x, sj, q, lo, up))
    psis = [(s.shifted(s.shifted(s.NormL1(0.7), xd), sd), "l1"),
            (s.shifted(s.shifted(s.NormL1(0.7), xd, ld, ud, selected), sd), "l1"),
            (s.shifted(s.shifted(s.RootNormLhalf(0.7), xd, 0.9, s.NormLinf(1.0)), sd), "lhalf")]
    try:
        for psi, kind in psis:
            y_plain = s.prox(psi, qd, 1.1).clone()
            exp = psi(y_plain)
            xkn_ref = (xd + sd) + y_plain
            for name, keys in FORMS:
                for k, v in keys.items():
                    _set(s, k, v)
                got = {}
                for k17 in (1, 0):
                    _set(s, 17, k17)
                    xkn = _buf(n)
                    y, h, qy, yy = s.prox_step(psi, qd, 1.1, xkn=xkn)
                    what = "%s %s key17=%d n=%d" % (type(psi).__name__, name, k17, n)
                    assert torch.equal(y, y_plain) and torch.equal(xkn, xkn_ref), what
                    _check_h(kind, h, exp, what)
                    _check_sums(q, y_plain.cpu().numpy(), qy, yy, what)
                    got[k17] = (h, qy, yy)
                assert got[0] == got[1], (type(psi).__name__, name, got)
                _set(s, 17, 1); _set(s, 3, 1); _set(s, 1, 1); _set(s, 0, 0)
    finally:
        _set(s, 17, 1); _set(s, 3, 1); _set(s, 1, 1); _set(s, 0, 0)


@pytest.mark.parametrize("n,vecb", [(6146, False), (30722, False), (3074, True)])
def test_prox_value_and_step_xcd_contiguous_tiles(s, n, vecb):
    """key 5 = 1 (XCD-contiguous tile ranges): the grid is rounded up to a multiple of 8 workgroups, the workgroup ids are
    remapped, and the workgroups left without a tile store zero slots.  Scalar bounds, 3072 elements per workgroup: n = 6146 is
    3 working workgroups of 8 launched, n = 30722 is 11 of 16 with remapped ids; vector bounds and a mask, 1536 per workgroup:
    n = 3074 is 3 of 8; the last tile is one pair each time.  Against the key 5 = 0 call: y and xkn have equal bits, and so
    have the value and the three sums -- the same tile lands in the same slot, and the extra slots add +0.0."""
    import torch
    x, sj, q, lo, up, selected = _data(n, 9550 + n)
    xd, sd, qd, ld, ud = _dev((x, sj, q, lo, up))
    if vecb:
        psi = s.shifted(s.shifted(s.NormL1(0.7), xd, ld, ud, selected), sd)
    else:
        psi = s.shifted(s.shifted(s.NormL1(0.7), xd, 0.9, s.NormLinf(1.0)), sd)
    got = {}
    try:
        for k5 in (0, 1):
            _set(s, 5, k5)
            y_pv, v = s.prox_value(psi, qd, 1.1)
            y_pv = y_pv.clone()
            xkn = _buf(n)
            y, h, qy, yy = s.prox_step(psi, qd, 1.1, xkn=xkn)
            got[k5] = (y_pv, y.clone(), xkn, [float(t).hex() for t in (v, h, qy, yy)])
    finally:
        _set(s, 5, 0)
    what = "key 5 n=%d vecb=%s" % (n, vecb)
    print(what, got[0][3], got[1][3])
    for a, b in zip(got[0][:3], got[1][:3]):
        assert torch.equal(a, b), what
    assert got[0][3] == got[1][3], (what, got[0][3], got[1][3])
    assert torch.equal(got[1][0], got[1][1]) and torch.equal(got[1][2], (xd + sd) + got[1][1]), what
    _check_h("l1", float.fromhex(got[1][3][1]), psi(got[1][1]), what)
    _check_sums(q, got[1][1].cpu().numpy(), float.fromhex(got[1][3][2]), float.fromhex(got[1][3][3]), what)


def test_prox_step_xkn_alone_misaligned(s):
    """every other vector 16-byte aligned and xkn 8 bytes off, and the reverse: the call takes the element-wise route, stores
    every element and nothing else"""
    import torch
    n = 3073
    x, sj, q, lo, up, selected = _data(n, 9600)
    for vec_mis, xkn_mis in ((False, True), (True, False)):
        xd, sd, qd, ld, ud = _dev((x, sj, q, lo, up), vec_mis)
        full = torch.full((n + 3,), POISON, dtype=torch.float64, device="cuda:0")
        xkn = full[2:n + 2] if not xkn_mis else full[1:n + 1]
        assert (xkn.data_ptr() % 16 == 8) == xkn_mis and (qd.data_ptr() % 16 == 8) == vec_mis
        for psi, kind, form in _nine(s, xd, sd, ld, ud, selected):
            _full_check(s, psi, kind, q, qd, xd, sd, xkn, "%s %s vec_mis=%s xkn_mis=%s" % (kind, form, vec_mis, xkn_mis),
                        same_form=False)
            lo_i = 1 if xkn_mis else 2
            assert bool((full[:lo_i] == POISON).all()) and bool((full[lo_i + n:] == POISON).all())


def test_prox_step_without_xkn(s):
    """xkn=None: y and the sums unchanged, a poisoned spare buffer stays untouched"""
    import torch
    for n in (1537, 3073):
        x, sj, q, lo, up, selected = _data(n, 9700 + n)
        xd, sd, qd, ld, ud = _dev((x, sj, q, lo, up))
        spare = _buf(n)
        for psi, kind, form in _nine(s, xd, sd, ld, ud, selected):
            xkn = _buf(n)
            y1, h1, qy1, yy1 = s.prox_step(psi, qd, 1.1, xkn=xkn)
            y1 = y1.clone()
            y2, h2, qy2, yy2 = s.prox_step(psi, qd, 1.1)
            assert torch.equal(y1, y2) and (h1, qy1, yy1) == (h2, qy2, yy2), (kind, form, n)
        torch.cuda.synchronize()
        assert bool((spare == POISON).all())


# ------------------------------------------------------------------ guard bands
def _D(v):
    return ctypes.c_double(v)


@pytest.mark.parametrize("mode", ["A", "B"])
@pytest.mark.parametrize("vecb", [False, True])
@pytest.mark.parametrize("n", [1537, 3073])
def test_prox_step_guard_bands(s, n, vecb, mode):
    """L1Box with scalar bounds / vector bounds + mask through the C ABI on guarded buffers: y and xkn are outputs (every
    element written, nothing outside them), the inputs are guarded against reads past the end (the poison would move y or a
    sum) and against writes"""
    import torch
    L, ctx = s._lib.load(), s.context("cuda:0")
    ay, ai = redzone.F64_MODES[mode]
    x, sj, q, lo, up, selected = _data(n, 9800 + n)
    mask = np.zeros(n, dtype=np.uint8)
    mask[selected] = 1
    z = redzone.Zone()
    yb = z.add(n, torch.float64, ay, role="out", name="y")
    kb = z.add(n, torch.float64, ay, role="out", name="xkn")
    qb, xb, sb = (z.add(n, torch.float64, ai, data=a, name=nm) for a, nm in ((q, "q"), (x, "xk"), (sj, "sj")))
    lam, sigma = 0.7, 1.1
    st = (ctypes.c_double * 3)()
    p = lambda g: ctypes.c_void_p(g.ptr())
    if vecb:
        lb, ub = z.add(n, torch.float64, ai, data=lo, name="l"), z.add(n, torch.float64, ai, data=up, name="u")
        mb = z.add(n, torch.uint8, 1 if mode == "B" else 0, data=mask, name="mask")   # (mode B: the mask peels with the vectors)
        s._lib.check(L.spx_proxstep_l1_box(ctx, p(yb), p(qb), p(xb), p(sb), n, _D(lam), _D(sigma), p(lb), p(ub), _D(0.0), _D(0.0),
                                           p(mb), _D(1.0), p(kb), st, None))
        xd, sd, qd, ld, ud = _dev((x, sj, q, lo, up))
        psi = s.shifted(s.shifted(s.NormL1(lam), xd, ld, ud, selected), sd)
    else:
        s._lib.check(L.spx_proxstep_l1_box(ctx, p(yb), p(qb), p(xb), p(sb), n, _D(lam), _D(sigma), None, None, _D(-0.9), _D(0.9),
                                           None, _D(1.0), p(kb), st, None))
        xd, sd, qd = _dev((x, sj, q))
        psi = s.shifted(s.shifted(s.NormL1(lam), xd, 0.9, s.NormLinf(1.0)), sd)
    torch.cuda.synchronize()
    z.check()
    y_plain = s.prox(psi, qd, sigma).clone()
    assert torch.equal(yb.t, y_plain) and torch.equal(kb.t, (xd + sd) + y_plain)
    _check_h("l1", st[0], psi(y_plain), "guard bands")
    _check_sums(q, y_plain.cpu().numpy(), st[1], st[2], "guard bands n=%d vecb=%s mode=%s" % (n, vecb, mode))


# ------------------------------------------------------------------ device results, graph
def test_prox_step_device_results_have_the_host_bits(s):
    import torch
    for n in (3072, 3073, 50_000):
        x, sj, q, lo, up, selected = _data(n, 9900 + n)
        xd, sd, qd, ld, ud = _dev((x, sj, q, lo, up))
        for psi, kind, form in _nine(s, xd, sd, ld, ud, selected):
            xkn = _buf(n)
            y1, h, qy, yy = s.prox_step(psi, qd, 1.1, xkn=xkn)
            y1 = y1.clone()
            out = torch.full((5,), POISON, dtype=torch.float64, device="cuda:0")
            y2, o = s.prox_step(psi, qd, 1.1, xkn=xkn, out=out)
            assert o is out and torch.equal(y1, y2)
            got = out.cpu().numpy()
            assert (got[0], got[1], got[2]) == (h, qy, yy), (kind, form, n)
            assert got[3] == POISON and got[4] == POISON


def test_prox_step_in_a_graph(s):
    """one prox_step(..., xkn=, out=) at n = 50_000 run eagerly, then captured and replayed three times with q changed between
    the replays: y, xkn and out after each replay are the eager call's"""
    import torch
    n = 50_000
    x, sj, q, lo, up, selected = _data(n, 9950)
    rng = np.random.default_rng(9951)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xd, sd, ld, ud = _dev((x, sj, lo, up))
        qd = torch.from_numpy(q).cuda()
        psi = s.shifted(s.shifted(s.NormL1(0.7), xd, ld, ud, selected), sd)
        y = torch.zeros(n, dtype=torch.float64, device="cuda")
        xkn = torch.zeros(n, dtype=torch.float64, device="cuda")
        out = torch.zeros(3, dtype=torch.float64, device="cuda")

        def step():
            s.prox_step_bang(y, psi, qd, 1.1, q_scale=-0.9, xkn=xkn, out=out)

        step(); step()      # eager, on the capture stream: the workspace reaches its size
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    for rep in range(3):
        qd.copy_(torch.from_numpy(rng.normal(size=n) * (1.0 + rep)))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            step()
        side.synchronize()
        want = (y.clone(), xkn.clone(), out.clone())
        for t in (y, xkn, out):
            t.fill_(POISON)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, want[0]) and torch.equal(xkn, want[1]), rep
        assert torch.equal(out.view(torch.int64), want[2].view(torch.int64)), (rep, out, want[2])
        _check_sums(qd.cpu().numpy(), y.cpu().numpy(), float(out[1]), float(out[2]), "replay %d" % rep)


# ------------------------------------------------------------------ errors
def test_prox_step_errors(s):
    import torch
    L, ctx = s._lib.load(), s.context("cuda:0")
    n = 1000
    x, sj, q, lo, up, selected = _data(n, 9960)
    xd, sd, qd, ld, ud = _dev((x, sj, q, lo, up))
    y = _buf(n)
    y0 = y.clone()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = (ctypes.c_double * 3)()
    spare = _buf(n)
    head = (ctx, p(y), p(qd), p(xd), p(sd), n, _D(0.7), _D(1.1), _D(1.0))
    cases = [L.spx_proxstep_l1(*head, p(t), st, None) for t in (y, qd, xd, sd)]                       # xkn is y / q / xk / sj
    cases.append(L.spx_proxstep_l1(ctx, p(y), p(y), p(xd), p(sd), n, _D(0.7), _D(1.1), _D(1.0), p(spare), st, None))  # y is q
    cases.append(L.spx_proxstep_l1(*head, p(spare), None, None))                                     # both results NULL
    cases.append(L.spx_proxstep_l1_box(ctx, p(y), p(qd), p(xd), p(sd), n, _D(0.7), _D(1.1), p(ld), p(ud), _D(0.0), _D(0.0), None,
                                       _D(1.0), p(ld), st, None))                                     # xkn is l_vec
    for k, rc in enumerate(cases):
        assert rc == INVALID, (k, rc)
    assert len(L.spx_last_error()) > 0
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and bool((spare == POISON).all())          # nothing was launched
    # the mirror: the same through SpxError / TypeError
    psi = s.shifted(s.shifted(s.NormL1(0.7), xd), sd)
    for bad in (qd, xd, sd):
        with pytest.raises(s.SpxError):
            s.prox_step_bang(y, psi, qd, 1.1, xkn=bad)
    with pytest.raises((TypeError, s.SpxError)):
        s.prox_step_bang(y, psi, qd, 1.1, xkn=y)
    with pytest.raises(TypeError):
        s.prox_step_bang(qd, psi, qd, 1.1)
    with pytest.raises(TypeError):
        s.prox_step(psi, qd, 1.1, out=torch.zeros(2, dtype=torch.float64, device="cuda:0"))
    grp = s.shifted(s.shifted(s.GroupNormL2.uniform([1.0] * (n // 100), 100), xd), sd)
    top = s.shifted(s.shifted(s.IndBallL0(10), xd), sd)
    b2 = s.shifted(s.shifted(s.NormL1(1.0), xd, 1.0, s.NormL2(1.0)), sd)
    f32 = s.shifted(s.shifted(s.NormL1(0.7), xd.float()), sd.float())
    host = s.shifted(s.shifted(s.NormL1(0.7), x.copy()), sj.copy())
    for psi_bad, qq in ((grp, qd), (top, qd), (b2, qd), (f32, qd.float()), (host, q)):
        with pytest.raises(TypeError, match="ShiftedNormL1 / ShiftedNormL0 / ShiftedRootNormLhalf"):
            s.prox_step(psi_bad, qq, 1.1)
    torch.cuda.synchronize()
    assert torch.equal(y, y0)


def test_prox_step_host_valued_call_is_refused_under_capture(s):
    import torch
    n = 4096
    x, sj, q, lo, up, selected = _data(n, 9970)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xd, sd, qd = _dev((x, sj, q))
        psi = s.shifted(s.shifted(s.NormL1(0.7), xd), sd)
        y = torch.full((n,), POISON, dtype=torch.float64, device="cuda")
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        s.prox_step_bang(y, psi, qd, 1.1, out=out)
        y.fill_(POISON)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        with pytest.raises(s.SpxError) as e:
            s.prox_step_bang(y, psi, qd, 1.1)          # host-valued: refused, nothing recorded
        assert e.value.status == INVALID
        s.prox_step_bang(y, psi, qd, 1.1, out=out)     # (a capture must record something)
    torch.cuda.synchronize()
    assert bool((y == POISON).all())                   # neither call has run


def test_prox_step_empty(s):
    """n == 0 is the success case: host zeros, and device zeros stored by a kernel"""
    import torch
    e = torch.zeros(0, dtype=torch.float64, device="cuda:0")
    psi = s.shifted(s.shifted(s.NormL1(0.7), e), e.clone())
    y, h, qy, yy = s.prox_step(psi, e.clone(), 1.1)
    assert (h, qy, yy) == (0.0, 0.0, 0.0) and y.numel() == 0
    out = torch.full((3,), POISON, dtype=torch.float64, device="cuda:0")
    s.prox_step(psi, e.clone(), 1.1, out=out)
    assert out.cpu().tolist() == [0.0, 0.0, 0.0]
    L, ctx = s._lib.load(), s.context("cuda:0")
    st = (ctypes.c_double * 3)(1.0, 2.0, 3.0)
    assert L.spx_proxstep_l0_box(ctx, None, None, None, None, 0, _D(0.7), _D(1.1), None, None, _D(-1.0), _D(1.0), None, _D(1.0),
                                 None, st, None) == 0
    assert list(st) == [0.0, 0.0, 0.0]


# ------------------------------------------------------------------ the context afterwards
def test_prox_step_leaves_the_context_clean(s):
    """after a prox_step call, psi(y), prox_value and a top-r prox! on the same context give their usual bits: tickets and
    workspace are left clean (the pattern of test_objective_one_launch_same_bits)"""
    import torch
    for n in (3072, 50_000, 1_000_000):
        x, sj, q, lo, up, selected = _data(n, 9980 + n)
        xd, sd, qd, ld, ud = _dev((x, sj, q, lo, up))
        psi = s.shifted(s.shifted(s.NormL1(0.7), xd, ld, ud, selected), sd)
        top = s.shifted(s.shifted(s.IndBallL0(max(1, n // 50)), xd, 0.8, s.NormLinf(1.0)), sd)
        yd = _dev((np.random.default_rng(n).normal(size=n) * 0.1,))[0]
        want_obj = psi(yd)
        y_pv, want_pv = s.prox_value(psi, qd, 1.1)
        y_pv = y_pv.clone()
        want_top = s.prox(top, qd, 1.0).clone()
        xkn = _buf(n)
        for _ in range(2):
            s.prox_step(psi, qd, 1.1, xkn=xkn)
            assert psi(yd) == want_obj
            s.prox_step(psi, qd, 1.1, xkn=xkn)
            y2, v2 = s.prox_value(psi, qd, 1.1)
            assert v2 == want_pv and torch.equal(y2, y_pv)
            s.prox_step(psi, qd, 1.1, xkn=xkn)
            assert torch.equal(s.prox(top, qd, 1.0), want_top)
        assert s._lib.load().spx_sync(s.context("cuda:0")) == 0
