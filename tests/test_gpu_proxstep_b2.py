"""spx_proxstep_l1_b2: prox! of ShiftedNormL1B2 fused with the step statistics of a trust-region iteration (csrc/spx_b2.hip,
include/spx.h): y with the bits of spx_prox_l1_b2 at q_scale * q on every form of k_b2_coop, xkn = (xk + sj) + y from the y that
stands, and {h, <q, y>, <y, y>}.

Two private contexts driven through the C ABI, the data and the sizes of test_gpu_proxval_b2.py (tuning key 8 = 4 caps the
resident grid at four workgroups: register form up to 32 768, LDS form up to 65 536, the streaming forms beyond).  Context A makes
the step call; context B makes the reference call -- the plain prox! in one run of a sequence, spx_proxval_l1_b2 in a second
run -- through the same sequence of regimes, so that SpxSyncHeader::b2_last_scaled (which selects the speculative paths) is the
same on both.  [1] and [2] are checked against math.fsum of the host products to the project's TOL = 1e-12 of sum |q y| and of
sum y^2 (test_gpu_proxstep.py)."""
import ctypes
import functools
import math

import numpy as np
import pytest

import redzone

pytestmark = pytest.mark.gpu

_D = ctypes.c_double
TOL = 1e-12
INVALID = 1
POISON = -777.25
LAM = SIGMA = CHI = 1.0
ACTIVE, INACTIVE = 1.0, 1e6
SEQUENCE = [INACTIVE, INACTIVE, ACTIVE, ACTIVE, INACTIVE, INACTIVE]
SIZES = [(1, 4), (2, 4), (3, 4), (1_000, 4), (20_001, 4), (50_001, 4), (70_001, 4), (300_001, 4), (100_001, 0)]
FORM_SIZES = [20_001, 50_001, 70_001, 300_001]   # register, LDS, streaming, streaming with many tiles (key 8 = 4)
FORM_IDS = ["reg", "lds", "stream", "stream-many-tiles"]


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
            c = ctypes.c_void_p()
            s._lib.check(L.spx_ctx_create_on_stream(0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(c)))
            ctxs.append(c)
        yield s, L, ctxs[0], ctxs[1]
    finally:
        torch.cuda.synchronize()
        for c in ctxs:
            L.spx_ctx_destroy(c)


def _cap(env, cap):
    s, L, A, B = env
    for c in (A, B):
        s._lib.check(L.spx_ctx_set_tuning(c, 8, cap))


def _key18(env, v):
    s, L, A, _ = env
    s._lib.check(L.spx_ctx_set_tuning(A, 18, v))


@functools.lru_cache(maxsize=None)
def _data(n):
    """as _data of test_gpu_proxval_b2.py (seed = n); read-only"""
    rng = np.random.default_rng(n)
    x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    for v in (x, sj, q):
        v.setflags(write=False)
    return x, sj, q


def _dev(a, align8=False):
    """device copy; align8: the vector starts 8 bytes past a 16-byte boundary"""
    import torch
    t = torch.from_numpy(np.array(a))
    buf = torch.empty(t.numel() + 2, dtype=t.dtype, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()] if align8 else buf[:t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == (8 if align8 else 0)
    return v


def _fill(n, align8=False, value=POISON):
    return _dev(np.full(n, value), align8)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _prox(env, ctx, y, q, x, sj, n, delta):
    s, L = env[0], env[1]
    s._lib.check(L.spx_prox_l1_b2(ctx, _p(y), _p(q), _p(x), _p(sj), n, _D(LAM), _D(SIGMA), _D(delta), _D(CHI)))
    return y


def _proxval(env, ctx, y, q, x, sj, n, delta, q_scale=1.0):
    s, L = env[0], env[1]
    out = _D(-1.0)
    s._lib.check(L.spx_proxval_l1_b2(ctx, _p(y), _p(q), _p(x), _p(sj), n, _D(LAM), _D(SIGMA), _D(delta), _D(CHI), _D(q_scale),
                                     ctypes.byref(out)))
    return y, out.value


def _step_rc(env, ctx, y, q, x, sj, n, delta, q_scale=1.0, xkn=None, host=True, dev=None):
    L = env[1]
    st = (ctypes.c_double * 3)(POISON, POISON, POISON) if host else None
    rc = L.spx_proxstep_l1_b2(ctx, _p(y), _p(q), _p(x), _p(sj), n, _D(LAM), _D(SIGMA), _D(delta), _D(CHI), _D(q_scale), _p(xkn),
                              st, _p(dev))
    return rc, (tuple(st) if host else None)


def _step(env, ctx, y, q, x, sj, n, delta, **kw):
    rc, st = _step_rc(env, ctx, y, q, x, sj, n, delta, **kw)
    env[0]._lib.check(rc)
    return st


def _bits(v):
    return np.float64(v).view(np.uint64)


def _same_bits(a, b):
    return all(_bits(u) == _bits(v) for u, v in zip(a, b))


def _check_sums(q, y, qy, yy, what):
    """q, y: host float64 arrays; the bar and reference of tests/test_gpu_proxstep.py::_check_sums"""
    pq, py = q * y, y * y
    rqy, mqy, ryy = math.fsum(pq), math.fsum(np.abs(pq)), math.fsum(py)
    print("%s: qy %.17g ref %.17g (bar %.3g)  yy %.17g ref %.17g (bar %.3g)" % (what, qy, rqy, TOL * mqy, yy, ryy, TOL * ryy))
    assert abs(qy - rqy) <= TOL * mqy, (what, qy, rqy, mqy)
    assert abs(yy - ryy) <= TOL * ryy, (what, yy, ryy)
    return rqy, mqy, ryy


def _run_sequence(env, n, cap, align8, reference):
    """SEQUENCE on A (the step call) and B (reference: "prox" or "proxval"); calls 2, 4 and 6 are repeated.  Both contexts are put
    into the same state first (one inactive plain prox! each)."""
    import torch
    _, _, A, B = env
    x, sj, q = _data(n)
    xd, sd, qd = _dev(x, align8), _dev(sj, align8), _dev(q, align8)
    _cap(env, cap)
    try:
        for c in (A, B):
            _prox(env, c, _fill(n, align8), qd, xd, sd, n, INACTIVE)
        for k, delta in enumerate(SEQUENCE):
            what = "n %d cap %d align8 %d call %d delta %g vs %s" % (n, cap, align8, k + 1, delta, reference)
            for rep in range(2 if k % 2 == 1 else 1):
                ya, xkn, yb = _fill(n, align8), _fill(n, align8), _fill(n, align8)
                st = _step(env, A, ya, qd, xd, sd, n, delta, xkn=xkn)
                if reference == "prox":
                    _prox(env, B, yb, qd, xd, sd, n, delta)
                else:
                    _, val = _proxval(env, B, yb, qd, xd, sd, n, delta)
                    print("%s: h %.17g proxval %.17g" % (what, st[0], val))
                    assert _bits(st[0]) == _bits(val), (what, st[0], val)
                assert torch.equal(ya, yb), what
                assert torch.equal(xkn, (xd + sd) + ya), what
                if rep == 1:
                    assert _same_bits(st, st0) and torch.equal(ya, ya0) and torch.equal(xkn, xkn0), (what, st, st0)
                    continue
                ya0, xkn0, st0 = ya, xkn, st
                yh = ya.cpu().numpy()
                _check_sums(q, yh, st[1], st[2], what)
                if n >= 1_000:   # the regime assertions of test_gpu_proxval_b2.py::test_sequence
                    nrm = float(np.linalg.norm(sj + yh))
                    assert (abs(nrm - delta) <= 1e-9 * delta) if delta == ACTIVE else (nrm < 1e-3 * delta), (what, nrm)
    finally:
        _cap(env, 0)


# ------------------------------------------------------------------ 1. the sequence
@pytest.mark.parametrize("reference", ["prox", "proxval"])
@pytest.mark.parametrize("align8", [False, True], ids=["a16", "a8"])
@pytest.mark.parametrize("n,cap", SIZES, ids=["n%d-cap%d" % nc for nc in SIZES])
def test_sequence(env, n, cap, align8, reference):
    _run_sequence(env, n, cap, align8, reference)


# ------------------------------------------------------------------ 2. q_scale
@pytest.mark.parametrize("delta", [ACTIVE, INACTIVE], ids=["active", "inactive"])
@pytest.mark.parametrize("n,align8", [(20_001, False), (50_001, False), (70_001, False), (70_001, True), (300_001, False)],
                         ids=["reg", "lds", "stream16", "stream8", "stream16-many-tiles"])
def test_q_scale(env, n, align8, delta):
    """q_scale = c: y, xkn, [0] and [2] have the bits of the call on c * q formed beforehand; [1] is fsum(q y) with the UNSCALED
    q, hence 1 / c times the [1] of the pre-scaled call, to the bar."""
    import torch
    _, _, A, B = env
    c = -0.37
    x, sj, q = _data(n)
    xd, sd, qd = _dev(x, align8), _dev(sj, align8), _dev(q, align8)
    qc = _dev(q, align8)
    qc.mul_(c)                                           # one rounded multiply per element
    _cap(env, 4)
    try:
        _step(env, A, _fill(n, align8), qc, xd, sd, n, delta)      # (sets the regime the calls below follow)
        _prox(env, B, _fill(n, align8), qc, xd, sd, n, delta)
        y1, v1 = _fill(n, align8), _fill(n, align8)
        st1 = _step(env, A, y1, qd, xd, sd, n, delta, q_scale=c, xkn=v1)
        y2, v2 = _fill(n, align8), _fill(n, align8)
        st2 = _step(env, A, y2, qc, xd, sd, n, delta, xkn=v2)
        y3 = _prox(env, B, _fill(n, align8), qc, xd, sd, n, delta)
    finally:
        _cap(env, 0)
    assert torch.equal(y1, y2) and torch.equal(y1, y3) and torch.equal(v1, v2)
    assert _bits(st1[0]) == _bits(st2[0]) and _bits(st1[2]) == _bits(st2[2]), (st1, st2)
    yh = y1.cpu().numpy()
    _, mqy, _ = _check_sums(q, yh, st1[1], st1[2], "q_scale n %d unscaled q" % n)
    _check_sums(qc.cpu().numpy(), yh, st2[1], st2[2], "q_scale n %d pre-scaled q" % n)
    # both sides are within the bar of their own exact sums, which differ by the factor c up to the rounding of c * q[i]
    # (relative 2^-53 per term): 2 bars + that
    assert abs(st1[1] - st2[1] / c) <= (2 * TOL + 2.0 ** -52) * mqy, (st1[1], st2[1] / c)


# ------------------------------------------------------------------ 3. the alignment of xkn alone
@pytest.mark.parametrize("n,in8", [(70_001, False), (300_001, False), (50_001, True), (70_001, True)],
                         ids=["stream16-xkn8", "stream16-many-xkn8", "lds8-xkn16", "stream8-xkn16"])
@pytest.mark.parametrize("delta", [ACTIVE, INACTIVE], ids=["active", "inactive"])
def test_xkn_alignment_does_not_change_the_form(env, n, in8, delta):
    import torch
    _, _, A, B = env
    x, sj, q = _data(n)
    xd, sd, qd = _dev(x, in8), _dev(sj, in8), _dev(q, in8)
    _cap(env, 4)
    try:
        for c in (A, B):
            _prox(env, c, _fill(n, in8), qd, xd, sd, n, delta)
        y, xkn = _fill(n, in8), _fill(n, not in8)
        st = _step(env, A, y, qd, xd, sd, n, delta, xkn=xkn)
        yb = _prox(env, B, _fill(n, in8), qd, xd, sd, n, delta)
    finally:
        _cap(env, 0)
    assert torch.equal(y, yb) and torch.equal(xkn, (xd + sd) + y)
    _check_sums(q, y.cpu().numpy(), st[1], st[2], "xkn alignment n %d" % n)


# ------------------------------------------------------------------ 4. key 18, 5. xkn = NULL
@pytest.mark.parametrize("delta", [ACTIVE, INACTIVE], ids=["active", "inactive"])
@pytest.mark.parametrize("n", FORM_SIZES, ids=FORM_IDS)
def test_key_18_and_without_xkn(env, n, delta):
    """key 18 = 1 (composed on every form) against 0: y, xkn and [0] bit-equal, [1] and [2] each within the bar of the reference;
    xkn = NULL: y and the three sums as with xkn."""
    import torch
    _, _, A, _ = env
    x, sj, q = _data(n)
    xd, sd, qd = _dev(x), _dev(sj), _dev(q)
    _cap(env, 4)
    try:
        _step(env, A, _fill(n), qd, xd, sd, n, delta)              # (the regime)
        y0, v0 = _fill(n), _fill(n)
        st0 = _step(env, A, y0, qd, xd, sd, n, delta, xkn=v0)
        yn = _fill(n)
        stn = _step(env, A, yn, qd, xd, sd, n, delta)
        _key18(env, 1)
        y1, v1 = _fill(n), _fill(n)
        st1 = _step(env, A, y1, qd, xd, sd, n, delta, xkn=v1)
        y1n = _fill(n)
        st1n = _step(env, A, y1n, qd, xd, sd, n, delta)
    finally:
        _key18(env, 0)
        _cap(env, 0)
    assert torch.equal(y0, y1) and torch.equal(v0, v1) and _bits(st0[0]) == _bits(st1[0]), (st0, st1)
    yh = y0.cpu().numpy()
    _check_sums(q, yh, st0[1], st0[2], "key 18 = 0 n %d" % n)
    _check_sums(q, yh, st1[1], st1[2], "key 18 = 1 n %d" % n)
    assert torch.equal(yn, y0) and _same_bits(stn, st0), (stn, st0)
    assert torch.equal(y1n, y1) and _same_bits(st1n, st1), (st1n, st1)


# ------------------------------------------------------------------ 6. device results, 11. the mirror
def _mirror_problem(s, n, delta=ACTIVE):
    import torch
    x, sj, q = _data(n)
    xd, sd, qd = (torch.from_numpy(v.copy()).to("cuda:0") for v in (x, sj, q))
    psi = s.shifted(s.shifted(s.NormL1(LAM), xd, delta, s.NormL2(CHI)), sd)
    assert type(psi).__name__ == "ShiftedNormL1B2"
    return psi, qd, xd, sd


@pytest.mark.parametrize("n", [20_001, 5_000_001], ids=["reg", "stream-native-grid"])
def test_device_results_have_the_host_bits(env, n):
    import torch
    s = env[0]
    psi, qd, xd, sd = _mirror_problem(s, n)
    s.b2_prox_step_bang(torch.empty_like(qd), psi, qd, SIGMA, q_scale=-0.5)          # (the regime)
    xkn0 = torch.empty_like(qd)
    y0, h, qy, yy = s.b2_prox_step_bang(torch.empty_like(qd), psi, qd, SIGMA, q_scale=-0.5, xkn=xkn0)
    assert h == s.prox_value_bang(torch.empty_like(qd), psi, qd, SIGMA, q_scale=-0.5)[1]
    for _ in range(2):
        out = torch.full((5,), POISON, dtype=torch.float64, device="cuda:0")
        xkn = torch.empty_like(qd)
        y, o = s.b2_prox_step_bang(torch.empty_like(qd), psi, qd, SIGMA, q_scale=-0.5, xkn=xkn, out=out)
        assert o is out
        got = out.cpu().numpy()
        assert _same_bits(got[:3], (h, qy, yy)) and got[3] == POISON and got[4] == POISON, (got, h, qy, yy)
        assert torch.equal(y, y0) and torch.equal(xkn, xkn0) and torch.equal(xkn, (xd + sd) + y)
    _check_sums(qd.cpu().numpy(), y0.cpu().numpy(), qy, yy, "mirror n %d" % n)
    # both given through the C ABI: the same bits in both
    _, L, A, _ = env
    out = torch.full((3,), POISON, dtype=torch.float64, device="cuda:0")
    st = _step(env, A, torch.empty_like(qd), qd, xd, sd, n, ACTIVE, dev=out)
    assert _same_bits(out.cpu().numpy(), st)


def test_mirror_refusals(env):
    import torch
    s = env[0]
    n = 1_000
    x, sj, q = _data(n)
    psi, qd, xd, sd = _mirror_problem(s, n)
    chi = s.NormL2(CHI)
    with pytest.raises(TypeError):                       # host psi
        s.b2_prox_step(s.shifted(s.shifted(s.NormL1(LAM), x.copy(), ACTIVE, chi), sj.copy()), q.copy(), SIGMA)
    with pytest.raises(TypeError):                       # Float32
        s.b2_prox_step(s.shifted(s.shifted(s.NormL1(LAM), xd.float(), ACTIVE, chi), sd.float()), qd.float(), SIGMA)
    with pytest.raises(TypeError):                       # a separable psi
        s.b2_prox_step(s.shifted(s.shifted(s.NormL1(0.7), xd), sd), qd, SIGMA)
    with pytest.raises(TypeError):                       # a group psi
        s.b2_prox_step(s.shifted(s.shifted(s.GroupNormL2.uniform([1.0] * (n // 8), 8), xd), sd), qd, SIGMA)
    with pytest.raises(TypeError):                       # prox_step keeps refusing this psi
        s.prox_step(psi, qd, SIGMA)
    with pytest.raises(TypeError):
        s.group_prox_step(psi, qd, SIGMA)
    with pytest.raises(TypeError):                       # y is q
        s.b2_prox_step_bang(qd, psi, qd, SIGMA)
    y, h, qy, yy = s.b2_prox_step(psi, qd, SIGMA)
    assert y is psi.sol and np.isfinite(h) and h == s.prox_value(psi, qd, SIGMA)[1]


# ------------------------------------------------------------------ 7. graph replay, 8. capture refusal
def test_graph_replay(env):
    """n = 20 001, the device-only form captured after one warm call; two replays reproduce the eager y, xkn and triple bit for
    bit.  (Default queue count; no graph environment variable is touched.)"""
    import torch
    s = env[0]
    n = 20_001
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        psi, qd, xd, sd = _mirror_problem(s, n)
        y = torch.zeros(n, dtype=torch.float64, device="cuda")
        xkn = torch.zeros(n, dtype=torch.float64, device="cuda")
        out = torch.zeros(3, dtype=torch.float64, device="cuda")

        def iteration():
            s.b2_prox_step_bang(y, psi, qd, SIGMA, q_scale=-0.5, xkn=xkn, out=out)

        iteration()                                      # the warm call
        side.synchronize()
        y0, v0, o0 = y.clone(), xkn.clone(), out.clone()
        assert bool(torch.isfinite(o0).all()) and float(o0[0]) > 0.0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        iteration()
    for rep in range(2):
        for t in (y, xkn, out):
            t.fill_(POISON)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, y0) and torch.equal(xkn, v0), rep
        assert torch.equal(out.view(torch.int64), o0.view(torch.int64)), (rep, out, o0)


def test_host_valued_call_is_refused_under_capture(env):
    import torch
    s = env[0]
    n = 20_001
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        psi, qd, xd, sd = _mirror_problem(s, n)
        y = torch.full((n,), POISON, dtype=torch.float64, device="cuda")
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        s.b2_prox_step_bang(y, psi, qd, SIGMA, out=out)
        y.fill_(POISON)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        with pytest.raises(s.SpxError) as e:
            s.b2_prox_step_bang(y, psi, qd, SIGMA)       # host-valued: refused, nothing recorded
        assert e.value.status == INVALID
        s.b2_prox_step_bang(y, psi, qd, SIGMA, out=out)  # (a capture must record something)
    torch.cuda.synchronize()
    assert bool((y == POISON).all())                     # no call has run


# ------------------------------------------------------------------ 9. refusals, 10. empty
def test_refusals(env):
    import torch
    s, L, A, _ = env
    n = 1_000
    x, sj, q = _data(n)
    xd, sd, qd = _dev(x), _dev(sj), _dev(q)
    inputs = [t.clone() for t in (qd, xd, sd)]
    y, spare = _fill(n, value=-9.0), _fill(n)
    out = torch.full((3,), POISON, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    rcs = [_step_rc(env, A, y, qd, xd, sd, n, ACTIVE, xkn=t)[0] for t in (y, qd, xd, sd)]     # xkn is y / q / xk / sj
    rcs.append(_step_rc(env, A, qd, qd, xd, sd, n, ACTIVE, xkn=spare, dev=out)[0])             # y is q
    rcs.append(_step_rc(env, A, y, qd, xd, sd, n, ACTIVE, xkn=spare, host=False, dev=None)[0])  # both results NULL
    assert rcs == [INVALID] * 6, rcs
    assert len(L.spx_last_error()) > 0
    torch.cuda.synchronize()
    assert bool((y == -9.0).all()) and bool((spare == POISON).all()) and bool((out == POISON).all())   # nothing was launched
    for t, t0 in zip((qd, xd, sd), inputs):
        assert torch.equal(t, t0)
    st = _step(env, A, y, qd, xd, sd, n, ACTIVE, xkn=spare)                                    # and the context is fine
    assert np.isfinite(st[0]) and st[0] > 0.0


def test_empty(env):
    import torch
    s, L, A, _ = env
    st = (ctypes.c_double * 3)(1.0, 2.0, 3.0)
    out = torch.full((3,), POISON, dtype=torch.float64, device="cuda:0")
    tail = (_D(LAM), _D(SIGMA), _D(ACTIVE), _D(CHI), _D(1.0), None)
    assert L.spx_proxstep_l1_b2(A, None, None, None, None, 0, *tail, st, _p(out)) == 0
    assert list(st) == [0.0, 0.0, 0.0] and out.cpu().tolist() == [0.0, 0.0, 0.0]
    out.fill_(POISON)
    assert L.spx_proxstep_l1_b2(A, None, None, None, None, 0, *tail, None, _p(out)) == 0
    assert out.cpu().tolist() == [0.0, 0.0, 0.0]


# ------------------------------------------------------------------ 12. guard bands
@pytest.mark.parametrize("key18", [0, 1], ids=["default-route", "composed"])
@pytest.mark.parametrize("mode", ["A", "C"])
@pytest.mark.parametrize("n", FORM_SIZES, ids=FORM_IDS)
def test_guard_bands(env, n, mode, key18):
    """y and xkn are outputs: no byte outside either written, no element of either left unwritten, no input modified.  A: every
    vector 16-byte aligned; C: the inputs at +8 B."""
    import torch
    s, L, A, B = env
    x, sj, q = _data(n)
    ay, ai = redzone.F64_MODES[mode]
    zone = redzone.Zone()
    yb = zone.add(n, torch.float64, ay, role="out", name="y")
    vb = zone.add(n, torch.float64, ay, role="out", name="xkn")
    qb, xb, sb = (zone.add(n, torch.float64, ai, data=np.array(v), name=nm) for v, nm in ((q, "q"), (x, "xk"), (sj, "sj")))
    st = (ctypes.c_double * 3)()
    cp = lambda b: ctypes.c_void_p(b.ptr())
    _cap(env, 4)
    _key18(env, key18)
    try:
        torch.cuda.synchronize()
        s._lib.check(L.spx_proxstep_l1_b2(A, cp(yb), cp(qb), cp(xb), cp(sb), n, _D(LAM), _D(SIGMA), _D(ACTIVE), _D(CHI), _D(1.0),
                                          cp(vb), st, None))
        torch.cuda.synchronize()
        zone.check()
        y0 = torch.empty(n, dtype=torch.float64, device="cuda:0")
        s._lib.check(L.spx_ctx_set_tuning(B, 8, 4))
        _prox(env, B, y0, qb.t, xb.t, sb.t, n, ACTIVE)
    finally:
        _key18(env, 0)
        _cap(env, 0)
    assert torch.equal(vb.t, (xb.t + sb.t) + yb.t)
    err = float((yb.t - y0).abs().max())
    print("guarded n %d mode %s: max |y - plain prox| %.3e" % (n, mode, err))
    assert err <= 1e-12 * max(float(np.linalg.norm(x)), 1.0)      # (the contexts' regimes may differ here: the bar of test_gpu_redzone.py::_b2)
    _check_sums(q, yb.t.cpu().numpy(), st[1], st[2], "guarded n %d mode %s" % (n, mode))


# ------------------------------------------------------------------ 13. the context afterwards
@pytest.mark.parametrize("n", FORM_SIZES, ids=FORM_IDS)
def test_leaves_the_context_clean(env, n):
    """after the step call -- both routes -- spx_prox_l1_b2, spx_proxval_l1_b2 and a top-r prox! on the same context give the bits
    they gave before"""
    import torch
    s, L, A, _ = env
    x, sj, q = _data(n)
    xd, sd, qd = _dev(x), _dev(sj), _dev(q)
    r = n // 100

    def topr():
        y = _fill(n)
        s._lib.check(L.spx_prox_indball_l0(A, _p(y), _p(qd), _p(xd), _p(sd), n, r))
        return y

    _cap(env, 4)
    try:
        _prox(env, A, _fill(n), qd, xd, sd, n, ACTIVE)             # (the regime: every call below follows an active one)
        y0 = _prox(env, A, _fill(n), qd, xd, sd, n, ACTIVE)
        y1, v1 = _proxval(env, A, _fill(n), qd, xd, sd, n, ACTIVE)
        t0 = topr()
        st0 = _step(env, A, _fill(n), qd, xd, sd, n, ACTIVE)
        for key18 in (0, 1, 0):
            _key18(env, key18)
            xkn = _fill(n)
            assert _bits(_step(env, A, _fill(n), qd, xd, sd, n, ACTIVE, xkn=xkn)[0]) == _bits(st0[0])
            assert torch.equal(_prox(env, A, _fill(n), qd, xd, sd, n, ACTIVE), y0)
            _step(env, A, _fill(n), qd, xd, sd, n, ACTIVE, xkn=xkn)
            y, v = _proxval(env, A, _fill(n), qd, xd, sd, n, ACTIVE)
            assert _bits(v) == _bits(v1) and torch.equal(y, y1)
            _step(env, A, _fill(n), qd, xd, sd, n, ACTIVE, xkn=xkn)
            assert torch.equal(topr(), t0)
    finally:
        _key18(env, 0)
        _cap(env, 0)
    assert L.spx_sync(A) == 0


# ------------------------------------------------------------------ 14. a trust-region loop
def test_trust_region_loop(env):
    """Ten iterations of a trust-region proximal-gradient loop on a lasso (f = 1/2 ||D x - b||^2 with a diagonal D, h = lambda
    ||.||_1), n = 20 001: written with b2_prox_step, and with prox_value + torch.dot + xk + y.  Identical iterates, bit for bit,
    and the same accept / reject decisions."""
    import torch
    s = env[0]
    n = 20_001
    rng = np.random.default_rng(14)
    d = torch.from_numpy(rng.uniform(0.5, 1.5, size=n)).cuda()
    b = torch.from_numpy(rng.normal(size=n)).cuda()
    lam, nu = 0.1, 0.5

    def run(fused):
        xk = torch.zeros(n, dtype=torch.float64, device="cuda")
        delta, trace, iterates = 1.0, [], []
        for it in range(10):
            res = d * xk - b
            fk, grad = 0.5 * float(torch.dot(res, res)), d * res
            hk = lam * float(xk.abs().sum())
            psi = s.shifted(s.NormL1(lam), xk, delta, s.NormL2(1.0))
            y = torch.empty_like(xk)
            if fused:
                xkn = torch.empty_like(xk)
                _, hn, gs, ss = s.b2_prox_step_bang(y, psi, grad, nu, q_scale=-nu, xkn=xkn)
            else:
                _, hn = s.prox_value_bang(y, psi, grad, nu, q_scale=-nu)
                gs, ss = float(torch.dot(grad, y)), float(torch.dot(y, y))
                xkn = (xk + psi.sj) + y
            resn = d * xkn - b
            fn = 0.5 * float(torch.dot(resn, resn))
            pred = -(gs + hn - hk)
            rho = ((fk + hk) - (fn + hn)) / pred if pred > 0 else -1.0
            accept = rho >= 1e-4
            trace.append((bool(accept), _bits(hn)))
            if accept:
                xk = xkn
            delta = 2.0 * delta if rho >= 0.9 else (delta if accept else 0.5 * delta)
            iterates.append(xk.clone())
        return trace, iterates

    ta, ia = run(True)
    tb, ib = run(False)
    print("accept / reject:", [a for a, _ in ta])
    assert [a for a, _ in ta] == [a for a, _ in tb]
    assert ta == tb
    for u, v in zip(ia, ib):
        assert torch.equal(u, v)
    assert any(a for a, _ in ta)


# ------------------------------------------------------------------ 15. soak
@pytest.mark.soak
@pytest.mark.parametrize("reference", ["prox", "proxval"])
def test_soak_native_grid(env, reference):
    _run_sequence(env, 16_000_000, 0, False, reference)
