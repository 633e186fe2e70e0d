"""spx_proxval_l1_b2: prox! of ShiftedNormL1B2 fused with the value of h at the result (csrc/spx_b2.hip, include/spx.h).

y must carry the bits of spx_prox_l1_b2 on q_scale * q on every form of k_b2_coop, whichever of its five store sites ends up
being the one whose stores stand; the value is lambda * sum |(xk + sj) + y| over that y -- the oracle's obj_plain("l1", ...) on
the host copy, to the project's psi bar (1e-12 relative: both sides add the same non-negative terms, only the order differs) --
and it is reproducible.

Two private contexts driven through the C ABI (A: the fused call, B: the plain prox!, through the same sequence of calls, so
that SpxSyncHeader::b2_last_scaled -- which selects the speculative paths -- is the same on both).  Tuning key 8 = 4 caps the
resident grid at four workgroups, what the key is documented for: the register form then ends at n = 32 768, the LDS form at
65 536, the streaming forms follow, the sample exists from 16 384, and from 8 tiles per workgroup (32 tiles of 6 144 elements:
n = 196 608) the plain prox! hands its tiles out on demand.  The mirror (shared context, native grid) serves the
device-target, capture and refusal cases."""
import ctypes
import functools

import numpy as np
import pytest

import redzone

pytestmark = pytest.mark.gpu

_D = ctypes.c_double
VALUE_TOL = 1e-12          # the bar of test_prox_value_fused
SPX_ERR_INVALID_ARG = 1
LAM = SIGMA = CHI = 1.0
ACTIVE, INACTIVE = 1.0, 1e6
# n under key 8 = 4: one lane / a pair / odd tail / register form (no sample) / register form with a sample-sized n / LDS form /
# streaming / streaming with on-demand tiles in the plain prox!.  (100 001, 0): the native grid.
SIZES = [(1, 4), (2, 4), (3, 4), (1_000, 4), (20_001, 4), (50_001, 4), (70_001, 4), (300_001, 4), (100_001, 0)]
FORM_SIZES = [20_001, 50_001, 70_001, 300_001]   # register, LDS, streaming, streaming with on-demand tiles (key 8 = 4)


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


@functools.lru_cache(maxsize=None)
def _data(n):
    """as _data of test_gpu_parity.py (seed = n); read-only"""
    rng = np.random.default_rng(n)
    x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    for v in (x, sj, q):
        v.setflags(write=False)
    return x, sj, q


_refs = {}


def _ref(orc, n, delta, c=1.0):
    """oracle prox at c * q, computed once per (n, delta, c); read-only"""
    key = (n, delta, c)
    if key not in _refs:
        x, sj, q = _data(n)
        r = orc.prox_l1_b2(c * q, x, sj, LAM, SIGMA, delta, CHI)
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def _dev(a, align8=False):
    """device copy; align8: the vector starts 8 bytes past a 16-byte boundary (the 8-byte forms)"""
    import torch
    t = torch.from_numpy(np.array(a))                    # (a writable copy: the shared data are read-only)
    buf = torch.empty(t.numel() + 2, dtype=t.dtype, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()] if align8 else buf[:t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == (8 if align8 else 0)
    return v


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


def _bits(v):
    return np.float64(v).view(np.uint64)


def _check_value(orc, val, yh, x, sj, what):
    ref = orc.obj_plain("l1", yh, x, sj, LAM)
    print("%s: value %.17g oracle %.17g rel %.3e" % (what, val, ref, abs(val - ref) / max(abs(ref), 1e-300)))
    assert np.isfinite(val) and abs(val - ref) <= VALUE_TOL * abs(ref), (what, val, ref)


def _check_y(orc, yh, n, delta, what, c=1.0):
    ref, x = _ref(orc, n, delta, c), _data(n)[0]
    err = float(np.max(np.abs(yh - ref)))
    bar = 1e-12 * max(np.linalg.norm(ref), np.linalg.norm(x))   # the bar of test_gpu_redzone.py::_b2
    print("%s: max |y - oracle| %.3e (bar %.3e)" % (what, err, bar))
    assert err <= bar, (what, err, bar)


@pytest.mark.parametrize("alias", [False, True], ids=["distinct", "y=q"])
@pytest.mark.parametrize("align8", [False, True], ids=["a16", "a8"])
@pytest.mark.parametrize("n,cap", SIZES, ids=["n%d-cap%d" % nc for nc in SIZES])
def test_sequence(env, orc, n, cap, align8, alias):
    """inactive, inactive, active, active, inactive, inactive on one context: a speculative store that stands, one that the final
    pass supersedes, non-speculative stores in both regimes.  Every call: (a) y has the bits of the plain prox! (context B, same
    sequence), (b) the value is the oracle's on that y, (c) y is within the existing bar of the oracle's prox; calls 2, 4 and 6:
    (d) a repeat made right after returns the same value bits (and the same y)."""
    import torch
    _, _, A, B = env
    x, sj, q = _data(n)
    xd, sd = _dev(x, align8), _dev(sj, align8)
    _cap(env, cap)
    try:
        for k, delta in enumerate([INACTIVE, INACTIVE, ACTIVE, ACTIVE, INACTIVE, INACTIVE]):
            what = "n %d cap %d align8 %d alias %d call %d delta %g" % (n, cap, align8, alias, k + 1, delta)
            for rep in range(2 if k % 2 == 1 else 1):
                qa, qb = _dev(q, align8), _dev(q, align8)
                ya = qa if alias else _dev(np.full(n, -777.0), align8)
                yb = qb if alias else _dev(np.full(n, -777.0), align8)
                ya, val = _proxval(env, A, ya, qa, xd, sd, n, delta)
                yb = _prox(env, B, yb, qb, xd, sd, n, delta)
                assert torch.equal(ya, yb), what                                     # (a)
                if rep == 1:
                    assert _bits(val) == _bits(val0) and torch.equal(ya, ya0), (what, val, val0)   # (d)
                    continue
                ya0, val0 = ya, val
                yh = ya.cpu().numpy()
                _check_value(orc, val, yh, x, sj, what)                              # (b)
                _check_y(orc, yh, n, delta, what)                                    # (c)
                if n >= 1_000:   # the regimes are what their names say: on the sphere / well inside the ball
                    nrm = float(np.linalg.norm(sj + yh))
                    assert (abs(nrm - delta) <= 1e-9 * delta) if delta == ACTIVE else (nrm < 1e-3 * delta), (what, nrm)
    finally:
        _cap(env, 0)


@pytest.mark.parametrize("alias", [False, True], ids=["distinct", "y=q"])
@pytest.mark.parametrize("delta", [ACTIVE, INACTIVE], ids=["active", "inactive"])
@pytest.mark.parametrize("n,align8", [(20_001, False), (50_001, False), (70_001, False), (70_001, True), (300_001, False)],
                         ids=["reg", "lds", "stream16", "stream8", "stream16-many-tiles"])
def test_q_scale(env, orc, n, align8, delta, alias):
    """q_scale = c gives the bits -- y and value -- of the call on c * q formed beforehand with q_scale = 1, and both are the plain
    prox! at c * q.  (Every call follows a call in the same regime: the same path on both.)"""
    import torch
    _, _, A, B = env
    c = -0.37
    x, sj, q = _data(n)
    xd, sd = _dev(x, align8), _dev(sj, align8)
    _cap(env, 4)
    try:
        def operands(scaled):
            qd = _dev(q, align8)
            if scaled:
                qd.mul_(c)                               # one rounded multiply per element
            return (qd if alias else _dev(np.full(n, -777.0), align8)), qd

        y0, q0 = operands(True)
        _proxval(env, A, y0, q0, xd, sd, n, delta)       # (sets the regime the two calls below follow)
        y1, q1 = operands(False)
        y1, v1 = _proxval(env, A, y1, q1, xd, sd, n, delta, q_scale=c)
        y2, q2 = operands(True)
        y2, v2 = _proxval(env, A, y2, q2, xd, sd, n, delta)
        y3, q3 = operands(True)
        y3 = _prox(env, B, y3, q3, xd, sd, n, delta)
        assert torch.equal(y1, y2) and _bits(v1) == _bits(v2), (n, align8, delta, alias, v1, v2)
        assert torch.equal(y1, y3)
        yh = y1.cpu().numpy()
        _check_value(orc, v1, yh, x, sj, "q_scale n %d" % n)
        _check_y(orc, yh, n, delta, "q_scale n %d" % n, c)
    finally:
        _cap(env, 0)


def _mirror_problem(s, n, delta=ACTIVE):
    import torch
    x, sj, q = _data(n)
    xd, sd, qd = (torch.from_numpy(v.copy()).to("cuda:0") for v in (x, sj, q))
    psi = s.shifted(s.shifted(s.NormL1(LAM), xd, delta, s.NormL2(CHI)), sd)
    assert type(psi).__name__ == "ShiftedNormL1B2"
    return psi, qd


def test_device_value_target(env, orc):
    """With a device value target the host value is NaN and the device double holds the bits of the host-valued call.  (That such a
    call does not synchronise is what test_graph_replay shows: a call that synchronises refuses to be captured.)"""
    import torch
    s = env[0]
    n = 20_001
    psi, qd = _mirror_problem(s, n)
    y0, v0 = s.prox_value_bang(torch.empty_like(qd), psi, qd, SIGMA, q_scale=-0.5)
    out = torch.full((1,), -3.0, dtype=torch.float64, device="cuda:0")
    for _ in range(2):
        with s.device_values(out):
            y, hv = s.prox_value_bang(torch.empty_like(qd), psi, qd, SIGMA, q_scale=-0.5)
        assert hv != hv, hv
        assert _bits(float(out.item())) == _bits(v0) and torch.equal(y, y0), (float(out.item()), v0)
        out.fill_(-3.0)
    y, v = s.prox_value(psi, qd, SIGMA, q_scale=-0.5)    # synchronous again, into psi.sol
    assert _bits(v) == _bits(v0) and torch.equal(y, y0)
    x, sj, _ = _data(n)
    _check_value(orc, v0, y0.cpu().numpy(), x, sj, "mirror n %d" % n)


def test_graph_replay(env):
    """One spx_proxval_l1_b2 at n = 20 001 captured with a device value target after one warm call; two replays give the eager y
    and value bit for bit.  (Default queue count; no graph environment variable is touched.)"""
    import torch
    s = env[0]
    n = 20_001
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        psi, qd = _mirror_problem(s, n)
        y = torch.zeros(n, dtype=torch.float64, device="cuda")
        val = torch.zeros(1, dtype=torch.float64, device="cuda")

        def iteration():
            with s.device_values(val):
                s.prox_value_bang(y, psi, qd, SIGMA, q_scale=-0.5)

        iteration()                                      # the warm call
        side.synchronize()
        y0, v0 = y.clone(), float(val.item())
        assert np.isfinite(v0) and v0 > 0.0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        iteration()
    for rep in range(2):
        y.fill_(-777.0)
        val.fill_(-1.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, y0) and _bits(float(val.item())) == _bits(v0), (rep, float(val.item()), v0)


def test_refusals(env):
    """value == NULL: SPX_ERR_INVALID_ARG, nothing launched; a host psi and the top-r operators keep their TypeError; n == 0: value
    0 on the host and in a device target."""
    import torch
    s, L, A, _ = env
    n = 1_000
    x, sj, q = _data(n)
    xd, sd, qd = _dev(x), _dev(sj), _dev(q)
    y = _dev(np.full(n, -9.0))
    torch.cuda.synchronize()
    rc = L.spx_proxval_l1_b2(A, _p(y), _p(qd), _p(xd), _p(sd), n, _D(LAM), _D(SIGMA), _D(ACTIVE), _D(CHI), _D(1.0), None)
    assert rc == SPX_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((y == -9.0).all())
    y, v = _proxval(env, A, y, qd, xd, sd, n, ACTIVE)    # and the context is fine
    assert np.isfinite(v) and v > 0.0
    with pytest.raises(TypeError):                       # host psi
        psi = s.shifted(s.shifted(s.NormL1(LAM), x.copy(), ACTIVE, s.NormL2(CHI)), sj.copy())
        s.prox_value(psi, q.copy(), SIGMA)
    with pytest.raises(TypeError):                       # top-r: h is 0 at any prox result
        s.prox_value(s.shifted(s.shifted(s.IndBallL0(3), xd), sd), qd, SIGMA)
    out = _D(-1.0)
    s._lib.check(L.spx_proxval_l1_b2(A, None, None, None, None, 0, _D(LAM), _D(SIGMA), _D(ACTIVE), _D(CHI), _D(1.0), ctypes.byref(out)))
    assert out.value == 0.0
    target = torch.full((1,), -3.0, dtype=torch.float64, device="cuda:0")
    s._lib.check(L.spx_ctx_set_value_target(A, _p(target)))
    try:
        s._lib.check(L.spx_proxval_l1_b2(A, None, None, None, None, 0, _D(LAM), _D(SIGMA), _D(ACTIVE), _D(CHI), _D(1.0), ctypes.byref(out)))
    finally:
        s._lib.check(L.spx_ctx_set_value_target(A, None))
    assert float(target.item()) == 0.0


@pytest.mark.parametrize("mode", ["A", "C"])
@pytest.mark.parametrize("n", FORM_SIZES, ids=["reg", "lds", "stream", "stream-many-tiles"])
def test_guard_bands(env, orc, n, mode):
    """No byte outside y written, no element of y left unwritten, no input modified, no read past the end of an input (the poison
    would move y and the value away from the oracle's).  A: every vector 16-byte aligned; C: the inputs at +8 B (the 8-byte
    streaming form beyond the LDS form's range)."""
    import torch
    s, L, A, _ = env
    x, sj, q = _data(n)
    ay, ai = redzone.F64_MODES[mode]
    zone = redzone.Zone()
    yb = zone.add(n, torch.float64, ay, role="out", name="y")
    qb, xb, sb = (zone.add(n, torch.float64, ai, data=np.array(v), name=nm) for v, nm in ((q, "q"), (x, "xk"), (sj, "sj")))
    out = _D(-1.0)
    _cap(env, 4)
    try:
        torch.cuda.synchronize()
        s._lib.check(L.spx_proxval_l1_b2(A, ctypes.c_void_p(yb.ptr()), ctypes.c_void_p(qb.ptr()), ctypes.c_void_p(xb.ptr()),
                                         ctypes.c_void_p(sb.ptr()), n, _D(LAM), _D(SIGMA), _D(ACTIVE), _D(CHI), _D(1.0), ctypes.byref(out)))
        torch.cuda.synchronize()
    finally:
        _cap(env, 0)
    got = yb.t.cpu().numpy()
    _check_y(orc, got, n, ACTIVE, "guarded n %d mode %s" % (n, mode))
    _check_value(orc, out.value, got, x, sj, "guarded n %d mode %s" % (n, mode))
    zone.check()


@pytest.mark.soak
def test_soak_native_grid(env, orc):
    """n = 16 000 000 on the native grid (the plain prox! hands its tiles out on demand there): (a), (b), (d) of test_sequence."""
    import torch
    _, _, A, B = env
    n = 16_000_000
    x, sj, q = _data(n)
    xd, sd, qd = _dev(x), _dev(sj), _dev(q)
    for k, delta in enumerate([INACTIVE, INACTIVE, ACTIVE, ACTIVE, INACTIVE, INACTIVE]):
        ya, val = _proxval(env, A, torch.empty_like(qd), qd, xd, sd, n, delta)
        yb = _prox(env, B, torch.empty_like(qd), qd, xd, sd, n, delta)
        assert torch.equal(ya, yb), (k, delta)
        _check_value(orc, val, ya.cpu().numpy(), x, sj, "soak call %d" % (k + 1))
        if k % 2 == 1:
            y2, v2 = _proxval(env, A, torch.empty_like(qd), qd, xd, sd, n, delta)
            _prox(env, B, torch.empty_like(qd), qd, xd, sd, n, delta)
            assert _bits(v2) == _bits(val) and torch.equal(y2, ya), (k, val, v2)
