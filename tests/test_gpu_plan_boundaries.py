"""Either side of the sizes at which the top-r select and ShiftedNormL1B2 change their kernel form (csrc/spx_plan.hpp: sel_plan,
b2_plan), on a private context whose resident grid is capped at two workgroups (tuning key 8 = 2), so that every boundary sits
at a small n:

  top-r Float64   v in registers up to 16 384, v in LDS up to 32 768, LDS + register slots up to 49 152 (16-byte aligned
                  vectors only), v parked in y beyond
  top-r Float32   v in registers up to 16 384, v in LDS up to 65 536, v parked in y beyond
  B2              register form up to 16 384, xk in LDS up to 32 768, the streaming forms (16-byte / 8-byte accesses) beyond

with all vectors 16-byte aligned and with all of them 8 bytes off.  Top-r: y bit for bit against the oracle, on data whose keys
do not tie, as tests/test_gpu_parity.py compares it.  B2: the bars of test_b2_one_launch_forms_at_their_boundaries
(tests/test_gpu_stress.py), and for spx_proxval_l1_b2 the value against the oracle's h at the returned y to the 1e-12 of
tests/test_gpu_proxval_b2.py."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_D = ctypes.c_double
_F = ctypes.c_float
CAP = 2
DELTA = 0.75   # (exact in Float32 too)


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    s = ge.build()
    from oracle import oracle
    L = s._lib.load()
    c = ctypes.c_void_p()
    s._lib.check(L.spx_ctx_create_on_stream(0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(c)))
    try:
        s._lib.check(L.spx_ctx_set_tuning(c, 8, CAP))
        yield s, L, c, oracle
    finally:
        torch.cuda.synchronize()
        L.spx_ctx_set_tuning(c, 8, 0)
        L.spx_ctx_destroy(c)


@functools.lru_cache(maxsize=None)
def _data(n, dtype):
    """x, sj, q of `dtype` whose keys |(x + sj) + q| are pairwise different; read-only"""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(5000 + n)
    x = rng.normal(size=n).astype(dt)
    sj = rng.uniform(-0.5, 0.5, size=n).astype(dt)
    q = rng.normal(size=n).astype(dt)
    for _ in range(100):
        key = np.abs(((x + sj).astype(dt) + q).astype(dt))
        _, first, count = np.unique(key, return_index=True, return_counts=True)
        if (count == 1).all():
            break
        again = np.setdiff1d(np.arange(n), first)
        q[again] = rng.normal(size=again.size).astype(dt)
    else:
        raise AssertionError("keys still tie")
    for v in (x, sj, q):
        v.setflags(write=False)
    return x, sj, q


def _dev(a, off8):
    """device copy; off8: the vector starts 8 bytes past a 16-byte boundary"""
    import torch
    t = torch.from_numpy(np.array(a))
    pad = 8 // t.element_size()
    buf = torch.empty(t.numel() + 2 * pad, dtype=t.dtype, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    v = buf[pad:pad + t.numel()] if off8 else buf[:t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == (8 if off8 else 0)
    return v


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("off8", [False, True], ids=["aligned", "off8"])
@pytest.mark.parametrize("n", [16384, 16385, 32768, 32769, 49152, 49153])
def test_topr_f64_forms_at_their_boundaries(env, n, off8):
    import torch
    s, L, c, orc = env
    x, sj, q = _data(n, "float64")
    xd, sd, qd = (_dev(v, off8) for v in (x, sj, q))
    top = orc.TopR(q, x, sj)
    for r in (1, n // 100, n // 2):
        y = _dev(np.full(n, -777.25), off8)
        s._lib.check(L.spx_prox_indball_l0(c, _p(y), _p(qd), _p(xd), _p(sd), n, r))
        assert np.array_equal(y.cpu().numpy().view(np.uint64), top.prox(r).view(np.uint64)), (n, r, off8)
        y = _dev(np.full(n, -777.25), off8)
        s._lib.check(L.spx_prox_indball_l0_binf(c, _p(y), _p(qd), _p(xd), _p(sd), n, r, _D(DELTA)))
        assert np.array_equal(y.cpu().numpy().view(np.uint64), top.prox(r, DELTA).view(np.uint64)), (n, r, off8, "binf")
    torch.cuda.synchronize()


@pytest.mark.parametrize("off8", [False, True], ids=["aligned", "off8"])
@pytest.mark.parametrize("n", [16384, 16385, 65536, 65537])
def test_topr_f32_forms_at_their_boundaries(env, n, off8):
    import torch
    s, L, c, orc = env
    x, sj, q = _data(n, "float32")
    xd, sd, qd = (_dev(v, off8) for v in (x, sj, q))
    order = orc.topr_order_f32(q, x, sj)
    for r in (1, n // 100, n // 2):
        y = _dev(np.full(n, -777.25, dtype=np.float32), off8)
        s._lib.check(L.spx_prox_indball_l0_f32(c, _p(y), _p(qd), _p(xd), _p(sd), n, r))
        ref = orc.prox_indball_l0_f32(q, x, sj, r, _order=order)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), ref.view(np.uint32)), (n, r, off8)
        y = _dev(np.full(n, -777.25, dtype=np.float32), off8)
        s._lib.check(L.spx_prox_indball_l0_binf_f32(c, _p(y), _p(qd), _p(xd), _p(sd), n, r, _F(DELTA)))
        ref = orc.prox_indball_l0_f32(q, x, sj, r, np.float32(DELTA), _order=order)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), ref.view(np.uint32)), (n, r, off8, "binf")
    torch.cuda.synchronize()


@pytest.mark.parametrize("off8", [False, True], ids=["aligned", "off8"])
@pytest.mark.parametrize("n", [16384, 16385, 32768, 32769])
def test_b2_forms_at_their_boundaries(env, n, off8):
    import torch
    s, L, c, orc = env
    x, sj, q = _data(n, "float64")
    xd, sd, qd = (_dev(v, off8) for v in (x, sj, q))
    nrm = float(np.linalg.norm(x))
    for lam, sigma, delta in ((1.0, 1.0, 1.0), (1.0, 1.0, 1e9), (1.0, 1.0, 1e9), (0.3, 0.7, 0.5 * nrm + 1e-3), (2.0, 1.0, 1e-3)):
        ref = orc.prox_l1_b2(q, x, sj, lam, sigma, delta, 1.0)
        scale = max(np.linalg.norm(ref), nrm, 1e-300)
        y = _dev(np.full(n, -777.25), off8)
        s._lib.check(L.spx_prox_l1_b2(c, _p(y), _p(qd), _p(xd), _p(sd), n, _D(lam), _D(sigma), _D(delta), _D(1.0)))
        assert np.max(np.abs(y.cpu().numpy() - ref)) <= 1e-12 * scale, (n, lam, sigma, delta)
        y = _dev(np.full(n, -777.25), off8)
        out = _D(-1.0)
        s._lib.check(L.spx_proxval_l1_b2(c, _p(y), _p(qd), _p(xd), _p(sd), n, _D(lam), _D(sigma), _D(delta), _D(1.0), _D(1.0),
                                         ctypes.byref(out)))
        yh = y.cpu().numpy()
        assert np.max(np.abs(yh - ref)) <= 1e-12 * scale, (n, lam, sigma, delta, "proxval")
        want = orc.obj_plain("l1", yh, x, sj, lam)
        assert np.isfinite(out.value) and abs(out.value - want) <= 1e-12 * abs(want), (n, lam, sigma, delta, out.value, want)
        qa = _dev(q, off8)
        s._lib.check(L.spx_prox_l1_b2(c, _p(qa), _p(qa), _p(xd), _p(sd), n, _D(lam), _D(sigma), _D(delta), _D(1.0)))
        assert np.max(np.abs(qa.cpu().numpy() - ref)) <= 1e-12 * scale, (n, lam, sigma, delta, "aliased")
    torch.cuda.synchronize()
