"""GPU: where the scalars of a call go -- the host doubles, the caller's device doubles, the context's value target.

The plumbing only (the arithmetic is held to the oracle by the parity files): every expected value is the host form of the same
call on the same inputs and the same grid, so every comparison is bit for bit.

  1. a step call (spx_proxstep_*, spx_iproxstep_*) neither uses nor disturbs the context's value target, on every route;
  2. the host result, the device result and, for the step calls, both at once agree for every value- and step-returning entry
     point, at n = 0, n = 1 and a size of several workgroups, with tuning key 17 at 1 and at 0;
  3. the step entry points refuse bad result pointers and aliased vectors before anything is enqueued.

The rule of 2. at n == 0 with a value target ("the device target zeroed", include/spx.h) is where the entry points used to
differ: the six separable spx_proxval_* and the spx_obj_group_* family returned 0 on the host and left the target unwritten
(16 cases of test_host_and_device_results_agree failed on that, and so did the device half of
test_separable_proxval_of_the_empty_vector_is_lambda_times_zero; nothing else in this file did, before the empty call was
stated once as spx_dest_empty)."""
import ctypes
import math
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAM, SIGMA, DELTA, CHI = 0.7, 1.1, 0.8, 1.0
LS, US = -0.9, 0.9
SENTINEL = -7.25
POISON = -777.25
INVALID_ARG = 1


@pytest.fixture(scope="module")
def s():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.build()


def _new_ctx(s):
    L = s._lib.load()
    c = ctypes.c_void_p()
    s._lib.check(L.spx_ctx_create(0, ctypes.byref(c)))
    return c


@pytest.fixture(scope="module")
def ctxs(s):
    """two private contexts: [0] gets a value target where a test says so, [1] never has one"""
    L = s._lib.load()
    pair = [_new_ctx(s), _new_ctx(s)]
    yield pair
    for c in pair:
        L.spx_ctx_set_value_target(c, None)
        L.spx_sync(c)
        L.spx_ctx_destroy(c)


def _hex(values):
    return [struct.pack("<d", float(v)).hex() for v in values]


class _Data:
    """device vectors of one size, drawn once; y and xkn are refilled before every call.  y_off: y starts 8 bytes off."""

    def __init__(self, n, offsets=None, gsize=0, ngroups=0, y_off=False):
        import torch
        self.n, self.gsize, self.ngroups = n, gsize, ngroups
        m = max(n, 1)
        rng = np.random.default_rng(52000 + n + 7 * gsize)
        up = lambda a: torch.tensor(np.ascontiguousarray(a)).to("cuda:0")
        self.x, self.sj, self.q = up(rng.normal(size=m)), up(rng.uniform(-0.5, 0.5, size=m)), up(rng.normal(size=m))
        self.d = up(rng.uniform(0.5, 2.0, size=m))
        self.lam = up(rng.uniform(0.3, 1.5, size=max(ngroups, 1)))
        self.off = up(np.asarray(offsets, dtype=np.int64)) if offsets is not None else None
        self.index = up(np.arange(m, dtype=np.int64))      # gather rows: the groups of the uniform layout as index sets
        self.ptr = up(np.arange(0, max(ngroups, 0) + 1, dtype=np.int64) * gsize)
        self.ybuf = torch.empty(m + 2, dtype=torch.float64, device="cuda:0")
        self.y = self.ybuf[1:m + 1] if y_off else self.ybuf[:m]
        self.xkn = torch.empty(m, dtype=torch.float64, device="cuda:0")
        self.sdev = torch.empty(4, dtype=torch.float64, device="cuda:0")

    def refill(self):
        import torch
        self.ybuf.fill_(POISON)
        self.xkn.fill_(POISON)
        self.sdev.fill_(SENTINEL)
        torch.cuda.synchronize()

    def p(self, name):
        t = getattr(self, name)
        return None if t is None else t.data_ptr()


# ------------------------------------------------------------------ the entry points
# name -> (family, doubles returned, arguments between `n` and the results)
BOX = (None, None, LS, US, None)


def _group(D, *tail):
    return (D.p("off"), D.gsize, D.ngroups, D.p("lam") if D.ngroups else None) + tail


ROWS = {
    "proxval_l1": ("val", 1, lambda D: (LAM, SIGMA, 1.0)),
    "proxval_l0": ("val", 1, lambda D: (LAM, SIGMA, 1.0)),
    "proxval_lhalf": ("val", 1, lambda D: (LAM, SIGMA, 1.0)),
    "proxval_l1_box": ("val", 1, lambda D: (LAM, SIGMA) + BOX + (1.0,)),
    "proxval_l0_box": ("val", 1, lambda D: (LAM, SIGMA) + BOX + (1.0,)),
    "proxval_lhalf_box": ("val", 1, lambda D: (LAM, SIGMA) + BOX + (1.0,)),
    "proxval_group_l2": ("val", 1, lambda D: _group(D, SIGMA, 1.0)),
    "proxval_group_l2_binf": ("val", 1, lambda D: _group(D, SIGMA, DELTA, 1.0)),
    "proxval_l1_b2": ("val", 1, lambda D: (LAM, SIGMA, DELTA, CHI, 1.0)),
    "proxstep_l1": ("step", 3, lambda D: (LAM, SIGMA, 1.0)),
    "proxstep_l0": ("step", 3, lambda D: (LAM, SIGMA, 1.0)),
    "proxstep_lhalf": ("step", 3, lambda D: (LAM, SIGMA, 1.0)),
    "proxstep_l1_box": ("step", 3, lambda D: (LAM, SIGMA) + BOX + (1.0,)),
    "proxstep_l0_box": ("step", 3, lambda D: (LAM, SIGMA) + BOX + (1.0,)),
    "proxstep_lhalf_box": ("step", 3, lambda D: (LAM, SIGMA) + BOX + (1.0,)),
    "proxstep_group_l2": ("step", 3, lambda D: _group(D, SIGMA, 1.0)),
    "proxstep_group_l2_binf": ("step", 3, lambda D: _group(D, SIGMA, DELTA, 1.0)),
    "proxstep_l1_b2": ("step", 3, lambda D: (LAM, SIGMA, DELTA, CHI, 1.0)),
    "iproxstep_l1": ("istep", 4, lambda D: (LAM, 0)),
    "iproxstep_l0": ("istep", 4, lambda D: (LAM, 0)),
    "iproxstep_l1_box": ("istep", 4, lambda D: (LAM,) + BOX),
    "iproxstep_l0_box": ("istep", 4, lambda D: (LAM,) + BOX),
    "obj_l1": ("obj", 1, lambda D: (LAM,)),
    "obj_l1_box": ("obj", 1, lambda D: (LAM,) + BOX),
    "obj_indball_l0_binf": ("obj", 1, lambda D: (D.n, 10.0)),
    "obj_group_l2_binf": ("obj", 1, lambda D: _group(D, 10.0)),
    "obj_group_l2_gather": ("obj", 1, lambda D: (D.p("ptr"), D.p("index"), D.ngroups, D.n, D.p("lam") if D.ngroups else None)),
    "obj_l1_b2": ("obj", 1, lambda D: (LAM, 10.0)),
}
GROUP_ROWS = [k for k in ROWS if "group" in k]


def _call(L, ctx, name, D, host=True, dev=False, xkn=True):
    """One call.  Value rows: `dev` is not an argument of theirs (the context's value target decides); -> [the host double].
    Step rows: -> the host statistics, or None without a host result."""
    fam, count, mid = ROWS[name]
    fn = getattr(L, "spx_" + name)
    vec = (D.p("y"), D.p("q")) + ((D.p("d"),) if fam == "istep" else ()) + (D.p("x"), D.p("sj"))
    if fam == "obj":
        vec = (D.p("q"), D.p("x"), D.p("sj"))          # psi at y := q
    if fam in ("val", "obj"):
        out = ctypes.c_double(POISON)
        rc = fn(ctx, *vec, D.n, *mid(D), ctypes.byref(out))
        res = [out.value]
    else:
        st = (ctypes.c_double * count)(*([POISON] * count)) if host else None
        rc = fn(ctx, *vec, D.n, *mid(D), D.p("xkn") if xkn else None, st, D.p("sdev") if dev else None)
        res = list(st) if host else None
    assert rc == 0 and L.spx_sync(ctx) == 0, (name, D.n, rc, L.spx_last_error())
    return res


# ------------------------------------------------------------------ 1. step calls and the value target
def _uniform(n, gs):
    return dict(n=n, gsize=gs, ngroups=n // gs)


RAGGED = [0, 3, 10, 64]
STEP_CASES = {
    "proxstep_l1": ("proxstep_l1", dict(n=1000), {}),
    "iproxstep_l1": ("iproxstep_l1", dict(n=1000), {}),
    "b2-fused": ("proxstep_l1_b2", dict(n=1000), {18: 0}),
    "b2-composed": ("proxstep_l1_b2", dict(n=1000), {18: 1}),
    "b2-composed-8byte": ("proxstep_l1_b2", dict(n=1001, y_off=True), {18: 1}),
}
for _sfx in ("", "_binf"):
    STEP_CASES["group%s-fused" % _sfx] = ("proxstep_group_l2" + _sfx, _uniform(64, 8), {})
    STEP_CASES["group%s-lds" % _sfx] = ("proxstep_group_l2" + _sfx, _uniform(1200, 600), {})
    STEP_CASES["group%s-general" % _sfx] = ("proxstep_group_l2" + _sfx, _uniform(20000, 20000), {})
    STEP_CASES["group%s-ragged-bound" % _sfx] = ("proxstep_group_l2" + _sfx, dict(n=64, offsets=RAGGED, gsize=54, ngroups=3), {})
    STEP_CASES["group%s-ragged" % _sfx] = ("proxstep_group_l2" + _sfx, dict(n=64, offsets=RAGGED, gsize=0, ngroups=3), {})


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_step_call_leaves_the_value_target_alone(s, ctxs, case):
    import torch
    L = s._lib.load()
    name, shape, keys = STEP_CASES[case]
    count = ROWS[name][1]
    with_target, without = ctxs
    D = _Data(**shape)
    target = torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    try:
        for c in ctxs:
            for k, v in keys.items():
                assert L.spx_ctx_set_tuning(c, k, v) == 0
        assert L.spx_ctx_set_value_target(with_target, target.data_ptr()) == 0
        for host in (True, False):
            got = {}
            for c in (with_target, without):
                D.refill()
                st = _call(L, c, name, D, host=host, dev=not host)
                got[c.value] = (_hex(st) if host else _hex(D.sdev.cpu().numpy()[:count]), _hex(D.y.cpu().numpy()), _hex(D.xkn.cpu().numpy()))
            print(case, "host" if host else "dev", got[with_target.value][0])
            assert _hex(target.cpu().numpy()) == _hex([SENTINEL]), (case, host, "the step call wrote the value target")
            assert got[with_target.value] == got[without.value], (case, host)
            # the target is still set: a value call stores into it and returns NaN on the host
            V = _Data(n=1000)
            V.refill()
            here = _call(L, with_target, "proxval_l1", V)
            assert math.isnan(here[0]), (case, here)
            V.refill()
            there = _call(L, without, "proxval_l1", V)
            assert _hex(target.cpu().numpy()) == _hex(there), (case, "the value call after the step call")
            target.fill_(SENTINEL)
            torch.cuda.synchronize()
    finally:
        L.spx_ctx_set_value_target(with_target, None)
        for c in ctxs:
            L.spx_ctx_set_tuning(c, 18, 0)


# ------------------------------------------------------------------ 2. host and device destinations agree
def _sizes(name):
    return (0, 8, 1200) if name in GROUP_ROWS else (0, 1, 1003)


@pytest.mark.parametrize("key17", [1, 0])
@pytest.mark.parametrize("name", list(ROWS))
def test_host_and_device_results_agree(s, ctxs, name, key17):
    import torch
    L = s._lib.load()
    ctx = ctxs[0]
    fam, count, _ = ROWS[name]
    target = torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda:0")
    try:
        assert L.spx_ctx_set_tuning(ctx, 17, key17) == 0
        for n in _sizes(name):
            D = _Data(n=n, gsize=8, ngroups=n // 8) if name in GROUP_ROWS else _Data(n=n)
            D.refill()
            ref = _call(L, ctx, name, D)            # the host form
            y_ref = _hex(D.y.cpu().numpy())
            print(name, key17, n, ref)
            if n == 0:
                assert _hex(ref) == _hex([0.0] * count), (name, n, ref)
            if fam in ("val", "obj"):
                target.fill_(SENTINEL)
                assert L.spx_ctx_set_value_target(ctx, target.data_ptr()) == 0
                D.refill()
                host = _call(L, ctx, name, D)
                assert L.spx_ctx_set_value_target(ctx, None) == 0
                assert _hex(target.cpu().numpy()) == _hex(ref), (name, n, "device value")
                assert _hex(host) == _hex([0.0]) if n == 0 else math.isnan(host[0]), (name, n, host)
            else:
                for host in (False, True):       # device only, then both at once
                    D.refill()
                    st = _call(L, ctx, name, D, host=host, dev=True)
                    sdev = D.sdev.cpu().numpy()
                    assert _hex(sdev[:count]) == _hex(ref), (name, n, host, "device statistics")
                    assert _hex(sdev[count:]) == _hex([SENTINEL] * (4 - count)), (name, n, host, "written past the statistics")
                    if host:
                        assert _hex(st) == _hex(ref), (name, n, "host statistics next to the device ones")
            if fam != "obj":
                assert _hex(D.y.cpu().numpy()) == y_ref, (name, n, "y")
    finally:
        L.spx_ctx_set_value_target(ctx, None)
        L.spx_ctx_set_tuning(ctx, 17, 1)


@pytest.mark.parametrize("lam", [-0.7, float("inf"), float("-inf"), float("nan")], ids=["negative", "inf", "-inf", "nan"])
@pytest.mark.parametrize("name", [k for k in ROWS if k.startswith("proxval_l") and k != "proxval_l1_b2"])
def test_separable_proxval_of_the_empty_vector_is_lambda_times_zero(s, ctxs, name, lam):
    """n == 0: the host double of the separable spx_proxval_* is lambda * 0.0 -- -0.0 for a negative lambda, NaN for a
    non-finite one -- with and without a value target (the bits the entry points have returned since lambda * sum was
    replaced there); with a target the device double is +0.0."""
    import torch
    L = s._lib.load()
    ctx = ctxs[0]
    fam, count, mid = ROWS[name]
    D = _Data(n=0)
    expected = _hex([lam * 0.0])
    target = torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda:0")
    try:
        for with_target in (False, True):
            assert L.spx_ctx_set_value_target(ctx, target.data_ptr() if with_target else None) == 0
            D.refill()
            out = ctypes.c_double(POISON)
            rc = getattr(L, "spx_" + name)(ctx, D.p("y"), D.p("q"), D.p("x"), D.p("sj"), 0, lam, *mid(D)[1:], ctypes.byref(out))
            assert rc == 0 and L.spx_sync(ctx) == 0, (name, lam, rc, L.spx_last_error())
            print(name, lam, with_target, _hex([out.value]), expected)
            assert _hex([out.value]) == expected, (name, lam, with_target)
            assert _hex(target.cpu().numpy()) == _hex([0.0 if with_target else SENTINEL]), (name, lam, with_target)
    finally:
        L.spx_ctx_set_value_target(ctx, None)


# ------------------------------------------------------------------ 3. refusals of the step entry points
REFUSAL_ROWS = ["proxstep_l1_box", "iproxstep_l1", "proxstep_group_l2", "proxstep_l1_b2"]


def _refusal_call(L, ctx, name, D, ptrs, st, sdev, check_d=0):
    fam, count, mid = ROWS[name]
    fn = getattr(L, "spx_" + name)
    if name == "proxstep_l1_box":
        middle = (LAM, SIGMA, ptrs["lo"], ptrs["up"], LS, US, ptrs["mask"], 1.0)
    elif name == "iproxstep_l1":
        middle = (LAM, check_d)
    else:
        middle = mid(D)
    vec = (ptrs["y"], ptrs["q"]) + ((ptrs["d"],) if fam == "istep" else ()) + (ptrs["x"], ptrs["sj"])
    return fn(ctx, *vec, D.n, *middle, ptrs["xkn"], st, sdev)


@pytest.mark.parametrize("name", REFUSAL_ROWS)
def test_step_refusals_enqueue_nothing(s, ctxs, name):
    import torch
    L = s._lib.load()
    ctx = ctxs[1]
    fam, count, _ = ROWS[name]
    D = _Data(n=64, gsize=8, ngroups=8) if "group" in name else _Data(n=64)
    lo = torch.full((64,), -1.0, dtype=torch.float64, device="cuda:0")
    up = torch.full((64,), 1.0, dtype=torch.float64, device="cuda:0")
    mask = torch.ones(64, dtype=torch.uint8, device="cuda:0")
    base = {k: D.p(k) for k in ("y", "q", "d", "x", "sj", "xkn")}
    base.update(lo=lo.data_ptr(), up=up.data_ptr(), mask=mask.data_ptr())
    inputs = ["q", "x", "sj"] + (["d"] if fam == "istep" else []) + (["lo", "up", "mask"] if name == "proxstep_l1_box" else [])
    cases = [("both NULL", {}, False, False, 0, "both NULL")]
    cases += [("y == %s" % k, {"y": base[k]}, True, True, 0, "aliases") for k in (["q", "d"] if fam == "istep" else ["q"])]
    cases += [("xkn == %s" % k, {"xkn": base[k]}, True, True, 0, "xkn is one of") for k in ["y"] + inputs]
    if name == "iproxstep_l1":
        cases.append(("check_d without stats", {}, False, True, 1, "check_d needs"))
    for what, change, host, dev, check_d, words in cases:
        D.refill()
        st = (ctypes.c_double * count)(*([POISON] * count)) if host else None
        rc = _refusal_call(L, ctx, name, D, dict(base, **change), st, D.p("sdev") if dev else None, check_d)
        msg = (L.spx_last_error() or b"").decode()
        print(name, what, rc, msg)
        assert rc == INVALID_ARG, (name, what, rc, msg)
        assert msg and words in msg, (name, what, msg)
        assert L.spx_sync(ctx) == 0
        assert _hex(D.ybuf.cpu().numpy()) == _hex([POISON] * len(D.ybuf)), (name, what, "y was written")
        assert _hex(D.sdev.cpu().numpy()) == _hex([SENTINEL] * 4), (name, what, "stats_dev was written")
        assert _hex(D.xkn.cpu().numpy()) == _hex([POISON] * len(D.xkn)), (name, what, "xkn was written")
    # the same arguments without the fault run
    D.refill()
    st = (ctypes.c_double * count)()
    assert _refusal_call(L, ctx, name, D, base, st, D.p("sdev")) == 0 and L.spx_sync(ctx) == 0, L.spx_last_error()
    assert _hex(D.sdev.cpu().numpy()[:count]) == _hex(st)
