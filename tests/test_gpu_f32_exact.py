"""The eleven Float32 entry points that had no oracle -- the ten spx_obj_*_f32 and spx_prox_group_l2_f32 -- against the exact
restatement (oracle/spx_oracle_f32.c through tests/f32_exact.py, which states the inputs, the bars and why they are what they are):

  * psi(y): nonfinite.check_sum at 1e-12 of sum |term| times (double)lambda; counts and the 0 / +Inf decisions exact;
  * the group prox: bit for bit, but for the groups the census finds on a Float32 rounding boundary of their norm.

Through the C ABI with ctypes on one private context, on guarded buffers (tests/redzone.py: guards intact, inputs unchanged, no
output element unwritten).  Every psi(y) case runs with tuning key 17 at 1 and at 0, into the host double and into a device
value target, and must give the same bits four times.  Each case prints a line `F32EXACT <entry point> ...` with the relative
deviation from the exact sum, or the ambiguous groups met."""
import ctypes
import itertools

import numpy as np
import pytest

import f32_exact as fx
import redzone

pytestmark = pytest.mark.gpu

_D, _F = ctypes.c_double, ctypes.c_float
F32 = np.float32
ALIGNS = (0, 4, 8, 12)


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    s = ge.build()
    L = s._lib.load()
    ctx = ctypes.c_void_p()
    s._lib.check(L.spx_ctx_create_on_stream(0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(ctx)))
    try:
        yield s, L, ctx
    finally:
        torch.cuda.synchronize()
        s._lib.check(L.spx_ctx_set_tuning(ctx, 17, 1))
        L.spx_ctx_destroy(ctx)


class Bufs:
    """the guarded buffers of one set of vectors, and the four ways to ask for a value"""

    def __init__(self, env):
        import torch
        self.torch = torch
        self.s, self.L, self.ctx = env
        self.zone = redzone.Zone()
        self.value = self.zone.add(1, torch.float64, 0, data=np.zeros(1), role="inout", name="value")
        self.b = {}

    def add(self, name, data, align, role="in"):
        t = self.torch
        dt = {np.dtype(np.float32): t.float32, np.dtype(np.uint8): t.uint8, np.dtype(np.int64): t.int64}[np.asarray(data).dtype]
        kw = {"poison": max(len(data) // 3, 0)} if dt == t.int64 else {}
        self.b[name] = self.zone.add(len(data), dt, align, data=np.ascontiguousarray(data), role=role, name=name, **kw)
        return self.b[name]

    def ptr(self, name):
        return self.b[name].ptr() if name in self.b else None

    def poke(self, name, p, v):
        """one element of an input rewritten, in the buffer and in the snapshot its check compares with"""
        self.b[name].set_input(p, float(v))

    def value_of(self, name, args, key17, target, rc_want=0):
        """one call: (the value, rc).  target "device": the value comes from the context's value target, the host double is NaN"""
        t = self.torch
        chk = self.s._lib.check
        chk(self.L.spx_ctx_set_tuning(self.ctx, 17, key17))
        if target == "device":
            self.value.t.fill_(-1.0)
            chk(self.L.spx_ctx_set_value_target(self.ctx, ctypes.c_void_p(self.value.ptr())))
        val = _D(-2.0)
        t.cuda.synchronize()
        try:
            rc = getattr(self.L, name)(self.ctx, *args, ctypes.byref(val))
            t.cuda.synchronize()
        finally:
            chk(self.L.spx_ctx_set_value_target(self.ctx, None))
            chk(self.L.spx_ctx_set_tuning(self.ctx, 17, 1))
        if rc_want == 0:
            chk(rc)
        if target == "device":
            assert rc != 0 or np.isnan(val.value), (name, val.value)
            return float(self.value.t.cpu()[0]), rc
        return val.value, rc

    def four(self, name, args, what):
        """key 17 at 1 and 0, host double and device target: the same bits four times; returns the value"""
        vals = [self.value_of(name, args, k, tg)[0] for k, tg in itertools.product((1, 0), ("host", "device"))]
        bits = {np.float64(v).view(np.int64).item() for v in vals}
        assert len(bits) == 1, (what, vals)
        return vals[0]


@pytest.fixture(scope="module")
def shared(env):
    """the guarded buffers of the latest (size, family) or layout: the entry points of a family run on the same vectors.  Any
    test order gives the same results; the parametrisations below keep the cases of one key together, so each is built once."""
    state = {}
    yield state
    state.clear()            # (before env destroys the context)


def _state(shared, key, make):
    if key not in shared:
        shared.clear()
        shared[key] = make()
    return shared[key]


def _report(entry, what, dev):
    print("F32EXACT spx_obj_%s_f32 %s relative deviation %.3e" % (entry, what, dev))


# ====================================================================================================== a. separable psi(y)
def _sep_bufs(env, n, family, flavour="plain"):
    d = fx.sep_data(n, family, flavour)
    b = Bufs(env)
    k = fx.SEP_SIZES.index(n) if n in fx.SEP_SIZES else 0
    names = ["y", "x", "sj"] + (["l", "u"] if family == "box" and np.ndim(d["l"]) else [])
    for j, nm in enumerate(names):                       # y, xk, sj, l, u at 0, 4, 8 or 12 bytes past a 256-byte boundary, mixed
        b.add(nm, d[nm], ALIGNS[(k + 3 * j + 1) % 4])
    if family == "box":
        b.add("mask", d["mask"], 1)                      # the mask at an odd address
    return d, b


def _sep_args(entry, d, b, n, variant, r):
    fam = fx.family_of(entry)
    head = (b.ptr("y"), b.ptr("x"), b.ptr("sj"), n)
    if fam == "box":
        l, u, m = fx.box_args(d, variant)
        return head + (_F(float(fx.LAM)), b.ptr("l") if np.ndim(l) else None, b.ptr("u") if np.ndim(u) else None,
                       _F(0.0 if np.ndim(l) else float(l)), _F(0.0 if np.ndim(u) else float(u)), b.ptr("mask") if m is not None else None)
    if entry == "indball_l0":
        return head + (r,)
    if entry == "indball_l0_binf":
        return head + (r, _F(float(fx.DELTA)))
    return head + (_F(float(fx.LAM)),)


def _sep_run(env, orc, d, b, entry, n, variants, pokes):
    name = "spx_obj_%s_f32" % entry
    worst = 0.0
    for variant in variants:
        terms, bad = fx.sep_terms(orc, entry, d, variant)
        assert not bad, (entry, n, variant)
        nnz = int(terms.sum()) if entry.startswith("indball") else None
        for r in ((max(nnz - 1, 0), nnz, n) if nnz is not None else (None,)):
            what = "%s n=%d %s r=%s" % (entry, n, variant, r)
            got = b.four(name, _sep_args(entry, d, b, n, variant, r), what)
            worst = max(worst, fx.check_value(got, entry, terms, bad, what, r=r))
        for poke in pokes:                               # the only infeasible element, one Float32 ulp outside
            _, p, vals = poke
            keep = {k: d[k][p] for k in vals if np.ndim(d[k])}
            for k, v in vals.items():
                if k in b.b:
                    b.poke(k, p, v)
            try:
                dp = fx.poked(d, poke)
                t2, bad2 = fx.sep_terms(orc, entry, dp, variant)
                assert bad2, (entry, n, variant, poke[0])
                got = b.four(name, _sep_args(entry, dp, b, n, variant, n), (entry, n, variant, poke[0]))
                assert got == np.inf, (entry, n, variant, poke[0], got)
            finally:
                for k, v in keep.items():
                    if k in b.b:
                        b.poke(k, p, v)
    b.zone.check()
    _report(entry, "n=%d" % n, worst)


SEP_CASES = [(n, e) for n in fx.SEP_SIZES for e in sorted(fx.SEP_ENTRIES, key=fx.family_of)]


@pytest.mark.parametrize("n,entry", SEP_CASES, ids=["%s-n%d" % (e, n) for n, e in SEP_CASES])
def test_psi_separable(env, shared, orc, n, entry):
    """the eight separable entry points: the value (sum forms to 1e-12 of sum |term|, counts and 0 / +Inf exact) with the planted
    exact zeros and the elements exactly on the box / ball edge; then +Inf with one element an ulp outside, at 0, at n - 1, in the
    last partial trip.  Box forms: vector and scalar bounds in every pairing, with and without the mask."""
    fam = fx.family_of(entry)
    d, b = _state(shared, ("sep", n, fam), lambda: _sep_bufs(env, n, fam))
    variants = fx.BOX_VARIANTS if fam == "box" else (None,)
    pokes = d["pokes"]
    if n > 300_001:                                       # (2 x 4 Mi-term exact sums a case, not 5)
        variants = variants[:1] + variants[2:3]
    _sep_run(env, orc, d, b, entry, n, variants, pokes)


@pytest.mark.parametrize("flavour", ["subnormal", "huge", "mixed", "overflow"])
def test_psi_lhalf_extreme_magnitudes(env, shared, orc, flavour):
    """RootNormLhalf (and NormL1) where every |v| is a Float32 subnormal, where every |v| ~ 1e38, with a few of both among
    N(0, 1) data, and where (xk + sj) + y overflows Float32: the term is +Inf and so is psi(y).  (A 1e38 term among terms of
    order one sets the bar by itself: the all-subnormal and all-huge vectors are what hold the small and the large roots.)"""
    n = 257
    for fam, entries in (("plain", ("lhalf", "l1")), ("box", ("lhalf_box",))):
        if flavour == "overflow" and fam == "box":
            continue
        d, b = _state(shared, ("sep", n, fam, flavour), lambda: _sep_bufs(env, n, fam, flavour))
        for entry in entries:
            terms, _ = fx.sep_terms(orc, entry, d, "scal-scal-mask")
            assert (fx.nonfinite.sum_class(terms) == "+inf") == (flavour == "overflow")
            _sep_run(env, orc, d, b, entry, n, ("scal-scal-mask",) if fam == "box" else (None,), ())


# ====================================================================================================== b. spx_prox_group_l2_f32
PROX_LAYOUTS = fx.group_layouts("prox")
OBJ_LAYOUTS = fx.group_layouts("obj")


def _group_bufs(env, lay, which):
    name, n, offsets, gs, ng, scale = lay
    d = fx.group_data(lay)
    b = Bufs(env)
    k = sum(map(ord, name))
    for j, nm in enumerate(("q", "x", "sj") if which == "prox" else ("y", "x", "sj")):
        b.add(nm, d[nm], ALIGNS[(k + 3 * j + 1) % 4])
    if ng:
        b.add("lam", d["lam"], ALIGNS[(k + 2) % 4])
    if offsets is not None:
        b.add("offsets", offsets, 0)
    return d, b


@pytest.mark.parametrize("lay", PROX_LAYOUTS, ids=[l[0] for l in PROX_LAYOUTS])
def test_prox_group_l2_bits(env, orc, lay):
    """bit for bit against the restatement with every group's exact norm rounded to Float32 once; a group the census finds within
    1e-12 of a rounding boundary may take either neighbour's result (at most max(1, ngroups / 1000) of them: asserted on the CPU).
    Then y === q.  Indices in no group: y on entry - (xk + sj), y on entry non-zero."""
    name, n, offsets, gs, ng, scale = lay
    s, L, ctx = env
    import torch
    d, b = _group_bufs(env, lay, "prox")
    offs = fx.offsets_of(lay)
    ref, amb, alts = fx.prox_reference(orc, lay, d)
    covered = offsets is None or (offs[0] == 0 and offs[-1] == n)
    k = sum(map(ord, name))
    if covered:
        y = b.zone.add(n, torch.float32, ALIGNS[k % 4], role="out", name="y")
    else:
        y = b.add("y", d["y0"], ALIGNS[k % 4], role="inout")
    tail = (n, b.ptr("offsets"), gs if offsets is None else 0, ng, b.ptr("lam"), _F(float(fx.SIGMA)))
    torch.cuda.synchronize()
    s._lib.check(L.spx_prox_group_l2_f32(ctx, y.ptr(), b.ptr("q"), b.ptr("x"), b.ptr("sj"), *tail))
    torch.cuda.synchronize()
    other = fx.check_prox(y.t.cpu().numpy(), lay, ref, amb, alts, name)
    b.zone.check()
    # y === q: the uncovered indices then hold q - (xk + sj)
    if not covered:
        ref, amb, alts = fx.prox_reference(orc, lay, dict(d, y0=d["q"]))
    b.b["q"].role = "inout"
    s._lib.check(L.spx_prox_group_l2_f32(ctx, b.ptr("q"), b.ptr("q"), b.ptr("x"), b.ptr("sj"), *tail))
    torch.cuda.synchronize()
    other2 = fx.check_prox(b.b["q"].t.cpu().numpy(), lay, ref, amb, alts, name + " y===q")
    b.zone.check()
    assert other2 == other
    print("F32EXACT spx_prox_group_l2_f32 %s groups %d ambiguous %d took-the-other-neighbour %d" % (name, ng, len(amb), other))


# ====================================================================================================== c. psi(y) of the group forms
@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("lay", OBJ_LAYOUTS, ids=[l[0] for l in OBJ_LAYOUTS])
def test_psi_group(env, shared, orc, lay, binf):
    """spx_obj_group_l2_f32 / spx_obj_group_l2_binf_f32: the per-group terms (double)lambda_g * sqrt(sum of exact squares) summed
    exactly, the value to 1e-12 of the sum.  Binf: sj + y on the largest Float32 inside 1.1 Delta is feasible, one ulp outside --
    at index 0 or n - 1, in no group where the layout leaves them uncovered (k_obj_linf_scan) -- is +Inf."""
    name, n, offsets, gs, ng, scale = lay
    d, b = _state(shared, ("grp", name), lambda: _group_bufs(env, lay, "obj"))
    entry = "group_l2_binf" if binf else "group_l2"
    fn = "spx_obj_%s_f32" % entry
    delta = float(fx.DELTA * F32(scale))
    args = (b.ptr("y"), b.ptr("x"), b.ptr("sj"), n, b.ptr("offsets"), gs if offsets is None else 0, ng, b.ptr("lam")) + ((_F(delta),) if binf else ())
    terms, outside, badoff = fx.obj_group_terms(orc, lay, d, binf)
    assert not outside and not badoff
    got = b.four(fn, args, name)
    dev = fx.check_group_value(got, terms, outside, "%s %s" % (entry, name))
    for poke in (d["pokes"] if binf else ()):
        _, p, vals = poke
        keep = {k: d[k][p] for k in vals}
        for k, v in vals.items():
            b.poke(k, p, v)
        try:
            assert fx.obj_group_terms(orc, lay, fx.poked(d, poke), True)[1]
            got = b.four(fn, args, (name, poke[0]))
            assert got == np.inf, (name, poke[0], got)
        finally:
            for k, v in keep.items():
                b.poke(k, p, v)
    b.zone.check()
    _report(entry, name, dev)


@pytest.mark.parametrize("layout", ["decreasing", "negative_first", "last_past_n"])
def test_psi_group_rejects_bad_offsets(env, orc, layout):
    """offsets that decrease or leave [0, n]: SPX_ERR_INVALID_ARG, NaN in a device value target, every buffer intact (the
    Float32 twin of test_gpu_redzone's check), and a valid call on the same context afterwards."""
    n = 1 << 16
    off = {"decreasing": [0, 40_000, 30_000, n], "negative_first": [-4096, 30_000, n], "last_past_n": [0, 30_000, n + 8192]}[layout]
    lay = ("bad-" + layout, n, np.asarray(off, dtype=np.int64), 0, len(off) - 1, 1.0)
    d = fx.group_data(("bad", n, None, 8, n // 8, 1.0))
    d["lam"] = np.ones(len(off) - 1, dtype=F32)
    assert fx.obj_group_terms(orc, lay, d, False)[2]
    s, L, ctx = env
    b = Bufs(env)
    for j, nm in enumerate(("y", "x", "sj")):
        b.add(nm, d[nm], ALIGNS[(j + 1) % 4])
    b.add("lam", d["lam"], 4)
    b.add("offsets", lay[2], 0)
    for binf, key17 in itertools.product((False, True), (1, 0)):
        fn = "spx_obj_group_l2%s_f32" % ("_binf" if binf else "")
        args = (b.ptr("y"), b.ptr("x"), b.ptr("sj"), n, b.ptr("offsets"), 0, len(off) - 1, b.ptr("lam")) + ((_F(float(fx.DELTA)),) if binf else ())
        _, rc = b.value_of(fn, args, key17, "host", rc_want=1)
        assert rc == 1 and "offsets" in L.spx_last_error().decode(), (layout, binf, key17, rc)
        v, rc = b.value_of(fn, args, key17, "device", rc_want=None)
        assert rc == 0 and np.isnan(v), (layout, binf, key17, rc, v)
        b.zone.check()
    good = ("good", n, np.array([0, 30_000, 30_001, n], dtype=np.int64), 0, 3, 1.0)
    b.add("good", good[2], 0)
    d3 = dict(d, lam=np.ones(3, dtype=F32))
    b.add("lam3", d3["lam"], 0)
    got = b.four("spx_obj_group_l2_f32", (b.ptr("y"), b.ptr("x"), b.ptr("sj"), n, b.ptr("good"), 0, 3, b.ptr("lam3")), "good")
    fx.check_group_value(got, fx.obj_group_terms(orc, good, d3, False)[0], False, "after bad offsets")
    b.zone.check()
