"""GPU: every operator family on WHOLE problems at scale 2^k, k up to +-500 (Float32: +-60), against the oracle on the scaled
problem and against the library's own unit-scale result.

The kernels carry their own arithmetic -- hardware rcp / rsq seeds with Newton steps (fast_rcp, sqrt_pos, the team form's and
the separable kernels' twins), an absolute threshold on sums of squares (binf_ab), masked operands that leave sub-2^-1042 residues
(keep_if), r * r * r of an inverse square root (lhalf_a), chil * chil * P / (delta * delta) -- and the other files run them on data
of magnitude ~1 (tests/test_gpu_fuzz.py: 1e-6 .. 1e6) or with single extreme elements among ordinary ones.  Here the problems of
tests/scales.py are multiplied through by 2^k (lambda by its own power of the scale): every term of every sum is large or tiny at
once, and every square, product, norm and root stays a normal double (scales.assert_in_range checks the inputs).

Through the C ABI on a private context, each family on the smallest shapes that reach the kernel bodies its arithmetic lives in.
The bars are the project's own, none is new:

  (a) against the oracle ON THE SCALED PROBLEM: bit for bit for NormL1 / NormL0, their boxes, iprox!, top-r and the Float32 forms;
      arbiter.check_lhalf for RootNormLhalf; arbiter.check_group for the groups; 1e-12 of max(||ref||, ||xk||) for ShiftedNormL1B2
      (tests/test_gpu_proxval_b2.py).  The reference is not scale-free (tests/test_scales_helpers.py): where the absolute
      epsilon = 1 of the Binf bracket makes it zero a group at small scale, the GPU must zero that group too.
  (b) against the GPU's own result at k = 0: y(2^k P) == 2^k y(P) in bits for the families of the first kind, within 1e-12 of the
      operand scale for RootNormLhalf, the groups and B2 (the largest deviation in ulps is printed per family and k:
      `scales-ulps ...`); for Binf only on the groups the oracle zeroes neither at k nor at 0.
  (c) the fused calls: y the bits of the plain call, xkn the bits of (xk + sj) + y, [0] the oracle's objective of that y (exactly
      for NormL0, 1e-12 otherwise), the other sums within 1e-12 of sum |term| of math.fsum; a batched call: every row the bits of
      the single call on that row, its sums to the bars of the batch files, the k = 0 row the bits of a batch of one; the
      batched ShiftedNormL1B2 call, whose root iteration is its own, to (a) and (b) at the B2 bar, its inactive rows to bits.
  (d) psi(y) at the feasibility edges: the B2 ball with its absolute eps, the box slack, the 1.1 Delta edge of the Binf forms.

The LDS and streaming forms of ShiftedNormL1B2 are reached with tuning key 8 = 4 at n = 50 001 and 70 001, as
tests/test_gpu_proxval_b2.py reaches them (tests/test_gpu_stress.py::test_b2_streaming_form_scenarios takes n = 2.3e6 for them)."""
import ctypes
import math

import numpy as np
import pytest

import arbiter
import f32_exact
import scales

pytestmark = pytest.mark.gpu

TOL = 1e-12
POISON = -777.25
_D = ctypes.c_double
K64, K64_LARGE, K32 = scales.K64, scales.K64_LARGE, scales.K32


@pytest.fixture(scope="module")
def s():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.build()


@pytest.fixture(scope="module")
def ctx(s):
    """a private context: the tuning keys set here never reach the context the other test files share"""
    L = s._lib.load()
    c = ctypes.c_void_p()
    s._lib.check(L.spx_ctx_create(0, ctypes.byref(c)))
    yield c
    L.spx_sync(c)
    L.spx_ctx_destroy(c)


def _dev(a):
    """a device copy, complete before the library's own stream may read it"""
    import torch
    t = torch.tensor(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _fresh(n, dtype=np.float64):
    import torch
    t = torch.full((n,), POISON, dtype=torch.float64 if dtype is np.float64 else torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _ok(L, rc, what):
    assert rc == 0, (what, rc, L.spx_last_error())


def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).tolist())


def _check_sum(got, terms, what):
    ref, mag = _fsum(terms), _fsum(np.abs(terms))
    print("%s: %.17g ref %.17g (bar %.3g)" % (what, got, ref, TOL * mag))
    assert math.isfinite(got) and abs(got - ref) <= TOL * mag, (what, got, ref, mag)


def _check_h(kind, h, exp, what):
    print("%s: h %.17g ref %.17g" % (what, h, exp))
    assert math.isfinite(exp), (what, exp)
    if kind == "l0":
        assert h == exp, (what, h, exp)
    else:
        assert abs(h - exp) <= TOL * abs(exp), (what, h, exp)


def _set(L, ctx, key, v):
    assert L.spx_ctx_set_tuning(ctx, key, v) == 0, (key, v)


_ULPS = {}


def _note_ulps(family, k, yk, y0):
    """(b) for the families held to a tolerance: the largest deviation of y(2^k P) / 2^k from y(P) in ulps, per family and k"""
    u = scales.ulps(scales.unscale(yk, k), y0)
    _ULPS[(family, k)] = max(_ULPS.get((family, k), 0.0), u)
    print("scales-ulps family=%s k=%d max=%.3g" % (family, k, _ULPS[(family, k)]))


# ====================================================================================================== separable, Float64
SEP_PROX = ["prox_l1", "prox_l0", "prox_lhalf", "prox_l1_box", "prox_l0_box", "prox_lhalf_box"]
SEP_IPROX = ["iprox_l1", "iprox_l0", "iprox_l1_box", "iprox_l0_box"]


class _SepDev:
    def __init__(self, P):
        self.P, self.n = P, P.n
        self.q, self.x, self.sj = _dev(P.q), _dev(P.xk), _dev(P.sj)
        self.d = _dev(P.d) if P.d is not None else None
        self.lv = _dev(P.l) if P.l is not None and np.ndim(P.l) else None
        self.uv = _dev(P.u) if P.u is not None and np.ndim(P.u) else None
        self.mask = _dev(P.mask) if P.mask is not None else None

    def box(self):
        P = self.P
        if P.l is None:
            return ()
        ls = 0.0 if self.lv is not None else float(P.l)
        us = 0.0 if self.uv is not None else float(P.u)
        return (_p(self.lv), _p(self.uv), ls, us, _p(self.mask))


def _sep_call(L, ctx, V, fam):
    """one call of the family -> (y, xkn or None, statistics)"""
    P, n = V.P, V.n
    y = _fresh(n)
    name = P.op
    box = V.box()
    if name.startswith("iprox"):
        head = (ctx, _p(y), _p(V.q), _p(V.d), _p(V.x), _p(V.sj), n, float(P.lam)) + (box if box else (0,))
        if fam == "plain":
            _ok(L, getattr(L, "spx_" + name)(*head), name)
            return y, None, []
        xkn, st = _fresh(n), (_D * 4)()
        _ok(L, getattr(L, "spx_iproxstep_" + name[6:])(*head, _p(xkn), st, None), name)
        return y, xkn, list(st)
    head = (ctx, _p(y), _p(V.q), _p(V.x), _p(V.sj), n, float(P.lam), float(P.sigma)) + box
    if fam == "plain":
        _ok(L, getattr(L, "spx_" + name)(*head), name)
        return y, None, []
    if fam == "val":
        val = _D(-1.0)
        _ok(L, getattr(L, "spx_proxval_" + name[5:])(*head, 1.0, ctypes.byref(val)), name)
        return y, None, [val.value]
    xkn, st = _fresh(n), (_D * 3)()
    _ok(L, getattr(L, "spx_proxstep_" + name[5:])(*head, 1.0, _p(xkn), st, None), name)
    return y, xkn, list(st)


def _sep_terms(P, y):
    if P.op.startswith("iprox"):
        return [("gy", P.q * y), ("ydy", (P.d * y) * y), ("yy", y * y)]
    return [("qy", P.q * y), ("yy", y * y)]


def _sep_at(L, ctx, orc, P, what):
    """(a) and (c) on the problem as it stands -> y of the plain call"""
    V = _SepDev(P)
    ref = scales.oracle_y(orc, P)
    y = _host(_sep_call(L, ctx, V, "plain")[0]).copy()
    if P.h == "lhalf":
        box = None if P.l is None else (P.l, P.u)
        arbiter.check_lhalf(orc, y, ref, P.q, P.xk, P.sj, P.lam, P.sigma, box=box, mask=P.mask, what=what)
    else:
        assert scales.same_bits(y, ref), (what, "y against the oracle", scales.ulps(y, ref))
    h_exp = scales.oracle_h(orc, P, y)
    for fam in (("step",) if P.op.startswith("iprox") else ("val", "step")):
        yf, xkn, st = _sep_call(L, ctx, V, fam)
        assert scales.same_bits(_host(yf), y), (what, fam, "y")
        if xkn is not None:
            assert scales.same_bits(_host(xkn), (P.xk + P.sj) + y), (what, fam, "xkn")
        _check_h(P.h, st[0], h_exp, "%s %s" % (what, fam))
        if fam == "step":
            for (nm, t), got in zip(_sep_terms(P, y), st[1:]):
                _check_sum(got, t, "%s %s" % (what, nm))
    return y


def _sep_problems(op):
    """n = 3 (the element-wise kernel) and 6145 (two tiles of the staged skeleton and an odd tail); the Box forms with scalar bounds
    and with two bound vectors and a mask"""
    out = []
    for n in (3, 6145):
        if op.endswith("_box"):
            out.append(("n=%d ss" % n, scales.separable(op, n)))
            out.append(("n=%d vv+mask" % n, scales.separable(op, n, vec_bounds=True, masked=True)))
        else:
            out.append(("n=%d" % n, scales.separable(op, n)))
    return out


@pytest.mark.parametrize("op", SEP_PROX + SEP_IPROX)
def test_separable_f64(s, orc, ctx, op):
    L = s._lib.load()
    try:
        for tag, P0 in _sep_problems(op):
            _set(L, ctx, 3, 1)
            y0 = _sep_at(L, ctx, orc, P0, "%s %s k=0" % (op, tag))
            for k in K64:
                scales.assert_in_range(P0, k)
                what = "%s %s k=%d" % (op, tag, k)
                yk = _sep_at(L, ctx, orc, scales.scaled(P0, k), what)
                if P0.h == "lhalf":                                                  # (b)
                    _note_ulps(op, k, yk, y0)
                    bar = TOL * arbiter.lhalf_scale(y0, P0.xk, P0.sj, P0.q)
                    assert (np.abs(scales.unscale(yk, k) - y0) <= bar).all(), (what, "against the unit-scale result")
                else:
                    assert scales.same_bits(scales.unscale(yk, k), y0), (what, "against the unit-scale result")
            if P0.n > 3 and P0.mask is None:       # the register-staged skeleton, once per operator, at the smallest scale
                _set(L, ctx, 3, 0)
                yr = _sep_at(L, ctx, orc, scales.scaled(P0, K64[0]), "%s %s k=%d key3=0" % (op, tag, K64[0]))
                _set(L, ctx, 3, 1)
                ys = _host(_sep_call(L, ctx, _SepDev(scales.scaled(P0, K64[0])), "plain")[0])
                assert scales.same_bits(yr, ys), (op, tag, "register-staged against LDS-staged")
    finally:
        _set(L, ctx, 3, 1)


# ====================================================================================================== separable, Float32
def _f32_call(L, ctx, P, name):
    n = P.n
    q, x, sj = _dev(P.q), _dev(P.xk), _dev(P.sj)
    d = _dev(P.d) if P.d is not None else None
    lv = _dev(P.l) if P.l is not None and np.ndim(P.l) else None
    uv = _dev(P.u) if P.u is not None and np.ndim(P.u) else None
    mk = _dev(P.mask) if P.mask is not None else None
    box = () if P.l is None else (_p(lv), _p(uv), 0.0 if lv is not None else float(P.l), 0.0 if uv is not None else float(P.u), _p(mk))
    y = _fresh(n, np.float32)
    fn = getattr(L, "spx_%s_f32" % name)
    if name.startswith("iprox"):
        rc = fn(ctx, _p(y), _p(q), _p(d), _p(x), _p(sj), n, float(P.lam), *(box if box else (0,)))
    else:
        rc = fn(ctx, _p(y), _p(q), _p(x), _p(sj), n, float(P.lam), float(np.float32(P.sigma)), *box)
    _ok(L, rc, name)
    _ok(L, L.spx_sync(ctx), name)
    return _host(y).copy(), (x, sj, lv, uv, mk, box)


@pytest.mark.parametrize("op", ["prox_l1", "prox_l0", "prox_l1_box", "prox_l0_box", "iprox_l1", "iprox_l0", "iprox_l1_box", "iprox_l0_box"])
def test_separable_f32(s, orc, ctx, op):
    """spx_prox_*_f32 / spx_iprox_*_f32 at n = 6145 over K32, bit for bit against the Float32 oracle on the scaled problem and
    against the unit-scale result; spx_obj_*_f32 of that y: (double)lambda times the exact sum of the oracle's terms, to 1e-12
    of sum |term| (tests/test_gpu_f32_exact.py)."""
    L = s._lib.load()
    for tag, kw in (("ss", {}), ("vv+mask", dict(vec_bounds=True, masked=True))) if op.endswith("_box") else (("", {}),):
        P0 = scales.separable(op, 6145, dtype=np.float32, **kw)
        y0 = None
        for k in (0,) + K32:
            scales.assert_in_range(P0, k)
            P = scales.scaled(P0, k) if k else P0
            what = "%s_f32 %s k=%d" % (op, tag, k)
            y, (x, sj, lv, uv, mk, box) = _f32_call(L, ctx, P, op)
            ref = scales.oracle_y(orc, P)
            assert y.dtype == np.float32 and scales.same_bits(y, ref), (what, "against the oracle")
            if y0 is None:
                y0 = y
            else:
                assert scales.same_bits(scales.unscale(y, k), y0), (what, "against the unit-scale result")
            # psi(y) of that y: the operator's own kind and, for the NormL1 forms, RootNormLhalf's (it has no Float32 prox!)
            for kind in ([P.h] + (["lhalf"] if P.h == "l1" else [])) if op.startswith("prox") else []:
                terms, bad = orc.obj_f32(kind, y, P.xk, P.sj, l=P.l, u=P.u, mask=P.mask)
                # (bad: the reference's feasibility scan has an ABSOLUTE slack sqrt(eps32); at scale 2^40 one rounding of sj + y at a
                #  bound is outside it, and psi(y) of the prox result is +Inf in the reference: the library must say so too)
                val = _D(-1.0)
                yd = _dev(y)
                fn = getattr(L, "spx_obj_%s%s_f32" % (kind, "_box" if op.endswith("_box") else ""))
                _ok(L, fn(ctx, _p(yd), _p(x), _p(sj), P.n, float(P.lam), *box, ctypes.byref(val)), what)
                lam = float(np.float32(P.lam))
                exp, mag = lam * _fsum(terms), lam * _fsum(np.abs(terms))
                print("%s: psi[%s] %.17g ref %.17g infeasible %s" % (what, kind, val.value, exp, bad))
                if bad:
                    assert val.value == math.inf, (what, kind, val.value)
                else:
                    assert abs(val.value - exp) <= TOL * mag, (what, kind, val.value, exp)


# ====================================================================================================== the group operators
class _Layout:
    """how the groups are handed to the library: uniform (group_size), CSR offsets (group_size = 0: no bound) or index sets"""

    def __init__(self, P, gather=False):
        self.P, self.gather = P, gather
        self.off = P.csr()
        self.ng = len(self.off) - 1
        self.offd = _dev(self.off) if (P.offsets is not None or gather) else None
        self.idx = _dev(np.arange(P.n, dtype=np.int64)) if gather else None

    def args(self):
        """(group_offsets, group_size, ngroups) / (group_ptr, group_index, ngroups, nnz)"""
        if self.gather:
            return (_p(self.offd), _p(self.idx), self.ng, self.P.n)
        return (_p(self.offd), self.P.gsize, self.ng)


def _group_calls(L, ctx, orc, P, lay, what, fused=True):
    """(a) the plain call against the oracle on the problem as it stands, the zero pattern, psi(y), and (c) the fused calls -> y"""
    import torch
    n, binf = P.n, P.delta is not None
    sfx = ("_binf" if binf else "") + ("_gather" if lay.gather else "")
    q, x, sj, lam = _dev(P.q), _dev(P.xk), _dev(P.sj), _dev(P.lam)
    tail = (float(P.delta),) if binf else ()
    y = _fresh(n)
    if lay.gather:
        y.zero_()
        torch.cuda.synchronize()
    head = lambda yt: (ctx, _p(yt), _p(q), _p(x), _p(sj), n) + lay.args() + (_p(lam), float(P.sigma)) + tail
    _ok(L, getattr(L, "spx_prox_group_l2" + sfx)(*head(y)), what)
    _ok(L, L.spx_sync(ctx), what)
    yh = _host(y).copy()
    ref = scales.oracle_y(orc, P)
    assert np.isfinite(yh).all(), what
    arbiter.check_group(orc, yh, ref, P.q, P.xk, P.sj, P.lam, P.sigma, lay.off, delta=P.delta, what=what)
    zg, zr = arbiter.zero_pattern(yh, P.xk, P.sj, lay.off), arbiter.zero_pattern(ref, P.xk, P.sj, lay.off)
    assert np.array_equal(zg, zr), (what, "zeroed groups", np.flatnonzero(zg != zr).tolist())
    # psi(y) on the same layout
    obj = _D(-1.0)
    rc = getattr(L, "spx_obj_group_l2" + sfx)(ctx, _p(y), _p(x), _p(sj), n, *lay.args(), _p(lam), *tail, ctypes.byref(obj))
    _ok(L, rc, what)
    exp = orc.obj_group_l2(yh, P.xk, P.sj, P.lam, offsets=lay.off, delta=P.delta)
    print("%s: psi(y) %.17g ref %.17g" % (what, obj.value, exp))
    assert obj.value == exp or abs(obj.value - exp) <= TOL * abs(exp), (what, "psi(y)", obj.value, exp)
    if not fused or lay.gather:
        return yh, zr
    h_exp = orc.obj_group_l2(yh, P.xk, P.sj, P.lam, offsets=lay.off)
    y1, val = _fresh(n), _D(-1.0)
    _ok(L, getattr(L, "spx_proxval_group_l2" + sfx)(*head(y1), 1.0, ctypes.byref(val)), what)
    assert scales.same_bits(_host(y1), yh), (what, "proxval y")
    _check_h("l1", val.value, h_exp, what + " value")
    y2, xkn, st = _fresh(n), _fresh(n), (_D * 3)()
    _ok(L, getattr(L, "spx_proxstep_group_l2" + sfx)(*head(y2), 1.0, _p(xkn), st, None), what)
    assert scales.same_bits(_host(y2), yh), (what, "proxstep y")
    assert scales.same_bits(_host(xkn), (P.xk + P.sj) + yh), (what, "xkn")
    _check_h("l1", st[0], h_exp, what + " step")
    _check_sum(st[1], P.q * yh, what + " qy")
    _check_sum(st[2], yh * yh, what + " yy")
    return yh, zr


def _group_sweep(L, ctx, orc, P0, ks, what, gather=False, family=None, fused=True):
    """k = 0 and every k of ks: (a), (c) and (b) -> {k: the groups the oracle zeroes}"""
    lay0 = _Layout(P0, gather)
    y0, z0 = _group_calls(L, ctx, orc, P0, lay0, "%s k=0" % what, fused)
    zeroed = {0: z0}
    scale0 = arbiter.group_scale(y0, P0.q, P0.xk, P0.sj, lay0.off)
    sizes = np.diff(lay0.off)
    for k in ks:
        scales.assert_in_range(P0, k)
        P = scales.scaled(P0, k)
        yk, zk = _group_calls(L, ctx, orc, P, _Layout(P, gather), "%s k=%d" % (what, k), fused)
        zeroed[k] = zk
        keep = np.ones(P0.n, dtype=bool)
        if P0.delta is not None:         # Binf: the reference is not equivariant -- only the groups it zeroes neither at k nor at 0
            keep[lay0.off[0]:lay0.off[-1]] = np.repeat(~(zk | z0), sizes)
        yu = scales.unscale(yk, k)
        _note_ulps(family or P0.op, k, yk[keep], y0[keep])
        assert (np.abs(yu - y0)[keep] <= (TOL * scale0)[keep]).all(), (
            what, k, "against the unit-scale result", float(np.max((np.abs(yu - y0) / np.maximum(scale0, 1e-300))[keep])))
    return zeroed


GROUP_SIZES = [1, 2, 8, 16, 33, 128, 300, 512, 1024]


UNIFORM = [(False, gs, 0) for gs in GROUP_SIZES] + [(True, gs, k9) for gs in GROUP_SIZES for k9 in (0, 1)]


@pytest.mark.parametrize("binf,gs,key9", UNIFORM, ids=["%s-%d-key9=%d" % ("binf" if b else "plain", g, k9) for b, g, k9 in UNIFORM])
def test_uniform_groups(s, orc, ctx, binf, gs, key9):
    """40 uniform groups of gs: the one- and two-lane tiles, the 4- and 8-lane tiles, partly filled tiles, and 1024 (LDS-resident).
    K64 up to n = 1e4; 300 and 512 take K64 and K64_LARGE, 1024 K64_LARGE."""
    L = s._lib.load()
    P0 = scales.groups(gs, 40, binf)
    ks = K64 if P0.n <= 10_000 else (K64_LARGE if gs > 512 else tuple(sorted(K64 + K64_LARGE)))
    try:
        _set(L, ctx, 9, key9)
        _group_sweep(L, ctx, orc, P0, ks, "groups %s gs=%d key9=%d" % ("binf" if binf else "plain", gs, key9),
                     family="group_l2%s_key9=%d" % ("_binf" if binf else "", key9))
    finally:
        _set(L, ctx, 9, 0)


@pytest.mark.parametrize("key9", [0, 1])
def test_binf_zeroes_the_groups_the_reference_zeroes_at_small_scale(s, orc, ctx, key9):
    """scales.binf_regime(): at k <= -10 the reference's bracket (absolute epsilon = 1) no longer encloses the root of one group of
    8 and it writes zeros there, which it does not at k = 0 (tests/test_scales_helpers.py).  The regime is among the cases, and
    the GPU zeroes the same groups: y == -(xk + sj) exactly there (_group_calls compares the zero patterns at every k)."""
    L = s._lib.load()
    P0 = scales.binf_regime()
    try:
        _set(L, ctx, 9, key9)
        zeroed = _group_sweep(L, ctx, orc, P0, K64, "binf regime key9=%d" % key9, family="group_l2_binf_key9=%d" % key9)
    finally:
        _set(L, ctx, 9, 0)
    small = [k for k in K64 if k <= -10]
    assert small and all((zeroed[k] & ~zeroed[0]).any() for k in small), {k: np.flatnonzero(z).tolist() for k, z in zeroed.items()}
    assert all(np.array_equal(zeroed[k], zeroed[0]) for k in K64 if k > 0)


def _ragged_offsets():
    rng = np.random.default_rng(5301)
    sizes = rng.integers(0, 31, size=60)
    sizes[0] = 7           # (the all-zero group)
    sizes[::13] = 0
    sizes[0] = 7
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
def test_ragged_groups(s, orc, ctx, binf):
    """CSR offsets without a size bound: the element provider that re-reads its group from memory (MemGroup)"""
    L = s._lib.load()
    P0 = scales.groups(0, 0, binf, seed=5302 + binf, offsets=_ragged_offsets())
    _group_sweep(L, ctx, orc, P0, K64, "ragged %s" % ("binf" if binf else "plain"), family="group_l2%s_ragged" % ("_binf" if binf else ""))


@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
def test_index_set_groups(s, orc, ctx, binf):
    """the gather kernels (spx_prox_group_l2[_binf]_gather, spx_obj_group_l2[_binf]_gather) on the ragged layout given as index
    sets: every index in exactly one group, in order, so the contiguous oracle is the expectation"""
    L = s._lib.load()
    P0 = scales.groups(0, 0, binf, seed=5304 + binf, offsets=_ragged_offsets())
    _group_sweep(L, ctx, orc, P0, K64, "gather %s" % ("binf" if binf else "plain"), gather=True,
                 family="group_l2%s_gather" % ("_binf" if binf else ""))


@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
def test_one_group_over_the_vector(s, orc, ctx, binf):
    """the team form (csrc/spx_group_team.hip, its own Newton iteration and square roots): one group over n = 120 000, lambda =
    0.4 sqrt(n) as in tests/test_gpu_graph.py, at K64_LARGE"""
    L = s._lib.load()
    n = 120_000
    x, sj, q = scales.draw(n, 5306, delta=0.8 if binf else None)
    P0 = scales.Problem(op="prox_group_l2_binf" if binf else "prox_group_l2", q=q, xk=x, sj=sj, lam=np.array([0.4 * math.sqrt(n)]),
                        sigma=0.9, delta=0.8 if binf else None, gsize=n)
    _group_sweep(L, ctx, orc, P0, K64_LARGE, "team %s" % ("binf" if binf else "plain"), family="group_l2%s_team" % ("_binf" if binf else ""))


@pytest.mark.parametrize("gs", [5, 129])
def test_groups_f32(s, orc, ctx, gs):
    """spx_prox_group_l2_f32 over K32: the bit rule of tests/test_gpu_f32_exact.py (the exact norm rounded to Float32 once; a group
    whose exact norm sits within 1e-12 of a midpoint may take either neighbour), and bits against the unit-scale result"""
    import torch
    L = s._lib.load()
    P0 = scales.groups(gs, 40, False, dtype=np.float32)
    y0 = None
    for k in (0,) + K32:
        scales.assert_in_range(P0, k)
        P = scales.scaled(P0, k) if k else P0
        q, x, sj, lam = _dev(P.q), _dev(P.xk), _dev(P.sj), _dev(P.lam)
        y = _fresh(P.n, np.float32)
        y.zero_()
        torch.cuda.synchronize()
        _ok(L, L.spx_prox_group_l2_f32(ctx, _p(y), _p(q), _p(x), _p(sj), P.n, None, gs, 40, _p(lam), float(np.float32(P.sigma))), "f32 groups")
        _ok(L, L.spx_sync(ctx), "f32 groups")
        lay = ("scales", P.n, None, gs, 40, 1.0)
        d = {"q": P.q, "x": P.xk, "sj": P.sj, "lam": P.lam, "y0": np.zeros(P.n, dtype=np.float32)}
        ref, amb, alts = f32_exact.prox_reference(orc, lay, d, sigma=P.sigma)
        yh = _host(y).copy()
        other = f32_exact.check_prox(yh, lay, ref, amb, alts, "f32 groups gs=%d k=%d" % (gs, k))
        if y0 is None:
            y0 = yh
        elif not amb and not other:
            assert scales.same_bits(scales.unscale(yh, k), y0), (gs, k, "against the unit-scale result")


# ====================================================================================================== top-r
@pytest.mark.parametrize("lattice", [False, True], ids=["continuous", "lattice8"])
@pytest.mark.parametrize("n", [5000, 70_001])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_topr(s, orc, ctx, f32, n, lattice):
    """spx_prox_indball_l0[_binf] and the _f32 twins, r = n / 3: one workgroup (n = 5000) and the on-chip form (70 001); bit for bit
    against the oracle on the scaled problem and against the unit-scale result.  (The larger forms compare bit patterns and
    have no arithmetic of their own.)"""
    L = s._lib.load()
    dt = np.float32 if f32 else np.float64
    for binf in (False, True):
        P0 = scales.topr(n, binf, lattice=lattice, dtype=dt)
        ks = K32 if f32 else (K64 if n <= 10_000 else K64_LARGE)
        y0 = None
        for k in (0,) + tuple(ks):
            scales.assert_in_range(P0, k)
            P = scales.scaled(P0, k) if k else P0
            q, x, sj = _dev(P.q), _dev(P.xk), _dev(P.sj)
            y = _fresh(n, dt)
            fn = getattr(L, "spx_prox_indball_l0%s%s" % ("_binf" if binf else "", "_f32" if f32 else ""))
            _ok(L, fn(ctx, _p(y), _p(q), _p(x), _p(sj), n, P.r, *((float(P.delta),) if binf else ())), "top-r")
            _ok(L, L.spx_sync(ctx), "top-r")
            yh = _host(y).copy()
            what = ("top-r", f32, n, lattice, binf, k)
            assert scales.same_bits(yh, scales.oracle_y(orc, P)), (what, "against the oracle")
            if y0 is None:
                y0 = yh
            else:
                assert scales.same_bits(scales.unscale(yh, k), y0), (what, "against the unit-scale result")


# ====================================================================================================== ShiftedNormL1B2
B2_FORMS = [("register", 10_000, 0, K64), ("lds", 50_001, 4, K64_LARGE), ("streaming", 70_001, 4, K64_LARGE)]


def _b2_at(L, ctx, orc, P, what):
    n = P.n
    q, x, sj = _dev(P.q), _dev(P.xk), _dev(P.sj)
    args = (n, float(P.lam), float(P.sigma), float(P.delta), float(P.chi))
    y = _fresh(n)
    _ok(L, L.spx_prox_l1_b2(ctx, _p(y), _p(q), _p(x), _p(sj), *args), what)
    _ok(L, L.spx_sync(ctx), what)
    yh = _host(y).copy()
    ref = scales.oracle_y(orc, P)
    err, bar = float(np.max(np.abs(yh - ref))), TOL * max(np.linalg.norm(ref), np.linalg.norm(P.xk))   # tests/test_gpu_proxval_b2.py
    print("%s: max |y - oracle| %.3e (bar %.3e)" % (what, err, bar))
    assert np.isfinite(yh).all() and err <= bar, (what, err, bar)
    h_exp = orc.obj_plain("l1", yh, P.xk, P.sj, P.lam)
    y1, val = _fresh(n), _D(-1.0)
    _ok(L, L.spx_proxval_l1_b2(ctx, _p(y1), _p(q), _p(x), _p(sj), *args, 1.0, ctypes.byref(val)), what)
    assert scales.same_bits(_host(y1), yh), (what, "proxval y")
    _check_h("l1", val.value, h_exp, what + " value")
    y2, xkn, st = _fresh(n), _fresh(n), (_D * 3)()
    _ok(L, L.spx_proxstep_l1_b2(ctx, _p(y2), _p(q), _p(x), _p(sj), *args, 1.0, _p(xkn), st, None), what)
    assert scales.same_bits(_host(y2), yh), (what, "proxstep y")
    assert scales.same_bits(_host(xkn), (P.xk + P.sj) + yh), (what, "xkn")
    _check_h("l1", st[0], h_exp, what + " step")
    _check_sum(st[1], P.q * yh, what + " qy")
    _check_sum(st[2], yh * yh, what + " yy")
    obj = _D(-1.0)
    _ok(L, L.spx_obj_l1_b2(ctx, _p(y), _p(x), _p(sj), n, float(P.lam), float(P.delta), ctypes.byref(obj)), what)
    exp = orc.obj_l1_b2(yh, P.xk, P.sj, P.lam, P.delta)
    print("%s: psi(y) %.17g ref %.17g" % (what, obj.value, exp))
    assert obj.value == exp or abs(obj.value - exp) <= TOL * abs(exp), (what, "psi(y)", obj.value, exp)
    return yh


@pytest.mark.parametrize("active", [True, False], ids=["active", "inactive"])
@pytest.mark.parametrize("form,n,cap,ks", B2_FORMS, ids=[f[0] for f in B2_FORMS])
def test_l1_b2(s, orc, ctx, form, n, cap, ks, active):
    L = s._lib.load()
    P0 = scales.b2(n, active)
    try:
        _set(L, ctx, 8, cap)
        y0 = _b2_at(L, ctx, orc, P0, "b2 %s %s k=0" % (form, active))
        nrm = float(np.linalg.norm(P0.sj + y0))
        assert (abs(nrm - P0.delta) <= 1e-9 * P0.delta) if active else (nrm < 0.9 * P0.delta), (form, active, nrm)
        bar0 = TOL * max(np.linalg.norm(y0), np.linalg.norm(P0.xk))
        for k in ks:
            scales.assert_in_range(P0, k)
            yk = _b2_at(L, ctx, orc, scales.scaled(P0, k), "b2 %s %s k=%d" % (form, active, k))
            _note_ulps("l1_b2_%s_%s" % (form, "active" if active else "inactive"), k, yk, y0)
            assert float(np.max(np.abs(scales.unscale(yk, k) - y0))) <= bar0, (form, active, k, "against the unit-scale result")
    finally:
        _set(L, ctx, 8, 0)


# ====================================================================================================== psi(y) at its edges
def test_obj_l1_b2_with_the_absolute_eps(s, orc, ctx):
    """the planted point of tests/test_scales_helpers.py: +Inf at k = 0 and k = 500, feasible at k = -500 (atol = eps)"""
    L = s._lib.load()
    y, x, sj, lam, delta = scales.b2_flip_point()
    seen = {}
    for k in (0, -500, 500, -200, 200):
        c = lambda a: np.ldexp(a, k)
        yd, xd, sd = _dev(c(y)), _dev(c(x)), _dev(c(sj))
        obj = _D(-1.0)
        _ok(L, L.spx_obj_l1_b2(ctx, _p(yd), _p(xd), _p(sd), len(y), math.ldexp(lam, k), math.ldexp(delta, k), ctypes.byref(obj)), "obj b2")
        exp = orc.obj_l1_b2(c(y), c(x), c(sj), math.ldexp(lam, k), math.ldexp(delta, k))
        seen[k] = exp
        assert obj.value == exp or (math.isfinite(exp) and abs(obj.value - exp) <= TOL * abs(exp)), (k, obj.value, exp)
    assert seen[0] == math.inf and seen[500] == math.inf and math.isfinite(seen[-500]), seen


@pytest.mark.parametrize("kind", ["l1", "l0", "lhalf"])
def test_obj_box_slack_is_absolute(s, orc, ctx, kind):
    """a point outside [l, u] by 1e-9 * 2^k: inside the reference's sqrt(eps) slack at k = -40, outside it at k = +40"""
    L = s._lib.load()
    y, x, sj, l, u = scales.box_slack_point()
    seen = {}
    for k in (-40, 0, 40):
        c = lambda a: np.ldexp(a, k)
        lam = math.ldexp(scales.LAM, int(scales.LAM_POW[kind] * k))
        yd, xd, sd = _dev(c(y)), _dev(c(x)), _dev(c(sj))
        obj = _D(-1.0)
        _ok(L, getattr(L, "spx_obj_%s_box" % kind)(ctx, _p(yd), _p(xd), _p(sd), len(y), lam, None, None, math.ldexp(l, k),
                                                    math.ldexp(u, k), None, ctypes.byref(obj)), "obj box")
        seen[k] = exp = orc.obj_box(kind, c(y), c(x), c(sj), lam, math.ldexp(l, k), math.ldexp(u, k))
        assert obj.value == exp or (math.isfinite(exp) and abs(obj.value - exp) <= TOL * abs(exp)), (kind, k, obj.value, exp)
    assert math.isfinite(seen[-40]) and math.isfinite(seen[0]) and seen[40] == math.inf, seen


@pytest.mark.parametrize("k", [-200, 200])
def test_obj_binf_edge_at_scale(s, orc, ctx, k):
    """|sj + y| at 1.1 Delta and one ulp above it, Delta = 0.8 * 2^k: spx_obj_group_l2_binf and spx_obj_indball_l0_binf give +Inf
    exactly where the oracle does, and the oracle's value otherwise"""
    L = s._lib.load()
    P = scales.scaled(scales.groups(8, 40, True), k)
    n = P.n
    edge = 1.1 * P.delta
    verdicts = []
    for t in (edge, np.nextafter(edge, math.inf)):
        sj = np.array(P.sj)
        sj[13] = 0.0
        y = np.clip(np.array(P.q), -0.5 * P.delta, 0.5 * P.delta) - sj
        y[13] = t
        assert (sj + y)[13] == t and float(np.max(np.abs(np.delete(sj + y, 13)))) < 0.6 * P.delta
        yd, xd, sd, ld = _dev(y), _dev(P.xk), _dev(sj), _dev(P.lam)
        obj = _D(-1.0)
        _ok(L, L.spx_obj_group_l2_binf(ctx, _p(yd), _p(xd), _p(sd), n, None, 8, 40, _p(ld), float(P.delta), ctypes.byref(obj)), "obj binf")
        exp = orc.obj_group_l2(y, P.xk, sj, P.lam, gsize=8, delta=P.delta)
        assert obj.value == exp or (math.isfinite(exp) and abs(obj.value - exp) <= TOL * abs(exp)), (k, t, obj.value, exp)
        obj2 = _D(-1.0)
        _ok(L, L.spx_obj_indball_l0_binf(ctx, _p(yd), _p(xd), _p(sd), n, n, float(P.delta), ctypes.byref(obj2)), "obj top-r binf")
        exp2 = orc.obj_indball_l0(y, P.xk, sj, n, delta=P.delta)
        assert obj2.value == exp2, (k, t, obj2.value, exp2)
        verdicts.append((exp, exp2))
    assert math.isfinite(verdicts[0][0]) and verdicts[0][1] == 0.0 and verdicts[1] == (math.inf, math.inf), verdicts


# ====================================================================================================== the batched calls
ROW_K = (-500, -200, -40, 0, 40, 200, 500)      # batch = 7: a different k in every row, one row at k = 0


def _rows(P0):
    out = []
    for k in ROW_K:
        scales.assert_in_range(P0, k)
        out.append(scales.scaled(P0, k) if k else P0)
    return out


def _stack(rows, name):
    return _dev(np.stack([np.asarray(getattr(P, name), dtype=np.float64) for P in rows]))


def _scalars(rows, name):
    return _dev(np.array([float(getattr(P, name)) for P in rows]))


def _check_batch_sums(got, single, terms, what):
    """the bars of the batch files: [0] within 1e-12 of the single call's, the other sums within 1e-12 sum |term| of math.fsum"""
    assert abs(got[0] - single[0]) <= TOL * abs(single[0]), (what, got[0], single[0])
    for (nm, t), g in zip(terms, got[1:]):
        _check_sum(float(g), t, "%s %s" % (what, nm))


BATCHED_SEP = ["prox_l1_box", "iprox_l1_box", "prox_l0", "prox_l0_box", "iprox_l0_box"]


@pytest.mark.parametrize("n", [1000, 12_289 + 3072])
@pytest.mark.parametrize("op", BATCHED_SEP, ids=["prox", "iprox", "l0-prox", "l0_box-prox", "l0_box-iprox"])
def test_batched_l1_box(s, orc, ctx, op, n):
    """spx_proxstep_l1_box_batch / spx_iproxstep_l1_box_batch, one call, seven rows at seven scales with lambda, l and u on the
    device scaled per row: every row the bits of the single call on that row (and of the oracle), the k = 0 row those of a batch
    of one.  The same for spx_proxstep_l0_batch, spx_proxstep_l0_box_batch and spx_iproxstep_l0_box_batch, lambda scaled by
    c^2: the single call takes NormL0's threshold sqrt(2 lambda sigma) from the host, the batched kernel forms it on the
    device, here at arguments from 2^-1000 to 2^1000; [0] is exactly lambda_b times the count of nonzeros."""
    import torch
    iprox, box = op.startswith("iprox"), op.endswith("_box")
    L = s._lib.load()
    B = s._lib.load_ibatch() if iprox else s._lib.load_batch()
    fn = getattr(B, "spx_%s_%s_batch" % ("iproxstep" if iprox else "proxstep", op.split("_", 1)[1]))
    P0 = scales.separable(op, n, masked=True)
    rows = _rows(P0)
    mask = _dev(P0.mask) if box else None
    assert (P0.mask is not None) == box

    def call(rs):
        nb = len(rs)
        Q, X, S = (_stack(rs, nm) for nm in ("q", "xk", "sj"))
        Y, K = torch.full_like(Q, POISON), torch.full_like(Q, POISON)
        lam = _scalars(rs, "lam")
        lo, up = (_scalars(rs, "l"), _scalars(rs, "u")) if box else (None, None)
        bounds = (_p(lo), _p(up), _p(mask)) if box else ()
        out = torch.full((nb, 4 if iprox else 3), POISON, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        if iprox:
            Dm = _stack(rs, "d")
            rc = fn(ctx, _p(Y), _p(Q), _p(Dm), _p(X), _p(S), n, nb, n, _p(lam), None, *bounds, _p(K), _p(out))
        else:
            sig, qs = _scalars(rs, "sigma"), _dev(np.ones(nb))
            rc = fn(ctx, _p(Y), _p(Q), _p(X), _p(S), n, nb, n, _p(lam), _p(sig), *bounds, _p(qs), _p(K), _p(out))
        _ok(L, rc, op + " batch")
        _ok(L, L.spx_sync(ctx), op + " batch")
        return _host(Y).copy(), _host(K).copy(), _host(out).copy()

    Y, K, out = call(rows)
    for b, P in enumerate(rows):
        what = "%s batch n=%d row %d k=%d" % (op, n, b, P.k)
        V = _SepDev(P)
        ys, ks_, st = _sep_call(L, ctx, V, "step")
        ys, ks_ = _host(ys), _host(ks_)
        assert scales.same_bits(Y[b], ys) and scales.same_bits(K[b], ks_), what
        assert scales.same_bits(Y[b], scales.oracle_y(orc, P)), (what, "against the oracle")
        assert scales.same_bits(scales.unscale(Y[b], P.k), Y[ROW_K.index(0)]), (what, "against the k = 0 row")
        _check_batch_sums(out[b], st, _sep_terms(P, Y[b]), what)
        _check_h(P0.h, float(out[b][0]), scales.oracle_h(orc, P, Y[b]), what + " [0]")      # h over the selected indices
        _check_h(P0.h, st[0], scales.oracle_h(orc, P, Y[b]), what + " single [0]")
        if P0.h == "l0":                                   # lambda_b * count, one rounded product, over the selected indices
            v = (P.xk + P.sj) + Y[b]
            count = int(np.count_nonzero(v if mask is None else v[P0.mask != 0]))
            assert count > 0 and float(out[b][0]) == float(P.lam) * count, (what, float(out[b][0]), float(P.lam), count)
    z = ROW_K.index(0)
    Y1, K1, out1 = call([rows[z]])
    assert scales.same_bits(Y1[0], Y[z]) and scales.same_bits(K1[0], K[z]), "the k = 0 row against a batch of one"
    _check_batch_sums(out1[0], out[z], _sep_terms(rows[z], Y[z]), "batch of one")


@pytest.mark.parametrize("shape", [(8, 125), (128, 8), (8, 1921), (128, 121)], ids=["8x125", "128x8", "8x1921", "128x121"])
@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
def test_batched_groups(s, orc, ctx, binf, shape):
    """spx_proxstep_group_l2_batch / spx_proxstep_group_l2_binf_batch: groups of 8 and 128, n about 1000 (one workgroup per
    problem) and about 15 400 (tiled); seven rows at seven scales, the weights per row (batch x ngroups), sigma and Delta on the
    device.  Rows: the bits of the single call on aligned vectors (group size and row stride are even), the oracle through
    arbiter.check_group, the zero pattern of the oracle AT THAT ROW'S SCALE; the k = 0 row the bits of a batch of one."""
    import torch
    gs, ng = shape
    L = s._lib.load()
    B = s._lib.load_gbinf_batch() if binf else s._lib.load_gbatch()
    P0 = scales.groups(gs, ng, binf)
    n = P0.n
    rows = _rows(P0)
    off = P0.csr()

    def call(rs):
        nb = len(rs)
        Q, X, S, lam = (_stack(rs, nm) for nm in ("q", "xk", "sj", "lam"))
        Y, K = torch.full_like(Q, POISON), torch.full_like(Q, POISON)
        sig, qs = _scalars(rs, "sigma"), _dev(np.ones(nb))
        out = torch.full((nb, 3), POISON, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        if binf:
            dl = _scalars(rs, "delta")
            rc = B.spx_proxstep_group_l2_binf_batch(ctx, _p(Y), _p(Q), _p(X), _p(S), gs, ng, nb, n, _p(lam), ng, None, _p(sig), _p(dl),
                                                    _p(qs), _p(K), _p(out))
        else:
            rc = B.spx_proxstep_group_l2_batch(ctx, _p(Y), _p(Q), _p(X), _p(S), gs, ng, nb, n, _p(lam), ng, None, _p(sig), _p(qs),
                                               _p(K), _p(out))
        _ok(L, rc, "group batch")
        _ok(L, L.spx_sync(ctx), "group batch")
        return _host(Y).copy(), _host(K).copy(), _host(out).copy()

    Y, K, out = call(rows)
    sfx = "_binf" if binf else ""
    for b, P in enumerate(rows):
        what = "group%s batch %dx%d row %d k=%d" % (sfx, gs, ng, b, P.k)
        q, x, sj, lam = _dev(P.q), _dev(P.xk), _dev(P.sj), _dev(P.lam)
        ys, ks_, st = _fresh(n), _fresh(n), (_D * 3)()
        tail = (float(P.delta),) if binf else ()
        _ok(L, getattr(L, "spx_proxstep_group_l2" + sfx)(ctx, _p(ys), _p(q), _p(x), _p(sj), n, None, gs, ng, _p(lam), float(P.sigma), *tail,
                                                        1.0, _p(ks_), st, None), what)
        assert scales.same_bits(Y[b], _host(ys)) and scales.same_bits(K[b], _host(ks_)), what
        ref = scales.oracle_y(orc, P)
        arbiter.check_group(orc, Y[b], ref, P.q, P.xk, P.sj, P.lam, P.sigma, off, delta=P.delta, what=what)
        assert np.array_equal(arbiter.zero_pattern(Y[b], P.xk, P.sj, off), arbiter.zero_pattern(ref, P.xk, P.sj, off)), (what, "zeroed groups")
        _check_batch_sums(out[b], list(st), [("qy", P.q * Y[b]), ("yy", Y[b] * Y[b])], what)
        h = orc.obj_group_l2(Y[b], P.xk, P.sj, P.lam, gsize=gs)
        assert abs(out[b][0] - h) <= TOL * h, (what, out[b][0], h)
    z = ROW_K.index(0)
    Y1, K1, out1 = call([rows[z]])
    assert scales.same_bits(Y1[0], Y[z]) and scales.same_bits(K1[0], K[z]), "the k = 0 row against a batch of one"
    _check_batch_sums(out1[0], out[z], [("qy", rows[z].q * Y[z]), ("yy", Y[z] * Y[z])], "batch of one")


B2_BATCH_FORMS = [("resident", 1000), ("registers", 8192), ("walk", 10_000)]
_B2_BATCH_WORST = {}


@pytest.mark.parametrize("active", [True, False], ids=["active", "inactive"])
@pytest.mark.parametrize("form,n", B2_BATCH_FORMS, ids=[f[0] for f in B2_BATCH_FORMS])
def test_batched_l1_b2(s, orc, ctx, form, n, active):
    """spx_proxstep_l1_b2_batch -- its own root iteration (csrc/spx_b2_row.hpp: delta * delta, r * r * P + C, C / den, the squares
    of the box ends sq -+ ls), not the single call's kernel -- at n = 1000 (a row-resident tile), 8192 (the last n whose row stays
    in registers, 512 lanes) and 10 000 (the row walk): ONE call, seven rows at seven scales, ld = n, lambda, sigma and Delta per
    row on the device.  The bars of _b2_at and of tests/test_gpu_proxstep_b2_batch.py: every row within 1e-12 of
    max(||ref||, ||xk||) of the oracle ON THE SCALED PROBLEM and, unscaled, of the k = 0 row of the same call; xkn the bits of
    (xk + sj) + y; [0] the oracle's objective of that y, [1] and [2] within 1e-12 of sum |term| of math.fsum.  Active rows end
    on the sphere, | ||sj + y|| - Delta | <= 1e-9 Delta; they are NOT held to bits across scales (the kernel squares sq -+ ls,
    which the range condition does not bound from below).  Inactive rows need no sum: the bits of spx_proxstep_l1_b2 on the
    row and of the oracle.  The k = 0 row has the bits of a batch of one in y, xkn and all three sums.
    On the CPU the oracle alone is scale-equivariant bit for bit on all six problems at all seven k, with
    ||sj + y_0|| = 1.0000000000000002, 0.9999999999999978, 1.0000000000000009 (active, Delta = 1) and 24.9, 72.0, 79.3
    (inactive, Delta = 512): it meets every bar here with room to spare."""
    import torch
    L, B = s._lib.load(), s._lib.load_b2_batch()
    P0 = scales.b2(n, active)
    rows = _rows(P0)
    tag = "active" if active else "inactive"

    def call(rs):
        nb = len(rs)
        Q, X, S = (_stack(rs, nm) for nm in ("q", "xk", "sj"))
        Y, K = torch.full_like(Q, POISON), torch.full_like(Q, POISON)
        lam, sig, dl, qs = _scalars(rs, "lam"), _scalars(rs, "sigma"), _scalars(rs, "delta"), _dev(np.ones(nb))
        out = torch.full((nb, 3), POISON, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        rc = B.spx_proxstep_l1_b2_batch(ctx, _p(Y), _p(Q), _p(X), _p(S), n, nb, n, _p(lam), _p(sig), _p(dl), _p(qs), 1.0, _p(K), _p(out))
        _ok(L, rc, "b2 batch")
        _ok(L, L.spx_sync(ctx), "b2 batch")
        return _host(Y).copy(), _host(K).copy(), _host(out).copy()

    Y, K, out = call(rows)
    z = ROW_K.index(0)
    y0 = Y[z]
    bar0 = TOL * max(np.linalg.norm(y0), np.linalg.norm(P0.xk))
    for b, P in enumerate(rows):
        what = "b2 batch %s %s row %d k=%d" % (form, tag, b, P.k)
        y = Y[b]
        ref = scales.oracle_y(orc, P)
        err, bar = float(np.max(np.abs(y - ref))), TOL * max(np.linalg.norm(ref), np.linalg.norm(P.xk))
        _B2_BATCH_WORST[P.k] = max(_B2_BATCH_WORST.get(P.k, 0.0), err / bar)
        print("%s: max |y - oracle| %.3e (bar %.3e, ratio %.3g; worst ratio at this k so far %.3g)" % (what, err, bar, err / bar,
                                                                                                     _B2_BATCH_WORST[P.k]))
        assert np.isfinite(y).all() and err <= bar, (what, err, bar)
        if b != z:
            _note_ulps("l1_b2_batch_%s_%s" % (form, tag), P.k, y, y0)
            dev0 = float(np.max(np.abs(scales.unscale(y, P.k) - y0)))
            assert dev0 <= bar0, (what, "against the k = 0 row", dev0, bar0)
        assert scales.same_bits(K[b], (P.xk + P.sj) + y), (what, "xkn")
        _check_h("l1", float(out[b][0]), orc.obj_plain("l1", y, P.xk, P.sj, P.lam), what + " [0]")
        _check_sum(float(out[b][1]), P.q * y, what + " qy")
        _check_sum(float(out[b][2]), y * y, what + " yy")
        nrm = float(np.linalg.norm(P.sj + y))
        print("%s: ||sj + y|| / Delta %.17g" % (what, nrm / P.delta))
        if active:
            assert abs(nrm - P.delta) <= 1e-9 * P.delta, (what, nrm, P.delta)
        else:
            assert nrm < 0.9 * P.delta, (what, nrm, P.delta)
            q, x, sj = _dev(P.q), _dev(P.xk), _dev(P.sj)
            ys, ks_, st = _fresh(n), _fresh(n), (_D * 3)()
            _ok(L, L.spx_proxstep_l1_b2(ctx, _p(ys), _p(q), _p(x), _p(sj), n, float(P.lam), float(P.sigma), float(P.delta), float(P.chi),
                                        1.0, _p(ks_), st, None), what)
            assert scales.same_bits(y, _host(ys)) and scales.same_bits(K[b], _host(ks_)), (what, "the single call's bits")
            assert scales.same_bits(y, ref), (what, "the oracle's bits")
    Y1, K1, out1 = call([rows[z]])
    assert scales.same_bits(Y1[0], Y[z]) and scales.same_bits(K1[0], K[z]) and scales.same_bits(out1[0], out[z]), \
        "the k = 0 row against a batch of one"
