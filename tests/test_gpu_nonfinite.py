"""Non-finite and extreme data through the fused entry points: spx_proxval_* / spx_proxstep_* (separable), spx_proxval_group_l2[_binf]
/ spx_proxstep_group_l2[_binf], spx_proxval_l1_b2 / spx_proxstep_l1_b2 (include/spx.h, "non-finite data").

Clean data are the seeded vectors of the neighbouring files (tests/nonfinite.py restates them on the host); a plant set overwrites
element 0, the last element (odd n: the scalar tail behind the 16-byte pairs) and an element of another workgroup / tile / group:
none, NaN in q / xk / sj, +Inf / -Inf / both in q, +Inf in xk / sj, `tiny` (+-0, +-5e-324, +-1e-150 over q, xk, sj) and, for the
separable operators, `huge` (+-1e150 in xk) and `large` (+-1e148 in q and sj: a y of that size through <q, y> and <y, y>).
Magnitudes whose squares overflow (1e200, 1e308) are out of scope, and so is 1e150 in q or sj, where y^2 reaches 1e300
(tests/nonfinite.py).

Two private contexts, as tests/test_gpu_proxstep_b2.py: A makes the step calls, B the plain prox! and spx_proxval_* calls through
the same sequence -- clean, planted, clean, clean.  For every call of the sequence:
  1. every return code is 0, spx_sync included: a data NaN is not an abandoned wait;
  2. y of the step call has the bits of the plain prox! (or both are NaN), xkn those of (xk + sj) + y;
  3. [0] has the bits of spx_proxval_*'s value (or both NaN); with device targets the device doubles equal the host ones;
  4. the three sums follow IEEE whatever the order of summation: from the terms formed on the host out of the y the device
     returned -- NaN if a term is NaN or both signs of Inf occur, that Inf if one sign occurs, else finite and within 1e-12 of
     sum |term| of math.fsum (the NormL0 count exactly); [0] has the class of spx_obj_* on that y and of the oracle's obj_*;
  5. y has the oracle's class per element and meets the operator's bar on the finite entries (bits for L1 / L0, LHALF_TOL with the
     Box mask of test_special_values_lhalf, arbiter.check_group on np.where(finite, ., 0), 1e-12 of the nan-aware norms for B2);
  6. on GroupNormL2Binf and L1B2 with +-Inf planted the reference runs its root finder on a non-finite bracket: the outcome of 5.
     is printed per case ("ITEM6 ...") and, since the root of ShiftedNormL1B2 is taken at infinity when chi(y) is +Inf (what
     the reference's bracket doubling ends on), every such case meets 5. in full;
  7. both clean calls after the plant meet every bar above on finite data, and the second repeats the first bit for bit."""
import ctypes
import functools
import hashlib
import math

import numpy as np
import pytest

import arbiter
import nonfinite as nf

pytestmark = pytest.mark.gpu

_D = ctypes.c_double
POISON = -777.25
YFILL = -777.0
VALUE_TOL = 1e-12


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


def _dev(a, align8=False):
    """device copy; align8: the vector starts 8 bytes past a 16-byte boundary"""
    import torch
    t = torch.from_numpy(np.array(a))
    buf = torch.empty(t.numel() + 2, dtype=t.dtype, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()] if (align8 and t.element_size() == 8) else buf[:t.numel()]
    v.copy_(t)
    return v


def _fill(n, align8=False, value=YFILL):
    import torch
    buf = torch.full((n + 2,), value, dtype=torch.float64, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    return buf[1:1 + n] if align8 else buf[:n]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _same(a, b):
    """device vectors: equal int64 bits, or both NaN, at every element (torch.equal is false on NaN)"""
    import torch
    return bool(((a.view(torch.int64) == b.view(torch.int64)) | (a.isnan() & b.isnan())).all())


def _tune(env, key, v):
    s, L, A, B = env
    for c in (A, B):
        s._lib.check(L.spx_ctx_set_tuning(c, key, v))


# ---------------------------------------------------------------------------------------------------------------------
# the three families behind one interface: prox / proxval / step on a context, psi's h part on the device and in the oracle,
# the host terms of [0], the oracle and its bar
# ---------------------------------------------------------------------------------------------------------------------
class Separable:
    family = "separable"

    def __init__(self, env, kind, form, n, lo, up, selected, align8):
        self.env, self.kind, self.form, self.n, self.align8 = env, kind, form, n, align8
        self.box = nf.sep_box(form, lo, up, selected, n)
        self.sel = nf.sep_selected(self.box, n)
        self.factor, self.exact = nf.SEP_LAM, kind == "l0"
        self.root_finder = False
        sfx = kind + ("" if self.box is None else "_box")
        L = env[1]
        self.f_prox, self.f_val, self.f_step = (getattr(L, "spx_%s_%s" % (e, sfx)) for e in ("prox", "proxval", "proxstep"))
        self.f_obj = getattr(L, "spx_obj_" + kind)
        if self.box is None:
            self.tail = ()
        elif self.box[2] is None:
            self.tail = (None, None, _D(self.box[0]), _D(self.box[1]), None)
        else:
            self.keep = (_dev(self.box[0], align8), _dev(self.box[1], align8), _dev(self.box[2]))
            self.tail = (_p(self.keep[0]), _p(self.keep[1]), _D(0.0), _D(0.0), _p(self.keep[2]))
            import torch
            self.sel_d = torch.from_numpy(self.sel).to("cuda:0")

    def _head(self, ctx, y, dv):
        return (ctx, _p(y), _p(dv[0]), _p(dv[1]), _p(dv[2]), self.n, _D(nf.SEP_LAM), _D(nf.SEP_SIGMA), *self.tail)

    def prox(self, ctx, y, dv):
        return self.f_prox(*self._head(ctx, y, dv))

    def proxval(self, ctx, y, dv):
        out = _D(-1.0)
        return self.f_val(*self._head(ctx, y, dv), _D(1.0), ctypes.byref(out)), out.value

    def step(self, ctx, y, dv, xkn, host=True, dev=None):
        st = (ctypes.c_double * 3)(POISON, POISON, POISON) if host else None
        rc = self.f_step(*self._head(ctx, y, dv), _D(1.0), _p(xkn), st, _p(dev))
        return rc, (tuple(st) if host else None)

    def obj_h(self, ctx, y, dv):
        """h over the selected indices of the same y: the unboxed spx_obj_* on the gathered vectors"""
        ys, xs, ss = (y, dv[1], dv[2]) if len(self.sel) == self.n else (t[self.sel_d].contiguous() for t in (y, dv[1], dv[2]))
        out = _D(-1.0)
        self.env[0]._lib.check(self.f_obj(ctx, _p(ys), _p(xs), _p(ss), len(self.sel), _D(nf.SEP_LAM), ctypes.byref(out)))
        return out.value

    def oracle_h(self, orc, y, host):
        q, x, sj = host
        return orc.obj_plain(self.kind, y[self.sel], x[self.sel], sj[self.sel], nf.SEP_LAM)

    def terms(self, v):
        return nf.h_terms(self.kind, v[self.sel])

    def oracle(self, orc, host):
        return nf.sep_oracle(orc, self.kind, self.box, *host)

    def check_oracle(self, orc, y, ref, host, what):
        nf.sep_check(orc, self.kind, self.box, y, ref, *host, what)


class Group:
    family = "group"

    def __init__(self, env, D, align8=False):
        self.env, self.D, self.n, self.align8 = env, D, D.n, align8
        self.factor, self.exact = 1.0, False
        self.ld = _dev(D.lam)
        self.od = _dev(D.offsets) if D.offsets is not None else None
        sfx = "_binf" if D.binf else ""
        L = env[1]
        self.f_prox, self.f_val, self.f_step = (getattr(L, "spx_%s_group_l2%s" % (e, sfx)) for e in ("prox", "proxval", "proxstep"))
        self.tail = (_D(D.delta),) if D.binf else ()
        self.root_finder = D.binf                               # item 6: the reference's root finder on a non-finite bracket

    def _head(self, ctx, y, dv):
        D = self.D
        return (ctx, _p(y), _p(dv[0]), _p(dv[1]), _p(dv[2]), D.n, _p(self.od), D.gsize, D.ng, _p(self.ld), _D(D.sigma), *self.tail)

    def prox(self, ctx, y, dv):
        return self.f_prox(*self._head(ctx, y, dv))

    def proxval(self, ctx, y, dv):
        out = _D(-1.0)
        return self.f_val(*self._head(ctx, y, dv), _D(1.0), ctypes.byref(out)), out.value

    def step(self, ctx, y, dv, xkn, host=True, dev=None):
        st = (ctypes.c_double * 3)(POISON, POISON, POISON) if host else None
        rc = self.f_step(*self._head(ctx, y, dv), _D(1.0), _p(xkn), st, _p(dev))
        return rc, (tuple(st) if host else None)

    def obj_h(self, ctx, y, dv):
        D = self.D
        out = _D(-1.0)
        self.env[0]._lib.check(self.env[1].spx_obj_group_l2(ctx, _p(y), _p(dv[1]), _p(dv[2]), D.n, _p(self.od), D.gsize, D.ng,
                                                            _p(self.ld), ctypes.byref(out)))
        return out.value

    def oracle_h(self, orc, y, host):
        D = self.D
        kw = dict(offsets=D.offsets) if D.offsets is not None else dict(gsize=D.gsize)
        return orc.obj_group_l2(y, host[1], host[2], D.lam, **kw)

    def terms(self, v):
        return nf.group_terms(v, self.D.lam, self.D.starts, self.D.sizes)

    def oracle(self, orc, host):
        return self.D.oracle(orc, *host, y0=YFILL)

    def check_oracle(self, orc, y, ref, host, what):
        D = self.D
        v = nf.check_group(orc, arbiter, y, ref, *host, D.lam, D.sigma, D.csr, D.delta if D.binf else None, what)
        print(what, v)


B2_LAM = B2_SIGMA = B2_CHI = 1.0


class B2:
    family = "b2"

    def __init__(self, env, n, delta, align8):
        self.env, self.n, self.delta, self.align8 = env, n, delta, align8
        self.factor, self.exact = B2_LAM, False
        self.root_finder = True                                 # item 6

    def _head(self, ctx, y, dv):
        return (ctx, _p(y), _p(dv[0]), _p(dv[1]), _p(dv[2]), self.n, _D(B2_LAM), _D(B2_SIGMA), _D(self.delta), _D(B2_CHI))

    def prox(self, ctx, y, dv):
        return self.env[1].spx_prox_l1_b2(*self._head(ctx, y, dv))

    def proxval(self, ctx, y, dv):
        out = _D(-1.0)
        return self.env[1].spx_proxval_l1_b2(*self._head(ctx, y, dv), _D(1.0), ctypes.byref(out)), out.value

    def step(self, ctx, y, dv, xkn, host=True, dev=None):
        st = (ctypes.c_double * 3)(POISON, POISON, POISON) if host else None
        rc = self.env[1].spx_proxstep_l1_b2(*self._head(ctx, y, dv), _D(1.0), _p(xkn), st, _p(dev))
        return rc, (tuple(st) if host else None)

    def obj_h(self, ctx, y, dv):
        """the h part, lambda ||xk + sj + y||_1, as tests/test_gpu_proxval_b2.py takes it: spx_obj_l1"""
        out = _D(-1.0)
        self.env[0]._lib.check(self.env[1].spx_obj_l1(ctx, _p(y), _p(dv[1]), _p(dv[2]), self.n, _D(B2_LAM), ctypes.byref(out)))
        return out.value

    def oracle_h(self, orc, y, host):
        return orc.obj_plain("l1", y, host[1], host[2], B2_LAM)

    def terms(self, v):
        return np.abs(v)

    def oracle(self, orc, host):
        with np.errstate(all="ignore"):
            return orc.prox_l1_b2(*host, B2_LAM, B2_SIGMA, self.delta, B2_CHI)

    def check_oracle(self, orc, y, ref, host, what):
        nf.check_b2(y, ref, host[1], what)


# ---------------------------------------------------------------------------------------------------------------------
# one sequence: clean, planted, clean, clean
# ---------------------------------------------------------------------------------------------------------------------
def _value_close(got, exp, exact):
    return got == exp if exact else abs(got - exp) <= VALUE_TOL * max(abs(exp), 1e-300)


# The host side of 4.-6. (three math.fsum over the vector, the oracle's bars, and the spx_obj_* call whose class they need) is a
# function of the problem's data and of the bits the device returned.  Most calls of this file return bits another call on the
# same problem has returned -- the clean calls of every sequence, the same problem at the other alignment or with the other
# reference on B -- and repeating the host side for them would only cost wall time (B2 at n = 300 001: 0.5 s a call).  Items 1.-3.
# and 7., which compare device results with each other, run on every call.
_VERIFIED = set()   # (problem, call kind, digest of y, bits of the triple) of the calls whose host side has passed


def _run_sequence(env, orc, fam, clean, planted, plant, what, refs, problem, reference="both"):
    """clean / planted: host (q, xk, sj).  refs: {"clean": y, "planted": y} of the oracle (computed once by the caller, never
    modified).  reference: what B calls -- "prox", "proxval" or "both" (B2: one kind per run, the regime word follows the calls).
    problem: a key that names the operator and the data; a call that returns the very bits (y and triple) another call on the same
    problem returned is not checked on the host a second time.  Returns the planted call's (y, xkn, triple)."""
    import torch
    s, L, A, B = env
    keep = None
    for k, (name, host) in enumerate((("clean", clean), ("planted", planted), ("clean", clean), ("clean", clean))):
        w = "%s call %d (%s)" % (what, k + 1, name)
        q, x, sj = host
        dv = tuple(_dev(v, fam.align8) for v in host)
        ya, xkn = _fill(fam.n, fam.align8), _fill(fam.n, fam.align8, POISON)
        rc, st = fam.step(A, ya, dv, xkn)
        assert rc == 0, (w, rc, L.spx_last_error())                                            # 1.
        if reference in ("prox", "both"):
            yb = _fill(fam.n, fam.align8)
            rc = fam.prox(B, yb, dv)
            assert rc == 0, (w, rc, L.spx_last_error())
            assert _same(ya, yb), w                                                            # 2.
        if reference in ("proxval", "both"):
            yv = _fill(fam.n, fam.align8)
            rc, val = fam.proxval(B, yv, dv)
            assert rc == 0, (w, rc, L.spx_last_error())
            assert _same(ya, yv), w
            print("%s: [0] %r proxval %r" % (w, st[0], val))
            assert nf.scalar_same(st[0], val), (w, st[0], val)                                 # 3.
        assert _same(xkn, (dv[1] + dv[2]) + ya), w
        yh = ya.cpu().numpy()
        if name == "clean":                                                                    # 7.
            assert np.isfinite(yh).all() and all(math.isfinite(t) for t in st), (w, st)
        if k == 1:
            planted_out = (ya, xkn, st)
        if k == 2:
            keep = (ya, xkn, st)
        if k == 3:
            assert torch.equal(ya, keep[0]) and torch.equal(xkn, keep[1]) and nf.triple_same(st, keep[2]), (w, st, keep[2])
        done = (problem, name, hashlib.sha1(yh.tobytes()).digest(), np.array(st).tobytes())
        if done in _VERIFIED:
            continue
        # 4. the sums from the y the device returned
        nf.check_qy_yy(q, yh, st[1], st[2], w)
        with np.errstate(all="ignore"):
            v = (x + sj) + yh
        cls = nf.check_sum(st[0], fam.terms(v), w + " [0]", factor=fam.factor, exact=fam.exact)
        dobj, oobj = fam.obj_h(B, ya, dv), fam.oracle_h(orc, yh, host)
        print("%s: [0] %r spx_obj %r oracle obj %r" % (w, st[0], dobj, oobj))
        assert nf.scalar_class(dobj) == cls and nf.scalar_class(oobj) == cls, (w, cls, dobj, oobj)
        if cls == "finite":
            assert _value_close(st[0], dobj, fam.exact) and _value_close(st[0], oobj, fam.exact), (w, st[0], dobj, oobj)
        # 5. / 6. the oracle
        fam.check_oracle(orc, yh, refs[name], host, w)
        if name == "planted" and plant in nf.INF_PLANTS and fam.root_finder:
            print("ITEM6 %s %s: full" % (fam.family, w))       # (+-Inf through a root finder: met in full, or the line above failed)
        _VERIFIED.add(done)
    assert L.spx_sync(A) == 0 and L.spx_sync(B) == 0, what                                     # 1.
    return planted_out


# ---------------------------------------------------------------------------------------------------------------------
# separable
# ---------------------------------------------------------------------------------------------------------------------
SEP_SIZES = [3, 1537, 3073, 6145]


@functools.lru_cache(maxsize=None)
def _sep_case(n, plant):
    x, sj, q, lo, up, selected = nf.separable_data(n, 7700 + n)
    # 2n/3: n = 6145 -> 4096, the second workgroup with scalar bounds (3072 each) and the third with vector bounds (1536 each);
    # n = 3073 -> 2048, the second workgroup with vector bounds; elsewhere (n = 1537; n = 3073 with scalar bounds) the last
    # element alone lies in the second workgroup
    pos = nf.positions(n, [(2 * n) // 3])
    qp, xp, sp = nf.plant(plant, q, x, sj, pos)
    for v in (x, sj, q, lo, up):
        v.setflags(write=False)
    return (q, x, sj), (qp, xp, sp), lo, up, tuple(selected)


@pytest.mark.parametrize("plant", nf.PLANTS_SEPARABLE)
@pytest.mark.parametrize("align8", [False, True], ids=["a16", "a8"])
@pytest.mark.parametrize("n", SEP_SIZES)
def test_separable(env, orc, n, align8, plant):
    """the six operators in the three constructions of _nine, on the LDS-staged and the register-staged skeleton (key 3), key 17
    at 1 and 0: the sequence on each, and the planted call's y, xkn and triple with equal bits (or both NaN) between key 17 = 0
    and 1"""
    clean, planted, lo, up, selected = _sep_case(n, plant)
    try:
        for kind, form in nf.SEP_OPS:
            fam = Separable(env, kind, form, n, lo, up, selected, align8)
            refs = {"clean": fam.oracle(orc, clean), "planted": fam.oracle(orc, planted)}
            for k3 in (1, 0):
                _tune(env, 3, k3)
                got = {}
                for k17 in (1, 0):
                    _tune(env, 17, k17)
                    what = "%s %s n %d a8 %d %s key3 %d key17 %d" % (kind, form, n, align8, plant, k3, k17)
                    got[k17] = _run_sequence(env, orc, fam, clean, planted, plant, what, refs, ("sep", kind, form, n, plant))
                assert _same(got[0][0], got[1][0]) and _same(got[0][1], got[1][1]), (kind, form, k3)
                assert nf.triple_same(got[0][2], got[1][2]), (kind, form, k3, got[0][2], got[1][2])
    finally:
        _tune(env, 17, 1)
        _tune(env, 3, 1)


def test_separable_lattice(env):
    """the 17^3 lattice of test_special_values_separable (every combination of +-0, +-Inf, NaN, subnormals, 1e308, thresholds in
    q, xk, sj) through spx_proxstep_l1, _l0, _l1_box, _l0_box: y and xkn as the plain prox! gives them (item 2); the three sums
    are NaN by construction"""
    s, L, A, B = env
    vals = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1e308, -1e308,
                     np.sqrt(2.0), -np.sqrt(2.0), np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)])
    Q, X, S = (g.ravel().copy() for g in np.meshgrid(vals, vals, vals, indexing="ij"))
    n = Q.size
    dv = (_dev(Q), _dev(X), _dev(S))
    for sfx, tails in (("l1", [()]), ("l0", [()]),
                       ("l1_box", [(None, None, _D(lo), _D(up), None) for lo, up in ((-1.0, 1.0), (0.0, 0.0), (-np.inf, np.inf), (-0.0, 2.0))]),
                       ("l0_box", [(None, None, _D(lo), _D(up), None) for lo, up in ((-1.0, 1.0), (0.0, 0.0), (-np.inf, np.inf), (-0.0, 2.0))])):
        for tail in tails:
            head = lambda ctx, y: (ctx, _p(y), _p(dv[0]), _p(dv[1]), _p(dv[2]), n, _D(1.0), _D(1.0), *tail)
            ya, xkn, yb = _fill(n), _fill(n, value=POISON), _fill(n)
            st = (ctypes.c_double * 3)(POISON, POISON, POISON)
            assert getattr(L, "spx_proxstep_" + sfx)(*head(A, ya), _D(1.0), _p(xkn), st, None) == 0, sfx
            assert getattr(L, "spx_prox_" + sfx)(*head(B, yb)) == 0, sfx
            assert _same(ya, yb) and _same(xkn, (dv[1] + dv[2]) + ya), sfx
            print(sfx, tuple(st))
            assert math.isnan(st[1]) and math.isnan(st[2]), (sfx, tuple(st))
            if sfx.startswith("l1"):
                assert math.isnan(st[0]), (sfx, tuple(st))         # (the NormL0 value is a count: always finite)
            else:
                assert math.isfinite(st[0]), (sfx, tuple(st))
    assert L.spx_sync(A) == 0 and L.spx_sync(B) == 0


# ---------------------------------------------------------------------------------------------------------------------
# groups
# ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = [("uniform", g) for g in (3, 16, 128, 300, 1024, 5000)] + [("csr_bound", 0), ("csr_over", 0), ("one", 1000), ("one", 20_001)]
# (layout, binf, key 9, key 8).  Key 8 = 4 on one group of 50 001: a team of four workgroups whose LDS holds 36 864 elements, so the
# group is STREAMED -- plain: the generic streaming form; Binf: the sample-predicted fast form (binf_team_fast) and, for what
# that leaves undecided, the generic one.  (One group of 20 001 at key 8 = 0 is a team on chip.)
GROUP_CASES = ([(lay, False, 0, 0) for lay in LAYOUTS] + [(lay, True, 0, 0) for lay in LAYOUTS] + [(("uniform", 16), True, 1, 0)] +
               [(("one", 50_001), False, 0, 4), (("one", 50_001), True, 0, 4)])
_gid = lambda c: "%s%s-%s%s%s" % (c[0][0], c[0][1] or "", "binf" if c[1] else "plain", "-key9" if c[2] else "", "-key8" if c[3] else "")


@functools.lru_cache(maxsize=None)
def _group_case(layout, binf):
    from oracle import oracle as orc
    D = nf.GroupData(layout, binf)
    for v in (D.x, D.sj, D.q, D.lam):
        v.setflags(write=False)
    y_clean = D.oracle(orc, D.q, D.x, D.sj, y0=YFILL)
    pos, gz, gsh = D.plant_positions(arbiter, y_clean)
    if D.ng > 1:            # one plant in a group the prox zeroes, one in a group it shrinks -- on the clean data
        zp = arbiter.zero_pattern(y_clean, D.x, D.sj, D.csr)
        assert zp[gz] and not zp[gsh] and gsh != 0
    y_clean.setflags(write=False)
    return D, y_clean, pos


@pytest.mark.parametrize("plant", nf.PLANTS)
@pytest.mark.parametrize("case", GROUP_CASES, ids=[_gid(c) for c in GROUP_CASES])
def test_group(env, orc, case, plant):
    layout, binf, key9, key8 = case
    D, y_clean, pos = _group_case(layout, binf)
    _group_run(env, orc, D, y_clean, pos, plant, key9, key8, "group %s %s" % (_gid(case), plant), ("group", case, plant))


def _group_run(env, orc, D, y_clean, pos, plant, key9, key8, what, problem):
    clean = (D.q, D.x, D.sj)
    planted = tuple(nf.plant(plant, D.q, D.x, D.sj, pos))
    fam = Group(env, D)
    refs = {"clean": y_clean, "planted": fam.oracle(orc, planted)}
    try:
        _tune(env, 9, key9)
        _tune(env, 8, key8)
        _run_sequence(env, orc, fam, clean, planted, plant, what, refs, problem)
    finally:
        _tune(env, 8, 0)
        _tune(env, 9, 0)


@pytest.mark.parametrize("plant", ["none", "nan-q", "nan-sj", "pinf-q", "tiny"])
@pytest.mark.parametrize("n,key8", [(50_001, 4), (20_001, 0), (1_000, 0)], ids=["team-streamed", "team-on-chip", "one-workgroup"])
def test_group_binf_zero_iterate(env, orc, n, key8, plant):
    """One Binf group with xk == 0 throughout -- the first iterate of a run -- and sigma lambda = 2 ||S||: the group every form
    zeroes by its `X == 0` shortcut, before any bracket is formed.  A NaN in q or sj must still make the whole group NaN: the
    shortcut compares with ||S||, and the kernels' sqrt_pos gives 0 for a NaN sum."""
    D = nf.GroupData(("one", n), True)
    D.x = np.zeros(n)
    D.lam = np.array([2.0 * float(np.linalg.norm(D.q + D.sj)) / D.sigma])
    y_clean = D.oracle(orc, D.q, D.x, D.sj, y0=YFILL)
    assert np.array_equal(y_clean, -(D.x + D.sj))              # zeroed on the clean data
    pos = nf.positions(n, [(2 * n) // 3])
    if plant.startswith("nan"):
        assert np.isnan(D.oracle(orc, *nf.plant(plant, D.q, D.x, D.sj, pos))).all()
    _group_run(env, orc, D, y_clean, pos, plant, 0, key8, "binf zero iterate n %d %s" % (n, plant), ("zero-iterate", n, plant))


# ---------------------------------------------------------------------------------------------------------------------
# B2
# ---------------------------------------------------------------------------------------------------------------------
ACTIVE, INACTIVE = 1.0, 1e6
B2_SIZES = [3, 1_000, 20_001, 50_001, 70_001, 300_001]      # key 8 = 4: register, register, register, LDS, streaming, many tiles
B2_CASES = [(n, a8, 0) for n in B2_SIZES for a8 in (False, True)] + [(n, False, 1) for n in (20_001, 50_001, 70_001, 300_001)]
_bid = lambda c: "n%d-%s%s" % (c[0], "a8" if c[1] else "a16", "-key18" if c[2] else "")


@functools.lru_cache(maxsize=None)
def _b2_case(n, plant, delta):
    from oracle import oracle as orc
    x, sj, q = nf.b2_data(n)
    for v in (x, sj, q):
        v.setflags(write=False)
    pos = nf.positions(n, [(2 * n) // 3])          # (four workgroups: the third one's share)
    planted = tuple(nf.plant(plant, q, x, sj, pos))
    with np.errstate(all="ignore"):
        refs = {"clean": orc.prox_l1_b2(q, x, sj, B2_LAM, B2_SIGMA, delta, B2_CHI),
                "planted": orc.prox_l1_b2(*planted, B2_LAM, B2_SIGMA, delta, B2_CHI)}
    for v in refs.values():
        v.setflags(write=False)
    return (q, x, sj), planted, refs


@pytest.mark.parametrize("reference", ["prox", "proxval"])
@pytest.mark.parametrize("delta", [ACTIVE, INACTIVE], ids=["active", "inactive"])
@pytest.mark.parametrize("plant", nf.PLANTS)
@pytest.mark.parametrize("case", B2_CASES, ids=[_bid(c) for c in B2_CASES])
def test_b2(env, orc, case, plant, delta, reference):
    """the sequence with the clean calls at Delta active and at Delta inactive: the plant lands between both kinds of speculation
    (SpxSyncHeader::b2_last_scaled); B follows with the plain prox! in one run and with spx_proxval_l1_b2 in another, so that the
    regime word is the same on both contexts.  Both are put into the same state first (one inactive plain prox! each)."""
    n, align8, key18 = case
    s, L, A, B = env
    clean, planted, refs = _b2_case(n, plant, delta)
    fam = B2(env, n, delta, align8)
    try:
        _tune(env, 8, 4)
        s._lib.check(L.spx_ctx_set_tuning(A, 18, key18))
        warm = B2(env, n, INACTIVE, align8)
        dv = tuple(_dev(v, align8) for v in clean)
        for c in (A, B):
            assert warm.prox(c, _fill(n, align8), dv) == 0
        _run_sequence(env, orc, fam, clean, planted, plant, "b2 %s %s delta %g vs %s" % (_bid(case), plant, delta, reference),
                      refs, ("b2", n, plant, delta), reference=reference)
    finally:
        s._lib.check(L.spx_ctx_set_tuning(A, 18, 0))
        _tune(env, 8, 0)


# ---------------------------------------------------------------------------------------------------------------------
# device targets: one planted case per family
# ---------------------------------------------------------------------------------------------------------------------
def _targets(env, fam, planted, what):
    """stats_dev and spx_ctx_set_value_target: the device doubles are the host-valued call's, NaN for NaN"""
    import torch
    s, L, A, B = env
    dv = tuple(_dev(v, fam.align8) for v in planted)
    n = fam.n
    assert fam.step(A, _fill(n, fam.align8), dv, None)[0] == 0 and fam.proxval(B, _fill(n, fam.align8), dv)[0] == 0   # (B2: the regime)
    y0, k0 = _fill(n, fam.align8), _fill(n, fam.align8, POISON)
    rc, want = fam.step(A, y0, dv, k0)
    assert rc == 0
    for host in (True, False):
        out = torch.full((5,), POISON, dtype=torch.float64, device="cuda:0")
        y, xkn = _fill(n, fam.align8), _fill(n, fam.align8, POISON)
        rc, st = fam.step(A, y, dv, xkn, host=host, dev=out)
        assert rc == 0, (what, rc)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        print("%s: host %r device %r" % (what, want, got[:3].tolist()))
        assert nf.triple_same(got[:3], want) and got[3] == POISON and got[4] == POISON, (what, got, want)
        assert _same(y, y0) and _same(xkn, k0), what
        if host:
            assert nf.triple_same(st, want), (what, st, want)
    yv = _fill(n, fam.align8)
    rc, val = fam.proxval(B, yv, dv)
    assert rc == 0
    tgt = torch.full((2,), POISON, dtype=torch.float64, device="cuda:0")
    try:
        s._lib.check(L.spx_ctx_set_value_target(B, _p(tgt)))
        yt = _fill(n, fam.align8)
        rc, hv = fam.proxval(B, yt, dv)
        assert rc == 0 and math.isnan(hv), (what, rc, hv)
        torch.cuda.synchronize()
    finally:
        s._lib.check(L.spx_ctx_set_value_target(B, None))
    got = tgt.cpu().numpy()
    print("%s: proxval host %r device %r step [0] %r" % (what, val, got[0], want[0]))
    assert nf.scalar_same(got[0], val) and got[1] == POISON and _same(yt, yv), (what, got, val)
    assert L.spx_sync(A) == 0 and L.spx_sync(B) == 0
    return want


@pytest.mark.parametrize("plant", ["nan-q", "pinf-sj"])
def test_device_targets_separable(env, plant):
    n = 3073
    clean, planted, lo, up, selected = _sep_case(n, plant)
    for kind, form in (("l1", "plain"), ("lhalf", "vecbox+mask")):
        want = _targets(env, Separable(env, kind, form, n, lo, up, selected, False), planted, "targets %s %s %s" % (kind, form, plant))
        assert not all(math.isfinite(t) for t in want), want      # (a planted case: something non-finite does travel)


@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
@pytest.mark.parametrize("layout", [("uniform", 16), ("uniform", 1024)], ids=["fused", "composed"])
def test_device_targets_group(env, layout, binf):
    D, y_clean, pos = _group_case(layout, binf)
    planted = tuple(nf.plant("nan-q", D.q, D.x, D.sj, pos))
    want = _targets(env, Group(env, D), planted, "targets group %s binf %d" % (layout, binf))
    assert all(math.isnan(t) for t in want), want


@pytest.mark.parametrize("n", [20_001, 70_001], ids=["reg", "stream"])
def test_device_targets_b2(env, n):
    s, L, A, B = env
    clean, planted, refs = _b2_case(n, "nan-q", ACTIVE)
    fam = B2(env, n, ACTIVE, False)
    try:
        _tune(env, 8, 4)
        dv = tuple(_dev(v) for v in clean)
        for c in (A, B):
            assert fam.prox(c, _fill(n), dv) == 0
        want = _targets(env, fam, planted, "targets b2 n %d" % n)
    finally:
        _tune(env, 8, 0)
    assert all(math.isnan(t) for t in want), want


# ---------------------------------------------------------------------------------------------------------------------
# the Python mirror, one planted case per family; the clean data are the neighbours'
# ---------------------------------------------------------------------------------------------------------------------
def _mirror_check(s, psi, step_bang, host, what, n):
    """step / prox_value / prox of the mirror on planted data: y and xkn by bits or both NaN, [0] the bits of prox_value's value,
    the sums by the IEEE rule.  Every call follows a call on the same data (ShiftedNormL1B2: the same regime)."""
    import torch
    q, x, sj = host
    qd = torch.from_numpy(np.array(q)).to("cuda:0")
    step_bang(torch.empty_like(qd), psi, qd, 1.1)                                  # (the regime)
    y, xkn = torch.full_like(qd, YFILL), torch.full_like(qd, POISON)
    _, h, qy, yy = step_bang(y, psi, qd, 1.1, xkn=xkn)
    yv, val = s.prox_value_bang(torch.full_like(qd, YFILL), psi, qd, 1.1)
    yp = s.prox_bang(torch.full_like(qd, YFILL), psi, qd, 1.1)
    print("%s: mirror (%r, %r, %r) prox_value %r" % (what, h, qy, yy, val))
    assert _same(y, yv) and _same(y, yp), what
    assert _same(xkn, (torch.from_numpy(np.array(x)).cuda() + torch.from_numpy(np.array(sj)).cuda()) + y), what
    assert nf.scalar_same(h, val), (what, h, val)
    out = torch.full((3,), POISON, dtype=torch.float64, device="cuda:0")
    y2, o = step_bang(torch.full_like(qd, YFILL), psi, qd, 1.1, out=out)
    assert _same(y2, y) and nf.triple_same(out.cpu().numpy(), (h, qy, yy)), (what, out, (h, qy, yy))
    yh = y.cpu().numpy()
    nf.check_qy_yy(q, yh, qy, yy, what)
    assert s._lib.load().spx_sync(s.context("cuda:0")) == 0
    return yh, h


@pytest.mark.parametrize("plant", ["nan-q", "pminf-q"])
def test_mirror(env, orc, plant):
    import torch
    s = env[0]
    dev = lambda a: torch.from_numpy(np.array(a)).to("cuda:0")
    # separable: ShiftedNormL1 with vector bounds and a mask
    n = 3073
    clean, planted, lo, up, selected = _sep_case(n, plant)
    psi = s.shifted(s.shifted(s.NormL1(nf.SEP_LAM), dev(planted[1]), dev(lo), dev(up), list(selected)), dev(planted[2]))
    yh, h = _mirror_check(s, psi, s.prox_step_bang, planted, "mirror l1 vecbox+mask %s" % plant, n)
    box = nf.sep_box("vecbox+mask", lo, up, selected, n)
    nf.sep_check(orc, "l1", box, yh, nf.sep_oracle(orc, "l1", box, *planted), *planted, "mirror l1 " + plant)
    with np.errstate(all="ignore"):
        nf.check_sum(h, nf.h_terms("l1", ((planted[1] + planted[2]) + yh)[nf.sep_selected(box, n)]), "mirror l1 [0]", factor=nf.SEP_LAM)
    # groups: plain, uniform 16 (fused) and 1024 (composed)
    for layout in (("uniform", 16), ("uniform", 1024)):
        D, y_clean, pos = _group_case(layout, False)
        gp = tuple(nf.plant(plant, D.q, D.x, D.sj, pos))
        psi = s.shifted(s.shifted(s.GroupNormL2.uniform(dev(D.lam), D.gsize), dev(gp[1])), dev(gp[2]))
        _mirror_check(s, psi, s.group_prox_step_bang, gp, "mirror group %s %s" % (layout, plant), D.n)
    # B2, register form
    n = 20_001
    bclean, bplanted, refs = _b2_case(n, plant, ACTIVE)
    psi = s.shifted(s.shifted(s.NormL1(B2_LAM), dev(bplanted[1]), ACTIVE, s.NormL2(B2_CHI)), dev(bplanted[2]))
    assert type(psi).__name__ == "ShiftedNormL1B2"
    _mirror_check(s, psi, s.b2_prox_step_bang, bplanted, "mirror b2 %s" % plant, n)


def test_clean_data_are_the_neighbours(env):
    """tests/nonfinite.py restates the data of the neighbouring files on the host (their constructors need a device): the same
    vectors, weights and offsets, so that a change there shows here"""
    import test_gpu_proxstep as T1
    import test_gpu_proxstep_b2 as T2
    import test_gpu_proxstep_group as T3
    for a, b in zip(nf.separable_data(1537, 11), T1._data(1537, 11)):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for a, b in zip(nf.b2_data(1_000), T2._data(1_000)):
        assert np.array_equal(a, b)
    for layout, binf in ((("uniform", 16), True), (("csr_over", 0), False), (("one", 1000), True)):
        P, D = T3.Problem(env[0], layout, binf), nf.GroupData(layout, binf)
        for name in ("x", "sj", "q", "lam"):
            assert np.array_equal(getattr(P, name), getattr(D, name)), (layout, name)
        assert (P.n, P.ng, P.gsize, P.sigma, P.delta) == (D.n, D.ng, D.gsize, D.sigma, D.delta)
        assert (P.offsets is None) == (D.offsets is None) and (P.offsets is None or np.array_equal(P.offsets, D.offsets))
