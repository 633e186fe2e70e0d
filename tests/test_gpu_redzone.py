"""Every kernel form on guarded buffers (tests/redzone.py): the oracle comparison of the interior, then check() on every buffer
the call was given -- guards intact, read-only inputs bit-identical, no output element left holding the poison.

The C ABI is driven through ctypes on ONE private context (created here, destroyed at teardown) bound to torch's current stream,
so that the tuning keys set per case never reach another module.  The flat case list interleaves the operator families: every
case runs on a workspace that another family has just left dirty, as a real caller's does.  Nothing fills the workspace.

Sizes sit on both sides of each dispatch boundary (the comments name it); alignment modes for Float64 (redzone.F64_MODES):
A all vectors 16-byte aligned (the vec forms), B all at +8 B (the ioff forms of top-r, the 8-byte forms elsewhere), C y aligned
and the inputs at +8 B (non-vec, non-ioff forms), D y aliases q.  Float32 vectors sit at +0, +4, +8, +12 B.

The Float32 psi(y) and group prox cases are held to the Float32 restatement of the oracle with the bars of tests/f32_exact.py
(check_sum at 1e-12 of sum |term|; the bit rule); tests/test_gpu_f32_exact.py runs those entry points at every size and edge."""
import ctypes
import itertools
import zlib

import numpy as np
import pytest

import arbiter
import f32_exact
import nonfinite
import redzone

pytestmark = pytest.mark.gpu

GROUP_TOL = 1e-12
_D = ctypes.c_double
_F = ctypes.c_float


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
        L.spx_ctx_destroy(ctx)


class Case:
    """One call on guarded buffers: `run(c)` gets this object (c.L, c.ctx, c.orc, c.zone, c.tune(key, value))."""

    def __init__(self, env, orc):
        import torch
        self.torch = torch
        self.s, self.L, self.ctx = env
        self.orc = orc
        self.zone = redzone.Zone()
        self.keys = []

    def tune(self, key, value):
        self.s._lib.check(self.L.spx_ctx_set_tuning(self.ctx, key, value))
        self.keys.append(key)

    def call(self, name, *args):
        self.torch.cuda.synchronize()
        rc = getattr(self.L, name)(self.ctx, *args)
        self.torch.cuda.synchronize()
        self.s._lib.check(rc)

    def vec(self, data, align=0, dtype=None, role="in", name=None):
        t = self.torch
        dtype = dtype or (t.float32 if np.asarray(data).dtype == np.float32 else t.float64)
        return self.zone.add(len(data), dtype, align, data=np.ascontiguousarray(data), role=role, name=name)

    def out(self, n, align=0, dtype=None, name="y"):
        return self.zone.add(n, dtype or self.torch.float64, align, role="out", name=name)

    def ints(self, data, nvec, name):
        return self.zone.add(len(data), self.torch.int64, 0, data=np.asarray(data, dtype=np.int64), poison=max(nvec // 3, 0),
                             name=name)

    def u8(self, data, name="mask"):
        return self.zone.add(len(data), self.torch.uint8, 0, data=np.asarray(data, dtype=np.uint8), name=name)

    def finish(self):
        self.zone.check()
        # the defaults of every key this case moved (a context fresh from spx_ctx_create)
        defaults = {2: 1, 3: 1, 4: 1, 11: 1, 12: 1, 13: 1, 14: 1, 17: 1}
        for k in set(self.keys):
            self.s._lib.check(self.L.spx_ctx_set_tuning(self.ctx, k, defaults[k]))


def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def _data(n, tag, quant=None):
    rng = _rng(tag)
    x = rng.normal(size=n)
    sj = rng.uniform(-0.5, 0.5, size=n)
    q = rng.normal(size=n)
    if quant:
        x, sj, q = (np.round(v * quant) / quant for v in (x, sj, q))
    return x, sj, q


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _yq(c, q, mode, n, dtype=None):
    """(y, q) guarded buffers for a float64 mode (D: y is q's buffer)"""
    ay, ai = redzone.F64_MODES[mode]
    if mode == "D":
        qb = c.vec(q, ai, dtype, role="inout", name="q=y")
        return qb, qb
    return c.out(n, ay, dtype), c.vec(q, ai, dtype, name="q")


# ================================================================== separable (run_separable, spx_separable.hip)
SEP_SIZES = [1, 2, 3, 63, 65, 3071, 3072, 3073, 6145, 1_000_003]   # a k_sep_lds workgroup: 256 lanes x 6 pairs = 3072


def _sep_cases():
    out = []
    for op, n, mode in itertools.product(("l1", "l0", "lhalf", "l1_box", "l0_box", "lhalf_box"), SEP_SIZES, "ABCD"):
        staged = [1, 0] if mode in "AC" and n >= 3071 and op in ("l1", "l1_box", "lhalf_box") else [1]
        for lds in staged:
            out.append(("sep-%s-n%d-%s-lds%d" % (op, n, mode, lds), lambda c, op=op, n=n, mode=mode, lds=lds: _sep(c, op, n, mode, lds)))
    return out


def _sep(c, op, n, mode, lds):
    tag = "sep%s%d%s" % (op, n, mode)
    x, sj, q = _data(n, tag)
    rng = _rng(tag + "b")
    lam, sigma = 0.7, 0.9
    if lds == 0:
        c.tune(3, 0)
    ai = redzone.F64_MODES[mode][1]
    y, qb = _yq(c, q, mode, n)
    xb, sb = c.vec(x, ai, name="xk"), c.vec(sj, ai, name="sj")
    if op.endswith("_box"):
        vector_bounds = mode in "AB"
        if vector_bounds:
            l = rng.uniform(-1.5, -0.2, size=n); u = rng.uniform(0.2, 1.5, size=n)
            mask = (rng.random(n) < 0.7).astype(np.uint8)
            lb, ub, mb = c.vec(l, ai, name="l"), c.vec(u, ai, name="u"), c.u8(mask)
            args = (lb.ptr(), ub.ptr(), _D(0.0), _D(0.0), mb.ptr())
        else:
            l, u, mask = -0.8, 0.9, None
            args = (None, None, _D(l), _D(u), None)
        c.call("spx_prox_" + op, y.ptr(), qb.ptr(), xb.ptr(), sb.ptr(), n, _D(lam), _D(sigma), *args)
        ref = getattr(c.orc, "prox_" + op)(q, x, sj, lam, sigma, l, u, mask)
    else:
        c.call("spx_prox_" + op, y.ptr(), qb.ptr(), xb.ptr(), sb.ptr(), n, _D(lam), _D(sigma))
        ref = getattr(c.orc, "prox_" + op)(q, x, sj, lam, sigma)
        if op == "l1" and mode == "D":   # ShiftedNormL1 with y === q: the reference's two-pass body reads the overwritten q
            ref = (-x) - sj
    got = y.t.cpu().numpy()
    if op.startswith("lhalf"):
        if not _bits(got, ref):
            box = (l, u) if op.endswith("_box") else None
            arbiter.check_lhalf(c.orc, got, ref, q, x, sj, lam, sigma, box=box, mask=mask if box else None, what=op)
    else:
        assert _bits(got, ref), (op, n, mode, int(np.sum(got != ref)))
    c.finish()


# ================================================================== iprox!, prox! + value
def _iprox_cases():
    out = []
    for op, n, mode in itertools.product(("l1", "l0", "l1_box", "l0_box"), (1, 65, 3073, 1_000_003), "ABC"):
        out.append(("iprox-%s-n%d-%s" % (op, n, mode), lambda c, op=op, n=n, mode=mode: _iprox(c, op, n, mode)))
    for op, n, target in itertools.product(("l1", "l0", "lhalf", "l1_box"), (65, 6145, 1_000_003), ("host", "device")):
        out.append(("proxval-%s-n%d-%s" % (op, n, target), lambda c, op=op, n=n, t=target: _proxval(c, op, n, t)))
    return out


def _iprox(c, op, n, mode):
    tag = "ip%s%d%s" % (op, n, mode)
    x, sj, g = _data(n, tag)
    rng = _rng(tag + "d")
    d = rng.uniform(0.2, 2.0, size=n)
    lam = 0.6
    ay, ai = redzone.F64_MODES[mode]
    y = c.out(n, ay)
    gb, db, xb, sb = c.vec(g, ai, name="g"), c.vec(d, ai, name="d"), c.vec(x, ai, name="xk"), c.vec(sj, ai, name="sj")
    if op.endswith("_box"):
        l = rng.uniform(-1.5, -0.2, size=n); u = rng.uniform(0.2, 1.5, size=n)
        mask = (rng.random(n) < 0.6).astype(np.uint8)        # unselected entries: the iprox_zero branch
        lb, ub, mb = c.vec(l, ai, name="l"), c.vec(u, ai, name="u"), c.u8(mask)
        c.call("spx_iprox_" + op, y.ptr(), gb.ptr(), db.ptr(), xb.ptr(), sb.ptr(), n, _D(lam), lb.ptr(), ub.ptr(), _D(0.0), _D(0.0),
               mb.ptr())
        ref = getattr(c.orc, "iprox_" + op)(g, d, x, sj, lam, l, u, mask)
    else:
        c.call("spx_iprox_" + op, y.ptr(), gb.ptr(), db.ptr(), xb.ptr(), sb.ptr(), n, _D(lam), 1)
        ref = getattr(c.orc, "iprox_" + op)(g, d, x, sj, lam)
    assert _bits(y.t.cpu().numpy(), ref), (op, n, mode)
    c.finish()


def _proxval(c, op, n, target):
    t = c.torch
    tag = "pv%s%d" % (op, n)
    x, sj, q = _data(n, tag)
    lam, sigma, qs = 0.7, 0.9, -1.25
    y, qb = c.out(n), c.vec(q, name="q")
    xb, sb = c.vec(x, name="xk"), c.vec(sj, name="sj")
    vt = c.zone.add(1, t.float64, 0, data=np.zeros(1), role="inout", name="value") if target == "device" else None
    if vt is not None:
        c.s._lib.check(c.L.spx_ctx_set_value_target(c.ctx, ctypes.c_void_p(vt.ptr())))
    val = _D(0.0)
    try:
        if op == "l1_box":
            l, u = -0.8, 0.9
            c.call("spx_proxval_l1_box", y.ptr(), qb.ptr(), xb.ptr(), sb.ptr(), n, _D(lam), _D(sigma), None, None, _D(l), _D(u), None,
                   _D(qs), ctypes.byref(val))
            ref = c.orc.prox_l1_box(qs * q, x, sj, lam, sigma, l, u)
            vref = c.orc.obj_box("l1", ref, x, sj, lam, l, u)
        else:
            c.call("spx_proxval_" + op, y.ptr(), qb.ptr(), xb.ptr(), sb.ptr(), n, _D(lam), _D(sigma), _D(qs), ctypes.byref(val))
            ref = getattr(c.orc, "prox_" + op)(qs * q, x, sj, lam, sigma)
            vref = c.orc.obj_plain(op, ref, x, sj, lam)
    finally:
        c.s._lib.check(c.L.spx_ctx_set_value_target(c.ctx, None))
    got = y.t.cpu().numpy()
    if op == "lhalf":
        if not _bits(got, ref):
            arbiter.check_lhalf(c.orc, got, ref, qs * q, x, sj, lam, sigma, what=op)
    else:
        assert _bits(got, ref), (op, n)
    v = float(vt.t.cpu()[0]) if vt is not None else val.value
    if vt is not None:
        assert np.isnan(val.value)
    assert abs(v - vref) <= 1e-12 * abs(vref) or (op == "l0" and v == vref), (op, n, target, v, vref)
    c.finish()


# ================================================================== Float32 separable / iprox!
def _f32_cases():
    out = []
    for op, n, off in itertools.product(("l1", "l0", "l1_box", "l0_box"), (1, 63, 3073, 1_000_003), redzone.F32_OFFSETS):
        out.append(("f32-%s-n%d-o%d" % (op, n, off), lambda c, op=op, n=n, off=off: _f32(c, op, n, off, False)))
        if n in (3073, 1_000_003):
            out.append(("f32-iprox-%s-n%d-o%d" % (op, n, off), lambda c, op=op, n=n, off=off: _f32(c, op, n, off, True)))
    return out


def _f32(c, op, n, off, ip):
    t = c.torch
    tag = "f32%s%d%d%d" % (op, n, off, ip)
    x, sj, q = (v.astype(np.float32) for v in _data(n, tag))
    rng = _rng(tag + "b")
    lam, sigma = 0.7, 0.9
    y = c.out(n, off, t.float32)
    qb, xb, sb = c.vec(q, off, name="q"), c.vec(x, off, name="xk"), c.vec(sj, off, name="sj")
    box = op.endswith("_box")
    if box:
        l = rng.uniform(-1.5, -0.2, size=n).astype(np.float32); u = rng.uniform(0.2, 1.5, size=n).astype(np.float32)
        mask = (rng.random(n) < 0.6).astype(np.uint8)
        lb, ub, mb = c.vec(l, off, name="l"), c.vec(u, off, name="u"), c.u8(mask)
        bargs = (lb.ptr(), ub.ptr(), _F(0.0), _F(0.0), mb.ptr())
    if ip:
        d = rng.uniform(0.2, 2.0, size=n).astype(np.float32)
        db = c.vec(d, off, name="d")
        if box:
            c.call("spx_iprox_%s_f32" % op, y.ptr(), qb.ptr(), db.ptr(), xb.ptr(), sb.ptr(), n, _F(lam), *bargs)
            ref = c.orc.iprox_f32(op, q, d, x, sj, lam, l, u, mask)
        else:
            c.call("spx_iprox_%s_f32" % op, y.ptr(), qb.ptr(), db.ptr(), xb.ptr(), sb.ptr(), n, _F(lam), 1)
            ref, bad = c.orc.iprox_f32(op, q, d, x, sj, lam)
            assert bad == -1
    elif box:
        c.call("spx_prox_%s_f32" % op, y.ptr(), qb.ptr(), xb.ptr(), sb.ptr(), n, _F(lam), _F(sigma), *bargs)
        ref = c.orc.prox_f32(op, q, x, sj, lam, sigma, l, u, mask)
    else:
        c.call("spx_prox_%s_f32" % op, y.ptr(), qb.ptr(), xb.ptr(), sb.ptr(), n, _F(lam), _F(sigma))
        ref = c.orc.prox_f32(op, q, x, sj, lam, sigma)
    assert _bits(y.t.cpu().numpy(), ref), (op, n, off, ip)
    c.finish()


# ================================================================== psi(y): run_obj, run_obj_group
def _obj_cases():
    out = []
    for op, n, fewer in itertools.product(("l1", "l0", "lhalf", "l1_box", "indball", "indball_binf"), (1, 65, 6145, 1_000_003), (1, 0)):
        out.append(("obj-%s-n%d-k17_%d" % (op, n, fewer), lambda c, op=op, n=n, f=fewer: _obj(c, op, n, f, False)))
    for op, n, fewer in itertools.product(("l1", "l0_box", "indball_binf"), (65, 1_000_003), (1, 0)):
        out.append(("obj-f32-%s-n%d-k17_%d" % (op, n, fewer), lambda c, op=op, n=n, f=fewer: _obj(c, op, n, f, True)))
    layouts = ["uniform8", "uniform128", "ragged", "gather", "chunk1_one", "chunk1_256", "chunk_csr", "chunk_uniform300", "one_huge"]
    for lay, binf, fewer in itertools.product(layouts, (False, True), (1, 0)):
        if lay == "gather" and fewer == 0:
            continue
        out.append(("objgrp-%s-binf%d-k17_%d" % (lay, binf, fewer), lambda c, lay=lay, b=binf, f=fewer: _obj_group(c, lay, b, f, False)))
    for lay in ("uniform8", "ragged", "chunk1_one"):
        out.append(("objgrp-f32-%s" % lay, lambda c, lay=lay: _obj_group(c, lay, False, 1, True)))
    return out


def _obj(c, op, n, fewer, f32):
    t = c.torch
    tag = "obj%s%d%d" % (op, n, f32)
    x, sj, y = _data(n, tag)
    y = 0.1 * y
    rng = _rng(tag + "b")
    c.tune(17, fewer)
    lam, delta = 0.7, 2.0
    if f32:
        x, sj, y = (v.astype(np.float32) for v in (x, sj, y))
    al = 4 if f32 else 8 * (n % 2)
    yb, xb, sb = c.vec(y, al, name="y"), c.vec(x, al, name="xk"), c.vec(sj, al, name="sj")
    val = _D(0.0)
    sfx = "_f32" if f32 else ""
    P = _F if f32 else _D
    if op.endswith("_box"):
        l = rng.uniform(-3.0, -1.5, size=n); u = rng.uniform(1.5, 3.0, size=n)   # (feasible: a finite value)
        if f32:
            l, u = l.astype(np.float32), u.astype(np.float32)
        mask = (rng.random(n) < 0.6).astype(np.uint8)
        lb, ub, mb = c.vec(l, al, name="l"), c.vec(u, al, name="u"), c.u8(mask)
        kind = op[:-4]
        c.call("spx_obj_%s%s" % (op, sfx), yb.ptr(), xb.ptr(), sb.ptr(), n, P(lam), lb.ptr(), ub.ptr(), P(0.0), P(0.0), mb.ptr(),
               ctypes.byref(val))
        if f32:
            return _obj_f32_check(c, op, n, val.value, lam, *c.orc.obj_f32(kind, y, x, sj, l=l, u=u, mask=mask))
        ref = c.orc.obj_box(kind, y, x, sj, lam, l, u, mask)
    elif op.startswith("indball"):
        r = max(n // 2, 1)
        if op == "indball_binf":
            c.call("spx_obj_indball_l0_binf" + sfx, yb.ptr(), xb.ptr(), sb.ptr(), n, r, P(delta), ctypes.byref(val))
        else:
            c.call("spx_obj_indball_l0" + sfx, yb.ptr(), xb.ptr(), sb.ptr(), n, r, ctypes.byref(val))
        d = delta if op == "indball_binf" else None
        if f32:   # the count of the Float32 terms and the Float64 ball test of the Float32 restatement: exact
            terms, outside = c.orc.obj_f32("l0", y, x, sj, delta=d)
            assert val.value == (np.inf if outside or int(terms.sum()) > r else 0.0), (op, n, val.value)
            c.finish()
            return
        ref = c.orc.obj_indball_l0(y, x, sj, r, delta=d)
        # a count over n elements: exact.  Every y of this data has more than r nonzeros: +Inf
        assert val.value == ref, (op, n, val.value, ref)
        c.finish()
        return
    else:
        c.call("spx_obj_%s%s" % (op, sfx), yb.ptr(), xb.ptr(), sb.ptr(), n, P(lam), ctypes.byref(val))
        if f32:
            return _obj_f32_check(c, op, n, val.value, lam, *c.orc.obj_f32(op, y, x, sj))
        ref = c.orc.obj_plain(op, y, x, sj, lam)
    assert val.value == ref or abs(val.value - ref) <= 1e-12 * abs(ref), (op, n, val.value, ref)
    c.finish()


def _obj_f32_check(c, op, n, got, lam, terms, infeasible):
    """a Float32 psi(y) against the terms of the Float32 restatement (oracle.obj_f32), summed exactly: the bar of the step
    statistics, 1e-12 of sum |term| times (double)lambda; NormL0 is one rounded product of a count; +Inf decisions are exact"""
    factor = float(np.float32(lam))
    if infeasible:
        assert got == np.inf, (op, n, got)
    elif op.startswith("l0"):
        assert got == factor * float(int(terms.sum())), (op, n, got)
    else:
        nonfinite.check_sum(got, terms, "obj-f32 %s n=%d" % (op, n), factor=factor)
    c.finish()


def _layout(lay, rng):
    """(n, offsets or None, gsize, groups for gather or None)"""
    if lay == "uniform8":
        return 8 * 5001, None, 8, None
    if lay == "uniform128":
        return 128 * 777, None, 128, None
    if lay == "ragged":
        n = 300_001
        cuts = np.sort(rng.choice(np.arange(1, n), size=4000, replace=False))
        return n, np.concatenate([[0], cuts, [n]]).astype(np.int64), 0, None
    if lay == "gather":
        n = 50_000
        perm = rng.permutation(n)
        cuts = np.sort(rng.choice(np.arange(1, n), size=999, replace=False))
        return n, None, 0, [g.tolist() for g in np.split(perm, cuts)]
    if lay == "chunk1_one":          # one group over the vector: chunked, one launch (k_obj_chunks with the last workgroup)
        n = (1 << 22) + 5
        return n, None, n, None
    if lay == "chunk1_256":          # 256 uniform groups of 8192 (2 chunks each: 512 <= 4096 chunks): one launch
        return 256 * 8192, None, 8192, None
    if lay == "chunk_uniform300":    # > 256 uniform groups of >= 8192: chunked, multi-launch
        return 300 * 8200, None, 8200, None
    if lay == "chunk_csr":           # CSR with average group size >= 8192: chunked multi-launch (prefix table)
        n = 3_000_017
        cuts = np.sort(rng.choice(np.arange(1, n), size=99, replace=False))
        return n, np.concatenate([[0], cuts, [n]]).astype(np.int64), 0, None
    if lay == "one_huge":            # one CSR group over the vector (offsets [0, n])
        n = 2_000_003
        return n, np.array([0, n], dtype=np.int64), 0, None
    raise KeyError(lay)


def _obj_group(c, lay, binf, fewer, f32):
    t = c.torch
    rng = _rng("og" + lay)
    n, offsets, gsize, groups = _layout(lay, rng)
    x, sj, y = _data(n, "og" + lay)
    y = 0.1 * y
    c.tune(17, fewer)
    ng = len(groups) if groups is not None else (len(offsets) - 1 if offsets is not None else n // gsize)
    lam = rng.uniform(0.5, 1.5, size=ng)
    delta = 1.0
    dt = t.float32 if f32 else t.float64
    if f32:
        x, sj, y, lam = (v.astype(np.float32) for v in (x, sj, y, lam))
    al = 4 if f32 else 8 * (ng % 2)
    yb, xb, sb, lb = c.vec(y, al, dt, name="y"), c.vec(x, al, dt, name="xk"), c.vec(sj, al, dt, name="sj"), c.vec(lam, 0, dt, name="lambda")
    val = _D(0.0)
    sfx = "_f32" if f32 else ""
    P = _F if f32 else _D
    tail = (P(delta),) if binf else ()
    name = "spx_obj_group_l2" + ("_binf" if binf else "")
    if groups is not None:
        ptr, index = c.orc._index_sets(groups)
        pb, ib = c.ints(ptr, n, "group_ptr"), c.ints(index, n, "group_index")
        c.call(name + "_gather", yb.ptr(), xb.ptr(), sb.ptr(), n, pb.ptr(), ib.ptr(), ng, len(index), lb.ptr(), *tail, ctypes.byref(val))
        ref = c.orc.obj_group_l2_idx(y, x, sj, lam, groups, delta=delta if binf else None)
    else:
        ob = c.ints(offsets, n, "offsets") if offsets is not None else None
        c.call(name + sfx, yb.ptr(), xb.ptr(), sb.ptr(), n, ob.ptr() if ob else None, gsize, ng, lb.ptr(), *tail, ctypes.byref(val))
        if f32:   # the per-group terms of the Float32 restatement, summed exactly
            terms, outside, bad = c.orc.obj_group_f32(y, x, sj, lam, offsets=offsets, gsize=gsize, delta=delta if binf else None)
            assert not outside and not bad
            nonfinite.check_sum(val.value, terms, "objgrp-f32 " + lay)
            c.finish()
            return
        ref = c.orc.obj_group_l2(y, x, sj, lam, offsets=offsets, gsize=gsize, delta=delta if binf else None)
    assert val.value == ref or abs(val.value - ref) <= 1e-12 * abs(ref), (lay, binf, fewer, val.value, ref)
    c.finish()


# ================================================================== top-r (run_select, spx_select.hip)
# (n, mode, keys): k_sel_small (n <= 8192); the register form in each elements-per-lane band (<= 65 536, <= 196 608, <= 655 360,
# <= 2^21); k_sel_lds vec (A) / non-vec (C) between 2^20 and ~4 Mi; the register-slot form (~4-6 Mi, A); k_sel_coop<.., false>
# (C at ~5e6); the sample-predicted path, single pass and two-pass (key 4 = 0) at ~8e6, A and B (ioff).
TOPR = [(5000, "A", {}), (5000, "B", {}), (60_000, "A", {}), (60_000, "C", {}), (190_000, "A", {}), (650_000, "B", {}),
        (2_000_000, "A", {}), (3_000_000, "A", {}), (3_000_000, "C", {}), (3_000_000, "D", {}), (5_000_000, "A", {}),
        (5_000_000, "C", {}), (8_000_000, "A", {}), (8_000_000, "B", {}), (8_000_000, "A", {4: 0}), (8_000_000, "B", {4: 0})]


def _topr_cases():
    out = []
    for n, mode, keys in TOPR:
        for binf in (False, True):
            kk = "".join("-k%d_%d" % kv for kv in keys.items())
            out.append(("topr-n%d-%s%s-binf%d" % (n, mode, kk, binf), lambda c, n=n, m=mode, k=keys, b=binf: _topr(c, n, m, k, b, False)))
        out.append(("topr-lattice-n%d-%s%s" % (n, mode, "".join("-k%d_%d" % kv for kv in keys.items())),
                    lambda c, n=n, m=mode, k=keys: _topr(c, n, m, k, True, True)))
    for n in ((1 << 23) - 1, (1 << 23) + 3):
        out.append(("topr-f32-n%d" % n, lambda c, n=n: _topr_f32(c, n)))
    return out


_TOPR_ORDER = {}


def _topr(c, n, mode, keys, binf, lattice):
    tag = "tr%d%s" % (n, "lat" if lattice else "")
    x, sj, q = _data(n, tag, quant=4 if lattice else None)
    if tag not in _TOPR_ORDER:             # (the oracle's sort, kept for the next case of the same data: two at most)
        while len(_TOPR_ORDER) >= 2:
            _TOPR_ORDER.pop(next(iter(_TOPR_ORDER)))
        _TOPR_ORDER[tag] = c.orc.TopR(q, x, sj)
    top = _TOPR_ORDER[tag]
    for k, v in keys.items():
        c.tune(k, v)
    delta = 0.9
    ai = redzone.F64_MODES[mode][1]
    xb, sb = c.vec(x, ai, name="xk"), c.vec(sj, ai, name="sj")
    rs = [n // 3] if lattice else [1, n // 100, n // 2, n - 1]
    for r in rs:
        c.zone.bufs = [xb, sb]
        y, qb = _yq(c, q, mode, n)
        if binf:
            c.call("spx_prox_indball_l0_binf", y.ptr(), qb.ptr(), xb.ptr(), sb.ptr(), n, r, _D(delta))
        else:
            c.call("spx_prox_indball_l0", y.ptr(), qb.ptr(), xb.ptr(), sb.ptr(), n, r)
        ref = top.prox(r, delta if binf else None)
        got = y.t.cpu().numpy()
        assert _bits(got, ref), (n, mode, keys, binf, r, int(np.sum(got != ref)))
        c.zone.check()
        del y, qb
    c.finish()


def _topr_f32(c, n):
    t = c.torch
    rng = _rng("trf%d" % n)
    q = rng.normal(size=n).astype(np.float32)
    z = np.zeros(n, dtype=np.float32)
    r = n // 100
    y, qb = c.out(n, 4, t.float32), c.vec(q, 4, name="q")
    xb, sb = c.vec(z, 4, name="xk"), c.vec(z, 4, name="sj")
    c.call("spx_prox_indball_l0_binf_f32", y.ptr(), qb.ptr(), xb.ptr(), sb.ptr(), n, r, _F(0.9))
    ref = c.orc.prox_indball_l0_f32(q, z, z, r, delta=0.9)
    got = y.t.cpu().numpy()
    assert _bits(got, ref), (n, int(np.sum(got != ref)))
    c.finish()


# ================================================================== B2 (spx_prox_l1_b2, spx_b2.hip)
# the register form per elements-per-lane band (<= 131 072, <= 524 288, <= 2^21); xk in LDS (2^21 < n <= 2^22); streaming (key 12 = 0
# at 3e6, by default at 6e6); tiles handed out on demand (ntiles >= 8 G: n = 1.6e7); an inactive trust region
B2 = [(100_001, "A", {}, 1.0), (100_001, "C", {}, 1.0), (500_000, "A", {}, 1.0), (1_500_001, "C", {}, 1.0), (3_000_000, "A", {}, 1.0),
      (3_000_001, "C", {}, 1.0), (3_000_000, "A", {12: 0}, 1.0), (6_000_001, "A", {}, 1.0), (6_000_000, "C", {}, 1.0),
      (16_000_000, "A", {}, 1.0), (500_000, "A", {}, 1e6), (6_000_000, "A", {}, 1e6)]


def _b2_cases():
    return [("b2-n%d-%s%s-d%g" % (n, m, "".join("-k%d_%d" % kv for kv in k.items()), d), lambda c, n=n, m=m, k=k, d=d: _b2(c, n, m, k, d))
            for n, m, k, d in B2]


def _b2(c, n, mode, keys, delta):
    x, sj, q = _data(n, "b2%d" % n)
    for k, v in keys.items():
        c.tune(k, v)
    ay, ai = redzone.F64_MODES[mode]
    y, qb = c.out(n, ay), c.vec(q, ai, name="q")
    xb, sb = c.vec(x, ai, name="xk"), c.vec(sj, ai, name="sj")
    c.call("spx_prox_l1_b2", y.ptr(), qb.ptr(), xb.ptr(), sb.ptr(), n, _D(1.0), _D(1.0), _D(delta), _D(1.0))
    ref = c.orc.prox_l1_b2(q, x, sj, 1.0, 1.0, delta, 1.0)
    got = y.t.cpu().numpy()
    assert np.max(np.abs(got - ref)) <= 1e-12 * max(np.linalg.norm(ref), np.linalg.norm(x)), (n, mode, keys, delta)
    c.finish()


# ================================================================== group prox! (run_group) and the team form
def _group_cases():
    out = []
    for gs in list(range(1, 18)) + [128, 512, 513]:
        for binf in (False, True):
            out.append(("grp-uniform%d-binf%d" % (gs, binf), lambda c, gs=gs, b=binf: _group(c, "uniform", b, gs=gs)))
    for lay in ("ragged", "ragged_bound", "uncovered", "empty", "gather", "team_chip", "team_stream", "team_ragged", "team_ondemand"):
        for binf in (False, True):
            keys = [{}]
            if binf and lay in ("team_chip", "team_stream"):
                keys = [{}, {14: 0}]                          # Binf fast path and generic body
            for k in keys:
                out.append(("grp-%s-binf%d%s" % (lay, binf, "".join("-k%d_%d" % kv for kv in k.items())),
                            lambda c, lay=lay, b=binf, k=k: _group(c, lay, b, keys=k)))
    for lay in ("uniform", "ragged"):
        out.append(("grp-f32-%s" % lay, lambda c, lay=lay: _group_f32(c, lay)))
    return out


def _group_f32(c, name):
    """spx_prox_group_l2_f32 on guarded buffers: the bit rule of tests/f32_exact.py -- the restatement with every group's exact
    norm rounded once; a group within 1e-12 of a rounding boundary of its norm may take either neighbour's result (the census of
    these seeds holds its cap: tests/test_oracle_f32_forms.py, on the CPU)"""
    t = c.torch
    lay, d, sigma = f32_exact.redzone_group_case(name)
    _, n, offsets, gs, ng, _ = lay
    y = c.out(n, 0, t.float32)
    qb, xb, sb, lb = (c.vec(d[k], 0, t.float32, name=nm) for k, nm in (("q", "q"), ("x", "xk"), ("sj", "sj"), ("lam", "lambda")))
    ob = c.ints(offsets, n, "offsets") if offsets is not None else None
    c.call("spx_prox_group_l2_f32", y.ptr(), qb.ptr(), xb.ptr(), sb.ptr(), n, ob.ptr() if ob else None, gs, ng, lb.ptr(), _F(float(sigma)))
    ref, amb, alts = f32_exact.prox_reference(c.orc, lay, d, sigma=sigma)
    f32_exact.check_prox(y.t.cpu().numpy(), lay, ref, amb, alts, "grp-f32-" + name)
    c.finish()


def _group(c, lay, binf, gs=0, keys=None):
    t = c.torch
    rng = _rng("g%s%d%d" % (lay, gs, binf))
    groups = offsets = None
    bound = 0
    if lay == "uniform":
        n = gs * 2001
    elif lay in ("ragged", "ragged_bound"):
        n = 200_003
        cuts = np.sort(rng.choice(np.arange(1, n), size=3000, replace=False))
        offsets = np.concatenate([[0], cuts, [n]])
        bound = int(np.max(np.diff(offsets))) if lay == "ragged_bound" else 0
    elif lay == "uncovered":        # CSR offsets that do not span 0:n (k_csr_uncovered)
        n = 100_000
        offsets = np.arange(1000, 90_001, 89)
    elif lay == "empty":            # ngroups = 0
        n = 70_001
        offsets = np.array([0])
    elif lay == "gather":
        n = 60_000
        perm = rng.permutation(n)
        cuts = np.sort(rng.choice(np.arange(1, n), size=999, replace=False))
        groups = [g.tolist() for g in np.split(perm, cuts)]
    elif lay == "team_chip":        # one group over the vector, on chip
        n = 120_000
        offsets = np.array([0, n])
    elif lay == "team_stream":      # one group over the vector, streamed (beyond the team's LDS)
        n = 3_000_001
        offsets = np.array([0, n])
    elif lay == "team_ragged":      # a few large ragged groups
        n = 2_500_000
        offsets = np.array([0, 700_001, 700_003, 1_900_000, n])
    else:                           # team_ondemand: the on-demand tile counters (ntiles >= 8 W)
        n = 13_000_000
        offsets = np.array([0, n])
    x, sj, q = _data(n, "g%s%d" % (lay, gs))
    ng = len(groups) if groups is not None else (len(offsets) - 1 if offsets is not None else n // gs)
    lam = rng.uniform(0.3, 1.5, size=ng)
    if lay.startswith("team"):
        lam = lam * 0.4 * np.sqrt(n)
    sigma, delta = 0.9, 0.8
    for k, v in (keys or {}).items():
        c.tune(k, v)
    dt = t.float64
    if lay in ("uncovered", "empty"):   # (y outside the groups: the shift-only entries, or y on entry)
        y = c.zone.add(n, dt, 0, data=np.zeros(n), role="inout", name="y")
    else:
        y = c.out(n, 0, dt)
    qb, xb, sb, lb = c.vec(q, 0, dt, name="q"), c.vec(x, 0, dt, name="xk"), c.vec(sj, 0, dt, name="sj"), c.vec(lam, 0, dt, name="lambda")
    tail = (_D(delta),) if binf else ()
    name = "spx_prox_group_l2" + ("_binf" if binf else "")
    if groups is not None:
        ptr, index = c.orc._index_sets(groups)
        pb, ib = c.ints(ptr, n, "group_ptr"), c.ints(index, n, "group_index")
        c.call(name + "_gather", y.ptr(), qb.ptr(), xb.ptr(), sb.ptr(), n, pb.ptr(), ib.ptr(), ng, len(index), lb.ptr(), _D(sigma), *tail)
        ref = c.orc.prox_group_l2_idx(q, x, sj, lam, sigma, groups, delta=delta if binf else None)
        S = (q + x) + sj
        scale = np.abs(ref).copy()
        for g in groups:
            scale[g] = np.maximum(scale[g], np.linalg.norm(S[g]))
        got = y.t.cpu().numpy()
        assert np.all(np.abs(got - ref) <= GROUP_TOL * np.maximum(scale, 1e-300)), (lay, binf)
        c.finish()
        return
    ob = c.ints(offsets, n, "offsets") if offsets is not None else None
    c.call(name, y.ptr(), qb.ptr(), xb.ptr(), sb.ptr(), n, ob.ptr() if ob else None, bound if ob else gs, ng, lb.ptr(), _D(sigma), *tail)
    offs = offsets if offsets is not None else np.arange(0, n + 1, gs)
    if binf:
        ref = c.orc.prox_group_l2_binf(q, x, sj, lam, sigma, delta, offsets=offsets, gsize=gs if offsets is None else 0)
    else:
        ref = c.orc.prox_group_l2(q, x, sj, lam, sigma, offsets=offsets, gsize=gs if offsets is None else 0)
    got = y.t.cpu().numpy()
    if lay in ("uncovered", "empty"):
        cov = np.zeros(n, dtype=bool)
        for a, b in zip(offs[:-1], offs[1:]):
            cov[a:b] = True
        # outside the groups: the shift-only entries of the reference, or y on entry (0) for the plain form
        assert _bits(got[~cov], ref[~cov]), (lay, binf)
        got, ref = np.where(cov, got, 0.0), np.where(cov, ref, 0.0)
    if ng:
        arbiter.check_group(c.orc, got, ref, q, x, sj, lam, sigma, offs, delta=delta if binf else None, what="%s binf %d" % (lay, binf))
    c.finish()


# ================================================================== helpers, host forms
def _helper_cases():
    out = []
    for es, ds, ss, n in itertools.product((4, 8), (1, 2, 3), (1, 3), (1, 1000, 300_001)):
        out.append(("copy-e%d-d%d-s%d-n%d" % (es, ds, ss, n), lambda c, es=es, ds=ds, ss=ss, n=n: _copy(c, es, ds, ss, n)))
    for n in (1, 5000, 1_000_003):
        out.append(("mask-n%d" % n, lambda c, n=n: _mask(c, n)))
        out.append(("synth-n%d" % n, lambda c, n=n: _synth(c, n)))
    for which in ("sep", "topr", "group"):
        out.append(("host-%s" % which, lambda c, w=which: _host(c, w)))
    return out


def _copy(c, es, ds, ss, n):
    t = c.torch
    dt = t.float32 if es == 4 else t.float64
    src = _rng("cp%d%d" % (n, ss)).normal(size=n * ss).astype(np.float32 if es == 4 else np.float64)
    sb = c.vec(src, 0, dt, name="src")
    if ds == 1:
        d = c.out(n, 0, dt, name="dst")
    else:   # a strided destination: the elements between the strided ones must stay as they were
        d = c.zone.add(n * ds, dt, 0, data=np.zeros(n * ds, dtype=src.dtype), role="inout", name="dst")
    c.call("spx_copy_strided", d.ptr(), ds, sb.ptr(), ss, n, es)
    got = d.t.cpu().numpy()
    want = np.zeros(n * ds, dtype=src.dtype)
    want[::ds] = src[::ss]
    assert _bits(got, want[: len(got)]), (es, ds, ss, n)
    c.finish()


def _mask(c, n):
    rng = _rng("mk%d" % n)
    sel = rng.integers(-3, n + 3, size=max(n // 3, 1))
    m = c.out(n, 0, c.torch.uint8, name="mask")
    sb = c.ints(sel, n, "selected")
    c.call("spx_build_mask", m.ptr(), n, sb.ptr(), len(sel))
    assert _bits(m.t.cpu().numpy(), c.orc.mask_from_selected(sel + 1, n))
    c.finish()


def _synth(c, n):
    o = c.out(n, 8, name="synth")
    c.call("spx_synth_fill", o.ptr(), n, ctypes.c_uint64(7), ctypes.c_uint64(2), 1, _D(0.5))   # writes exactly n
    assert _bits(o.t.cpu().numpy(), c.orc.synth_fill(n, 7, 2, 1, 0.5))
    c.finish()


def _host(c, which):
    """spx_host_* on guarded numpy arrays (host memory, same guard layout)"""
    t = c.torch
    z = redzone.Zone(device="cpu")
    c.zone = z
    n = {"sep": 100_003, "topr": 250_001, "group": 7 * 14_287}[which]
    x, sj, q = _data(n, "host" + which)
    y = z.add(n, t.float64, 0, role="out", name="y")
    qb, xb, sb = (z.add(n, t.float64, 8, data=v, name=nm) for v, nm in ((q, "q"), (x, "xk"), (sj, "sj")))
    p = lambda g: ctypes.c_void_p(g.a.ctypes.data)
    if which == "sep":
        c.call("spx_host_prox_l1", p(y), p(qb), p(xb), p(sb), n, _D(0.7), _D(0.9))
        assert _bits(y.a, c.orc.prox_l1(q, x, sj, 0.7, 0.9))
    elif which == "topr":
        c.call("spx_host_prox_indball_l0_binf", p(y), p(qb), p(xb), p(sb), n, n // 100, _D(0.9))
        assert _bits(y.a, c.orc.prox_indball_l0_binf(q, x, sj, n // 100, 0.9))
    else:
        gs = 7
        lam = _rng("hl").uniform(0.3, 1.5, size=n // gs)
        lb = z.add(len(lam), t.float64, 0, data=lam, name="lambda")
        c.call("spx_host_prox_group_l2", p(y), p(qb), p(xb), p(sb), n, None, gs, n // gs, p(lb), _D(0.9))
        ref = c.orc.prox_group_l2(q, x, sj, lam, 0.9, gsize=gs)
        arbiter.check_group(c.orc, y.a.copy(), ref, q, x, sj, lam, 0.9, np.arange(0, n + 1, gs), what="host group")
    c.finish()


# ================================================================== the flat, interleaved case list
def _interleave(*families):
    out = []
    for row in itertools.zip_longest(*families):
        out.extend(cs for cs in row if cs is not None)
    return out


CASES = _interleave(_sep_cases(), _obj_cases(), _topr_cases(), _iprox_cases(), _group_cases(), _b2_cases(), _f32_cases(), _helper_cases())


@pytest.mark.parametrize("case", [fn for _, fn in CASES], ids=[cid for cid, _ in CASES])
def test_guarded(env, orc, case):
    case(Case(env, orc))


# ================================================================== psi(y) on offsets that break the contract
@pytest.mark.parametrize("layout", ["repeat", "decreasing", "negative_first", "last_past_n"])
def test_objective_rejects_bad_offsets_inside_its_buffers(env, orc, layout):
    """the chunked psi(y) sized its chunk table for n / 4096 + ngroups chunks and then wrote as many as the offsets
    make ([0, n, 0, n]: 512 against 259).  Now both forms (key 13 = 1: chunked; 0: a wavefront per group) report the layout --
    SPX_ERR_INVALID_ARG, or NaN in a device value target -- and stay inside every buffer."""
    s, L, ctx = env
    import torch
    n = 1 << 20
    off = {"repeat": [0, n, 0, n], "decreasing": [0, 600_000, 500_000, n], "negative_first": [-4096, 500_000, n],
           "last_past_n": [0, 500_000, n + 8192]}[layout]
    x, sj, y = _data(n, "bad" + layout)
    lam = np.ones(len(off) - 1)
    for key13, target, binf in itertools.product((1, 0), ("host", "device"), (False, True)):
        c = Case(env, orc)
        c.tune(13, key13)
        yb, xb, sb = c.vec(0.1 * y, name="y"), c.vec(x, name="xk"), c.vec(sj, name="sj")
        lb, ob = c.vec(lam, name="lambda"), c.ints(off, n, "offsets")
        vt = c.zone.add(1, torch.float64, 0, data=np.zeros(1), role="inout", name="value") if target == "device" else None
        if vt is not None:
            s._lib.check(L.spx_ctx_set_value_target(ctx, ctypes.c_void_p(vt.ptr())))
        val = _D(0.0)
        tail = (_D(1.0),) if binf else ()
        torch.cuda.synchronize()
        rc = getattr(L, "spx_obj_group_l2" + ("_binf" if binf else ""))(ctx, yb.ptr(), xb.ptr(), sb.ptr(), n, ob.ptr(), 0, len(off) - 1,
                                                                          lb.ptr(), *tail, ctypes.byref(val))
        torch.cuda.synchronize()
        s._lib.check(L.spx_ctx_set_value_target(ctx, None))
        what = (layout, key13, target, binf)
        if vt is None:
            assert rc == 1, what      # SPX_ERR_INVALID_ARG
            assert "offsets" in L.spx_last_error().decode(), what
        else:
            assert rc == 0 and np.isnan(float(vt.t.cpu()[0])), what
        c.finish()
    # the context is sound afterwards: a valid CSR call on it
    c = Case(env, orc)
    good = np.array([0, 300_000, 300_001, n], dtype=np.int64)
    yb, xb, sb = c.vec(0.1 * y, name="y"), c.vec(x, name="xk"), c.vec(sj, name="sj")
    lb, ob = c.vec(np.ones(3), name="lambda"), c.ints(good, n, "offsets")
    val = _D(0.0)
    c.call("spx_obj_group_l2", yb.ptr(), xb.ptr(), sb.ptr(), n, ob.ptr(), 0, 3, lb.ptr(), ctypes.byref(val))
    ref = orc.obj_group_l2(0.1 * y, x, sj, np.ones(3), offsets=good)
    assert abs(val.value - ref) <= 1e-12 * ref
    c.finish()
