"""GPU: every argument error of the separable entry points -- status, the literal message, the precedence among the checks --
and that a refused call writes nothing.

One table over the 34 separable prox! / iprox! entry points (6 prox, 6 proxval, 6 proxstep, 4 iprox, 4 iproxstep, 4 prox_*_f32,
4 iprox_*_f32) and one over the 6 Float64 and 6 Float32 separable spx_obj_*.  A row's refusals follow from its kind (CASES
below); the cases with two faults pin the order of the checks, accidental or not:

  - spx_proxval_l1 with y == q and lambda * sigma >= 0 tests q_scale == 1 before anything else, so it refuses even n == 0 with
    all-NULL vectors, a NULL ctx and a NULL value;
  - the other value calls test ctx, n and the vectors before `value`; the spx_obj_* test `value` before ctx;
  - the iprox forms test d after ctx, n and the vectors, and the step forms test d before the result pointers;
  - the step forms test the result pointers before check_d, check_d before the aliases of y, those before the aliases of xkn.

Every case is refused before anything is enqueued: after spx_sync the vectors of the call (y, xkn and the device statistics
hold poison) have the bytes they had.  Each row ends with the same arguments without a fault, which must run.  n = 8.

The expectations were taken from the library as it was before the call's operands travelled as one struct (SepCall, SpxBox:
csrc/spx_common.hpp): this file passed unchanged on that build.

The last test holds the NormL1 y === q rule, which differs by precision, to its two statements (spx_prox_l1: only for
lambda * sigma >= 0; spx_prox_l1_f32: for any lambda)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 8
LAM, SIGMA, LS, US = 0.7, 1.1, -0.9, 0.9
POISON = -777.25
INVALID_ARG = 1
SLOT = 16  # elements between the vectors of an arena
VECTORS = ["y", "q", "d", "xk", "sj", "l", "u", "xkn", "sdev"]

NULL_VECTOR = "NULL vector with n > 0"
BOTH_NULL = "stats and stats_dev are both NULL"
CHECK_D = "check_d needs the host form of the statistics (stats != NULL): it synchronises"
Y_IS_Q = "y aliases q (<q, y> of an overwritten q)"
Y_IS_G_OR_D = "y aliases g or d (the sums would read an overwritten input)"
XKN_ALIAS = "xkn is one of the other vectors"
Q_SCALE = "q_scale != 1 with y aliasing q"


@pytest.fixture(scope="module")
def s():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.build()


@pytest.fixture(scope="module")
def ctx(s):
    L = s._lib.load()
    c = ctypes.c_void_p()
    s._lib.check(L.spx_ctx_create(0, ctypes.byref(c)))
    yield c
    L.spx_sync(c)
    L.spx_ctx_destroy(c)


class _Arena:
    """every vector of a call in one device buffer, SLOT elements apart: the outputs hold poison, l = -1, u = 1, the rest 0.75"""

    def __init__(self, dtype):
        import torch
        self.buf = torch.full((SLOT * len(VECTORS),), 0.75, dtype=dtype, device="cuda:0")
        self.mask = torch.ones(SLOT, dtype=torch.uint8, device="cuda:0")
        for name, v in (("y", POISON), ("xkn", POISON), ("sdev", POISON), ("l", -1.0), ("u", 1.0)):
            self.view(name).fill_(v)
        self.ref = self.buf.clone()

    def view(self, name):
        i = VECTORS.index(name)
        return self.buf[SLOT * i:SLOT * (i + 1)]

    def p(self, name):
        return self.mask.data_ptr() if name == "mask" else self.view(name).data_ptr()

    def untouched(self):
        import torch
        return torch.equal(self.buf, self.ref) and bool((self.mask == 1).all())

    def restore(self):
        self.buf.copy_(self.ref)


@pytest.fixture(scope="module")
def arenas(s):
    import torch
    return {"d": _Arena(torch.float64), "f": _Arena(torch.float32)}


# ------------------------------------------------------------------ the tables
# name -> (kind, element type, Box form?)
SEP_ROWS = {}
for _op in ("l1", "l0", "lhalf", "l1_box", "l0_box", "lhalf_box"):
    for _kind in ("prox", "proxval", "proxstep"):
        SEP_ROWS["%s_%s" % (_kind, _op)] = (_kind, "d", _op.endswith("_box"))
for _op in ("l1", "l0", "l1_box", "l0_box"):
    SEP_ROWS["iprox_" + _op] = ("iprox", "d", _op.endswith("_box"))
    SEP_ROWS["iproxstep_" + _op] = ("iproxstep", "d", _op.endswith("_box"))
    SEP_ROWS["prox_%s_f32" % _op] = ("prox", "f", _op.endswith("_box"))
    SEP_ROWS["iprox_%s_f32" % _op] = ("iprox", "f", _op.endswith("_box"))
OBJ_ROWS = {"obj_%s%s" % (_op, _sfx): ("obj", "f" if _sfx else "d", _op.endswith("_box"))
            for _op in ("l1", "l0", "lhalf", "l1_box", "l0_box", "lhalf_box") for _sfx in ("", "_f32")}


def test_the_tables_cover_the_separable_entry_points(s):
    assert len(SEP_ROWS) == 34 and len(OBJ_ROWS) == 12
    kinds = [k for k, _, _ in SEP_ROWS.values()]
    assert [kinds.count(k) for k in ("prox", "proxval", "proxstep", "iprox", "iproxstep")] == [6 + 4, 6, 6, 4 + 4, 4]
    separable = [n for n in s._lib.SIGNATURES if n.startswith(("spx_prox", "spx_iprox", "spx_obj_"))
                 and not any(w in n for w in ("group", "b2", "indball", "host"))]
    assert sorted(separable) == sorted("spx_" + n for n in list(SEP_ROWS) + list(OBJ_ROWS))


def _cases(name, kind, box):
    """[(what, changed arguments, message)]: every refusal of the row, then its two-fault cases"""
    inputs = {"obj": ["y", "xk", "sj"]}.get(kind, ["y", "q", "xk", "sj"])
    cases = [("ctx NULL", dict(ctx=None), "ctx is NULL"), ("n < 0", dict(n=-1), "n < 0")]
    cases += [("%s NULL" % v, {v: None}, NULL_VECTOR) for v in inputs]
    if kind in ("iprox", "iproxstep"):
        cases += [("d NULL", dict(d=None), "d is NULL"),
                  ("d NULL and sj NULL", dict(d=None, sj=None), NULL_VECTOR),
                  ("d NULL and ctx NULL", dict(d=None, ctx=None), "ctx is NULL"),
                  ("d NULL and n < 0", dict(d=None, n=-1), "n < 0")]
    if kind == "proxval":
        cases += [("value NULL", dict(value=None), "value is NULL"),
                  ("value NULL and xk NULL", dict(value=None, xk=None), NULL_VECTOR),
                  ("value NULL and ctx NULL", dict(value=None, ctx=None), "ctx is NULL")]
    if kind == "obj":
        cases += [("value NULL", dict(value=None), "value is NULL"),
                  ("value NULL and ctx NULL", dict(value=None, ctx=None), "value is NULL"),
                  ("value NULL and n < 0", dict(value=None, n=-1), "value is NULL"),
                  ("value NULL and y NULL", dict(value=None, y=None), "value is NULL")]
    if name == "proxval_l1":
        empty = dict(y=None, q=None, xk=None, sj=None, n=0, q_scale=2.0)
        cases += [("q_scale != 1 with y == q", dict(y="q", q_scale=2.0), Q_SCALE),
                  ("q_scale != 1 with y == q, n == 0 and all-NULL vectors", empty, Q_SCALE),
                  ("... and ctx NULL and value NULL", dict(empty, ctx=None, value=None), Q_SCALE),
                  ("q_scale != 1 with y == q and n < 0", dict(y="q", q_scale=2.0, n=-1), Q_SCALE)]
    if kind in ("proxstep", "iproxstep"):
        y_msg = Y_IS_Q if kind == "proxstep" else Y_IS_G_OR_D
        aliases = ["q"] if kind == "proxstep" else ["q", "d"]
        others = ["y", "q"] + (["d"] if kind == "iproxstep" else []) + ["xk", "sj"] + (["l", "u", "mask"] if box else [])
        cases += [("stats and stats_dev NULL", dict(stats=None, sdev=None), BOTH_NULL)]
        cases += [("y == %s" % v, dict(y=v), y_msg) for v in aliases]
        cases += [("xkn == %s" % v, dict(xkn=v), XKN_ALIAS) for v in others]
        cases += [("ctx NULL and both stats NULL", dict(ctx=None, stats=None, sdev=None), "ctx is NULL"),
                  ("sj NULL and both stats NULL", dict(sj=None, stats=None, sdev=None), NULL_VECTOR),
                  ("both stats NULL and y == q", dict(stats=None, sdev=None, y="q"), BOTH_NULL),
                  ("y == q and xkn == xk", dict(y="q", xkn="xk"), y_msg)]
        if kind == "iproxstep":
            cases += [("d NULL and both stats NULL", dict(d=None, stats=None, sdev=None), "d is NULL")]
            if not box:
                cases += [("check_d without host stats", dict(check_d=1, stats=None), CHECK_D),
                          ("check_d without host stats and y == d", dict(check_d=1, stats=None, y="d"), CHECK_D),
                          ("check_d without any stats", dict(check_d=1, stats=None, sdev=None), BOTH_NULL)]
    return cases


def _call(L, A, ctx, name, kind, box, change):
    """the row's call with `change` applied to its good arguments (a vector's name as a value: that vector's address)"""
    host_stats = (ctypes.c_double * 4)(POISON, POISON, POISON, POISON)
    value = ctypes.c_double(POISON)
    a = {v: A.p(v) for v in VECTORS + ["mask"]}
    a.update(ctx=ctx, n=N, check_d=0, q_scale=1.0, stats=host_stats, value=ctypes.byref(value))
    for k, v in change.items():
        a[k] = A.p(v) if isinstance(v, str) else v
    args = [a["ctx"], a["y"]] + ([] if kind == "obj" else [a["q"]]) + ([a["d"]] if kind.startswith("iprox") else [])
    args += [a["xk"], a["sj"], a["n"], LAM]
    if kind.startswith("iprox"):
        args += [] if box else [a["check_d"]]
    elif kind != "obj":
        args += [SIGMA]
    if box:
        args += [a["l"], a["u"], LS, US, a["mask"]]
    if kind in ("proxval", "proxstep"):
        args += [a["q_scale"]]
    if kind in ("proxval", "obj"):
        args += [a["value"]]
    if kind in ("proxstep", "iproxstep"):
        args += [a["xkn"], a["stats"], a["sdev"]]
    return getattr(L, "spx_" + name)(*args)


def _run_row(s, ctx, arenas, name, row):
    L = s._lib.load()
    kind, T, box = row
    A = arenas[T]
    assert A.untouched()
    for what, change, words in _cases(name, kind, box):
        rc = _call(L, A, ctx, name, kind, box, change)
        msg = (L.spx_last_error() or b"").decode()
        print(name, "|", what, "|", rc, "|", msg)
        assert rc == INVALID_ARG, (name, what, rc, msg)
        assert msg == "invalid argument: " + words, (name, what, msg)
        assert L.spx_sync(ctx) == 0
        assert A.untouched(), (name, what, "a refused call wrote to a vector")
    # the same arguments without a fault run
    try:
        assert _call(L, A, ctx, name, kind, box, {}) == 0 and L.spx_sync(ctx) == 0, (name, L.spx_last_error())
        if kind != "obj":
            assert bool((A.view("y")[:N] != POISON).all()) and bool((A.view("y")[N:] == POISON).all())
    finally:
        A.restore()


@pytest.mark.parametrize("name", list(SEP_ROWS))
def test_separable_refusals(s, ctx, arenas, name):
    _run_row(s, ctx, arenas, name, SEP_ROWS[name])


@pytest.mark.parametrize("name", list(OBJ_ROWS))
def test_objective_refusals(s, ctx, arenas, name):
    _run_row(s, ctx, arenas, name, OBJ_ROWS[name])


def test_l1_in_place_rule_by_precision(s, ctx):
    """y === q: the reference's body gives -xk - sj (the broadcast overwrites q).  Float64 takes that body only where it equals the
    one-pass formula bit for bit, lambda * sigma >= 0, and evaluates the formula otherwise: min(max(t, q - ls), q + ls) = q + ls
    for ls < 0.  Float32 takes it for any lambda."""
    import torch
    L = s._lib.load()
    rng = np.random.default_rng(7)
    q, x, sj = (rng.normal(size=N) for _ in range(3))
    for dtype, fn, lam, want in (
            (np.float64, L.spx_prox_l1, LAM, (-x) - sj),
            (np.float64, L.spx_prox_l1, -LAM, q + (-LAM) * SIGMA),
            (np.float32, L.spx_prox_l1_f32, -LAM, (-x.astype(np.float32)) - sj.astype(np.float32))):
        y, xd, sd = (torch.tensor(v.astype(dtype)).to("cuda:0") for v in (q, x, sj))
        assert fn(ctx, y.data_ptr(), y.data_ptr(), xd.data_ptr(), sd.data_ptr(), N, lam, SIGMA) == 0 and L.spx_sync(ctx) == 0
        assert np.array_equal(y.cpu().numpy(), want.astype(dtype)), (dtype, lam)
