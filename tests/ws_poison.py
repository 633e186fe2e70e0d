"""The driver of tests/test_gpu_ws_poison.py (a plain helper module, like tests/redzone.py and tests/nonfinite.py).

The library's scratch -- spx_ctx::ws, reserved through spx_ws_reserve, and the staging block of the spx_host_* forms -- is a bare
hipMalloc that is freed and allocated anew when it grows: no call may depend on what it held on entry.  The hooks build
(libspx_hooks.so, -DSPX_TEST_HOOKS) fills both blocks on request (tuning key 103: 1 zero bytes, 2 the word 0x00000001, 3 0xFF
bytes) and names every reserving call site on stdout (key 104: "SPX_WS_SITE <file> <function> <line> <bytes>").

`python tests/ws_poison.py CASE` runs one case in this process: every call of the case three times on one context, with key 103
set to 1, 2, 3 immediately before the call -- all of pattern 1 first, then 2, then 3 -- and stops at the first mismatch:

  (a) pattern 1: every result meets, against the CPU oracle, the bar its entry point has in the neighbouring test files;
  (b) patterns 2 and 3: every output (y, xkn, values, statistics, flag words, device targets) has the BITS of pattern 1;
  (c) every return code is 0, and spx_sync returns 0 at the end of each pattern.

Then the growth step: on a fresh context per pattern the case's smallest call, its largest, the smallest again (the second runs
on a block spx_ws_reserve allocated, and filled, inside that very call), held to the bits of the main run -- ShiftedNormL1B2,
whose speculative pass depends on the regime of the previous call, to (a) there.

Every form that reserves scratch promises run-to-run reproducibility ("added in a fixed order", include/spx.h), so no call is
held to (a) instead of (b) under patterns 2 and 3.

It prints the trace lines of key 104 and ends with one line "RESULT ok <calls>" or "RESULT FAIL <what>".

`python tests/ws_poison.py row_batch` is the case of the calls that promise to reserve NOTHING (spx_proxstep_l1_b2_batch,
spx_proxstep_indball_l0[_binf]_batch).  A tiled spx_proxstep_l1_batch call first grows the context's workspace (its trace line
shows that key 104 is live), so that there is a block to fill; then, between the lines "NO_WS_BEGIN" and "NO_WS_END", every
call runs under patterns 1, 2, 3 as above -- (a), (b), (c) -- and no trace line may appear between the two markers (the caller,
tests/test_gpu_ws_poison.py, reads them; the library flushes every trace line, the markers are flushed here).  There is no
growth step: nothing grows.

Two shapes differ from what the issue's list names, because of what the plan functions (csrc/spx_plan.hpp) do:
  * top-r at n = 3e5 under key 8 = 4 is the one-launch exact select (the front kernel of the sample-predicted pipeline needs 64
    resident workgroups): it runs, and reserves nothing.  The pipeline -- the only top-r form that reserves -- runs at
    n = 2^21 + 3001 under key 11 = 0, as tests/test_gpu_census_forms.py reaches it;
  * top-r at n = 5000 and n = 70 001 reserve nothing either (one workgroup; v on chip)."""
import ctypes
import math
import os
import sys
import traceback

import numpy as np

_D = ctypes.c_double
_F = ctypes.c_float
POISON = -777.25
YFILL = -777.0
TOL = 1e-12
# every key a case touches, at its default
DEFAULT_KEYS = {0: 0, 1: 1, 2: 1, 3: 1, 5: 0, 8: 0, 9: 0, 10: 0, 11: 1, 13: 1, 14: 1, 17: 1, 18: 0}
CASES = ("separable", "topr", "group", "b2", "host", "batch", "ibatch", "gbatch", "gbinf_batch", "lhalf_batch")
# the cases whose calls promise "workspace: NONE" (include/spx_b2_batch.h, include/spx_topr_batch.h): run_no_ws
NO_WS_CASES = ("row_batch",)


class Env:
    def __init__(self):
        import torch
        import __graft_entry__ as ge
        from oracle import oracle
        import arbiter
        import nonfinite
        oracle.build()
        self.torch, self.orc, self.arbiter, self.nf = torch, oracle, arbiter, nonfinite
        self.s = ge.build()
        self.L = self.s._lib.load()
        self.main = self.new_ctx()               # a private context: every call goes through the C ABI
        self.ctx = self.main

    def new_ctx(self):
        c = ctypes.c_void_p()
        self.s._lib.check(self.L.spx_ctx_create_on_stream(0, ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream), ctypes.byref(c)))
        return c

    def key(self, k, v):
        rc = self.L.spx_ctx_set_tuning(self.ctx, k, v)
        assert rc == 0, ("spx_ctx_set_tuning", k, v, rc, self.L.spx_last_error())

    def dev(self, a, off8=False):
        """device copy; off8: the vector starts 8 bytes past a 16-byte boundary (a 1-byte mask: 1 byte past a 2-byte one)"""
        torch = self.torch
        t = torch.from_numpy(np.ascontiguousarray(a))
        pad = max(1, 8 // t.element_size())
        buf = torch.empty(t.numel() + 2 * pad, dtype=t.dtype, device="cuda:0")
        assert buf.data_ptr() % 16 == 0
        shift = (1 if t.element_size() == 1 else pad) if off8 else 0
        v = buf[shift:shift + t.numel()]
        v.copy_(t)
        return v

    def fill(self, n, off8=False, value=YFILL, dtype=np.float64):
        return self.dev(np.full(n, value, dtype=dtype), off8)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def host(t):
    return t.cpu().numpy().copy()


def fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).ravel().tolist())


def sum_bar(got, terms, what, factor=1.0, exact=False):
    """`got` against factor * sum(terms): within 1e-12 of |factor| * sum |term| of math.fsum; exact: equality (the NormL0 count)"""
    got = float(got)
    ref, mag = factor * fsum(terms), abs(factor) * fsum(np.abs(terms))
    assert math.isfinite(got), (what, got, ref)
    if exact:
        assert got == ref, (what, got, ref)
    else:
        assert abs(got - ref) <= TOL * max(mag, 1e-300), (what, got, ref, mag)


def value_bar(got, exp, what, exact=False):
    """a value against the oracle's: the bar of tests/test_gpu_census_forms.py::_check_h"""
    got, exp = float(got), float(exp)
    if exact or not math.isfinite(exp):
        assert got == exp, (what, got, exp)
    else:
        assert abs(got - exp) <= TOL * max(abs(exp), 1e-300), (what, got, exp)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Call:
    """One library call of a case.  run(env) makes it on env.ctx and returns {name: host array} of EVERY output; check(env, out)
    holds that to the oracle (a).  keys: tuning keys on top of the defaults.  regime: the result's bits follow the context's
    previous call (ShiftedNormL1B2) -- the growth step holds such a call to (a)."""

    def __init__(self, name, run, check, keys=None, regime=False):
        self.name, self.run, self.check, self.keys, self.regime = name, run, check, dict(keys or {}), regime


def make(env, call, pattern):
    for k, v in DEFAULT_KEYS.items():
        env.key(k, v)
    for k, v in call.keys.items():
        env.key(k, v)
    env.key(103, pattern)            # immediately before the call: refills the workspace and the staging block
    out = call.run(env)
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def compare(base, out, what):
    assert sorted(base) == sorted(out), (what, sorted(base), sorted(out))
    for k in sorted(base):
        if not same_bits(base[k], out[k]):
            a, b = base[k].ravel(), out[k].ravel()
            assert a.size == b.size, (what, k, a.size, b.size)
            bad = np.flatnonzero((a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(axis=1))
            first = int(bad[0]) if bad.size else -1
            raise AssertionError("%s: output %r differs from pattern 1 at %d of %d places, first %d: %r vs %r" % (
                what, k, bad.size, a.size, first, a[first] if first >= 0 else None, b[first] if first >= 0 else None))


def run_case(name):
    env = Env()
    torch, L = env.torch, env.L
    calls, growth = BUILDERS[name](env)
    env.key(104, 1)
    base = {}
    done = 0
    for pattern in (1, 2, 3):
        for i, call in enumerate(calls):
            what = "%s pattern %d call %d (%s)" % (name, pattern, i, call.name)
            out = make(env, call, pattern)
            if pattern == 1:
                call.check(env, out)
                base[i] = out
            else:
                compare(base[i], out, what)
            done += 1
        rc = L.spx_sync(env.ctx)
        assert rc == 0, ("%s pattern %d: spx_sync" % (name, pattern), rc, L.spx_last_error())
    # the growth step: smallest, largest, smallest on a context that has no workspace yet
    small, large = growth
    for pattern in (1, 2, 3):
        env.ctx = env.new_ctx()
        try:
            env.key(104, 1)
            for i in (small, large, small):
                call = calls[i]
                what = "%s growth pattern %d call %d (%s)" % (name, pattern, i, call.name)
                out = make(env, call, pattern)
                if call.regime:
                    call.check(env, out)
                else:
                    compare(base[i], out, what)
                done += 1
            rc = L.spx_sync(env.ctx)
            assert rc == 0, ("%s growth pattern %d: spx_sync" % (name, pattern), rc, L.spx_last_error())
        finally:
            torch.cuda.synchronize()
            L.spx_ctx_destroy(env.ctx)
            env.ctx = env.main
    for k, v in DEFAULT_KEYS.items():
        env.key(k, v)
    env.key(103, 0)
    env.key(104, 0)
    return done


# ---------------------------------------------------------------------------------------------------------------------
# separable value and step, iprox, psi(y)
# ---------------------------------------------------------------------------------------------------------------------
SEP_LAM, SEP_SIGMA = 0.7, 1.1


def build_separable(env):
    nf, orc, L = env.nf, env.orc, env.L
    calls = []
    refs = {}

    def box_tail(box, V):
        if box is None:
            return ()
        if box[2] is None:
            return (None, None, _D(box[0]), _D(box[1]), None)
        return (P(V["lo"]), P(V["up"]), _D(0.0), _D(0.0), P(V["mask"]))

    def oracle_y(kind, form, n, H, box):
        key = ("prox", kind, form, n)
        if key not in refs:
            refs[key] = nf.sep_oracle(orc, kind, box, H["q"], H["x"], H["sj"])
        return refs[key]

    def check_y(kind, box, y, ref, H, what):
        if kind == "lhalf":
            l_u = None if box is None else (box[0], box[1])
            env.arbiter.check_lhalf(orc, y, ref, H["q"], H["x"], H["sj"], SEP_LAM, SEP_SIGMA, box=l_u,
                                    mask=None if box is None else box[2], what=what)
        else:
            nf.check_exact(y, ref, what)

    def h_terms(kind, box, v, n):
        return nf.h_terms(kind, v[nf.sep_selected(box, n)])

    def prox_call(kind, form, fam, n, off8, H, V, keys, target=False):
        box = nf.sep_box(form, H["lo"], H["up"], H["selected"], n)
        sfx = kind + ("" if box is None else "_box")
        fn = getattr(L, "spx_%s_%s" % ({"val": "proxval", "step": "proxstep"}[fam], sfx))
        name = "spx_%s_%s %s n=%d off8=%d keys=%r target=%d" % ({"val": "proxval", "step": "proxstep"}[fam], sfx, form, n, off8, keys, target)

        def run(env):
            y = env.fill(n, off8)
            head = (env.ctx, P(y), P(V["q"]), P(V["x"]), P(V["sj"]), n, _D(SEP_LAM), _D(SEP_SIGMA), *box_tail(box, V))
            out = {}
            if fam == "val":
                v = _D(POISON)
                tgt = env.fill(1, value=POISON) if target else None
                if target:
                    assert L.spx_ctx_set_value_target(env.ctx, P(tgt)) == 0
                try:
                    rc = fn(*head, _D(1.0), ctypes.byref(v))
                finally:
                    L.spx_ctx_set_value_target(env.ctx, None)
                assert rc == 0, (name, rc, L.spx_last_error())
                out["value"] = host(tgt) if target else np.array([v.value])
            else:
                xkn = env.fill(n, off8, POISON)
                st = (_D * 3)(POISON, POISON, POISON)
                sd = env.fill(3, value=POISON)
                rc = fn(*head, _D(1.0), P(xkn), st, P(sd))
                assert rc == 0, (name, rc, L.spx_last_error())
                out["xkn"], out["stats"], out["stats_dev"] = host(xkn), np.array(list(st)), host(sd)
            out["y"] = host(y)
            return out

        def check(env, out):
            y = out["y"]
            check_y(kind, box, y, oracle_y(kind, form, n, H, box), H, name)
            v = (H["x"] + H["sj"]) + y
            if fam == "val":
                sum_bar(out["value"][0], h_terms(kind, box, v, n), name + " value", SEP_LAM, kind == "l0")
            else:
                assert same_bits(out["xkn"], v), (name, "xkn")
                assert same_bits(out["stats"], out["stats_dev"]), (name, out["stats"], out["stats_dev"])
                sum_bar(out["stats"][0], h_terms(kind, box, v, n), name + " [0]", SEP_LAM, kind == "l0")
                sum_bar(out["stats"][1], H["q"] * y, name + " [1]")
                sum_bar(out["stats"][2], y * y, name + " [2]")

        return Call(name, run, check, keys)

    def istep_call(kind, form, n, off8, H, V, keys):
        box = nf.sep_box(form, H["lo"], H["up"], H["selected"], n)
        sfx = kind + ("" if box is None else "_box")
        fn = getattr(L, "spx_iproxstep_" + sfx)
        name = "spx_iproxstep_%s %s n=%d off8=%d keys=%r" % (sfx, form, n, off8, keys)
        d_h, d_d = (H["dpos"], V["dpos"]) if box is None else (H["d"], V["d"])

        def run(env):
            y, xkn = env.fill(n, off8), env.fill(n, off8, POISON)
            st = (_D * 4)(POISON, POISON, POISON, POISON)
            sd = env.fill(4, value=POISON)
            head = (env.ctx, P(y), P(V["q"]), P(d_d), P(V["x"]), P(V["sj"]), n, _D(SEP_LAM))
            if box is None:
                rc = fn(*head, 1, P(xkn), st, None)      # (check_d needs the host form of the statistics)
                sd = None
            else:
                rc = fn(*head, *box_tail(box, V), P(xkn), st, P(sd))
            assert rc == 0, (name, rc, L.spx_last_error())
            out = {"y": host(y), "xkn": host(xkn), "stats": np.array(list(st))}
            if sd is not None:
                out["stats_dev"] = host(sd)
            return out

        def check(env, out):
            y = out["y"]
            key = ("iprox", kind, form, n)
            if key not in refs:
                if box is None:
                    refs[key] = getattr(orc, "iprox_" + kind)(H["q"], d_h, H["x"], H["sj"], SEP_LAM)
                else:
                    refs[key] = getattr(orc, "iprox_%s_box" % kind)(H["q"], d_h, H["x"], H["sj"], SEP_LAM, box[0], box[1], mask=box[2])
            nf.check_exact(y, refs[key], name)
            v = (H["x"] + H["sj"]) + y
            assert same_bits(out["xkn"], v), (name, "xkn")
            if "stats_dev" in out:
                assert same_bits(out["stats"], out["stats_dev"]), (name, out["stats"], out["stats_dev"])
            sum_bar(out["stats"][0], h_terms(kind, box, v, n), name + " [0]", SEP_LAM, kind == "l0")
            sum_bar(out["stats"][1], H["q"] * y, name + " [1]")
            sum_bar(out["stats"][2], (d_h * y) * y, name + " [2]")
            sum_bar(out["stats"][3], y * y, name + " [3]")

        return Call(name, run, check, keys)

    def iprox_flag_call(kind, n, H, V, f32):
        """the plain iprox! with its d > 0 check: the 256-byte flag word"""
        name = "spx_iprox_%s%s check_d n=%d" % (kind, "_f32" if f32 else "", n)
        if f32:
            f = np.float32
            hq, hd, hx, hs = (H[k].astype(f) for k in ("q", "dpos", "x", "sj"))
            dq, dd, dx, ds = (env.dev(a) for a in (hq, hd, hx, hs))
        else:
            hq, hd, hx, hs = H["q"], H["dpos"], H["x"], H["sj"]
            dq, dd, dx, ds = V["q"], V["dpos"], V["x"], V["sj"]

        def run(env):
            y = env.fill(n, dtype=np.float32 if f32 else np.float64)
            rc = getattr(L, "spx_iprox_%s%s" % (kind, "_f32" if f32 else ""))(env.ctx, P(y), P(dq), P(dd), P(dx), P(ds), n,
                                                                             (_F if f32 else _D)(SEP_LAM), 1)
            assert rc == 0, (name, rc, L.spx_last_error())
            return {"y": host(y)}

        def check(env, out):
            if f32:
                ref, bad = orc.iprox_f32(kind, hq, hd, hx, hs, np.float32(SEP_LAM))
                assert bad < 0
                assert same_bits(out["y"], ref), name
            else:
                nf.check_exact(out["y"], getattr(orc, "iprox_" + kind)(hq, hd, hx, hs, SEP_LAM), name)

        return Call(name, run, check)

    def bounds_call(n, H, V, flip):
        name = "spx_check_bounds n=%d flip=%d" % (n, flip)
        up = H["up"].copy()
        if flip:
            up[n - 1] = H["lo"][n - 1] - 1.0
        ud = env.dev(up)

        def run(env):
            flag = ctypes.c_int(-7)
            rc = L.spx_check_bounds(env.ctx, P(V["lo"]), P(ud), _D(0.0), _D(0.0), n, ctypes.byref(flag))
            assert rc == 0, (name, rc, L.spx_last_error())
            return {"flag": np.array([flag.value])}

        def check(env, out):
            assert out["flag"][0] == (1 if flip else 0), (name, out)

        return Call(name, run, check)

    def obj_call(kind, form, n, H, V, keys, target=False):
        box = nf.sep_box(form, H["lo"], H["up"], H["selected"], n)
        sfx = kind + ("" if box is None else "_box")
        name = "spx_obj_%s %s n=%d keys=%r target=%d" % (sfx, form, n, keys, target)
        yh = oracle_y(kind, form, n, H, box)
        yd = env.dev(yh)

        def run(env):
            v = _D(POISON)
            tgt = env.fill(1, value=POISON) if target else None
            if target:
                assert L.spx_ctx_set_value_target(env.ctx, P(tgt)) == 0
            try:
                rc = getattr(L, "spx_obj_" + sfx)(env.ctx, P(yd), P(V["x"]), P(V["sj"]), n, _D(SEP_LAM), *box_tail(box, V), ctypes.byref(v))
            finally:
                L.spx_ctx_set_value_target(env.ctx, None)
            assert rc == 0, (name, rc, L.spx_last_error())
            return {"value": host(tgt) if target else np.array([v.value])}

        def check(env, out):
            exp = orc.obj_plain(kind, yh, H["x"], H["sj"], SEP_LAM) if box is None else \
                orc.obj_box(kind, yh, H["x"], H["sj"], SEP_LAM, box[0], box[1], mask=box[2])
            assert math.isfinite(exp), (name, exp)
            value_bar(out["value"][0], exp, name, kind == "l0")

        return Call(name, run, check, keys)

    for n in (6144, 2 * 3072 + 1):
        x, sj, q, lo, up, selected = nf.separable_data(n, 7700 + n)
        rng = np.random.default_rng(31000 + n)
        d = rng.uniform(0.5, 2.0, size=n)
        r = rng.random(n)
        d = np.where(r < 0.15, 0.0, np.where(r < 0.30, -d, d))       # (the Box forms accept any d: tests/test_gpu_iproxstep.py)
        mask = np.zeros(n, dtype=np.uint8)
        mask[np.asarray(selected, dtype=np.int64)] = 1
        H = dict(x=x, sj=sj, q=q, lo=lo, up=up, selected=selected, d=d, dpos=np.abs(d) + (d == 0.0), mask=mask)
        for off8 in (False, True):
            V = {k: env.dev(H[k], off8) for k in ("x", "sj", "q", "lo", "up", "d", "dpos", "mask")}
            for kind, form in nf.SEP_OPS:
                for k17 in (1, 0):
                    calls.append(prox_call(kind, form, "val", n, off8, H, V, {17: k17}))
                    calls.append(prox_call(kind, form, "step", n, off8, H, V, {17: k17}))
                if not off8:
                    calls.append(prox_call(kind, form, "step", n, off8, H, V, {3: 0, 0: 2}))          # a capped grid
                    calls.append(prox_call(kind, form, "val", n, off8, H, V, {3: 0, 0: 2, 17: 0}))
                    calls.append(prox_call(kind, form, "step", n, off8, H, V, {5: 1}))                # idle workgroups of k_sep_lds
                    calls.append(prox_call(kind, form, "val", n, off8, H, V, {5: 1, 17: 0}))
            for kind in ("l1", "l0"):
                for form in ("plain", "box", "vecbox+mask"):
                    for k17 in (1, 0):
                        calls.append(istep_call(kind, form, n, off8, H, V, {17: k17}))
                if not off8:
                    calls.append(istep_call(kind, "plain", n, off8, H, V, {5: 1}))
                    calls.append(istep_call(kind, "vecbox+mask", n, off8, H, V, {3: 0, 0: 2}))
            if not off8:
                calls.append(prox_call("l1", "plain", "val", n, off8, H, V, {}, target=True))
                for kind in ("l1", "l0"):
                    calls.append(iprox_flag_call(kind, n, H, V, False))
                    calls.append(iprox_flag_call(kind, n, H, V, True))
                calls.append(bounds_call(n, H, V, 0))
                calls.append(bounds_call(n, H, V, 1))
                for kind, form in nf.SEP_OPS:
                    for k17 in (1, 0):
                        calls.append(obj_call(kind, form, n, H, V, {17: k17}))
                calls.append(obj_call("l1", "plain", n, H, V, {}, target=True))
    calls += build_psi_groups(env)
    first = lambda prefix: next(i for i, c in enumerate(calls) if c.name.startswith(prefix))
    # growth: the 256 bytes of spx_check_bounds, then the four planes of partials of spx_iproxstep_l1 at n = 6145
    return calls, (first("spx_check_bounds"), first("spx_iproxstep_l1 plain n=6145"))


def build_psi_groups(env):
    """psi(y) on contiguous groups: few uniform large groups (the one-launch chunks), CSR offsets with one group above the
    4096-element chunk among small ones (the chunk sums, the prefix table), and index sets (the gather form)"""
    orc, L = env.orc, env.L
    calls = []

    def obj_call(tag, n, off_h, gsize, ng, lam, binf, keys, seed):
        rng = np.random.default_rng(seed)
        x, sj = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n)
        y = 0.3 * rng.normal(size=n)
        delta = 4.0                                  # |sj + y| < 1.1 Delta everywhere: a finite value
        xd, sd, yd, ld = (env.dev(a) for a in (x, sj, y, lam))
        od = env.dev(off_h) if off_h is not None else None
        name = "spx_obj_group_l2%s %s keys=%r" % ("_binf" if binf else "", tag, keys)

        def run(env):
            v = _D(POISON)
            head = (env.ctx, P(yd), P(xd), P(sd), n, P(od), gsize, ng, P(ld))
            rc = L.spx_obj_group_l2_binf(*head, _D(delta), ctypes.byref(v)) if binf else L.spx_obj_group_l2(*head, ctypes.byref(v))
            assert rc == 0, (name, rc, L.spx_last_error())
            return {"value": np.array([v.value])}

        def check(env, out):
            kw = dict(offsets=off_h) if off_h is not None else dict(gsize=gsize)
            exp = orc.obj_group_l2(y, x, sj, lam, delta=delta if binf else None, **kw)
            assert math.isfinite(exp) and exp > 0
            value_bar(out["value"][0], exp, name)

        return Call(name, run, check, keys)

    for binf in (False, True):
        for k17 in (1, 0):
            lam = np.array([0.4, 1.3, 0.0])
            calls.append(obj_call("uniform 3 x 9000", 27000, None, 9000, 3, lam, binf, {17: k17}, 611))
    sizes = np.array([10, 50000, 7, 0, 33])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    lam = np.array([0.5, 0.9, 1.5, 2.0, 0.25])

    def gather_call(binf):
        rng = np.random.default_rng(4200 + 16 + binf)
        gs, ng = 16, 500
        n = ng * gs + 7
        groups = [list(range(k, ng * gs, ng)) for k in range(ng)]
        x, sj, y = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), 0.3 * rng.normal(size=n)
        lam = rng.uniform(0.3, 1.5, size=ng)
        ptr = np.arange(0, ng * gs + 1, gs, dtype=np.int64)
        index = np.array([i for g in groups for i in g], dtype=np.int64)
        xd, sd, yd, ld, pd, idd = (env.dev(a) for a in (x, sj, y, lam, ptr, index))
        name = "spx_obj_group_l2%s_gather" % ("_binf" if binf else "")

        def run(env):
            v = _D(POISON)
            head = (env.ctx, P(yd), P(xd), P(sd), n, P(pd), P(idd), ng, len(index), P(ld))
            rc = L.spx_obj_group_l2_binf_gather(*head, _D(4.0), ctypes.byref(v)) if binf else L.spx_obj_group_l2_gather(*head, ctypes.byref(v))
            assert rc == 0, (name, rc, L.spx_last_error())
            return {"value": np.array([v.value])}

        def check(env, out):
            value_bar(out["value"][0], orc.obj_group_l2_idx(y, x, sj, lam, groups, delta=4.0 if binf else None), name)

        return Call(name, run, check)

    calls += [gather_call(False), gather_call(True)]
    for binf in (False, True):
        calls.append(obj_call("csr one large", int(off[-1]), off, 0, 5, lam, binf, {}, 612))
    return calls


# ---------------------------------------------------------------------------------------------------------------------
# top-r
# ---------------------------------------------------------------------------------------------------------------------
def build_topr(env):
    orc, L = env.orc, env.L
    calls = []
    DELTA = 0.75
    tops = {}

    def data(kind, n):
        rng = np.random.default_rng(5000 + n)
        if kind == "lattice":          # the cut lies inside a class: the tie scan
            q = np.round(rng.normal(size=n) * 4) / 4
            return np.zeros(n), np.zeros(n), q
        if kind == "moderate":         # 5000 candidates share the cut's key: the candidate select
            q = rng.normal(size=n)
            at = rng.choice(n, size=min(5000, n // 4), replace=False)
            q[at] = np.where(rng.random(at.size) < 0.5, 1.0, -1.0)
            return np.zeros(n), np.zeros(n), q
        if kind == "sorted":           # the band is contiguous in the vector: the overflow list
            return np.zeros(n), np.zeros(n), np.sort(rng.normal(size=n))
        return rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)

    def call(kind, n, r, keys, f32=False, off8=False, aliased=False, binf=True):
        dt = np.float32 if f32 else np.float64
        x, sj, q = (a.astype(dt) for a in data(kind, n))
        if kind == "moderate":
            r = int((np.abs(q) > 1.0).sum()) + min(5000, n // 4) // 2
        xd, sd, qd = (env.dev(a, off8) for a in (x, sj, q))
        sfx = ("_binf" if binf else "") + ("_f32" if f32 else "")
        name = "spx_prox_indball_l0%s %s n=%d r=%d off8=%d aliased=%d keys=%r" % (sfx, kind, n, r, off8, aliased, keys)

        def run(env):
            y = env.dev(q, off8) if aliased else env.fill(n, off8, dtype=dt)
            head = (env.ctx, P(y), P(y if aliased else qd), P(xd), P(sd), n, r)
            rc = getattr(L, "spx_prox_indball_l0" + sfx)(*head, *(((_F if f32 else _D)(DELTA),) if binf else ()))
            assert rc == 0, (name, rc, L.spx_last_error())
            return {"y": host(y)}

        def check(env, out):
            if f32:
                ref = orc.prox_indball_l0_f32(q, x, sj, r, np.float32(DELTA) if binf else None)
            else:
                key = (kind, n)
                if key not in tops:
                    tops.clear()                 # (one order at a time: 2^21 elements each)
                    tops[key] = orc.TopR(q, x, sj)
                ref = tops[key].prox(r, DELTA) if binf else tops[key].prox(r)
            assert same_bits(out["y"], ref), name

        return Call(name, run, check, keys)

    for f32 in (False, True):
        for n in (5000, 70_001):
            for kind in ("continuous", "lattice"):
                calls.append(call(kind, n, n // 10, {}, f32=f32))
    small = 0
    n = 300_000
    for kind in ("continuous", "lattice"):
        calls.append(call(kind, n, n // 3, {8: 4}))
        calls.append(call(kind, n, n // 3, {8: 4, 2: 0}))
    n = (1 << 21) + 3001                                             # the sample-predicted pipeline (key 11 = 0: nothing parked in LDS)
    calls.append(call("continuous", n, n // 100, {11: 0}))
    calls.append(call("continuous", n, n // 2, {11: 0}, off8=True))  # the aligned rest + element 0
    calls.append(call("continuous", n, 777, {11: 0}, binf=False))
    calls.append(call("lattice", n, n // 3, {11: 0}))
    calls.append(call("lattice", n, n // 3, {11: 0}, aliased=True))  # y === q: the two-pass form (k_sel_final_q)
    calls.append(call("moderate", n, 0, {11: 0}))
    calls.append(call("sorted", n, n // 3, {11: 0}))
    calls.append(call("continuous", n, n // 100, {11: 0, 2: 0}))     # key 2 = 0: the exact select at the same size
    large = len(calls) - 5                                           # (the lattice call of the pipeline)
    return calls, (small, large)


# ---------------------------------------------------------------------------------------------------------------------
# group operators
# ---------------------------------------------------------------------------------------------------------------------
def build_group(env):
    nf, orc, L, arbiter = env.nf, env.orc, env.L, env.arbiter
    calls = []

    class Layout:
        def __init__(self, D, off8=False):
            self.D, self.off8 = D, off8
            self.xd, self.sd, self.qd = (env.dev(a, off8) for a in (D.x, D.sj, D.q))
            self.ld = env.dev(D.lam)
            self.od = env.dev(D.offsets) if D.offsets is not None else None
            self.ref = None

        def oracle(self):
            if self.ref is None:
                self.ref = self.D.oracle(orc, self.D.q, self.D.x, self.D.sj, y0=YFILL)
            return self.ref

    def call(Lay, fam, keys, tag):
        D = Lay.D
        sfx = "_binf" if D.binf else ""
        fn = getattr(L, "spx_%s_group_l2%s" % (fam, sfx))
        name = "spx_%s_group_l2%s %s off8=%d keys=%r" % (fam, sfx, tag, Lay.off8, keys)

        def run(env):
            y = env.fill(D.n, Lay.off8)
            head = (env.ctx, P(y), P(Lay.qd), P(Lay.xd), P(Lay.sd), D.n, P(Lay.od), D.gsize, D.ng, P(Lay.ld), _D(D.sigma),
                    *((_D(D.delta),) if D.binf else ()))
            out = {}
            if fam == "prox":
                rc = fn(*head)
            elif fam == "proxval":
                v = _D(POISON)
                rc = fn(*head, _D(1.0), ctypes.byref(v))
                out["value"] = np.array([v.value])
            else:
                xkn = env.fill(D.n, Lay.off8, POISON)
                st = (_D * 3)(POISON, POISON, POISON)
                sd = env.fill(3, value=POISON)
                rc = fn(*head, _D(1.0), P(xkn), st, P(sd))
                out["xkn"], out["stats"], out["stats_dev"] = host(xkn), np.array(list(st)), host(sd)
            assert rc == 0, (name, rc, L.spx_last_error())
            out["y"] = host(y)
            return out

        def check(env, out):
            y = out["y"]
            nf.check_group(orc, arbiter, y, Lay.oracle(), D.q, D.x, D.sj, D.lam, D.sigma, D.csr, D.delta if D.binf else None, name)
            kw = dict(offsets=D.offsets) if D.offsets is not None else dict(gsize=D.gsize)
            if fam == "proxval":
                value_bar(out["value"][0], orc.obj_group_l2(y, D.x, D.sj, D.lam, **kw), name + " value")
            if fam == "proxstep":
                assert same_bits(out["xkn"], (D.x + D.sj) + y), (name, "xkn")
                assert same_bits(out["stats"], out["stats_dev"]), (name, out["stats"], out["stats_dev"])
                value_bar(out["stats"][0], orc.obj_group_l2(y, D.x, D.sj, D.lam, **kw), name + " [0]")
                sum_bar(out["stats"][1], D.q * y, name + " [1]")
                sum_bar(out["stats"][2], y * y, name + " [2]")

        return Call(name, run, check, keys)

    small = None
    for binf in (False, True):
        for layout in (("uniform", 8), ("uniform", 128), ("csr_over", 0), ("csr_bound", 0)):
            for off8 in ((False, True) if layout == ("uniform", 8) else (False,)):
                Lay = Layout(nf.GroupData(layout, binf), off8)
                for k17 in (1, 0):
                    for fam in ("prox", "proxval", "proxstep"):
                        calls.append(call(Lay, fam, {17: k17}, "%s%s" % layout))
                        if small is None and fam == "proxval":
                            small = len(calls) - 1
        # the team forms: one group over the vector (on chip; key 14 = 0: the generic body), few large groups, and -- key 8 = 4
        # -- one streamed group on a team of four (Binf: the sample-predicted form and, key 14 = 0, the generic one)
        Lay = Layout(nf.GroupData(("one", 120_000), binf))
        for k14 in (1, 0):
            for fam in ("prox", "proxval", "proxstep"):
                calls.append(call(Lay, fam, {14: k14}, "one120000"))
        Lay = Layout(nf.GroupData(("uniform", 5000), binf))
        for fam in ("prox", "proxstep"):
            calls.append(call(Lay, fam, {}, "uniform5000"))
        Lay = Layout(nf.GroupData(("one", 50_001), binf))
        for k14 in (1, 0):
            for fam in ("prox", "proxstep"):
                calls.append(call(Lay, fam, {8: 4, 14: k14}, "one50001"))
    large = len(calls) - 1
    calls += build_group_plan_and_gather(env)
    return calls, (small, large)


def build_group_plan_and_gather(env):
    """a ragged layout with large groups (tests/test_gpu_team.py::test_few_workgroups_resident: the device-side plan of the team
    form, more large groups than workgroups under key 8 = 4, and the default grid) and index-set groups (the gather scratch)"""
    orc, L, arbiter = env.orc, env.L, env.arbiter
    calls = []
    n = 6 * 50_000
    rng = np.random.default_rng(41)
    x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
    off = np.array([0, 50_000, 110_000, 150_000, 150_010, 220_000, 260_000, n], dtype=np.int64)
    lam = np.full(7, 30.0)
    xd, sd, qd, ld, od = (env.dev(a) for a in (x, sj, q, lam, off))
    refs = {}

    def plan_call(binf, keys):
        name = "spx_prox_group_l2%s ragged plan keys=%r" % ("_binf" if binf else "", keys)

        def run(env):
            y = env.fill(n)
            head = (env.ctx, P(y), P(qd), P(xd), P(sd), n, P(od), 0, 7, P(ld), _D(1.0))
            rc = L.spx_prox_group_l2_binf(*head, _D(1.0)) if binf else L.spx_prox_group_l2(*head)
            assert rc == 0, (name, rc, L.spx_last_error())
            return {"y": host(y)}

        def check(env, out):
            if binf not in refs:
                refs[binf] = orc.prox_group_l2_binf(q, x, sj, lam, 1.0, 1.0, offsets=off) if binf else orc.prox_group_l2(q, x, sj, lam, 1.0, offsets=off)
            arbiter.check_group(orc, out["y"], refs[binf], q, x, sj, lam, 1.0, off, delta=1.0 if binf else None, what=name, max_arbitrated=8)

        return Call(name, run, check, keys)

    for binf in (False, True):
        calls.append(plan_call(binf, {8: 4}))
        calls.append(plan_call(binf, {}))

    def gather_call(binf):
        g = np.random.default_rng(4200 + 16 + binf)
        gs, ng = 16, 500
        m = ng * gs + 7                                   # the last 7 indices are in no group
        groups = [list(range(k, ng * gs, ng)) for k in range(ng)]
        gx, gsj, gq, y0 = g.normal(size=m), g.uniform(-0.5, 0.5, size=m), g.normal(size=m), g.normal(size=m)
        glam = g.uniform(0.3, 1.5, size=ng)
        ptr = np.arange(0, ng * gs + 1, gs, dtype=np.int64)
        index = np.array([i for grp in groups for i in grp], dtype=np.int64)
        dx, ds, dq, dl, dp, di = (env.dev(a) for a in (gx, gsj, gq, glam, ptr, index))
        name = "spx_prox_group_l2%s_gather" % ("_binf" if binf else "")

        def run(env):
            y = env.dev(y0)
            head = (env.ctx, P(y), P(dq), P(dx), P(ds), m, P(dp), P(di), ng, len(index), P(dl), _D(0.9))
            rc = L.spx_prox_group_l2_binf_gather(*head, _D(0.8)) if binf else L.spx_prox_group_l2_gather(*head)
            assert rc == 0, (name, rc, L.spx_last_error())
            return {"y": host(y)}

        def check(env, out):
            ref = orc.prox_group_l2_idx(gq, gx, gsj, glam, 0.9, groups, delta=0.8 if binf else None, y0=y0)
            S = (gq + gx) + gsj
            scale = np.abs(ref).copy()
            for grp in groups:
                scale[grp] = np.maximum(scale[grp], np.linalg.norm(S[grp]))
            bad = np.abs(out["y"] - ref) > TOL * np.maximum(scale, 1e-300)
            assert not bad.any(), (name, int(bad.sum()))
            assert same_bits(out["y"][ng * gs:], ref[ng * gs:]), name

        return Call(name, run, check)

    calls += [gather_call(False), gather_call(True)]
    return calls


# ---------------------------------------------------------------------------------------------------------------------
# ShiftedNormL1B2
# ---------------------------------------------------------------------------------------------------------------------
def build_b2(env):
    nf, orc, L = env.nf, env.orc, env.L
    ACTIVE, INACTIVE = 1.0, 1e6
    calls = []
    refs = {}
    devs = {}

    def vecs(n, off8):
        if (n, off8) not in devs:
            x, sj, q = nf.b2_data(n)
            devs[(n, off8)] = tuple(env.dev(a, off8) for a in (x, sj, q))
        return devs[(n, off8)]

    def call(fam, n, delta, keys, off8=False, xkn_off8=None):
        x, sj, q = nf.b2_data(n)
        xd, sd, qd = vecs(n, off8)
        xkn_off8 = off8 if xkn_off8 is None else xkn_off8
        name = "spx_%s_l1_b2 n=%d delta=%g off8=%d xkn_off8=%d keys=%r" % (fam, n, delta, off8, xkn_off8, keys)

        def run(env):
            y = env.fill(n, off8)
            head = (env.ctx, P(y), P(qd), P(xd), P(sd), n, _D(1.0), _D(1.0), _D(delta), _D(1.0))
            out = {}
            if fam == "prox":
                rc = L.spx_prox_l1_b2(*head)
            elif fam == "proxval":
                v = _D(POISON)
                rc = L.spx_proxval_l1_b2(*head, _D(1.0), ctypes.byref(v))
                out["value"] = np.array([v.value])
            else:
                xkn = env.fill(n, xkn_off8, POISON)
                st = (_D * 3)(POISON, POISON, POISON)
                sdv = env.fill(3, value=POISON)
                rc = L.spx_proxstep_l1_b2(*head, _D(1.0), P(xkn), st, P(sdv))
                out["xkn"], out["stats"], out["stats_dev"] = host(xkn), np.array(list(st)), host(sdv)
            assert rc == 0, (name, rc, L.spx_last_error())
            out["y"] = host(y)
            return out

        def check(env, out):
            if (n, delta) not in refs:
                refs[(n, delta)] = orc.prox_l1_b2(q, x, sj, 1.0, 1.0, delta, 1.0)
            y = out["y"]
            nf.check_b2(y, refs[(n, delta)], x, name)
            h = np.abs((x + sj) + y)
            if fam == "proxval":
                sum_bar(out["value"][0], h, name + " value")
            if fam == "proxstep":
                assert same_bits(out["xkn"], (x + sj) + y), (name, "xkn")
                assert same_bits(out["stats"], out["stats_dev"]), (name, out["stats"], out["stats_dev"])
                sum_bar(out["stats"][0], h, name + " [0]")
                sum_bar(out["stats"][1], q * y, name + " [1]")
                sum_bar(out["stats"][2], y * y, name + " [2]")

        return Call(name, run, check, {**keys, 8: 4}, regime=True)

    def obj_call(n):
        x, sj, q = nf.b2_data(n)
        xd, sd, _ = vecs(n, False)
        y = 0.001 * q
        yd = env.dev(y)
        name = "spx_obj_l1_b2 n=%d" % n

        def run(env):
            v = _D(POISON)
            rc = L.spx_obj_l1_b2(env.ctx, P(yd), P(xd), P(sd), n, _D(0.7), _D(1e6), ctypes.byref(v))
            assert rc == 0, (name, rc, L.spx_last_error())
            return {"value": np.array([v.value])}

        def check(env, out):
            value_bar(out["value"][0], orc.obj_l1_b2(y, x, sj, 0.7, 1e6), name)

        return Call(name, run, check)

    # register, LDS, streaming, streaming with many tiles (key 8 = 4: tests/test_gpu_proxstep_b2.py).  Every run of regimes ends
    # on an inactive call: the first call of the next pattern follows what the first call of pattern 1 followed on a new context
    for n in (20_001, 50_001, 70_001, 300_001):
        for delta in (INACTIVE, ACTIVE, ACTIVE, INACTIVE):
            calls.append(call("prox", n, delta, {}))
            calls.append(call("proxval", n, delta, {}))
            for k18 in (0, 1):
                calls.append(call("proxstep", n, delta, {18: k18}))
        for delta in (ACTIVE, INACTIVE):
            calls.append(call("proxstep", n, delta, {}, off8=False, xkn_off8=True))    # mixed alignment: xkn alone 8 bytes off
            calls.append(call("proxstep", n, delta, {}, off8=True))
            calls.append(call("proxstep", n, delta, {18: 1}, off8=True, xkn_off8=False))
        calls.append(call("prox", n, INACTIVE, {}))
    calls.append(obj_call(20_001))
    large = len(calls) - 3
    return calls, (3, large)                                  # spx_proxstep_l1_b2, key 18 = 1, at n = 20 001 and at n = 300 001


# ---------------------------------------------------------------------------------------------------------------------
# host-pointer forms
# ---------------------------------------------------------------------------------------------------------------------
def build_host(env):
    nf, orc, L, arbiter = env.nf, env.orc, env.L, env.arbiter

    def H(a):
        return ctypes.c_void_p(a.ctypes.data)

    def family(n):
        rng = np.random.default_rng(4000 + n)
        x, sj, q = rng.normal(size=n), rng.uniform(-0.5, 0.5, size=n), rng.normal(size=n)
        g, d = rng.normal(size=n), rng.choice([1.0, -1.0, 0.0], size=n) * rng.uniform(0.2, 3.0, size=n)
        yq = q * 0.1
        lam, sigma = 0.7, 0.9
        r = max(1, n // 10)
        sizes = [1, 5, 64, 129, n - 234, 2, 33]
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        glam = rng.uniform(0.2, 2.0, size=len(sizes))
        out = []

        def add(tag, fn, chk):
            name = "spx_host_%s n=%d" % (tag, n)

            def run(env):
                y = np.full(n, YFILL)
                v = _D(POISON)
                rc = fn(env.ctx, y, v)
                assert rc == 0, (name, rc, L.spx_last_error())
                return {"y": y, "value": np.array([v.value])}

            out.append(Call(name, run, lambda env, o, chk=chk, name=name: chk(o, name)))

        def bits(ref):
            return lambda o, name: nf.check_exact(o["y"], ref(), name)

        add("prox_l1_box", lambda c, y, v: L.spx_host_prox_l1_box(c, H(y), H(q), H(x), H(sj), n, _D(lam), _D(sigma), None, None, _D(-0.8), _D(0.8), None),
            bits(lambda: orc.prox_l1_box(q, x, sj, lam, sigma, -0.8, 0.8)))
        add("prox_l0", lambda c, y, v: L.spx_host_prox_l0(c, H(y), H(q), H(x), H(sj), n, _D(lam), _D(sigma)),
            bits(lambda: orc.prox_l0(q, x, sj, lam, sigma)))
        add("iprox_l1_box", lambda c, y, v: L.spx_host_iprox_l1_box(c, H(y), H(g), H(d), H(x), H(sj), n, _D(0.6), None, None, _D(-0.7), _D(0.9), None),
            bits(lambda: orc.iprox_l1_box(g, d, x, sj, 0.6, -0.7, 0.9)))
        add("obj_l1", lambda c, y, v: L.spx_host_obj_l1(c, H(yq), H(x), H(sj), n, _D(0.6), ctypes.byref(v)),
            lambda o, name: value_bar(o["value"][0], orc.obj_plain("l1", yq, x, sj, 0.6), name))
        add("prox_indball_l0_binf", lambda c, y, v: L.spx_host_prox_indball_l0_binf(c, H(y), H(q), H(x), H(sj), n, r, _D(0.6)),
            bits(lambda: orc.prox_indball_l0_binf(q, x, sj, r, 0.6)))
        add("prox_group_l2_binf",
            lambda c, y, v: L.spx_host_prox_group_l2_binf(c, H(y), H(q), H(x), H(sj), n, H(off), 0, len(sizes), H(glam), _D(sigma), _D(0.9)),
            lambda o, name: arbiter.check_group(orc, o["y"], orc.prox_group_l2_binf(q, x, sj, glam, sigma, 0.9, offsets=off), q, x, sj, glam,
                                                sigma, off, delta=0.9, what=name))
        add("prox_l1_b2", lambda c, y, v: L.spx_host_prox_l1_b2(c, H(y), H(q), H(x), H(sj), n, _D(lam), _D(sigma), _D(0.8), _D(1.0)),
            lambda o, name: nf.check_b2(o["y"], orc.prox_l1_b2(q, x, sj, lam, sigma, 0.8, 1.0), x, name))
        return out

    big, little = family(4097), family(513)          # then the same at n = 513: a staging block larger than the call needs
    calls = big + little
    return calls, (len(big), 0)                      # growth: n = 513, n = 4097, n = 513 (ShiftedNormL1Box)


# ---------------------------------------------------------------------------------------------------------------------
# the four batched libraries: the tiled form (the only one that reserves)
# ---------------------------------------------------------------------------------------------------------------------
R, TILE = 12288, 3072


def _rows(env, n, rows, seed):
    rng = np.random.default_rng(seed)
    H = dict(X=rng.normal(size=(rows, n)), SJ=rng.uniform(-0.5, 0.5, size=(rows, n)), Q=rng.normal(size=(rows, n)))
    H["lam"], H["sig"], H["qs"], H["dl"] = (rng.uniform(0.3, 1.5, size=rows) for _ in range(4))
    return H, rng


def _dev2(env, a, pad=1):
    """rows x n as a view of a flat buffer with row stride n + pad"""
    torch = env.torch
    rows, n = a.shape
    ld = n + pad
    flat = torch.full((rows * ld + 2,), POISON, dtype=torch.float64, device="cuda:0")
    v = flat[:rows * ld].as_strided((rows, n), (ld, 1))
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v


def build_batch(env, long_reduce=True):
    orc, nf = env.orc, env.nf
    torch = env.torch
    LB = env.s._lib.load_batch()
    calls = []

    def call(kind, box, msk, n, rows, xkn, seed):
        H, rng = _rows(env, n, rows, seed)
        mask = np.zeros(n, dtype=np.uint8)
        mask[rng.choice(n, size=max(1, n // 3), replace=False)] = 1
        Xd, Sd, Qd = (_dev2(env, H[k]) for k in ("X", "SJ", "Q"))
        P1 = {k: env.dev(H[k]) for k in ("lam", "sig", "qs", "dl")}
        md, lo = env.dev(mask), env.dev(-H["dl"])
        name = "spx_proxstep_%s%s_batch mask=%d n=%d rows=%d xkn=%d" % (kind, "_box" if box else "", msk, n, rows, xkn)

        def run(env):
            Y, K = _dev2(env, np.full((rows, n), YFILL)), (_dev2(env, np.full((rows, n), POISON)) if xkn else None)
            out = torch.full((rows, 3), POISON, dtype=torch.float64, device="cuda:0")
            head = (env.ctx, P(Y), P(Qd), P(Xd), P(Sd), n, rows, n + 1, P(P1["lam"]), P(P1["sig"]))
            if box:
                rc = getattr(LB, "spx_proxstep_%s_box_batch" % kind)(*head, P(lo), P(P1["dl"]), P(md) if msk else None, P(P1["qs"]), P(K), P(out))
            else:
                rc = getattr(LB, "spx_proxstep_%s_batch" % kind)(*head, P(P1["qs"]), P(K), P(out))
            assert rc == 0, (name, rc, env.L.spx_last_error())
            res = {"y": host(Y), "stats": host(out)}
            if xkn:
                res["xkn"] = host(K)
            return res

        def check(env, out):
            for b in range(rows):
                what = "%s row %d" % (name, b)
                qb = H["qs"][b] * H["Q"][b]                      # one rounded multiply per element
                if box:
                    ref = getattr(orc, "prox_%s_box" % kind)(qb, H["X"][b], H["SJ"][b], H["lam"][b], H["sig"][b], -H["dl"][b], H["dl"][b],
                                                            mask=mask if msk else None)
                else:
                    ref = getattr(orc, "prox_" + kind)(qb, H["X"][b], H["SJ"][b], H["lam"][b], H["sig"][b])
                y = out["y"][b]
                nf.check_exact(y, ref, what)
                v = (H["X"][b] + H["SJ"][b]) + y
                if xkn:
                    assert same_bits(out["xkn"][b], v), (what, "xkn")
                if n > (1 << 20) and b != rows - 1:              # (millions of terms through math.fsum: the last row's sums)
                    continue
                sel = mask.astype(bool) if msk else np.ones(n, dtype=bool)
                sum_bar(out["stats"][b, 0], nf.h_terms(kind, v[sel]), what + " [0]", H["lam"][b], kind == "l0")
                sum_bar(out["stats"][b, 1], H["Q"][b] * y, what + " [1]")
                sum_bar(out["stats"][b, 2], y * y, what + " [2]")

        return Call(name, run, check)

    for kind, box, msk in (("l1", False, False), ("l0", True, True), ("l1", True, False), ("l0", False, False)):
        calls.append(call(kind, box, msk, R + 1, 3, True, 7100 + R + 1))
        calls.append(call(kind, box, msk, R + 1, 3, False, 7100 + R + 1))
    if long_reduce:
        calls.append(call("l1", True, False, 2048 * TILE + 1, 2, True, 7400))     # 2049 tiles: the long reduce loop
    return calls, (0, len(calls) - 1)


def build_ibatch(env):
    orc, nf = env.orc, env.nf
    torch = env.torch
    LB = env.s._lib.load_ibatch()
    calls = []

    def call(kind, box, msk, n, rows, xkn, seed, shift):
        H, rng = _rows(env, n, rows, seed)
        D = rng.uniform(0.5, 2.0, size=(rows, n))
        if box:
            r = rng.random((rows, n))
            D = np.where(r < 0.15, 0.0, np.where(r < 0.30, -D, D))
        dsh = rng.uniform(0.1, 0.9, size=rows)
        mask = np.zeros(n, dtype=np.uint8)
        mask[rng.choice(n, size=max(1, n // 3), replace=False)] = 1
        Xd, Sd, Gd, Dd = (_dev2(env, a) for a in (H["X"], H["SJ"], H["Q"], D))
        P1 = {k: env.dev(H[k]) for k in ("lam", "dl")}
        dshd, md, lo = env.dev(dsh), env.dev(mask), env.dev(-H["dl"])
        name = "spx_iproxstep_%s%s_batch mask=%d n=%d rows=%d xkn=%d d_shift=%d" % (kind, "_box" if box else "", msk, n, rows, xkn, shift)

        def run(env):
            Y, K = _dev2(env, np.full((rows, n), YFILL)), (_dev2(env, np.full((rows, n), POISON)) if xkn else None)
            out = torch.full((rows, 4), POISON, dtype=torch.float64, device="cuda:0")
            flag = None if box else torch.full((rows,), -7, dtype=torch.int32, device="cuda:0")
            head = (env.ctx, P(Y), P(Gd), P(Dd), P(Xd), P(Sd), n, rows, n + 1, P(P1["lam"]), P(dshd) if shift else None)
            if box:
                rc = getattr(LB, "spx_iproxstep_%s_box_batch" % kind)(*head, P(lo), P(P1["dl"]), P(md) if msk else None, P(K), P(out))
            else:
                rc = getattr(LB, "spx_iproxstep_%s_batch" % kind)(*head, P(flag), P(K), P(out))
            assert rc == 0, (name, rc, env.L.spx_last_error())
            res = {"y": host(Y), "stats": host(out)}
            if xkn:
                res["xkn"] = host(K)
            if flag is not None:
                res["d_flag"] = host(flag)
            return res

        def check(env, out):
            for b in range(rows):
                what = "%s row %d" % (name, b)
                deff = D[b] + dsh[b] if shift else D[b]          # one rounded add per element
                if box:
                    ref = getattr(orc, "iprox_%s_box" % kind)(H["Q"][b], deff, H["X"][b], H["SJ"][b], H["lam"][b], -H["dl"][b], H["dl"][b],
                                                             mask=mask if msk else None)
                else:
                    ref = getattr(orc, "iprox_" + kind)(H["Q"][b], deff, H["X"][b], H["SJ"][b], H["lam"][b])
                    assert out["d_flag"][b] == 0, (what, out["d_flag"])
                y = out["y"][b]
                nf.check_exact(y, ref, what)
                v = (H["X"][b] + H["SJ"][b]) + y
                if xkn:
                    assert same_bits(out["xkn"][b], v), (what, "xkn")
                if n > (1 << 20) and b != rows - 1:              # (millions of terms through math.fsum: the last row's sums)
                    continue
                sel = mask.astype(bool) if msk else np.ones(n, dtype=bool)
                sum_bar(out["stats"][b, 0], nf.h_terms(kind, v[sel]), what + " [0]", H["lam"][b], kind == "l0")
                sum_bar(out["stats"][b, 1], H["Q"][b] * y, what + " [1]")
                sum_bar(out["stats"][b, 2], (deff * y) * y, what + " [2]")
                sum_bar(out["stats"][b, 3], y * y, what + " [3]")

        return Call(name, run, check)

    for kind, box, msk in (("l1", False, False), ("l0", True, True), ("l1", True, False), ("l0", False, False)):
        calls.append(call(kind, box, msk, R + 1, 3, True, 7600 + R + 1, True))
        calls.append(call(kind, box, msk, R + 1, 3, False, 7600 + R + 1, False))
    calls.append(call("l1", False, False, 2048 * TILE + 1, 2, True, 7700, True))
    return calls, (0, len(calls) - 1)


def _build_gbatch(env, binf):
    orc, arbiter = env.orc, env.arbiter
    torch = env.torch
    LB = env.s._lib.load_gbinf_batch() if binf else env.s._lib.load_gbatch()
    calls = []

    def call(gs, ng, rows, xkn, seed):
        n = gs * ng
        H, rng = _rows(env, n, rows, seed)
        S = (H["qs"][:, None] * H["Q"] + H["X"]) + H["SJ"]
        nS = np.sqrt((S.reshape(rows, ng, gs) ** 2).sum(axis=2))
        lam = np.where(nS > 0, nS, 1.0) * rng.choice([0.3, 0.7, 1.0, 1.5, 4.0], size=(rows, ng)) / H["sig"][:, None]
        Xd, Sd, Qd = (_dev2(env, H[k]) for k in ("X", "SJ", "Q"))
        P1 = {k: env.dev(H[k]) for k in ("sig", "qs", "dl")}
        ld = env.dev(lam.reshape(-1))
        off = np.arange(0, n + 1, gs, dtype=np.int64)
        name = "spx_proxstep_group_l2%s_batch gs=%d ng=%d rows=%d xkn=%d" % ("_binf" if binf else "", gs, ng, rows, xkn)

        def run(env):
            Y, K = _dev2(env, np.full((rows, n), YFILL)), (_dev2(env, np.full((rows, n), POISON)) if xkn else None)
            out = torch.full((rows, 3), POISON, dtype=torch.float64, device="cuda:0")
            head = (env.ctx, P(Y), P(Qd), P(Xd), P(Sd), gs, ng, rows, n + 1, P(ld), ng, None, P(P1["sig"]))
            if binf:
                rc = LB.spx_proxstep_group_l2_binf_batch(*head, P(P1["dl"]), P(P1["qs"]), P(K), P(out))
            else:
                rc = LB.spx_proxstep_group_l2_batch(*head, P(P1["qs"]), P(K), P(out))
            assert rc == 0, (name, rc, env.L.spx_last_error())
            res = {"y": host(Y), "stats": host(out)}
            if xkn:
                res["xkn"] = host(K)
            return res

        def check(env, out):
            for b in range(rows):
                what = "%s row %d" % (name, b)
                qb = H["qs"][b] * H["Q"][b]
                x, sj, y = H["X"][b], H["SJ"][b], out["y"][b]
                if binf:
                    ref = orc.prox_group_l2_binf(qb, x, sj, lam[b], H["sig"][b], H["dl"][b], gsize=gs)
                else:
                    ref = orc.prox_group_l2(qb, x, sj, lam[b], H["sig"][b], gsize=gs)
                arbiter.check_group(orc, y, ref, qb, x, sj, lam[b], H["sig"][b], off, delta=H["dl"][b] if binf else None, what=what)
                if xkn:
                    assert same_bits(out["xkn"][b], (x + sj) + y), (what, "xkn")
                value_bar(out["stats"][b, 0], orc.obj_group_l2(y, x, sj, lam[b], gsize=gs), what + " [0]")
                if n > (1 << 20) and b != rows - 1:              # (millions of terms through math.fsum: the last row's sums)
                    continue
                sum_bar(out["stats"][b, 1], H["Q"][b] * y, what + " [1]")
                sum_bar(out["stats"][b, 2], y * y, what + " [2]")

        return Call(name, run, check)

    for gs in (128, 33):
        ng = R // gs + 1
        calls.append(call(gs, ng, 3, True, 9100 + gs))
        calls.append(call(gs, ng, 3, False, 9100 + gs))
    calls.append(call(512, 4 * 2048 + 4, 2, True, 9200))          # 2049 tiles of four groups: the long reduce loop
    return calls, (0, len(calls) - 1)


def build_lhalf_batch(env):
    """spx_proxstep_lhalf[_box]_batch through the same run_batch (csrc/spx_batch_device.hpp) and the same partials as the NormL1 /
    NormL0 calls, tiled form only (n > 12288).  The bar of tests/test_gpu_proxstep_lhalf_batch.py: every row the bits of the
    single call on that row (made on a context of its own, whose scratch is not the one under test), with the band rule of
    include/spx_lhalf_batch.h for the unboxed threshold, and the oracle through arbiter.check_lhalf; the sums within 1e-12 of
    sum |term| of math.fsum.  spx_lhalf_threshold_batch reserves nothing (one small kernel): it is used here, on the other
    context, to read the device's thresholds, and is not a call of the case."""
    orc, nf, arbiter, L = env.orc, env.nf, env.arbiter, env.L
    torch = env.torch
    LB = env.s._lib.load_lhalf_batch()
    calls = []
    refctx = env.new_ctx()

    def p_host(lam, sig):
        return 54.0 ** (1 / 3) * (2 * (float(sig) * float(lam))) ** (2 / 3) / 4

    def stationary(a, lam, sig):
        """the oracle's formula for the stationary point at sol = a (oracle/spx_oracle.c)"""
        phi = np.arccos(sig * lam / 4 * (np.abs(a) / 3) ** -1.5)
        return 2.0 / 3.0 * a * (1 + np.cos(2 * np.pi / 3 - 2.0 / 3.0 * phi))

    def call(box, msk, n, rows, xkn, seed):
        H, rng = _rows(env, n, rows, seed)
        mask = np.zeros(n, dtype=np.uint8)
        mask[rng.choice(n, size=max(1, n // 3), replace=False)] = 1
        Xd, Sd, Qd = (_dev2(env, H[k]) for k in ("X", "SJ", "Q"))
        P1 = {k: env.dev(H[k]) for k in ("lam", "sig", "qs", "dl")}
        md, lo = env.dev(mask), env.dev(-H["dl"])
        name = "spx_proxstep_lhalf%s_batch mask=%d n=%d rows=%d xkn=%d" % ("_box" if box else "", msk, n, rows, xkn)
        single = {}

        def run(env):
            Y, K = _dev2(env, np.full((rows, n), YFILL)), (_dev2(env, np.full((rows, n), POISON)) if xkn else None)
            out = torch.full((rows, 3), POISON, dtype=torch.float64, device="cuda:0")
            head = (env.ctx, P(Y), P(Qd), P(Xd), P(Sd), n, rows, n + 1, P(P1["lam"]), P(P1["sig"]))
            if box:
                rc = LB.spx_proxstep_lhalf_box_batch(*head, P(lo), P(P1["dl"]), P(md) if msk else None, P(P1["qs"]), P(K), P(out))
            else:
                rc = LB.spx_proxstep_lhalf_batch(*head, P(P1["qs"]), P(K), P(out))
            assert rc == 0, (name, rc, L.spx_last_error())
            res = {"y": host(Y), "stats": host(out)}
            if xkn:
                res["xkn"] = host(K)
            return res

        def single_call(b):
            """spx_proxstep_lhalf[_box] on row b with host copies of its scalars, on the other context: (y, xkn)"""
            if b not in single:
                q, x, sj = (env.dev(H[k][b]) for k in ("Q", "X", "SJ"))
                y, k = env.fill(n), env.fill(n, value=POISON)
                st = (_D * 3)()
                lam, sig, qs, dl = (float(H[k][b]) for k in ("lam", "sig", "qs", "dl"))
                if box:
                    rc = L.spx_proxstep_lhalf_box(refctx, P(y), P(q), P(x), P(sj), n, lam, sig, None, None, -dl, dl, P(md) if msk else None,
                                                  qs, P(k), st, None)
                else:
                    rc = L.spx_proxstep_lhalf(refctx, P(y), P(q), P(x), P(sj), n, lam, sig, qs, P(k), st, None)
                assert rc == 0, (name, "single call", rc, L.spx_last_error())
                single[b] = (host(y), host(k))
            return single[b]

        def thresholds():
            pd = env.fill(rows, value=POISON)
            rc = LB.spx_lhalf_threshold_batch(refctx, P(P1["lam"]), P(P1["sig"]), rows, P(pd))
            assert rc == 0, (name, "threshold", rc, L.spx_last_error())
            assert L.spx_sync(refctx) == 0
            return host(pd)

        def check(env, out):
            pd = None if box else thresholds()
            for b in range(rows):
                what = "%s row %d" % (name, b)
                lam, sig, qs, dl = (float(H[k][b]) for k in ("lam", "sig", "qs", "dl"))
                q, x, sj = H["Q"][b], H["X"][b], H["SJ"][b]
                qb = qs * q                                       # one rounded multiply per element
                y = out["y"][b]
                ys, ks = single_call(b)
                xs = x + sj
                band = np.zeros(n, dtype=bool)
                if not box:                                       # the band rule: between the host's threshold and the device's
                    ph = p_host(lam, sig)
                    assert abs(pd[b] - ph) <= 4 * np.spacing(ph), (what, pd[b], ph)
                    a = np.abs(qb + xs)
                    band = (a <= ph) != (a <= pd[b])
                    for i in np.flatnonzero(band):
                        if a[i] <= pd[b]:
                            assert y[i] == 0.0 - xs[i], (what, i)
                        else:
                            st = stationary(np.array([qb[i] + xs[i]]), lam, sig)[0] - xs[i]
                            assert abs(y[i] - st) <= TOL * max(abs(y[i]), abs(xs[i]), abs(q[i])), (what, i)
                assert same_bits(y[~band], ys[~band]), (what, "the single call's bits")
                if xkn:
                    assert same_bits(out["xkn"][b], xs + y), (what, "xkn")
                    assert same_bits(out["xkn"][b][~band], ks[~band]), (what, "the single call's xkn")
                m = mask if msk else None
                with np.errstate(all="ignore"):
                    if box:
                        ref = orc.prox_lhalf_box(qb, x, sj, lam, sig, -dl, dl, mask=m)
                    else:
                        ref = orc.prox_lhalf(qb, x, sj, lam, sig)
                    yo = np.where(band, ref, y)                   # (the band's elements were held to their branch above)
                    arbiter.check_lhalf(orc, yo, ref, qb, x, sj, lam, sig, box=(-dl, dl) if box else None, mask=m, what=what)
                v = xs + y
                sel = mask.astype(bool) if msk else np.ones(n, dtype=bool)
                sum_bar(out["stats"][b, 0], nf.h_terms("lhalf", v[sel]), what + " [0]", lam)
                sum_bar(out["stats"][b, 1], q * y, what + " [1]")
                sum_bar(out["stats"][b, 2], y * y, what + " [2]")

        return Call(name, run, check)

    n = R + TILE + 1                                                  # 15 361: five tiles and one element
    for box, msk in ((False, False), (True, False), (True, True)):
        calls.append(call(box, msk, n, 3, True, 7800 + n))
        calls.append(call(box, msk, n, 3, False, 7800 + n))
    calls.append(call(True, True, R + 6 * TILE + 1, 3, True, 7900))   # 30 721: the growth step's larger block
    return calls, (0, len(calls) - 1)


def _b2_chi0(q, xk, sj, ls):
    """chi(ProjB(-xk)) = ||min(max(-xk, (sj + q) - ls), (sj + q) + ls)||: the radius below which the trust region is active"""
    sq = sj + q
    return math.sqrt(fsum(np.minimum(np.maximum(-xk, sq - ls), sq + ls) ** 2))


def build_row_batch(env):
    """The one-workgroup-per-row batched calls, spx_proxstep_l1_b2_batch and spx_proxstep_indball_l0[_binf]_batch, at n = 1000
    (the row in registers) and n = 8200 (the row walk), rows = 3, ld = n (the pairs form) and ld = n + 1 (element-wise),
    against the oracle at the bars of tests/test_gpu_proxstep_b2_batch.py and tests/test_gpu_proxstep_topr_batch.py.
    -> (the warm-up call that grows the workspace, the calls)"""
    orc, L = env.orc, env.L
    torch = env.torch
    LB2, LT = env.s._lib.load_b2_batch(), env.s._lib.load_topr_batch()
    calls = []
    rows = 3

    def data(n, pad, seed):
        H, rng = _rows(env, n, rows, seed)
        D = {k: _dev2(env, H[k], pad) for k in ("X", "SJ", "Q")}
        return H, rng, D

    def outputs(n, pad):
        Y, K = _dev2(env, np.full((rows, n), YFILL), pad), _dev2(env, np.full((rows, n), POISON), pad)
        return Y, K, torch.full((rows, 3), POISON, dtype=torch.float64, device="cuda:0")

    def b2_call(n, pad):
        H, rng, D = data(n, pad, 8300 + n)
        H["lam"] = rng.uniform(0.05, 0.6, size=rows)
        dl = np.empty(rows)
        kinds = ["active", "inactive", "active"]
        for b in range(rows):
            c = _b2_chi0(H["qs"][b] * H["Q"][b], H["X"][b], H["SJ"][b], H["lam"][b] * H["sig"][b])
            dl[b] = 0.3 * c if kinds[b] == "active" else 2.0 * c + 1.0
        P1 = {k: env.dev(a) for k, a in (("lam", H["lam"]), ("sig", H["sig"]), ("qs", H["qs"]), ("dl", dl))}
        name = "spx_proxstep_l1_b2_batch n=%d rows=%d ld=n+%d" % (n, rows, pad)

        def run(env):
            Y, K, out = outputs(n, pad)
            rc = LB2.spx_proxstep_l1_b2_batch(env.ctx, P(Y), P(D["Q"]), P(D["X"]), P(D["SJ"]), n, rows, n + pad, P(P1["lam"]), P(P1["sig"]),
                                              P(P1["dl"]), P(P1["qs"]), _D(1.0), P(K), P(out))
            assert rc == 0, (name, rc, L.spx_last_error())
            return {"y": host(Y), "xkn": host(K), "stats": host(out)}

        def check(env, out):
            for b in range(rows):
                what = "%s row %d (%s)" % (name, b, kinds[b])
                q, x, sj, lam = H["Q"][b], H["X"][b], H["SJ"][b], float(H["lam"][b])
                ref = orc.prox_l1_b2(H["qs"][b] * q, x, sj, lam, float(H["sig"][b]), float(dl[b]))
                y = out["y"][b]
                scale = max(float(np.linalg.norm(ref)), float(np.linalg.norm(x)))
                err = float(np.max(np.abs(y - ref)))
                assert np.isfinite(y).all() and err <= TOL * scale, (what, err, scale)
                v = (x + sj) + y
                assert same_bits(out["xkn"][b], v), (what, "xkn")
                sum_bar(out["stats"][b, 0], np.abs(v), what + " [0]", lam)
                sum_bar(out["stats"][b, 1], q * y, what + " [1]")
                sum_bar(out["stats"][b, 2], y * y, what + " [2]")
                if kinds[b] == "inactive":
                    assert same_bits(y, ref), (what, "an inactive row equals the oracle")
                else:
                    nrm = math.sqrt(fsum((sj + y) ** 2))
                    assert abs(nrm - dl[b]) <= TOL * dl[b], (what, nrm, dl[b])

        return Call(name, run, check)

    def topr_call(binf, n, pad):
        H, rng, D = data(n, pad, 8400 + n)
        r = np.array([n // 100, n // 2, n - 1], dtype=np.int64)
        rd = env.dev(r)
        P1 = {k: env.dev(H[k]) for k in ("qs", "dl")}
        name = "spx_proxstep_indball_l0%s_batch n=%d rows=%d ld=n+%d" % ("_binf" if binf else "", n, rows, pad)

        def run(env):
            Y, K, out = outputs(n, pad)
            head = (env.ctx, P(Y), P(D["Q"]), P(D["X"]), P(D["SJ"]), n, rows, n + pad, P(rd))
            if binf:
                rc = LT.spx_proxstep_indball_l0_binf_batch(*head, P(P1["dl"]), P(P1["qs"]), P(K), P(out))
            else:
                rc = LT.spx_proxstep_indball_l0_batch(*head, P(P1["qs"]), P(K), P(out))
            assert rc == 0, (name, rc, L.spx_last_error())
            return {"y": host(Y), "xkn": host(K), "stats": host(out)}

        def check(env, out):
            for b in range(rows):
                what = "%s row %d" % (name, b)
                q, x, sj = H["Q"][b], H["X"][b], H["SJ"][b]
                top = orc.TopR(H["qs"][b] * q, x, sj)
                ref = top.prox(int(r[b]), float(H["dl"][b])) if binf else top.prox(int(r[b]))
                y = out["y"][b]
                assert same_bits(y, ref), (what, "against the oracle")
                v = (x + sj) + y
                assert same_bits(out["xkn"][b], v), (what, "xkn")
                assert float(out["stats"][b, 0]) == float(np.count_nonzero(v != 0.0)), (what, "[0]", out["stats"][b, 0])
                sum_bar(out["stats"][b, 1], q * y, what + " [1]")
                sum_bar(out["stats"][b, 2], y * y, what + " [2]")

        return Call(name, run, check)

    for n in (1000, 8192 + 8):
        for pad in (0, 1):
            calls.append(b2_call(n, pad))
            calls.append(topr_call(False, n, pad))
            calls.append(topr_call(True, n, pad))
    warm = build_batch(env, long_reduce=False)[0][0]                  # spx_proxstep_l1_batch, tiled: n = 12 289, rows = 3
    assert warm.name.startswith("spx_proxstep_l1_batch mask=0 n=%d" % (R + 1)), warm.name
    return warm, calls


def run_no_ws(name):
    """the calls that reserve nothing, on a context whose workspace an earlier tiled call has grown (see the module's text)"""
    env = Env()
    L = env.L
    warm, calls = NO_WS_BUILDERS[name](env)
    env.key(104, 1)
    warm.check(env, make(env, warm, 1))
    assert L.spx_sync(env.ctx) == 0
    sys.stdout.flush()
    print("NO_WS_BEGIN", flush=True)
    base = {}
    done = 0
    for pattern in (1, 2, 3):
        for i, call in enumerate(calls):
            what = "%s pattern %d call %d (%s)" % (name, pattern, i, call.name)
            out = make(env, call, pattern)
            if pattern == 1:
                call.check(env, out)
                base[i] = out
            else:
                compare(base[i], out, what)
            done += 1
        rc = L.spx_sync(env.ctx)
        assert rc == 0, ("%s pattern %d: spx_sync" % (name, pattern), rc, L.spx_last_error())
    print("NO_WS_END", flush=True)
    env.key(103, 0)
    env.key(104, 0)
    return done


BUILDERS = {"separable": build_separable, "topr": build_topr, "group": build_group, "b2": build_b2, "host": build_host,
            "batch": build_batch, "ibatch": build_ibatch, "gbatch": lambda env: _build_gbatch(env, False),
            "gbinf_batch": lambda env: _build_gbatch(env, True), "lhalf_batch": build_lhalf_batch}
NO_WS_BUILDERS = {"row_batch": build_row_batch}


def main(argv):
    name = argv[1]
    try:
        done = run_no_ws(name) if name in NO_WS_CASES else run_case(name)
    except BaseException as e:           # (the first mismatch ends the case)
        traceback.print_exc()
        sys.stdout.flush()
        print("RESULT FAIL %s: %s" % (name, " ".join(str(e).split())[:1500]), flush=True)
        return 1
    print("RESULT ok %d" % done, flush=True)
    return 0


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    sys.exit(main(sys.argv))
