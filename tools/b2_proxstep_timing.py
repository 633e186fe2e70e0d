"""prox! + step statistics of ShiftedNormL1B2: what one spx_proxstep_l1_b2 call costs against what a caller does today.

    (a)  spx_proxval_l1_b2                              y and h            56 B/element on the streaming form (40 inactive)
    (b)  (a), torch.dot(q, y), torch.add(xk, y, out=xkn), torch.dot(y, y)   three more launches, 48 B/element more
    (c)  spx_proxstep_l1_b2 with xkn                    y, xkn, h, qy, yy  64 B/element (40 + 8 inactive), one launch where fused
    (d)  spx_proxstep_l1_b2 without xkn                 y, h, qy, yy
    (c') (c) with tuning key 18 = 1: the composed route on every form

Warm, HIP-event stopwatch on the context's stream, every result in device doubles (no read-back in any leg).  The legs of a
shape alternate round by round; the figure is the median of 7 rounds; the spread (max - min) / median of the rounds is printed
for (a) and for (b) -- (c) is to be read against (b) and its spread.  With --parent-lib PATH (a libspx.so built from the parent
commit) leg (a) is also timed on that build, in the same rounds: the difference is to be read against the spread of repeating
(a) on one build, which is measured as a second, independent series of (a) in the same rounds.

    timeout -k 10 900 python tools/b2_proxstep_timing.py [--out profiles/b2_proxstep_timing.txt] [--quick] [--parent-lib PATH]

One process, every status checked, no retry: a failing call ends the run with its message."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the table to this file")
ap.add_argument("--quick", action="store_true", help="n <= 1e6 only, fewer rounds (a rehearsal of the tool, not a measurement)")
ap.add_argument("--parent-lib", default=None, help="libspx.so of the parent commit: leg (a) is timed on it too")
ap.add_argument("--one", action="store_true", help="only 20 calls of the fused call at n = 4e6 (for a profiler run)")
args = ap.parse_args()

s = ge.build()
L = s._lib.load()
dev = torch.device("cuda:0")
ctx = s.context(dev)
gen = torch.Generator(device=dev).manual_seed(7)
_D = ctypes.c_double


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def check_rc(lib, rc):
    if rc != 0:
        raise RuntimeError("status %d: %s" % (rc, lib.spx_last_error().decode()))


LP = ctxp = None
if args.parent_lib:
    LP = ctypes.CDLL(os.path.abspath(args.parent_lib))
    for name, sig in s._lib.SIGNATURES.items():
        if hasattr(LP, name):
            getattr(LP, name).argtypes = sig
            getattr(LP, name).restype = ctypes.c_char_p if name == "spx_last_error" else ctypes.c_int
    assert not hasattr(LP, "spx_proxstep_l1_b2"), "--parent-lib has spx_proxstep_l1_b2: not a build of the parent commit"
    ctxp = ctypes.c_void_p()
    check_rc(LP, LP.spx_ctx_create_on_stream(0, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), ctypes.byref(ctxp)))

# register form, register form at its upper end, LDS form, streaming form
SIZES = [10_000, 1_000_000, 4_000_000, 100_000_000]
if args.quick:
    SIZES = [10_000, 1_000_000]
if args.one:
    SIZES = [4_000_000]
ROUNDS = 3 if args.quick else 7

lines = ["# (a) spx_proxval_l1_b2  (b) (a) + dot(q, y) + add(xk, y, out=xkn) + dot(y, y)  (c) spx_proxstep_l1_b2 with xkn  (d) without xkn  (c') (c), key 18 = 1",
         "# [ms per call, median of %d rounds; spread = (max - min) / median of the rounds of that leg]" % ROUNDS,
         "# (a') = a second, independent series of (a) on this build; (a-parent) = (a) on the parent commit's build, same rounds",
         "# device: %s" % torch.cuda.get_device_name(0),
         "%11s %-9s %8s %8s %8s %8s %8s %7s %7s %8s | %8s %10s %7s %7s" % (
             "n", "region", "(a)", "(b)", "(c)", "(d)", "(c')", "(c)/(b)", "spr(b)", "(c)/(c')", "(a')", "(a-parent)", "spr(a)", "par/(a)")]
print("\n".join(lines), flush=True)
target = torch.zeros(1, dtype=torch.float64, device=dev)
stats = torch.zeros(3, dtype=torch.float64, device=dev)
s._lib.check(L.spx_ctx_set_value_target(ctx, ptr(target)))
if LP is not None:
    check_rc(LP, LP.spx_ctx_set_value_target(ctxp, ptr(target)))
try:
    for n in SIZES:
        xk = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
        sj = torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5
        q = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
        y, xkn = torch.empty_like(q), torch.empty_like(q)
        dots = torch.zeros(2, dtype=torch.float64, device=dev)
        host = _D(0.0)
        for region, delta in (("active", 1.0), ("inactive", 1e6 * n ** 0.5)):
            vec = (ptr(y), ptr(q), ptr(xk), ptr(sj), n, _D(1.0), _D(1.0), _D(delta), _D(1.0))
            qs = _D(-0.9)

            def leg_a(lib=L, c=ctx):
                check_rc(lib, lib.spx_proxval_l1_b2(c, *vec, qs, ctypes.byref(host)))

            def leg_b():
                leg_a()
                torch.dot(q, y, out=dots[0])
                torch.add(xk, y, out=xkn)
                torch.dot(y, y, out=dots[1])

            def leg_c():
                check_rc(L, L.spx_proxstep_l1_b2(ctx, *vec, qs, ptr(xkn), None, ptr(stats)))

            def leg_d():
                check_rc(L, L.spx_proxstep_l1_b2(ctx, *vec, qs, None, None, ptr(stats)))

            def leg_c18():
                s._lib.check(L.spx_ctx_set_tuning(ctx, 18, 1))
                try:
                    leg_c()
                finally:
                    s._lib.check(L.spx_ctx_set_tuning(ctx, 18, 0))

            legs = [leg_a, leg_b, leg_c, leg_d, leg_c18, leg_a]
            if LP is not None:
                legs.append(lambda: leg_a(LP, ctxp))
            for leg in legs:                      # warm every leg (code objects, workspace sizes, the regime of the previous call)
                leg(); leg()
            torch.cuda.synchronize()
            if args.one:
                for _ in range(20):
                    leg_c()
                torch.cuda.synchronize()
                continue
            # (c) returns the h of (a), and its sums are those of leg (b)
            leg_b(); torch.cuda.synchronize()
            h_a, qy_b, yy_b = float(target.item()), float(dots[0]), float(dots[1])
            leg_c(); torch.cuda.synchronize()
            h_c, qy_c, yy_c = stats.tolist()
            assert h_c == h_a, (n, region, h_c, h_a)
            assert abs(qy_c - qy_b) <= 1e-9 * max(1.0, abs(yy_b)) and abs(yy_c - yy_b) <= 1e-9 * abs(yy_b), (qy_c, qy_b, yy_c, yy_b)
            inner = 5 if n >= 10_000_000 else 50
            ts = [[] for _ in legs]
            for _ in range(ROUNDS):               # the legs alternate: drift of the box hits all of them alike
                for k, leg in enumerate(legs):
                    ms = ctypes.c_float()
                    s._lib.check(L.spx_timer_start(ctx))
                    for _ in range(inner):
                        leg()
                    s._lib.check(L.spx_timer_stop(ctx, ctypes.byref(ms)))
                    ts[k].append(ms.value / inner)
            med = [sorted(t)[len(t) // 2] for t in ts]
            a, b, c, d, c18, a2 = med[:6]
            spr_a, spr_b = (max(ts[0]) - min(ts[0])) / a, (max(ts[1]) - min(ts[1])) / b
            par = med[6] if LP is not None else float("nan")
            line = "%11d %-9s %8.4f %8.4f %8.4f %8.4f %8.4f %7.3f %6.1f%% %8.3f | %8.4f %10.4f %6.1f%% %7.3f" % (
                n, region, a, b, c, d, c18, c / b, 100.0 * spr_b, c / c18, a2, par, 100.0 * spr_a, par / a)
            lines.append(line)
            print(line, flush=True)
        del xk, sj, q, y, xkn
finally:
    s._lib.check(L.spx_ctx_set_value_target(ctx, None))
    if LP is not None:
        check_rc(LP, LP.spx_ctx_set_value_target(ctxp, None))
if args.out and not args.one:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
