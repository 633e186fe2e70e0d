"""prox! + step statistics of the separable operators: what one spx_proxstep_X call costs against what a caller does today.

    (a) spx_proxval_X                                   y and h            32 B/element
    (b) spx_proxval_X, torch.dot(q, y), torch.add(xk, y, out=xkn), torch.dot(y, y)      four launches or more, 72-80 B/element
    (c) spx_proxstep_X with xkn                         y, xkn, h, qy, yy  40 B/element, one launch
    (d) spx_proxstep_X without xkn                      y, h, qy, yy       32 B/element, one launch

Warm, HIP-event stopwatch on the context's stream, every result in device doubles (no read-back in any leg).  The legs of a
shape alternate round by round; the figure is the median round, the spread (max - min) / median of the rounds of (a) is
printed beside it.  With --parent-lib PATH (a libspx.so built from the parent commit) leg (a) is also timed on that build, in
the same rounds, and so are (c) and (d) when that build has spx_proxstep_*: they must not have moved -- new / parent of each
is to be read against the spread of repeating (a) on one build, which is measured as a second, independent series of (a) in
the same rounds: the last column says whether every ratio lies within max(spread, |(a') / (a) - 1|) of 1.

    timeout -k 10 900 python tools/proxstep_timing.py [--out profiles/proxstep_timing.txt] [--quick] [--parent-lib PATH]
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -- python tools/proxstep_timing.py --one    # a profile of its own

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
ap.add_argument("--parent-lib", default=None, help="libspx.so of the parent commit: leg (a), and (c), (d) if it has them, are timed on it too")
ap.add_argument("--one", action="store_true", help="only 20 calls of spx_proxstep_l1_box at n = 1e8 (for a profiler run)")
args = ap.parse_args()

s = ge.build()
L = s._lib.load()
dev = torch.device("cuda:0")
ctx = s.context(dev)
gen = torch.Generator(device=dev).manual_seed(11)
_D = ctypes.c_double


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def check_rc(lib, rc):
    if rc != 0:
        raise RuntimeError("status %d: %s" % (rc, lib.spx_last_error().decode()))


# the parent build, loaded beside this one: its own context on the same stream
LP = ctxp = None
parent_step = False
if args.parent_lib:
    LP = ctypes.CDLL(os.path.abspath(args.parent_lib))
    for name, sig in s._lib.SIGNATURES.items():
        if hasattr(LP, name):
            getattr(LP, name).argtypes = sig
            getattr(LP, name).restype = ctypes.c_char_p if name == "spx_last_error" else ctypes.c_int
    parent_step = hasattr(LP, "spx_proxstep_l1")
    ctxp = ctypes.c_void_p()
    check_rc(LP, LP.spx_ctx_create_on_stream(0, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), ctypes.byref(ctxp)))

OPS = ["l1", "l1_box scalar", "l1_box vec+mask", "lhalf_box scalar"]
SIZES = [100_000_000, 10_000_000, 1_000_000, 10_000]
if args.quick:
    SIZES = [1_000_000, 10_000]
if args.one:
    OPS, SIZES = ["l1_box scalar"], [100_000_000]

lines = ["# (a) spx_proxval_X  (b) proxval + dot(q, y) + add(xk, y, out=xkn) + dot(y, y)  (c) spx_proxstep_X with xkn  (d) without xkn",
         "# [ms per call, median of the rounds; spread = (max - min) / median of the rounds of (a)]",
         "# (a') = a second, independent series of (a) on this build; (x-parent) = (x) on the parent commit's build, same rounds",
         "# a/par, c/par, d/par = this build over the parent's; within: every one of them within max(spread, |(a')/(a) - 1|) of 1",
         "# device: %s" % torch.cuda.get_device_name(0),
         "%-18s %10s %9s %9s %9s %9s %7s %7s %7s | %9s %9s %8s %8s" % ("operator", "n", "(a)", "(b)", "(c)", "(d)", "(c)/(b)", "(c)/(a)",
                                                                          "(d)/(a)", "(a')", "(a-parent)", "spread", "par/(a)")
         + (" | %10s %10s %7s %7s %7s %6s" % ("(c-parent)", "(d-parent)", "a/par", "c/par", "d/par", "within") if parent_step else "")]
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
        lo = -1.0 - 0.1 * torch.rand(n, dtype=torch.float64, device=dev, generator=gen)
        up = 1.0 + 0.1 * torch.rand(n, dtype=torch.float64, device=dev, generator=gen)
        mask = (torch.rand(n, device=dev, generator=gen) < 0.6).to(torch.uint8)
        dots = torch.zeros(2, dtype=torch.float64, device=dev)
        host = _D(0.0)
        for op in OPS:
            sym, form = op.split()[0], (op.split() + ["plain"])[1]
            vec = (ptr(y), ptr(q), ptr(xk), ptr(sj), n, _D(0.7), _D(1.1))
            if sym.endswith("_box"):
                box = (ptr(lo), ptr(up), _D(0.0), _D(0.0), ptr(mask)) if form == "vec+mask" else (None, None, _D(-0.9), _D(0.9), None)
            else:
                box = ()
            qs = _D(-0.9)

            def leg_a(lib=L, c=ctx):
                check_rc(lib, getattr(lib, "spx_proxval_" + sym)(c, *vec, *box, qs, ctypes.byref(host)))

            def leg_b():
                leg_a()
                torch.dot(q, y, out=dots[0])
                torch.add(xk, y, out=xkn)
                torch.dot(y, y, out=dots[1])

            def leg_c(lib=L, c=ctx):
                check_rc(lib, getattr(lib, "spx_proxstep_" + sym)(c, *vec, *box, qs, ptr(xkn), None, ptr(stats)))

            def leg_d(lib=L, c=ctx):
                check_rc(lib, getattr(lib, "spx_proxstep_" + sym)(c, *vec, *box, qs, None, None, ptr(stats)))

            legs = [leg_a, leg_b, leg_c, leg_d, leg_a]
            if LP is not None:
                legs.append(lambda: leg_a(LP, ctxp))
            if parent_step:
                legs += [lambda: leg_c(LP, ctxp), lambda: leg_d(LP, ctxp)]
            if args.one:
                for _ in range(20):
                    leg_c()
                torch.cuda.synchronize()
                continue
            for leg in legs:                      # warm every leg (code objects, workspace sizes)
                leg(); leg()
            torch.cuda.synchronize()
            # (c) returns the h of (a), and its sums are those of leg (b)
            leg_b(); torch.cuda.synchronize()
            h_a, qy_b, yy_b = float(target.item()), float(dots[0]), float(dots[1])
            leg_c(); torch.cuda.synchronize()
            h_c, qy_c, yy_c = stats.tolist()
            assert h_c == h_a, (op, n, h_c, h_a)
            assert abs(qy_c - qy_b) <= 1e-9 * max(1.0, abs(yy_b)) and abs(yy_c - yy_b) <= 1e-9 * abs(yy_b), (qy_c, qy_b, yy_c, yy_b)
            inner = 5 if n >= 10_000_000 else 50
            rounds = 3 if args.quick else 9
            ts = [[] for _ in legs]
            for _ in range(rounds):               # the legs alternate: drift of the box hits all of them alike
                for k, leg in enumerate(legs):
                    ms = ctypes.c_float()
                    s._lib.check(L.spx_timer_start(ctx))
                    for _ in range(inner):
                        leg()
                    s._lib.check(L.spx_timer_stop(ctx, ctypes.byref(ms)))
                    ts[k].append(ms.value / inner)
            med = [sorted(t)[len(t) // 2] for t in ts]
            a, b, c, d, a2 = med[:5]
            spread = (max(ts[0]) - min(ts[0])) / a
            par = med[5] if LP is not None else float("nan")
            line = "%-18s %10d %9.4f %9.4f %9.4f %9.4f %7.3f %7.3f %7.3f | %9.4f %9.4f %7.1f%% %8.3f" % (
                op, n, a, b, c, d, c / b, c / a, d / a, a2, par, 100.0 * spread, par / a)
            if parent_step:
                cp, dp = med[6], med[7]
                tol = max(spread, abs(a2 / a - 1.0))
                ok = all(abs(r - 1.0) <= tol for r in (a / par, c / cp, d / dp))
                line += " | %10.4f %10.4f %7.3f %7.3f %7.3f %6s" % (cp, dp, a / par, c / cp, d / dp, "yes" if ok else "NO")
            lines.append(line)
            print(line, flush=True)
        del xk, sj, q, y, xkn, lo, up, mask
finally:
    s._lib.check(L.spx_ctx_set_value_target(ctx, None))
    if LP is not None:
        check_rc(LP, LP.spx_ctx_set_value_target(ctxp, None))
if args.out and not args.one:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
