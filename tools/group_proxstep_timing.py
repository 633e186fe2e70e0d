"""prox! + step statistics of the group operators: what one spx_proxstep_group_l2[_binf] call costs against what a caller does today.

    (a) spx_proxval_group_*                             y and h            32 B/element
    (b) spx_proxval_group_*, torch.dot(q, y), torch.add(xk, y, out=xkn), torch.dot(y, y)     four launches or more, 80 B/element
    (c) spx_proxstep_group_* with xkn                   y, xkn, h, qy, yy  40 B/element (fused route)
    (d) spx_proxstep_group_* without xkn                y, h, qy, yy       32 B/element (fused route)

Warm, HIP-event stopwatch on the context's stream, every result in device doubles (no read-back in any leg).  The legs of a
shape alternate round by round; the figure is the median round; the spread (max - min) / median of the rounds is printed for
(a) and for (b) -- (c) is to be read against (b) and its spread.  With --parent-lib PATH (a libspx.so built from the parent
commit) leg (a) is also timed on that build, in the same rounds: (a) must not have moved -- the difference is to be read against
the spread of repeating (a) on one build, which is measured as a second, independent series of (a) in the same rounds.

    timeout -k 10 900 python tools/group_proxstep_timing.py [--out profiles/group_proxstep_timing.txt] [--quick] [--parent-lib PATH]
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -- python tools/group_proxstep_timing.py --one    # a profile of its own

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
ap.add_argument("--one", action="store_true", help="only 20 calls of each leg of the Binf form at 1e6 x 128 (for a profiler run)")
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


# the parent build, loaded beside this one: its own context on the same stream
LP = ctxp = None
if args.parent_lib:
    LP = ctypes.CDLL(os.path.abspath(args.parent_lib))
    for name, sig in s._lib.SIGNATURES.items():
        if hasattr(LP, name):
            getattr(LP, name).argtypes = sig
            getattr(LP, name).restype = ctypes.c_char_p if name == "spx_last_error" else ctypes.c_int
    assert not hasattr(LP, "spx_proxstep_group_l2"), "--parent-lib has spx_proxstep_group_*: not a build of the parent commit"
    ctxp = ctypes.c_void_p()
    check_rc(LP, LP.spx_ctx_create_on_stream(0, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), ctypes.byref(ctxp)))

# (groups, group size): the rows of profiles/group_proxval_timing.txt -- BASELINE group shape, small groups, a partly filled tile at
# n = 1e8, two latency shapes (fused route); then the composed routes (LDS-resident groups, one group over the vector) for the record
SHAPES = [(1_000_000, 128), (12_500_000, 8), (1_000_000, 100), (78, 128), (7_812, 128), (100_000, 1000), (1, 4_000_000)]
if args.quick:
    SHAPES = [(78, 128), (7_812, 128), (10_000, 100), (1_000, 1000)]
if args.one:
    SHAPES = [(1_000_000, 128)]

lines = ["# (a) spx_proxval_group_*  (b) proxval + dot(q, y) + add(xk, y, out=xkn) + dot(y, y)  (c) spx_proxstep_group_* with xkn  (d) without xkn",
         "# [ms per call, median of the rounds; spread = (max - min) / median of the rounds of that leg]",
         "# (a') = a second, independent series of (a) on this build; (a-parent) = (a) on the parent commit's build, same rounds",
         "# device: %s" % torch.cuda.get_device_name(0),
         "%-22s %9s %7s %-8s %8s %8s %8s %8s %7s %7s %7s %7s | %8s %10s %7s %7s" % (
             "operator", "groups", "size", "route", "(a)", "(b)", "(c)", "(d)", "(c)/(b)", "spr(b)", "(c)/(a)", "(d)/(a)", "(a')", "(a-parent)",
             "spr(a)", "par/(a)")]
print("\n".join(lines), flush=True)
target = torch.zeros(1, dtype=torch.float64, device=dev)
stats = torch.zeros(3, dtype=torch.float64, device=dev)
s._lib.check(L.spx_ctx_set_value_target(ctx, ptr(target)))
if LP is not None:
    check_rc(LP, LP.spx_ctx_set_value_target(ctxp, ptr(target)))
try:
    for ng, gs in SHAPES:
        n = ng * gs
        xk = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
        sj = torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5
        q = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
        y, xkn = torch.empty_like(q), torch.empty_like(q)
        # sigma * lambda around ||S_g|| ~ 1.45 sqrt(gs): zeroed and active groups both occur
        lam = (torch.rand(ng, dtype=torch.float64, device=dev, generator=gen) + 0.5) * 1.45 * gs ** 0.5
        dots = torch.zeros(2, dtype=torch.float64, device=dev)
        host = _D(0.0)
        for binf in ((True,) if args.one else (False, True)):
            sfx = "_binf" if binf else ""
            tail = (_D(1.0),) if binf else ()
            vec = (ptr(y), ptr(q), ptr(xk), ptr(sj), n, None, gs, ng, ptr(lam), _D(1.0), *tail)
            qs = _D(-0.9)

            def leg_a(lib=L, c=ctx):
                check_rc(lib, getattr(lib, "spx_proxval_group_l2" + sfx)(c, *vec, qs, ctypes.byref(host)))

            def leg_b():
                leg_a()
                torch.dot(q, y, out=dots[0])
                torch.add(xk, y, out=xkn)
                torch.dot(y, y, out=dots[1])

            def leg_c():
                check_rc(L, getattr(L, "spx_proxstep_group_l2" + sfx)(ctx, *vec, qs, ptr(xkn), None, ptr(stats)))

            def leg_d():
                check_rc(L, getattr(L, "spx_proxstep_group_l2" + sfx)(ctx, *vec, qs, None, None, ptr(stats)))

            legs = [leg_a, leg_b, leg_c, leg_d, leg_a]
            if LP is not None:
                legs.append(lambda: leg_a(LP, ctxp))
            for leg in legs:                      # warm every leg (code objects, workspace sizes)
                leg(); leg()
            torch.cuda.synchronize()
            if args.one:
                for leg in legs[:4]:
                    for _ in range(20):
                        leg()
                torch.cuda.synchronize()
                continue
            # (c) returns the h of (a), and its sums are those of leg (b)
            leg_b(); torch.cuda.synchronize()
            h_a, qy_b, yy_b = float(target.item()), float(dots[0]), float(dots[1])
            leg_c(); torch.cuda.synchronize()
            h_c, qy_c, yy_c = stats.tolist()
            assert h_c == h_a, (gs, binf, h_c, h_a)
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
            spr_a, spr_b = (max(ts[0]) - min(ts[0])) / a, (max(ts[1]) - min(ts[1])) / b
            par = med[5] if LP is not None else float("nan")
            line = "%-22s %9d %7d %-8s %8.4f %8.4f %8.4f %8.4f %7.3f %6.1f%% %7.3f %7.3f | %8.4f %10.4f %6.1f%% %7.3f" % (
                "ShiftedGroupNormL2" + ("Binf" if binf else ""), ng, gs, "fused" if gs <= 512 else "composed", a, b, c, d, c / b,
                100.0 * spr_b, c / a, d / a, a2, par, 100.0 * spr_a, par / a)
            lines.append(line)
            print(line, flush=True)
        del xk, sj, q, y, xkn, lam
finally:
    s._lib.check(L.spx_ctx_set_value_target(ctx, None))
    if LP is not None:
        check_rc(LP, LP.spx_ctx_set_value_target(ctxp, None))
if args.out and not args.one:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
