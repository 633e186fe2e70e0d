"""prox! + h(xk + s) of ShiftedGroupNormL2 / ShiftedGroupNormL2Binf: (a) the plain prox!, (b) prox! then psi(y) as two calls,
(c) the fused spx_proxval_group_l2[_binf] -- warm, HIP-event stopwatch on the context's stream, value in a device double (no
read-back in any leg).  The three legs of a shape alternate round by round; the figure is the median round.

    timeout -k 10 900 python tools/group_proxval_timing.py [--out profiles/group_proxval_timing.txt] [--quick]

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
ap.add_argument("--quick", action="store_true", help="n <= 1e6 only (a rehearsal of the tool, not a measurement)")
args = ap.parse_args()

s = ge.build()
L = s._lib.load()
dev = torch.device("cuda:0")
ctx = s.context(dev)
gen = torch.Generator(device=dev).manual_seed(7)
_D = ctypes.c_double
# (groups, group size): BASELINE group shape, small groups, a partly filled tile at n = 1e8, two latency shapes; then the composed
# routes (LDS-resident groups, one group over the vector) for the record
SHAPES = [(1_000_000, 128), (12_500_000, 8), (1_000_000, 100), (78, 128), (7_812, 128), (100_000, 1000), (1, 4_000_000)]
if args.quick:
    SHAPES = [(78, 128), (7_812, 128), (10_000, 100), (1_000, 1000)]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


lines = ["# (a) prox!  (b) prox! then psi(y), two calls  (c) fused spx_proxval_group_*   [ms per call, median of the rounds]",
         "# device: %s" % torch.cuda.get_device_name(0),
         "%-24s %10s %6s %-9s %9s %9s %9s %7s %7s" % ("operator", "groups", "size", "route", "(a)", "(b)", "(c)", "(c)/(b)", "(c)/(a)")]
print("\n".join(lines), flush=True)
target = torch.zeros(1, dtype=torch.float64, device=dev)
s._lib.check(L.spx_ctx_set_value_target(ctx, ptr(target)))
try:
    for ng, gs in SHAPES:
        n = ng * gs
        xk = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
        sj = torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5
        q = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
        y = torch.empty_like(q)
        # sigma * lambda around ||S_g|| ~ 1.45 sqrt(gs): zeroed and active groups both occur
        lam = (torch.rand(ng, dtype=torch.float64, device=dev, generator=gen) + 0.5) * 1.45 * gs ** 0.5
        host = _D(0.0)
        for binf in (False, True):
            tail = (_D(1.0),) if binf else ()
            sfx = "_binf" if binf else ""
            head = (ctx, ptr(y), ptr(q), ptr(xk), ptr(sj), n, None, gs, ng, ptr(lam), _D(1.0))

            def leg_a():
                s._lib.check(getattr(L, "spx_prox_group_l2" + sfx)(*head, *tail))

            def leg_b():
                leg_a()
                s._lib.check(L.spx_obj_group_l2(ctx, ptr(y), ptr(xk), ptr(sj), n, None, gs, ng, ptr(lam), ctypes.byref(host)))

            def leg_c():
                s._lib.check(getattr(L, "spx_proxval_group_l2" + sfx)(*head, *tail, _D(1.0), ctypes.byref(host)))

            legs = (leg_a, leg_b, leg_c)
            inner = 5 if n >= 10_000_000 else 50
            rounds = 7
            vals = []
            for leg in legs:                      # warm every leg (code objects, workspace sizes) and keep its value
                leg(); leg()
                s._lib.check(L.spx_sync(ctx))
                vals.append(float(target.item()))
            assert vals[1] == vals[1] and abs(vals[2] - vals[1]) <= 1e-12 * abs(vals[1]), vals   # (c) and (b) return the same h
            ts = [[], [], []]
            for _ in range(rounds):               # the legs alternate: drift of the box hits all three alike
                for k, leg in enumerate(legs):
                    ms = ctypes.c_float()
                    s._lib.check(L.spx_timer_start(ctx))
                    for _ in range(inner):
                        leg()
                    s._lib.check(L.spx_timer_stop(ctx, ctypes.byref(ms)))
                    ts[k].append(ms.value / inner)
            a, b, c = (sorted(t)[len(t) // 2] for t in ts)
            route = "fused" if gs <= 512 else "composed"
            line = "%-24s %10d %6d %-9s %9.4f %9.4f %9.4f %7.3f %7.3f" % ("ShiftedGroupNormL2" + ("Binf" if binf else ""), ng, gs,
                                                                            route, a, b, c, c / b, c / a)
            lines.append(line)
            print(line, flush=True)
        del xk, sj, q, y, lam
finally:
    s._lib.check(L.spx_ctx_set_value_target(ctx, None))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
