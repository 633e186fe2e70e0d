"""iprox! + step statistics (spx_iproxstep_*): what one fused call costs against what a caller does today.

    (a) spx_iprox_X alone                                y                       40 B/element
    (b) the caller's sequence today: spx_iprox_X, psi(y) (spx_obj_X), torch.dot(g, y), torch.add(xk, y, out=xkn),
        torch.dot(y, d * y), torch.dot(y, y)             five or six passes, about 128 B/element
    (c) spx_iproxstep_X with xkn                         y, xkn, h, gy, ydy, yy  48 B/element, one launch
    (d) spx_iproxstep_X without xkn                      y, h, gy, ydy, yy       40 B/element, one launch

Warm, HIP-event stopwatch on the context's stream (spx_timer_start / spx_timer_stop), every result in device doubles (the
value target for psi(y), stats_dev for the fused call: no read-back in any leg).  The legs of a shape alternate round by round;
the figure is the median round, the spread (max - min) / median of the rounds of (a) is printed beside it.  The fused call
must beat (b) at every size: the last column says so.

    timeout -k 10 900 python tools/iproxstep_timing.py [--out profiles/iproxstep_timing.txt] [--quick]

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
args = ap.parse_args()

s = ge.build()
L = s._lib.load()
dev = torch.device("cuda:0")
ctx = s.context(dev)
gen = torch.Generator(device=dev).manual_seed(11)
_D = ctypes.c_double


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def check_rc(rc):
    if rc != 0:
        raise RuntimeError("status %d: %s" % (rc, L.spx_last_error().decode()))


OPS = ["l1", "l0", "l1_box scalar", "l1_box vec+mask", "l0_box scalar", "l0_box vec+mask"]
SIZES = [100_000_000, 10_000_000, 1_000_000, 10_000]
if args.quick:
    SIZES = [1_000_000, 10_000]

lines = ["# (a) spx_iprox_X  (b) iprox + psi(y) + dot(g, y) + add(xk, y, out=xkn) + dot(y, d * y) + dot(y, y)  (c) spx_iproxstep_X with xkn  (d) without xkn",
         "# [ms per call, median of the rounds; spread = (max - min) / median of the rounds of (a)]",
         "# device: %s" % torch.cuda.get_device_name(0),
         "%-18s %10s %9s %9s %9s %9s %7s %7s %7s %8s %6s" % ("operator", "n", "(a)", "(b)", "(c)", "(d)", "(c)/(b)", "(c)/(a)", "(d)/(a)",
                                                              "spread", "c<b")]
print("\n".join(lines), flush=True)
target = torch.zeros(1, dtype=torch.float64, device=dev)
stats = torch.zeros(4, dtype=torch.float64, device=dev)
s._lib.check(L.spx_ctx_set_value_target(ctx, ptr(target)))
try:
    for n in SIZES:
        xk = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
        sj = torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5
        g = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
        d = 0.5 + 1.5 * torch.rand(n, dtype=torch.float64, device=dev, generator=gen)
        y, xkn, tmp = torch.empty_like(g), torch.empty_like(g), torch.empty_like(g)
        lo = -1.0 - 0.1 * torch.rand(n, dtype=torch.float64, device=dev, generator=gen)
        up = 1.0 + 0.1 * torch.rand(n, dtype=torch.float64, device=dev, generator=gen)
        mask = (torch.rand(n, device=dev, generator=gen) < 0.6).to(torch.uint8)
        dots = torch.zeros(3, dtype=torch.float64, device=dev)
        host = _D(0.0)
        for op in OPS:
            sym, form = op.split()[0], (op.split() + ["plain"])[1]
            vec = (ptr(y), ptr(g), ptr(d), ptr(xk), ptr(sj), n, _D(0.7))
            if sym.endswith("_box"):
                mid = (ptr(lo), ptr(up), _D(0.0), _D(0.0), ptr(mask)) if form == "vec+mask" else (None, None, _D(-0.9), _D(0.9), None)
            else:
                mid = (0,)                      # check_d = 0: asynchronous
            obj = (ptr(y), ptr(xk), ptr(sj), n, _D(0.7)) + (mid if sym.endswith("_box") else ())

            def leg_a():
                check_rc(getattr(L, "spx_iprox_" + sym)(ctx, *vec, *mid))

            def leg_b():
                leg_a()
                check_rc(getattr(L, "spx_obj_" + sym)(ctx, *obj, ctypes.byref(host)))
                torch.dot(g, y, out=dots[0])
                torch.add(xk, y, out=xkn)
                torch.mul(d, y, out=tmp)
                torch.dot(y, tmp, out=dots[1])
                torch.dot(y, y, out=dots[2])

            def leg_c():
                check_rc(getattr(L, "spx_iproxstep_" + sym)(ctx, *vec, *mid, ptr(xkn), None, ptr(stats)))

            def leg_d():
                check_rc(getattr(L, "spx_iproxstep_" + sym)(ctx, *vec, *mid, None, None, ptr(stats)))

            legs = [leg_a, leg_b, leg_c, leg_d]
            for leg in legs:                      # warm every leg (code objects, workspace sizes)
                leg(); leg()
            torch.cuda.synchronize()
            # (c) returns the sums of leg (b)
            leg_b(); torch.cuda.synchronize()
            ref = [float(target.item())] + dots.tolist()
            leg_c(); torch.cuda.synchronize()
            got = stats.tolist()
            for r, v in zip(ref, got):
                assert abs(v - r) <= 1e-9 * max(1.0, abs(ref[0]), abs(ref[3])), (op, n, got, ref)
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
            a, b, c, dd = [sorted(t)[len(t) // 2] for t in ts]
            spread = (max(ts[0]) - min(ts[0])) / a
            line = "%-18s %10d %9.4f %9.4f %9.4f %9.4f %7.3f %7.3f %7.3f %7.1f%% %6s" % (
                op, n, a, b, c, dd, c / b, c / a, dd / a, 100.0 * spread, "yes" if c < b else "NO")
            lines.append(line)
            print(line, flush=True)
        del xk, sj, g, d, y, xkn, tmp, lo, up, mask
finally:
    s._lib.check(L.spx_ctx_set_value_target(ctx, None))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
