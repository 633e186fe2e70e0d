"""Batched RootNormLhalf(Box) prox! + step statistics: what one spx_proxstep_lhalf[_box]_batch call (with xkn) costs against what a
caller does today, for both operators.

    (a) spx_proxstep_lhalf[_box]_batch                    batch problems, one call (n > 12288: two launches)
    (b) batch sequential spx_proxstep_lhalf[_box] calls   the same rows, one call each, on the same build, results in device doubles
    (c) the bytes (a) moves -- 40 B/element: q, xk, sj in; y, xkn out -- per microsecond of (a)
    (d) spx_proxstep_l1_box_batch on the same shapes      what the walk does when the functor is cheap
    (e) where batch * n >= 1e7: ONE spx_proxstep_lhalf[_box] call over the concatenated rows with common scalars
    (a') with --alt LIB: (a) through another build of libspx_lhalf_batch.so (csrc/build.sh -DSPX_LHALF_BATCH_STAGES=K under
         SPX_LIB_NAME): the kStages decision of DESIGN.md 5.5c

Warm, HIP-event stopwatch on the context's (launching) stream, nothing read back in any leg.  The legs of a shape alternate round
by round; the figure is the median round, spread = (max - min) / median of the rounds of the leg.  Leg (b) is driven through
ctypes like every caller of the C ABI from Python: where its launches are shorter than the host's call overhead, (b) measures
that overhead -- which is what such a caller pays.  Before a shape is timed the rows of (a) are compared with the rows of (b): y and
xkn bit for bit (the unboxed operator: on every element that is not within 4 ulps of the host's threshold).

    timeout -k 10 900 python tools/lhalf_proxstep_batch_timing.py [--out profiles/lhalf_proxstep_batch_timing.txt] [--quick]
                                                                  [--alt lib/libspx_s6_lhalf_batch.so]

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
ap.add_argument("--quick", action="store_true", help="small shapes and few rounds (a rehearsal of the tool, not a measurement)")
ap.add_argument("--alt", default=None, help="another build of libspx_lhalf_batch.so, timed as leg (a')")
ap.add_argument("--only", default=None, help="n:batch[,n:batch...]: only these shapes")
args = ap.parse_args()

s = ge.build()
L = s._lib.load()
B = s._lib.load_batch()
H = s._lib.load_lhalf_batch()
ALT = None
if args.alt:
    ALT = ctypes.CDLL(os.path.abspath(args.alt))
    for name, sig in s._lib.LHALF_BATCH_SIGNATURES.items():
        getattr(ALT, name).argtypes, getattr(ALT, name).restype = sig, ctypes.c_int
dev = torch.device("cuda:0")
ctx = s.context(dev)
gen = torch.Generator(device=dev).manual_seed(12)
_D = ctypes.c_double


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def check_rc(rc):
    if rc != 0:
        raise RuntimeError("status %d: %s" % (rc, L.spx_last_error().decode()))


SIZES = [1_000, 10_000, 100_000]
BATCHES = [1, 16, 256, 4096]
if args.quick:
    SIZES, BATCHES = [1_000, 20_000], [1, 16]
SHAPES = [(n, b) for n in SIZES for b in BATCHES]
if args.only:
    SHAPES = [tuple(int(v) for v in p.split(":")) for p in args.only.split(",")]

lines = ["# (a) spx_proxstep_lhalf[_box]_batch with xkn   (b) batch sequential spx_proxstep_lhalf[_box] calls with xkn, same build",
         "# (d) spx_proxstep_l1_box_batch, same shape   (e) ONE spx_proxstep_lhalf[_box] over the batch * n elements (batch * n >= 1e7)",
         "# [us per call / per loop of (b), median of the rounds; spread = (max - min) / median of the rounds of that leg]",
         "# (c) = 40 B x n x batch / (a), in bytes per us (1e6 B/us = 1 TB/s)" + ("   (a') = (a) through %s" % os.path.basename(args.alt) if ALT else ""),
         "# device: %s" % torch.cuda.get_device_name(0),
         "%-9s %8s %6s %-6s %11s %7s %11s %7s %8s %11s %11s %7s %11s %11s %7s" % (
             "op", "n", "batch", "form", "(a) us", "spread", "(b) us", "spread", "(b)/(a)", "(c) B/us", "(d) us", "spread", "(e) us", "(a') us", "spread")]
print("\n".join(lines), flush=True)
for n, batch in SHAPES:
    ld = n
    mk = lambda: torch.randn((batch, n), dtype=torch.float64, device=dev, generator=gen)
    XK, Q = mk(), mk()
    SJ = torch.rand((batch, n), dtype=torch.float64, device=dev, generator=gen) - 0.5
    Y, XN, Y1, XN1 = (torch.empty_like(Q) for _ in range(4))
    u01 = lambda: 0.3 + 1.2 * torch.rand(batch, dtype=torch.float64, device=dev, generator=gen)
    lam, sig, dl = u01(), u01(), u01()
    qs = -sig
    lo, up = -dl, dl.clone()
    stats, stats1 = torch.zeros((batch, 3), dtype=torch.float64, device=dev), torch.zeros((batch, 3), dtype=torch.float64, device=dev)
    lam_h, sig_h, qs_h, dl_h = lam.tolist(), sig.tolist(), qs.tolist(), dl.tolist()
    for box in (False, True):
        # leg (b): the argument tuples are built once, the loop only calls
        if box:
            rows = [(ctx, ptr(Y1[b]), ptr(Q[b]), ptr(XK[b]), ptr(SJ[b]), n, _D(lam_h[b]), _D(sig_h[b]), None, None, _D(-dl_h[b]), _D(dl_h[b]),
                     None, _D(qs_h[b]), ptr(XN1[b]), None, ptr(stats1[b])) for b in range(batch)]
            single = L.spx_proxstep_lhalf_box
            a_args = (ctx, ptr(Y), ptr(Q), ptr(XK), ptr(SJ), n, batch, ld, ptr(lam), ptr(sig), ptr(lo), ptr(up), None, ptr(qs), ptr(XN), ptr(stats))
            one = (ctx, ptr(Y1), ptr(Q), ptr(XK), ptr(SJ), n * batch, _D(lam_h[0]), _D(sig_h[0]), None, None, _D(-dl_h[0]), _D(dl_h[0]),
                   None, _D(qs_h[0]), ptr(XN1), None, ptr(stats1[0]))
            batched, alt = H.spx_proxstep_lhalf_box_batch, ALT.spx_proxstep_lhalf_box_batch if ALT else None
        else:
            rows = [(ctx, ptr(Y1[b]), ptr(Q[b]), ptr(XK[b]), ptr(SJ[b]), n, _D(lam_h[b]), _D(sig_h[b]), _D(qs_h[b]), ptr(XN1[b]), None,
                     ptr(stats1[b])) for b in range(batch)]
            single = L.spx_proxstep_lhalf
            a_args = (ctx, ptr(Y), ptr(Q), ptr(XK), ptr(SJ), n, batch, ld, ptr(lam), ptr(sig), ptr(qs), ptr(XN), ptr(stats))
            one = (ctx, ptr(Y1), ptr(Q), ptr(XK), ptr(SJ), n * batch, _D(lam_h[0]), _D(sig_h[0]), _D(qs_h[0]), ptr(XN1), None, ptr(stats1[0]))
            batched, alt = H.spx_proxstep_lhalf_batch, ALT.spx_proxstep_lhalf_batch if ALT else None
        d_args = (ctx, ptr(Y), ptr(Q), ptr(XK), ptr(SJ), n, batch, ld, ptr(lam), ptr(sig), ptr(lo), ptr(up), None, ptr(qs), ptr(XN), ptr(stats))

        def leg_a():
            check_rc(batched(*a_args))

        def leg_alt():
            check_rc(alt(*a_args))

        def leg_b():
            for r in rows:
                rc = single(*r)
                if rc:
                    check_rc(rc)

        def leg_d():
            check_rc(B.spx_proxstep_l1_box_batch(*d_args))

        def leg_e():
            check_rc(single(*one))

        for _ in range(2):                     # warm the legs (code objects, workspace)
            leg_b(); leg_a()
        torch.cuda.synchronize()
        if box:
            assert torch.equal(Y, Y1) and torch.equal(XN, XN1), (n, batch)
        else:                                  # (elements within 4 ulps of the threshold may take the other branch)
            p = (54.0 ** (1 / 3) * (2 * (sig * lam)) ** (2 / 3) / 4)[:, None]
            a = (qs[:, None] * Q + (XK + SJ)).abs()
            near = (a - p).abs() <= 4 * 2.0 ** -52 * p
            assert bool(((Y == Y1) | near).all()) and bool(((XN == XN1) | near).all()), (n, batch)
            del p, a, near
        assert torch.allclose(stats, stats1, rtol=1e-10, atol=1e-11 * float(stats[:, 2].max())), (n, batch)   # (other orders of addition)
        if ALT:
            Ya = Y.clone()
            leg_alt()
            torch.cuda.synchronize()
            assert torch.equal(Y, Ya), (n, batch)      # kStages does not change a bit
            del Ya
        big = batch * n >= 10_000_000
        inner_a = max(5, min(200, 2_000_000_000 // (40 * n * batch)))
        inner_b = max(1, 2048 // batch)
        rounds = 3 if args.quick else 9
        legs = [(leg_a, inner_a, []), (leg_b, inner_b, []), (leg_d, inner_a, [])]
        if big:
            legs.append((leg_e, inner_a, []))
        if ALT:
            legs.append((leg_alt, inner_a, []))
        for leg, inner, ts in legs[2:]:
            leg()
        for _ in range(rounds):                # the legs alternate: drift of the machine hits all alike
            for leg, inner, ts in legs:
                ms = ctypes.c_float()
                check_rc(L.spx_timer_start(ctx))
                for _ in range(inner):
                    leg()
                check_rc(L.spx_timer_stop(ctx, ctypes.byref(ms)))
                ts.append(1e3 * ms.value / inner)
        med = lambda ts: sorted(ts)[len(ts) // 2]
        spr = lambda ts: "%6.1f%%" % (100.0 * (max(ts) - min(ts)) / med(ts))
        ta, tb, td = legs[0][2], legs[1][2], legs[2][2]
        te = legs[3][2] if big else None
        tx = legs[-1][2] if ALT else None
        line = "%-9s %8d %6d %-6s %11.2f %7s %11.2f %7s %8.2f %11.0f %11.2f %7s %11s %11s %7s" % (
            "lhalf-box" if box else "lhalf", n, batch, "row" if n <= 12288 else "tiled", med(ta), spr(ta), med(tb), spr(tb), med(tb) / med(ta),
            40.0 * n * batch / med(ta), med(td), spr(td), "%.2f" % med(te) if big else "-", "%.2f" % med(tx) if ALT else "-",
            spr(tx) if ALT else "-")
        lines.append(line)
        print(line, flush=True)
    del XK, Q, SJ, Y, XN, Y1, XN1
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
