"""Batched ShiftedNormL1B2 prox! + step statistics: what one spx_proxstep_l1_b2_batch call (with xkn) costs against what a caller
does today.

    (a) spx_proxstep_l1_b2_batch                      batch problems, one call, one launch (one workgroup per problem)
    (b) batch sequential spx_proxstep_l1_b2 calls     the same rows, one call each (one launch of a resident grid each), on the same
                                                      build (its kernels are the ones every earlier commit measured), results in
                                                      device doubles
    (c) the bytes (a) moves at least -- 40 B/element: q, xk, sj in; y, xkn out -- per microsecond of (a).  The row walk
        (n > 8192) re-reads q, xk, sj once per reduction on top of that, from L2 / the Infinity Cache.

Every shape is timed twice: with the trust region ACTIVE in every row (Delta_b = 0.3 chi(ProjB(-xk_b)): the root iteration runs,
five reductions or so) and INACTIVE in every row (Delta_b = 2 chi + 1: one reduction, then the store).  lambda = 0.3, sigma = 0.9,
q_scale = 1; Gaussian xk and q, sj uniform in [-0.5, 0.5].

Warm, HIP-event stopwatch on the context's (launching) stream, nothing read back in any leg.  The legs of a shape alternate
round by round; the figure is the median of nine rounds, spread = (max - min) / median of the rounds of that leg.  Leg (b) is
driven through ctypes like every caller of the C ABI from Python: where its launches are shorter than the host's call overhead,
(b) measures that overhead -- which is what such a caller pays.  Before a shape is timed the rows of (a) are compared with the
rows of (b): to 1e-12 max(||y||, ||xk||) per row where the trust region is active, bit for bit where it is not.

    timeout -k 10 1100 python tools/b2_proxstep_batch_timing.py [--out profiles/b2_proxstep_batch_timing.txt] [--quick] [--only-a]

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
ap.add_argument("--only-a", action="store_true", help="time leg (a) alone (A/B runs of two builds); the comparison with leg (b) before it stays")
args = ap.parse_args()

s = ge.build()
L = s._lib.load()
G = s._lib.load_b2_batch()
dev = torch.device("cuda:0")
ctx = s.context(dev)
gen = torch.Generator(device=dev).manual_seed(14)
_D = ctypes.c_double
LAM, SIG = 0.3, 0.9


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def check_rc(rc):
    if rc != 0:
        raise RuntimeError("status %d: %s" % (rc, L.spx_last_error().decode()))


SHAPES = [(n, b) for n in (1_000, 8_192, 10_000) for b in (1, 16, 256, 4096)] + [(100_000, b) for b in (1, 16, 256)]
if args.quick:
    SHAPES = [(1_000, 1), (1_000, 16), (10_000, 16)]

lines = ["# (a) spx_proxstep_l1_b2_batch with xkn   (b) batch sequential spx_proxstep_l1_b2 calls with xkn, same build",
         "# tr: the trust region of every row is active (Delta = 0.3 chi(ProjB(-xk))) or inactive (Delta = 2 chi + 1)",
         "# [us per call of (a) / per loop of (b), median of nine rounds; spread = (max - min) / median of the leg's rounds]",
         "# (c) = 40 B x n x batch / (a), in bytes per us (1e6 B/us = 1 TB/s)",
         "# device: %s" % torch.cuda.get_device_name(0),
         "# rows whose (a) is a few microseconds are launch-bound: their spread is large and their (b)/(a) is a ratio of launch costs",
         "%8s %6s %-8s %-9s %11s %8s %11s %8s %8s %11s" % ("n", "batch", "tr", "form", "(a) us", "sprd(a)", "(b) us", "sprd(b)", "(b)/(a)",
                                                        "(c) B/us")]
print("\n".join(lines), flush=True)
for n, batch in SHAPES:
    for tr in ("active", "inactive"):
        ld = n
        XK = torch.randn((batch, n), dtype=torch.float64, device=dev, generator=gen)
        Q = torch.randn((batch, n), dtype=torch.float64, device=dev, generator=gen)
        SJ = torch.rand((batch, n), dtype=torch.float64, device=dev, generator=gen) - 0.5
        sq = SJ + Q
        chi = torch.linalg.norm(torch.minimum(torch.maximum(-XK, sq - LAM * SIG), sq + LAM * SIG), dim=1)
        del sq
        dlt = (0.3 * chi if tr == "active" else 2.0 * chi + 1.0).contiguous()
        dlt_h = dlt.cpu().tolist()
        Y, XN, Y1, XN1 = (torch.empty_like(Q) for _ in range(4))
        lam = torch.full((batch,), LAM, dtype=torch.float64, device=dev)
        sig = torch.full((batch,), SIG, dtype=torch.float64, device=dev)
        qs = torch.ones(batch, dtype=torch.float64, device=dev)
        stats, stats1 = torch.zeros((batch, 3), dtype=torch.float64, device=dev), torch.zeros((batch, 3), dtype=torch.float64, device=dev)
        # leg (b): the argument tuples are built once, the loop only calls
        rows = [(ctx, ptr(Y1[b]), ptr(Q[b]), ptr(XK[b]), ptr(SJ[b]), n, _D(LAM), _D(SIG), _D(dlt_h[b]), _D(1.0), _D(1.0), ptr(XN1[b]), None,
                 ptr(stats1[b])) for b in range(batch)]
        single = L.spx_proxstep_l1_b2
        a_args = (ctx, ptr(Y), ptr(Q), ptr(XK), ptr(SJ), n, batch, ld, ptr(lam), ptr(sig), ptr(dlt), ptr(qs), _D(1.0), ptr(XN), ptr(stats))

        def leg_a():
            check_rc(G.spx_proxstep_l1_b2_batch(*a_args))

        def leg_b():
            for r in rows:
                rc = single(*r)
                if rc:
                    check_rc(rc)

        for _ in range(2):                     # warm the legs (code objects, the single call's residency queries)
            leg_a(); leg_b()
        torch.cuda.synchronize()
        if tr == "inactive":
            assert torch.equal(Y, Y1) and torch.equal(XN, XN1), (n, batch, tr)
        else:
            scale = torch.maximum(torch.linalg.norm(Y1, dim=1), torch.linalg.norm(XK, dim=1))
            assert bool(((Y - Y1).abs().amax(dim=1) <= 2e-12 * scale).all()), (n, batch, tr)   # (each within 1e-12 of the exact prox)
        assert torch.allclose(stats, stats1, rtol=1e-10, atol=1e-10 * float(stats[:, 2].max())), (n, batch, tr)
        inner_a = max(5, min(200, 2_000_000_000 // (40 * n * batch)))
        inner_b = max(1, 2048 // batch)
        rounds = 3 if args.quick else 9
        legs = [(leg_a, inner_a, []), (leg_b, 0 if args.only_a else inner_b, [0.0] if args.only_a else [])]
        for _ in range(rounds):                # the legs alternate: drift of the machine hits all alike
            for leg, inner, ts in legs:
                if inner == 0:                 # --only-a: leg (b) is not timed, its columns read 0
                    continue
                ms = ctypes.c_float()
                check_rc(L.spx_timer_start(ctx))
                for _ in range(inner):
                    leg()
                check_rc(L.spx_timer_stop(ctx, ctypes.byref(ms)))
                ts.append(1e3 * ms.value / inner)
        med = lambda ts: sorted(ts)[len(ts) // 2]
        sprd = lambda ts: 100.0 * (max(ts) - min(ts)) / med(ts) if med(ts) else 0.0
        ta, tb = legs[0][2], legs[1][2]
        a, b = med(ta), med(tb)
        line = "%8d %6d %-8s %-9s %11.2f %7.1f%% %11.2f %7.1f%% %8.2f %11.0f" % (n, batch, tr, "resident" if n <= 8192 else "walk", a, sprd(ta),
                                                                             b, sprd(tb), b / a, 40.0 * n * batch / a)
        lines.append(line)
        print(line, flush=True)
        del XK, Q, SJ, Y, XN, Y1, XN1
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
