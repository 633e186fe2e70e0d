"""Batched ShiftedIndBallL0 / ShiftedIndBallL0BInf prox! + step statistics: what one spx_proxstep_indball_l0[_binf]_batch call
(with xkn) costs against what a caller does today.

    (a) spx_proxstep_indball_l0[_binf]_batch            batch problems, one call, one launch (one workgroup per problem)
    (b) batch sequential spx_prox_indball_l0[_binf]     the same rows, one call each, on the same build (libspx.so is untouched:
                                                        its kernels are the ones every earlier commit measured).  The loop forms
                                                        neither xkn nor the sums: it does LESS than (a)
    (c) the bytes (a) moves at least -- 40 B/element: q, xk, sj in; y, xkn out -- per microsecond of (a).  The row walk
        (n > 8192) writes and re-reads v in y once per digit on top of that, from L2 / the Infinity Cache.

Every shape is timed at r = n/100 and r = n/2 in every row, plain and BInf (Delta = 0.5), q_scale = 1; Gaussian xk and q, sj
uniform in [-0.5, 0.5].  One tie-heavy shape: a 1/4 lattice (|v| takes ~40 values: every digit pass ends in the index digits).

Warm, HIP-event stopwatch on the context's (launching) stream, nothing read back in any leg.  The legs of a shape alternate
round by round; the figure is the median of nine rounds, spread = (max - min) / median of the rounds of that leg.  Leg (b) is
driven through ctypes like every caller of the C ABI from Python: where its launches are shorter than the host's call overhead,
(b) measures that overhead -- which is what such a caller pays.  Before a shape is timed the rows of (a) are compared with the
rows of (b) bit for bit.

    timeout -k 10 1100 python tools/topr_proxstep_batch_timing.py [--out profiles/topr_proxstep_batch_timing.txt] [--quick] [--only-a]

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
G = s._lib.load_topr_batch()
dev = torch.device("cuda:0")
ctx = s.context(dev)
gen = torch.Generator(device=dev).manual_seed(15)
_D = ctypes.c_double
DELTA = 0.5


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def check_rc(rc):
    if rc != 0:
        raise RuntimeError("status %d: %s" % (rc, L.spx_last_error().decode()))


SHAPES = [(n, b, "gauss") for n in (1_000, 8_192, 10_000) for b in (1, 16, 256, 4096)] + [(100_000, b, "gauss") for b in (1, 16, 256)]
SHAPES.append((8_192, 256, "lattice"))
if args.quick:
    SHAPES = [(1_000, 1, "gauss"), (1_000, 16, "gauss"), (10_000, 16, "gauss"), (1_000, 16, "lattice")]

lines = ["# (a) spx_proxstep_indball_l0[_binf]_batch with xkn   (b) batch sequential spx_prox_indball_l0[_binf] calls, same build",
         "# [us per call of (a) / per loop of (b), median of nine rounds; spread = (max - min) / median of the leg's rounds]",
         "# (c) = 40 B x n x batch / (a), in bytes per us (1e6 B/us = 1 TB/s)",
         "# device: %s" % torch.cuda.get_device_name(0),
         "# rows whose (a) is a few microseconds are launch-bound: their spread is large and their (b)/(a) is a ratio of launch costs",
         "%8s %6s %-7s %-5s %7s %-9s %11s %8s %11s %8s %8s %11s" % ("n", "batch", "data", "op", "r", "form", "(a) us", "sprd(a)", "(b) us",
                                                                  "sprd(b)", "(b)/(a)", "(c) B/us")]
print("\n".join(lines), flush=True)
for n, batch, data in SHAPES:
    ld = n
    if data == "lattice":
        XK = torch.randint(-8, 9, (batch, n), device=dev, generator=gen).to(torch.float64) / 4.0
        Q = torch.randint(-12, 13, (batch, n), device=dev, generator=gen).to(torch.float64) / 4.0
        SJ = torch.randint(-2, 3, (batch, n), device=dev, generator=gen).to(torch.float64) / 4.0
    else:
        XK = torch.randn((batch, n), dtype=torch.float64, device=dev, generator=gen)
        Q = torch.randn((batch, n), dtype=torch.float64, device=dev, generator=gen)
        SJ = torch.rand((batch, n), dtype=torch.float64, device=dev, generator=gen) - 0.5
    Y, XN, Y1 = (torch.empty_like(Q) for _ in range(3))
    qs = torch.ones(batch, dtype=torch.float64, device=dev)
    dlt = torch.full((batch,), DELTA, dtype=torch.float64, device=dev)
    stats = torch.zeros((batch, 3), dtype=torch.float64, device=dev)
    for op in ("plain", "binf"):
        for r in (max(n // 100, 1), n // 2):
            rd = torch.full((batch,), r, dtype=torch.int64, device=dev)
            # leg (b): the argument tuples are built once, the loop only calls
            if op == "plain":
                single = L.spx_prox_indball_l0
                rows = [(ctx, ptr(Y1[b]), ptr(Q[b]), ptr(XK[b]), ptr(SJ[b]), n, r) for b in range(batch)]
                batched = G.spx_proxstep_indball_l0_batch
                a_args = (ctx, ptr(Y), ptr(Q), ptr(XK), ptr(SJ), n, batch, ld, ptr(rd), ptr(qs), ptr(XN), ptr(stats))
            else:
                single = L.spx_prox_indball_l0_binf
                rows = [(ctx, ptr(Y1[b]), ptr(Q[b]), ptr(XK[b]), ptr(SJ[b]), n, r, _D(DELTA)) for b in range(batch)]
                batched = G.spx_proxstep_indball_l0_binf_batch
                a_args = (ctx, ptr(Y), ptr(Q), ptr(XK), ptr(SJ), n, batch, ld, ptr(rd), ptr(dlt), ptr(qs), ptr(XN), ptr(stats))

            def leg_a():
                check_rc(batched(*a_args))

            def leg_b():
                for row in rows:
                    rc = single(*row)
                    if rc:
                        check_rc(rc)

            for _ in range(2):                     # warm the legs (code objects, the single call's residency queries)
                leg_a(); leg_b()
            torch.cuda.synchronize()
            assert torch.equal(Y.view(torch.int64), Y1.view(torch.int64)), (n, batch, op, r)
            assert torch.equal(XN.view(torch.int64), ((XK + SJ) + Y1).view(torch.int64)), (n, batch, op, r)
            assert torch.equal(stats[:, 0], (XN != 0).sum(dim=1).to(torch.float64)), (n, batch, op, r)
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
            line = "%8d %6d %-7s %-5s %7d %-9s %11.2f %7.1f%% %11.2f %7.1f%% %8.2f %11.0f" % (
                n, batch, data, op, r, "resident" if n <= 8192 else "walk", a, sprd(ta), b, sprd(tb), b / a, 40.0 * n * batch / a)
            lines.append(line)
            print(line, flush=True)
            if args.out:
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
    del XK, Q, SJ, Y, XN, Y1
