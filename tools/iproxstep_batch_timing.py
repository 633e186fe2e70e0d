"""Batched iprox! + step statistics: what one spx_iproxstep_l1_box_batch call (with xkn and d_shift) costs against what a caller
does today.

    (a) spx_iproxstep_l1_box_batch                        batch problems, one call (n > 12288: two launches), d + sigma_b formed
                                                          on the fly from d_shift
    (b) batch times: the d + sigma_b pass (torch.add into a work vector, as a caller forms D + sigma today) followed by one
        spx_iproxstep_l1_box call on that row             the same rows, on the same build (its kernels are the ones every
                                                          earlier commit measured), results in device doubles
    (c) the bytes (a) moves -- 48 B/element: g, d, xk, sj in; y, xkn out -- per microsecond of (a)

Warm, HIP-event stopwatch on the context's (launching) stream, nothing read back in either leg.  The two legs of a shape alternate
round by round; the figure is the median round, spread = (max - min) / median of the rounds of (a).  Leg (b) is driven through
ctypes and torch like every caller of the C ABI from Python: where its launches are shorter than the host's call overhead, (b)
measures that overhead -- which is what such a caller pays.  Before a shape is timed the rows of (a) are compared with the rows
of (b): y and xkn bit for bit.

The one condition: at n = 10000, batch = 256 leg (a) is at least 10 x faster than leg (b); the last line of
the table says whether it held.

    timeout -k 10 600 python tools/iproxstep_batch_timing.py [--out profiles/iproxstep_batch_timing.txt] [--quick]

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
args = ap.parse_args()

s = ge.build()
L = s._lib.load()
B = s._lib.load_ibatch()
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

lines = ["# (a) spx_iproxstep_l1_box_batch with xkn and d_shift   (b) batch x (d + sigma_b pass, spx_iproxstep_l1_box with xkn), same build",
         "# [us per call of (a) / per loop of (b), median of the rounds; spread = (max - min) / median of the rounds of (a)]",
         "# (c) = 48 B x n x batch / (a), in bytes per us (= MB/s x 1e-6 ... 1e6 B/us = 1 TB/s)",
         "# device: %s" % torch.cuda.get_device_name(0),
         "%8s %6s %-6s %12s %12s %9s %9s %12s" % ("n", "batch", "form", "(a) us", "(b) us", "(b)/(a)", "spread", "(c) B/us")]
print("\n".join(lines), flush=True)
verdict = None
for n in SIZES:
    for batch in BATCHES:
        ld = n
        mk = lambda: torch.randn((batch, n), dtype=torch.float64, device=dev, generator=gen)
        XK, G, D = mk(), mk(), mk()              # d of both signs: the Box form takes any d
        SJ = torch.rand((batch, n), dtype=torch.float64, device=dev, generator=gen) - 0.5
        Y, XN, Y1, XN1, DE = (torch.empty_like(G) for _ in range(5))
        u01 = lambda: 0.3 + 1.2 * torch.rand(batch, dtype=torch.float64, device=dev, generator=gen)
        lam, sig, dl = u01(), u01(), u01()
        lo, up = -dl, dl.clone()
        stats, stats1 = torch.zeros((batch, 4), dtype=torch.float64, device=dev), torch.zeros((batch, 4), dtype=torch.float64, device=dev)
        lam_h, sig_h, dl_h = lam.tolist(), sig.tolist(), dl.tolist()
        # leg (b): the argument tuples and the row views are built once, the loop only calls
        rows = [(ctx, ptr(Y1[b]), ptr(G[b]), ptr(DE[b]), ptr(XK[b]), ptr(SJ[b]), n, _D(lam_h[b]), None, None, _D(-dl_h[b]), _D(dl_h[b]),
                 None, ptr(XN1[b]), None, ptr(stats1[b])) for b in range(batch)]
        adds = [(D[b], sig_h[b], DE[b]) for b in range(batch)]
        single = L.spx_iproxstep_l1_box
        a_args = (ctx, ptr(Y), ptr(G), ptr(D), ptr(XK), ptr(SJ), n, batch, ld, ptr(lam), ptr(sig), ptr(lo), ptr(up), None, ptr(XN), ptr(stats))

        def leg_a():
            check_rc(B.spx_iproxstep_l1_box_batch(*a_args))

        def leg_b():
            for r, (d_row, sg, de_row) in zip(rows, adds):
                torch.add(d_row, sg, out=de_row)          # the D + sigma_b pass
                rc = single(*r)
                if rc:
                    check_rc(rc)

        for _ in range(2):                     # warm both legs (code objects, workspace)
            leg_a(); leg_b()
        torch.cuda.synchronize()
        assert torch.equal(Y, Y1) and torch.equal(XN, XN1), (n, batch)
        assert torch.allclose(stats, stats1, rtol=1e-11, atol=1e-11 * float(stats[:, 3].max())), (n, batch)   # (other orders of addition)
        inner_a = max(5, min(200, 2_000_000_000 // (48 * n * batch)))
        inner_b = max(1, 2048 // batch)
        rounds = 3 if args.quick else 9
        ta, tb = [], []
        for _ in range(rounds):                # the legs alternate: drift of the machine hits both alike
            for leg, inner, ts in ((leg_a, inner_a, ta), (leg_b, inner_b, tb)):
                ms = ctypes.c_float()
                check_rc(L.spx_timer_start(ctx))
                for _ in range(inner):
                    leg()
                check_rc(L.spx_timer_stop(ctx, ctypes.byref(ms)))
                ts.append(1e3 * ms.value / inner)
        a, b = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
        line = "%8d %6d %-6s %12.2f %12.2f %9.2f %8.1f%% %12.0f" % (n, batch, "row" if n <= 12288 else "tiled", a, b, b / a,
                                                                  100.0 * (max(ta) - min(ta)) / a, 48.0 * n * batch / a)
        lines.append(line)
        print(line, flush=True)
        if (n, batch) == (10_000, 256):
            verdict = "# condition at n = 10000, batch = 256: (b) / (a) = %.1f, required >= 10: %s" % (b / a, "met" if b >= 10 * a else "MISSED")
        del XK, G, D, DE, SJ, Y, XN, Y1, XN1
if verdict:
    lines.append(verdict)
    print(verdict, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
