"""Batched Binf group prox! + step statistics: what one spx_proxstep_group_l2_binf_batch call (with xkn) costs against what a
caller does today.

    (a) spx_proxstep_group_l2_binf_batch                      batch problems, one call (n > 12288: two launches)
    (b) batch sequential spx_proxstep_group_l2_binf calls     the same rows, one call each (two launches each), on the same build
                                                              (its kernels are the ones every earlier commit measured), results
                                                              in device doubles
    (c) ONE spx_proxstep_group_l2_binf over the concatenation where batch * n >= 1e7: all rows as one problem of batch * ngroups
                                                              groups (sigma, Delta and q_scale are common to the rows in this
                                                              tool's data, the only case in which a caller may do this)
    (d) the bytes (a) moves -- 40 B/element: q, xk, sj in; y, xkn out -- per microsecond of (a)

Every shape is timed twice: on data with no group on the literal path ("lit 0": continuous data on the scale of the Binf tests,
entries O(1) / sqrt(group size), Delta = 0.3 of that, lambda from {0.7, 2, 10}) and with an entry of xk exactly on the
trust-region boundary in about 5 % of the groups ("lit 5": those groups take the reference's literal evaluation -- the second
phase of the batched kernel, the second launch of the single call).

Warm, HIP-event stopwatch on the context's (launching) stream, nothing read back in any leg.  The legs of a shape alternate
round by round; the figure is the median round, spread = (max - min) / median of the rounds of that leg.  Leg (b) is driven
through ctypes like every caller of the C ABI from Python: where its launches are shorter than the host's call overhead, (b)
measures that overhead -- which is what such a caller pays.  Before a shape is timed the rows of (a) are compared with the rows
of (b): y and xkn bit for bit.

    timeout -k 10 1100 python tools/group_binf_proxstep_batch_timing.py [--out profiles/group_binf_proxstep_batch_timing.txt] [--quick]

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
G = s._lib.load_gbinf_batch()
dev = torch.device("cuda:0")
ctx = s.context(dev)
gen = torch.Generator(device=dev).manual_seed(12)
_D = ctypes.c_double


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def check_rc(rc):
    if rc != 0:
        raise RuntimeError("status %d: %s" % (rc, L.spx_last_error().decode()))


GROUPS = [8, 128]
SIZES = [1_000, 10_000, 100_000]
BATCHES = [1, 16, 256, 4096]
if args.quick:
    SIZES, BATCHES = [1_000, 20_000], [1, 16]

lines = ["# (a) spx_proxstep_group_l2_binf_batch with xkn   (b) batch sequential spx_proxstep_group_l2_binf calls with xkn, same build",
         "# (c) ONE spx_proxstep_group_l2_binf with xkn over the concatenated rows (common sigma, Delta, q_scale), where batch * n >= 1e7",
         "# lit: per cent of the groups with an entry of xk exactly on the trust-region boundary (the literal evaluation)",
         "# [us per call of (a), (c) / per loop of (b), median of the rounds; spread = (max - min) / median of the leg's rounds]",
         "# (d) = 40 B x n x batch / (a), in bytes per us (1e6 B/us = 1 TB/s)",
         "# n is rounded down to a multiple of the group size",
         "# device: %s" % torch.cuda.get_device_name(0),
         "# rows whose (a) is a few microseconds are launch-bound: their spread is large and their (b)/(a) is a ratio of launch costs",
         "%6s %8s %6s %3s %-6s %11s %8s %11s %8s %8s %11s %8s %8s %11s" % ("group", "n", "batch", "lit", "form", "(a) us", "sprd(a)", "(b) us", "sprd(b)",
                                                                   "(b)/(a)", "(c) us", "sprd(c)", "(a)/(c)", "(d) B/us")]
print("\n".join(lines), flush=True)
for gs in GROUPS:
    for n0 in SIZES:
        ng = n0 // gs
        n = ng * gs
        for batch, lit in [(b, l) for b in BATCHES for l in (0, 5)]:
            ld = n
            scale = 0.6 / gs ** 0.5
            mk = lambda: torch.randn((batch, n), dtype=torch.float64, device=dev, generator=gen) * scale
            XK, Q = mk(), mk()
            SJ = (torch.rand((batch, n), dtype=torch.float64, device=dev, generator=gen) - 0.5) * scale
            sig_v, dlt_v = 0.9, 0.3 * scale      # common to the rows (leg (c)); the batched call still reads them per row
            if lit:                              # one entry ON the boundary in every 20th group of every row
                where = torch.arange(0, ng, 20, device=dev) * gs + torch.randint(0, gs, ((ng + 19) // 20,), device=dev, generator=gen)
                XK[:, where] = dlt_v
            Y, XN, Y1, XN1 = (torch.empty_like(Q) for _ in range(4))
            choice = torch.tensor([0.7, 2.0, 10.0], dtype=torch.float64, device=dev)
            lam = choice[torch.randint(0, 3, (batch, ng), device=dev, generator=gen)]
            sig = torch.full((batch,), sig_v, dtype=torch.float64, device=dev)
            dlt = torch.full((batch,), dlt_v, dtype=torch.float64, device=dev)
            qs = -sig
            stats, stats1 = torch.zeros((batch, 3), dtype=torch.float64, device=dev), torch.zeros((batch, 3), dtype=torch.float64, device=dev)
            # leg (b): the argument tuples are built once, the loop only calls
            rows = [(ctx, ptr(Y1[b]), ptr(Q[b]), ptr(XK[b]), ptr(SJ[b]), n, None, gs, ng, ptr(lam[b]), _D(sig_v), _D(dlt_v), _D(-sig_v),
                     ptr(XN1[b]), None, ptr(stats1[b])) for b in range(batch)]
            single = L.spx_proxstep_group_l2_binf
            a_args = (ctx, ptr(Y), ptr(Q), ptr(XK), ptr(SJ), gs, ng, batch, ld, ptr(lam), ng, None, ptr(sig), ptr(dlt), ptr(qs), ptr(XN),
                      ptr(stats))
            concat = batch * n >= 10_000_000
            c_stats = torch.zeros(3, dtype=torch.float64, device=dev)
            c_args = (ctx, ptr(Y1), ptr(Q), ptr(XK), ptr(SJ), batch * n, None, gs, batch * ng, ptr(lam), _D(sig_v), _D(dlt_v), _D(-sig_v),
                      ptr(XN1), None, ptr(c_stats))

            def leg_a():
                check_rc(G.spx_proxstep_group_l2_binf_batch(*a_args))

            def leg_b():
                for r in rows:
                    rc = single(*r)
                    if rc:
                        check_rc(rc)

            def leg_c():
                check_rc(single(*c_args))

            for _ in range(2):                     # warm the legs (code objects, workspace)
                leg_a(); leg_b()
            torch.cuda.synchronize()
            assert torch.equal(Y, Y1) and torch.equal(XN, XN1), (gs, n, batch, lit)
            assert torch.allclose(stats, stats1, rtol=1e-11, atol=1e-11 * float(stats[:, 2].max())), (gs, n, batch)   # (other orders of addition)
            if concat:
                leg_c(); leg_c()
                torch.cuda.synchronize()
            inner_a = max(5, min(200, 2_000_000_000 // (40 * n * batch)))
            inner_b = max(1, 2048 // batch)
            rounds = 3 if args.quick else 9
            legs = [(leg_a, inner_a, []), (leg_b, inner_b, [])] + ([(leg_c, inner_a, [])] if concat else [])
            for _ in range(rounds):                # the legs alternate: drift of the machine hits all alike
                for leg, inner, ts in legs:
                    ms = ctypes.c_float()
                    check_rc(L.spx_timer_start(ctx))
                    for _ in range(inner):
                        leg()
                    check_rc(L.spx_timer_stop(ctx, ctypes.byref(ms)))
                    ts.append(1e3 * ms.value / inner)
            med = lambda ts: sorted(ts)[len(ts) // 2]
            sprd = lambda ts: 100.0 * (max(ts) - min(ts)) / med(ts)
            ta, tb = legs[0][2], legs[1][2]
            a, b = med(ta), med(tb)
            if concat:
                tc = legs[2][2]
                ctxt = "%11.2f %7.1f%% %8.2f" % (med(tc), sprd(tc), a / med(tc))
            else:
                ctxt = "%11s %8s %8s" % ("-", "-", "-")
            line = "%6d %8d %6d %3d %-6s %11.2f %7.1f%% %11.2f %7.1f%% %8.2f %s %11.0f" % (gs, n, batch, lit, "row" if n <= 12288 else "tiled", a,
                                                                                     sprd(ta), b, sprd(tb), b / a, ctxt,
                                                                                     40.0 * n * batch / a)
            lines.append(line)
            print(line, flush=True)
            del XK, Q, SJ, Y, XN, Y1, XN1
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
