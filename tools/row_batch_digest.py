"""The bits of the row-owner batched calls (spx_proxstep_l1_b2_batch, spx_proxstep_indball_l0[_binf]_batch), for comparing two
builds: one SHA-256 per case over the WHOLE y, xkn and stats buffers, padding included.

The tests hold top-r's y to the single call's bits, B2's y to 1e-12 and neither call's sums to anything but a tolerance, so a
build that adds in another order would pass them.  Two builds from sources that claim the same device code are run through this
tool (the build is the one SPX_LIB_NAME names) and the outputs compared line by line:

    SPX_LIB_NAME=libspx_parent.so timeout -k 10 300 python tools/row_batch_digest.py > parent.txt
    timeout -k 10 300 python tools/row_batch_digest.py > new.txt

Inputs are made on the CPU as a pure function of (case, index) (oracle/synth.py), the output buffers are pre-filled with a
fixed pattern, every call is one launch of batch = 3.  Cases: every n in NS -- each tile's edge, the resident / walk bound, a walk
of more than two rounds in the pairs form and more than four in the element-wise form -- in four layouts (everything on a
16-byte boundary with ld even; the same with xkn 8 bytes off; ld odd; xkn NULL), for B2 (lambda, sigma, q_scale distinct per
row; the trust region active at 0.3 of the projected norm in row 0, barely active at 0.9 ||xk|| in row 1, inactive in row 2) and
for top-r plain and BInf (r = 1, n / 2, n over the rows, delta distinct per row); top-r on a 1/4 lattice at n = 4097 and 8193
(the index digits decide); every call at n = 1025 with a NaN in one row's q and an Inf in another row's xk.

One process, every status checked, no retry: a failing call ends the run with its message."""
import ctypes
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import __graft_entry__ as ge
from oracle import synth

NS = (1, 2, 3, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 16387)
LAYOUTS = ("aligned", "xkn+8", "ld-odd", "no-xkn")
BATCH = 3
FILL = 0x7FF85A5A5A5A5A5A   # what an output word holds before the call: a NaN no kernel produces

s = ge.build(with_oracle=False)
L = s._lib.load()
B2 = s._lib.load_b2_batch()
TOPR = s._lib.load_topr_batch()
dev = torch.device("cuda:0")
ctx = s.context(dev)
_D = ctypes.c_double


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def inputs(case, n, ld, lattice):
    """q, xk, sj as (BATCH, ld) host arrays: element i of vector k is a function of (case, k, i) alone"""
    m = BATCH * ld
    if lattice:   # multiples of 1/4: |v| takes some forty values
        u = [synth.fill(m, case, k, 0) + 0.5 for k in range(3)]
        q, xk, sj = (np.floor(u[0] * 25) - 12) / 4.0, (np.floor(u[1] * 17) - 8) / 4.0, (np.floor(u[2] * 5) - 2) / 4.0
    else:
        q, xk, sj = synth.fill(m, case, 0, 1), synth.fill(m, case, 1, 1), synth.fill(m, case, 2, 0)
    return q.reshape(BATCH, ld), xk.reshape(BATCH, ld), sj.reshape(BATCH, ld)


def run(case, call, n, layout, lattice=False, nonfinite=False):
    ld = (n + 2) | 1 if layout == "ld-odd" else n + (n & 1) + 2
    q, xk, sj = inputs(case, n, ld, lattice)
    if nonfinite:
        q[1, 17] = np.nan
        xk[2, 1000] = np.inf
    qs = np.array([1.0, 0.7, -1.3])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Q, XK, SJ = up(q), up(xk), up(sj)
    fill = lambda words: torch.full((words,), FILL, dtype=torch.int64, device=dev).view(torch.float64)
    Y, XN, ST = fill(BATCH * ld), fill(BATCH * ld + 2), fill(BATCH * 3)
    xkn = None if layout == "no-xkn" else XN[1:] if layout == "xkn+8" else XN
    if call == "b2":
        lam, sig = np.array([0.1, 1.0, 0.5]), np.array([1.0, 0.5, 0.9])
        ls = (lam * sig)[:, None]
        sq = sj[:, :n] + qs[:, None] * q[:, :n]
        with np.errstate(invalid="ignore"):
            chi0 = np.linalg.norm(np.minimum(np.maximum(-xk[:, :n], sq - ls), sq + ls), axis=1)   # the projected norm
        nx = np.linalg.norm(xk[:, :n], axis=1)
        delta = np.array([0.3 * chi0[0] if chi0[0] > 0 else 1.0, 0.9 * nx[1] if nx[1] > 0 else 1.0, 2.0 * chi0[2] + 1.0])
        P = [up(a) for a in (lam, sig, delta, qs)]
        torch.cuda.synchronize()
        rc = B2.spx_proxstep_l1_b2_batch(ctx, ptr(Y), ptr(Q), ptr(XK), ptr(SJ), n, BATCH, ld, ptr(P[0]), ptr(P[1]), ptr(P[2]), ptr(P[3]),
                                         _D(1.0), ptr(xkn), ptr(ST))
    else:
        R = up(np.array([1, n // 2, n], dtype=np.int64))
        DL, QS = up(np.array([0.5, 0.25, 1.0])), up(qs)
        torch.cuda.synchronize()
        if call == "topr":
            rc = TOPR.spx_proxstep_indball_l0_batch(ctx, ptr(Y), ptr(Q), ptr(XK), ptr(SJ), n, BATCH, ld, ptr(R), ptr(QS), ptr(xkn), ptr(ST))
        else:
            rc = TOPR.spx_proxstep_indball_l0_binf_batch(ctx, ptr(Y), ptr(Q), ptr(XK), ptr(SJ), n, BATCH, ld, ptr(R), ptr(DL), ptr(QS),
                                                         ptr(xkn), ptr(ST))
    if rc != 0:
        raise RuntimeError("status %d: %s" % (rc, L.spx_last_error().decode()))
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in (Y, XN, ST):
        h.update(t.view(torch.int64).cpu().numpy().tobytes())
    what = "lattice" if lattice else "nonfinite" if nonfinite else "gauss"
    print("%-9s n=%-6d %-8s %-9s %s" % (call, n, layout, what, h.hexdigest()), flush=True)


case = 0
for call in ("b2", "topr", "topr_binf"):
    for n in NS:
        for layout in LAYOUTS:
            case += 1
            run(case, call, n, layout)
for call in ("topr", "topr_binf"):
    for n in (4097, 8193):
        case += 1
        run(case, call, n, "aligned", lattice=True)
for call in ("b2", "topr", "topr_binf"):
    case += 1
    run(case, call, 1025, "aligned", nonfinite=True)
print("cases %d" % case)
