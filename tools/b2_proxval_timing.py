"""prox! + h(xk + s) of ShiftedNormL1B2: (a) the plain prox!, (b) prox! then psi(y) (spx_obj_l1_b2) as two calls, (c) the fused
spx_proxval_l1_b2 -- warm, HIP-event stopwatch on each context's stream, value in a device double (no read-back in any leg).
All legs of a shape alternate round by round; the figure is the median round, the spread (max - min) / median of the rounds.

    timeout -k 10 900 python tools/b2_proxval_timing.py [--out profiles/b2_proxval_timing.txt] [--quick]
                      [--parent-lib libspx_parent.so] [--ab-lib libspx_b2dyn.so] [--append notes.txt]

--parent-lib: a libspx.so built from the parent commit (a name under the package's lib/ or a path).  Legs (a0) and (b) then
run on IT, in this process and in the same rounds: (b) is what a caller paid before the fused call existed, (a0) against (a)
shows that the plain prox! did not move.  Without it (b) runs on the current library and (a0) is left out.
--ab-lib: a build of the current sources with -DSPX_B2_VALUE_DYNAMIC_AB (the fused kernel takes its tiles on demand wherever
the plain prox! does: NOT reproducible, for this measurement only): leg (c') = the fused call on it, the upper bound of what
per-tile partial sums added in tile order could reach.
--append: a text file copied verbatim to the end of the table (the kernel resource lines of the build that was measured).

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
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--ab-lib", default=None)
ap.add_argument("--append", default=None)
args = ap.parse_args()

s = ge.build()
dev = torch.device("cuda:0")
_D = ctypes.c_double
NEEDED = ["spx_last_error", "spx_ctx_create_on_stream", "spx_ctx_destroy", "spx_sync", "spx_timer_start", "spx_timer_stop",
          "spx_ctx_set_value_target", "spx_prox_l1_b2", "spx_obj_l1_b2", "spx_proxval_l1_b2"]


class Lib:
    """one libspx build with a context of its own on torch's current stream and a device double for its values"""

    def __init__(self, name):
        path = name if os.path.sep in name else os.path.join(os.path.dirname(s._lib.LIB_PATH), name)
        self.L = ctypes.CDLL(path)
        for fn in NEEDED:
            if hasattr(self.L, fn):
                f = getattr(self.L, fn)
                f.argtypes = s._lib.SIGNATURES[fn]
                f.restype = ctypes.c_char_p if fn == "spx_last_error" else ctypes.c_int
        self.ctx = ctypes.c_void_p()
        self.check(self.L.spx_ctx_create_on_stream(0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(self.ctx)))
        self.target = torch.zeros(1, dtype=torch.float64, device=dev)
        self.check(self.L.spx_ctx_set_value_target(self.ctx, ctypes.c_void_p(self.target.data_ptr())))

    def check(self, rc):
        if rc != 0:
            msg = self.L.spx_last_error()
            raise RuntimeError("libspx status %d: %s" % (rc, msg.decode() if msg else ""))

    def close(self):
        torch.cuda.synchronize()
        self.L.spx_ctx_destroy(self.ctx)


new = Lib(os.path.basename(s._lib.LIB_PATH))
parent = Lib(args.parent_lib) if args.parent_lib else None
ab = Lib(args.ab_lib) if args.ab_lib else None
pair = parent or new
gen = torch.Generator(device=dev).manual_seed(7)
SIZES = [10_000, 100_000, 1_000_000, 4_000_000, 16_000_000, 100_000_000]
if args.quick:
    SIZES = [10_000, 100_000, 1_000_000]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def median(t):
    return sorted(t)[len(t) // 2]


names = ["(a)"] + (["(a0)"] if parent else []) + ["(b)", "(c)"] + (["(c')"] if ab else [])
lines = ["# ShiftedNormL1B2, lambda = sigma = chi = 1   [ms per call: median of the rounds; +-: (max - min) / median of the rounds, per cent]",
         "# (a) spx_prox_l1_b2, this library" + ("   (a0) the same on the parent commit's library" if parent else ""),
         "# (b) spx_prox_l1_b2 then spx_obj_l1_b2, two calls, on %s" % ("the parent commit's library" if parent else "this library"),
         "# (c) spx_proxval_l1_b2, this library: fused on every form, static partition in the passes that store y"
         + ("   (c') the same with on-demand tiles (A/B build, sums not reproducible)" if ab else ""),
         "# device: %s" % torch.cuda.get_device_name(0),
         "%11s %-8s " % ("n", "region") + " ".join("%9s %5s" % (nm, "+-%") for nm in names) + " %7s %7s" % ("(c)/(b)", "(c)/(a)")
         + (" %7s" % "(a)/(a0)" if parent else "") + (" %7s" % "(c')/(c)" if ab else "")]
print("\n".join(lines), flush=True)
try:
    for n in SIZES:
        xk = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
        sj = torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5
        q = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
        y = torch.empty_like(q)
        host = _D(0.0)
        for region, delta in (("active", 1.0), ("inactive", 1e9)):
            def prox(lib):
                lib.check(lib.L.spx_prox_l1_b2(lib.ctx, ptr(y), ptr(q), ptr(xk), ptr(sj), n, _D(1.0), _D(1.0), _D(delta), _D(1.0)))

            def obj(lib):
                lib.check(lib.L.spx_obj_l1_b2(lib.ctx, ptr(y), ptr(xk), ptr(sj), n, _D(1.0), _D(delta), ctypes.byref(host)))

            def fused(lib):
                lib.check(lib.L.spx_proxval_l1_b2(lib.ctx, ptr(y), ptr(q), ptr(xk), ptr(sj), n, _D(1.0), _D(1.0), _D(delta), _D(1.0),
                                                  _D(1.0), ctypes.byref(host)))

            legs = [(new, lambda: prox(new))]
            if parent:
                legs.append((parent, lambda: prox(parent)))
            legs.append((pair, lambda: (prox(pair), obj(pair))))
            legs.append((new, lambda: fused(new)))
            if ab:
                legs.append((ab, lambda: fused(ab)))
            inner = 5 if n >= 10_000_000 else 50
            rounds = 7
            vals = {}
            for nm, (lib, leg) in zip(names, legs):   # warm every leg (code objects, workspace sizes, the regime) and keep its value
                leg(); leg()
                lib.check(lib.L.spx_sync(lib.ctx))
                vals[nm] = float(lib.target.item())
            vb, vc = vals["(b)"], vals["(c)"]
            assert vb == vb and abs(vc - vb) <= 1e-12 * abs(vb), (vb, vc)   # (c) and (b) return the same h
            ts = [[] for _ in legs]
            for _ in range(rounds):                   # the legs alternate: drift of the box hits all of them alike
                for k, (lib, leg) in enumerate(legs):
                    leg()                             # (the regime of THIS library's previous call is this leg's own)
                    ms = ctypes.c_float()
                    lib.check(lib.L.spx_timer_start(lib.ctx))
                    for _ in range(inner):
                        leg()
                    lib.check(lib.L.spx_timer_stop(lib.ctx, ctypes.byref(ms)))
                    ts[k].append(ms.value / inner)
            med = dict(zip(names, (median(t) for t in ts)))
            line = "%11d %-8s " % (n, region) + " ".join("%9.4f %5.1f" % (median(t), 100.0 * (max(t) - min(t)) / median(t)) for t in ts)
            line += " %7.3f %7.3f" % (med["(c)"] / med["(b)"], med["(c)"] / med["(a)"])
            if parent:
                line += " %7.3f" % (med["(a)"] / med["(a0)"])
            if ab:
                line += " %7.3f" % (med["(c')"] / med["(c)"])
            lines.append(line)
            print(line, flush=True)
        del xk, sj, q, y
finally:
    for lib in (new, parent, ab):
        if lib is not None:
            lib.close()
if args.append:
    lines.append("")
    lines.extend(open(args.append).read().rstrip("\n").split("\n"))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
