"""Trust-region proximal gradient for a group lasso at the BASELINE group shape (1e6 groups x 128):

    min_x  1/2 ||x - b||^2 + sum_g lambda_g ||x_g||_2 ,      step:  s = prox!(psi, -nu grad, nu),  psi = shifted(h, xk, Delta, chi)

i.e. ShiftedGroupNormL2Binf (src/shiftedGroupNormL2Binf.jl) called the way a TR solver of RegularizedOptimization.jl [ext]
calls it.  b is zero on 90 % of the groups, so after the first steps most groups of xk are exactly zero and sit under a
sigma*lambda above ||S|| -- the reversed-bracket regime of the reference's root find.  The point of the
example: the per-iteration prox! time stays at the bandwidth figure while the iterate becomes sparse.

    python examples/tr_group_lasso.py [groups] [fused]

With a second argument `fused` (off by default) the iteration is one library call: group_prox_step_bang stores the step AND the
next iterate xkn = xk + step, and returns h(xk + step), <q, s> and ||s||^2 from the same pass (spx_proxstep_group_l2_binf) --
no `xk.add_(step)`, no pass for the step norm; xk and xkn trade places.
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as ge

s = ge.build(); L = s._lib.load()
dev = torch.device("cuda:0"); ctx = s.context(dev)
g = torch.Generator(device=dev).manual_seed(11)
ng, gs = (int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000), 128
fused = len(sys.argv) > 2 and sys.argv[2] == "fused"
n = ng * gs
active = (torch.rand(ng, dtype=torch.float64, device=dev, generator=g) < 0.1).to(torch.float64).repeat_interleave(gs)
b = (3.0 * torch.randn(n, dtype=torch.float64, device=dev, generator=g) + 0.3) * active
b += 0.05 * torch.randn(n, dtype=torch.float64, device=dev, generator=g)            # noise everywhere
lam = torch.full((ng,), 4.0, dtype=torch.float64, device=dev)                     # kills the noise-only groups
h = s.GroupNormL2.uniform(lam, gs)
xk = 0.1 * torch.randn(n, dtype=torch.float64, device=dev, generator=g)            # dense start
sj = torch.zeros_like(xk)
delta, nu = 1.0, 0.5
psi = s.shifted(s.shifted(h, xk, delta, s.NormLinf(1.0)), sj)
step = torch.empty_like(xk); q = torch.empty_like(xk)
torch.mul(xk - b, -nu, out=q)
s.prox_bang(step, psi, q, nu)                        # untimed first calls: the context allocates its scratch here
s.prox_value_bang(step, psi, q, nu)
if fused:
    xkn = torch.empty_like(xk)
    psi_n = s.shifted(s.shifted(h, xkn, delta, s.NormLinf(1.0)), sj)               # the same operator centred on the other buffer
    s.group_prox_step_bang(step, psi, q, nu, xkn=xkn)                               # (untimed first call)
    print("it   objective      zero groups   step ms    <q, s>         ||s||")
for it in range(25 if fused else 0):
    torch.mul(xk - b, -nu, out=q)                                                   # q = -nu grad f(xk)
    ms = ctypes.c_float(); L.spx_timer_start(ctx)
    _, hval, qs, ss = s.group_prox_step_bang(step, psi, q, nu, xkn=xkn)             # step, xkn = xk + step, h(xkn), <q, s>, ||s||^2
    L.spx_timer_stop(ctx, ctypes.byref(ms))
    xk, xkn, psi, psi_n = xkn, xk, psi_n, psi                                       # the new iterate and the operator centred on it
    zero_groups = int((xk.view(ng, gs).abs().amax(dim=1) == 0).sum())
    obj = 0.5 * float(torch.dot(xk - b, xk - b)) + hval
    print("%2d   %.6e   %8d      %.3f      %+.6e  %.3e" % (it, obj, zero_groups, ms.value, qs, ss ** 0.5), flush=True)
    if ss ** 0.5 < 1e-9:
        break
    delta = min(4.0 * delta, 64.0)                                                  # every step is a descent step here
    s.set_radius_bang(psi, delta)
    s.set_radius_bang(psi_n, delta)
if not fused:
    print("it   objective      zero groups   prox! ms   prox!+h ms")
for it in range(0 if fused else 25):
    torch.mul(xk - b, -nu, out=q)                                                   # q = -nu grad f(xk)
    ms = ctypes.c_float(); L.spx_timer_start(ctx)
    s.prox_bang(step, psi, q, nu)
    L.spx_timer_stop(ctx, ctypes.byref(ms))
    # the same step once more, fused with the regulariser at the new iterate: h(xk + sj + step), sj = 0 -- the launch that
    # stores the step also returns sum_g lambda_g ||(xk + step)_g|| (spx_proxval_group_l2_binf; no pass over xk on the side)
    msv = ctypes.c_float(); L.spx_timer_start(ctx)
    _, hval = s.prox_value_bang(step, psi, q, nu)
    L.spx_timer_stop(ctx, ctypes.byref(msv))
    xk.add_(step)                                                                   # psi borrows xk: re-centred in place
    zero_groups = int((xk.view(ng, gs).abs().amax(dim=1) == 0).sum())
    obj = 0.5 * float(torch.dot(xk - b, xk - b)) + hval
    print("%2d   %.6e   %8d      %.3f      %.3f" % (it, obj, zero_groups, ms.value, msv.value), flush=True)
    if float(step.abs().max()) < 1e-9:
        break
    delta = min(4.0 * delta, 64.0)                                                  # every step is a descent step here
    s.set_radius_bang(psi, delta)
