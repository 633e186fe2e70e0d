"""GPU: a few R2 iterations on min 1/2 ||A x - d||^2 + lambda_b sum sqrt|x_i| over 8 values of lambda (n = 3073), one
prox_step_lhalf_batch_bang call per iteration for the whole path -- q = -nu_b * grad f through q_scale, sigma = nu_b, accept /
reject and the nu update as torch operations on device tensors fed by the call's statistics -- against the loop a caller writes
today: 8 spx_proxstep_lhalf[_box] calls per iteration with host copies of the scalars.  Every iteration both start from the
batched loop's iterate; the rows are equal bit for bit for the Box form, and for the unboxed form under the band rule of
include/spx_lhalf_batch.h: an element whose |q_scale q + xk| lies between the host's and the device's threshold (4 ulps) may
have the other branch of the jump, every other element has the single call's bits."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, M, BATCH, ITERS = 3073, 48, 8, 6


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("box", [False, True], ids=["lhalf", "lhalf-box"])
def test_r2_lhalf_path_batched_equals_the_loop_of_single_calls(box):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    s = ge.build()
    L, ctx = s._lib.load(), s.context("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(9100)
    A = (torch.randn(M, N, dtype=torch.float64, generator=g) / math.sqrt(M)).cuda()
    x0 = torch.zeros(N, dtype=torch.float64)
    x0[torch.randperm(N, generator=g)[:40]] = torch.randn(40, dtype=torch.float64, generator=g) * 3
    d = A @ x0.cuda()
    lam = torch.logspace(-2, 0, BATCH, dtype=torch.float64).cuda()
    nu = torch.full((BATCH,), 0.2, dtype=torch.float64, device="cuda:0")
    delta = torch.full((BATCH,), 2.0, dtype=torch.float64, device="cuda:0")
    X = torch.zeros(BATCH, N, dtype=torch.float64, device="cuda:0")
    SJ = torch.zeros_like(X)
    Y, XN, Ys, XNs = (torch.empty_like(X) for _ in range(4))
    out = torch.empty(BATCH, 3, dtype=torch.float64, device="cuda:0")
    f = lambda Z: 0.5 * ((Z @ A.T - d) ** 2).sum(dim=1)
    h = lambda Z: lam * Z.abs().sqrt().sum(dim=1)
    start = (f(X) + h(X)).clone()
    accepted = 0
    for it in range(ITERS):
        G = (X @ A.T - d) @ A                      # grad f, a row per problem
        mnu = -nu
        kw = dict(l=-delta, u=delta) if box else {}
        s.prox_step_lhalf_batch_bang(Y, G, X, SJ, lam, nu, mnu, xkn=XN, out=out, **kw)
        # the loop of single calls from the same iterate, with host copies of the scalars
        lam_h, nu_h, dl_h = lam.cpu().numpy(), nu.cpu().numpy(), delta.cpu().numpy()
        for b in range(BATCH):
            st = (ctypes.c_double * 3)()
            if box:
                rc = L.spx_proxstep_lhalf_box(ctx, _P(Ys[b]), _P(G[b]), _P(X[b]), _P(SJ[b]), N, float(lam_h[b]), float(nu_h[b]), None, None,
                                              -float(dl_h[b]), float(dl_h[b]), None, -float(nu_h[b]), _P(XNs[b]), st, None)
            else:
                rc = L.spx_proxstep_lhalf(ctx, _P(Ys[b]), _P(G[b]), _P(X[b]), _P(SJ[b]), N, float(lam_h[b]), float(nu_h[b]),
                                          -float(nu_h[b]), _P(XNs[b]), st, None)
            assert rc == 0, L.spx_last_error()
        torch.cuda.synchronize()
        if box:
            assert torch.equal(Y, Ys) and torch.equal(XN, XNs), it
        else:
            pd = s.lhalf_threshold_batch(lam, nu).cpu().numpy()
            Gh, Xh = G.cpu().numpy(), X.cpu().numpy()
            same = (Y == Ys).cpu().numpy()
            for b in range(BATCH):
                ph = 54.0 ** (1 / 3) * (2 * (float(nu_h[b]) * float(lam_h[b]))) ** (2 / 3) / 4
                assert abs(pd[b] - ph) <= 4 * np.spacing(ph)
                a = np.abs(-nu_h[b] * Gh[b] + (Xh[b] + 0.0))
                band = (a <= ph) != (a <= pd[b])
                assert same[b][~band].all(), (it, b, np.flatnonzero(~same[b] & ~band)[:5])
                yb = Y[b].cpu().numpy()
                assert np.all(yb[band & (a <= pd[b])] == 0.0 - Xh[b][band & (a <= pd[b])]), (it, b)
            assert torch.equal(XN, (X + SJ) + Y), it
        # R2's accept / reject on the device, from the batched call's statistics: model decrease xi = hk - (qy + yy / (2 nu) + h)
        hk = h(X)
        xi = hk - (out[:, 1] + out[:, 2] / (2 * nu) + out[:, 0])
        rho = ((f(X) + hk) - (f(XN) + out[:, 0])) / torch.clamp(xi, min=1e-300)
        ok = (rho >= 1e-4) & (xi > 0)
        X = torch.where(ok[:, None], XN, X).clone()
        nu = torch.where(rho >= 0.9, nu * 2.0, torch.where(ok, nu, nu / 2.0))
        accepted += int(ok.sum())
    end = f(X) + h(X)
    assert accepted > 0 and bool((end <= start).all()) and bool((end < start).any()), (start.tolist(), end.tolist())
