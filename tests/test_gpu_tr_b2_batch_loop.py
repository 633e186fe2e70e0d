"""GPU: the lock-step trust-region loop of tests/tr_b2_lasso_path.py -- one prox_step_b2_batch_bang call per iteration for a whole
lambda path of a lasso, rho, accept / reject and the update of every problem's radius as torch operations on device tensors -- on
5 problems, m = 64, at n = 4096 (the row stays in registers) and n = 8200 (the row walk): 12 iterations run eagerly, and one
iteration captured into a graph (a single stream, no parallel branches) and replayed 12 times.  The captured call reads Delta, nu
and lambda from the device, so the replays follow the radii the previous replays left there: iterates, radii, fk and hk are
bit-identical between the two runs (had the scalars been baked into the launch, the replays would keep Delta0) -- the header's
promise that a row's bits depend on neither batch, row nor timing.  Every problem's objective decreased; every iteration's rows
meet spx_proxstep_l1_b2 on that row at the B2 bar.

Both regimes of the root iteration occur.  Seed 11, nu = 0.02 (1 + 0.1 b), Delta0 = 0.1, gamma = 3: through the CPU oracle
(`python tests/tr_b2_lasso_path.py`) the step of 21 of the 60 row-iterations ends on the sphere and of 39 inside the ball at
n = 4096, of 37 and 23 at n = 8200; the radii end at 4 different values at either size."""
import ctypes
import math

import numpy as np
import pytest

import tr_b2_lasso_path as tr

pytestmark = pytest.mark.gpu
TOL = 1e-12


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("n", tr.SIZES, ids=["registers", "row-walk"])
def test_lock_step_b2_tr_eager_and_replayed_agree_bit_for_bit(n):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    s = ge.build()
    A, d, lam = tr.make_problem(n)
    eager, replayed = tr.TRB2LassoPath(A, d, lam), tr.TRB2LassoPath(A, d, lam)
    start = eager.objective().clone()
    steps = []                                       # what every eager call read and stored: (X, Delta, S)
    for _ in range(tr.ITERS):
        before = (eager.X.clone(), eager.delta.clone())
        eager.iteration()
        steps.append(before + (eager.S.clone(),))
    tr.run(replayed, tr.ITERS, graph=True)
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int64)
    assert torch.equal(bits(eager.X), bits(replayed.X))
    assert torch.equal(bits(eager.delta), bits(replayed.delta))
    assert torch.equal(bits(eager.fk), bits(replayed.fk)) and torch.equal(bits(eager.hk), bits(replayed.hk))
    # the loop did something: steps were accepted and the radii moved away from Delta0, not all the same way
    assert bool((eager.X != 0).any(dim=1).all())
    assert bool((eager.delta != eager.delta0).any()) and eager.delta.unique().numel() > 1
    end = eager.objective()
    assert bool((end < start).all()), (start.tolist(), end.tolist())
    # h as the call's statistics carried it is h of the iterate, to the bar of the blocked sums
    assert torch.allclose(eager.hk, eager.h(eager.X), rtol=1e-12, atol=0.0)
    # a condition on the run, not a measurement: both regimes of the root iteration occurred
    on, inside = tr.regimes([(dl, S) for _, dl, S in steps])
    print("n = %d: %d row-iterations on the sphere, %d inside the ball" % (n, on, inside))
    assert on >= 1 and inside >= 1, (on, inside)
    # every iteration's rows against the single call on that row with host copies of its scalars
    L, ctx = s._lib.load(), s.context("cuda:0")
    lam_h, nu_h = lam.cpu().numpy(), eager.nu.cpu().numpy()
    worst = 0.0
    for it, (X, dl, S) in enumerate(steps):
        G = eager.grad(eager.f(X)[1])
        dl_h = dl.cpu().numpy()
        for b in range(lam.numel()):
            q, xk, sj = G[b].clone(), X[b].clone(), torch.zeros_like(X[b])
            ys, ks = torch.empty_like(q), torch.empty_like(q)
            st = (ctypes.c_double * 3)()
            rc = L.spx_proxstep_l1_b2(ctx, _P(ys), _P(q), _P(xk), _P(sj), n, float(lam_h[b]), float(nu_h[b]), float(dl_h[b]), 1.0,
                                      -float(nu_h[b]), _P(ks), st, None)
            assert rc == 0, L.spx_last_error()
            ref, y = ys.cpu().numpy(), S[b].cpu().numpy()
            bar = TOL * max(float(np.linalg.norm(ref)), float(np.linalg.norm(xk.cpu().numpy())))
            err = float(np.max(np.abs(y - ref)))
            worst = max(worst, err / bar)
            assert math.isfinite(err) and err <= bar, (n, it, b, err, bar)
    print("n = %d: worst max |y - single call| / bar over %d rows: %.3g" % (n, len(steps) * lam.numel(), worst))
