"""R2 (examples/r2_lasso.py) with fused_step=True -- s, h(xk + s), grad' s and xk + s from ONE prox_step call per iteration --
against the same loop with fused_step=False, on the problem and with the bars of tests/test_gpu_r2_loop.py: the same accept /
reject sequence and step sizes, the objective within 1e-10 relative per iteration, x within 1e-9 with the same support."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_r2_lasso_fused_step_follows_the_unfused_loop():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    ge.build()
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from r2_lasso import r2_lasso
    rng = np.random.default_rng(0)
    m, n = 300, 2000
    A = rng.normal(size=(m, n)) / np.sqrt(m)
    xtrue = np.zeros(n)
    xtrue[rng.choice(n, size=25, replace=False)] = rng.normal(size=25) * 3
    b = A @ xtrue + 0.01 * rng.normal(size=m)
    lam = 0.05
    Ad, bd = torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda()
    x0 = torch.zeros(n, dtype=torch.float64, device="cuda")
    x_ref, h_ref = r2_lasso(Ad, bd, lam, x0, "gpu", max_iter=120, nu0=0.2, fused_step=False)
    x_fus, h_fus = r2_lasso(Ad, bd, lam, x0, "gpu", max_iter=120, nu0=0.2, fused_step=True)
    assert len(h_ref) == len(h_fus) and len(h_fus) > 10
    for (i0, o0, nu0, a0), (i1, o1, nu1, a1) in zip(h_ref, h_fus):
        assert a0 == a1 and nu0 == nu1 and abs(o0 - o1) <= 1e-10 * abs(o0)
    xr, xf = x_ref.cpu().numpy(), x_fus.cpu().numpy()
    assert np.max(np.abs(xf - xr)) <= 1e-9 * max(1.0, np.max(np.abs(xr)))
    assert np.array_equal(xf != 0, xr != 0)                     # same support
    assert h_fus[-1][1] < 0.5 * h_fus[0][1]                      # and it did minimise
    with pytest.raises(ValueError):
        r2_lasso(A, b, lam, np.zeros(n), "oracle", max_iter=1, fused_step=True)
