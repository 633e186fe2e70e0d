"""GPU: the lock-step R2DH loop of examples/r2dh_lasso_path.py -- one iprox_step_batch call per iteration for a whole lambda
path, D_b = delta_b I as a batch x n tensor, sigma_b in a device tensor passed as d_shift, rho, accept / reject and the sigma and
delta updates as torch operations on device tensors -- on 5 problems with n = 4096: 12 iterations run eagerly, and one iteration
captured into a graph (on one stream) and replayed 12 times.  The captured call reads lambda and sigma from the device and forms
D + sigma on the fly, so the replays follow the sigma and delta the previous replays left there: X, sigma, delta, f and h are
bit-identical between the two runs (had the scalars been baked into the launch, the replays would keep sigma0).  sigma moved away
from sigma0, not the same way in every problem, and no objective rose."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lock_step_r2dh_eager_and_replayed_agree_bit_for_bit():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    ge.build()
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from r2dh_lasso_path import R2DHLassoPath, make_problem, run
    A, d, lam = make_problem(n=4096, m=64, batch=5, seed=3)
    eager, replayed = R2DHLassoPath(A, d, lam), R2DHLassoPath(A, d, lam)
    start = eager.objective().clone()
    run(eager, 12)
    run(replayed, 12, graph=True)
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int64)
    assert torch.equal(bits(eager.X), bits(replayed.X))
    assert torch.equal(bits(eager.sigma), bits(replayed.sigma)) and torch.equal(bits(eager.delta), bits(replayed.delta))
    assert torch.equal(bits(eager.fk), bits(replayed.fk)) and torch.equal(bits(eager.hk), bits(replayed.hk))
    # the loop did something: steps were accepted, sigma moved away from sigma0, not the same way in every problem, and the
    # spectral estimate replaced delta0
    assert bool((eager.X != 0).any(dim=1).all())
    assert bool((eager.sigma != eager.sigma0).all()) and eager.sigma.unique().numel() > 1, eager.sigma.tolist()
    assert bool((eager.delta != eager.delta0).all()), eager.delta.tolist()
    assert eager.d_flag.tolist() == [0] * 5          # D + sigma stayed positive in every problem
    end = eager.objective()
    assert bool((end <= start).all()) and bool((end < start).all()), (start.tolist(), end.tolist())
