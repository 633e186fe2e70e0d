"""GPU: the lock-step trust-region loop of examples/tr_group_lasso_path.py -- one prox_step_group_binf_batch call per iteration
for a whole lambda path of a group lasso, rho, accept / reject and the update of every problem's radius as torch operations on
device tensors -- on 5 problems with n = 4096 in groups of 8: 12 iterations run eagerly, and one iteration captured into a graph
(a single stream, no parallel branches) and replayed 12 times.  The captured call reads Delta, nu and lambda from the device, so
the replays follow the radii the previous replays left there: iterates, radii, fk and hk are bit-identical between the two runs
(had the scalars been baked into the launch, the replays would keep Delta0).  Every problem's objective decreased."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lock_step_group_tr_eager_and_replayed_agree_bit_for_bit():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    ge.build()
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from tr_group_lasso_path import TRGroupLassoPath, make_problem, run
    A, d, w, lam = make_problem(n=4096, m=64, batch=5, group_size=8, seed=3)
    eager, replayed = TRGroupLassoPath(A, d, w, lam, 8), TRGroupLassoPath(A, d, w, lam, 8)
    start = eager.objective().clone()
    run(eager, 12)
    run(replayed, 12, graph=True)
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
