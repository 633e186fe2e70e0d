"""R2DH in miniature (examples/r2dh_lasso.py) at n = 1e4 for a few iterations: one iprox_step call per iteration against the
`--unfused` loop of separate calls.  The iterates have equal bits after every iteration -- y and xkn of the fused call are
those of iprox! and xk + s, and the sums only steer the accept / reject decisions, which must agree -- and the objective
agrees to 1e-12 relative per iteration."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_r2dh_lasso_fused_follows_the_unfused_loop():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    ge.build()
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import r2dh_lasso
    args = ["--n", "10000", "--iters", "12"]
    x_fus, h_fus, it_fus = r2dh_lasso.main(args)
    x_ref, h_ref, it_ref = r2dh_lasso.main(args + ["--unfused"])
    assert len(h_fus) == len(h_ref) and len(it_fus) == len(it_ref) and len(h_fus) >= 6
    for (i0, o0, s0, a0), (i1, o1, s1, a1) in zip(h_ref, h_fus):
        print(i0, o0, o1, s0, a0)
        assert a0 == a1 and s0 == s1 and abs(o0 - o1) <= 1e-12 * abs(o0)
    for k, (u, v) in enumerate(zip(it_ref, it_fus)):
        assert torch.equal(u, v), k
    assert torch.equal(x_fus, x_ref)
    assert sum(1 for h in h_fus if h[3]) >= 3 and h_fus[-1][1] < 0.5 * h_fus[0][1]      # steps were accepted and it did minimise
