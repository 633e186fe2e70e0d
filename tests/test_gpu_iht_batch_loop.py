"""GPU: iterative hard thresholding over a path of r in ONE call per iteration, through the Python mirror
(prox_step_topr_batch_bang): five iterations of projected gradient on a 64 x 256 least-squares problem, min ||A x - b||^2 over
||x||_0 <= r, for 8 values of r at once -- row k of the 8 x 256 iterate is the problem with r[k].

    g = A' (A x - b);   x+ = H_r(x - mu g) = xk + prox!(shifted(IndBallL0(r), xk), -mu g)   (sj = 0, q_scale = -mu, xkn = x+)

Every iterate is compared bit for bit with the same loop over single calls (spx_prox_indball_l0[_binf] on each row with
q = -mu g multiplied beforehand): both loops form each row's gradient by the same two matrix-vector products, so the iterates
can be held to equality.  The BInf form runs the same loop inside a trust region of radius Delta_k per row."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, N, ITERS = 64, 256, 5
RS = [1, 2, 5, 12, 32, 77, 200, 256]


@pytest.fixture(scope="module")
def s():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.build()


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _bits(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


@pytest.mark.parametrize("binf", [False, True], ids=["plain", "binf"])
def test_iht_over_a_path_of_r_matches_the_loop_of_single_calls(s, binf):
    import torch
    rng = np.random.default_rng(7100)
    A = torch.from_numpy(rng.normal(size=(M, N)) / np.sqrt(M)).cuda()
    x_true = np.zeros(N)
    x_true[rng.choice(N, size=12, replace=False)] = rng.normal(size=12) * 3.0
    b = A @ torch.from_numpy(x_true).cuda() + 0.01 * torch.from_numpy(rng.normal(size=M)).cuda()
    mu = 0.5 / float(torch.linalg.matrix_norm(A, 2) ** 2)
    batch = len(RS)
    r = torch.tensor(RS, dtype=torch.int64, device="cuda:0")
    qs = torch.full((batch,), -mu, dtype=torch.float64, device="cuda:0")
    dlt = torch.from_numpy(rng.uniform(0.05, 0.6, size=batch)).cuda() if binf else None
    dlt_h = dlt.cpu().numpy() if binf else None
    L, ctx = s._lib.load(), s.context("cuda:0")

    def gradient(x):          # one row: two matrix-vector products, the same in both loops
        return A.T @ (A @ x - b)

    X = torch.zeros(batch, N, dtype=torch.float64, device="cuda:0")           # the batched loop's iterates
    Xs = X.clone()                                                            # the single-call loop's
    SJ = torch.zeros_like(X)
    Y, Xn, out = torch.empty_like(X), torch.empty_like(X), torch.empty(batch, 3, dtype=torch.float64, device="cuda:0")
    for it in range(ITERS):
        G = torch.stack([gradient(X[k]) for k in range(batch)])
        s.prox_step_topr_batch_bang(Y, G, X, SJ, r, qs, delta=dlt, xkn=Xn, out=out)
        for k in range(batch):
            q = (-mu) * gradient(Xs[k])                                       # multiplied beforehand: one rounded multiply
            y = torch.empty(N, dtype=torch.float64, device="cuda:0")
            xk, sj = Xs[k].clone(), SJ[k].clone()
            if binf:
                rc = L.spx_prox_indball_l0_binf(ctx, _P(y), _P(q), _P(xk), _P(sj), N, RS[k], float(dlt_h[k]))
            else:
                rc = L.spx_prox_indball_l0(ctx, _P(y), _P(q), _P(xk), _P(sj), N, RS[k])
            assert rc == 0, L.spx_last_error()
            assert _bits(Y[k], y), (it, k)
            Xs[k] = (xk + sj) + y
        assert _bits(Xn, Xs), it                                              # every iterate, bit for bit
        nnz = out[:, 0].cpu().numpy()
        assert np.array_equal(nnz, (Xn != 0).sum(dim=1).cpu().numpy().astype(np.float64)), it
        if not binf:
            assert (nnz <= np.array(RS)).all(), (it, nnz)                     # h = 0: the iterate is in the ball
        X, Xn = Xn, X
    if not binf:   # the path is nested in r and the large-r end has found the support
        res = [float(torch.linalg.vector_norm(A @ X[k] - b)) for k in range(batch)]
        print("residuals over r:", ["%.3e" % v for v in res])
        assert res[-1] < res[0]
