"""R2DH on a regularisation path in lock step:  min_x 1/2 ||A x - d||^2 + lambda_b ||x||_1  for a whole path lambda_0 > lambda_1
> ... at once, one problem per row of a batch x n tensor, ONE iprox_step_batch call per iteration for all of them.

Every problem keeps its own regularisation sigma_b and its own spectral (Barzilai-Borwein) diagonal D_b = delta_b I, held as a
batch x n tensor.  The call reads lambda_b and sigma_b from DEVICE tensors and forms d = D_b + sigma_b on the fly (d_shift), so
the `d.fill_(delta + sigma)` pass of examples/r2dh_lasso.py is gone, and rho, the accept / reject test and the updates of sigma
and delta are torch operations on device tensors: no .item(), no synchronisation, nothing baked into a launch.  That also makes
one iteration a graph -- captured once, replayed for every iteration, with the sigma and delta the previous replay left on the
device:

    iprox_step_batch_bang(S, "l1", G, D, X, 0, lam, d_shift=sigma, xkn=XN, out=stats)   # s_b, h(x_b + s_b), grad' s_b,
                                                                                         # s_b' ((D_b + sigma_b) s_b), s_b' s_b, x_b + s_b
    phi = grad' s + (s' (d .* s) - sigma s' s) / 2            # the model grad' s + 1/2 s' D s, per problem
    xi  = h(X) - (phi + h(X + s))
    rho = (f(X) + h(X) - f(XN) - h(XN)) / xi
    X[b] <- XN[b] and delta_b <- <dg, dg> / <s, dg> where rho_b >= eta1;
    sigma_b <- sigma_b / gamma where rho_b >= eta2,  gamma sigma_b where rho_b < eta1

f and grad f are written as broadcast products and sums rather than BLAS calls: every reduction then runs in a fixed order, and
an eager run and a graph replay of the loop agree bit for bit (tests/test_gpu_r2dh_batch_loop.py).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repository root: spx_amd

from r2_lasso_path import make_problem  # noqa: E402  (the same problems as the first-order path)


class R2DHLassoPath:
    """the state of the lock-step loop (all device tensors, updated in place) and one iteration of it"""

    def __init__(self, A, d, lam, sigma0=1.0, delta0=1.0, eta1=1e-4, eta2=0.9, gamma=3.0):
        import torch
        self.A, self.d, self.lam = A, d, lam
        self.eta1, self.eta2, self.gamma, self.sigma0, self.delta0 = eta1, eta2, gamma, sigma0, delta0
        batch, n = lam.numel(), A.shape[1]
        new = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=A.device)
        self.X, self.SJ, self.S, self.XN, self.G, self.D = (new(batch, n) for _ in range(6))
        self.stats = new(batch, 4)
        self.sigma, self.delta, self.fk, self.hk = new(batch), new(batch), new(batch), new(batch)
        self.d_flag = torch.zeros(batch, dtype=torch.int32, device=A.device)
        self.reset()

    def f(self, X):
        r = (X.unsqueeze(1) * self.A).sum(2) - self.d          # batch x m
        return 0.5 * (r * r).sum(1), r

    def grad(self, r):
        return (r.unsqueeze(2) * self.A).sum(1)                # batch x n

    def reset(self):
        self.X.zero_()
        self.sigma.fill_(self.sigma0)
        self.delta.fill_(self.delta0)
        self.D.fill_(self.delta0)
        fk, r = self.f(self.X)
        self.fk.copy_(fk)
        self.G.copy_(self.grad(r))
        self.hk.copy_(self.lam * self.X.abs().sum(1))

    def objective(self):
        return self.fk + self.hk

    def step(self):
        """S, XN and the four sums of every problem: one library call"""
        import spx_amd as spx
        spx.iprox_step_batch_bang(self.S, "l1", self.G, self.D, self.X, self.SJ, self.lam, d_shift=self.sigma, xkn=self.XN,
                                  out=self.stats, d_flag=self.d_flag)

    def iteration(self):
        """one R2DH iteration of every problem; enqueues only"""
        import torch
        self.step()
        hkn, gs, sds, ss = (self.stats[:, j] for j in range(4))
        xi = self.hk - ((gs + 0.5 * (sds - self.sigma * ss)) + hkn)     # model decrease
        fkn, rn = self.f(self.XN)
        rho = torch.where(xi > 0, ((self.fk + self.hk) - (fkn + hkn)) / xi, torch.full_like(xi, -1.0))
        acc = rho >= self.eta1
        Gn = self.grad(rn)
        dg = Gn - self.G
        sy, gg = (self.S * dg).sum(1), (dg * dg).sum(1)
        # spectral estimate <dg, dg> / <s, dg>, kept positive, where the step was accepted
        est = torch.clamp(gg / torch.where(sy > 0, sy, torch.ones_like(sy)), 1e-8, 1e8)
        self.delta.copy_(torch.where(acc & (sy > 0), est, self.delta))
        self.D.copy_(self.delta.unsqueeze(1).expand_as(self.D))
        rows = acc.unsqueeze(1)
        self.X.copy_(torch.where(rows, self.XN, self.X))
        self.G.copy_(torch.where(rows, Gn, self.G))
        self.fk.copy_(torch.where(acc, fkn, self.fk))
        self.hk.copy_(torch.where(acc, hkn, self.hk))
        self.sigma.copy_(torch.where(rho >= self.eta2, self.sigma / self.gamma, torch.where(acc, self.sigma, self.sigma * self.gamma)))


def run(solver, iters, graph=False):
    """`iters` iterations: eagerly, or one iteration captured into a graph (after a warm-up on the capture stream, from which
    the state is reset) and replayed.  The capture is made on ONE stream: the graph has no parallel branches."""
    import torch
    if not graph:
        for _ in range(iters):
            solver.iteration()
        return solver
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        solver.iteration(); solver.iteration()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        solver.iteration()
    solver.reset()
    torch.cuda.synchronize()
    for _ in range(iters):
        g.replay()
    return solver


if __name__ == "__main__":
    import torch
    import __graft_entry__ as ge
    ge.build()
    A, d, lam = make_problem(n=4096, m=64, batch=8, seed=0)
    sol = R2DHLassoPath(A, d, lam)
    start = sol.objective().clone()
    run(sol, 60, graph="--graph" in sys.argv)
    torch.cuda.synchronize()                                  # the first time the host waits
    for b in range(lam.numel()):
        print("lambda %.4f  objective %.6f -> %.6f  nonzeros %d  sigma %.4g  delta %.4g" % (
            float(lam[b]), float(start[b]), float(sol.objective()[b]), int((sol.X[b] != 0).sum()), float(sol.sigma[b]),
            float(sol.delta[b])))
