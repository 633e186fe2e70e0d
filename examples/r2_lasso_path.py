"""R2 on a regularisation path in lock step:  min_x 1/2 ||A x - d||^2 + lambda_b ||x||_1  for a whole path lambda_0 > lambda_1 >
... at once, one problem per row of a batch x n tensor, ONE prox_step_batch call per iteration for all of them.

Every problem keeps its own step size nu_b.  The call reads lambda_b, sigma_b = nu_b and q_scale_b = -nu_b from DEVICE tensors,
so rho, the accept / reject test and the update of nu are torch operations on device tensors and the loop never comes back to
the host: no .item(), no synchronisation, nothing baked into a launch.  That also makes one iteration a graph -- captured once,
replayed for every iteration, with the nu the previous replay left on the device:

    G = grad f(X)                                             # torch
    prox_step_batch_bang(S, "l1", G, X, 0, lam, nu, -nu, xkn=XN, out=stats)   # s_b, h(x_b + s_b), grad' s_b, x_b + s_b
    xi  = h(X) - (grad' s + h(X + s))                         # decrease of the first-order model, per problem
    rho = (f(X) + h(X) - f(XN) - h(XN)) / xi
    X[b] <- XN[b] where rho_b >= eta1;   nu_b <- gamma nu_b where rho_b >= eta2,  nu_b / gamma where rho_b < eta1

A x is written as a broadcast product and a sum rather than a BLAS call: every reduction then runs in a fixed order, and an eager
run and a graph replay of the loop agree bit for bit (tests/test_gpu_r2_batch_loop.py).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repository root: spx_amd


def make_problem(n, m, batch, seed, device="cuda"):
    """A (m x n), d (m), and a geometric path of `batch` values of lambda below lambda_max = ||A' d||_inf"""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(m, n)) / np.sqrt(m)
    xtrue = np.zeros(n)
    k = max(1, n // 100)
    xtrue[rng.choice(n, size=k, replace=False)] = 3.0 * rng.normal(size=k)
    d = A @ xtrue + 0.01 * rng.normal(size=m)
    lam_max = float(np.max(np.abs(A.T @ d)))
    lam = lam_max * np.geomspace(0.5, 0.02, batch)
    return (torch.from_numpy(A).to(device), torch.from_numpy(d).to(device), torch.from_numpy(lam).to(device))


class R2LassoPath:
    """the state of the lock-step loop (all device tensors, updated in place) and one iteration of it"""

    def __init__(self, A, d, lam, nu0=0.2, eta1=1e-4, eta2=0.9, gamma=3.0):
        import torch
        import spx_amd as spx
        self.spx, self.A, self.d, self.lam = spx, A, d, lam
        self.eta1, self.eta2, self.gamma, self.nu0 = eta1, eta2, gamma, nu0
        batch, n = lam.numel(), A.shape[1]
        new = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=A.device)
        self.X, self.SJ, self.S, self.XN = new(batch, n), new(batch, n), new(batch, n), new(batch, n)
        self.stats = new(batch, 3)
        self.nu, self.mnu, self.fk, self.hk = new(batch), new(batch), new(batch), new(batch)
        self.reset()

    def f(self, X):
        r = (X.unsqueeze(1) * self.A).sum(2) - self.d          # batch x m
        return 0.5 * (r * r).sum(1), r

    def grad(self, r):
        return (r.unsqueeze(2) * self.A).sum(1)                # batch x n

    def reset(self):
        self.X.zero_()
        self.nu.fill_(self.nu0)
        self.mnu.fill_(-self.nu0)
        self.fk.copy_(self.f(self.X)[0])
        self.hk.copy_(self.lam * self.X.abs().sum(1))

    def objective(self):
        return self.fk + self.hk

    def iteration(self):
        """one R2 iteration of every problem; enqueues only"""
        import torch
        G = self.grad(self.f(self.X)[1])
        self.spx.prox_step_batch_bang(self.S, "l1", G, self.X, self.SJ, self.lam, self.nu, self.mnu, xkn=self.XN, out=self.stats)
        hkn, gts = self.stats[:, 0], self.stats[:, 1]
        fkn = self.f(self.XN)[0]
        xi = self.hk - (gts + hkn)
        rho = torch.where(xi > 0, ((self.fk + self.hk) - (fkn + hkn)) / xi, torch.full_like(xi, -1.0))
        acc = rho >= self.eta1
        self.X.copy_(torch.where(acc.unsqueeze(1), self.XN, self.X))
        self.fk.copy_(torch.where(acc, fkn, self.fk))
        self.hk.copy_(torch.where(acc, hkn, self.hk))
        self.nu.copy_(torch.where(rho >= self.eta2, self.nu * self.gamma, torch.where(acc, self.nu, self.nu / self.gamma)))
        self.mnu.copy_(-self.nu)


def run(solver, iters, graph=False):
    """`iters` iterations: eagerly, or one iteration captured into a graph (after a warm-up on the capture stream, from which
    the state is reset) and replayed"""
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
    sol = R2LassoPath(A, d, lam)
    start = sol.objective().clone()
    run(sol, 60, graph="--graph" in sys.argv)
    torch.cuda.synchronize()                                  # the first time the host waits
    for b in range(lam.numel()):
        print("lambda %.4f  objective %.6f -> %.6f  nonzeros %d  nu %.4g" % (
            float(lam[b]), float(start[b]), float(sol.objective()[b]), int((sol.X[b] != 0).sum()), float(sol.nu[b])))
