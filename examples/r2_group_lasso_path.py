"""R2 on a regularisation path of a GROUP lasso in lock step:  min_x 1/2 ||A x - d||^2 + lambda_b sum_g w_g ||x[g]||_2  for a
whole path lambda_0 > lambda_1 > ... at once, one problem per row of a batch x n tensor, uniform contiguous groups, ONE
prox_step_group_batch call per iteration for all of them.

The group weights w are ONE device vector shared by the problems; the path is the `batch` scalars lambda_b, handed to the call
as lam_scale (the weight of group g of problem b is lambda_b * w_g, one rounded multiply).  Every problem keeps its own step
size nu_b.  The call reads lambda_b, sigma_b = nu_b and q_scale_b = -nu_b from DEVICE tensors, so rho, the accept / reject test
and the update of nu are torch operations on device tensors and the loop never comes back to the host: no .item(), no
synchronisation, nothing baked into a launch.  That also makes one iteration a graph -- captured once, replayed for every
iteration, with the nu the previous replay left on the device:

    G = grad f(X)                                             # torch
    prox_step_group_batch_bang(S, G, X, 0, group_size, w, nu, -nu, lam_scale=lam, xkn=XN, out=stats)
    xi  = h(X) - (grad' s + h(X + s))                         # decrease of the first-order model, per problem
    rho = (f(X) + h(X) - f(XN) - h(XN)) / xi
    X[b] <- XN[b] where rho_b >= eta1;   nu_b <- gamma nu_b where rho_b >= eta2,  nu_b / gamma where rho_b < eta1

A x is written as a broadcast product and a sum rather than a BLAS call: every reduction then runs in a fixed order, and an eager
run and a graph replay of the loop agree bit for bit (tests/test_gpu_r2_group_batch_loop.py).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repository root: spx_amd


def make_problem(n, m, batch, group_size, seed, device="cuda"):
    """A (m x n), d (m), the group weights w (n / group_size, sqrt(group_size) each) and a geometric path of `batch` values of
    lambda below lambda_max = max_g ||A[:, g]' d|| / w_g"""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    ng = n // group_size
    A = rng.normal(size=(m, n)) / np.sqrt(m)
    xtrue = np.zeros(n)
    for g in rng.choice(ng, size=max(1, ng // 50), replace=False):
        xtrue[g * group_size:(g + 1) * group_size] = 3.0 * rng.normal(size=group_size)
    d = A @ xtrue + 0.01 * rng.normal(size=m)
    w = np.full(ng, np.sqrt(group_size))
    lam_max = float(np.max(np.linalg.norm((A.T @ d).reshape(ng, group_size), axis=1) / w))
    lam = lam_max * np.geomspace(0.5, 0.02, batch)
    return tuple(torch.from_numpy(a).to(device) for a in (A, d, w, lam))


class R2GroupLassoPath:
    """the state of the lock-step loop (all device tensors, updated in place) and one iteration of it"""

    def __init__(self, A, d, w, lam, group_size, nu0=0.2, eta1=1e-4, eta2=0.9, gamma=3.0):
        import torch
        import spx_amd as spx
        self.spx, self.A, self.d, self.w, self.lam, self.group_size = spx, A, d, w, lam, group_size
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

    def h(self, X):
        norms = (X * X).reshape(X.shape[0], -1, self.group_size).sum(2).sqrt()   # batch x ngroups
        return self.lam * (norms * self.w).sum(1)

    def reset(self):
        self.X.zero_()
        self.nu.fill_(self.nu0)
        self.mnu.fill_(-self.nu0)
        self.fk.copy_(self.f(self.X)[0])
        self.hk.copy_(self.h(self.X))

    def objective(self):
        return self.fk + self.hk

    def iteration(self):
        """one R2 iteration of every problem; enqueues only"""
        import torch
        G = self.grad(self.f(self.X)[1])
        self.spx.prox_step_group_batch_bang(self.S, G, self.X, self.SJ, self.group_size, self.w, self.nu, self.mnu,
                                            lam_scale=self.lam, xkn=self.XN, out=self.stats)
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
    gs = 8
    A, d, w, lam = make_problem(n=4096, m=64, batch=8, group_size=gs, seed=0)
    sol = R2GroupLassoPath(A, d, w, lam, gs)
    start = sol.objective().clone()
    run(sol, 60, graph="--graph" in sys.argv)
    torch.cuda.synchronize()                                  # the first time the host waits
    for b in range(lam.numel()):
        groups = int((sol.X[b].reshape(-1, gs) != 0).any(dim=1).sum())
        print("lambda %.4f  objective %.6f -> %.6f  nonzero groups %d  nu %.4g" % (
            float(lam[b]), float(start[b]), float(sol.objective()[b]), groups, float(sol.nu[b])))
