"""The loop of tests/test_gpu_tr_b2_batch_loop.py (a plain helper module, like tests/ws_poison.py): a trust-region proximal
gradient method on a regularisation path of a lasso in lock step,

    min_x 1/2 ||A x - d||^2 + lambda_b ||x||_1      for lambda_0 > lambda_1 > ... at once,

one problem per row of a batch x n tensor and ONE prox_step_b2_batch_bang call per iteration for all of them -- the loop of
examples/tr_group_lasso_path.py with the l2 ball of ShiftedNormL1B2 in place of the box of the Binf group operator.

Every problem keeps its own radius Delta_b (the ball ||s||_2 <= Delta_b the step is confined to) next to its own step length
nu_b, fixed here.  The call reads lambda_b, sigma_b = nu_b, q_scale_b = -nu_b and Delta_b from DEVICE tensors, so rho, the accept
/ reject test and the update of the radii are torch operations on device tensors formed from the call's `out`, and the loop never
comes back to the host; one iteration is a graph on a single stream, replayed with the radii the previous replay left there:

    G = grad f(X)
    prox_step_b2_batch_bang(S, G, X, 0, lam, nu, Delta, -nu, xkn=XN, out=stats)
    xi  = h(X) - (grad' s + h(X + s))                         # decrease of the first-order model: out[:, 1], out[:, 0]
    rho = (f(X) + h(X) - f(XN) - h(XN)) / xi
    X[b] <- XN[b] where rho_b >= eta1;   Delta_b <- gamma Delta_b where rho_b >= eta2,  Delta_b / gamma where rho_b < eta1

A x is a broadcast product and a sum, not a BLAS call: every reduction runs in a fixed order, so an eager run and a replay agree
bit for bit.

The state lives on the device of A.  With A on the CPU the step comes from the CPU oracle (oracle.prox_l1_b2 row by row): that
is how Delta0 and the path were chosen -- `python tests/tr_b2_lasso_path.py` prints, for both sizes of the test, in how many
row-iterations the oracle's step ends on the sphere and in how many inside the ball."""
import math
import os
import sys

import numpy as np

SEED, M, BATCH, ITERS = 11, 64, 5, 12
SIZES = (4096, 8200)            # the row in registers (512 lanes), the row walk
NU, DELTA0 = 0.02, 0.1
ON_SPHERE = 1e-12               # | ||s|| - Delta | <= 1e-12 Delta: the trust region is active


def make_problem(n, m=M, batch=BATCH, seed=SEED, device="cuda"):
    """A (m x n), d (m) and a geometric path of `batch` values of lambda below lambda_max = ||A' d||_inf"""
    import torch
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(m, n)) / np.sqrt(m)
    xtrue = np.zeros(n)
    k = max(1, n // 100)
    xtrue[rng.choice(n, size=k, replace=False)] = 3.0 * rng.normal(size=k)
    d = A @ xtrue + 0.01 * rng.normal(size=m)
    lam = float(np.max(np.abs(A.T @ d))) * np.geomspace(0.5, 0.02, batch)
    return tuple(torch.from_numpy(a).to(device) for a in (A, d, lam))


def oracle_step(S, G, X, SJ, lam, nu, delta, mnu, xkn, out):
    """prox_step_b2_batch_bang on CPU tensors through the CPU oracle, row by row"""
    import torch
    from oracle import oracle
    for b in range(S.shape[0]):
        q, x, sj = G[b].numpy(), X[b].numpy(), SJ[b].numpy()
        y = oracle.prox_l1_b2(float(mnu[b]) * q, x, sj, float(lam[b]), float(nu[b]), float(delta[b]))
        v = (x + sj) + y
        S[b].copy_(torch.from_numpy(y))
        xkn[b].copy_(torch.from_numpy(v))
        out[b, 0] = float(lam[b]) * math.fsum(np.abs(v).tolist())
        out[b, 1] = math.fsum((q * y).tolist())
        out[b, 2] = math.fsum((y * y).tolist())


class TRB2LassoPath:
    """the state of the lock-step loop (tensors on A's device, updated in place) and one iteration of it"""

    def __init__(self, A, d, lam, nu=NU, delta0=DELTA0, eta1=1e-4, eta2=0.9, gamma=3.0, delta_max=1e3):
        import torch
        self.A, self.d, self.lam = A, d, lam
        self.eta1, self.eta2, self.gamma, self.delta0, self.delta_max = eta1, eta2, gamma, delta0, delta_max
        if A.is_cuda:
            import spx_amd
            self.step = spx_amd.prox_step_b2_batch_bang
        else:
            self.step = oracle_step
        batch, n = lam.numel(), A.shape[1]
        new = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=A.device)
        self.X, self.SJ, self.S, self.XN = new(batch, n), new(batch, n), new(batch, n), new(batch, n)
        self.stats = new(batch, 3)
        # a step length of its own for every problem, fixed; the radii move
        self.nu = nu * (1.0 + 0.1 * torch.arange(batch, dtype=torch.float64, device=A.device))
        self.mnu = -self.nu
        self.delta, self.fk, self.hk = new(batch), new(batch), new(batch)
        self.reset()

    def f(self, X):
        r = (X.unsqueeze(1) * self.A).sum(2) - self.d          # batch x m
        return 0.5 * (r * r).sum(1), r

    def grad(self, r):
        return (r.unsqueeze(2) * self.A).sum(1)                # batch x n

    def h(self, X):
        return self.lam * X.abs().sum(1)

    def reset(self):
        self.X.zero_()
        self.delta.fill_(self.delta0)
        self.fk.copy_(self.f(self.X)[0])
        self.hk.copy_(self.h(self.X))

    def objective(self):
        return self.fk + self.hk

    def iteration(self):
        """one trust-region iteration of every problem; on the device it enqueues only"""
        import torch
        G = self.grad(self.f(self.X)[1])
        self.step(self.S, G, self.X, self.SJ, self.lam, self.nu, self.delta, self.mnu, xkn=self.XN, out=self.stats)
        hkn, gts = self.stats[:, 0], self.stats[:, 1]
        fkn = self.f(self.XN)[0]
        xi = self.hk - (gts + hkn)
        rho = torch.where(xi > 0, ((self.fk + self.hk) - (fkn + hkn)) / xi, torch.full_like(xi, -1.0))
        acc = rho >= self.eta1
        self.X.copy_(torch.where(acc.unsqueeze(1), self.XN, self.X))
        self.fk.copy_(torch.where(acc, fkn, self.fk))
        self.hk.copy_(torch.where(acc, hkn, self.hk))
        grown = torch.clamp(self.delta * self.gamma, max=self.delta_max)
        self.delta.copy_(torch.where(rho >= self.eta2, grown, torch.where(acc, self.delta, self.delta / self.gamma)))


def run(solver, iters, graph=False):
    """`iters` iterations: eagerly, or one iteration captured into a graph (a single stream, after a warm-up on it, from which
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


def regimes(steps):
    """[(Delta as the call read it, S of that call)] -> (row-iterations on the sphere, row-iterations strictly inside the ball),
    the norms by math.fsum on the host"""
    on = inside = 0
    for delta, S in steps:
        for b in range(S.shape[0]):
            nrm, dl = math.sqrt(math.fsum((S[b].double().cpu().numpy() ** 2).tolist())), float(delta[b])
            if abs(nrm - dl) <= ON_SPHERE * dl:
                on += 1
            elif nrm < dl:
                inside += 1
    return on, inside


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle
    oracle.build()
    for n in SIZES:
        sol = TRB2LassoPath(*make_problem(n, device="cpu"))
        start = sol.objective().clone()
        steps = []
        for _ in range(ITERS):
            dl = sol.delta.clone()
            sol.iteration()
            steps.append((dl, sol.S.clone()))
        on, inside = regimes(steps)
        print("n = %d, seed %d: %d row-iterations on the sphere, %d inside the ball; Delta %s; objective %s -> %s" % (
            n, SEED, on, inside, ["%.4g" % v for v in sol.delta.tolist()], ["%.5g" % v for v in start.tolist()],
            ["%.5g" % v for v in sol.objective().tolist()]))
