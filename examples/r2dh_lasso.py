"""R2DH (quadratic regularisation with a diagonal quasi-Newton model, RegularizedOptimization.jl [ext]) for
min_x 1/2 ||A x - b||^2 + lambda ||x||_1  with the iprox! hot path on the GPU.  The loop below is the solver's inner loop in
miniature, using only the mirrored API; the diagonal is the spectral (Barzilai-Borwein) estimate D = delta I, and the step
solves  min_s grad' s + 1/2 s'(D + sigma I) s + psi(s)  with d = delta + sigma as a vector:

    psi = shifted(h, xk)                                    # borrows xk: updating xk in place re-centres psi
    s, hkn, gs, sds, ss = iprox_step(psi, grad, d, xkn=xkn) # s, h(xk + s), grad' s, s'(d .* s), s's and xk + s: ONE pass
    phi = gs + (sds - sigma * ss) / 2                       # the model grad' s + 1/2 s' D s (the caller halves)

`--unfused` makes the separate calls instead -- iprox, psi(s), torch.dot three times, xk + s -- and follows the same
trajectory: the iterates have equal bits as long as the accept / reject decisions agree (tests/test_gpu_r2dh_loop.py).

    python examples/r2dh_lasso.py --n 10000 --iters 20 [--unfused]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repository root: spx_amd


def r2dh_lasso(A, b, lam, x0, max_iter=50, tol=1e-8, eta1=1e-4, eta2=0.9, gamma=3.0, sigma0=1.0, fused=True):
    """returns (x, history of (iteration, objective, sigma, accepted), the iterates after every iteration)"""
    import torch
    import spx_amd as spx
    xk = x0.clone()
    psi = spx.shifted(spx.NormL1(lam), xk)
    xkn = torch.empty_like(xk)
    d = torch.empty_like(xk)
    res = A @ xk - b
    fk, hk = 0.5 * float(torch.dot(res, res)), psi(torch.zeros_like(xk))
    grad = A.T @ res
    sigma, delta = sigma0, 1.0
    hist, iterates = [], []
    for it in range(max_iter):
        d.fill_(delta + sigma)
        if fused:
            s, hkn, gs, sds, ss = spx.iprox_step(psi, grad, d, xkn=xkn)
        else:
            s = spx.iprox(psi, grad, d)
            hkn = psi(s)
            gs, sds, ss = float(torch.dot(grad, s)), float(torch.dot(s, d * s)), float(torch.dot(s, s))
            torch.add(xk, s, out=xkn)
        xi = hk - ((gs + 0.5 * (sds - sigma * ss)) + hkn)     # model decrease
        if xi < 0 or np.sqrt(max(xi, 0.0)) < tol:
            hist.append((it, fk + hk, sigma, None))
            break
        resn = A @ xkn - b
        fkn = 0.5 * float(torch.dot(resn, resn))
        rho = (fk + hk - fkn - hkn) / xi
        accepted = rho >= eta1
        hist.append((it, fk + hk, sigma, accepted))
        if accepted:
            gradn = A.T @ resn
            dg = gradn - grad
            # spectral estimate <dg, dg> / <s, dg>, dg = grad+ - grad, kept positive.  (Formed from the smooth part's own
            # dot products in either mode: the step statistics steer the accept / reject decisions only, so the fused
            # and the unfused loop keep the same d, hence the same iterates, bit for bit.)
            sy, gg = float(torch.dot(s, dg)), float(torch.dot(dg, dg))
            delta = min(max(gg / sy, 1e-8), 1e8) if sy > 0 else delta
            xk.copy_(xkn)                                 # in place: psi.xk IS xk  (shift!(psi, xk))
            res, fk, hk, grad = resn, fkn, hkn, gradn
        if rho >= eta2:
            sigma /= gamma
        elif rho < eta1:
            sigma *= gamma
        iterates.append(xk.clone())
    return xk, hist, iterates


def problem(n, m=None, seed=0, device="cuda"):
    import torch
    m = m if m is not None else max(10, n // 20)
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(m, n)) / np.sqrt(m)
    xtrue = np.zeros(n)
    k = max(1, n // 100)
    xtrue[rng.choice(n, size=k, replace=False)] = rng.normal(size=k) * 3
    b = A @ xtrue + 0.01 * rng.normal(size=m)
    return torch.from_numpy(A).to(device), torch.from_numpy(b).to(device)


def main(argv=None):
    import torch
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lam", type=float, default=0.05)
    ap.add_argument("--unfused", action="store_true", help="separate iprox / psi / dot / add calls instead of one iprox_step")
    a = ap.parse_args(argv)
    A, b = problem(a.n)
    x0 = torch.zeros(a.n, dtype=torch.float64, device="cuda")
    x, hist, iterates = r2dh_lasso(A, b, a.lam, x0, max_iter=a.iters, fused=not a.unfused)
    print("iterations", len(hist), "objective", hist[-1][1], "nnz", int((x != 0).sum()), "unfused" if a.unfused else "fused")
    return x, hist, iterates


if __name__ == "__main__":
    main()
