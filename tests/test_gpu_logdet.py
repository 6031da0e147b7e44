"""logdet (stochastic Lanczos quadrature over mbcg), PivotedCholeskyPreconditioner.sample and inv_quad_logdet on the device, fp64.
Problem: EQ(l = 0.5), d = 2, n = 257, N(0, I) points, A = G + 0.1 I (case A of tests/test_gpu_mbcg.py).

The statistical bounds are exact deviations computed by numpy: for Rademacher probes Var(z' log(A) z) = 2 (|log A|_F^2 - sum diag(log A)^2),
for probes ~ N(0, M) with the preconditioner Var = 2 |log(M^-1/2 A M^-1/2)|_F^2; sigma is the deviation of the mean of 64 draws.  The
estimate must lie within 5 sigma of numpy's slogdet, and the reported standard error within [sigma / 2, 2 sigma] (a sample deviation over
64 draws is within 9 % at one sigma)."""
import functools

import numpy as np
import pytest
import torch

import covgram_oracle as o
import mbcg_ref as mr

pytestmark = pytest.mark.gpu

N, SHIFT, RANK = 257, 0.1, 32


@functools.lru_cache(maxsize=None)
def problem():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((N, 2))
    A = o.matrix(o.Kernel(o.EQ, lengthscale=0.5), X) + SHIFT * np.eye(N)
    logA = mr.sym_fun(A, np.log)
    Z = rng.choice([-1.0, 1.0], size=(N, 5))
    b = rng.standard_normal(N)
    return X, A, logA, float(np.linalg.slogdet(A)[1]), Z, b, float(np.linalg.cond(A))


def device(cg):
    Xt = torch.from_numpy(problem()[0]).cuda()
    G = cg.gramian(cg.Lengthscale(cg.EQ(), 0.5), Xt)
    return G, G + torch.full((N,), SHIFT, dtype=torch.float64, device="cuda")


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def test_explicit_probes(cg):
    X, Am, logA, ld, Z, b, cond = problem()
    G, A = device(cg)
    exact = np.einsum("ij,ik,kj->j", Z, logA, Z)
    _, ref = mr.mbcg(Am, Z, maxiter=80, reltol=0.0)
    q_ref = np.array([N * mr.quadrature(mr.tridiagonal(ref["alpha"][:, j], ref["beta"][:, j], 80), np.log) for j in range(5)])
    e_ref = float(np.max(np.abs(q_ref - exact) / np.abs(exact)))
    est, info = cg.logdet(A, probes=torch.from_numpy(Z).cuda(), reltol=0.0, maxiter=80)
    vals = info["values"].numpy()
    print(f"\nexplicit probes: estimate {est:.12g}, mean of the exact values {exact.mean():.12g}; per-probe error {np.max(np.abs(vals - exact) / np.abs(exact)):.3g} "
          f"(restatement {e_ref:.3g})")
    assert info["probes"] == 5 and vals.shape == (5,)
    assert (np.abs(vals - exact) <= 10 * e_ref * np.abs(exact)).all()
    assert abs(est - exact.mean()) <= 10 * e_ref * np.abs(exact).mean()
    assert abs(info["stderr"] - vals.std(ddof=1) / np.sqrt(5)) <= 1e-12 * abs(info["stderr"])


def test_rademacher(cg):
    X, Am, logA, ld, Z, b, cond = problem()
    G, A = device(cg)
    sigma = float(np.sqrt(2.0 * (np.sum(logA ** 2) - np.sum(np.diag(logA) ** 2)) / 64))
    est, info = cg.logdet(A, probes=64, generator=gen(1))
    print(f"\nRademacher: estimate {est:.6g} against {ld:.6g} (sigma {sigma:.3g}, {abs(est - ld) / sigma:.2f} sigma), stderr {info['stderr']:.3g}, "
          f"{info['iterations']} iterations")
    assert info["converged"] and info["probes"] == 64
    assert torch.allclose(info["rz0"], torch.full((64,), float(N), dtype=torch.float64), rtol=1e-14, atol=0)   # z'z = n for ±1 probes
    assert abs(est - ld) <= 5 * sigma
    assert sigma / 2 <= info["stderr"] <= 2 * sigma
    est2, _ = cg.logdet(A, probes=64, generator=gen(1))
    assert est2 == est                                                          # the same seed: the same bits


def test_preconditioned(cg):
    X, Am, logA, ld, Z, b, cond = problem()
    G, A = device(cg)
    P = cg.PivotedCholeskyPreconditioner(G, SHIFT, RANK)
    L = P.factor.L.cpu().numpy()
    M = L @ L.T + SHIFT * np.eye(N)
    Mih = mr.sym_fun(M, lambda lam: lam ** -0.5)
    At = Mih @ Am @ Mih
    logAt = mr.sym_fun(0.5 * (At + At.T), np.log)
    sigma = float(np.sqrt(2.0 * np.sum(logAt ** 2) / 64))
    est, info = cg.logdet(A, probes=64, precond=P, generator=gen(2))
    est0, info0 = cg.logdet(A, probes=64, generator=gen(2))
    print(f"\npreconditioned: estimate {est:.6g} against {ld:.6g} (sigma {sigma:.3g}, {abs(est - ld) / sigma:.2f} sigma), stderr {info['stderr']:.3g}, "
          f"{info['iterations']} iterations ({info0['iterations']} without)")
    assert info["converged"]
    assert abs(est - ld) <= 5 * sigma
    assert sigma / 2 <= info["stderr"] <= 2 * sigma
    assert info["iterations"] < info0["iterations"]


def test_sample(cg):
    G, A = device(cg)
    P = cg.PivotedCholeskyPreconditioner(G, SHIFT, RANK)
    S = P.sample(4096, generator=gen(3))
    assert tuple(S.shape) == (N, 4096) and S.dtype == torch.float64 and S.is_cuda
    q = (S * P(S)).sum(dim=0)                                                   # z' M^-1 z ~ chi^2_n: mean n, variance 2 n
    print(f"\nsample: mean z'M^-1 z = {float(q.mean()):.4f} (n = {N}, bound {5 * np.sqrt(2 * N / 4096):.3f})")
    assert abs(float(q.mean()) - N) <= 5 * np.sqrt(2 * N / 4096)
    assert torch.equal(P.sample(4096, generator=gen(3)), S)


def test_inv_quad_logdet(cg):
    X, Am, logA, ld, Z, b, cond = problem()
    G, A = device(cg)
    calls = []
    for op in (G, A):
        def counted(y, a, *args, _orig=op.mul_, **kw):
            calls.append(tuple(a.shape))
            return _orig(y, a, *args, **kw)
        op.mul_ = counted
    reltol = 1e-8
    bt = torch.from_numpy(b).cuda()
    quad, est, x, info = cg.inv_quad_logdet(A, bt, probes=16, reltol=reltol, generator=gen(4))
    assert len(calls) == info["iterations"] and set(calls) == {(N, 17)}, calls      # ONE batched solve on [b | Z]
    exact = float(b @ np.linalg.solve(Am, b))
    print(f"\ninv_quad_logdet: b'A^-1 b = {float(quad):.12g} against {exact:.12g}; logdet {est:.6g} against {ld:.6g}, {info['iterations']} iterations")
    assert abs(float(quad) - exact) <= cond * reltol * abs(exact)
    assert np.linalg.norm(x.cpu().numpy() - np.linalg.solve(Am, b)) <= cond * reltol * np.linalg.norm(np.linalg.solve(Am, b))
    del G.mul_, A.mul_
    est1, info1 = cg.logdet(A, probes=16, reltol=reltol, generator=gen(4))
    print(f"    logdet alone with the same generator: {est1:.15g} against {est:.15g}")
    # the same probes through the same recurrences; the block product of 17 columns may round in another order than that of 16, and a
    # column may then stop an iteration apart at a residual of reltol
    assert abs(est1 - est) <= reltol * abs(est1)
    assert info["probes"] == 16 and info["values"].shape == (16,)
