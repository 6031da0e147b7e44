"""mbcg on the device: accuracy against numpy's solve of the oracle's matrix, per-column stopping, the dispatch from cg, the
preconditioned solve, fp32, a GradientKernel block Gramian, and the Lanczos logs (quadrature and the CG identity).

Case A: EQ(l = 0.5), d = 2, n = 257, + 0.1 I (cond ~ 4e2);  case B: EQ(l = 0.7), d = 3, n = 515, + 0.05 I (cond ~ 1.4e3); N(0, I) points.
Right-hand sides: [random, random, a zero column, a copy of column 0, A·1]."""
import functools

import numpy as np
import pytest
import torch

import covgram_oracle as o
import mbcg_ref as mr

pytestmark = pytest.mark.gpu

CASES = {"A": (0.5, 2, 257, 0.1, 0), "B": (0.7, 3, 515, 0.05, 1)}
RELTOL = 1e-10


@functools.lru_cache(maxsize=None)
def problem(case):
    l, d, n, shift, seed = CASES[case]
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    G = o.matrix(o.Kernel(o.EQ, lengthscale=l), X)
    A = G + shift * np.eye(n)
    B = rng.standard_normal((n, 5))
    B[:, 2] = 0.0
    B[:, 3] = B[:, 0]
    B[:, 4] = A @ np.ones(n)
    Xs = np.linalg.solve(A, B)
    Z = rng.choice([-1.0, 1.0], size=(n, 5))
    g1, g2 = rng.standard_normal((32, 5)), rng.standard_normal((n, 5))
    return X, G, A, B, Xs, float(np.linalg.cond(A)), Z, g1, g2


def device(cg, case, dtype=torch.float64):
    l, d, n, shift, _ = CASES[case]
    Xt = torch.from_numpy(problem(case)[0]).to(dtype).cuda()
    G = cg.gramian(cg.Lengthscale(cg.EQ(), l), Xt)
    return G, G + torch.full((n,), shift, dtype=dtype, device="cuda")


def colrel(X, ref):
    return np.linalg.norm(X - ref, axis=0) / np.maximum(np.linalg.norm(ref, axis=0), 1e-300)


@pytest.mark.parametrize("case", list(CASES))
def test_solve(cg, case):
    X, Gm, Am, B, Xs, cond, *_ = problem(case)
    G, A = device(cg, case)
    Bt = torch.from_numpy(B).cuda()
    Xd, info = cg.mbcg(A, Bt, reltol=RELTOL)
    Xn = Xd.cpu().numpy()
    live = [0, 1, 3, 4]
    err = colrel(Xn[:, live], Xs[:, live])
    res = np.linalg.norm(B - Am @ Xn, axis=0)[live] / np.linalg.norm(B, axis=0)[live]
    print(f"\ncase {case}: cond {cond:.3g}, iterations {info['iterations']} {info['column_iterations']}, error {err.max():.3g}, residual {res.max():.3g}")
    assert info["converged"] and all(info["column_converged"])
    assert (err <= cond * RELTOL).all() and (res <= 2 * RELTOL).all()
    its = info["column_iterations"]
    assert its[2] == 0 and not Xn[:, 2].any()                                   # the zero column
    assert its[3] == its[0] and np.array_equal(Xn[:, 3], Xn[:, 0])                # the copy: the same bits
    assert all(0 < its[j] <= info["iterations"] for j in live) and max(its) <= info["iterations"]
    assert tuple(Xd.shape) == tuple(Bt.shape) and len(info["residual_norm"]) == 5
    # the other ways in
    X2, info2 = cg.cg(A, Bt, reltol=RELTOL)
    assert torch.equal(X2, Xd) and info2["column_iterations"] == its
    x1, _ = cg.cg(A, Bt[:, 0].contiguous(), reltol=RELTOL)
    assert colrel(x1.cpu().numpy()[:, None], Xn[:, :1])[0] <= 2 * cond * RELTOL
    with pytest.raises(ValueError, match="graph"):
        cg.cg(A, Bt, graph=True)
    with pytest.raises(cg.DimensionMismatch):
        cg.mbcg(A, Bt[:-1])
    with pytest.raises(cg.DimensionMismatch):
        cg.mbcg(A, Bt, x0=Bt[:, :2])
    if case == "A":                                                             # a start vector, once
        x0 = Xs + 1e-3 * np.random.default_rng(5).standard_normal(Xs.shape)
        X3, info3 = cg.mbcg(A, Bt, x0=torch.from_numpy(x0).cuda(), reltol=1e-6, check_every=1)
        r0 = np.linalg.norm(B - Am @ x0, axis=0)                               # the tolerance is relative to the START residual
        r3 = np.linalg.norm(B - Am @ X3.cpu().numpy(), axis=0)
        assert info3["converged"] and (r3 <= 2e-6 * r0).all(), r3 / r0
        assert info3["iterations"] < info["iterations"]


def test_preconditioned(cg):
    X, Gm, Am, B, Xs, cond, *_ = problem("A")
    G, A = device(cg, "A")
    Bt = torch.from_numpy(B).cuda()
    P = cg.PivotedCholeskyPreconditioner(G, 0.1, 32)
    X0, info0 = cg.mbcg(A, Bt, reltol=RELTOL)
    X1, info1 = cg.mbcg(A, Bt, reltol=RELTOL, precond=P)
    live = [0, 1, 3, 4]
    err = colrel(X1.cpu().numpy()[:, live], Xs[:, live])
    res = np.linalg.norm(B - Am @ X1.cpu().numpy(), axis=0)[live] / np.linalg.norm(B, axis=0)[live]
    print(f"\n{info0['iterations']} iterations plain, {info1['iterations']} preconditioned; error {err.max():.3g}, residual {res.max():.3g}")
    assert info1["converged"] and (err <= cond * RELTOL).all() and (res <= 2 * RELTOL).all()
    assert info1["iterations"] < info0["iterations"]
    assert info1["column_iterations"][2] == 0 and not X1[:, 2].any()
    assert torch.equal(X1[:, 3], X1[:, 0])


def test_fp32(cg):
    X, Gm, Am, B, Xs, cond, *_ = problem("A")
    G, A = device(cg, "A", torch.float32)
    B32 = B.astype(np.float32)
    Xd, info = cg.mbcg(A, torch.from_numpy(B32).cuda(), reltol=1e-4)
    assert Xd.dtype == torch.float32 and info["converged"]
    live = [0, 1, 3, 4]
    B8 = B32.astype(np.float64)
    res = np.linalg.norm(B8 - Am @ Xd.cpu().numpy().astype(np.float64), axis=0)[live] / np.linalg.norm(B8, axis=0)[live]
    print(f"\nfp32: {info['iterations']} iterations, true residual {res.max():.3g}")
    assert (res <= 2e-4).all()


def test_gradient_kernel(cg):
    """The block Gramian of GradientKernel(EQ) + 0.1 I, three right-hand sides, against the dense solve of the oracle's block matrix (what the
    reference's `G \\ b` converges to, column by column)."""
    n, d = 64, 2
    rng = np.random.default_rng(11)
    X = rng.standard_normal((n, d))
    Am = o.grad_matrix(o.Kernel(o.EQ), X) + 0.1 * np.eye(n * d)
    B = rng.standard_normal((n * d, 3))
    Xs = np.linalg.solve(Am, B)
    cond = float(np.linalg.cond(Am))
    K = cg.gramian(cg.GradientKernel(cg.EQ()), torch.from_numpy(X).cuda())
    A = K + torch.full((n * d,), 0.1, dtype=torch.float64, device="cuda")
    Xd, info = cg.mbcg(A, torch.from_numpy(B).cuda(), reltol=RELTOL)
    Xn = Xd.cpu().numpy()
    err = colrel(Xn, Xs)
    res = np.linalg.norm(B - Am @ Xn, axis=0) / np.linalg.norm(B, axis=0)
    print(f"\ngradient kernel: cond {cond:.3g}, {info['iterations']} iterations, error {err.max():.3g}, residual {res.max():.3g}")
    assert info["converged"] and (err <= cond * RELTOL).all() and (res <= 2 * RELTOL).all()


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "preconditioned"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_lanczos_logs(cg, dtype, pre):
    """The device's own coefficient logs: the quadrature e1' log(T) e1 against numpy's exact value within 10x the restatement's error in
    the same dtype, and the CG identity b'x = rz0 e1' T^-1 e1 within 10x the restatement's own discrepancy."""
    X, Gm, Am, B, Xs, cond, Z, g1, g2 = problem("A")
    n = Am.shape[0]
    npdt = np.float32 if dtype == torch.float32 else np.float64
    G, A = device(cg, "A", dtype)
    if pre:
        P = cg.PivotedCholeskyPreconditioner(G, 0.1, 32)
        L = P.factor.L.cpu().numpy().astype(np.float64)
        M = L @ L.T + 0.1 * np.eye(n)
        Minv = np.linalg.inv(M)
        Zp = (L @ g1 + np.sqrt(0.1) * g2).astype(npdt)
        Mih = mr.sym_fun(M, lambda lam: lam ** -0.5)
        At = Mih @ Am @ Mih
        logm = mr.sym_fun(0.5 * (At + At.T), np.log)
        W = Mih @ Zp.astype(np.float64)
        iters = 40
    else:
        P, Minv, Zp, logm, W, iters = None, None, Z.astype(npdt), mr.sym_fun(Am, np.log), Z, 80
    exact = np.einsum("ij,ik,kj->j", W, logm, W)
    Xr, ref = mr.mbcg(Am, Zp, Minv=Minv, maxiter=iters, reltol=0.0, dtype=npdt)
    Xd, info = cg.mbcg(A, torch.from_numpy(Zp).cuda(), reltol=0.0, maxiter=iters, precond=P, lanczos=True)
    assert info["iterations"] == iters and info["column_iterations"] == [iters] * 5
    assert tuple(info["alpha"].shape) == (iters, 5) and info["alpha"].dtype == torch.float64
    Z8 = Zp.astype(np.float64)
    q_ref = np.array([ref["rz0"][j] * mr.quadrature(mr.tridiagonal(ref["alpha"][:, j], ref["beta"][:, j], iters), np.log) for j in range(5)])
    q_dev = np.array([float(info["rz0"][j]) * cg.lanczos_quadrature(info["tridiagonals"][j], torch.log) for j in range(5)])
    e_ref = float(np.max(np.abs(q_ref - exact) / np.abs(exact)))
    e_dev = np.abs(q_dev - exact) / np.abs(exact)
    inv = lambda lam: 1.0 / lam
    i_ref = np.array([ref["rz0"][j] * mr.quadrature(mr.tridiagonal(ref["alpha"][:, j], ref["beta"][:, j], iters), inv) for j in range(5)])
    i_dev = np.array([float(info["rz0"][j]) * cg.lanczos_quadrature(info["tridiagonals"][j], inv) for j in range(5)])
    bx_ref = np.einsum("ij,ij->j", Z8, Xr.astype(np.float64))
    bx_dev = np.einsum("ij,ij->j", Z8, Xd.cpu().numpy().astype(np.float64))
    d_ref = float(np.max(np.abs(i_ref - bx_ref) / np.abs(bx_ref)))
    d_dev = np.abs(i_dev - bx_dev) / np.abs(bx_dev)
    print(f"\n{dtype} pre={pre}: quadrature error device {e_dev.max():.3g}, restatement {e_ref:.3g}; CG identity device {d_dev.max():.3g}, restatement {d_ref:.3g}")
    assert (e_dev <= 10 * e_ref).all()
    assert (d_dev <= 10 * d_ref).all()
