"""PivotedCholeskyPreconditioner on the device: (L L' + D)^-1 through covgram_lowrank_mvm, its log-determinant, and what it does to CG.

Cases: MaternP(2), n = 1031, d = 3 and EQ(l = 0.3), n = 1031, d = 2, N(0, I) points, fp64; D once the float 1e-2 and once a 1-D tensor
drawn from [0.5, 2] * 1e-2; rank 64.  The reference of apply and logdet is numpy's dense solve / slogdet of L L' + D with the DEVICE's
own L (1e-9 relative; the numpy restatement of the W form, tests/test_pivchol_host.py, is at 4e-10 absolute at n = 2000).  CG on G + D
must converge to numpy's solution of the oracle's matrix (1e-7, the tolerance of the existing CG tests) in at most 0.75 of the
unpreconditioned iterations (the numpy restatement of these four solves: 0.32 to 0.59)."""
import functools

import numpy as np
import pytest
import torch

import covgram_oracle as o

pytestmark = pytest.mark.gpu

N, RANK = 1031, 64
KERNELS = {
    "MaternP(2)": (lambda cg: cg.MaternP(2), o.Kernel(o.MATERNP, p=2), 3),
    "EQ(l=0.3)": (lambda cg: cg.Lengthscale(cg.EQ(), 0.3), o.Kernel(o.EQ, lengthscale=0.3), 2),
}
DIAGS = ["float", "tensor"]


@functools.lru_cache(maxsize=None)
def problem(kname):
    """(X, M, b, {diag kind: D vector}) on the host, computed once per kernel."""
    d = KERNELS[kname][2]
    rng = np.random.default_rng(9000 + N + d)
    X = rng.standard_normal((N, d))
    M = o.matrix(KERNELS[kname][1], X)
    b = rng.standard_normal(N)
    D = {"float": np.full(N, 1e-2), "tensor": 1e-2 * rng.uniform(0.5, 2.0, N)}
    return X, M, b, D


def build(cg, kname, kind, dtype=torch.float64):
    X, M, b, D = problem(kname)
    Xt = torch.from_numpy(X).to(dtype).cuda()
    G = cg.gramian(KERNELS[kname][0](cg), Xt)
    Dt = torch.from_numpy(D[kind]).to(dtype).cuda()
    P = cg.PivotedCholeskyPreconditioner(G, 1e-2 if kind == "float" else Dt, RANK)
    return G, Dt, P


def rel(a, ref):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("kind", DIAGS)
@pytest.mark.parametrize("kname", list(KERNELS))
def test_apply_and_logdet(cg, kname, kind):
    X, M, b, D = problem(kname)
    G, Dt, P = build(cg, kname, kind)
    assert P.rank == RANK and tuple(P.shape) == (N, N)
    L = P.factor.L.cpu().numpy()
    A = L @ L.T + np.diag(D[kind])
    r = torch.from_numpy(b).cuda()
    r_before = r.clone()
    y = P(r)
    assert y.data_ptr() != r.data_ptr() and torch.equal(r, r_before)          # a fresh tensor; r is not written
    e = rel(y.cpu().numpy(), np.linalg.solve(A, b))
    sign, ld = np.linalg.slogdet(A)
    e_ld = abs(float(P.logdet()) - ld) / abs(ld)
    print(f"\n{kname} D={kind}: apply {e:.3g}, logdet {e_ld:.3g}")
    assert e <= 1e-9
    assert sign == 1.0 and e_ld <= 1e-9
    # the operator surface: to_dense is the dense inverse, mul_ the 5-argument product, a matrix right-hand side goes column by column
    Minv = P.to_dense().cpu().numpy()
    assert rel(Minv @ b, np.linalg.solve(A, b)) <= 1e-9
    B = torch.from_numpy(np.stack([b, b[::-1].copy(), np.ones(N)], axis=1)).cuda()
    assert rel(P(B).cpu().numpy(), np.linalg.solve(A, B.cpu().numpy())) <= 1e-9
    y0 = torch.ones(N, dtype=torch.float64, device="cuda")
    P.mul_(y0, r, 2.0, -0.5)
    assert rel(y0.cpu().numpy(), 2.0 * np.linalg.solve(A, b) - 0.5) <= 1e-9


def test_apply_fp32(cg):
    kname = "MaternP(2)"
    X, M, b, D = problem(kname)
    G, Dt, P = build(cg, kname, "tensor", torch.float32)
    assert P.dtype == torch.float32 and P.rank == RANK
    L = P.factor.L.cpu().numpy().astype(np.float64)
    A = L @ L.T + np.diag(Dt.cpu().numpy().astype(np.float64))
    r32 = b.astype(np.float32)
    y = P(torch.from_numpy(r32).cuda())
    assert y.dtype == torch.float32
    e = rel(y.cpu().numpy(), np.linalg.solve(A, r32.astype(np.float64)))
    lim = 64.0 * np.sqrt(N) * float(np.finfo(np.float32).eps)
    print(f"\nfp32 apply: {e:.3g} against {lim:.3g}")
    assert e <= lim


@pytest.mark.parametrize("kind", DIAGS)
@pytest.mark.parametrize("kname", list(KERNELS))
def test_cg(cg, kname, kind):
    X, M, b, D = problem(kname)
    G, Dt, P = build(cg, kname, kind)
    xs = np.linalg.solve(M + np.diag(D[kind]), b)
    bt = torch.from_numpy(b).cuda()
    A = G + Dt
    x0, info0 = cg.cg(A, bt, reltol=1e-8, maxiter=4 * N)
    x1, info1 = cg.cg(A, bt, reltol=1e-8, maxiter=4 * N, precond=P)
    e0, e1 = rel(x0.cpu().numpy(), xs), rel(x1.cpu().numpy(), xs)
    print(f"\n{kname} D={kind}: {info0['iterations']} iterations plain ({e0:.3g}), {info1['iterations']} preconditioned ({e1:.3g}), "
          f"ratio {info1['iterations'] / info0['iterations']:.3f}")
    assert info0["converged"] and info1["converged"], (info0, info1)
    assert e1 <= 1e-7
    assert info1["iterations"] <= 0.75 * info0["iterations"]
    # the same solve with the iteration body replayed as a graph
    x2, info2 = cg.cg(A, bt, reltol=1e-8, maxiter=4 * N, precond=P, graph=True, check_every=4)
    e2 = rel(x2.cpu().numpy(), xs)
    print(f"    graph: {info2['iterations']} iterations ({e2:.3g})")
    assert info2.get("graph") is True and info2["converged"], info2
    assert e2 <= 1e-7


def test_convenience(cg):
    kname = "MaternP(2)"
    X, M, b, D = problem(kname)
    G, Dt, P = build(cg, kname, "tensor")
    Q = cg.preconditioner(G + Dt, rank=RANK)
    assert isinstance(Q, cg.PivotedCholeskyPreconditioner) and Q.rank == P.rank
    r = torch.from_numpy(b).cuda()
    assert torch.equal(Q(r), P(r))
    with pytest.raises(cg.UnsupportedKernel):
        cg.preconditioner(G, rank=RANK)
    U = torch.ones((N, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(cg.UnsupportedKernel):
        cg.preconditioner(cg.LazyMatrixProduct(U, U) + Dt, rank=RANK)          # a diagonal, but not on a Gramian
    with pytest.raises(ValueError):
        cg.PivotedCholeskyPreconditioner(G, -1.0, RANK)
    with pytest.raises(cg.DimensionMismatch):
        cg.PivotedCholeskyPreconditioner(G, Dt[:-1], RANK)
    # a rank above n is the full factor's
    Xs = torch.from_numpy(X[:40]).cuda()
    Ps = cg.PivotedCholeskyPreconditioner(cg.gramian(cg.MaternP(2), Xs), 1e-2, RANK)
    assert Ps.rank == 40
