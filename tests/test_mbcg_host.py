"""CPU tier of the batched CG / stochastic Lanczos quadrature feature: the host functions `cg_tridiagonals` and `lanczos_quadrature`
on the coefficients of the numpy restatement (tests/mbcg_ref.py), the preconditioned identity the log-determinant estimate rests on, and
the new C ABI entry points in the header and the ctypes mirror.

Problem: EQ(l = 0.5), d = 2, n = 257, N(0, I) points (seed 0), A = G + 0.1 I (cond ~ 4e2)."""
import functools
import os
import re

import numpy as np
import torch

import covgram_oracle as o
import mbcg_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SHIFT = 257, 0.1


@functools.lru_cache(maxsize=None)
def problem():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((N, 2))
    G = o.matrix(o.Kernel(o.EQ, lengthscale=0.5), X)
    A = G + SHIFT * np.eye(N)
    Z = rng.choice([-1.0, 1.0], size=(N, 5))
    g1, g2 = rng.standard_normal((32, 5)), rng.standard_normal((N, 5))
    return X, G, A, Z, g1, g2


def test_tridiagonals_and_quadrature_unpreconditioned(cg):
    X, G, A, Z, _, _ = problem()
    _, info = mr.mbcg(A, Z, maxiter=80, reltol=0.0)
    assert (info["iters"] == 80).all()
    Ts = cg.cg_tridiagonals(torch.from_numpy(info["alpha"]), torch.from_numpy(info["beta"]), torch.from_numpy(info["iters"]))
    logA = mr.sym_fun(A, np.log)
    for j in range(Z.shape[1]):
        assert tuple(Ts[j].shape) == (80, 80) and Ts[j].dtype == torch.float64
        assert np.allclose(Ts[j].numpy(), mr.tridiagonal(info["alpha"][:, j], info["beta"][:, j], 80), rtol=1e-15, atol=0)
        got = N * cg.lanczos_quadrature(Ts[j], torch.log)
        exact = Z[:, j] @ logA @ Z[:, j]
        err = abs(got - exact) / abs(exact)
        print(f"probe {j}: quadrature {got:.12g}, exact {exact:.12g}, rel {err:.3g}")
        assert err <= 1e-12
    # truncation per column, and at a frozen (alpha = 0) row
    it = torch.tensor([80, 3, 0, 80, 80])
    al = torch.from_numpy(info["alpha"]).clone()
    al[10:, 3] = 0.0
    Tt = cg.cg_tridiagonals(al, torch.from_numpy(info["beta"]), it)
    assert [t.shape[0] for t in Tt] == [80, 3, 0, 10, 80]
    assert torch.equal(Tt[1], Ts[1][:3, :3]) and torch.equal(Tt[3], Ts[3][:10, :10])
    assert cg.lanczos_quadrature(Tt[2], torch.log) == 0.0


def test_preconditioned_identity(cg):
    X, G, A, _, g1, g2 = problem()
    L, piv, rank = o.pivoted_cholesky(G, max_rank=32)
    assert rank == 32
    M = L @ L.T + SHIFT * np.eye(N)
    Zp = L @ g1 + np.sqrt(SHIFT) * g2                        # ~ N(0, M)
    Minv = np.linalg.inv(M)
    _, info = mr.mbcg(A, Zp, Minv=Minv, maxiter=40, reltol=0.0)
    Ts = cg.cg_tridiagonals(info["alpha"], info["beta"], info["iters"])
    Mih = mr.sym_fun(M, lambda lam: lam ** -0.5)
    At = Mih @ A @ Mih
    At = 0.5 * (At + At.T)
    logAt = mr.sym_fun(At, np.log)
    for j in range(Zp.shape[1]):
        w = Mih @ Zp[:, j]
        rz0 = Zp[:, j] @ Minv @ Zp[:, j]
        assert abs(info["rz0"][j] - rz0) <= 1e-12 * rz0
        got = info["rz0"][j] * cg.lanczos_quadrature(Ts[j], torch.log)
        exact = w @ logAt @ w
        print(f"probe {j}: {got:.12g} against {exact:.12g}: {abs(got - exact) / N:.3g} n")
        assert abs(got - exact) <= 1e-11 * N
    ldM, ldA = np.linalg.slogdet(M)[1], np.linalg.slogdet(A)[1]
    assert abs(ldM + np.trace(logAt) - ldA) <= 1e-10 * abs(ldA)


def test_abi_declares_the_batched_step(cg):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "covgram.h")).read(), flags=re.S)
    for name in ("covgram_bcg_init", "covgram_bcg_step", "covgram_bcg_update", "covgram_bcg_direction"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/covgram.h"
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in cg._ffi.PROTOTYPES, name
        assert len(cg._ffi.PROTOTYPES[name][1]) == nargs, (name, nargs)
    f = cg._ffi
    for macro, val in (("COVGRAM_BCG_SLAB", f.BCG_SLAB), ("COVGRAM_BCG_FIELDS", f.BCG_FIELDS), ("COVGRAM_BCG_RZ", f.BCG_RZ),
                       ("COVGRAM_BCG_TOL2", f.BCG_TOL2), ("COVGRAM_BCG_RR", f.BCG_RR), ("COVGRAM_BCG_ACTIVE", f.BCG_ACTIVE),
                       ("COVGRAM_BCG_ITERS", f.BCG_ITERS)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(val) + r"\b", header), macro
    assert re.search(r"#define COVGRAM_VERSION 113\b", header)
    for name in ("mbcg", "cg_tridiagonals", "lanczos_quadrature", "logdet", "inv_quad_logdet"):
        assert callable(getattr(cg, name))
    assert callable(cg.PivotedCholeskyPreconditioner.sample)
