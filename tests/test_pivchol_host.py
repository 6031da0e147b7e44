"""CPU tier of the device pivoted Cholesky and its preconditioner: the entry point is declared, exported and refuses bad arguments
before any device call; the host-side kernel check; the numpy restatements the GPU tests lean on (tests/pivchol_ref.py) against the
oracle and against numpy's dense solve."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import covgram_oracle as o
import pivchol_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_and_exported(cg):
    header = open(os.path.join(ROOT, "include", "covgram.h")).read()
    assert re.search(r"\bint\s+covgram_pivoted_cholesky\s*\(", header)
    cap = int(re.search(r"#define COVGRAM_PIVCHOL_MAX_RANK (\d+)", header).group(1))
    assert cap == 1024 == cg._ffi.PIVCHOL_MAX_RANK
    assert "covgram_pivoted_cholesky" in cg._ffi.PROTOTYPES
    lib = cg._ffi.lib()
    assert hasattr(lib, "covgram_pivoted_cholesky")
    jl = open(os.path.join(ROOT, "covariancefunctions.jl_amd", "julia", "CovGram.jl")).read()
    assert ":covgram_pivoted_cholesky" in jl and re.search(r"const PIVCHOL_MAX_RANK = %d\b" % cap, jl)
    for name in ("pivoted_cholesky", "PivotedCholeskyPreconditioner", "preconditioner", "require_pivchol_spec"):
        assert hasattr(cg, name), name


def _call(cg, spec, max_rank, tol, ctx=None):
    f = cg._ffi
    rc = f.lib().covgram_pivoted_cholesky(ctx, f.kref(spec), None, max_rank, tol, None, 1, None, None, None)
    return rc, f.lib().covgram_last_error().decode()


def test_argument_errors_need_no_device(cg):
    f = cg._ffi
    spec = cg.require_pivchol_spec(cg.MaternP(2))
    rc, msg = _call(cg, spec, 4, 0.0)                       # NULL ctx
    assert rc == f.EINVAL and "NULL" in msg, (rc, msg)
    rc, msg = _call(cg, spec, 4, -1e-3)
    assert rc == f.EINVAL and "tol" in msg, (rc, msg)
    rc, msg = _call(cg, spec, 4, float("nan"))
    assert rc == f.EINVAL and "tol" in msg, (rc, msg)
    rc, msg = _call(cg, spec, 1025, 0.0)
    assert rc == f.EUNSUPPORTED and "COVGRAM_PIVCHOL_MAX_RANK" in msg and "1025" in msg, (rc, msg)
    rc, msg = _call(cg, spec, -1, 0.0)
    assert rc == f.EINVAL and "max_rank" in msg, (rc, msg)
    rc, msg = _call(cg, cg.device_spec(cg.Dot()), 4, 0.0)
    assert rc == f.EUNSUPPORTED and "Dot" in msg, (rc, msg)
    rc, msg = _call(cg, cg.device_spec(cg.EQ() + cg.MaternP(1)), 4, 0.0)
    assert rc == f.EUNSUPPORTED and "Sum" in msg, (rc, msg)
    with pytest.raises(cg.UnsupportedKernel):
        f.check(rc)


def test_require_pivchol_spec(cg):
    f = cg._ffi
    s = cg.require_pivchol_spec(2 * cg.Lengthscale(cg.MaternP(2), 0.7))
    assert isinstance(s, f.covgram_kernel)
    assert (s.family, s.p, s.trait, s.power) == (f.MATERNP, 2, f.ISOTROPIC, 1) and s.scale == 2.0 and s.lengthscale == 0.7
    assert cg.require_pivchol_spec(cg.Matern(0.8)).family == f.MATERN
    assert cg.require_pivchol_spec(cg.EQ() ** 2).power == 2
    for bad in (cg.Dot(), cg.EQ() + cg.MaternP(1)):
        with pytest.raises(cg.UnsupportedKernel) as e:
            cg.require_pivchol_spec(bad)
        assert f"pivoted_cholesky({type(bad).__name__})" in str(e.value)
        assert isinstance(e.value, NotImplementedError)


def test_replay_reproduces_the_oracle():
    """replay() along the oracle's own pivots is the oracle's factor (1e-8: the tolerance of the pivoted factor in test_gpu_parity.py);
    every step is greedy, and the residual diagonal is diag(M - L L')."""
    rng = np.random.default_rng(300)
    X = rng.standard_normal((300, 2))
    M = o.matrix(o.Kernel(o.EQ), X)
    L, piv, rank = o.pivoted_cholesky(M, tol=1e-6)
    assert 0 < rank < 300
    Lr, gaps, dres = pr.replay(M, piv[:rank])
    assert Lr.shape == L.shape
    assert np.abs(Lr - L).max() <= 1e-8
    assert np.all(gaps == 0.0)
    resid = np.diag(M - Lr @ Lr.T).copy()
    resid[piv[:rank]] = 0.0
    assert np.abs(dres - resid).max() <= 1e-12 and dres.max() <= 1e-6
    assert np.all(dres[piv[:rank]] == 0.0)
    # the float32 emulation follows the same recurrence: it differs from the fp64 factor by rounding only
    Le, de = pr.emulate(M, piv[:16], np.float32)
    assert Le.dtype == np.float32 and np.abs(Le - Lr[:, :16]).max() <= 1e-4
    Ld, dd = pr.emulate(M, piv[:rank], np.float64)
    assert np.abs(Ld - Lr).max() <= 1e-8


def test_woodbury_and_logdet_identities():
    """(L L' + D)^-1 r = D^-1 r - W (W' r) and log det(L L' + D) = log det C + sum log D_i in numpy fp64, to 1e-9 relative."""
    rng = np.random.default_rng(200)
    n = 200
    X = rng.standard_normal((n, 3))
    M = o.matrix(o.Kernel(o.MATERNP, p=2), X)
    L, piv, rank = o.pivoted_cholesky(M, max_rank=32)
    assert rank == 32
    r = rng.standard_normal(n)
    for D in (np.full(n, 1e-2), 1e-2 * rng.uniform(0.5, 2.0, n)):
        Dinv, W, R = pr.woodbury(L, D)
        A = L @ L.T + np.diag(D)
        ref = np.linalg.solve(A, r)
        got = Dinv * r - W @ (W.T @ r)
        assert np.linalg.norm(got - ref) <= 1e-9 * np.linalg.norm(ref)
        sign, ld = np.linalg.slogdet(A)
        assert sign == 1.0
        got_ld = 2.0 * np.log(np.diag(R)).sum() + np.log(D).sum()
        assert abs(got_ld - ld) <= 1e-9 * abs(ld)
