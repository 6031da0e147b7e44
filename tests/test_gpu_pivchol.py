"""covgram_pivoted_cholesky on the device (csrc/pivchol.hip) and the Python pivoted_cholesky on top of it.

Points are N(0, I) with fixed seeds (fp32 cases: rounded to fp32 first, so the oracle sees the device's points).  With M the oracle's
fp64 matrix and piv the DEVICE's pivots, tests/pivchol_ref.py gives replay(M, piv) — the fp64 factor along those pivots, with every
step's greedy gap — and emulate(M, piv, float32), the recurrence carried in fp32.  Checked per case:
  1. structure: rank, pivots distinct and in range, piv a permutation, dres exactly zero on the pivots;
  2. greedy pivots: every step's gap <= 8 (k + 2) eps max diag(M) — each residual-diagonal entry is the result of k + 1 rounded
     operations on values bounded by the diagonal; fp64: the pivots ARE oracle.pivoted_cholesky's (fp32 may break the near-ties
     of a constant diagonal differently, on purpose not asked);
  3. factor: max|L - replay.L| <= 1e-8 in fp64 (the project's tolerance for this factor, test_gpu_parity.py); in fp32
     8 max|emulate.L - replay.L| (floor 16 eps32): the 8 covers the device's own kernel evaluation against numpy's rounded fp64 entries;
  4. identities that hold for any pivot order, within lim4 = (limit of 3) * 2 sqrt(rank) max|L|: (L L')[P, P] = M[P, P],
     dres = diag(M - L L'), max|M - L L'| <= max dres + lim4 (the residual is positive semidefinite).
Shapes: n = 1 (degenerate), 63 (full rank, less than a wave), 257 (one lane past a workgroup), 1031 (prime, several workgroups), and
n = 1024 * 256 + 1, one row more than one pass of the capped grid covers (columns for the four pivots only, no n x n matrix)."""
import functools

import numpy as np
import pytest
import torch

import covgram_oracle as o
import pivchol_ref as pr

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TDT = {F32: torch.float32, F64: torch.float64}
EPS = {F32: float(np.finfo(np.float32).eps), F64: float(np.finfo(np.float64).eps)}
SENTINEL = -12345.0

SHAPES = [(1, 2, 1), (63, 2, 63), (257, 2, 64), (1031, 3, 64)]
KERNELS = {
    "EQ(l=0.5)": (lambda cg: cg.Lengthscale(cg.EQ(), 0.5), o.Kernel(o.EQ, lengthscale=0.5)),
    "MaternP(2)": (lambda cg: cg.MaternP(2), o.Kernel(o.MATERNP, p=2)),
    "Exponential": (lambda cg: cg.Exp(), o.Kernel(o.EXP)),
    "2*Lengthscale(RQ(1.5),0.7)": (lambda cg: 2 * cg.Lengthscale(cg.RQ(1.5), 0.7), o.Kernel(o.RQ, param=1.5, lengthscale=0.7, scale=2.0)),
    "Matern(0.8)": (lambda cg: cg.Matern(0.8), o.Kernel(o.MATERN, param=0.8)),
}
CASES = [(kn, n, d, r) for kn in list(KERNELS)[:4] for (n, d, r) in SHAPES] + [("Matern(0.8)", 257, 2, 64)]


@functools.lru_cache(maxsize=None)
def points(n, d, dt):
    rng = np.random.default_rng(7000 + 13 * n + d)
    return np.ascontiguousarray(rng.standard_normal((n, d)).astype(dt))


@functools.lru_cache(maxsize=None)
def matrix(kname, n, d, dt):
    M = o.matrix(KERNELS[kname][1], points(n, d, dt).astype(F64))
    M.setflags(write=False)
    return M


def raw_call(cg, k, X, max_rank, tol):
    """covgram_pivoted_cholesky through the C ABI with pre-filled outputs -> (L n x max_rank, piv, dres, rank) on the host."""
    f = cg._ffi
    Xt = torch.from_numpy(X).cuda()
    G = cg.Gramian(k, Xt)
    n = X.shape[0]
    Lcm = torch.full((max_rank, n), SENTINEL, dtype=Xt.dtype, device=Xt.device)
    piv = torch.full((max_rank,), -1, dtype=torch.int32, device=Xt.device)
    dres = torch.full((n,), SENTINEL, dtype=Xt.dtype, device=Xt.device)
    rk = torch.full((1,), -7, dtype=torch.int32, device=Xt.device)
    P = f._P
    f.check(f.lib().covgram_pivoted_cholesky(G._px.ctx.bind_stream(), f.kref(cg.require_pivchol_spec(k)), G._px.handle, max_rank, float(tol),
                                             P(Lcm.data_ptr()), n, P(piv.data_ptr()), P(dres.data_ptr()), P(rk.data_ptr())))
    return Lcm.t().cpu().numpy(), piv.cpu().numpy(), dres.cpu().numpy(), int(rk)


def check_structure(n, max_rank, L, piv, dres, rank):
    assert 0 <= rank <= max_rank
    head = piv[:rank]
    assert np.all((head >= 0) & (head < n)) and len(set(head.tolist())) == rank
    assert np.all(piv[rank:] == -1)                             # untouched
    assert np.all(L[:, rank:] == SENTINEL)                      # untouched
    assert np.all(dres[head] == 0.0)
    assert not np.isnan(L[:, :rank]).any() and not np.isnan(dres).any()


def factor_limit(dt, ref, emu_L):
    if dt == F64:
        return 1e-8
    return max(8.0 * float(np.abs(emu_L.astype(F64) - ref).max()), 16.0 * EPS[F32])


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kname,n,d,max_rank", CASES, ids=[f"{c[0]}-n{c[1]}" for c in CASES])
def test_factor(cg, kname, n, d, max_rank, dt):
    X = points(n, d, dt)
    M = matrix(kname, n, d, dt)
    L, piv, dres, rank = raw_call(cg, KERNELS[kname][0](cg), X, max_rank, 0.0)
    # 1. structure
    check_structure(n, max_rank, L, piv, dres, rank)
    assert rank >= 1
    head = piv[:rank].astype(np.int64)
    Ld = L[:, :rank].astype(F64)
    ref, gaps, dref = pr.replay(M, head)
    # 2. greedy pivots
    dmax = float(np.diag(M).max())
    bound = 8.0 * (np.arange(rank) + 2) * EPS[dt] * dmax
    print(f"\n{kname} n={n} {dt.__name__}: rank {rank}, worst gap / bound {float((gaps / bound).max()):.3g}")
    assert np.all(gaps <= bound), (gaps / bound).max()
    if dt == F64:
        Lo, pivo, ranko = o.pivoted_cholesky(M, 0.0, max_rank)
        assert rank == ranko and np.array_equal(head, pivo[:ranko])
    # 3. factor
    emu = pr.emulate(M, head, F32)[0] if dt == F32 else None
    lim = factor_limit(dt, ref, emu)
    err = float(np.abs(Ld - ref).max())
    print(f"    max|L - replay| {err:.3g}, limit {lim:.3g}")
    assert np.isfinite(lim) and err <= lim
    # 4. identities
    lim4 = lim * 2.0 * np.sqrt(rank) * float(np.abs(Ld).max())
    LLt = Ld @ Ld.T
    ix = np.ix_(head, head)
    e_pp = float(np.abs(LLt[ix] - M[ix]).max())
    e_d = float(np.abs(dres.astype(F64) - np.diag(M - LLt)).max())
    e_m = float(np.abs(M - LLt).max())
    print(f"    pivot block {e_pp:.3g}, dres {e_d:.3g} (limit {lim4:.3g}); max|M - LL'| {e_m:.3g} against max dres {float(dres.max()):.3g}")
    assert e_pp <= lim4
    assert e_d <= lim4
    assert e_m <= float(dres.max()) + lim4


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_rows_beyond_one_pass_of_the_grid(cg, dt):
    """n = 1024 workgroups x 256 rows + 1: workgroup 0 walks a second row block.  The reference is the recurrence on the four pivot
    columns, evaluated in numpy — no n x n matrix."""
    n, d, max_rank = 1024 * 256 + 1, 2, 4
    X = points(n, d, dt)
    ko = KERNELS["MaternP(2)"][1]
    L, piv, dres, rank = raw_call(cg, KERNELS["MaternP(2)"][0](cg), X, max_rank, 0.0)
    check_structure(n, max_rank, L, piv, dres, rank)
    assert rank == max_rank and piv[0] == 0                    # the constant diagonal: an n-way tie that goes to the smallest index
    head = piv.astype(np.int64)
    X64 = X.astype(F64)
    cols = o.matrix(ko, X64, X64[head])
    diag = np.full(n, float(o.matrix(ko, X64[:1], X64[:1])[0, 0]))
    ref, gaps, dref = pr.replay(None, head, cols=cols, diag=diag)
    bound = 8.0 * (np.arange(rank) + 2) * EPS[dt] * diag[0]
    assert np.all(gaps <= bound), (gaps / bound).max()
    emu = pr.emulate(None, head, F32, cols=cols, diag=diag)[0] if dt == F32 else None
    lim = factor_limit(dt, ref, emu)
    err = np.abs(L.astype(F64) - ref).max(axis=1)
    print(f"\nn={n} {dt.__name__}: max|L - replay| {float(err.max()):.3g} (last row {float(err[-1]):.3g}), limit {lim:.3g}")
    assert err.max() <= lim
    lim4 = lim * 2.0 * np.sqrt(rank) * float(np.abs(L).max())
    assert np.abs(dres.astype(F64) - dref).max() <= lim4
    assert dres[-1] != SENTINEL and L[-1, 0] != SENTINEL        # the row of the second pass was written


def test_stopping(cg):
    """tol stops the factorisation where the oracle stops; columns beyond rank stay untouched (check_structure: the sentinel), and a
    shorter call returns the same leading columns and pivots bit for bit."""
    n, d = 257, 2
    X = points(n, d, F64)
    k = cg.EQ()
    M = o.matrix(o.Kernel(o.EQ), X)
    Lo, pivo, ranko = o.pivoted_cholesky(M, 1e-6, n)
    L, piv, dres, rank = raw_call(cg, k, X, n, 1e-6)
    check_structure(n, n, L, piv, dres, rank)
    assert rank == ranko and rank < n
    assert np.array_equal(piv[:rank], pivo[:rank])
    assert np.abs(L[:, :rank] - Lo).max() <= 1e-8
    assert dres.max() <= 1e-6
    L2, piv2, dres2, rank2 = raw_call(cg, k, X, rank - 3, 1e-6)
    check_structure(n, rank - 3, L2, piv2, dres2, rank2)
    assert rank2 == rank - 3
    assert np.array_equal(piv2, piv[:rank - 3])
    assert np.array_equal(L2.view(np.uint64), L[:, :rank - 3].view(np.uint64))
    # a tolerance above the diagonal stops at once: rank 0, nothing written
    L3, piv3, dres3, rank3 = raw_call(cg, k, X, 8, 2.0)
    assert rank3 == 0 and np.all(L3 == SENTINEL) and np.all(piv3 == -1)


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_python_layer(cg, dt):
    n, d, max_rank = 257, 2, 64
    X = points(n, d, dt)
    k = 2 * cg.Lengthscale(cg.RQ(1.5), 0.7)
    L, piv, dres, rank = raw_call(cg, k, X, max_rank, 0.0)
    Xt = torch.from_numpy(X).cuda()
    F = cg.pivoted_cholesky(cg.gramian(k, Xt), max_rank)
    assert isinstance(F, cg.PivotedCholesky)
    assert F.rank == rank and tuple(F.L.shape) == (n, rank) and F.L.dtype == TDT[dt]
    assert np.array_equal(F.L.cpu().numpy(), L[:, :rank])
    p = F.piv.cpu().numpy()
    assert np.array_equal(p[:rank], piv[:rank])
    assert np.array_equal(np.sort(p), np.arange(n)) and np.all(np.diff(p[rank:]) > 0)
    assert np.array_equal(F.residual_diagonal.cpu().numpy(), dres)
    assert float((F.to_dense() - F.L @ F.L.T).abs().max()) == 0.0
    # a stopped factorisation through the Python layer, and the degenerate sizes
    F0 = cg.pivoted_cholesky(cg.gramian(cg.EQ(), Xt), n, tol=1e-6)
    assert 0 < F0.rank < n and tuple(F0.L.shape) == (n, F0.rank) and F0.piv.shape[0] == n
    E = cg.pivoted_cholesky(cg.gramian(k, Xt), 0)
    assert E.rank == 0 and tuple(E.L.shape) == (n, 0) and np.array_equal(E.piv.cpu().numpy(), np.arange(n))
    # refused before any launch
    Yt = Xt.clone()
    with pytest.raises(cg.DimensionMismatch):
        cg.pivoted_cholesky(cg.Gramian(k, Xt, Yt), 8)
    with pytest.raises(cg.UnsupportedKernel):
        cg.pivoted_cholesky(cg.Gramian(cg.EQ() + cg.MaternP(1), Xt), 8)
    with pytest.raises(cg.UnsupportedKernel):
        cg.pivoted_cholesky(cg.Gramian(cg.Dot(), Xt), 8)
    with pytest.raises(cg.DimensionMismatch):
        cg.pivoted_cholesky(cg.gramian(k, Xt), n + 1)
    with pytest.raises(cg.UnsupportedKernel):
        cg.pivoted_cholesky(cg.gramian(k, torch.from_numpy(points(1031, 3, dt)).cuda()), 1025)
