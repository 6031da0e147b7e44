"""Dense / low-rank factorizations of a lazy Gramian: `cholesky`, `factorize`.

The reference instantiates `Matrix(G)` and calls LAPACK (src/gramian.jl:192-213); its own comment asks for "a special
cholesky implementation to avoid instantiating G in the low rank case" (:191).  Here
  * `cholesky(G)`               = device `Matrix(G)` tile (covgram_matrix) handed to torch.linalg.cholesky (rocSOLVER);
  * `cholesky(G, pivoted=True)` = that special implementation: a LAZY diagonally pivoted Cholesky that evaluates only the
                                   diagonal and one Gramian column per step (n kernel evaluations on the device each), so a
                                   rank-r factor of an n x n Gramian costs O(n r) kernel evaluations and O(n r^2) flops and
                                   never forms the matrix;
  * `factorize(G)`              = pivoted Cholesky with tol = 1e-6 up to n = 2^14, else the lazy G itself (CG path);
  * `pivoted_cholesky(G, r)`    = the same factor by covgram_pivoted_cholesky (csrc/pivchol.hip): one launch per pivot, no host
                                   synchronisation before the end — the set-up of
  * `PivotedCholeskyPreconditioner(G, D, r)` = (L L' + D)^-1 for CG on G + D, applied through covgram_lowrank_mvm.
Everything besides the kernel evaluations is torch plumbing on the same stream.
"""
from __future__ import annotations

from typing import Optional, Union

import torch

from . import _ffi
from . import kernels as K
from .gramian import Gramian, LazyOperator, MixedGramian, SpectralMixtureGramian, _axpby_, _dtype_code

DEFAULT_MAX_CHOLESKY_SIZE = 2 ** 14     # src/gramian.jl:201
DEFAULT_TOL = 1e-6                      # src/gramian.jl:202


class CholeskyFactor(LazyOperator):
    """Lower factor L (n x n) with G = L L'."""

    def __init__(self, L: torch.Tensor):
        self.L = L
        self.shape = (L.shape[0], L.shape[0])
        self.dtype, self.device = L.dtype, L.device

    def to_dense(self):
        return self.L @ self.L.T

    def solve(self, b: torch.Tensor) -> torch.Tensor:
        return torch.cholesky_solve(b.reshape(b.shape[0], -1), self.L).reshape(b.shape)

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        t = self.L @ (self.L.T @ a)
        return y.mul_(beta).add_(t, alpha=alpha) if beta != 0 else y.copy_(alpha * t)


class PivotedCholesky(LazyOperator):
    """P' G P ≈ L L' of rank r: `L` is n x r in ORIGINAL row order (row piv[k] is the k-th pivot), `piv`, `rank`;
    `residual_diagonal` = diag(G - L L') where the factorisation kept it (pivoted_cholesky), else None."""

    def __init__(self, L: torch.Tensor, piv: torch.Tensor, rank: int, residual_diagonal: Optional[torch.Tensor] = None):
        self.L, self.piv, self.rank = L, piv, rank
        self.residual_diagonal = residual_diagonal
        self.shape = (L.shape[0], L.shape[0])
        self.dtype, self.device = L.dtype, L.device

    def to_dense(self):
        return self.L @ self.L.T

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        t = self.L @ (self.L.T @ a)
        return y.mul_(beta).add_(t, alpha=alpha) if beta != 0 else y.copy_(alpha * t)


def diagonal(G: Gramian) -> torch.Tensor:
    """diag(G) for a square Gramian with x ≡ y: k(x_i, x_i) evaluated on the device (n kernel evaluations)."""
    n = G.shape[0]
    if isinstance(G, SpectralMixtureGramian):                 # cos(0) exp(0) = 1 for every component: the constant sum of the weights
        if not G.issymmetric():
            raise ValueError("diagonal: a Gramian with x = y expected")
        return torch.full((n,), float(G.w.sum()), dtype=G.dtype, device=G.device)
    tr = K.input_trait(G.k)
    if isinstance(tr, K.IsotropicInput):                      # phi(0) for every point
        v = Gramian(G.k, G.x[:1], G.x[:1]).to_dense()[0, 0]
        return v.expand(n).clone()
    if isinstance(tr, K.DotProductInput):                     # phi(|x_i|^2): a 1-d dot-product Gramian against the point 1
        z = (G.x * G.x).sum(dim=1, keepdim=True)
        one = torch.ones(1, 1, dtype=G.dtype, device=G.device)
        return Gramian(G.k, z, one).to_dense()[:, 0].contiguous()
    raise NotImplementedError("diagonal: GenericInput kernels have no device path")


def cholesky(G: LazyOperator, pivoted: bool = False, check: bool = True, tol: float = 0.0, max_rank: Optional[int] = None):
    """LinearAlgebra.cholesky(G::Gramian, Val(pivoted); check, tol) (src/gramian.jl:192-199)."""
    n, m = G.shape
    if n != m:
        raise ValueError("DimensionMismatch: matrix is not square")
    if not pivoted:
        L, info = torch.linalg.cholesky_ex(G.to_dense())
        if check and int(info) != 0:
            raise ValueError(f"PosDefException: matrix is not positive definite; Cholesky factorization failed at {int(info)}")
        return CholeskyFactor(L)
    if not isinstance(G, Gramian) or not G.issymmetric():
        raise NotImplementedError("pivoted cholesky: symmetric Gramian expected")
    max_rank = n if max_rank is None else min(max_rank, n)
    d = diagonal(G)
    live = torch.ones(n, dtype=torch.bool, device=G.device)
    L = torch.zeros((n, max_rank), dtype=G.dtype, device=G.device)
    piv, rank = [], 0
    neg_inf = torch.tensor(float("-inf"), dtype=G.dtype, device=G.device)
    for k in range(max_rank):
        dm = torch.where(live, d, neg_inf)
        p = int(torch.argmax(dm))                             # one host sync per pivot (the stopping test needs it anyway)
        dmax = float(dm[p])
        if not dmax > tol:                                    # LAPACK pstrf: stop at the first pivot <= tol
            break
        col = Gramian(G.k, G.x, G.x[p:p + 1]).to_dense()[:, 0]                   # G[:, p]: n kernel evaluations, on the device
        if k:
            col = col - L[:, :k] @ L[p, :k]
        L[:, k] = col / (dmax ** 0.5)
        d = d - L[:, k] ** 2
        live[p] = False
        piv.append(p)
        rank = k + 1
    rest = torch.nonzero(live).flatten().tolist()
    return PivotedCholesky(L[:, :rank].contiguous(), torch.tensor(piv + rest, device=G.device), rank)


def factorize(G: LazyOperator, max_cholesky_size: int = DEFAULT_MAX_CHOLESKY_SIZE, tol: float = DEFAULT_TOL):
    """LinearAlgebra.factorize(G::Gramian) (src/gramian.jl:205-213): pivoted Cholesky (detects low rank) up to
    max_cholesky_size, otherwise G stays lazy and solves go through CG."""
    n, m = G.shape
    if n != m:
        raise ValueError("DimensionMismatch: matrix is not square")
    if n <= max_cholesky_size and isinstance(G, Gramian) and G.issymmetric():
        return cholesky(G, pivoted=True, check=False, tol=tol)
    return G


# ----------------------------------------------------------------------------------------------
# the device factorisation and the preconditioner built on it
# ----------------------------------------------------------------------------------------------
def pivoted_cholesky(G: Gramian, max_rank: int, tol: float = 0.0) -> PivotedCholesky:
    """P' G P ≈ L L' of rank <= max_rank for a symmetric Gramian (x ≡ y) of one isotropic profile, fp32 or fp64, by
    covgram_pivoted_cholesky: LAPACK pstrf's rule (stop at the first pivot <= tol, ties to the smallest index), one launch per pivot,
    G never formed.  The only host read is `rank`, at the end.  Returns the PivotedCholesky of `cholesky(G, pivoted=True)`: L is
    n x rank (rows in the original order), piv = the pivots followed by the remaining indices in ascending order, and
    `residual_diagonal` = diag(G - L L')."""
    if isinstance(G, MixedGramian):
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, "pivoted_cholesky: MixedGramian is not supported (one isotropic profile only)")
    if not isinstance(G, Gramian):
        raise NotImplementedError("pivoted_cholesky: a Gramian is expected")
    if G.y is not G.x:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, "pivoted_cholesky: a symmetric Gramian gramian(k, x) is expected (y is not x)")
    spec = K.require_pivchol_spec(G.k)
    n = G.shape[0]
    max_rank = int(max_rank)
    dev, dt = G.device, G.dtype
    Lcm = torch.empty((max(max_rank, 0), n), dtype=dt, device=dev)        # column-major n x max_rank
    piv = torch.empty(max(max_rank, 0), dtype=torch.int32, device=dev)
    dres = torch.empty(n, dtype=dt, device=dev)
    rk = torch.zeros(1, dtype=torch.int32, device=dev)
    ctx = G._px.ctx.bind_stream()
    P = _ffi._P
    _ffi.check(_ffi.lib().covgram_pivoted_cholesky(ctx, _ffi.kref(spec), G._px.handle, max_rank, float(tol), P(Lcm.data_ptr()), max(n, 1),
                                                   P(piv.data_ptr()), P(dres.data_ptr()), P(rk.data_ptr())))
    rank = int(rk)                                            # the one synchronisation
    live = torch.ones(n, dtype=torch.int8, device=dev)
    head = piv[:rank].long()
    live[head] = 0
    rest = torch.sort(live, descending=True, stable=True).indices[:n - rank]   # the unpivoted indices, ascending (no host read)
    return PivotedCholesky(Lcm[:rank].t(), torch.cat([head, rest]), rank, residual_diagonal=dres)


class PivotedCholeskyPreconditioner(LazyOperator):
    """M^-1 = (L L' + D)^-1 with L the rank-r pivoted Cholesky factor of the Gramian G and D a positive diagonal (a float, or a 1-D
    tensor of length n): the preconditioner of CG on G + D.  Set-up: L by `pivoted_cholesky`, C = I_r + L' D^-1 L = R' R (r x r,
    torch, factored on the host in fp64), W = D^-1 L R^-1.  By Woodbury's identity M^-1 = D^-1 - W W', so `P(r)` is one elementwise product and ONE
    covgram_lowrank_mvm (alpha = -1, beta = 1 onto y = D^-1 r, a fresh tensor).  `logdet()` = log det(L L' + D) = log det C +
    sum log D_i.  Callable: cg(G + D, b, precond=P), with or without graph=True."""

    def __init__(self, G: Gramian, diag: Union[float, torch.Tensor], rank: int, tol: float = 0.0):
        n = G.shape[0]
        self.shape = (n, n)
        self.dtype, self.device = G.dtype, G.device
        if torch.is_tensor(diag):
            if diag.dim() != 1 or diag.shape[0] != n:
                raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: diag has shape {tuple(diag.shape)}, expected ({n},)")
            D = diag.to(device=self.device, dtype=self.dtype).contiguous()
            if not bool((D > 0).all()):
                raise ValueError("PivotedCholeskyPreconditioner: every entry of diag must be positive")
        else:
            if not float(diag) > 0:
                raise ValueError(f"PivotedCholeskyPreconditioner: diag = {diag} must be positive")
            D = torch.full((n,), float(diag), dtype=self.dtype, device=self.device)
        self.factor = pivoted_cholesky(G, min(int(rank), n), tol)
        self.rank = self.factor.rank
        self.D, self.Dinv = D, 1.0 / D
        L = self.factor.L
        DL = self.Dinv[:, None] * L
        Cm = L.T @ DL
        Cm.diagonal().add_(1.0)
        # The r x r part runs on the host, in fp64: the set-up has synchronised on `rank` already, r <= 1024, and the n x r operand then
        # meets the device only in GEMMs (a right-sided triangular solve on the 131072 x 128 fp64 operand ran out of rocBLAS workspace and
        # faulted, profiles/pivchol.txt).  C = R' R;  W = D^-1 L R^-1.
        R64 = torch.linalg.cholesky(Cm.to(device="cpu", dtype=torch.float64), upper=True)
        Rinv = torch.linalg.solve_triangular(R64, torch.eye(R64.shape[0], dtype=torch.float64), upper=True)
        self.R = R64.to(device=self.device, dtype=self.dtype)
        W = DL @ Rinv.to(device=self.device, dtype=self.dtype)
        self._Wcm = W.t().contiguous()                                                # column-major n x r for the library

    @property
    def W(self):
        return self._Wcm.t()

    def __call__(self, r: torch.Tensor) -> torch.Tensor:
        n, rk = self.shape[0], self.rank
        if r.shape[0] != n:
            raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: r has length {r.shape[0]}, expected {n}")
        r = r.to(device=self.device, dtype=self.dtype)
        vec = r.dim() == 1
        a = r.contiguous() if vec else r.t().contiguous()                             # column-major n x p
        y = (self.Dinv * a).contiguous()                                              # fresh: never aliases a
        if rk > 0 and n > 0:
            from .gramian import get_ctx
            ctx = get_ctx(self.device).bind_stream()
            P = _ffi._P
            _ffi.check(_ffi.lib().covgram_lowrank_mvm(ctx, P(self._Wcm.data_ptr()), n, P(self._Wcm.data_ptr()), n, n, n, rk, _dtype_code(self.dtype),
                                                      P(a.data_ptr()), n, P(y.data_ptr()), n, 1 if vec else a.shape[0], -1.0, 1.0, _ffi.DEVICE))
        return y if vec else y.t()

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        return _axpby_(y, self(a), alpha, beta)

    def logdet(self) -> torch.Tensor:
        """log det(L L' + D) (a 0-dim device tensor)."""
        return 2.0 * torch.log(self.R.diagonal()).sum() + torch.log(self.D).sum()

    def sample(self, p: int, generator=None) -> torch.Tensor:
        """(n, p) draws L g₁ + √D g₂ ~ N(0, L L' + D), g₁ and g₂ standard normal: the probes under which `logdet`'s preconditioned
        estimate is unbiased.  `generator`: a torch.Generator (the draws are made on its device), or None."""
        n, p = self.shape[0], int(p)
        gdev = generator.device if generator is not None else self.device
        g1 = torch.randn((self.rank, p), generator=generator, device=gdev, dtype=self.dtype).to(self.device)
        g2 = torch.randn((n, p), generator=generator, device=gdev, dtype=self.dtype).to(self.device)
        return self.factor.L @ g1 + self.D.sqrt()[:, None] * g2

    def to_dense(self):
        """The dense M^-1 = D^-1 - W W' (tests)."""
        return torch.diag(self.Dinv) - self.W @ self.W.T


def preconditioner(A, rank: int, tol: float = 0.0) -> PivotedCholeskyPreconditioner:
    """The pivoted-Cholesky preconditioner of A = G + Diagonal(d) (a Gramian plus a 1-D tensor, as `G + d` builds it) for
    cg(A, b, precond=...).  Anything else raises UnsupportedKernel."""
    from .solve import _split_shift
    G, d = _split_shift(A)
    if d is None or not isinstance(G, Gramian):
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"preconditioner: {type(A).__name__} is not a Gramian plus a diagonal (G + d with a 1-D "
                                                        "tensor d); no preconditioner is defined for it")
    return PivotedCholeskyPreconditioner(G, d, rank, tol)
