"""Krylov callers of the hot path: conjugate gradients for `G \\ b` and `(G + σ²I) \\ b`.

The reference solves lazy (block) Gramians with IterativeSolvers.cg! (src/gramian.jl:229-238,
src/lazy_linear_algebra.jl:135-144).  Here every MVM is a device kernel of libcovgram and all vectors stay resident on
the GPU.  Without a preconditioner the O(n) vector updates and the two dot products of an iteration are ONE library call
(covgram_cg_step_shifted: one launch for vectors that fit a workgroup's registers, three above, scalars on the device; the
diagonal term of G + σ²I and ‖r‖ ride along) — as torch ops they were eleven small launches, 45 us next to a 40 us MVM at
n = 16384; with a preconditioner they stay torch ops on the same stream.  One host synchronisation per
iteration (the convergence test), none inside the MVM.

A block of right-hand sides goes through `mbcg`: p independent recurrences over ONE matrix right-hand-side MVM per iteration, their vector
work and per-column stopping in covgram_bcg_* (csrc/bcg.hip).  The coefficients it logs are Lanczos coefficients: `logdet` and
`inv_quad_logdet` (stochastic Lanczos quadrature) are built on the same solve.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _ffi
from .gramian import LazyOperator, get_ctx, _dtype_code


NORM_SLOT = 2 + 512            # scal[NORM_SLOT] = |r| after a step (include/covgram.h: covgram_cg_step_shifted)


def _split_shift(A):
    """A = G + Diagonal(d) with one lazy term and one 1-D tensor -> (G, d); otherwise (A, None).  The library's CG step adds the
    diagonal term to Ap inside its first launch (covgram_cg_step_shifted), so the MVM of the iteration is the Gramian's alone."""
    from .gramian import LazyMatrixSum
    if isinstance(A, LazyMatrixSum) and len(A.args) == 2:
        lazy = [t for t in A.args if hasattr(t, "mul_") and not torch.is_tensor(t)]
        diag = [t for t in A.args if torch.is_tensor(t) and t.dim() == 1]
        if len(lazy) == 1 and len(diag) == 1:
            return lazy[0], diag[0]
    return A, None


def _fused_step(A, x, r, p, Ap):
    """The iteration's work through the library when everything is a contiguous CUDA vector of one supported dtype:
    returns (iterate, scal) or None; iterate() = the MVM Ap = G p + covgram_cg_step_shifted (alpha, x, r, rho', p, |r|: three
    launches).  scal[1] = |r|^2 and scal[NORM_SLOT] = |r| after every step."""
    if not (x.is_cuda and x.dim() == 1 and x.dtype in (torch.float32, torch.float64)):
        return None
    if not all(t.is_contiguous() and t.dtype == x.dtype and t.device == x.device for t in (r, p, Ap)):
        return None
    G, diag = _split_shift(A)
    if diag is not None:
        diag = diag.to(device=x.device, dtype=x.dtype).contiguous()
        if diag.shape[0] != x.shape[0]:
            G, diag = A, None
    lib = _ffi.lib()
    scal = torch.zeros(NORM_SLOT + 1, dtype=x.dtype, device=x.device)
    scal[1] = torch.dot(r, r)
    ctx = get_ctx(x.device)
    code, n = _dtype_code(x.dtype), x.shape[0]
    P = _ffi._P
    dptr = P(diag.data_ptr()) if diag is not None else None

    def iterate():
        G.mul_(Ap, p)                       # the hot path
        _ffi.check(lib.covgram_cg_step_shifted(ctx.bind_stream(), n, code, P(x.data_ptr()), P(r.data_ptr()), P(p.data_ptr()),
                                               P(Ap.data_ptr()), P(scal.data_ptr()), dptr))
    iterate.keep = (diag, G)                # (the captured graph holds raw pointers)
    return iterate, scal


def cg(A: LazyOperator, b: torch.Tensor, x0: Optional[torch.Tensor] = None, reltol: float = 1e-8, abstol: float = 0.0,
       maxiter: Optional[int] = None, precond=None, graph: bool = False, check_every: int = 8) -> Tuple[torch.Tensor, dict]:
    """Solve A x = b for a symmetric positive definite lazy operator A (cg!, IterativeSolvers 0.9.2 semantics:
    stops when ‖r‖ ≤ max(reltol·‖r₀‖, abstol)); `precond(r)` applies an SPD preconditioner M⁻¹ (Pl = M in the reference's
    keyword).  Returns (x, {"iterations", "residual_norm", "converged"}).  All scalars of the recurrence stay on the device;
    the only host synchronisation per iteration is the convergence test.

    graph=True (small, launch-bound systems): `check_every` iterations — the MVM's kernels and the vector updates — are captured
    once into a HIP graph and replayed; the residual is read back between replays, so the solve may run up to
    check_every − 1 iterations past the tolerance (they only refine x).

    A matrix b (n, p) is solved by `mbcg`: p independent recurrences over one matrix right-hand-side MVM per iteration (graph=True is
    not available for it)."""
    if torch.is_tensor(b) and b.dim() == 2:
        if graph:
            raise ValueError("cg: graph=True is restricted to a vector right-hand side; the batched iteration of a matrix right-hand side "
                             "(mbcg) is not captured")
        return mbcg(A, b, x0, reltol, abstol, maxiter, precond, check_every)
    if graph:
        return _cg_graph(A, b, x0, reltol, abstol, maxiter, precond, max(1, int(check_every)))
    n = A.shape[0]
    if A.shape[0] != A.shape[1] or b.shape[0] != n:
        raise ValueError("cg: A must be square and match b")
    b = b.to(device=A.device, dtype=A.dtype)
    x = torch.zeros_like(b) if x0 is None else x0.to(device=A.device, dtype=A.dtype).clone()
    r = b.clone()
    Ap = torch.empty_like(b)
    if x0 is not None:
        A.mul_(Ap, x)
        r -= Ap
    z = precond(r) if precond is not None else r
    p = z.clone()
    rz = torch.dot(r, z)
    r0 = float(torch.linalg.vector_norm(r))
    tol = max(reltol * r0, abstol)
    maxiter = n if maxiter is None else maxiter
    it, res = 0, r0
    fused = _fused_step(A, x, r, p, Ap) if precond is None else None
    if fused is not None:
        iterate, scal = fused
        while it < maxiter and res > tol:
            iterate()                       # Ap = A p; alpha, x, r, rho', p
            res = float(scal[NORM_SLOT])    # the convergence test: the iteration's one synchronisation
            it += 1
        return x, {"iterations": it, "residual_norm": res, "converged": res <= tol}
    while it < maxiter and res > tol:
        A.mul_(Ap, p)                       # the hot path
        alpha = rz / torch.dot(p, Ap)       # 0-dim device tensors: no synchronisation
        x.addcmul_(p, alpha)
        r.addcmul_(Ap, -alpha)
        z = precond(r) if precond is not None else r
        rz_new = torch.dot(r, z)
        p.mul_(rz_new / rz).add_(z)
        rz = rz_new
        res = float(torch.linalg.vector_norm(r))
        it += 1
    return x, {"iterations": it, "residual_norm": res, "converged": res <= tol}


def _cg_graph(A, b, x0, reltol, abstol, maxiter, precond, check_every):
    """cg with the iteration body as a replayed HIP graph (torch.cuda.CUDAGraph on ROCm = hipGraph).  The body is warmed up
    once eagerly (one real iteration: libcovgram sizes its workspaces and fragment caches outside the capture), then captured;
    every tensor the body touches is persistent, scalars are 0-dim device tensors."""
    n = A.shape[0]
    if A.shape[0] != A.shape[1] or b.shape[0] != n:
        raise ValueError("cg: A must be square and match b")
    b = b.to(device=A.device, dtype=A.dtype)
    x = torch.zeros_like(b) if x0 is None else x0.to(device=A.device, dtype=A.dtype).clone()
    r = b.clone()
    Ap = torch.empty_like(b)
    if x0 is not None:
        A.mul_(Ap, x)
        r -= Ap
    z = precond(r) if precond is not None else r
    p = z.clone()
    rz = torch.dot(r, z).clone()
    res = torch.linalg.vector_norm(r).clone()
    r0 = float(res)
    tol = max(reltol * r0, abstol)
    maxiter = n if maxiter is None else maxiter
    it = 0
    if not (r0 > tol) or maxiter <= 0:
        return x, {"iterations": 0, "residual_norm": r0, "converged": r0 <= tol}

    fused = _fused_step(A, x, r, p, Ap) if precond is None else None

    def body():
        if fused is not None:
            fused[0]()                      # |r| is left in scal[NORM_SLOT]
            return
        A.mul_(Ap, p)
        alpha = rz / torch.dot(p, Ap)
        x.addcmul_(p, alpha)
        r.addcmul_(Ap, -alpha)
        zz = precond(r) if precond is not None else r
        rz_new = torch.dot(r, zz)
        p.mul_(rz_new / rz).add_(zz)
        rz.copy_(rz_new)
        res.copy_(torch.linalg.vector_norm(r))

    side = torch.cuda.Stream(device=A.device)
    side.wait_stream(torch.cuda.current_stream(A.device))
    with torch.cuda.stream(side):
        body(); it += 1                                    # eager warm-up = iteration 1 (on the capture stream)
    torch.cuda.current_stream(A.device).wait_stream(side)
    # ONE graph holds check_every iterations: a replay costs the host tens of microseconds whatever it holds (n = 8192 fp32: 62 us per
    # replayed single iteration against 25 us of kernels), and the residual is only looked at between replays anyway
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(check_every):
            body()
    if fused is not None:
        res = fused[1][NORM_SLOT]
    resf = float(res)
    while it + check_every <= maxiter and resf > tol:
        g.replay()
        it += check_every
        resf = float(res)
    while it < maxiter and resf > tol:      # fewer than check_every iterations left of maxiter: eagerly
        body()
        it += 1
        resf = float(res)
    return x, {"iterations": it, "residual_norm": resf, "converged": resf <= tol, "graph": True}


# ---- batched CG on a block of right-hand sides, and what its coefficients give: log det by stochastic Lanczos quadrature --------------
def _rows(M: torch.Tensor) -> torch.Tensor:
    """The (p, n) row-major tensor whose transpose is the (n, p) matrix M: column-major n x p for the library (no copy when M is the
    transpose of a contiguous tensor, which is what every matrix `mul_` and the preconditioner return)."""
    return M.t().contiguous()


def mbcg(A: LazyOperator, B: torch.Tensor, x0: Optional[torch.Tensor] = None, reltol: float = 1e-8, abstol: float = 0.0,
         maxiter: Optional[int] = None, precond=None, check_every: int = 8, lanczos: bool = False) -> Tuple[torch.Tensor, dict]:
    """Solve A X = B for an (n, p) block of right-hand sides: p INDEPENDENT conjugate-gradient recurrences (the iteration of `cg`, per
    column) that share one matrix right-hand-side `mul_` per iteration.  Column j stops — its x_j and r_j frozen — when
    ‖r_j‖ ≤ max(reltol·‖r₀ⱼ‖, abstol); the solve ends when every column has, or after `maxiter` iterations.

    The vector work of an iteration is covgram_bcg_step (one launch for columns that fit a workgroup's registers, three above), or with
    a preconditioner covgram_bcg_update / `precond` on the whole block / covgram_bcg_direction; the diagonal of A = G + d is folded into
    the step.  All scalars live on the device in fp64; the one host synchronisation is the read of the number of active columns every
    `check_every` iterations (a finished column does no work meanwhile, so nothing runs past its tolerance).

    Returns (X, info): "iterations" (the total), "column_iterations", "residual_norm" (per column, the recurrence's), "converged" and
    "column_converged".  lanczos=True adds the CG coefficients "alpha", "beta" (iterations x p, fp64, 0 where a column was frozen), "rz0"
    (r₀ⱼᵀM⁻¹r₀ⱼ) and "tridiagonals" (cg_tridiagonals)."""
    n = A.shape[0]
    if A.shape[0] != A.shape[1]:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: mbcg needs a square operator, got {tuple(A.shape)}")
    if not torch.is_tensor(B) or B.dim() != 2 or B.shape[0] != n:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: B has shape {tuple(getattr(B, 'shape', ()))}, expected ({n}, p)")
    if x0 is not None and tuple(x0.shape) != tuple(B.shape):
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: x0 has shape {tuple(x0.shape)}, expected {tuple(B.shape)}")
    dev, dt, p = A.device, A.dtype, B.shape[1]
    code = _dtype_code(dt)
    Rt = torch.empty((p, n), dtype=dt, device=dev)             # every block is (p, n) row-major: column-major n x p, ld = n
    Rt.copy_(B.t())
    Xt = torch.zeros_like(Rt)
    APt = torch.empty_like(Rt)
    G, diag = _split_shift(A)
    if diag is not None:
        diag = diag.to(device=dev, dtype=dt).contiguous()
        if diag.shape[0] != n:
            G, diag = A, None
    if x0 is not None:
        Xt.copy_(x0.t())
        A.mul_(APt.t(), Xt.t())
        Rt -= APt
    Zt = _rows(precond(Rt.t())) if precond is not None else Rt
    Pt = Zt.clone()
    maxiter = n if maxiter is None else int(maxiter)
    check_every = max(1, int(check_every))
    state = torch.zeros(max(p, 1) * (_ffi.BCG_FIELDS + 2 * _ffi.BCG_SLAB), dtype=torch.float64, device=dev)
    nact = torch.zeros(1, dtype=torch.int32, device=dev)
    alog = torch.zeros((max(maxiter, 1), p), dtype=torch.float64, device=dev) if lanczos else None
    blog = torch.zeros_like(alog) if lanczos else None
    lib, ctx, P = _ffi.lib(), get_ctx(dev), _ffi._P
    ld = max(n, 1)
    ptr = lambda t: P(t.data_ptr()) if t is not None else None
    _ffi.check(lib.covgram_bcg_init(ctx.bind_stream(), n, p, code, ptr(Rt), ld, ptr(Zt), ld, float(reltol), float(abstol), ptr(state), ptr(nact)))
    field = lambda f: state[f * p:(f + 1) * p]
    rz0 = field(_ffi.BCG_RZ).clone() if lanczos else None
    it = 0
    active = int(nact) if n > 0 and p > 0 else 0
    while it < maxiter and active > 0:
        G.mul_(APt.t(), Pt.t())                                 # the hot path: one product for all p columns
        if precond is None:
            _ffi.check(lib.covgram_bcg_step(ctx.bind_stream(), n, p, code, ptr(Xt), ld, ptr(Rt), ld, ptr(Pt), ld, ptr(APt), ld, ptr(diag),
                                            ptr(state), ptr(nact), ptr(alog), ptr(blog), it))
        else:
            _ffi.check(lib.covgram_bcg_update(ctx.bind_stream(), n, p, code, ptr(Xt), ld, ptr(Rt), ld, ptr(Pt), ld, ptr(APt), ld, ptr(diag),
                                              ptr(state), ptr(alog), it))
            Zt = _rows(precond(Rt.t()))
            _ffi.check(lib.covgram_bcg_direction(ctx.bind_stream(), n, p, code, ptr(Rt), ld, ptr(Zt), ld, ptr(Pt), ld, ptr(state), ptr(nact),
                                                 ptr(blog), it))
        it += 1
        if it % check_every == 0 or it == maxiter:
            active = int(nact)                                  # the only synchronisation
    host = state[:_ffi.BCG_FIELDS * p].cpu().reshape(_ffi.BCG_FIELDS, p)
    iters = host[_ffi.BCG_ITERS].to(torch.int64)
    conv = host[_ffi.BCG_RR] <= host[_ffi.BCG_TOL2]
    info = {"iterations": it, "column_iterations": iters.tolist(), "residual_norm": host[_ffi.BCG_RR].sqrt(),
            "converged": bool(conv.all()), "column_converged": conv.tolist()}
    if lanczos:
        info["alpha"], info["beta"], info["rz0"] = alog[:it].cpu(), blog[:it].cpu(), rz0.cpu()
        info["tridiagonals"] = cg_tridiagonals(info["alpha"], info["beta"], iters)
    return Xt.t(), info


def cg_tridiagonals(alpha, beta, iters):
    """The Lanczos matrices of p CG recurrences from their coefficients (alpha, beta: iterations x p; column j took iters[j] steps):
    T_j = tridiag with  T[i, i] = 1/α_i + β_{i−1}/α_{i−1}  (the second term for i > 0)  and  T[i, i+1] = T[i+1, i] = √β_i / α_i,
    of order iters[j] — or up to the first α_i = 0 (a recurrence that broke down or was frozen).  T_j is the projection of M^-1/2 A M^-1/2
    onto the Krylov space of the (preconditioned) start residual.  Host, fp64: a list of p CPU tensors."""
    alpha = torch.as_tensor(alpha).to(device="cpu", dtype=torch.float64)
    alpha = alpha[:, None] if alpha.dim() == 1 else alpha
    beta = torch.as_tensor(beta).to(device="cpu", dtype=torch.float64).reshape(alpha.shape)
    p = alpha.shape[1]
    iters = [int(v) for v in torch.as_tensor(iters).reshape(-1).tolist()]
    if len(iters) != p:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: {len(iters)} iteration counts for {p} columns")
    out = []
    for j in range(p):
        m = min(iters[j], alpha.shape[0])
        a, b = alpha[:m, j], beta[:m, j]
        zero = torch.nonzero(a == 0).flatten()
        if zero.numel():
            m = int(zero[0])
            a, b = a[:m], b[:m]
        T = torch.zeros((m, m), dtype=torch.float64)
        if m:
            d = 1.0 / a
            d[1:] += b[:-1] / a[:-1]
            off = b[:-1].sqrt() / a[:-1]
            T.diagonal().copy_(d)
            T.diagonal(1).copy_(off)
            T.diagonal(-1).copy_(off)
        out.append(T)
    return out


def lanczos_quadrature(T: torch.Tensor, f) -> float:
    """e₁ᵀ f(T) e₁ = Σ_k (first component of eigenvector k)² f(λ_k) of a symmetric (tridiagonal) T, by `eigh` on the host in fp64 — the
    Gauss quadrature of the unit start vector's spectral measure.  An empty T gives 0."""
    T = torch.as_tensor(T, dtype=torch.float64, device="cpu")
    if T.shape[0] == 0:
        return 0.0
    lam, V = torch.linalg.eigh(T)
    return float((V[0] ** 2 * f(lam)).sum())


def _probes(A, probes, precond, generator):
    n = A.shape[0]
    if torch.is_tensor(probes):
        if probes.dim() != 2 or probes.shape[0] != n:
            raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: probes have shape {tuple(probes.shape)}, expected ({n}, p)")
        return probes.to(device=A.device, dtype=A.dtype)
    p = int(probes)
    if p < 1:
        raise ValueError(f"logdet: probes = {probes} must be at least 1")
    if precond is not None:
        if not hasattr(precond, "sample") or not hasattr(precond, "logdet"):
            raise TypeError("logdet: the preconditioner must offer sample(p, generator) and logdet() (PivotedCholeskyPreconditioner)")
        return precond.sample(p, generator)
    gdev = generator.device if generator is not None else A.device
    Z = torch.randint(0, 2, (n, p), generator=generator, device=gdev)           # Rademacher: ±1
    return (2 * Z - 1).to(device=A.device, dtype=A.dtype)


def _slq(info, cols, precond):
    """(estimate, values, stderr) of log det from the Lanczos matrices of the probe columns `cols` of an mbcg run."""
    vals = torch.tensor([float(info["rz0"][j]) * lanczos_quadrature(info["tridiagonals"][j], torch.log) for j in cols], dtype=torch.float64)
    base = float(precond.logdet()) if precond is not None else 0.0
    stderr = float(vals.std(unbiased=True) / len(cols) ** 0.5) if len(cols) > 1 else float("nan")
    return base + float(vals.mean()), vals, stderr


def logdet(A: LazyOperator, probes=16, maxiter: Optional[int] = None, reltol: float = 1e-6, precond=None, generator=None):
    """log det A of a symmetric positive definite lazy operator by stochastic Lanczos quadrature: with probes z_j,
    log det A = log det M + tr log(M^-1/2 A M^-1/2) ≈ precond.logdet() + (1/p) Σ_j rz₀ⱼ · e₁ᵀ log(T_j) e₁, where T_j is the Lanczos matrix
    of column j of ONE mbcg(A, Z, precond=precond) and rz₀ⱼ = z_jᵀM⁻¹z_j (= n for Rademacher probes without a preconditioner).
    `probes`: an (n, p) tensor, or a count — Rademacher draws without a preconditioner, precond.sample(p) ~ N(0, M) with one (the
    distribution under which the estimate is unbiased).  Returns (estimate, info): info["values"] the per-probe terms, "stderr" their
    standard error, and the solve's info."""
    Z = _probes(A, probes, precond, generator)
    _, info = mbcg(A, Z, reltol=reltol, maxiter=maxiter, precond=precond, lanczos=True)
    est, vals, stderr = _slq(info, range(Z.shape[1]), precond)
    info.update(values=vals, stderr=stderr, probes=Z.shape[1])
    return est, info


def inv_quad_logdet(A: LazyOperator, b: torch.Tensor, probes=16, maxiter: Optional[int] = None, reltol: float = 1e-6, precond=None,
                    generator=None):
    """(bᵀA⁻¹b, log det A, x = A⁻¹b, info) — the two terms of a Gaussian process's negative log marginal likelihood — from ONE
    mbcg on the block [b | Z]: column 0 is the solve, the probe columns give the log-determinant as in `logdet`."""
    n = A.shape[0]
    if not torch.is_tensor(b) or b.dim() != 1 or b.shape[0] != n:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: b has shape {tuple(getattr(b, 'shape', ()))}, expected ({n},)")
    Z = _probes(A, probes, precond, generator)
    b = b.to(device=A.device, dtype=A.dtype)
    X, info = mbcg(A, torch.cat([b[:, None], Z], dim=1), reltol=reltol, maxiter=maxiter, precond=precond, lanczos=True)
    x = X[:, 0].contiguous()
    est, vals, stderr = _slq(info, range(1, Z.shape[1] + 1), precond)
    info.update(values=vals, stderr=stderr, probes=Z.shape[1])
    return torch.dot(b, x), est, x, info


def inv_quad_logdet_gradient(A: LazyOperator, b: torch.Tensor, probes=16, maxiter: Optional[int] = None, reltol: float = 1e-6, precond=None,
                             generator=None):
    """(bᵀA⁻¹b, log det A, x = A⁻¹b, grad_inv_quad, grad_logdet, info): inv_quad_logdet and the derivatives of its two terms with respect
    to the hyper-parameters of the kernel, for A = G + σ²I or G + Diagonal(d) (as _split_shift splits it; G alone works too) with G the
    Gramian of gramian(k, x) — or the SpectralMixtureGramian of a spectral mixture, whose bilinear forms spectral_mixture_gradient
    evaluates in place of bilinear_gradient, or the MixedGramian of a mixed-trait Sum / Product, whose forms mixed_bilinear_gradient evaluates.  ONE mbcg on [b | Z], exactly as inv_quad_logdet runs it, then with α = A⁻¹b and the probe solves A⁻¹z_t
        grad_inv_quad = −αᵀ(∂G/∂θ)α,     grad_logdet ≈ (1/p) Σ_t (M⁻¹z_t)ᵀ(∂G/∂θ)(A⁻¹z_t)   (M⁻¹z = z without a preconditioner),
    both float64 CPU tensors in hyperparameters(k) order.  The negative log marginal likelihood ½ bᵀA⁻¹b + ½ log det A has the gradient
    ½ (grad_inv_quad + grad_logdet).  When the diagonal term is a scalar shift — every entry of the 1-D tensor equal — the derivative
    with respect to σ² is appended to both: −αᵀα and (1/p) Σ_t (M⁻¹z_t)ᵀ(A⁻¹z_t).
    The bilinear forms are evaluated one column at a time (1 + p calls of bilinear_gradient or spectral_mixture_gradient with nvec = 1), NOT as one rank-(1 + p)
    pass: that is what gives the per-probe terms, info["grad_logdet_values"] (p × parameters), and from them
    info["grad_logdet_stderr"], the per-parameter standard error of grad_logdet.  The gradient of precond.logdet() is not part of
    grad_logdet: with a preconditioner that depends on θ the estimate is that of tr(A⁻¹∂A) all the same, since E[(M⁻¹z)zᵀ] = I for z ~ N(0, M)."""
    from .gramian import Gramian, MixedGramian, SpectralMixtureGramian, bilinear_gradient, mixed_bilinear_gradient, spectral_mixture_gradient, _bilinear_plan
    from .kernels import require_mixed_parameter_spec
    G, diag = _split_shift(A)
    if type(G) is SpectralMixtureGramian:
        form_gradient = spectral_mixture_gradient
    elif type(G) is MixedGramian:
        lowered = require_mixed_parameter_spec(G.k)             # UnsupportedKernel by name, before the solve
        form_gradient = lambda G, u, a: mixed_bilinear_gradient(G, u, a, _spec=lowered)
    elif type(G) is Gramian:
        form_gradient = bilinear_gradient
        _bilinear_plan(G.k)                                     # UnsupportedKernel by name, before the solve
    else:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"inv_quad_logdet_gradient: {type(G).__name__} is not supported (gramian(k, x) [+ diagonal] only)")
    n = A.shape[0]
    if not torch.is_tensor(b) or b.dim() != 1 or b.shape[0] != n:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: b has shape {tuple(getattr(b, 'shape', ()))}, expected ({n},)")
    Z = _probes(A, probes, precond, generator)
    b = b.to(device=A.device, dtype=A.dtype)
    X, info = mbcg(A, torch.cat([b[:, None], Z], dim=1), reltol=reltol, maxiter=maxiter, precond=precond, lanczos=True)
    x = X[:, 0].contiguous()
    p = Z.shape[1]
    est, vals, stderr = _slq(info, range(1, p + 1), precond)
    MZ = precond(Z) if precond is not None else Z
    _, gq = form_gradient(G, x, x)
    rows = [form_gradient(G, MZ[:, t].contiguous(), X[:, 1 + t].contiguous())[1] for t in range(p)]
    gq = -gq
    scalar_shift = diag is not None and diag.numel() > 0 and bool((diag == diag.reshape(-1)[0]).all())
    if scalar_shift:
        gq = torch.cat([gq, -torch.dot(x, x).double().cpu().reshape(1)])
        shift = (MZ * X[:, 1:]).sum(0).double().cpu()
        rows = [torch.cat([r, shift[t].reshape(1)]) for t, r in enumerate(rows)]
    per_probe = torch.stack(rows) if rows else torch.zeros((0, gq.shape[0]), dtype=torch.float64)
    gl = per_probe.mean(0)
    gl_stderr = per_probe.std(0, unbiased=True) / p ** 0.5 if p > 1 else torch.full_like(gl, float("nan"))
    info.update(values=vals, stderr=stderr, probes=p, grad_logdet_values=per_probe, grad_logdet_stderr=gl_stderr)
    return torch.dot(b, x), est, x, gq, gl, info


def minres(A: LazyOperator, b: torch.Tensor, x0: Optional[torch.Tensor] = None, reltol: Optional[float] = None, abstol: float = 0.0,
           maxiter: Optional[int] = None, check_every: int = 1) -> Tuple[torch.Tensor, dict]:
    """Solve A x = b for a square SYMMETRIC lazy operator A, definite or not (minres!, IterativeSolvers 0.9.2; the reference's
    `F \\ b` for a BarnesHutFactorization, src/barneshut.jl:64-72): the Paige-Saunders recurrence — Lanczos vectors, one Givens
    rotation per iteration, the iterate updated from three direction vectors.  Stops when the recurrence's residual norm is
    ≤ max(reltol·‖r₀‖, abstol); reltol defaults to sqrt(eps(dtype)).  Returns (x, {"iterations", "residual_norm", "converged"}).
    Every scalar of the recurrence is a 0-dim device tensor; the only host synchronisation is the convergence read every
    `check_every` iterations (the solve may then run up to check_every − 1 iterations past the tolerance)."""
    n = A.shape[0]
    if A.shape[0] != A.shape[1] or b.shape[0] != n:
        raise ValueError("minres: A must be square and match b")
    if b.dim() != 1:
        raise ValueError(f"minres: b must be a vector, got shape {tuple(b.shape)} (solve a matrix right-hand side column by column)")
    b = b.to(device=A.device, dtype=A.dtype)
    if reltol is None:
        reltol = float(torch.finfo(A.dtype).eps) ** 0.5
    x = torch.zeros_like(b) if x0 is None else x0.to(device=A.device, dtype=A.dtype).clone()
    r2 = b.clone()
    y = torch.empty_like(b)
    if x0 is not None:
        A.mul_(y, x)
        r2 -= y
    beta = torch.linalg.vector_norm(r2)
    r0 = float(beta)
    tol = max(reltol * r0, abstol)
    maxiter = n if maxiter is None else maxiter
    check_every = max(1, int(check_every))
    it, res = 0, r0
    if not (r0 > tol):
        return x, {"iterations": 0, "residual_norm": r0, "converged": r0 <= tol}
    zero, one = torch.zeros_like(beta), torch.ones_like(beta)
    tiny = torch.full_like(beta, float(torch.finfo(A.dtype).tiny))
    r1 = torch.zeros_like(b)                # (the first iteration subtracts (beta / oldb) r1 = 0)
    v = torch.empty_like(b)
    w, w1, w2 = torch.zeros_like(b), torch.zeros_like(b), torch.zeros_like(b)
    oldb, dbar, epsln, phibar, cs, sn = one, zero, zero, beta, -one, zero
    while it < maxiter and res > tol:
        torch.mul(r2, torch.where(beta > 0, 1 / beta, zero), out=v)      # the Lanczos vector (beta = 0: the Krylov space is exhausted)
        A.mul_(y, v)                        # the hot path
        y.addcmul_(r1, -(beta / oldb))
        alfa = torch.dot(v, y)
        y.addcmul_(r2, -(alfa / torch.maximum(beta, tiny)))
        r1, r2, y = r2, y, r1               # (y is overwritten by the next product)
        oldb, beta = beta, torch.linalg.vector_norm(r2)
        oldeps = epsln                      # the previous rotation on the new column of the tridiagonal matrix
        delta = cs * dbar + sn * alfa
        gbar = sn * dbar - cs * alfa
        epsln, dbar = sn * beta, -cs * beta
        gamma = torch.maximum(torch.hypot(gbar, beta), tiny)             # the new rotation
        cs, sn = gbar / gamma, beta / gamma
        phi, phibar = cs * phibar, sn * phibar
        w1, w2, w = w2, w, w1               # w <- (v - oldeps w1 - delta w2) / gamma
        w.copy_(v).addcmul_(w1, -oldeps).addcmul_(w2, -delta).div_(gamma)
        x.addcmul_(w, phi)
        it += 1
        if it % check_every == 0 or it == maxiter:
            res = float(phibar)             # |r| of the recurrence: the convergence test's synchronisation
    return x, {"iterations": it, "residual_norm": res, "converged": res <= tol}


def solve(A: LazyOperator, b: torch.Tensor, **kw) -> torch.Tensor:
    """`A \\ b` for lazy Gramians (src/gramian.jl:229-238)."""
    return cg(A, b, **kw)[0]


def toeplitz_solve(T, b: torch.Tensor, reltol: float = 1e-12, maxiter: Optional[int] = None):
    """x = T \\ b for a symmetric positive definite Toeplitz operator.

    The reference's direct solvers (`levinson`, src/toeplitz.jl:77-111) are O(n²) recurrences of n−1 dependent steps — no
    parallelism to give a GPU.  The device answer is preconditioned CG over the O(n log n) FFT MVM of `covgram_toeplitz_mvm`
    with T. Chan's optimal circulant preconditioner c_k = ((n−k) t_k + k t_{n−k}) / n, applied by FFT (torch.fft → rocFFT);
    it is positive definite whenever T is.  Returns (x, info)."""
    vc = T.vc
    n = vc.shape[0]
    if getattr(T, "vr", None) is not None or T.shape[0] != T.shape[1]:
        raise NotImplementedError("toeplitz_solve: symmetric Toeplitz expected")
    k = torch.arange(n, device=vc.device, dtype=vc.dtype)
    c = ((n - k) * vc + k * torch.roll(vc.flip(0), 1)) / n          # t_{n-k} with t_n := t_0 at k = 0 (weight 0)
    lam = torch.fft.rfft(c)                                          # real spectrum of the symmetric circulant
    inv = 1.0 / lam.real
    def precond(r):
        return torch.fft.irfft(torch.fft.rfft(r) * inv, n)
    return cg(T, b, reltol=reltol, maxiter=maxiter if maxiter is not None else 10 * n, precond=precond)


# ---- the reference's direct Toeplitz solvers on the device (src/toeplitz.jl:12-111; csrc/toeplitz_direct.hip) ---------------
def _unit_diagonal(r_or_T, dtype=None):
    """(r, r0): r = first column without its leading entry, scaled to a unit diagonal; a SymmetricToeplitz operator T gives
    r = T.vc[1:] / T.vc[0] and r0 = T.vc[0] (src/toeplitz.jl:40-46,100-111 — the reference tests `r_0 == 1` where it means
    `r_0 != 1`; the normalisation is done right here, as in the oracle)."""
    from .gramian import get_ctx
    if hasattr(r_or_T, "vc"):
        if getattr(r_or_T, "vr", None) is not None:
            raise NotImplementedError("direct Toeplitz solvers: symmetric Toeplitz expected")
        vc = r_or_T.vc
        return (vc[1:] / vc[0]).contiguous(), float(vc[0])
    r = torch.as_tensor(r_or_T)
    if not r.is_cuda:
        r = r.to(get_ctx().device)
    if dtype is not None:
        r = r.to(dtype)
    return r.contiguous(), 1.0


def durbin(r: torch.Tensor) -> torch.Tensor:
    """durbin(r): y = K \\ (-r), K = SymmetricToeplitz([1, r[1:end-1]]) (src/toeplitz.jl:12-27)."""
    from . import _ffi
    from .gramian import get_ctx, _dtype_code
    r, _ = _unit_diagonal(r)
    y = torch.empty_like(r)
    ctx = get_ctx(r.device).bind_stream()
    _ffi.check(_ffi.lib().covgram_toeplitz_durbin(ctx, _ffi._P(r.data_ptr()), r.shape[0], _ffi._P(y.data_ptr()), _dtype_code(r.dtype), _ffi.DEVICE))
    return y


def levinson(r_or_T, b: torch.Tensor) -> torch.Tensor:
    """levinson(r, b) = SymmetricToeplitz([1; r]) \\ b, or levinson(T, b) = T \\ b (src/toeplitz.jl:75-111): the O(n²) chain of
    n - 1 dependent steps on one workgroup.  For large n `toeplitz_solve` (PCG over the FFT MVM) is the faster path."""
    from . import _ffi
    from .gramian import get_ctx, _dtype_code
    r, r0 = _unit_diagonal(r_or_T, b.dtype if torch.is_tensor(b) else None)
    b = torch.as_tensor(b).to(device=r.device, dtype=r.dtype).contiguous()
    n = b.shape[0]
    if r.shape[0] != n - 1:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: length(b) = {n} ≠ {r.shape[0] + 1} = length(r) + 1")
    x = torch.empty_like(b)
    ctx = get_ctx(r.device).bind_stream()
    _ffi.check(_ffi.lib().covgram_toeplitz_levinson(ctx, _ffi._P(r.data_ptr()), _ffi._P(b.data_ptr()), n, _ffi._P(x.data_ptr()), _dtype_code(r.dtype), _ffi.DEVICE))
    return x / r0 if r0 != 1.0 else x


def trench(r_or_T) -> torch.Tensor:
    """trench(r) = inv(SymmetricToeplitz([1; r])), or trench(T) = inv(T) (src/toeplitz.jl:29-71), as a full symmetric matrix."""
    from . import _ffi
    from .gramian import get_ctx, _dtype_code
    r, r0 = _unit_diagonal(r_or_T)
    n = r.shape[0] + 1
    Bt = torch.empty((n, n), dtype=r.dtype, device=r.device)       # column-major n x n == the transpose of a C-contiguous tensor
    ctx = get_ctx(r.device).bind_stream()
    _ffi.check(_ffi.lib().covgram_toeplitz_trench(ctx, _ffi._P(r.data_ptr()) if n > 1 else _ffi._P(Bt.data_ptr()), n, _ffi._P(Bt.data_ptr()), n,
                                                  _dtype_code(r.dtype), _ffi.DEVICE))
    B = Bt.t()
    return B / r0 if r0 != 1.0 else B
