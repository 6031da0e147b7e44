"""numpy restatements of the batched CG recurrences (include/covgram.h: covgram_bcg_*; covgram/solve.py: mbcg), of the Lanczos matrices
their coefficients give and of the quadrature on them — for the tests, no GPU.

Vectors are (n, p) arrays STORED in `dtype` (every update is evaluated in extended precision and rounded once, which is what a fused
multiply-add gives up to a rare double rounding); every scalar — the dot products, alpha, beta, the thresholds — is fp64, as on the device."""
import numpy as np


def step(X, R, P, AP, Z, diag, rz, tol2, rr, active, iters, dtype=np.float64):
    """One iteration on all columns after AP = G P.  Z = None means Z = R (no preconditioner); with a preconditioner Z must be
    M^-1 applied to the UPDATED R, so pass a callable Z(R) -> array.  Returns a dict: the new X, R, P, AP, rz, rr, active, iters (copies),
    alpha, beta, gamma, and for the error bounds the sums of absolute terms abs_gamma = Σ|p·ap|, abs_rz = Σ|r·z|."""
    f8, hp = np.float64, np.longdouble
    X, R, P, AP = (np.array(a, dtype=dtype) for a in (X, R, P, AP))
    rz, rr, iters = np.array(rz, dtype=f8), np.array(rr, dtype=f8), np.array(iters, dtype=np.int64)
    act = np.array(active, dtype=bool)
    p = X.shape[1]
    if diag is not None:
        APs = (AP.astype(hp) + np.asarray(diag, dtype=dtype).astype(hp)[:, None] * P.astype(hp)).astype(dtype)
        AP[:, act] = APs[:, act]
    gamma = np.einsum("ij,ij->j", P.astype(f8), AP.astype(f8))
    abs_gamma = np.einsum("ij,ij->j", np.abs(P).astype(f8), np.abs(AP).astype(f8))
    ok = act & (rz != 0) & (gamma != 0)
    alpha = np.where(ok, rz / np.where(ok, gamma, 1.0), 0.0)
    alpha_t = alpha.astype(dtype).astype(hp)
    Xn = (X.astype(hp) + alpha_t * P.astype(hp)).astype(dtype)
    Rn = (R.astype(hp) - alpha_t * AP.astype(hp)).astype(dtype)
    Xn[:, ~act], Rn[:, ~act] = X[:, ~act], R[:, ~act]
    rr_new = np.where(act, np.einsum("ij,ij->j", Rn.astype(f8), Rn.astype(f8)), rr)
    Zn = Rn if Z is None else np.array(Z(Rn) if callable(Z) else Z, dtype=dtype)
    rzn = np.einsum("ij,ij->j", Rn.astype(f8), Zn.astype(f8))
    abs_rz = np.einsum("ij,ij->j", np.abs(Rn).astype(f8), np.abs(Zn).astype(f8))
    okb = act & (rz != 0)
    beta = np.where(okb, rzn / np.where(okb, rz, 1.0), 0.0)
    beta_t = beta.astype(dtype).astype(hp)
    Pn = (Zn.astype(hp) + beta_t * P.astype(hp)).astype(dtype)
    Pn[:, beta_t == 0] = Zn[:, beta_t == 0]
    rz_new = np.where(act, rzn, rz)
    iters = iters + act
    act_new = act & (rr_new > np.asarray(tol2, dtype=f8))
    return dict(X=Xn, R=Rn, P=Pn, AP=AP, Z=Zn, rz=rz_new, rr=rr_new, active=act_new, iters=iters, alpha=alpha, beta=beta, gamma=gamma,
                abs_gamma=abs_gamma, abs_rz=abs_rz)


def mbcg(A, B, Minv=None, maxiter=None, reltol=1e-8, abstol=0.0, x0=None, dtype=np.float64):
    """p independent CG recurrences on the dense A (n x n) with right-hand sides B (n x p), preconditioner matrix Minv or None.  The
    products A P and Minv R are taken in `dtype` too (the matrix rounded to it, the accumulation numpy's for that type), as the device's are.
    Returns (X, info): alpha, beta (maxiter x p, 0 where frozen), iters, rz0, rr, active."""
    f8 = np.float64
    A, B = np.asarray(A, dtype=f8), np.asarray(B, dtype=dtype)
    At, Mt = A.astype(dtype), (None if Minv is None else np.asarray(Minv, dtype=f8).astype(dtype))
    n, p = B.shape
    maxiter = n if maxiter is None else maxiter
    X = np.zeros((n, p), dtype=dtype) if x0 is None else np.array(x0, dtype=dtype)
    R = B.copy() if x0 is None else (B - At @ X).astype(dtype)
    prec = None if Minv is None else (lambda Rn: (Mt @ Rn).astype(dtype))
    Z = R if prec is None else prec(R)
    P = Z.copy()
    rr = np.einsum("ij,ij->j", R.astype(f8), R.astype(f8))
    rz = np.einsum("ij,ij->j", R.astype(f8), Z.astype(f8))
    tol2 = np.maximum(reltol ** 2 * rr, abstol ** 2)
    active = rr > tol2
    iters = np.zeros(p, dtype=np.int64)
    alpha, beta = np.zeros((maxiter, p)), np.zeros((maxiter, p))
    rz0 = rz.copy()
    for it in range(maxiter):
        if not active.any():
            break
        AP = (At @ P).astype(dtype)
        s = step(X, R, P, AP, prec, None, rz, tol2, rr, active, iters, dtype)
        X, R, P, rz, rr, active, iters = s["X"], s["R"], s["P"], s["rz"], s["rr"], s["active"], s["iters"]
        alpha[it], beta[it] = s["alpha"], s["beta"]
    return X, dict(alpha=alpha, beta=beta, iters=iters, rz0=rz0, rr=rr, active=active)


def tridiagonal(alpha, beta, m):
    """The Lanczos matrix of one recurrence from its first m coefficients: T[i,i] = 1/α_i + β_{i-1}/α_{i-1}, T[i,i+1] = √β_i / α_i."""
    a, b = np.asarray(alpha, dtype=np.float64)[:m], np.asarray(beta, dtype=np.float64)[:m]
    T = np.zeros((m, m))
    for i in range(m):
        T[i, i] = 1.0 / a[i] + (b[i - 1] / a[i - 1] if i else 0.0)
        if i + 1 < m:
            T[i, i + 1] = T[i + 1, i] = np.sqrt(b[i]) / a[i]
    return T


def quadrature(T, f):
    """e1' f(T) e1 by the eigendecomposition."""
    lam, V = np.linalg.eigh(T)
    return float(np.sum(V[0] ** 2 * f(lam)))


def sym_fun(A, f):
    """f(A) of a symmetric matrix by the eigendecomposition."""
    lam, V = np.linalg.eigh(A)
    return (V * f(lam)) @ V.T
