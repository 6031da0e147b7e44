"""numpy restatements of the diagonally pivoted Cholesky recurrence (include/covgram.h: covgram_pivoted_cholesky) for the tests, no GPU:

  replay(M, piv)          the fp64 factor that FOLLOWS a given pivot sequence, with each step's greedy gap and the final residual diagonal;
  emulate(M, piv, dtype)  the same recurrence carried in `dtype`, with the fixed-order sums of the device kernel;
  woodbury(L, D)          the (D^-1, W, R) of (L L' + D)^-1 = D^-1 - W W', C = I + L' D^-1 L = R' R, W = D^-1 L R^-1.
"""
import numpy as np


def _columns(M, piv, cols, diag):
    """(columns M[:, piv] as an n x r array, diag(M)) from the matrix, or from the caller's columns and diagonal (large n: no n x n matrix)."""
    if M is not None:
        M = np.asarray(M, dtype=np.float64)
        return M[:, np.asarray(piv, dtype=np.int64)], np.diag(M).copy()
    return np.asarray(cols, dtype=np.float64), np.array(diag, dtype=np.float64)


def replay(M, piv, cols=None, diag=None):
    """(L, gaps, dres): L[:, k] is the pivoted-Cholesky column for pivot piv[k] in fp64 (rows in the original order);
    gaps[k] = max over the live residual diagonal - its value at piv[k] (0 for a greedy choice); dres = diag(M - L L') with exact zeros
    on the pivots.  M = None: the columns M[:, piv] and diag(M) are given instead of the matrix."""
    Mc, d = _columns(M, piv, cols, diag)
    n, r = Mc.shape[0], len(piv)
    live = np.ones(n, dtype=bool)
    L = np.zeros((n, r))
    gaps = np.zeros(r)
    for k, p in enumerate(piv):
        p = int(p)
        gaps[k] = d[live].max() - d[p]
        col = Mc[:, k] - L[:, :k] @ L[p, :k]
        L[:, k] = col / np.sqrt(d[p])
        d = d - L[:, k] ** 2
        live[p] = False
        d[~live] = 0.0
    return L, gaps, d


def _fma(a, b, c, dtype):
    """a b + c rounded once to dtype: exact for float32 up to a double rounding (the product of two float32 is exact in float64);
    float64 has no fused operation in numpy and takes two roundings."""
    if dtype == np.float32:
        return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def _fnma_square(l, d, dtype):
    """d - l l rounded once to dtype (float64: two roundings, as in _fma)."""
    if dtype == np.float32:
        l64 = l.astype(np.float64)
        return (d.astype(np.float64) - l64 * l64).astype(np.float32)
    return d - l * l


def emulate(M, piv, dtype, cols=None, diag=None):
    """(L, dres) of the same recurrence with every quantity held in `dtype`: the entries of M rounded to dtype, the sum
    sum_{j<k} L[i,j] L[p,j] by fused multiply-adds in the order j = 0 .. k-1 from zero, one subtraction, one division by the rounded
    square root of the residual diagonal at the pivot, dres[i] <- fma(-L[i,k], L[i,k], dres[i]), zero on the pivots so far."""
    dtype = np.dtype(dtype).type
    Mc, d = _columns(M, piv, cols, diag)
    A, d = Mc.astype(dtype), d.astype(dtype)
    n, r = A.shape[0], len(piv)
    L = np.zeros((n, r), dtype=dtype)
    for k, p in enumerate(piv):
        p = int(p)
        acc = np.zeros(n, dtype=dtype)
        for j in range(k):
            acc = _fma(L[:, j], L[p, j], acc, dtype)
        rs = np.sqrt(d[p])
        L[:, k] = (A[:, k] - acc) / rs
        d = _fnma_square(L[:, k], d, dtype)
        d[np.asarray(piv[:k + 1], dtype=np.int64)] = 0             # retired entries stay exactly zero
    return L, d


def woodbury(L, D):
    """(Dinv, W, R) with (L L' + diag(D))^-1 = diag(Dinv) - W W' and log det(L L' + diag(D)) = 2 sum log diag(R) + sum log D."""
    L = np.asarray(L, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    Dinv = 1.0 / D
    DL = Dinv[:, None] * L
    C = np.eye(L.shape[1]) + L.T @ DL
    R = np.linalg.cholesky(C).T                     # C = R' R, R upper
    W = np.linalg.solve(R.T, DL.T).T                # W R = D^-1 L
    return Dinv, W, R
