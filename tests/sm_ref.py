"""Shared by tests/test_gpu_sm.py (device) and tests/test_sm_bound_host.py (no GPU): the parameters, the fp64 reference by definition
and the ENTRYWISE error bound of a SpectralMixture Gramian, and an emulation of exactly rounded fp32 arithmetic in both forms a kernel
may take (per-point phases or a per-pair cosine).

    G_ij = sum_q w_q cos(2 pi mu_q . (x_i - y_j)) exp(-s_q,ij / 2),    s_q,ij = sum_k ((x_ik - y_jk) inv_l_qk)^2

Bound (a condition, not a measurement; TOL = matrix_cases.TOL = 1e-5 fp32 / 1e-12 fp64; tiny = smallest normal, since denormal results
may flush), with e_q = exp(-s_q / 2):

    bound_ij = TOL sum_q |w_q| e_q,ij ( max(1, s_q,ij / 20) + 2 pi sum_k |mu_qk| (|x_ik| + |y_jk|) ) + tiny

It extends the project's two conventions: the isotropic rule (the exp has condition number L = s / 2 in its argument, allowed at L / 10)
and the derivative rule for the argument of a profile (the phase 2 pi mu . (x - y) cancels, so its error scales with
sum_k |mu_k| (|x_k| + |y_k|) and reaches the entry through |d cos| <= 1).  The |x| + |y| form (not |x - y|) allows a kernel that
rounds the per-point phases mu . x and mu . y separately as well as one that forms mu . (x - y) per pair.  Data and parameters are
rounded to the case's dtype FIRST, as matrix_cases.reference_and_bound does; everything after that is fp64."""
import numpy as np

import matrix_cases as mc

F32, F64 = np.float32, np.float64
TOL = mc.TOL
tiny = mc.tiny


def params(rng, Q, d, scalar_l):
    """w = +-exp(0.5 N) with one negative weight when Q > 1, mu = +-exp(0.7 N) with mu_0 = 0, l = exp(0.5 N) (one per component if
    scalar_l, else one per component and dimension).  Returns (w[Q], mu[Q, d], l: Q numbers or Q length-d vectors)."""
    w = np.exp(0.5 * rng.standard_normal(Q))
    if Q > 1:
        w[Q // 2] = -w[Q // 2]
    mu = np.exp(0.7 * rng.standard_normal((Q, d))) * rng.choice([-1.0, 1.0], size=(Q, d))
    mu[0] = 0.0
    l = np.exp(0.5 * rng.standard_normal(Q if scalar_l else (Q, d)))
    return w, mu, l


def inv_l_of(l, d):
    """The Q x d inverse lengthscales of params()' l."""
    l = np.asarray(l, dtype=F64)
    return np.ascontiguousarray(1.0 / (np.repeat(l[:, None], d, axis=1) if l.ndim == 1 else l))


def rounded(dt, *arrays):
    return tuple(np.asarray(a, dtype=F64).astype(dt).astype(F64) for a in arrays)


def reference_and_bound(w, mu, inv_l, X, Y, dt):
    """(ref, bound) of every entry, n x m: parameters rounded to dt, X and Y as given (already of dtype dt), fp64 arithmetic, direct
    differences."""
    w, mu, inv_l = rounded(dt, w, mu, inv_l)
    Xd, Yd = X.astype(F64), Y.astype(F64)
    D = Xd[:, None, :] - Yd[None, :, :]                          # n x m x d
    D2 = D * D
    ref = np.zeros(D.shape[:2]); bound = np.zeros(D.shape[:2])
    aX, aY = np.abs(Xd), np.abs(Yd)
    for q in range(w.shape[0]):
        s = D2 @ (inv_l[q] ** 2)
        e = np.exp(-0.5 * s)
        ref += w[q] * np.cos(2 * np.pi * (D @ mu[q])) * e
        ph = 2 * np.pi * ((aX @ np.abs(mu[q]))[:, None] + (aY @ np.abs(mu[q]))[None, :])
        bound += np.abs(w[q]) * e * (np.maximum(1.0, s / 20.0) + ph)
    return ref, TOL[dt] * bound + tiny(dt)


worst_entry = mc.worst_entry


def _r(v):
    return np.asarray(v, dtype=F64).astype(F32)


def _fma(a, b, c):
    """One fp32 fused multiply-add (the fp64 product of two fp32 numbers is exact)."""
    return _r(a.astype(F64) * b.astype(F64) + c.astype(F64))


def emulate_f32(w, mu, inv_l, X, Y, form):
    """What exactly rounded fp32 arithmetic gives, entry by entry (X, Y fp32): differences, their squares, fused accumulation of
    s_q over the dimensions with the rounded coefficients inv_l^2, exp and cos / sin exact on their fp32 arguments and rounded once,
    fused accumulation over the components.
      form = "phase": u_qi = mu_q . x_i and v_qj = mu_q . y_j accumulated in fp32, reduced exactly to [-1/2, 1/2], and
                      cos(2 pi (u - v)) = cos u cos v + sin u sin v from the four rounded factors;
      form = "pair":  mu_q . (x_i - y_j) accumulated in fp32 per pair, reduced exactly, one cosine."""
    w32, mu32, il32 = _r(w), _r(mu), _r(inv_l)
    c32 = _r(il32.astype(F64) ** 2)
    n, m, d = X.shape[0], Y.shape[0], X.shape[1]
    R = [_r(X[:, k][:, None].astype(F64) - Y[:, k][None, :].astype(F64)) for k in range(d)]
    R2 = [_r(r.astype(F64) ** 2) for r in R]
    out = np.zeros((n, m), F32)

    def phase(P, q):
        u = np.zeros(P.shape[0], F32)
        for k in range(d):
            u = _fma(np.full(P.shape[0], mu32[q, k], F32), P[:, k], u)
        f = u.astype(F64) - np.rint(u.astype(F64))
        return _r(np.cos(2 * np.pi * f)), _r(np.sin(2 * np.pi * f))

    for q in range(w32.shape[0]):
        s = np.zeros((n, m), F32)
        for k in range(d):
            s = _fma(np.full((n, m), c32[q, k], F32), R2[k], s)
        e = _r(np.exp(-0.5 * s.astype(F64)))
        if form == "phase":
            cu, su = phase(X, q)
            cv, sv = phase(Y, q)
            ss = _r(su[:, None].astype(F64) * sv[None, :].astype(F64))
            ph = _fma(np.broadcast_to(cu[:, None], (n, m)), np.broadcast_to(cv[None, :], (n, m)), ss)
        else:
            u = np.zeros((n, m), F32)
            for k in range(d):
                u = _fma(np.full((n, m), mu32[q, k], F32), R[k], u)
            f = u.astype(F64) - np.rint(u.astype(F64))
            ph = _r(np.cos(2 * np.pi * f))
        g = _r(np.full((n, m), w32[q], F32).astype(F64) * ph.astype(F64))
        out = _fma(e, g, out)
    return out


# the clouds and parameters of the device test (n, m, d, Q, scalar lengthscale): every n, m, d and Q of the issue, both lengthscale
# forms at every d bucket, one column tile and many, one component chunk and eight
CASES = [
    (1, 193, 1, 1, True), (63, 193, 3, 3, False), (257, 193, 8, 32, False), (257, 1500, 16, 3, False), (63, 1500, 1, 32, True),
    (1, 1500, 3, 1, False), (257, 193, 3, 3, True), (63, 193, 8, 1, True), (257, 1500, 16, 32, True), (63, 1500, 8, 3, False),
    (1, 193, 16, 3, True), (257, 1500, 1, 3, False), (63, 193, 16, 32, False), (257, 1500, 3, 3, False),
]


def case_name(c, dt):
    n, m, d, Q, sc = c
    return f"n{n}-m{m}-d{d}-Q{Q}-{'iso' if sc else 'ard'}-{np.dtype(dt).name}"


def make_case(c, dt, seed=0x5A1):
    """(X, Y, w, mu, l, inv_l): the cloud of matrix_cases.iso_cloud (spread 0.8, shift 0.2, 8 far rows, 4 copied rows) and params()."""
    n, m, d, Q, sc = c
    rng = np.random.default_rng([seed, n, m, d, Q, int(sc)])
    X, Y = mc.iso_cloud(rng, n, m, d, dt)[:2]
    w, mu, l = params(rng, Q, d, sc)
    return X, Y, w, mu, l, inv_l_of(l, d)
