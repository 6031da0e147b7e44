"""Shared by tests/test_sm_grad_host.py (no GPU) and tests/test_gpu_sm_grad.py: the fp64 reference of covgram_bilinear_grad_sm by
definition, the error bound its results are held to, the cases of the device test, and an fp32 emulation of the kernel's own order
of operations.

Reference (numpy fp64, on data and parameters rounded to the points' dtype FIRST, as sm_ref does): with W = U A', r = x_i - y_j by
direct differences, phi_q = 2 pi mu_q . r, s_q = sum_k (r_k inv_l_qk)^2 and e_q = exp(-s_q / 2), component-major:
    out[q (1 + 2d)]             = sum_ij W_ij cos phi_q e_q                      (dF/dw_q; not multiplied by w_q)
    out[q (1 + 2d) + 1 + k]     = sum_ij W_ij (-2 pi w_q) r_k sin phi_q e_q      (dF/dmu_qk)
    out[q (1 + 2d) + 1 + d + k] = sum_ij W_ij w_q cos phi_q e_q r_k^2            (E_qk; dF/d(inv_l_qk^2) = -E_qk / 2)

Bound (a condition, not a fit).  TOL = matrix_cases.TOL, B_q = max(1, s_q / 20) + 2 pi sum_k |mu_qk| (|x_ik| + |y_jk|) (the conventions
of sm_ref: the exponential's condition number allowed at a tenth, the phase's cancellation), |W| = |U| |A|', u = eps / 2 and
gamma_k = k u / (1 - k u); with Q_ij an output's per-pair quantity:
    |out - ref| <= sum_ij |W|_ij b_ij + (gamma_nvec + gamma_{L+6}) sum_ij |W|_ij |Q_ij| + tiny
    b(dw)    = TOL e_q B_q
    b(dmu_k) = TOL |w_q| 2 pi |r_k| e_q (B_q + 1)
    b(E_k)   = TOL |w_q| r_k^2 e_q (B_q + 2)
gamma_nvec is the error of W_ij formed by nvec fused multiply-adds; gamma_{L+6}: a lane adds L = HANDOFF pairs in the working
precision, then 6 butterfly steps; everything after is fp64."""
import numpy as np

import matrix_cases as mc
import sm_ref as sr

F32, F64 = np.float32, np.float64
TOL = mc.TOL
HANDOFF = 128            # BG_L of csrc/bilin_common.hpp, the hand-off constant of smg_pair_kernel (csrc/sm_grad.hip)
LANE_COLS, TILE, GROUP = 16, 64, 8   # fp32: columns per lane and tile, tile edge, tiles per hand-off (HANDOFF = LANE_COLS * GROUP)

# the main sweep of the device test
SHAPES = [(257, 130), (63, 193), (1, 193), (257, 1)]
DIMS = [1, 3, 8, 16]
COMPONENTS = [1, 3, 5, 32]           # one chunk, a ragged second chunk (fp32: 4 + 1; fp64: 2 + 2 + 1), the maximum
NVECS = [1, 3, 17, 32]


def make_case(n, m, d, Q, scalar_l, dt, seed=0x5A6):
    """(X, Y, w, mu, l, inv_l): the cloud of matrix_cases.iso_cloud and the parameters of sm_ref.params (one negative weight, mu_0 = 0)."""
    rng = np.random.default_rng([seed, n, m, d, Q, int(scalar_l)])
    X, Y = mc.iso_cloud(rng, n, m, d, dt)[:2]
    w, mu, l = sr.params(rng, Q, d, scalar_l)
    return X, Y, w, mu, l, sr.inv_l_of(l, d)


def weights(n, m, nvec, dt, seed=0x5A7):
    rng = np.random.default_rng([seed, n, m, nvec])
    return rng.standard_normal((n, nvec)).astype(dt), rng.standard_normal((m, nvec)).astype(dt)


def pair_quantities(w, mu, inv_l, X, Y, dt):
    """Per component q: (Qs, bs), each (1 + 2d) x n x m — the per-pair quantities of the component's outputs and their per-pair
    bounds b — from parameters rounded to dt and X, Y as given (already of dtype dt).  A generator: a component at a time."""
    w, mu, inv_l = sr.rounded(dt, w, mu, inv_l)
    Xd, Yd = X.astype(F64), Y.astype(F64)
    D = Xd[:, None, :] - Yd[None, :, :]                          # n x m x d
    D2 = D * D
    Dt, D2t = np.ascontiguousarray(np.moveaxis(D, 2, 0)), np.ascontiguousarray(np.moveaxis(D2, 2, 0))   # d x n x m
    aDt = np.abs(Dt)
    aX, aY = np.abs(Xd), np.abs(Yd)
    d = X.shape[1]
    for q in range(w.shape[0]):
        s = D2 @ (inv_l[q] ** 2)
        e = np.exp(-0.5 * s)
        phi = 2 * np.pi * (D @ mu[q])
        c, sn = np.cos(phi), np.sin(phi)
        B = np.maximum(1.0, s / 20.0) + 2 * np.pi * ((aX @ np.abs(mu[q]))[:, None] + (aY @ np.abs(mu[q]))[None, :])
        Qs = np.empty((1 + 2 * d,) + s.shape); bs = np.empty_like(Qs)
        Qs[0] = c * e
        bs[0] = TOL[dt] * e * B
        np.multiply((-2 * np.pi * w[q]) * sn * e, Dt, out=Qs[1:1 + d])
        np.multiply((TOL[dt] * abs(w[q]) * 2 * np.pi) * e * (B + 1), aDt, out=bs[1:1 + d])
        np.multiply(w[q] * c * e, D2t, out=Qs[1 + d:])
        np.multiply((TOL[dt] * abs(w[q])) * e * (B + 2), D2t, out=bs[1 + d:])
        yield Qs, bs


def reference_and_bound(w, mu, inv_l, X, Y, weight_sets, dt):
    """[(ref, bound)] for every (U, A) of `weight_sets`, each ncomp (1 + 2d) numbers: the per-pair quantities are formed once and shared."""
    eps = float(np.finfo(dt).eps); u = eps / 2
    gam = lambda k: k * u / (1 - k * u)
    nm = X.shape[0] * Y.shape[0]
    Ws, Wabs, g = [], [], []
    for U, A in weight_sets:
        U2 = U.reshape(U.shape[0], -1).astype(F64); A2 = A.reshape(A.shape[0], -1).astype(F64)
        Ws.append((U2 @ A2.T).reshape(nm)); Wabs.append((np.abs(U2) @ np.abs(A2).T).reshape(nm))
        g.append(gam(U2.shape[1]) + gam(HANDOFF + 6))
    Ws, Wabs, g = np.stack(Ws, axis=1), np.stack(Wabs, axis=1), np.array(g)
    refs, bounds = [], []
    for Qs, bs in pair_quantities(w, mu, inv_l, X, Y, dt):
        Qf, bf = Qs.reshape(Qs.shape[0], nm), bs.reshape(bs.shape[0], nm)
        refs.append(Qf @ Ws)
        bounds.append(bf @ Wabs + g[None, :] * (np.abs(Qf) @ Wabs) + mc.tiny(dt))
    refs, bounds = np.concatenate(refs, axis=0), np.concatenate(bounds, axis=0)
    return [(refs[:, t].copy(), bounds[:, t].copy()) for t in range(len(weight_sets))]


def reference(w, mu, inv_l, X, Y, U, A, dt=F64):
    return reference_and_bound(w, mu, inv_l, X, Y, [(U, A)], dt)[0][0]


def worst(got, ref, bound):
    """(err / bound, index) of the worst output; a non-finite output is infinitely wrong."""
    with np.errstate(invalid="ignore"):
        r = np.where(np.isfinite(got), np.abs(got - ref) / bound, np.inf)
    i = int(np.argmax(r))
    return float(r[i]), i


# ---- fp32 emulation ------------------------------------------------------------------------------------------------------------------
def _r32(a):
    return np.asarray(a, F64).astype(F32).astype(F64)


def _lane_sums(a, b, n, m):
    """sum_ij in the lanes' order of fma(a, b, acc) (b None: acc + a), for stacks a, b of shape (..., n, m) holding fp32 values: lane =
    (row, wave) takes the 16 columns of its wave in every 64-column tile, GROUP tiles between hand-offs (one column chunk: the shapes of
    the device test are not split), then the 6-step butterfly over the 64 rows of the tile; fp64 from there."""
    lead = a.shape[:-2]
    npad = -(-n // TILE) * TILE; mpad = -(-m // (TILE * GROUP)) * (TILE * GROUP)
    def lanes(t):
        p = np.zeros(lead + (npad, mpad)); p[..., :n, :m] = t
        shp = lead + (npad // TILE, TILE, mpad // (TILE * GROUP), GROUP, TILE // LANE_COLS, LANE_COLS)
        k = len(lead)
        p = p.reshape(shp).transpose(tuple(range(k)) + (k, k + 2, k + 4, k + 1, k + 3, k + 5))
        return p.reshape(p.shape[:k + 4] + (GROUP * LANE_COLS,))
    al = lanes(a); bl = None if b is None else lanes(b)
    acc = np.zeros(al.shape[:-1])
    for t in range(al.shape[-1]):
        if not al[..., t].any():                                    # columns beyond the set: an exact zero is added
            continue
        acc = _r32(acc + al[..., t]) if bl is None else _r32(al[..., t] * bl[..., t] + acc)
    for o_ in (32, 16, 8, 4, 2, 1):                                 # the same sum in every lane: a + b == b + a
        acc = _r32(acc + acc[..., np.arange(TILE) ^ o_])
    return acc[..., 0].reshape(lead + (-1,)).sum(-1)


def emulate_f32(w, mu, inv_l, X, Y, U, A):
    """The outputs an exactly rounded fp32 evaluation in the kernel's order gives (X, Y, U, A fp32): the per-point phases accumulated in
    fp64, reduced exactly, their cos / sin rounded once; differences, squares, the exponent's fused accumulation with the rounded
    coefficients log2(e) / (2 l^2), exp2 exact on its fp32 argument and rounded once; W_ij as nvec fused multiply-adds; W e, then the
    products with cos phi = fma(cu, cv, su sv) and sin phi = fma(su, cv, -cu sv); each lane's sequential fp32 accumulation over its pairs
    (_lane_sums), the butterfly, and fp64 from there."""
    w32, mu32, il32 = sr.rounded(F32, w, mu, inv_l)
    c32 = _r32(0.72134752044448170368 * il32 * il32)
    n, m, d = X.shape[0], Y.shape[0], X.shape[1]
    Xd, Yd = X.astype(F64), Y.astype(F64)
    U2 = U.reshape(n, -1).astype(F64); A2 = A.reshape(m, -1).astype(F64)
    W = np.zeros((n, m))
    for t in range(U2.shape[1]):
        W = _r32(U2[:, t][:, None] * A2[:, t][None, :] + W)
    R = np.stack([_r32(Xd[:, k][:, None] - Yd[:, k][None, :]) for k in range(d)])      # d x n x m
    R2 = _r32(R * R)
    zero = R2.sum(0) == 0

    def phase(P, q):
        uu = P @ mu32[q]
        f = uu - np.rint(uu)
        return _r32(np.cos(2 * np.pi * f)), _r32(np.sin(2 * np.pi * f))

    out = []
    for q in range(w32.shape[0]):
        t = np.zeros((n, m))
        for k in range(d):
            t = _r32(c32[q, k] * R2[k] + t)
        we = _r32(W * _r32(np.exp2(-t)))
        cu, su = phase(Xd, q)
        cv, sv = phase(Yd, q)
        cosv = _r32(cu[:, None] * cv[None, :] + _r32(su[:, None] * sv[None, :]))
        cosv = np.where(zero, 1.0, cosv)
        sinv = _r32(su[:, None] * cv[None, :] - _r32(cu[:, None] * sv[None, :]))
        gc, gs = _r32(we * cosv), _r32(we * sinv)
        o0 = _lane_sums(gc, None, n, m)
        om = _lane_sums(np.broadcast_to(gs, R.shape), R, n, m)
        oe = _lane_sums(np.broadcast_to(gc, R.shape), R2, n, m)
        out += [o0] + list(-2 * np.pi * w32[q] * om) + list(w32[q] * oe)
    return np.array(out, dtype=F64)
