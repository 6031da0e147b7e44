"""Shared by tests/test_sm_input_grad_host.py (no GPU) and tests/test_gpu_sm_input_grad.py: the fp64 reference of
covgram_bilinear_input_grad_sm by definition, the error bound its results are held to, the cases of the device test (those of
sm_grad_ref) and an fp32 emulation of the kernel's own order of operations.

Reference (numpy fp64, on data and parameters rounded to the points' dtype FIRST, as sm_ref does): with W = U A', r = x_i - y_j by
direct differences, phi_q = 2 pi mu_q . r and e_q = exp(-1/2 sum_k (r_k inv_l_qk)^2),
    ref[i, c] = sum_j W_ij sum_q w_q e_q ( -2 pi mu_qc sin phi_q - inv_l_qc^2 r_c cos phi_q )
with sin phi := 0 where r = 0 (a coincident pair adds exactly nothing).  The derivative in the column points is the same call with the
roles swapped, (Y, X, A, U); the one-point-set case with both sides moving is call(X, X, U, A) + call(X, X, A, U).

Bound (a condition, not a fit).  TOL = matrix_cases.TOL, B_q = max(1, s_q / 20) + 2 pi sum_k |mu_qk| (|x_ik| + |y_jk|)
(the conventions of sm_ref and sm_grad_ref), |W| = |U| |A|', u = eps / 2, gamma_k = k u / (1 - k u), L = HANDOFF = 128:
    |dX_ic - ref_ic| <= sum_j |W|_ij b_ijc + (gamma_nvec + gamma_{2Q+2} + gamma_L) sum_j |W|_ij M_ijc + tiny
    b_ijc = TOL sum_q |w_q| e_q ( 2 pi |mu_qc| (B_q + 1) + inv_l_qc^2 |r_c| (B_q + 2) )
    M_ijc = sum_q |w_q| e_q ( 2 pi |mu_qc| |sin phi_q| + inv_l_qc^2 |r_c| |cos phi_q| )
gamma_nvec is the error of W_ij formed by nvec fused multiply-adds, gamma_{2Q+2} covers the sums over the components in the working
precision, gamma_L the lane's own sum of at most L pairs before fp64 takes over.  There is no butterfly term: the row is lane-private.
In fp32 the kernel forms e_q = h^2, h = exp2(-t_q / 2): the error of h enters e_q twice and (W h) h has one more rounding than W e, about
3 u |W e_q| per component more than a single exponential — inside the TOL (B_q + 1) |W e_q| >= 335 u |W e_q| that b allows for it.
Nothing here is fitted to a device."""
import numpy as np

import matrix_cases as mc
import sm_grad_ref as gr
import sm_ref as sr

F32, F64 = np.float32, np.float64
TOL = mc.TOL
HANDOFF = gr.HANDOFF     # BG_L of csrc/bilin_common.hpp
LANE_COLS, TILE = gr.LANE_COLS, gr.TILE   # fp32: 16 columns per lane and tile, 64-column tiles, 4 waves
CHUNK = 4                # SM_QC of csrc/sm_common.hpp: components per pass over the pairs

# the main sweep of the device test: sm_grad_ref's
SHAPES, DIMS, COMPONENTS, NVECS = gr.SHAPES, gr.DIMS, gr.COMPONENTS, gr.NVECS
make_case, weights = gr.make_case, gr.weights


def pair_terms(w, mu, inv_l, X, Y, dt):
    """(Ts, Tc, b, M), each d x n x m: the sine half and the cosine half of the per-pair quantity (their sum multiplies W_ij), the
    per-pair bound b and the magnitude M of the module docstring — parameters rounded to dt, X and Y as given (already of dtype dt)."""
    w, mu, inv_l = sr.rounded(dt, w, mu, inv_l)
    Xd, Yd = X.astype(F64), Y.astype(F64)
    D = Xd[:, None, :] - Yd[None, :, :]                          # n x m x d
    D2 = D * D
    Dt = np.ascontiguousarray(np.moveaxis(D, 2, 0))              # d x n x m
    aDt = np.abs(Dt)
    zero = D2.sum(axis=2) == 0
    aX, aY = np.abs(Xd), np.abs(Yd)
    Ts = np.zeros_like(Dt); Tc = np.zeros_like(Dt); b = np.zeros_like(Dt); M = np.zeros_like(Dt)
    for q in range(w.shape[0]):
        s = D2 @ (inv_l[q] ** 2)
        e = np.exp(-0.5 * s)
        phi = 2 * np.pi * (D @ mu[q])
        c, sn = np.cos(phi), np.where(zero, 0.0, np.sin(phi))
        B = np.maximum(1.0, s / 20.0) + 2 * np.pi * ((aX @ np.abs(mu[q]))[:, None] + (aY @ np.abs(mu[q]))[None, :])
        awe = abs(w[q]) * e
        fs = (2 * np.pi * np.abs(mu[q]))[:, None, None]           # d x 1 x 1
        fc = (inv_l[q] ** 2)[:, None, None]
        Ts += (-2 * np.pi * w[q] * mu[q])[:, None, None] * (e * sn)[None]
        Tc -= (w[q] * fc) * Dt * (e * c)[None]
        b += TOL[dt] * (fs * (awe * (B + 1))[None] + fc * aDt * (awe * (B + 2))[None])
        M += fs * (awe * np.abs(sn))[None] + fc * aDt * (awe * np.abs(c))[None]
    return Ts, Tc, b, M


def reference_and_bound(w, mu, inv_l, X, Y, weight_sets, dt, halves=False):
    """[(ref, bound)] for every (U, A) of `weight_sets`, each (n, d): the per-pair quantities are formed once and shared.  halves = True:
    [(ref, bound, sine half, cosine half)], ref = the sum of the two halves."""
    eps = float(np.finfo(dt).eps); u = eps / 2
    gam = lambda k: k * u / (1 - k * u)
    Q = np.asarray(w).shape[0]
    Ts, Tc, b, M = pair_terms(w, mu, inv_l, X, Y, dt)
    out = []
    for U, A in weight_sets:
        U2 = U.reshape(U.shape[0], -1).astype(F64); A2 = A.reshape(A.shape[0], -1).astype(F64)
        W = U2 @ A2.T; Wabs = np.abs(U2) @ np.abs(A2).T
        g = gam(U2.shape[1]) + gam(2 * Q + 2) + gam(HANDOFF)
        hs = np.einsum("cij,ij->ic", Ts, W); hc = np.einsum("cij,ij->ic", Tc, W)
        bound = np.einsum("cij,ij->ic", b, Wabs) + g * np.einsum("cij,ij->ic", M, Wabs) + mc.tiny(dt)
        out.append((hs + hc, bound, hs, hc) if halves else (hs + hc, bound))
    return out


def reference(w, mu, inv_l, X, Y, U, A, dt=F64):
    return reference_and_bound(w, mu, inv_l, X, Y, [(U, A)], dt)[0][0]


def magnitude(w, mu, inv_l, X, Y, U, A):
    """sum_j |W|_ij M_ijc per row and dimension: what the finite-difference checks are relative to."""
    M = pair_terms(w, mu, inv_l, X, Y, F64)[3]
    return np.einsum("cij,ij->ic", M, np.abs(U.reshape(U.shape[0], -1).astype(F64)) @ np.abs(A.reshape(A.shape[0], -1).astype(F64)).T)


def form(w, mu, inv_l, X, Y, W):
    """F(X, Y) = sum_ij W_ij sum_q w_q cos phi_q e_q in fp64."""
    D = X[:, None, :] - Y[None, :, :]
    return float(sum((W * w[q] * np.cos(2 * np.pi * (D @ mu[q])) * np.exp(-0.5 * ((D * D) @ (inv_l[q] ** 2)))).sum() for q in range(len(w))))


def worst(got, ref, bound):
    """(err / bound, flat index) of the worst output; a non-finite output is infinitely wrong."""
    return gr.worst(np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1), np.asarray(bound).reshape(-1))


# ---- fp32 emulation ------------------------------------------------------------------------------------------------------------------
_r32 = gr._r32


def emulate_f32(w, mu, inv_l, X, Y, U, A):
    """The (n, d) result an exactly rounded fp32 evaluation in the kernel's order gives (X, Y, U, A fp32): the per-point phases
    accumulated in fp64, reduced exactly, their cos / sin rounded once; W_ij as nvec fused multiply-adds; differences; the exponent by
    fused accumulation of the rounded coefficients log2(e) / (2 l^2) times the rounded squares (one lengthscale per component: the
    coefficient times the fused sum of squares); the exponential split as the kernel splits it in fp32, h = exp2(-t / 2) exact on
    its fp32 argument and rounded once, W e = (W h) h (no product before the last can leave the normal range: the hardware exp2
    flushes a denormal result, and a far row's whole sum lies there); gc = (W e) cos phi and
    gs = (W e) sin phi with cos phi = fma(cu, cv, su sv) and sin phi = fma(su, cv, -cu sv), 1 and 0 at r = 0; then per chunk of CHUNK
    components and dimension the two fma chains S = sum_q gsin_qc gs_q and C = sum_q gcos_qc gc_q over the rounded coefficients
    -2 pi w mu and w inv_l^2 (one lengthscale per component: one chain C per pair), the pair's value fma(-r_c, C, S), and each lane's
    sequential fp32 sum of its pairs' values — row i; within a 64-column tile the 16 columns of its wave; HANDOFF / 16 = 8 tiles —
    and fp64 from there: the hand-offs of a lane in order, chunk after chunk, then the four waves in order.  (One column chunk: the GPU
    test's clouds are narrower than a hand-off interval.)"""
    w32, mu32, il32 = sr.rounded(F32, w, mu, inv_l)
    Q = w32.shape[0]
    n, m, d = X.shape[0], Y.shape[0], X.shape[1]
    iso = bool(np.all(il32 == il32[:, :1]))
    c32 = _r32(0.72134752044448170368 * il32 * il32)
    gsin = _r32(-6.283185307179586476925 * w32[:, None] * mu32)
    gcos = _r32(w32[:, None] * il32 * il32)
    Xd, Yd = X.astype(F64), Y.astype(F64)
    U2 = U.reshape(n, -1).astype(F64); A2 = A.reshape(m, -1).astype(F64)
    W = np.zeros((n, m))
    for t in range(U2.shape[1]):
        W = _r32(U2[:, t][:, None] * A2[:, t][None, :] + W)
    R = np.stack([_r32(Xd[:, k][:, None] - Yd[:, k][None, :]) for k in range(d)])      # d x n x m
    R2 = _r32(R * R)
    zero = ~R.any(axis=0)
    ssum = np.zeros((n, m))
    for k in range(d):
        ssum = _r32(R[k] * R[k] + ssum)

    def phase(P, q):
        uu = P @ mu32[q]
        f = uu - np.rint(uu)
        return _r32(np.cos(2 * np.pi * f)), _r32(np.sin(2 * np.pi * f))

    gc, gs = [], []
    for q in range(Q):
        if iso:
            t = _r32(c32[q, 0] * ssum)
        else:
            t = np.zeros((n, m))
            for k in range(d):
                t = _r32(c32[q, k] * R2[k] + t)
        h = _r32(np.exp2(-0.5 * t))                                 # the half exponent has the bits of t / 2: its coefficients are halved
        we = _r32(_r32(W * h) * h)
        cu, su = phase(Xd, q)
        cv, sv = phase(Yd, q)
        cosv = np.where(zero, 1.0, _r32(cu[:, None] * cv[None, :] + _r32(su[:, None] * sv[None, :])))
        sinv = np.where(zero, 0.0, _r32(su[:, None] * cv[None, :] - _r32(cu[:, None] * sv[None, :])))
        gc.append(_r32(we * cosv)); gs.append(_r32(we * sinv))

    group, waves = HANDOFF // LANE_COLS, TILE // LANE_COLS
    mpad = -(-m // (TILE * group)) * (TILE * group)
    shp = (n, mpad // (TILE * group), group, waves, LANE_COLS)      # [row, hand-off, tile, wave, column]

    def lanes(Mx):
        P = np.zeros((n, mpad)); P[:, :m] = Mx
        return P.reshape(shp).transpose(0, 1, 3, 2, 4).reshape(n, shp[1], waves, group * LANE_COLS)

    out = np.empty((n, d))
    for c in range(d):
        tot = np.zeros((n, waves))
        for q0 in range(0, Q, CHUNK):
            S = np.zeros((n, m)); Cc = np.zeros((n, m))
            for q in range(q0, min(q0 + CHUNK, Q)):
                S = _r32(gsin[q, c] * gs[q] + S)
                Cc = _r32(gcos[q, 0 if iso else c] * gc[q] + Cc)
            vl = lanes(_r32(S - R[c] * Cc))
            acc = np.zeros(vl.shape[:-1])
            for t in range(vl.shape[-1]):
                acc = _r32(acc + vl[..., t])
            for h in range(acc.shape[1]):
                tot = tot + acc[:, h, :]
        row = tot[:, 0]
        for wv in range(1, waves):
            row = row + tot[:, wv]
        out[:, c] = row
    return out
