"""Shared by tests/test_input_grad_host.py (no GPU) and tests/test_gpu_input_grad.py: the fp64 reference of covgram_bilinear_input_grad,
the error bound its results are held to, and an fp32 emulation of the kernel's own order of operations.

Reference (numpy fp64, on the data as rounded to the points' dtype): with W = U A', S the squared distances by direct differences,
    ref[i, c] = sum_j W_ij Q_ij,   Q_ij = 2 d1_ij (x_ic - y_jc),
d1 = dk/dS and d2 = d2k/dS2 from oracle.profile_derivatives, both zeroed where S = 0 (a coincident pair adds nothing).  The derivative in
the column points is the same call with the roles swapped, reference(o, ko, Y, X, A, U); the symmetric case (Y = X, both sides moving) is
reference(o, ko, X, X, U, A) + reference(o, ko, X, X, A, U).

Bound, per row i and dimension c; eps = the dtype's machine epsilon, u = eps / 2, gamma_k = k u / (1 - k u):
    |dX_ic - ref_ic| <= sum_j ( |W|_ij b_ij + gamma_nvec |W|_ij |Q_ij| )  +  gamma_L sum_j |W|_ij |Q_ij|  +  tiny
    b_ij = eps ( (d + 2) / 2 |2 d2_ij (x_ic - y_jc)| S_ij  +  (C_EVAL q + 2 + C_ARG E_ij) |Q_ij| )
  * |W| = |U| |A|' bounds |W_ij|, gamma_nvec the error of W_ij formed by nvec fused multiply-adds;
  * the first term of b_ij: S by direct differences carries (d + 2) roundings of relative size u, which reach Q through dQ/dS;
  * C_EVAL, C_ARG and E_ij (the magnitude of the exponents the profile forms, with the gamma-exponential's extra term) are those of
    bilin_grad_ref; the 2 stands for the rounded difference x_ic - y_jc and its product with W dk/ds;
  * gamma_L, L = HANDOFF = 128: a lane adds at most L pairs of its own row in the working precision, everything after is fp64.  There is
    no butterfly term: the row is lane-private.
Nothing here is fitted to a device."""
import numpy as np

import bilin_grad_ref as br
from bilin_grad_ref import C_ARG, C_EVAL, HANDOFF, _r32

F32, F64 = np.float32, np.float64
LANE_COLS, TILE = br.LANE_COLS, br.TILE        # fp32: 16 columns per lane and tile, 64-column tiles, 4 waves


def _weights(U, A):
    U2 = U.reshape(U.shape[0], -1).astype(F64); A2 = A.reshape(A.shape[0], -1).astype(F64)
    return U2 @ A2.T, np.abs(U2) @ np.abs(A2).T, U2.shape[1]


def reference_and_bound(o, ko, X, Y, U, A, dt=F64):
    """(ref, bound), both (n, d): the gradient in the row points X of sum_ij W_ij k(x_i, y_j) and the bound of the module docstring."""
    eps = float(np.finfo(dt).eps); u = eps / 2
    n, d = X.shape
    Xd, Yd = X.astype(F64), Y.astype(F64)
    W, Wabs, nvec = _weights(U, A)
    S = o.pair_arg(ko, Xd, Yd)
    zero = S == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        _, d1, d2 = o.profile_derivatives(ko, S, dt)
    d1 = np.where(zero, 0.0, d1); d2 = np.where(zero, 0.0, d2)
    E = br.pair_quantities(o, ko, X, Y, 0, dt)[1]
    gam = lambda k: k * u / (1 - k * u)
    ref = np.empty((n, d)); bound = np.empty((n, d))
    for c in range(d):
        df = Xd[:, c][:, None] - Yd[:, c][None, :]
        Q = 2.0 * d1 * df
        b = eps * ((d + 2) / 2 * np.abs(2.0 * d2 * df) * S + (C_EVAL * ko.power + 2.0 + C_ARG * E) * np.abs(Q))
        WQ = (Wabs * np.abs(Q)).sum(axis=1)
        ref[:, c] = (W * Q).sum(axis=1)
        bound[:, c] = (Wabs * b).sum(axis=1) + (gam(nvec) + gam(HANDOFF)) * WQ + np.finfo(dt).tiny
    return ref, bound


def reference(o, ko, X, Y, U, A, dt=F64):
    return reference_and_bound(o, ko, X, Y, U, A, dt)[0]


def magnitude(o, ko, X, Y, U, A):
    """sum_j |W|_ij |Q_ij| per row and dimension: what the finite-difference checks are relative to."""
    Xd, Yd = X.astype(F64), Y.astype(F64)
    _, Wabs, _ = _weights(U, A)
    S = o.pair_arg(ko, Xd, Yd)
    with np.errstate(divide="ignore", invalid="ignore"):
        d1 = np.where(S == 0, 0.0, o.profile_derivatives(ko, S, F64)[1])
    return np.stack([(Wabs * np.abs(2.0 * d1 * (Xd[:, c][:, None] - Yd[:, c][None, :]))).sum(axis=1) for c in range(X.shape[1])], axis=1)


def emulate_f32(o, ko, X, Y, U, A):
    """The (n, d) result an exactly rounded fp32 evaluation in the kernel's order gives: direct differences and FMA accumulation of S over
    the dimensions, the scaled argument, dk/ds rounded once per factor (as bilin_grad_ref.emulate_f32), W_ij as nvec fused multiply-adds,
    gw = W dk/ds rounded, then each lane's sequential fp32 FMA accumulation acc = fma(gw, x_c - y_c, acc) over its pairs — row i; within a
    64-column tile the 16 columns of its wave; HANDOFF / 16 = 8 tiles — and fp64 from there: the hand-offs of a wave in order, the four
    waves in order, the factor 2 last.  (One column chunk: the GPU test's clouds are narrower than a hand-off interval.)"""
    n, m = X.shape[0], Y.shape[0]
    d = X.shape[1]
    X = X.astype(F32); Y = Y.astype(F32)
    U2 = U.reshape(n, -1).astype(F32); A2 = A.reshape(m, -1).astype(F32)
    S = np.zeros((n, m))
    diffs = []
    for c in range(d):
        df = _r32(X[:, c][:, None].astype(F64) - Y[:, c][None, :].astype(F64))
        diffs.append(df)
        S = _r32(df * df + S)
    W = np.zeros((n, m))
    for t in range(U2.shape[1]):
        W = _r32(U2[:, t][:, None].astype(F64) * A2[:, t][None, :].astype(F64) + W)
    g2 = _r32(_r32(1.0 / ko.lengthscale) ** 2)
    s = _r32(S * g2)
    k1 = o.Kernel(ko.family, p=ko.p, param=ko.param, power=ko.power)
    with np.errstate(divide="ignore", invalid="ignore"):
        d1 = o.profile_derivatives(k1, s, F32)[1]
    sc = _r32(ko.scale)
    ds = np.where(s == 0, 0.0, _r32(_r32(_r32(d1) * g2) * sc))
    gw = _r32(W * ds)
    group = HANDOFF // LANE_COLS
    waves = TILE // LANE_COLS
    mpad = -(-m // (TILE * group)) * (TILE * group)
    shp = (n, mpad // (TILE * group), group, waves, LANE_COLS)      # [row, hand-off, tile, wave, column]

    def lanes(M):
        P = np.zeros((n, mpad)); P[:, :m] = M
        return P.reshape(shp).transpose(0, 1, 3, 2, 4).reshape(n, shp[1], waves, group * LANE_COLS)
    gl = lanes(gw)
    out = np.empty((n, d))
    for c in range(d):
        dl = lanes(diffs[c])
        acc = np.zeros(gl.shape[:-1])
        for t in range(gl.shape[-1]):
            acc = _r32(gl[..., t] * dl[..., t] + acc)
        tot = np.zeros((n, waves))
        for h in range(acc.shape[1]):
            tot = tot + acc[:, h, :]
        row = tot[:, 0]
        for w in range(1, waves):
            row = row + tot[:, w]
        out[:, c] = 2.0 * row
    return out
