"""Shared by tests/test_bilin_grad_host.py (no GPU) and tests/test_gpu_bilin_grad.py: the fp64 reference of covgram_bilinear_grad, the
error bound its results are held to, and an fp32 emulation of the kernel's own order of operations.

Reference (numpy fp64, on the data as rounded to the points' dtype): with W = U A', S the squared distances by direct differences,
    out[0] = sum W k(S),  out[1] = sum W dk/dparam,  out[2 + c] = sum W (dk/dS) (x_c - y_c)^2   (per_dim; else out[2] = sum W (dk/dS) S),
k, dk/dS from oracle.profile_derivatives, a pair with S = 0 adding nothing to out[2 ..]; dk/dparam from the closed forms
    RQ:  phi (s / (2 alpha + s) - log1p(s / (2 alpha))),   gamma-exponential:  -1/4 phi s^(gamma/2) log s  (0 at s = 0),
    IMQ: -c (s + c^2)^(-3/2),   s = S / l^2,   chained through scale phi^q as  scale q phi^(q-1) dphi/dparam.

Bound (eps = the dtype's machine epsilon, u = eps / 2).  For each output, with Q_ij its per-pair quantity:
    |out - ref| <= sum_ij ( |W|_ij b_ij + w_ij |Q_ij| )  +  gamma_{L+6} sum_ij |W|_ij |Q_ij|  +  tiny
  * |W| = |U| |A|' bounds |W_ij|, and w_ij = gamma_nvec |W|_ij the error of W_ij formed by nvec fused multiply-adds;
  * b_ij = eps ( (d + 2) / 2 |dQ/dS| S  +  (C_EVAL q + extra + C_ARG E_ij) M_ij ):
      - S by direct differences carries (d + 2) roundings of relative size u (difference, square, d - 1 additions; all terms
        positive), which reach Q through dQ/dS;
      - E_ij = -ln(|k| / |k(0)|) (+ |gamma/2 ln s| for the gamma-exponential) is the magnitude of the exponents the profile forms: an
        exponent of size E rounded once moves the result by E u; C_ARG = 4 such roundings at most (scaling by 1 / l^2, the constant
        log2 e, the product with alpha or gamma / 2, the range reduction of the exponential);
      - C_EVAL = 16 bounds the remaining rounded operations of a closed form (square root, reciprocal, the hardware exp2 / log2 at
        1 ulp, a Horner polynomial with positive coefficients up to degree 8, the chain-rule products), times the Power exponent q;
        `extra` = 1 or 2 for the product with S or (x_c - y_c)^2 and its square;
      - M_ij = |Q_ij|, except where the closed form subtracts or where log s passes through zero: RQ's dk/dalpha uses
        |k| (s / (2 alpha + s) + log1p(s / (2 alpha))), the gamma-exponential's dk/dgamma uses 1/4 |k| s^(gamma/2) (|log s| + 1);
  * gamma_{L+6}: a lane adds L = HANDOFF pairs in the working precision, then 6 butterfly steps; everything after is fp64.
dQ/dS of the parameter derivatives is taken by a central difference of the closed form in fp64 (a bound needs no more).
Nothing here is fitted to a device."""
import numpy as np

F32, F64 = np.float32, np.float64
HANDOFF = 128            # BG_L of csrc/bilin_grad.hip: pairs a lane adds before the fp64 hand-off
LANE_COLS, TILE, GROUP = 16, 64, 8   # columns per lane and tile, tile edge, tiles per hand-off (HANDOFF = LANE_COLS * GROUP)
C_EVAL, C_ARG = 16.0, 4.0


def unit_phi(o, ko, s):
    """phi of the bare profile (no scale, power, lengthscale) at the scaled argument s."""
    return o.profile(o.Kernel(ko.family, p=ko.p, param=ko.param), s)


def param_parts(o, ko, S):
    """(dk/dparam, M) per pair: the closed form and the magnitude its evaluation error scales with."""
    S = np.asarray(S, F64)
    s = S / ko.lengthscale ** 2
    phi = unit_phi(o, ko, s)
    q = ko.power
    chain = ko.scale * q * phi ** (q - 1)
    if ko.family == o.RQ:
        a = ko.param
        t1, t2 = s / (2 * a + s), np.log1p(s / (2 * a))
        return chain * phi * (t1 - t2), np.abs(chain * phi) * (t1 + t2)
    if ko.family == o.GAMMAEXP:
        g = ko.param / 2
        with np.errstate(divide="ignore", invalid="ignore"):
            ls = np.where(s > 0, np.log(np.where(s > 0, s, 1.0)), 0.0)
            sg = np.where(s > 0, s ** g, 0.0)
        return chain * (-0.25) * phi * sg * ls, np.abs(chain * 0.25 * phi * sg) * (np.abs(ls) + 1)
    if ko.family == o.IMQ:
        c = ko.param
        v = chain * (-c) * (s + c * c) ** -1.5
        return v, np.abs(v)
    z = np.zeros_like(S)
    return z, z


def param_derivative(o, ko, S):
    return param_parts(o, ko, S)[0]


def pair_quantities(o, ko, X, Y, per_dim, dt):
    """Per output: (Q, |dQ/dS| S, M, extra) as n x m arrays, and E (exponent magnitudes) — everything the reference and the bound need."""
    Xd, Yd = X.astype(F64), Y.astype(F64)
    S = o.pair_arg(ko, Xd, Yd)
    zero = S == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        v, d1, d2 = o.profile_derivatives(ko, S, dt)
    d1 = np.where(zero, 0.0, d1); d2 = np.where(zero, 0.0, d2)
    k0 = abs(float(o.profile(ko, np.zeros(1), dt)[0]))
    with np.errstate(divide="ignore"):
        E = np.maximum(0.0, -np.log(np.abs(v) / k0))
    E = np.where(np.isfinite(E), E, 800.0)                          # an entry that underflowed in fp64: its weight is 0 anyway
    if ko.family == o.GAMMAEXP:
        s = S / ko.lengthscale ** 2
        E = E + np.abs(ko.param / 2 * np.log(np.where(zero, 1.0, s)))
    dp, Mp = param_parts(o, ko, S)
    h = 1e-6 * S
    with np.errstate(divide="ignore", invalid="ignore"):
        dps = np.where(zero, 0.0, (param_derivative(o, ko, S + h) - param_derivative(o, ko, S - h)) / np.where(zero, 1.0, 2 * h))
    quantities = [(v, np.abs(d1) * S, np.abs(v), 0.0), (dp, np.abs(dps) * S, Mp, 0.0)]
    if per_dim:
        for c in range(X.shape[1]):
            D2 = (Xd[:, c][:, None] - Yd[:, c][None, :]) ** 2
            quantities.append((d1 * D2, np.abs(d2) * S * D2, np.abs(d1) * D2, 2.0))
    else:
        quantities.append((d1 * S, np.abs(d2 * S + d1) * S, np.abs(d1) * S, 1.0))
    return quantities, E


def reference_and_bound(o, ko, X, Y, U, A, per_dim, dt):
    """(ref, bound): the 2 + (d or 1) outputs in fp64 and the bound of the module docstring."""
    eps = float(np.finfo(dt).eps); u = eps / 2
    d = X.shape[1]
    U2 = U.reshape(U.shape[0], -1).astype(F64); A2 = A.reshape(A.shape[0], -1).astype(F64)
    nvec = U2.shape[1]
    W = U2 @ A2.T
    Wabs = np.abs(U2) @ np.abs(A2).T
    gam = lambda k: k * u / (1 - k * u)
    quantities, E = pair_quantities(o, ko, X, Y, per_dim, dt)
    ref, bound = [], []
    for Q, cond, M, extra in quantities:
        b = eps * ((d + 2) / 2 * cond + (C_EVAL * ko.power + extra + C_ARG * E) * M)
        ref.append(float((W * Q).sum()))
        bound.append(float((Wabs * b).sum() + (gam(nvec) + gam(HANDOFF + 6)) * (Wabs * np.abs(Q)).sum() + np.finfo(dt).tiny))
    return np.array(ref), np.array(bound)


def reference(o, ko, X, Y, U, A, per_dim, dt=F64):
    return reference_and_bound(o, ko, X, Y, U, A, per_dim, dt)[0]


def _r32(a):
    return np.asarray(a, F64).astype(F32).astype(F64)


def emulate_f32(o, ko, X, Y, U, A, per_dim):
    """The outputs an exactly rounded fp32 evaluation in the kernel's order gives: direct differences and FMA accumulation of S over the
    dimensions, the scaled argument, the jet rounded once per factor, W_ij as nvec fused multiply-adds (column order), each lane's
    sequential fp32 FMA accumulation over its pairs (row i; within a 64-column tile the 16 columns of its wave; GROUP tiles, per-dimension
    sums one tile) followed by the 6-step butterfly over the 64 rows of the tile, and fp64 from there."""
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
    zero = s == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        v, d1, _ = o.profile_derivatives(k1, s, F32)
    sc = _r32(ko.scale)
    v = _r32(_r32(v) * sc)
    ds = np.where(zero, 0.0, _r32(_r32(_r32(d1) * g2) * sc))
    kp = o.Kernel(ko.family, p=ko.p, param=ko.param, power=ko.power, scale=1.0)
    dp = _r32(_r32(param_derivative(o, kp, s)) * sc)
    gw = _r32(W * ds)

    def lane_sum(Wt, Qt, group):
        """sum_ij fma(Wt, Qt, acc) in the lanes' order; group = tiles between hand-offs."""
        npad = -(-n // TILE) * TILE; mpad = -(-m // (TILE * group)) * (TILE * group)
        Wp = np.zeros((npad, mpad)); Qp = np.zeros((npad, mpad))
        Wp[:n, :m] = Wt; Qp[:n, :m] = Qt
        # [row tile, row, hand-off group, tile, wave, column] -> a lane's sequence: tiles of the group, then its 16 columns
        shp = (npad // TILE, TILE, mpad // (TILE * group), group, TILE // LANE_COLS, LANE_COLS)
        Wl = Wp.reshape(shp).transpose(0, 2, 4, 1, 3, 5).reshape(shp[0], shp[2], shp[4], TILE, group * LANE_COLS)
        Ql = Qp.reshape(shp).transpose(0, 2, 4, 1, 3, 5).reshape(shp[0], shp[2], shp[4], TILE, group * LANE_COLS)
        acc = np.zeros(Wl.shape[:-1])
        for t in range(Wl.shape[-1]):
            acc = _r32(Wl[..., t] * Ql[..., t] + acc)
        for o_ in (32, 16, 8, 4, 2, 1):                             # butterfly over the 64 rows: every lane ends with the same sum
            idx = np.arange(TILE) ^ o_
            acc = _r32(acc + acc[..., idx])
        return float(acc[..., 0].sum())

    out = [lane_sum(W, v, GROUP), lane_sum(W, dp, GROUP)]
    if per_dim:
        for c in range(d):
            out.append(lane_sum(gw, _r32(diffs[c] * diffs[c]), 1))
    else:
        out.append(lane_sum(gw, S, GROUP))
    return np.array(out)
