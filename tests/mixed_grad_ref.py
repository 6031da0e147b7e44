"""Shared by tests/test_mixed_grad_host.py (no GPU) and tests/test_gpu_mixed_grad.py: the fp64 reference of the 24 outputs of
covgram_bilinear_grad_mixed, the error bound they are held to, and an fp32 emulation of the kernel's order of operations.

Reference.  The LAYOUT (which term is t, which factor is f) is read from the covgram_kernel_composite the lowering produced; every
number is recomputed here in numpy fp64 from the factor's family, power, parameter and lengthscale with tests/mixed_ref.py's leaf
profiles (plus InverseMultiQuadratic, which that file has no use for).  With W = U Aᵀ, ψ_f = φ_f(z_f)^power_f and c_t the term's
coefficient,
    out[t]      = Σ W Π_{f∈t} ψ_f
    out[8 + f]  = c_t Σ W z_f ∂ψ_f/∂z_f Π_{g≠f} ψ_g      isotropic factors, z = r²/l², a pair with z = 0 adding nothing
    out[16 + f] = c_t Σ W ∂ψ_f/∂θ_f Π_{g≠f} ψ_g          RQ α, γ-exponential γ (0 at z = 0), IMQ c, NeuralNetwork σ
NeuralNetwork's ∂ψ/∂σ is taken as ψ_p + ψ_q + ψ_s of mixed_ref.nn_partials (σ enters as p + σ, q + σ, s + σ): not the closed form
the kernel evaluates.  The lowering itself is checked against finite differences of the kernel OBJECTS (test_mixed_grad_host.py).

Bound (ε the dtype's machine epsilon, u = ε/2, γ_k = k u / (1 − k u)).  For output k with per-pair quantity Q_k = D_f Π_{g≠f} ψ_g
(D_f = ψ_f for out[t], z ∂ψ_f/∂z or ∂ψ_f/∂θ otherwise; c_t multiplies both sides):
    |out_k − ref_k| ≤ Σ_ij ( |W|_ij b_ij,k + γ_nvec |W|_ij |Q_ij,k| ) + γ_{L+6} Σ_ij |W|_ij |Q_ij,k| + tiny
  * |W| = |U| |A|ᵀ; γ_nvec: W_ij is nvec fused multiply-adds;
  * b_ij,k = ε [ (d + 2)/2 · cond + count ]:
      - cond = S(D_f) Π_{g≠f} |ψ_g| + M(D_f) Σ_{g≠f} S(ψ_g) Π_{h≠f,g} |ψ_h| is the conditioning majorant of Q_k in the arguments the kernel
        forms, S(F) = Σ_z |∂F/∂z| z̄ with z̄ as in mixed_ref.majorant (isotropic: z = r²/l², z̄ = z; dot product: z = p, z̄ = Σ_l |x_l y_l|;
        NeuralNetwork: z ∈ {p, q, s}, z̄ ∈ {Σ_l |x_l y_l|, q, s}).  r² by direct differences carries d + 2 roundings of size u, all terms
        positive; p, q and s are d fused multiply-adds, error ≤ γ_d of their majorant: (d + 2)/2 · ε covers each.  ∂D/∂z of the
        derivative quantities is a central difference of the closed form in fp64 (a bound needs no more);
      - count = [ Σ_{g} (C_EVAL power_g + C_ARG E_g) + nf + 2 ] · M(D_f) Π_{g≠f} M(ψ_g): per factor of the term C_EVAL = 16 rounded
        operations of a closed form times the Power exponent (bilin_grad_ref's count: square root, reciprocal, hardware exp2 / log2 at
        1 ulp, a Horner polynomial, the chain-rule products; here also asin at 2 ulp and the four operations that form NeuralNetwork's
        argument) and C_ARG = 4 roundings of an exponent of magnitude E_g = −ln|φ_g / φ_g(0)| (+ |γ/2 ln z| for the γ-exponential; |p| for
        ExponentialDot); nf − 1 products for Π_{g≠f} ψ_g, one for W · L, one fused multiply-add, one for the lane's accumulator;
      - M(F) = |F| except where the closed form subtracts: RQ's ∂/∂α uses |ψ| (x/(1+x) + log1p x), the γ-exponential's ∂/∂γ
        ¼ |ψ| z^{γ/2} (|ln z| + 1) (both as bilin_grad_ref), NeuralNetwork's ∂/∂σ (2/π)(1 + |p+σ|(A+B)/(2AB))(1 + (AB + (p+σ)²)/(2 rad))/√rad
        with rad = AB − (p+σ)², and NeuralNetwork's value |ψ| + (2/π)|u|/√(1 − u²) (the roundings of the asin's argument);
  * γ_{L+6}: a lane adds at most L = 128 pairs in the working precision (16 or 8 per tile in a register, the tiles into its accumulator),
    then 6 butterfly steps; everything after is fp64.
Nothing here is fitted to a device."""
import math

import numpy as np

import mixed_ref as M

F32, F64 = np.float32, np.float64
NOUT, Z0, P0 = 24, 8, 16
HANDOFF = 128                       # BG_L
C_EVAL, C_ARG = 16.0, 4.0
NUM_CUS = 256                       # MI355X: enters bg_column_split only where the column count does not already decide

# covgram_family numbers (include/covgram.h)
EQ, EXP, RQ, GAMMAEXP, CAUCHY, IMQ, MATERNP, DOT, EXPDOT, MATERN, ASINDOT, CONSTANT, NEURALNETWORK = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 100, 102
C2PI = 2 / math.pi


# ---- the composite as plain Python -----------------------------------------------------------------------------------------------------
def terms_of(comp):
    """[(c_t, [factor])] with factor = dict(f = flat index, family, p, power, param, l); Constant factors only add to c_t."""
    out, fi = [], 0
    for t in range(comp.nterms):
        c, fs = comp.head.scale, []
        for _ in range(comp.nfactors[t]):
            k = comp.factors[fi]
            c *= k.scale
            if k.family != CONSTANT:
                fs.append(dict(f=fi, family=k.family, p=k.p, power=k.power, param=k.param, l=k.lengthscale))
            fi += 1
        out.append((c, fs))
    return out


def _leaf_object(cg, fac):
    fam = fac["family"]
    if fam == EQ: return cg.EQ()
    if fam == EXP: return cg.Exponential()
    if fam == RQ: return cg.RQ(fac["param"])
    if fam == GAMMAEXP: return cg.GammaExponential(fac["param"])
    if fam == CAUCHY: return cg.Cauchy()
    if fam == MATERNP: return cg.MaternP(fac["p"])
    if fam == DOT: return cg.Dot()
    if fam == EXPDOT: return cg.ExponentialDot()
    raise NotImplementedError(fam)


def _phi(cg, oracle, fac, z):
    """(φ, φ′, ∂φ/∂θ, M(∂φ/∂θ), E) of a non-NeuralNetwork factor's bare profile at its argument z (fp64)."""
    fam = fac["family"]
    zero = np.zeros_like(z)
    with np.errstate(divide="ignore", invalid="ignore"):
        if fam == IMQ:
            c = fac["param"]
            v = (z + c * c) ** -0.5
            d1 = -0.5 * (z + c * c) ** -1.5
            dp = -c * (z + c * c) ** -1.5
            return v, d1, dp, np.abs(dp), np.maximum(0.0, -np.log(v * abs(c)))
        if fam == ASINDOT:
            v = C2PI * np.arcsin(z)
            return v, C2PI / np.sqrt(1 - z * z), zero, zero, zero
        v, d1 = M.leaf_profile(cg, oracle, _leaf_object(cg, fac), z)
        if fam in (DOT,):
            return v, d1, zero, zero, zero
        if fam == EXPDOT:
            return v, d1, zero, zero, np.abs(z)
        E = np.maximum(0.0, -np.log(np.abs(v)))
        E = np.where(np.isfinite(E), E, 800.0)
        if fam == RQ:
            x = z / (2 * fac["param"])
            t1, t2 = x / (1 + x), np.log1p(x)
            return v, d1, v * (t1 - t2), np.abs(v) * (t1 + t2), E
        if fam == GAMMAEXP:
            g = fac["param"] / 2
            pos = z > 0
            ls = np.where(pos, np.log(np.where(pos, z, 1.0)), 0.0)
            sg = np.where(pos, np.where(pos, z, 1.0) ** g, 0.0)
            return v, d1, -0.25 * v * sg * ls, 0.25 * np.abs(v) * sg * (np.abs(ls) + 1), E + np.abs(g * ls)
        return v, d1, zero, zero, E


def _nn(sigma, sc):
    """NeuralNetwork(σ) on the pair scalars: ψ, ∂ψ/∂σ, M(ψ), M(∂ψ/∂σ), and the (p, q, s) partials of ψ."""
    p, q, s = sc["p"], sc["q"], sc["s"]
    v, vp, vq, vs = M.nn_partials(F64(sigma), p, q, s)
    A, B = 1 + q + sigma, 1 + s + sigma
    num = p + sigma
    rad = A * B - num * num
    u = num / np.sqrt(A * B)
    Mv = np.abs(v) + C2PI * np.abs(u) / np.sqrt(1 - u * u)
    Mp = C2PI * (1 + np.abs(num) * (A + B) / (2 * A * B)) * (1 + (A * B + num * num) / (2 * rad)) / np.sqrt(rad)
    return v, vp + vq + vs, Mv, Mp, (vp, vq, vs)


def _factor(cg, oracle, fac, sc):
    """Everything about one factor on the pair scalars (fp64):
    psi, zd (z ∂ψ/∂z; None where the factor is not isotropic), dp (∂ψ/∂θ; None without a parameter), their M's, their S's, count."""
    pw = fac["power"]
    fam = fac["family"]
    out = dict(zd=None, dp=None)
    if fam == NEURALNETWORK:
        sig = fac["param"]
        phi, dphi, Mv, Mp, (vp, vq, vs) = _nn(sig, sc)
        bars = (sc["pbar"], sc["q"], sc["s"])
        Sphi = np.abs(vp) * bars[0] + np.abs(vq) * bars[1] + np.abs(vs) * bars[2]
        chain = pw * phi ** (pw - 1)
        out.update(psi=phi ** pw, Mpsi=Mv * np.abs(phi) ** (pw - 1), Spsi=np.abs(chain) * Sphi, dp=chain * dphi, Mdp=np.abs(chain) * Mp)
        # S(∂ψ/∂σ): central differences in p, q, s
        Sd = np.zeros_like(phi)
        for key, bar in zip(("p", "q", "s"), bars):
            h = 1e-6 * np.maximum(bar, 1e-3)
            hi, lo = dict(sc), dict(sc)
            hi[key] = sc[key] + h; lo[key] = sc[key] - h
            fh = _nn(sig, hi); fl = _nn(sig, lo)
            Sd += np.abs((pw * fh[0] ** (pw - 1) * fh[1] - pw * fl[0] ** (pw - 1) * fl[1]) / (2 * h)) * bar
        out.update(Sdp=Sd, count=C_EVAL * pw)
        return out
    iso = fam not in (DOT, EXPDOT, ASINDOT)
    z = sc["r2"] / fac["l"] ** 2 if iso else sc["p"]
    zbar = z if iso else sc["pbar"]
    phi, d1, dth, Mth, E = _phi(cg, oracle, fac, z)
    chain = pw * phi ** (pw - 1)
    with np.errstate(invalid="ignore"):
        S1 = np.where(zbar == 0, 0.0, np.abs(d1) * zbar) if iso else np.abs(d1) * zbar
    out.update(psi=phi ** pw, Mpsi=np.abs(phi) ** pw, Spsi=np.abs(chain) * S1, count=C_EVAL * pw + C_ARG * E)

    def D(zz):                                             # (z ∂ψ/∂z, ∂ψ/∂θ) as functions of z, for the central differences
        f, f1, ft, _, _ = _phi(cg, oracle, fac, zz)
        ch = pw * f ** (pw - 1)
        with np.errstate(invalid="ignore"):
            return np.where(zz == 0, 0.0, ch * f1 * zz), ch * ft
    if iso:
        zd, dp = D(z)
        h = 1e-6 * z
        with np.errstate(divide="ignore", invalid="ignore"):
            zh, ph = D(z + h); zl, pl = D(z - h)
            Szd = np.where(z == 0, 0.0, np.abs((zh - zl) / np.where(z == 0, 1.0, 2 * h)) * z)
            Sdp = np.where(z == 0, 0.0, np.abs((ph - pl) / np.where(z == 0, 1.0, 2 * h)) * z)
        out.update(zd=zd, Mzd=np.abs(zd), Szd=Szd)
        if fam in (RQ, GAMMAEXP, IMQ):
            out.update(dp=dp, Mdp=np.abs(chain) * Mth, Sdp=Sdp)
    return out


def pair_quantities(cg, oracle, comp, X, Y):
    """{k: (Q, cond, countM, c)}: per live output its per-pair quantity, conditioning majorant, count·M and the coefficient that scales it."""
    sc = M.pair_scalars(np.asarray(X, F64), np.asarray(Y, F64))
    shape = sc["p"].shape
    res = {}
    for t, (c, fs) in enumerate(terms_of(comp)):
        F = [_factor(cg, oracle, fac, sc) for fac in fs]
        nf = len(F)
        count = sum(f["count"] for f in F) + nf + 2

        def quantity(i, D, MD, SD):
            others = [g for j, g in enumerate(F) if j != i]
            L = np.ones(shape); ML = np.ones(shape)
            for g in others:
                L = L * g["psi"]; ML = ML * g["Mpsi"]
            cond = SD * np.prod([np.abs(g["psi"]) for g in others], axis=0) if others else SD
            for j, g in enumerate(others):
                rest = np.ones(shape)
                for h, g2 in enumerate(others):
                    if h != j:
                        rest = rest * np.abs(g2["psi"])
                cond = cond + MD * g["Spsi"] * rest
            return D * L, cond, count * MD * ML
        if nf == 0:
            res[t] = (np.ones(shape), np.zeros(shape), 2.0 * np.ones(shape), 1.0)
            continue
        res[t] = quantity(0, F[0]["psi"], F[0]["Mpsi"], F[0]["Spsi"]) + (1.0,)
        for i, (fac, f) in enumerate(zip(fs, F)):
            if f["zd"] is not None:
                res[Z0 + fac["f"]] = quantity(i, f["zd"], f["Mzd"], f["Szd"]) + (c,)
            if f["dp"] is not None:
                res[P0 + fac["f"]] = quantity(i, f["dp"], f["Mdp"], f["Sdp"]) + (c,)
    return res


def weights(U, A):
    U2 = np.asarray(U, F64).reshape(np.shape(U)[0], -1); A2 = np.asarray(A, F64).reshape(np.shape(A)[0], -1)
    return U2, A2


def reference_and_bound(cg, oracle, comp, X, Y, U, A, dt, drop=None):
    """(ref, bound), 24 entries each; dead outputs have ref 0 and bound 0.  drop: an output whose quantity is left out (sensitivity)."""
    eps = float(np.finfo(dt).eps); u = eps / 2
    d = np.shape(X)[1]
    U2, A2 = weights(U, A)
    nvec = U2.shape[1]
    W = U2 @ A2.T
    Wabs = np.abs(U2) @ np.abs(A2).T
    gam = lambda k: k * u / (1 - k * u)
    ref, bound = np.zeros(NOUT), np.zeros(NOUT)
    for k, (Q, cond, cm, c) in pair_quantities(cg, oracle, comp, X, Y).items():
        b = eps * ((d + 2) / 2 * cond + cm)
        ref[k] = c * float((W * Q).sum())
        bound[k] = abs(c) * float((Wabs * b).sum() + (gam(nvec) + gam(HANDOFF + 6)) * (Wabs * np.abs(Q)).sum()) + float(np.finfo(dt).tiny)
    return ref, bound


def majorant_sums(cg, oracle, comp, X, Y, U, A):
    """Σ |W| |c Q_k| per output: the scale of a perturbation in the sensitivity test."""
    U2, A2 = weights(U, A)
    Wabs = np.abs(U2) @ np.abs(A2).T
    out = np.zeros(NOUT)
    for k, (Q, _, _, c) in pair_quantities(cg, oracle, comp, X, Y).items():
        out[k] = abs(c) * float((Wabs * np.abs(Q)).sum())
    return out


# ---- the kernel's order of operations in exactly rounded fp32 --------------------------------------------------------------------------------
def _r32(a):
    return np.asarray(a, F64).astype(F32).astype(F64)


def column_chunk(m, rowtiles, jsplit_opt=0, jpl=16):
    """Columns per chunk: mbg_column_split (bg_column_split, or option jsplit) for fp32 tiles."""
    tj, kt = 4 * jpl, HANDOFF // jpl
    ntiles = -(-m // tj)
    if jsplit_opt > 0:
        js = max(1, min(jsplit_opt, ntiles))
    else:
        js = max(1, min(-(-NUM_CUS * 8 // rowtiles), max(1, ntiles // kt), 65535))
    return -(-ntiles // js) * tj


def emulate_f32(cg, oracle, comp, X, Y, U, A, jsplit_opt=0, drop=None):
    """The 24 outputs of an exactly rounded fp32 evaluation in the kernel's order: r², p, q, s as fused multiply-add chains over the
    dimensions; each factor's argument and jet rounded once; Π_{g≠f} ψ_g multiplied up in factor order from 1; W as nvec fused
    multiply-adds; W·L rounded, the 16 pairs of a lane and tile added by fused multiply-adds from 0 and joined to the lane's accumulator;
    after 8 tiles (or at the chunk's end) the 6-step butterfly over the 64 rows; fp64 from there, c_t applied last.
    drop = (k): the derivative of output k's factor is left out (set to 0), for the sensitivity test."""
    n, m = np.shape(X)[0], np.shape(Y)[0]
    d = np.shape(X)[1]
    X = _r32(X); Y = _r32(Y)
    U2, A2 = weights(_r32(U), _r32(A))
    r2, p = np.zeros((n, m)), np.zeros((n, m))
    q, s = np.zeros(n), np.zeros(m)
    for c in range(d):
        df = _r32(X[:, c][:, None] - Y[:, c][None, :])
        r2 = _r32(df * df + r2)
        p = _r32(X[:, c][:, None] * Y[:, c][None, :] + p)
        q = _r32(X[:, c] * X[:, c] + q); s = _r32(Y[:, c] * Y[:, c] + s)
    W = np.zeros((n, m))
    for t in range(U2.shape[1]):
        W = _r32(U2[:, t][:, None] * A2[:, t][None, :] + W)
    sc = {"r2": r2, "p": p, "q": np.broadcast_to(q[:, None], (n, m)), "s": np.broadcast_to(s[None, :], (n, m)), "pbar": np.abs(p)}
    jpl, tile = 16, 64
    jchunk = column_chunk(m, -(-n // tile), jsplit_opt, jpl)
    kt = HANDOFF // jpl

    def lane_sum(Q):
        """Σ over the lanes' order of fma(W·L.., Q) — Q already includes L: the term W·L·D is formed as r32(W L) D by one fma."""
        WL, D = Q
        total = 0.0
        npad = -(-n // tile) * tile
        Wp = np.zeros((npad, m)); Dp = np.zeros((npad, m))
        Wp[:n] = WL; Dp[:n] = D
        for j0 in range(0, m, jchunk):
            j1 = min(j0 + jchunk, m)
            ntile = -(-(j1 - j0) // tile)
            acc = np.zeros((npad, 4))                      # [row, wave]
            held = 0
            for ti in range(ntile):
                cols = j0 + ti * tile + np.arange(tile)
                ok = cols < j1
                wt = np.where(ok[None, :], Wp[:, np.minimum(cols, m - 1)], 0.0).reshape(npad, 4, jpl)
                dt_ = np.where(ok[None, :], Dp[:, np.minimum(cols, m - 1)], 0.0).reshape(npad, 4, jpl)
                part = np.zeros((npad, 4))
                for jj in range(jpl):
                    part = _r32(wt[:, :, jj] * dt_[:, :, jj] + part)
                acc = _r32(acc + part)
                held += 1
                if held == kt or ti == ntile - 1:
                    b = acc.reshape(npad // tile, tile, 4)
                    for o_ in (32, 16, 8, 4, 2, 1):
                        b = _r32(b + b[:, np.arange(tile) ^ o_, :])
                    total += float(b[:, 0, :].sum())
                    acc = np.zeros((npad, 4)); held = 0
        return total

    out = np.zeros(NOUT)
    for t, (c, fs) in enumerate(terms_of(comp)):
        if not fs:
            out[t] = lane_sum((W, np.ones((n, m))))
            continue
        jets = []
        for fac in fs:
            if fac["family"] == NEURALNETWORK:
                sig = float(_r32(fac["param"]))
                A_ = _r32(_r32(1 + sc["q"]) + sig); B_ = _r32(_r32(1 + sc["s"]) + sig)
                num = _r32(p + sig)
                phi, dphi = _nn(sig, {"p": num - sig, "q": A_ - 1 - sig, "s": B_ - 1 - sig})[:2]
                pw = fac["power"]
                psi = _r32(_r32(phi) ** pw) if pw > 1 else _r32(phi)
                jets.append((psi, None, _r32(_r32(pw * _r32(phi) ** (pw - 1)) * _r32(dphi))))
                continue
            iso = fac["family"] not in (DOT, EXPDOT, ASINDOT)
            g2 = float(_r32((1.0 / fac["l"]) ** 2))
            z = _r32(r2 * g2) if iso else p
            f32fac = dict(fac, param=float(_r32(fac["param"])) if fac["family"] != GAMMAEXP else 2 * float(_r32(fac["param"] / 2)))
            phi, d1, dth, _, _ = _phi(cg, oracle, f32fac, z)
            pw = fac["power"]
            phi, d1, dth = _r32(phi), _r32(np.where(np.isfinite(d1), d1, 0.0)), _r32(dth)
            mult = _r32(pw * _r32(phi ** (pw - 1))) if pw > 1 else 1.0
            psi = _r32(_r32(phi ** (pw - 1)) * phi) if pw > 1 else phi
            zd = np.where(z == 0, 0.0, _r32(z * _r32(d1 * mult))) if iso else None
            dp = _r32(dth * mult) if fac["family"] in (RQ, GAMMAEXP, IMQ) else None
            jets.append((psi, zd, dp))
        for i, fac in enumerate(fs):
            L = np.ones((n, m))
            for j, (psi, _, _) in enumerate(jets):
                if j != i:
                    L = _r32(L * psi)
            WL = _r32(W * L)
            psi, zd, dp = jets[i]
            if i == 0:
                out[t] = lane_sum((WL, psi))
            if zd is not None:
                out[Z0 + fac["f"]] = c * (0.0 if drop == Z0 + fac["f"] else lane_sum((WL, zd)))
            if dp is not None:
                out[P0 + fac["f"]] = c * (0.0 if drop == P0 + fac["f"] else lane_sum((WL, dp)))
    return out


# ---- the cases both test files use -------------------------------------------------------------------------------------------------------
def kernels(cg):
    """name -> kernel: the eight of the issue."""
    LS = cg.Lengthscale
    return {
        "1.5ls(eq,.7)+.5dot": 1.5 * LS(cg.EQ(), 0.7) + 0.5 * cg.Dot(),
        "ls(eq,.8)*(dot^2+1)": LS(cg.EQ(), 0.8) * (cg.Dot() ** 2 + 1),
        ".7ls(maternp2,1.3)+.2poly(3,.4)": 0.7 * LS(cg.MaternP(2), 1.3) + 0.2 * cg.Polynomial(3, 0.4),
        "ls(rq(.37),1.2)*nn(.5)+.3imq(.6)": LS(cg.RQ(0.37), 1.2) * cg.NN(0.5) + 0.3 * cg.InverseMultiQuadratic(0.6),
        "nn(.3)+.1expdot": cg.NN(0.3) + 0.1 * cg.ExponentialDot(),
        "ls(exp,.9)*dot": LS(cg.Exponential(), 0.9) * cg.Dot(),
        "gammaexp(1.5)*dot+1": cg.GammaExponential(1.5) * cg.Dot() + 1,
        "ls(eq,.7)*ls(rq(.5),1.4)": LS(cg.EQ(), 0.7) * LS(cg.RQ(0.5), 1.4),
    }


def extra_kernels(cg):
    """Beyond the issue's eight: a Sum with 18 live outputs, more than one pass holds in fp64 beside the tiles of 32 columns of U."""
    return {"6 ls(rq)": cg.Sum(tuple(cg.Lengthscale(cg.RQ(0.3 + 0.2 * i), 0.8 + 0.1 * i) for i in range(6)))}


# (n, m, d, x is y, options)
SHAPES = [(130, 130, 3, True, {}), (70, 1100, 5, False, {}), (70, 1100, 5, False, {"jsplit": 3}), (100, 37, 17, False, {}), (33, 70, 64, False, {}),
          (1, 1, 1, False, {})]


def clouds(name, n, m, d, same, seed=0):
    """(X, Y) rounded to fp32, as fp64 arrays: N(0, σ²) with σ = 0.75 / sqrt(d) so that |x| ≲ 1.5; ExponentialDot sees the coordinates
    scaled by 0.5; where the sets differ Y[0] = X[3] (X[0] when n < 4) plants one pair at distance exactly 0."""
    rng = np.random.default_rng(7000 * d + 11 * n + m + seed)
    sd = 0.75 / math.sqrt(d) * (0.5 if "expdot" in name else 1.0)
    X = _r32(sd * rng.standard_normal((n, d)))
    if same:
        return X, X
    Y = _r32(sd * rng.standard_normal((m, d)))
    Y[0] = X[3 if n > 3 else 0]
    return X, Y


def weights_for(n, m, nvec, seed=5):
    rng = np.random.default_rng(seed + 13 * nvec + n + 3 * m)
    return _r32(rng.standard_normal((n, nvec))), _r32(rng.standard_normal((m, nvec)))
