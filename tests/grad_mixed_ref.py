"""fp64 numpy restatement of the gradient kernels of mixed-trait composites (csrc/grad_mixed.hpp).

Every supported leaf is a function of p = x·y, q = |x|², s = |y|² (isotropic leaves through u = γ²|x − y|², formed by direct
differences).  With k(x, y) = F(p, q, s):

    ∇x k = F_p y + 2 F_q x            ∇y k = F_p x + 2 F_s y
    ∂x∂yᵀ k = F_p I + y (F_pp x + 2 F_ps y)ᵀ + 2 x (F_qp x + 2 F_qs y)ᵀ

A jet is the dict of the eight (n, m) arrays F, F_p, F_q, F_s, F_pp, F_ps, F_qp, F_qs.  Sum adds jets, Product is the Leibniz rule,
Power is a repeated product.  This module walks the covgram kernel OBJECTS itself (it does not use covgram's lowering)."""
import math

import numpy as np

KEYS = ("v", "p", "q", "s", "pp", "ps", "qp", "qs")


def _leaf(f0, f1, f2, u):
    """φ(u) with u a dict jet of the argument (u_pp = 0 for every leaf here): F_i = φ' u_i, F_ij = φ'' u_i u_j + φ' u_ij."""
    return {"v": f0, "p": f1 * u["p"], "q": f1 * u["q"], "s": f1 * u["s"],
            "pp": f2 * u["p"] * u["p"] + f1 * u["pp"], "ps": f2 * u["p"] * u["s"] + f1 * u["ps"],
            "qp": f2 * u["q"] * u["p"] + f1 * u["qp"], "qs": f2 * u["q"] * u["s"] + f1 * u["qs"]}


def _mul(f, g):
    return {"v": f["v"] * g["v"],
            "p": f["p"] * g["v"] + f["v"] * g["p"], "q": f["q"] * g["v"] + f["v"] * g["q"], "s": f["s"] * g["v"] + f["v"] * g["s"],
            "pp": f["pp"] * g["v"] + 2 * f["p"] * g["p"] + f["v"] * g["pp"],
            "ps": f["ps"] * g["v"] + f["p"] * g["s"] + f["s"] * g["p"] + f["v"] * g["ps"],
            "qp": f["qp"] * g["v"] + f["q"] * g["p"] + f["p"] * g["q"] + f["v"] * g["qp"],
            "qs": f["qs"] * g["v"] + f["q"] * g["s"] + f["s"] * g["q"] + f["v"] * g["qs"]}


def _const(c, shape, dtype=np.float64):
    z = np.zeros(shape, dtype=dtype)
    return {k: (z + c if k == "v" else z.copy()) for k in KEYS}


def pair_scalars(X, Y):
    X = np.asarray(X, dtype=np.float64); Y = np.asarray(Y, dtype=np.float64)
    R = X[:, None, :] - Y[None, :, :]
    return {"r2": (R * R).sum(-1), "p": X @ Y.T, "q": np.broadcast_to((X * X).sum(1)[:, None], (X.shape[0], Y.shape[0])),
            "s": np.broadcast_to((Y * Y).sum(1)[None, :], (X.shape[0], Y.shape[0]))}


def jet(cg, k, sc, gamma2=1.0):
    """The jet of the covgram kernel object k on the pair scalars sc (pair_scalars); gamma2 = 1 / l² of the enclosing Lengthscales."""
    shape, dt = sc["p"].shape, sc["p"].dtype
    zero, one = np.zeros(shape, dtype=dt), np.ones(shape, dtype=dt)
    if isinstance(k, cg.Constant):
        return _const(k.c, shape, dt)
    if isinstance(k, cg.Sum):
        js = [jet(cg, a, sc, gamma2) for a in k.args]
        return {key: sum(j[key] for j in js) for key in KEYS}
    if isinstance(k, cg.Product):
        out = _const(1.0, shape, dt)
        for a in k.args:
            out = _mul(out, jet(cg, a, sc, gamma2))
        return out
    if isinstance(k, cg.Power):
        base, out = jet(cg, k.k, sc, gamma2), _const(1.0, shape, dt)
        for _ in range(k.p):
            out = _mul(out, base)
        return out
    if isinstance(k, cg.Lengthscale):
        return jet(cg, k.k, sc, gamma2 / k.l ** 2)
    if isinstance(k, cg.IsotropicKernel):
        u = {"v": gamma2 * sc["r2"], "p": -2 * gamma2 * one, "q": gamma2 * one, "s": gamma2 * one, "pp": zero, "ps": zero, "qp": zero, "qs": zero}
        a = u["v"]
        if isinstance(k, cg.EQ):
            e = np.exp(-a / 2)
            return _leaf(e, -e / 2, e / 4, u)
        if isinstance(k, cg.MaternP) and k.p == 2:
            r = np.sqrt(5 * a); e = np.exp(-r)
            return _leaf((1 + r + r * r / 3) * e, -(5.0 / 6.0) * (1 + r) * e, (25.0 / 12.0) * e, u)
        if isinstance(k, cg.RQ):
            w = 1 + a / (2 * k.alpha)
            return _leaf(w ** -k.alpha, -0.5 * w ** (-k.alpha - 1), (k.alpha + 1) / (4 * k.alpha) * w ** (-k.alpha - 2), u)
        if isinstance(k, cg.Cauchy):
            v = 1 / (1 + a)
            return _leaf(v, -v * v, 2 * v ** 3, u)
        raise NotImplementedError(type(k).__name__)
    if isinstance(k, cg.Dot):
        return {"v": sc["p"], "p": one, "q": zero, "s": zero, "pp": zero, "ps": zero, "qp": zero, "qs": zero}
    if isinstance(k, cg.ExponentialDot):
        e = np.exp(sc["p"])
        return {"v": e, "p": e, "q": zero, "s": zero, "pp": e, "ps": zero, "qp": zero, "qs": zero}
    if isinstance(k, cg.NeuralNetwork):
        sg = k.sigma
        A, B = 1 + sc["q"] + sg, 1 + sc["s"] + sg
        D = 1 / np.sqrt(A * B)
        uv = (sc["p"] + sg) * D
        u = {"v": uv, "p": D, "q": -uv / (2 * A), "s": -uv / (2 * B), "pp": zero, "ps": -D / (2 * B), "qp": -D / (2 * A), "qs": uv / (4 * A * B)}
        c = 2 / math.pi
        om = 1 - uv * uv
        return _leaf(c * np.arcsin(uv), c / np.sqrt(om), c * uv / om ** 1.5, u)
    raise NotImplementedError(type(k).__name__)


def dense(cg, k, X, Y, value=False):
    """The dense block Gramian ((n B) x (m B), B = d + value), point-major blocks; value blocks in the layout of the oracle's
    valgrad_block: [k, (∇y k)ᵀ; ∇x k, ∂x∂yᵀ k]."""
    X = np.asarray(X, dtype=np.float64); Y = np.asarray(Y, dtype=np.float64)
    n, d = X.shape; m = Y.shape[0]
    F = jet(cg, k, pair_scalars(X, Y))
    xi, yj = X[:, None, :, None], Y[None, :, :, None]                  # component a (rows of the block)
    xb, yb = X[:, None, None, :], Y[None, :, None, :]                  # component b (columns of the block)
    f = lambda key: F[key][:, :, None, None]
    G = f("p") * np.eye(d)[None, None] + yj * (f("pp") * xb + 2 * f("ps") * yb) + 2 * xi * (f("qp") * xb + 2 * f("qs") * yb)
    if not value:
        return G.transpose(0, 2, 1, 3).reshape(n * d, m * d)
    B = d + 1
    M = np.zeros((n, m, B, B))
    M[:, :, 1:, 1:] = G
    M[:, :, 0, 0] = F["v"]
    M[:, :, 0, 1:] = F["p"][:, :, None] * X[:, None, :] + 2 * F["s"][:, :, None] * Y[None, :, :]     # value row: ∇y k
    M[:, :, 1:, 0] = F["p"][:, :, None] * Y[None, :, :] + 2 * F["q"][:, :, None] * X[:, None, :]     # value column: ∇x k
    return M.transpose(0, 2, 1, 3).reshape(n * B, m * B)


def _terms(cg, k, X, Y, A, value, absolute):
    """The block product as the kernel forms it, Σ_j [F_p a_j + (F_pp t + 2 F_ps w [+ F_p a0]) y_j + 2 (F_qp t + 2 F_qs w [+ F_q a0]) x_i]
    (+ the value row F a0 + F_p t + 2 F_s w); absolute: every term replaced by its absolute value."""
    X = np.asarray(X, dtype=np.float64); Y = np.asarray(Y, dtype=np.float64)
    n, d = X.shape; m = Y.shape[0]
    vg = 1 if value else 0
    A = np.asarray(A, dtype=np.float64).reshape(m, d + vg)
    a0, Av = (A[:, 0], A[:, 1:]) if value else (np.zeros(m), A)
    F = jet(cg, k, pair_scalars(X, Y))
    ab = np.abs if absolute else (lambda v: v)
    Xa, Ya, Aa, a0a = ab(X), ab(Y), ab(Av), ab(a0)
    t = (Xa @ Aa.T) if absolute else X @ Av.T                      # Σ_k |x_k a_k|  /  x·a
    w = ((Ya * Aa).sum(1) if absolute else (Y * Av).sum(1))[None, :]
    Fa = {key: ab(F[key]) for key in KEYS}
    cy = Fa["pp"] * t + 2 * Fa["ps"] * w + (Fa["p"] * a0a[None, :] if value else 0)
    cx = Fa["qp"] * t + 2 * Fa["qs"] * w + (Fa["q"] * a0a[None, :] if value else 0)
    out = np.zeros((n, d + vg))
    out[:, vg:] = Fa["p"] @ Aa + cy @ Ya + 2 * cx.sum(1)[:, None] * Xa
    if value:
        out[:, 0] = (Fa["v"] * a0a[None, :] + Fa["p"] * t + 2 * Fa["s"] * w).sum(1)
    return out.reshape(-1)


def mvm(cg, k, X, Y, A, value=False):
    """G a for one right-hand side a (flat, point-major blocks of d + value)."""
    return _terms(cg, k, X, Y, A, value, False)


def absref(cg, k, X, Y, A, value=False):
    """The same product with every term replaced by its absolute value, as the kernel forms it:
    |F_p||a_l| + |y_l|(|F_pp| Σ|x_k a_k| + 2|F_ps| Σ|y_k a_k|) + 2|x_l|(|F_qp| Σ|x_k a_k| + 2|F_qs| Σ|y_k a_k|)."""
    return _terms(cg, k, X, Y, A, value, True)


def mvm_float32(cg, k, X, Y, A, value=False):
    """A float32 emulation of the formation order of the device kernel: inputs rounded to fp32, the pair scalars, the jets and the
    per-pair terms formed in fp32 (numpy float32 arithmetic, no fused multiply-adds), columns accumulated in ascending order."""
    f32 = np.float32
    X = np.asarray(X, dtype=f32); Y = np.asarray(Y, dtype=f32)
    n, d = X.shape; m = Y.shape[0]
    vg = 1 if value else 0
    A = np.asarray(A, dtype=f32).reshape(m, d + vg)
    a0, Av = (A[:, 0], A[:, 1:]) if value else (np.zeros(m, dtype=f32), A)
    R = X[:, None, :] - Y[None, :, :]
    r2, p, t = np.zeros((n, m), f32), np.zeros((n, m), f32), np.zeros((n, m), f32)
    q, s, w = np.zeros(n, f32), np.zeros(m, f32), np.zeros(m, f32)
    for l in range(d):
        r2 += R[:, :, l] * R[:, :, l]; p += X[:, None, l] * Y[None, :, l]; t += X[:, None, l] * Av[None, :, l]
        q += X[:, l] * X[:, l]; s += Y[:, l] * Y[:, l]; w += Y[:, l] * Av[:, l]
    sc = {"r2": r2, "p": p, "q": np.broadcast_to(q[:, None], (n, m)), "s": np.broadcast_to(s[None, :], (n, m))}
    F = {key: np.asarray(v, dtype=f32) for key, v in _jet32(cg, k, sc).items()}
    w2 = f32(2) * w[None, :]
    cy = F["pp"] * t + F["ps"] * w2
    cx = F["qp"] * t + F["qs"] * w2
    if value:
        cy = cy + F["p"] * a0[None, :]; cx = cx + F["q"] * a0[None, :]
    out = np.zeros((n, d + vg), f32)
    csum = np.zeros(n, f32)
    for j in range(m):
        out[:, vg:] += F["p"][:, j, None] * Av[None, j, :] + cy[:, j, None] * Y[None, j, :]
        csum += cx[:, j]
        if value:
            out[:, 0] += F["v"][:, j] * a0[j] + (F["p"][:, j] * t[:, j] + F["s"][:, j] * w2[0, j])
    out[:, vg:] += X * (f32(2) * csum)[:, None]
    return out.reshape(-1).astype(np.float64)


def _jet32(cg, k, sc):
    """jet() with every intermediate rounded to float32: the inputs are float32 arrays and numpy keeps float32 arithmetic; Python
    scalars (weak) do not promote."""
    sc32 = {key: np.asarray(v, dtype=np.float32) for key, v in sc.items()}
    return jet(cg, k, sc32)


# ---- the inputs both test files use (tests/test_grad_mixed_host.py checks them for feasibility, tests/test_gpu_grad_mixed.py runs them) ----
def kernels(cg):
    """name -> kernel: the eight composites of the GPU test."""
    return {
        "eq+dot": cg.EQ() + cg.Dot(),
        "eq+(dot^2+1)": cg.EQ() + (cg.Dot() ** 2 + 1),
        "eq*(dot^2+1)": cg.EQ() * (cg.Dot() ** 2 + 1),
        "dot*dot": cg.Dot() * cg.Dot(),
        "maternp2+dot^2+nn": cg.MaternP(2) + cg.Dot() ** 2 + cg.NeuralNetwork(),
        "nn(0.5)*ls(eq,2)": cg.NeuralNetwork(0.5) * cg.Lengthscale(cg.EQ(), 2.0),
        "(eq*dot)^2": (cg.EQ() * cg.Dot()) ** 2,
        "eq*dot zero": cg.EQ() * cg.Dot(),
    }


def clouds(name, n, m, d, same=False, seed=0):
    """(X, Y) in fp64: N(0, 0.8²) (|x| stays moderate, so asin′ of the NeuralNetwork leaf does too), scaled by sqrt(3 / d) beyond
    d = 3 so that x·y and |x − y|² keep their size as d grows; "eq*dot zero": some x_i·y_j are EXACTLY 0 (the reference throws there)."""
    rng = np.random.default_rng(1000 * d + 7 * n + m + seed)
    sd = 0.8 * min(1.0, math.sqrt(3.0 / d))
    X = sd * rng.standard_normal((n, d))
    Y = X if same else sd * rng.standard_normal((m, d))
    if name == "eq*dot zero":
        X = X.copy(); X[::3, 0] = 0.0
        if same:
            Y = X
        else:
            Y = Y.copy(); Y[::2, 1:] = 0.0
    return X, Y
