"""fp64 numpy restatement of the SCALAR Gramians of mixed-trait composites (csrc/mixed_mvm.hpp).

Every supported leaf is a function of p = x·y, q = |x|², s = |y|²; isotropic leaves through u = γ²|x − y|², the distance formed by
direct differences.  This module walks the covgram kernel OBJECTS itself (it does not use covgram's lowering).  It provides

    matrix(cg, k, X, Y)      k(x_i, y_j)
    majorant(cg, k, X, Y)    the entry-wise conditioning majorant K̄ (below)
    mvm_float32 / matrix_float32   an emulation of the device's formation order in float32 numpy arithmetic

    K̄_ij = Σ_t |c_t| [ Π_f |ψ_f| + Σ_f S_f Π_{g≠f} |ψ_g| ],     ψ_f = φ_f^power,
    S_f  = Σ_z |∂ψ_f/∂z| z̄    over the arguments the kernel forms for that leaf:
           isotropic: z = u = γ²r², z̄ = u;   dot product: z = p, z̄ = Σ_l |x_l y_l|;
           NeuralNetwork: z ∈ {p, q, s}, z̄ ∈ {Σ_l |x_l y_l|, q, s}

computed recursively over the expression as the pair (A, B) = (Π|ψ| part, sensitivity part): a leaf is (|ψ|, S), a Constant (|c|, 0), a
Sum adds both, a Product is (Π A_i, Σ_i B_i Π_{j≠i} A_j), Power(n) is the n-fold Product; K̄ = A + B.  Multiplied out this is the
formula above for every expression whose like terms do not cancel (all of this file's).  At r = 0, |φ′(u)| u is taken as its limit 0
for Exponential, GammaExponential and MaternP(0).  Matern(ν) and its derivative come from the oracle's profile functions (scipy's
Bessel functions)."""
import math

import numpy as np

import grad_mixed_ref as G


# ---- leaves: (φ, φ′) of the profile's own argument, in the dtype of the argument -------------------------------------------------------
def leaf_profile(cg, oracle, k, u):
    """(φ(u), φ′(u)) of an isotropic or dot-product leaf object k; float32 arguments keep float32 arithmetic (Matern(ν) excepted:
    the oracle's fp64 value, rounded)."""
    dt = u.dtype
    with np.errstate(divide="ignore", invalid="ignore"):
        if isinstance(k, cg.EQ):
            e = np.exp(-u / 2)
            return e, -e / 2
        if isinstance(k, cg.Exponential) or (isinstance(k, cg.MaternP) and k.p == 0):
            r = np.sqrt(u); e = np.exp(-r)
            return e, -e / (2 * r)
        if isinstance(k, cg.GammaExponential):
            g = dt.type(k.gamma / 2)
            t = u ** g
            e = np.exp(-t / 2)
            return e, -(g / 2) * u ** (g - 1) * e
        if isinstance(k, cg.MaternP) and k.p == 2:
            r = np.sqrt(5 * u); e = np.exp(-r)
            return (1 + r + r * r / 3) * e, -(dt.type(5.0) / 6) * (1 + r) * e
        if isinstance(k, cg.RQ):
            w = 1 + u / (2 * k.alpha)
            return w ** dt.type(-k.alpha), -w ** dt.type(-k.alpha - 1) / 2
        if isinstance(k, cg.Cauchy):
            v = 1 / (1 + u)
            return v, -v * v
        if isinstance(k, cg.Matern):
            o = oracle
            v, d1, _ = o.profile_derivatives(o.Kernel(o.MATERN, param=float(k.nu)), np.asarray(u, dtype=np.float64))
            return v.astype(dt), d1.astype(dt)
        if isinstance(k, cg.Dot):
            return u, np.ones_like(u)
        if isinstance(k, cg.ExponentialDot):
            e = np.exp(u)
            return e, e
    raise NotImplementedError(type(k).__name__)


def nn_partials(sigma, p, q, s):
    """(ψ, ψ_p, ψ_q, ψ_s) of NeuralNetwork(σ): ψ = (2/π) asin((p + σ) / sqrt((1 + q + σ)(1 + s + σ)))."""
    A, B = 1 + q + sigma, 1 + s + sigma
    D = 1 / np.sqrt(A * B)
    u = (p + sigma) * D
    c = p.dtype.type(2 / math.pi)
    f1 = c / np.sqrt(1 - u * u)
    return c * np.arcsin(u), f1 * D, -f1 * u / (2 * A), -f1 * u / (2 * B)


def _walk(cg, oracle, k, sc, gamma2, bound):
    """(value, A, B) of the kernel object k on the pair scalars sc; bound = False: A and B are None."""
    shape, dt = sc["p"].shape, sc["p"].dtype
    if isinstance(k, cg.Constant):
        c = np.full(shape, k.c, dtype=dt)
        return c, (np.abs(c) if bound else None), (np.zeros(shape) if bound else None)
    if isinstance(k, cg.Sum):
        parts = [_walk(cg, oracle, a, sc, gamma2, bound) for a in k.args]
        return sum(v for v, _, _ in parts), (sum(a for _, a, _ in parts) if bound else None), (sum(b for _, _, b in parts) if bound else None)
    if isinstance(k, (cg.Product, cg.Power)):
        v, A, B = np.ones(shape, dtype=dt), (np.ones(shape) if bound else None), (np.zeros(shape) if bound else None)
        for a in (k.args if isinstance(k, cg.Product) else (k.k,) * k.p):
            va, Aa, Ba = _walk(cg, oracle, a, sc, gamma2, bound)
            v = v * va
            if bound:
                A, B = A * Aa, B * Aa + A * Ba
        return v, A, B
    if isinstance(k, cg.Lengthscale):
        return _walk(cg, oracle, k.k, sc, gamma2 / k.l ** 2, bound)
    if isinstance(k, cg.NeuralNetwork):
        v, vp, vq, vs = nn_partials(dt.type(k.sigma), sc["p"], sc["q"], sc["s"])
        if not bound:
            return v, None, None
        return v, np.abs(v), np.abs(vp) * sc["pbar"] + np.abs(vq) * sc["q"] + np.abs(vs) * sc["s"]
    if isinstance(k, cg.IsotropicKernel):
        u = dt.type(gamma2) * sc["r2"]
        v, d1 = leaf_profile(cg, oracle, k, u)
        if not bound:
            return v, None, None
        with np.errstate(invalid="ignore"):
            S = np.where(u == 0, 0.0, np.abs(d1) * u)            # the limit 0 of |φ′(u)| u at r = 0 for the singular profiles
        return v, np.abs(v), S
    if isinstance(k, (cg.Dot, cg.ExponentialDot)):
        v, d1 = leaf_profile(cg, oracle, k, sc["p"])
        return v, (np.abs(v) if bound else None), (np.abs(d1) * sc["pbar"] if bound else None)
    raise NotImplementedError(type(k).__name__)


def pair_scalars(X, Y):
    sc = dict(G.pair_scalars(X, Y))
    sc["pbar"] = np.abs(np.asarray(X, dtype=np.float64)) @ np.abs(np.asarray(Y, dtype=np.float64)).T
    return sc


def matrix(cg, oracle, k, X, Y):
    """k(x_i, y_j) in fp64, (n, m)."""
    return _walk(cg, oracle, k, pair_scalars(X, Y), 1.0, False)[0]


def majorant(cg, oracle, k, X, Y):
    """K̄ (module docstring), (n, m)."""
    _, A, B = _walk(cg, oracle, k, pair_scalars(X, Y), 1.0, True)
    return A + B


# ---- the device's formation order in float32 --------------------------------------------------------------------------------------------
def matrix_float32(cg, oracle, k, X, Y):
    """The entries as the kernels form them, in float32 numpy arithmetic (no fused multiply-adds): r² and p by ascending-l sums of the
    direct differences and products, q and s the same, every leaf in float32."""
    f32 = np.float32
    X = np.asarray(X, dtype=f32); Y = np.asarray(Y, dtype=f32)
    n, d = X.shape; m = Y.shape[0]
    r2, p = np.zeros((n, m), f32), np.zeros((n, m), f32)
    q, s = np.zeros(n, f32), np.zeros(m, f32)
    for l in range(d):
        R = X[:, None, l] - Y[None, :, l]
        r2 += R * R; p += X[:, None, l] * Y[None, :, l]
        q += X[:, l] * X[:, l]; s += Y[:, l] * Y[:, l]
    sc = {"r2": r2, "p": p, "q": np.broadcast_to(q[:, None], (n, m)), "s": np.broadcast_to(s[None, :], (n, m))}
    v = _walk(cg, oracle, k, sc, 1.0, False)[0]
    assert v.dtype == f32, v.dtype
    return v


def mvm_float32(cg, oracle, k, X, Y, A):
    """G a with matrix_float32's entries, the columns accumulated in ascending j in float32."""
    K = matrix_float32(cg, oracle, k, X, Y)
    A = np.asarray(A, dtype=np.float32).reshape(K.shape[1], -1)
    out = np.zeros((K.shape[0], A.shape[1]), np.float32)
    for j in range(K.shape[1]):
        out += K[:, j, None] * A[None, j, :]
    return out.astype(np.float64)


# ---- the inputs both test files use -----------------------------------------------------------------------------------------------------
EXTRA = ["exp+dot", "gammaexp(1.5)*dot", "maternp0+dot", "matern(2.3)+dot"]
SLOW = "matern(2.3)+dot"              # Bessel functions in the reference: the two smallest shapes only

# (n, m, d, x is y, options)
SHAPES = [(333, 517, 3, False, {"jsplit": 3}), (130, 130, 5, True, {}), (70, 193, 32, False, {}), (100, 37, 33, False, {}), (100, 70, 70, False, {}),
          (1, 1, 3, False, {}), (65, 9, 3, False, {})]
SMALLEST = SHAPES[5:]


def kernels(cg):
    """name -> kernel: the eight of grad_mixed_ref.kernels and the four with leaves the gradient kernels refuse."""
    ks = dict(G.kernels(cg))
    ks.update({"exp+dot": cg.Exponential() + cg.Dot(), "gammaexp(1.5)*dot": cg.GammaExponential(1.5) * cg.Dot(),
               "maternp0+dot": cg.MaternP(0) + cg.Dot(), "matern(2.3)+dot": cg.Matern(2.3) + cg.Dot()})
    return ks


def shapes_of(name):
    return SMALLEST if name == SLOW else SHAPES


def clouds32(name, n, m, d, same):
    """grad_mixed_ref.clouds rounded to fp32 (both dtypes see the same points), as fp64 arrays."""
    X, Y = G.clouds(name, n, m, d, same)
    X = X.astype(np.float32).astype(np.float64)
    return X, (X if same else Y.astype(np.float32).astype(np.float64))


def weights32(m, nrhs=1, seed=11):
    return np.random.default_rng(seed).standard_normal((m, nrhs)).astype(np.float32).astype(np.float64)
