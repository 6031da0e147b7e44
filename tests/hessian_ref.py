"""fp64 numpy reference of the Hessian-kernel Gramian (tests/test_hessian_host.py pins it against torch.func; tests/test_gpu_hessian.py
compares the device kernel with it).  Block (i, j) is T[(a,b),(c,e)] = d^4 k(x_i, y_j) / dx_a dx_b dy_c dy_e; with the block input as a
d x d matrix A (flat entry a + b d), Abar = A + A', t = tr A, the block output B (d x d, flat a + b d) is

  isotropic, k = f(|r|^2 / l^2), r = x - y, g_m = 2^m f^(m) l^(-2m):   u = Abar r, q = r'u / 2
      B = g2 (t I + Abar) + g3 (q I + t r r' + u r' + r u') + g4 q r r'
  dot product, k = f(x . y), g_m = f^(m):                               w = Abar x, q = x'w / 2
      B = g2 Abar + g3 (y w' + w y') + g4 q y y'

A kernel is a tuple (name, param, lengthscale, scale), name in PROFILES."""
import numpy as np

ISO = ("EQ", "RQ", "Cauchy", "IMQ")
DOT = ("ExponentialDot", "Dot")
PROFILES = ISO + DOT


def profile(kern, s):
    """f(s) of the un-scaled profile (s already divided by l^2)."""
    name, p = kern[0], kern[1]
    if name == "EQ": return np.exp(-s / 2)
    if name == "RQ": return (1 + s / (2 * p)) ** (-p)
    if name == "Cauchy": return 1 / (1 + s)
    if name == "IMQ": return 1 / np.sqrt(s + p * p)
    if name == "ExponentialDot": return np.exp(s)
    if name == "Dot": return s
    raise KeyError(name)


def jet(kern, s):
    """(g2, g3, g4) for the raw argument s = |r|^2 (isotropic; lengthscale and the factors 2^m included) or x . y, times scale."""
    name, p, l, scale = kern
    if name in ISO:
        s = s / (l * l)
    if name == "EQ":
        f = np.exp(-s / 2); d = (f / 4, -f / 8, f / 16)
    elif name == "RQ":
        u = 1 + s / (2 * p)
        d = ((p + 1) / (4 * p) * u ** (-p - 2), -(p + 1) * (p + 2) / (8 * p * p) * u ** (-p - 3),
             (p + 1) * (p + 2) * (p + 3) / (16 * p ** 3) * u ** (-p - 4))
    elif name == "Cauchy":
        v = 1 / (1 + s); d = (2 * v ** 3, -6 * v ** 4, 24 * v ** 5)
    elif name == "IMQ":
        u = s + p * p; d = (0.75 * u ** -2.5, -15 / 8 * u ** -3.5, 105 / 16 * u ** -4.5)
    elif name == "ExponentialDot":
        f = np.exp(s); d = (f, f, f)
    elif name == "Dot":
        z = np.zeros_like(s); d = (z, z, z)
    else:
        raise KeyError(name)
    if name in ISO:
        return tuple(scale * (2.0 ** m) * dm / l ** (2 * m) for m, dm in zip((2, 3, 4), d))
    return tuple(scale * dm for dm in d)


def hess_mul(kern, X, Y, a, absolute=False, chunk=256):
    """G a for the rows X: (len(X) d^2,) flat.  absolute: the same product with every term of T and of a in absolute value."""
    X = np.asarray(X, np.float64); Y = np.asarray(Y, np.float64)
    n, d = X.shape; m = Y.shape[0]
    A = np.asarray(a, np.float64).reshape(m, d, d)
    if absolute:
        A = np.abs(A)
    Ab = A + A.transpose(0, 2, 1)
    t = np.trace(A, axis1=1, axis2=2)
    I = np.eye(d)
    B = np.zeros((n, d, d))
    iso = kern[0] in ISO
    for j0 in range(0, m, chunk):
        Yc, Abc, tc = Y[j0:j0 + chunk], Ab[j0:j0 + chunk], t[j0:j0 + chunk]
        if iso:
            r = X[:, None, :] - Yc[None, :, :]
            s = (r * r).sum(-1)
            vec, outer = r, r
        else:
            s = X @ Yc.T
            vec = np.broadcast_to(X[:, None, :], (n, len(Yc), d))
            outer = np.broadcast_to(Yc[None, :, :], (n, len(Yc), d))
        g2, g3, g4 = jet(kern, s)
        if absolute:
            g2, g3, g4, vec, outer = np.abs(g2), np.abs(g3), np.abs(g4), np.abs(vec), np.abs(outer)
        u = np.einsum("jab,ijb->ija", Abc, vec)
        q = 0.5 * (vec * u).sum(-1)
        B += np.einsum("ij,jab->iab", g2, Abc)
        uo = np.einsum("ij,ija,ijb->iab", g3, u, outer)
        B += uo + uo.transpose(0, 2, 1)
        if iso:
            B += ((g2 * tc[None, :]).sum(1) + (g3 * q).sum(1))[:, None, None] * I
            B += np.einsum("ij,ija,ijb->iab", g3 * tc[None, :] + g4 * q, outer, outer)
        else:
            B += np.einsum("ij,ija,ijb->iab", g4 * q, outer, outer)
    return B.transpose(0, 2, 1).reshape(n * d * d)          # flat a + b d (B is symmetric)


def hess_matrix(kern, X, Y):
    """The dense (n d^2) x (m d^2) matrix, column by column (small shapes only)."""
    n, d = X.shape; m = Y.shape[0]
    cols = []
    for c in range(m * d * d):
        e = np.zeros(m * d * d); e[c] = 1.0
        cols.append(hess_mul(kern, X, Y, e))
    return np.stack(cols, axis=1)


def cond_L(kern, X, Y):
    """L_i = -ln(max_j k(x_i, y_j) / k(0)) (isotropic) or max_j |x_i . y_j| (dot product): the condition of the profile's exp."""
    X = np.asarray(X, np.float64); Y = np.asarray(Y, np.float64)
    if kern[0] in ISO:
        s = np.maximum(((X[:, None, :] - Y[None, :, :]) ** 2).sum(-1).min(axis=1), 0.0) / kern[2] ** 2
        return np.maximum(0.0, -np.log(profile(kern, s) / profile(kern, np.zeros(1))[0]))
    return np.abs(X @ Y.T).max(axis=1)
