"""fp64 numpy reference of the value-gradient-Hessian-kernel Gramian (tests/test_vgh_host.py pins it against torch.func;
tests/test_gpu_vgh.py compares the device kernel with it).  Block (i, j) is the (1 + d + d^2) x (1 + d + d^2) joint covariance of
[f, grad f, vec hess f]: entry (row functional on x_i, column functional on y_j) of k(x_i, y_j), the functionals being id, d/d._a and
d^2/d._a d._b.  Flat blocks: entry 0 the value, 1 ... d the gradient, 1 + d + a + b d the Hessian component (a, b).  With the block
input (a_v, a_g, A), Abar = A + A', t = tr A, the block output (b_v, b_g, B) is

  isotropic, k = f(|r|^2 / l^2), r = x - y, g_m = 2^m f^(m) l^(-2m):   u = Abar r, q = r'u / 2, rho = r . a_g,
      c1 = g1 a_v - g2 rho + g2 t + g3 q,   c2 = g2 a_v - g3 rho + g3 t + g4 q
      b_v = g0 a_v - g1 rho + g1 t + g2 q
      b_g = c1 r - g1 a_g + g2 u
      B   = c1 I + c2 r r' - g2 (a_g r' + r a_g') + g2 Abar + g3 (u r' + r u')
  dot product, k = f(x . y), g_m = f^(m):                               w = Abar x, q = x'w / 2, rho = x . a_g,
      b_v = g0 a_v + g1 rho + g2 q
      b_g = (g1 a_v + g2 rho + g3 q) y + g1 a_g + g2 w
      B   = (g2 a_v + g3 rho + g4 q) y y' + g2 (a_g y' + y a_g') + g2 Abar + g3 (y w' + w y')

A kernel is a tuple (name, param, lengthscale, scale) as in tests/hessian_ref.py."""
import numpy as np

import hessian_ref as R


def jet(kern, s):
    """(g0, ..., g4) for the raw argument s = |r|^2 (isotropic; lengthscale and the factors 2^m included) or x . y, times scale."""
    name, p, l, scale = kern
    g2, g3, g4 = R.jet(kern, s)
    sl = s / (l * l) if name in R.ISO else s
    f0 = R.profile(kern, sl)
    if name == "EQ": f1 = -f0 / 2
    elif name == "RQ": f1 = -0.5 * (1 + sl / (2 * p)) ** (-p - 1)
    elif name == "Cauchy": f1 = -f0 * f0
    elif name == "IMQ": f1 = -0.5 * (sl + p * p) ** -1.5
    elif name == "ExponentialDot": f1 = f0
    elif name == "Dot": f1 = np.ones_like(sl)
    else: raise KeyError(name)
    if name in R.ISO:
        return scale * f0, scale * 2.0 * f1 / (l * l), g2, g3, g4
    return scale * f0, scale * f1, g2, g3, g4


def vgh_mul(kern, X, Y, a, absolute=False, chunk=256):
    """G a for the rows X: (len(X) (1 + d + d^2),) flat.  absolute: the same product with every term of the block and of a in absolute
    value (|Abar| formed from |A|)."""
    X = np.asarray(X, np.float64); Y = np.asarray(Y, np.float64)
    n, d = X.shape; m = Y.shape[0]
    bd = 1 + d + d * d
    a = np.asarray(a, np.float64).reshape(m, bd)
    if absolute:
        a = np.abs(a)
    av, ag = a[:, 0], a[:, 1:1 + d]
    A = a[:, 1 + d:].reshape(m, d, d).transpose(0, 2, 1)    # A[a, b] = flat a + b d
    Ab = A + A.transpose(0, 2, 1)
    t = np.trace(A, axis1=1, axis2=2)
    I = np.eye(d)
    iso = kern[0] in R.ISO
    sg = 1.0 if (absolute or not iso) else -1.0             # the sign of the terms that are odd in r
    bv = np.zeros(n); bg = np.zeros((n, d)); B = np.zeros((n, d, d))
    for j0 in range(0, m, chunk):
        Yc, Abc, tc, avc, agc = Y[j0:j0 + chunk], Ab[j0:j0 + chunk], t[j0:j0 + chunk], av[j0:j0 + chunk], ag[j0:j0 + chunk]
        if iso:
            r = X[:, None, :] - Yc[None, :, :]
            s = (r * r).sum(-1)
            vec, outer = r, r
        else:
            s = X @ Yc.T
            vec = np.broadcast_to(X[:, None, :], (n, len(Yc), d))
            outer = np.broadcast_to(Yc[None, :, :], (n, len(Yc), d))
        g0, g1, g2, g3, g4 = jet(kern, s)
        if absolute:
            g0, g1, g2, g3, g4, vec, outer = np.abs(g0), np.abs(g1), np.abs(g2), np.abs(g3), np.abs(g4), np.abs(vec), np.abs(outer)
        u = np.einsum("jab,ijb->ija", Abc, vec)
        q = 0.5 * (vec * u).sum(-1)
        rho = np.einsum("ijc,jc->ij", vec, agc)
        tt = tc[None, :] if iso else 0.0                    # the trace terms exist for the isotropic kernels only
        c0 = g0 * avc[None, :] + sg * g1 * rho + g1 * tt + g2 * q
        c1 = g1 * avc[None, :] + sg * g2 * rho + g2 * tt + g3 * q
        c2 = g2 * avc[None, :] + sg * g3 * rho + g3 * tt + g4 * q
        bv += c0.sum(1)
        bg += np.einsum("ij,ija->ia", c1, outer) + sg * np.einsum("ij,ja->ia", g1, agc) + np.einsum("ij,ija->ia", g2, u)
        B += np.einsum("ij,jab->iab", g2, Abc)
        uo = np.einsum("ij,ija,ijb->iab", g3, u, outer) + sg * np.einsum("ij,ja,ijb->iab", g2, agc, outer)
        B += uo + uo.transpose(0, 2, 1)
        B += np.einsum("ij,ija,ijb->iab", c2, outer, outer)
        if iso:
            B += c1.sum(1)[:, None, None] * I
    out = np.empty((n, bd))
    out[:, 0] = bv; out[:, 1:1 + d] = bg
    out[:, 1 + d:] = B.transpose(0, 2, 1).reshape(n, d * d)  # flat a + b d
    return out.reshape(n * bd)


def vgh_matrix(kern, X, Y):
    """The dense n (1 + d + d^2) x m (1 + d + d^2) matrix, column by column (small shapes only)."""
    n, d = X.shape; m = Y.shape[0]
    N = m * (1 + d + d * d)
    cols = []
    for c in range(N):
        e = np.zeros(N); e[c] = 1.0
        cols.append(vgh_mul(kern, X, Y, e))
    return np.stack(cols, axis=1)
