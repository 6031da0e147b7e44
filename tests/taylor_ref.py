"""Reference restatement of src/taylor.jl:7-57 (taylor! / taylor_recursion) in numpy / fp64 over a tests/barneshut_ref.py-style tree, and
a numpy Paige-Saunders MINRES; shared by tests/test_bh_taylor_host.py (no GPU) and tests/test_gpu_bh_taylor.py (device).

A compressed node v adds, for a row x with ri = x - c[v] and s = |ri|^2,
    f0(s) sums[v] - 2 f1(s) (ri . m1[v]),      sums = sum w_j,   m1 = sum w_j y_j - sums c   (src/taylor.jl:15-18, 43-50),
where c is the |w|-weighted centre of mass (use_com) or the ball centre.  `jet(s) -> (f0, f1, b0, lf)`: the kernel and its derivative
w.r.t. the squared distance, an absolute error bound b0 of f0 and the relative allowance lf of f1 (zeros on the host, where the
evaluation is fp64; the device test passes tests/matrix_cases.py's isotropic convention)."""
import numpy as np

F64 = np.float64
LD = np.longdouble


def moments(tree, Y, w, eps, use_com=True, centers=None):
    """Per node, over the tree's ranges, accumulated in np.longdouble like barneshut_ref.moments and rounded to fp64 at the end:
      sums  sum w                     sabs  sum |w|                    mabs  sum |w| |y_l|   (nnodes x d)
      cen   the expansion centre: `centers` when given (the device's own, as rounded), otherwise sum |w| y / (sum |w| + eps) (use_com)
            or the tree's ball centre
      m1    sum w y - sums cen."""
    Yl = np.asarray(Y, dtype=F64).astype(LD); wl = np.asarray(w, dtype=F64).astype(LD)
    idx = tree["indices"].astype(np.int64)
    nn, d = len(tree["lo"]), Yl.shape[1]
    out = {"sums": np.zeros(nn), "sabs": np.zeros(nn), "cen": np.zeros((nn, d)), "m1": np.zeros((nn, d)), "mabs": np.zeros((nn, d))}
    for v in range(nn):
        j = idx[tree["lo"][v]:tree["hi"][v]]
        aw = np.abs(wl[j])
        S, A = wl[j].sum(), aw.sum()
        if centers is not None:
            c = np.asarray(centers[v], dtype=F64).astype(LD)
        elif use_com:
            c = ((aw[:, None] * Yl[j]).sum(0) / (A + LD(eps))).astype(F64).astype(LD)
        else:
            c = np.asarray(tree["centers"][v], dtype=F64).astype(LD)
        out["sums"][v] = F64(S); out["sabs"][v] = F64(A)
        out["cen"][v] = c.astype(F64)
        out["m1"][v] = ((wl[j][:, None] * Yl[j]).sum(0) - S * c).astype(F64)
        out["mabs"][v] = (aw[:, None] * np.abs(Yl[j])).sum(0).astype(F64)
    return out


def recursion(tree, X, Y, w, cen, sums, m1, theta, entries, jet, band_eps=None):
    """taylor_recursion for every row of X, the rows that reach a node carried as an index set (barneshut_ref.recursion).
    entries(rows, P) -> (ref, bound) for the leaves.  Returns the dict of barneshut_ref.recursion: want / babs / eabs / ambiguous /
    compressed / visits.  A far-field term adds b0 |sums| + lf 2 |f1| sum_l |ri_l| |m1_l| to babs and |f0| |sums| + 2 |f1| sum_l |ri_l| |m1_l|
    to eabs."""
    X = np.asarray(X); Y = np.asarray(Y)
    X64 = X.astype(F64)
    n = X.shape[0]
    idx = tree["indices"].astype(np.int64)
    w64 = np.asarray(w, dtype=F64)
    cen = np.asarray(cen, dtype=F64); sums64 = np.asarray(sums, dtype=F64); m164 = np.asarray(m1, dtype=F64)
    out = {"want": np.zeros(n), "babs": np.zeros(n), "eabs": np.zeros(n), "ambiguous": np.zeros(n, dtype=bool),
           "compressed": np.zeros(n, dtype=np.int64), "visits": 0}
    if len(tree["lo"]) == 0 or n == 0:
        return out
    stack = [(0, np.arange(n))]
    while stack:
        v, act = stack.pop()
        if act.size == 0:
            continue
        out["visits"] += act.size
        lo, hi, l, r = int(tree["lo"][v]), int(tree["hi"][v]), int(tree["left"][v]), int(tree["right"][v])
        if l < 0:
            j = idx[lo:hi]
            ref, bnd = entries(act, Y[j])
            out["want"][act] += ref @ w64[j]; out["babs"][act] += bnd @ np.abs(w64[j]); out["eabs"][act] += np.abs(ref) @ np.abs(w64[j])
            continue
        c = cen[v]
        ri = X64[act] - c
        s = (ri ** 2).sum(1)
        dist = np.sqrt(s)
        hr = float(tree["radii"][v])
        if band_eps is not None:
            band = 64 * band_eps * (hr + theta * (np.linalg.norm(X64[act], axis=1) + np.linalg.norm(c)))
            out["ambiguous"][act] |= np.abs(hr - theta * dist) <= band
        far = hr < theta * dist
        if far.any():
            rows = act[far]
            f0, f1, b0, lf = jet(s[far])
            dot = ri[far] @ m164[v]
            adot = np.abs(ri[far]) @ np.abs(m164[v])
            out["want"][rows] += f0 * sums64[v] - 2 * f1 * dot
            out["babs"][rows] += b0 * abs(sums64[v]) + lf * 2 * np.abs(f1) * adot
            out["eabs"][rows] += np.abs(f0) * abs(sums64[v]) + 2 * np.abs(f1) * adot
            out["compressed"][rows] += 1
        stack.append((r, act[~far])); stack.append((l, act[~far]))
    return out


def far_jet(o, mc, ko, dt):
    """jet(s) of `recursion` under the project's isotropic condition convention (tests/matrix_cases.py): f0 within
    TOL max(1, L / 10) |f0| + tiny and f1 within the relative TOL max(1, L / 10), L = -ln(|f0| / phi(0)); o = covgram_oracle."""
    phi0 = abs(float(o.profile(ko, np.zeros(1), dt)[0]))

    def jet(s):
        f0, f1, _ = o.profile_derivatives(ko, s, dt)
        with np.errstate(divide="ignore"):
            L = -np.log(np.abs(f0) / phi0)
        lf = mc.TOL[dt] * np.maximum(1.0, L / 10.0)
        return f0, f1, np.where(np.abs(f0) > 0, lf * np.abs(f0), 0.0) + mc.tiny(dt), lf
    return jet


def taylor(tree, X, Y, w, theta, entries, jet, eps, use_com=True):
    """taylor!(b, F, w, 1, 0, theta; use_com) in fp64 with its own moments: the product alone (no alpha, beta, D)."""
    mo = moments(tree, Y, w, eps, use_com)
    return recursion(tree, X, Y, w, mo["cen"], mo["sums"], mo["m1"], theta, entries, jet)["want"]


def minres(A, b, reltol=1e-10, maxiter=None, shift=0.0):
    """Paige-Saunders MINRES for a symmetric A (a matrix, or a function v -> A v), x0 = 0: (x, iterations, recurrence residual norm).
    Stops when the recurrence's residual norm <= reltol |b|."""
    mv = (lambda v: A @ v) if isinstance(A, np.ndarray) else A
    b = np.asarray(b, dtype=F64)
    n = b.shape[0]
    maxiter = n if maxiter is None else maxiter
    x = np.zeros(n)
    r1 = np.zeros(n); r2 = b.copy()
    beta = float(np.linalg.norm(r2))
    tol = reltol * beta
    if beta == 0:
        return x, 0, 0.0
    oldb, dbar, epsln, phibar, cs, sn = 1.0, 0.0, 0.0, beta, -1.0, 0.0
    w1 = np.zeros(n); w2 = np.zeros(n)
    it = 0
    tiny = np.finfo(F64).tiny
    while it < maxiter and phibar > tol:
        v = r2 / beta if beta > 0 else np.zeros(n)
        y = mv(v) + shift * v
        y = y - (beta / oldb) * r1
        alfa = float(v @ y)
        y = y - (alfa / max(beta, tiny)) * r2
        r1, r2 = r2, y
        oldb, beta = beta, float(np.linalg.norm(r2))
        oldeps = epsln
        delta = cs * dbar + sn * alfa
        gbar = sn * dbar - cs * alfa
        epsln, dbar = sn * beta, -cs * beta
        gamma = max(float(np.hypot(gbar, beta)), tiny)
        cs, sn = gbar / gamma, beta / gamma
        phi, phibar = cs * phibar, sn * phibar
        wn = (v - oldeps * w1 - delta * w2) / gamma
        w1, w2 = w2, wn
        x = x + phi * wn
        it += 1
    return x, it, phibar
