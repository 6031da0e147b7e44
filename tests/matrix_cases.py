"""Shared by tests/test_gpu_matrix.py (device) and tests/test_matrix_bound_host.py (no GPU): the point clouds, the fp64 reference
and the ENTRYWISE error bound of Matrix(G), and an fp32 emulation of the matrix kernels' own order of operations.

Bound (a condition, not a measurement; TOL = 1e-5 fp32 / 1e-12 fp64, BASELINE's contracts; tiny = smallest normal, since denormal
results may flush):
  * isotropic:    |M_ij - ref_ij| <= TOL max(1, L_ij / 10) |ref_ij| + tiny,  L_ij = -ln(|ref_ij| / |phi(0)|)  — the profile's exp
    has condition number L in its argument (tests/test_gpu_grad_rowwise.py and rowwise_err of tests/test_gpu_parity.py);
  * dot product:  |M_ij - ref_ij| <= TOL (|phi(s_ij)| + |phi'(s_ij)| sum_l |x_il| |y_jl|) + tiny  — x . y cancels, so the error of
    s scales with sum |x_l| |y_l| and reaches the entry through phi'.
Composites use the same two forms with phi, phi' of the composite."""
import numpy as np

F32, F64 = np.float32, np.float64
TOL = {F32: 1e-5, F64: 1e-12}


def tiny(dt):
    return float(np.finfo(dt).tiny)


def is_iso(o, ko):
    return ko.trait == o.ISOTROPIC


def lengthscale_of(ko):
    return float(getattr(ko, "lengthscale", 1.0))


def iso_cloud(rng, n, m, d, dt, lscale=1.0, far=8, copies=4, spread=0.8, shift=0.2):
    """X, Y = spread randn + shift / spread randn; `far` rows of X moved 6..10 lengthscales outside the cloud (add_far of
    tests/test_gpu_grad_rowwise.py) and `copies` rows of X copied from Y (s = 0 exactly).  Returns X, Y, far rows, copied rows."""
    X = spread * rng.standard_normal((n, d)) + shift
    Y = spread * rng.standard_normal((m, d))
    far = min(far, max(0, n - 1)); copies = min(copies, max(0, n - 1 - far), m)
    idx = rng.choice(n, size=far + copies, replace=False) if far + copies else np.zeros(0, dtype=np.int64)
    fi, ci = idx[:far], idx[far:]
    c = X.mean(axis=0); reach = np.abs(X - c).max()
    for i, r in zip(fi, np.linspace(6.0, 10.0, max(far, 1))):
        v = rng.standard_normal(d); v /= np.linalg.norm(v)
        X[i] = c + (reach + r * lscale) * v
    X = X.astype(dt); Y = Y.astype(dt)
    for t, i in enumerate(ci):
        X[i] = Y[(7 * t + 1) % m]
    return X, Y, [int(i) for i in fi], [int(i) for i in ci]


def dot_cloud(rng, n, m, d, dt, unit_ball=False):
    """0.8 randn / sqrt(d) on both sides; unit_ball: x / sqrt(1 + |x|^2), the NeuralNetwork kernel's normalisation (sigma = 0), which
    keeps |x . y| < 1 for the asin profile."""
    X = 0.8 * rng.standard_normal((n, d)) / np.sqrt(d)
    Y = 0.8 * rng.standard_normal((m, d)) / np.sqrt(d)
    if unit_ball:
        X = X / np.sqrt(1 + (X ** 2).sum(1))[:, None]; Y = Y / np.sqrt(1 + (Y ** 2).sum(1))[:, None]
    return X.astype(dt), Y.astype(dt)


def cloud(o, ko, rng, n, m, d, dt, unit_ball=False):
    if is_iso(o, ko):
        return iso_cloud(rng, n, m, d, dt, lscale=lengthscale_of(ko))[:2]
    return dot_cloud(rng, n, m, d, dt, unit_ball)


def wide_cloud(o, ko, rng, n, m, d, dt):
    """Clouds for d > 64 (the generic kernels).  At spread 0.8 every fp32 entry of EQ would underflow (|x - y|^2 / 2 ~ 0.64 d), so the
    spread and the shift shrink with d by sqrt(8 / d): |x - y|^2 as at d = 8.  Sequential fp32 FMA accumulation over d terms leaves a relative
    error of about sqrt(d) u in s (worst case d u), which the profile's exp multiplies by L; beyond L = 10 the bound allows
    TOL / 10 = 16.8 u per unit of L.  At d = 256, sqrt(d) u = 16 u: rows far from the cloud sit AT the bound in exactly rounded
    arithmetic (emulate_f32: 0.87 .. 1.15 of it), so no kernel can be held to it there, and d > 128 runs without far rows (L <= 10
    on the cloud itself for unit lengthscales).  tests/test_matrix_bound_host.py asserts the emulation's headroom on these clouds."""
    if is_iso(o, ko):
        return iso_cloud(rng, n, m, d, dt, lscale=lengthscale_of(ko), far=8 if d <= 128 else 0, spread=0.8 * np.sqrt(8.0 / d),
                         shift=0.2 * np.sqrt(8.0 / d))[:2]
    return dot_cloud(rng, n, m, d, dt)


def reference_and_bound(o, ko, X, Y, dt):
    """(ref, bound) of every entry, n x m, on the data as rounded to dt (fp64 arithmetic, direct differences)."""
    ref = o.matrix(ko, X, Y, dt)
    aref = np.abs(ref)
    if is_iso(o, ko):
        phi0 = abs(float(o.profile(ko, np.zeros(1), dt)[0]))
        with np.errstate(divide="ignore"):
            L = -np.log(aref / phi0)
        bound = np.where(aref > 0, TOL[dt] * np.maximum(1.0, L / 10.0) * aref, 0.0)
    else:
        Xd = X.astype(F64); Yd = Y.astype(F64)
        v, d1, _ = o.profile_derivatives(ko, Xd @ Yd.T, dt)
        bound = TOL[dt] * (np.abs(v) + np.abs(d1) * (np.abs(Xd) @ np.abs(Yd).T))
    return ref, bound + tiny(dt)


def worst_entry(got, ref, bound):
    """(err / bound, i, j) of the worst entry; a non-finite entry is infinitely wrong."""
    got = np.asarray(got, dtype=F64)
    with np.errstate(invalid="ignore"):
        r = np.where(np.isfinite(got), np.abs(got - ref) / bound, np.inf)
    i, j = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i, j]), int(i), int(j)


def emulate_f32(o, ko, X, Y):
    """What an exactly rounded fp32 evaluation in the matrix kernels' order gives: differences, scale by 1/l, FMA accumulation over
    the dimensions (one rounding per step), the profile on the fp32 argument, one final rounding.  Composites accumulate the unscaled
    s (their factors carry the lengthscales)."""
    iso = is_iso(o, ko)
    single = isinstance(ko, o.Kernel)
    g = F32(1.0 / ko.lengthscale) if (iso and single) else F32(1)
    s = np.zeros((X.shape[0], Y.shape[0]), F32)
    for l in range(X.shape[1]):
        if iso:
            q = ((X[:, l][:, None] - Y[:, l][None, :]).astype(F32) * g).astype(F32)
            s = (q.astype(F64) ** 2 + s.astype(F64)).astype(F32)
        else:
            s = (X[:, l][:, None].astype(F64) * Y[:, l][None, :].astype(F64) + s.astype(F64)).astype(F32)
    k1 = o.Kernel(ko.family, p=ko.p, param=ko.param, power=ko.power, scale=ko.scale) if (iso and single) else ko
    return o.profile(k1, s.astype(F64), F32).astype(F32)
