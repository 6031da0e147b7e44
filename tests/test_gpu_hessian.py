"""Entry-wise parity of the Hessian-kernel Gramian MVM (covgram_hess_mvm, csrc/hess_mvm.hpp) with the fp64 numpy reference of
tests/hessian_ref.py (itself pinned against torch.func in tests/test_hessian_host.py).

Error measure, as in tests/test_gpu_grad_rowwise.py: for every checked entry  e = |b - ref| / (|alpha| absref + |beta| |y0|), absref = the
same product with every term of T and of a in absolute value;  e <= 1e-12 (fp64) / 1e-5 (fp32) times max(1, L_i / 10), L_i =
-ln(max_j k(x_i, y_j) / k(0)) (dot product: max_j |x_i . y_j|).  An entry whose absref is 0 must be exactly 0.  The info key
last_hess_path is asserted before any number is compared.

Isotropic clouds are N(0, I) with lengthscales of c sqrt(d), c != 1 (a unit lengthscale at d = 32 puts |r|^2 / 2 ~ 32 + and the far
rows' entries below fp32's normal range); the far row sits 8 lengthscales outside the cloud."""
import ctypes as C

import numpy as np
import pytest
import torch

import hessian_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TOL = {F32: 1e-5, F64: 1e-12}
NANV = float("nan")
DIMS = [1, 2, 3, 5, 8, 16, 32]
PROFILES = [("EQ", 0.0, 0.8, 1.0), ("RQ", 1.5, 0.7, 1.3), ("Cauchy", 0.0, 1.2, 1.0), ("IMQ", 1.3, 0.9, 0.6), ("ExponentialDot", 0.0, 1.0, 1.4),
            ("Dot", 0.0, 1.0, 1.0)]


def row_subset(n, wg, rng, extra=()):
    """The rows tests/test_gpu_grad_rowwise.py checks: first, last, the ragged tail (or the last wave), one full workgroup, 32 random."""
    rows = {0, n - 1}
    rows.update(range(n - n % 64 if n % 64 else max(0, n - 64), n))
    w0 = wg if n >= 2 * wg else 0
    rows.update(range(w0, min(n, w0 + wg)))
    rows.update(int(r) for r in rng.choice(n, size=min(n, 32), replace=False))
    rows.update(extra)
    return np.array(sorted(rows), dtype=np.int64)


def make_kernel(cg, kern, d):
    """(covgram kernel, reference tuple) with the lengthscale factor of `kern` times sqrt(d) for the isotropic profiles."""
    name, p, lf, scale = kern
    l = lf * np.sqrt(d) if name in R.ISO else 1.0
    base = {"EQ": lambda: cg.EQ(), "RQ": lambda: cg.RQ(p), "Cauchy": lambda: cg.Cauchy(), "IMQ": lambda: cg.InverseMultiQuadratic(p),
            "ExponentialDot": lambda: cg.ExponentialDot(), "Dot": lambda: cg.Dot()}[name]()
    k = cg.Lengthscale(base, l) if name in R.ISO else base
    if scale != 1.0:
        k = scale * k
    return k, (name, p, float(l), scale)


def clouds(rng, kern, n, m, d, dt, same=False, far=True):
    """x, y and the index of the far row (isotropic only)."""
    if kern[0] in R.ISO:
        X = rng.standard_normal((n, d)).astype(dt)
        Y = X if same else (0.9 * rng.standard_normal((m, d)) + 0.1).astype(dt)
        if far and not same:
            v = rng.standard_normal(d); v /= np.linalg.norm(v)
            i = int(rng.integers(n))
            X[i] = (Y.mean(axis=0) + (np.abs(Y - Y.mean(axis=0)).max() + 8.0 * kern[2]) * v).astype(dt)
            return X, Y, [i]
        return X, Y, []
    s = 0.6 / np.sqrt(d)
    X = (s * rng.standard_normal((n, d)) + 0.05).astype(dt)
    Y = X if same else (s * rng.standard_normal((m, d))).astype(dt)
    return X, Y, []


def rowwise(kern, X, Y, a, b, y0, alpha, beta, rows, dt):
    """max over the checked entries of e / bound (<= 1 passes), printed figures included."""
    d = X.shape[1]; bd = d * d
    Xs = X[rows].astype(np.float64); Yd = Y.astype(np.float64)
    ref = R.hess_mul(kern, Xs, Yd, a).reshape(-1, bd)
    absref = R.hess_mul(kern, Xs, Yd, a, absolute=True).reshape(-1, bd)
    got = b.reshape(-1, bd)[rows].astype(np.float64)
    yb = np.zeros_like(got) if beta == 0 else y0.reshape(-1, bd)[rows].astype(np.float64)
    want = alpha * ref + beta * yb
    den = abs(alpha) * absref + abs(beta) * np.abs(yb)
    bound = TOL[dt] * np.maximum(1.0, R.cond_L(kern, Xs, Yd) / 10.0)
    assert np.all(np.isfinite(got)), "non-finite output"
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(den > 0, np.abs(got - want) / den, np.abs(got - want))   # an all-zero entry must come out zero
    worst = (e / bound[:, None]).max(axis=1)
    i = int(np.argmax(worst))
    print(f"hessian {kern} d={d} {np.dtype(dt).name} alpha={alpha} beta={beta}: worst row {int(rows[i])} e={e[i].max():.3e} = {worst[i]:.3f} x bound")
    return float(worst[i]), int(rows[i]), float(e[i].max())


def run_case(cg, kern_t, n, m, d, dt, seed, same=False, nrhs=1, rows=None, inplace=False):
    rng = np.random.default_rng(seed)
    k, kern = make_kernel(cg, kern_t, d)
    X, Y, far = clouds(rng, kern, n, m, d, dt, same=same)
    Xt = torch.from_numpy(X).cuda()
    G = cg.gramian(cg.HessianKernel(k), Xt) if same else cg.gramian(cg.HessianKernel(k), Xt, torch.from_numpy(Y).cuda())
    bd = d * d
    assert G.shape == (n * bd, m * bd)
    if rows is None:
        rows = np.arange(n)
    rows = np.array(sorted(set(int(r) for r in rows) | set(far)), dtype=np.int64)
    shape = (m * bd,) if nrhs == 1 else (m * bd, nrhs)
    a = rng.standard_normal(shape).astype(dt)
    y0 = rng.standard_normal((n * bd,) + shape[1:]).astype(dt)
    for alpha, beta in ((-0.7, 1.3), (1.6, 0.0)):
        if inplace:                                        # y aliases a (n == m): mul_(a, G, a)
            yt = torch.from_numpy(a.copy()).cuda()
            G.mul_(yt, yt, alpha, beta)
            yref = a
        else:
            yt = torch.from_numpy(y0.copy()).cuda() if beta != 0 else torch.full((n * bd,) + shape[1:], NANV, dtype=Xt.dtype, device="cuda")
            G.mul_(yt, torch.from_numpy(a).cuda(), alpha, beta)
            yref = y0
        assert cg.get_info("last_hess_path") == 1
        b = yt.cpu().numpy()
        for c in range(nrhs):
            sel = (lambda v: v) if nrhs == 1 else (lambda v: v[:, c])
            worst, row, e = rowwise(kern, X, Y, sel(a), sel(b), sel(yref), alpha, beta, rows, dt)
            assert worst <= 1.0, (kern, d, alpha, beta, c, "row", row, "error", e, "of its bound x", worst)
    return G


CASES = [(i, dt, d) for i in range(len(PROFILES)) for dt in (F64, F32) for d in (DIMS[i], DIMS[(i + 3) % 7])]


@pytest.mark.parametrize("i,dt,d", CASES, ids=[f"{PROFILES[i][0]}-{np.dtype(dt).name}-d{d}" for i, dt, d in CASES])
def test_profiles_dtypes_dimensions_ragged_with_far_row(cg, i, dt, d):
    """Every profile in both dtypes, every d of {1, 2, 3, 5, 8, 16, 32} in both dtypes; n = 193, m = 131 (ragged for every tile size),
    x != y, lengthscale != 1, a far row; alpha, beta != 0 on a random y and beta = 0 on a NaN-filled y."""
    run_case(cg, PROFILES[i], 193, 131, d, dt, seed=1000 + 10 * i + d)


@pytest.mark.parametrize("dt,d", [(F64, 3), (F32, 8), (F64, 16)])
def test_symmetric_gramian_and_in_place(cg, dt, d):
    """x = y (one point set), and y aliasing a: the library reads a from a private copy."""
    G = run_case(cg, PROFILES[0], 150, 150, d, dt, seed=20 + d, same=True)
    assert G.issymmetric()
    run_case(cg, PROFILES[1], 150, 150, d, dt, seed=30 + d, same=True, inplace=True)


@pytest.mark.parametrize("dt,d", [(F64, 5), (F32, 3)])
def test_matrix_right_hand_sides(cg, dt, d):
    run_case(cg, PROFILES[3], 97, 131, d, dt, seed=40 + d, nrhs=3)


@pytest.mark.parametrize("loc_host", [False, True])
@pytest.mark.parametrize("nrhs", [1, 3])
def test_c_abi_padded_leading_dimensions_and_host_pointers(cg, nrhs, loc_host):
    """covgram_hess_mvm directly: lda > m d^2, ldy > n d^2 (the padding rows of y must stay untouched), device and host pointers."""
    from covgram import _ffi
    from covgram.gramian import _Points
    rng = np.random.default_rng(50 + nrhs)
    n, m, d, dt = 70, 45, 3, F64
    k, kern = make_kernel(cg, PROFILES[0], d)
    X, Y, far = clouds(rng, kern, n, m, d, dt)
    px, py = _Points(torch.from_numpy(X).cuda()), _Points(torch.from_numpy(Y).cuda())
    bd = d * d
    lda, ldy = m * bd + 5, n * bd + 3
    a = rng.standard_normal((nrhs, lda)); y0 = rng.standard_normal((nrhs, ldy))
    spec = cg.require_hessian_spec(k, d)
    alpha, beta = 0.9, -0.4
    if loc_host:
        yh = y0.copy()
        ap, yp, loc = a.ctypes.data, yh.ctypes.data, _ffi.HOST
    else:
        at, yt = torch.from_numpy(a).cuda(), torch.from_numpy(y0.copy()).cuda()
        ap, yp, loc = at.data_ptr(), yt.data_ptr(), _ffi.DEVICE
    _ffi.check(_ffi.lib().covgram_hess_mvm(px.ctx.bind_stream(), _ffi.kref(spec), px.handle, py.handle, C.c_void_p(ap), lda, C.c_void_p(yp), ldy,
                                           nrhs, alpha, beta, loc))
    assert cg.get_info("last_hess_path") == 1
    got = yh if loc_host else yt.cpu().numpy()
    assert np.array_equal(got[:, n * bd:], y0[:, n * bd:]), "padding rows of y were written"
    for c in range(nrhs):
        worst, row, e = rowwise(kern, X, Y, a[c, :m * bd], got[c, :n * bd], y0[c, :n * bd], alpha, beta, np.arange(n), dt)
        assert worst <= 1.0, (c, row, e, worst)


def test_to_dense_matches_the_reference_matrix_and_is_symmetric(cg):
    rng = np.random.default_rng(60)
    n, d = 7, 3
    k, kern = make_kernel(cg, PROFILES[1], d)
    X = rng.standard_normal((n, d))
    G = cg.gramian(cg.HessianKernel(k), torch.from_numpy(X).cuda())
    M = G.to_dense().cpu().numpy()
    assert cg.get_info("last_hess_path") == 1
    ref = R.hess_matrix(kern, X, X)
    assert M.shape == ref.shape == (n * d * d, n * d * d)
    assert np.abs(M - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(M - M.T).max() <= 1e-12 * np.abs(ref).max()
    assert G.issymmetric()


def test_conjugate_gradients_on_the_shifted_operator(cg):
    """cg(G + sigma^2 I, b), n = 64, d = 4, fp64, with the solver as it is."""
    rng = np.random.default_rng(70)
    n, d = 64, 4
    k, kern = make_kernel(cg, PROFILES[0], d)
    X = rng.standard_normal((n, d))
    G = cg.gramian(cg.HessianKernel(k), torch.from_numpy(X).cuda())
    N = n * d * d
    A = G + 0.1 * torch.ones(N, dtype=torch.float64, device="cuda")
    b = torch.from_numpy(rng.standard_normal(N)).cuda()
    x, info = cg.cg(A, b, reltol=1e-9, maxiter=4 * N)
    assert info["converged"], info
    res = (G @ x + 0.1 * x - b).cpu().numpy()
    assert np.linalg.norm(res) <= 2e-9 * np.linalg.norm(b.cpu().numpy()), info


@pytest.mark.parametrize("n", [128, 2048])
def test_readme_shape_and_a_larger_one_on_a_row_subset(cg, n):
    """EQ, d = 16, fp64: n = 128 (the reference's README shape) and n = 2048, x = y, on first / last rows, the ragged tail, one full
    workgroup (256 / 16 = 16 points) and 32 random rows."""
    rng = np.random.default_rng(80 + n)
    run_case(cg, PROFILES[0], n, n, 16, F64, seed=80 + n, same=True, rows=row_subset(n, 16, rng))


@pytest.mark.parametrize("i,dt,d,n,m,jsplit", [(0, F64, 3, 37, 29, 3), (0, F32, 5, 19, 23, 2), (4, F32, 5, 19, 23, 2)])
def test_forced_column_split(cg, i, dt, d, n, m, jsplit):
    """Option jsplit: partial slabs and the fixed-order reduce meet the same bar on all rows.  Three slabs in fp64 at d = 3; two in fp32
    at d = 5, which is padded to 8: the padded lanes a >= d and the padding of the column records are live."""
    cg.set_option("jsplit", jsplit)
    try:
        run_case(cg, PROFILES[i], n, m, d, dt, seed=90 + d)
    finally:
        cg.set_option("jsplit", 0)


def abi_mvm(cg, n, m, d, a, y, alpha, beta):
    """covgram_hess_mvm through the C ABI on device pointers, fp64 EQ with a lengthscale, lda = max(1, m d^2), ldy = max(1, n d^2); the
    return code."""
    from covgram import _ffi
    from covgram.gramian import _Points
    rng = np.random.default_rng(7)
    k, kern = make_kernel(cg, PROFILES[0], d)
    px = _Points(torch.from_numpy(rng.standard_normal((n, d))).cuda())
    py = _Points(torch.from_numpy(rng.standard_normal((m, d))).cuda())
    bd = d * d
    rc = _ffi.lib().covgram_hess_mvm(px.ctx.bind_stream(), _ffi.kref(cg.require_hessian_spec(k, d)), px.handle, py.handle,
                                     C.c_void_p(a.data_ptr()), max(1, m * bd), C.c_void_p(y.data_ptr()), max(1, n * bd), 1, alpha, beta,
                                     _ffi.DEVICE)
    torch.cuda.synchronize()
    return rc


def test_no_columns_scales_y_and_no_rows_writes_nothing(cg):
    """m = 0: y <- beta y exactly (the reduce launch with no slabs), beta = 0 never reads y; n = 0: nothing is launched or written.
    Either way the call succeeds and last_hess_path is 0 afterwards."""
    from covgram import _ffi
    rng = np.random.default_rng(95)
    n, d = 5, 2
    bd = d * d
    a = torch.from_numpy(rng.standard_normal(4 * bd)).cuda()
    run_case(cg, PROFILES[0], 6, 6, d, F64, seed=96)                      # leaves last_hess_path at 1
    y0 = rng.standard_normal(n * bd)
    y = torch.from_numpy(y0.copy()).cuda()
    assert abi_mvm(cg, n, 0, d, a, y, 0.9, -0.4) == _ffi.OK
    assert cg.get_info("last_hess_path") == 0
    assert np.array_equal(y.cpu().numpy(), -0.4 * y0)
    y = torch.full((n * bd,), NANV, dtype=torch.float64, device="cuda")
    assert abi_mvm(cg, n, 0, d, a, y, 0.9, 0.0) == _ffi.OK
    assert cg.get_info("last_hess_path") == 0
    assert np.array_equal(y.cpu().numpy(), np.zeros(n * bd))
    run_case(cg, PROFILES[0], 6, 6, d, F64, seed=96)
    y = torch.from_numpy(y0.copy()).cuda()
    assert abi_mvm(cg, 0, 4, d, a, y, 0.9, -0.4) == _ffi.OK
    assert cg.get_info("last_hess_path") == 0
    assert np.array_equal(y.cpu().numpy(), y0)


def test_unsupported_kernels_and_dimensions_raise(cg):
    X = torch.randn(10, 3, dtype=torch.float64, device="cuda")
    a = torch.randn(90, dtype=torch.float64, device="cuda")
    for k in (cg.MaternP(2), cg.EQ() + cg.Cauchy(), cg.EQ() ** 2, cg.Exp(), cg.Matern(1.3), cg.AsinDot()):
        with pytest.raises(cg.UnsupportedKernel):
            cg.gramian(cg.HessianKernel(k), X) @ a
    X33 = torch.randn(4, 33, dtype=torch.float64, device="cuda")
    with pytest.raises(cg.UnsupportedKernel, match="33"):
        cg.gramian(cg.HessianKernel(cg.EQ()), X33) @ torch.randn(4 * 33 * 33, dtype=torch.float64, device="cuda")
    # the library makes the same checks behind the ABI
    from covgram import _ffi
    from covgram.gramian import _Points
    px = _Points(X)
    y = torch.empty(90, dtype=torch.float64, device="cuda")
    spec = cg.device_spec(cg.MaternP(2))
    rc = _ffi.lib().covgram_hess_mvm(px.ctx.bind_stream(), _ffi.kref(spec), px.handle, px.handle, C.c_void_p(a.data_ptr()), 90,
                                     C.c_void_p(y.data_ptr()), 90, 1, 1.0, 0.0, _ffi.DEVICE)
    assert rc == _ffi.EUNSUPPORTED and b"MaternP" in _ffi.lib().covgram_last_error()
    with pytest.raises(cg.DimensionMismatch):
        cg.gramian(cg.HessianKernel(cg.EQ()), X) @ torch.randn(91, dtype=torch.float64, device="cuda")
