"""GPU tier: the C ABI exactly as a `ccall` shim would use it — HOST pointers (numpy arrays), library-side staging — for
every entry point of include/covgram.h, plus the edge cases the reference's loops accept (empty inputs, many RHS)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def relerr(b, ref):
    b = np.asarray(b, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    den = np.linalg.norm(ref)
    return np.linalg.norm(b - ref) / (den if den > 0 else 1.0)


def P(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def ctx(cg):
    lib = cg._ffi.lib()
    h = cg._ffi._P()
    cg._ffi.check(lib.covgram_ctx_create(C.byref(h), 0, None))     # NULL stream = the default stream
    yield h
    assert lib.covgram_ctx_destroy(h) == 0


def make_points(cg, ctx, X):
    lib = cg._ffi.lib()
    h = cg._ffi._P()
    X = np.ascontiguousarray(X)
    cg._ffi.check(lib.covgram_points_create(ctx, C.byref(h), P(X), X.shape[0], X.shape[1],
                                            cg._ffi.F64 if X.dtype == np.float64 else cg._ffi.F32, cg._ffi.HOST))
    return h


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_host_pointer_mvm_matrix_gradient(cg, oracle, ctx, dt):
    lib, f = cg._ffi.lib(), cg._ffi
    tol = 1e-5 if dt == np.float32 else 1e-12
    rng = np.random.default_rng(3)
    n, m, d = 301, 123, 3
    X = rng.standard_normal((n, d)).astype(dt); Y = rng.standard_normal((m, d)).astype(dt)
    hx, hy = make_points(cg, ctx, X), make_points(cg, ctx, Y)
    nn, dd, tt = C.c_int64(), C.c_int32(), C.c_int32()
    assert lib.covgram_points_info(hx, C.byref(nn), C.byref(dd), C.byref(tt)) == 0 and (nn.value, dd.value) == (n, d)
    spec = cg.device_spec(cg.Lengthscale(cg.MaternP(2), 0.8) * 1.7)
    ko = oracle.Kernel(oracle.MATERNP, p=2, lengthscale=0.8, scale=1.7)
    # vector, 7-column and (fp32: fp32 matrix cores, dense_mfma_mrhs_kernel) 13- / 40- / 70-column right-hand sides, leading dimensions
    # larger than the extents
    for nrhs in (1, 7, 13, 40, 70):
        lda, ldy = m + 5, n + 3
        A = np.zeros((nrhs, lda), dtype=dt); A[:, :m] = rng.standard_normal((nrhs, m))          # column-major m x nrhs, lda
        Yo = np.zeros((nrhs, ldy), dtype=dt); Yo[:, :n] = rng.standard_normal((nrhs, n))
        Y0 = Yo.copy()
        f.check(lib.covgram_mvm(ctx, C.byref(spec), hx, hy, P(A), lda, P(Yo), ldy, nrhs, -0.7, 1.3, f.HOST))
        ref = oracle.mul(Y0[:, :n].T, ko, X, Y, A[:, :m].T, -0.7, 1.3, dt)
        assert relerr(Yo[:, :n].T, ref) <= tol
        assert np.array_equal(Yo[:, n:], Y0[:, n:])                                              # padding rows untouched
    # Matrix(G)
    M = np.zeros((m, n + 2), dtype=dt)
    f.check(lib.covgram_matrix(ctx, C.byref(spec), hx, hy, P(M), n + 2, f.HOST))
    assert relerr(M[:, :n].T, oracle.matrix(ko, X, Y, dt)) <= tol
    # row-shard slice == the corresponding rows
    hs = f._P()
    f.check(lib.covgram_points_slice(hx, 100, 50, C.byref(hs)))
    a = rng.standard_normal(m).astype(dt); ys = np.zeros(50, dtype=dt)
    f.check(lib.covgram_mvm(ctx, C.byref(spec), hs, hy, P(a), m, P(ys), 50, 1, 1.0, 0.0, f.HOST))
    assert relerr(ys, oracle.mul(None, ko, X[100:150], Y, a, dtype=dt)) <= tol
    assert lib.covgram_points_slice(hx, 290, 50, C.byref(f._P())) == f.EINVAL
    # gradient MVM through host pointers
    ag = rng.standard_normal(m * d).astype(dt); yg = rng.standard_normal(n * d).astype(dt); yg0 = yg.copy()
    f.check(lib.covgram_grad_mvm(ctx, C.byref(spec), hx, hy, P(ag), ag.size, P(yg), yg.size, 1, 0.4, -0.9, f.HOST))
    assert relerr(yg, oracle.grad_mul(yg0, ko, X, Y, ag, 0.4, -0.9, dt)) <= (1e-5 if dt == np.float32 else 1e-12)
    # value-gradient blocks and a composite kernel through host pointers (the composite goes in through its head)
    av = rng.standard_normal(m * (d + 1)).astype(dt); yv = rng.standard_normal(n * (d + 1)).astype(dt); yv0 = yv.copy()
    f.check(lib.covgram_valgrad_mvm(ctx, C.byref(spec), hx, hy, P(av), av.size, P(yv), yv.size, 1, 0.4, -0.9, f.HOST))
    assert relerr(yv, oracle.valgrad_mul(yv0, ko, X, Y, av, 0.4, -0.9, dt)) <= (1e-5 if dt == np.float32 else 1e-12)
    comp = cg.device_spec(1.5 * cg.Lengthscale(cg.MaternP(2), 0.8) + 0.5 * cg.EQ())
    kc = oracle.Composite(((oracle.Kernel(oracle.MATERNP, p=2, lengthscale=0.8, scale=1.5),), (oracle.Kernel(oracle.EQ, scale=0.5),)))
    yc = np.zeros(n, dtype=dt)
    f.check(lib.covgram_mvm(ctx, f.kref(comp), hx, hy, P(a), m, P(yc), n, 1, 1.0, 0.0, f.HOST))
    assert relerr(yc, oracle.mul(None, kc, X, Y, a, dtype=dt)) <= tol
    f.check(lib.covgram_grad_mvm(ctx, f.kref(comp), hx, hy, P(ag), ag.size, P(yg), yg.size, 1, 1.0, 0.0, f.HOST))
    assert relerr(yg, oracle.grad_mul(None, kc, X, Y, ag, dtype=dt)) <= (1e-5 if dt == np.float32 else 1e-12)
    Mc = np.zeros((m, n), dtype=dt)
    f.check(lib.covgram_matrix(ctx, f.kref(comp), hx, hy, P(Mc), n, f.HOST))
    assert relerr(Mc.T, oracle.matrix(kc, X, Y, dt)) <= tol
    bad = cg.device_spec(cg.EQ() + cg.RQ(1.0)); bad.factors[1].trait = f.DOTPRODUCT
    assert lib.covgram_mvm(ctx, f.kref(bad), hx, hy, P(a), m, P(yc), n, 1, 1.0, 0.0, f.HOST) == f.EINVAL
    v = C.c_int64(-1)
    assert lib.covgram_ctx_get_info(ctx, b"last_dense_path", C.byref(v)) == 0 and v.value in (1, 2)
    assert lib.covgram_ctx_get_info(ctx, b"num_cus", C.byref(v)) == 0 and v.value >= 64
    assert lib.covgram_ctx_get_info(ctx, b"nonsense", C.byref(v)) == f.EINVAL
    # dimension mismatch -> status, not a crash
    hz = make_points(cg, ctx, rng.standard_normal((5, 2)).astype(dt))
    assert lib.covgram_mvm(ctx, C.byref(spec), hx, hz, P(a), m, P(ys), n, 1, 1.0, 0.0, f.HOST) == f.EINVAL
    assert b"same length" in lib.covgram_last_error()
    for h in (hs, hx, hy, hz):
        assert lib.covgram_points_destroy(h) == 0


def test_host_pointer_toeplitz_kron_lowrank(cg, oracle, ctx):
    lib, f = cg._ffi.lib(), cg._ffi
    rng = np.random.default_rng(4)
    # Toeplitz, non-symmetric, both the rocFFT path (small) and the four-step path (N >= 16384)
    for n, m in ((300, 200), (9000, 9000)):
        vc = rng.standard_normal(n); vr = rng.standard_normal(m); vr[0] = vc[0]
        a = rng.standard_normal(m); y = rng.standard_normal(n); y0 = y.copy()
        h = f._P()
        f.check(lib.covgram_toeplitz_create(ctx, C.byref(h), P(vc), P(vr), n, m, f.F64, f.HOST, 0))
        f.check(lib.covgram_toeplitz_mvm(h, P(a), P(y), 0.5, 2.0, f.HOST))
        assert relerr(y, oracle.toeplitz_mul(y0, vc, vr, a, 0.5, 2.0)) <= 1e-10
        assert lib.covgram_toeplitz_destroy(h) == 0
    # circulant of odd length
    vc = rng.standard_normal(33); a = rng.standard_normal(33); y = np.zeros(33)
    h = f._P()
    f.check(lib.covgram_toeplitz_create(ctx, C.byref(h), P(vc), None, 33, 33, f.F64, f.HOST, 1))
    f.check(lib.covgram_toeplitz_mvm(h, P(a), P(y), 1.0, 0.0, f.HOST))
    assert relerr(y, oracle.toeplitz_dense(vc, circulant=True) @ a) <= 1e-12
    assert lib.covgram_toeplitz_destroy(h) == 0
    # Kronecker with host factors (column-major with padding in the leading dimension)
    shapes = [(3, 5), (4, 2), (2, 6)]
    Fs = [rng.standard_normal(s) for s in shapes]
    lds = [s[0] + 1 for s in shapes]
    bufs = []
    for Fm, ld in zip(Fs, lds):
        b = np.zeros((Fm.shape[1], ld)); b[:, :Fm.shape[0]] = Fm.T
        bufs.append(b)
    ptrs = (f._P * 3)(*[P(b) for b in bufs])
    rows = (C.c_int64 * 3)(*[s[0] for s in shapes]); cols = (C.c_int64 * 3)(*[s[1] for s in shapes]); ldarr = (C.c_int64 * 3)(*lds)
    av = rng.standard_normal(5 * 2 * 6); yv = rng.standard_normal(3 * 4 * 2); yv0 = yv.copy()
    f.check(lib.covgram_kron_mvm(ctx, ptrs, rows, cols, ldarr, 3, f.F64, P(av), av.size, P(yv), yv.size, 1, 1.5, -0.5, f.HOST))
    assert relerr(yv, 1.5 * np.kron(np.kron(Fs[0], Fs[1]), Fs[2]) @ av - 0.5 * yv0) <= 1e-12
    # low rank
    n, m, r = 500, 300, 5
    U = rng.standard_normal((n, r)); V = rng.standard_normal((m, r))
    Uc = np.asfortranarray(U); Vc = np.asfortranarray(V)
    a = rng.standard_normal(m); y = rng.standard_normal(n); y0 = y.copy()
    f.check(lib.covgram_lowrank_mvm(ctx, P(Uc), n, P(Vc), m, n, m, r, f.F64, P(a), m, P(y), n, 1, 2.0, 0.25, f.HOST))
    assert relerr(y, oracle.lowrank_mul(y0, U, V, a, 2.0, 0.25)) <= 1e-12


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_host_pointer_direct_toeplitz_solvers(cg, oracle, ctx, dt):
    """covgram_toeplitz_durbin / _levinson / _trench with HOST pointers — the form julia/CovGram.jl's `\\`, durbin!, levinson!, trench!
    (src/toeplitz.jl:12-111) use — on the on-chip kernel (n <= 16384), on the global-memory kernel above it, at n = 1, and above the
    size cap (COVGRAM_EUNSUPPORTED, nothing launched)."""
    lib, f = cg._ffi.lib(), cg._ffi
    code = f.F64 if dt == np.float64 else f.F32
    tol = 1e-9 if dt == np.float64 else 2e-3
    rng = np.random.default_rng(77)
    for m in (1, 2, 300, 16384, 16500):
        vc = (1.5 * (np.arange(m) == 0) + np.exp(-np.abs(np.linspace(0.0, 3.0, m)))).astype(np.float64)   # diagonal 2.5: well conditioned
        r = (vc[1:] / vc[0]).astype(dt)
        b = rng.standard_normal(m).astype(dt)
        x = np.full(m, np.nan, dtype=dt)
        f.check(lib.covgram_toeplitz_levinson(ctx, P(r) if m > 1 else None, P(b), m, P(x), code, f.HOST))
        r64, b64 = r.astype(np.float64), b.astype(np.float64)
        if m <= 300:
            K = np.array([[1.0 if i == j else r64[abs(i - j) - 1] for j in range(m)] for i in range(m)])
            assert relerr(x, np.linalg.solve(K, b64)) <= tol, ("levinson", m)
        else:                                                       # residual through the FFT MVM of the same matrix
            T = cg.SymmetricToeplitz(torch.from_numpy(np.concatenate([[1.0], r64])).cuda())
            assert relerr((T @ torch.from_numpy(x.astype(np.float64)).cuda()).cpu().numpy(), b64) <= tol, ("levinson", m)
        if m > 1:
            y = np.full(m - 1, np.nan, dtype=dt)
            f.check(lib.covgram_toeplitz_durbin(ctx, P(r), m - 1, P(y), code, f.HOST))
            assert relerr(y, oracle.durbin(r64)) <= tol, ("durbin", m)
        if m <= 300:
            B = np.full((m, m + 1), np.nan, dtype=dt)               # column-major with ldb = m + 1: as a (m, m + 1) C array of columns
            Bc = np.zeros((m, m + 1), dtype=dt)
            f.check(lib.covgram_toeplitz_trench(ctx, P(r) if m > 1 else None, m, P(Bc), m + 1, code, f.HOST))
            Binv = Bc[:, :m].T                                       # entry (i, j) at i + j * ldb
            assert relerr(Binv @ K, np.eye(m)) <= tol * 10, ("trench", m)
    big = int(lib.covgram_version() and 65536) + 1
    z = np.zeros(8, dtype=np.float64)
    assert lib.covgram_toeplitz_levinson(ctx, P(z), P(z), big, P(z), f.F64, f.HOST) == f.EUNSUPPORTED
    assert lib.covgram_toeplitz_durbin(ctx, P(z), big, P(z), f.F64, f.HOST) == f.EUNSUPPORTED
    assert lib.covgram_toeplitz_levinson(ctx, P(z), P(z), 0, P(z), f.F64, f.HOST) == f.EINVAL


def test_empty_and_degenerate_inputs(cg, oracle):
    """Edge cases the reference's loops accept: no columns (y <- beta y), no rows, one point, many RHS, d at the boundaries."""
    dev = "cuda"
    x = torch.randn(17, 3, device=dev, dtype=torch.float64)
    empty = torch.zeros(0, 3, device=dev, dtype=torch.float64)
    G = cg.gramian(cg.EQ(), x, empty)                       # 17 x 0
    y = torch.randn(17, device=dev, dtype=torch.float64); y0 = y.clone()
    cg.mul_(y, G, torch.zeros(0, device=dev, dtype=torch.float64), 1.0, 0.5)
    assert torch.allclose(y, 0.5 * y0)
    yn = torch.full((17,), float("nan"), device=dev, dtype=torch.float64)
    cg.mul_(yn, G, torch.zeros(0, device=dev, dtype=torch.float64), 1.0, 0.0)
    assert torch.all(yn == 0)                               # beta == 0: zero-filled, NaN ignored (gramian.jl:80)
    G0 = cg.gramian(cg.EQ(), empty, x)                      # 0 x 17
    assert (G0 @ torch.randn(17, device=dev, dtype=torch.float64)).shape == (0,)
    Kg = cg.gramian(cg.GradientKernel(cg.EQ()), x, empty)
    yg = torch.randn(51, device=dev, dtype=torch.float64); yg0 = yg.clone()
    cg.mul_(yg, Kg, torch.zeros(0, device=dev, dtype=torch.float64), 1.0, -2.0)
    assert torch.allclose(yg, -2.0 * yg0)
    # d exactly at the lane-owned limits and one past them (dense 64/65; gradient fp64 48/49)
    rng = np.random.default_rng(12)
    for d in (64, 65):
        X = rng.standard_normal((130, d)) / np.sqrt(d); a = rng.standard_normal(130)
        Gd = cg.gramian(cg.EQ(), torch.from_numpy(X).cuda())
        assert relerr((Gd @ torch.from_numpy(a).cuda()).cpu().numpy(), oracle.mul(None, oracle.Kernel(oracle.EQ), X, X, a)) <= 1e-12
    for d in (48, 49):
        X = rng.standard_normal((40, d)) / np.sqrt(d); a = rng.standard_normal(40 * d)
        Kd = cg.gramian(cg.GradientKernel(cg.RQ(1.0)), torch.from_numpy(X).cuda())
        assert relerr((Kd @ torch.from_numpy(a).cuda()).cpu().numpy(), oracle.grad_mul(None, oracle.Kernel(oracle.RQ, param=1.0), X, X, a)) <= 1e-12
    # 9 right-hand sides (three kernel passes of <= 4 columns), non-contiguous inputs
    X = rng.standard_normal((200, 2)); A = rng.standard_normal((200, 9))
    Gm = cg.gramian(cg.Cauchy(), torch.from_numpy(X).cuda())
    At = torch.from_numpy(np.asfortranarray(A)).cuda()      # non-C-contiguous tensor
    assert relerr((Gm @ At).cpu().numpy(), oracle.mul(None, oracle.Kernel(oracle.CAUCHY), X, X, A)) <= 1e-12
    one = torch.randn(1, 3, device=dev, dtype=torch.float32)
    assert abs(float((cg.gramian(cg.EQ(), one) @ torch.ones(1, device=dev))[0]) - 1.0) < 1e-6


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_cg_step_is_the_cg_recurrence(cg, ctx, dt):
    """covgram_cg_step against the recurrences of IterativeSolvers.cg! written out in numpy (src/gramian.jl:229-238 calls it):
    alpha = rho / (p . Ap); x += alpha p; r -= alpha Ap; rho' = r . r; p = r + (rho' / rho) p — two consecutive steps (the
    second divides by the rho the first committed), ragged n, and n = 0."""
    lib, f = cg._ffi.lib(), cg._ffi
    DP = lambda t: f._P(t.data_ptr())                      # device pointers (this entry point takes no host memory)
    tdt = torch.float32 if dt == np.float32 else torch.float64
    tol = 2e-6 if dt == np.float32 else 1e-14
    rng = np.random.default_rng(17)
    for n in (1, 777, 70001):
        x, r, p = (rng.standard_normal(n).astype(dt) for _ in range(3))
        xd, rd, pd = (torch.from_numpy(v.copy()).cuda() for v in (x, r, p))
        scal = torch.zeros(2 + 512, dtype=tdt, device="cuda")
        scal[1] = torch.dot(rd, rd)
        x64, r64, p64 = (v.astype(np.float64) for v in (x, r, p))
        rho = float(r64 @ r64)
        for step in range(2):
            Ap = rng.standard_normal(n).astype(dt)
            Apd = torch.from_numpy(Ap).cuda()
            torch.cuda.synchronize()
            f.check(lib.covgram_cg_step(ctx, n, f.F32 if dt == np.float32 else f.F64, DP(xd), DP(rd), DP(pd), DP(Apd), DP(scal)))
            torch.cuda.synchronize()
            Ap64 = Ap.astype(np.float64)
            alpha = rho / float(p64 @ Ap64)
            x64 = x64 + alpha * p64; r64 = r64 - alpha * Ap64
            rho_new = float(r64 @ r64)
            p64 = r64 + (rho_new / rho) * p64
            assert abs(float(scal[0]) - rho) <= tol * abs(rho) * 10 and abs(float(scal[1]) - rho_new) <= tol * abs(rho_new) * 10
            rho = rho_new
            for got, want in ((xd, x64), (rd, r64), (pd, p64)):
                assert relerr(got.cpu().numpy(), want) <= tol * 50, (n, step, relerr(got.cpu().numpy(), want))
    f.check(lib.covgram_cg_step(ctx, 0, f.F64, None, None, None, None, None))
    assert lib.covgram_cg_step(ctx, 5, 7, None, None, None, None, None) == f.EINVAL


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_cg_step_shifted_adds_the_diagonal_term_and_leaves_the_norm(cg, ctx, dt):
    """covgram_cg_step_shifted: the step for A = G + Diagonal(d) (src/gramian.jl:55-60; mul! of the lazy sum,
    src/lazy_linear_algebra.jl:126-133) given Ap = G p of the Gramian alone — Ap comes back completed (Ap + d .* p), the
    recurrences use it, and |r| sits in scal[2 + 512]; diag = NULL is the plain step plus the norm."""
    lib, f = cg._ffi.lib(), cg._ffi
    DP = lambda t: f._P(t.data_ptr())
    tdt = torch.float32 if dt == np.float32 else torch.float64
    tol = 2e-6 if dt == np.float32 else 1e-14
    rng = np.random.default_rng(23)
    for n in (1, 1000, 70001):
        for with_diag in (True, False):
            x, r, p, d = (rng.standard_normal(n).astype(dt) for _ in range(4))
            d = np.abs(d) + dt(0.1)
            xd, rd, pd, dd = (torch.from_numpy(v.copy()).cuda() for v in (x, r, p, d))
            scal = torch.zeros(2 + 512 + 1, dtype=tdt, device="cuda")
            scal[1] = torch.dot(rd, rd)
            x64, r64, p64, d64 = (v.astype(np.float64) for v in (x, r, p, d))
            rho = float(r64 @ r64)
            for step in range(2):
                Gp = rng.standard_normal(n).astype(dt)
                Apd = torch.from_numpy(Gp.copy()).cuda()
                f.check(lib.covgram_cg_step_shifted(ctx, n, f.F32 if dt == np.float32 else f.F64, DP(xd), DP(rd), DP(pd), DP(Apd), DP(scal),
                                                    DP(dd) if with_diag else None))
                torch.cuda.synchronize()
                Ap64 = Gp.astype(np.float64) + (d64 * p64 if with_diag else 0.0)
                assert relerr(Apd.cpu().numpy(), Ap64) <= tol * 10
                alpha = rho / float(p64 @ Ap64)
                x64 = x64 + alpha * p64; r64 = r64 - alpha * Ap64
                rho_new = float(r64 @ r64)
                p64 = r64 + (rho_new / rho) * p64
                assert abs(float(scal[1]) - rho_new) <= tol * abs(rho_new) * 50
                assert abs(float(scal[2 + 512]) - np.sqrt(rho_new)) <= tol * np.sqrt(rho_new) * 50
                rho = rho_new
                for got, want in ((xd, x64), (rd, r64), (pd, p64)):
                    assert relerr(got.cpu().numpy(), want) <= tol * 200, (n, step, relerr(got.cpu().numpy(), want))
    f.check(lib.covgram_cg_step_shifted(ctx, 0, f.F64, None, None, None, None, None, None))


# ------------------------------------------------------------------------------------------------------------------------------------
# The entry points whose a / y (or output tile) go through the shared staging helpers of csrc/driver.hpp (StagedVectors, StagedTile):
# HOST pointers must give the bits DEVICE pointers give, and the timer bracket (TimerScope) must count what it always counted.
# ------------------------------------------------------------------------------------------------------------------------------------
_SN, _SM, _SD, _SNRHS = 130, 67, 3, 3
_BLOCK_KINDS = ("gradient", "value_gradient", "hessian", "value_gradient_hessian")


def _staged_entry_points(cg, ctx, dt):
    """{name: (square_ok, run)}; run(loc, inplace) -> (result, prefill, rows): the whole column-major buffer after the call (leading dimension
    included), what it held before, and the rows the call may write.  Seeded inputs: every run of one name sees the same numbers.
    A single-profile kernel (EQ, l = 0.9, scale 1.7; sparse: l = 0.3), nrhs = 3, lda = rows + 5, ldy = rows + 3, alpha = -0.7, beta = 1.3 on a
    prefilled y; inplace (square products only, X on both sides): y is a."""
    lib, f = cg._ffi.lib(), cg._ffi
    code = f.F64 if dt == np.float64 else f.F32
    rng = np.random.default_rng(20)
    X = rng.standard_normal((_SN, _SD)).astype(dt); Y = rng.standard_normal((_SM, _SD)).astype(dt)
    hx, hy = make_points(cg, ctx, X), make_points(cg, ctx, Y)
    spec = cg.device_spec(cg.Lengthscale(cg.EQ(), 0.9) * 1.7)
    kp = f.kref(spec)
    keep = [X, Y, spec]                                           # what the handles and pointers below refer to

    def buffers(loc, arrays):
        """the arrays as the call's pointers: numpy memory (HOST) or device copies (DEVICE), and a function that reads them back"""
        if loc == f.HOST:
            return [P(a) for a in arrays], lambda i: arrays[i]
        dev = [torch.from_numpy(a).cuda() for a in arrays]
        torch.cuda.synchronize()
        def back(i):
            f.check(lib.covgram_sync(ctx))
            return dev[i].cpu().numpy()
        return [f._P(t.data_ptr()) for t in dev], back

    def mvm_like(call, bd_of, seed):
        def run(loc, inplace):
            r = np.random.default_rng(seed)
            hcol = hx if inplace else hy
            rows_a, rows_y = (_SN if inplace else _SM) * bd_of, _SN * bd_of
            lda, ldy = (rows_y + 3, rows_y + 3) if inplace else (rows_a + 5, rows_y + 3)
            A = r.standard_normal((_SNRHS, lda)).astype(dt); Yv = r.standard_normal((_SNRHS, ldy)).astype(dt)
            Y0 = Yv.copy()
            if inplace:
                (p,), back = buffers(loc, [Yv])
                f.check(call(hcol, p, lda, p, ldy, loc))
                return back(0), Y0, rows_y
            (pa, py), back = buffers(loc, [A, Yv])
            f.check(call(hcol, pa, lda, py, ldy, loc))
            return back(1), Y0, rows_y
        return run

    def tile_like(call, rows, cols, seed, inputs=(), pad=3):
        """call(po, ldo, loc, *inputs as pointers of loc): a rows x cols output in a prefilled column-major buffer of leading dimension rows + pad"""
        def run(loc, inplace):
            ldo = rows + pad
            O = np.random.default_rng(seed).standard_normal((cols, ldo)).astype(dt)
            O0 = O.copy()
            (po, *pin), back = buffers(loc, [O] + list(inputs))
            f.check(call(po, ldo, loc, *pin))
            return back(0), O0, rows
        return run

    def op_like(call, rows_a, rows_y, seed, nrhs=1, pad=(5, 3), operands=lambda r: ()):
        """A structured operator, y <- alpha G a + beta y: call(pa, lda, py, ldy, loc, *operands as pointers of loc).  a and y are padded (lda = rows_a +
        pad[0], ldy = rows_y + pad[1]); operands(rng) are the operator's own arrays (first column, factors, U and V, a diagonal), packed: HOST packs
        them anyway, so both calls hand the kernels the same leading dimensions.  inplace (rows_a == rows_y): y is a."""
        def run(loc, inplace):
            r = np.random.default_rng(seed)
            ops = [np.ascontiguousarray(o, dtype=dt) for o in operands(r)]
            lda, ldy = rows_a + pad[0], rows_y + pad[1]
            if inplace:
                lda = ldy
            A = r.standard_normal((nrhs, lda)).astype(dt); Yv = r.standard_normal((nrhs, ldy)).astype(dt)
            Y0 = Yv.copy()
            own = [Yv] if inplace else [A, Yv]
            ptrs, back = buffers(loc, own + ops)
            f.check(call(ptrs[0], lda, ptrs[len(own) - 1], ldy, loc, *ptrs[len(own):]))
            return back(len(own) - 1), Y0, rows_y
        return run

    d = _SD
    eps = {}
    for name, fn, bd in (("covgram_mvm", lib.covgram_mvm, 1), ("covgram_grad_mvm", lib.covgram_grad_mvm, d), ("covgram_valgrad_mvm", lib.covgram_valgrad_mvm, d + 1),
                         ("covgram_hess_mvm", lib.covgram_hess_mvm, d * d), ("covgram_valgradhess_mvm", lib.covgram_valgradhess_mvm, 1 + d + d * d)):
        eps[name] = (True, mvm_like(lambda hc, pa, lda, py, ldy, loc, fn=fn: fn(ctx, kp, hx, hc, pa, lda, py, ldy, _SNRHS, -0.7, 1.3, loc), bd, 31))
    as_d = lambda v: np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    w, mu, il = np.array([0.7, 1.1]), rng.standard_normal((2, d)) * 0.3, 1.0 / (0.6 + rng.random((2, d)))
    hsm = f._P()
    f.check(lib.covgram_sm_create(ctx, C.byref(hsm), 2, d, as_d(w), as_d(mu), as_d(il), code))
    eps["covgram_sm_mvm"] = (True, mvm_like(lambda hc, pa, lda, py, ldy, loc: lib.covgram_sm_mvm(hsm, hx, hc, pa, lda, py, ldy, _SNRHS, -0.7, 1.3, loc), 1, 32))
    sparse_spec = cg.device_spec(cg.Lengthscale(cg.EQ(), 0.3))
    keep.append(sparse_spec)
    hsp = {}
    for square, hc in ((False, hy), (True, hx)):
        hsp[square] = f._P()
        f.check(lib.covgram_sparse_create(ctx, C.byref(hsp[square]), f.kref(sparse_spec), hx, hc, 1e-6))
    eps["covgram_sparse_mvm"] = (True, mvm_like(lambda hc, pa, lda, py, ldy, loc: lib.covgram_sparse_mvm(hsp[hc is hx], pa, lda, py, ldy, _SNRHS, -0.7, 1.3, loc), 1, 33))
    eps["covgram_matrix"] = (False, tile_like(lambda po, ldo, loc: lib.covgram_matrix(ctx, kp, hx, hy, po, ldo, loc), _SN, _SM, 34))
    for kind, B in zip(range(4), (d, d + 1, d * d, 1 + d + d * d)):
        eps["covgram_block_matrix:" + _BLOCK_KINDS[kind]] = (False, tile_like(
            lambda po, ldo, loc, kind=kind: lib.covgram_block_matrix(ctx, kind, kp, hx, hy, po, ldo, loc), _SN * B, _SM * B, 35))
    eps["covgram_sm_matrix"] = (False, tile_like(lambda po, ldo, loc: lib.covgram_sm_matrix(hsm, hx, hy, po, ldo, loc), _SN, _SM, 36))

    # ---- the structured operators: the smallest shapes that reach every branch of their drivers ----
    # Toeplitz (n, m, symmetric, circulant, beta): rocFFT path; four-step path without a fused row kernel (N = 2^15, M' = 16); fused radix-4 row
    # kernel (N = 2^17, M' = 64); radix-16 row kernel (N = 2^22, M' = 4096: fp64 runs its persistent grid, fp32 one pair per workgroup) with a real
    # and a complex spectrum; circulant.  A case has one handle per loc, created from pointers of that loc by the first run that needs it; they live
    # until close(), so that rocFFT is set up once (covgram_toeplitz_destroy of the last live handle tears it down: half a second per cycle).
    htz = []
    def toeplitz(n, m, sym, circ, beta):
        handles = {}
        def call(pa, lda, py, ldy, loc, pvc, pvr=None):
            if loc not in handles:
                handles[loc] = f._P()
                f.check(lib.covgram_toeplitz_create(ctx, C.byref(handles[loc]), pvc, pvr, n, m, code, loc, int(circ)))
                htz.append(handles[loc])
            return lib.covgram_toeplitz_mvm(handles[loc], pa, py, -0.7, beta, loc)
        def operands(r):
            vc, vr = r.standard_normal(n), r.standard_normal(m)
            vr[0] = vc[0]
            return (vc,) if sym or circ else (vc, vr)
        return (n == m, op_like(call, m, n, 41, pad=(0, 0), operands=operands))
    for tag, n, m, sym, circ, beta in (("rocfft", 300, 200, False, False, 1.3), ("fourstep", 9000, 9000, False, False, 0.0),
                                       ("row4", 33000, 33000, False, False, 1.3), ("row16:symmetric", 1 << 21, 1 << 21, True, False, 1.3),
                                       ("row16", 1 << 21, 1 << 21, False, False, 0.0), ("circulant", 33, 33, False, True, 1.3)):
        eps["covgram_toeplitz_mvm:" + tag] = toeplitz(n, m, sym, circ, beta)

    # Kronecker: three small factors at nrhs = 1 and at nrhs = 3 with padded a and y (packed on the device), and a factor with a side of 1024
    def kron(shapes, nrhs, pad):
        q = len(shapes)
        rows = (C.c_int64 * q)(*[sh[0] for sh in shapes]); cols = (C.c_int64 * q)(*[sh[1] for sh in shapes])
        nin, nout = int(np.prod([sh[1] for sh in shapes])), int(np.prod([sh[0] for sh in shapes]))
        def call(pa, lda, py, ldy, loc, *pf):
            return lib.covgram_kron_mvm(ctx, (f._P * q)(*pf), rows, cols, rows, q, code, pa, lda, py, ldy, nrhs, -0.7, 1.3, loc)
        return (False, op_like(call, nin, nout, 42, nrhs=nrhs, pad=pad, operands=lambda r: [r.standard_normal((sh[1], sh[0])) for sh in shapes]))
    eps["covgram_kron_mvm:small"] = kron([(3, 5), (4, 2), (2, 6)], 1, (0, 0))
    eps["covgram_kron_mvm:small:nrhs3"] = kron([(3, 5), (4, 2), (2, 6)], 3, (5, 3))
    eps["covgram_kron_mvm:side1024"] = kron([(1024, 8), (8, 8)], 1, (0, 0))

    # low rank U V' (n = m = 300): the ticketed z sum (r <= 128), the separate z-sum kernel, the matrix-core form (nrhs >= 8; lda a multiple of the
    # vector width in both calls: one kernel instance)
    def lowrank(r_, nrhs, pad):
        n = m = 300
        def call(pa, lda, py, ldy, loc, pu, pv):
            return lib.covgram_lowrank_mvm(ctx, pu, n, pv, m, n, m, r_, code, pa, lda, py, ldy, nrhs, -0.7, 1.3, loc)
        return (True, op_like(call, m, n, 43, nrhs=nrhs, pad=pad, operands=lambda r: (r.standard_normal((r_, n)), r.standard_normal((r_, m)))))
    for r_, nrhs, ldt, pad in ((5, 1, np.float64, (5, 3)), (300, 1, np.float64, (5, 3)), (16, 8, np.float32, (8, 3))):
        if dt == ldt:
            eps["covgram_lowrank_mvm:r%d:nrhs%d" % (r_, nrhs)] = lowrank(r_, nrhs, pad)

    # Barnes-Hut: fp64 on gramian(k, x), n = 300 (leafsize 16: several levels), without a diagonal and with one of length 1 and n; fp32 rectangular,
    # d = 2; no rows at all.  Both products, each in both of its forms.
    hbh = []
    def barneshut(hr, hc, n, m, diag_len):
        h = f._P()
        f.check(lib.covgram_bh_create(ctx, C.byref(h), kp, hr, hc, 0.5, 16))
        hbh.append(h)
        def entry(fn, flag):
            def call(pa, lda, py, ldy, loc, pd=None):
                return fn(h, pa, py, -0.7, 1.3, -1.0, flag, pd, diag_len, loc)
            return (n == m, op_like(call, m, n, 44, pad=(0, 0), operands=lambda r: (0.5 + r.random(diag_len),) if diag_len else ()))
        return {"%s:%s%d" % (name, what, flag): entry(fn, flag) for name, fn, what in (
            ("covgram_bh_mvm", lib.covgram_bh_mvm, "split"), ("covgram_bh_taylor_mvm", lib.covgram_bh_taylor_mvm, "use_com")) for flag in (0, 1)}
    bh_cases = []
    if dt == np.float64:
        X3 = rng.standard_normal((300, _SD)).astype(dt)
        h3 = make_points(cg, ctx, X3)
        keep.append(X3); hbh_points = [h3]
        bh_cases += [(":diag%d" % dl, h3, h3, 300, 300, dl) for dl in (0, 1, 300)]
    else:
        X2 = rng.standard_normal((_SN, 2)).astype(dt); Y2 = rng.standard_normal((_SM, 2)).astype(dt)
        hx2, hy2 = make_points(cg, ctx, X2), make_points(cg, ctx, Y2)
        keep += [X2, Y2]; hbh_points = [hx2, hy2]
        bh_cases.append((":d2", hx2, hy2, _SN, _SM, 0))
    h0 = make_points(cg, ctx, np.zeros((0, _SD), dtype=dt))
    hbh_points.append(h0)
    bh_cases.append((":norows", h0, hy, 0, _SM, 0))
    for tag, hr, hc, n, m, dl in bh_cases:
        eps.update({name + tag: e for name, e in barneshut(hr, hc, n, m, dl).items()})

    # the direct Toeplitz solvers at n = 1, 2 and 300 (sizes 16384 and 16500: test_host_pointer_direct_toeplitz_solvers): vectors are tiles of
    # one column without padding, Trench's matrix has ldb = n + 3
    for n in (1, 2, 300):
        vc = 1.5 * (np.arange(n + 1) == 0) + np.exp(-np.abs(np.linspace(0.0, 3.0, n + 1)))     # diagonal 2.5: well conditioned
        r1 = (vc[1:] / vc[0]).astype(dt)                                                        # n entries; Levinson and Trench read n - 1
        b1 = np.random.default_rng(45).standard_normal(n).astype(dt)
        eps["covgram_toeplitz_levinson:n%d" % n] = (False, tile_like(
            lambda po, ldo, loc, pb, pr=None, n=n: lib.covgram_toeplitz_levinson(ctx, pr, pb, n, po, code, loc), n, 1, 46, inputs=[b1, r1][:2 if n > 1 else 1], pad=0))
        eps["covgram_toeplitz_durbin:n%d" % n] = (False, tile_like(
            lambda po, ldo, loc, pr, n=n: lib.covgram_toeplitz_durbin(ctx, pr, n, po, code, loc), n, 1, 47, inputs=[r1], pad=0))
        eps["covgram_toeplitz_trench:n%d" % n] = (False, tile_like(
            lambda po, ldo, loc, pr=None, n=n: lib.covgram_toeplitz_trench(ctx, pr, n, po, ldo, code, loc), n, n, 48, inputs=[r1][:1 if n > 1 else 0]))

    def close():
        for h in htz:
            assert lib.covgram_toeplitz_destroy(h) == 0
        for h in hbh:
            assert lib.covgram_bh_destroy(h) == 0
        for h in hbh_points:
            assert lib.covgram_points_destroy(h) == 0
        assert lib.covgram_sm_destroy(hsm) == 0
        for h in hsp.values():
            assert lib.covgram_sparse_destroy(h) == 0
        for h in (hx, hy):
            assert lib.covgram_points_destroy(h) == 0
        keep.clear()
    return eps, close


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_host_pointers_give_the_bits_of_device_pointers(cg, ctx, dt):
    """covgram_mvm, _grad_mvm, _valgrad_mvm, _hess_mvm, _valgradhess_mvm, _sm_mvm, _sparse_mvm (y <- alpha G a + beta y, and in place: y is a)
    and covgram_matrix, _block_matrix (four kinds), _sm_matrix at n = 130, m = 67, d = 3, and the structured operators at the shapes listed in
    _staged_entry_points (covgram_toeplitz_mvm, _kron_mvm, _lowrank_mvm, _bh_mvm, _bh_taylor_mvm, _toeplitz_levinson, _durbin, _trench): the HOST
    call returns the bits of the DEVICE call, and neither writes the padding rows between the extent and the leading dimension."""
    f = cg._ffi
    eps, close = _staged_entry_points(cg, ctx, dt)
    try:
        for name, (square_ok, run) in eps.items():
            for inplace in ((False, True) if square_ok else (False,)):
                host, h0, rows = run(f.HOST, inplace)
                dev, d0, _ = run(f.DEVICE, inplace)
                assert host.shape == dev.shape and np.all(np.isfinite(host[:, :rows])), (name, inplace)
                assert host.tobytes() == dev.tobytes(), (name, inplace, float(np.abs(host.astype(np.float64) - dev).max()))
                if not inplace:
                    assert np.array_equal(host[:, rows:], h0[:, rows:]) and np.array_equal(dev[:, rows:], d0[:, rows:]), (name, "padding rows")
                    assert rows == 0 or not np.array_equal(host[:, :rows], h0[:, :rows]), (name, "nothing written")
    finally:
        close()


# launches covgram_ctx_kernel_time reports after ONE call of each entry point above with "time_kernels" = 1, fp32 and fp64 alike: the literals
# were recorded from the library as it was before the brackets became TimerScope (profiles/driver_refactor_ab.txt: the same calls, HOST and
# DEVICE).  covgram_matrix has no bracket; the gradient MVMs run the three right-hand sides as a pass of two and a pass of one, the Hessian
# MVMs one pass per right-hand side.
_TIMED_LAUNCHES = {
    "covgram_mvm": 1, "covgram_grad_mvm": 2, "covgram_valgrad_mvm": 2, "covgram_hess_mvm": 3, "covgram_valgradhess_mvm": 3, "covgram_sm_mvm": 1,
    "covgram_sparse_mvm": 1, "covgram_matrix": 0, "covgram_block_matrix:gradient": 1, "covgram_block_matrix:value_gradient": 1,
    "covgram_block_matrix:hessian": 1, "covgram_block_matrix:value_gradient_hessian": 1, "covgram_sm_matrix": 1,
    # the structured operators, by entry point (every shape of one entry counts the same; profiles/structured_driver_ab.txt): only the Barnes-Hut
    # walks are bracketed, and a factorization without rows returns before any launch
    "covgram_toeplitz_mvm": 0, "covgram_kron_mvm": 0, "covgram_lowrank_mvm": 0, "covgram_bh_mvm": 1, "covgram_bh_taylor_mvm": 1, "norows": 0,
    "covgram_toeplitz_levinson": 0, "covgram_toeplitz_durbin": 0, "covgram_toeplitz_trench": 0,
}


def _timed_launches(name):
    if name in _TIMED_LAUNCHES:
        return _TIMED_LAUNCHES[name]
    return _TIMED_LAUNCHES["norows" if name.endswith(":norows") else name.split(":")[0]]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_timer_bracket_counts_one_pair_per_bracketed_launch(cg, dt):
    """With "time_kernels" = 1 every call leaves only complete event pairs (covgram_ctx_kernel_time returns OK: hipEventElapsedTime
    refuses a pair whose second event was never recorded) and as many of them as the library always counted."""
    lib, f = cg._ffi.lib(), cg._ffi
    h = f._P()
    f.check(lib.covgram_ctx_create(C.byref(h), 0, None))
    eps, close = _staged_entry_points(cg, h, dt)
    try:
        f.check(lib.covgram_ctx_set_option(h, b"time_kernels", 1))
        ms, cnt = C.c_double(), C.c_int64()
        for name, (square_ok, run) in eps.items():
            for loc in (f.HOST, f.DEVICE):
                f.check(lib.covgram_ctx_kernel_time(h, C.byref(ms), C.byref(cnt), 1))
                run(loc, False)
                f.check(lib.covgram_ctx_kernel_time(h, C.byref(ms), C.byref(cnt), 1))
                assert cnt.value == _timed_launches(name) and ms.value >= 0.0, (name, loc, cnt.value)
        f.check(lib.covgram_ctx_set_option(h, b"time_kernels", 0))
    finally:
        close()
        assert lib.covgram_ctx_destroy(h) == 0
