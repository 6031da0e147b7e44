"""SpectralMixture Gramians on the device (covgram_sm_*, csrc/sm.hip): Matrix(G) entry by entry and the product row by row against the
fp64 reference and the bound of tests/sm_ref.py, on every d bucket, one and several component chunks, both lengthscale forms, one
column tile and many, the direct and the column-split product; the public routes (gramian, Toeplitz, diagonal, cg, mbcg) and the
refusals of the C ABI.

Products are judged row-wise with the formula of tests/test_gpu_sparse.py:
    |y_i - ref_i| <= |alpha| sum_j bound_ij |a_j| + TOL (|alpha| sum_j |ref_ij| |a_j| + |beta| |y0_i|) + tiny."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sm_ref as sr

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TDT = {F32: torch.float32, F64: torch.float64}
DTYPES = [F32, F64]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def case_data(case, dtname):
    """The cloud, the parameters and (ref, bound), computed once and shared (read-only) by the tests that need them."""
    dt = F32 if dtname == "float32" else F64
    X, Y, w, mu, l, inv_l = sr.make_case(case, dt)
    ref, bound = sr.reference_and_bound(w, mu, inv_l, X, Y, dt)
    for a in (X, Y, ref, bound):
        a.setflags(write=False)
    return X, Y, w, mu, l, inv_l, ref, bound


def kernel_of(cg, w, mu, l):
    return cg.SM(w, [m for m in mu], [lq for lq in l])


def rowwise(name, dt, got, ref, bound, a, y0, alpha, beta):
    a64 = a.astype(F64).reshape(a.shape[0], -1)
    g = np.asarray(got, dtype=F64).reshape(ref.shape[0], -1)
    yb = np.zeros_like(g) if beta == 0 else y0.astype(F64).reshape(g.shape)
    want = alpha * (ref @ a64) + beta * yb
    lim = abs(alpha) * (bound @ np.abs(a64)) + sr.TOL[dt] * (abs(alpha) * (np.abs(ref) @ np.abs(a64)) + abs(beta) * np.abs(yb)) + sr.tiny(dt)
    with np.errstate(invalid="ignore"):
        r = np.where(np.isfinite(g), np.abs(g - want) / lim, np.inf)
    worst = float(r.max()) if r.size else 0.0
    print(f"sm-rowwise {name}: worst err/bound {worst:.3f}")
    return worst


# ---- Matrix(G) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", sr.CASES, ids=lambda c: sr.case_name(c, F64)[:-8])
def test_matrix_entrywise(cg, dev, case, dt):
    X, Y, w, mu, l, inv_l, ref, bound = case_data(case, np.dtype(dt).name)
    G = cg.gramian(kernel_of(cg, w, mu, l), torch.from_numpy(X.copy()).to(dev), torch.from_numpy(Y.copy()).to(dev))
    assert isinstance(G, cg.SpectralMixtureGramian) and G.shape == ref.shape and G.dtype == TDT[dt]
    assert G.isotropic() == (case[4] or case[2] == 1)
    M = G.to_dense().cpu().numpy()
    r, i, j = sr.worst_entry(M, ref, bound)
    print(f"sm-matrix {sr.case_name(case, dt)}: worst err/bound {r:.3f} at ({i}, {j}) got {M[i, j]!r} ref {ref[i, j]!r}")
    assert r <= 1.0


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_matrix_one_handle_on_both_sides_and_indexing(cg, dev, dt):
    rng = np.random.default_rng(11)
    n, d, Q = 257, 3, 3
    X = sr.mc.iso_cloud(rng, n, n, d, dt)[0]
    w, mu, l = sr.params(rng, Q, d, False)
    ref, bound = sr.reference_and_bound(w, mu, sr.inv_l_of(l, d), X, X, dt)
    G = cg.gramian(kernel_of(cg, w, mu, l), torch.from_numpy(X).to(dev))
    assert isinstance(G, cg.SpectralMixtureGramian) and G.issymmetric() and G._px is G._py
    M = G.to_dense().cpu().numpy()
    r, i, j = sr.worst_entry(M, ref, bound)
    print(f"sm-matrix symmetric {np.dtype(dt).name}: worst err/bound {r:.3f} at ({i}, {j})")
    assert r <= 1.0
    assert sr.worst_entry(G.T.to_dense().cpu().numpy(), ref.T, bound.T)[0] <= 1.0
    sub = G[3:40, 100:257].cpu().numpy()
    assert sr.worst_entry(sub, ref[3:40, 100:257], bound[3:40, 100:257])[0] <= 1.0
    assert abs(float(G[5, 7]) - ref[5, 7]) <= bound[5, 7]
    assert sr.worst_entry(G[5, :].cpu().numpy()[None, :], ref[5:6], bound[5:6])[0] <= 1.0


def _sm_handle(cg, ctx, w, mu, inv_l, code):
    h = cg._ffi._P()
    as_d = lambda v: np.ascontiguousarray(v, dtype=F64).ctypes.data_as(C.POINTER(C.c_double))
    st = cg._ffi.lib().covgram_sm_create(ctx, C.byref(h), int(np.shape(w)[0]), int(np.shape(mu)[1]), as_d(w), as_d(mu), as_d(inv_l), code)
    return st, h


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_matrix_leading_dimension_keeps_sentinel_rows(cg, dev, dt):
    case = (63, 193, 3, 3, False)
    X, Y, w, mu, l, inv_l, ref, bound = case_data(case, np.dtype(dt).name)
    n, m = ref.shape
    ldo = n + 5
    lib, P = cg._ffi.lib(), cg._ffi._P
    G = cg.gramian(kernel_of(cg, w, mu, l), torch.from_numpy(X.copy()).to(dev), torch.from_numpy(Y.copy()).to(dev))
    out = torch.full((m, ldo), -7.5, dtype=TDT[dt], device=dev)          # column-major ldo x m
    G._px.ctx.bind_stream()
    cg._ffi.check(lib.covgram_sm_matrix(G.handle, G._px.handle, G._py.handle, P(out.data_ptr()), ldo, cg._ffi.DEVICE))
    o = out.cpu().numpy()
    assert np.all(o[:, n:] == -7.5)
    assert sr.worst_entry(o[:, :n].T, ref, bound)[0] <= 1.0
    host = np.full((m, ldo), -7.5, dtype=dt)                               # the same through host memory
    cg._ffi.check(lib.covgram_sm_matrix(G.handle, G._px.handle, G._py.handle, P(host.ctypes.data), ldo, cg._ffi.HOST))
    assert np.all(host[:, n:] == -7.5) and np.array_equal(host[:, :n], o[:, :n])


# ---- products ------------------------------------------------------------------------------------------------------------------------
MVM_CASES = [(257, 193, 3, 3, True), (63, 1500, 8, 3, False), (257, 1500, 1, 3, False), (257, 193, 8, 32, False)]


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", MVM_CASES, ids=lambda c: sr.case_name(c, F64)[:-8])
def test_products_rowwise(cg, dev, case, dt):
    X, Y, w, mu, l, inv_l, ref, bound = case_data(case, np.dtype(dt).name)
    n, m = ref.shape
    G = cg.gramian(kernel_of(cg, w, mu, l), torch.from_numpy(X.copy()).to(dev), torch.from_numpy(Y.copy()).to(dev))
    rng = np.random.default_rng(3)
    worst = 0.0
    for nrhs in (1, 3, 17):
        a = rng.standard_normal((m, nrhs)).astype(dt)
        y0 = rng.standard_normal((n, nrhs)).astype(dt)
        at = torch.from_numpy(a).to(dev)
        for alpha, beta in ((1.0, 0.0), (-0.7, 1.3)):
            yt = torch.full((n, nrhs), float("nan"), dtype=TDT[dt], device=dev) if beta == 0 else torch.from_numpy(y0).to(dev)
            if nrhs == 1:
                got = cg.mul_(yt[:, 0].contiguous(), G, at[:, 0].contiguous(), alpha, beta).cpu().numpy()
            else:
                got = cg.mul_(yt, G, at, alpha, beta).cpu().numpy()
            worst = max(worst, rowwise(f"{sr.case_name(case, dt)} nrhs={nrhs} alpha={alpha} beta={beta}", dt, got, ref, bound, a, y0, alpha, beta))
    # non-contiguous y: a strided vector and the columns of a wider matrix
    a = rng.standard_normal((m, 3)).astype(dt); y0 = rng.standard_normal((n, 3)).astype(dt)
    at = torch.from_numpy(a).to(dev)
    wide = torch.zeros((n, 6), dtype=TDT[dt], device=dev)
    wide[:, ::2] = torch.from_numpy(y0).to(dev)
    cg.mul_(wide[:, ::2], G, at, -0.7, 1.3)
    worst = max(worst, rowwise("strided matrix y", dt, wide[:, ::2].cpu().numpy(), ref, bound, a, y0, -0.7, 1.3))
    assert bool(torch.all(wide[:, 1::2] == 0))
    long = torch.full((2 * n,), float("nan"), dtype=TDT[dt], device=dev)
    cg.mul_(long[::2], G, at[:, 0].contiguous(), 1.0, 0.0)
    worst = max(worst, rowwise("strided vector y", dt, long[::2].cpu().numpy(), ref, bound, a[:, :1], y0[:, :1], 1.0, 0.0))
    assert (G @ at).shape == (n, 3) and (G @ at[:, 0].contiguous()).shape == (n,)
    assert worst <= 1.0


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_product_in_place_and_empty_sides(cg, dev, dt):
    rng = np.random.default_rng(12)
    n, d, Q = 257, 3, 3
    X = sr.mc.iso_cloud(rng, n, n, d, dt)[0]
    w, mu, l = sr.params(rng, Q, d, True)
    ref, bound = sr.reference_and_bound(w, mu, sr.inv_l_of(l, d), X, X, dt)
    k = kernel_of(cg, w, mu, l)
    Xt = torch.from_numpy(X).to(dev)
    G = cg.gramian(k, Xt)
    a = rng.standard_normal((n, 3)).astype(dt)
    v = torch.from_numpy(a[:, 0].copy()).to(dev)
    cg.mul_(v, G, v, 1.0, 0.0)                                             # y aliases a
    assert rowwise("in place vector", dt, v.cpu().numpy(), ref, bound, a[:, :1], a[:, :1], 1.0, 0.0) <= 1.0
    Vt = torch.from_numpy(a.T.copy()).to(dev).t()                          # column-major storage: the library writes y where it reads a
    cg.mul_(Vt, G, Vt, -0.7, 1.3)
    assert rowwise("in place matrix", dt, Vt.cpu().numpy(), ref, bound, a, a, -0.7, 1.3) <= 1.0
    # n = 0 and m = 0
    empty = torch.zeros((0, d), dtype=TDT[dt], device=dev)
    G0 = cg.gramian(k, empty, Xt)
    assert isinstance(G0, cg.SpectralMixtureGramian) and G0.shape == (0, n)
    assert cg.mul_(torch.zeros(0, dtype=TDT[dt], device=dev), G0, torch.from_numpy(a[:, 0].copy()).to(dev)).shape == (0,)
    assert G0.to_dense().shape == (0, n)
    Gm = cg.gramian(k, Xt, empty)
    y0 = rng.standard_normal(n).astype(dt)
    y = torch.from_numpy(y0.copy()).to(dev)
    cg.mul_(y, Gm, torch.zeros(0, dtype=TDT[dt], device=dev), 1.0, 1.3)
    assert np.allclose(y.cpu().numpy(), dt(1.3) * y0, rtol=4 * np.finfo(dt).eps)
    ynan = torch.full((n, 2), float("nan"), dtype=TDT[dt], device=dev)
    cg.mul_(ynan, Gm, torch.zeros((0, 2), dtype=TDT[dt], device=dev), 1.0, 0.0)
    assert bool(torch.all(ynan == 0))


# ---- agreement with the routes that already exist ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_pure_cosine_term_agrees_with_the_rank_two_product(cg, dev, dt):
    rng = np.random.default_rng(13)
    n, m, d = 63, 193, 3
    X, Y = sr.mc.iso_cloud(rng, n, m, d, dt)[:2]
    c = np.array([0.4, -1.1, 0.7])
    k = 1.5 * cg.Cosine(c)                                                # inv_l = 0: no EQ factor
    Xt, Yt = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    G = cg.gramian(k, Xt, Yt)
    assert isinstance(G, cg.SpectralMixtureGramian) and np.array_equal(G.inv_l, np.zeros((1, d)))
    L = cg.gramian(cg.Cosine(c), Xt, Yt)
    assert isinstance(L, cg.LazyMatrixProduct)                            # a bare Cosine keeps its rank-2 route
    ref, bound = sr.reference_and_bound(np.array([1.5]), c[None, :], np.zeros((1, d)), X, Y, dt)
    A = G.to_dense().cpu().numpy().astype(F64); B = 1.5 * L.to_dense().cpu().numpy().astype(F64)
    r = float(np.max(np.abs(A - B) / (2 * bound)))
    print(f"sm-vs-rank2 {np.dtype(dt).name}: worst |difference| / (sum of both bounds) {r:.3f}")
    assert r <= 1.0 and sr.worst_entry(A, ref, bound)[0] <= 1.0


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_zero_frequencies_agree_with_the_composite_eq_sum(cg, dev, dt):
    rng = np.random.default_rng(14)
    n, m, d = 257, 193, 3
    X, Y = sr.mc.iso_cloud(rng, n, m, d, dt)[:2]
    w, l = [1.3, 0.6], [0.8, 1.7]
    ksm = cg.Sum(tuple(cg.Product((cg.Constant(wq), cg.Cosine(0.0), cg.Lengthscale(cg.EQ(), lq))) for wq, lq in zip(w, l)))
    keq = cg.Sum(tuple(wq * cg.Lengthscale(cg.EQ(), lq) for wq, lq in zip(w, l)))
    Xt, Yt = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    G, E = cg.gramian(ksm, Xt, Yt), cg.gramian(keq, Xt, Yt)
    assert isinstance(G, cg.SpectralMixtureGramian) and type(E) is cg.Gramian   # sums of EQs stay composites
    ref, bound = sr.reference_and_bound(np.array(w), np.zeros((2, d)), sr.inv_l_of(np.array(l), d), X, Y, dt)
    with np.errstate(divide="ignore"):
        L = -np.log(np.abs(ref) / sum(w))
    biso = np.where(ref != 0, sr.TOL[dt] * np.maximum(1.0, L / 10.0) * np.abs(ref), 0.0) + sr.tiny(dt)   # matrix_cases' isotropic rule
    A = G.to_dense().cpu().numpy().astype(F64); B = E.to_dense().cpu().numpy().astype(F64)
    r = float(np.max(np.abs(A - B) / (bound + biso)))
    print(f"sm-vs-composite {np.dtype(dt).name}: worst |difference| / (sum of both bounds) {r:.3f}")
    assert r <= 1.0 and sr.worst_entry(A, ref, bound)[0] <= 1.0


# ---- the public API ------------------------------------------------------------------------------------------------------------------
def test_ranges_toeplitz_and_diagonal(cg, dev):
    n = 257
    w = np.array([1.2, 0.5, 0.8]); mu = np.array([[0.0], [1.7], [-0.6]]); l = np.array([0.4, 1.1, 0.25])
    k = cg.SM(w, mu, l)
    x = cg.srange(-1.0, 1.5, n)
    pts = (x.start + x.step * np.arange(n))[:, None]
    ref, bound = sr.reference_and_bound(w, mu, sr.inv_l_of(l, 1), pts, pts, F64)
    T = cg.gramian(k, x, cg.StationaryInput())
    assert isinstance(T, cg.SymmetricToeplitz)
    assert isinstance(cg.gramian(k, x, cg.IsotropicInput()), cg.SymmetricToeplitz)
    G = cg.gramian(k, x)                                                   # no trait passed: the reference's GenericInput rule
    assert isinstance(G, cg.SpectralMixtureGramian)
    rng = np.random.default_rng(15)
    a = rng.standard_normal(n)
    at = torch.from_numpy(a).to(dev)
    assert rowwise("toeplitz", F64, (T @ at).cpu().numpy(), ref, bound, a[:, None], a[:, None], 1.0, 0.0) <= 1.0
    assert rowwise("dense on a range", F64, (G @ at).cpu().numpy(), ref, bound, a[:, None], a[:, None], 1.0, 0.0) <= 1.0
    y = cg.srange(-0.7, 1.8, n)                                            # the same step: a non-symmetric Toeplitz matrix
    T2 = cg.gramian(k, x, y, cg.StationaryInput())
    assert isinstance(T2, cg.Toeplitz)
    ptsy = (y.start + y.step * np.arange(n))[:, None]
    ref2, bound2 = sr.reference_and_bound(w, mu, sr.inv_l_of(l, 1), pts, ptsy, F64)
    assert rowwise("toeplitz x != y", F64, (T2 @ at).cpu().numpy(), ref2, bound2, a[:, None], a[:, None], 1.0, 0.0) <= 1.0
    dg = cg.diagonal(G)
    assert dg.shape == (n,) and bool(torch.all(dg == float(np.sum(w))))   # cos(0) exp(0) = 1: exactly the sum of the weights


def test_cg_and_mbcg_on_a_noisy_mixture(cg, dev):
    rng = np.random.default_rng(16)
    n, d, Q = 257, 3, 3
    X = sr.mc.iso_cloud(rng, n, n, d, F64)[0]
    w, mu, l = sr.params(rng, Q, d, False)
    w = np.abs(w)                                                          # positive weights: G is positive semi-definite
    ref, _ = sr.reference_and_bound(w, mu, sr.inv_l_of(l, d), X, X, F64)
    G = cg.gramian(kernel_of(cg, w, mu, l), torch.from_numpy(X).to(dev))
    assert G.isposdef()
    A = G + torch.full((n,), 0.1, dtype=torch.float64, device=dev)
    B = rng.standard_normal((n, 4))
    want = np.linalg.solve(ref + 0.1 * np.eye(n), B)
    x, info = cg.cg(A, torch.from_numpy(B[:, 0].copy()).to(dev), reltol=1e-13, maxiter=20 * n)
    e = float(np.linalg.norm(x.cpu().numpy() - want[:, 0]) / np.linalg.norm(want[:, 0]))
    print(f"sm-cg: {info['iterations']} iterations, relative error {e:.2e}")
    assert e <= 1e-8
    Xs, info = cg.mbcg(A, torch.from_numpy(B).to(dev), reltol=1e-13, maxiter=20 * n)
    e = float(np.max(np.linalg.norm(Xs.cpu().numpy() - want, axis=0) / np.linalg.norm(want, axis=0)))
    print(f"sm-mbcg: {info['iterations']} iterations, worst relative error {e:.2e}")
    assert e <= 1e-8


# ---- refusals of the C ABI -----------------------------------------------------------------------------------------------------------
def test_abi_refusals(cg, dev):
    ffi = cg._ffi
    ctx = cg.get_ctx(dev).bind_stream()
    ones = lambda q, d: (np.ones(q), np.zeros((q, d)), np.ones((q, d)))
    st, h = _sm_handle(cg, ctx, np.ones(0), np.zeros((0, 2)), np.ones((0, 2)), ffi.F64)
    assert st == ffi.EINVAL and not h                                      # ncomp = 0
    w, mu, il = ones(2, 2); il[1, 0] = -0.5
    assert _sm_handle(cg, ctx, w, mu, il, ffi.F64)[0] == ffi.EINVAL       # a negative inverse lengthscale
    w, mu, il = ones(2, 2); w[0] = np.nan
    assert _sm_handle(cg, ctx, w, mu, il, ffi.F32)[0] == ffi.EINVAL       # a NaN weight
    assert _sm_handle(cg, ctx, *ones(33, 1), ffi.F32)[0] == ffi.EUNSUPPORTED
    assert _sm_handle(cg, ctx, *ones(1, 17), ffi.F64)[0] == ffi.EUNSUPPORTED
    assert b"32" in ffi.lib().covgram_last_error() and b"16" in ffi.lib().covgram_last_error()
    st, h = _sm_handle(cg, ctx, *ones(2, 3), ffi.F64)
    assert st == ffi.OK and h
    q, d, dtc, iso = C.c_int32(0), C.c_int32(0), C.c_int32(-1), C.c_int32(0)
    assert ffi.lib().covgram_sm_info(h, C.byref(q), C.byref(d), C.byref(dtc), C.byref(iso)) == ffi.OK
    assert (q.value, d.value, dtc.value, iso.value) == (2, 3, ffi.F64, 1)
    G2 = cg.Gramian(cg.EQ(), torch.zeros((5, 2), dtype=torch.float64, device=dev))          # points of another dimension
    y = torch.zeros(5, dtype=torch.float64, device=dev)
    P = ffi._P
    assert ffi.lib().covgram_sm_mvm(h, G2._px.handle, G2._py.handle, P(y.data_ptr()), 5, P(y.data_ptr()), 5, 1, 1.0, 0.0, ffi.DEVICE) == ffi.EINVAL
    assert ffi.lib().covgram_sm_matrix(h, G2._px.handle, G2._py.handle, P(y.data_ptr()), 5, ffi.DEVICE) == ffi.EINVAL
    G3 = cg.Gramian(cg.EQ(), torch.zeros((5, 3), dtype=torch.float32, device=dev))          # points of another dtype
    assert ffi.lib().covgram_sm_mvm(h, G3._px.handle, G3._py.handle, P(y.data_ptr()), 5, P(y.data_ptr()), 5, 1, 1.0, 0.0, ffi.DEVICE) == ffi.EINVAL
    assert ffi.lib().covgram_sm_destroy(h) == ffi.OK
    with pytest.raises(cg.UnsupportedKernel):                              # out of scope, refused by name before any device call
        cg.sparse(cg.gramian(cg.SM([1.0], [0.3], [1.0]), torch.zeros((4, 1), dtype=torch.float64, device=dev)))
