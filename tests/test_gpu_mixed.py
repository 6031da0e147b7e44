"""Scalar Gramians of mixed-trait composites on the device (covgram_mvm_mixed / covgram_matrix_mixed, csrc/mixed_mvm.hpp) against the
fp64 restatement tests/mixed_ref.py, ENTRY BY ENTRY, with the conditioning majorant K̄ of that module:

    Matrix:  |G_ij − ref_ij| <= TOL · K̄_ij + tiny
    MVM:     |b_i − (α ref_i + β y0_i)| <= TOL · (|α| Σ_j K̄_ij |a_j| + |β| |y0_i|)

fp64: TOL = 1e-12, fp32: 1e-5 (BASELINE.json's contracts, as the row-wise and entry-wise tests use them).  Every case asserts its
route from the info key last_mixed_path BEFORE its numbers and prints worst err / bound.  The inputs are those
tests/test_mixed_host.py checks for feasibility (rounded to fp32, so that both dtypes see the same points)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mixed_ref as R

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-5, torch.float64: 1e-12}
TINY = float(np.finfo(np.float64).tiny)
LANE, CHUNKED, ISO, DOT, JSPLIT, CONST = 1, 2, 4, 8, 16, 32
GRAD_NAMES = ["eq+dot", "eq+(dot^2+1)", "eq*(dot^2+1)", "dot*dot", "maternp2+dot^2+nn", "nn(0.5)*ls(eq,2)", "(eq*dot)^2", "eq*dot zero"]
NAMES = GRAD_NAMES + R.EXTRA
# what the default partition must report: (delegated / constant bits, whether the fused kernel runs)
DEFAULT = {"eq+dot": (ISO | DOT, False), "eq+(dot^2+1)": (ISO | DOT | CONST, False), "eq*(dot^2+1)": (0, True), "dot*dot": (DOT, False),
           "maternp2+dot^2+nn": (ISO | DOT, True), "nn(0.5)*ls(eq,2)": (0, True), "(eq*dot)^2": (0, True), "eq*dot zero": (0, True),
           "exp+dot": (ISO | DOT, False), "gammaexp(1.5)*dot": (0, True), "maternp0+dot": (ISO | DOT, False), "matern(2.3)+dot": (ISO | DOT, False)}
CASES = [(name, i) for name in NAMES for i, shape in enumerate(R.SHAPES) if shape in R.shapes_of(name)]
_CACHE = {}


@pytest.fixture
def options(cg):
    yield lambda kv: [cg.set_option(k, v) for k, v in kv.items()]
    cg.set_option("jsplit", 0)
    cg.set_option("mixed_fuse", 0)


def inputs(cg, oracle, name, n, m, d, same, nrhs=1):
    """(k, X, Y, A, M, Kb) in fp64, computed once per case and left unchanged: M the reference matrix, Kb the majorant."""
    key = (name, n, m, d, same, nrhs)
    if key not in _CACHE:
        k = R.kernels(cg)[name]
        X, Y = R.clouds32(name, n, m, d, same)
        _CACHE[key] = (k, X, Y, R.weights32(Y.shape[0], nrhs), R.matrix(cg, oracle, k, X, Y), R.majorant(cg, oracle, k, X, Y))
    return _CACHE[key]


def operator(cg, k, X, Y, same, dt):
    """The Gramian as gramian() returns it — a MixedGramian — except for Dot() * Dot(), whose factors share one trait: gramian() keeps
    its old route, so the mixed operator is built directly to run the same kernel through covgram_mvm_mixed."""
    x = torch.tensor(X, dtype=dt, device="cuda")
    y = None if same else torch.tensor(Y, dtype=dt, device="cuda")
    if cg.device_spec(k) is None:
        G = cg.gramian(k, x, y)
        assert type(G) is cg.MixedGramian
        return G
    assert type(cg.gramian(k, x, y)) is cg.Gramian
    return cg.MixedGramian(k, x, y)


def check(label, got, ref, bound, dt, floor=0.0):
    """worst |got − ref| / bound over the entries (an exact zero against a zero bound is no error)"""
    assert np.all(np.isfinite(got)), f"{label}: non-finite entries"
    diff = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(diff <= floor, 0.0, diff / bound)
    worst = float(e.max()) if e.size else 0.0
    print(f"{label}: worst err / bound = {worst:.3e} / {TOL[dt]:.0e}")
    assert worst <= TOL[dt], f"{label}: {worst:.3e} > {TOL[dt]:.0e} at flat entry {int(e.argmax())}"


def assert_path(cg, name, d, fuse, opts):
    path, js = cg.get_info("last_mixed_path"), cg.get_info("last_mixed_jsplit")
    route = LANE if d <= 32 else CHUNKED
    deleg, fused = (0, True) if fuse else DEFAULT[name]
    assert path & (ISO | DOT | CONST) == deleg, (name, fuse, path)
    assert path & (LANE | CHUNKED) == (route if fused else 0), (name, fuse, path)
    assert bool(path & JSPLIT) == (fused and js > 1) and (js >= 1) == fused, (name, fuse, path, js)
    if fused and "jsplit" in opts:
        assert js == opts["jsplit"] and path & JSPLIT, (path, js)
    return path


@pytest.mark.parametrize("fuse", [1, 0], ids=["fused", "default"])
@pytest.mark.parametrize("name,shape", CASES, ids=[f"{n}-{'x'.join(str(v) for v in R.SHAPES[i][:3])}" for n, i in CASES])
def test_every_entry_of_the_product(cg, oracle, options, name, shape, fuse):
    n, m, d, same, opts = R.SHAPES[shape]
    k, X, Y, A, M, Kb = inputs(cg, oracle, name, n, m, d, same)
    ref, bound = M @ A[:, 0], Kb @ np.abs(A[:, 0])
    for dt in (torch.float64, torch.float32):
        G = operator(cg, k, X, Y, same, dt)
        options(dict(opts, mixed_fuse=fuse))
        b = G @ torch.tensor(A[:, 0], dtype=dt, device="cuda")
        path = assert_path(cg, name, d, fuse, opts)
        check(f"{name} {n}x{m}x{d} fuse={fuse} path={path} | {dt}", b.cpu().numpy().astype(np.float64), ref, bound, dt)


@pytest.mark.parametrize("name,shape", CASES, ids=[f"{n}-{'x'.join(str(v) for v in R.SHAPES[i][:3])}" for n, i in CASES])
def test_every_entry_of_the_matrix(cg, oracle, name, shape):
    n, m, d, same, _ = R.SHAPES[shape]
    k, X, Y, A, M, Kb = inputs(cg, oracle, name, n, m, d, same)
    for dt in (torch.float64, torch.float32):
        D = operator(cg, k, X, Y, same, dt).to_dense()
        assert cg.get_info("last_mixed_matrix_path") == (1 if d <= 32 else 2)
        assert tuple(D.shape) == (n, m)
        check(f"matrix {name} {n}x{m}x{d} | {dt}", D.cpu().numpy().astype(np.float64), M, Kb + TINY, dt)


@pytest.mark.parametrize("shape", [6, 3], ids=["registers", "chunked"])
def test_matrix_leading_dimension_and_host_memory(cg, oracle, shape):
    """ldo > n: the padding rows stay untouched; loc = HOST writes the caller's host array; the transpose, G[i, j] and block slices."""
    f = cg._ffi
    name = "maternp2+dot^2+nn"
    n, m, d, same, _ = R.SHAPES[shape]
    k, X, Y, A, M, Kb = inputs(cg, oracle, name, n, m, d, same)
    for dt, npdt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        G = operator(cg, k, X, Y, same, dt)
        ctx = G._px.ctx.bind_stream()
        ldo = n + 5
        for loc in (f.DEVICE, f.HOST):
            if loc == f.DEVICE:
                out = torch.full((m, ldo), -7.0, dtype=dt, device="cuda")
                ptr = out.data_ptr()
            else:
                out = np.full((m, ldo), -7.0, dtype=npdt)
                ptr = out.ctypes.data
            f.check(f.lib().covgram_matrix_mixed(ctx, C.byref(G._spec), G._px.handle, G._py.handle, f._P(ptr), ldo, loc))
            assert cg.get_info("last_mixed_matrix_path") == (1 if d <= 32 else 2)
            got = (out.cpu().numpy() if loc == f.DEVICE else out).astype(np.float64)
            assert np.all(got[:, n:] == -7.0), "padding rows were written"
            check(f"matrix ldo > n loc={loc} {n}x{m}x{d} | {dt}", got[:, :n].T, M, Kb + TINY, dt)
        check(f"transpose | {dt}", G.T.to_dense().cpu().numpy().astype(np.float64), M.T, Kb.T + TINY, dt)
        assert type(G.T) is cg.MixedGramian and G.T.shape == (m, n)
        check(f"G[3, 5] | {dt}", np.array([float(G[3, 5])]), M[3:4, 5], Kb[3:4, 5] + TINY, dt)
        sub = G[2:9, [1, 4]]
        check(f"G[2:9, [1, 4]] | {dt}", sub.cpu().numpy().astype(np.float64), M[2:9][:, [1, 4]], Kb[2:9][:, [1, 4]] + TINY, dt)


# ---- semantics of the product ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [1, 0], ids=["fused", "default"])
@pytest.mark.parametrize("name", ["maternp2+dot^2+nn", "eq*(dot^2+1)"])
@pytest.mark.parametrize("shape", [(130, 130, 5), (70, 70, 40)], ids=["lane", "chunked"])
def test_mul_semantics(cg, oracle, options, shape, name, fuse):
    """nrhs = 3 (three single columns) and nrhs = 5 (a group of four and a remainder); α, β ≠ 0 on a random y; β = 0 on a NaN-filled y;
    y aliasing a (square case)."""
    n, m, d = shape
    rng = np.random.default_rng(3)
    k, X, Y, A5, M, Kb = inputs(cg, oracle, name, n, m, d, True, nrhs=5)
    for nrhs in (3, 5):
        A = A5[:, :nrhs]
        ref, bound = M @ A, Kb @ np.abs(A)
        for dt in (torch.float64, torch.float32):
            G = operator(cg, k, X, Y, True, dt)
            options({"mixed_fuse": fuse})
            a = torch.tensor(A, dtype=dt, device="cuda")
            y0 = rng.standard_normal(ref.shape).astype(np.float32).astype(np.float64)
            y = torch.tensor(y0, dtype=dt, device="cuda")
            cg.mul_(y, G, a, -1.75, 0.5)
            assert_path(cg, name, d, fuse, {})
            check(f"{name} nrhs={nrhs} alpha, beta fuse={fuse} | {dt}", y.cpu().numpy().astype(np.float64), -1.75 * ref + 0.5 * y0,
                  1.75 * bound + 0.5 * np.abs(y0), dt)
            y = torch.full(ref.shape, float("nan"), dtype=dt, device="cuda")
            cg.mul_(y, G, a, 2.0, 0.0)
            check(f"{name} nrhs={nrhs} beta=0 on NaN fuse={fuse} | {dt}", y.cpu().numpy().astype(np.float64), 2.0 * ref, 2.0 * bound, dt)
            v = a[:, 1].clone()
            cg.mul_(v, G, v)                                                    # y aliases a
            check(f"{name} y aliasing a fuse={fuse} | {dt}", v.cpu().numpy().astype(np.float64), ref[:, 1], bound[:, 1], dt)
            w = a.clone()
            cg.mul_(w, G, w)                                                    # ... and a whole block of right-hand sides
            check(f"{name} nrhs={nrhs} Y aliasing A fuse={fuse} | {dt}", w.cpu().numpy().astype(np.float64), ref, bound, dt)


@pytest.mark.parametrize("d", [5, 40], ids=["lane", "chunked"])
def test_no_columns_gives_beta_y(cg, d):
    k = cg.MaternP(2) + cg.Dot() ** 2 + cg.NeuralNetwork()
    for dt in (torch.float64, torch.float32):
        x = torch.randn(37, d, dtype=dt, device="cuda")
        G = cg.gramian(k, x, torch.zeros((0, d), dtype=dt, device="cuda"))
        assert type(G) is cg.MixedGramian and G.shape == (37, 0)
        y0 = torch.randn(37, 2, dtype=dt, device="cuda")
        y = y0.clone()
        cg.mul_(y, G, torch.zeros((0, 2), dtype=dt, device="cuda"), 3.0, -0.5)
        assert cg.get_info("last_mixed_path") == 0 and cg.get_info("last_mixed_jsplit") == 0
        assert torch.equal(y, -0.5 * y0)
        y = torch.full((37,), float("nan"), dtype=dt, device="cuda")
        cg.mul_(y, G, torch.zeros(0, dtype=dt, device="cuda"), 3.0, 0.0)
        assert torch.equal(y, torch.zeros_like(y))
        # and no rows: nothing to do
        G0 = cg.gramian(k, torch.zeros((0, d), dtype=dt, device="cuda"), x)
        assert (G0 @ torch.ones(37, dtype=dt, device="cuda")).shape == (0,)


@pytest.mark.parametrize("fuse", [1, 0], ids=["fused", "default"])
def test_two_identical_calls_agree_bit_for_bit(cg, oracle, options, fuse):
    for name, (n, m, d) in (("maternp2+dot^2+nn", (333, 517, 3)), ("eq*(dot^2+1)", (100, 384, 40))):
        k, X, Y, A, M, Kb = inputs(cg, oracle, name, n, m, d, False, nrhs=5)
        for dt in (torch.float64, torch.float32):
            G = operator(cg, k, X, Y, False, dt)
            a = torch.tensor(A, dtype=dt, device="cuda")
            for js in (1, 3):
                options({"mixed_fuse": fuse, "jsplit": js})
                b1 = G @ a
                path = cg.get_info("last_mixed_path")
                assert bool(path & JSPLIT) == (js > 1) and cg.get_info("last_mixed_jsplit") == js, (path, js)
                b2 = G @ a
                assert torch.equal(b1, b2), (name, dt, js)


# ---- what gramian()'s recursion gives without further code -------------------------------------------------------------------------------
def test_cg_mbcg_and_logdet_on_g_plus_diagonal(cg, oracle):
    n, d = 300, 3
    k = cg.EQ() + 0.5 * cg.Dot()
    X, _ = R.clouds32("x", n, n, d, True)
    x = torch.tensor(X, device="cuda")
    G = cg.gramian(k, x)
    assert type(G) is cg.MixedGramian and G.issymmetric() and G.isposdef()
    sig = 1e-2 * torch.ones(n, dtype=torch.float64, device="cuda")
    A = G + sig
    assert type(A) is cg.LazyMatrixSum
    rng = np.random.default_rng(21)
    B = torch.tensor(rng.standard_normal((n, 3)), device="cuda")
    b = B[:, 0].contiguous()
    xs, info = cg.cg(A, b, reltol=1e-9, maxiter=4 * n)
    res = float((G @ xs + sig * xs - b).norm())
    print(f"mixed cg: residual {res:.3e}, |b| {float(b.norm()):.3e}, {info['iterations']} iterations")
    assert info["converged"] and res <= 2e-9 * float(b.norm())                  # the tolerance the CG tests of the other operators use
    Xs, info = cg.mbcg(A, B, reltol=1e-9, maxiter=4 * n)
    assert info["converged"]
    Md = R.matrix(cg, oracle, k, X, X) + 1e-2 * np.eye(n)
    cond = float(np.linalg.cond(Md))
    for c in range(3):
        xc, _ = cg.cg(A, B[:, c].contiguous(), reltol=1e-9, maxiter=4 * n)
        assert float((Xs[:, c] - xc).norm()) <= 2 * cond * 1e-9 * float(xc.norm()), c
    est, info = cg.logdet(A, probes=32, generator=torch.Generator(device="cuda").manual_seed(1))
    ld = float(np.linalg.slogdet(Md)[1])
    print(f"mixed logdet: {est:.6g} against {ld:.6g}, stderr {info['stderr']:.3g}")
    assert info["converged"] and abs(est - ld) <= 5 * info["stderr"] + 1e-3 * abs(ld)


def test_transformed_inputs(cg, oracle):
    """ARD, Warped and VerticalRescaling of a mixed kernel: gramian() transforms the points once and builds a MixedGramian on them."""
    n, m, d = 40, 33, 3
    X, Y = R.clouds32("x", n, m, d, False)
    x, y = torch.tensor(X, device="cuda"), torch.tensor(Y, device="cuda")
    a = R.weights32(m)[:, 0]
    at = torch.tensor(a, device="cuda")
    k = cg.EQ() + cg.Dot()
    l = np.array([0.5, 2.0, 1.25])
    G = cg.gramian(cg.ARD(k, l), x, y)
    assert type(G) is cg.MixedGramian
    M, Kb = R.matrix(cg, oracle, k, X / l, Y / l), R.majorant(cg, oracle, k, X / l, Y / l)
    check("ARD(EQ + Dot, l)", (G @ at).cpu().numpy(), M @ a, Kb @ np.abs(a), torch.float64)
    U = np.array([[1.0, 0.5, 0.0], [0.0, -1.0, 2.0]])
    G = cg.gramian(cg.Warped(k, U), x, y)
    assert type(G) is cg.MixedGramian
    M, Kb = R.matrix(cg, oracle, k, X @ U.T, Y @ U.T), R.majorant(cg, oracle, k, X @ U.T, Y @ U.T)
    check("Warped(EQ + Dot, U)", (G @ at).cpu().numpy(), M @ a, Kb @ np.abs(a), torch.float64)
    f = lambda p: 1.0 + (p * p).sum(1)
    V = cg.gramian(cg.VerticalRescaling(cg.EQ() * (cg.Dot() ** 2 + 1), f), x, y)
    assert type(V) is cg.ScaledOperator and type(V.K) is cg.MixedGramian
    k2 = cg.EQ() * (cg.Dot() ** 2 + 1)
    fx, fy = 1.0 + (X * X).sum(1), 1.0 + (Y * Y).sum(1)
    M, Kb = R.matrix(cg, oracle, k2, X, Y), R.majorant(cg, oracle, k2, X, Y)
    check("VerticalRescaling(EQ (Dot^2 + 1), f)", (V @ at).cpu().numpy(), fx * (M @ (fy * a)), fx * (Kb @ np.abs(fy * a)), torch.float64)


def test_refusals_on_the_device_tier(cg):
    """nrhs < 1 and lda < m / ldy < n / ldo < n (they need point handles); and the functions without a mixed path name the class."""
    f = cg._ffi
    x = torch.randn(9, 3, dtype=torch.float64, device="cuda")
    G = cg.gramian(cg.EQ() + cg.Dot(), x)
    assert type(G) is cg.MixedGramian
    ctx = G._px.ctx.bind_stream()
    a, y = torch.zeros(9, dtype=torch.float64, device="cuda"), torch.zeros(9, dtype=torch.float64, device="cuda")
    call = lambda lda, ldy, nrhs: f.lib().covgram_mvm_mixed(ctx, C.byref(G._spec), G._px.handle, G._py.handle, f._P(a.data_ptr()), lda, f._P(y.data_ptr()),
                                                             ldy, nrhs, 1.0, 0.0, f.DEVICE)
    assert call(9, 9, 0) == f.EINVAL and b"nrhs" in f.lib().covgram_last_error()
    assert call(8, 9, 1) == f.EINVAL and call(9, 8, 1) == f.EINVAL
    assert f.lib().covgram_matrix_mixed(ctx, C.byref(G._spec), G._px.handle, G._py.handle, f._P(y.data_ptr()), 8, f.DEVICE) == f.EINVAL
    assert call(9, 9, 1) == f.OK
    u = torch.zeros(9, dtype=torch.float64, device="cuda")
    for fn in (lambda: cg.sparse(G), lambda: cg.BarnesHutFactorization(G), lambda: cg.pivoted_cholesky(G, 4), lambda: cg.bilinear_gradient(G, u, u),
               lambda: cg.bilinear_input_gradient(G, u, u), lambda: G.sym_partial_(y, a, 0, 2), lambda: cg.ShardedGramian(cg.EQ() + cg.Dot(), x)):
        with pytest.raises(cg.UnsupportedKernel, match="MixedGramian"):
            fn()
