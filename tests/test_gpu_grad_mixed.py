"""Gradient and value-gradient Gramians of mixed-trait composites on the device (covgram_grad_mvm_mixed, csrc/grad_mixed.hpp) against
the fp64 restatement tests/grad_mixed_ref.py, ENTRY BY ENTRY:

    e = |b − ref| / (|α| absref + |β| |y0|),   absref = the same product with every term replaced by its absolute value,

fp64: e <= 1e-12, fp32: e <= 1e-5 (BASELINE.json's contracts, as tests/test_gpu_grad_rowwise.py uses them).  Every case asserts its
route from the info keys last_grad_mixed_path / last_grad_mixed_jsplit BEFORE its numbers and prints worst err / bound.  The inputs
are those tests/test_grad_mixed_host.py checks for feasibility (rounded to fp32, so that both dtypes see the same points)."""
import numpy as np
import pytest
import torch

import grad_mixed_ref as R

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-5, torch.float64: 1e-12}
LANE, PANEL, MULTI, ZSPLIT, JSPLIT = 1, 2, 4, 8, 16
NAMES = ["eq+dot", "eq+(dot^2+1)", "eq*(dot^2+1)", "dot*dot", "maternp2+dot^2+nn", "nn(0.5)*ls(eq,2)", "(eq*dot)^2", "eq*dot zero"]

# route -> (n, m, d, x is y, options, the path bits it must report)
ROUTES = {
    "lane ragged jsplit": (333, 517, 3, False, {"jsplit": 3}, LANE | JSPLIT),
    "lane same padded": (130, 130, 5, True, {}, None),
    "lane d32": (70, 193, 32, False, {}, None),
    "panel ragged": (100, 37, 33, False, {}, None),
    "panel two panels": (100, 70, 70, False, {"grad_mixed_panel": 48}, PANEL | MULTI | ZSPLIT),
    "panel zsplit": (100, 70, 70, False, {}, PANEL | ZSPLIT),
    "panel one block per panel": (100, 70, 70, False, {"grad_mixed_panel": 1}, PANEL | MULTI),
}
_CACHE = {}


@pytest.fixture
def options(cg):
    yield lambda kv: [cg.set_option(k, v) for k, v in kv.items()]
    cg.set_option("jsplit", 0)
    cg.set_option("grad_mixed_panel", 0)


def inputs(cg, name, n, m, d, same, value, nrhs=1):
    """(k, X, Y, A, ref, absref) in fp64, computed once per case and left unchanged; the points and a are fp32-representable."""
    key = (name, n, m, d, same, value, nrhs)
    if key not in _CACHE:
        k = R.kernels(cg)[name]
        X, Y = R.clouds(name, n, m, d, same)
        X = X.astype(np.float32).astype(np.float64)
        Y = X if same else Y.astype(np.float32).astype(np.float64)
        A = np.random.default_rng(11).standard_normal((Y.shape[0] * (d + value), nrhs)).astype(np.float32).astype(np.float64)
        ref = np.stack([R.mvm(cg, k, X, Y, A[:, c], value) for c in range(nrhs)], 1)
        ab = np.stack([R.absref(cg, k, X, Y, A[:, c], value) for c in range(nrhs)], 1)
        _CACHE[key] = (k, X, Y, A, ref, ab)
    return _CACHE[key]


def operator(cg, k, X, Y, same, value, dt):
    """The Gramian as gramian() returns it — a MixedBlockGramian — except for Dot() * Dot(), whose factors share one trait: gramian()
    keeps its old route, so the mixed operator is built directly to run the same kernel through covgram_grad_mvm_mixed."""
    wrap = cg.ValueGradientKernel if value else cg.GradientKernel
    x = torch.tensor(X, dtype=dt, device="cuda")
    y = None if same else torch.tensor(Y, dtype=dt, device="cuda")
    if cg.device_spec(k) is None:
        G = cg.gramian(wrap(k), x, y)
        assert type(G) is cg.MixedBlockGramian
        return G
    assert type(cg.gramian(wrap(k), x, y)) is cg.BlockGramian
    return cg.MixedBlockGramian(wrap(k), x, y)


def check(label, got, ref, ab, dt, alpha=1.0, beta=0.0, y0=None):
    den = abs(alpha) * ab + (abs(beta) * np.abs(y0) if y0 is not None else 0.0)
    diff = np.abs(got - (alpha * ref + (beta * y0 if y0 is not None else 0.0)))
    assert np.all(np.isfinite(got)), f"{label}: non-finite entries"
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(diff == 0, 0.0, diff / den)
    worst = float(e.max()) if e.size else 0.0
    print(f"{label}: worst err / bound = {worst:.3e} / {TOL[dt]:.0e}")
    assert worst <= TOL[dt], f"{label}: {worst:.3e} > {TOL[dt]:.0e} at flat entry {int(e.argmax())}"


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_every_entry_on_every_route(cg, options, route, name):
    n, m, d, same, opts, bits = ROUTES[route]
    for value in (0, 1):
        k, X, Y, A, ref, ab = inputs(cg, name, n, m, d, same, value)
        for dt in (torch.float64, torch.float32):
            G = operator(cg, k, X, Y, same, value, dt)
            options(opts)
            b = G @ torch.tensor(A[:, 0], dtype=dt, device="cuda")
            path, js = cg.get_info("last_grad_mixed_path"), cg.get_info("last_grad_mixed_jsplit")
            if route.startswith("lane"):
                assert path & LANE and not path & (PANEL | MULTI | ZSPLIT) and js >= 1 and bool(path & JSPLIT) == (js > 1), (path, js)
                if "jsplit" in opts:
                    assert js == opts["jsplit"]
            else:
                assert path & PANEL and not path & (LANE | JSPLIT) and js == 0, (path, js)
            if bits is not None:
                assert path == bits, (route, path, bits)
            check(f"{route} | {name} | value={value} | {dt}", b.cpu().numpy().astype(np.float64), ref[:, 0], ab[:, 0], dt)


@pytest.mark.parametrize("name", ["maternp2+dot^2+nn", "eq*(dot^2+1)"])
@pytest.mark.parametrize("shape", [(130, 130, 5), (70, 70, 40)], ids=["lane", "panel"])
def test_mul_semantics(cg, options, shape, name):
    """nrhs = 3; α, β ≠ 0 on a random y; β = 0 on a NaN-filled y; y aliasing a (square case)."""
    n, m, d = shape
    rng = np.random.default_rng(3)
    for value in (0, 1):
        k, X, Y, A, ref, ab = inputs(cg, name, n, m, d, True, value, nrhs=3)
        for dt in (torch.float64, torch.float32):
            G = operator(cg, k, X, Y, True, value, dt)
            a = torch.tensor(A, dtype=dt, device="cuda")
            want = PANEL if d > 32 else LANE
            y0 = rng.standard_normal(ref.shape).astype(np.float32).astype(np.float64)
            y = torch.tensor(y0, dtype=dt, device="cuda")
            cg.mul_(y, G, a, -1.75, 0.5)
            assert cg.get_info("last_grad_mixed_path") & want
            check(f"{name} nrhs=3 alpha, beta | value={value} | {dt}", y.cpu().numpy().astype(np.float64), ref, ab, dt, -1.75, 0.5, y0)
            y = torch.full(ref.shape, float("nan"), dtype=dt, device="cuda")
            cg.mul_(y, G, a, 2.0, 0.0)
            check(f"{name} beta=0 on NaN | value={value} | {dt}", y.cpu().numpy().astype(np.float64), ref, ab, dt, 2.0)
            v = a[:, 1].clone()
            cg.mul_(v, G, v)                                                    # y aliases a
            check(f"{name} y aliasing a | value={value} | {dt}", v.cpu().numpy().astype(np.float64), ref[:, 1], ab[:, 1], dt)


@pytest.mark.parametrize("d", [5, 40], ids=["lane", "panel"])
def test_no_columns_gives_beta_y(cg, d):
    k = cg.MaternP(2) + cg.Dot() ** 2 + cg.NeuralNetwork()
    for value, wrap in ((0, cg.GradientKernel), (1, cg.ValueGradientKernel)):
        for dt in (torch.float64, torch.float32):
            x = torch.randn(37, d, dtype=dt, device="cuda")
            G = cg.gramian(wrap(k), x, torch.zeros((0, d), dtype=dt, device="cuda"))
            assert type(G) is cg.MixedBlockGramian and G.shape == (37 * (d + value), 0)
            y0 = torch.randn(G.shape[0], dtype=dt, device="cuda")
            y = y0.clone()
            cg.mul_(y, G, torch.zeros(0, dtype=dt, device="cuda"), 3.0, -0.5)
            assert cg.get_info("last_grad_mixed_path") == 0
            assert torch.equal(y, -0.5 * y0)
            y = torch.full((G.shape[0],), float("nan"), dtype=dt, device="cuda")
            cg.mul_(y, G, torch.zeros(0, dtype=dt, device="cuda"), 3.0, 0.0)
            assert torch.equal(y, torch.zeros_like(y))


def test_zero_products_are_ordinary_numbers(cg):
    """EQ * Dot on points with x_i·y_j exactly 0: the reference throws DomainError there (src/gradient_algebra.jl:74-76)."""
    k, X, Y, A, ref, ab = inputs(cg, "eq*dot zero", 20, 24, 3, False, 0)
    assert np.count_nonzero(X @ Y.T == 0.0) >= 20
    G = operator(cg, k, X, Y, False, 0, torch.float64)
    b = G @ torch.tensor(A[:, 0], dtype=torch.float64, device="cuda")
    check("eq*dot with exact zeros", b.cpu().numpy(), ref[:, 0], ab[:, 0], torch.float64)


@pytest.mark.parametrize("value", [0, 1])
def test_dense_block_and_index(cg, value):
    name, n, m, d = "maternp2+dot^2+nn", 20, 20, 3
    k, X, Y, A, _, _ = inputs(cg, name, n, m, d, False, value)
    D = R.dense(cg, k, X, Y, bool(value))
    Dabs = np.abs(D).max()
    G = operator(cg, k, X, Y, False, value, torch.float64)
    M = G.to_dense().cpu().numpy()
    assert M.shape == D.shape and np.abs(M - D).max() <= 1e-12 * Dabs
    B = d + value
    blk = G.block(3, 7).cpu().numpy()
    assert blk.shape == (B, B) and np.abs(blk - D[3 * B:4 * B, 7 * B:8 * B]).max() <= 1e-12 * Dabs
    sub = G.block(slice(2, 5), slice(0, 4)).cpu().numpy()
    assert np.abs(sub - D[2 * B:5 * B, 0:4 * B]).max() <= 1e-12 * Dabs
    assert abs(float(G[3 * B + 1, 7 * B]) - D[3 * B + 1, 7 * B]) <= 1e-12 * Dabs


def test_cg_solves_g_plus_identity(cg):
    """One cg solve of G + I on a 40-point value-gradient case: the operator works through mul_ as any other."""
    name, n, d = "maternp2+dot^2+nn", 40, 3
    k, X, _, _, _, _ = inputs(cg, name, n, n, d, True, 1)
    D = R.dense(cg, k, X, X, True)
    G = operator(cg, k, X, X, True, 1, torch.float64)
    N = G.shape[0]
    rhs = np.random.default_rng(2).standard_normal(N)
    A = G + torch.ones(N, dtype=torch.float64, device="cuda")
    sol, info = cg.cg(A, torch.tensor(rhs, device="cuda"), reltol=1e-12, maxiter=4 * N)
    assert info["converged"], info
    sol = sol.cpu().numpy()
    ref = np.linalg.solve(D + np.eye(N), rhs)
    assert np.abs(sol - ref).max() <= 1e-8 * np.abs(ref).max(), np.abs(sol - ref).max()
