"""Every library-backed Python operator through the one staging path (covgram/gramian.py: _staged): the product on plain contiguous a
and y against the fp64 oracle, norm-wise and row-wise (tests/test_gpu_inplace.py: tol_of, oracle_errors), and then every other memory
layout of a and of y — column-major, and an every-second-element view of a larger tensor — bitwise equal to the contiguous result: the
layouts differ in the staging only, the library sees the same column-major numbers (the products use no atomics; test_gpu_inplace.py
relies on the same run-to-run bit equality).  (alpha, beta) = (1, 0) on a y prefilled with NaN and (0.7, -1.3); a vector and three
columns; one call without columns per operator, which must leave y alone.  Shapes: the smallest with more than one workgroup, odd, and
n != m where the operator allows it."""
import itertools

import numpy as np
import pytest
import torch

import hessian_ref as hr
import vgh_ref as vr
from test_gpu_inplace import oracle_errors, points, tol_of

pytestmark = pytest.mark.gpu

COEF = [(1.0, 0.0), (0.7, -1.3)]
LAYOUTS = ["c", "colmajor", "strided"]
SENTINEL = -7.0


# --------------------------------------------------------------------------------------------------------------------------------------
# the operators: name -> build(cg, o, dtype, rng) -> (operator, its dense fp64 matrix, gradient tolerance?)
# --------------------------------------------------------------------------------------------------------------------------------------
def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gramian(cg, o, dtype, rng):
    X, Y = points(rng, 257, 3, dtype), points(rng, 131, 3, dtype)
    return cg.gramian(cg.MaternP(2), _cuda(X), _cuda(Y)), o.matrix(o.Kernel(o.MATERNP, p=2), X.astype(np.float64), Y.astype(np.float64)), False


def _sm(cg, o, dtype, rng):
    X, Y = points(rng, 257, 3, dtype), points(rng, 131, 3, dtype)
    w, mu, l = [1.0, 0.6], [np.zeros(3), np.array([0.3, -0.2, 0.25])], [0.9, 1.3]
    G = cg.gramian(cg.SM(w, mu, l), _cuda(X), _cuda(Y))
    assert isinstance(G, cg.SpectralMixtureGramian)
    Xd, Yd = X.astype(np.float64), Y.astype(np.float64)
    M = sum(wq * o.cosine_matrix(mq, Xd, Yd) * o.matrix(o.Kernel(o.EQ, lengthscale=lq), Xd, Yd) for wq, mq, lq in zip(w, mu, l))
    return G, M, False


def _sparse(cg, o, dtype, rng):
    X, Y = points(rng, 257, 3, dtype), points(rng, 131, 3, dtype)
    S = cg.sparse(cg.gramian(cg.Lengthscale(cg.EQ(), 0.2), _cuda(X), _cuda(Y)))
    Xd, Yd = X.astype(np.float64), Y.astype(np.float64)
    s = ((Xd[:, None, :] - Yd[None, :, :]) ** 2).sum(-1)
    M = np.where(s <= S.radius ** 2, o.matrix(o.Kernel(o.EQ, lengthscale=0.2), Xd, Yd), 0.0)
    assert 0 < S.nnz < M.size and S.nnz == int((M != 0).sum())
    return S, M, False


def _block(kind):
    def build(cg, o, dtype, rng):
        X = points(rng, 33, 3, dtype)
        Xd = X.astype(np.float64)
        if kind == "grad":
            return cg.gramian(cg.GradientKernel(cg.EQ()), _cuda(X)), o.grad_matrix(o.Kernel(o.EQ), Xd), True
        if kind == "valgrad":
            return cg.gramian(cg.ValueGradientKernel(cg.EQ()), _cuda(X)), o.valgrad_matrix(o.Kernel(o.EQ), Xd), True
        if kind == "hess":
            return cg.gramian(cg.HessianKernel(cg.EQ()), _cuda(X)), hr.hess_matrix(("EQ", 0.0, 1.0, 1.0), Xd, Xd), True
        return cg.gramian(cg.ValueGradientHessianKernel(cg.EQ()), _cuda(X)), vr.vgh_matrix(("EQ", 0.0, 1.0, 1.0), Xd, Xd), True
    return build


def _toeplitz(kind):
    def build(cg, o, dtype, rng):
        n = 257
        npd = np.float32 if dtype == torch.float32 else np.float64
        xs = np.linspace(-1, 1, n)
        vc = np.exp(-np.abs(xs - xs[0]) / 0.3).astype(npd)
        vrow = (np.exp(-np.abs(xs - xs[0]) / 0.2) * 0.9).astype(npd); vrow[0] = vc[0]
        vcirc = np.exp(-np.minimum(np.arange(n), n - np.arange(n)) / (0.1 * n)).astype(npd)
        if kind == "sym":
            return cg.SymmetricToeplitz(_cuda(vc)), o.toeplitz_dense(vc.astype(np.float64)), False
        if kind == "gen":
            return cg.Toeplitz(_cuda(vc), _cuda(vrow)), o.toeplitz_dense(vc.astype(np.float64), vrow.astype(np.float64)), False
        return cg.Circulant(_cuda(vcirc)), o.toeplitz_dense(vcirc.astype(np.float64), circulant=True), False
    return build


def _kron(cg, o, dtype, rng):
    g1, g2 = points(rng, 12, 2, dtype), points(rng, 16, 2, dtype)
    Kp = cg.KroneckerProduct(cg.gramian(cg.EQ(), _cuda(g1)), cg.gramian(cg.MaternP(1), _cuda(g2)))
    return Kp, np.kron(o.matrix(o.Kernel(o.EQ), g1.astype(np.float64)), o.matrix(o.Kernel(o.MATERNP, p=1), g2.astype(np.float64))), False


def _lowrank(cg, o, dtype, rng):
    X = points(rng, 257, 3, dtype)
    c = np.array([0.4, -0.3, 0.2])
    L = cg.gramian(cg.Cosine(c), _cuda(X))
    assert isinstance(L, cg.LazyMatrixProduct) and L.U.shape == (257, 2)
    return L, o.cosine_matrix(c, X.astype(np.float64)), False


def _barneshut(product):
    def build(cg, o, dtype, rng):
        X = points(rng, 300, 2, dtype)
        F = cg.BarnesHutFactorization(cg.Cauchy(), _cuda(X), theta=0.0, product=product)        # theta = 0: the exact product
        return F, o.matrix(o.Kernel(o.CAUCHY), X.astype(np.float64)), False
    return build


OPERATORS = {"gramian": _gramian, "sm": _sm, "sparse": _sparse, "block_grad": _block("grad"), "block_valgrad": _block("valgrad"),
             "block_hess": _block("hess"), "block_vgh": _block("vgh"), "toeplitz_sym": _toeplitz("sym"), "toeplitz_gen": _toeplitz("gen"),
             "circulant": _toeplitz("circ"), "kron": _kron, "lowrank": _lowrank, "bh_split": _barneshut("split"), "bh_taylor": _barneshut("taylor")}


# --------------------------------------------------------------------------------------------------------------------------------------
# layouts
# --------------------------------------------------------------------------------------------------------------------------------------
def laid_out(t, layout):
    """(tensor with t's values in the given memory layout, the larger tensor it is a view of or None)."""
    if layout == "c":
        return t.clone(), None
    if layout == "colmajor":
        return (t.t().contiguous().t() if t.dim() == 2 else t.clone()), None
    big = torch.full(tuple(2 * s + 1 for s in t.shape), SENTINEL, dtype=t.dtype, device=t.device)
    view = big[tuple(slice(0, 2 * s, 2) for s in t.shape)]
    view.copy_(t)
    return view, big


def gaps_untouched(view, big):
    if big is None:
        return True
    rest = big.clone()
    rest[tuple(slice(0, 2 * s, 2) for s in view.shape)] = SENTINEL
    return bool((rest == SENTINEL).all())


def layout_pairs(p):
    """(layout of a, layout of y) beside the contiguous pair; a vector has no column-major form of its own."""
    ls = ["c", "strided"] if p is None else LAYOUTS
    return [pair for pair in itertools.product(ls, ls) if pair != ("c", "c")]


def inputs(op, dtype, rng, p, beta):
    n, m = op.shape
    npd = np.float32 if dtype == torch.float32 else np.float64
    a0 = rng.standard_normal((m,) if p is None else (m, p)).astype(npd)
    y0 = rng.standard_normal((n,) if p is None else (n, p)).astype(npd) if beta != 0 else np.full((n,) if p is None else (n, p), np.nan, dtype=npd)
    return a0, y0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(OPERATORS))
def test_layouts(cg, oracle, name, dtype):
    rng = np.random.default_rng(sorted(OPERATORS).index(name) + (100 if dtype == torch.float64 else 0))
    op, M, grad = OPERATORS[name](cg, oracle, dtype, rng)
    assert tuple(op.shape) == M.shape and op.dtype == dtype
    tol = tol_of(dtype, grad=grad)
    absM = np.abs(M)
    errs = []
    for p, (alpha, beta) in itertools.product((None, 3), COEF):
        a0, y0 = inputs(op, dtype, rng, p, beta)
        a, y = _cuda(a0), _cuda(y0)
        assert cg.mul_(y, op, a, alpha, beta) is y
        if name == "gramian" and dtype == torch.float32:
            assert cg.get_info("last_dense_path") == 2                    # the matrix-core route
        base = y.clone()
        what = f"{name} {'vector' if p is None else f'p={p}'} beta={beta}"
        A, Y0 = a0.astype(np.float64).reshape(M.shape[1], -1), (y0.astype(np.float64) if beta != 0 else np.zeros(y0.shape)).reshape(M.shape[0], -1)
        got = base.cpu().numpy().reshape(M.shape[0], -1)
        for c in range(A.shape[1]):
            ref = alpha * (M @ A[:, c]) + beta * Y0[:, c]
            scale = abs(alpha) * (absM @ np.abs(A[:, c])) + abs(beta) * np.abs(Y0[:, c])
            e = oracle_errors(f"{what} col {c}", got[:, c], ref, scale, tol)
            print(f"layouts {what} col {c}: row-wise {float(np.max(np.abs(got[:, c] - ref) / (scale + 1e-300))):.3e} (tol {tol:g})")
            errs += e
        for la, ly in layout_pairs(p):
            (av, abig), (yv, ybig) = laid_out(a, la), laid_out(_cuda(y0), ly)
            assert cg.mul_(yv, op, av, alpha, beta) is yv
            if not torch.equal(yv, base):
                errs.append(f"{what}: a {la}, y {ly} differs from the contiguous result, max |diff| {float((yv.double() - base.double()).abs().max()):.3e}")
            if not torch.equal(av, a):
                errs.append(f"{what}: a {la}, y {ly}: a was written")
            if not (gaps_untouched(av, abig) and gaps_untouched(yv, ybig)):
                errs.append(f"{what}: a {la}, y {ly}: memory between the elements of a view was written")
    # no columns: y is left alone (the C entries refuse nrhs = 0; the staging never calls them)
    keep = torch.full((op.shape[0], 3), 2.5, dtype=dtype, device="cuda")
    y_empty = keep[:, :0]
    assert cg.mul_(y_empty, op, torch.zeros((op.shape[1], 0), dtype=dtype, device="cuda"), 0.7, -1.3) is y_empty
    assert bool((keep == 2.5).all())
    assert (op @ torch.zeros((op.shape[1], 0), dtype=dtype, device="cuda")).shape == (op.shape[0], 0)
    assert not errs, "\n".join(errs)
