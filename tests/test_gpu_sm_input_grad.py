"""covgram_bilinear_input_grad_sm, spectral_mixture_input_gradient and spectral_mixture_product on the device against the fp64 reference
and the bound of tests/sm_input_grad_ref.py (run with -s for the worst err / bound of every case)."""
import ctypes as C

import numpy as np
import pytest
import torch

import matrix_cases as mc
import sm_input_grad_ref as ir
import sm_ref as sr

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
ONE = 1 + 4 * np.finfo(F64).eps     # sums of bounds and of references formed in fp64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def kernel_of(cg, w, mu, l):
    return cg.SM(w, [m for m in mu], [lq for lq in l])


def raw_status(cg, G, U, A, nvec=None, px=None, py=None, swap=False, null_out=False):
    """(status, dX, guard rows) of one covgram_bilinear_input_grad_sm call with G's handle on numpy weights: rows = G's row points
    against its column points (swap: the column points against the row points); px / py: point handles to pass in place of G's.  dX is
    allocated with a NaN row on either side."""
    f = cg._ffi
    dev = G.device
    U2 = U if U.ndim == 2 else U[:, None]; A2 = A if A.ndim == 2 else A[:, None]
    ut = torch.as_tensor(np.ascontiguousarray(U2.T)).to(dev); at = torch.as_tensor(np.ascontiguousarray(A2.T)).to(dev)
    nv = U2.shape[1] if nvec is None else nvec
    d = G.x.shape[1]
    out = torch.full((U2.shape[0] + 2, d), float("nan"), dtype=torch.float64, device=dev)
    G._px.ctx.bind_stream()
    rows, cols = (G._py, G._px) if swap else (G._px, G._py)
    hx = rows.handle if px is None else px
    hy = (None if cols is rows else cols.handle) if py is None else py
    st = f.lib().covgram_bilinear_input_grad_sm(G.handle, hx, hy, f._P(ut.data_ptr()), max(U2.shape[0], 1), f._P(at.data_ptr()), max(A2.shape[0], 1), nv,
                                                None if null_out else C.cast(out.data_ptr() + d * 8, C.POINTER(C.c_double)), f.DEVICE)
    res = out.cpu().numpy()
    return st, res[1:-1], res[[0, -1]]


def raw(cg, G, U, A, **kw):
    st, dX, guard = raw_status(cg, G, U, A, **kw)
    cg._ffi.check(st)
    assert np.all(np.isnan(guard)), "written outside the n d doubles"
    return dX


def check(tag, got, ref, bound):
    got = np.asarray(got)
    r, i = ir.worst(got, ref, bound)
    w = np.unravel_index(i, ref.shape)
    print(f"sm-input-grad {tag}: worst err/bound {r:.3f} at row {w[0]} dimension {w[1]} (ref {ref[w]:.6e}, got {got[w]:.6e})")
    assert r <= 1.0, (tag, w, got[w], ref[w], bound[w])
    return r


# ---- the raw entry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", ir.COMPONENTS)
@pytest.mark.parametrize("d", ir.DIMS)
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_main_sweep(cg, dev, dt, d, Q):
    """Every shape, both lengthscale forms and every column count at this (dtype, d, Q): X != Y, ragged tiles in both directions, one
    row, one column; one component chunk, a ragged last chunk and the maximum; far and copied rows (r = 0 exactly); NaN guard rows
    around dX."""
    top = 0.0
    for n, m in ir.SHAPES:
        for scalar_l in (True, False):
            X, Y, w, mu, l, inv_l = ir.make_case(n, m, d, Q, scalar_l, dt)
            G = cg.gramian(kernel_of(cg, w, mu, l), torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev))
            assert isinstance(G, cg.SpectralMixtureGramian) and G.isotropic() == (scalar_l or d == 1)
            ws = [ir.weights(n, m, nv, dt) for nv in ir.NVECS]
            for (U, A), (ref, bound) in zip(ws, ir.reference_and_bound(w, mu, inv_l, X, Y, ws, dt)):
                top = max(top, check(f"{n}x{m} d={d} Q={Q} {'iso' if scalar_l else 'ard'} nvec={U.shape[1]} {dt.__name__}", raw(cg, G, U, A), ref, bound))
    print(f"sm-input-grad sweep {dt.__name__} d={d} Q={Q}: worst err/bound {top:.3f}")


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_symmetric_call_and_its_diagonal(cg, dev, dt):
    """Y = NULL against a copy of X within the bound; with U and A supported on one index each that row (and every other) is exactly 0."""
    n, d, Q = 257, 3, 5
    rng = np.random.default_rng(3000)
    X = mc.iso_cloud(rng, n, n, d, dt)[0]
    w, mu, l = sr.params(rng, Q, d, False)
    inv_l = sr.inv_l_of(l, d)
    k = kernel_of(cg, w, mu, l)
    Xt = torch.from_numpy(X).to(dev)
    Gs = cg.gramian(k, Xt)
    Gc = cg.gramian(k, Xt, torch.from_numpy(X.copy()).to(dev))
    assert Gs._py is Gs._px and Gc._py is not Gc._px
    U, A = ir.weights(n, n, 3, dt)
    ref, bound = ir.reference_and_bound(w, mu, inv_l, X, X, [(U, A)], dt)[0]
    check(f"Y=NULL {dt.__name__}", raw(cg, Gs, U, A), ref, bound)
    check(f"Y=copy {dt.__name__}", raw(cg, Gc, U, A), ref, bound)
    for i in (0, 100, 256):
        e1 = np.zeros((n, 1), dt); e1[i] = dt(1.5)
        e2 = np.zeros((n, 1), dt); e2[i] = dt(-2.0)
        for G in (Gs, Gc):
            out = raw(cg, G, e1, e2)
            assert np.all(out == 0.0), (i, out[i])


def test_two_calls_agree_bitwise(cg, dev):
    """No atomics — on a shape with a column split, several hand-offs and two component chunks."""
    rng = np.random.default_rng(6000)
    n, m, d, Q = 70, 2100, 3, 5
    X = rng.standard_normal((n, d)).astype(F32); Y = rng.standard_normal((m, d)).astype(F32)
    w, mu, l = sr.params(rng, Q, d, False)
    G = cg.gramian(kernel_of(cg, w, mu, l), torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev))
    U, A = ir.weights(n, m, 17, F32)
    a, b = raw(cg, G, U, A), raw(cg, G, U, A)
    assert a.tobytes() == b.tobytes()
    ref, bound = ir.reference_and_bound(w, mu, sr.inv_l_of(l, d), X, Y, [(U, A)], F32)[0]
    check("bitwise shape 70x2100", a, ref, bound)


def test_empty_sides(cg, dev):
    """m == 0 gives zeros; n == 0 returns COVGRAM_OK and writes nothing."""
    f = cg._ffi
    w, mu, l = sr.params(np.random.default_rng(1), 3, 2, True)
    k = kernel_of(cg, w, mu, l)
    X = torch.zeros((5, 2), dtype=torch.float64, device=dev); E = torch.zeros((0, 2), dtype=torch.float64, device=dev)
    st, dX, guard = raw_status(cg, cg.gramian(k, X, E), np.ones((5, 2)), np.ones((0, 2)))
    assert st == f.OK and dX.shape == (5, 2) and np.all(dX == 0.0) and np.all(np.isnan(guard))
    st, dX, guard = raw_status(cg, cg.gramian(k, E, X), np.ones((0, 2)), np.ones((5, 2)))
    assert st == f.OK and dX.shape == (0, 2) and np.all(np.isnan(guard))


def test_status_codes(cg, dev):
    f = cg._ffi
    rng = np.random.default_rng(8000)
    X = rng.standard_normal((40, 3)); Y = rng.standard_normal((30, 3))
    w, mu, l = sr.params(rng, 2, 3, True)
    G = cg.gramian(kernel_of(cg, w, mu, l), torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev))
    U, A = ir.weights(40, 30, 2, F64)
    assert raw_status(cg, G, U, A, nvec=0)[0] == f.EINVAL
    U33, A33 = ir.weights(40, 30, 33, F64)
    st, dX, guard = raw_status(cg, G, U33, A33)
    assert st == f.EINVAL and np.all(np.isnan(dX)) and np.all(np.isnan(guard))
    assert b"nvec" in f.lib().covgram_last_error()
    assert raw_status(cg, G, U, A, null_out=True)[0] == f.EINVAL                                                 # dX is NULL
    G32 = cg.Gramian(cg.EQ(), torch.from_numpy(X.astype(F32)).to(dev), torch.from_numpy(Y.astype(F32)).to(dev))   # points of another dtype
    assert raw_status(cg, G, U, A, px=G32._px.handle, py=G32._py.handle)[0] == f.EINVAL
    G2 = cg.Gramian(cg.EQ(), torch.zeros((40, 2), dtype=torch.float64, device=dev))                              # points of another dimension
    assert raw_status(cg, G, U, U, px=G2._px.handle, py=G2._px.handle)[0] == f.EINVAL
    st, dX, guard = raw_status(cg, G, U, A)
    assert st == f.OK and np.all(np.isfinite(dX)) and np.all(np.isnan(guard))


# ---- spectral_mixture_input_gradient -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_input_gradient_both_sides_chunks_and_equal_weights(cg, dev, dt):
    """Two point sets with 33 columns (chunks of 32 summed in fp64, the chunks' bounds added): dX, and dY against the reference with the
    roles swapped; one point set: dY is None and the reference is the sum of the two calls; U and A one tensor: bit-equal to the
    two-call route."""
    n, m, d, Q = 257, 130, 3, 3
    X, Y, w, mu, l, inv_l = ir.make_case(n, m, d, Q, False, dt)
    k = kernel_of(cg, w, mu, l)
    G = cg.gramian(k, torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev))
    U, A = ir.weights(n, m, 33, dt)
    dX, dY = cg.spectral_mixture_input_gradient(G, torch.from_numpy(U), torch.from_numpy(A))
    assert dX.shape == (n, d) and dY.shape == (m, d) and dX.dtype == dY.dtype == torch.float64 and dX.is_cuda and dY.is_cuda
    for name, got, (P, R, V, B) in (("dX", dX, (X, Y, U, A)), ("dY", dY, (Y, X, A, U))):
        (r1, b1), (r2, b2) = ir.reference_and_bound(w, mu, inv_l, P, R, [(V[:, :32], B[:, :32]), (V[:, 32:], B[:, 32:])], dt)
        check(f"spectral_mixture_input_gradient nvec=33 {name} {dt.__name__}", got.cpu().numpy(), r1 + r2, (b1 + b2) * ONE)
    assert np.array_equal(dX.cpu().numpy(), raw(cg, G, U[:, :32], A[:, :32]) + raw(cg, G, U[:, 32:], A[:, 32:]))
    assert np.array_equal(dY.cpu().numpy(), raw(cg, G, A[:, :32], U[:, :32], swap=True) + raw(cg, G, A[:, 32:], U[:, 32:], swap=True))
    Gs = cg.gramian(k, torch.from_numpy(X).to(dev))
    V = ir.weights(n, n, 5, dt)[1]
    one, none = cg.spectral_mixture_input_gradient(Gs, torch.from_numpy(U[:, :5]), torch.from_numpy(V))
    assert none is None and one.shape == (n, d)
    (r1, b1), (r2, b2) = ir.reference_and_bound(w, mu, inv_l, X, X, [(U[:, :5], V), (V, U[:, :5])], dt)
    check(f"spectral_mixture_input_gradient one point set {dt.__name__}", one.cpu().numpy(), r1 + r2, (b1 + b2) * ONE)
    Ut = torch.from_numpy(U[:, :5]).to(dev)
    single, none = cg.spectral_mixture_input_gradient(Gs, Ut, Ut)
    double = cg.spectral_mixture_input_gradient(Gs, Ut, Ut.clone())[0]
    assert none is None and torch.equal(single, double)
    ra, ba = ir.reference_and_bound(w, mu, inv_l, X, X, [(U[:, :5], U[:, :5])], dt)[0]
    check(f"spectral_mixture_input_gradient U is A {dt.__name__}", single.cpu().numpy(), 2 * ra, 2 * ba * ONE)


# ---- spectral_mixture_product --------------------------------------------------------------------------------------------------------
def product_problem(cg, n, m, d, Q, p, dt, seed):
    rng = np.random.default_rng(seed)
    X, Y = mc.iso_cloud(rng, n, m, d, dt)[:2]
    w, mu, l = sr.params(rng, Q, d, False)
    k = kernel_of(cg, w, mu, l)
    theta = [v for _, _, v in cg.hyperparameters(k)]
    return X, Y, k, theta, rng.standard_normal((m, p)).astype(dt), rng.standard_normal((n, p)).astype(dt)


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_spectral_mixture_product_autograd(cg, dev, dt):
    """x, y, a and theta all requiring a gradient: the output is G @ a and every gradient is the library's own pass, bit for bit (after
    the cast to the input's dtype); x.grad is within the bound of the fp64 reference; then y = None."""
    n, m, d, Q, p = 70, 45, 3, 3, 2
    X, Y, k, th, An, gn = product_problem(cg, n, m, d, Q, p, dt, 10000)
    w, mu, inv_l = cg.spectral_mixture_spec(k, d)
    for sym in (False, True):
        x = torch.as_tensor(X).to(dev).requires_grad_()
        y = None if sym else torch.as_tensor(Y).to(dev).requires_grad_()
        a = torch.as_tensor(gn if sym else An).to(dev).requires_grad_()
        theta = torch.tensor(th, dtype=torch.float64, requires_grad=True)
        gbar = torch.as_tensor(gn[::-1].copy()).to(dev)
        out = cg.spectral_mixture_product(k, x, a, y=y, theta=theta)
        G = cg.gramian(k, x.detach(), None if sym else y.detach())
        assert isinstance(G, cg.SpectralMixtureGramian)
        assert out.shape == (n, p) and torch.equal(out.detach(), G @ a.detach())
        out.backward(gbar)
        assert torch.equal(a.grad, (G if sym else G.T) @ gbar)
        assert theta.grad.shape == (len(th),) and torch.equal(theta.grad, cg.spectral_mixture_gradient(G, gbar, a.detach())[1])
        dX, dY = cg.spectral_mixture_input_gradient(G, gbar, a.detach())
        assert x.grad.dtype == x.dtype and torch.equal(x.grad, dX.to(x.dtype))
        if sym:
            assert dY is None
            (r1, b1), (r2, b2) = ir.reference_and_bound(w, mu, inv_l, X, X, [(gn[::-1], gn), (gn, gn[::-1])], dt)
            ref, bound = r1 + r2, (b1 + b2) * ONE
        else:
            assert y.grad.dtype == y.dtype and torch.equal(y.grad, dY.to(y.dtype))
            ref, bound = ir.reference_and_bound(w, mu, inv_l, X, Y, [(gn[::-1], An)], dt)[0]
        check(f"spectral_mixture_product x.grad sym={sym} {dt.__name__}", x.grad.double().cpu().numpy(), ref, bound)


def test_spectral_mixture_product_gradcheck(cg, dev):
    """torch.autograd.gradcheck with its default settings in fp64, x, y, a and theta together, then one point set."""
    n, m, d, Q, p = 12, 9, 2, 2, 2
    X, Y, k, th, An, gn = product_problem(cg, n, m, d, Q, p, F64, 11000)
    x = torch.as_tensor(X).to(dev).requires_grad_()
    y = torch.as_tensor(Y).to(dev).requires_grad_()
    theta = torch.tensor(th, dtype=torch.float64, requires_grad=True)
    a = torch.as_tensor(An).to(dev).requires_grad_()
    assert torch.autograd.gradcheck(lambda x_, a_, y_, t_: cg.spectral_mixture_product(k, x_, a_, y=y_, theta=t_), (x, a, y, theta))
    a1 = torch.as_tensor(gn).to(dev).requires_grad_()
    assert torch.autograd.gradcheck(lambda x_, a_, t_: cg.spectral_mixture_product(k, x_, a_, theta=t_), (x, a1, theta))
