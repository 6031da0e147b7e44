"""covgram_bilinear_input_grad, bilinear_input_gradient and gram_product on the device against the fp64 reference and the derived bound
of tests/input_grad_ref.py (run with -s for the worst err / bound of every case)."""
import ctypes as C

import numpy as np
import pytest
import torch

import covgram_oracle as o
import input_grad_ref as ir
import matrix_cases as mc
from test_gpu_bilin_grad import FAMILIES, M, N, spec_of, weights

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TDT = {F32: torch.float32, F64: torch.float64}


def raw_status(cg, spec, X, Y, U, A, nvec=None, kptr=None, loc="device"):
    """(status, dX, guard rows) of one covgram_bilinear_input_grad call on numpy inputs (Y None = the symmetric call).  The output buffer
    has one NaN-filled row in front of and behind the n d doubles; `guard` is those two rows after the call."""
    from covgram.gramian import _Points
    f = cg._ffi
    dev = cg.get_ctx().device
    n, d = X.shape
    px = _Points(torch.as_tensor(X).to(dev).contiguous())
    py = None if Y is None else _Points(torch.as_tensor(Y).to(dev).contiguous())
    cols = U.shape[1] if U.ndim > 1 else 1
    U2 = np.ascontiguousarray(U.reshape(U.shape[0], cols).T); A2 = np.ascontiguousarray(A.reshape(A.shape[0], cols).T)
    nv = U2.shape[0] if nvec is None else nvec
    if loc == "device":
        ut, at = torch.as_tensor(U2).to(dev), torch.as_tensor(A2).to(dev)
        out = torch.full((n + 2, d), float("nan"), dtype=torch.float64, device=dev)
        where = f.DEVICE
    else:
        ut, at = torch.as_tensor(U2), torch.as_tensor(A2)
        out = torch.full((n + 2, d), float("nan"), dtype=torch.float64)
        where = f.HOST
    st = f.lib().covgram_bilinear_input_grad(px.ctx.bind_stream(), kptr if kptr is not None else f.kref(spec), px.handle,
                                             py.handle if py is not None else None, f._P(ut.data_ptr()), n, f._P(at.data_ptr()), A2.shape[1], nv,
                                             C.cast(out.data_ptr() + d * 8, C.POINTER(C.c_double)), where)
    res = out.cpu().numpy()
    return st, res[1:-1], res[[0, -1]]


def raw(cg, ko, X, Y, U, A, loc="device"):
    st, dX, guard = raw_status(cg, spec_of(cg, ko), X, Y, U, A, loc=loc)
    cg._ffi.check(st)
    assert np.all(np.isnan(guard)), "written outside the n d doubles"
    return dX


def check(tag, got, ref, bound):
    with np.errstate(invalid="ignore"):
        r = np.where(np.isfinite(got), np.abs(got - ref) / bound, np.inf)
    w = np.unravel_index(int(np.argmax(r)), r.shape)
    print(f"input-grad {tag}: worst err/bound {r[w]:.3f} at row {w[0]} dimension {w[1]} (ref {ref[w]:.6e}, got {got[w]:.6e})")
    assert r[w] <= 1.0, (tag, w, got[w], ref[w], bound[w])
    return float(r[w])


@pytest.mark.parametrize("d", [1, 3, 8])
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_every_family_against_the_reference(cg, dt, d):
    """(a): every supported family, nvec in {1, 3, 17}, X != Y with far and copied rows, ragged tiles in both directions; dX from the
    call, dY from the call with the roles swapped."""
    for name, ko in FAMILIES:
        rng = np.random.default_rng(1000 + d)
        X, Y, far, cop = mc.iso_cloud(rng, N, M, d, dt, lscale=ko.lengthscale)
        assert len(far) == 8 and len(cop) == 4
        for nvec in (1, 3, 17):
            U, A = weights(rng, N, M, nvec, dt)
            ref, bound = ir.reference_and_bound(o, ko, X, Y, U, A, dt)
            check(f"{name} d={d} nvec={nvec} dX {dt.__name__}", raw(cg, ko, X, Y, U, A), ref, bound)
            ref, bound = ir.reference_and_bound(o, ko, Y, X, A, U, dt)
            check(f"{name} d={d} nvec={nvec} dY {dt.__name__}", raw(cg, ko, Y, X, A, U), ref, bound)


@pytest.mark.parametrize("d", [33, 64])
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_wide_points(cg, dt, d):
    """(b): dimension groups and LDS slabs (d > 16), on the shrunken cloud of tests/test_gpu_bilin_grad.py's wide test; nvec = 5 and, for
    the narrower dimension groups of fp64 with many columns, nvec = 29."""
    for name, ko in (FAMILIES[0], FAMILIES[6]):
        rng = np.random.default_rng(2000 + d)
        X, Y = mc.iso_cloud(rng, N, M, d, dt, lscale=ko.lengthscale, spread=0.8 * np.sqrt(8.0 / d), shift=0.2 * np.sqrt(8.0 / d))[:2]
        for nvec in (5, 29):
            U, A = weights(rng, N, M, nvec, dt)
            ref, bound = ir.reference_and_bound(o, ko, X, Y, U, A, dt)
            check(f"{name} d={d} nvec={nvec} {dt.__name__}", raw(cg, ko, X, Y, U, A), ref, bound)


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_column_split_and_handoffs_bitwise(cg, dt):
    """(c): n = 70, m = 1100 — a column split and several hand-offs per lane; no atomics: two calls agree bit for bit."""
    rng = np.random.default_rng(6000)
    name, ko = FAMILIES[6]
    X, Y = mc.iso_cloud(rng, 70, 1100, 3, dt, lscale=ko.lengthscale)[:2]
    U, A = weights(rng, 70, 1100, 17, dt)
    a, b = raw(cg, ko, X, Y, U, A), raw(cg, ko, X, Y, U, A)
    assert a.tobytes() == b.tobytes()
    ref, bound = ir.reference_and_bound(o, ko, X, Y, U, A, dt)
    check(f"{name} 70x1100 {dt.__name__}", a, ref, bound)


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_symmetric_call_and_its_diagonal(cg, dt):
    """(d): Y = NULL against a copy of X, within the bound; with U and A supported on one index each that row's result is exactly 0 (and
    every other row's), also for the profiles whose derivative is unbounded at 0."""
    d = 3
    for name, ko in (FAMILIES[0], FAMILIES[1], FAMILIES[3], FAMILIES[7], FAMILIES[6]):
        rng = np.random.default_rng(3000)
        X = mc.iso_cloud(rng, N, N, d, dt, lscale=ko.lengthscale)[0]
        U, A = weights(rng, N, N, 3, dt)
        ref, bound = ir.reference_and_bound(o, ko, X, X, U, A, dt)
        check(f"{name} Y=NULL {dt.__name__}", raw(cg, ko, X, None, U, A), ref, bound)
        check(f"{name} Y=copy {dt.__name__}", raw(cg, ko, X, X.copy(), U, A), ref, bound)
        for i in (0, 100, 256):
            e1 = np.zeros((N, 1), dt); e1[i] = dt(1.5)
            e2 = np.zeros((N, 1), dt); e2[i] = dt(-2.0)
            out = raw(cg, ko, X, None, e1, e2)
            assert np.all(out == 0.0), (name, i, out[i])


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_column_limit_chunking_and_equal_weights(cg, dt):
    """(e): nvec = 32 through the raw entry, 33 through bilinear_input_gradient (chunks of 32 summed in fp64); with U and A one tensor the
    single doubled call equals the two-call route bit for bit."""
    d = 3
    name, ko = FAMILIES[6]
    rng = np.random.default_rng(4000)
    X, Y = mc.iso_cloud(rng, N, M, d, dt, lscale=ko.lengthscale)[:2]
    U, A = weights(rng, N, M, 33, dt)
    ref, bound = ir.reference_and_bound(o, ko, X, Y, U[:, :32], A[:, :32], dt)
    check(f"{name} nvec=32 {dt.__name__}", raw(cg, ko, X, Y, U[:, :32], A[:, :32]), ref, bound)
    k = 2.5 * cg.Lengthscale(cg.MaternP(2), 1.3)
    G = cg.gramian(k, torch.as_tensor(X).cuda(), torch.as_tensor(Y).cuda())
    dX, dY = cg.bilinear_input_gradient(G, torch.as_tensor(U), torch.as_tensor(A))
    assert dX.shape == (N, d) and dY.shape == (M, d) and dX.dtype == torch.float64 and dX.is_cuda
    one = 1 + 4 * np.finfo(F64).eps
    for got, (P, Q, V, B) in ((dX, (X, Y, U, A)), (dY, (Y, X, A, U))):
        r1, b1 = ir.reference_and_bound(o, ko, P, Q, V[:, :32], B[:, :32], dt)
        r2, b2 = ir.reference_and_bound(o, ko, P, Q, V[:, 32:], B[:, 32:], dt)
        check(f"{name} nvec=33 bilinear_input_gradient {dt.__name__}", got.cpu().numpy(), r1 + r2, (b1 + b2) * one)
    Gs = cg.gramian(k, torch.as_tensor(X).cuda())
    Ut = torch.as_tensor(U[:, :5]).cuda()
    single, none = cg.bilinear_input_gradient(Gs, Ut, Ut)
    double = cg.bilinear_input_gradient(Gs, Ut, Ut.clone())[0]
    assert none is None and torch.equal(single, double)
    ra, ba = ir.reference_and_bound(o, ko, X, X, U[:, :5], U[:, :5], dt)
    check(f"{name} symmetric U is A {dt.__name__}", single.cpu().numpy(), 2 * ra, 2 * ba * one)


def test_guarding_locations_and_status_codes(cg):
    """(f): nothing outside the n d doubles is written (raw() asserts the NaN rows around them in every test of this file); host memory
    gives the bits device memory gives; m = 0 gives zeros, n = 0 writes nothing; the status codes of the refusals."""
    f = cg._ffi
    rng = np.random.default_rng(8000)
    name, ko = FAMILIES[2]
    for dt in (F32, F64):
        X, Y = mc.iso_cloud(rng, 70, 45, 5, dt)[:2]
        U, A = weights(rng, 70, 45, 3, dt)
        assert raw(cg, ko, X, Y, U, A, loc="host").tobytes() == raw(cg, ko, X, Y, U, A, loc="device").tobytes()
        for loc in ("host", "device"):
            st, dX, guard = raw_status(cg, spec_of(cg, ko), X, Y[:0], U, A[:0], loc=loc)
            assert st == f.OK and np.all(dX == 0.0) and np.all(np.isnan(guard))
            st, dX, guard = raw_status(cg, spec_of(cg, ko), X[:0], Y, U[:0], A, loc=loc)
            assert st == f.OK and dX.shape == (0, 5) and np.all(np.isnan(guard))
    X = rng.standard_normal((40, 3)); Y = rng.standard_normal((30, 3))
    U, A = weights(rng, 40, 30, 2, F64)
    comp = cg.device_spec(cg.EQ() * cg.Lengthscale(cg.Cauchy(), 1.5))
    assert isinstance(comp, f.covgram_kernel_composite)
    assert raw_status(cg, None, X, Y, U, A, kptr=f.kref(comp))[0] == f.EUNSUPPORTED
    for bad in (o.Kernel(o.DOT), o.Kernel(o.MATERN, param=0.8)):
        st, dX, guard = raw_status(cg, spec_of(cg, bad), X, Y, U, A)
        assert st == f.EUNSUPPORTED and np.all(np.isnan(dX)) and np.all(np.isnan(guard))
    with pytest.raises(cg.UnsupportedKernel):
        f.check(raw_status(cg, spec_of(cg, o.Kernel(o.MATERN, param=0.8)), X, Y, U, A)[0])
    U33, A33 = weights(rng, 40, 30, 33, F64)
    assert raw_status(cg, spec_of(cg, o.Kernel(o.EQ)), X, Y, U33, A33)[0] == f.EINVAL
    assert raw_status(cg, spec_of(cg, o.Kernel(o.EQ)), X, Y, U, A, nvec=0)[0] == f.EINVAL
    X65 = rng.standard_normal((40, 65)); Y65 = rng.standard_normal((30, 65))
    assert raw_status(cg, spec_of(cg, o.Kernel(o.EQ)), X65, Y65, U, A)[0] == f.EINVAL
    assert raw_status(cg, spec_of(cg, o.Kernel(o.EQ)), X, rng.standard_normal((30, 4)), U, A)[0] == f.EINVAL     # d mismatch
    assert raw_status(cg, spec_of(cg, o.Kernel(o.EQ)), X, Y.astype(F32), U, A)[0] == f.EINVAL                    # dtype mismatch
    st, dX, guard = raw_status(cg, spec_of(cg, o.Kernel(o.EQ)), X, Y, U, A)
    assert st == f.OK and np.all(np.isfinite(dX)) and np.all(np.isnan(guard))


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_chain_rules_on_the_device(cg, dt):
    """(g): ARD (the Gramian holds x / l: the result is with respect to the points passed) and a Sum with a Constant term, against the
    reference with the chain rule and the summed bounds."""
    d = 3
    rng = np.random.default_rng(9000)
    X, Y = mc.iso_cloud(rng, N, M, d, dt)[:2]
    U, A = weights(rng, N, M, 3, dt)
    tx, ty = torch.as_tensor(X).cuda(), torch.as_tensor(Y).cuda()
    one = 1 + 4 * np.finfo(F64).eps
    l = np.array([0.7, 1.1, 1.9])
    G = cg.gramian(cg.ARD(cg.EQ(), l), tx, ty)
    dX, dY = cg.bilinear_input_gradient(G, torch.as_tensor(U), torch.as_tensor(A))
    Xh, Yh = G.x.cpu().numpy(), G.y.cpu().numpy()                  # the points the device sees, as the library rounded them
    for got, (P, Q, V, B) in ((dX, (Xh, Yh, U, A)), (dY, (Yh, Xh, A, U))):
        ref, bound = ir.reference_and_bound(o, o.Kernel(o.EQ), P, Q, V, B, dt)
        check(f"ARD(EQ) {dt.__name__}", got.cpu().numpy(), ref / l, bound / l * one)
    k = 1.5 * cg.Lengthscale(cg.EQ(), 0.7) + cg.Constant(0.25) + 0.5 * cg.RQ(0.37)
    terms = (o.Kernel(o.EQ, lengthscale=0.7, scale=1.5), o.Kernel(o.RQ, param=0.37, scale=0.5))
    dX, dY = cg.bilinear_input_gradient(cg.gramian(k, tx, ty), torch.as_tensor(U), torch.as_tensor(A))
    for got, (P, Q, V, B) in ((dX, (X, Y, U, A)), (dY, (Y, X, A, U))):
        parts = [ir.reference_and_bound(o, ko, P, Q, V, B, dt) for ko in terms]
        check(f"Sum with a Constant {dt.__name__}", got.cpu().numpy(), parts[0][0] + parts[1][0], (parts[0][1] + parts[1][1]) * one)


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_gram_product_autograd(cg, dt):
    """(h): gram_product with x, y, a and theta all requiring a gradient: every gradient is the library's own fused pass, bit for bit, and
    x.grad is within the bound of the fp64 reference; then y = None; last, only `a` through a Toeplitz Gramian."""
    n, m, d, p = 70, 45, 3, 2
    rng = np.random.default_rng(10000)
    X, Y = mc.iso_cloud(rng, n, m, d, dt, lscale=1.3)[:2]
    k = 2.5 * cg.Lengthscale(cg.MaternP(2), 1.3)
    ko = o.Kernel(o.MATERNP, p=2, lengthscale=1.3, scale=2.5)
    assert [nm for _, nm, _ in cg.hyperparameters(k)] == ["scale", "l"]
    An, gn = rng.standard_normal((m, p)).astype(dt), rng.standard_normal((n, p)).astype(dt)
    for sym in (False, True):
        x = torch.as_tensor(X).cuda().requires_grad_()
        y = None if sym else torch.as_tensor(Y).cuda().requires_grad_()
        a = torch.as_tensor(gn if sym else An).cuda().requires_grad_()
        theta = torch.tensor([2.5, 1.3], dtype=torch.float64, requires_grad=True)
        gbar = torch.as_tensor(gn[::-1].copy()).cuda()
        out = cg.gram_product(k, x, a, y=y, theta=theta)
        G = cg.gramian(k, x.detach(), None if sym else y.detach())
        assert out.shape == (n, p) and torch.equal(out.detach(), G @ a.detach())
        out.backward(gbar)
        assert torch.equal(a.grad, (G if sym else G.T) @ gbar)
        assert torch.equal(theta.grad, cg.bilinear_gradient(G, gbar, a.detach())[1])
        dX, dY = cg.bilinear_input_gradient(G, gbar, a.detach())
        assert x.grad.dtype == x.dtype and torch.equal(x.grad, dX.to(x.dtype))
        if sym:
            assert dY is None
            r1, b1 = ir.reference_and_bound(o, ko, X, X, gn[::-1], gn, dt)
            r2, b2 = ir.reference_and_bound(o, ko, X, X, gn, gn[::-1], dt)
            ref, bound = r1 + r2, (b1 + b2) * (1 + 4 * np.finfo(F64).eps)
        else:
            assert torch.equal(y.grad, dY.to(y.dtype))
            ref, bound = ir.reference_and_bound(o, ko, X, Y, gn[::-1], An, dt)
        check(f"gram_product x.grad sym={sym} {dt.__name__}", x.grad.double().cpu().numpy(), ref, bound)
    # only `a`: every operator with .T
    nt = 300
    at = torch.as_tensor(rng.standard_normal(nt)).cuda().requires_grad_()
    gt = torch.as_tensor(rng.standard_normal(nt)).cuda()
    T = cg.gramian(cg.Exp(), cg.srange(-1, 1, nt))
    assert type(T).__name__ == "SymmetricToeplitz"
    cg.gram_product(cg.Exp(), cg.srange(-1, 1, nt), at).backward(gt)
    assert torch.equal(at.grad, T @ gt)
    at.grad = None
    cg.gram_product(T, None, at).backward(gt)
    assert torch.equal(at.grad, T.T @ gt)
    # the transposes this relies on
    R = cg.gramian(cg.Exp(), cg.srange(-1, 1, 40), cg.srange(-0.5, 1.5, 40))
    assert type(R).__name__ == "Toeplitz" and torch.equal(R.T.to_dense(), R.to_dense().t()) and not torch.equal(R.to_dense(), R.to_dense().t())
    Cc = cg.Circulant(torch.as_tensor(rng.standard_normal(7)).cuda())
    assert torch.equal(Cc.T.to_dense(), Cc.to_dense().t())
