"""covgram_bilinear_grad_mixed, mixed_bilinear_gradient and inv_quad_logdet_gradient of a MixedGramian on the device, entry by entry against
the fp64 reference and the derived bound of tests/mixed_grad_ref.py (run with -s for the worst err / bound of every case)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mixed_grad_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TDT = {F32: torch.float32, F64: torch.float64}
NAMES = ["1.5ls(eq,.7)+.5dot", "ls(eq,.8)*(dot^2+1)", ".7ls(maternp2,1.3)+.2poly(3,.4)", "ls(rq(.37),1.2)*nn(.5)+.3imq(.6)", "nn(.3)+.1expdot",
         "ls(exp,.9)*dot", "gammaexp(1.5)*dot+1", "ls(eq,.7)*ls(rq(.5),1.4)"]


def raw_status(cg, comp, X, Y, U, A, dt, nvec=None, loc=None, null_out=False):
    """(status, out) of one covgram_bilinear_grad_mixed call on numpy inputs (Y None = the symmetric call); out starts as NaN."""
    from covgram.gramian import _Points
    f = cg._ffi
    loc = f.DEVICE if loc is None else loc
    dev = cg.get_ctx().device
    px = _Points(torch.as_tensor(np.array(X, dtype=dt)).to(dev))
    py = None if Y is None else _Points(torch.as_tensor(np.array(Y, dtype=dt)).to(dev))
    m = X.shape[0] if Y is None else Y.shape[0]
    cols = np.shape(U)[1] if np.ndim(U) > 1 else 1
    U2 = np.array(np.asarray(U, dtype=dt).reshape(X.shape[0], cols).T, order="C"); A2 = np.array(np.asarray(A, dtype=dt).reshape(m, cols).T, order="C")
    nv = U2.shape[0] if nvec is None else nvec
    ctx = px.ctx.bind_stream()
    hy = py.handle if py is not None else None
    if loc == f.HOST:
        out = np.full(24, np.nan)
        st = f.lib().covgram_bilinear_grad_mixed(ctx, C.byref(comp), px.handle, hy, f._P(U2.ctypes.data), max(X.shape[0], 1), f._P(A2.ctypes.data), max(m, 1), nv,
                                                 None if null_out else out.ctypes.data_as(C.POINTER(C.c_double)), loc)
        return st, out
    ut = torch.as_tensor(U2).to(dev); at = torch.as_tensor(A2).to(dev)
    out = torch.full((24,), float("nan"), dtype=torch.float64, device=dev)
    st = f.lib().covgram_bilinear_grad_mixed(ctx, C.byref(comp), px.handle, hy, f._P(ut.data_ptr()), max(X.shape[0], 1), f._P(at.data_ptr()), max(m, 1), nv,
                                             None if null_out else C.cast(out.data_ptr(), C.POINTER(C.c_double)), loc)
    return st, out.cpu().numpy()


def raw(cg, comp, X, Y, U, A, dt, **kw):
    st, out = raw_status(cg, comp, X, Y, U, A, dt, **kw)
    cg._ffi.check(st)
    return out


@functools.lru_cache(maxsize=None)
def case(name, shape_index, nvec):
    """(comp, X, Y, U, A, ref, {dtype: bound}): computed once, shared by the tests, never modified."""
    import covgram as cg
    import covgram_oracle as oracle
    n, m, d, same, _ = R.SHAPES[shape_index]
    comp, _ = cg.require_mixed_parameter_spec({**R.kernels(cg), **R.extra_kernels(cg)}[name])
    X, Y = R.clouds(name, n, m, d, same)
    U, A = R.weights_for(n, m, nvec)
    ref, b32 = R.reference_and_bound(cg, oracle, comp, X, Y, U, A, F32)
    _, b64 = R.reference_and_bound(cg, oracle, comp, X, Y, U, A, F64)
    for a in (X, Y, U, A, ref, b32, b64):
        a.setflags(write=False)
    return comp, X, Y, U, A, ref, {F32: b32, F64: b64}


def check(tag, got, ref, bound):
    live = bound > 0
    assert np.all(got[~live] == 0.0), (tag, "dead outputs are not exact zeros", got)
    with np.errstate(invalid="ignore"):
        r = np.where(np.isfinite(got[live]), np.abs(got - ref)[live] / bound[live], np.inf)
    w = int(np.argmax(r)); k = int(np.nonzero(live)[0][w])
    print(f"mixed-grad {tag}: worst err/bound {r[w]:.3f} at out[{k}] (ref {ref[k]:.6e}, got {got[k]:.6e})")
    assert r[w] <= 1.0, (tag, k, got[k], ref[k], bound[k])
    return float(r[w])


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", NAMES)
def test_every_kernel_and_shape_against_the_reference(cg, name, dt):
    """Entry by entry, every shape of the table: the row-tile edge and the diagonal's zero distances (Y = NULL), the hand-off and the
    column split (and option jsplit = 3), two LDS slabs, d = 64, 1 x 1; Y[0] = X[3] planted wherever the sets differ."""
    assert list(R.kernels(cg)) == NAMES
    for si, (n, m, d, same, opts) in enumerate(R.SHAPES):
        comp, X, Y, U, A, ref, bound = case(name, si, 3)
        for key, v in opts.items():
            cg.set_option(key, v)
        try:
            got = raw(cg, comp, X, None if same else Y, U, A, dt)
        finally:
            for key in opts:
                cg.set_option(key, 0)
        check(f"{name} {n}x{m} d={d} {opts} {dt.__name__}", got, ref, bound[dt])


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_one_and_thirty_two_columns(cg, dt):
    """nvec = 1 and 32 (fp64 at 32: the live outputs no longer fit one pass beside the tiles and are walked in chunks)."""
    for name in (NAMES[1], NAMES[3], "6 ls(rq)"):
        for nvec in (1, 32):
            comp, X, Y, U, A, ref, bound = case(name, 3, nvec)
            check(f"{name} nvec={nvec} {dt.__name__}", raw(cg, comp, X, Y, U, A, dt), ref, bound[dt])


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_host_weights_bitwise_and_symmetric_copy(cg, dt):
    f = cg._ffi
    comp, X, Y, U, A, ref, bound = case(NAMES[3], 1, 3)
    dev1 = raw(cg, comp, X, Y, U, A, dt)
    dev2 = raw(cg, comp, X, Y, U, A, dt)
    assert np.array_equal(dev1, dev2), "two calls with the same arguments differ"
    host = raw(cg, comp, X, Y, U, A, dt, loc=f.HOST)
    assert np.array_equal(host, dev1), "loc = HOST differs from loc = DEVICE"
    comp, X, _, U, A, ref, bound = case(NAMES[5], 0, 3)                         # Exponential * Dot on one point set: the whole diagonal has z = 0
    sym = raw(cg, comp, X, None, U, A, dt)
    cpy = raw(cg, comp, X, X.copy(), U, A, dt)
    assert np.array_equal(sym, cpy) and np.all(np.isfinite(sym))


def test_empty_sums_and_status_codes(cg):
    f = cg._ffi
    comp, X, Y, U, A, _, _ = case(NAMES[0], 3, 3)
    for loc in (f.DEVICE, f.HOST):
        for Xs, Ys, Us, As in ((X, Y[:0], U, A[:0]), (X[:0], Y, U[:0], A)):
            st, out = raw_status(cg, comp, Xs, Ys, Us, As, F64, nvec=3, loc=loc)
            assert st == f.OK and np.all(out == 0.0), (loc, out)
    assert raw_status(cg, comp, X, Y, U, A, F64, nvec=0)[0] == f.EINVAL
    U33, A33 = R.weights_for(X.shape[0], Y.shape[0], 33)
    assert raw_status(cg, comp, X, Y, U33, A33, F64)[0] == f.EINVAL
    rng = np.random.default_rng(1)
    X65, Y65 = 0.1 * rng.standard_normal((X.shape[0], 65)), 0.1 * rng.standard_normal((Y.shape[0], 65))
    assert raw_status(cg, comp, X65, Y65, U, A, F64)[0] == f.EINVAL
    assert raw_status(cg, comp, X, Y, U, A, F64, null_out=True)[0] == f.EINVAL
    matern = cg.mixed_spec(cg.Matern(2.3) + cg.Dot())
    assert raw_status(cg, matern, X, Y, U, A, F64)[0] == f.EUNSUPPORTED
    assert "Matern" in f.lib().covgram_last_error().decode()
    with pytest.raises(cg.UnsupportedKernel):
        f.check(raw_status(cg, matern, X, Y, U, A, F64)[0])
    st, out = raw_status(cg, comp, X, Y, U, A, F64)
    assert st == f.OK and np.all(np.isfinite(out))


def fd5(f, h):
    return (f(-2 * h) - 8 * f(-h) + 8 * f(h) - f(2 * h)) / (12 * h)


@pytest.mark.parametrize("name", [NAMES[0], NAMES[2], NAMES[3], NAMES[7]])
def test_mixed_bilinear_gradient_against_device_finite_differences(cg, oracle, name):
    """grad against 5-point differences of uᵀ(gramian(k_θ, x) @ a) formed by the EXISTING fp64 product on the device, 40 columns (two
    chunks); value against that product.  Tolerance: the product's rounding, at most 64 ε Σ|u|ᵀ|K̄||a| per evaluation (its own entry-wise
    bound with room), enters the difference quotient with the weights 18/12 and 1/h; the truncation h⁴f⁽⁵⁾/30 is below 1e-8 relative."""
    n, m, d, same, _ = R.SHAPES[0]
    k = R.kernels(cg)[name]
    X, _ = R.clouds(name, n, m, d, True)
    U, A = R.weights_for(n, n, 40)
    dev = cg.get_ctx().device
    tx, tu, ta = (torch.as_tensor(v, dtype=torch.float64).to(dev) for v in (X, U, A))
    G = cg.gramian(k, tx)
    assert type(G).__name__ == ("Gramian" if name == NAMES[7] else "MixedGramian")
    value, grad = cg.mixed_bilinear_gradient(G, tu, ta)
    comp, _ = cg.require_mixed_parameter_spec(k)
    maj = R.majorant_sums(cg, oracle, comp, X, X, U, A)
    S = float(sum(abs(c) * maj[t] for t, (c, _) in enumerate(R.terms_of(comp))))          # Σ|u|ᵀ|K̄||a|, K̄ = Σ_t |c_t| Π|ψ|
    noise = 64 * np.finfo(F64).eps * S
    form = lambda kk: float((tu * (cg.gramian(kk, tx) @ ta)).sum())
    assert abs(float(value) - form(k)) <= 2 * noise, (name, float(value), form(k))
    theta = np.array([v for _, _, v in cg.hyperparameters(k)])
    assert grad.shape == (len(theta),) and grad.dtype == torch.float64
    for i in range(len(theta)):
        h = 1e-3 * max(abs(theta[i]), 0.1)
        def f(s):
            th = theta.copy(); th[i] += s
            return form(cg.with_hyperparameters(k, th))
        fd = fd5(f, h)
        tol = 1e-8 * max(abs(fd), 1.0) + 1.5 * noise / h
        print(f"mixed_bilinear_gradient {name} θ[{i}] = {cg.hyperparameters(k)[i][1]}: grad {float(grad[i]):.10e} fd {fd:.10e} err/tol {abs(float(grad[i]) - fd) / tol:.3f}")
        assert abs(float(grad[i]) - fd) <= tol, (name, i, float(grad[i]), fd, tol)


IQ_N, IQ_D, IQ_P, IQ_SHIFT = 256, 2, 8, 0.1


def test_inv_quad_logdet_gradient_of_a_mixed_gramian(cg):
    """A = gramian(1.5 Lengthscale(EQ, 0.7) + 0.5 Dot, x) + 0.1 I against a dense fp64 host computation of −αᵀ∂Gα and (1/p) Σ z_tᵀA⁻¹∂G z_t,
    with test_gpu_bilin_grad.py's tolerance for the same check."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((IQ_N, IQ_D)); b = rng.standard_normal(IQ_N)
    Z = 2.0 * rng.integers(0, 2, size=(IQ_N, IQ_P)) - 1.0
    k = 1.5 * cg.Lengthscale(cg.EQ(), 0.7) + 0.5 * cg.Dot()
    tx = torch.as_tensor(x).cuda()
    G = cg.gramian(k, tx)
    assert type(G) is cg.MixedGramian
    Aop = G + torch.full((IQ_N,), IQ_SHIFT, dtype=torch.float64, device=tx.device)
    iq, ld, sol, gq, gl, info = cg.inv_quad_logdet_gradient(Aop, torch.as_tensor(b).cuda(), probes=torch.as_tensor(Z).cuda(), reltol=1e-10)
    assert info["converged"]
    r2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    E = np.exp(-r2 / (2 * 0.7 ** 2)); P = x @ x.T
    Amat = 1.5 * E + 0.5 * P + IQ_SHIFT * np.eye(IQ_N)
    dA = [E, 1.5 * E * r2 / 0.7 ** 3, P, np.eye(IQ_N)]                           # scale, l, scale, shift: hyperparameters order, then σ²
    alpha = np.linalg.solve(Amat, b); AZ = np.linalg.solve(Amat, Z)
    gq_ref = np.array([-alpha @ D @ alpha for D in dA])
    per = np.array([[Z[:, t] @ D @ AZ[:, t] for D in dA] for t in range(IQ_P)])
    rel = lambda a, r: np.abs(np.asarray(a) - r) / np.abs(r)
    print("inv_quad_logdet_gradient (mixed): rel err grad_inv_quad", rel(gq, gq_ref), "grad_logdet", rel(gl, per.mean(0)))
    assert gq.shape == (4,) and gl.shape == (4,)
    assert np.all(rel(gq, gq_ref) <= 1e-7) and np.all(rel(gl, per.mean(0)) <= 1e-7)
    assert abs(float(iq) - b @ alpha) <= 1e-7 * abs(float(iq))
    se = info["grad_logdet_stderr"].numpy()
    assert np.all(rel(se, per.std(0, ddof=1) / np.sqrt(IQ_P)) <= 1e-6)
