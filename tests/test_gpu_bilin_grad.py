"""covgram_bilinear_grad, bilinear_gradient and inv_quad_logdet_gradient on the device against the fp64 reference and the derived
bound of tests/bilin_grad_ref.py (run with -s for the worst err / bound of every case)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bilin_grad_ref as br
import covgram_oracle as o
import matrix_cases as mc

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TDT = {F32: torch.float32, F64: torch.float64}
N, M = 257, 130

FAMILIES = [("EQ l=0.7", o.Kernel(o.EQ, lengthscale=0.7)), ("Exp", o.Kernel(o.EXP)), ("RQ(0.37)", o.Kernel(o.RQ, param=0.37)),
            ("gammaExp(1.5)", o.Kernel(o.GAMMAEXP, param=1.5)), ("Cauchy^2", o.Kernel(o.CAUCHY, power=2)),
            ("IMQ(0.6) l=0.9", o.Kernel(o.IMQ, param=0.6, lengthscale=0.9)), ("2.5*MaternP(2) l=1.3", o.Kernel(o.MATERNP, p=2, lengthscale=1.3, scale=2.5)),
            ("MaternP(0)", o.Kernel(o.MATERNP, p=0)), ("MaternP(5)^2", o.Kernel(o.MATERNP, p=5, power=2)),
            ("1.7*RQ(2.5)^3 l=0.8", o.Kernel(o.RQ, param=2.5, power=3, lengthscale=0.8, scale=1.7))]


def spec_of(cg, ko):
    s = cg._ffi.covgram_kernel()
    s.family, s.trait, s.p, s.power = ko.family, ko.trait, ko.p, ko.power
    s.param, s.lengthscale, s.scale = ko.param, ko.lengthscale, ko.scale
    return s


def raw_status(cg, spec, X, Y, U, A, per_dim, nvec=None, kptr=None):
    """(status, out) of one covgram_bilinear_grad call on numpy inputs (Y None = the symmetric call)."""
    from covgram.gramian import _Points
    dev = cg.get_ctx().device
    tx = torch.as_tensor(X).to(dev).contiguous()
    px = _Points(tx)
    py = None
    if Y is not None:
        ty = torch.as_tensor(Y).to(dev).contiguous()
        py = _Points(ty)
    U2 = U.reshape(U.shape[0], -1); A2 = A.reshape(A.shape[0], -1)
    ut = torch.as_tensor(np.ascontiguousarray(U2.T)).to(dev); at = torch.as_tensor(np.ascontiguousarray(A2.T)).to(dev)
    nv = U2.shape[1] if nvec is None else nvec
    nout = 2 + (X.shape[1] if per_dim else 1)
    out = torch.full((nout,), float("nan"), dtype=torch.float64, device=dev)
    st = cg._ffi.lib().covgram_bilinear_grad(px.ctx.bind_stream(), kptr if kptr is not None else cg._ffi.kref(spec), px.handle,
                                             py.handle if py is not None else None, cg._ffi._P(ut.data_ptr()), X.shape[0],
                                             cg._ffi._P(at.data_ptr()), A2.shape[0], nv, per_dim,
                                             C.cast(out.data_ptr(), C.POINTER(C.c_double)), cg._ffi.DEVICE)
    return st, out.cpu().numpy()


def raw(cg, ko, X, Y, U, A, per_dim):
    st, out = raw_status(cg, spec_of(cg, ko), X, Y, U, A, per_dim)
    cg._ffi.check(st)
    return out


def check(tag, got, ref, bound):
    with np.errstate(invalid="ignore"):
        r = np.where(np.isfinite(got), np.abs(got - ref) / bound, np.inf)
    w = int(np.argmax(r))
    print(f"bilin-grad {tag}: worst err/bound {r[w]:.3f} at out[{w}] (ref {ref[w]:.6e}, got {got[w]:.6e})")
    assert r[w] <= 1.0, (tag, w, got[w], ref[w], bound[w])
    return float(r[w])


def weights(rng, n, m, nvec, dt):
    return rng.standard_normal((n, nvec)).astype(dt), rng.standard_normal((m, nvec)).astype(dt)


@pytest.mark.parametrize("d", [1, 3, 8])
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_every_family_against_the_reference(cg, dt, d):
    """(a): every supported family, nvec in {1, 3, 17}, per_dim on and off, X != Y, ragged tiles in both directions."""
    for name, ko in FAMILIES:
        rng = np.random.default_rng(1000 + d)
        X, Y, far, cop = mc.iso_cloud(rng, N, M, d, dt, lscale=ko.lengthscale)
        assert len(far) == 8 and len(cop) == 4
        for nvec in (1, 3, 17):
            U, A = weights(rng, N, M, nvec, dt)
            for per_dim in (0, 1):
                ref, bound = br.reference_and_bound(o, ko, X, Y, U, A, per_dim, dt)
                check(f"{name} d={d} nvec={nvec} per_dim={per_dim} {dt.__name__}", raw(cg, ko, X, Y, U, A, per_dim), ref, bound)


@pytest.mark.parametrize("d", [33, 64])
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_wide_points_per_dimension(cg, dt, d):
    """(b): the slab path (d > 16), per_dim on.  The cloud shrinks with d as matrix_cases.wide_cloud's does (|x - y|^2 as at d = 8)."""
    for name, ko in (FAMILIES[0], FAMILIES[6]):
        rng = np.random.default_rng(2000 + d)
        X, Y = mc.iso_cloud(rng, N, M, d, dt, lscale=ko.lengthscale, spread=0.8 * np.sqrt(8.0 / d), shift=0.2 * np.sqrt(8.0 / d))[:2]
        U, A = weights(rng, N, M, 5, dt)
        ref, bound = br.reference_and_bound(o, ko, X, Y, U, A, 1, dt)
        check(f"{name} d={d} per_dim=1 {dt.__name__}", raw(cg, ko, X, Y, U, A, 1), ref, bound)


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_symmetric_call_and_its_diagonal(cg, dt):
    """(c): Y = NULL equals X against a copy of X within the bound; with U and A supported on one index each the diagonal gives exactly
    W_ii k(0) to out[0] and 0 to out[2 ..], also for the profiles whose derivative is unbounded at 0."""
    d = 3
    for name, ko in (FAMILIES[0], FAMILIES[1], FAMILIES[3], FAMILIES[7], FAMILIES[6]):
        rng = np.random.default_rng(3000)
        X = mc.iso_cloud(rng, N, N, d, dt, lscale=ko.lengthscale)[0]
        U, A = weights(rng, N, N, 3, dt)
        for per_dim in (0, 1):
            ref, bound = br.reference_and_bound(o, ko, X, X, U, A, per_dim, dt)
            sym = raw(cg, ko, X, None, U, A, per_dim)
            check(f"{name} Y=NULL per_dim={per_dim} {dt.__name__}", sym, ref, bound)
            check(f"{name} Y=copy per_dim={per_dim} {dt.__name__}", raw(cg, ko, X, X.copy(), U, A, per_dim), ref, bound)
            for i in (0, 100, 256):
                e1 = np.zeros((N, 1), dt); e1[i] = dt(1.5)
                e2 = np.zeros((N, 1), dt); e2[i] = dt(-2.0)
                out = raw(cg, ko, X, None, e1, e2, per_dim)
                k0 = float(o.profile(ko, np.zeros(1), dt)[0])
                assert abs(out[0] - (-3.0 * k0)) <= 4 * np.finfo(dt).eps * 3.0 * abs(k0), (name, i, out)
                assert np.all(out[2:] == 0.0), (name, i, out)
                assert np.isfinite(out[1]), (name, i, out)


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_column_limit_and_chunking(cg, dt):
    """(d): nvec = 32 through the raw entry, 33 through bilinear_gradient (chunks of 32 summed in fp64)."""
    d = 3
    name, ko = FAMILIES[6]
    rng = np.random.default_rng(4000)
    X, Y = mc.iso_cloud(rng, N, M, d, dt, lscale=ko.lengthscale)[:2]
    U, A = weights(rng, N, M, 33, dt)
    ref, bound = br.reference_and_bound(o, ko, X, Y, U[:, :32], A[:, :32], 0, dt)
    check(f"{name} nvec=32 {dt.__name__}", raw(cg, ko, X, Y, U[:, :32], A[:, :32], 0), ref, bound)
    k = 2.5 * cg.Lengthscale(cg.MaternP(2), 1.3)
    G = cg.gramian(k, torch.as_tensor(X).cuda(), torch.as_tensor(Y).cuda())
    value, grad = cg.bilinear_gradient(G, torch.as_tensor(U), torch.as_tensor(A))
    r1, b1 = br.reference_and_bound(o, ko, X, Y, U[:, :32], A[:, :32], 0, dt)
    r2, b2 = br.reference_and_bound(o, ko, X, Y, U[:, 32:], A[:, 32:], 0, dt)
    ref, bound = r1 + r2, b1 + b2
    assert [nm for _, nm, _ in cg.hyperparameters(k)] == ["scale", "l"]
    got = np.array([float(value), float(grad[0]) * 2.5, float(grad[1]) * 1.3 / -2.0])
    check(f"{name} nvec=33 bilinear_gradient {dt.__name__}", got, ref[[0, 0, 2]], bound[[0, 0, 2]] * (1 + 4 * np.finfo(F64).eps))


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_single_row_or_column(cg, dt):
    """(e): n = 1 or m = 1."""
    d = 3
    name, ko = FAMILIES[2]
    rng = np.random.default_rng(5000)
    X, Y = mc.iso_cloud(rng, N, M, d, dt)[:2]
    for Xs, Ys in ((X[:1], Y), (X, Y[:1]), (X[:1], Y[:1])):
        U, A = weights(rng, Xs.shape[0], Ys.shape[0], 3, dt)
        for per_dim in (0, 1):
            ref, bound = br.reference_and_bound(o, ko, Xs, Ys, U, A, per_dim, dt)
            check(f"{name} {Xs.shape[0]}x{Ys.shape[0]} per_dim={per_dim} {dt.__name__}", raw(cg, ko, Xs, Ys, U, A, per_dim), ref, bound)


def test_two_calls_agree_bitwise(cg):
    """(f): no atomics — on a shape with several row tiles, a column split and several hand-offs."""
    rng = np.random.default_rng(6000)
    ko = FAMILIES[6][1]
    X = rng.standard_normal((1500, 3)).astype(F32); Y = rng.standard_normal((2100, 3)).astype(F32)
    U, A = weights(rng, 1500, 2100, 17, F32)
    a, b = raw(cg, ko, X, Y, U, A, 1), raw(cg, ko, X, Y, U, A, 1)
    assert a.tobytes() == b.tobytes()
    ref, bound = br.reference_and_bound(o, ko, X, Y, U, A, 1, F32)
    check("bitwise shape 1500x2100", a, ref, bound)


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_value_agrees_with_the_product(cg, dt):
    """(g): out[0] against sum_t U[:, t] . (G A[:, t]) from the existing mul_, within the sum of both bounds: the product's is the
    entrywise bound of Matrix(G) weighted by |U| |A|' plus the summation error gamma_{m + n} sum |U| |K| |A| of its two sums."""
    d = 3
    for name, ko, k in ((FAMILIES[0][0], FAMILIES[0][1], cg.Lengthscale(cg.EQ(), 0.7)),
                        (FAMILIES[6][0], FAMILIES[6][1], 2.5 * cg.Lengthscale(cg.MaternP(2), 1.3))):
        rng = np.random.default_rng(7000)
        X, Y = mc.iso_cloud(rng, N, M, d, dt, lscale=ko.lengthscale)[:2]
        U, A = weights(rng, N, M, 3, dt)
        ref, bound = br.reference_and_bound(o, ko, X, Y, U, A, 0, dt)
        got = raw(cg, ko, X, Y, U, A, 0)
        G = cg.gramian(k, torch.as_tensor(X).cuda(), torch.as_tensor(Y).cuda())
        GA = (G @ torch.as_tensor(A).cuda()).double().cpu().numpy()
        prod = float((U.astype(F64) * GA).sum())
        Kref, kb = mc.reference_and_bound(o, ko, X, Y, dt)
        Wabs = np.abs(U.astype(F64)) @ np.abs(A.astype(F64)).T
        u = np.finfo(dt).eps / 2
        pb = float((Wabs * kb).sum() + (N + M) * u * (Wabs * np.abs(Kref)).sum())
        print(f"bilin-grad value vs product {name} {dt.__name__}: |diff| / (bound + product bound) = {abs(got[0] - prod) / (bound[0] + pb):.3f}")
        assert abs(got[0] - prod) <= bound[0] + pb


# ---- inv_quad_logdet_gradient ----------------------------------------------------------------------------------------------------
IQ_N, IQ_D, IQ_P, IQ_SEED, IQ_SHIFT = 512, 2, 8, 0, 0.1


def iq_problem():
    """x, b and the (n, 8) Rademacher probes of seed IQ_SEED; the seed is one for which the dense computation alone puts the exact
    tr(A^-1 dA) inside 4 standard errors of the fixed-probe estimate for every parameter (tests/test_bilin_grad_host.py checks that)."""
    rng = np.random.default_rng(IQ_SEED)
    x = rng.standard_normal((IQ_N, IQ_D))
    b = rng.standard_normal(IQ_N)
    Z = 2.0 * rng.integers(0, 2, size=(IQ_N, IQ_P)) - 1.0
    return x, b, Z


def iq_dense(x, K=None):
    """A = K + shift I and [dA/dscale, dA/dl, dA/dshift] for k = 2.0 Lengthscale(MaternP(2), 0.8), dense fp64 (K: a dense Gramian to
    use in place of the oracle's)."""
    ko = o.Kernel(o.MATERNP, p=2, lengthscale=0.8, scale=2.0)
    S = o.pair_arg(ko, x, x)
    v, d1, _ = o.profile_derivatives(ko, S)
    K = v if K is None else K
    return K + IQ_SHIFT * np.eye(len(x)), [K / 2.0, -2.0 / 0.8 * d1 * S, np.eye(len(x))]


def iq_expressions(Amat, dA, b, Z):
    """(grad_inv_quad, per-probe terms, exact traces) evaluated densely."""
    alpha = np.linalg.solve(Amat, b)
    AZ = np.linalg.solve(Amat, Z)
    gq = np.array([-alpha @ D @ alpha for D in dA])
    per = np.array([[Z[:, t] @ D @ AZ[:, t] for D in dA] for t in range(Z.shape[1])])
    exact = np.array([np.trace(np.linalg.solve(Amat, D)) for D in dA])
    return gq, per, exact


def test_inv_quad_logdet_gradient(cg):
    x, b, Z = iq_problem()
    k = 2.0 * cg.Lengthscale(cg.MaternP(2), 0.8)
    tx = torch.as_tensor(x).cuda()
    G = cg.gramian(k, tx)
    Aop = G + torch.full((IQ_N,), IQ_SHIFT, dtype=torch.float64, device=tx.device)
    iq, ld, sol, gq, gl, info = cg.inv_quad_logdet_gradient(Aop, torch.as_tensor(b).cuda(), probes=torch.as_tensor(Z).cuda(), reltol=1e-10)
    assert info["converged"]
    Amat, dA = iq_dense(x, G.to_dense().double().cpu().numpy())
    gq_ref, per, exact = iq_expressions(Amat, dA, b, Z)
    gl_ref = per.mean(0)
    rel = lambda a, r: np.abs(np.asarray(a) - r) / np.abs(r)
    print("inv_quad_logdet_gradient: rel err grad_inv_quad", rel(gq, gq_ref), "grad_logdet", rel(gl, gl_ref))
    assert gq.shape == (3,) and gl.shape == (3,)
    assert np.all(rel(gq, gq_ref) <= 1e-7) and np.all(rel(gl, gl_ref) <= 1e-7)
    assert abs(float(iq) - b @ np.linalg.solve(Amat, b)) <= 1e-7 * abs(float(iq))
    se = info["grad_logdet_stderr"].numpy()
    assert np.all(rel(se, per.std(0, ddof=1) / np.sqrt(IQ_P)) <= 1e-6)
    print("inv_quad_logdet_gradient: (exact trace - estimate) / stderr", (exact - gl.numpy()) / se)
    assert np.all(np.abs(exact - gl.numpy()) <= 4 * se)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_raw_entry_refusals(cg):
    f = cg._ffi
    rng = np.random.default_rng(8000)
    X = rng.standard_normal((40, 3)); Y = rng.standard_normal((30, 3))
    U, A = weights(rng, 40, 30, 2, F64)
    comp = cg.device_spec(cg.EQ() * cg.Lengthscale(cg.Cauchy(), 1.5))
    assert isinstance(comp, f.covgram_kernel_composite)
    assert raw_status(cg, None, X, Y, U, A, 0, kptr=f.kref(comp))[0] == f.EUNSUPPORTED
    assert raw_status(cg, spec_of(cg, o.Kernel(o.DOT)), X, Y, U, A, 0)[0] == f.EUNSUPPORTED
    assert raw_status(cg, spec_of(cg, o.Kernel(o.MATERN, param=0.8)), X, Y, U, A, 0)[0] == f.EUNSUPPORTED
    with pytest.raises(cg.UnsupportedKernel):
        f.check(raw_status(cg, spec_of(cg, o.Kernel(o.MATERN, param=0.8)), X, Y, U, A, 0)[0])
    U33, A33 = weights(rng, 40, 30, 33, F64)
    assert raw_status(cg, spec_of(cg, o.Kernel(o.EQ)), X, Y, U33, A33, 0)[0] == f.EINVAL
    X65 = rng.standard_normal((40, 65)); Y65 = rng.standard_normal((30, 65))
    assert raw_status(cg, spec_of(cg, o.Kernel(o.EQ)), X65, Y65, U, A, 1)[0] == f.EINVAL
    st, out = raw_status(cg, spec_of(cg, o.Kernel(o.EQ)), X, Y, U, A, 0)
    assert st == f.OK and np.all(np.isfinite(out))
