"""covgram_bilinear_grad_sm, spectral_mixture_gradient and inv_quad_logdet_gradient of a spectral mixture on the device against the fp64
reference and the bound of tests/sm_grad_ref.py (run with -s for the worst err / bound of every case)."""
import ctypes as C

import numpy as np
import pytest
import torch

import matrix_cases as mc
import sm_grad_ref as gr
import sm_ref as sr

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def kernel_of(cg, w, mu, l):
    return cg.SM(w, [m for m in mu], [lq for lq in l])


def raw_status(cg, G, U, A, nvec=None, px=None, py=None):
    """(status, out) of one covgram_bilinear_grad_sm call with G's handle on numpy weights; px / py: point handles to pass in place of G's."""
    f = cg._ffi
    dev = G.device
    U2 = U if U.ndim == 2 else U[:, None]; A2 = A if A.ndim == 2 else A[:, None]
    ut = torch.as_tensor(np.ascontiguousarray(U2.T)).to(dev); at = torch.as_tensor(np.ascontiguousarray(A2.T)).to(dev)
    nv = U2.shape[1] if nvec is None else nvec
    nout = G.w.shape[0] * (1 + 2 * G.x.shape[1])
    out = torch.full((nout,), float("nan"), dtype=torch.float64, device=dev)
    G._px.ctx.bind_stream()
    hx = G._px.handle if px is None else px
    hy = (None if G._py is G._px else G._py.handle) if py is None else py
    st = f.lib().covgram_bilinear_grad_sm(G.handle, hx, hy, f._P(ut.data_ptr()), max(U2.shape[0], 1), f._P(at.data_ptr()), max(A2.shape[0], 1), nv,
                                          C.cast(out.data_ptr(), C.POINTER(C.c_double)), f.DEVICE)
    return st, out.cpu().numpy()


def raw(cg, G, U, A):
    st, out = raw_status(cg, G, U, A)
    cg._ffi.check(st)
    return out


def check(tag, got, ref, bound, d):
    r, i = gr.worst(got, ref, bound)
    kind = ["dw", "dmu", "E"][0 if i % (1 + 2 * d) == 0 else (1 if i % (1 + 2 * d) <= d else 2)]
    print(f"sm-grad {tag}: worst err/bound {r:.3f} at out[{i}] ({kind}; ref {ref[i]:.6e}, got {got[i]:.6e})")
    assert r <= 1.0, (tag, i, got[i], ref[i], bound[i])
    return r


# ---- the raw entry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", gr.COMPONENTS)
@pytest.mark.parametrize("d", gr.DIMS)
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_main_sweep(cg, dev, dt, d, Q):
    """Every shape, both lengthscale forms and every column count at this (dtype, d, Q): X != Y, ragged tiles in both directions, one
    row, one column; one component chunk, a ragged last chunk and the maximum; 4 far and 4 copied rows (r = 0 exactly)."""
    for n, m in gr.SHAPES:
        for scalar_l in (True, False):
            X, Y, w, mu, l, inv_l = gr.make_case(n, m, d, Q, scalar_l, dt)
            G = cg.gramian(kernel_of(cg, w, mu, l), torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev))
            assert isinstance(G, cg.SpectralMixtureGramian)
            ws = [gr.weights(n, m, nv, dt) for nv in gr.NVECS]
            for (U, A), (ref, bound) in zip(ws, gr.reference_and_bound(w, mu, inv_l, X, Y, ws, dt)):
                check(f"{n}x{m} d={d} Q={Q} {'iso' if scalar_l else 'ard'} nvec={U.shape[1]} {dt.__name__}", raw(cg, G, U, A), ref, bound, d)


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_symmetric_call_and_its_diagonal(cg, dev, dt):
    """Y = NULL equals X against a copy of X within the bound; with U and A supported on one index each the diagonal gives exactly W_ii
    to the first output of every component and exact zeros to the others."""
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
    U, A = gr.weights(n, n, 3, dt)
    ref, bound = gr.reference_and_bound(w, mu, inv_l, X, X, [(U, A)], dt)[0]
    check(f"Y=NULL {dt.__name__}", raw(cg, Gs, U, A), ref, bound, d)
    check(f"Y=copy {dt.__name__}", raw(cg, Gc, U, A), ref, bound, d)
    for i in (0, 100, 256):
        e1 = np.zeros((n, 1), dt); e1[i] = dt(1.5)
        e2 = np.zeros((n, 1), dt); e2[i] = dt(-2.0)
        for G in (Gs, Gc):
            out = raw(cg, G, e1, e2).reshape(Q, 1 + 2 * d)
            assert np.all(out[:, 0] == -3.0), (i, out)
            assert np.all(out[:, 1:] == 0.0), (i, out)


def test_two_calls_agree_bitwise(cg, dev):
    """No atomics — on a shape with several row tiles, a column split, several hand-offs and two component chunks."""
    rng = np.random.default_rng(6000)
    n, m, d, Q = 1500, 2100, 3, 5
    X = rng.standard_normal((n, d)).astype(F32); Y = rng.standard_normal((m, d)).astype(F32)
    w, mu, l = sr.params(rng, Q, d, False)
    G = cg.gramian(kernel_of(cg, w, mu, l), torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev))
    U, A = gr.weights(n, m, 17, F32)
    a, b = raw(cg, G, U, A), raw(cg, G, U, A)
    assert a.tobytes() == b.tobytes()
    ref, bound = gr.reference_and_bound(w, mu, sr.inv_l_of(l, d), X, Y, [(U, A)], F32)[0]
    check("bitwise shape 1500x2100", a, ref, bound, d)


def test_empty_sides_give_zeros(cg, dev):
    w, mu, l = sr.params(np.random.default_rng(1), 3, 2, True)
    k = kernel_of(cg, w, mu, l)
    X = torch.zeros((5, 2), dtype=torch.float64, device=dev); E = torch.zeros((0, 2), dtype=torch.float64, device=dev)
    for G, n, m in ((cg.gramian(k, X, E), 5, 0), (cg.gramian(k, E, X), 0, 5)):
        out = raw(cg, G, np.ones((n, 2)), np.ones((m, 2)))
        assert out.shape == (15,) and np.all(out == 0.0)


def test_status_codes(cg, dev):
    f = cg._ffi
    rng = np.random.default_rng(8000)
    X = rng.standard_normal((40, 3)); Y = rng.standard_normal((30, 3))
    w, mu, l = sr.params(rng, 2, 3, True)
    G = cg.gramian(kernel_of(cg, w, mu, l), torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev))
    U, A = gr.weights(40, 30, 2, F64)
    assert raw_status(cg, G, U, A, nvec=0)[0] == f.EINVAL
    U33, A33 = gr.weights(40, 30, 33, F64)
    assert raw_status(cg, G, U33, A33)[0] == f.EINVAL
    assert b"nvec" in f.lib().covgram_last_error()
    G32 = cg.Gramian(cg.EQ(), torch.from_numpy(X.astype(F32)).to(dev), torch.from_numpy(Y.astype(F32)).to(dev))   # points of another dtype
    assert raw_status(cg, G, U, A, px=G32._px.handle, py=G32._py.handle)[0] == f.EINVAL
    G2 = cg.Gramian(cg.EQ(), torch.zeros((40, 2), dtype=torch.float64, device=dev))                              # points of another dimension
    assert raw_status(cg, G, U, U, px=G2._px.handle, py=G2._px.handle)[0] == f.EINVAL
    G._px.ctx.bind_stream()
    ut = torch.zeros((2, 40), dtype=torch.float64, device=dev); at = torch.zeros((2, 30), dtype=torch.float64, device=dev)
    assert f.lib().covgram_bilinear_grad_sm(G.handle, G._px.handle, G._py.handle, f._P(ut.data_ptr()), 40, f._P(at.data_ptr()), 30, 2, None,
                                            f.DEVICE) == f.EINVAL                                                # out is NULL
    st, out = raw_status(cg, G, U, A)
    assert st == f.OK and np.all(np.isfinite(out))


# ---- spectral_mixture_gradient -------------------------------------------------------------------------------------------------------
def chain_matrix(cg, k, d, nout):
    """The chain rules are linear in the device's numbers: value = v . out and grad = J out; the rows from unit vectors."""
    cols = [cg.spectral_mixture_chain_rules(k, e, d) for e in np.eye(nout)]
    return np.array([c[0] for c in cols]), np.array([c[1] for c in cols]).T


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_gradient_in_chunks_and_value_against_the_product(cg, dev, dt):
    """33 columns (chunks of 32 summed in fp64): value and gradient against the reference through the same chain rules, within the
    chain rules' |J| times the sum of the chunks' bounds; the value also against sum_t U[:, t] . (G A[:, t]) from the existing mul_, within
    the sum of both bounds — the product's is the entrywise bound of Matrix(G) weighted by |U| |A|' plus the summation error
    gamma_{m + n} sum |U| |G| |A| of its two sums."""
    n, m, d, Q = 257, 130, 3, 3
    X, Y, w, mu, l, inv_l = gr.make_case(n, m, d, Q, False, dt)
    k = kernel_of(cg, w, mu, l)
    G = cg.gramian(k, torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev))
    U, A = gr.weights(n, m, 33, dt)
    value, grad = cg.spectral_mixture_gradient(G, torch.from_numpy(U), torch.from_numpy(A))
    assert value.dtype == torch.float64 and value.dim() == 0 and value.device.type == "cpu"
    assert grad.dtype == torch.float64 and grad.device.type == "cpu" and grad.shape == (len(cg.hyperparameters(k)),)
    (r1, b1), (r2, b2) = gr.reference_and_bound(w, mu, inv_l, X, Y, [(U[:, :32], A[:, :32]), (U[:, 32:], A[:, 32:])], dt)
    ref, bound = r1 + r2, (b1 + b2) * (1 + 4 * np.finfo(F64).eps)
    v, J = chain_matrix(cg, k, d, Q * (1 + 2 * d))               # (of the tree's parameters, as spectral_mixture_gradient applies them)
    got = np.concatenate([[float(value)], grad.numpy()])
    want = np.concatenate([[v @ ref], J @ ref])
    lim = np.concatenate([[np.abs(v) @ bound], np.abs(J) @ bound]) + 16 * np.finfo(F64).eps * np.concatenate([[np.abs(v) @ np.abs(ref)], np.abs(J) @ np.abs(ref)])
    r = np.abs(got - want) / lim
    print(f"sm-grad spectral_mixture_gradient nvec=33 {dt.__name__}: worst err/bound {r.max():.3f} at entry {int(r.argmax())} (0 = value)")
    assert np.all(r <= 1.0), (got, want, lim)
    GA = (G @ torch.from_numpy(A).to(dev)).double().cpu().numpy()
    prod = float((U.astype(F64) * GA).sum())
    Kref, kb = sr.reference_and_bound(w, mu, inv_l, X, Y, dt)
    Wabs = np.abs(U.astype(F64)) @ np.abs(A.astype(F64)).T
    u = np.finfo(dt).eps / 2
    pb = float((Wabs * kb).sum() + (n + m) * u * (Wabs * np.abs(Kref)).sum())
    print(f"sm-grad value vs product {dt.__name__}: |diff| / (bound + product bound) = {abs(float(value) - prod) / (lim[0] + pb):.3f}")
    assert abs(float(value) - prod) <= lim[0] + pb


# ---- inv_quad_logdet_gradient --------------------------------------------------------------------------------------------------------
IQ_N, IQ_D, IQ_Q, IQ_P, IQ_SEED, IQ_SHIFT = 256, 2, 2, 8, 0, 0.1


def iq_problem():
    rng = np.random.default_rng(IQ_SEED)
    x = rng.standard_normal((IQ_N, IQ_D))
    b = rng.standard_normal(IQ_N)
    Z = 2.0 * rng.integers(0, 2, size=(IQ_N, IQ_P)) - 1.0
    w = np.array([1.3, 0.6]); mu = np.array([[0.15, 0.1], [0.35, -0.2]]); l = [0.8, np.array([0.6, 1.1])]
    return x, b, Z, w, mu, l


def iq_dense(cg, k, x, w, mu, l, K=None):
    """A = K + shift I and [dA/dtheta_p ..., dA/dshift] in dense fp64: dK/dtheta_p = sum_o J[p, o] Q_o, the chain rules applied to the
    reference's per-pair quantities (K: a dense Gramian to use in place of the reference's)."""
    inv_l = sr.inv_l_of(np.array([np.broadcast_to(lq, (IQ_D,)) for lq in l]), IQ_D)
    Qs = np.concatenate([q for q, _ in gr.pair_quantities(w, mu, inv_l, x, x, F64)], axis=0)      # Q (1 + 2d) x n x n
    v, J = chain_matrix(cg, k, IQ_D, Qs.shape[0])
    K = np.tensordot(v, Qs, axes=1) if K is None else K
    return K + IQ_SHIFT * np.eye(len(x)), [np.tensordot(J[p], Qs, axes=1) for p in range(J.shape[0])] + [np.eye(len(x))]


def iq_expressions(Amat, dA, b, Z):
    """(grad_inv_quad, per-probe terms) evaluated densely."""
    alpha = np.linalg.solve(Amat, b)
    AZ = np.linalg.solve(Amat, Z)
    gq = np.array([-alpha @ D @ alpha for D in dA])
    per = np.array([[Z[:, t] @ D @ AZ[:, t] for D in dA] for t in range(Z.shape[1])])
    return gq, per


def test_inv_quad_logdet_gradient(cg, dev):
    x, b, Z, w, mu, l = iq_problem()
    k = kernel_of(cg, w, mu, l)
    tx = torch.as_tensor(x).to(dev)
    G = cg.gramian(k, tx)
    assert isinstance(G, cg.SpectralMixtureGramian)
    Aop = G + torch.full((IQ_N,), IQ_SHIFT, dtype=torch.float64, device=dev)
    iq, ld, sol, gq, gl, info = cg.inv_quad_logdet_gradient(Aop, torch.as_tensor(b).to(dev), probes=torch.as_tensor(Z).to(dev), reltol=1e-10)
    assert info["converged"]
    nparam = len(cg.hyperparameters(k))
    assert nparam == 2 + 2 * 2 + 1 + 2 and gq.shape == (nparam + 1,) and gl.shape == (nparam + 1,)
    Kd = G.to_dense().double().cpu().numpy()
    Amat, dA = iq_dense(cg, k, x, w, mu, l, Kd)
    assert np.max(np.abs(Kd - (iq_dense(cg, k, x, w, mu, l)[0] - IQ_SHIFT * np.eye(IQ_N)))) <= 1e-11
    gq_ref, per = iq_expressions(Amat, dA, b, Z)
    gl_ref = per.mean(0)
    rel = lambda a, r: np.abs(np.asarray(a) - r) / np.abs(r)
    print("sm inv_quad_logdet_gradient: rel err grad_inv_quad", rel(gq, gq_ref), "grad_logdet", rel(gl, gl_ref))
    assert np.all(rel(gq, gq_ref) <= 1e-7) and np.all(rel(gl, gl_ref) <= 1e-7)
    assert abs(float(iq) - b @ np.linalg.solve(Amat, b)) <= 1e-7 * abs(float(iq))
    se = info["grad_logdet_stderr"].numpy()
    assert info["grad_logdet_values"].shape == (IQ_P, nparam + 1)
    assert np.all(rel(se, per.std(0, ddof=1) / np.sqrt(IQ_P)) <= 1e-6)
