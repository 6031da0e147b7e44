"""Host side of the input gradients (no GPU): the reference of tests/input_grad_ref.py against finite differences, the zero-distance rule
and the symmetric composition, the host chain rules of bilinear_input_gradient, the refusals of it and of gram_product, and the
feasibility of the GPU test's bound."""
import types

import numpy as np
import pytest
import torch

import covgram_oracle as o
import input_grad_ref as ir
import matrix_cases as mc
from test_bilin_grad_host import LENGTHSCALE_KERNELS, fd5, host_form, oracle_kernel, small_cloud

F32, F64 = np.float32, np.float64
SMOOTH_AND_KINKED = [(n, k) for n, k in LENGTHSCALE_KERNELS if k.family != o.MATERN] + \
    [("MaternP(0)", o.Kernel(o.MATERNP, p=0)), ("MaternP(1)", o.Kernel(o.MATERNP, p=1)),
     ("1.7*RQ(2.5)^3 l=0.8", o.Kernel(o.RQ, param=2.5, power=3, lengthscale=0.8, scale=1.7))]


def distinct_cloud():
    """small_cloud() without its four copied rows: kinked profiles have no derivative at a coincident pair."""
    X, Y, W = small_cloud()
    return X, Y[4:].copy(), W[:, 4:].copy()


@pytest.mark.parametrize("name,ko", SMOOTH_AND_KINKED, ids=[n for n, _ in SMOOTH_AND_KINKED])
def test_reference_against_finite_differences(name, ko):
    """Both sides: d/dx_ic from the row call, d/dy_jc from the call with the roles swapped, against a five-point difference of
    sum W o matrix(k, X, Y); relative to sum_j |W| |Q| of that row and dimension."""
    X, Y, W = distinct_cloud()
    n, m = W.shape
    refx = ir.reference(o, ko, X, Y, W, np.eye(m)); magx = ir.magnitude(o, ko, X, Y, W, np.eye(m))
    refy = ir.reference(o, ko, Y, X, np.eye(m), W); magy = ir.magnitude(o, ko, Y, X, np.eye(m), W)
    assert refx.shape == (n, 3) and refy.shape == (m, 3)
    worst = 0.0
    for side, ref, mag, coords in (("x", refx, magx, ((0, 0), (5, 1), (17, 2), (40, 0), (66, 1), (33, 2))), ("y", refy, magy, ((0, 0), (11, 1), (28, 2)))):
        for i, c in coords:
            def f(h):
                P = (X if side == "x" else Y).copy(); P[i, c] += h
                return float((W * (o.matrix(ko, P, Y) if side == "x" else o.matrix(ko, X, P))).sum())
            r = abs(ref[i, c] - fd5(f)) / mag[i, c]
            worst = max(worst, r)
            assert r <= 1e-9, (name, side, i, c, ref[i, c], fd5(f))
    print(f"input-grad-host {name}: worst |ref - fd5| / sum |W||Q| = {worst:.2e}")


def test_reference_zero_distance_and_symmetric_composition():
    X, Y, W = small_cloud()                                        # Y[:4] = X[[5, 17, 40, 66]]
    for name, ko in SMOOTH_AND_KINKED:
        ref = ir.reference(o, ko, X, Y, W, np.eye(33))
        assert np.all(np.isfinite(ref)), name
        e1 = np.zeros((67, 1)); e1[5] = 1.5
        e2 = np.zeros((33, 1)); e2[0] = -2.0
        assert np.array_equal(ir.reference(o, ko, X, Y, e1, e2), np.zeros((67, 3))), name
        assert np.array_equal(ir.reference(o, ko, Y, X, e2, e1), np.zeros((33, 3))), name
    # Y = X with both sides moving: the row call plus the call with U and A swapped
    rng = np.random.default_rng(12)
    Xs = X[:20]
    U, A = rng.standard_normal((20, 3)), rng.standard_normal((20, 3))
    for ko in (o.Kernel(o.EQ, lengthscale=0.7), o.Kernel(o.MATERNP, p=2, scale=2.5), o.Kernel(o.EXP)):
        total = ir.reference(o, ko, Xs, Xs, U, A) + ir.reference(o, ko, Xs, Xs, A, U)
        mag = ir.magnitude(o, ko, Xs, Xs, U, A) + ir.magnitude(o, ko, Xs, Xs, A, U)
        for i, c in ((0, 0), (7, 1), (19, 2)):
            def f(h):
                P = Xs.copy(); P[i, c] += h
                return float(((U @ A.T) * o.matrix(ko, P, P)).sum())
            assert abs(total[i, c] - fd5(f)) <= 1e-9 * mag[i, c], (ko.family, i, c)


# ---- the host chain rules, with the device call replaced by the reference -----------------------------------------------------------
def fake_gramian(cg, k, Xt, Yt=None, scaled=None):
    """A Gramian as gramian() would hand it to bilinear_input_gradient, without a device: `Xt`, `Yt` are the points it HOLDS."""
    import sys
    gm = sys.modules["covgram.gramian"]
    G = object.__new__(gm.Gramian)
    G.k = k
    G.x = torch.as_tensor(Xt)
    G._px = types.SimpleNamespace(pts=np.asarray(Xt))
    if Yt is None:
        G.y, G._py = G.x, G._px
    else:
        G.y = torch.as_tensor(Yt)
        G._py = types.SimpleNamespace(pts=np.asarray(Yt))
    G.shape = (G.x.shape[0], G.y.shape[0])
    G.dtype, G.device = torch.float64, torch.device("cpu")
    if scaled is not None:
        G.scaled_input = scaled
    return G


@pytest.fixture
def reference_device(cg, monkeypatch):
    """covgram.gramian._input_grad_device computes the reference; returns the list of calls made."""
    import sys
    gm = sys.modules["covgram.gramian"]
    calls = []

    def device(spec, px, py, Ut, At, rows, cols, d, device):
        Xn, Yn = px.pts, (px.pts if py is None else py.pts)
        assert Xn.shape == (rows, d) and Yn.shape == (cols, d) and Ut.shape[1] == rows and At.shape[1] == cols
        calls.append(spec)
        return torch.from_numpy(ir.reference(o, oracle_kernel(spec), Xn, Yn, Ut.numpy().T, At.numpy().T))
    monkeypatch.setattr(gm, "_input_grad_device", device)
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(cg._ffi, "lib", no_lib)
    return calls


def chain_rule_cloud():
    rng = np.random.default_rng(5)
    X = 0.8 * rng.standard_normal((12, 3)) + 0.2; Y = 0.8 * rng.standard_normal((9, 3))
    return X, Y, rng.standard_normal((12, 2)), rng.standard_normal((9, 2))


def check_against_fd(cg, top, X, Y, U, A, dX, dY):
    W = U @ A.T
    for side, got, coords in (("x", dX, ((0, 0), (3, 1), (11, 2))), ("y", dY, ((0, 2), (8, 0)))):
        for i, c in coords:
            def f(h):
                P = (X if side == "x" else Y).copy(); P[i, c] += h
                return host_form(top, P, Y, W) if side == "x" else host_form(top, X, P, W)
            fd = fd5(f)
            print(f"input-grad-host chain rule d/d{side}[{i}, {c}]: {float(got[i, c]):.12e} against {fd:.12e}")
            assert abs(float(got[i, c]) - fd) <= 1e-8 * max(abs(fd), 1.0), (side, i, c, float(got[i, c]), fd)


def test_chain_rules_ard_and_scaled_input(cg, reference_device):
    X, Y, U, A = chain_rule_cloud()
    for top in (cg.ARD(2.0 * cg.MaternP(2), [0.7, 1.1, 1.9]), cg.ScaledInputKernel(cg.Lengthscale(cg.RQ(0.37), 1.2), np.array([1.4, 0.6, 0.9]))):
        G = fake_gramian(cg, top.k, X * top.U, Y * top.U, scaled=top)
        dX, dY = cg.bilinear_input_gradient(G, torch.as_tensor(U), torch.as_tensor(A))
        assert dX.shape == (12, 3) and dY.shape == (9, 3) and dX.dtype == torch.float64
        check_against_fd(cg, top, X, Y, U, A, dX, dY)
    assert len(reference_device) == 4


def test_chain_rules_sum_with_a_constant(cg, reference_device):
    X, Y, U, A = chain_rule_cloud()
    k = 1.5 * cg.Lengthscale(cg.EQ(), 0.7) + cg.Constant(0.25) + cg.Power(0.5 * cg.Lengthscale(cg.InverseMultiQuadratic(0.6), 0.9), 2)
    dX, dY = cg.bilinear_input_gradient(fake_gramian(cg, k, X, Y), U, A)
    check_against_fd(cg, k, X, Y, U, A, dX, dY)
    assert len(reference_device) == 4                               # two terms, two sides: the Constant launches nothing
    only_constant = cg.bilinear_input_gradient(fake_gramian(cg, cg.Constant(0.25) + cg.Constant(1.0), X, Y), U, A)
    assert not only_constant[0].any() and not only_constant[1].any() and len(reference_device) == 4


def test_symmetric_case_and_the_single_call_route(cg, reference_device):
    X, _, U, A = chain_rule_cloud()
    k = 2.5 * cg.Lengthscale(cg.MaternP(2), 1.3)
    A = np.random.default_rng(6).standard_normal((12, 2))
    dX, dY = cg.bilinear_input_gradient(fake_gramian(cg, k, X), U, A)
    assert dY is None and len(reference_device) == 2
    W = U @ A.T
    for i, c in ((0, 0), (3, 1), (11, 2)):
        def f(h):
            P = X.copy(); P[i, c] += h
            return host_form(k, P, P, W)
        fd = fd5(f)
        assert abs(float(dX[i, c]) - fd) <= 1e-8 * max(abs(fd), 1.0), (i, c, float(dX[i, c]), fd)
    # U is A: one call, doubled, bit for bit the two-call route
    del reference_device[:]
    Ut = torch.as_tensor(U)
    one = cg.bilinear_input_gradient(fake_gramian(cg, k, X), Ut, Ut)[0]
    assert len(reference_device) == 1
    two = cg.bilinear_input_gradient(fake_gramian(cg, k, X), Ut, Ut.clone())[0]
    assert len(reference_device) == 3
    assert torch.equal(one, two)
    # a view with other strides is another tensor
    cg.bilinear_input_gradient(fake_gramian(cg, k, X), Ut, torch.as_tensor(np.asfortranarray(U)))
    assert len(reference_device) == 5


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_device_call(cg, monkeypatch):
    import sys
    gm, dist = sys.modules["covgram.gramian"], sys.modules["covgram.dist"]
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(cg._ffi, "lib", no_lib)
    u = np.zeros(4)

    def bare(k):
        G = object.__new__(gm.Gramian)
        G.k = k
        return G
    kernels = ((cg.EQ() * cg.Cauchy(), "Product of two non-constant"), (cg.Dot(), "Dot"), (2.0 * cg.ExponentialDot(), "ExponentialDot"),
               (cg.Matern(0.8), "real nu"), (cg.Lengthscale(cg.EQ(), 0.7) + cg.Matern(1.3), "real nu"),
               (cg.SpectralMixture([1.0], [[0.3]], [[1.0]]), ""), (cg.VerticalRescaling(cg.EQ(), lambda x: x), "VerticalRescaling"),
               (cg.Power(cg.EQ(), 2) * cg.RQ(1.0), "Product of two non-constant"), (cg.GradientKernel(cg.EQ()), "GradientKernel"))
    operators = (gm.BlockGramian, gm.HessianGramian, gm.ValueGradientHessianGramian, gm.SymmetricToeplitz, gm.Toeplitz, gm.Circulant,
                 gm.KroneckerProduct, gm.SparseGramian, gm.BarnesHutFactorization, gm.SpectralMixtureGramian, gm.LazyMatrixProduct,
                 dist.ShardedGramian)
    for k, word in kernels:
        with pytest.raises(cg.UnsupportedKernel, match="bilinear_input_gradient.*" + word):
            cg.bilinear_input_gradient(bare(k), u, u)
    for cls in operators:
        with pytest.raises(cg.UnsupportedKernel, match="bilinear_input_gradient: " + cls.__name__):
            cg.bilinear_input_gradient(object.__new__(cls), u, u)
    full = bare(cg.EQ())
    full.scaled_input = cg.ScaledInputKernel(cg.EQ(), np.eye(2))
    with pytest.raises(cg.UnsupportedKernel, match="full matrix"):
        cg.bilinear_input_gradient(full, u, u)
    ard_sum = bare(cg.EQ() + cg.RQ(1.0))
    ard_sum.scaled_input = cg.ARD(cg.EQ(), [1.0, 2.0])
    with pytest.raises(cg.UnsupportedKernel, match="ARD over a Sum"):
        cg.bilinear_input_gradient(ard_sum, u, u)

    # gram_product: anything but a plain Gramian once x, y or theta need a gradient
    a = torch.zeros(4, dtype=torch.float64)
    x = torch.zeros((4, 2), dtype=torch.float64, requires_grad=True)
    theta = torch.ones(1, dtype=torch.float64, requires_grad=True)
    for k, word in kernels:
        with pytest.raises(cg.UnsupportedKernel, match="gram_product.*" + word):
            cg.gram_product(k, x, a)
    for cls in operators:
        with pytest.raises(cg.UnsupportedKernel, match="gram_product.*" + cls.__name__):
            cg.gram_product(object.__new__(cls), None, a, theta=theta)
        with pytest.raises(cg.UnsupportedKernel, match="gram_product.*" + cls.__name__):
            cg.gram_product(object.__new__(cls), x, a)
    with pytest.raises(cg.UnsupportedKernel, match="gram_product.*StepRangeLen"):
        cg.gram_product(cg.Lengthscale(cg.EQ(), 1.0), cg.srange(-1, 1, 4), a, theta=theta)
    # what gramian() builds from a supported kernel and tensors but is no plain Gramian
    monkeypatch.setattr(sys.modules["covgram.autograd"], "gramian", lambda k, x, y=None: object.__new__(gm.SparseGramian))
    with pytest.raises(cg.UnsupportedKernel, match="gram_product.*SparseGramian"):
        cg.gram_product(cg.EQ(), x, a)


# ---- the GPU test's bound is feasible -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 8])
def test_fp32_emulation_within_the_gpu_bound(d):
    """An exactly rounded fp32 evaluation in the kernel's order (input_grad_ref.emulate_f32) on the GPU test's own clouds.  The device's
    exp / log / pow are not part of this emulation: their headroom is what the GPU test measures.  A ratio above 1 is a finding about
    the bound, never a number to fit."""
    import test_gpu_bilin_grad as tg
    for name, ko in tg.FAMILIES:
        rng = np.random.default_rng(1000 + d)
        X, Y = mc.iso_cloud(rng, tg.N, tg.M, d, F32, lscale=ko.lengthscale)[:2]
        for nvec in (1, 17):
            U, A = tg.weights(rng, tg.N, tg.M, nvec, F32)
            ref, bound = ir.reference_and_bound(o, ko, X, Y, U, A, F32)
            r = np.abs(ir.emulate_f32(o, ko, X, Y, U, A) - ref) / bound
            w = np.unravel_index(int(r.argmax()), r.shape)
            print(f"input-grad-bound-host {name:22s} d={d} nvec={nvec:2d}: worst err/bound {r.max():.3f} at row {w[0]} dimension {w[1]}")
            assert r.max() <= 1.0, (name, d, nvec, w, r.max())
