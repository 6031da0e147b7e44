"""Host side of the input gradients of SpectralMixture Gramians (no GPU): the reference of tests/sm_input_grad_ref.py against finite
differences on both sides and for one point set, the zero-distance rule, the feasibility and the sensitivity of the GPU test's bound,
the refusals of spectral_mixture_input_gradient and spectral_mixture_product, and the ABI."""
import os
import re

import numpy as np
import pytest
import torch

import sm_input_grad_ref as ir
import sm_ref as sr

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fd5(f, h=1e-3):
    return (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)


def small_case(scalar_l):
    """12 x 9 points in 3 dimensions, 3 components with |mu| <= 0.6 and l >= 0.6: the five-point difference at h = 1e-3 truncates at
    (2 pi |mu| h)^4 / 30 < 1e-11 of a term and rounds at eps / h ~ 1e-13 of the form."""
    rng = np.random.default_rng(5)
    X = 0.8 * rng.standard_normal((12, 3)) + 0.2; Y = 0.8 * rng.standard_normal((9, 3))
    w = np.array([1.3, -0.7, 0.4])
    mu = np.array([[0.0, 0.0, 0.0], [0.3, -0.2, 0.5], [-0.6, 0.4, 0.1]])
    l = np.array([0.8, 1.4, 0.6]) if scalar_l else np.array([[0.7, 1.1, 1.9], [1.2, 0.6, 0.9], [0.8, 1.5, 1.0]])
    return X, Y, w, mu, sr.inv_l_of(l, 3), rng.standard_normal((12, 2)), rng.standard_normal((9, 2))


@pytest.mark.parametrize("scalar_l", [True, False], ids=["iso", "ard"])
def test_reference_against_finite_differences(scalar_l):
    """Both sides: d/dx_ic from the row call, d/dy_jc from the call with the roles swapped, and one point set with both sides moving,
    against a five-point difference of F; relative to sum_j |W| M of that row and dimension."""
    X, Y, w, mu, inv_l, U, A = small_case(scalar_l)
    W = U @ A.T
    refx = ir.reference(w, mu, inv_l, X, Y, U, A); magx = ir.magnitude(w, mu, inv_l, X, Y, U, A)
    refy = ir.reference(w, mu, inv_l, Y, X, A, U); magy = ir.magnitude(w, mu, inv_l, Y, X, A, U)
    assert refx.shape == (12, 3) and refy.shape == (9, 3)
    worst = 0.0
    for side, ref, mag in (("x", refx, magx), ("y", refy, magy)):
        for i in range(ref.shape[0]):
            for c in range(3):
                def f(h):
                    P = (X if side == "x" else Y).copy(); P[i, c] += h
                    return ir.form(w, mu, inv_l, P, Y, W) if side == "x" else ir.form(w, mu, inv_l, X, P, W)
                r = abs(ref[i, c] - fd5(f)) / mag[i, c]
                worst = max(worst, r)
                assert r <= 1e-9, (side, i, c, ref[i, c], fd5(f))
    Xs = X[:9]
    total = ir.reference(w, mu, inv_l, Xs, Xs, A, U[:9]) + ir.reference(w, mu, inv_l, Xs, Xs, U[:9], A)
    mag = ir.magnitude(w, mu, inv_l, Xs, Xs, A, U[:9]) + ir.magnitude(w, mu, inv_l, Xs, Xs, U[:9], A)
    for i in range(9):
        for c in range(3):
            def f(h):
                P = Xs.copy(); P[i, c] += h
                return ir.form(w, mu, inv_l, P, P, A @ U[:9].T)
            r = abs(total[i, c] - fd5(f)) / mag[i, c]
            worst = max(worst, r)
            assert r <= 1e-9, ("one point set", i, c, total[i, c], fd5(f))
    print(f"sm-input-grad-host {'iso' if scalar_l else 'ard'}: worst |ref - fd5| / sum |W| M = {worst:.2e}")


def test_reference_zero_distance_pair():
    """A pair with r = 0 adds exactly 0 to every output, on a copied row."""
    X, Y, w, mu, l, inv_l = ir.make_case(63, 193, 3, 3, False, F64)
    Xc = X.copy(); Xc[5] = Y[7]
    e1 = np.zeros((63, 1)); e2 = np.zeros((193, 1))
    e1[5] = 1.5; e2[7] = -2.0
    assert np.array_equal(ir.reference(w, mu, inv_l, Xc, Y, e1, e2), np.zeros((63, 3)))
    assert np.array_equal(ir.reference(w, mu, inv_l, Y, Xc, e2, e1), np.zeros((193, 3)))
    emu = ir.emulate_f32(w, mu, inv_l, Xc.astype(F32), Y.astype(F32), e1.astype(F32), e2.astype(F32))
    assert np.array_equal(emu, np.zeros((63, 3)))


# ---- the GPU test's bound is feasible, and it notices a missing half -----------------------------------------------------------------
def sweep_cases(Q, full):
    """(n, m, nvecs, scalar_l) of the device sweep at this Q, every shape in both lengthscale forms; full = False: one column count
    per shape."""
    for (n, m), nv in zip(ir.SHAPES, (32, 1, 3, 17)):
        for scalar_l in (True, False):
            yield n, m, (ir.NVECS if full else (nv,)), scalar_l


@pytest.mark.parametrize("Q", ir.COMPONENTS)
@pytest.mark.parametrize("d", ir.DIMS)
def test_fp32_emulation_within_the_gpu_bound(d, Q):
    """An exactly rounded fp32 evaluation in the kernel's order, lane hand-off included (sm_input_grad_ref.emulate_f32), on the GPU
    test's own clouds, parameters and weights.  The device's exp2 is not part of this emulation: its headroom is what the GPU test
    measures.  A ratio above 1 is a finding about the bound, never a number to fit."""
    for n, m, nvecs, scalar_l in sweep_cases(Q, False):
        X, Y, w, mu, l, inv_l = ir.make_case(n, m, d, Q, scalar_l, F32)
        ws = [ir.weights(n, m, nv, F32) for nv in nvecs]
        for (U, A), (ref, bound) in zip(ws, ir.reference_and_bound(w, mu, inv_l, X, Y, ws, F32)):
            emu = ir.emulate_f32(w, mu, inv_l, X, Y, U, A)
            r, i = ir.worst(emu, ref, bound)
            print(f"sm-input-grad-bound-host {n}x{m} d={d} Q={Q} {'iso' if scalar_l else 'ard'} nvec={U.shape[1]:2d}: worst err/bound {r:.3f} at dX[{i // d}, {i % d}]")
            assert r <= 1.0, (n, m, d, Q, scalar_l, U.shape[1], i)


@pytest.mark.parametrize("Q", ir.COMPONENTS)
@pytest.mark.parametrize("d", ir.DIMS)
def test_bound_notices_a_missing_half(d, Q):
    """A result with the sine half dropped, and one with the cosine half dropped, must exceed the bound: in fp64 in every case of the
    sweep (not the sine half at Q = 1, where mu_0 = 0), in fp32 in at least one shape of every (d, Q)."""
    seen32 = {"sin": 0.0, "cos": 0.0}
    low64 = {"sin": np.inf, "cos": np.inf}
    for dt in (F64, F32):
        for n, m, nvecs, scalar_l in sweep_cases(Q, True):
            X, Y, w, mu, l, inv_l = ir.make_case(n, m, d, Q, scalar_l, dt)
            ws = [ir.weights(n, m, nv, dt) for nv in nvecs]
            for (U, A), (ref, bound, hs, hc) in zip(ws, ir.reference_and_bound(w, mu, inv_l, X, Y, ws, dt, halves=True)):
                for half, kept in (("sin", hc), ("cos", hs)):
                    if half == "sin" and Q == 1:
                        continue
                    r = ir.worst(kept, ref, bound)[0]
                    if dt is F64:
                        low64[half] = min(low64[half], r)
                        assert r > 1.0, (half, n, m, d, Q, scalar_l, U.shape[1], r)
                    else:
                        seen32[half] = max(seen32[half], r)
    print(f"sm-input-grad-sensitivity d={d} Q={Q}: fp64 least err/bound without sin {low64['sin']:.3g}, without cos {low64['cos']:.3g}; "
          f"fp32 largest {seen32['sin']:.3g}, {seen32['cos']:.3g}")
    assert seen32["cos"] > 1.0 and (Q == 1 or seen32["sin"] > 1.0)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_device_call(cg, monkeypatch):
    import sys
    gm, dist = sys.modules["covgram.gramian"], sys.modules["covgram.dist"]      # (the package attribute `gramian` is the function)
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(cg._ffi, "lib", no_lib)
    u = np.zeros(4)
    for cls in (gm.Gramian, gm.BlockGramian, gm.HessianGramian, gm.ValueGradientHessianGramian, gm.SymmetricToeplitz, gm.Toeplitz, gm.Circulant,
                gm.KroneckerProduct, gm.SparseGramian, gm.BarnesHutFactorization, gm.LazyMatrixProduct, dist.ShardedGramian):
        with pytest.raises(cg.UnsupportedKernel, match=cls.__name__):
            cg.spectral_mixture_input_gradient(object.__new__(cls), u, u)
    fake = object.__new__(gm.SpectralMixtureGramian)                             # a tree spectral_mixture_spec does not accept
    fake.k = cg.Product((cg.Cosine(0.3), cg.Cosine(0.2), cg.EQ()))
    fake.shape = (4, 4)
    fake.x = np.zeros((4, 1))
    with pytest.raises(cg.UnsupportedKernel, match="Product"):
        cg.spectral_mixture_input_gradient(fake, u, u)
    # spectral_mixture_product: a kernel with a device_spec, points that are not tensors, a gramian() result of another type
    x = torch.zeros((4, 2), dtype=torch.float64, requires_grad=True)
    a = torch.zeros(4, dtype=torch.float64)
    sm = cg.SpectralMixture([1.3, 0.7], [np.array([0.3, -0.2]), 0.4], [0.8, 1.1])
    with pytest.raises(cg.UnsupportedKernel, match="Lengthscale"):
        cg.spectral_mixture_product(cg.Lengthscale(cg.EQ(), 0.7), x, a)
    with pytest.raises(cg.UnsupportedKernel, match="Product"):
        cg.spectral_mixture_product(fake.k, x, a)
    with pytest.raises(cg.UnsupportedKernel, match="StepRangeLen"):
        cg.spectral_mixture_product(cg.SpectralMixture([1.0], [0.3], [0.8]), cg.srange(0.0, 1.0, 4), a)
    with pytest.raises(cg.UnsupportedKernel, match="StepRangeLen"):
        cg.spectral_mixture_product(sm, x, a, y=cg.srange(0.0, 1.0, 4))
    with pytest.raises(cg.UnsupportedKernel, match="str"):                       # not a kernel: named before theta is applied to it
        cg.spectral_mixture_product("EQ", x, a, theta=torch.zeros(3, dtype=torch.float64))
    am = sys.modules["covgram.autograd"]
    monkeypatch.setattr(am, "gramian", lambda k, x, y=None: object.__new__(gm.LazyMatrixSum))
    with pytest.raises(cg.UnsupportedKernel, match="LazyMatrixSum"):
        cg.spectral_mixture_product(sm, x, a)


def test_existing_entries_still_refuse_a_mixture(cg, monkeypatch):
    import sys
    gm = sys.modules["covgram.gramian"]
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(cg._ffi, "lib", no_lib)
    G = object.__new__(gm.SpectralMixtureGramian)
    u = np.zeros(4)
    with pytest.raises(cg.UnsupportedKernel, match="SpectralMixtureGramian"):
        cg.bilinear_input_gradient(G, u, u)
    x = torch.zeros((4, 2), dtype=torch.float64, requires_grad=True)
    sm = cg.SpectralMixture([1.3, 0.7], [np.array([0.3, -0.2]), 0.4], [0.8, 1.1])
    with pytest.raises(cg.UnsupportedKernel):
        cg.gram_product(sm, x, torch.zeros(4, dtype=torch.float64))


def test_abi_symbol_in_header_binding_and_julia(cg):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "covgram.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+covgram_bilinear_input_grad_sm\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m is not None
    assert len(cg._ffi.PROTOTYPES["covgram_bilinear_input_grad_sm"][1]) == len(m.group(1).split(",")) == 10
    jl = open(os.path.join(ROOT, "covariancefunctions.jl_amd", "julia", "CovGram.jl")).read()
    assert ":covgram_bilinear_input_grad_sm, libcovgram" in jl
    assert re.search(r"#define COVGRAM_VERSION 113\b", header) and re.search(r"const ABI_VERSION = 113\b", jl)
    assert cg._ffi.ABI_VERSION == 113
