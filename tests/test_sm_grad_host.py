"""Host side of the hyper-parameter gradients of SpectralMixture Gramians (no GPU): the parameter tree with Cosine leaves and signed
weights, the host chain rules of spectral_mixture_gradient against finite differences, the refusals, and the feasibility of the GPU
test's bound (tests/sm_grad_ref.py)."""
import os
import re

import numpy as np
import pytest

import sm_grad_ref as gr

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fd5(f, h=1e-3):
    return (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)


# ---- parameter tree ------------------------------------------------------------------------------------------------------------------
def test_parameter_tree_round_trip(cg):
    """SpectralMixture with a negative weight, scalar and per-dimension l, a scalar Cosine, and a term with no Cosine."""
    sm = cg.SpectralMixture([1.3, -0.7], [np.array([0.3, -0.2, 0.5]), 0.4], [0.8, np.array([0.7, 1.1, 1.9])])
    k = cg.Sum((sm, cg.Product((cg.Constant(0.6), cg.Lengthscale(cg.EQ(), 2.5)))))
    leaves = cg.hyperparameters(k)
    assert [nm for _, nm, _ in leaves] == ["scale", "mu", "mu", "mu", "l", "scale", "mu", "l", "l", "l", "scale", "l"]
    assert [v for _, _, v in leaves] == [1.3, 0.3, -0.2, 0.5, 0.8, -0.7, 0.4, 0.7, 1.1, 1.9, 0.6, 2.5]
    assert [p for p, _, _ in leaves] == [(0, 0, 0), (0, 0, 1, 0), (0, 0, 1, 1), (0, 0, 1, 2), (0, 0, 2), (0, 1, 0), (0, 1, 1, 0), (0, 1, 2, 0),
                                         (0, 1, 2, 1), (0, 1, 2, 2), (1, 0), (1, 1)]
    assert len({p + (nm,) for p, nm, _ in leaves}) == len(leaves)                # every leaf has its own address
    theta = [v + 0.125 for _, _, v in leaves]
    k2 = cg.with_hyperparameters(k, theta)
    assert [(p, nm) for p, nm, _ in cg.hyperparameters(k2)] == [(p, nm) for p, nm, _ in leaves]
    assert [v for _, _, v in cg.hyperparameters(k2)] == theta
    same = cg.with_hyperparameters(k, [v for _, _, v in leaves])                 # the negative weight survives the rebuild
    assert same.args[0].args[1].args[0].c == -0.7 and same.args[0].args[1].args[0].check is False
    assert same.args[1].args[0].check is True and cg.Constant(2.0).check is True
    x, y = np.array([0.3, -0.2, 0.9]), np.array([-0.1, 0.4, 0.2])
    assert same(x, y) == k(x, y) and k2(x, y) != k(x, y)
    assert same.args[0].args[1].args[1].c.shape == (1,) and same.args[0].args[0].args[1].c.shape == (3,)   # scalar and vector Cosine
    for a, b in ((cg.spectral_mixture_spec(k, 3), cg.spectral_mixture_spec(same, 3)),):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    with pytest.raises(cg.DomainError):                                          # a checked Constant still refuses a negative value
        cg.with_hyperparameters(cg.Product((cg.Constant(1.0), cg.EQ())), [-1.0])


def test_existing_leaves_keep_their_names_and_order(cg):
    k = cg.Sum((1.5 * cg.Lengthscale(cg.EQ(), 0.7), cg.Power(0.5 * cg.RQ(0.37), 2), 0.3 * cg.InverseMultiQuadratic(0.6)))
    assert [(nm, v) for _, nm, v in cg.hyperparameters(k)] == [("scale", 1.5), ("l", 0.7), ("scale", 0.5), ("alpha", 0.37), ("scale", 0.3), ("c", 0.6)]


# ---- the host chain rules ------------------------------------------------------------------------------------------------------------
def host_form(k, X, Y, W):
    return sum(W[i, j] * k(X[i], Y[j]) for i in range(X.shape[0]) for j in range(Y.shape[0]))


def chain_rule_case(cg, k, d=3):
    """The point counts and the tolerance of test_bilin_grad_host.chain_rule_case; `out` is the fp64 reference of the device's numbers."""
    rng = np.random.default_rng(5)
    X = 0.8 * rng.standard_normal((12, d)) + 0.2; Y = 0.8 * rng.standard_normal((9, d))
    Y[0] = X[3]
    W = rng.standard_normal((12, 9))
    w, mu, inv_l = cg.spectral_mixture_spec(k, d)
    out = gr.reference(w, mu, inv_l, X, Y, W, np.eye(9))
    value, grad = cg.spectral_mixture_chain_rules(k, out, d)
    assert abs(value - host_form(k, X, Y, W)) <= 1e-12 * np.abs(W).sum()
    theta = [v for _, _, v in cg.hyperparameters(k)]
    assert len(grad) == len(theta)
    for p in range(len(theta)):
        def f(h):
            t = list(theta); t[p] += h
            return host_form(cg.with_hyperparameters(k, t), X, Y, W)
        fd = fd5(f)
        print(f"sm-grad-host chain rule {cg.hyperparameters(k)[p][:2]}: {grad[p]:.12e} against {fd:.12e}")
        assert abs(grad[p] - fd) <= 1e-8 * max(abs(fd), 1.0), (p, grad[p], fd)


def test_chain_rules_spectral_scalar_l(cg):
    chain_rule_case(cg, cg.SpectralMixture([1.3, -0.7], [np.array([0.3, -0.2, 0.5]), np.array([0.0, 0.6, -0.4])], [0.8, 1.4]))


def test_chain_rules_spectral_ard_l(cg):
    chain_rule_case(cg, cg.SpectralMixture([1.3, -0.7], [np.array([0.3, -0.2, 0.5]), 0.4], [np.array([0.7, 1.1, 1.9]), np.array([1.2, 0.6, 0.9])]))


def test_chain_rules_scaled_input_factor(cg):
    U = np.array([1.4, 0.6, 0.9])
    chain_rule_case(cg, cg.Product((cg.Constant(0.9), cg.Cosine(np.array([0.2, 0.5, -0.3])), cg.ScaledInputKernel(cg.EQ(), U))))
    chain_rule_case(cg, cg.Sum((cg.Product((cg.Constant(-0.8, False), cg.ScaledInputKernel(cg.Lengthscale(cg.EQ(), 0.8), U))),
                                cg.Product((cg.Cosine(0.3), cg.EQ())))))


def test_chain_rules_two_constants_in_a_term(cg):
    chain_rule_case(cg, cg.Sum((cg.Product((cg.Constant(1.2), cg.Constant(-0.5, False), cg.Cosine(0.4), cg.Lengthscale(cg.EQ(), 0.9))),
                                cg.Product((cg.Constant(0.7), cg.Lengthscale(cg.EQ(), 1.6), cg.Constant(1.1), cg.Constant(0.4))))))


def test_chain_rules_nested_lengthscales(cg):
    chain_rule_case(cg, cg.Product((cg.Constant(1.1), cg.Cosine(np.array([0.3, 0.1, -0.2])), cg.Lengthscale(cg.Lengthscale(cg.EQ(), 0.8), 1.5),
                                    cg.ARD(cg.EQ(), np.array([2.0, 1.3, 0.9])))))
    chain_rule_case(cg, cg.SpectralMixture([0.9], [0.7], [0.6]), d=1)


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
            cg.spectral_mixture_gradient(object.__new__(cls), u, u)
    fake = object.__new__(gm.SpectralMixtureGramian)                             # a tree spectral_mixture_spec does not accept
    fake.k = cg.Product((cg.Cosine(0.3), cg.Cosine(0.2), cg.EQ()))
    fake.shape = (4, 4)
    fake.x = np.zeros((4, 1))
    with pytest.raises(cg.UnsupportedKernel, match="Product"):
        cg.spectral_mixture_gradient(fake, u, u)
    # the three entries that refuse mixtures keep doing so
    G = object.__new__(gm.SpectralMixtureGramian)
    with pytest.raises(cg.UnsupportedKernel, match="SpectralMixtureGramian"):
        cg.bilinear_gradient(G, u, u)
    with pytest.raises(cg.UnsupportedKernel, match="SpectralMixtureGramian"):
        cg.bilinear_input_gradient(G, u, u)
    with pytest.raises(cg.UnsupportedKernel, match="SymmetricToeplitz"):
        cg.inv_quad_logdet_gradient(object.__new__(gm.SymmetricToeplitz), None)


def test_abi_symbol_in_header_binding_and_julia(cg):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "covgram.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+covgram_bilinear_grad_sm\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m is not None
    assert len(cg._ffi.PROTOTYPES["covgram_bilinear_grad_sm"][1]) == len(m.group(1).split(",")) == 10
    jl = open(os.path.join(ROOT, "covariancefunctions.jl_amd", "julia", "CovGram.jl")).read()
    assert ":covgram_bilinear_grad_sm, libcovgram" in jl
    assert re.search(r"#define COVGRAM_VERSION 113\b", header) and re.search(r"const ABI_VERSION = 113\b", jl)


# ---- the reference itself ------------------------------------------------------------------------------------------------------------
def test_reference_zero_distance_pair():
    """A pair with r = 0 adds exactly W_ij to the first output of each component and exactly 0 to the others."""
    X, Y, w, mu, l, inv_l = gr.make_case(63, 193, 3, 3, False, F64)
    e1 = np.zeros((63, 1)); e2 = np.zeros((193, 1))
    Xc = X.copy(); Xc[5] = Y[7]
    e1[5] = 1.5; e2[7] = -2.0
    out = gr.reference(w, mu, inv_l, Xc, Y, e1, e2).reshape(3, 7)
    assert np.all(out[:, 0] == -3.0) and np.all(out[:, 1:] == 0.0)


# ---- the GPU test's bound is feasible ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", gr.COMPONENTS)
@pytest.mark.parametrize("d", gr.DIMS)
def test_fp32_emulation_within_the_gpu_bound(d, Q):
    """An exactly rounded fp32 evaluation in the kernel's order, lane hand-off included (sm_grad_ref.emulate_f32), on the GPU test's own
    clouds, parameters and weights.  The device's exp2 is not part of this emulation: its headroom is what the GPU test measures.  A
    ratio above 1 is a finding about the bound, never a number to fit.  (Every shape, dimension, component count and both lengthscale
    forms; one column count per shape; at Q = 32 the two larger shapes take one lengthscale form each.)"""
    for (n, m), nvecs in zip(gr.SHAPES, ((32,), (1,), (3,), (17,))):
        for scalar_l in ((True, False) if Q < 32 or n * m < 1000 else ((n == 63),)):
            X, Y, w, mu, l, inv_l = gr.make_case(n, m, d, Q, scalar_l, F32)
            ws = [gr.weights(n, m, nv, F32) for nv in nvecs]
            for (U, A), (ref, bound) in zip(ws, gr.reference_and_bound(w, mu, inv_l, X, Y, ws, F32)):
                emu = gr.emulate_f32(w, mu, inv_l, X, Y, U, A)
                r, i = gr.worst(emu, ref, bound)
                kind = ["dw", "dmu", "E"][0 if i % (1 + 2 * d) == 0 else (1 if i % (1 + 2 * d) <= d else 2)]
                print(f"sm-grad-bound-host {n}x{m} d={d} Q={Q} {'iso' if scalar_l else 'ard'} nvec={U.shape[1]:2d}: worst err/bound {r:.3f} at out[{i}] ({kind})")
                assert r <= 1.0, (n, m, d, Q, scalar_l, U.shape[1], i)
