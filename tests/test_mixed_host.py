"""CPU tier of the scalar Gramians of mixed-trait composites (covgram_mvm_mixed / covgram_matrix_mixed, csrc/mixed_mvm.hpp):
  * the lowering kernels.mixed_spec: per-factor traits, the leaves the gradient kernels refuse, field-by-field equality with
    mixed_gradient_spec, the limits, the Cosine refusal by name, and the rule gramian() picks MixedGramian by;
  * both symbols in the header, the ctypes prototypes, the library and the Julia shim;
  * the fp64 restatement tests/mixed_ref.py against the kernel objects' own __call__, and the majorant's derivatives against central
    differences;
  * bound feasibility: a float32 emulation of the device's formation order on the inputs of tests/test_gpu_mixed.py stays within 0.25
    of that test's fp32 bound, 1e-5 of the majorant (BASELINE.json's contract), entry by entry;
  * the kernel refusals of the two C entries, which come before any device call (no context exists on this tier).  The refusals of
    nrhs < 1 and lda < m need point handles, hence a device: tests/test_gpu_mixed.py has them."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import grad_mixed_ref as GR
import mixed_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_NAMES = ["eq+dot", "eq+(dot^2+1)", "eq*(dot^2+1)", "dot*dot", "maternp2+dot^2+nn", "nn(0.5)*ls(eq,2)", "(eq*dot)^2", "eq*dot zero"]   # grad_mixed_ref.kernels
NAMES = GRAD_NAMES + R.EXTRA


def _factors(c):
    out, fi = [], 0
    for t in range(c.nterms):
        out.append([c.factors[fi + q] for q in range(c.nfactors[t])])
        fi += c.nfactors[t]
    return out


def _fields(c):
    f = lambda k: tuple(getattr(k, name) for name, _ in type(k)._fields_)
    return (f(c.head), c.nterms, list(c.nfactors), [f(q) for t in _factors(c) for q in t])


# ---- lowering --------------------------------------------------------------------------------------------------------------------------
def test_mixed_spec_lowers_every_leaf_on_its_own_trait(cg):
    f = cg._ffi
    fams = lambda c: sorted((t[0].family, t[0].trait) for t in _factors(c))
    assert fams(cg.mixed_spec(cg.EQ() + cg.Dot())) == [(f.EQ, f.ISOTROPIC), (f.DOT, f.DOTPRODUCT)]
    c = cg.mixed_spec(cg.MaternP(2) + cg.Dot() ** 2 + cg.NeuralNetwork(0.25))
    fam = {t[0].family: t[0] for t in _factors(c)}
    assert set(fam) == {f.MATERNP, f.DOT, f.NEURALNETWORK}
    assert fam[f.MATERNP].p == 2 and fam[f.DOT].power == 2 and fam[f.NEURALNETWORK].param == 0.25 and fam[f.NEURALNETWORK].trait == 0
    # the leaves the gradient lowering refuses: singular at zero distance, or without a closed-form jet
    assert fams(cg.mixed_spec(cg.Exponential() + cg.Dot())) == [(f.EXP, f.ISOTROPIC), (f.DOT, f.DOTPRODUCT)]
    (term,) = _factors(cg.mixed_spec(cg.GammaExponential(1.5) * cg.Dot()))
    assert sorted((q.family, q.trait, q.param) for q in term) == [(f.GAMMAEXP, f.ISOTROPIC, 1.5), (f.DOT, f.DOTPRODUCT, 0.0)]
    c = cg.mixed_spec(cg.MaternP(0) + cg.Dot())
    assert fams(c) == [(f.MATERNP, f.ISOTROPIC), (f.DOT, f.DOTPRODUCT)] and _factors(c)[0][0].p == 0
    c = cg.mixed_spec(cg.Matern(2.3) + cg.Dot())
    assert fams(c) == [(f.DOT, f.DOTPRODUCT), (f.MATERN, f.ISOTROPIC)] and _factors(c)[0][0].param == 2.3
    for k in (cg.EQ() + cg.Dot(), cg.Exponential() + cg.Dot(), cg.GammaExponential(1.5) * cg.Dot(), cg.MaternP(0) + cg.Dot(),
              cg.Matern(2.3) + cg.Dot(), cg.MaternP(2) + cg.Dot() ** 2 + cg.NeuralNetwork()):
        assert cg.device_spec(k) is None                                  # unchanged: GenericInput has no common-trait composite
        assert cg.mixed_spec(k).head.family == f.COMPOSITE and cg.mixed_spec(k).head.trait == 0


@pytest.mark.parametrize("name", GRAD_NAMES)
def test_mixed_spec_equals_the_gradient_lowering_field_by_field(cg, name):
    k = GR.kernels(cg)[name]
    a, b = cg.mixed_spec(k), cg.mixed_gradient_spec(k)
    assert a is not None and b is not None and _fields(a) == _fields(b)
    assert _fields(cg.require_mixed_spec(k)) == _fields(a)


def test_limits_and_the_cosine_refusal(cg):
    f = cg._ffi
    many = cg.EQ()
    for i in range(f.COMPOSITE_MAX_TERMS):
        many = many + cg.Lengthscale(cg.EQ(), 2.0 + i) * cg.Dot()
    assert cg.mixed_spec(many) is None
    with pytest.raises(cg.UnsupportedKernel, match=r"9 terms and 17 factors"):
        cg.require_mixed_spec(many)
    k = cg.EQ() * cg.Cosine([1.0, 2.0])
    assert cg.mixed_spec(k) is None
    with pytest.raises(cg.UnsupportedKernel, match=r"CosineKernel.*spectral mixtures"):
        cg.require_mixed_spec(k)
    with pytest.raises(cg.UnsupportedKernel, match="not a kernel expression"):
        cg.require_mixed_spec(3.0)
    # the order rules of the gradient lowering: the constant where it first stood, a cancelling expression the one term 0
    c = cg.mixed_spec(cg.EQ() + 2.0 + cg.Dot())
    assert [[q.family for q in t] for t in _factors(c)] == [[f.EQ], [f.CONSTANT], [f.DOT]]
    c = cg.mixed_spec(cg.EQ() + cg.Constant(-1.0, False) * cg.EQ())
    assert [[(q.family, q.scale) for q in t] for t in _factors(c)] == [[(f.CONSTANT, 0.0)]]


def test_the_rule_gramian_picks_the_mixed_operator_by(cg):
    """gramian() returns MixedGramian exactly when device_spec(k) is None, spectral_mixture_spec(k) is None and mixed_spec(k) is not
    (a Gramian needs a device to exist: tests/test_gpu_mixed.py checks the classes themselves); every kernel with a route keeps it."""
    mixed = lambda k: cg.device_spec(k) is None and cg.spectral_mixture_spec(k, 2) is None and cg.mixed_spec(k) is not None
    names = {n for n, k in R.kernels(cg).items() if mixed(k)}
    assert names == set(R.kernels(cg)) - {"dot*dot"}                     # Dot * Dot has a common trait: its old route
    for k in (cg.EQ(), cg.EQ() * cg.RQ(2.0), cg.Dot() ** 2 + 1, cg.SM([1.0, 0.5], [[0.3, 0.1], [0.2, 0.4]], [[1.0, 2.0], [0.5, 0.7]])):
        assert not mixed(k)
    assert issubclass(cg.MixedGramian, cg.LazyOperator) and not issubclass(cg.MixedGramian, cg.Gramian)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_both_symbols_everywhere(cg):
    header = open(os.path.join(ROOT, "include", "covgram.h")).read()
    jl = open(os.path.join(ROOT, "covariancefunctions.jl_amd", "julia", "CovGram.jl")).read()
    lib = cg._ffi.lib()
    for name in ("covgram_mvm_mixed", "covgram_matrix_mixed"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
        assert name in cg._ffi.PROTOTYPES and hasattr(lib, name)
        assert re.search(r"ccall\(\(:" + name + r", libcovgram\)", jl)
    assert len(cg._ffi.PROTOTYPES["covgram_mvm_mixed"][1]) == 12 and len(cg._ffi.PROTOTYPES["covgram_matrix_mixed"][1]) == 7
    assert lib.covgram_version() == 113 and cg._ffi.ABI_VERSION == 113


def test_kernel_refusals_come_before_any_device_call(cg):
    """No context, no points: what the two entries refuse about the KERNEL is answered on the host, with its own message."""
    f = cg._ffi
    lib = f.lib()
    good = lambda: cg.mixed_spec(cg.EQ() + cg.Dot() * cg.NeuralNetwork(0.5))

    def both(spec, status, word):
        for call in (lambda: lib.covgram_mvm_mixed(None, C.byref(spec), None, None, None, 0, None, 0, 1, 1.0, 0.0, f.DEVICE),
                     lambda: lib.covgram_matrix_mixed(None, C.byref(spec), None, None, None, 0, f.DEVICE)):
            assert call() == status
            assert re.search(word, lib.covgram_last_error().decode()), lib.covgram_last_error()

    c = good(); c.head.family = f.EQ
    both(c, f.EINVAL, "takes a covgram_kernel_composite")                   # wrong head family
    c = good(); c.nterms = 0
    both(c, f.EUNSUPPORTED, "0 terms")                                       # zero terms
    c = good(); [q for q in c.factors if q.family == f.NEURALNETWORK][0].param = -0.5
    both(c, f.EINVAL, "sigma = -0.5 is negative")
    c = good(); [q for q in c.factors if q.family == f.DOT][0].lengthscale = 2.0
    both(c, f.EINVAL, "Lengthscale applies to isotropic kernels only")
    c = good(); [q for q in c.factors if q.family == f.EQ][0].trait = f.DOTPRODUCT
    both(c, f.EINVAL, "trait 2 does not match family 0")                     # every factor is validated on its own trait
    c = good(); c.factors[0].power = 0
    both(c, f.EINVAL, "Power exponent must be >= 1")
    # a valid kernel gets as far as the missing context; the gradient entry still refuses the singular leaves the scalar entries take
    c = cg.mixed_spec(cg.Exponential() + cg.Dot())
    both(c, f.EINVAL, "NULL argument")
    assert lib.covgram_mvm_mixed(None, None, None, None, None, 0, None, 0, 1, 1.0, 0.0, f.DEVICE) == f.EINVAL


def test_type_named_refusals_before_any_device_call(cg, monkeypatch):
    """Every function that takes a Gramian and has no mixed path names MixedGramian, without touching the library."""
    import sys
    import torch
    gm, dist = sys.modules["covgram.gramian"], sys.modules["covgram.dist"]
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(cg._ffi, "lib", no_lib)
    G = object.__new__(gm.MixedGramian)
    G.k = cg.EQ() + cg.Dot()
    u = np.zeros(4)
    for fn in (lambda: cg.sparse(G), lambda: cg.BarnesHutFactorization(G), lambda: cg.pivoted_cholesky(G, 4), lambda: cg.bilinear_gradient(G, u, u),
               lambda: cg.bilinear_input_gradient(G, u, u), lambda: G.sym_partial_(None, None, 0, 2)):
        with pytest.raises(cg.UnsupportedKernel, match="MixedGramian"):
            fn()
    assert G.sym_partial_supported(2) is False
    a = torch.zeros(4, dtype=torch.float64)
    x = torch.zeros((4, 2), dtype=torch.float64, requires_grad=True)
    with pytest.raises(cg.UnsupportedKernel, match="gram_product.*MixedGramian"):
        cg.gram_product(G, x, a)
    with pytest.raises(cg.UnsupportedKernel, match="gram_product.*MixedGramian"):
        cg.gram_product(cg.EQ() + cg.Dot(), x, a)
    with pytest.raises(cg.UnsupportedKernel, match="ShardedGramian.*MixedGramian"):
        dist.ShardedGramian(cg.EQ() + cg.Dot(), x.detach())


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_reference_matrix_is_the_kernel_objects_own_call(cg, oracle, name):
    assert list(R.kernels(cg)) == NAMES and list(GR.kernels(cg)) == GRAD_NAMES
    k = R.kernels(cg)[name]
    X, Y = R.clouds32(name, 7, 5, 3, False)
    M = R.matrix(cg, oracle, k, X, Y)
    for i in range(7):
        for j in range(5):
            ref = float(k(X[i], Y[j]))
            assert abs(M[i, j] - ref) <= 1e-13 * max(1.0, abs(ref)), (name, i, j, M[i, j], ref)
    # x = y: the diagonal has r = 0 (the Taylor / limit branches of the singular leaves)
    M = R.matrix(cg, oracle, k, X, X)
    for i in range(7):
        assert abs(M[i, i] - float(k(X[i], X[i]))) <= 1e-13 * max(1.0, abs(M[i, i])), (name, i)
    assert np.all(R.majorant(cg, oracle, k, X, X) >= np.abs(M) * (1 - 1e-15))


def test_majorant_derivatives_match_central_differences(cg, oracle):
    u = np.array([0.07, 0.4, 1.3, 3.1, 6.5])
    for k in (cg.EQ(), cg.Exponential(), cg.GammaExponential(1.5), cg.MaternP(0), cg.MaternP(2), cg.RQ(2.0), cg.Cauchy(), cg.Matern(2.3), cg.Dot(),
              cg.ExponentialDot()):
        h = 1e-5 * u
        d = R.leaf_profile(cg, oracle, k, u)[1]
        fd = (R.leaf_profile(cg, oracle, k, u + h)[0] - R.leaf_profile(cg, oracle, k, u - h)[0]) / (2 * h)
        assert np.abs(d - fd).max() <= 1e-8 * np.abs(d).max(), (type(k).__name__, d, fd)
    p, q, s = np.array([0.3, -0.8, 1.1]), np.array([0.9, 1.4, 2.0]), np.array([0.5, 2.2, 1.7])
    for sigma in (0.0, 0.5):
        v, vp, vq, vs = R.nn_partials(sigma, p, q, s)
        h = 1e-6
        for got, (dp, dq, ds) in ((vp, (h, 0, 0)), (vq, (0, h, 0)), (vs, (0, 0, h))):
            fd = (R.nn_partials(sigma, p + dp, q + dq, s + ds)[0] - R.nn_partials(sigma, p - dp, q - dq, s - ds)[0]) / (2 * h)
            assert np.abs(got - fd).max() <= 1e-8, (sigma, got, fd)
    # the composite rule on one pair: K̄ of EQ * (Dot^2 + 1) multiplied out by hand
    X, Y = np.array([[0.3, -0.5]]), np.array([[0.7, 0.2]])
    r2, pd, pbar = 0.16 + 0.49, 0.21 - 0.10, 0.21 + 0.10
    e = math.exp(-r2 / 2)
    want = (e * pd * pd + e * r2 / 2 * pd * pd + e * 2 * abs(pd) * pbar) + (e + e * r2 / 2)
    assert abs(R.majorant(cg, oracle, cg.EQ() * (cg.Dot() ** 2 + 1), X, Y)[0, 0] - want) <= 1e-15


# ---- bound feasibility of the GPU test's inputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(str(v) for v in s[:3]))
def test_fp32_bound_is_feasible_on_the_gpu_inputs(cg, oracle, shape):
    n, m, d, same, _ = shape
    tiny = np.finfo(np.float64).tiny
    for name, k in R.kernels(cg).items():
        if shape not in R.shapes_of(name):
            continue
        X, Y = R.clouds32(name, n, m, d, same)
        a = R.weights32(Y.shape[0])
        ref, Kb = R.matrix(cg, oracle, k, X, Y), R.majorant(cg, oracle, k, X, Y)
        em = float((np.abs(R.matrix_float32(cg, oracle, k, X, Y) - ref) / (Kb + tiny)).max())
        dv = np.abs(R.mvm_float32(cg, oracle, k, X, Y, a) - ref @ a)
        with np.errstate(divide="ignore", invalid="ignore"):
            ev = float(np.where(dv == 0, 0.0, dv / (Kb @ np.abs(a))).max())            # (an exact zero against a zero bound is no error)
        print(f"{name:20s} fp32 emulation: worst err / majorant: matrix {em:.2e}, mvm {ev:.2e}")
        assert max(em, ev) <= 0.25 * 1e-5, (name, em, ev)
