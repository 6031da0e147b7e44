"""CPU tier of the hyper-parameter gradients of mixed-trait composites (covgram_bilinear_grad_mixed):
  * the "sigma" leaf of hyperparameters / with_hyperparameters;
  * the lowering kernels.require_mixed_parameter_spec and its chain-rule matrix J: J @ reference_out against 5-point finite differences
    of the host form Σ W_ij k(x_i, y_j) evaluated by the kernel OBJECTS' own __call__, and Σ c_t out[t] against that form itself;
  * the provenance cases: Polynomial(3, σ), a Power over a scaled leaf, two equal-valued leaves with coefficients +1 and −1, a Constant 0;
  * refusals by name without touching the library;
  * the entry in the header, the ctypes prototypes, the library and the Julia shim;
  * bound feasibility: an exactly rounded fp32 evaluation in the kernel's order stays within 0.1 of the GPU test's bound on that test's clouds;
  * bound sensitivity: a dropped derivative, or one output moved by 1e-3 of its majorant sum, exceeds the fp32 bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mixed_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["1.5ls(eq,.7)+.5dot", "ls(eq,.8)*(dot^2+1)", ".7ls(maternp2,1.3)+.2poly(3,.4)", "ls(rq(.37),1.2)*nn(.5)+.3imq(.6)", "nn(.3)+.1expdot",
         "ls(exp,.9)*dot", "gammaexp(1.5)*dot+1", "ls(eq,.7)*ls(rq(.5),1.4)"]


def provenance_cases(cg):
    eq = lambda: cg.Lengthscale(cg.EQ(), 0.7)
    return {
        "poly(3,.4)": cg.Polynomial(3, 0.4),
        "(.5ls(rq(.9),1.1))^2*dot": cg.Power(0.5 * cg.Lengthscale(cg.RQ(0.9), 1.1), 2) * cg.Dot(),
        "eq-eq": cg.Sum((cg.Constant(1.0) * eq(), cg.Constant(-1.0, check=False) * eq())),
        "0*eq+dot": cg.Constant(0.0, check=False) * eq() + cg.Dot(),       # (unchecked: the finite differences step below 0)
        "ls(ls(imq(.6),2),.9)*nn(.2)^2": cg.Lengthscale(cg.Lengthscale(cg.InverseMultiQuadratic(0.6), 2.0), 0.9) * cg.NN(0.2) ** 2,
    }


def host_form(k, X, Y, W):
    return float(sum(W[i, j] * float(k(X[i], Y[j])) for i in range(X.shape[0]) for j in range(Y.shape[0])))


def fd5(f, h):
    return (f(-2 * h) - 8 * f(-h) + 8 * f(h) - f(2 * h)) / (12 * h)


def small_case(name):
    X, Y = R.clouds(name, 6, 5, 3, False, seed=3)
    U, A = R.weights_for(6, 5, 2)
    return X, Y, U, A, U @ A.T


# ---- the parameter tree ----------------------------------------------------------------------------------------------------------------
def test_sigma_leaf_round_trip(cg):
    k = 1.5 * cg.Lengthscale(cg.RQ(0.37), 1.2) * cg.NN(0.5) + cg.NN(0.25) ** 2
    leaves = cg.hyperparameters(k)
    assert [nm for _, nm, _ in leaves] == ["scale", "alpha", "l", "sigma", "sigma"]
    assert [v for _, _, v in leaves] == [1.5, 0.37, 1.2, 0.5, 0.25]
    assert len({p + (nm,) for p, nm, _ in leaves}) == len(leaves)
    k2 = cg.with_hyperparameters(k, [2.0, 0.5, 0.9, 0.75, 0.125])
    assert [v for _, _, v in cg.hyperparameters(k2)] == [2.0, 0.5, 0.9, 0.75, 0.125]
    x, y = np.array([0.3, -0.2]), np.array([0.1, 0.4])
    ref = 2.0 * cg.Lengthscale(cg.RQ(0.5), 0.9)(x, y) * cg.NN(0.75)(x, y) + cg.NN(0.125)(x, y) ** 2
    assert abs(k2(x, y) - ref) <= 1e-15
    # the existing leaves keep their names and order
    old = 1.5 * cg.Lengthscale(cg.EQ(), 0.7) + 0.3 * cg.InverseMultiQuadratic(0.6)
    assert [nm for _, nm, _ in cg.hyperparameters(old)] == ["scale", "l", "scale", "c"]


# ---- lowering and chain rules -------------------------------------------------------------------------------------------------------------
def all_cases(cg):
    ks = dict(R.kernels(cg))
    ks.update(provenance_cases(cg))
    return ks


@pytest.mark.parametrize("name", NAMES + ["poly(3,.4)", "(.5ls(rq(.9),1.1))^2*dot", "eq-eq", "0*eq+dot", "ls(ls(imq(.6),2),.9)*nn(.2)^2"])
def test_chain_rules_against_finite_differences_of_the_kernel_objects(cg, oracle, name):
    assert list(R.kernels(cg)) == NAMES
    k = all_cases(cg)[name]
    X, Y, U, A, W = small_case(name)
    comp, J = cg.require_mixed_parameter_spec(k)
    theta = np.array([v for _, _, v in cg.hyperparameters(k)])
    assert J.shape == (len(theta), 24) and J.dtype == np.float64
    out, _ = R.reference_and_bound(cg, oracle, comp, X, Y, U, A, np.float64)
    value = sum(c * out[t] for t, (c, _) in enumerate(R.terms_of(comp)))
    host = host_form(k, X, Y, W)
    assert abs(value - host) <= 1e-12 * max(abs(host), 1.0), (name, value, host)
    grad = J @ out
    for i in range(len(theta)):
        def f(h):
            th = theta.copy(); th[i] += h
            return host_form(cg.with_hyperparameters(k, th), X, Y, W)
        fd = fd5(f, 1e-3 * max(abs(theta[i]), 0.1))
        assert abs(grad[i] - fd) <= 1e-8 * max(abs(fd), 1.0), (name, i, cg.hyperparameters(k)[i], grad[i], fd)


def test_provenance_merges_copies_not_equal_numbers(cg):
    f = cg._ffi
    comp, J = cg.require_mixed_parameter_spec(cg.Polynomial(3, 0.4))            # Dot³ + 3σ Dot² + 3σ² Dot + σ³
    terms = R.terms_of(comp)
    assert comp.nterms == 4 and sorted(fs[0]["power"] if fs else 0 for _, fs in terms) == [0, 1, 2, 3]
    coef = {(fs[0]["power"] if fs else 0): c for c, fs in terms}
    assert np.allclose([coef[3], coef[2], coef[1], coef[0]], [1.0, 3 * 0.4, 3 * 0.16, 0.064], rtol=1e-15)
    row = {(fs[0]["power"] if fs else 0): J[0, t] for t, (_, fs) in enumerate(terms)}
    assert np.allclose([row[3], row[2], row[1], row[0]], [0.0, 3.0, 6 * 0.4, 3 * 0.16], rtol=1e-15)
    comp, J = cg.require_mixed_parameter_spec(provenance_cases(cg)["(.5ls(rq(.9),1.1))^2*dot"])
    assert comp.nterms == 1 and comp.nfactors[0] == 2
    rq = comp.factors[0]
    assert (rq.family, rq.power, rq.lengthscale, rq.param, rq.scale) == (f.RQ, 2, 1.1, 0.9, 0.25)
    assert J[0, 0] == 1.0 and J[1, 16] == 1.0 and J[2, 8] == -2.0 / 1.1 and np.count_nonzero(J) == 3
    # equal numbers in different leaves: two terms, two lengthscale rows; mixed_spec cancels the same expression to the zero term
    k = provenance_cases(cg)["eq-eq"]
    comp, J = cg.require_mixed_parameter_spec(k)
    assert comp.nterms == 2 and [c for c, _ in R.terms_of(comp)] == [1.0, -1.0]
    names = [nm for _, nm, _ in cg.hyperparameters(k)]
    assert names == ["scale", "l", "scale", "l"]
    assert J[1, 8] == -2.0 / 0.7 and J[3, 9] == -2.0 / 0.7 and J[0, 0] == 1.0 and J[2, 1] == 1.0
    assert cg.mixed_spec(k).nterms == 1 and cg.mixed_spec(k).factors[0].family == f.CONSTANT
    # a Constant equal to 0 keeps its derivative
    k = provenance_cases(cg)["0*eq+dot"]
    comp, J = cg.require_mixed_parameter_spec(k)
    assert comp.nterms == 2 and R.terms_of(comp)[0][0] == 0.0 and J[0, 0] == 1.0


def test_refusals_by_name_without_the_library(cg, monkeypatch):
    import sys
    import torch
    gm, dist = sys.modules["covgram.gramian"], sys.modules["covgram.dist"]
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(cg._ffi, "lib", no_lib)
    u = np.zeros(4)
    nine_terms = cg.Sum(tuple(cg.Lengthscale(cg.EQ(), 1.0 + i) for i in range(8)) + (cg.Dot(),))
    nine_factors = cg.Product(tuple(cg.Lengthscale(cg.EQ(), 1.0 + i) for i in range(8)) + (cg.Dot(),))
    for k, word in ((nine_terms, "9 terms"), (nine_factors, "9 factors"), (cg.Matern(2.3) + cg.Dot(), r"Matern\(ν = 2.3\)"),
                    (cg.CosineKernel(np.array([0.3])) * cg.Dot(), "CosineKernel"), (cg.VerticalRescaling(cg.EQ(), lambda x: x) + cg.Dot(), "VerticalRescaling")):
        with pytest.raises(cg.UnsupportedKernel, match=word):
            cg.require_mixed_parameter_spec(k)
        assert cg.mixed_parameter_spec(k) is None
        G = object.__new__(gm.MixedGramian)
        G.k = k
        with pytest.raises(cg.UnsupportedKernel, match=word):
            cg.mixed_bilinear_gradient(G, u, u)
        with pytest.raises(cg.UnsupportedKernel, match=word):
            cg.inv_quad_logdet_gradient(G, torch.zeros(4))
    ard = object.__new__(gm.Gramian)
    ard.k = cg.EQ()
    ard.scaled_input = cg.ARD(cg.EQ(), [0.5, 2.0])
    with pytest.raises(cg.UnsupportedKernel, match="ScaledInputKernel"):
        cg.mixed_bilinear_gradient(ard, u, u)
    for cls in (gm.SpectralMixtureGramian, gm.Toeplitz, gm.SymmetricToeplitz, gm.BlockGramian, gm.MixedBlockGramian, gm.KroneckerProduct, gm.SparseGramian,
                gm.BarnesHutFactorization, dist.ShardedGramian):
        with pytest.raises(cg.UnsupportedKernel, match=cls.__name__):
            cg.mixed_bilinear_gradient(object.__new__(cls), u, u)
    # bilinear_gradient keeps refusing the mixed Gramian
    G = object.__new__(gm.MixedGramian)
    G.k = cg.EQ() + cg.Dot()
    with pytest.raises(cg.UnsupportedKernel, match="MixedGramian"):
        cg.bilinear_gradient(G, u, u)


def test_entry_is_declared_bound_and_exported(cg):
    header = open(os.path.join(ROOT, "include", "covgram.h")).read()
    jl = open(os.path.join(ROOT, "covariancefunctions.jl_amd", "julia", "CovGram.jl")).read()
    lib = cg._ffi.lib()
    name = "covgram_bilinear_grad_mixed"
    assert re.search(r"\bint\s+" + name + r"\s*\(", header) and re.search(r"#define\s+COVGRAM_MIXED_GRAD_NOUT\s+24\b", header)
    assert name in cg._ffi.PROTOTYPES and hasattr(lib, name) and len(cg._ffi.PROTOTYPES[name][1]) == 11
    assert re.search(r"ccall\(\(:" + name + r", libcovgram\)", jl)
    assert cg._ffi.MIXED_GRAD_NOUT == 24 == cg._ffi.COMPOSITE_MAX_TERMS + 2 * cg._ffi.COMPOSITE_MAX_FACTORS
    assert lib.covgram_version() == 113 and cg._ffi.ABI_VERSION == 113
    # the kernel's refusals need no context: Matern(nu) by name, a plain covgram_kernel head
    f = cg._ffi
    out = (C.c_double * 24)()
    c = cg.mixed_spec(cg.Matern(2.3) + cg.Dot())
    assert lib.covgram_bilinear_grad_mixed(None, C.byref(c), None, None, None, 0, None, 0, 1, out, f.DEVICE) == f.EINVAL      # no ctx
    c = cg.mixed_spec(cg.EQ() + cg.Dot())
    assert lib.covgram_bilinear_grad_mixed(None, C.byref(c), None, None, None, 0, None, 0, 1, out, f.DEVICE) == f.EINVAL
    assert re.search("NULL argument", lib.covgram_last_error().decode())


# ---- the GPU test's bound ---------------------------------------------------------------------------------------------------------------------
FEASIBILITY_SHAPES = [(130, 130, 3, True, {}), (70, 1100, 5, False, {}), (70, 1100, 5, False, {"jsplit": 3}), (100, 37, 17, False, {}), (33, 70, 64, False, {}),
                      (1, 1, 1, False, {})]


@pytest.mark.parametrize("name", NAMES)
def test_fp32_emulation_within_a_tenth_of_the_gpu_bound(cg, oracle, name):
    """A condition on the clouds and the bound, not a measurement of the device: its exp / log / pow / asin are not emulated."""
    assert FEASIBILITY_SHAPES == R.SHAPES
    k = R.kernels(cg)[name]
    comp, _ = cg.require_mixed_parameter_spec(k)
    for n, m, d, same, opts in R.SHAPES:
        X, Y = R.clouds(name, n, m, d, same)
        U, A = R.weights_for(n, m, 3)
        ref, bound = R.reference_and_bound(cg, oracle, comp, X, Y, U, A, np.float32)
        emu = R.emulate_f32(cg, oracle, comp, X, Y, U, A, opts.get("jsplit", 0))
        live = bound > 0
        assert np.all(emu[~live] == 0.0) and np.all(ref[~live] == 0.0)
        ratio = np.abs(emu - ref)[live] / bound[live]
        print(f"{name} {n}x{m} d={d} {opts}: worst emulation err / bound = {ratio.max():.3f}")
        assert ratio.max() <= 0.1, (name, n, m, d, ratio)


@pytest.mark.parametrize("name", ["1.5ls(eq,.7)+.5dot", "ls(rq(.37),1.2)*nn(.5)+.3imq(.6)", "ls(eq,.7)*ls(rq(.5),1.4)"])
def test_bound_is_sensitive(cg, oracle, name):
    k = R.kernels(cg)[name]
    comp, _ = cg.require_mixed_parameter_spec(k)
    n, m, d, same, _ = R.SHAPES[0]
    X, Y = R.clouds(name, n, m, d, same)
    U, A = R.weights_for(n, m, 3)
    ref, bound = R.reference_and_bound(cg, oracle, comp, X, Y, U, A, np.float32)
    maj = R.majorant_sums(cg, oracle, comp, X, Y, U, A)
    emu = R.emulate_f32(cg, oracle, comp, X, Y, U, A)
    for kk in np.nonzero(bound > 0)[0]:
        moved = emu.copy(); moved[kk] += 1e-3 * maj[kk]
        assert abs(moved[kk] - ref[kk]) > bound[kk], (name, kk)
        if kk >= 8:                                         # a factor's derivative left out
            dropped = R.emulate_f32(cg, oracle, comp, X, Y, U, A, drop=int(kk))
            assert abs(dropped[kk] - ref[kk]) > bound[kk], (name, kk, dropped[kk], ref[kk], bound[kk])
