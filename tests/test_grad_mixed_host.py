"""CPU tier of the gradient kernels of mixed-trait composites (covgram_grad_mvm_mixed, csrc/grad_mixed.hpp):
  * the fp64 restatement tests/grad_mixed_ref.py against independent routes — torch fp64 autograd of a plain expression of each
    kernel, and for Sums the oracle's grad_matrix / valgrad_matrix / nn_grad_matrix term by term;
  * the lowering kernels.mixed_gradient_spec: per-factor traits, the Constant factor, Power folding, the limits, the refusals by
    name, and gramian() returning MixedBlockGramian exactly where device_spec is None and the mixed lowering exists;
  * bound feasibility: a float32 emulation of the device kernel's formation order on the inputs of tests/test_gpu_grad_mixed.py
    must stay within 0.25 of that test's fp32 bound, 1e-5 of absref (BASELINE.json's contract) — entry by entry."""
import math

import numpy as np
import pytest
import torch

import grad_mixed_ref as R


# ---- the reference against independent routes ----------------------------------------------------------------------------------------
def _torch_value(cg, k, x, y, gamma2=1.0):
    """A plain expression of k(x, y) on two torch vectors."""
    if isinstance(k, cg.Constant):
        return torch.as_tensor(k.c, dtype=x.dtype)
    if isinstance(k, cg.Sum):
        return sum(_torch_value(cg, a, x, y, gamma2) for a in k.args)
    if isinstance(k, cg.Product):
        out = torch.ones((), dtype=x.dtype)
        for a in k.args:
            out = out * _torch_value(cg, a, x, y, gamma2)
        return out
    if isinstance(k, cg.Power):
        return _torch_value(cg, k.k, x, y, gamma2) ** k.p
    if isinstance(k, cg.Lengthscale):
        return _torch_value(cg, k.k, x, y, gamma2 / k.l ** 2)
    if isinstance(k, cg.EQ):
        return torch.exp(-gamma2 * ((x - y) ** 2).sum() / 2)
    if isinstance(k, cg.MaternP) and k.p == 2:
        r = torch.sqrt(5 * gamma2 * ((x - y) ** 2).sum())
        return (1 + r + r * r / 3) * torch.exp(-r)
    if isinstance(k, cg.Dot):
        return (x * y).sum()
    if isinstance(k, cg.NeuralNetwork):
        l = lambda u, v: (u * v).sum() + k.sigma
        return 2 / math.pi * torch.asin(l(x, y) / torch.sqrt((1 + l(x, x)) * (1 + l(y, y))))
    raise NotImplementedError(type(k).__name__)


def _autograd_dense(cg, k, X, Y, value):
    n, d = X.shape; m = Y.shape[0]
    B = d + (1 if value else 0)
    M = np.zeros((n * B, m * B))
    for i in range(n):
        for j in range(m):
            x = torch.tensor(X[i], dtype=torch.float64, requires_grad=True)
            y = torch.tensor(Y[j], dtype=torch.float64, requires_grad=True)
            v = _torch_value(cg, k, x, y)
            gx, gy = torch.autograd.grad(v, (x, y), create_graph=True)
            blk = np.zeros((B, B))
            o = B - d
            for a in range(d):
                blk[o + a, o:] = torch.autograd.grad(gx[a], y, retain_graph=True)[0].numpy()
            if value:
                blk[0, 0] = float(v.detach()); blk[0, 1:] = gy.detach().numpy(); blk[1:, 0] = gx.detach().numpy()
            M[i * B:(i + 1) * B, j * B:(j + 1) * B] = blk
    return M


@pytest.mark.parametrize("name", ["eq+dot", "eq+(dot^2+1)", "eq*(dot^2+1)", "dot*dot", "maternp2+dot^2+nn", "nn(0.5)*ls(eq,2)", "(eq*dot)^2", "eq*dot zero"])
@pytest.mark.parametrize("value", [False, True])
def test_reference_matches_autograd(cg, name, value):
    k = R.kernels(cg)[name]
    X, Y = R.clouds(name, 4, 3, 3)
    got, ref = R.dense(cg, k, X, Y, value), _autograd_dense(cg, k, X, Y, value)
    assert np.abs(got - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max()), np.abs(got - ref).max()
    # the block product and its absolute-value twin against the dense matrix
    a = np.random.default_rng(5).standard_normal(got.shape[1])
    assert np.abs(R.mvm(cg, k, X, Y, a, value) - got @ a).max() <= 1e-13 * np.abs(got).max() * np.abs(a).sum()
    assert np.all(R.absref(cg, k, X, Y, a, value) >= np.abs(got) @ np.abs(a) * (1 - 1e-12))


def test_reference_sums_match_the_oracle_term_by_term(cg, oracle):
    o = oracle
    X, Y = R.clouds("x", 5, 4, 3)
    ref = o.grad_matrix(o.Kernel(o.MATERNP, p=2), X, Y) + o.grad_matrix(o.Kernel(o.DOT, power=2), X, Y) + o.nn_grad_matrix(X, Y)
    got = R.dense(cg, cg.MaternP(2) + cg.Dot() ** 2 + cg.NeuralNetwork(), X, Y)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
    for value, fn in ((False, o.grad_matrix), (True, o.valgrad_matrix)):
        ref = fn(o.Kernel(o.EQ), X, Y) + fn(o.Kernel(o.DOT), X, Y)
        got = R.dense(cg, cg.EQ() + cg.Dot(), X, Y, value)
        assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


# ---- lowering ------------------------------------------------------------------------------------------------------------------------
def _factors(c):
    out, fi = [], 0
    for t in range(c.nterms):
        out.append([c.factors[fi + q] for q in range(c.nfactors[t])])
        fi += c.nfactors[t]
    return out


def test_lowering_keeps_every_factor_its_own_trait(cg):
    f = cg._ffi
    assert cg.device_spec(cg.EQ() + cg.Dot()) is None                      # unchanged: GenericInput has no common-trait composite
    c = cg.mixed_gradient_spec(cg.EQ() + cg.Dot())
    assert c.head.family == f.COMPOSITE and c.nterms == 2
    assert sorted((t[0].family, t[0].trait) for t in _factors(c)) == [(f.EQ, f.ISOTROPIC), (f.DOT, f.DOTPRODUCT)]
    # the README kernel: three terms, the NeuralNetwork leaf with sigma in param and neither trait
    c = cg.mixed_gradient_spec(cg.MaternP(2) + cg.Dot() ** 2 + cg.NeuralNetwork(0.25))
    fam = {t[0].family: t[0] for t in _factors(c)}
    assert set(fam) == {f.MATERNP, f.DOT, f.NEURALNETWORK}
    assert fam[f.MATERNP].p == 2 and fam[f.DOT].power == 2 and fam[f.NEURALNETWORK].param == 0.25 and fam[f.NEURALNETWORK].trait == 0
    # Lengthscale stays with its own isotropic factor
    c = cg.mixed_gradient_spec(cg.NeuralNetwork(0.5) * cg.Lengthscale(cg.EQ(), 2.0))
    (term,) = _factors(c)
    assert {q.family: q.lengthscale for q in term} == {f.EQ: 2.0, f.NEURALNETWORK: 1.0}


def test_lowering_constants_and_power_folding(cg):
    f = cg._ffi
    # EQ + (Dot^2 + 1): the Constant is a term of its own, one CONSTANT factor carrying the value
    c = cg.mixed_gradient_spec(cg.EQ() + (cg.Dot() ** 2 + 1))
    terms = _factors(c)
    const = [t for t in terms if t[0].family == f.CONSTANT]
    assert c.nterms == 3 and len(const) == 1 and len(const[0]) == 1 and const[0][0].scale == 1.0
    # EQ * (Dot^2 + 1) multiplies out to EQ Dot^2 + EQ; a Constant factor rides on the first factor's scale
    c = cg.mixed_gradient_spec(3.0 * cg.EQ() * (cg.Dot() ** 2 + 1))
    terms = _factors(c)
    assert sorted(len(t) for t in terms) == [1, 2] and all(t[0].scale == 3.0 and all(q.scale == 1.0 for q in t[1:]) for t in terms)
    # Power of a product: (EQ Dot)^2 = EQ^2 Dot^2, like leaves merged into one factor with the exponents added
    c = cg.mixed_gradient_spec((cg.EQ() * cg.Dot()) ** 2)
    (term,) = _factors(c)
    assert sorted((q.family, q.power) for q in term) == [(f.EQ, 2), (f.DOT, 2)]
    c = cg.mixed_gradient_spec(cg.Dot() * cg.Dot())
    (term,) = _factors(c)
    assert [(q.family, q.power) for q in term] == [(f.DOT, 2)]


def test_the_two_normal_forms_differ_where_the_device_reads_them(cg):
    """device_spec and mixed_gradient_spec share one walker and one composite writer; the order of terms and factors decides the order of
    the floating-point products on the device, so what differs between the two forms is pinned with literal orders."""
    f = cg._ffi
    shape = lambda c: [[(q.family, q.param, q.power) for q in t] for t in _factors(c)]
    # a constant in the middle of a Sum: last in the common-trait form, where it stood in the mixed form
    k = cg.EQ() + 2.0 + cg.RQ(2.0)
    c = cg.device_spec(k)
    assert c.head.trait == f.ISOTROPIC and shape(c) == [[(f.EQ, 0.0, 1)], [(f.RQ, 2.0, 1)], [(f.CONSTANT, 0.0, 1)]]
    assert [t[0].scale for t in _factors(c)] == [1.0, 1.0, 2.0] and _factors(c)[2][0].trait == f.ISOTROPIC
    c = cg.mixed_gradient_spec(k)
    assert c.head.trait == 0 and shape(c) == [[(f.EQ, 0.0, 1)], [(f.CONSTANT, 0.0, 1)], [(f.RQ, 2.0, 1)]]
    assert [t[0].scale for t in _factors(c)] == [1.0, 2.0, 1.0] and _factors(c)[1][0].trait == 0
    c = cg.mixed_gradient_spec(cg.EQ() + 2.0 + cg.Dot())
    assert shape(c) == [[(f.EQ, 0.0, 1)], [(f.CONSTANT, 0.0, 1)], [(f.DOT, 0.0, 1)]]
    # a term's factors: (family, p, power, param, lengthscale) against (family, p, param, lengthscale, power)
    k = cg.RQ(2.0) ** 3 * cg.RQ(3.0) ** 2
    assert shape(cg.device_spec(k)) == [[(f.RQ, 3.0, 2), (f.RQ, 2.0, 3)]]
    assert shape(cg.mixed_gradient_spec(k)) == [[(f.RQ, 2.0, 3), (f.RQ, 3.0, 2)]]
    # like terms meet whatever order their factors were written in, coefficient on the first factor
    c = cg.mixed_gradient_spec(2.0 * k + cg.RQ(3.0) ** 2 * cg.RQ(2.0) ** 3)
    assert shape(c) == [[(f.RQ, 2.0, 3), (f.RQ, 3.0, 2)]] and [q.scale for q in _factors(c)[0]] == [3.0, 1.0]
    # an expression that cancels: nothing left in one form, the single term 0 in the other
    k = cg.EQ() + cg.Constant(-1.0, False) * cg.EQ()
    assert cg.device_spec(k) is None
    c = cg.mixed_gradient_spec(k)
    assert shape(c) == [[(f.CONSTANT, 0.0, 1)]] and _factors(c)[0][0].scale == 0.0
    # a single profile stays a plain covgram_kernel in one form and becomes a one-term composite in the other
    assert type(cg.device_spec(cg.EQ())) is f.covgram_kernel
    assert type(cg.mixed_gradient_spec(cg.EQ())) is f.covgram_kernel_composite


def test_lowering_limits_and_refusals_by_name(cg):
    f = cg._ffi
    many = cg.EQ()
    for i in range(f.COMPOSITE_MAX_TERMS):
        many = many + cg.Lengthscale(cg.EQ(), 2.0 + i) * cg.Dot()
    assert cg.mixed_gradient_spec(many) is None
    with pytest.raises(cg.UnsupportedKernel, match=r"9 terms and 17 factors"):
        cg.require_mixed_gradient_spec(many)
    for k, word in ((cg.Exponential() + cg.Dot(), "Exponential"), (cg.GammaExponential(1.5) * cg.Dot(), "GammaExponential"),
                    (cg.MaternP(0) + cg.Dot(), r"MaternP\(0\)"), (cg.Matern(2.3) + cg.Dot(), "Matern"), (cg.EQ() * cg.Cosine([1.0, 2.0]), "CosineKernel")):
        assert cg.mixed_gradient_spec(k) is None
        with pytest.raises(cg.UnsupportedKernel, match=word):
            cg.require_mixed_gradient_spec(k)
    # a half-integer Matern IS MaternP
    assert cg.mixed_gradient_spec(cg.Matern(2.5) + cg.Dot()) is not None


def test_the_rule_gramian_picks_the_mixed_operator_by(cg):
    """gramian() returns MixedBlockGramian exactly when device_spec(k) is None and mixed_gradient_spec(k) is not (a Gramian needs a
    device to exist: tests/test_gpu_grad_mixed.py checks the classes themselves); every kernel with a route of its own keeps it."""
    mixed = lambda k: cg.device_spec(k) is None and cg.mixed_gradient_spec(k) is not None
    names = {n for n, k in R.kernels(cg).items() if mixed(k)}
    assert names == set(R.kernels(cg)) - {"dot*dot"}                     # Dot * Dot has a common trait: its old route
    for k in (cg.EQ(), cg.EQ() * cg.RQ(2.0), cg.Dot() ** 2 + 1, cg.MaternP(2), cg.Exponential() + cg.Dot(), cg.Exponential() * cg.EQ()):
        assert not mixed(k)
    assert issubclass(cg.MixedBlockGramian, cg.BlockGramian)


# ---- bound feasibility of the GPU test's inputs ----------------------------------------------------------------------------------------
SHAPES = [(333, 517, 3, False), (130, 130, 5, True), (70, 193, 32, False), (100, 37, 33, False), (100, 70, 70, False)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s[:3]))
def test_fp32_bound_is_feasible_on_the_gpu_inputs(cg, shape):
    n, m, d, same = shape
    worst = 0.0
    for name, k in R.kernels(cg).items():
        for value in (False, True):
            X, Y = R.clouds(name, n, m, d, same)
            X32, Y32 = X.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64)
            a = np.random.default_rng(11).standard_normal(Y.shape[0] * (d + value)).astype(np.float32).astype(np.float64)
            ref, ab = R.mvm(cg, k, X32, Y32, a, value), R.absref(cg, k, X32, Y32, a, value)
            err = float((np.abs(R.mvm_float32(cg, k, X32, Y32, a, value) - ref) / ab).max())
            print(f"{name:20s} value={int(value)} fp32 emulation: worst err / absref {err:.2e}")
            worst = max(worst, err)
    assert worst <= 0.25 * 1e-5, worst
