"""Host side of the hyper-parameter gradients (no GPU): the reference formulas of tests/bilin_grad_ref.py against finite differences,
the parameter tree, the host chain rules of bilinear_gradient, the refusals, and the feasibility of the GPU test's bound."""
import numpy as np
import pytest

import bilin_grad_ref as br
import covgram_oracle as o
import matrix_cases as mc

F32, F64 = np.float32, np.float64


def fd5(f, h=1e-3):
    return (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)


def small_cloud():
    rng = np.random.default_rng(11)
    X = 0.8 * rng.standard_normal((67, 3)) + 0.2
    Y = 0.8 * rng.standard_normal((33, 3))
    Y[:4] = X[[5, 17, 40, 66]]                                   # s = 0 exactly
    return X, Y, rng.standard_normal((67, 33))


LENGTHSCALE_KERNELS = [("EQ", o.Kernel(o.EQ)), ("Exponential", o.Kernel(o.EXP)), ("RQ(0.37)", o.Kernel(o.RQ, param=0.37)),
                       ("2.5*MaternP(2)", o.Kernel(o.MATERNP, p=2, scale=2.5)), ("gammaExp(1.5)", o.Kernel(o.GAMMAEXP, param=1.5)),
                       ("Cauchy^2", o.Kernel(o.CAUCHY, power=2)), ("IMQ(0.6)", o.Kernel(o.IMQ, param=0.6)), ("Matern(0.8)", o.Kernel(o.MATERN, param=0.8))]
PARAM_KERNELS = [("RQ(0.37)", o.Kernel(o.RQ, param=0.37)), ("1.7*RQ(2.5)^3 l=0.8", o.Kernel(o.RQ, param=2.5, power=3, lengthscale=0.8, scale=1.7)),
                 ("gammaExp(1.5)", o.Kernel(o.GAMMAEXP, param=1.5)), ("gammaExp(0.7)^2 l=1.2", o.Kernel(o.GAMMAEXP, param=0.7, power=2, lengthscale=1.2)),
                 ("IMQ(0.6)", o.Kernel(o.IMQ, param=0.6)), ("0.4*IMQ(1.3)^2 l=0.7", o.Kernel(o.IMQ, param=1.3, power=2, lengthscale=0.7, scale=0.4))]


def replace(ko, **kw):
    f = dict(family=ko.family, p=ko.p, power=ko.power, param=ko.param, lengthscale=ko.lengthscale, scale=ko.scale)
    f.update(kw)
    return o.Kernel(**f)


def reference_parts(ko, X, Y, W):
    """The reference sums with the full-rank weight W (U = W, A = I) and the magnitudes sum |W| |d_p K| of the three derivatives."""
    quantities, _ = br.pair_quantities(o, ko, X, Y, 0, F64)
    out = [float((W * Q).sum()) for Q, _, _, _ in quantities]
    mag = [float((np.abs(W) * np.abs(Q)).sum()) for Q, _, _, _ in quantities]
    assert np.allclose(out, br.reference(o, ko, X, Y, W, np.eye(Y.shape[0]), 0), rtol=1e-13, atol=0)
    return out, mag


@pytest.mark.parametrize("name,ko", LENGTHSCALE_KERNELS, ids=[n for n, _ in LENGTHSCALE_KERNELS])
def test_reference_lengthscale_and_scale_against_finite_differences(name, ko):
    X, Y, W = small_cloud()
    out, mag = reference_parts(ko, X, Y, W)
    l, c = ko.lengthscale, ko.scale
    fl = fd5(lambda h: float((W * o.matrix(replace(ko, lengthscale=l + h), X, Y)).sum()))
    fc = fd5(lambda h: float((W * o.matrix(replace(ko, scale=c + h), X, Y)).sum()))
    rl = abs(-2.0 / l * out[2] - fl) / (2.0 / l * mag[2])
    rc = abs(out[0] / c - fc) / (mag[0] / c)
    print(f"bilin-grad-host {name}: lengthscale {rl:.2e}, scale {rc:.2e} (relative to sum |W| |dK|)")
    assert rl <= 1e-9 and rc <= 1e-9


@pytest.mark.parametrize("name,ko", PARAM_KERNELS, ids=[n for n, _ in PARAM_KERNELS])
def test_reference_parameter_derivatives_against_finite_differences(name, ko):
    X, Y, W = small_cloud()
    out, mag = reference_parts(ko, X, Y, W)
    fp = fd5(lambda h: float((W * o.matrix(replace(ko, param=ko.param + h), X, Y)).sum()))
    rp = abs(out[1] - fp) / mag[1]
    fl = fd5(lambda h: float((W * o.matrix(replace(ko, lengthscale=ko.lengthscale + h), X, Y)).sum()))
    rl = abs(-2.0 / ko.lengthscale * out[2] - fl) / (2.0 / ko.lengthscale * mag[2])
    print(f"bilin-grad-host {name}: param {rp:.2e}, lengthscale {rl:.2e}")
    assert rp <= 1e-9 and rl <= 1e-9


def test_reference_zero_distance_and_per_dimension_split():
    """Pairs with s = 0 add nothing to out[2 ..] (also where phi' is unbounded) and the per-dimension sums add up to the isotropic one."""
    X, Y, W = small_cloud()
    for name, ko in LENGTHSCALE_KERNELS[:7]:
        a = br.reference(o, ko, X, Y, W, np.eye(33), 0)
        b = br.reference(o, ko, X, Y, W, np.eye(33), 1)
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)), name
        assert abs(b[2:].sum() - a[2]) <= 1e-12 * np.abs(b[2:]).sum() and np.allclose(a[:2], b[:2], rtol=1e-14), name
    ko = o.Kernel(o.EXP)
    e1 = np.zeros((67, 1)); e1[5] = 1.0
    e2 = np.zeros((33, 1)); e2[0] = 1.0
    assert np.array_equal(br.reference(o, ko, X, Y, e1, e2, 1), [1.0, 0.0, 0.0, 0.0, 0.0])


# ---- parameter tree ----------------------------------------------------------------------------------------------------------------
def test_parameter_tree_round_trip(cg):
    k = cg.Sum((1.5 * cg.Lengthscale(cg.EQ(), 0.7), cg.Power(0.5 * cg.RQ(0.37), 2),
                cg.Sum((cg.Lengthscale(cg.Lengthscale(cg.GammaExponential(1.5), 2.0), 3.0), cg.Constant(0.25))), 0.3 * cg.InverseMultiQuadratic(0.6)))
    leaves = cg.hyperparameters(k)
    assert [nm for _, nm, _ in leaves] == ["scale", "l", "scale", "alpha", "gamma", "l", "l", "scale", "scale", "c"]
    assert [v for _, _, v in leaves] == [1.5, 0.7, 0.5, 0.37, 1.5, 2.0, 3.0, 0.25, 0.3, 0.6]
    assert leaves[0][0] == (0, 0) and leaves[1][0] == (0, 1) and leaves[3][0] == (1, "k", 1) and leaves[5][0] == (2, 0, "k")
    assert len({p + (nm,) for p, nm, _ in leaves}) == len(leaves)                # every leaf has its own address
    assert cg.hyperparameters(k) == leaves                                       # stable
    theta = [v + 0.125 for _, _, v in leaves]
    k2 = cg.with_hyperparameters(k, theta)
    assert [(p, nm) for p, nm, _ in cg.hyperparameters(k2)] == [(p, nm) for p, nm, _ in leaves]
    assert [v for _, _, v in cg.hyperparameters(k2)] == theta
    x, y = np.array([0.3, -0.2]), np.array([-0.1, 0.4])
    assert cg.with_hyperparameters(k, [v for _, _, v in leaves])(x, y) == k(x, y)
    assert k2(x, y) != k(x, y)
    ard = cg.ARD(2.0 * cg.MaternP(2), [0.5, 1.0, 2.0])
    la = cg.hyperparameters(ard)
    assert [nm for _, nm, _ in la] == ["scale", "l", "l", "l"] and [v for _, _, v in la] == [2.0, 0.5, 1.0, 2.0]
    ard2 = cg.with_hyperparameters(ard, [3.0, 0.25, 0.5, 4.0])
    assert np.array_equal(ard2.U, 1.0 / np.array([0.25, 0.5, 4.0])) and [v for _, _, v in cg.hyperparameters(ard2)] == [3.0, 0.25, 0.5, 4.0]
    su = cg.ScaledInputKernel(cg.EQ(), np.array([2.0, 0.5]))
    assert [(nm, v) for _, nm, v in cg.hyperparameters(su)] == [("U", 2.0), ("U", 0.5)]
    assert np.array_equal(cg.with_hyperparameters(su, [1.0, 3.0]).U, [1.0, 3.0])
    assert cg.hyperparameters(cg.Power(cg.MaternP(3), 2)) == [] and cg.hyperparameters(cg.Matern(0.8)) == []   # p, nu, exponent: structure


def test_parameter_tree_length_mismatch(cg):
    k = 1.5 * cg.Lengthscale(cg.EQ(), 0.7)
    with pytest.raises(cg.DimensionMismatch, match=r"length\(θ\) = 3 ≠ 2 = nparameters\(k\)"):
        cg.with_hyperparameters(k, [1.0, 2.0, 3.0])
    with pytest.raises(cg.DimensionMismatch, match=r"length\(θ\) = 0 ≠ 2 = nparameters\(k\)"):
        cg.with_hyperparameters(k, [])
    with pytest.raises(cg.UnsupportedKernel, match="VerticalRescaling"):
        cg.hyperparameters(cg.VerticalRescaling(cg.EQ(), lambda x: x))


# ---- the host chain rules ----------------------------------------------------------------------------------------------------------
def oracle_kernel(spec):
    return o.Kernel(spec.family, p=spec.p, power=spec.power, param=spec.param, lengthscale=spec.lengthscale, scale=spec.scale)


def host_form(k, X, Y, W):
    return sum(W[i, j] * k(X[i], Y[j]) for i in range(X.shape[0]) for j in range(Y.shape[0]))


def chain_rule_case(cg, k, scaled):
    from covgram.gramian import _bilinear_plan
    rng = np.random.default_rng(5)
    X = 0.8 * rng.standard_normal((12, 3)) + 0.2; Y = 0.8 * rng.standard_normal((9, 3))
    Y[0] = X[3]
    W = rng.standard_normal((12, 9))
    top = scaled if scaled is not None else k
    Xt, Yt = (X * scaled.U, Y * scaled.U) if scaled is not None else (X, Y)       # what gramian() hands the device
    grad = []
    for spec, rules in _bilinear_plan(k):
        if spec is None:                                          # a Constant term: bilinear_gradient hands the rule sum W
            out = [float(W.sum()), 0.0, 0.0]
        else:
            out = br.reference(o, oracle_kernel(spec), Xt, Yt, W, np.eye(9), 1 if scaled is not None else 0)
        grad += cg.bilinear_chain_rules(rules, out, scaled)
    theta = [v for _, _, v in cg.hyperparameters(top)]
    assert len(grad) == len(theta)
    for p in range(len(theta)):
        def f(h):
            t = list(theta); t[p] += h
            return host_form(cg.with_hyperparameters(top, t), X, Y, W)
        fd = fd5(f)
        print(f"bilin-grad-host chain rule {cg.hyperparameters(top)[p][:2]}: {grad[p]:.12e} against {fd:.12e}")
        assert abs(grad[p] - fd) <= 1e-8 * max(abs(fd), 1.0), (p, grad[p], fd)


def test_chain_rules_ard(cg):
    ard = cg.ARD(2.0 * cg.MaternP(2), [0.7, 1.1, 1.9])
    chain_rule_case(cg, ard.k, ard)
    su = cg.ScaledInputKernel(cg.Lengthscale(cg.RQ(0.37), 1.2), np.array([1.4, 0.6, 0.9]))
    chain_rule_case(cg, su.k, su)


def test_chain_rules_sum(cg):
    chain_rule_case(cg, 1.5 * cg.Lengthscale(cg.EQ(), 0.7) + 0.5 * cg.RQ(0.37), None)
    chain_rule_case(cg, cg.Power(0.5 * cg.Lengthscale(cg.InverseMultiQuadratic(0.6), 0.9), 2) + cg.Constant(0.25), None)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_device_call(cg, monkeypatch):
    import sys
    gm, dist = sys.modules["covgram.gramian"], sys.modules["covgram.dist"]      # (the package attribute `gramian` is the function)
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(cg._ffi, "lib", no_lib)
    u = np.zeros(4)

    def fake_gramian(k):
        G = object.__new__(gm.Gramian)
        G.k = k
        return G
    for k, word in ((cg.EQ() * cg.Cauchy(), "Product of two non-constant"), (cg.Dot(), "Dot"), (2.0 * cg.ExponentialDot(), "ExponentialDot"),
                    (cg.Matern(0.8), "real nu"), (cg.Lengthscale(cg.EQ(), 0.7) + cg.Matern(1.3), "real nu"),
                    (cg.SpectralMixture([1.0], [[0.3]], [[1.0]]), ""), (cg.VerticalRescaling(cg.EQ(), lambda x: x), "VerticalRescaling"),
                    (cg.Power(cg.EQ(), 2) * cg.RQ(1.0), "Product of two non-constant")):
        with pytest.raises(cg.UnsupportedKernel, match=word):
            cg.bilinear_gradient(fake_gramian(k), u, u)
    for cls in (gm.BlockGramian, gm.HessianGramian, gm.ValueGradientHessianGramian, gm.SymmetricToeplitz, gm.Toeplitz, gm.Circulant,
                gm.KroneckerProduct, gm.SparseGramian, gm.BarnesHutFactorization, gm.SpectralMixtureGramian, gm.LazyMatrixProduct,
                dist.ShardedGramian):
        with pytest.raises(cg.UnsupportedKernel, match=cls.__name__):
            cg.bilinear_gradient(object.__new__(cls), u, u)
    full = fake_gramian(cg.EQ())
    full.scaled_input = cg.ScaledInputKernel(cg.EQ(), np.eye(2))
    with pytest.raises(cg.UnsupportedKernel, match="full matrix"):
        cg.bilinear_gradient(full, u, u)
    with pytest.raises(cg.UnsupportedKernel, match="SymmetricToeplitz"):
        cg.inv_quad_logdet_gradient(object.__new__(gm.SymmetricToeplitz), None)


# ---- the GPU test's bound is feasible -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 8])
def test_fp32_emulation_within_the_gpu_bound(d):
    """An exactly rounded fp32 evaluation in the kernel's order (bilin_grad_ref.emulate_f32) on the GPU test's own clouds.  The device's
    exp / log / pow are not part of this emulation: their headroom is what the GPU test measures.  A ratio above 1 is a finding about
    the bound, never a number to fit."""
    import test_gpu_bilin_grad as tg
    for name, ko in tg.FAMILIES:
        rng = np.random.default_rng(1000 + d)
        X, Y = mc.iso_cloud(rng, tg.N, tg.M, d, F32, lscale=ko.lengthscale)[:2]
        for nvec in (1, 17):
            U, A = tg.weights(rng, tg.N, tg.M, nvec, F32)
            for per_dim in (0, 1):
                ref, bound = br.reference_and_bound(o, ko, X, Y, U, A, per_dim, F32)
                emu = br.emulate_f32(o, ko, X, Y, U, A, per_dim)
                r = np.abs(emu - ref) / bound
                print(f"bilin-grad-bound-host {name:22s} d={d} nvec={nvec:2d} per_dim={per_dim}: worst err/bound {r.max():.3f} at out[{int(r.argmax())}]")
                assert r.max() <= 1.0, (name, d, nvec, per_dim, r)


def test_fixed_probes_of_the_gpu_test_are_a_fair_draw():
    """The committed seed of tests/test_gpu_bilin_grad.py: in dense fp64 alone the exact tr(A^-1 dA) lies within 4 standard errors of the
    fixed-probe estimate for every parameter."""
    import test_gpu_bilin_grad as tg
    x, b, Z = tg.iq_problem()
    Amat, dA = tg.iq_dense(x)
    gq, per, exact = tg.iq_expressions(Amat, dA, b, Z)
    se = per.std(0, ddof=1) / np.sqrt(tg.IQ_P)
    print("fixed probes: (exact - estimate) / stderr", (exact - per.mean(0)) / se)
    assert np.all(np.abs(exact - per.mean(0)) <= 4 * se)
