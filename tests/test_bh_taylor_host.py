"""taylor! and minres without a GPU: tests/taylor_ref.py against the reference's own pins (test/barneshut.jl:78-82) on a tree that
barneshut_ref builds itself, the fp32 feasibility of the far-field bound that tests/test_gpu_bh_taylor.py applies, and the two new
symbols in the header, the ctypes mirror, the library and the Julia shim."""
import os
import re

import numpy as np
import pytest

import barneshut_ref as br
import covgram_oracle as o
import matrix_cases as mc
import taylor_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("covgram_bh_taylor_moments", "covgram_bh_taylor_mvm")
F32, F64 = np.float32, np.float64
EPS = float(np.finfo(F64).eps)


def cauchy_entries(X):
    def entries(rows, P):
        s = ((X[rows][:, None, :] - np.asarray(P, dtype=F64)[None]) ** 2).sum(2)
        ref = 1.0 / (1.0 + s)
        return ref, np.zeros_like(ref)
    return entries


def cauchy_jet(s):
    u = 1.0 / (1.0 + s)
    return u, -u * u, np.zeros_like(s), np.zeros_like(s)


@pytest.fixture(scope="module")
def pin():
    rng = np.random.default_rng(20260)
    n, d = 1024, 2
    X = rng.standard_normal((n, d))
    tree = br.build_tree(X, 16)
    K = 1.0 / (1.0 + ((X[:, None] - X[None]) ** 2).sum(2))
    weights = {"ones": np.ones(n), "rand": rng.random(n), "signed rand": rng.random(n) - 0.5, "randn": rng.standard_normal(n)}
    return X, tree, K, weights


def product(pin, w, theta, use_com):
    X, tree, _, _ = pin
    return tr.taylor(tree, X, X, w, theta, cauchy_entries(X), cauchy_jet, EPS, use_com=use_com)


def test_theta_zero_is_the_dense_product(pin):
    X, tree, K, weights = pin
    for name, w in weights.items():
        for use_com in (True, False):
            got = product(pin, w, 0.0, use_com)
            assert (np.abs(got - K @ w) <= 1e-13 * (np.abs(K) @ np.abs(w))).all(), (name, use_com)


def test_accuracy_pin_of_the_reference(pin):
    """test/barneshut.jl:80 with the product that the reference's mul! runs: norm-wise relative error < 1e-3 at theta = 1/8."""
    X, tree, K, weights = pin
    for name, w in weights.items():
        want = K @ w
        err = {uc: np.linalg.norm(product(pin, w, 0.125, uc) - want) / np.linalg.norm(want) for uc in (True, False)}
        print(f"taylor-ref pin {name}: centre of mass {err[True]:.2e}, ball centres {err[False]:.2e}")
        assert err[True] < 1e-3, (name, err)


def test_nonnegative_weights_give_the_unsplit_barnes_hut_product(pin):
    """About the centre of mass of nonnegative weights the first moment vanishes up to rounding: taylor! is barneshut!(split = false)."""
    X, tree, K, weights = pin
    for name in ("ones", "rand"):
        w = weights[name]
        got = product(pin, w, 0.125, True)
        want = br.barneshut(tree, X, X, w, 0.125, cauchy_entries(X), EPS, split=False)
        assert (np.abs(got - want) <= 1e-10 * np.abs(want)).all(), (name, np.abs(got / want - 1).max())


def test_linearity_defect(pin):
    """About the ball centres the product is a linear map of w; about the centres of mass it is not."""
    X, tree, K, weights = pin
    w1, w2 = weights["randn"], weights["signed rand"]
    defect = {}
    for use_com in (True, False):
        lhs = product(pin, 0.3 * w1 - 1.7 * w2, 0.25, use_com)
        rhs = 0.3 * product(pin, w1, 0.25, use_com) - 1.7 * product(pin, w2, 0.25, use_com)
        defect[use_com] = np.linalg.norm(lhs - rhs) / np.linalg.norm(rhs)
    print(f"taylor-ref linearity defect: ball centres {defect[False]:.2e}, centres of mass {defect[True]:.2e}")
    assert defect[False] <= 1e-13 and defect[True] >= 1e-5, defect


def test_zero_weights_contribute_exact_zeros(pin):
    X, tree, _, _ = pin
    for use_com in (True, False):
        mo = tr.moments(tree, X, np.zeros(X.shape[0]), float(np.finfo(F32).eps), use_com)
        assert not mo["sums"].any() and not mo["m1"].any()
        assert not product(pin, np.zeros(X.shape[0]), 0.25, use_com).any()


def indefinite_system():
    """Cauchy on 300 points of N(0, I) (seed 5, rounded to fp32), shifted by the midpoint of its 4th and 5th largest eigenvalues."""
    X = np.random.default_rng(5).standard_normal((300, 2)).astype(F32).astype(F64)
    K = 1.0 / (1.0 + ((X[:, None] - X[None]) ** 2).sum(2))
    ev = np.linalg.eigvalsh(K)
    sigma = 0.5 * (ev[-4] + ev[-5])
    return X, K, sigma


def test_minres_on_an_indefinite_matrix():
    X, K, sigma = indefinite_system()
    A = K - sigma * np.eye(300)
    ev = np.linalg.eigvalsh(A)
    assert (ev > 0).sum() == 4 and np.abs(ev).max() / np.abs(ev).min() <= 100
    b = np.random.default_rng(6).standard_normal(300)
    x, it, res = tr.minres(A, b, reltol=1e-12, maxiter=600)
    want = np.linalg.solve(A, b)
    err = np.linalg.norm(x - want) / np.linalg.norm(want)
    print(f"minres-ref indefinite: sigma {sigma:.4f}, {it} iterations, recurrence {res:.2e}, error {err:.2e}")
    assert err <= 1e-8, err


def test_minres_pin_of_the_reference(pin):
    """test/barneshut.jl:81-82: x = F \\ b with b = F w, maxiter = 128, and |F x - b| < 1e-3 |b|, F = taylor! + 1e-2 I."""
    X, tree, K, weights = pin
    F = lambda v: product(pin, v, 0.125, True) + 1e-2 * v
    for name, w in weights.items():
        b = F(w)
        x, it, rec = tr.minres(F, b, reltol=1e-4, maxiter=128)
        res = np.linalg.norm(F(x) - b) / np.linalg.norm(b)
        print(f"minres-ref pin {name}: {it} iterations, recurrence {rec / np.linalg.norm(b):.2e}, residual {res:.2e}")
        assert res < 1e-3, (name, res)


# ---- the far-field bound of tests/test_gpu_bh_taylor.py in exactly rounded fp32 ---------------------------------------------------------
def far_kernels():
    return [("Cauchy", o.Kernel(o.CAUCHY)), ("2.5 EQ(l=0.7)", o.Kernel(o.EQ, lengthscale=0.7, scale=2.5)), ("MaternP(2)", o.Kernel(o.MATERNP, p=2)),
            ("RQ(1.5)", o.Kernel(o.RQ, param=1.5)), ("Exp", o.Kernel(o.EXP)), ("Matern(1.3)", o.Kernel(o.MATERN, param=1.3))]


def r32(a):
    return np.asarray(a, dtype=F64).astype(F32)


def emulate_far_f32(ko, x, c, m1, sums):
    """The device's order of operations with every step rounded to fp32 once: q = x - c, s and q . m1 by sequential fma, the argument
    s / l^2, value and derivative of the unscaled profile, acc = f0 sums, acc = fma(-2 (f1 / l^2), dot, acc), times the scale."""
    g2 = F32(1.0 / ko.lengthscale ** 2)
    s = np.zeros(x.shape[0], F32); dot = np.zeros(x.shape[0], F32)
    for l in range(x.shape[1]):
        q = r32(x[:, l].astype(F64) - c[:, l].astype(F64))
        s = r32(q.astype(F64) ** 2 + s.astype(F64))
        dot = r32(q.astype(F64) * m1[:, l].astype(F64) + dot.astype(F64))
    k1 = o.Kernel(ko.family, p=ko.p, param=ko.param, power=ko.power)
    f0, f1, _ = o.profile_derivatives(k1, r32(s.astype(F64) * F64(g2)).astype(F64), F32)
    f0, f1 = r32(f0), r32(r32(f1).astype(F64) * F64(g2))
    acc = r32(f0.astype(F64) * sums.astype(F64))
    acc = r32(-2.0 * f1.astype(F64) * dot.astype(F64) + acc.astype(F64))
    return r32(F64(F32(ko.scale)) * acc.astype(F64))


def test_far_field_bound_is_feasible_in_fp32():
    rng = np.random.default_rng(8)
    count = 4000
    for kname, ko in far_kernels():
        jet = tr.far_jet(o, mc, ko, F32)
        for d in (1, 2, 3, 8):
            x = (rng.standard_normal((count, d)) * rng.choice([0.5, 1.0, 3.0], (count, 1))).astype(F32)
            c = rng.standard_normal((count, d)).astype(F32)
            m1 = (rng.standard_normal((count, d)) * rng.choice([1e-3, 0.1, 1.0], (count, 1))).astype(F32)
            sums = rng.standard_normal(count).astype(F32)
            ri = x.astype(F64) - c.astype(F64)
            f0, f1, b0, lf = jet((ri ** 2).sum(1))
            adot = (np.abs(ri) * np.abs(m1.astype(F64))).sum(1)
            want = f0 * sums - 2 * f1 * (ri * m1.astype(F64)).sum(1)
            bound = b0 * np.abs(sums) + lf * 2 * np.abs(f1) * adot
            got = emulate_far_f32(ko, x, c, m1, sums).astype(F64)
            ratio = float((np.abs(got - want) / bound).max())
            print(f"taylor far-field fp32 emulation {kname} d={d}: worst err/bound {ratio:.3f}")
            assert ratio <= 0.5, (kname, d, ratio)


def test_profile_derivative_against_a_central_difference():
    s = np.linspace(0.05, 9.0, 60)
    for kname, ko in far_kernels() + [("Cauchy(l=1.5)^2", o.Kernel(o.CAUCHY, lengthscale=1.5, power=2))]:
        h = 1e-5 * s
        f1 = o.profile_derivatives(ko, s)[1]
        fd = (o.profile(ko, s + h) - o.profile(ko, s - h)) / (2 * h)
        assert (np.abs(f1 - fd) <= 1e-7 * np.abs(f1)).all() and (f1 < 0).all(), (kname, np.abs(f1 / fd - 1).max())


def test_header_ffi_library_and_shim_name_the_two_symbols(cg):
    header = open(os.path.join(ROOT, "include", "covgram.h")).read()
    jl = open(os.path.join(ROOT, "covariancefunctions.jl_amd", "julia", "CovGram.jl")).read()
    lib = cg._ffi.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in cg._ffi.PROTOTYPES, name
        assert hasattr(lib, name), name
        assert re.search(r"ccall\(\(:%s, libcovgram\)" % name, jl), name
    assert lib.covgram_version() == 113
    assert "function taylor!(b::StridedVector{T}, F::DeviceBarnesHut{T}" in jl and "minres!" in jl
    assert callable(cg.minres) and all(hasattr(cg.BarnesHutFactorization, a) for a in ("taylor_", "taylor", "taylor_moments", "solve"))


def test_abi_refusals_come_before_any_launch(cg):
    f, lib = cg._ffi, cg._ffi.lib()
    assert lib.covgram_bh_taylor_mvm(None, None, None, 1.0, 0.0, -1.0, 1, None, 0, f.DEVICE) == f.EINVAL
    assert lib.covgram_bh_taylor_moments(None, None, 1, None, None, None, f.DEVICE) == f.EINVAL
    with pytest.raises(ValueError):
        cg.BarnesHutFactorization(cg.Cauchy(), np.zeros((5, 2)), product="fmm")


def test_why_the_d5_targets_of_the_device_test_move_by_two():
    """tests/test_gpu_bh_taylor.py moves every second target of its d = 5 shape by +2, not by the +4 of the small shapes: with EQ(l = 0.7)
    more than half of the moved rows' entries would lie below the smallest normal fp32 number, where the hardware exponential returns
    zero for the profile and for its derivative; at +2 fewer than 1 % do."""
    import test_gpu_bh_taylor as g
    X, Y = g.cloud(129, 500, 5, F32, "xy")
    X4 = X.copy(); X4[::2] += F32(2)
    ko = o.Kernel(o.EQ, lengthscale=0.7)
    below = {name: float((o.matrix(ko, P, Y, F32)[::2] < mc.tiny(F32)).mean()) for name, P in (("+2", X), ("+4", X4))}
    print(f"share of the moved rows' EQ(l=0.7) entries below the smallest normal fp32: {below}")
    assert below["+4"] > 0.5 and below["+2"] < 0.01, below
