"""decay_radius without a GPU: the closed forms of src/sparse.jl:25-35 for every supported kernel, the two corrections of the reference
(Lengthscale multiplies, a Constant factor divides delta), the refusals, and covgram_decay_radius through ctypes."""
import ctypes as C
import math

import pytest

import covgram_oracle as o
import sparse_ref as sr

DELTAS = (1e-6, 1e-3, 0.5)


def supported(cg):
    """(name, kernel, closed form r0(de))"""
    return [
        ("EQ", cg.EQ(), lambda de: math.sqrt(-2 * math.log(de))),
        ("Exponential", cg.Exp(), lambda de: -math.log(de)),
        ("GammaExponential(1.5)", cg.GammaExponential(1.5), lambda de: (-2 * math.log(de)) ** (1 / 1.5)),
        ("GammaExponential(0.7)", cg.GammaExponential(0.7), lambda de: (-2 * math.log(de)) ** (1 / 0.7)),
        ("MaternP(0)", cg.MaternP(0), lambda de: -math.log(de)),
        ("MaternP(2)", cg.MaternP(2), lambda de: -math.log(de)),
        ("Matern(0.5)", cg.Matern(0.5), lambda de: -math.log(de)),
        ("Matern(1.3)", cg.Matern(1.3), lambda de: -math.log(de)),
        ("Matern(2.5)", cg.Matern(2.5), lambda de: -math.log(de)),
    ]


def close(a, b, tol=1e-15):
    return abs(a - b) <= tol * abs(b)


def test_closed_forms(cg):
    for name, k, r0 in supported(cg):
        for de in DELTAS:
            assert close(cg.decay_radius(k, de), r0(de)), (name, de)
    assert close(cg.decay_radius(cg.EQ()), math.sqrt(-2 * math.log(1e-6)))          # default delta
    # the helper the GPU tests use agrees with the same closed forms
    assert close(sr.radius(o.Kernel(o.GAMMAEXP, param=1.5, lengthscale=0.3, scale=2.0), 1e-6), 0.3 * (-2 * math.log(0.5e-6)) ** (1 / 1.5))


def test_lengthscale_multiplies(cg):
    """Lengthscale(k, l) evaluates k(r / l): the radius is l r0 (src/sparse.jl:38 divides, and drops delta)."""
    for name, k, r0 in supported(cg):
        for l in (0.05, 1.0, 7.5):
            assert close(cg.decay_radius(cg.Lengthscale(k, l), 1e-6), l * r0(1e-6)), (name, l)
        assert close(cg.decay_radius(cg.Lengthscale(cg.Lengthscale(k, 2.0), 0.25), 1e-4), 0.5 * r0(1e-4)), name
        # the radius is where the kernel itself crosses delta (EQ, Exponential exactly; the Matern radii are conservative)
        kl = cg.Lengthscale(k, 0.3)
        s = cg.decay_radius(kl, 1e-6) ** 2
        assert kl.profile(s) <= 1e-6 * (1 + 1e-9), (name, kl.profile(s))


def test_constant_divides_delta(cg):
    for name, k, r0 in supported(cg):
        for c in (2.5, 0.01):
            assert close(cg.decay_radius(c * k, 1e-6), r0(1e-6 / c)), (name, c)
            assert close(cg.decay_radius(c * cg.Lengthscale(k, 0.4), 1e-6), 0.4 * r0(1e-6 / c)), (name, c)
    with pytest.raises(ValueError):
        cg.decay_radius(1e-7 * cg.EQ(), 1e-6)                  # delta / |c| >= 1: the whole matrix is below delta
    with pytest.raises(ValueError):
        cg.decay_radius(cg.EQ(), 0.0)
    with pytest.raises(ValueError):
        cg.decay_radius(cg.EQ(), 1.0)


def refused(cg):
    return [
        ("RationalQuadratic", cg.RQ(1.0)), ("Cauchy", cg.Cauchy()), ("InverseMultiQuadratic", cg.InverseMultiQuadratic(1.0)),
        ("Dot", cg.Dot()), ("ExponentialDot", cg.ExponentialDot()), ("Sum", cg.EQ() + cg.Exp()), ("Product", cg.EQ() * cg.Exp()),
        ("Power", cg.EQ() ** 2), ("Power", 2.0 * (cg.Lengthscale(cg.Exp(), 0.5) ** 3)), ("Periodic", cg.Periodic(cg.EQ())),
        ("CosineKernel", cg.Cosine([1.0])), ("NeuralNetwork", cg.NeuralNetwork()),
    ]


def test_refusals_name_the_kernel(cg):
    for name, k in refused(cg):
        with pytest.raises(cg.UnsupportedKernel) as e:
            cg.decay_radius(k, 1e-6)
        assert name in str(e.value), (name, str(e.value))
    with pytest.raises(cg.DomainError) as e:
        cg.decay_radius(cg.Matern(0.3), 1e-6)
    assert "Matern" in str(e.value)
    with pytest.raises(cg.DomainError):
        cg.decay_radius(3.0 * cg.Lengthscale(cg.Matern(0.3), 2.0), 1e-6)


def test_sparse_refuses_what_is_not_a_plain_gramian(cg):
    """sparse() checks its argument on the host before any device call."""
    class NotAGramian(cg.LazyOperator):
        pass
    with pytest.raises(cg.UnsupportedKernel) as e:
        cg.sparse(NotAGramian(), 1e-6)
    assert "NotAGramian" in str(e.value)


def test_abi_decay_radius_matches_python(cg):
    f, lib = cg._ffi, cg._ffi.lib()
    for name, k, _ in supported(cg):
        for kk in (k, 2.5 * cg.Lengthscale(k, 0.37), 0.01 * cg.Lengthscale(k, 11.0)):
            for de in DELTAS[:2]:
                r = C.c_double(0)
                assert lib.covgram_decay_radius(f.kref(cg.device_spec(kk)), de, C.byref(r)) == f.OK, lib.covgram_last_error()
                assert close(r.value, cg.decay_radius(kk, de)), (name, de, r.value)
    r = C.c_double(0)
    for name, k in refused(cg)[:9]:
        spec = cg.device_spec(k)
        assert lib.covgram_decay_radius(f.kref(spec), 1e-6, C.byref(r)) == f.EUNSUPPORTED, name
        msg = lib.covgram_last_error().decode()
        assert (name in msg) or (name == "Power" and "Power(" in msg), (name, msg)
    assert lib.covgram_decay_radius(f.kref(cg.device_spec(cg.Matern(0.3))), 1e-6, C.byref(r)) == f.EINVAL
    assert "DomainError" in lib.covgram_last_error().decode()
    assert lib.covgram_decay_radius(f.kref(cg.device_spec(1e-7 * cg.EQ())), 1e-6, C.byref(r)) == f.EINVAL
    assert lib.covgram_decay_radius(f.kref(cg.device_spec(cg.EQ())), 1e-6, None) == f.EINVAL
