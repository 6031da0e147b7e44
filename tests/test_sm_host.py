"""SpectralMixture kernels on the host (no GPU): the constructors mirror the reference's structure (src/stationary.jl:213-217), the scalar
call operator equals the definition, and spectral_mixture_spec lowers exactly the expressions the fused device kernels take."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def definition(w, mu, l, x, y):
    x = np.atleast_1d(np.asarray(x, float)); y = np.atleast_1d(np.asarray(y, float))
    out = 0.0
    for wq, mq, lq in zip(w, mu, l):
        r = x - y
        out += wq * math.cos(2 * math.pi * float(np.dot(np.broadcast_to(mq, r.shape), r))) * math.exp(-0.5 * float(np.sum((r / lq) ** 2)))
    return out


def test_constructors_have_the_reference_structure(cg):
    assert cg.SM is cg.SpectralMixture
    s = cg.Spectral(1.5, [0.3, -0.2], 0.7)
    assert isinstance(s, cg.Product) and len(s.args) == 3
    c, co, e = s.args
    assert isinstance(c, cg.Constant) and c.c == 1.5
    assert isinstance(co, cg.CosineKernel) and np.array_equal(co.c, [0.3, -0.2])
    assert isinstance(e, cg.Lengthscale) and isinstance(e.k, cg.EQ) and e.l == 0.7           # a scalar l: Lengthscale
    e2 = cg.Spectral(1.5, [0.3, -0.2], [0.7, 2.0]).args[2]
    assert isinstance(e2, cg.ScaledInputKernel) and isinstance(e2.k, cg.EQ) and np.allclose(e2.U, [1 / 0.7, 0.5])   # a vector l: ARD
    k = cg.SM([1.0, -0.5, 2.0], [[0.0, 0.0], [0.4, 0.1], [1.0, -1.0]], [1.0, 0.5, [2.0, 3.0]])
    assert isinstance(k, cg.Sum) and len(k.args) == 3 and all(isinstance(t, cg.Product) for t in k.args)
    assert k.args[1].args[0].c == -0.5                                                      # a negative weight is kept
    assert cg.input_trait(k) == cg.GenericInput() and cg.input_trait(s) == cg.GenericInput()   # as in the reference
    assert cg.isstationary(s) and not cg.isisotropic(s)                                     # from the existing classes
    with pytest.raises(ValueError):
        cg.SM([1.0, 2.0], [[0.0]], [1.0, 1.0])


def test_call_equals_the_definition(cg):
    rng = np.random.default_rng(5)
    w = [1.2, -0.4, 0.8]; mu = [np.zeros(3), rng.standard_normal(3), rng.standard_normal(3)]
    l = [0.9, np.exp(0.3 * rng.standard_normal(3)), 1.7]
    k = cg.SM(w, mu, l)
    for _ in range(5):
        x, y = rng.standard_normal(3), rng.standard_normal(3)
        assert math.isclose(k(x, y), definition(w, mu, l, x, y), rel_tol=1e-13, abs_tol=1e-15)
    k1 = cg.Spectral(2.0, 0.35, 0.6)                                                        # scalar inputs
    assert math.isclose(k1(0.3, -0.4), 2.0 * math.cos(2 * math.pi * 0.35 * 0.7) * math.exp(-0.5 * (0.7 / 0.6) ** 2), rel_tol=1e-14)


def test_spec_of_the_constructors(cg):
    w = [1.2, -0.4]; mu = [[0.0, 0.0], [0.5, -1.5]]
    sp = cg.spectral_mixture_spec(cg.SM(w, mu, [0.5, 2.0]), 2)                               # scalar l
    assert sp is not None and all(a.dtype == np.float64 for a in sp)
    assert np.array_equal(sp[0], w) and np.array_equal(sp[1], mu) and np.allclose(sp[2], [[2.0, 2.0], [0.5, 0.5]], rtol=1e-15)
    sp = cg.spectral_mixture_spec(cg.SM(w, mu, [[0.5, 4.0], [2.0, 0.25]]), 2)               # vector l
    assert np.allclose(sp[2], [[2.0, 0.25], [0.5, 4.0]], rtol=1e-15) and sp[1].shape == (2, 2)
    assert cg.spectral_mixture_spec(cg.SM(w, mu, [0.5, 2.0])) is not None                    # d from the parameters themselves
    one = cg.spectral_mixture_spec(cg.Spectral(3.0, [0.1, 0.2, 0.3], 2.0), 3)                # a single term
    assert one[0].shape == (1,) and one[1].shape == (1, 3) and np.allclose(one[2], 0.5)
    assert cg.require_sm_spec(cg.SM(w, mu, [0.5, 2.0]), 2)[0].shape == (2,)


def test_spec_of_hand_built_expressions(cg):
    EQ, LS, Cos, Const = cg.EQ, cg.Lengthscale, cg.Cosine, cg.Constant
    sp = cg.spectral_mixture_spec(LS(LS(EQ(), 2.0), 3.0), 2)                                 # nested Lengthscale: l multiplies
    assert np.array_equal(sp[0], [1.0]) and np.array_equal(sp[1], [[0.0, 0.0]]) and np.allclose(sp[2], 1 / 6.0, rtol=1e-15)
    sp = cg.spectral_mixture_spec(cg.Product((LS(EQ(), 2.0), cg.ARD(EQ(), [1.0, 0.5]), Const(3.0), Const(0.5))), 2)   # two EQ factors
    assert np.allclose(sp[0], [1.5]) and np.allclose(sp[2] ** 2, [[0.25 + 1.0, 0.25 + 4.0]], rtol=1e-15)
    sp = cg.spectral_mixture_spec(cg.Sum((2.0 * EQ(), cg.Spectral(1.0, 0.3, 1.0))), 1)      # a term without Cosine: mu = 0
    assert np.array_equal(sp[1], [[0.0], [0.3]]) and np.array_equal(sp[0], [2.0, 1.0])
    sp = cg.spectral_mixture_spec(cg.Sum((2.0 * Cos([0.3, 0.1]), EQ())), 2)                  # a term without EQ: inv_l = 0
    assert np.array_equal(sp[2], [[0.0, 0.0], [1.0, 1.0]]) and np.array_equal(sp[1][0], [0.3, 0.1])
    k = 2.0 * Cos(0.7) * LS(EQ(), 0.5) + 0.5 * EQ()                                         # operators nest Products
    sp = cg.spectral_mixture_spec(k, 3)                                                      # a scalar c broadcasts to d
    assert np.array_equal(sp[0], [2.0, 0.5]) and np.array_equal(sp[1], [[0.7] * 3, [0.0] * 3]) and np.allclose(sp[2], [[2.0] * 3, [1.0] * 3])
    nested = cg.Sum((cg.Sum((cg.Spectral(1.0, 0.1, 1.0), cg.Spectral(2.0, 0.2, 1.0))), cg.Spectral(3.0, 0.3, 1.0)))   # nested Sums are flattened
    assert np.array_equal(cg.spectral_mixture_spec(nested, 1)[0], [1.0, 2.0, 3.0])


def test_refusals(cg):
    EQ, Cos = cg.EQ, cg.Cosine
    bad = [
        (cg.Product((Cos([0.1, 0.2]), cg.ScaledInputKernel(EQ(), np.array([[1.0, 0.5], [0.0, 1.0]])))), 2),   # a non-diagonal U
        (cg.Sum((cg.Spectral(1.0, 0.1, 1.0), cg.Product((Cos(0.2), cg.MaternP(1))))), 1),                        # another profile
        (cg.Product((Cos(0.1), Cos(0.2), EQ())), 1),                                                            # two Cosines in one term
        (cg.Sum((cg.Spectral(1.0, 0.1, 1.0), cg.Spectral(1.0, 0.2, 1.0) ** 2)), 1),                             # a Power
        (cg.SM(np.ones(33), [0.1 * q for q in range(33)], np.ones(33)), 1),                                     # Q = 33
        (cg.Spectral(1.0, np.full(17, 0.1), 1.0), 17),                                                          # d = 17
        (cg.Spectral(1.0, [0.1, 0.2], 1.0), 3),                                                                 # lengths disagree with d
        (cg.Product((cg.Sum((EQ(), Cos(0.1))), EQ())), 1),                                                      # no distribution over sums
    ]
    for k, d in bad:
        assert cg.spectral_mixture_spec(k, d) is None, (k, d)
        with pytest.raises(cg.UnsupportedKernel) as e:
            cg.require_sm_spec(k, d)
        assert type(k).__name__ in str(e.value) and "32" in str(e.value) and "16" in str(e.value)
    assert cg.spectral_mixture_spec(cg.SM(np.ones(32), [0.1 * q for q in range(32)], np.ones(32)), 1) is not None   # the limits themselves
    assert cg.spectral_mixture_spec(cg.Spectral(1.0, np.full(16, 0.1), 1.0), 16) is not None


def test_device_spec_of_pure_eq_sums_is_unchanged(cg):
    """Every kernel that has a route today keeps it: gramian() asks spectral_mixture_spec only where device_spec gives None."""
    k = cg.Lengthscale(cg.EQ(), 0.5) + 2.0 * cg.EQ()
    sp = cg.device_spec(k)
    assert isinstance(sp, cg._ffi.covgram_kernel_composite) and sp.nterms == 2 and sp.head.trait == cg._ffi.ISOTROPIC
    assert isinstance(cg.device_spec(cg.EQ()), cg._ffi.covgram_kernel)
    assert cg.device_spec(cg.SM([1.0, 2.0], [0.0, 0.3], [1.0, 0.5])) is None                  # mixed traits: GenericInput
    assert cg.device_spec(cg.Spectral(1.0, 0.3, 1.0)) is None


def test_abi_symbols_in_header_and_binding(cg):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "covgram.h")).read(), flags=re.S)
    protos = {m.group(1): [a for a in m.group(2).split(",") if a.strip()]
              for m in re.finditer(r"\bint\s+(covgram_sm_\w+)\s*\(([^;]*?)\)\s*;", header, re.S)}
    names = ("covgram_sm_create", "covgram_sm_info", "covgram_sm_mvm", "covgram_sm_matrix", "covgram_sm_destroy")
    assert set(protos) == set(names)
    for name in names:
        assert name in cg._ffi.PROTOTYPES, name
        assert len(cg._ffi.PROTOTYPES[name][1]) == len(protos[name]), name
    assert re.search(r"#define COVGRAM_SM_MAX_COMPONENTS 32\b", header) and re.search(r"#define COVGRAM_SM_MAX_D 16\b", header)
    assert (cg._ffi.SM_MAX_COMPONENTS, cg._ffi.SM_MAX_D) == (32, 16)
