"""CPU tier of the value-gradient-Hessian-kernel Gramian: the numpy reference of tests/vgh_ref.py is pinned against the derivative
definition from torch.func, and the host-side surface (class, trait, symbol in header / prototypes / exports, lowering check) is
checked."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hessian_ref as R
import vgh_ref as V
from test_hessian_host import KERNELS, torch_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_block(kern, x, y):
    """The (1 + d + d^2) x (1 + d + d^2) block from the definition: value, grad and hessian on the x side (rows) of the vector of value,
    grad and hessian on the y side (columns); Hessian component (a, b) at 1 + d + a + b d."""
    from torch.func import grad, hessian, jacfwd
    k = torch_kernel(kern)
    d = len(x)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)

    def cols(xx):
        kv = k(xx, yt)
        g = grad(lambda yy: k(xx, yy))(yt)
        H = hessian(lambda yy: k(xx, yy))(yt)
        return torch.cat([kv.reshape(1), g, H.T.reshape(-1)])
    bd = 1 + d + d * d
    T = np.empty((bd, bd))
    T[0] = cols(xt).numpy()
    T[1:1 + d] = jacfwd(cols)(xt).numpy().T                  # [column, a] -> row 1 + a
    H2 = hessian(cols)(xt).numpy()                           # [column, a, b]
    T[1 + d:] = H2.transpose(2, 1, 0).reshape(d * d, bd)     # row 1 + d + a + b d
    return T


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("kern", KERNELS, ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}-{k[3]}")
def test_reference_block_is_the_derivative_definition(kern, d):
    """Every entry of the reference block = (row functional on x, column functional on y) of k from torch.func (fp64), to 1e-11 of the
    block's largest entry; lengthscale != 1 and scale != 1 are among the kernels (a wrong power of gamma fails here)."""
    rng = np.random.default_rng(17 * d + len(kern[0]))
    x = rng.standard_normal(d); y = 0.8 * rng.standard_normal(d) + 0.1
    want = torch_block(kern, x, y)
    got = V.vgh_matrix(kern, x[None, :], y[None, :])
    assert got.shape == want.shape
    scale = max(np.abs(want).max(), np.abs(got).max())
    assert scale > 0
    print(f"vgh block {kern} d={d}: max error {np.abs(got - want).max():.3e}, largest entry {scale:.3e}")
    assert np.abs(got - want).max() <= 1e-11 * scale, (np.abs(got - want).max(), scale)


def test_reference_absolute_product_bounds_the_product():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((6, 3)); Y = rng.standard_normal((5, 3)); a = rng.standard_normal(5 * 13)
    for kern in KERNELS:
        assert np.all(np.abs(V.vgh_mul(kern, X, Y, a)) <= V.vgh_mul(kern, X, Y, a, absolute=True) * (1 + 1e-14))


def test_reference_reduces_to_the_hessian_reference():
    """a_v = a_g = 0: the Hessian part of the product is hessian_ref.hess_mul."""
    rng = np.random.default_rng(6)
    d = 3
    X = rng.standard_normal((6, d)); Y = rng.standard_normal((5, d))
    a = rng.standard_normal((5, 1 + d + d * d)); a[:, :1 + d] = 0.0
    for kern in KERNELS:
        for absolute in (False, True):
            got = V.vgh_mul(kern, X, Y, a.reshape(-1), absolute=absolute).reshape(6, -1)[:, 1 + d:]
            want = R.hess_mul(kern, X, Y, a[:, 1 + d:].reshape(-1), absolute=absolute).reshape(6, -1)
            assert np.abs(got - want).max() <= 1e-13 * max(np.abs(want).max(), 1e-300), kern


def test_kernel_class_and_trait(cg):
    for k in (cg.EQ(), cg.Lengthscale(cg.RQ(1.5), 0.7), cg.ExponentialDot(), cg.Dot(), cg.EQ() + cg.Cauchy()):
        h = cg.ValueGradientHessianKernel(k)
        assert isinstance(h, cg.MultiKernel)
        assert cg.input_trait(h) == cg.input_trait(k)
    assert cg.input_trait(cg.ValueGradientHessianKernel(cg.EQ())) == cg.IsotropicInput()
    assert cg.input_trait(cg.ValueGradientHessianKernel(cg.Dot())) == cg.DotProductInput()
    assert issubclass(cg.ValueGradientHessianGramian, cg.BlockGramian)


def test_symbol_in_header_prototypes_and_exports(cg):
    header = open(os.path.join(ROOT, "include", "covgram.h")).read()
    decl = re.search(r"int\s+covgram_valgradhess_mvm\s*\(([^;]*)\)\s*;", header)
    assert decl, "covgram_valgradhess_mvm is not declared in include/covgram.h"
    grad = re.search(r"int\s+covgram_grad_mvm\s*\(([^;]*)\)\s*;", header)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert norm(decl.group(1)) == norm(grad.group(1)), "covgram_valgradhess_mvm must have exactly the signature of covgram_grad_mvm"
    assert "covgram_valgradhess_mvm" in cg._ffi.PROTOTYPES
    assert cg._ffi.PROTOTYPES["covgram_valgradhess_mvm"] == cg._ffi.PROTOTYPES["covgram_grad_mvm"]
    lib = os.path.join(ROOT, "covariancefunctions.jl_amd", "lib", "libcovgram.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT covgram_valgradhess_mvm\b", out), "libcovgram.so does not export covgram_valgradhess_mvm"
    assert cg._ffi.lib().covgram_version() == 113


def test_supported_kernels_lower_to_one_profile(cg):
    L = cg.Lengthscale
    for k, fam in ((cg.EQ(), cg._ffi.EQ), (2.0 * L(cg.RQ(1.5), 0.7), cg._ffi.RQ), (cg.Cauchy(), cg._ffi.CAUCHY),
                   (L(cg.InverseMultiQuadratic(1.3), 2.0), cg._ffi.IMQ), (cg.ExponentialDot(), cg._ffi.EXPDOT), (cg.Dot(), cg._ffi.DOT)):
        spec = cg.require_vgh_spec(k, 32)
        assert spec.family == fam and spec.power == 1
    assert cg.require_vgh_spec(2.0 * L(cg.RQ(1.5), 0.7)).scale == 2.0


@pytest.mark.parametrize("make,word", [
    (lambda cg: cg.MaternP(2), "MaternP"), (lambda cg: cg.EQ() + cg.Cauchy(), "Sum"), (lambda cg: cg.EQ() * cg.RQ(1.0), "Product"),
    (lambda cg: cg.EQ() ** 2, "Power"), (lambda cg: cg.Exp(), "Exponential"), (lambda cg: cg.GammaExp(1.5), "GammaExponential"),
    (lambda cg: cg.Matern(1.3), "Matern"), (lambda cg: cg.AsinDot(), "AsinDot"), (lambda cg: cg.Dot() ** 3, "Power")])
def test_unsupported_kernels_raise_before_any_device_call(cg, make, word):
    """The lowering check needs no GPU: it raises UnsupportedKernel with a message that names the kernel."""
    k = make(cg)
    with pytest.raises(cg.UnsupportedKernel) as e:
        cg.require_vgh_spec(k, 3)
    assert word in str(e.value) and "ValueGradientHessianKernel" in str(e.value)


def test_dimension_beyond_32_is_unsupported(cg):
    cg.require_vgh_spec(cg.EQ(), 32)
    with pytest.raises(cg.UnsupportedKernel, match="33") as e:
        cg.require_vgh_spec(cg.EQ(), 33)
    assert "ValueGradientHessianKernel" in str(e.value)
