"""CPU tier of the Hessian-kernel Gramian: the numpy reference of tests/hessian_ref.py is pinned against a fourth-order torch.func
derivative, and the host-side surface (class, trait, symbol in header / prototypes / exports, lowering check) is checked."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hessian_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = [("EQ", 0.0, 1.0, 1.0), ("EQ", 0.0, 0.8, 1.7), ("RQ", 1.5, 0.7, 1.0), ("Cauchy", 0.0, 1.0, 1.0), ("Cauchy", 0.0, 1.3, 0.5),
           ("IMQ", 1.3, 1.0, 1.0), ("IMQ", 0.9, 1.4, 2.0), ("ExponentialDot", 0.0, 1.0, 1.0), ("ExponentialDot", 0.0, 1.0, 0.6),
           ("Dot", 0.0, 1.0, 1.0)]


def torch_kernel(kern):
    name, p, l, scale = kern

    def k(x, y):
        if name in R.ISO:
            s = ((x - y) ** 2).sum() / (l * l)
        else:
            s = (x * y).sum()
        f = {"EQ": lambda: torch.exp(-s / 2), "RQ": lambda: (1 + s / (2 * p)) ** (-p), "Cauchy": lambda: 1 / (1 + s),
             "IMQ": lambda: 1 / torch.sqrt(s + p * p), "ExponentialDot": lambda: torch.exp(s), "Dot": lambda: s}[name]()
        return scale * f
    return k


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("kern", KERNELS, ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}-{k[3]}")
def test_reference_block_is_the_fourth_derivative(kern, d):
    """T[(a,b),(c,e)] of the reference = d^4 k / dx_a dx_b dy_c dy_e from torch.func (fp64), to 1e-11 of the block's largest entry."""
    from torch.func import hessian
    rng = np.random.default_rng(17 * d + len(kern[0]))
    x = rng.standard_normal(d); y = 0.8 * rng.standard_normal(d) + 0.1
    k = torch_kernel(kern)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    T4 = hessian(lambda xx: hessian(lambda yy: k(xx, yy))(yt))(xt).numpy()          # [c, e, a, b]
    want = T4.transpose(3, 2, 1, 0).reshape(d * d, d * d)                           # row a + b d, column c + e d
    got = R.hess_matrix(kern, x[None, :], y[None, :])
    scale = max(np.abs(want).max(), np.abs(got).max())
    if kern[0] == "Dot":
        assert scale == 0.0
        return
    assert scale > 0
    assert np.abs(got - want).max() <= 1e-11 * scale, (np.abs(got - want).max(), scale)


def test_reference_absolute_product_bounds_the_product():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((6, 3)); Y = rng.standard_normal((5, 3)); a = rng.standard_normal(5 * 9)
    for kern in KERNELS:
        assert np.all(np.abs(R.hess_mul(kern, X, Y, a)) <= R.hess_mul(kern, X, Y, a, absolute=True) * (1 + 1e-14))


def test_hessian_kernel_class_and_trait(cg):
    for k in (cg.EQ(), cg.Lengthscale(cg.RQ(1.5), 0.7), cg.ExponentialDot(), cg.Dot(), cg.EQ() + cg.Cauchy()):
        h = cg.HessianKernel(k)
        assert isinstance(h, cg.MultiKernel)
        assert cg.input_trait(h) == cg.input_trait(k)
    assert cg.input_trait(cg.HessianKernel(cg.EQ())) == cg.IsotropicInput()
    assert cg.input_trait(cg.HessianKernel(cg.Dot())) == cg.DotProductInput()


def test_symbol_in_header_prototypes_and_exports(cg):
    header = open(os.path.join(ROOT, "include", "covgram.h")).read()
    decl = re.search(r"int\s+covgram_hess_mvm\s*\(([^;]*)\)\s*;", header)
    assert decl, "covgram_hess_mvm is not declared in include/covgram.h"
    grad = re.search(r"int\s+covgram_grad_mvm\s*\(([^;]*)\)\s*;", header)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert norm(decl.group(1)) == norm(grad.group(1)), "covgram_hess_mvm must have exactly the signature of covgram_grad_mvm"
    assert "covgram_hess_mvm" in cg._ffi.PROTOTYPES
    assert cg._ffi.PROTOTYPES["covgram_hess_mvm"] == cg._ffi.PROTOTYPES["covgram_grad_mvm"]
    lib = os.path.join(ROOT, "covariancefunctions.jl_amd", "lib", "libcovgram.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT covgram_hess_mvm\b", out), "libcovgram.so does not export covgram_hess_mvm"
    assert cg._ffi.lib().covgram_version() == 113


def test_supported_kernels_lower_to_one_profile(cg):
    L = cg.Lengthscale
    for k, fam in ((cg.EQ(), cg._ffi.EQ), (2.0 * L(cg.RQ(1.5), 0.7), cg._ffi.RQ), (cg.Cauchy(), cg._ffi.CAUCHY),
                   (L(cg.InverseMultiQuadratic(1.3), 2.0), cg._ffi.IMQ), (cg.ExponentialDot(), cg._ffi.EXPDOT), (cg.Dot(), cg._ffi.DOT)):
        spec = cg.require_hessian_spec(k, 32)
        assert spec.family == fam and spec.power == 1
    assert cg.require_hessian_spec(2.0 * L(cg.RQ(1.5), 0.7)).scale == 2.0


@pytest.mark.parametrize("make,word", [
    (lambda cg: cg.MaternP(2), "MaternP"), (lambda cg: cg.EQ() + cg.Cauchy(), "Sum"), (lambda cg: cg.EQ() * cg.RQ(1.0), "Product"),
    (lambda cg: cg.EQ() ** 2, "Power"), (lambda cg: cg.Exp(), "Exponential"), (lambda cg: cg.GammaExp(1.5), "GammaExponential"),
    (lambda cg: cg.Matern(1.3), "Matern"), (lambda cg: cg.AsinDot(), "AsinDot"), (lambda cg: cg.Dot() ** 3, "Power")])
def test_unsupported_kernels_raise_before_any_device_call(cg, make, word):
    """The lowering check needs no GPU: it raises UnsupportedKernel with a message that names the kernel."""
    k = make(cg)
    with pytest.raises(cg.UnsupportedKernel) as e:
        cg.require_hessian_spec(k, 3)
    assert word in str(e.value) and "HessianKernel" in str(e.value)


def test_dimension_beyond_32_is_unsupported(cg):
    cg.require_hessian_spec(cg.EQ(), 32)
    with pytest.raises(cg.UnsupportedKernel, match="33"):
        cg.require_hessian_spec(cg.EQ(), 33)
