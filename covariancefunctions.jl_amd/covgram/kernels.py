"""Kernel structs and `input_trait` — the host-side mirror of the reference's kernel zoo for the hot path.

Same names, argument meaning and error behaviour as CovarianceFunctions.jl (citations relative to the
reference root).  A kernel object is a *description*; `device_spec(k)` lowers it to the C struct
`covgram_kernel` that selects the HIP kernel, exactly the role `input_trait(k)` plays in the
reference (src/properties.jl:31-63, README.md:90-99).  Calling a kernel, `k(x, y)`, evaluates the
scalar definition on the host for single pairs (API parity with the Julia call operators); the MVM,
`Matrix(G)` and Toeplitz/Kronecker constructions never use it — they run on the device.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

from . import _ffi

# ----------------------------------------------------------------------------------------------
# input traits (src/properties.jl:31-37)
# ----------------------------------------------------------------------------------------------


class InputTrait:
    def __eq__(self, other):
        return type(self) is type(other)

    def __hash__(self):
        return hash(type(self).__name__)

    def __repr__(self):
        return type(self).__name__ + "()"


class GenericInput(InputTrait): pass
class IsotropicInput(InputTrait): pass            # dependent on |r|²
class DotProductInput(InputTrait): pass           # dependent on x ⋅ y
class StationaryInput(InputTrait): pass           # dependent on r
class StationaryLinearFunctionalInput(InputTrait): pass   # dependent on c ⋅ r
class PeriodicInput(InputTrait): pass


class DomainError(ValueError):
    pass


def _dot(x, y):
    return float(np.dot(np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(y, dtype=np.float64))))


def _euclidean2(x, y):
    """src/util.jl:40-47 — direct differences, DimensionMismatch on unequal lengths."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64)); y = np.atleast_1d(np.asarray(y, dtype=np.float64))
    if x.shape != y.shape:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"inputs have to have the same length: {x.size}, {y.size}")
    d = x - y
    return float(np.dot(d, d))


# ----------------------------------------------------------------------------------------------
# type tree (src/CovarianceFunctions.jl:32-40)
# ----------------------------------------------------------------------------------------------
class AbstractKernel:
    def __mul__(self, other):
        if isinstance(other, (int, float)):
            return Product((Constant(other), self))          # src/algebra.jl:24-25
        if isinstance(other, AbstractKernel):
            return Product((self, other))
        return NotImplemented

    __rmul__ = __mul__

    def __add__(self, other):
        if isinstance(other, (int, float)):
            return Sum((self, Constant(other)))              # src/algebra.jl:46-47
        if isinstance(other, AbstractKernel):
            return Sum((self, other))
        return NotImplemented

    __radd__ = __add__

    def __pow__(self, p):
        return Power(self, p)                                # src/algebra.jl:63


class MercerKernel(AbstractKernel): pass
class StationaryKernel(MercerKernel): pass


class IsotropicKernel(StationaryKernel):
    """(k::IsotropicKernel)(x, y) = k(euclidean2(x, y)); one-argument form takes r² (src/stationary.jl:9-10)."""

    def profile(self, s: float) -> float:
        raise NotImplementedError

    def __call__(self, *args):
        if len(args) == 2:
            return self.profile(_euclidean2(args[0], args[1]))
        (a,) = args
        if np.ndim(a) == 0:
            return self.profile(float(a))                    # k(r²)
        a = np.asarray(a, dtype=np.float64)
        return self.profile(float(np.dot(a, a)))             # k(τ) = k(sum(abs2, τ))


class MultiKernel(AbstractKernel): pass


class Constant(IsotropicKernel):
    """src/stationary.jl:15-34."""

    def __init__(self, c, check: bool = True):
        if check and not (c >= 0):
            raise DomainError(f"Constant is not positive semi-definite: {c}")
        self.c = float(c)
        self.check = bool(check)                               # with_hyperparameters rebuilds a signed weight the way it was built

    def profile(self, s):
        return self.c

    def __call__(self, *args):
        return self.c


class ExponentiatedQuadratic(IsotropicKernel):
    def profile(self, s):
        return math.exp(-s / 2)                              # src/stationary.jl:42


EQ = ExponentiatedQuadratic


class RationalQuadratic(IsotropicKernel):
    def __init__(self, alpha):
        if not alpha > 0:
            raise DomainError("α not positive")             # src/stationary.jl:47
        self.alpha = float(alpha)

    def profile(self, s):
        return (1 + s / (2 * self.alpha)) ** (-self.alpha)   # src/stationary.jl:53


RQ = RationalQuadratic


class Exponential(IsotropicKernel):
    def profile(self, s):
        return math.exp(-math.sqrt(s))                       # src/stationary.jl:60


Exp = Exponential


class GammaExponential(IsotropicKernel):
    def __init__(self, gamma):
        if not (0 <= gamma <= 2):
            raise DomainError("γ not in [0,2]")             # src/stationary.jl:65
        self.gamma = float(gamma)

    def profile(self, s):
        return math.exp(-(s ** (self.gamma / 2)) / 2)        # src/stationary.jl:71


GammaExp = GammaExponential


class Cauchy(IsotropicKernel):
    def profile(self, s):
        return 1.0 / (1.0 + s)                               # src/stationary.jl:224


class InverseMultiQuadratic(IsotropicKernel):
    def __init__(self, c):
        self.c = float(c)

    def profile(self, s):
        return 1.0 / math.sqrt(s + self.c ** 2)              # src/stationary.jl:235


def maternp_coefficients(p: int):
    """src/stationary.jl:184-191 (reversed binomial(p,i) * (p+i)!/p!)."""
    fp = math.factorial(p)
    return [math.comb(p, i) * (math.factorial(p + i) // fp) for i in range(1, p + 1)][::-1]


def maternp_derivatives_at_zero(p: int):
    """src/stationary.jl:172-182 — SymEngine there; here from the exact power series of exp(-r) q_p(r)."""
    from fractions import Fraction
    c = [Fraction(v) for v in maternp_coefficients(p)] + [Fraction(1)]
    nrm = math.factorial(2 * p) // math.factorial(p)
    h = [c[m] * 2 ** m / nrm for m in range(p + 1)]
    out = []
    for i in range(1, p + 1):
        coef = sum(h[m] * Fraction((-1) ** (2 * i - m), math.factorial(2 * i - m)) for m in range(0, min(p, 2 * i) + 1))
        out.append(float(coef * (2 * p + 1) ** i * math.factorial(i)))
    return out


class MaternP(IsotropicKernel):
    """Matern with ν = p + 1/2 (src/stationary.jl:117-158), including the Taylor guard near zero."""

    def __init__(self, p):
        if isinstance(p, Matern):
            p = int(math.floor(p.nu))                        # src/stationary.jl:130
        if p < 0:
            raise DomainError(f"p = {p} is negative")        # src/stationary.jl:124
        self.p = int(p)
        self.coefficients = [float(v) for v in maternp_coefficients(self.p)]
        self.derivatives = maternp_derivatives_at_zero(self.p)

    def profile(self, s, eps=np.finfo(np.float64).eps):
        p = self.p
        if p >= 1 and s < eps ** (1.0 / p):                  # src/stationary.jl:135-146
            y, si = 1.0, s
            for i in range(1, p + 1):
                y += self.derivatives[i - 1] * si / math.factorial(i)
                si *= s
            return y
        r = math.sqrt((2 * p + 1) * s)
        y, ri = 0.0, 1.0
        for i in range(p):
            y += self.coefficients[i] * ri
            ri *= 2 * r
        y += ri
        return y * math.exp(-r) / (math.factorial(2 * p) // math.factorial(p))


class Matern(IsotropicKernel):
    """src/stationary.jl:87-114 (Bessel form, real ν > 0); on the device Temme's series / Steed's continued fraction."""

    def __init__(self, nu):
        if not nu > 0:
            raise DomainError(f"ν = {nu} is negative")
        self.nu = float(nu)

    def profile(self, s):
        from scipy.special import gamma, kv
        nu = self.nu
        if s == 0:
            return 1.0
        r = math.sqrt(2 * nu * s)
        return 2 ** (1 - nu) / gamma(nu) * r ** nu * kv(nu, r)


class DotProductKernel(MercerKernel):
    """(k::DotProductKernel)(x, y) = k(dot(x, y)) (src/mercer.jl:2-3)."""

    def profile(self, s):
        raise NotImplementedError

    def __call__(self, *args):
        if len(args) == 2:
            return self.profile(_dot(args[0], args[1]))
        return self.profile(float(args[0]))


class Dot(DotProductKernel):
    def profile(self, s):
        return s                                             # src/mercer.jl:9


class ExponentialDot(DotProductKernel):
    def profile(self, s):
        return math.exp(s)                                   # src/mercer.jl:22


def Line(sigma: float = 0.0):
    """Line(σ) = Dot() + σ (src/mercer.jl:12)."""
    return Dot() + sigma


def Polynomial(d: int, sigma: float = 0.0):
    """Polynomial(d, σ) = Line(σ)^d (src/mercer.jl:13-14); lowers to a composite of Dot powers on the device."""
    return Line(sigma) ** int(d)


Poly = Polynomial


class CosineKernel(StationaryKernel):
    """k(x, y) = cos(2π c·(x − y)) (src/stationary.jl:197-211), input_trait = StationaryLinearFunctionalInput.
    cos(u_i − v_j) = cos u_i cos v_j + sin u_i sin v_j: its Gramian has rank 2 (the reference's own "IDEA: trig-identity ->
    low-rank gramian", :204) and is represented as such here."""

    def __init__(self, c):
        self.c = np.atleast_1d(np.asarray(c, dtype=np.float64))

    def __call__(self, *args):
        if len(args) == 2:
            x = np.atleast_1d(np.asarray(args[0], dtype=np.float64)); y = np.atleast_1d(np.asarray(args[1], dtype=np.float64))
            c = self.c if self.c.size != 1 else np.broadcast_to(self.c, x.shape)   # a scalar c over d dimensions, as spectral_mixture_spec reads it
            return math.cos(2 * math.pi * float(np.dot(c, x - y)))
        return math.cos(2 * math.pi * float(args[0]))


Cosine = Cos = CosineKernel


def Spectral(w, mu, l):
    """Spectral(w, μ, l) = prod((w, Cosine(μ), ARD(EQ(), l))) (src/stationary.jl:215): a Product of Constant(w), Cosine(μ) and the EQ
    kernel under a scalar (Lengthscale) or per-dimension (ScaledInputKernel) lengthscale.  A weight of either sign is taken as it is
    (Constant(w, check = False)): a mixture may carry negative weights."""
    return Product((Constant(w, False), CosineKernel(mu), ARD(ExponentiatedQuadratic(), l)))


def SpectralMixture(w, mu, l):
    """SpectralMixture(w, μ, l) = sum(Spectral.(w, μ, l)) (src/stationary.jl:216): w of length Q, μ and l with one entry (a number or a
    length-d vector) per component."""
    w = list(np.atleast_1d(np.asarray(w, dtype=np.float64)))
    if not (len(mu) == len(w) and len(l) == len(w)):
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"SpectralMixture: {len(w)} weights, {len(mu)} frequencies and {len(l)} lengthscales")
    return Sum(tuple(Spectral(wq, mq, lq) for wq, mq, lq in zip(w, mu, l)))


SM = SpectralMixture


class Periodic(StationaryKernel):
    """Periodic(k)(τ) = k((2 sin(πτ))²) for 1-D inputs (src/transformation.jl:54-65): the isotropic kernel k on the circle
    embedding e(x) = (cos 2πx, sin 2πx), since |e(x) − e(y)|² = 4 sin²(π(x − y))."""

    def __init__(self, k):
        if not isinstance(k, IsotropicKernel):
            raise TypeError("Periodic(k::IsotropicKernel)")
        self.k = k

    def __call__(self, *args):
        tau = float(args[0]) - float(args[1]) if len(args) == 2 else float(args[0])
        return self.k.profile((2 * math.sin(math.pi * tau)) ** 2)


class ScaledInputKernel(AbstractKernel):
    """ScaledInputKernel(k, U)(x, y) = k(U x, U y) (src/transformation.jl:71-79); `gramian` pre-multiplies the points once
    (:82-90).  ARD(k, l) (:42-46) is the diagonal case U = Diagonal(1 ./ l)."""

    def __init__(self, k, U, l=None):
        self.k = k
        self.U = np.asarray(U, dtype=np.float64)
        self.diagonal = self.U.ndim == 1
        self.l = None if l is None else np.asarray(l, dtype=np.float64)   # ARD(k, l): the lengthscales it was built from (hyperparameters)

    def __call__(self, x, y):
        x = np.atleast_1d(np.asarray(x, dtype=np.float64)); y = np.atleast_1d(np.asarray(y, dtype=np.float64))
        return self.k(self.U * x, self.U * y) if self.diagonal else self.k(self.U @ x, self.U @ y)


def ARD(k, l):
    """Automatic relevance determination (src/transformation.jl:42-46): k on inputs scaled by 1 ./ l; scalar l = Lengthscale."""
    if np.ndim(l) == 0:
        return Lengthscale(k, l)
    l = np.asarray(l, dtype=np.float64)
    if not np.all(l > 0):
        raise DomainError(f"l = {l} is non-positive")
    return ScaledInputKernel(k, 1.0 / l, l=l)


class Warped(AbstractKernel):
    """Warped(k, u)(x, y) = k(u(x), u(y)) (src/transformation.jl:98-110); u is a matrix or a callable that maps an (n, d) tensor of
    points to an (n, d') tensor (vectorised over points); `gramian` warps the points once (:114-118)."""

    def __init__(self, k, u):
        self.k = k
        self.u = u

    def __call__(self, x, y):
        u = (lambda z: np.asarray(self.u) @ z) if not callable(self.u) else (lambda z: np.asarray(self.u(np.atleast_2d(z)))[0])
        return self.k(u(np.atleast_1d(np.asarray(x, dtype=np.float64))), u(np.atleast_1d(np.asarray(y, dtype=np.float64))))


class VerticalRescaling(AbstractKernel):
    """VerticalRescaling(k, f)(x, y) = f(x) k(x, y) f(y) (src/transformation.jl:156-171): Diagonal · gramian(k) · Diagonal; f is
    vectorised over an (n, d) tensor of points and returns n values."""

    def __init__(self, k, f):
        self.k, self.f = k, f

    def __call__(self, x, y):
        fx = float(np.asarray(self.f(np.atleast_2d(np.asarray(x, dtype=np.float64)))).reshape(-1)[0])
        fy = float(np.asarray(self.f(np.atleast_2d(np.asarray(y, dtype=np.float64)))).reshape(-1)[0])
        return fx * self.k(x, y) * fy


class AsinDot(DotProductKernel):
    """φ(s) = (2/π) asin(s): what the NeuralNetwork kernel is on its normalised augmented inputs (device family ASINDOT)."""

    def profile(self, s):
        return 2 / math.pi * math.asin(s)


class NeuralNetwork(MercerKernel):
    """NN(σ)(x, y) = 2/π asin(l(x,y) / sqrt((1 + l(x,x)) (1 + l(y,y)))), l = Line(σ) = x·y + σ (src/mercer.jl:73-85).
    With x̂ = [x, √σ] / sqrt(1 + |x|² + σ) this is AsinDot on (x̂, ŷ): `gramian` warps the points once and the dot-product
    hot path does the rest; the gradient Gramian follows by the chain rule through the warp (per-point Jacobians, O(d) each),
    which for σ = 0 is exactly the reference's Woodbury block (src/gradient.jl:187-210)."""

    def __init__(self, sigma: float = 0.0):
        if sigma < 0:
            raise DomainError(f"σ = {sigma} is negative")
        self.sigma = float(sigma)

    def __call__(self, x, y):
        x = np.atleast_1d(np.asarray(x, dtype=np.float64)); y = np.atleast_1d(np.asarray(y, dtype=np.float64))
        l = lambda u, v: float(np.dot(u, v)) + self.sigma
        return 2 / math.pi * math.asin(l(x, y) / math.sqrt((1 + l(x, x)) * (1 + l(y, y))))


NN = NeuralNetwork


class FiniteBasis(MercerKernel):
    """src/mercer.jl:41-70: k(x,y) = Σ_b b(x) b(y); basis functions are vectorised callables."""

    def __init__(self, basis: Sequence):
        if len(basis) < 1:
            raise ValueError(f"basis is empty: length(basis) = {len(basis)}")
        self.basis = list(basis)

    def __call__(self, x, y):
        return float(sum(b(x) * b(y) for b in self.basis))


# ----------------------------------------------------------------------------------------------
# algebra (src/algebra.jl) and Lengthscale (src/transformation.jl:6-19)
# ----------------------------------------------------------------------------------------------
def sum_and_product_input_trait(args):
    """src/properties.jl:47-63: common trait of the non-Constant arguments, else GenericInput."""
    non_const = [k for k in args if not isinstance(k, Constant)]
    if not non_const:
        return IsotropicInput()
    trait = input_trait(non_const[0])
    for k in non_const[1:]:
        if input_trait(k) != trait:
            return GenericInput()
    return trait


class Product(AbstractKernel):
    def __init__(self, args):
        self.args = tuple(args)
        self.input_trait = sum_and_product_input_trait(self.args)

    def __call__(self, *a):
        out = 1.0
        for k in self.args:
            out *= k(*a)
        return out


class Sum(AbstractKernel):
    def __init__(self, args):
        self.args = tuple(args)
        self.input_trait = sum_and_product_input_trait(self.args)

    def __call__(self, *a):
        return sum(k(*a) for k in self.args)


class Power(AbstractKernel):
    def __init__(self, k, p):
        if int(p) != p:
            raise TypeError("Power exponent must be an Int (src/algebra.jl:52)")
        self.k, self.p = k, int(p)
        self.input_trait = input_trait(k)

    def __call__(self, *a):
        return self.k(*a) ** self.p


class Lengthscale(IsotropicKernel):
    def __init__(self, k, l):
        if not isinstance(k, IsotropicKernel):
            raise TypeError("Lengthscale(k::IsotropicKernel, l)")
        if np.ndim(l) != 0 and np.size(l) != 1:
            raise _ffi.DimensionMismatch(_ffi.EINVAL, "lengthscale l has to has length 1")
        l = float(np.asarray(l).reshape(()))
        if not l > 0:
            raise DomainError(f"l = {l} is non-positive")    # src/transformation.jl:10
        self.k, self.l = k, l

    def profile(self, s):
        return self.k.profile(s / self.l ** 2)               # src/transformation.jl:19


class SeparableProduct(AbstractKernel):
    """src/algebra.jl:68-95: product kernel evaluating component kernels on separate input dimensions."""

    def __init__(self, *args):
        self.args = tuple(args[0]) if len(args) == 1 and isinstance(args[0], (tuple, list)) else tuple(args)

    def __call__(self, x, y):
        x = np.atleast_1d(x); y = np.atleast_1d(y)
        if len(x) != len(y):
            raise _ffi.DimensionMismatch(_ffi.EINVAL, f"length(x) ({len(x)}) ≠ length(y) ({len(y)})")
        if len(self.args) != len(x):
            raise _ffi.DimensionMismatch(_ffi.EINVAL, f"SeparableProduct needs d = {len(x)} kernels but has r = {len(self.args)}")
        out = 1.0
        for ki, xi, yi in zip(self.args, x, y):
            out *= ki(xi, yi)
        return out


def separable(op, *k):
    """src/algebra.jl:140-143."""
    import operator
    if op in (operator.mul, "*"):
        return SeparableProduct(*k)
    if op in (operator.pow, "^", "**"):
        kern, d = k
        return SeparableProduct(*([kern] * int(d)))
    raise NotImplementedError("separable(+, ...) has no structured Gramian in the reference either (src/algebra.jl:125-138)")


class SeparableKernel(MultiKernel):
    """SeparableKernel(B, k): matrix-valued kernel B * k(x, y) (src/separable.jl:2-16)."""

    def __init__(self, B, k=None):
        if isinstance(B, AbstractKernel):   # Separable(k, B) argument order used in test/separable.jl:13
            B, k = k, B
        self.B = np.asarray(B, dtype=np.float64)
        self.k = k

    def __call__(self, x, y):
        return self.B * self.k(x, y)


Separable = SeparableKernel


class GradientKernel(MultiKernel):
    """src/gradient.jl:7-24: the d×d block kernel ∂x ∂yᵀ k(x, y); carries input_trait(k)."""

    def __init__(self, k, it: Optional[InputTrait] = None):
        self.k = k
        self.input_trait = input_trait(k) if it is None else it


class ValueGradientKernel(MultiKernel):
    """src/gradient.jl:400-411: the (d+1)×(d+1) block kernel of [f, ∂f]; carries input_trait(k)."""

    def __init__(self, k, it: Optional[InputTrait] = None):
        self.k = k
        self.input_trait = input_trait(k) if it is None else it


class HessianKernel(MultiKernel):
    """src/hessian.jl:2-23: the d²×d² block kernel ∂x ∂xᵀ ∂y ∂yᵀ k(x, y); carries input_trait(k) (src/hessian.jl:7)."""

    def __init__(self, k, it: Optional[InputTrait] = None):
        self.k = k
        self.input_trait = input_trait(k) if it is None else it


class ValueGradientHessianKernel(MultiKernel):
    """src/hessian.jl:279-299: the (1+d+d²)×(1+d+d²) block kernel of [f, ∂f, vec ∂²f]; carries input_trait(k) (src/hessian.jl:283)."""

    def __init__(self, k, it: Optional[InputTrait] = None):
        self.k = k
        self.input_trait = input_trait(k) if it is None else it


# ----------------------------------------------------------------------------------------------
# input_trait (src/properties.jl:39-45, gradient.jl:16) — user-extensible like the reference
# ----------------------------------------------------------------------------------------------
_USER_TRAITS = {}


def register_input_trait(obj_or_type, trait: InputTrait):
    """Counterpart of defining `CovarianceFunctions.input_trait(::typeof(k)) = ...` (test/gramian.jl:163)."""
    _USER_TRAITS[obj_or_type if isinstance(obj_or_type, type) else id(obj_or_type)] = trait


def input_trait(k) -> InputTrait:
    if id(k) in _USER_TRAITS:
        return _USER_TRAITS[id(k)]
    for t, tr in _USER_TRAITS.items():
        if isinstance(t, type) and isinstance(k, t):
            return tr
    if isinstance(k, (Product, Sum, Power, GradientKernel, ValueGradientKernel, HessianKernel, ValueGradientHessianKernel)):
        return k.input_trait
    if isinstance(k, (Dot, ExponentialDot, AsinDot)):
        return DotProductInput()
    if isinstance(k, CosineKernel):
        return StationaryLinearFunctionalInput()             # src/stationary.jl:206
    if isinstance(k, IsotropicKernel):
        return IsotropicInput()
    if isinstance(k, StationaryKernel):
        return StationaryInput()
    return GenericInput()


def ismercer(k): return isinstance(k, MercerKernel) or (isinstance(k, (Product, Sum)) and all(ismercer(a) for a in k.args)) or (isinstance(k, Power) and ismercer(k.k))
def isstationary(k): return isinstance(k, StationaryKernel) or (isinstance(k, (Product, Sum)) and all(isstationary(a) for a in k.args)) or (isinstance(k, Power) and isstationary(k.k))
def isisotropic(k): return isinstance(k, IsotropicKernel) or (isinstance(k, (Product, Sum)) and all(isisotropic(a) for a in k.args)) or (isinstance(k, Power) and isisotropic(k.k))
def isdot(k): return isinstance(k, (Dot, ExponentialDot)) or (isinstance(k, (Product, Sum)) and all(isdot(a) for a in k.args)) or (isinstance(k, Power) and isdot(k.k))


# ----------------------------------------------------------------------------------------------
# lowering to the C struct
# ----------------------------------------------------------------------------------------------
_BASE = {
    ExponentiatedQuadratic: _ffi.EQ, Exponential: _ffi.EXP, RationalQuadratic: _ffi.RQ, GammaExponential: _ffi.GAMMAEXP,
    Cauchy: _ffi.CAUCHY, InverseMultiQuadratic: _ffi.IMQ, MaternP: _ffi.MATERNP, Dot: _ffi.DOT, ExponentialDot: _ffi.EXPDOT,
    Matern: _ffi.MATERN, AsinDot: _ffi.ASINDOT,
}


def _simple_spec(k) -> Optional[_ffi.covgram_kernel]:
    """covgram_kernel for a single profile, or None.

    Handles base profiles, Lengthscale nesting, Power (exponents multiply; (c·k)^p = c^p k^p) and
    products with Constants (scale) — the compositions that keep the IsotropicInput / DotProductInput
    trait of a single profile."""
    scale, power, ls = 1.0, 1, 1.0
    while True:
        if isinstance(k, Product):
            consts = [a for a in k.args if isinstance(a, Constant)]
            rest = [a for a in k.args if not isinstance(a, Constant)]
            if len(rest) != 1:
                return None
            for c in consts:
                scale *= c.c ** power
            k = rest[0]
        elif isinstance(k, Power):
            if k.p < 1:
                return None
            power *= k.p
            k = k.k
        elif isinstance(k, Lengthscale):
            ls *= k.l
            k = k.k
        else:
            break
    fam = _BASE.get(type(k))
    if fam is None:
        return None
    if fam == _ffi.MATERN and float(k.nu - 0.5).is_integer() and 0 <= int(k.nu - 0.5) <= _ffi.MATERNP_MAX_P:
        # half-integer ν: the same function has the closed form of MaternP(ν − 1/2) (the reference's own "IDEA: use rational types
        # to dispatch to MaternP evaluation", src/stationary.jl:85) — ~50x cheaper per pair than the Bessel-function path
        k = MaternP(int(k.nu - 0.5))
        fam = _ffi.MATERNP
    spec = _ffi.covgram_kernel()
    spec.family = fam
    spec.trait = _ffi.DOTPRODUCT if fam in (_ffi.DOT, _ffi.EXPDOT, _ffi.ASINDOT) else _ffi.ISOTROPIC
    spec.p = getattr(k, "p", 0) if fam == _ffi.MATERNP else 0
    spec.power = power
    spec.param = {_ffi.RQ: getattr(k, "alpha", 0.0), _ffi.GAMMAEXP: getattr(k, "gamma", 0.0), _ffi.IMQ: getattr(k, "c", 0.0),
                  _ffi.MATERN: getattr(k, "nu", 0.0)}.get(fam, 0.0)
    spec.lengthscale = ls
    spec.scale = scale
    if spec.trait == _ffi.DOTPRODUCT and ls != 1.0:
        return None
    return spec


class _Refusal(Exception):
    """An expression without a normal form; the message says why."""


def _normal_form(k, leaf, budget=64):
    """Sum-of-products normal form of a kernel expression: list of (coefficient, [leaf specs]).

    Sum concatenates, Product distributes over sums, Power of a composite multiplies out; a Constant is a bare coefficient.
    `leaf(k)` is the covgram_kernel of a leaf (its scale moves into the coefficient), None where k is none, or raises _Refusal
    for a leaf it will not take.  Anything else — and more than `budget` terms — raises _Refusal."""
    if isinstance(k, Constant):
        return [(k.c, [])]
    s = leaf(k)
    if s is not None:
        c, s.scale = s.scale, 1.0
        return [(c, [s])]
    if isinstance(k, Sum):
        out = [term for a in k.args for term in _normal_form(a, leaf, budget)]
    elif isinstance(k, Product) or (isinstance(k, Power) and k.p >= 1):
        out = [(1.0, [])]
        for a in (k.args if isinstance(k, Product) else (k.k,) * k.p):
            e = _normal_form(a, leaf, budget)
            out = [(c1 * c2, f1 + f2) for (c1, f1) in out for (c2, f2) in e]
            if len(out) > budget:
                break
    else:
        raise _Refusal(f"{type(k).__name__} is not a Sum / Product / Power / Constant / Lengthscale over the supported leaves")
    if len(out) > budget:
        raise _Refusal(f"the expression multiplies out to more than {budget} terms")
    return out


def _copy_spec(dst, src):
    for name, _ in _ffi.covgram_kernel._fields_:
        setattr(dst, name, getattr(src, name))


def _merge_leaf_powers(fs):
    """Within a term, identical leaves multiply into one factor with a higher Power: φ^a φ^b = φ^(a+b)."""
    out = {}
    for f in fs:
        key = (f.family, f.p, f.param, f.lengthscale)
        if key in out:
            out[key].power += f.power
        else:
            g = _ffi.covgram_kernel(); _copy_spec(g, f); out[key] = g
    return list(out.values())


def _merge_like_terms(terms, key_of):
    """{factor keys: (coefficient, factors)}: like leaves merged, each term's factors sorted by `key_of`, like terms (pure
    constants included, under the key ()) added up where the first of them stood."""
    merged = {}
    for c, fs in terms:
        fs = sorted(_merge_leaf_powers(fs), key=key_of)
        key = tuple(key_of(f) for f in fs)
        merged[key] = (merged[key][0] + c if key in merged else c, fs)
    return merged


def _composite(terms, trait):
    """The covgram_kernel_composite of (coefficient, factors) terms under the head trait `trait`; the caller has checked the limits."""
    comp = _ffi.covgram_kernel_composite()
    comp.head.family, comp.head.trait, comp.head.p, comp.head.power = _ffi.COMPOSITE, trait, 0, 1
    comp.head.param, comp.head.lengthscale, comp.head.scale = 0.0, 1.0, 1.0
    comp.nterms = len(terms)
    fi = 0
    for t, (c, fs) in enumerate(terms):
        if not fs:
            comp.nfactors[t] = 1
            comp.factors[fi].family, comp.factors[fi].trait, comp.factors[fi].power = _ffi.CONSTANT, trait, 1
            comp.factors[fi].lengthscale, comp.factors[fi].scale = 1.0, c
            fi += 1
            continue
        comp.nfactors[t] = len(fs)
        for q, f in enumerate(fs):
            _copy_spec(comp.factors[fi], f)
            comp.factors[fi].scale = c if q == 0 else 1.0     # the term's coefficient rides on its first factor
            fi += 1
    return comp


def _within_limits(terms):
    nfac = sum(max(len(fs), 1) for _, fs in terms)
    return len(terms) <= _ffi.COMPOSITE_MAX_TERMS and nfac <= _ffi.COMPOSITE_MAX_FACTORS, nfac


def device_spec(k):
    """What the device runs for `k`: a covgram_kernel (single profile), a covgram_kernel_composite (Sum / Product /
    Power of kernels sharing one input trait, src/algebra.jl:5-63 with the trait rule of src/properties.jl:47-63),
    or None if k is GenericInput in the reference's terms or exceeds the composite limits (8 terms, 8 factors)."""
    s = _simple_spec(k)
    if s is not None:
        return s
    try:                                                      # leaves: the compiled profiles (no closures, FiniteBasis, ...)
        terms = _normal_form(k, _simple_spec)
    except _Refusal:
        return None
    merged = _merge_like_terms(terms, lambda f: (f.family, f.p, f.power, f.param, f.lengthscale))
    # zero terms drop out; the pure constant goes last
    terms = [(c, fs) for key, (c, fs) in merged.items() if key and c != 0.0]
    if () in merged and merged[()][0] != 0.0:
        terms.append(merged[()])
    traits = {f.trait for _, fs in terms for f in fs}
    if len(traits) != 1:
        return None                                           # mixed traits: GenericInput (src/properties.jl:56-62)
    if not _within_limits(terms)[0]:
        return None
    return _composite(terms, traits.pop())


def require_device_spec(k):
    spec = device_spec(k)
    if spec is None:
        raise _ffi.UnsupportedKernel(
            _ffi.EUNSUPPORTED,
            f"{type(k).__name__} has input_trait {input_trait(k)!r} / no compiled device profile; the reference would run its "
            "generic threaded loop (src/gramian.jl:78-87) here — this engine has no CPU fallback")
    return spec


# ----------------------------------------------------------------------------------------------
# gradient kernels of mixed-trait composites (src/gradient_algebra.jl): the composite of covgram_grad_mvm_mixed
# ----------------------------------------------------------------------------------------------
def _mixed_leaf(k):
    """The leaf hook of the mixed gradient kernels: the compiled profiles, NeuralNetwork(σ) as a leaf of its own (family NEURALNETWORK,
    trait 0, σ in param), and the leaves without a jet refused by name."""
    if isinstance(k, NeuralNetwork):
        s = _ffi.covgram_kernel()
        s.family, s.trait, s.p, s.power = _ffi.NEURALNETWORK, 0, 0, 1
        s.param, s.lengthscale, s.scale = k.sigma, 1.0, 1.0
        return s
    if isinstance(k, CosineKernel):
        raise _Refusal(f"{type(k).__name__} belongs with the gradient kernels of spectral mixtures")
    s = _simple_spec(k)
    if s is None:
        return None
    leaf = k
    while isinstance(leaf, (Product, Power, Lengthscale)):
        leaf = [a for a in leaf.args if not isinstance(a, Constant)][0] if isinstance(leaf, Product) else leaf.k
    name = type(leaf).__name__                               # (a half-integer Matern has lowered to MaternP: judged as such)
    if s.family in (_ffi.EXP, _ffi.GAMMAEXP) or (s.family == _ffi.MATERNP and s.p == 0):
        raise _Refusal(f"{name}{'(0)' if isinstance(leaf, MaternP) else ''} is singular at zero distance")
    if s.family == _ffi.MATERN:
        raise _Refusal(f"{name}(ν = {leaf.nu}) has no closed-form jet here (MaternP does)")
    return s


def _mixed_value_leaf(k):
    """The leaf hook of the scalar mixed Gramians: only a leaf's VALUE is needed, so every profile _simple_spec lowers is taken — the
    ones singular at zero distance and Matern(ν) too — and NeuralNetwork(σ); CosineKernel alone is refused by name."""
    if isinstance(k, NeuralNetwork):
        return _mixed_leaf(k)
    if isinstance(k, CosineKernel):
        raise _Refusal(f"{type(k).__name__} belongs with the spectral mixtures (spectral_mixture_spec)")
    return _simple_spec(k)


def _mixed_lower(k, leaf=_mixed_leaf):
    """The mixed composite of `k`, or _Refusal: the normal form of device_spec with every factor on its own trait (the head's is 0), a
    term's factors sorted with the power last, the constant term where it first appeared, and an expression that cancels lowered to
    the one term 0.  `leaf`: the hook of the gradient kernels (_mixed_leaf) or of the scalar Gramians (_mixed_value_leaf)."""
    merged = _merge_like_terms(_normal_form(k, leaf), lambda f: (f.family, f.p, f.param, f.lengthscale, f.power))
    terms = [term for term in merged.values() if term[0] != 0.0] or [(0.0, [])]
    ok, nfac = _within_limits(terms)
    if not ok:
        raise _Refusal(f"the normal form has {len(terms)} terms and {nfac} factors; the composite holds {_ffi.COMPOSITE_MAX_TERMS} terms "
                       f"and {_ffi.COMPOSITE_MAX_FACTORS} factors")
    return _composite(terms, 0)


def mixed_gradient_spec(k):
    """The covgram_kernel_composite that covgram_grad_mvm_mixed runs for GradientKernel(k) / ValueGradientKernel(k), or None: Sum /
    Product / Power / Constant / Lengthscale over the leaves with a jet in (x·y, |x|², |y|²) — the isotropic profiles that are smooth
    at zero distance (EQ, RQ, Cauchy, InverseMultiQuadratic, MaternP(p ≥ 1)), Dot, ExponentialDot, AsinDot and NeuralNetwork(σ) — in
    the normal form of device_spec, EVERY FACTOR WITH ITS OWN TRAIT (the head's is 0), within the same limits (8 terms, 8 factors)."""
    try:
        return require_mixed_gradient_spec(k)
    except _ffi.UnsupportedKernel:
        return None


def require_mixed_gradient_spec(k):
    try:
        if not isinstance(k, AbstractKernel):
            raise _Refusal(f"{type(k).__name__} is not a kernel expression")
        return _mixed_lower(k)
    except _Refusal as why:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"gradient kernel of a mixed-trait composite ({type(k).__name__}): {why}") from None


def mixed_spec(k):
    """The covgram_kernel_composite that covgram_mvm_mixed / covgram_matrix_mixed run for the SCALAR Gramian of `k`, or None: the normal
    form of mixed_gradient_spec (same walker, merge, order rules, writer and limits: 8 terms, 8 factors) over every leaf _simple_spec
    lowers plus NeuralNetwork(σ).  For every kernel both accept, the two composites are equal field by field."""
    try:
        return require_mixed_spec(k)
    except _ffi.UnsupportedKernel:
        return None


def require_mixed_spec(k):
    try:
        if not isinstance(k, AbstractKernel):
            raise _Refusal(f"{type(k).__name__} is not a kernel expression")
        return _mixed_lower(k, _mixed_value_leaf)
    except _Refusal as why:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"Gramian of a mixed-trait composite ({type(k).__name__}): {why}") from None


# ----------------------------------------------------------------------------------------------
# hyper-parameters: the ordered leaves of a kernel expression (the role of parameters / Base.similar in src/parameters.jl)
# ----------------------------------------------------------------------------------------------
_OWN_PARAMETER = {RationalQuadratic: "alpha", GammaExponential: "gamma", InverseMultiQuadratic: "c"}
_NO_PARAMETER = (ExponentiatedQuadratic, Exponential, Cauchy, MaternP, Matern, Dot, ExponentialDot, AsinDot)   # p, nu: structure


def hyperparameters(k):
    """[(path, name, value)]: the leaves of the kernel expression `k` in a fixed order — depth first, arguments left to right, a
    wrapper's own parameter after its inner kernel's.  Leaves: Constant.c ("scale"), Lengthscale.l ("l"), RationalQuadratic.alpha,
    GammaExponential.gamma, InverseMultiQuadratic.c ("c"), NeuralNetwork.sigma ("sigma"), the entries of a Cosine's frequency vector ("mu"), and the entries of a
    diagonal ScaledInputKernel in the parametrisation the object stores: "l" for ARD(k, l) (lengthscales), "U" for
    ScaledInputKernel(k, U) (the multipliers).  `path` is the tuple of steps from the root (argument index of a Sum / Product, "k"
    into a wrapper, the dimension of an ARD or Cosine entry).  MaternP's p, Matern's nu
    and Power's exponent are structure, not parameters.  Any other node raises UnsupportedKernel naming it."""
    def walk(k, path):
        if isinstance(k, Constant):
            return [(path, "scale", k.c)]
        if isinstance(k, (Sum, Product)):
            return [leaf for i, a in enumerate(k.args) for leaf in walk(a, path + (i,))]
        if isinstance(k, Power):
            return walk(k.k, path + ("k",))
        if isinstance(k, Lengthscale):
            return walk(k.k, path + ("k",)) + [(path, "l", k.l)]
        if isinstance(k, ScaledInputKernel) and k.diagonal:
            name, vals = ("l", k.l) if k.l is not None else ("U", k.U)
            return walk(k.k, path + ("k",)) + [(path + (c,), name, float(v)) for c, v in enumerate(vals)]
        if isinstance(k, CosineKernel):
            return [(path + (c,), "mu", float(v)) for c, v in enumerate(k.c)]
        if type(k) in _OWN_PARAMETER:
            name = _OWN_PARAMETER[type(k)]
            return [(path, name, getattr(k, name))]
        if isinstance(k, NeuralNetwork):
            return [(path, "sigma", k.sigma)]
        if isinstance(k, _NO_PARAMETER):
            return []
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"hyperparameters: {type(k).__name__} is not a node of a parameter tree")
    return walk(k, ())


def with_hyperparameters(k, theta):
    """The kernel `k` rebuilt with the flat vector `theta` in the order of hyperparameters(k) (Base.similar(k, θ), src/parameters.jl:24-48)."""
    theta = [float(v) for v in np.asarray(theta, dtype=np.float64).reshape(-1)]
    nparam = len(hyperparameters(k))
    if len(theta) != nparam:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"length(θ) = {len(theta)} ≠ {nparam} = nparameters(k)")   # src/parameters.jl:15
    it = iter(theta)
    def build(k):
        if isinstance(k, Constant):
            return Constant(next(it), getattr(k, "check", True))
        if isinstance(k, CosineKernel):
            return CosineKernel(np.array([next(it) for _ in range(k.c.size)]))
        if isinstance(k, (Sum, Product)):
            return type(k)(tuple(build(a) for a in k.args))
        if isinstance(k, Power):
            return Power(build(k.k), k.p)
        if isinstance(k, Lengthscale):
            inner = build(k.k)
            return Lengthscale(inner, next(it))
        if isinstance(k, ScaledInputKernel):
            inner = build(k.k)
            vals = np.array([next(it) for _ in range(len(k.U))])
            return ARD(inner, vals) if k.l is not None else ScaledInputKernel(inner, vals)
        if type(k) in _OWN_PARAMETER or isinstance(k, NeuralNetwork):
            return type(k)(next(it))
        return k
    return build(k)


# ----------------------------------------------------------------------------------------------
# hyper-parameter gradients of mixed-trait composites: the composite of covgram_bilinear_grad_mixed and the host chain rules
# ----------------------------------------------------------------------------------------------
MIXED_GRAD_NOUT = _ffi.MIXED_GRAD_NOUT
_MIXED_Z0, _MIXED_P0 = _ffi.COMPOSITE_MAX_TERMS, _ffi.COMPOSITE_MAX_TERMS + _ffi.COMPOSITE_MAX_FACTORS


def _provenance_form(k, path=(), scales=(), budget=64):
    """Sum-of-products normal form of `k` that remembers where everything came from: a list of terms (consts, leaves), `consts` the tuple
    of paths of the Constant leaves multiplied into the term (one entry per occurrence) and `leaves` a tuple of (path, leaf kernel,
    ((path, l) of every Lengthscale node above it)), one entry per occurrence.  The walk is _normal_form's: Sum concatenates, Product
    distributes, Power(k, p) multiplies p copies of k out — copies that share their paths, which is what lets them merge again."""
    if isinstance(k, Constant):
        return [((path,), ())]
    if isinstance(k, Lengthscale):
        return _provenance_form(k.k, path + ("k",), scales + ((path, k.l),), budget)
    if isinstance(k, CosineKernel):
        raise _Refusal(f"{type(k).__name__} belongs with the spectral mixtures (spectral_mixture_gradient)")
    if isinstance(k, NeuralNetwork) or type(k) in _BASE:
        if isinstance(k, Matern) and _simple_spec(k).family == _ffi.MATERN:
            raise _Refusal(f"Matern(ν = {k.nu}) has no parameter derivatives on the device (half-integer ν: MaternP)")
        if scales and not isinstance(k, IsotropicKernel):
            raise _Refusal(f"Lengthscale over {type(k).__name__}: lengthscales apply to isotropic kernels only")
        return [((), ((path, k, scales),))]
    if isinstance(k, Sum):
        out = [term for i, a in enumerate(k.args) for term in _provenance_form(a, path + (i,), scales, budget)]
    elif isinstance(k, Product) or (isinstance(k, Power) and k.p >= 1):
        parts = [(a, path + (i,)) for i, a in enumerate(k.args)] if isinstance(k, Product) else [(k.k, path + ("k",))] * k.p
        out = [((), ())]
        for a, pa in parts:
            e = _provenance_form(a, pa, scales, budget)
            out = [(c1 + c2, f1 + f2) for (c1, f1) in out for (c2, f2) in e]
            if len(out) > budget:
                break
    else:
        raise _Refusal(f"{type(k).__name__} is not a Sum / Product / Power / Constant / Lengthscale over the supported leaves")
    if len(out) > budget:
        raise _Refusal(f"the expression multiplies out to more than {budget} terms")
    return out


def _mixed_parameter_lower(k):
    leaves = hyperparameters(k)
    row_of = {(path, name): i for i, (path, name, _) in enumerate(leaves)}
    value_of = {path: v for path, name, v in leaves if name == "scale"}
    # merge by PROVENANCE: the copies of a leaf within a term into one factor with a power, the terms over the same (leaf, power) set into one
    # term whose coefficient is a polynomial in the Constants: {sorted tuple of Constant paths: multiplicity}
    merged = {}
    for consts, occ in _provenance_form(k):
        fac = {}
        for path, leaf, scales in occ:
            fac[path] = (leaf, scales, fac[path][2] + 1 if path in fac else 1)
        key = frozenset((path, pw) for path, (_, _, pw) in fac.items())
        mono = tuple(sorted(consts, key=repr))
        if key not in merged:
            merged[key] = ({}, fac)
        merged[key][0][mono] = merged[key][0].get(mono, 0) + 1
    terms = list(merged.values())
    nfac = sum(max(len(fac), 1) for _, fac in terms)
    if len(terms) > _ffi.COMPOSITE_MAX_TERMS or nfac > _ffi.COMPOSITE_MAX_FACTORS:
        raise _Refusal(f"the normal form has {len(terms)} terms and {nfac} factors; the composite holds {_ffi.COMPOSITE_MAX_TERMS} terms "
                       f"and {_ffi.COMPOSITE_MAX_FACTORS} factors")
    J = np.zeros((len(leaves), MIXED_GRAD_NOUT))
    lowered, fi = [], 0
    for t, (poly, fac) in enumerate(terms):
        c = 0.0
        for mono, mult in poly.items():
            c += mult * math.prod(value_of[p] for p in mono)
            for i, p in enumerate(mono):                     # d/dconst of the monomial: leave ONE occurrence out (never a division)
                J[row_of[(p, "scale")], t] += mult * math.prod(value_of[o] for j, o in enumerate(mono) if j != i)
        specs = []
        for path, (leaf, scales, pw) in fac.items():
            s = _mixed_leaf_any(leaf)
            s.power, s.scale = pw, 1.0
            s.lengthscale = math.prod(l for _, l in scales)
            specs.append(s)
            for lpath, l in scales:
                J[row_of[(lpath, "l")], _MIXED_Z0 + fi] += -2.0 / l
            name = "sigma" if isinstance(leaf, NeuralNetwork) else _OWN_PARAMETER.get(type(leaf))
            if name is not None:
                J[row_of[(path, name)], _MIXED_P0 + fi] += 1.0
            fi += 1
        fi += 0 if fac else 1                                 # a term of constants only occupies one Constant factor
        lowered.append((c, specs))
    return _composite(lowered, 0), J


def _mixed_leaf_any(leaf):
    """The covgram_kernel of one leaf of the parameter lowering: NeuralNetwork(σ) as its own family, every compiled profile otherwise."""
    if isinstance(leaf, NeuralNetwork):
        return _mixed_leaf(leaf)
    return _simple_spec(leaf)


def require_mixed_parameter_spec(k):
    """(composite, J) for covgram_bilinear_grad_mixed and its host chain rules: `composite` the covgram_kernel_composite of `k` in the
    normal form of mixed_spec MERGED BY PROVENANCE — the p copies of a leaf under Power(k, p) become one factor of power p, terms over the
    same leaves add their coefficients (Polynomial(2, σ) is Dot² + 2σ·Dot + σ²), but two different leaves that hold equal numbers stay
    separate factors and terms, and no term is dropped because its coefficient is 0: every leaf keeps its own derivative.  `J` is the
    dense len(hyperparameters(k)) × 24 float64 matrix of the chain rules: with `out` the 24 numbers of the device,
        grad = J @ out,        value = Σ_t c_t out[t]   (c_t: the scale of term t's first factor in `composite`)
    Rows: a Constant gets Σ_t ∂c_t/∂const · e_t (c_t is a polynomial in the Constants, differentiated here, never divided); a
    Lengthscale node −(2/l) Σ e_{8+f} over the isotropic factors beneath it (nested lengthscales each with their own l); an own
    parameter (RQ α, γ-exponential γ, IMQ c, NeuralNetwork σ) e_{16+f}.  Leaves: the isotropic profiles except Matern with real ν,
    Dot, ExponentialDot, AsinDot, NeuralNetwork, Constant.  More than 8 terms or 8 factors, a CosineKernel, Matern(ν) and any other node
    raise UnsupportedKernel naming what and why, before any device call."""
    try:
        if not isinstance(k, AbstractKernel):
            raise _Refusal(f"{type(k).__name__} is not a kernel expression")
        return _mixed_parameter_lower(k)
    except _Refusal as why:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"hyper-parameter gradients of a mixed-trait composite ({type(k).__name__}): {why}") from None


def mixed_term_coefficients(comp):
    """[c_t]: the coefficient of every term of a covgram_kernel_composite — head scale times the scales of the term's factors."""
    out, fi = [], 0
    for t in range(comp.nterms):
        c = comp.head.scale
        for _ in range(comp.nfactors[t]):
            c *= comp.factors[fi].scale
            fi += 1
        out.append(c)
    return out


def mixed_parameter_spec(k):
    """require_mixed_parameter_spec(k), or None where it refuses."""
    try:
        return require_mixed_parameter_spec(k)
    except _ffi.UnsupportedKernel:
        return None


# ----------------------------------------------------------------------------------------------
# spectral mixtures: Σ_q w_q cos(2π μ_q·r) exp(−½ Σ_k (r_k / l_qk)²), the parameters of covgram_sm_create
# ----------------------------------------------------------------------------------------------
SM_MAX_COMPONENTS, SM_MAX_D = _ffi.SM_MAX_COMPONENTS, _ffi.SM_MAX_D


def _sm_eq_factor(k):
    """Squared inverse lengthscale(s) of an EQ factor — a number (isotropic) or a length-d vector — or None if k is not one:
    EQ(), Lengthscale(EQ, l) (nesting multiplies) or ScaledInputKernel(EQ-factor, diagonal U)."""
    if isinstance(k, ExponentiatedQuadratic):
        return 1.0
    if isinstance(k, Lengthscale):
        inner = _sm_eq_factor(k.k)
        return None if inner is None else inner / k.l ** 2
    if isinstance(k, ScaledInputKernel):
        inner = _sm_eq_factor(k.k)
        if inner is None or not k.diagonal or np.ndim(inner) != 0:
            return None
        return inner * k.U ** 2
    return None


def _sm_term(k, d):
    """(w, mu[d], inv_l2[d]) of one term — a Product, or a bare factor, of Constants, at most one Cosine and EQ factors — or None."""
    w, mu, il2 = 1.0, None, np.zeros(d)
    factors = []

    def flatten(f):                                          # a * b * c is Product((Product((a, b)), c))
        if isinstance(f, Product):
            for a in f.args:
                flatten(a)
        else:
            factors.append(f)
    flatten(k)
    for f in factors:
        if isinstance(f, Constant):
            w *= f.c
        elif isinstance(f, CosineKernel):
            if mu is not None or f.c.size not in (1, d):
                return None
            mu = np.broadcast_to(f.c, (d,)).astype(np.float64)
        else:
            e = _sm_eq_factor(f)
            if e is None or (np.ndim(e) != 0 and np.size(e) != d):
                return None
            il2 = il2 + e
    return w, (np.zeros(d) if mu is None else mu), il2


def _sm_dim(k):
    """The dimension a mixture's own parameters fix (the length of a vector-valued c or U), 1 if they are all scalars, None if they disagree."""
    dims = set()

    def walk(f):
        if isinstance(f, (Sum, Product)):
            for a in f.args:
                walk(a)
        elif isinstance(f, CosineKernel) and f.c.size > 1:
            dims.add(int(f.c.size))
        elif isinstance(f, ScaledInputKernel):
            if f.diagonal:
                dims.add(int(f.U.size))
            walk(f.k)
        elif isinstance(f, Lengthscale):
            walk(f.k)
    walk(k)
    return None if len(dims) > 1 else (dims.pop() if dims else 1)


def spectral_mixture_spec(k, d=None):
    """(w[Q], mu[Q, d], inv_l[Q, d]) as float64 arrays if k is a spectral mixture the fused kernels of covgram_sm_mvm take, else None.

    Accepted: a Sum (nested Sums are flattened) of terms, or one term; a term is a Product (or a bare factor) of any number of
    Constants (they multiply into w), at most one Cosine (a scalar c broadcasts to d; none: μ = 0) and any number of EQ factors —
    EQ(), Lengthscale(EQ, l), ScaledInputKernel(EQ, diagonal U) — whose squared inverse lengthscales add (none: inv_l = 0).
    Anything else (a non-diagonal U, Power, other profiles, two Cosines in a term), lengths that disagree with d, Q > 32 or d > 16
    give None.  Products are not distributed over Sums.  d = None: the dimension the parameters themselves fix (1 if all are scalars)."""
    if not isinstance(k, AbstractKernel):
        return None
    if d is None:
        d = _sm_dim(k)
        if d is None:
            return None
    d = int(d)
    if not 1 <= d <= SM_MAX_D:
        return None
    terms = []

    def flatten(f):
        if isinstance(f, Sum):
            for a in f.args:
                flatten(a)
        else:
            terms.append(f)
    flatten(k)
    if not 1 <= len(terms) <= SM_MAX_COMPONENTS:
        return None
    out = []
    for t in terms:
        r = _sm_term(t, d)
        if r is None:
            return None
        out.append(r)
    w = np.array([r[0] for r in out], dtype=np.float64)
    mu = np.stack([r[1] for r in out]).astype(np.float64)
    inv_l = np.sqrt(np.stack([r[2] for r in out]).astype(np.float64))
    return w, mu, inv_l


def _sm_eq_factor_jet(k):
    """(a, [∂a/∂θ]) of an EQ factor _sm_eq_factor accepts: its squared inverse lengthscale(s) a — a number or a length-d vector — and
    the derivative of a with respect to each of the factor's leaves, in hyperparameters order (each a number or a length-d vector)."""
    if isinstance(k, ExponentiatedQuadratic):
        return 1.0, []
    if isinstance(k, Lengthscale):
        a, da = _sm_eq_factor_jet(k.k)
        return a / k.l ** 2, [t / k.l ** 2 for t in da] + [-2.0 * a / k.l ** 3]
    a, da = _sm_eq_factor_jet(k.k)                             # a diagonal ScaledInputKernel over an isotropic factor: a_c = a U_c²
    U = k.U
    own = []
    for c in range(U.size):
        e = np.zeros(U.size)
        e[c] = -2.0 * a / float(k.l[c]) ** 3 if k.l is not None else 2.0 * a * float(U[c])   # ARD stores l: U_c = 1 / l_c
        own.append(e)
    return a * U ** 2, [t * U ** 2 for t in da] + own


def spectral_mixture_chain_rules(k, out, d):
    """The host chain rules of spectral_mixture_gradient: `k` a tree spectral_mixture_spec(k, d) accepts, `out` the Q × (1 + 2d)
    numbers of covgram_bilinear_grad_sm (row q: ∂F/∂w_q, ∂F/∂μ_qk, E_qk with ∂F/∂(inv_l_qk²) = −½ E_qk).  Returns (value, grad): the
    bilinear form Σ_q w_q out[q, 0] and its gradient in hyperparameters(k) order.  For term q with Constants c_1 … c_p (w_q = Π c_j)
    and EQ factors f contributing a_fk to inv_l_qk² = Σ_f a_fk:
        ∂/∂c_i = (Π_{j≠i} c_j) out[q, 0]
        ∂/∂μ_k = out[q, 1 + k] for a vector Cosine, Σ_k out[q, 1 + k] for a scalar c broadcast over d
        ∂/∂θ   = −½ Σ_k E_qk ∂a_fk/∂θ for a parameter θ of factor f: Lengthscale(EQ, l): Σ_k E_qk / l³; ARD(EQ, l): E_qk / l_k³;
                 ScaledInputKernel(EQ, U): −U_k E_qk; nested lengthscales by the product rule (_sm_eq_factor_jet)."""
    d = int(d)
    out = np.asarray(out, dtype=np.float64).reshape(-1, 1 + 2 * d)
    terms = []

    def flatten(f, kind, into):
        if isinstance(f, kind):
            for a in f.args:
                flatten(a, kind, into)
        else:
            into.append(f)
    flatten(k, Sum, terms)
    if len(terms) != out.shape[0]:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"spectral_mixture_chain_rules: {len(terms)} terms, {out.shape[0]} rows of out")
    value, grad = 0.0, []
    for q, t in enumerate(terms):
        factors = []
        flatten(t, Product, factors)
        consts = [f.c for f in factors if isinstance(f, Constant)]
        value += float(np.prod(consts)) * out[q, 0]
        E = out[q, 1 + d:]
        ci = 0
        for f in factors:
            if isinstance(f, Constant):
                grad.append(float(np.prod(consts[:ci] + consts[ci + 1:])) * out[q, 0])
                ci += 1
            elif isinstance(f, CosineKernel):
                grad += [float(v) for v in out[q, 1:1 + d]] if f.c.size == d else [float(out[q, 1:1 + d].sum())]
            else:
                grad += [float(-0.5 * np.sum(E * da)) for da in _sm_eq_factor_jet(f)[1]]
    return value, grad


def require_sm_spec(k, d=None):
    spec = spectral_mixture_spec(k, d)
    if spec is None:
        raise _ffi.UnsupportedKernel(
            _ffi.EUNSUPPORTED,
            f"{type(k).__name__} is not a spectral mixture with a device path: a Sum of at most {SM_MAX_COMPONENTS} terms, each a Product of "
            f"Constants, at most one Cosine and EQ factors under Lengthscale or a diagonal ScaledInputKernel, on points of d <= {SM_MAX_D} "
            f"dimensions (here d = {d}); products are not distributed over sums")
    return spec


HESSIAN_MAX_D = 32
# the families of COVGRAM_HESS_FAMILIES in csrc/hess_mvm.hpp, which the library's own checks and launchers are generated from
_HESSIAN_FAMILIES = (_ffi.EQ, _ffi.RQ, _ffi.CAUCHY, _ffi.IMQ, _ffi.DOT, _ffi.EXPDOT)


def _require_hess_spec(wrapper: str, k, d: Optional[int]):
    name = type(k).__name__
    spec = device_spec(k)
    if spec is None or not isinstance(spec, _ffi.covgram_kernel):
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"{wrapper}({name}): only single profiles have a device path, "
                                                        "not composites or GenericInput kernels")
    if spec.family not in _HESSIAN_FAMILIES:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"{wrapper}({name}): no closed-form fourth derivative is compiled for this profile "
                                                        "(supported: EQ, RQ, Cauchy, InverseMultiQuadratic, ExponentialDot, Dot)")
    if spec.power != 1:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"{wrapper}({name}): Power wrappers (exponent {spec.power}) have no device path")
    if d is not None and d > HESSIAN_MAX_D:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"{wrapper}({name}): d = {d} exceeds the compiled maximum {HESSIAN_MAX_D}")
    return spec


def require_hessian_spec(k, d: Optional[int] = None):
    """The covgram_kernel that covgram_hess_mvm runs for HessianKernel(k), checked on the host before any device call: a single
    profile whose derivatives up to the fourth have closed forms in the library (EQ, RQ, Cauchy, IMQ with Lengthscale and Constant
    factors; ExponentialDot, Dot), no Power wrapper, d <= 32.  Everything else raises UnsupportedKernel naming the kernel."""
    return _require_hess_spec("HessianKernel", k, d)


def require_vgh_spec(k, d: Optional[int] = None):
    """The covgram_kernel that covgram_valgradhess_mvm runs for ValueGradientHessianKernel(k), checked on the host before any device
    call: the kernels and the bound on d of require_hessian_spec.  Everything else raises UnsupportedKernel naming the kernel."""
    return _require_hess_spec("ValueGradientHessianKernel", k, d)


def require_pivchol_spec(k):
    """The covgram_kernel that covgram_pivoted_cholesky runs for gramian(k, x), checked on the host before any device call: ONE
    isotropic profile (EQ, Exponential, RQ, GammaExponential, Cauchy, IMQ, MaternP, Matern) under Lengthscale, Constant and Power
    wrappers.  Composites, dot-product and GenericInput kernels raise UnsupportedKernel naming the kernel."""
    name = type(k).__name__
    spec = device_spec(k)
    if spec is None or not isinstance(spec, _ffi.covgram_kernel):
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"pivoted_cholesky({name}): only single isotropic profiles have a device "
                                                        "factorisation, not composites (Sum, Product of profiles) or GenericInput kernels")
    if spec.trait != _ffi.ISOTROPIC:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"pivoted_cholesky({name}): dot-product kernels have no device factorisation (supported: "
                                                        "EQ, Exponential, RQ, GammaExponential, Cauchy, InverseMultiQuadratic, MaternP, Matern)")
    return spec


# ----------------------------------------------------------------------------------------------
# decay radius of exponentially decaying isotropic kernels (src/sparse.jl:24-38)
# ----------------------------------------------------------------------------------------------
def decay_radius(k, delta: float = 1e-6) -> float:
    """The distance beyond which |k| < delta, for ONE isotropic profile under Lengthscale and Constant factors (src/sparse.jl:25-38):
    EQ sqrt(-2 ln de), Exponential -ln de, GammaExponential(g) (-2 ln de)^(1/g), MaternP and Matern(nu >= 1/2) -ln de (conservative).

    Two deliberate corrections of the reference (the same as covgram_decay_radius, include/covgram.h): Lengthscale(k, l) evaluates
    k(r / l), so the radius is l r0 (src/sparse.jl:38 drops its delta argument and divides by l); a Constant factor c uses
    de = delta / |c| in place of delta.  0 < delta / |c| < 1 is required (ValueError).  Matern(nu < 1/2) raises DomainError as in the
    reference; kernels without exponential decay (RQ, Cauchy, IMQ, dot-product kernels), Power wrappers, composites and GenericInput
    kernels raise UnsupportedKernel naming the kernel (the reference's TypeError branch)."""
    top = k
    scale, ls = 1.0, 1.0

    def refuse(what):
        return _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"decay_radius: {what} (defined for EQ, Exponential, GammaExponential, MaternP and "
                                                         f"Matern under Lengthscale and Constant factors); kernel: {type(top).__name__}")

    while True:
        if isinstance(k, Product):
            rest = [a for a in k.args if not isinstance(a, Constant)]
            if len(rest) != 1:
                raise refuse(f"a Product of {len(rest)} profiles has no single decay radius")
            for c in k.args:
                if isinstance(c, Constant):
                    scale *= c.c
            k = rest[0]
        elif isinstance(k, Lengthscale):
            ls *= k.l
            k = k.k
        elif isinstance(k, (Sum, Power)):
            raise refuse(f"{type(k).__name__} has no single decay radius")
        else:
            break
    if isinstance(k, (RationalQuadratic, Cauchy, InverseMultiQuadratic, DotProductKernel, Constant)):
        raise refuse(f"{type(k).__name__} does not decay exponentially")
    if not isinstance(k, (ExponentiatedQuadratic, Exponential, GammaExponential, MaternP, Matern)):
        raise refuse(f"{type(k).__name__} is not an isotropic profile with a known decay radius")
    if isinstance(k, Matern) and k.nu < 0.5:
        raise DomainError(f"decay_radius not defined for Matern kernel with ν = {k.nu} < 1/2")
    delta = float(delta)
    c = abs(scale)
    if not (c > 0 and 0 < delta / c < 1):
        raise ValueError(f"decay_radius: need 0 < delta / |c| < 1 (delta = {delta}, Constant factor c = {scale})")
    de = delta / c
    if isinstance(k, ExponentiatedQuadratic):
        r0 = math.sqrt(-2.0 * math.log(de))
    elif isinstance(k, GammaExponential):
        if not k.gamma > 0:
            raise DomainError(f"decay_radius: gamma = {k.gamma} not in (0, 2]")
        r0 = math.pow(-2.0 * math.log(de), 1.0 / k.gamma)
    else:
        r0 = -math.log(de)
    return ls * r0
