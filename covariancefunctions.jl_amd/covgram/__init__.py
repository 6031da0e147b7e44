"""covgram — MI355X-native lazy-Gramian MVM engine behind the CovarianceFunctions.jl API surface.

    import covgram as cg
    G = cg.gramian(cg.EQ(), x)          # x: (n, d) tensor on the GPU; O(1), lazy
    b = G @ a                           # mul!(b, G, a) — hand-written HIP kernel in libcovgram.so
    cg.mul_(b, G, a, alpha, beta)       # 5-argument mul!

Only the hot path `mul!(b, gramian(k, x), a)` and its GradientKernel / Toeplitz / Kronecker / low-rank
siblings exist here.  No CPU fallback: without libcovgram.so or a gfx950 device every
product raises.
"""
from . import _ffi
from ._ffi import CovgramError, DimensionMismatch, UnsupportedKernel, NoDevice
from .kernels import (AbstractKernel, MercerKernel, StationaryKernel, IsotropicKernel, MultiKernel, Constant,
                      ExponentiatedQuadratic, EQ, RationalQuadratic, RQ, Exponential, Exp, GammaExponential, GammaExp,
                      Cauchy, InverseMultiQuadratic, MaternP, Matern, Dot, ExponentialDot, FiniteBasis, Product, Sum, Power,
                      Lengthscale, ARD, ScaledInputKernel, Warped, Periodic, VerticalRescaling, CosineKernel, Cosine, Cos, Line, Polynomial, Poly, NeuralNetwork, NN, AsinDot,
                      SeparableProduct, separable, SeparableKernel, Separable, GradientKernel, ValueGradientKernel, HessianKernel, ValueGradientHessianKernel, InputTrait,
                      GenericInput, IsotropicInput, DotProductInput, StationaryInput, StationaryLinearFunctionalInput,
                      PeriodicInput, input_trait, register_input_trait, ismercer, isstationary, isisotropic, isdot,
                      device_spec, Spectral, SpectralMixture, SM, spectral_mixture_spec, require_sm_spec, require_hessian_spec, require_vgh_spec, require_pivchol_spec, DomainError,
                      hyperparameters, with_hyperparameters, spectral_mixture_chain_rules, mixed_gradient_spec, require_mixed_gradient_spec, mixed_spec, require_mixed_spec,
                      mixed_parameter_spec, require_mixed_parameter_spec)
from .gramian import (Gramian, MixedGramian, BlockGramian, MixedBlockGramian, HessianGramian, ValueGradientHessianGramian, SymmetricToeplitz, Toeplitz, Circulant, KroneckerProduct, kronecker,
                      SeparableGramian, LazyMatrixProduct, LazyMatrixSum, ScaledOperator, LinearMapBlockGramian, CosineBlockGramian, PointJacobianBlockGramian, Fill, LazyOperator, LazyGrid, StepRangeLen,
                      srange, gramian, mul_, get_ctx, set_option, get_info, kernel_time, SparseGramian, sparse, decay_radius,
                      BarnesHutFactorization, require_barneshut_spec, SpectralMixtureGramian, bilinear_gradient, bilinear_chain_rules,
                      bilinear_input_gradient, mixed_bilinear_gradient, spectral_mixture_gradient, spectral_mixture_input_gradient)
from .dist import ShardedGramian, shard_bounds
from .solve import (cg, mbcg, cg_tridiagonals, lanczos_quadrature, logdet, inv_quad_logdet, inv_quad_logdet_gradient, minres, solve, toeplitz_solve, durbin, levinson,
                    trench)
from .factorize import (cholesky, factorize, diagonal, CholeskyFactor, PivotedCholesky, pivoted_cholesky, PivotedCholeskyPreconditioner,
                        preconditioner)
from .autograd import gram_product, spectral_mixture_product

__all__ = [n for n in dir() if not n.startswith("_")]
