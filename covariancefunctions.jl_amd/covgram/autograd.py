"""The lazy Gramian product as a differentiable PyTorch operation.

    out = cg.gram_product(k, x, a, y=None, theta=None)      # = gramian(k′, x, y) @ a

is a torch.autograd.Function: the forward pass is the library's own product, and the backward pass of an incoming ḡ (same shape as
out) is three of its fused passes, each run only when the corresponding input requires a gradient:

    ∂a     = Gᵀ ḡ                                      one product with G.T (G itself when y is None)
    ∂theta = bilinear_gradient(G, ḡ, a)[1]              hyper-parameter gradients of Σ_t ḡ_tᵀ G a_t (csrc/bilin_grad.hip)
    ∂x, ∂y = bilinear_input_gradient(G, ḡ, a)           its gradients in the points (csrc/input_grad.hip), cast to their dtype

The backward pass is once differentiable (no second derivatives).

    out = cg.spectral_mixture_product(k, x, a, y=None, theta=None)

is the same operation for a spectral mixture (a kernel gramian() runs through covgram_sm_mvm): the backward pass takes ∂theta from
spectral_mixture_gradient (csrc/sm_grad.hip) and ∂x, ∂y from spectral_mixture_input_gradient (csrc/sm_input_grad.hip)."""
import torch
from torch.autograd.function import once_differentiable

from . import _ffi
from . import kernels as K
from .gramian import (Gramian, LazyOperator, SpectralMixtureGramian, bilinear_gradient, bilinear_input_gradient, gramian, spectral_mixture_gradient,
                      spectral_mixture_input_gradient, _bilinear_plan, _point_dim)


def _refuse(what):
    return _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"gram_product: gradients with respect to x, y or theta through {what} are not supported "
                                                     "(the Gramian of gramian(k, x[, y]) on point tensors only; gradients with respect to a work for every operator)")


class _GramProduct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, k, x, a, y, theta):
        need_x, need_y, need_theta = ctx.needs_input_grad[1], ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        structural = need_x or need_y or need_theta
        operator = isinstance(k, LazyOperator) or hasattr(type(k), "mul_")
        if operator:                                            # an operator built by the caller: differentiable in `a` only
            if structural or x is not None or y is not None or theta is not None:
                raise _refuse(type(k).__name__)
            if not hasattr(type(k), "T") or not hasattr(type(k), "__matmul__"):
                raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"gram_product: {type(k).__name__} has no transpose (.T) to carry the gradient of a")
            G = k
        else:
            if theta is not None:
                k = K.with_hyperparameters(k, theta.detach().cpu().numpy())
            if structural:                                      # what can be refused before anything is built
                inner = k.k if isinstance(k, K.ScaledInputKernel) and k.diagonal else k
                if isinstance(inner, K.AbstractKernel) and K.device_spec(inner) is None and K.spectral_mixture_spec(inner) is None and K.mixed_spec(inner) is not None:
                    raise _refuse("MixedGramian")               # what gramian() would build: no gradient passes exist for it
                _bilinear_plan(inner, "gram_product")
                for p in (x, y):
                    if p is not None and not isinstance(p, torch.Tensor):
                        raise _refuse(f"points of type {type(p).__name__}")
            same = y is None or y is x
            xd = x.detach() if isinstance(x, torch.Tensor) else x
            G = gramian(k, xd, None if same else (y.detach() if isinstance(y, torch.Tensor) else y))
            if structural and type(G) is not Gramian:
                raise _refuse(type(G).__name__)
        ctx.G, ctx.symmetric = G, (not operator) and (y is None or y is x)
        ctx.shapes = (None if not isinstance(x, torch.Tensor) else (x.shape, x.dtype), None if not isinstance(y, torch.Tensor) else (y.shape, y.dtype),
                      None if theta is None else (theta.dtype, theta.device))
        ctx.save_for_backward(a)
        return G @ a.detach()

    @staticmethod
    @once_differentiable
    def backward(ctx, gbar):
        G = ctx.G
        a, = ctx.saved_tensors
        gbar = gbar.contiguous()
        _, need_x, need_a, need_y, need_theta = ctx.needs_input_grad
        gx = ga = gy = gtheta = None
        if need_a:
            ga = ((G if ctx.symmetric else G.T) @ gbar).to(a.dtype).reshape(a.shape)
        if need_theta:
            dt, dev = ctx.shapes[2]
            gtheta = bilinear_gradient(G, gbar, a)[1].to(device=dev, dtype=dt)
        if need_x or need_y:
            dX, dY = bilinear_input_gradient(G, gbar, a)
            if need_x:
                gx = dX.to(ctx.shapes[0][1]).reshape(ctx.shapes[0][0])
            if need_y and dY is not None:                       # (y is x: the whole gradient is x's)
                gy = dY.to(ctx.shapes[1][1]).reshape(ctx.shapes[1][0])
        return None, gx, ga, gy, gtheta


def gram_product(k, x, a, y=None, theta=None):
    """gramian(k′, x, y) @ a as a differentiable operation: k′ = with_hyperparameters(k, theta) when `theta` (a float64 tensor in
    hyperparameters(k) order) is given, otherwise k; `a` is (m,) or (m, p).  Gradients flow to whichever of x, y, a and theta require
    them (module docstring); the points are detached for the forward pass, so the Gramian itself holds no graph.

    When x, y or theta require a gradient the operator has to be the plain Gramian of a kernel bilinear_gradient supports (a simple
    isotropic kernel or a Sum of them, optionally under ARD / a diagonal ScaledInputKernel) on point tensors: everything else —
    Toeplitz, Kronecker, block, spectral-mixture and sharded operators among them — raises UnsupportedKernel by name, the kernel and the
    point types before anything is built (a spectral mixture has its own entry: spectral_mixture_product).  When only `a` requires a gradient every operator with `.T` works; `k` may then also be an
    operator that was built already (x, y and theta None)."""
    return _GramProduct.apply(k, x, a, y, theta)


def _refuse_sm(what):
    return _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"spectral_mixture_product: {what} is not supported (a spectral mixture that gramian(k, x[, y]) runs "
                                                     "as a SpectralMixtureGramian, on point tensors; every other kernel: gram_product)")


class _SpectralMixtureProduct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, k, x, a, y, theta):
        if not isinstance(k, K.AbstractKernel):                 # what can be refused before anything is built
            raise _refuse_sm(type(k).__name__)
        for p in (x, y):
            if p is not None and not isinstance(p, torch.Tensor):
                raise _refuse_sm(f"points of type {type(p).__name__}")
        if x is None:
            raise _refuse_sm("x = None")
        if theta is not None:
            k = K.with_hyperparameters(k, theta.detach().cpu().numpy())
        if K.device_spec(k) is not None:
            raise _refuse_sm(f"{type(k).__name__} (a kernel with a device path of its own)")
        if K.spectral_mixture_spec(k, _point_dim(x)) is None:
            raise _refuse_sm(f"{type(k).__name__} (not a spectral mixture with a device path)")
        same = y is None or y is x
        G = gramian(k, x.detach(), None if same else y.detach())
        if type(G) is not SpectralMixtureGramian:
            raise _refuse_sm(type(G).__name__)
        ctx.G, ctx.symmetric = G, same
        ctx.shapes = ((x.shape, x.dtype), None if y is None else (y.shape, y.dtype), None if theta is None else (theta.dtype, theta.device))
        ctx.save_for_backward(a)
        return G @ a.detach()

    @staticmethod
    @once_differentiable
    def backward(ctx, gbar):
        G = ctx.G
        a, = ctx.saved_tensors
        gbar = gbar.contiguous()
        _, need_x, need_a, need_y, need_theta = ctx.needs_input_grad
        gx = ga = gy = gtheta = None
        if need_a:
            ga = ((G if ctx.symmetric else G.T) @ gbar).to(a.dtype).reshape(a.shape)
        if need_theta:
            dt, dev = ctx.shapes[2]
            gtheta = spectral_mixture_gradient(G, gbar, a)[1].to(device=dev, dtype=dt)
        if need_x or need_y:
            dX, dY = spectral_mixture_input_gradient(G, gbar, a)
            if need_x:
                gx = dX.to(ctx.shapes[0][1]).reshape(ctx.shapes[0][0])
            if need_y and dY is not None:                       # (y is x: the whole gradient is x's)
                gy = dY.to(ctx.shapes[1][1]).reshape(ctx.shapes[1][0])
        return None, gx, ga, gy, gtheta


def spectral_mixture_product(k, x, a, y=None, theta=None):
    """gramian(k′, x, y) @ a of a spectral mixture as a differentiable operation: k′ = with_hyperparameters(k, theta) when `theta` (a
    float64 tensor in hyperparameters(k) order: weights — signed Constants included —, Cosine frequencies and lengthscales) is given,
    otherwise k; `a` is (m,) or (m, p).  The forward pass is the fused product of the SpectralMixtureGramian on detached points; the
    backward pass of an incoming ḡ runs, each only where the input requires a gradient,
        ∂a     = Gᵀ ḡ                                           (G itself for one point set)
        ∂theta = spectral_mixture_gradient(G, ḡ, a)[1]
        ∂x, ∂y = spectral_mixture_input_gradient(G, ḡ, a)        cast to the points' dtypes
    and is once differentiable.  Refused with UnsupportedKernel naming the offender, before anything is built where possible: a kernel
    with a device_spec (gram_product's ground) or one spectral_mixture_spec does not accept, points that are not tensors, and a
    gramian() result that is not a SpectralMixtureGramian."""
    return _SpectralMixtureProduct.apply(k, x, a, y, theta)
