"""`gramian` / `Gramian` / `mul!` — the host-side mirror of src/gramian.jl for the device engine.

Layout conventions (the reference's):
  * a point set is a tensor of shape (n, d) (C-contiguous) — the same memory as Julia's d×n matrix whose
    columns are the points (src/gramian.jl:2,154-155); a 1-D tensor is n scalar points;
  * block vectors of multi-output Gramians are flat and point-major;
  * matrix right-hand sides have shape (m, p).
torch is used for device memory and streams only; every product below runs in libcovgram.so.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _ffi
from . import kernels as K

# ----------------------------------------------------------------------------------------------
# context handling: one covgram_ctx per device, bound to torch's current stream at call time
# ----------------------------------------------------------------------------------------------
_CTX = {}


class _Ctx:
    def __init__(self, device: torch.device):
        self.device = device
        self.handle = _ffi._P()
        self._stream = torch.cuda.current_stream(device).cuda_stream
        _ffi.check(_ffi.lib().covgram_ctx_create(C.byref(self.handle), device.index, _ffi._P(self._stream)))

    def bind_stream(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != self._stream:
            _ffi.check(_ffi.lib().covgram_ctx_set_stream(self.handle, _ffi._P(s)))
            self._stream = s
        return self.handle

    def set_option(self, key: str, value: int):
        _ffi.check(_ffi.lib().covgram_ctx_set_option(self.handle, key.encode(), int(value)))


def kernel_time(device=None, reset=True):
    """(total_ms, launches) of the HIP-event-bracketed dominant kernels since the last reset
    (enable with set_option("time_kernels", 1))."""
    ctx = get_ctx(device)
    ms, cnt = C.c_double(0), C.c_int64(0)
    _ffi.check(_ffi.lib().covgram_ctx_kernel_time(ctx.handle, C.byref(ms), C.byref(cnt), 1 if reset else 0))
    return ms.value, cnt.value


def get_ctx(device=None) -> _Ctx:
    """The library context for `device` (default: torch's current CUDA/HIP device).  Raises if the
    shared library is missing or no gfx950 device is visible — there is no CPU fallback."""
    lib = _ffi.lib()
    if device is None or (isinstance(device, torch.device) and device.type != "cuda"):
        n = C.c_int(0)
        lib.covgram_device_count(C.byref(n))
        if n.value <= 0 or not torch.cuda.is_available():
            raise _ffi.NoDevice(_ffi.ENODEVICE, "no HIP device visible — covgram has no CPU fallback")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device.index not in _CTX:
        _CTX[device.index] = _Ctx(device)
    return _CTX[device.index]


def set_option(key: str, value: int, device=None):
    get_ctx(device).set_option(key, value)


def get_info(key: str, device=None) -> int:
    """covgram_ctx_get_info: e.g. "last_dense_path" (1 lane-per-row direct differences, 2 matrix-core EQ, 3 wide rows)."""
    v = C.c_int64(0)
    _ffi.check(_ffi.lib().covgram_ctx_get_info(get_ctx(device).handle, key.encode(), C.byref(v)))
    return v.value


def _dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return _ffi.F32
    if dt == torch.float64:
        return _ffi.F64
    raise TypeError(f"covgram supports float32/float64 points, got {dt}")


# ----------------------------------------------------------------------------------------------
# inputs: ranges, grids, point tensors
# ----------------------------------------------------------------------------------------------
class StepRangeLen:
    """Julia's `range(start, stop, length)` / StepRangeLen: the trigger for Toeplitz structure
    (src/gramian.jl:167-189)."""

    def __init__(self, start, step, length, dtype=torch.float64):
        self.start, self.step, self.length, self.dtype = float(start), float(step), int(length), dtype

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        if isinstance(i, slice):
            return self.tensor("cpu")[i]
        if i < 0:
            i += self.length
        return self.start + self.step * i

    def __add__(self, c):   # x .+ c keeps the step (test/gramian.jl:169)
        return StepRangeLen(self.start + float(c), self.step, self.length, self.dtype)

    def tensor(self, device):
        idx = torch.arange(self.length, dtype=torch.float64, device=device)
        return (self.start + self.step * idx).to(self.dtype)


def srange(start, stop, length, dtype=torch.float64) -> StepRangeLen:
    """range(start, stop, length)."""
    step = (float(stop) - float(start)) / (length - 1) if length > 1 else 0.0
    return StepRangeLen(start, step, length, dtype)


class LazyGrid:
    """Lazy Cartesian grid (src/lazy_grid.jl:3-38); default enumeration: FIRST axis varies fastest."""

    def __init__(self, *args):
        if len(args) == 2 and isinstance(args[1], int) and not isinstance(args[0], (int, float)):
            args = tuple([args[0]] * args[1])                 # LazyGrid(x, d) = Fill(x, d)  (lazy_grid.jl:11)
        self.args = tuple(args)

    def __len__(self):
        return int(np.prod([len(a) for a in self.args]))

    def ndims(self):
        return len(self.args)

    def points(self, device, dtype=torch.float64, rowmajor=False):
        axes = [(a.tensor(device) if isinstance(a, StepRangeLen) else torch.as_tensor(a, device=device)).to(dtype).reshape(-1)
                for a in self.args]
        mesh = torch.meshgrid(*axes, indexing="ij")
        if rowmajor:       # lazy_grid.jl:40-58
            cols = [g.reshape(-1) for g in mesh]
        else:              # lazy_grid.jl:20-38: first axis fastest == Fortran-order flattening
            cols = [g.permute(*reversed(range(g.dim()))).reshape(-1) for g in mesh]
        return torch.stack(cols, dim=1).contiguous()


def _as_points(x, device=None, dtype=None) -> torch.Tensor:
    if isinstance(x, StepRangeLen):
        dev = device if device is not None else get_ctx().device
        t = x.tensor(dev)
    elif isinstance(x, LazyGrid):
        dev = device if device is not None else get_ctx().device
        t = x.points(dev)
    elif isinstance(x, torch.Tensor):
        t = x
    else:
        t = torch.as_tensor(np.asarray(x))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    if dtype is not None:
        t = t.to(dtype)
    if t.dim() == 1:
        t = t.reshape(-1, 1)
    if t.dim() != 2:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"points must be (n,) or (n, d), got shape {tuple(t.shape)}")
    if t.device.type != "cuda":
        t = t.to(device if device is not None else get_ctx().device)
    return t.contiguous()


class _OwnsHandle:
    """Owner of ONE library handle, a plain ctypes.c_void_p in the attribute named `_slot`, which the C entry named `_destroy` frees:
    at most once, and silently while the interpreter shuts down."""

    _destroy = None
    _slot = "handle"

    def _release(self):
        h = getattr(self, self._slot, None)
        setattr(self, self._slot, None)
        if h:
            getattr(_ffi.lib(), self._destroy)(h)

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


class _Points(_OwnsHandle):
    """Device-resident point set + its covgram_points handle (borrowing the tensor's memory).

    The C ABI's contract for borrowed memory is "unchanged while the handle lives" (the library caches the point set's max norm
    and, on the matrix-core path, its packed fragments).  A lazy Gramian in the reference, however, follows in-place changes of
    its points, so this wrapper watches torch's in-place version counter and re-creates the handle when the tensor was written
    to since the handle was made."""

    _destroy, _slot = "covgram_points_destroy", "_h"

    def __init__(self, t: torch.Tensor):
        self.t = t
        self.ctx = get_ctx(t.device)
        self._create()

    def _create(self):
        t = self.t
        self._h = _ffi._P()
        _ffi.check(_ffi.lib().covgram_points_create(self.ctx.handle, C.byref(self._h), _ffi._P(t.data_ptr()), t.shape[0],
                                                    t.shape[1], _dtype_code(t.dtype), _ffi.DEVICE))
        self._ver = t._version

    @property
    def handle(self):
        if self.t._version != self._ver:                      # points were modified in place: norms / fragments are stale
            self._release()
            self._create()
        return self._h


def _vec_arg(a: torch.Tensor, n: int, dtype, device, what: str) -> torch.Tensor:
    if not isinstance(a, torch.Tensor):
        a = torch.as_tensor(np.asarray(a))
    if a.shape[0] != n:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: {what} has length {a.shape[0]}, expected {n}")
    return a.to(device=device, dtype=dtype)


def _rhs(op, y: torch.Tensor, a, what: str = "a") -> torch.Tensor:
    """The right-hand side of op.mul_(y, a): `a` in op's dtype on op's device, after the one shape check of every product."""
    a = _vec_arg(a, op.shape[1], op.dtype, op.device, what)
    if y.shape[0] != op.shape[0] or y.dtype != op.dtype or tuple(y.shape[1:]) != tuple(a.shape[1:]):
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: y has shape {tuple(y.shape)}, expected ({op.shape[0]}, ...) of {op.dtype}")
    return a


def _staged(y: torch.Tensor, a: torch.Tensor, beta, call) -> torch.Tensor:
    """The one place where a and y of a product y ← α A a + β y meet a C entry, as column-major memory: runs
    call(a_ptr, lda, y_ptr, ldy, nrhs) once and returns y.  A vector is passed contiguous; a matrix (m, p) as its transpose's storage,
    (p, m) row-major == m × p column-major.  The library writes into y itself when y's memory already has that layout; otherwise into a
    staging tensor that is copied back, and that holds y's values only when β ≠ 0 (nothing reads them otherwise).  a is always staged
    before y is written and every C entry accepts any overlap of a and y, so y may alias a.  No columns: y is returned untouched, call
    does not run (the ABI requires nrhs >= 1).  Touches tensor layouts and pointers only: no context, no library, no device API."""
    vec = a.dim() == 1
    if not vec and a.shape[1] == 0:
        return y
    at, yt = (a, y) if vec else (a.t(), y.t())
    a_c = at.contiguous()
    if yt.is_contiguous():
        y_c = yt
    elif beta == 0 and not vec:
        y_c = torch.empty(yt.shape, dtype=y.dtype, device=y.device)
    else:
        y_c = yt.contiguous()
    call(a_c.data_ptr(), max(a.shape[0], 1), y_c.data_ptr(), max(y.shape[0], 1), 1 if vec else a.shape[1])
    if y_c is not yt:
        yt.copy_(y_c)
    return y


def _axpby_(y: torch.Tensor, t: torch.Tensor, alpha, beta) -> torch.Tensor:
    """y ← α t + β y for a product t that was computed in full before y is written (y may alias the product's input)."""
    return y.copy_(alpha * t) if beta == 0 else y.mul_(beta).add_(t, alpha=alpha)


def _overlaps(y: torch.Tensor, a: torch.Tensor) -> bool:
    """True when the memory y may write intersects the memory a is read from (same storage, intersecting byte ranges)."""
    if y.device != a.device or y.untyped_storage().data_ptr() != a.untyped_storage().data_ptr() or y.numel() == 0 or a.numel() == 0:
        return False

    def span(t):
        lo = hi = t.data_ptr()
        for size, stride in zip(t.shape, t.stride()):
            ext = (size - 1) * stride * t.element_size()
            lo, hi = (lo + ext, hi) if ext < 0 else (lo, hi + ext)
        return lo, hi + t.element_size()

    (ylo, yhi), (alo, ahi) = span(y), span(a)
    return ylo < ahi and alo < yhi


# ----------------------------------------------------------------------------------------------
# lazy operators
# ----------------------------------------------------------------------------------------------
class LazyOperator:
    """Common surface of every lazily represented matrix: shape, `@`, `mul_` (= mul!), `to_dense()`."""

    shape = (0, 0)
    dtype = torch.float64
    device = None

    def size(self, i=None):
        return self.shape if i is None else self.shape[i]

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        raise NotImplementedError

    def __matmul__(self, a):
        a = _vec_arg(a, self.shape[1], self.dtype, self.device, "a")
        y = torch.empty((self.shape[0],) + tuple(a.shape[1:]), dtype=self.dtype, device=self.device)
        return self.mul_(y, a, 1.0, 0.0)                      # src/gramian.jl:66-75: zeros + mul!

    def to_dense(self):
        eye = torch.eye(self.shape[1], dtype=self.dtype, device=self.device)
        return self @ eye

    def __add__(self, D):
        return LazyMatrixSum(self, D)                         # src/gramian.jl:55-60

    __radd__ = __add__


def mul_(y, A: LazyOperator, a, alpha=1.0, beta=0.0):
    """LinearAlgebra.mul!(y, A, a, α, β): y ← α A a + β y, returns y."""
    return A.mul_(y, a, alpha, beta)


class _PointPairGramian(LazyOperator):
    """What the lazy Gramians of ONE kernel on two point sets share: the points and their handles, symmetry, the transpose, Matrix(G)
    and indexing.  A subclass says how to build its kind of operator on other points (_on) and makes the one library call of Matrix(G)
    (_matrix)."""

    def __init__(self, k, x, y=None):
        self.k = k
        self.x = _as_points(x)
        self.y = self.x if (y is None or y is x) else _as_points(y, device=self.x.device, dtype=self.x.dtype)
        if self.x.shape[1] != self.y.shape[1]:
            raise _ffi.DimensionMismatch(_ffi.EINVAL, f"inputs have to have the same length: {self.x.shape[1]}, {self.y.shape[1]}")
        self.dtype = self.x.dtype                              # gramian_eltype: T follows the data (src/gramian.jl:30-33)
        self.device = self.x.device
        self.shape = (self.x.shape[0], self.y.shape[0])
        self._px = _Points(self.x)
        self._py = self._px if self.y is self.x else _Points(self.y)

    def _on(self, xi, yj):
        """The same kind of operator, of the same kernel, on the points xi and yj."""
        raise NotImplementedError

    def _matrix(self, out, ldo):
        """The library call that writes the column-major n × m matrix (leading dimension ldo) to the device pointer `out`."""
        raise NotImplementedError

    # -- structure ------------------------------------------------------------------------------
    @property
    def T(self):
        return self._on(self.y, self.x)                        # src/gramian.jl:116-117

    adjoint = T

    def issymmetric(self):
        return self.x is self.y or (self.x.shape == self.y.shape and bool(torch.equal(self.x, self.y)))   # :132

    def to_dense(self):
        """Matrix(G) (src/gramian.jl:102-114) on the device, with the per-pair arithmetic of the product."""
        n, m = self.shape
        buf = torch.empty((m, n), dtype=self.dtype, device=self.device)   # column-major n×m
        if n * m:
            self._px.ctx.bind_stream()
            self._matrix(_ffi._P(buf.data_ptr()), n)
        return buf.t()

    def __getitem__(self, ij):
        """G[i, j] = k(x[i], y[j]) and sub-block indexing (src/gramian.jl:37-52), evaluated on the device from the sliced point sets."""
        i, j = ij
        xi = self.x[i] if not isinstance(i, int) else self.x[i:i + 1]
        yj = self.y[j] if not isinstance(j, int) else self.y[j:j + 1]
        sub = self._on(xi.reshape(-1, self.x.shape[1]), yj.reshape(-1, self.y.shape[1])).to_dense()
        if isinstance(i, int) and isinstance(j, int):
            return sub[0, 0]
        if isinstance(i, int):
            return sub[0]
        if isinstance(j, int):
            return sub[:, 0]
        return sub


class Gramian(_PointPairGramian):
    """Lazy kernel matrix holding (k, x, y) (src/gramian.jl:10-21); O(1) construction, O(n m d) `mul!`."""

    def _on(self, xi, yj):
        return Gramian(self.k, xi, yj)

    def isposdef(self):
        return isinstance(self.k, (K.MercerKernel, K.MultiKernel)) and self.issymmetric()               # :135-137

    def _spec(self):
        # lowered once per Gramian: like the reference's Gramian{T, K, ...}, which holds an immutable kernel by value
        sp = getattr(self, "_spec_cached", None)
        if sp is None:
            sp = self._spec_cached = K.require_device_spec(self.k)
        return sp

    # -- products ---------------------------------------------------------------------------------
    def mul_(self, y, a, alpha=1.0, beta=0.0):
        """src/gramian.jl:78-99.  β == 0 ⇒ y's previous contents (NaN included) are ignored."""
        a = _rhs(self, y, a)
        spec = self._spec()
        ctx = self._px.ctx.bind_stream()
        return _staged(y, a, beta, lambda ap, lda, yp, ldy, nrhs: _ffi.check(_ffi.lib().covgram_mvm(
            ctx, _ffi.kref(spec), self._px.handle, self._py.handle, _ffi._P(ap), lda, _ffi._P(yp), ldy, nrhs, float(alpha), float(beta), _ffi.DEVICE)))

    # -- multi-GPU symmetric form (include/covgram.h: covgram_mvm_sym_partial) ---------------------
    def sym_partial_supported(self, world: int = 1) -> bool:
        """True when rank r of `world` can take its cyclic panels / row blocks of the upper triangle (one point set on both sides: the
        symmetric matrix-core kernels in fp32, the direct-difference symmetric kernels in fp64 and for what the matrix cores refuse);
        depends on the kernel, the points and the world size only, so every rank answers alike — and sym_partial_ raises
        UnsupportedKernel exactly when this says False."""
        if self._px is not self._py and not (self._px.t.data_ptr() == self._py.t.data_ptr() and self.shape[0] == self.shape[1]):
            return False
        try:
            spec = self._spec()
        except Exception:
            return False
        ok = C.c_int32(0)
        _ffi.check(_ffi.lib().covgram_mvm_sym_supported(self._px.ctx.bind_stream(), _ffi.kref(spec), self._px.handle, int(world), C.byref(ok)))
        return bool(ok.value)

    def sym_partial_(self, y, a, rank: int, world: int):
        """y <- the part of G a that comes from the upper-triangle tiles of the panels p ≡ rank (mod world) and their mirror
        images; the partials of all ranks sum to G a.  Vectors only."""
        n, m = self.shape
        a = _vec_arg(a, m, self.dtype, self.device, "a")
        if a.dim() != 1 or y.shape != (n,) or y.dtype != self.dtype or not y.is_contiguous():
            raise _ffi.DimensionMismatch(_ffi.EINVAL, "sym_partial_: contiguous vectors of length n expected")
        a_c = a.contiguous()
        _ffi.check(_ffi.lib().covgram_mvm_sym_partial(self._px.ctx.bind_stream(), _ffi.kref(self._spec()), self._px.handle,
                                                      _ffi._P(a_c.data_ptr()), _ffi._P(y.data_ptr()), int(rank), int(world)))
        return y

    def _matrix(self, out, ldo):
        _ffi.check(_ffi.lib().covgram_matrix(self._px.ctx.handle, _ffi.kref(self._spec()), self._px.handle, self._py.handle, out, ldo, _ffi.DEVICE))


# ----------------------------------------------------------------------------------------------
# hyper-parameter and input gradients of bilinear forms (include/covgram.h: covgram_bilinear_grad, covgram_bilinear_input_grad)
# ----------------------------------------------------------------------------------------------
BILINEAR_MAX_NVEC, BILINEAR_MAX_D = _ffi.BILINEAR_MAX_NVEC, _ffi.BILINEAR_MAX_D


def _bilinear_term(k, fn="bilinear_gradient"):
    """(spec, rules) of one simple isotropic term: the covgram_kernel the device runs and, per leaf of hyperparameters(k) in its
    order, the chain rule ("scale", power, c) | ("l", l) | ("param",).  Raises UnsupportedKernel naming what is not supported."""
    rules = []
    def unsupported(what):
        return _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"{fn}: {what} is not supported (simple isotropic kernels and Sums of them only)")
    def walk(node, power):
        if isinstance(node, K.Product):
            rest = [a for a in node.args if not isinstance(a, K.Constant)]
            if len(rest) != 1:
                raise unsupported("a Product of two non-constant kernels" if len(rest) > 1 else "a Product of Constants")
            for a in node.args:
                if isinstance(a, K.Constant):
                    rules.append(("scale", power, a.c))
                else:
                    walk(a, power)
        elif isinstance(node, K.Power):
            if node.p < 1:
                raise unsupported(f"Power with exponent {node.p}")
            walk(node.k, power * node.p)
        elif isinstance(node, K.Lengthscale):
            walk(node.k, power)
            rules.append(("l", node.l))
        elif isinstance(node, (K.DotProductKernel,)):
            raise unsupported(f"the dot-product kernel {type(node).__name__}")
        elif isinstance(node, K.Matern) and not (float(node.nu - 0.5).is_integer() and 0 <= int(node.nu - 0.5) <= _ffi.MATERNP_MAX_P):
            raise unsupported(f"Matern with real nu = {node.nu}")
        elif type(node) in K._OWN_PARAMETER:
            rules.append(("param",))
        elif isinstance(node, K._NO_PARAMETER):
            pass
        else:
            raise unsupported(type(node).__name__)
    walk(k, 1)
    spec = K._simple_spec(k)
    if spec is None or spec.trait != _ffi.ISOTROPIC:
        raise unsupported(type(k).__name__)
    return spec, rules


def _bilinear_plan(k, fn="bilinear_gradient"):
    """Terms of `k` (a simple kernel, or a Sum of simple kernels and Constants, nested Sums flattened in walk order)."""
    if isinstance(k, K.Sum):
        return [t for a in k.args for t in _bilinear_plan(a, fn)]
    if isinstance(k, K.Constant):
        return [(None, [("const", k.c)])]
    return [_bilinear_term(k, fn)]


def _bilinear_setup(fn, G, U, A):
    """What bilinear_gradient and bilinear_input_gradient (`fn`: the name in the messages) share: the refusals, before any device call,
    and the weights as the device wants them.  Returns (scaled, plan, U, A, Ut, At): the diagonal ScaledInputKernel in front of the
    kernel or None, the terms, U (n, nvec) and A (m, nvec) in the Gramian's dtype on its device and their transposes (nvec, n) / (nvec, m)
    row-major == column-major n × nvec / m × nvec."""
    if type(G) is not Gramian:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"{fn}: {type(G).__name__} is not supported (the Gramian of gramian(k, x[, y]) only)")
    scaled = getattr(G, "scaled_input", None)
    if scaled is not None and not scaled.diagonal:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"{fn}: ScaledInputKernel with a full matrix U is not supported")
    plan = _bilinear_plan(G.k, fn)
    if scaled is not None and (len(plan) != 1 or plan[0][0] is None):
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"{fn}: ARD over a Sum is not supported")
    n, m = G.shape
    d = G.x.shape[1]
    if d > BILINEAR_MAX_D:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"{fn}: d = {d} exceeds {BILINEAR_MAX_D}")
    U = _vec_arg(U, n, G.dtype, G.device, "U")
    A = _vec_arg(A, m, G.dtype, G.device, "A")
    U = U[:, None] if U.dim() == 1 else U
    A = A[:, None] if A.dim() == 1 else A
    if U.dim() != 2 or A.dim() != 2 or U.shape[1] != A.shape[1] or U.shape[1] < 1:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: U has shape {tuple(U.shape)}, A {tuple(A.shape)}: equal column counts expected")
    return scaled, plan, U, A, U.t().contiguous(), A.t().contiguous()


def bilinear_chain_rules(rules, out, scaled=None):
    """The host chain rules of bilinear_gradient for one term: `out` = the numbers of covgram_bilinear_grad (fp64), `rules` from
    _bilinear_term, `scaled` = the diagonal ScaledInputKernel in front of the term (out is then per dimension, on the transformed
    points).  Returns the term's gradient entries in hyperparameters order (the ARD entries last)."""
    out = [float(v) for v in out]
    ssum = math.fsum(out[2:])
    g = []
    for r in rules:
        if r[0] == "scale":
            g.append(r[1] * out[0] / r[2])                     # k ∝ c^power
        elif r[0] == "l":
            g.append(-2.0 / r[1] * ssum)                       # k = f(s / l²)
        elif r[0] == "param":
            g.append(out[1])
        else:                                                  # a Constant term of a Sum: Σ W
            g.append(out[0])
    if scaled is not None:
        if scaled.l is not None:
            g += [-2.0 / float(l) * out[2 + c] for c, l in enumerate(scaled.l)]
        else:                                                  # s = Σ_c (U_c Δ_c)²: ∂/∂U_c = (2 / U_c) (∂k/∂s) (U_c Δ_c)²
            g += [(2.0 / float(u) * out[2 + c]) if u != 0 else 0.0 for c, u in enumerate(scaled.U)]
    return g


def bilinear_gradient(G, U, A):
    """(value, grad) of the bilinear form Σ_t U[:, t]ᵀ G A[:, t] = Σ_ij W_ij k(x_i, y_j), W = U Aᵀ, with respect to the
    hyper-parameters of the kernel G was built from, in ONE fused pass over the pairs per term (csrc/bilin_grad.hip): W is formed per
    pair in registers, nothing of size n × m exists.  `G` is the Gramian of gramian(k, x[, y]); U is (n,) or (n, nvec), A (m,) or
    (m, nvec).  `grad` is a float64 CPU tensor in hyperparameters(k) order, `value` a float64 0-dim CPU tensor.

    The device returns, per term, out[0] = Σ W k, out[1] = Σ W ∂k/∂param and out[2 + c] = Σ W (∂k/∂s)(x_c − y_c)² (one number Σ W (∂k/∂s) s
    without ARD); the chain rules are applied here (bilinear_chain_rules):
        ∂/∂scale = power · out[0] / scale          (Constant(c) · k under Power: k ∝ c^power)
        ∂/∂l     = −(2 / l) Σ_c out[2 + c]         (Lengthscale; nested lengthscales each get this with their own l)
        ∂/∂param = out[1]                          (RQ α, γ-exponential γ, IMQ c)
        ∂/∂l_c   = −(2 / l_c) out[2 + c]           (ARD(k, l): on the points as gramian pre-scaled them; ScaledInputKernel(k, U) stores
                                                    the multipliers: ∂/∂U_c = +(2 / U_c) out[2 + c])
    A Sum of such terms takes one launch per term, gradients concatenate; a Constant term's derivative is Σ W.  More than 32 columns
    run in chunks of 32 summed in fp64.  Everything else — a Product of two non-constant kernels, dot-product kernels, Matérn with real
    ν, spectral mixtures (their own pass: spectral_mixture_gradient), block Gramians, Toeplitz / Kronecker / sparse / Barnes–Hut operators,
    ShardedGramian — raises UnsupportedKernel by name before any device call."""
    scaled, plan, U, A, Ut, At = _bilinear_setup("bilinear_gradient", G, U, A)
    n, m = G.shape
    d = G.x.shape[1]
    nvec = U.shape[1]
    per_dim = 1 if scaled is not None else 0
    nout = 2 + (d if per_dim else 1)
    lib = _ffi.lib()
    ctx = G._px.ctx.bind_stream()
    py = None if G._py is G._px else G._py.handle
    value, grad = 0.0, []
    for spec, rules in plan:
        if spec is None:                                       # Constant term c: value c Σ W, derivative Σ W = Σ_t (1ᵀu_t)(1ᵀa_t)
            sw = float((U.sum(0).double() * A.sum(0).double()).sum())
            out = [sw] + [0.0] * (nout - 1)
            value += rules[0][1] * sw
        else:
            acc = torch.zeros(nout, dtype=torch.float64)
            for c0 in range(0, nvec, BILINEAR_MAX_NVEC):
                nv = min(BILINEAR_MAX_NVEC, nvec - c0)
                o = torch.empty(nout, dtype=torch.float64, device=G.device)
                _ffi.check(lib.covgram_bilinear_grad(ctx, _ffi.kref(spec), G._px.handle, py, _ffi._P(Ut[c0:].data_ptr()), max(n, 1),
                                                     _ffi._P(At[c0:].data_ptr()), max(m, 1), nv, per_dim,
                                                     C.cast(o.data_ptr(), C.POINTER(C.c_double)), _ffi.DEVICE))
                acc += o.cpu()
            out = acc.tolist()
            value += out[0]
        grad += bilinear_chain_rules(rules, out, scaled)
    return torch.tensor(value, dtype=torch.float64), torch.tensor(grad, dtype=torch.float64)


def _input_grad_device(spec, px, py, Ut, At, rows, cols, d, device):
    """Σ_j W_ij 2 (∂k/∂s)_ij (x_i − y_j) for the row points `px` against the column points `py` (None: the row points themselves) as a
    float64 (rows, d) tensor on `device`: covgram_bilinear_input_grad on chunks of at most 32 of the columns of Ut (nvec, rows) and
    At (nvec, cols), summed in fp64 on the device."""
    lib = _ffi.lib()
    ctx = px.ctx.bind_stream()
    total = None
    for c0 in range(0, Ut.shape[0], BILINEAR_MAX_NVEC):
        nv = min(BILINEAR_MAX_NVEC, Ut.shape[0] - c0)
        o = torch.empty((rows, d), dtype=torch.float64, device=device)
        _ffi.check(lib.covgram_bilinear_input_grad(ctx, _ffi.kref(spec), px.handle, None if py is None else py.handle, _ffi._P(Ut[c0:].data_ptr()),
                                                   max(rows, 1), _ffi._P(At[c0:].data_ptr()), max(cols, 1), nv,
                                                   C.cast(o.data_ptr(), C.POINTER(C.c_double)), _ffi.DEVICE))
        total = o if total is None else total.add_(o)
    return total


def _same_tensor(U, A) -> bool:
    return (isinstance(U, torch.Tensor) and isinstance(A, torch.Tensor) and U.dtype == A.dtype and U.device == A.device
            and U.data_ptr() == A.data_ptr() and U.shape == A.shape and U.stride() == A.stride())


def bilinear_input_gradient(G, U, A):
    """(dX, dY): the gradients of the bilinear form F = Σ_t U[:, t]ᵀ G A[:, t] = Σ_ij W_ij k(x_i, y_j), W = U Aᵀ, with respect to the
    points of G, as float64 tensors (n, d) and (m, d) on G's device, in ONE fused pass over the pairs per term and side
    (csrc/input_grad.hip): with s_ij = |x_i − y_j|²
        dX[i, c] =  Σ_j W_ij · 2 (∂k/∂s)_ij (x_ic − y_jc)        dY[j, c] = −Σ_i W_ij · 2 (∂k/∂s)_ij (x_ic − y_jc)
    dY is the same device call with the roles swapped, (Y, X, A, U): an isotropic k is symmetric in its arguments.  When G was built
    from one point set (G.y is G.x) ONE array is returned and dY is None: dX = call(X, U, A) + call(X, A, U); when U and A are the same
    tensor (same storage, shape and strides) that is one call, doubled (exact: both routes agree bit for bit).  A pair at distance 0
    adds exactly 0, also for kernels whose derivative is unbounded there (Exponential, γ-exponential, MaternP(0)).

    `G`, U and A are those of bilinear_gradient: the Gramian of a simple isotropic kernel or of a Sum of them (one launch per term and
    side, summed in fp64 on the device; a Constant term adds 0); more than 32 columns run in chunks of 32 summed in fp64; everything
    bilinear_gradient refuses is refused here by name before any device call.  Under a diagonal ScaledInputKernel / ARD the Gramian holds
    x′ = x ∘ u (u_c = 1 / l_c or U_c), and the result is multiplied by u_c: the gradients are with respect to the points the caller passed.
    For any other Gramian whose points were transformed when it was built (Warped, Periodic) the gradients are with respect to the
    points the Gramian HOLDS, G.x and G.y."""
    same_weights = _same_tensor(U, A)
    scaled, plan, U, A, Ut, At = _bilinear_setup("bilinear_input_gradient", G, U, A)
    n, m = G.shape
    d = G.x.shape[1]
    symmetric = G._py is G._px
    dX = torch.zeros((n, d), dtype=torch.float64, device=G.device)
    dY = None if symmetric else torch.zeros((m, d), dtype=torch.float64, device=G.device)
    for spec, _ in plan:
        if spec is None:                                       # a Constant term does not depend on the points
            continue
        if symmetric:
            t = _input_grad_device(spec, G._px, None, Ut, At, n, n, d, G.device)
            dX += 2.0 * t if same_weights else t + _input_grad_device(spec, G._px, None, At, Ut, n, n, d, G.device)
        else:
            dX += _input_grad_device(spec, G._px, G._py, Ut, At, n, m, d, G.device)
            dY += _input_grad_device(spec, G._py, G._px, At, Ut, m, n, d, G.device)
    if scaled is not None:                                     # x′ = x ∘ u: ∂/∂x_c = u_c ∂/∂x′_c
        u = torch.as_tensor(scaled.U, dtype=torch.float64, device=G.device)
        dX *= u
        if dY is not None:
            dY *= u
    return dX, dY


class SpectralMixtureGramian(_OwnsHandle, _PointPairGramian):
    """Lazy Gramian of a spectral mixture Σ_q w_q Cosine(μ_q) ARD(EQ(), l_q) (src/stationary.jl:213-217), a GenericInput kernel in the
    reference's terms: holds (k, x, y), the point handles and the covgram_sm handle with the mixture's parameters; `mul!` and
    Matrix(G) are ONE fused pass each (covgram_sm_mvm / covgram_sm_matrix).  `gramian` builds it for exactly the kernels that
    kernels.spectral_mixture_spec recognises and kernels.device_spec does not."""

    _destroy = "covgram_sm_destroy"

    def __init__(self, k, x, y=None, spec=None):
        self.w, self.mu, self.inv_l = spec if spec is not None else K.require_sm_spec(k, _point_dim(x))   # refusals come before any device call
        super().__init__(k, x, y)
        self.handle = _ffi._P()
        as_d = lambda v: np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
        _ffi.check(_ffi.lib().covgram_sm_create(self._px.ctx.bind_stream(), C.byref(self.handle), int(self.w.shape[0]), int(self.x.shape[1]), as_d(self.w),
                                                as_d(self.mu), as_d(self.inv_l), _dtype_code(self.dtype)))

    def _on(self, xi, yj):
        return SpectralMixtureGramian(self.k, xi, yj, (self.w, self.mu, self.inv_l))   # the transpose too: cos is even, k(y, x) = k(x, y)

    def isposdef(self):
        return self.issymmetric() and bool(np.all(self.w >= 0))

    def isotropic(self) -> bool:
        """covgram_sm_info's flag: every component has one lengthscale over all dimensions."""
        iso = C.c_int32(0)
        _ffi.check(_ffi.lib().covgram_sm_info(self.handle, None, None, None, C.byref(iso)))
        return bool(iso.value)

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        """y ← α G a + β y for a vector or a matrix a; β == 0 ⇒ y's previous contents (NaN included) are ignored."""
        a = _rhs(self, y, a)
        self._px.ctx.bind_stream()
        return _staged(y, a, beta, lambda ap, lda, yp, ldy, nrhs: _ffi.check(_ffi.lib().covgram_sm_mvm(
            self.handle, self._px.handle, self._py.handle, _ffi._P(ap), lda, _ffi._P(yp), ldy, nrhs, float(alpha), float(beta), _ffi.DEVICE)))

    def _matrix(self, out, ldo):
        _ffi.check(_ffi.lib().covgram_sm_matrix(self.handle, self._px.handle, self._py.handle, out, ldo, _ffi.DEVICE))


class MixedGramian(_PointPairGramian):
    """Lazy SCALAR Gramian of a Sum / Product / Power whose factors do not share one input trait — EQ() + Dot(), EQ() * (Dot()**2 + 1),
    MaternP(2) + Dot()**2 + NeuralNetwork(): GenericInput in the reference's terms, its threaded loop src/gramian.jl:78-87.  `mul!` is
    covgram_mvm_mixed (plain terms on the kernels behind covgram_mvm, the rest in one fused pass), Matrix(G) and indexing are
    covgram_matrix_mixed.  `gramian` builds it for exactly the kernels that have neither a covgram_kernel encoding nor a
    spectral-mixture one and that kernels.mixed_spec lowers.  Hyper-parameter gradients of its bilinear forms are mixed_bilinear_gradient
    (bilinear_gradient refuses it).  Input gradients, sparse, Barnes-Hut, pivoted Cholesky and sharded forms do not exist: they raise
    UnsupportedKernel naming this class."""

    def __init__(self, k, x, y=None, spec=None):
        self._spec = spec if spec is not None else K.require_mixed_spec(k)   # refusals come before any device call
        super().__init__(k, x, y)

    def _on(self, xi, yj):
        return MixedGramian(self.k, xi, yj, self._spec)

    def isposdef(self):
        return K.ismercer(self.k) and self.issymmetric()

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        """y ← α G a + β y for a vector or a matrix a; β == 0 ⇒ y's previous contents (NaN included) are ignored."""
        a = _rhs(self, y, a)
        ctx = self._px.ctx.bind_stream()
        return _staged(y, a, beta, lambda ap, lda, yp, ldy, nrhs: _ffi.check(_ffi.lib().covgram_mvm_mixed(
            ctx, C.byref(self._spec), self._px.handle, self._py.handle, _ffi._P(ap), lda, _ffi._P(yp), ldy, nrhs, float(alpha), float(beta), _ffi.DEVICE)))

    def _matrix(self, out, ldo):
        _ffi.check(_ffi.lib().covgram_matrix_mixed(self._px.ctx.handle, C.byref(self._spec), self._px.handle, self._py.handle, out, ldo, _ffi.DEVICE))

    def sym_partial_supported(self, world: int = 1) -> bool:
        return False

    def sym_partial_(self, y, a, rank: int, world: int):
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, "sym_partial_: MixedGramian has no symmetric (upper-triangle) partial form")


def mixed_bilinear_gradient(G, U, A, _spec=None):
    """(value, grad) of the bilinear form Σ_t U[:, t]ᵀ G A[:, t] = Σ_ij W_ij k(x_i, y_j), W = U Aᵀ, with respect to EVERY hyper-parameter of
    a Sum / Product / Power whose factors carry their own input traits, in ONE fused pass over the pairs (csrc/mixed_bilin_grad.hip,
    covgram_bilinear_grad_mixed): W is formed per pair in registers, nothing of size n × m exists.  `G` is the MixedGramian of
    gramian(k, x[, y]) — EQ() + Dot(), EQ() * (Dot()**2 + 1), MaternP(2) + Dot()**2 + NeuralNetwork() — or a plain Gramian without
    ARD / ScaledInputKernel in front, which covers what bilinear_gradient leaves out: Products of two non-constant same-trait kernels and
    dot-product kernels such as Polynomial(3, σ).  U is (n,) or (n, nvec), A (m,) or (m, nvec).  `value` is a float64 0-dim CPU tensor,
    `grad` a float64 CPU tensor in hyperparameters(G.k) order.  The device returns 24 numbers (include/covgram.h); the chain rules to the
    leaves of the kernel tree are the matrix J of kernels.require_mixed_parameter_spec: grad = J @ out, value = Σ_t c_t out[t].  More
    than 32 columns run in chunks of 32 summed in fp64.  Everything else — spectral mixtures, block, structured, sparse and sharded
    operators, a Gramian behind ARD / ScaledInputKernel, and every kernel the lowering refuses (Matern with real ν, Cosine, more than
    8 terms or factors) — raises UnsupportedKernel by name before any device call."""
    fn = "mixed_bilinear_gradient"
    if type(G) is not MixedGramian and type(G) is not Gramian:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"{fn}: {type(G).__name__} is not supported (the MixedGramian or Gramian of gramian(k, x[, y]) only)")
    if getattr(G, "scaled_input", None) is not None:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"{fn}: a Gramian behind {type(G.scaled_input).__name__} (ARD) is not supported")
    comp, J = _spec if _spec is not None else K.require_mixed_parameter_spec(G.k)
    n, m = G.shape
    d = G.x.shape[1]
    if d > BILINEAR_MAX_D:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"{fn}: d = {d} exceeds {BILINEAR_MAX_D}")
    U = _vec_arg(U, n, G.dtype, G.device, "U")
    A = _vec_arg(A, m, G.dtype, G.device, "A")
    U = U[:, None] if U.dim() == 1 else U
    A = A[:, None] if A.dim() == 1 else A
    if U.dim() != 2 or A.dim() != 2 or U.shape[1] != A.shape[1] or U.shape[1] < 1:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: U has shape {tuple(U.shape)}, A {tuple(A.shape)}: equal column counts expected")
    Ut, At = U.t().contiguous(), A.t().contiguous()
    nvec = U.shape[1]
    lib = _ffi.lib()
    ctx = G._px.ctx.bind_stream()
    py = None if G._py is G._px else G._py.handle
    acc = torch.zeros(_ffi.MIXED_GRAD_NOUT, dtype=torch.float64)
    for c0 in range(0, nvec, BILINEAR_MAX_NVEC):
        nv = min(BILINEAR_MAX_NVEC, nvec - c0)
        o = torch.empty(_ffi.MIXED_GRAD_NOUT, dtype=torch.float64, device=G.device)
        _ffi.check(lib.covgram_bilinear_grad_mixed(ctx, C.byref(comp), G._px.handle, py, _ffi._P(Ut[c0:].data_ptr()), max(n, 1),
                                                   _ffi._P(At[c0:].data_ptr()), max(m, 1), nv, C.cast(o.data_ptr(), C.POINTER(C.c_double)), _ffi.DEVICE))
        acc += o.cpu()
    out = acc.numpy()
    value = math.fsum(c * out[t] for t, c in enumerate(K.mixed_term_coefficients(comp)))
    return torch.tensor(value, dtype=torch.float64), torch.from_numpy(J @ out)


def _sm_setup(fn, G, U, A):
    """What spectral_mixture_gradient and spectral_mixture_input_gradient (`fn`: the name in the messages) share: the refusals, before any
    device call, and the weights as the device wants them.  Returns (U, A, Ut, At): U (n, nvec) and A (m, nvec) in the Gramian's dtype
    on its device and their transposes (nvec, n) / (nvec, m), row-major == column-major n × nvec / m × nvec."""
    if type(G) is not SpectralMixtureGramian:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"{fn}: {type(G).__name__} is not supported (the SpectralMixtureGramian of gramian(k, x[, y]) only)")
    n, m = G.shape
    d = G.x.shape[1]
    if K.spectral_mixture_spec(G.k, d) is None:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"{fn}: {type(G.k).__name__} is not a spectral mixture with a device path")
    U = _vec_arg(U, n, G.dtype, G.device, "U")
    A = _vec_arg(A, m, G.dtype, G.device, "A")
    U = U[:, None] if U.dim() == 1 else U
    A = A[:, None] if A.dim() == 1 else A
    if U.dim() != 2 or A.dim() != 2 or U.shape[1] != A.shape[1] or U.shape[1] < 1:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: U has shape {tuple(U.shape)}, A {tuple(A.shape)}: equal column counts expected")
    return U, A, U.t().contiguous(), A.t().contiguous()


def spectral_mixture_gradient(G, U, A):
    """(value, grad) of the bilinear form Σ_t U[:, t]ᵀ G A[:, t] = Σ_ij W_ij k(x_i, y_j), W = U Aᵀ, with respect to the weights,
    frequencies and lengthscales of the spectral mixture G was built from, in ONE fused pass over the pairs (csrc/sm_grad.hip,
    covgram_bilinear_grad_sm): all Q(1 + 2d) derivatives at once, W formed per pair in registers, nothing of size n × m exists.
    `G` is a SpectralMixtureGramian; U is (n,) or (n, nvec), A (m,) or (m, nvec).  `value` is a float64 0-dim CPU tensor, `grad` a
    float64 CPU tensor in hyperparameters(G.k) order; the chain rules from the device's numbers to the leaves of the kernel tree are
    kernels.spectral_mixture_chain_rules.  More than 32 columns run in chunks of 32 summed in fp64.  The parameters are those the
    handle holds: rounded once to the points' dtype.  Anything but a SpectralMixtureGramian of a tree spectral_mixture_spec accepts
    raises UnsupportedKernel by name before any device call.  The gradients with respect to the points are
    spectral_mixture_input_gradient, and autograd through the product of a mixture is spectral_mixture_product
    (bilinear_input_gradient and gram_product themselves refuse mixtures)."""
    U, A, Ut, At = _sm_setup("spectral_mixture_gradient", G, U, A)
    n, m = G.shape
    d = G.x.shape[1]
    nvec = U.shape[1]
    nout = int(G.w.shape[0]) * (1 + 2 * d)
    lib = _ffi.lib()
    G._px.ctx.bind_stream()
    py = None if G._py is G._px else G._py.handle
    acc = torch.zeros(nout, dtype=torch.float64)
    for c0 in range(0, nvec, BILINEAR_MAX_NVEC):
        nv = min(BILINEAR_MAX_NVEC, nvec - c0)
        o = torch.empty(nout, dtype=torch.float64, device=G.device)
        _ffi.check(lib.covgram_bilinear_grad_sm(G.handle, G._px.handle, py, _ffi._P(Ut[c0:].data_ptr()), max(n, 1), _ffi._P(At[c0:].data_ptr()),
                                                max(m, 1), nv, C.cast(o.data_ptr(), C.POINTER(C.c_double)), _ffi.DEVICE))
        acc += o.cpu()
    value, grad = K.spectral_mixture_chain_rules(G.k, acc.numpy(), d)
    return torch.tensor(value, dtype=torch.float64), torch.tensor(grad, dtype=torch.float64)


def _sm_input_grad_device(G, px, py, Ut, At, rows, cols, d):
    """covgram_bilinear_input_grad_sm with G's handle for the row points `px` against the column points `py` (None: the row points
    themselves) as a float64 (rows, d) tensor on G's device: chunks of at most 32 of the columns of Ut (nvec, rows) and At (nvec, cols),
    summed in fp64 on the device."""
    lib = _ffi.lib()
    px.ctx.bind_stream()
    total = None
    for c0 in range(0, Ut.shape[0], BILINEAR_MAX_NVEC):
        nv = min(BILINEAR_MAX_NVEC, Ut.shape[0] - c0)
        o = torch.empty((rows, d), dtype=torch.float64, device=G.device)
        _ffi.check(lib.covgram_bilinear_input_grad_sm(G.handle, px.handle, None if py is None else py.handle, _ffi._P(Ut[c0:].data_ptr()), max(rows, 1),
                                                      _ffi._P(At[c0:].data_ptr()), max(cols, 1), nv, C.cast(o.data_ptr(), C.POINTER(C.c_double)),
                                                      _ffi.DEVICE))
        total = o if total is None else total.add_(o)
    return total


def spectral_mixture_input_gradient(G, U, A):
    """(dX, dY): the gradients of the bilinear form F = Σ_t U[:, t]ᵀ G A[:, t] = Σ_ij W_ij k(x_i, y_j), W = U Aᵀ, of a spectral mixture
    with respect to the points of G, as float64 tensors (n, d) and (m, d) on G's device, in ONE fused pass over the pairs per side
    (csrc/sm_input_grad.hip, covgram_bilinear_input_grad_sm): with r = x_i − y_j, φ_q = 2π μ_q·r and e_q = exp(−½ Σ_k (r_k / l_qk)²)
        dX[i, c] = Σ_j W_ij Σ_q w_q e_q (−2π μ_qc sin φ_q − r_c cos φ_q / l_qc²)
    dY is the same device call with the roles swapped, (Y, X, A, U): the mixture is symmetric in its arguments.  When G was built from
    one point set (G.y is G.x) ONE array is returned and dY is None: dX = call(X, U, A) + call(X, A, U); when U and A are the same tensor
    (same storage, shape and strides) that is one call, doubled (exact: both routes agree bit for bit).  A pair at distance 0 adds
    exactly 0.  `G` is a SpectralMixtureGramian; U is (n,) or (n, nvec), A (m,) or (m, nvec); more than 32 columns run in chunks of 32
    summed in fp64 on the device.  The parameters are those the handle holds: rounded once to the points' dtype.  Anything but a
    SpectralMixtureGramian of a tree spectral_mixture_spec accepts raises UnsupportedKernel by name before any device call, as
    spectral_mixture_gradient does.  The gradients are with respect to the points the Gramian HOLDS, G.x and G.y."""
    same_weights = _same_tensor(U, A)
    U, A, Ut, At = _sm_setup("spectral_mixture_input_gradient", G, U, A)
    n, m = G.shape
    d = G.x.shape[1]
    if G._py is G._px:
        t = _sm_input_grad_device(G, G._px, None, Ut, At, n, n, d)
        return (2.0 * t if same_weights else t + _sm_input_grad_device(G, G._px, None, At, Ut, n, n, d)), None
    return _sm_input_grad_device(G, G._px, G._py, Ut, At, n, m, d), _sm_input_grad_device(G, G._py, G._px, At, Ut, m, n, d)


BLOCK_MATRIX_MAX_D = 64     # covgram_block_matrix, gradient kinds: rows in registers (include/covgram.h)


def flat_cover(I, size, B):
    """A flat index (int or slice) into a point-major block vector of `size` = (points) B entries -> (p0, p1, rel): the points
    [p0, p1) that cover it and the same index relative to entry p0 B (flat index I = point I // B, component I % B)."""
    if isinstance(I, slice):
        idx = range(*I.indices(size))
        if len(idx) == 0:
            return 0, 0, slice(0, 0)
        lo, hi = min(idx[0], idx[-1]), max(idx[0], idx[-1])
        p0, p1 = lo // B, hi // B + 1
        if idx.step < 0:                                     # torch has no negative strides: an index list
            return p0, p1, [v - p0 * B for v in idx]
        return p0, p1, slice(idx[0] - p0 * B, idx[-1] + 1 - p0 * B, idx.step)
    I = int(I)
    if I < 0:
        I += size
    if not 0 <= I < size:
        raise IndexError(f"index {I} out of range for {size} entries")
    return I // B, I // B + 1, I % B


class BlockGramian(LazyOperator):
    """Gramian of a GradientKernel: the lazy (n d)×(m d) BlockFactorization of src/gramian.jl:120-123 whose
    `mul!` is blockmul! (src/gramian.jl:241-257) with the O(d) block product of src/gradient.jl:86-115."""

    def __init__(self, g, x, y=None):
        self.g = g
        self.value = isinstance(g, K.ValueGradientKernel)      # blocks of d+1: src/gradient.jl:400-474
        self.inner = Gramian(g.k, x, y)
        n, m = self.inner.shape
        self.d = self.inner.x.shape[1]
        self.block_size = self._block_size(self.d)
        self.shape = (n * self.block_size, m * self.block_size)
        self.dtype, self.device = self.inner.dtype, self.inner.device

    def issymmetric(self):
        return self.inner.issymmetric()

    def _block_size(self, d):
        return d + 1 if self.value else d

    def _lower(self):
        return K.require_device_spec(self.g.k)   # GenericInput gradient kernels have no device path

    def _entry(self):
        return _ffi.lib().covgram_valgrad_mvm if self.value else _ffi.lib().covgram_grad_mvm

    def _kind(self):
        return _ffi.BLOCK_VALUE_GRADIENT if self.value else _ffi.BLOCK_GRADIENT

    # -- dense instantiation and indexing -----------------------------------------------------------
    def _dense(self, inner):
        """The dense block matrix of `inner`'s point sets: ONE covgram_block_matrix call into a column-major buffer."""
        B = self.block_size
        if self.d > BLOCK_MATRIX_MAX_D and self._kind() in (_ffi.BLOCK_GRADIENT, _ffi.BLOCK_VALUE_GRADIENT):
            # wider points than covgram_block_matrix keeps in registers: the MVM (its panel path) applied to an identity, as before
            sub = self if inner is self.inner else type(self)(self.g, inner.x, None if inner.y is inner.x else inner.y)
            return LazyOperator.to_dense(sub)
        nb, mb = inner.shape[0] * B, inner.shape[1] * B
        buf = torch.empty((mb, nb), dtype=self.dtype, device=self.device)   # column-major (n B) x (m B)
        if nb * mb:
            ctx = inner._px.ctx.bind_stream()
            _ffi.check(_ffi.lib().covgram_block_matrix(ctx, self._kind(), _ffi.kref(self._lower()), inner._px.handle, inner._py.handle,
                                                       _ffi._P(buf.data_ptr()), nb, _ffi.DEVICE))
        return buf.t()

    def to_dense(self):
        """Matrix(G) of the block Gramian (the reference's gramian(k, x, y, Val(false)), src/gramian.jl:125-130) on the device: one
        store-bound pass, every pair's jet evaluated once."""
        return self._dense(self.inner)

    def block(self, i, j):
        """The dense (|i| B) x (|j| B) sub-matrix of the blocks of the points i x j (ints, slices or index tensors OVER POINTS; two ints: one
        B x B block), evaluated from the sliced point sets, never from the full matrix."""
        x, y = self.inner.x, self.inner.y
        d = x.shape[1]
        xi = x[i % x.shape[0]].reshape(1, d) if isinstance(i, int) else x[i]
        yj = y[j % y.shape[0]].reshape(1, d) if isinstance(j, int) else y[j]
        return self._dense(Gramian(self.g.k, xi.reshape(-1, d), yj.reshape(-1, d)))

    def __getitem__(self, IJ):
        """G[I, J] over the flat (n B) x (m B) indices, ints and slices (getindex of the reference's BlockFactorization): the entries
        are taken from block() of the points that cover them."""
        I, J = IJ
        (p0, p1, ri), (q0, q1, rj) = flat_cover(I, self.shape[0], self.block_size), flat_cover(J, self.shape[1], self.block_size)
        sub = self.block(slice(p0, p1), slice(q0, q1))
        return sub[ri][..., rj]

    def _mvm(self, ctx, spec, px, py, ap, lda, yp, ldy, nrhs, alpha, beta):
        """The library call of mul_ on device-resident a and y."""
        return self._entry()(ctx, _ffi.kref(spec), px, py, ap, lda, yp, ldy, nrhs, alpha, beta, _ffi.DEVICE)

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        """Matrix right-hand sides (block solvers; src/gramian.jl:241-257 takes vectors of matrices) go down in ONE library call: the
        library shares the pair evaluations between two columns at a time where its kernel holds two accumulators."""
        spec = self._lower()
        a = _rhs(self, y, a)
        ctx = self.inner._px.ctx.bind_stream()
        return _staged(y, a, beta, lambda ap, lda, yp, ldy, nrhs: _ffi.check(self._mvm(
            ctx, spec, self.inner._px.handle, self.inner._py.handle, _ffi._P(ap), lda, _ffi._P(yp), ldy, nrhs, float(alpha), float(beta))))


class MixedBlockGramian(BlockGramian):
    """Gramian of GradientKernel(k) / ValueGradientKernel(k) for a Sum / Product / Power whose factors do not share one input trait
    (the reference's gradient algebra, src/gradient_algebra.jl:6-89, e.g. MaternP(2) + Dot()**2 + NeuralNetwork()): ONE fused pass of
    covgram_grad_mvm_mixed, every factor a function of (x·y, |x|², |y|²).  Matrix(G), block() and [] are the product applied to
    identity columns on the sliced point sets."""

    def _lower(self):
        return K.require_mixed_gradient_spec(self.g.k)

    def _dense(self, inner):
        sub = self if inner is self.inner else type(self)(self.g, inner.x, None if inner.y is inner.x else inner.y)
        return LazyOperator.to_dense(sub)

    def _mvm(self, ctx, spec, px, py, ap, lda, yp, ldy, nrhs, alpha, beta):
        return _ffi.lib().covgram_grad_mvm_mixed(ctx, C.byref(spec), px, py, ap, lda, yp, ldy, nrhs, alpha, beta, 1 if self.value else 0, _ffi.DEVICE)


class HessianGramian(BlockGramian):
    """Gramian of a HessianKernel: the lazy (n d²)×(m d²) BlockFactorization whose blocks are ∂⁴k / ∂x∂x∂y∂y (src/hessian.jl:33-41),
    applied in O(d²) per pair by covgram_hess_mvm.  Block vectors are point-major, entry i d² + a + b d."""

    def _block_size(self, d):
        return d * d

    def _lower(self):
        return K.require_hessian_spec(self.g.k, self.d)

    def _entry(self):
        return _ffi.lib().covgram_hess_mvm

    def _kind(self):
        return _ffi.BLOCK_HESSIAN


class ValueGradientHessianGramian(BlockGramian):
    """Gramian of a ValueGradientHessianKernel: the lazy n(1+d+d²)×m(1+d+d²) BlockFactorization whose blocks are the joint covariance of
    [f, ∂f, vec ∂²f] (src/hessian.jl:301-325), applied in O(d²) per pair by covgram_valgradhess_mvm.  Block vectors are point-major:
    entry i(1+d+d²) the value, then the d gradient components, then Hessian component (a, b) at 1 + d + a + b d."""

    def _block_size(self, d):
        return 1 + d + d * d

    def _lower(self):
        return K.require_vgh_spec(self.g.k, self.d)

    def _entry(self):
        return _ffi.lib().covgram_valgradhess_mvm

    def _kind(self):
        return _ffi.BLOCK_VALUE_GRADIENT_HESSIAN


class _ToeplitzBase(_OwnsHandle, LazyOperator):
    _destroy = "covgram_toeplitz_destroy"

    def __init__(self, vc: torch.Tensor, vr: Optional[torch.Tensor], circulant: bool):
        self.vc = vc.contiguous()
        self.vr = None if vr is None else vr.contiguous()
        self.circulant = circulant
        n = vc.shape[0]
        m = n if vr is None else vr.shape[0]
        self.shape = (n, m)
        self.dtype, self.device = vc.dtype, vc.device
        self._ctx = get_ctx(vc.device)
        self.handle = _ffi._P()
        _ffi.check(_ffi.lib().covgram_toeplitz_create(self._ctx.bind_stream(), C.byref(self.handle), _ffi._P(self.vc.data_ptr()),
                                                      _ffi._P(self.vr.data_ptr()) if self.vr is not None else None, n, m,
                                                      _dtype_code(self.dtype), _ffi.DEVICE, 1 if circulant else 0))

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        a = _rhs(self, y, a)
        if a.dim() != 1:                                       # covgram_toeplitz_mvm takes vectors
            return _by_columns(self, y, a, alpha, beta)
        self._ctx.bind_stream()
        return _staged(y, a, beta, lambda ap, lda, yp, ldy, nrhs: _ffi.check(_ffi.lib().covgram_toeplitz_mvm(
            self.handle, _ffi._P(ap), _ffi._P(yp), float(alpha), float(beta), _ffi.DEVICE)))

    def to_dense(self):
        n, m = self.shape
        i = torch.arange(n, device=self.device)[:, None]
        j = torch.arange(m, device=self.device)[None, :]
        if self.circulant:
            return self.vc[(i - j) % n]
        vr = self.vc if self.vr is None else self.vr
        return torch.where(i >= j, self.vc[(i - j).clamp(min=0)], vr[(j - i).clamp(min=0)])


class SymmetricToeplitz(_ToeplitzBase):
    def __init__(self, vc):
        super().__init__(vc, None, False)

    @property
    def T(self):
        return self


class Toeplitz(_ToeplitzBase):
    def __init__(self, vc, vr):
        super().__init__(vc, vr, False)

    @property
    def T(self):
        return Toeplitz(self.vr, self.vc)                       # first column and first row change places


class Circulant(_ToeplitzBase):
    def __init__(self, vc):
        super().__init__(vc, None, True)

    @property
    def T(self):
        return Circulant(torch.roll(self.vc.flip(0), 1))        # C[i, j] = vc[(i - j) mod n]: the transpose's first column is vc[-i mod n]


class SparseGramian(_OwnsHandle, LazyOperator):
    """sparse(G, δ) (src/sparse.jl:5-22): the entries of gramian(k, x, y) within the kernel's decay radius, as a CSR matrix that lives
    on the device (covgram_sparse_create); `mul!` is the library's CSR product (covgram_sparse_mvm).  The handle owns its arrays and
    keeps no reference to the Gramian's points."""

    _destroy = "covgram_sparse_destroy"

    def __init__(self, G: "Gramian", delta: float = 1e-6):
        self.delta = float(delta)
        self.shape, self.dtype, self.device = G.shape, G.dtype, G.device
        self._ctx = G._px.ctx
        self.handle = _ffi._P()
        _ffi.check(_ffi.lib().covgram_sparse_create(self._ctx.bind_stream(), C.byref(self.handle), _ffi.kref(G._spec()), G._px.handle,
                                                    G._py.handle, self.delta))
        n, m, nnz, dt, r = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_double(0)
        _ffi.check(_ffi.lib().covgram_sparse_info(self.handle, C.byref(n), C.byref(m), C.byref(nnz), C.byref(dt), C.byref(r)))
        self.nnz, self.radius = int(nnz.value), float(r.value)

    def csr(self):
        """(rowptr, colind, vals): int64 n + 1, int32 nnz (0-based, ascending within a row), nnz scalars — copies, as device tensors."""
        rowptr = torch.empty(self.shape[0] + 1, dtype=torch.int64, device=self.device)
        colind = torch.empty(self.nnz, dtype=torch.int32, device=self.device)
        vals = torch.empty(self.nnz, dtype=self.dtype, device=self.device)
        self._ctx.bind_stream()
        _ffi.check(_ffi.lib().covgram_sparse_export(self.handle, _ffi._P(rowptr.data_ptr()), _ffi._P(colind.data_ptr()),
                                                    _ffi._P(vals.data_ptr()), _ffi.DEVICE))
        return rowptr, colind, vals

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        a = _rhs(self, y, a)
        self._ctx.bind_stream()
        return _staged(y, a, beta, lambda ap, lda, yp, ldy, nrhs: _ffi.check(_ffi.lib().covgram_sparse_mvm(
            self.handle, _ffi._P(ap), lda, _ffi._P(yp), ldy, nrhs, float(alpha), float(beta), _ffi.DEVICE)))

    def to_dense(self):
        n, m = self.shape
        rowptr, colind, vals = self.csr()
        out = torch.zeros((n, m), dtype=self.dtype, device=self.device)
        if self.nnz:
            rows = torch.repeat_interleave(torch.arange(n, device=self.device), rowptr[1:] - rowptr[:-1])
            out[rows, colind.long()] = vals
        return out


def decay_radius(k, delta: float = 1e-6) -> float:
    """decay_radius(k, δ) of src/sparse.jl:24-38, with the two corrections described at kernels.decay_radius."""
    return K.decay_radius(k, delta)


def sparse(G, delta: float = 1e-6) -> SparseGramian:
    """SparseArrays.sparse(G::Gramian, δ = 1e-6): a plain scalar Gramian of a kernel that has a decay radius; block and structured
    Gramians and every other kernel raise UnsupportedKernel."""
    if type(G) is not Gramian:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"sparse: {type(G).__name__} is not a plain scalar Gramian (block and structured "
                                                        "Gramians have no sparse form)")
    # refusals name the kernel before anything touches the device; the value is discarded: the radius in use is the library's own
    # (covgram_sparse_create computes it again, S.radius reports it), and tests/test_sparse_host.py holds the two together to 1e-15
    K.decay_radius(G.k, delta)
    return SparseGramian(G, delta)


BARNES_HUT_THETA = 0.25       # src/barneshut.jl:3-4
BARNES_HUT_LEAFSIZE = 16
BARNES_HUT_MAX_D = 8          # covgram_bh_create: points in registers (include/covgram.h)


def _point_dim(x) -> int:
    """d of a point set as given by the caller, read without moving anything to a device."""
    if isinstance(x, StepRangeLen):
        return 1
    if isinstance(x, LazyGrid):
        return x.ndims()
    shape = tuple(x.shape) if isinstance(x, torch.Tensor) else np.shape(x)
    return int(shape[1]) if len(shape) >= 2 else 1


def require_barneshut_spec(k, d: Optional[int] = None, theta: float = BARNES_HUT_THETA, leafsize: int = BARNES_HUT_LEAFSIZE):
    """The covgram_kernel that covgram_bh_create runs for k, checked on the host before any device call: ONE isotropic profile under
    Lengthscale, Constant factors and Power.  Block (derivative) kernels, composites, dot-product kernels and d > 8 raise
    UnsupportedKernel naming what was refused; theta < 0 or leafsize < 1 raise DimensionMismatch (COVGRAM_EINVAL, a ValueError)."""
    name = type(k).__name__
    if isinstance(k, K.MultiKernel):
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"BarnesHutFactorization: {name} is a block (derivative) kernel; only scalar "
                                                        "isotropic kernels have a Barnes-Hut product")
    spec = K.require_device_spec(k)
    if not isinstance(spec, _ffi.covgram_kernel):
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"BarnesHutFactorization: {name} lowers to a composite of profiles; only single "
                                                        "isotropic profiles under Lengthscale, Constant and Power are supported")
    if spec.trait != _ffi.ISOTROPIC:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"BarnesHutFactorization: {name} is a dot-product kernel; the far field of a ball "
                                                        "tree needs an isotropic profile")
    if d is not None and d > BARNES_HUT_MAX_D:
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"BarnesHutFactorization: d = {d} exceeds the limit of {BARNES_HUT_MAX_D} dimensions "
                                                        "(a ball tree compresses nothing beyond)")
    if not float(theta) >= 0:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"BarnesHutFactorization: theta = {theta} is negative (0 = the exact product)")
    if int(leafsize) < 1:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"BarnesHutFactorization: leafsize = {leafsize} is smaller than 1")
    return spec


class BarnesHutFactorization(_OwnsHandle, LazyOperator):
    """BarnesHutFactorization(k, x, y = x, D = nothing; θ = 1/4, leafsize = 16) (src/barneshut.jl:8-39): a ball tree over y, built once on
    the device (covgram_bh_create), and the tree-based approximate product F w + D w (covgram_bh_mvm).  `BarnesHutFactorization(G)` takes
    k, x, y from a Gramian.  D is None, a number, or n values (n == m).

    Two products:
      - product="split" (the default): mul_ / @ is the SPLIT product BH(w⁺) − BH(w⁻), the default of the reference's barneshut!.  It is not
        exactly linear in w (the far-field points depend on the weights), which costs a Krylov recurrence iterations;
      - product="taylor": mul_ / @ is taylor_ (src/taylor.jl:7-57, covgram_bh_taylor_mvm), the first-order expansion of the far field in
        ONE pass for weights of any sign — the product the reference's mul! runs for signed weights.  mul_'s `split` is then not
        consulted.  use_com=True expands about the |w|-weighted centres of mass; for w ≥ 0 the first moment is then rounding-level and
        the product is the reference's unsplit single pass, so the reference's mul! is reproduced without inspecting the weights on the
        host.  use_com=False expands about the ball centres, which do not depend on w: the product is an exactly linear map, the
        variant a Krylov solver wants.  The operator is not exactly symmetric either way (targets and sources are treated differently).
    taylor_ / taylor / taylor_moments are available whatever `product` is.  `solve.cg(F, b)` and `solve.minres(F, b)` run on mul_;
    `F.solve(b)` is the reference's `\\` (minres!, src/barneshut.jl:64-72).  The expansion stops at first order, like the reference's."""

    _destroy = "covgram_bh_destroy"

    def __init__(self, k, x=None, y=None, D=None, theta: float = BARNES_HUT_THETA, leafsize: int = BARNES_HUT_LEAFSIZE,
                 product: str = "split", use_com: bool = True):
        if product not in ("split", "taylor"):
            raise ValueError(f"BarnesHutFactorization: product = {product!r} (\"split\" or \"taylor\")")
        self.product, self.use_com = product, bool(use_com)
        if isinstance(k, Gramian):
            if type(k) is not Gramian:
                raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"BarnesHutFactorization: {type(k).__name__} is not a plain scalar Gramian")
            G = k
            k, x, y = G.k, G.x, G.y
        else:
            G = None
            if isinstance(k, LazyOperator):
                raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, f"BarnesHutFactorization: {type(k).__name__} is not a plain scalar Gramian")
        spec = require_barneshut_spec(k, _point_dim(x), theta, leafsize)      # every refusal comes before the first device call
        self._G = G if G is not None else Gramian(k, x, y)
        G = self._G
        self.k, self.x, self.y = G.k, G.x, G.y
        self.shape, self.dtype, self.device = G.shape, G.dtype, G.device
        self.theta, self.leafsize = float(theta), int(leafsize)
        n, m = self.shape
        if D is None:
            self.D = None
        else:
            if n != m:
                raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: a diagonal on a {n} x {m} factorization")
            Dt = torch.as_tensor(D, dtype=self.dtype).reshape(-1).to(self.device).contiguous()
            if Dt.shape[0] not in (1, n):
                raise _ffi.DimensionMismatch(_ffi.EINVAL, f"DimensionMismatch: D has length {Dt.shape[0]}, expected 1 or {n}")
            self.D = Dt
        self._ctx = G._px.ctx
        self.handle = _ffi._P()
        _ffi.check(_ffi.lib().covgram_bh_create(self._ctx.bind_stream(), C.byref(self.handle), _ffi.kref(spec), G._px.handle, G._py.handle,
                                                self.theta, self.leafsize))
        nn = C.c_int64(0)
        _ffi.check(_ffi.lib().covgram_bh_info(self.handle, None, None, None, None, C.byref(nn), None, None))
        self.nnodes = int(nn.value)

    def __getitem__(self, ij):
        return self._G[ij]                                     # src/barneshut.jl:42: F[i, j] = k(x[i], y[j])

    def tree(self):
        """The export: {"indices": int32 m, "lo" / "hi" / "left" / "right": int32 per node (root = node 0, −1 at a leaf),
        "centers": nnodes × d, "radii": nnodes} — copies, as device tensors."""
        m, nn, d = self.shape[1], self.nnodes, self.x.shape[1]
        i32 = lambda count: torch.empty(count, dtype=torch.int32, device=self.device)
        out = {"indices": i32(m if nn else 0), "lo": i32(nn), "hi": i32(nn), "left": i32(nn), "right": i32(nn),
               "centers": torch.empty((nn, d), dtype=self.dtype, device=self.device), "radii": torch.empty(nn, dtype=self.dtype, device=self.device)}
        self._ctx.bind_stream()
        _ffi.check(_ffi.lib().covgram_bh_export(self.handle, *[_ffi._P(out[key].data_ptr()) for key in
                                                               ("indices", "lo", "hi", "left", "right", "centers", "radii")], _ffi.DEVICE))
        return out

    def moments(self, w):
        """(sums, com) of the weights w: per node Σ w_j and Σ|w_j| y_j / (Σ|w_j| + eps(T)) (src/barneshut.jl:157-163), as device tensors."""
        m, nn, d = self.shape[1], self.nnodes, self.x.shape[1]
        w = _vec_arg(w, m, self.dtype, self.device, "w").contiguous()
        sums = torch.empty(nn, dtype=self.dtype, device=self.device)
        com = torch.empty((nn, d), dtype=self.dtype, device=self.device)
        self._ctx.bind_stream()
        _ffi.check(_ffi.lib().covgram_bh_moments(self.handle, _ffi._P(w.data_ptr()), _ffi._P(sums.data_ptr()), _ffi._P(com.data_ptr()), _ffi.DEVICE))
        return sums, com

    def taylor_moments(self, w, use_com: bool = True):
        """(sums, centers, m1) of taylor! for the weights w, as device tensors: per node Σ w_j, the expansion centre (use_com: the
        |w|-weighted centre of mass; otherwise the ball centre) and the centred signed first moment Σ w_j y_j − sums · centre."""
        m, nn, d = self.shape[1], self.nnodes, self.x.shape[1]
        w = _vec_arg(w, m, self.dtype, self.device, "w").contiguous()
        sums = torch.empty(nn, dtype=self.dtype, device=self.device)
        cen = torch.empty((nn, d), dtype=self.dtype, device=self.device)
        m1 = torch.empty((nn, d), dtype=self.dtype, device=self.device)
        self._ctx.bind_stream()
        _ffi.check(_ffi.lib().covgram_bh_taylor_moments(self.handle, _ffi._P(w.data_ptr()), 1 if use_com else 0, _ffi._P(sums.data_ptr()),
                                                        _ffi._P(cen.data_ptr()), _ffi._P(m1.data_ptr()), _ffi.DEVICE))
        return sums, cen, m1

    def _mvm(self, y, a, alpha, beta, taylor, theta, flag):
        a = _rhs(self, y, a)
        if theta is not None and not float(theta) >= 0:
            raise _ffi.DimensionMismatch(_ffi.EINVAL, f"BarnesHutFactorization: theta = {theta} is negative (0 = the exact product)")
        if a.dim() == 2:                                       # covgram_bh_mvm / covgram_bh_taylor_mvm take vectors
            return _by_columns(self, y, a, alpha, beta, method="_mvm", taylor=taylor, theta=theta, flag=flag)
        self._ctx.bind_stream()
        dptr, dlen = (None, 0) if self.D is None else (_ffi._P(self.D.data_ptr()), self.D.shape[0])
        fn = _ffi.lib().covgram_bh_taylor_mvm if taylor else _ffi.lib().covgram_bh_mvm
        return _staged(y, a, beta, lambda ap, lda, yp, ldy, nrhs: _ffi.check(fn(
            self.handle, _ffi._P(ap), _ffi._P(yp), float(alpha), float(beta), -1.0 if theta is None else float(theta), 1 if flag else 0, dptr, dlen,
            _ffi.DEVICE)))

    def taylor_(self, y, w, alpha=1.0, beta=0.0, theta: Optional[float] = None, use_com: bool = True):
        """b ← α (T w) + β b + α D w with T the first-order Taylor product taylor!(b, F, w, α, β, θ; use_com) (src/taylor.jl:7-57).
        theta=None: the handle's θ; θ = 0 is the exact product.  A matrix right-hand side goes column by column."""
        return self._mvm(y, w, alpha, beta, True, theta, use_com)

    def taylor(self, w, **kw):
        """T w + D w as a new tensor (kw: theta, use_com)."""
        w = _vec_arg(w, self.shape[1], self.dtype, self.device, "w")
        y = torch.empty((self.shape[0],) + tuple(w.shape[1:]), dtype=self.dtype, device=self.device)
        return self.taylor_(y, w, 1.0, 0.0, **kw)

    def solve(self, b, **kw):
        """F \\ b (src/barneshut.jl:64-72): MINRES on mul_ (kw: the keywords of solve.minres)."""
        from .solve import minres
        return minres(self, b, **kw)[0]

    def mul_(self, y, a, alpha=1.0, beta=0.0, theta: Optional[float] = None, split: bool = True):
        """b ← α (F w) + β b + α D w.  theta=None: the handle's θ; θ = 0 is the exact product.  split=False: the single pass of
        barneshut!(…; split = false).  With product="taylor" this is taylor_ with the constructor's use_com, and `split` is not consulted."""
        if self.product == "taylor":
            return self._mvm(y, a, alpha, beta, True, theta, self.use_com)
        return self._mvm(y, a, alpha, beta, False, theta, split)

    def to_dense(self):
        """The matrix the factorization approximates, Matrix(G) + D."""
        out = self._G.to_dense().clone()
        if self.D is not None:
            out.diagonal().add_(self.D if self.D.shape[0] > 1 else self.D[0])
        return out


class KroneckerProduct(LazyOperator):
    """kronecker(F_1, ..., F_q) (KroneckerProducts 1.1.1): standard order, F_1 = slowest index.  Factors are
    lazy Gramians or dense matrices; lazy factors are instantiated once on the device (they are the small
    per-axis matrices, cf. README.md:205-210) and the MVM runs as mode products in libcovgram."""

    def __init__(self, *factors):
        self.factors = list(factors)
        rows = [f.shape[0] for f in self.factors]
        cols = [f.shape[1] for f in self.factors]
        self.shape = (int(np.prod(rows)), int(np.prod(cols)))
        f0 = self.factors[0]
        self.dtype = f0.dtype
        self.device = f0.device
        self._dense = None

    def _dense_factors(self):
        if self._dense is None:
            out = []
            for f in self.factors:
                D = f.to_dense() if isinstance(f, LazyOperator) else f
                out.append(D.to(self.dtype).t().contiguous())    # (cols, rows) row-major == column-major rows×cols
            self._dense = out
        return self._dense

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        a = _rhs(self, y, a)
        fs = self._dense_factors()
        q = len(fs)
        ptrs = (_ffi._P * q)(*[_ffi._P(f.data_ptr()) for f in fs])
        rows = (C.c_int64 * q)(*[f.shape[1] for f in fs])
        cols = (C.c_int64 * q)(*[f.shape[0] for f in fs])
        lds = (C.c_int64 * q)(*[f.shape[1] for f in fs])
        ctx = get_ctx(self.device).bind_stream()
        return _staged(y, a, beta, lambda ap, lda, yp, ldy, nrhs: _ffi.check(_ffi.lib().covgram_kron_mvm(
            ctx, ptrs, rows, cols, lds, q, _dtype_code(self.dtype), _ffi._P(ap), lda, _ffi._P(yp), ldy, nrhs, float(alpha), float(beta), _ffi.DEVICE)))

    def to_dense(self):
        out = None
        for f in self.factors:
            D = f.to_dense() if isinstance(f, LazyOperator) else f
            D = D.contiguous()
            out = D if out is None else torch.kron(out, D)
        return out


def kronecker(*factors):
    if len(factors) == 1 and isinstance(factors[0], SeparableGramian):
        return factors[0].kronecker()
    return KroneckerProduct(*factors)


class SeparableGramian(LazyOperator):
    """Gramian of a SeparableKernel: mul! = kronecker(G) = gramian(k.k, x, y) ⊗ B (src/separable.jl:33-42)."""

    def __init__(self, s: K.SeparableKernel, x, y=None):
        self.s = s
        self.inner = Gramian(s.k, x, y)
        self.dtype, self.device = self.inner.dtype, self.inner.device
        self.B = torch.as_tensor(s.B, dtype=self.dtype, device=self.device)
        n, m = self.inner.shape
        self.shape = (n * self.B.shape[0], m * self.B.shape[1])
        self._kron = None

    def kronecker(self):
        if self._kron is None:
            self._kron = KroneckerProduct(self.inner, self.B)
        return self._kron

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        return self.kronecker().mul_(y, a, alpha, beta)

    def to_dense(self):
        return self.kronecker().to_dense()


class LazyMatrixProduct(LazyOperator):
    """LazyMatrixProduct(U, V') — the low-rank Gramian of a FiniteBasis kernel (src/mercer.jl:61-70);
    mul! applies the factors right to left (src/lazy_linear_algebra.jl:78-85): y = α U (Vᵀ a) + β y."""

    def __init__(self, U: torch.Tensor, V: torch.Tensor):
        # U: (n, r), V: (m, r) in torch indexing; stored column-major for the library
        self.U, self.V = U, V
        self.shape = (U.shape[0], V.shape[0])
        self.dtype, self.device = U.dtype, U.device
        self._Ucm = U.t().contiguous()
        self._Vcm = self._Ucm if V is U else V.t().contiguous()

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        """A matrix right-hand side goes down in ONE call: from 8 columns on both products run on the matrix cores (csrc/lowrank.hip)."""
        a = _rhs(self, y, a)
        n, m = self.shape
        r = self.U.shape[1]
        ctx = get_ctx(self.device).bind_stream()
        return _staged(y, a, beta, lambda ap, lda, yp, ldy, nrhs: _ffi.check(_ffi.lib().covgram_lowrank_mvm(
            ctx, _ffi._P(self._Ucm.data_ptr()), n, _ffi._P(self._Vcm.data_ptr()), m, n, m, r, _dtype_code(self.dtype), _ffi._P(ap), lda, _ffi._P(yp), ldy,
            nrhs, float(alpha), float(beta), _ffi.DEVICE)))

    def to_dense(self):
        return self.U @ self.V.t()


def _by_columns(op, y, a, alpha, beta, method="mul_", **kw):
    """Matrix right-hand side for operators whose mul_ is written for vectors: one column at a time (kw: further keywords of op.mul_;
    method: another product of op with mul_'s leading arguments)."""
    product = getattr(op, method)
    for c in range(a.shape[1]):
        product(y[:, c], a[:, c], alpha, beta, **kw)           # views: the product stages what is not contiguous
    return y


class ScaledOperator(LazyOperator):
    """Diagonal(dx) · K · Diagonal(dy), lazy — gramian(::VerticalRescaling) (src/transformation.jl:165-171 builds exactly this
    LazyMatrixProduct(Dx, K, Dy)).  The two diagonal scalings are O(n) vector ops around K's own MVM."""

    def __init__(self, dx: torch.Tensor, K: LazyOperator, dy: torch.Tensor):
        self.dx, self.K, self.dy = dx, K, dy
        self.shape, self.dtype, self.device = K.shape, K.dtype, K.device

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        a = _vec_arg(a, self.shape[1], self.dtype, self.device, "a")
        sa = self.dy * a if a.dim() == 1 else self.dy[:, None] * a
        t = self.K @ sa
        t = self.dx * t if t.dim() == 1 else self.dx[:, None] * t
        return _axpby_(y, t, alpha, beta)

    def to_dense(self):
        return self.dx[:, None] * self.K.to_dense() * self.dy[None, :]


class LinearMapBlockGramian(LazyOperator):
    """Gradient Gramian of k(Ux, Uy): block (i, j) = Uᵀ B_ij(Ux, Uy) U (chain rule), applied as  b_i = Uᵀ Σ_j B_ij (U a_j):
    two small (d′ × d) maps around the device block MVM on the transformed points.  U: (d′, d) matrix or a length-d diagonal."""

    def __init__(self, U: torch.Tensor, inner: "BlockGramian", d: int):
        self.U, self.inner, self.d = U, inner, d
        n, m = inner.inner.shape
        self.shape = (n * d, m * d)
        self.dtype, self.device = inner.dtype, inner.device

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        if torch.is_tensor(a) and a.dim() == 2:
            return _by_columns(self, y, a, alpha, beta)
        n, m = self.inner.inner.shape
        A = _vec_arg(a, self.shape[1], self.dtype, self.device, "a").reshape(m, self.d)
        UA = (A * self.U if self.U.dim() == 1 else A @ self.U.t()).contiguous()
        t = (self.inner @ UA.reshape(-1)).reshape(n, -1)
        b = (t * self.U if self.U.dim() == 1 else t @ self.U).reshape(-1)
        return _axpby_(y, b, alpha, beta)


class CosineBlockGramian(LazyOperator):
    """Gradient Gramian of the Cosine kernel (src/gradient.jl:129-136): block (i, j) = −k₂ c cᵀ with k₂ = −4π² cos(2π c·(x_i − y_j)),
    i.e. (rank-2 scalar Gramian) ⊗ c cᵀ:  b_i = 4π² c Σ_j cos(u_i − v_j) (c·a_j)."""

    def __init__(self, c: torch.Tensor, scalar: "LazyMatrixProduct"):
        self.c, self.scalar = c, scalar
        d = c.shape[0]
        self.d = d
        self.shape = (scalar.shape[0] * d, scalar.shape[1] * d)
        self.dtype, self.device = scalar.dtype, scalar.device

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        if torch.is_tensor(a) and a.dim() == 2:
            return _by_columns(self, y, a, alpha, beta)
        n, m = self.scalar.shape
        A = _vec_arg(a, self.shape[1], self.dtype, self.device, "a").reshape(m, self.d)
        t = self.scalar @ (A @ self.c).contiguous()
        b = ((4 * math.pi ** 2) * t[:, None] * self.c[None, :]).reshape(-1)
        return _axpby_(y, b, alpha, beta)


class PointJacobianBlockGramian(LazyOperator):
    """Gradient Gramian of k(u(x), u(y)) for a pointwise warp u: block (i, j) = J_iᵀ B̂_ij J_j.  Here u is the NeuralNetwork
    normalisation x ↦ x̂ = [x, √σ] / ρ, ρ = sqrt(1 + |x|² + σ):  J a = [a; 0]/ρ − x̂ (x·a)/ρ²,  Jᵀ v = v[:d]/ρ − x (x̂·v)/ρ²."""

    def __init__(self, x: torch.Tensor, y: torch.Tensor, xh: torch.Tensor, yh: torch.Tensor, rx: torch.Tensor, ry: torch.Tensor,
                 inner: "BlockGramian"):
        self.x, self.y, self.xh, self.yh, self.rx, self.ry, self.inner = x, y, xh, yh, rx, ry, inner
        n, m, d = x.shape[0], y.shape[0], x.shape[1]
        self.d = d
        self.shape = (n * d, m * d)
        self.dtype, self.device = inner.dtype, inner.device

    def mul_(self, yv, a, alpha=1.0, beta=0.0):
        if torch.is_tensor(a) and a.dim() == 2:
            return _by_columns(self, yv, a, alpha, beta)
        n, m, d = self.x.shape[0], self.y.shape[0], self.d
        A = _vec_arg(a, self.shape[1], self.dtype, self.device, "a").reshape(m, d)
        ya = (self.y * A).sum(dim=1)
        JA = torch.cat([A, torch.zeros(m, 1, dtype=self.dtype, device=self.device)], dim=1) / self.ry[:, None] \
            - self.yh * (ya / self.ry ** 2)[:, None]
        V = (self.inner @ JA.reshape(-1).contiguous()).reshape(n, d + 1)
        xv = (self.xh * V).sum(dim=1)
        b = (V[:, :d] / self.rx[:, None] - self.x * (xv / self.rx ** 2)[:, None]).reshape(-1)
        return _axpby_(yv, b, alpha, beta)


class LazyMatrixSum(LazyOperator):
    """D + G kept lazy (src/gramian.jl:55-60, src/lazy_linear_algebra.jl:91-133): mul! accumulates the
    terms with β = 1 after the first."""

    def __init__(self, *args):
        self.args = []
        for a in args:
            self.args.extend(a.args if isinstance(a, LazyMatrixSum) else [a])
        lazy = [a for a in self.args if (hasattr(a, "mul_") and not torch.is_tensor(a))][0]
        self.shape, self.dtype, self.device = lazy.shape, lazy.dtype, lazy.device

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        a = _vec_arg(a, self.shape[1], self.dtype, self.device, "a")
        if _overlaps(y, a):           # in place (mul!(x, G + D, x)): every term after the first must still see the a the caller passed
            a = a.clone()
        first = True
        for A in self.args:
            b = beta if first else 1.0
            if (hasattr(A, "mul_") and not torch.is_tensor(A)):
                A.mul_(y, a, alpha, b)
            else:   # Diagonal given as a 1-D tensor, or a dense matrix
                A = torch.as_tensor(A, dtype=self.dtype, device=self.device)
                if A.dim() == 1 and b != 0:                   # the noise term of G + sigma^2 I inside a Krylov loop: ONE launch
                    if b != 1:
                        y.mul_(b)
                    y.addcmul_(A if a.dim() == 1 else A[:, None], a, value=alpha)
                    first = False
                    continue
                t = (A * a if a.dim() == 1 else A[:, None] * a) if A.dim() == 1 else A @ a
                _axpby_(y, t, alpha, b)
            first = False
        return y


class Fill(LazyOperator):
    """gramian(k::Constant, x, y) = Fill(k.c, n, m) (src/stationary.jl:34)."""

    def __init__(self, c, n, m, dtype, device):
        self.c, self.shape, self.dtype, self.device = float(c), (n, m), dtype, device

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        a = _vec_arg(a, self.shape[1], self.dtype, self.device, "a")
        s = a.sum(dim=0, keepdim=True) * (alpha * self.c)
        if beta == 0:
            y.copy_(s.expand_as(y) if a.dim() > 1 else s.expand(y.shape[0]))
        else:
            y.mul_(beta).add_(s.expand_as(y) if a.dim() > 1 else s.expand(y.shape[0]))
        return y

    def to_dense(self):
        return torch.full(self.shape, self.c, dtype=self.dtype, device=self.device)


# ----------------------------------------------------------------------------------------------
# the smart pseudo-constructor (src/gramian.jl:139-189 and the specialisations listed in SURVEY §3.1)
# ----------------------------------------------------------------------------------------------
def _first_column(k, x: torch.Tensor, y0: torch.Tensor) -> torch.Tensor:
    """k.(x, y0) for n points x against ONE point y0 — n kernel evaluations on the device."""
    return _plain_gramian(k, x, y0.reshape(1, -1)).to_dense()[:, 0].contiguous()


def _plain_gramian(k, x, y=None):
    """The lazy Gramian without structure: the fused spectral-mixture operator exactly when k has no covgram_kernel encoding but is a
    mixture the covgram_sm kernels take; MixedGramian exactly when it has neither encoding and kernels.mixed_spec lowers it; otherwise
    Gramian (whose products raise UnsupportedKernel for a kernel without a device path)."""
    if isinstance(k, K.AbstractKernel) and K.device_spec(k) is None:
        spec = K.spectral_mixture_spec(k, _point_dim(x))
        if spec is not None:
            return SpectralMixtureGramian(k, x, y, spec)
        spec = K.mixed_spec(k)
        if spec is not None:
            return MixedGramian(k, x, y, spec)
    return Gramian(k, x, y)


def _transform_points(k, p: torch.Tensor) -> torch.Tensor:
    """u(x) for every point (one O(n d d′) pass on the device): ScaledInputKernel / ARD, Warped, Periodic."""
    if isinstance(k, K.ScaledInputKernel):
        U = torch.as_tensor(k.U, dtype=p.dtype, device=p.device)
        return (p * U if U.dim() == 1 else p @ U.t()).contiguous()
    if isinstance(k, K.Warped):
        if callable(k.u):
            return torch.as_tensor(k.u(p), dtype=p.dtype, device=p.device).reshape(p.shape[0], -1).contiguous()
        U = torch.as_tensor(k.u, dtype=p.dtype, device=p.device)
        return (p @ U.t()).contiguous()
    if isinstance(k, K.Periodic):
        if p.shape[1] != 1:
            raise _ffi.DimensionMismatch(_ffi.EINVAL, "Periodic: input has to be one-dimensional (src/transformation.jl:53)")
        ang = (2 * math.pi) * p[:, 0]
        return torch.stack([torch.cos(ang), torch.sin(ang)], dim=1).contiguous()
    raise TypeError(type(k))


def _cosine_lowrank(k, px: torch.Tensor, py: torch.Tensor, same: bool):
    c = torch.as_tensor(k.c, dtype=px.dtype, device=px.device)
    if c.numel() == 1 and px.shape[1] != 1:
        c = c.expand(px.shape[1])
    if c.shape[0] != px.shape[1]:
        raise _ffi.DimensionMismatch(_ffi.EINVAL, f"Cosine: length(c) = {c.shape[0]} ≠ d = {px.shape[1]}")
    u = (2 * math.pi) * (px @ c)
    U = torch.stack([torch.cos(u), torch.sin(u)], dim=1)
    if same:
        return LazyMatrixProduct(U, U)
    v = (2 * math.pi) * (py @ c)
    return LazyMatrixProduct(U, torch.stack([torch.cos(v), torch.sin(v)], dim=1))


def _point_pair(x, y, same: bool):
    """(px, py): the two point sets as device tensors, py on px's device in px's dtype — and px itself when `same`."""
    px = _as_points(x)
    return px, (px if same else _as_points(y, device=px.device, dtype=px.dtype))


def gramian(k, x=None, y=None, trait: Optional[K.InputTrait] = None):
    """gramian(k, x[, y][, trait]) — picks the representation exactly as the reference does."""
    if x is None:
        raise TypeError("gramian(k, x[, y])")
    if not isinstance(k, (K.AbstractKernel,)) and not callable(k):   # gramian(x, y) = Gramian(Dot(), x, y)  (:150-151)
        return Gramian(K.Dot(), k, x)
    periodic = isinstance(y, K.PeriodicInput) or isinstance(trait, K.PeriodicInput)
    if isinstance(y, K.InputTrait):
        trait, y = y, None
    same = y is None or y is x

    if isinstance(k, K.Constant):                               # src/stationary.jl:34
        px, py = _point_pair(x, y, same)
        return Fill(k.c, px.shape[0], py.shape[0], px.dtype, px.device)

    if isinstance(k, K.FiniteBasis):                            # src/mercer.jl:61-70
        px, py = _point_pair(x, y, same)
        r = len(k.basis)
        if px.shape[0] > r and py.shape[0] > r:
            def basis(p):
                arg = p[:, 0] if p.shape[1] == 1 else p
                return torch.stack([torch.as_tensor(b(arg), dtype=p.dtype, device=p.device).reshape(-1) for b in k.basis], dim=1)
            U = basis(px)
            V = U if same else basis(py)
            return LazyMatrixProduct(U, V)
        raise _ffi.UnsupportedKernel(_ffi.EUNSUPPORTED, "FiniteBasis with fewer points than basis functions is a GenericInput Gramian (src/mercer.jl:68)")

    # ---- input / output transformations: the points are transformed ONCE, the hot path runs on the result -------------------
    if isinstance(k, K.VerticalRescaling):                     # src/transformation.jl:165-171
        px, py = _point_pair(x, y, same)
        fx = torch.as_tensor(k.f(px), dtype=px.dtype, device=px.device).reshape(-1)
        fy = fx if same else torch.as_tensor(k.f(py), dtype=px.dtype, device=px.device).reshape(-1)
        return ScaledOperator(fx, gramian(k.k, px, None if same else py), fy)
    if isinstance(k, (K.ScaledInputKernel, K.Warped, K.Periodic)):   # src/transformation.jl:82-90, 114-118, 54-65
        px, py = _point_pair(x, y, same)
        tx = _transform_points(k, px)
        g = gramian(k.k, tx, None if same else _transform_points(k, py))
        if isinstance(k, K.ScaledInputKernel) and type(g) is Gramian:
            g.scaled_input = k                                  # bilinear_gradient's chain rule to the entries of U / l
        return g
    if isinstance(k, K.NeuralNetwork) or (isinstance(k, K.GradientKernel) and isinstance(k.k, K.NeuralNetwork)):
        nn = k if isinstance(k, K.NeuralNetwork) else k.k          # src/mercer.jl:82-85 on normalised augmented inputs
        px, py = _point_pair(x, y, same)
        def warp(p):
            rho = torch.sqrt(1 + (p * p).sum(dim=1) + nn.sigma)
            z = torch.cat([p, torch.full((p.shape[0], 1), math.sqrt(nn.sigma), dtype=p.dtype, device=p.device)], dim=1)
            return (z / rho[:, None]).contiguous(), rho
        xh, rx = warp(px)
        yh, ry = (xh, rx) if same else warp(py)
        if isinstance(k, K.NeuralNetwork):
            return Gramian(K.AsinDot(), xh, None if same else yh)
        return PointJacobianBlockGramian(px, py, xh, yh, rx, ry, BlockGramian(K.GradientKernel(K.AsinDot()), xh, None if same else yh))
    if isinstance(k, K.CosineKernel):                           # rank 2: cos(u_i − v_j) = cos u_i cos v_j + sin u_i sin v_j
        px, py = _point_pair(x, y, same)
        return _cosine_lowrank(k, px, py, same)
    if isinstance(k, K.GradientKernel) and isinstance(k.k, K.ScaledInputKernel):
        px, py = _point_pair(x, y, same)
        U = torch.as_tensor(k.k.U, dtype=px.dtype, device=px.device)
        tx = _transform_points(k.k, px)
        inner = BlockGramian(K.GradientKernel(k.k.k), tx, None if same else _transform_points(k.k, py))
        return LinearMapBlockGramian(U, inner, px.shape[1])
    if isinstance(k, K.GradientKernel) and isinstance(k.k, K.CosineKernel):
        px, py = _point_pair(x, y, same)
        return CosineBlockGramian(torch.as_tensor(k.k.c, dtype=px.dtype, device=px.device), _cosine_lowrank(k.k, px, py, same))

    if isinstance(k, (K.GradientKernel, K.ValueGradientKernel)):   # src/gramian.jl:120-123
        if isinstance(k.k, K.AbstractKernel) and K.device_spec(k.k) is None and K.mixed_gradient_spec(k.k) is not None:
            return MixedBlockGramian(k, x, None if same else y)     # factors of different traits: src/gradient_algebra.jl
        return BlockGramian(k, x, None if same else y)
    if isinstance(k, K.HessianKernel):
        return HessianGramian(k, x, None if same else y)
    if isinstance(k, K.ValueGradientHessianKernel):
        return ValueGradientHessianGramian(k, x, None if same else y)
    if isinstance(k, K.SeparableKernel):
        return SeparableGramian(k, x, None if same else y)

    if isinstance(k, K.SeparableProduct) and isinstance(x, LazyGrid):   # src/algebra.jl:91-95
        gy = x if same else y
        if not isinstance(gy, LazyGrid) or len(gy.args) != len(x.args):
            raise _ffi.DimensionMismatch(_ffi.EINVAL, f"length(X.args) = {len(x.args)} ≠ length(Y.args)")
        if len(k.args) != len(x.args):
            raise _ffi.DimensionMismatch(_ffi.EINVAL, f"SeparableProduct needs d = {len(x.args)} kernels but has r = {len(k.args)}")
        return KroneckerProduct(*[gramian(ki, xi, None if yi is xi else yi) for ki, xi, yi in zip(k.args, x.args, gy.args)])

    if isinstance(x, StepRangeLen) and (same or isinstance(y, StepRangeLen)):   # src/gramian.jl:167-189
        tr = trait if trait is not None else K.input_trait(k)
        dev = get_ctx().device
        if periodic and isinstance(k, K.StationaryKernel):      # :186-189
            xt = _as_points(x, dev)
            return Circulant(_first_column(k, xt, xt[0]))
        if isinstance(tr, (K.IsotropicInput, K.StationaryInput)) and (K.device_spec(k) is not None or K.spectral_mixture_spec(k, 1) is not None):
            xt = _as_points(x, dev)
            if same:
                return SymmetricToeplitz(_first_column(k, xt, xt[0]))          # k.(x[1], x)
            if x.step == y.step and len(x) >= 1:
                yt = _as_points(y, dev, xt.dtype)
                vc = _first_column(k, xt, yt[0])                                  # k.(x, y[1])
                vr = _first_column(k, yt, xt[0])                                  # k.(x[1], y)
                return Toeplitz(vc, vr)
        return _plain_gramian(k, x, None if same else y)        # different step / GenericInput: plain Gramian

    return _plain_gramian(k, x, None if same else y)
