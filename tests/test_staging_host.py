"""The one staging path of the Python operators (covgram/gramian.py: _rhs, _staged, _OwnsHandle) on CPU tensors, no library call.

_staged hands a and y of y <- alpha M a + beta y to a C entry as column-major memory.  Here the C entry is a fake that views the two raw
pointers as (nrhs, ld) arrays, computes alpha M a + beta y column by column for a fixed random M (a is read in full before y is written:
the C ABI accepts any overlap of a and y) and logs its arguments.  Every combination of shape, right-hand-side form, (alpha, beta) and
memory layout of a and of y is compared with numpy, and the log says which memory the library was given."""
import ctypes as C
import itertools
import sys

import numpy as np
import pytest
import torch

SHAPES = [(5, 4), (1, 1), (7, 7), (3, 0)]
RHS = [None, 1, 3]                                   # a vector, or p columns
COEF = [(1.0, 0.0), (0.7, -1.3)]
LAYOUTS = ["c", "colmajor", "strided"]


@pytest.fixture(scope="module")
def gm(cg):
    return sys.modules["covgram.gramian"]


def laid_out(values, layout):
    """A float64 CPU tensor with `values` in the given memory layout."""
    t = torch.from_numpy(np.array(values, dtype=np.float64))
    if layout == "c":
        return t.contiguous()
    if layout == "colmajor":
        return t.t().contiguous().t() if t.dim() == 2 else t.contiguous()
    big = torch.full(tuple(2 * s + 1 for s in t.shape), -7.0, dtype=torch.float64)    # every second element of a larger tensor
    view = big[tuple(slice(0, 2 * s, 2) for s in t.shape)]
    view.copy_(t)
    return view


def is_column_major(t):
    """Whether t's own memory is what the C ABI reads: a contiguous vector, or rows x p column-major with leading dimension max(rows, 1)
    (the stride of an axis of length 1 addresses nothing)."""
    if t.dim() == 1:
        return t.shape[0] <= 1 or t.stride(0) == 1
    rows, p = t.shape
    return (rows <= 1 or t.stride(0) == 1) and (p <= 1 or t.stride(1) == max(rows, 1))


class FakeEntry:
    def __init__(self, M, alpha, beta):
        self.M, self.alpha, self.beta, self.log = M, alpha, beta, []

    def __call__(self, a_ptr, lda, y_ptr, ldy, nrhs):
        n, m = self.M.shape

        def view(ptr, ld, rows):
            if rows == 0:
                return np.zeros((nrhs, 0))
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(nrhs, ld))[:, :rows]
        A = view(a_ptr, lda, m).copy()                       # the library reads a from a private copy when it overlaps y
        Y = view(y_ptr, ldy, n)
        self.log.append(dict(a_ptr=a_ptr, lda=lda, y_ptr=y_ptr, ldy=ldy, nrhs=nrhs, a_seen=A.copy()))
        for c in range(nrhs):
            Y[c] = self.alpha * (self.M @ A[c]) + (self.beta * Y[c] if self.beta != 0 else 0.0)


def reference(M, a, y, alpha, beta):
    return alpha * (M @ a) + (beta * y if beta != 0 else 0.0)


@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("p", RHS)
@pytest.mark.parametrize("alpha,beta", COEF)
def test_staged_layouts(gm, n, m, p, alpha, beta):
    rng = np.random.default_rng(1000 * n + 10 * m + (p or 0))
    M = rng.standard_normal((n, m))
    a0 = rng.standard_normal((m,) if p is None else (m, p))
    y0 = rng.standard_normal((n,) if p is None else (n, p)) if beta != 0 else np.full((n,) if p is None else (n, p), np.nan)
    ref = reference(M, a0, y0, alpha, beta)
    for la, ly in itertools.product(LAYOUTS, LAYOUTS):
        a, y = laid_out(a0, la), laid_out(y0, ly)
        entry = FakeEntry(M, alpha, beta)
        out = gm._staged(y, a, beta, entry)
        what = f"a {la}, y {ly}"
        assert out is y, what
        got = y.numpy()
        assert np.isfinite(got).all(), what
        assert np.abs(got - ref).max(initial=0.0) <= 1e-13 * max(1.0, np.abs(ref).max(initial=0.0)), what
        assert torch.equal(a, torch.from_numpy(a0)), f"{what}: a was written"
        (call,) = entry.log
        assert call["nrhs"] == (1 if p is None else p) and call["lda"] == max(m, 1) and call["ldy"] == max(n, 1), what
        assert (call["y_ptr"] == y.data_ptr()) == is_column_major(y), f"{what}: direct write {call['y_ptr'] == y.data_ptr()}"
        if is_column_major(a) and a.numel():
            assert call["a_ptr"] == a.data_ptr(), f"{what}: a was copied though it is column-major"


@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_no_columns_is_a_no_op(gm, n, m, layout):
    big = torch.full((2 * n + 1, 3), 3.5, dtype=torch.float64)
    y = {"c": big[:n, :0], "colmajor": big.t()[:0, :n].t(), "strided": big[0:2 * n:2, :0]}[layout]
    before = big.clone()

    def entry(*args):
        raise AssertionError("the C entry was called for a right-hand side without columns")
    assert gm._staged(y, torch.zeros((m, 0), dtype=torch.float64), 0.0, entry) is y
    assert gm._staged(y, torch.zeros((m, 0), dtype=torch.float64), -1.3, entry) is y
    assert big.numpy().tobytes() == before.numpy().tobytes()


@pytest.mark.parametrize("p", RHS)
@pytest.mark.parametrize("alpha,beta", COEF)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_y_aliasing_a(gm, p, alpha, beta, layout):
    """mul!(x, G, x): the C entry still sees the caller's a — in place for the layouts the library takes as they are (its contract: any
    overlap), and because a is staged before y is written for the others."""
    n = 6
    rng = np.random.default_rng(77 + (p or 0))
    M = rng.standard_normal((n, n))
    a0 = rng.standard_normal((n,) if p is None else (n, p))
    x = laid_out(a0, layout)
    entry = FakeEntry(M, alpha, beta)
    assert gm._staged(x, x, beta, entry) is x
    (call,) = entry.log
    seen = call["a_seen"][0] if p is None else call["a_seen"].T
    assert np.array_equal(seen, a0)
    ref = alpha * (M @ a0) + beta * a0
    assert np.abs(x.numpy() - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
    assert (call["y_ptr"] == x.data_ptr()) == is_column_major(x)


class _Op:
    shape, dtype, device = (5, 4), torch.float64, torch.device("cpu")


def test_rhs_checks(cg, gm):
    op = _Op()
    a = torch.zeros(4, dtype=torch.float64)
    assert gm._rhs(op, torch.zeros(5, dtype=torch.float64), a) is a
    A = gm._rhs(op, torch.zeros((5, 3), dtype=torch.float64), np.zeros((4, 3), dtype=np.float32))     # converted like every right-hand side
    assert A.dtype == torch.float64 and tuple(A.shape) == (4, 3)
    with pytest.raises(cg.DimensionMismatch):                                                          # a of the wrong length
        gm._rhs(op, torch.zeros(5, dtype=torch.float64), torch.zeros(5, dtype=torch.float64))
    with pytest.raises(cg.DimensionMismatch) as raised:                                                # y of the wrong length
        gm._rhs(op, torch.zeros(4, dtype=torch.float64), a)
    assert raised.value.status == cg._ffi.EINVAL and isinstance(raised.value, ValueError)
    with pytest.raises(cg.DimensionMismatch):                                                          # y of the wrong dtype
        gm._rhs(op, torch.zeros(5, dtype=torch.float32), a)
    with pytest.raises(cg.DimensionMismatch):                                                          # column counts differ
        gm._rhs(op, torch.zeros((5, 2), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(cg.DimensionMismatch):                                                          # a matrix into a vector
        gm._rhs(op, torch.zeros(5, dtype=torch.float64), torch.zeros((4, 1), dtype=torch.float64))


def test_handle_owner_destroys_once(cg, gm, monkeypatch):
    calls = []

    class Lib:
        def fake_destroy(self, h):
            calls.append(h.value)

        def failing_destroy(self, h):
            calls.append(h.value)
            raise OSError("library already unloaded")
    monkeypatch.setattr(cg._ffi, "lib", lambda: Lib())

    class Owner(gm._OwnsHandle):
        _destroy = "fake_destroy"

        def __init__(self, value):
            self.handle = C.c_void_p(value)

    o = Owner(41)
    assert type(o.handle) is C.c_void_p
    o.__del__()
    assert calls == [41] and o.handle is None
    o.__del__()
    del o
    assert calls == [41]

    Owner(None).__del__()                                # a NULL handle (creation failed) is not destroyed
    half_made = object.__new__(Owner)                    # __init__ raised before the handle existed
    half_made.__del__()
    assert calls == [41]

    class Failing(Owner):
        _destroy = "failing_destroy"
    f = Failing(43)
    f.__del__()                                          # swallowed: interpreter shutdown
    f.__del__()
    assert calls == [41, 43] and f.handle is None

    class Slot(gm._OwnsHandle):                          # the point sets keep theirs behind a property
        _destroy, _slot = "fake_destroy", "_h"
    s = Slot()
    s._h = C.c_void_p(47)
    s._release()
    s._release()
    assert calls == [41, 43, 47] and s._h is None
