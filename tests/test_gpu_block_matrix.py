"""covgram_block_matrix — the dense (n B) x (m B) matrix of the four block Gramians — entry by entry through the raw C ABI, and the
Python surface on top of it (BlockGramian.to_dense / block / __getitem__, cholesky).

Error measure (that of the row-wise MVM tests, tests/test_gpu_hessian.py, tests/test_gpu_grad_rowwise.py): column c of the matrix is the
MVM of the unit vector e_c, so every entry obeys  |M - ref| / absref <= TOL max(1, L_ij / 10),  TOL = 1e-12 (fp64) / 1e-5 (fp32), absref
the same entry with every term in absolute value (oracle.valgrad_absmul / hess_mul(absolute=True) / vgh_mul(absolute=True) on e_c),
L_ij = -ln(k(x_i, y_j) / k(0)) (dot product: |x_i . y_j|); an entry whose absref is 0 must be exactly 0.  No expanded-form allowance: the
kernel takes direct differences.  References: oracle.valgrad_matrix (its gradient part is oracle.grad_matrix), hessian_ref.hess_matrix,
vgh_ref.vgh_matrix, column by column, on the data as rounded to the dtype (the clouds are fp32 numbers in both precisions, so one
reference serves both).  The route key last_block_matrix_path = (kind + 1) + 10 VR is asserted before any number is looked at; out is
pre-filled with NaN with guards in front and behind, padding rows n B <= I < ldo stay NaN, every entry < n B is finite."""
import numpy as np
import pytest
import torch

import covgram_oracle as o
import hessian_ref as R
import kernel_cases
import vgh_ref as V
from test_gpu_hessian import PROFILES, make_kernel
from test_gpu_matrix import GUARD, TDT, VRS, Dev

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TOL = {F32: 1e-5, F64: 1e-12}
GRAD, VALGRAD, HESS, VGH = 0, 1, 2, 3
KIND_NAME = {GRAD: "gradient", VALGRAD: "value-gradient", HESS: "hessian", VGH: "value-gradient-hessian"}
DIMS = [1, 2, 3, 5, 8, 16, 32]


def bsize(kind, d):
    return {GRAD: d, VALGRAD: d + 1, HESS: d * d, VGH: 1 + d + d * d}[kind]


def expected_key(kind, dt, d, ld, aligned=True):
    vr = VRS[dt] if (bsize(kind, d) % VRS[dt] == 0 and ld % VRS[dt] == 0 and aligned) else 1
    return (kind + 1) + 10 * vr


class BDev(Dev):
    def block_matrix(self, kind, spec, hx, hy, nb, mb, dt, ld=None, offset=0, loc_host=False):
        """(route key, M as an nb x mb array) with the sentinel checks of the module docstring."""
        ld = nb if ld is None else ld
        buf = torch.full((GUARD + offset + ld * mb + GUARD,), float("nan"), dtype=TDT[dt], device="cpu" if loc_host else "cuda")
        start = GUARD + offset
        ptr = buf.data_ptr() + start * buf.element_size()
        if not loc_host:
            assert buf.data_ptr() % 16 == 0
        self.f.check(self.lib.covgram_block_matrix(self.ctx.bind_stream(), kind, self.f.kref(spec), hx, hy, self.f._P(ptr), ld,
                                                   self.f.HOST if loc_host else self.f.DEVICE))
        key = self.cg.get_info("last_block_matrix_path")
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert np.isnan(h[:start]).all() and np.isnan(h[start + ld * mb:]).all(), "written outside the ld x (m B) output"
        T = h[start:start + ld * mb].reshape(mb, ld)
        assert np.isnan(T[:, nb:]).all(), f"padding rows n B <= I < ld written (nb={nb}, ld={ld}, key={key})"
        assert np.isfinite(T[:, :nb]).all(), "non-finite entry"
        return key, T[:, :nb].T


@pytest.fixture()
def dev(cg):
    d = BDev(cg)
    yield d
    d.close()


def cloud(rng, iso, n, m, d, lscale, same, far=True):
    """fp32-representable clouds (exact in both dtypes); isotropic: one row of x eight lengthscales out (tests/test_gpu_hessian.clouds)."""
    if iso:
        X = rng.standard_normal((n, d)).astype(F32)
        Y = X if same else (0.9 * rng.standard_normal((m, d)) + 0.1).astype(F32)
        if far and not same:
            v = rng.standard_normal(d); v /= np.linalg.norm(v)
            X[int(rng.integers(n))] = (Y.mean(axis=0) + (np.abs(Y - Y.mean(axis=0)).max() + 8.0 * lscale) * v).astype(F32)
        return X, Y
    s = 0.6 / np.sqrt(d)
    X = (s * rng.standard_normal((n, d)) + 0.05).astype(F32)
    Y = X if same else (s * rng.standard_normal((m, d))).astype(F32)
    return X, Y


def column_subset(kind, d, m, rng):
    """All columns up to d = 8; beyond: at least 64 seeded ones with the first and last column of the first and last block column."""
    B = bsize(kind, d); mb = m * B
    if d <= 8 or mb <= 64:
        return np.arange(mb)
    cols = {0, B - 1, (m - 1) * B, mb - 1}
    cols.update(int(c) for c in rng.choice(mb, size=64, replace=False))
    return np.array(sorted(cols))


def pair_L(iso, kfun, X, Y):
    if iso:
        with np.errstate(divide="ignore"):
            return np.maximum(0.0, -np.log(np.abs(kfun(X, Y)) / abs(float(kfun(X[:1], X[:1])[0, 0]))))
    return np.abs(X @ Y.T)


_REFS = {}


def grad_refs(name, ko, d, same, X, Y, cols):
    """(ref, absref, L) of the VALUE-GRADIENT matrix on `cols`; the gradient matrix is the part without the value rows / columns."""
    key = ("g", name, d, same)
    if key not in _REFS:
        X64, Y64 = X.astype(F64), Y.astype(F64)
        m, b = len(Y), d + 1
        ref = o.valgrad_matrix(ko, X64, Y64)[:, cols]
        absref = np.empty_like(ref)
        for t, c in enumerate(cols):
            e = np.zeros(m * b); e[c] = 1.0
            absref[:, t] = o.valgrad_absmul(ko, X64, Y64, e)
        L = pair_L(ko.trait == o.ISOTROPIC, lambda A, Bm: o.matrix(ko, A, Bm), X64, Y64)
        _REFS[key] = (ref, absref, L)
    return _REFS[key]


def hess_refs(kind, kern, d, same, X, Y, cols):
    key = ("h", kind, kern, d, same)
    if key not in _REFS:
        X64, Y64 = X.astype(F64), Y.astype(F64)
        mul = R.hess_mul if kind == HESS else V.vgh_mul
        mb = len(Y) * bsize(kind, d)
        ref = np.empty((len(X) * bsize(kind, d), len(cols))); absref = np.empty_like(ref)
        for t, c in enumerate(cols):
            e = np.zeros(mb); e[c] = 1.0
            ref[:, t] = mul(kern, X64, Y64, e)
            absref[:, t] = mul(kern, X64, Y64, e, absolute=True)
        iso = kern[0] in R.ISO
        kf = (lambda A, Bm: R.profile(kern, ((A[:, None, :] - Bm[None, :, :]) ** 2).sum(-1) / kern[2] ** 2)) if iso else None
        _REFS[key] = (ref, absref, pair_L(iso, kf, X64, Y64))
    return _REFS[key]


def worst(got, ref, absref, L, B, cols, dt):
    """max err / bound over the entries, its position and figures."""
    bound = TOL[dt] * np.maximum(1.0, np.kron(L, np.ones((B, B)))[:, cols] / 10.0)
    diff = np.abs(got.astype(F64) - ref)
    # The one allowance beside the issue's measure, from the number format alone.  The case that needs it: the far row at d >= 5 in fp32 —
    # EQ^2 at d = 16 has k = exp(-121) = 3e-53 there, Lengthscale(EQ, 0.7) at d = 32 likewise: the true entries lie below fp32's smallest
    # denormal (1.4e-45), the device writes 0 and e = 1 whatever the arithmetic.  A jet value below finfo.tiny (1.2e-38) is flushed, i.e.
    # off by up to finfo.tiny, and is multiplied by at most 4 gamma^2 r_a r_c (< 1e4 on these clouds, r <= 8 lengthscales + the cloud):
    # 1e-34 in fp32, 2e-304 in fp64, taken off the difference as tests/test_gpu_matrix.py takes off its "+ tiny".  No entry above 1e-29
    # is eased by a part in 1e5 of the bound.
    diff = np.maximum(diff - 1e4 * float(np.finfo(dt).tiny), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(absref > 0, diff / absref, np.where(np.abs(got) > 0, np.inf, 0.0))   # an entry whose absref is 0 must be exactly 0
    w = e / bound
    i, j = np.unravel_index(int(np.argmax(w)), w.shape)
    return float(w[i, j]), int(i), int(cols[j]), float(e[i, j])


def shapes(kind, d):
    if kind in (GRAD, VALGRAD):
        return (37, 4) if d <= 8 else (5, 4)          # one workgroup in x up to d = 5; two at d = 8 on the one-row route (n B = 296, 333)
    return (5, 3) if d <= 8 else (3, 2)               # d = 32: 3072 x 2048 (x 1057^2 / 1024^2 for the joint kind), well under 256 MiB


# ---- 1. every kind x dtype x d x kernel, rectangular with a far row and square on the same points ------------------------------------------
@pytest.mark.parametrize("dt", [F64, F32])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("kind", [GRAD, VALGRAD])
def test_gradient_kinds_entrywise(cg, dev, kind, d, dt):
    fails = []
    b = d + 1
    for name, k, ko in kernel_cases.valgrad_cases(cg):
        spec = cg.device_spec(k)
        iso = ko.trait == o.ISOTROPIC
        for same in (False, True):
            n, m = shapes(kind, d)
            m = n if same else m
            rng = np.random.default_rng(7 * d + 1000 * same + len(name))
            X, Y = cloud(rng, iso, n, m, d, getattr(ko, "lengthscale", 1.0), same)
            cols_vg = np.arange(m * b)
            ref, absref, L = grad_refs(name, ko, d, same, X, Y, cols_vg)
            if kind == GRAD:                              # drop the value rows and columns
                rsel = np.array([i * b + 1 + l for i in range(n) for l in range(d)]); csel = np.array([j * b + 1 + l for j in range(m) for l in range(d)])
                ref, absref = ref[np.ix_(rsel, csel)], absref[np.ix_(rsel, csel)]
            B = bsize(kind, d)
            hx = dev.points(X.astype(dt)); hy = hx if same else dev.points(Y.astype(dt))
            key, M = dev.block_matrix(kind, spec, hx, hy, n * B, m * B, dt)
            assert key == expected_key(kind, dt, d, n * B), (name, kind, d, key)
            w, i, c, e = worst(M, ref, absref, L, B, np.arange(m * B), dt)
            line = f"block-matrix {KIND_NAME[kind]} {name} {np.dtype(dt).name} d={d} n={n} m={m} same={same} key={key}: worst err/bound {w:.3f} at ({i}, {c}) e={e:.3e}"
            print(line)
            if not w <= 1.0:
                fails.append(line)
            if same:                                      # 6. the reference's issymmetric pin: equal to its transpose to the bound
                ws, i, c, e = worst(M.T, ref, absref, L, B, np.arange(m * B), dt)
                if not ws <= 1.0:
                    fails.append(f"transpose of {line}: {ws:.3f}")
            dev.close()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dt", [F64, F32])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("kind", [HESS, VGH])
def test_hessian_kinds_entrywise(cg, dev, kind, d, dt):
    fails = []
    for kern_t in PROFILES:
        k, kern = make_kernel(cg, kern_t, d)
        spec = cg.device_spec(k)
        iso = kern[0] in R.ISO
        for same in (False, True):
            n, m = shapes(kind, d)
            m = n if same else m
            rng = np.random.default_rng(11 * d + 1000 * same + len(kern[0]))
            X, Y = cloud(rng, iso, n, m, d, kern[2], same)
            B = bsize(kind, d)
            cols = column_subset(kind, d, m, rng)
            ref, absref, L = hess_refs(kind, kern, d, same, X, Y, cols)
            hx = dev.points(X.astype(dt)); hy = hx if same else dev.points(Y.astype(dt))
            key, M = dev.block_matrix(kind, spec, hx, hy, n * B, m * B, dt)
            assert key == expected_key(kind, dt, d, n * B), (kern, kind, d, key)
            w, i, c, e = worst(M[:, cols], ref, absref, L, B, cols, dt)
            line = f"block-matrix {KIND_NAME[kind]} {kern[0]} {np.dtype(dt).name} d={d} n={n} m={m} same={same} key={key} cols={len(cols)}: worst err/bound {w:.3f} at ({i}, {c}) e={e:.3e}"
            print(line)
            if not w <= 1.0:
                fails.append(line)
            if kern[0] == "Dot" and kind == HESS:
                assert not M.any(), "HessianKernel(Dot) is a zero operator: zeros are written"
            if same:                                      # 6. symmetric to the bound: rows `cols` of M against the same reference columns
                ws, i, c, e = worst(M[cols, :].T, ref, absref, L, B, cols, dt)
                if not ws <= 1.0:
                    fails.append(f"transpose of {line}: {ws:.3f}")
            dev.close()
    assert not fails, "\n".join(fails)


# ---- 2. store routes: one arithmetic, several store shapes --------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F64, F32])
@pytest.mark.parametrize("kind", [GRAD, VALGRAD, HESS, VGH])
def test_store_routes_are_bit_identical(cg, dev, kind, dt):
    vr = VRS[dt]
    d = {GRAD: 8, VALGRAD: 7, HESS: 4, VGH: 3}[kind]        # B = 8, 8, 16 and 13: 1 + d + d^2 is always odd, that kind has the one-row route only
    B = bsize(kind, d)
    k = cg.Lengthscale(cg.RQ(1.5), 1.1)
    spec = cg.device_spec(k)
    rng = np.random.default_rng(3 + kind)
    n, m = 70, 9
    X, Y = cloud(rng, True, n, m, d, 1.1, False)
    hx, hy = dev.points(X.astype(dt)), dev.points(Y.astype(dt))
    nb, mb = n * B, m * B
    wide = B % vr == 0
    ka, Ma = dev.block_matrix(kind, spec, hx, hy, nb, mb, dt)                                  # (a) aligned, ldo % VR == 0
    assert ka == (kind + 1) + 10 * (vr if wide else 1)
    ka2, Ma2 = dev.block_matrix(kind, spec, hx, hy, nb, mb, dt, ld=nb + 2 * vr)                # (a') padded but still a multiple of VR
    assert ka2 == ka
    ld_odd = nb + 1 if (nb + 1) % 2 else nb + 3
    kb, Mb = dev.block_matrix(kind, spec, hx, hy, nb, mb, dt, ld=ld_odd)                       # (b) odd ldo
    kc, Mc = dev.block_matrix(kind, spec, hx, hy, nb, mb, dt, offset=1)                        # (c) out off its 16-byte boundary
    assert kb == (kind + 1) + 10 and kc == (kind + 1) + 10, (kb, kc)
    for other in (Ma2, Mb, Mc):
        assert np.array_equal(np.ascontiguousarray(Ma).view(np.uint8), np.ascontiguousarray(other).view(np.uint8)), "store routes differ bitwise"
    kh, Mh = dev.block_matrix(kind, spec, hx, hy, nb, mb, dt, ld=nb + 3, loc_host=True)        # loc == HOST equals loc == DEVICE bit for bit
    assert kh == ka
    assert np.array_equal(np.ascontiguousarray(Ma).view(np.uint8), np.ascontiguousarray(Mh).view(np.uint8))


@pytest.mark.parametrize("dt", [F64, F32])
def test_odd_block_sizes_take_the_one_row_route(cg, dev, dt):
    """(d) odd B: gradient d = 3, value-gradient-Hessian d = 1 (B = 3) -> key (kind + 1) + 10, entries checked."""
    spec = cg.device_spec(cg.EQ())
    rng = np.random.default_rng(12)
    for kind, d in ((GRAD, 3), (VGH, 1)):
        B = bsize(kind, d)
        X, Y = cloud(rng, True, 6, 5, d, 1.0, False, far=False)
        key, M = dev.block_matrix(kind, spec, dev.points(X.astype(dt)), dev.points(Y.astype(dt)), 6 * B, 5 * B, dt)
        assert key == (kind + 1) + 10
        X64, Y64 = X.astype(F64), Y.astype(F64)
        ref = o.grad_matrix(o.Kernel(o.EQ), X64, Y64) if kind == GRAD else V.vgh_matrix(("EQ", 0.0, 1.0, 1.0), X64, Y64)
        assert np.abs(M - ref).max() <= 50 * TOL[dt] * np.abs(ref).max()


# ---- 3. matrix <-> MVM on the device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F64, F32])
@pytest.mark.parametrize("kind", [GRAD, VALGRAD, HESS, VGH])
def test_matrix_times_vector_is_the_mvm(cg, kind, dt):
    d = 5
    rng = np.random.default_rng(40 + kind)
    X, Y = cloud(rng, True, 40, 33, d, 1.2, False, far=False)
    wrap = {GRAD: cg.GradientKernel, VALGRAD: cg.ValueGradientKernel, HESS: cg.HessianKernel, VGH: cg.ValueGradientHessianKernel}[kind]
    G = cg.gramian(wrap(cg.Lengthscale(cg.EQ(), 1.2)), torch.from_numpy(X.astype(dt)).cuda(), torch.from_numpy(Y.astype(dt)).cuda())
    a = torch.from_numpy(rng.standard_normal(G.shape[1]).astype(dt)).cuda()
    M = G.to_dense()
    assert cg.get_info("last_block_matrix_path") % 10 == kind + 1
    assert M.shape == G.shape
    got, want = (M @ a).double(), (G @ a).double()
    den = (M.double().abs() @ a.double().abs())
    err = ((got - want).abs() / den).max().item()
    print(f"block-matrix {KIND_NAME[kind]} {np.dtype(dt).name}: max |M a - G a| / (|M| |a|) = {err:.3e}")
    # both sides are within TOL of the exact product relative to |M| |a| (here L <= 10 does not hold for every pair: the far pairs' share of |M| |a| is negligible)
    assert err <= 2 * TOL[dt]


# ---- 4. empty products, argument errors, refusals ---------------------------------------------------------------------------------------------
def test_empty_products_and_bad_leading_dimension(cg, dev):
    f = cg._ffi
    spec = cg.device_spec(cg.EQ())
    X = np.random.default_rng(1).standard_normal((4, 3))
    hx = dev.points(X)
    h0 = dev.points(np.zeros((0, 3)))
    for kind in (GRAD, VALGRAD, HESS, VGH):
        B = bsize(kind, 3)
        key, M = dev.block_matrix(kind, spec, hx, hx, 4 * B, 4 * B, F64)
        assert key != 0
        for a, b_, nb, mb in ((h0, hx, 0, 4 * B), (hx, h0, 4 * B, 0)):
            key, M = dev.block_matrix(kind, spec, a, b_, nb, mb, F64, ld=max(nb, 1))
            assert key == 0 and M.size == 0
        with pytest.raises(f.DimensionMismatch):
            dev.block_matrix(kind, spec, hx, hx, 4 * B, 4 * B, F64, ld=4 * B - 1)
    with pytest.raises(f.DimensionMismatch):
        dev.block_matrix(7, spec, hx, hx, 12, 12, F64)


def test_unsupported_kernels_under_the_hessian_kinds_are_accepted_under_the_gradient_kinds(cg, dev):
    f = cg._ffi
    X = np.random.default_rng(2).standard_normal((3, 2))
    hx = dev.points(X)
    for k, word in ((cg.MaternP(2), "MaternP"), (cg.EQ() + cg.Cauchy(), "composite"), (cg.EQ() ** 2, "ExponentiatedQuadratic^2")):
        spec = cg.device_spec(k)
        for kind, wrapper in ((HESS, "HessianKernel"), (VGH, "ValueGradientHessianKernel")):
            with pytest.raises(f.UnsupportedKernel) as ei:
                dev.block_matrix(kind, spec, hx, hx, 3 * bsize(kind, 2), 3 * bsize(kind, 2), F64)
            assert word in str(ei.value) and wrapper in str(ei.value), str(ei.value)
        for kind in (GRAD, VALGRAD):
            key, M = dev.block_matrix(kind, spec, hx, hx, 3 * bsize(kind, 2), 3 * bsize(kind, 2), F64)
            assert key % 10 == kind + 1
    h33 = dev.points(np.random.default_rng(3).standard_normal((1, 33)))
    spec = cg.device_spec(cg.EQ())
    for kind, wrapper in ((HESS, "HessianKernel"), (VGH, "ValueGradientHessianKernel")):
        with pytest.raises(f.UnsupportedKernel) as ei:
            dev.block_matrix(kind, spec, h33, h33, bsize(kind, 33), bsize(kind, 33), F64)
        assert "d = 33" in str(ei.value) and wrapper in str(ei.value)
    key, M = dev.block_matrix(GRAD, spec, h33, h33, 33, 33, F64)
    assert key == 1 + 10


# ---- 5. Python ---------------------------------------------------------------------------------------------------------------------------
def all_four(cg, X, Y=None):
    k = cg.Lengthscale(cg.RQ(2.0), 1.3)
    return [cg.gramian(w(k), X, Y) for w in (cg.GradientKernel, cg.ValueGradientKernel, cg.HessianKernel, cg.ValueGradientHessianKernel)]


def test_python_to_dense_block_and_getitem(cg, dev):
    rng = np.random.default_rng(8)
    d, n, m = 3, 9, 7
    Xn, Yn = rng.standard_normal((n, d)), rng.standard_normal((m, d))
    X, Y = torch.from_numpy(Xn).cuda(), torch.from_numpy(Yn).cuda()
    spec = cg.device_spec(cg.Lengthscale(cg.RQ(2.0), 1.3))
    hx, hy = dev.points(Xn), dev.points(Yn)
    for kind, G in enumerate(all_four(cg, X, Y)):
        B = bsize(kind, d)
        assert G.block_size == B and G.shape == (n * B, m * B)
        M = G.to_dense()
        assert M.shape == G.shape
        _, raw = dev.block_matrix(kind, spec, hx, hy, n * B, m * B, F64)
        assert np.array_equal(M.cpu().numpy(), raw), "to_dense() differs from the raw call"
        idx = torch.tensor([6, 0, 3], device="cuda")
        for i, j, rows, cols in ((2, 5, [2], [5]), (slice(1, 6), slice(None, None, 2), range(1, 6), range(0, m, 2)), (idx, 4, [6, 0, 3], [4]),
                                 (-1, slice(2, 4), [n - 1], [2, 3])):
            sub = G.block(i, j)
            R_ = np.concatenate([np.arange(r * B, (r + 1) * B) for r in rows]); C_ = np.concatenate([np.arange(c * B, (c + 1) * B) for c in cols])
            assert torch.equal(sub, M[R_][:, C_]), (kind, i, j)
        for I, J in ((0, 0), (n * B - 1, m * B - 1), (-1, 3), (slice(B - 1, 2 * B + 1), 5), (slice(None), slice(None)),
                     (slice(3, None, 4), slice(2 * B, 3 * B)), (7, slice(m * B - 2, None, -3))):
            got = G[I, J]
            want = M.cpu().numpy()[I, J]
            assert np.array_equal(got.cpu().numpy(), want), (kind, I, J)


@pytest.mark.parametrize("value", [False, True])
def test_wider_points_than_the_register_route_keep_working(cg, value):
    """d = 65 > 64: covgram_block_matrix refuses the gradient kinds (rows in registers), the MVMs do not (panel path); to_dense(), block()
    and G[I, J] of such a Gramian go through the MVM as they did before the entry point existed."""
    d, n, m = 65, 6, 4
    rng = np.random.default_rng(65)
    Xn, Yn = rng.standard_normal((n, d)), rng.standard_normal((m, d))
    k, ko = cg.Lengthscale(cg.EQ(), 8.0), o.Kernel(o.EQ, lengthscale=8.0)
    G = cg.gramian((cg.ValueGradientKernel if value else cg.GradientKernel)(k), torch.from_numpy(Xn).cuda(), torch.from_numpy(Yn).cuda())
    B = d + 1 if value else d
    ref = (o.valgrad_matrix if value else o.grad_matrix)(ko, Xn, Yn)
    M = G.to_dense().cpu().numpy()
    assert M.shape == (n * B, m * B)
    assert np.abs(M - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(G.block(2, slice(1, 3)).cpu().numpy() - ref[2 * B:3 * B, B:3 * B]).max() <= 1e-12 * np.abs(ref).max()
    assert abs(float(G[B + 3, 2 * B + 1]) - ref[B + 3, 2 * B + 1]) <= 1e-12 * np.abs(ref).max()
    with pytest.raises(cg._ffi.UnsupportedKernel):
        BDev(cg).block_matrix(int(value), cg.device_spec(k), G.inner._px.handle, G.inner._py.handle, n * B, m * B, F64)


def test_cholesky_of_a_symmetric_gradient_gramian(cg):
    X = torch.from_numpy(np.random.default_rng(7).standard_normal((20, 3))).cuda()
    G = cg.gramian(cg.GradientKernel(cg.EQ()), X)
    M = G.to_dense()
    F = cg.cholesky(G)
    L = F.L
    err = ((L @ L.T - M).norm() / M.norm()).item()
    print(f"cholesky(GradientKernel(EQ)) n=20 d=3: |L L' - M| / |M| = {err:.2e}")
    assert err <= 1e-10


def test_large_hessian_to_dense_finishes_and_matches_a_column_subset(cg):
    d, n = 8, 128                                       # n B = m B = 8192, fp32: 256 MiB
    rng = np.random.default_rng(21)
    Xn = rng.standard_normal((n, d)).astype(F32)
    kern_t = PROFILES[0]
    k, kern = make_kernel(cg, kern_t, d)
    G = cg.gramian(cg.HessianKernel(k), torch.from_numpy(Xn).cuda())
    M = G.to_dense()
    assert cg.get_info("last_block_matrix_path") == 3 + 10 * 4
    assert M.shape == (8192, 8192)
    cols = np.array(sorted({0, 63, 8128, 8191} | set(int(c) for c in rng.choice(8192, size=12, replace=False))))
    ref, absref, L = hess_refs(HESS, kern, d, "large", Xn, Xn, cols)
    w, i, c, e = worst(M[:, torch.from_numpy(cols).cuda()].cpu().numpy(), ref, absref, L, d * d, cols, F32)
    print(f"block-matrix hessian EQ float32 d=8 n=m=128 (256 MiB): worst err/bound {w:.3f} at ({i}, {c}) e={e:.3e}")
    assert w <= 1.0
