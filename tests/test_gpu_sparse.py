"""sparse(G, delta) on the device: covgram_sparse_create / _info / _export / _mvm / _destroy and the Python SparseGramian.

Clouds, the choice of the lengthscale and the reference are in tests/sparse_ref.py: seeded Gaussian clouds (spread 0.8 sqrt(8 / d) for
d > 8), one row of X far outside (it keeps nothing), rows of X copied from Y (s = 0), and a lengthscale that leaves the band
|s / R^2 - 1| <= 8 (d + 2) eps_T empty — asserted on the CPU, together with a kept share in (0.01, 0.6) and an empty row, before the
device is touched.  Then the pattern must equal the fp64 pattern EXACTLY; values meet the entrywise bound of tests/matrix_cases.py.

Shapes: n in {1, 63, 257}, m in {193, 1500}, d in {1, 3, 8, 32, 70} (every register bucket's edge cases and the generic kernel), both
dtypes, X != Y and gramian(k, x) on one handle.  m = 1500 is 24 LDS tiles and, with n <= 257 (one or two row blocks), a column split
over 6 chunks.  (257, 1500) in fp32 at d = 70 has 385 500 pair distances against a band of 6.9e-5: SEEDED names the cloud seed and
the share window (1.2 % to 58 %, the sparser tail of the distances) at which a gap 1.46 times the band exists; every other case finds
its gap with seed 0 in the default window.

Products are judged row-wise, the project's convention (tests/test_gpu_grad_rowwise.py) for the 5-argument mul!:
    |y_i - ref_i| <= |alpha| sum_j bound_ij |a_j| + TOL (|alpha| sum_j |ref_ij| |a_j| + |beta| |y0_i|) + tiny."""
import ctypes as C

import numpy as np
import pytest
import torch

import covgram_oracle as o
import matrix_cases as mc
import sparse_ref as sr

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TDT = {F32: torch.float32, F64: torch.float64}
DELTA = sr.DELTA
NANV = float("nan")


def kernels(cg):
    """(name, l -> cg kernel, l -> oracle kernel): each with a Lengthscale and a Constant factor."""
    return [
        ("EQ", lambda l: 2.5 * cg.Lengthscale(cg.EQ(), l), lambda l: o.Kernel(o.EQ, lengthscale=l, scale=2.5)),
        ("Exponential", lambda l: 0.5 * cg.Lengthscale(cg.Exp(), l), lambda l: o.Kernel(o.EXP, lengthscale=l, scale=0.5)),
        ("GammaExponential(1.5)", lambda l: 3.0 * cg.Lengthscale(cg.GammaExponential(1.5), l),
         lambda l: o.Kernel(o.GAMMAEXP, param=1.5, lengthscale=l, scale=3.0)),
        ("MaternP(2)", lambda l: 1.5 * cg.Lengthscale(cg.MaternP(2), l), lambda l: o.Kernel(o.MATERNP, p=2, lengthscale=l, scale=1.5)),
        ("Matern(1.3)", lambda l: 0.7 * cg.Lengthscale(cg.Matern(1.3), l), lambda l: o.Kernel(o.MATERN, param=1.3, lengthscale=l, scale=0.7)),
    ]


SHAPES = [(1, 193, False), (63, 193, False), (63, 1500, False), (257, 193, False), (257, 1500, False), (63, 63, True), (257, 257, True)]

# (dtype, d, n, m) -> (cloud seed, share window) of test_pattern_values_and_dense where seed 0 and the default window leave no gap
# wider than the band; found by a search over seeds on the CPU, which the asserts of sparse_ref.fit_kernel repeat on every run
SEEDED = {(F32, 70, 257, 1500): (341, (0.012, 0.58))}


class Case:
    """One cloud + kernel with everything the checks need, computed once on the CPU."""

    def __init__(self, cg, kname, mk, mko, n, m, d, dt, same, seed=0, window=sr.WINDOW):
        rng = np.random.default_rng(1000 * d + n + m + 7919 * seed)
        self.X, self.Y, self.far, self.copies = sr.cloud(rng, n, m, d, dt, same)
        self.ko, self.s, self.keep, self.R = sr.fit_kernel(mko, self.X, self.Y, d, dt, DELTA, window)
        self.k = mk(self.ko.lengthscale)
        self.n, self.m, self.d, self.dt, self.same = n, m, d, dt, same
        self.name = f"{kname} {np.dtype(dt).name} d={d} n={n} m={m}{' (x, x)' if same else ''}"
        if not same and n >= 2:
            assert not self.keep[self.far].any(), "the far row keeps something"
            assert (self.keep.sum(axis=1) == 0).any()
        for i in self.copies:
            assert (self.s[i] == 0).any()
        self.rowptr, self.colind = sr.csr_of(self.keep)
        self.ref, self.bound = sr.reference_and_bound(self.ko, self.X, self.Y, dt)

    def gramian(self, cg):
        Xt = torch.from_numpy(self.X).cuda()
        return cg.gramian(self.k, Xt) if self.same else cg.gramian(self.k, Xt, torch.from_numpy(self.Y).cuda())


def rowwise_check(case, got, a, y0, alpha, beta, what, fails):
    """got, a, y0: (n, p) / (m, p) / (n, p) arrays; ref from the fp64 reference entries of the kept pattern."""
    Sref = np.where(case.keep, case.ref, 0.0)
    Sb = np.where(case.keep, case.bound, 0.0)
    a64 = a.astype(F64)
    yb = np.zeros_like(got, dtype=F64) if beta == 0 else y0.astype(F64)
    want = alpha * (Sref @ a64) + beta * yb
    lim = abs(alpha) * (Sb @ np.abs(a64)) + mc.TOL[case.dt] * (abs(alpha) * (np.abs(Sref) @ np.abs(a64)) + abs(beta) * np.abs(yb)) + mc.tiny(case.dt)
    g = got.astype(F64)
    with np.errstate(invalid="ignore"):
        r = np.where(np.isfinite(g), np.abs(g - want) / lim, np.inf)
    i, c = np.unravel_index(int(np.argmax(r)), r.shape)
    line = f"sparse-rowwise {case.name} {what}: worst err/bound {r[i, c]:.3f} at row {i} col {c} got {g[i, c]!r} want {want[i, c]!r}"
    print(line)
    if not r[i, c] <= 1.0:
        fails.append(line)


# ---- 1. pattern, values, Matrix(G) - to_dense(S) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("d", [1, 3, 8, 32, 70])
def test_pattern_values_and_dense(cg, dt, d):
    fails = []
    for kname, mk, mko in kernels(cg):
        for n, m, same in SHAPES:
            seed, window = SEEDED.get((dt, d, n, m), (0, sr.WINDOW))
            case = Case(cg, kname, mk, mko, n, m, d, dt, same, seed=seed, window=window)
            G = case.gramian(cg)
            S = cg.sparse(G, DELTA)
            assert S.shape == (n, m) and S.dtype == TDT[dt]
            assert abs(S.radius - case.R) <= 1e-15 * case.R, (case.name, S.radius, case.R)
            rowptr, colind, vals = (t.cpu().numpy() for t in S.csr())
            assert rowptr.dtype == np.int64 and colind.dtype == np.int32 and vals.dtype == dt
            ok = S.nnz == int(case.rowptr[-1]) and np.array_equal(rowptr, case.rowptr) and np.array_equal(colind, case.colind)
            print(f"sparse-pattern {case.name}: nnz {S.nnz} (reference {int(case.rowptr[-1])}, share {case.keep.mean():.3f}) "
                  f"{'equal' if ok else 'DIFFERENT'}")
            if not ok:
                fails.append(f"pattern {case.name}: nnz {S.nnz} vs {int(case.rowptr[-1])}")
                continue
            for i in range(n):                                  # ascending within every row (implied by equality; stated by the header)
                assert np.all(np.diff(colind[rowptr[i]:rowptr[i + 1]]) > 0)
            w, _, j = mc.worst_entry(vals.reshape(1, -1), case.ref[case.keep].reshape(1, -1), case.bound[case.keep].reshape(1, -1))
            print(f"sparse-values {case.name}: worst err/bound {w:.3f} at entry {j}")
            if not w <= 1.0:
                fails.append(f"values {case.name}: {w}")
            D = S.to_dense().cpu().numpy().astype(F64)
            M = G.to_dense().cpu().numpy().astype(F64)
            diff = float(np.abs(M - D).max())
            print(f"sparse-dense {case.name}: max |Matrix(G) - to_dense(S)| = {diff:.3e} (delta {DELTA:g})")
            if not diff <= DELTA:
                fails.append(f"dense {case.name}: {diff}")
    assert not fails, "\n".join(fails)


# ---- 2. the product -----------------------------------------------------------------------------------------------------------------
class Raw:
    """Raw C ABI calls on the library context of the Python API."""

    def __init__(self, cg):
        self.cg, self.f, self.lib, self.ctx = cg, cg._ffi, cg._ffi.lib(), cg.get_ctx()
        self.keep = []

    def points(self, A, loc_host=False):
        h = self.f._P()
        code = self.f.F64 if A.dtype == F64 else self.f.F32
        if loc_host:
            A = np.ascontiguousarray(A)
            self.f.check(self.lib.covgram_points_create(self.ctx.bind_stream(), C.byref(h), A.ctypes.data_as(C.c_void_p), A.shape[0], A.shape[1], code, self.f.HOST))
            self.keep.append((h, A))
        else:
            t = torch.from_numpy(np.ascontiguousarray(A)).cuda()
            self.f.check(self.lib.covgram_points_create(self.ctx.bind_stream(), C.byref(h), self.f._P(t.data_ptr()), t.shape[0], t.shape[1], code, self.f.DEVICE))
            self.keep.append((h, t))
        return h

    def drop_points(self):
        for h, _ in reversed(self.keep):
            self.lib.covgram_points_destroy(h)
        self.keep = []

    def create(self, k, hx, hy, delta=DELTA):
        S = self.f._P()
        rc = self.lib.covgram_sparse_create(self.ctx.bind_stream(), C.byref(S), self.f.kref(self.cg.device_spec(k)), hx, hy, delta)
        return rc, S

    def info(self, S):
        n, m, nnz, dt, r = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1), C.c_int32(-1), C.c_double(-1)
        self.f.check(self.lib.covgram_sparse_info(S, C.byref(n), C.byref(m), C.byref(nnz), C.byref(dt), C.byref(r)))
        return n.value, m.value, nnz.value, dt.value, r.value


@pytest.fixture()
def raw(cg):
    r = Raw(cg)
    yield r
    r.drop_points()


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("d", [3, 32, 70])
def test_product_rowwise(cg, raw, dt, d):
    """nrhs in {1, 3} with lda > m and ldy > n through the raw ABI (device pointers, padding rows of y untouched), alpha, beta != 0 and
    beta = 0 over a NaN-filled y; host pointers; y aliasing a (n = m); the Python operator's @ and mul_ with a matrix."""
    f, lib = raw.f, raw.lib
    fails = []
    alpha, beta = -1.5, 0.75
    for kname, mk, mko in kernels(cg):
        for n, m, same in ((63, 1500, False), (257, 193, False), (257, 257, True)):
            case = Case(cg, kname, mk, mko, n, m, d, dt, same, seed=1)
            rng = np.random.default_rng(5 + d + n)
            hx = raw.points(case.X)
            hy = hx if same else raw.points(case.Y)
            rc, S = raw.create(case.k, hx, hy)
            assert rc == 0, lib.covgram_last_error()
            raw.drop_points()                                   # the handle keeps no reference to X or Y
            try:
                assert raw.info(S)[2] == int(case.rowptr[-1]), case.name
                for nrhs in (1, 3):
                    lda, ldy = m + 5, n + 3
                    a = rng.standard_normal((m, nrhs)).astype(dt)
                    y0 = rng.standard_normal((n, nrhs)).astype(dt)
                    A = np.full((nrhs, lda), 7.0, dtype=dt); A[:, :m] = a.T
                    for al, be in ((alpha, beta), (alpha, 0.0)):
                        Yb = np.full((nrhs, ldy), NANV, dtype=dt)
                        if be != 0:
                            Yb[:, :n] = y0.T
                        At, Yt = torch.from_numpy(A).cuda(), torch.from_numpy(Yb).cuda()
                        f.check(lib.covgram_sparse_mvm(S, f._P(At.data_ptr()), lda, f._P(Yt.data_ptr()), ldy, nrhs, al, be, f.DEVICE))
                        got = Yt.cpu().numpy()
                        assert np.isnan(got[:, n:]).all(), "padding rows of y written"
                        rowwise_check(case, got[:, :n].T, a, y0, al, be, f"device nrhs={nrhs} beta={be}", fails)
                        # host pointers, same call
                        Yh = Yb.copy()
                        f.check(lib.covgram_sparse_mvm(S, A.ctypes.data_as(C.c_void_p), lda, Yh.ctypes.data_as(C.c_void_p), ldy, nrhs, al, be, f.HOST))
                        assert np.isnan(Yh[:, n:]).all(), "host padding rows of y written"
                        assert np.array_equal(Yh[:, :n], got[:, :n]), "host and device products differ"
                if n == m:                                      # y aliasing a: in place, and a shifted overlap
                    a = rng.standard_normal((n, 1)).astype(dt)
                    Vt = torch.from_numpy(a[:, 0].copy()).cuda()
                    f.check(lib.covgram_sparse_mvm(S, f._P(Vt.data_ptr()), n, f._P(Vt.data_ptr()), n, 1, alpha, beta, f.DEVICE))
                    rowwise_check(case, Vt.cpu().numpy().reshape(n, 1), a, a, alpha, beta, "in place y = a", fails)
                    buf = torch.zeros(n + 8, dtype=TDT[dt], device="cuda")
                    buf[8:] = torch.from_numpy(a[:, 0].copy()).cuda()
                    f.check(lib.covgram_sparse_mvm(S, f._P(buf.data_ptr() + 8 * buf.element_size()), n, f._P(buf.data_ptr()), n, 1, alpha, 0.0, f.DEVICE))
                    rowwise_check(case, buf[:n].cpu().numpy().reshape(n, 1), a, a, alpha, 0.0, "overlapping y = a - 8", fails)
            finally:
                assert lib.covgram_sparse_destroy(S) == 0
            # the Python operator
            Sp = cg.sparse(case.gramian(cg), DELTA)
            a = rng.standard_normal((m, 3)).astype(dt)
            y0 = rng.standard_normal((n, 3)).astype(dt)
            rowwise_check(case, (Sp @ torch.from_numpy(a[:, 0].copy()).cuda()).cpu().numpy().reshape(n, 1), a[:, :1], y0[:, :1], 1.0, 0.0, "S @ a", fails)
            yt = torch.from_numpy(y0.copy()).cuda()
            cg.mul_(yt, Sp, torch.from_numpy(a).cuda(), alpha, beta)
            rowwise_check(case, yt.cpu().numpy(), a, y0, alpha, beta, "mul_ matrix", fails)
    assert not fails, "\n".join(fails)


# share window -> lanes per row: nnz / n = share x m falls below 4, below 32, below 256 and above for these four
GROUPS = [(63, 193, (0.011, 0.019), 1), (63, 1500, (0.012, 0.02), 4), (63, 1500, (0.03, 0.15), 16), (63, 1500, (0.2, 0.5), 64)]


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("n,m,window,group", GROUPS)
def test_product_every_group_width_and_second_pass(cg, dt, n, m, window, group):
    """Each of the product kernel's 1, 4, 16 and 64 lanes per row, asserted from nnz / n of the reference pattern, with 6 right-hand
    sides (a pass of four and a pass of two) and 5 (a pass of four, then the single-column instance in the same call)."""
    kname, mk, mko = kernels(cg)[0]
    case = Case(cg, kname, mk, mko, n, m, 3, dt, False, seed=4, window=window)
    assert sr.group_width(int(case.rowptr[-1]), n) == group, (int(case.rowptr[-1]), n)
    S = cg.sparse(case.gramian(cg), DELTA)
    assert S.nnz == int(case.rowptr[-1])
    rng = np.random.default_rng(11 + group)
    fails = []
    for nrhs in (6, 5):
        a = rng.standard_normal((m, nrhs)).astype(dt)
        y0 = rng.standard_normal((n, nrhs)).astype(dt)
        yt = torch.from_numpy(y0.copy()).cuda()
        cg.mul_(yt, S, torch.from_numpy(a).cuda(), -1.5, 0.75)
        rowwise_check(case, yt.cpu().numpy(), a, y0, -1.5, 0.75, f"group {group} nrhs={nrhs}", fails)
        cols = torch.stack([S @ torch.from_numpy(a[:, c].copy()).cuda() for c in range(nrhs)], dim=1)
        assert torch.equal(S @ torch.from_numpy(a).cuda(), cols), "a column of a later pass differs from the single-column product"
    assert not fails, "\n".join(fails)


# ---- 3. determinism -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
def test_two_creates_and_two_products_bit_identical(cg, dt):
    kname, mk, mko = kernels(cg)[0]
    for n, m, d, same in ((63, 1500, 8, False), (257, 257, 70, True)):
        case = Case(cg, kname, mk, mko, n, m, d, dt, same, seed=2)
        G = case.gramian(cg)
        S1, S2 = cg.sparse(G, DELTA), cg.sparse(G, DELTA)
        for t1, t2 in zip(S1.csr(), S2.csr()):
            assert torch.equal(t1, t2)
        a = torch.from_numpy(np.random.default_rng(3).standard_normal((m, 3)).astype(dt)).cuda()
        y1, y2, y3 = S1 @ a, S1 @ a, S2 @ a
        assert torch.equal(y1, y2) and torch.equal(y1, y3)
        assert np.array_equal(y1.cpu().numpy().view(np.uint8), y2.cpu().numpy().view(np.uint8))


# ---- 4. empty products --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
def test_empty_products(cg, raw, dt):
    k = cg.Lengthscale(cg.EQ(), 0.1)
    X = np.random.default_rng(4).standard_normal((5, 3)).astype(dt)
    E = np.zeros((0, 3), dtype=dt)
    for A, B, n, m in ((E, X, 0, 5), (X, E, 5, 0), (E, E, 0, 0)):
        S = cg.sparse(cg.gramian(k, torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()), DELTA)
        assert S.shape == (n, m) and S.nnz == 0
        rowptr, colind, vals = S.csr()
        assert rowptr.shape == (n + 1,) and not rowptr.any() and colind.numel() == 0 and vals.numel() == 0
        assert S.to_dense().shape == (n, m)
        a = torch.ones(m, dtype=TDT[dt], device="cuda")
        y = torch.full((n,), NANV, dtype=TDT[dt], device="cuda")
        S.mul_(y, a, 2.0, 0.0)
        assert not y.any()                                      # beta = 0 over NaN: zeros
        y = torch.full((n,), 3.0, dtype=TDT[dt], device="cuda")
        S.mul_(y, a, 2.0, 0.5)
        assert bool((y == 1.5).all())
    # a radius that keeps nothing between two distant clouds: nnz = 0 with rows and columns
    S = cg.sparse(cg.gramian(k, torch.from_numpy(X).cuda(), torch.from_numpy(X + 100).cuda()), DELTA)
    assert S.nnz == 0 and not (S @ torch.ones(5, dtype=TDT[dt], device="cuda")).any()


# ---- 5. CG --------------------------------------------------------------------------------------------------------------------------
def test_cg_reaches_the_dense_operators_residual(cg):
    """solve.cg on S + sigma^2 I like any other operator: converged, the residual of the SPARSE system at the tolerance the CG tests of
    the block Gramians use (2 reltol), and the solution within delta-sized perturbation of the dense operator's."""
    rng = np.random.default_rng(21)
    n, d = 400, 3
    X = rng.standard_normal((n, d))
    k = cg.Lengthscale(cg.MaternP(2), 0.05)
    G = cg.gramian(k, torch.from_numpy(X).cuda())
    S = cg.sparse(G, DELTA)
    assert n <= S.nnz < 0.6 * n * n
    sig = 1e-2 * torch.ones(n, device="cuda", dtype=torch.float64)
    b = torch.from_numpy(rng.standard_normal(n)).cuda()
    xs, info_s = cg.cg(S + sig, b, reltol=1e-9, maxiter=4 * n)
    xd, info_d = cg.cg(G + sig, b, reltol=1e-9, maxiter=4 * n)
    assert info_s["converged"] and info_d["converged"], (info_s, info_d)
    nb = float(b.norm())
    res_s = float((S @ xs + sig * xs - b).norm())
    res_d = float((G @ xd + sig * xd - b).norm())
    print(f"sparse cg: residual {res_s:.3e} (dense operator {res_d:.3e}), |b| {nb:.3e}, iterations {info_s['iterations']} / {info_d['iterations']}")
    assert res_s <= 2e-9 * nb and res_d <= 2e-9 * nb
    # |S - G| <= delta entrywise, so |xs - xd| <= |A^-1| n delta |x| with |A^-1| <= 1 / sigma^2
    assert float((xs - xd).norm()) <= n * DELTA / 1e-2 * float(xd.norm())


# ---- 6. the raw ABI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
def test_raw_abi(cg, raw, dt):
    f, lib = raw.f, raw.lib
    kname, mk, mko = kernels(cg)[3]
    n, m, d = 63, 193, 3
    case = Case(cg, kname, mk, mko, n, m, d, dt, False, seed=3)
    hx, hy = raw.points(case.X, loc_host=True), raw.points(case.Y)
    rc, S = raw.create(case.k, hx, hy)
    assert rc == 0, lib.covgram_last_error()
    try:
        nn, mm, nnz, code, r = raw.info(S)
        assert (nn, mm, nnz, code) == (n, m, int(case.rowptr[-1]), f.F64 if dt == F64 else f.F32)
        assert abs(r - case.R) <= 1e-15 * case.R
        assert lib.covgram_sparse_info(S, None, None, None, None, None) == 0
        # export to the host
        rp, ci, va = np.full(n + 1, -1, np.int64), np.full(nnz, -1, np.int32), np.full(nnz, NANV, dt)
        f.check(lib.covgram_sparse_export(S, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p), va.ctypes.data_as(C.c_void_p), f.HOST))
        assert np.array_equal(rp, case.rowptr) and np.array_equal(ci, case.colind)
        w, _, _ = mc.worst_entry(va.reshape(1, -1), case.ref[case.keep].reshape(1, -1), case.bound[case.keep].reshape(1, -1))
        assert w <= 1.0, w
        # ... and to the device, bitwise the same; NULL pointers skip an array
        rpt = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        cit = torch.full((nnz,), -1, dtype=torch.int32, device="cuda")
        vat = torch.full((nnz,), NANV, dtype=TDT[dt], device="cuda")
        f.check(lib.covgram_sparse_export(S, f._P(rpt.data_ptr()), None, None, f.DEVICE))
        assert np.array_equal(rpt.cpu().numpy(), rp) and bool((cit == -1).all())
        f.check(lib.covgram_sparse_export(S, None, f._P(cit.data_ptr()), f._P(vat.data_ptr()), f.DEVICE))
        assert np.array_equal(cit.cpu().numpy(), ci) and np.array_equal(vat.cpu().numpy().view(np.uint8), va.view(np.uint8))
        # argument checks
        a = torch.ones(m, dtype=TDT[dt], device="cuda"); y = torch.zeros(n, dtype=TDT[dt], device="cuda")
        assert lib.covgram_sparse_mvm(S, f._P(a.data_ptr()), m - 1, f._P(y.data_ptr()), n, 1, 1.0, 0.0, f.DEVICE) == f.EINVAL
        assert lib.covgram_sparse_mvm(S, f._P(a.data_ptr()), m, f._P(y.data_ptr()), n - 1, 1, 1.0, 0.0, f.DEVICE) == f.EINVAL
        assert lib.covgram_sparse_mvm(S, f._P(a.data_ptr()), m, f._P(y.data_ptr()), n, 0, 1.0, 0.0, f.DEVICE) == f.EINVAL
        f.check(lib.covgram_sparse_mvm(S, f._P(a.data_ptr()), m, f._P(y.data_ptr()), n, 1, 1.0, 0.0, f.DEVICE))
        fails = []
        rowwise_check(case, y.cpu().numpy().reshape(n, 1), np.ones((m, 1), dt), np.zeros((n, 1), dt), 1.0, 0.0, "raw", fails)
        assert not fails, fails
    finally:
        assert lib.covgram_sparse_destroy(S) == 0
    assert lib.covgram_sparse_destroy(None) == 0
    # refusals: COVGRAM_EUNSUPPORTED and a message that names the kernel; no handle is made
    for k, word in ((cg.RQ(1.0), "RationalQuadratic"), (cg.EQ() + cg.Lengthscale(cg.Exp(), 0.5), "Sum")):
        rc, S2 = raw.create(k, hx, hy)
        assert rc == f.EUNSUPPORTED and not S2
        assert word in lib.covgram_last_error().decode(), lib.covgram_last_error()
        with pytest.raises(cg.UnsupportedKernel) as e:
            cg.sparse(cg.gramian(k, torch.from_numpy(case.X).cuda()), DELTA)
        assert word in str(e.value)
    rc, S2 = raw.create(1e-7 * cg.EQ(), hx, hy)
    assert rc == f.EINVAL and not S2
    with pytest.raises(cg.UnsupportedKernel):
        cg.sparse(cg.gramian(cg.GradientKernel(cg.EQ()), torch.from_numpy(case.X).cuda()), DELTA)
    with pytest.raises(cg.UnsupportedKernel):
        cg.sparse(cg.gramian(cg.EQ(), cg.srange(0, 1, 50)), DELTA)


def test_time_kernels_brackets_fill_and_product(cg):
    kname, mk, mko = kernels(cg)[0]
    case = Case(cg, kname, mk, mko, 257, 193, 3, F64, False)
    G = case.gramian(cg)
    try:
        cg.set_option("time_kernels", 1)
        cg.kernel_time()
        S = cg.sparse(G, DELTA)
        ms, launches = cg.kernel_time()
        assert launches == 1 and ms > 0
        S @ torch.ones(193, dtype=torch.float64, device="cuda")
        ms, launches = cg.kernel_time()
        assert launches == 1 and ms > 0
    finally:
        cg.set_option("time_kernels", 0)
