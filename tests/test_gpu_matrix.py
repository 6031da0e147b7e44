"""Matrix(G) entry by entry on every kernel route of covgram_matrix (csrc/matrix.hip), each route pinned by the info key
last_matrix_path (route + 10 DM + 1000 VR, include/covgram.h) BEFORE any number is looked at.

Reference: covgram_oracle.matrix on the data as rounded to the dtype (fp64 arithmetic, direct differences).  Error measure: ENTRYWISE,
|M_ij - ref_ij| <= bound_ij + tiny, bound_ij as derived in tests/matrix_cases.py (TOL = 1e-5 fp32 / 1e-12 fp64; relative with the
allowance max(1, L_ij / 10) for isotropic kernels, TOL (|phi| + |phi'| sum |x_l||y_l|) for dot-product kernels).  That an exactly
rounded fp32 evaluation stays inside the bound is asserted without a GPU in tests/test_matrix_bound_host.py.

Unless noted every call goes through the raw C ABI with device pointers into an allocation pre-filled with NaN, with guard elements
in front and behind: afterwards every entry i < n is finite and checked, and every padding row n <= i < ld, and every guard, still
is the sentinel.  Every case prints its worst err / bound, where it was, family and route key."""
import ctypes as C

import numpy as np
import pytest
import torch

import covgram_oracle as o
import kernel_cases
import matrix_cases as mc

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TDT = {F32: torch.float32, F64: torch.float64}
VRS = {F32: 4, F64: 2}                         # rows per thread of the 16-byte-store route
GUARD = 16                                     # sentinel elements in front of and behind the output (a multiple of 16 bytes)


def bucket(d):
    return next(b for b in (4, 8, 16, 32, 64) if d <= b)


def expected_key(dt, d, n, ld, composite=False, variant=0, aligned=True):
    if d > 64 or variant == 1:
        return (2 if composite else 1) + 1000
    if composite:
        return 4 + 10 * bucket(d) + 1000
    vr = VRS[dt] if (d <= 16 and n % VRS[dt] == 0 and ld % VRS[dt] == 0 and aligned) else 1
    return 3 + 10 * bucket(d) + 1000 * vr


class Dev:
    """Raw C ABI calls on the library context of the Python API (so cg.set_option / cg.get_info address the same context)."""

    def __init__(self, cg):
        self.cg, self.f, self.lib, self.ctx = cg, cg._ffi, cg._ffi.lib(), cg.get_ctx()
        self.keep = []

    def points(self, A):
        t = torch.from_numpy(np.ascontiguousarray(A)).cuda()
        h = self.f._P()
        self.f.check(self.lib.covgram_points_create(self.ctx.bind_stream(), C.byref(h), self.f._P(t.data_ptr()), t.shape[0], t.shape[1],
                                                    self.f.F64 if t.dtype == torch.float64 else self.f.F32, self.f.DEVICE))
        self.keep.append((h, t))
        return h

    def slice(self, parent, start, count):
        h = self.f._P()
        self.f.check(self.lib.covgram_points_slice(parent, start, count, C.byref(h)))
        self.keep.append((h, None))
        return h

    def close(self):
        for h, _ in reversed(self.keep):
            self.lib.covgram_points_destroy(h)
        self.keep = []

    def matrix(self, spec, hx, hy, n, m, dt, ld=None, offset=0):
        """(route key, M as an n x m array) with the sentinel checks described in the module docstring; `offset` elements move out
        off its 16-byte boundary."""
        ld = n if ld is None else ld
        buf = torch.full((GUARD + offset + ld * m + GUARD,), float("nan"), dtype=TDT[dt], device="cuda")
        assert buf.data_ptr() % 16 == 0
        start = GUARD + offset
        ptr = buf.data_ptr() + start * buf.element_size()
        assert (ptr % 16 == 0) == (offset * buf.element_size() % 16 == 0)
        self.f.check(self.lib.covgram_matrix(self.ctx.bind_stream(), self.f.kref(spec), hx, hy, self.f._P(ptr), ld, self.f.DEVICE))
        key = self.cg.get_info("last_matrix_path")
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert np.isnan(h[:start]).all() and np.isnan(h[start + ld * m:]).all(), "written outside the ld x m output"
        T = h[start:start + ld * m].reshape(m, ld)
        assert np.isnan(T[:, n:]).all(), f"padding rows n <= i < ld written (n={n}, ld={ld}, key={key})"
        return key, T[:, :n].T


@pytest.fixture()
def dev(cg):
    d = Dev(cg)
    yield d
    d.close()
    cg.set_option("matrix_variant", 0)


def spec_of(cg, k):
    spec = cg.device_spec(k)
    assert spec is not None
    return spec, isinstance(spec, cg._ffi.covgram_kernel_composite)


class Tally:
    """Collects entrywise failures so that one test prints the figures of all its cases before it fails."""

    def __init__(self):
        self.fails = []

    def entries(self, name, dt, d, n, m, ld, key, got, ref, bound, note=""):
        w, i, j = mc.worst_entry(got, ref, bound)
        line = (f"matrix-entrywise {name} {np.dtype(dt).name} d={d} n={n} m={m} ld={ld} key={key}{note}: worst err/bound {w:.3f} at "
                f"({i}, {j}) got {got[i, j]!r} want {ref[i, j]!r}")
        print(line)
        if not w <= 1.0:
            self.fails.append(line)

    def same_bits(self, what, A, B):
        if not np.array_equal(A.view(np.uint8), B.view(np.uint8)):
            bad = np.argwhere(A != B)
            i, j = (int(v) for v in bad[0]) if len(bad) else (-1, -1)
            line = f"matrix-bitwise {what}: {len(bad)} entries differ, first at ({i}, {j}): {A[i, j]!r} vs {B[i, j]!r}"
            print(line)
            self.fails.append(line)
            return False
        return True

    def done(self):
        assert not self.fails, "\n".join(self.fails)


def bits(A):
    return np.ascontiguousarray(A)


GRID_KERNELS = ("2.5*Lengthscale(MaternP(2),1.3)", "EQ")
GRID_PAIRS = [(4, 65), (1028, 130), (2052, 64), (255, 63), (1, 1), (1024, 1), (3, 64), (256, 130), (1020, 65)]


# ---- 1. route x bucket x raggedness -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("d", [1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64])
def test_route_bucket_raggedness_grid(cg, dev, dt, d):
    """Both sides of every DM bucket ("full" d == DM and padded d < DM bodies), n around the VR multiples, the wave and the workgroup
    (256 rows; 1024 rows on the fp32 VR route), m around the 64-column strip."""
    kc = {c[0]: c for c in kernel_cases.cases(cg)}
    tally = Tally()
    for name in GRID_KERNELS:
        _, k, ko = kc[name]
        spec, comp = spec_of(cg, k)
        assert not comp
        for n, m in GRID_PAIRS:
            rng = np.random.default_rng(1000 * d + n + m)
            X, Y = mc.cloud(o, ko, rng, n, m, d, dt)
            key, M = dev.matrix(spec, dev.points(X), dev.points(Y), n, m, dt)
            assert key == expected_key(dt, d, n, n), (name, dt, d, n, m, key)
            ref, bound = mc.reference_and_bound(o, ko, X, Y, dt)
            tally.entries(name, dt, d, n, m, n, key, M, ref, bound)
            dev.close()
    tally.done()


# ---- 2. the VR gate from both sides -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("d", [3, 12])
def test_vr_gate_both_sides(cg, dev, dt, d):
    """ld = n (VR), ld = n + VR (VR, padding untouched under 16-byte stores), ld = n + 1 and an out one element off its 16-byte
    boundary (both fall back to one row per thread): the same template, the same arithmetic — the four results are bitwise equal."""
    kc = {c[0]: c for c in kernel_cases.cases(cg)}
    n, m, vr = 1028, 130, VRS[dt]
    tally = Tally()
    for name in GRID_KERNELS:
        _, k, ko = kc[name]
        spec, _ = spec_of(cg, k)
        X, Y = mc.cloud(o, ko, np.random.default_rng(77 + d), n, m, d, dt)
        hx, hy = dev.points(X), dev.points(Y)
        ref, bound = mc.reference_and_bound(o, ko, X, Y, dt)
        dm = bucket(d)
        res = []
        for ld, off, want, note in ((n, 0, 3 + 10 * dm + 1000 * vr, ""), (n + vr, 0, 3 + 10 * dm + 1000 * vr, ""),
                                    (n + 1, 0, 3 + 10 * dm + 1000, ""), (n, 1, 3 + 10 * dm + 1000, " out+1")):
            key, M = dev.matrix(spec, hx, hy, n, m, dt, ld=ld, offset=off)
            assert key == want, (name, dt, d, ld, off, key, want)
            tally.entries(name, dt, d, n, m, ld, key, M, ref, bound, note)
            res.append(bits(M))
        for t in (1, 2, 3):
            tally.same_bits(f"{name} {np.dtype(dt).name} d={d} gate variant 0 vs {t}", res[0], res[t])
    tally.done()


# ---- 3. the generic kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("d,variant", [(65, 0), (100, 0), (256, 0), (3, 1), (16, 1), (64, 1)])
def test_generic_kernels(cg, dev, dt, d, variant):
    """d > 64 (automatic) and option matrix_variant = 1: matrix_kernel (16-column strips) and matrix_expr_kernel for a composite."""
    kc = {c[0]: c for c in kernel_cases.cases(cg)}
    cases = [kc[name] for name in GRID_KERNELS] + [kernel_cases.composite_cases(cg)[0], kernel_cases.composite_cases(cg)[2]]
    tally = Tally()
    try:
        cg.set_option("matrix_variant", variant)
        for name, k, ko in cases:
            spec, comp = spec_of(cg, k)
            for n, m in ((1028, 130), (255, 17), (1, 1)):
                X, Y = (mc.wide_cloud if d > 64 else mc.cloud)(o, ko, np.random.default_rng(d + n), n, m, d, dt)
                key, M = dev.matrix(spec, dev.points(X), dev.points(Y), n, m, dt, ld=n + (n % 2))
                assert key == (2 if comp else 1) + 1000 == expected_key(dt, d, n, n, comp, variant), (name, dt, d, n, m, key)
                ref, bound = mc.reference_and_bound(o, ko, X, Y, dt)
                tally.entries(name, dt, d, n, m, n + (n % 2), key, M, ref, bound)
                dev.close()
    finally:
        cg.set_option("matrix_variant", 0)
    tally.done()


def family_cases(cg):
    """Every family of kernel_cases.cases, the NeuralNetwork kernel's device profile (ASINDOT on normalised points) and the composites."""
    return kernel_cases.cases(cg) + [("AsinDot", cg.AsinDot(), o.Kernel(o.ASINDOT))] + kernel_cases.composite_cases(cg)


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("d", [3, 20])
def test_register_kernel_bit_identical_to_generic(cg, dev, dt, d):
    """csrc/matrix.hip says of the register kernel: "same arithmetic in the same order (entries are bit-identical)" to the generic one."""
    n, m = 516, 130
    tally = Tally()
    try:
        for name, k, ko in family_cases(cg):
            spec, comp = spec_of(cg, k)
            if comp:
                continue
            X, Y = mc.cloud(o, ko, np.random.default_rng(300 + d), n, m, d, dt, unit_ball=name == "AsinDot")
            hx, hy = dev.points(X), dev.points(Y)
            res = []
            for variant in (0, 1):
                cg.set_option("matrix_variant", variant)
                key, M = dev.matrix(spec, hx, hy, n, m, dt)
                assert key == expected_key(dt, d, n, n, False, variant), (name, dt, d, variant, key)
                res.append(bits(M))
            tally.same_bits(f"{name} {np.dtype(dt).name} d={d} matrix_variant 0 vs 1", res[0], res[1])
            dev.close()
    finally:
        cg.set_option("matrix_variant", 0)
    tally.done()


# ---- 4. every family ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("d", [3, 12, 40])
def test_every_family_entrywise(cg, dev, dt, d):
    """n = 516, m = 130, ld = n (the VR route for single profiles at d <= 16) and ld = n + 1.  Isotropic clouds carry 8 rows 6..10
    lengthscales away and 4 rows of X copied from Y (s = 0 exactly: the Taylor guards of MaternP / Matern(nu), r = 0 of Matern(nu <= 1))."""
    n, m = 516, 130
    tally = Tally()
    for name, k, ko in family_cases(cg):
        spec, comp = spec_of(cg, k)
        X, Y = mc.cloud(o, ko, np.random.default_rng(400 + d), n, m, d, dt, unit_ball=name == "AsinDot")
        hx, hy = dev.points(X), dev.points(Y)
        ref, bound = mc.reference_and_bound(o, ko, X, Y, dt)
        for ld in (n, n + 1):
            key, M = dev.matrix(spec, hx, hy, n, m, dt, ld=ld)
            assert key == expected_key(dt, d, n, ld, comp), (name, dt, d, ld, key)
            tally.entries(name, dt, d, n, m, ld, key, M, ref, bound)
        dev.close()
    tally.done()


# ---- 5. one point set ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("d", [3, 12, 40])
def test_one_point_set_symmetric_bitwise(cg, dev, dt, d):
    """gramian(k, x): M == M.T bitwise ((x - y)^2 and the FMA's operand order make it exact; cholesky hands this tile to rocSOLVER), a
    constant diagonal for isotropic kernels, and the bound — on both matrix_variants."""
    kc = {c[0]: c for c in kernel_cases.cases(cg)}
    tally = Tally()
    try:
        for name in ("EQ", "RQ(1.0)", "MaternP(3)", "Dot()^3", "ExponentialDot"):
            _, k, ko = kc[name]
            spec, _ = spec_of(cg, k)
            for n in (260, 1028):
                X, _ = mc.cloud(o, ko, np.random.default_rng(500 + d + n), n, 8, d, dt)
                hx = dev.points(X)
                ref, bound = mc.reference_and_bound(o, ko, X, X, dt)
                for variant in (0, 1):
                    cg.set_option("matrix_variant", variant)
                    key, M = dev.matrix(spec, hx, hx, n, n, dt)
                    assert key == expected_key(dt, d, n, n, False, variant), (name, dt, d, n, variant, key)
                    tally.entries(name + " (x, x)", dt, d, n, n, n, key, M, ref, bound)
                    tally.same_bits(f"{name} {np.dtype(dt).name} d={d} n={n} variant={variant} M vs M.T", bits(M), bits(M.T))
                    if mc.is_iso(o, ko):
                        dg = np.ascontiguousarray(np.diag(M)).reshape(1, -1)
                        tally.same_bits(f"{name} {np.dtype(dt).name} d={d} n={n} variant={variant} diagonal", dg, np.full_like(dg, dg[0, 0]))
                dev.close()
    finally:
        cg.set_option("matrix_variant", 0)
    tally.done()


# ---- 6. sliced handles --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("d", [3, 5])
def test_sliced_handles(cg, dev, dt, d):
    """X = rows 3 .. 3 + 1028 of one parent, Y = rows 5 .. 5 + 130 of another: the slices' base pointers are not 16-byte aligned, and only
    out's alignment may gate the VR route.  Bitwise equal to the same call on fresh handles of the same rows."""
    kc = {c[0]: c for c in kernel_cases.cases(cg)}
    n, m = 1028, 130
    tally = Tally()
    for name in GRID_KERNELS:
        _, k, ko = kc[name]
        spec, _ = spec_of(cg, k)
        PX, PY = mc.cloud(o, ko, np.random.default_rng(600 + d), n + 9, m + 11, d, dt)
        itemsize = np.dtype(dt).itemsize
        assert (3 * d * itemsize) % 16 != 0 and (5 * d * itemsize) % 16 != 0
        hx = dev.slice(dev.points(PX), 3, n); hy = dev.slice(dev.points(PY), 5, m)
        X, Y = PX[3:3 + n], PY[5:5 + m]
        key, M = dev.matrix(spec, hx, hy, n, m, dt)
        assert key == 3 + 10 * bucket(d) + 1000 * VRS[dt], (name, dt, d, key)
        ref, bound = mc.reference_and_bound(o, ko, X, Y, dt)
        tally.entries(name + " sliced", dt, d, n, m, n, key, M, ref, bound)
        key2, M2 = dev.matrix(spec, dev.points(X), dev.points(Y), n, m, dt)
        assert key2 == key
        tally.same_bits(f"{name} {np.dtype(dt).name} d={d} sliced vs fresh handles", bits(M), bits(M2))
        dev.close()
    tally.done()


# ---- 7. host pointers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
def test_host_pointers_padding_untouched(cg, dev, dt):
    """loc = HOST with ldo = n + 3: the staged tile has ld = n (VR route); the 2-D copy back leaves the host padding rows untouched."""
    f, lib = cg._ffi, cg._ffi.lib()
    kc = {c[0]: c for c in kernel_cases.cases(cg)}
    n, m, d = 1028, 130, 3
    tally = Tally()
    for name in GRID_KERNELS:
        _, k, ko = kc[name]
        spec, _ = spec_of(cg, k)
        X, Y = mc.cloud(o, ko, np.random.default_rng(700), n, m, d, dt)
        hs = []
        for A in (X, Y):
            h = f._P()
            f.check(lib.covgram_points_create(dev.ctx.bind_stream(), C.byref(h), A.ctypes.data_as(C.c_void_p), A.shape[0], d,
                                              f.F64 if dt == F64 else f.F32, f.HOST))
            dev.keep.append((h, A))
            hs.append(h)
        ldo = n + 3
        out = np.full((m, ldo), np.nan, dtype=dt)
        f.check(lib.covgram_matrix(dev.ctx.bind_stream(), f.kref(spec), hs[0], hs[1], out.ctypes.data_as(C.c_void_p), ldo, f.HOST))
        key = cg.get_info("last_matrix_path")
        assert key == 3 + 10 * bucket(d) + 1000 * VRS[dt], (name, dt, key)
        assert np.isnan(out[:, n:]).all(), "host padding rows written"
        ref, bound = mc.reference_and_bound(o, ko, X, Y, dt)
        tally.entries(name + " host", dt, d, n, m, ldo, key, out[:, :n].T, ref, bound)
        dev.close()
    tally.done()


# ---- 8. what rests on it (Python API) -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
def test_indexing_and_diagonal_rest_on_matrix(cg, dev, dt):
    """G[i, j], sub-blocks, rows and columns against the same entries of the checked matrix: bitwise for isotropic kernels (the same
    arithmetic on the same points, whatever route the small tile takes), to the bound otherwise; diagonal(G) for EQ and Dot^2."""
    kc = {c[0]: c for c in kernel_cases.cases(cg)}
    n, m, d = 516, 130, 5
    tally = Tally()
    for name in ("EQ", "2.5*Lengthscale(MaternP(2),1.3)", "Matern(0.8)", "Dot()^3", "ExponentialDot"):
        _, k, ko = kc[name]
        iso = mc.is_iso(o, ko)
        X, Y = mc.cloud(o, ko, np.random.default_rng(800), n, m, d, dt)
        ref, bound = mc.reference_and_bound(o, ko, X, Y, dt)
        G = cg.gramian(k, torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())
        M = G.to_dense().cpu().numpy()
        key = cg.get_info("last_matrix_path")
        assert key == expected_key(dt, d, n, n), (name, dt, key)
        tally.entries(name + " to_dense", dt, d, n, m, n, key, M, ref, bound)

        def sub(what, got, rows, cols):
            got = np.asarray(got.cpu().numpy()).reshape(len(rows), len(cols))
            ix = np.ix_(rows, cols)
            if iso:
                tally.same_bits(f"{name} {np.dtype(dt).name} {what}", bits(got), bits(M[ix]))
            tally.entries(f"{name} {what}", dt, d, len(rows), len(cols), len(rows), cg.get_info("last_matrix_path"), got, ref[ix], bound[ix])

        sub("G[7, 129]", G[7, 129], [7], [129])
        sub("G[3:260, 60:70]", G[3:260, 60:70], list(range(3, 260)), list(range(60, 70)))
        sub("G[4:260, 1:66]", G[4:260, 1:66], list(range(4, 260)), list(range(1, 66)))
        sub("G[515, :]", G[515, :], [515], list(range(m)))
        sub("G[:, 64]", G[:, 64], list(range(n)), [64])
    for name, k, ko in (("EQ", cg.EQ(), o.Kernel(o.EQ)), ("Dot()^2", cg.Dot() ** 2, o.Kernel(o.DOT, power=2))):
        X, _ = mc.cloud(o, ko, np.random.default_rng(801), 300, 4, d, dt)
        dg = cg.diagonal(cg.gramian(k, torch.from_numpy(X).cuda())).cpu().numpy()
        ref, bound = mc.reference_and_bound(o, ko, X, X, dt)
        tally.entries(name + " diagonal", dt, d, 300, 1, 300, cg.get_info("last_matrix_path"), dg.reshape(-1, 1),
                      np.diag(ref).reshape(-1, 1), np.diag(bound).reshape(-1, 1))
    tally.done()


@pytest.mark.parametrize("dt", [F32, F64])
def test_pivot_column_equals_full_matrix_column(cg, dt):
    """The lazy pivoted Cholesky's column: Gramian(k, x, x[p:p+1]).to_dense() at n = 4097 is column p of the full matrix, bitwise."""
    n, d, p = 4097, 3, 1234
    ko = o.Kernel(o.EQ)
    X, _ = mc.cloud(o, ko, np.random.default_rng(900), n, 4, d, dt)
    Xt = torch.from_numpy(X).cuda()
    full = cg.gramian(cg.EQ(), Xt).to_dense()
    assert cg.get_info("last_matrix_path") == 3 + 10 * 4 + 1000                                # n odd: one row per thread
    col = cg.gramian(cg.EQ(), Xt, Xt[p:p + 1]).to_dense()
    assert cg.get_info("last_matrix_path") == 3 + 10 * 4 + 1000
    assert col.shape == (n, 1) and torch.equal(col[:, 0], full[:, p])
    ref, bound = mc.reference_and_bound(o, ko, X, X[p:p + 1], dt)
    tally = Tally()
    tally.entries("EQ pivot column", dt, d, n, 1, n, 1043, col.cpu().numpy(), ref, bound)
    tally.done()


# ---- 9. more strips than a grid's y extent (last: the largest outputs) --------------------------------------------------------------
@pytest.mark.parametrize("n,m,variant", [(4, 64 * 65536 + 70, 0), (2, 16 * 65536 + 20, 1)])
def test_more_strips_than_65535(cg, dev, n, m, variant):
    """include/covgram.h promises no limit on m: 65538 strips of 64 columns on the register (VR) kernel, 65538 strips of 16 on the
    generic one.  Reference on the last 4096 columns and 4096 random earlier ones."""
    dt, d = F32, 3
    k, ko = cg.Lengthscale(cg.EQ(), 2.0), o.Kernel(o.EQ, lengthscale=2.0)
    spec, _ = spec_of(cg, k)
    rng = np.random.default_rng(9)
    X = (0.8 * rng.standard_normal((n, d)) + 0.2).astype(dt); Y = (0.8 * rng.standard_normal((m, d))).astype(dt)
    tally = Tally()
    try:
        cg.set_option("matrix_variant", variant)
        buf = torch.full((m, n), float("nan"), dtype=torch.float32, device="cuda")
        rc = dev.lib.covgram_matrix(dev.ctx.bind_stream(), dev.f.kref(spec), dev.points(X), dev.points(Y), dev.f._P(buf.data_ptr()), n, dev.f.DEVICE)
        assert rc == 0, (rc, dev.lib.covgram_last_error())
        key = cg.get_info("last_matrix_path")
        assert key == (1001 if variant else 3 + 10 * 4 + 1000 * 4), key
        torch.cuda.synchronize()
        assert bool(torch.isfinite(buf).all()), "entries left unwritten"
        cols = np.concatenate([np.sort(rng.choice(m - 4096, size=4096, replace=False)), np.arange(m - 4096, m)])
        M = buf[torch.from_numpy(cols).cuda()].cpu().numpy().T
        ref, bound = mc.reference_and_bound(o, ko, X, Y[cols], dt)
        tally.entries(f"EQ l=2 m={m} (sampled columns)", dt, d, n, len(cols), n, key, M, ref, bound)
    finally:
        cg.set_option("matrix_variant", 0)
    tally.done()
