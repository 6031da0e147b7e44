"""Kronecker MVM kernels (csrc/kron.hip, csrc/kron_kernels.hpp) ENTRY BY ENTRY against the oracle's mode products
(oracle/covgram_oracle.py::kron_mul, the identity KroneckerProducts 1.1.1 implements for the operators src/algebra.jl:91-95 and
src/separable.jl:33-42 build) and the bound of tests/kron_ref.py, on every route of the planner and every template arm of the kernels.

The case table lives in tests/kron_ref.py; what each case reaches is what its plan() says, and every run here asserts the library's own
record of what it launched (info keys "last_kron_path" and "last_kron_arms") against that plan computed for the chip's CU count — a case
cannot silently stop reaching the kernel it is here for.  On the MI355X (256 CUs):

    fused last-two-modes pass   128^3 (<8,8,VEC>, after one mode pass) and the "pair..." cases: all eight <NB1, NB2, VEC> arms in both dtypes,
                                ragged strips and strip groups, 1 .. 129 slab rows (less than one chunk, exactly one, rounds of the
                                register sets that are not whole), K2 and N2 at 48 / 64 / 65 / 128 / 129 / 257 (one to three output chunks),
                                129 and 160 slabs from right-hand sides (the slab >= pre exit; the pair as the only pass, applying
                                alpha / beta), the pair first when it shrinks the tensor
    NOT the fused pass          64^3, 32^3, 20/36/52, 7/130/96, 9/33/200, 3/48/300, 2/120/16, 40/100, 500/17/23: too few slabs or a side
                                below 48 — these run mode by mode (kron_mode_kernel, then kron_modet_kernel)
    single-mode kernels         all twelve <NBP, NW, VEC> arms of kron_mode_kernel (post = 2, 3, 17, 31, ... 65536) and all eight
                                <NBB, NW, VEC> arms of kron_modet_kernel (q = 1, c_q > 128, too few slabs, pre up to 262144)
    multiplied-out pair         16^4, 16^5, the tiny q = 5 case, 8^3 with right-hand sides
    rocBLAS                     a side >= 1024 with post > 1 and post = 1; a side of 256 with 2.1e9 flops (blas-mid)

plus misaligned a and y (views one element into a buffer: the scalar arms through alignment alone), matrix right-hand sides staged
and in place, padded leading dimensions with host and device pointers through the raw ABI (an odd ld of the last factor: the scalar arm
of the fused pass through the leading dimension alone), argument errors, and the full-size lazy-grid properties.  Every product runs
(alpha, beta) = (1, 0) into a NaN-filled y — twice, bit for bit — and (-0.7, 1.3) into a random one; `worst err/bound` is printed per case
(-s)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import kron_ref as kr

pytestmark = pytest.mark.gpu

F32, F64 = kr.F32, kr.F64
TDT = {F32: torch.float32, F64: torch.float64}


def relerr(b, ref):
    b = np.asarray(b, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    den = np.linalg.norm(ref)
    return np.linalg.norm(b - ref) / (den if den > 0 else 1.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def reference(tag, dt):
    """Inputs of a case and the fp64 operator applications its wants and bounds are made of: computed once, shared, read-only."""
    case = kr.BY_TAG[tag]
    Fs, a, y0 = kr.inputs(case, dt)
    cache = {}
    kr.want_and_bound(Fs, a, y0, 1.0, 0.0, dt, cache)
    for x in Fs + [a, y0, cache["t"], cache["tabs"]]:
        x.setflags(write=False)
    return Fs, a, y0, cache


def judge(name, shapes, nrhs, y, want, bound, pl, dev, norm_tol):
    """Every entry of a device result against want and bound, and the whole result norm-wise against norm_tol (both compared on the
    device); returns (worst err / bound, message or None)."""
    if not bool(torch.isfinite(y).all()):
        return float("inf"), f"{name}: {int((~torch.isfinite(y)).sum())} entries are not finite; plan {kr.describe(pl)}"
    want, bound = to_device(want, dev), to_device(bound, dev)
    assert tuple(y.shape) == tuple(want.shape)
    err = (y.double() - want).abs()
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, 0.0, float("inf"))).reshape(-1)
    i = int(torch.argmax(r))
    worst = float(r[i])
    den = float(torch.linalg.vector_norm(want))
    e = float(torch.linalg.vector_norm(y.double() - want)) / (den if den > 0 else 1.0)
    if e > norm_tol:
        return worst, f"{name}: ||got - want|| / ||want|| = {e:.3g} > {norm_tol:.3g} (worst entry err/bound {worst:.3g}); plan {kr.describe(pl)}"
    if worst <= 1:
        return worst, None
    return worst, (f"{name}: worst entry {i} = (o_1..o_q[, column]) {kr.coordinates(i, shapes, nrhs)}: got {float(y.reshape(-1)[i])!r} want "
                   f"{float(want.reshape(-1)[i])!r} err/bound {worst:.3g}; {int((r > 1).sum())} of {r.numel()} entries over the bound; plan {kr.describe(pl)}")


def to_device(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)         # (a copy: the shared references are read-only)


def device_vector(x, dev, offset):
    """x on the device; offset: as a view that starts one element into its buffer (not 16-byte, in fp32 not 8-byte aligned)."""
    if not offset:
        return to_device(x, dev)
    buf = torch.empty(x.shape[0] + 1, dtype=TDT[x.dtype.type], device=dev)
    v = buf[1:]
    v.copy_(to_device(x, dev))
    assert v.data_ptr() % 16 != 0 and v.data_ptr() % 8 == (0 if x.dtype == np.float64 else 4)
    return v


def run_tag(cg, dev, tag, dt, offset=False, inplace_layout=False, label=""):
    """One case on the device: route and arms against plan(), both (alpha, beta) entry by entry, the first product twice.
    offset: a and y one element into their buffers (vectors only).  inplace_layout: a matrix y whose memory is column-major
    (y.t() contiguous: the layout the binding passes on as it is) instead of torch's row-major (which it stages through a copy).  Returns the list of failures."""
    case = kr.BY_TAG[tag]
    Fs, a, y0, cache = reference(tag, dt)
    name = f"{dt.__name__} {tag}{label} {case.shapes} nrhs={case.nrhs}"
    pl = kr.plan(case.shapes, dt, case.nrhs, cg.get_info("num_cus"), a_aligned=not offset)
    Kp = cg.kronecker(*[to_device(Fm, dev) for Fm in Fs])
    assert tuple(Kp.shape) == (y0.shape[0], a.shape[0])
    assert not (offset and case.nrhs), "matrix right-hand sides are staged into aligned memory"
    ad = device_vector(a, dev, offset)

    def fresh(fill):
        if case.nrhs and inplace_layout:
            y = torch.empty((case.nrhs, y0.shape[0]), dtype=TDT[dt], device=dev).t()
            y.copy_(to_device(fill, dev))
            assert y.t().is_contiguous()            # the condition under which the binding hands y's own memory to the library
            return y
        return device_vector(fill, dev, offset)

    errs, worst, outs = [], 0.0, []
    for al, be in kr.ALPHA_BETA + (kr.ALPHA_BETA[0],):
        y = fresh(np.full(y0.shape, np.nan, dtype=dt) if be == 0 else y0)       # beta == 0: previous contents are not read (src/gramian.jl:80)
        cg.mul_(y, Kp, ad, al, be)
        path, arms = cg.get_info("last_kron_path"), cg.get_info("last_kron_arms")
        if (path, arms) != (pl.path, pl.arms):
            errs.append(f"{name} ({al}, {be}): last_kron_path = {path}, last_kron_arms = {arms:#x}; plan has {pl.path}, {pl.arms:#x}: {kr.describe(pl)}")
        outs.append(y)
    if not torch.equal(outs[2], outs[0]):
        errs.append(f"{name}: two identical calls differ in {int((outs[2] != outs[0]).sum())} entries")
    for (al, be), y in zip(kr.ALPHA_BETA, outs):
        want, bound = kr.want_and_bound(Fs, a, y0, al, be, dt, cache, merged=bool(pl.path & kr.PATH_MERGED))
        w, msg = judge(f"{name} ({al}, {be})", case.shapes, case.nrhs, y, want, bound, pl, dev, kr.norm_tol(case.shapes, dt))
        worst = max(worst, w)
        if msg:
            errs.append(msg)
    print(f"kron {dt.__name__} {tag}{label}: worst err/bound {worst:.3f}   [{kr.describe(pl)}]")
    return errs


def run_tags(cg, dev, tags, dt, **kw):
    errs = []
    for tag in tags:
        if dt in kr.BY_TAG[tag].dts:
            errs += run_tag(cg, dev, tag, dt, **kw)
    assert not errs, "\n".join(errs)


# every case of tests/kron_ref.py::CASES belongs to one of these groups (asserted below)
PAIR_TAGS = ["128^3", "64^3", "32^3", "16^4", "20,36,52", "7,130,96", "9,33,200", "3,48,300", "40,100", "500,17,23", "2,120,16"] + \
            [c.tag for c in kr.CASES if c.tag.startswith("pair") and not c.nrhs]
SINGLE_TAGS = ["37x41", "200x513", "1x1", "16x4", "30,50", "129,129", "5,3x260", "64,256", "q5-tiny", "1,9,4", "256,256", "5,33,40", "300x200", "32^4", "16^5",
               "separable"] + [c.tag for c in kr.CASES if c.tag.startswith(("mode", "modet")) and not c.nrhs]
RHS_TAGS = [c.tag for c in kr.CASES if c.nrhs and c.tag != "blas-mid"]
BLAS_TAGS = ["1024,24", "12,1100", "blas-mid"]
assert sorted(PAIR_TAGS + SINGLE_TAGS + RHS_TAGS + BLAS_TAGS) == sorted(kr.BY_TAG), set(kr.BY_TAG) ^ set(PAIR_TAGS + SINGLE_TAGS + RHS_TAGS + BLAS_TAGS)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_kron_pair_kernel_shapes(cg, dev, dt):
    """The fused pass arm by arm, and the shapes around its gates that run mode by mode (module docstring)."""
    run_tags(cg, dev, PAIR_TAGS, dt)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_kron_single_mode_kernels(cg, dev, dt):
    run_tags(cg, dev, SINGLE_TAGS, dt)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_kron_matrix_right_hand_sides(cg, dev, dt):
    """Y = (F1 x ... x Fq) A: the columns are one more leading tensor index (src/gramian.jl:89-99 shape of mul!).  Fused-pass routes
    (pair-slabs129, pair-only) and mode routes; then one of each with Y as column-major memory, the layout the binding passes to the
    library without a staging copy."""
    run_tags(cg, dev, RHS_TAGS, dt)
    pair = "pair-slabs129-f64" if dt == np.float64 else "pair-slabs129-f32"
    assert kr.plan(kr.BY_TAG[pair].shapes, dt, 129, cg.get_info("num_cus")).path == kr.PATH_PAIR
    assert kr.plan(kr.BY_TAG["30,50-rhs4"].shapes, dt, 4, cg.get_info("num_cus")).path == kr.PATH_MODE | kr.PATH_MODET
    run_tags(cg, dev, [pair, "30,50-rhs4"], dt, inplace_layout=True, label=" (column-major y)")


MISALIGNED_TAGS = ["128^3", "3,48,300", "pair-first-aligned", "pair-first-f64", "pair-first-f32", "mode<8,8>", "mode-NBP8", "300x200", "16x4", "16^5", "64^3"]


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_kron_misaligned_vectors(cg, dev, dt):
    """a and y as views that start one element into their buffers: the first pass takes its scalar arm through alignment alone (the
    fused pass when it runs first, the mode kernel, the last-mode kernel for q = 1), every later pass reads the aligned workspace."""
    ncu = cg.get_info("num_cus")
    first = lambda pl: next(p for p in pl.passes if p.kernel != "merged")       # (the multiplied-out pair reads the factors, not a)
    lost = []
    for tag in MISALIGNED_TAGS:
        c = kr.BY_TAG[tag]
        if dt in c.dts:
            al, mis = kr.plan(c.shapes, dt, 0, ncu), kr.plan(c.shapes, dt, 0, ncu, a_aligned=False)
            assert first(mis).arm is None or not first(mis).arm[2]
            assert mis.passes[mis.passes.index(first(mis)) + 1:] == al.passes[al.passes.index(first(al)) + 1:]
            if first(al).arm is not None and first(al).arm[2]:
                lost.append(first(al).kernel)
    # each kernel loses its vector arm through alignment alone (the fused pass: where the CU count lets it run first, 256 CUs among them)
    pair_first = any(kr.plan(kr.BY_TAG[t].shapes, dt, 0, ncu).pair_first for t in MISALIGNED_TAGS if dt in kr.BY_TAG[t].dts)
    assert {"mode", "modet"} <= set(lost) and (("pair" in lost) == pair_first) and (pair_first or ncu != 256), lost
    run_tags(cg, dev, MISALIGNED_TAGS, dt, offset=True, label=" (misaligned)")


def raw_abi_case(cg, dev, shapes, p, ldpad, last_kernel):
    """covgram_kron_mvm with padded lds / lda / ldy, host and device pointers; the padding of Y must come back untouched.
    last_kernel: the kernel of the last pass.  Its vector arm needs even leading dimensions: with host pointers the factors are packed
    (ld = rows), with device pointers the odd padded ld of the last factor alone must switch the fused pass to its scalar arm."""
    rng = np.random.default_rng(14)
    f = cg._ffi; lib = f.lib()
    ctx = cg.get_ctx(dev).bind_stream()
    q = len(shapes)
    Fs = [rng.standard_normal(s) for s in shapes]
    nin = int(np.prod([s[1] for s in shapes])); nout = int(np.prod([s[0] for s in shapes]))
    lda, ldy = nin + 5, nout + 2
    A = rng.standard_normal((p, lda)); Y = rng.standard_normal((p, ldy)); Y0 = Y.copy()
    lds = [s[0] + ldpad for s in shapes]
    bufs = []
    for Fm, ld in zip(Fs, lds):
        b = np.full((Fm.shape[1], ld), np.nan); b[:, :Fm.shape[0]] = Fm.T
        bufs.append(b)
    P = lambda arr: arr.ctypes.data_as(C.c_void_p)
    rows = (C.c_int64 * q)(*[s[0] for s in shapes]); cols = (C.c_int64 * q)(*[s[1] for s in shapes]); ldarr = (C.c_int64 * q)(*lds)
    al, be = 0.5, 2.0
    want, bound = kr.want_and_bound(Fs, A[:, :nin].T, Y0[:, :nout].T, al, be, F64)
    ncu = cg.get_info("num_cus")
    # host pointers: the factors are packed on the way to the device (ld = rows, 256-byte aligned), a and y too
    pl = kr.plan(shapes, F64, p, ncu)
    assert pl.passes[-1].kernel == last_kernel and pl.passes[-1].arm[2], kr.describe(pl)
    ptrs = (f._P * q)(*[P(b) for b in bufs])
    f.check(lib.covgram_kron_mvm(ctx, ptrs, rows, cols, ldarr, q, f.F64, P(A), lda, P(Y), ldy, p, al, be, f.HOST))
    assert (cg.get_info("last_kron_path"), cg.get_info("last_kron_arms")) == (pl.path, pl.arms), kr.describe(pl)
    w1, msg = judge(f"raw ABI host {shapes}", shapes, p, torch.from_numpy(np.ascontiguousarray(Y[:, :nout].T)).to(dev), want, bound, pl, dev, 1e-13)
    assert msg is None, msg
    assert np.array_equal(Y[:, nout:], Y0[:, nout:])
    # device pointers: the factors as they are (padded lds); padded a and y with several columns are packed in the workspace
    pl = kr.plan(shapes, F64, p, ncu, lds=lds)
    assert lds[-1] % 2 == 1 and pl.passes[-1].kernel == last_kernel and pl.passes[-1].arm[2] == (last_kernel != "pair"), kr.describe(pl)
    dbufs = [torch.from_numpy(b).to(dev) for b in bufs]
    Ad = torch.from_numpy(A).to(dev); Yd = torch.from_numpy(Y0.copy()).to(dev)
    ptrs = (f._P * q)(*[f._P(b.data_ptr()) for b in dbufs])
    f.check(lib.covgram_kron_mvm(ctx, ptrs, rows, cols, ldarr, q, f.F64, f._P(Ad.data_ptr()), lda, f._P(Yd.data_ptr()), ldy, p, al, be, f.DEVICE))
    assert (cg.get_info("last_kron_path"), cg.get_info("last_kron_arms")) == (pl.path, pl.arms), kr.describe(pl)
    w2, msg = judge(f"raw ABI device {shapes}", shapes, p, Yd[:, :nout].t().contiguous(), want, bound, pl, dev, 1e-13)
    assert msg is None, msg
    assert torch.equal(Yd[:, nout:].cpu(), torch.from_numpy(Y0[:, nout:]))
    print(f"kron raw ABI {shapes}: worst err/bound host {w1:.3f}, device {w2:.3f}")
    return f, lib, ctx, ptrs, rows, cols, ldarr, Ad, Yd, lda, ldy, nin, p


def test_kron_raw_abi_padded_leading_dimensions(cg, dev):
    """Device and host pointers, padded lds / lda / ldy, through the C ABI itself: a mode-route shape, and a fused-pass shape whose K2 and
    N2 are vector-aligned while ld3 = 131 is odd — with device pointers the fused pass runs its scalar arm through the leading dimension
    alone, with host pointers (packed factors) the vector arm."""
    f, lib, ctx, ptrs, rows, cols, ldarr, Ad, Yd, lda, ldy, nin, p = raw_abi_case(
        cg, dev, [(5, 6), (33, 20), (40, 70)], 3, 3, "modet")
    # argument errors are reported, not executed
    assert lib.covgram_kron_mvm(ctx, ptrs, rows, cols, ldarr, 3, f.F64, f._P(Ad.data_ptr()), nin - 1, f._P(Yd.data_ptr()), ldy, p, 1.0, 0.0, f.DEVICE) == f.EINVAL
    assert lib.covgram_kron_mvm(ctx, ptrs, rows, cols, ldarr, 0, f.F64, f._P(Ad.data_ptr()), lda, f._P(Yd.data_ptr()), ldy, p, 1.0, 0.0, f.DEVICE) == f.EINVAL
    # 3 x 128 slabs in two strip groups: the fused pass on any chip of up to 1536 CUs (units = 768 >= num_cus / 2)
    raw_abi_case(cg, dev, [(128, 2), (70, 40), (128, 128)], 3, 3, "pair")


def test_kron_large_factor_takes_the_library_gemm(cg, dev):
    """A factor side >= 1024 is a compute-bound dense GEMM, and so is one >= 256 with 2e9 flops in its mode (blas-mid, the one larger
    case: 4096 x 1024 right-hand sides): rocBLAS for that mode, the hand-written kernels for the others."""
    for dt in (np.float64, np.float32):
        for tag in BLAS_TAGS:
            c = kr.BY_TAG[tag]
            assert kr.plan(c.shapes, dt, c.nrhs, cg.get_info("num_cus")).path & kr.PATH_BLAS
        run_tags(cg, dev, BLAS_TAGS, dt)


def test_kron_paths_by_shape(cg, dev):
    """Which kernels a shape runs (info key "last_kron_path", round 4 — csrc/kron.hip sent shapes its kernels refuse to rocBLAS silently):
    bit 1 = fused last-two-modes pass, 2 = single-mode kernel, 4 = last-mode kernel, 8 = rocBLAS, 16 = two small trailing factors multiplied
    out.  The README case and everything GP-sized stays on the hand-written kernels; only compute-bound modes reach the library."""
    expect = [("128^3", 1 | 2), ("64^3", 2 | 4),          # 64 slabs are too few for the fused pass: mode by mode
              ("32^4", None), ("16^5", None), ("40,100", None),
              ("300x200", 4), ("1024,24", None), ("256,256", None)]
    for tag, want in expect:
        shapes = kr.BY_TAG[tag].shapes
        errs = run_tag(cg, dev, tag, np.float64)
        assert not errs, "\n".join(errs)
        path = cg.get_info("last_kron_path")
        assert path != 0
        big = any(max(sh) >= 1024 for sh in shapes)
        assert bool(path & 8) == big, (shapes, path)            # rocBLAS exactly for the factor sides >= 1024 among these shapes
        if want is not None:
            assert path == want, (shapes, path, want)


def test_kron_lazy_grid_full_size_properties(cg, oracle):
    """README.md:205-210's case (128^3 grid, three 128 x 128 Gramians) at full size: linearity and the transpose identity
    <u, K v> = <K^T u, v> (size-independent), plus 64 entries of K a against explicit rows of the Kronecker matrix."""
    rng = np.random.default_rng(16)
    ax = torch.linspace(0, 1, 128, dtype=torch.float64, device="cuda")
    G = cg.gramian(cg.separable("*", cg.Exp(), cg.EQ(), cg.MaternP(2)), cg.LazyGrid(ax, ax, ax))
    N = 128 ** 3
    u = torch.from_numpy(rng.standard_normal(N)).cuda(); v = torch.from_numpy(rng.standard_normal(N)).cuda()
    Gu, Gv = G @ u, G @ v
    assert relerr((G @ (2.0 * u - 3.0 * v)).cpu().numpy(), (2.0 * Gu - 3.0 * Gv).cpu().numpy()) <= 1e-13
    lhs = float(torch.dot(u, Gv)); rhs = float(torch.dot(Gu, v))      # the factors are symmetric Gramians
    assert abs(lhs - rhs) <= 1e-11 * max(abs(lhs), 1.0)
    xs = np.linspace(0, 1, 128)
    F = [oracle.matrix(oracle.Kernel(fam, **kw), xs, xs) for fam, kw in ((oracle.EXP, {}), (oracle.EQ, {}), (oracle.MATERNP, {"p": 2}))]
    vh = v.cpu().numpy().reshape(128, 128, 128)
    got = Gv.cpu().numpy()
    for idx in rng.integers(0, N, 64):
        i, j, k = idx // 16384, (idx // 128) % 128, idx % 128
        ref = np.einsum("a,b,c,abc->", F[0][i], F[1][j], F[2][k], vh)
        assert abs(got[idx] - ref) <= 1e-12 * max(abs(ref), 1.0)
