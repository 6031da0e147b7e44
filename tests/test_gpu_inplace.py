"""In-place MVMs: y sharing memory with a (mul!(x, G, x, alpha, beta)) on every product path.  include/covgram.h lets a and y overlap
in any way at every entry that takes both; the library then reads a from a private copy.  Each case pins its route (options in, info
keys out), runs the product twice out of place and asserts the two runs are bitwise equal, then runs it in place and asserts the result
equals the out-of-place one bitwise; where the size allows it also compares the in-place result with the fp64 oracle
alpha K a0 + beta a0 norm-wise and row-wise (test_gpu_fuzz.py's tolerances).  The large cases (n = 8192 fp32, 4096 fp64) give many
workgroups, so a kernel that writes y while other workgroups still read a would show there."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEFAULTS = {"dense_variant": 0, "jsplit": 0, "inkernel_reduce": -1, "mfma_sym": -1, "mfma_sym_rt": -1, "mfma_fuse_w": -1, "mfma_f16": -1,
            "mfma_lds": -1, "dense_sym": -1, "dense_bcast": -1, "sum_fused": -1, "composite_termwise": 1, "mfma_mrhs": -1, "grad_expand": -1,
            "grad_bcast": -1, "grad_keep_r": -1, "toeplitz_fused": 1}
ORACLE_MAX = 4_000_000          # n * m up to which a case is also checked against the oracle


@contextlib.contextmanager
def options(cg, **opts):
    try:
        for k, v in opts.items():
            cg.set_option(k, v)
        yield
    finally:
        for k in opts:
            cg.set_option(k, DEFAULTS[k])


def P(t):
    return C.c_void_p(t.data_ptr() if torch.is_tensor(t) else t.ctypes.data)


def route_errors(cg, what, expect):
    got = {k: cg.get_info(k) for k in expect}
    bad = {k: (got[k], v) for k, v in expect.items() if (got[k] <= 0 if v == ">0" else got[k] != v)}
    return [f"{what}: route {bad} (got, expected)"] if bad else []


def maxdiff(u, v):
    return float((u.double() - v.double()).abs().max()) if u.numel() else 0.0


def three_way(run, a0, what, y0=None):
    """run(a, y) computes into y.  Out of place twice (bitwise equal), then in place (y is a): bitwise equal to out of place.
    y0: y's contents before an out-of-place call (default a0, what an in-place call sees)."""
    y0 = a0 if y0 is None else y0
    y1 = y0.clone(); run(a0.clone(), y1)
    y2 = y0.clone(); run(a0.clone(), y2)
    x = a0.clone(); run(x, x)
    torch.cuda.synchronize()
    errs = []
    if not torch.equal(y1, y2):
        errs.append(f"{what}: out of place not bit-reproducible (max |diff| {maxdiff(y1, y2):.3e})")
    if not torch.equal(x, y1):
        errs.append(f"{what}: in place differs from out of place, max |diff| {maxdiff(x, y1):.3e} (|y| {float(y1.double().abs().max()):.3e})")
    return x, y1, errs


def oracle_errors(what, got, ref, scale, tol):
    got = np.asarray(got, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64); scale = np.asarray(scale, dtype=np.float64) + 1e-300
    errs = []
    if not np.isfinite(got).all():
        return [f"{what}: non-finite result"]
    nerr = np.linalg.norm(got - ref); nbound = tol * max(np.linalg.norm(ref), np.linalg.norm(scale) * 1e-2)
    if nerr > nbound:
        errs.append(f"{what}: oracle norm-wise {nerr / max(np.linalg.norm(ref), 1e-300):.3e} > {tol:g}")
    row = float(np.max(np.abs(got - ref) / scale)) if got.size else 0.0
    if row > tol:
        errs.append(f"{what}: oracle row-wise {row:.3e} > {tol:g}")
    return errs


def dense_ref(o, terms, X, Y, a, alpha, beta, const=0.0):
    """alpha (sum_t c_t K_t + const 1 1') a + beta a, and its row-wise scale alpha |K| |a| + beta |a|."""
    Xd, Yd, ad = (np.asarray(v, dtype=np.float64) for v in (X, Y, a))
    M = sum(c * o.matrix(kk, Xd, Yd) for c, kk in terms) + const
    absM = sum(abs(c) * np.abs(o.matrix(kk, Xd, Yd)) for c, kk in terms) + abs(const)
    return alpha * (M @ ad) + beta * ad, abs(alpha) * (absM @ np.abs(ad)) + abs(beta) * np.abs(ad)


def points(rng, n, d, dtype, scale=0.5):
    npd = np.float32 if dtype == torch.float32 else np.float64
    return (scale * rng.standard_normal((n, d))).astype(npd)


def tol_of(dtype, grad=False):
    if grad:
        return 2e-5 if dtype == torch.float32 else 1e-11
    return 1e-5 if dtype == torch.float32 else 1e-12


# --------------------------------------------------------------------------------------------------------------------------------------
# dense scalar covgram_mvm through the Python surface (Gramian.mul_ hands a and y to the C ABI as they are)
# --------------------------------------------------------------------------------------------------------------------------------------
def _dense_cases(cg, o):
    EQ, M2, EXP = o.Kernel(o.EQ), o.Kernel(o.MATERNP, p=2), o.Kernel(o.EXP)
    f32, f64 = torch.float32, torch.float64
    # (name, kernel, oracle terms, dtype, d, options, expected info, two point sets)
    return [
        ("lane32_js1", cg.EQ(), [(1.0, EQ)], f32, 3, dict(dense_variant=1, jsplit=1), dict(last_dense_path=1, last_jsplit=1), False),
        ("lane32_js8", cg.EQ(), [(1.0, EQ)], f32, 3, dict(dense_variant=1, jsplit=8, inkernel_reduce=0),
         dict(last_dense_path=1, last_jsplit=8, last_inkernel_reduce=0), False),
        ("lane32_ikr", cg.EQ(), [(1.0, EQ)], f32, 3, dict(dense_variant=1, jsplit=8, inkernel_reduce=1),
         dict(last_dense_path=1, last_jsplit=8, last_inkernel_reduce=1), False),
        ("lane64_js1", cg.EQ(), [(1.0, EQ)], f64, 3, dict(jsplit=1, dense_sym=0, dense_bcast=0), dict(last_dense_path=1, last_jsplit=1, last_dense_sym=0), False),
        ("lane64_js8", cg.EQ(), [(1.0, EQ)], f64, 3, dict(jsplit=8, dense_sym=0, dense_bcast=0, inkernel_reduce=0),
         dict(last_dense_path=1, last_jsplit=8, last_dense_sym=0), False),
        ("lane64_ikr", cg.EQ(), [(1.0, EQ)], f64, 3, dict(jsplit=8, dense_sym=0, dense_bcast=0, inkernel_reduce=1),
         dict(last_dense_path=1, last_inkernel_reduce=1), False),
        ("mfma_fuse1_f16", cg.EQ(), [(1.0, EQ)], f32, 3, dict(mfma_sym=0, mfma_fuse_w=1, mfma_f16=1, mfma_lds=1),
         dict(last_dense_path=2, last_mfma_sym=0, last_mfma_f16=1, last_mfma_lds=1), False),
        ("mfma_fuse0_bf16", cg.EQ(), [(1.0, EQ)], f32, 3, dict(mfma_sym=0, mfma_fuse_w=0, mfma_f16=0, mfma_lds=1),
         dict(last_dense_path=2, last_mfma_sym=0, last_mfma_f16=0, last_mfma_lds=1), False),
        ("mfma_fuse1_bf16", cg.EQ(), [(1.0, EQ)], f32, 3, dict(mfma_sym=0, mfma_fuse_w=1, mfma_f16=0, mfma_lds=1),
         dict(last_dense_path=2, last_mfma_sym=0, last_mfma_f16=0, last_mfma_lds=1), False),
        ("mfma_sym_rt1", cg.EQ(), [(1.0, EQ)], f32, 3, dict(mfma_sym=1, mfma_sym_rt=1), dict(last_dense_path=2, last_mfma_sym=1, last_mfma_sym_rt=1), False),
        ("mfma_sym_rt2", cg.EQ(), [(1.0, EQ)], f32, 3, dict(mfma_sym=1, mfma_sym_rt=2), dict(last_dense_path=2, last_mfma_sym=1, last_mfma_sym_rt=2), False),
        ("gen_sym_rt1", cg.MaternP(2), [(1.0, M2)], f32, 3, dict(mfma_sym=1, mfma_sym_rt=1), dict(last_dense_path=2, last_mfma_sym=1, last_mfma_sym_rt=1), False),
        ("gen_sym_rt2", cg.MaternP(2), [(1.0, M2)], f32, 3, dict(mfma_sym=1, mfma_sym_rt=2), dict(last_dense_path=2, last_mfma_sym=1, last_mfma_sym_rt=2), False),
        ("gen_nonsym", cg.MaternP(2), [(1.0, M2)], f32, 3, dict(), dict(last_dense_path=2, last_mfma_sym=0), True),
        ("wide_d65", cg.EQ(), [(1.0, EQ)], f32, 65, dict(), dict(last_dense_path=3), False),
        ("dot_factored", cg.Dot(), [(1.0, o.Kernel(o.DOT))], f32, 3, dict(), dict(last_dense_path=4), False),
        ("bcast64", cg.EQ(), [(1.0, EQ)], f64, 16, dict(dense_bcast=1, dense_sym=0), dict(last_dense_path=1, last_dense_bcast=1, last_dense_sym=0), False),
        ("bcast64_sym", cg.EQ(), [(1.0, EQ)], f64, 16, dict(dense_bcast=1, dense_sym=1), dict(last_dense_path=1, last_dense_bcast=1, last_dense_sym=1), False),
        ("sym64_exp", cg.Exp(), [(1.0, EXP)], f64, 3, dict(dense_sym=1, dense_bcast=0), dict(last_dense_path=1, last_dense_sym=1), False),
        ("sym32_exp", cg.Exp(), [(1.0, EXP)], f32, 3, dict(dense_sym=1), dict(last_dense_path=1, last_dense_sym=1), False),
    ]


def _dense_run(cg, o, case, n, alpha, beta, seed, oracle):
    name, k, terms, dtype, d, opts, info, two = case
    rng = np.random.default_rng(seed)
    Xh = points(rng, n, d, dtype, 0.5 if d < 60 else 0.12)
    Yh = points(rng, n, d, dtype, 0.5 if d < 60 else 0.12) if two else Xh
    X = torch.from_numpy(Xh).cuda()
    G = cg.gramian(k, X, torch.from_numpy(Yh).cuda()) if two else cg.gramian(k, X)
    a0 = torch.from_numpy(rng.standard_normal(n).astype(Xh.dtype)).cuda()
    what = f"{name} n={n} beta={beta}"
    if n < 2048:    # a forced column split is clamped to the columns there are (and no split, no in-kernel reduce)
        info = {k: v for k, v in info.items() if k not in ("last_jsplit", "last_inkernel_reduce")}
    with options(cg, **opts):
        x, _, errs = three_way(lambda a, y: cg.mul_(y, G, a, alpha, beta), a0, what)
        errs += route_errors(cg, what, info)
    if oracle:
        ref, sc = dense_ref(o, terms, Xh, Yh, a0.cpu().numpy(), alpha, beta)
        errs += oracle_errors(what, x.cpu().numpy(), ref, sc, tol_of(dtype))
    return errs


@pytest.mark.parametrize("idx", range(20))
def test_dense_in_place(cg, oracle, idx):
    case = _dense_cases(cg, oracle)[idx]
    dtype, d = case[3], case[4]
    big = 8192 if dtype == torch.float32 else 4096
    if d > 60:
        big = 2048
    errs = _dense_run(cg, oracle, case, big, 0.8, 0.0, 100 + idx, False)
    errs += _dense_run(cg, oracle, case, big, -0.6, 1.3, 200 + idx, False)
    for j, n in enumerate((1, 31, 257) if idx % 2 else (33, 257)):
        errs += _dense_run(cg, oracle, case, n, 0.7, (0.0, -1.1, 0.9)[j], 300 + idx * 7 + j, True)
    assert not errs, "\n".join(errs)


# --------------------------------------------------------------------------------------------------------------------------------------
# Sums and composites: the termwise split reads a again for every term after the first and for a Constant
# --------------------------------------------------------------------------------------------------------------------------------------
def _sum_cases(cg, o):
    L = cg.Lengthscale
    two = (1.5 * L(cg.MaternP(2), 0.9) + 0.5 * cg.EQ(), [(1.5, o.Kernel(o.MATERNP, p=2, lengthscale=0.9)), (0.5, o.Kernel(o.EQ))], 0.0)
    withc = (cg.EQ() + cg.Constant(0.3), [(1.0, o.Kernel(o.EQ))], 0.3)
    three = (L(cg.EQ(), 1.2) + 0.7 * cg.RQ(1.5) + 0.2 * cg.MaternP(1),
             [(1.0, o.Kernel(o.EQ, lengthscale=1.2)), (0.7, o.Kernel(o.RQ, param=1.5)), (0.2, o.Kernel(o.MATERNP, p=1))], 0.0)
    prod = (cg.EQ() * cg.RQ(1.5), None, 0.0)
    f32, f64 = torch.float32, torch.float64
    return [
        ("sum2_f32", two, f32, dict(mfma_sym=0), dict(last_sum_fused=0)),
        ("sum2_f64", two, f64, dict(), dict(last_sum_fused=0)),
        ("sum_const_f32", withc, f32, dict(), dict(last_sum_fused=0)),
        ("sum_const_f64", withc, f64, dict(), dict(last_sum_fused=0)),
        ("sum3_onepass", three, f32, dict(mfma_sym=0), dict(last_sum_fused=1, last_dense_path=2)),
        ("sum2_fused", two, f32, dict(mfma_sym=0, sum_fused=1), dict(last_sum_fused=1, last_dense_path=2)),
        ("sum2_interp_f64", two, f64, dict(composite_termwise=0), dict(last_sum_fused=0)),
        ("product_f32", prod, f32, dict(), dict(last_sum_fused=0)),
        ("product_f64", prod, f64, dict(), dict(last_sum_fused=0)),
    ]


def _prod_terms(o):
    return o.Composite(((o.Kernel(o.EQ), o.Kernel(o.RQ, param=1.5)),))


@pytest.mark.parametrize("idx", range(9))
def test_sum_in_place(cg, oracle, idx):
    o = oracle
    name, (k, terms, const), dtype, opts, info = _sum_cases(cg, o)[idx]
    errs = []
    for j, (n, alpha, beta) in enumerate(((8192 if dtype == torch.float32 else 4096, 1.0, 0.0), (4096, -0.7, 1.2), (257, 0.9, -0.8), (31, 1.0, 0.0))):
        rng = np.random.default_rng(400 + 10 * idx + j)
        Xh = points(rng, n, 3, dtype)
        G = cg.gramian(k, torch.from_numpy(Xh).cuda())
        a0 = torch.from_numpy(rng.standard_normal(n).astype(Xh.dtype)).cuda()
        what = f"{name} n={n} beta={beta}"
        with options(cg, **opts):
            x, _, e = three_way(lambda a, y: cg.mul_(y, G, a, alpha, beta), a0, what)
            errs += e + route_errors(cg, what, info)
        if n * n <= ORACLE_MAX:
            ah = a0.cpu().numpy().astype(np.float64)
            if terms is None:
                kc = _prod_terms(o)
                ref = alpha * o.mul(None, kc, Xh, Xh, ah) + beta * ah
                sc = abs(alpha) * (np.abs(o.matrix(kc, Xh, Xh)) @ np.abs(ah)) + abs(beta) * np.abs(ah)
            else:
                ref, sc = dense_ref(o, terms, Xh, Xh, ah, alpha, beta, const)
            errs += oracle_errors(what, x.cpu().numpy(), ref, sc, tol_of(dtype))
    assert not errs, "\n".join(errs)


# --------------------------------------------------------------------------------------------------------------------------------------
# raw C ABI: matrix right-hand sides (y == a, lda == ldy), host pointers, partial overlap
# --------------------------------------------------------------------------------------------------------------------------------------
def _abi(cg, G):
    f = cg._ffi
    return f, f.lib(), G._px.ctx.bind_stream(), f.kref(G._spec())


@pytest.mark.parametrize("dtype,nrhs,mrhs", [(torch.float32, 8, 1), (torch.float32, 7, 0), (torch.float64, 6, -1)])
def test_matrix_rhs_in_place(cg, oracle, dtype, nrhs, mrhs):
    o = oracle
    errs = []
    for n in (2000, 257):
        rng = np.random.default_rng(500 + n + nrhs)
        Xh = points(rng, n, 3, dtype)
        G = cg.gramian(cg.EQ(), torch.from_numpy(Xh).cuda())
        f, lib, ctx, kp = _abi(cg, G)
        for ld in (n, n + 5):
            for alpha, beta in ((1.0, 0.0), (-0.6, 1.4)):
                a0 = torch.from_numpy(rng.standard_normal((nrhs, ld)).astype(Xh.dtype)).cuda()     # column-major n x nrhs, leading dimension ld

                def run(a, y):
                    f.check(lib.covgram_mvm(ctx, kp, G._px.handle, G._py.handle, P(a), ld, P(y), ld, nrhs, alpha, beta, f.DEVICE))
                what = f"nrhs={nrhs} mrhs={mrhs} n={n} ld={ld} beta={beta}"
                with options(cg, mfma_mrhs=mrhs):
                    x, _, e = three_way(run, a0, what)
                    errs += e + route_errors(cg, what, {"last_dense_path": 2 if dtype == torch.float32 else 1})
                A = a0.cpu().numpy()[:, :n].T.astype(np.float64)
                ref, sc = dense_ref(o, [(1.0, o.Kernel(o.EQ))], Xh, Xh, A, alpha, beta)
                errs += oracle_errors(what, x.cpu().numpy()[:, :n].T, ref, sc, tol_of(dtype))
    assert not errs, "\n".join(errs)


def test_host_pointers_in_place(cg, oracle):
    """loc == HOST with the same host array as a and y: one plain kernel and one two-term Sum (each term used to re-stage a from the host
    array the previous term had already written)."""
    o = oracle
    errs = []
    two = (1.5 * cg.Lengthscale(cg.MaternP(2), 0.9) + 0.5 * cg.EQ(), [(1.5, o.Kernel(o.MATERNP, p=2, lengthscale=0.9)), (0.5, o.Kernel(o.EQ))])
    for name, (k, terms) in (("EQ", (cg.EQ(), [(1.0, o.Kernel(o.EQ))])), ("sum2", two)):
        for dtype in (torch.float32, torch.float64):
            n = 1500
            rng = np.random.default_rng(600)
            Xh = points(rng, n, 3, dtype)
            G = cg.gramian(k, torch.from_numpy(Xh).cuda())
            f, lib, ctx, kp = _abi(cg, G)
            for alpha, beta in ((1.0, 0.0), (0.8, -1.2)):
                a0 = rng.standard_normal(n).astype(Xh.dtype)
                outs = []
                for mode in ("oop", "oop", "inplace"):
                    a = a0.copy(); y = a if mode == "inplace" else a0.copy()
                    f.check(lib.covgram_mvm(ctx, kp, G._px.handle, G._py.handle, P(a), n, P(y), n, 1, alpha, beta, f.HOST))
                    outs.append(y.copy())
                what = f"host {name} {dtype} beta={beta}"
                if not np.array_equal(outs[0], outs[1]):
                    errs.append(f"{what}: out of place not bit-reproducible")
                if not np.array_equal(outs[2], outs[0]):
                    errs.append(f"{what}: in place differs from out of place, max |diff| {np.abs(outs[2] - outs[0]).max():.3e}")
                ref, sc = dense_ref(o, terms, Xh, Xh, a0, alpha, beta)
                errs += oracle_errors(what, outs[2], ref, sc, tol_of(dtype))
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("s", [1, 17])
def test_partial_overlap(cg, oracle, s):
    """One buffer of n + s entries: a = buf[:n], y = buf[s:s+n], and the other way round (y before a)."""
    o = oracle
    errs = []
    L = cg.Lengthscale
    cases = [("direct64", cg.EQ(), [(1.0, o.Kernel(o.EQ))], torch.float64, dict(dense_sym=0, dense_bcast=0), dict(last_dense_path=1)),
             ("mfma32", cg.EQ(), [(1.0, o.Kernel(o.EQ))], torch.float32, dict(mfma_sym=0, mfma_fuse_w=1), dict(last_dense_path=2, last_mfma_sym=0)),
             ("sum32", 1.5 * L(cg.MaternP(2), 0.9) + 0.5 * cg.EQ(), [(1.5, o.Kernel(o.MATERNP, p=2, lengthscale=0.9)), (0.5, o.Kernel(o.EQ))],
              torch.float32, dict(mfma_sym=0), dict(last_sum_fused=0))]
    n = 2000
    for name, k, terms, dtype, opts, info in cases:
        rng = np.random.default_rng(700 + s)
        Xh = points(rng, n, 3, dtype)
        G = cg.gramian(k, torch.from_numpy(Xh).cuda())
        f, lib, ctx, kp = _abi(cg, G)
        for a_first in (True, False):
            for alpha, beta in ((1.0, 0.0), (0.7, -1.3)):
                buf0 = torch.from_numpy(rng.standard_normal(n + s).astype(Xh.dtype)).cuda()
                ao, yo = (0, s) if a_first else (s, 0)
                what = f"overlap {name} s={s} a_first={a_first} beta={beta}"
                outs = []
                with options(cg, **opts):
                    for mode in ("oop", "oop", "inplace"):
                        if mode == "inplace":
                            buf = buf0.clone(); a, y = buf[ao:ao + n], buf[yo:yo + n]
                        else:   # separate buffers at the same offsets (same alignment of a and y)
                            a = buf0.clone()[ao:ao + n]; y = buf0.clone()[yo:yo + n]
                        f.check(lib.covgram_mvm(ctx, kp, G._px.handle, G._py.handle, P(a), n, P(y), n, 1, alpha, beta, f.DEVICE))
                        torch.cuda.synchronize()
                        outs.append(y.clone())
                    errs += route_errors(cg, what, info)
                if not torch.equal(outs[0], outs[1]):
                    errs.append(f"{what}: out of place not bit-reproducible")
                if not torch.equal(outs[2], outs[0]):
                    errs.append(f"{what}: in place differs from out of place, max |diff| {maxdiff(outs[2], outs[0]):.3e}")
                b0 = buf0.cpu().numpy().astype(np.float64)
                ah, yh = b0[ao:ao + n], b0[yo:yo + n]
                ref, sc = dense_ref(o, terms, Xh, Xh, ah, alpha, 0.0)
                ref = ref + beta * yh; sc = sc + abs(beta) * np.abs(yh)
                errs += oracle_errors(what, outs[2].cpu().numpy(), ref, sc, tol_of(dtype))
    assert not errs, "\n".join(errs)


# --------------------------------------------------------------------------------------------------------------------------------------
# covgram_grad_mvm / covgram_valgrad_mvm
# --------------------------------------------------------------------------------------------------------------------------------------
def _grad_cases(cg, o):
    L = cg.Lengthscale
    f32, f64 = torch.float32, torch.float64
    EQ = o.Kernel(o.EQ)
    sum2 = (1.5 * L(cg.MaternP(2), 0.9) + 0.5 * cg.EQ(),
            o.Composite(((o.Kernel(o.MATERNP, p=2, lengthscale=0.9, scale=1.5),), (o.Kernel(o.EQ, scale=0.5),))))
    withc = (cg.EQ() + cg.Constant(0.3), o.Composite(((o.Kernel(o.EQ),), (o.Kernel(o.CONSTANT, scale=0.3),))) if hasattr(o, "CONSTANT") else None)
    # (name, kernel, oracle kernel, dtype, d, value-gradient, nrhs, options, info)
    return [
        ("direct64", cg.EQ(), EQ, f64, 3, False, 1, dict(grad_expand=0), dict(last_grad_expand=0)),
        ("expanded64", cg.EQ(), EQ, f64, 3, False, 1, dict(grad_expand=1), dict(last_grad_expand=1)),
        ("expanded32", cg.EQ(), EQ, f32, 8, False, 1, dict(grad_expand=1), dict(last_grad_expand=1)),
        ("bcast64_d16", cg.EQ(), EQ, f64, 16, False, 1, dict(grad_expand=1, grad_bcast=1), dict(last_grad_bcast=">0")),
        ("wide_d65", cg.EQ(), EQ, f64, 65, False, 1, dict(), dict()),
        ("keep_r2", cg.MaternP(2), o.Kernel(o.MATERNP, p=2), f64, 5, False, 1, dict(grad_keep_r=2), dict()),
        ("nrhs2", cg.EQ(), EQ, f64, 3, False, 2, dict(grad_expand=0), dict(last_grad_expand=0)),
        ("nrhs2_val32", cg.RQ(1.5), o.Kernel(o.RQ, param=1.5), f32, 3, True, 2, dict(), dict()),
        ("dot3", cg.Dot() ** 3, o.Kernel(o.DOT, power=3), f64, 3, False, 1, dict(), dict()),
        ("sum2", sum2[0], sum2[1], f64, 3, False, 1, dict(), dict()),
        ("sum2_val", sum2[0], sum2[1], f32, 3, True, 1, dict(), dict()),
        ("sum_const_val", withc[0], withc[1], f64, 3, True, 1, dict(), dict()),
    ]


@pytest.mark.parametrize("idx", range(12))
def test_gradient_in_place(cg, oracle, idx):
    o = oracle
    name, k, ko, dtype, d, value, nrhs, opts, info = _grad_cases(cg, o)[idx]
    bd = d + 1 if value else d
    errs = []
    for j, (n, alpha, beta) in enumerate(((4096 if d <= 16 else 512, 1.0, 0.0), (1024 if d <= 16 else 256, -0.7, 1.2), (120, 0.9, 0.0), (33, 1.0, -0.8))):
        rng = np.random.default_rng(800 + 10 * idx + j)
        Xh = points(rng, n, d, dtype, 0.5 / np.sqrt(max(d / 3, 1)))
        G = cg.gramian((cg.ValueGradientKernel if value else cg.GradientKernel)(k), torch.from_numpy(Xh).cuda())
        f = cg._ffi; lib = f.lib()
        ctx = G.inner._px.ctx.bind_stream(); kp = f.kref(cg.device_spec(k))
        fn = lib.covgram_valgrad_mvm if value else lib.covgram_grad_mvm
        N = n * bd
        a0 = torch.from_numpy(rng.standard_normal((nrhs, N)).astype(Xh.dtype)).cuda()

        def run(a, y):
            f.check(fn(ctx, kp, G.inner._px.handle, G.inner._py.handle, P(a), N, P(y), N, nrhs, alpha, beta, f.DEVICE))
        what = f"grad {name} n={n} beta={beta}"
        with options(cg, **opts):
            x, _, e = three_way(run, a0, what)
            errs += e + route_errors(cg, what, info)
        if n <= 120 and ko is not None:
            mul = o.valgrad_mul if value else o.grad_mul
            Mfull = (o.valgrad_matrix if value else o.grad_matrix)(ko, Xh.astype(np.float64))
            A = a0.cpu().numpy().astype(np.float64)
            for c in range(nrhs):
                ref = mul(A[c], ko, Xh, Xh, A[c], alpha, beta)
                sc = abs(alpha) * (np.abs(Mfull) @ np.abs(A[c])) + abs(beta) * np.abs(A[c])
                errs += oracle_errors(f"{what} col {c}", x.cpu().numpy()[c], ref, sc, tol_of(dtype, grad=True))
    assert not errs, "\n".join(errs)


# --------------------------------------------------------------------------------------------------------------------------------------
# structured products: Toeplitz, Kronecker, low rank
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
def test_toeplitz_in_place(cg, oracle, fused):
    o = oracle
    errs = []
    for n in (65536, 257):
        rng = np.random.default_rng(900 + n + fused)
        xs = np.linspace(-1, 1, n)
        vc = np.exp(-np.abs(xs - xs[0]) / 0.3); vr = np.exp(-np.abs(xs - xs[0]) / 0.2) * 0.9; vr[0] = vc[0]
        vcirc = np.exp(-np.minimum(np.arange(n), n - np.arange(n)) / (0.1 * n))
        for kind in ("sym", "gen", "circ"):
            with options(cg, toeplitz_fused=fused):
                if kind == "sym":
                    T = cg.SymmetricToeplitz(torch.from_numpy(vc).cuda()); v1, v2, circ = vc, None, False
                elif kind == "gen":
                    T = cg.Toeplitz(torch.from_numpy(vc).cuda(), torch.from_numpy(vr).cuda()); v1, v2, circ = vc, vr, False
                else:
                    T = cg.Circulant(torch.from_numpy(vcirc).cuda()); v1, v2, circ = vcirc, None, True
                for alpha, beta in ((1.0, 0.0), (-0.5, 1.5)):
                    a0 = torch.from_numpy(rng.standard_normal(n)).cuda()
                    what = f"toeplitz {kind} fused={fused} n={n} beta={beta}"
                    x, _, e = three_way(lambda a, y: cg.mul_(y, T, a, alpha, beta), a0, what)
                    errs += e
                    ah = a0.cpu().numpy()
                    ref = o.toeplitz_mul(ah, v1, v2, ah, alpha, beta, circulant=circ)
                    err = np.linalg.norm(x.cpu().numpy() - ref) / np.linalg.norm(ref)
                    if err > 1e-10:
                        errs.append(f"{what}: oracle rel-err {err:.3e}")
            del T
    assert not errs, "\n".join(errs)


def _kron_cases():
    f32, f64 = torch.float32, torch.float64
    # (name, factor sides, dtype, nrhs, bit of last_kron_path that must be set, bits that must be clear)
    return [
        ("q1_mode", [(256, 256)], f32, 4, 4, 8),
        ("q1_blas", [(1024, 1024)], f32, 2, 8, 0),
        ("q2_pair", [(96, 96), (96, 96)], f64, 64, 1, 16),
        ("q2_merged", [(12, 12), (16, 16)], f32, 512, 16, 1),
        ("q3", [(16, 16), (32, 32), (32, 32)], f32, 4, 2, 0),
        ("q2_blas", [(1024, 1024), (4, 4)], f64, 1, 8, 0),
    ]


@pytest.mark.parametrize("idx", range(6))
def test_kron_in_place(cg, oracle, idx):
    o = oracle
    name, sides, dtype, nrhs, must, mustnot = _kron_cases()[idx]
    rng = np.random.default_rng(1000 + idx)
    npd = np.float32 if dtype == torch.float32 else np.float64
    Fs = [(rng.standard_normal((r, c)) / np.sqrt(c)).astype(npd) for r, c in sides]
    Fd = [torch.from_numpy(np.ascontiguousarray(F.T)).cuda() for F in Fs]       # column-major r x c
    q = len(Fs)
    f = cg._ffi; lib = f.lib(); ctx = cg.get_ctx().bind_stream()
    ptrs = (f._P * q)(*[f._P(F.data_ptr()) for F in Fd])
    rows = (C.c_int64 * q)(*[r for r, _ in sides]); cols = (C.c_int64 * q)(*[c for _, c in sides]); lds = (C.c_int64 * q)(*[r for r, _ in sides])
    N = int(np.prod([c for _, c in sides]))
    code = f.F32 if dtype == torch.float32 else f.F64
    errs = []
    for alpha, beta in ((1.0, 0.0), (0.6, -1.1)):
        a0 = torch.from_numpy(rng.standard_normal((nrhs, N)).astype(npd)).cuda()

        def run(a, y):
            f.check(lib.covgram_kron_mvm(ctx, ptrs, rows, cols, lds, q, code, P(a), N, P(y), N, nrhs, alpha, beta, f.DEVICE))
        what = f"kron {name} beta={beta}"
        x, _, e = three_way(run, a0, what)
        errs += e
        path = cg.get_info("last_kron_path")
        if not (path & must) or (path & mustnot):
            errs.append(f"{what}: route last_kron_path = {path}")
        A = a0.cpu().numpy().astype(np.float64); got = x.cpu().numpy()
        for c in range(min(nrhs, 3)):
            ref = o.kron_mul(A[c], Fs, A[c], alpha, beta)
            err = np.linalg.norm(got[c] - ref) / np.linalg.norm(ref)
            if err > (1e-5 if dtype == torch.float32 else 1e-12):
                errs.append(f"{what} col {c}: oracle rel-err {err:.3e}")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("r,dtype,nrhs", [(32, torch.float64, 1), (300, torch.float64, 1), (16, torch.float32, 8), (64, torch.float32, 3)])
def test_lowrank_in_place(cg, oracle, r, dtype, nrhs):
    o = oracle
    errs = []
    npd = np.float32 if dtype == torch.float32 else np.float64
    f = cg._ffi; lib = f.lib(); ctx = cg.get_ctx().bind_stream()
    code = f.F32 if dtype == torch.float32 else f.F64
    for n in (1 << 17, 257):
        rng = np.random.default_rng(1100 + r + n)
        U = (rng.standard_normal((n, r)) / np.sqrt(n)).astype(npd); V = (rng.standard_normal((n, r)) / np.sqrt(r)).astype(npd)
        Ud = torch.from_numpy(np.ascontiguousarray(U.T)).cuda(); Vd = torch.from_numpy(np.ascontiguousarray(V.T)).cuda()
        for alpha, beta in ((1.0, 0.0), (-0.8, 1.3)):
            a0 = torch.from_numpy(rng.standard_normal((nrhs, n)).astype(npd)).cuda()

            def run(a, y):
                f.check(lib.covgram_lowrank_mvm(ctx, P(Ud), n, P(Vd), n, n, n, r, code, P(a), n, P(y), n, nrhs, alpha, beta, f.DEVICE))
            what = f"lowrank r={r} nrhs={nrhs} n={n} beta={beta}"
            x, _, e = three_way(run, a0, what)
            errs += e
            A = a0.cpu().numpy().astype(np.float64); got = x.cpu().numpy()
            for c in range(min(nrhs, 3)):
                ref = o.lowrank_mul(A[c], U, V, A[c], alpha, beta)
                sc = abs(alpha) * (np.abs(U.astype(np.float64)) @ (np.abs(V.astype(np.float64)).T @ np.abs(A[c]))) + abs(beta) * np.abs(A[c])
                errs += oracle_errors(f"{what} col {c}", got[c], ref, sc, 1e-5 if dtype == torch.float32 else 1e-12)
    assert not errs, "\n".join(errs)


# --------------------------------------------------------------------------------------------------------------------------------------
# covgram_mvm_sym_partial (rank 0 of world 1 is the whole product)
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_sym_partial_in_place(cg, oracle, dtype):
    o = oracle
    errs = []
    for n in ((8192 if dtype == torch.float32 else 4096), 257):
        rng = np.random.default_rng(1200 + n)
        Xh = points(rng, n, 3, dtype)
        G = cg.gramian(cg.EQ(), torch.from_numpy(Xh).cuda())
        a0 = torch.from_numpy(rng.standard_normal(n).astype(Xh.dtype)).cuda()
        what = f"sym_partial {dtype} n={n}"
        with options(cg, mfma_sym=1, dense_bcast=0):     # fp32: the symmetric matrix-core kernel below its automatic size
            assert G.sym_partial_supported(1)
            x, _, e = three_way(lambda a, y: G.sym_partial_(y, a, 0, 1), a0, what)
            errs += e
            errs += route_errors(cg, what, {"last_dense_path": 2, "last_mfma_sym": 1} if dtype == torch.float32 else {"last_dense_path": 1, "last_dense_sym": 1})
        if n * n <= ORACLE_MAX:
            ref, sc = dense_ref(o, [(1.0, o.Kernel(o.EQ))], Xh, Xh, a0.cpu().numpy(), 1.0, 0.0)
            errs += oracle_errors(what, x.cpu().numpy(), ref, sc, tol_of(dtype))
    assert not errs, "\n".join(errs)


# --------------------------------------------------------------------------------------------------------------------------------------
# Python operators
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_python_operators_in_place(cg, oracle, dtype):
    o = oracle
    errs = []
    n = 1500
    rng = np.random.default_rng(1300)
    Xh = points(rng, n, 3, dtype)
    X = torch.from_numpy(Xh).cuda()
    G = cg.gramian(cg.MaternP(2), X)
    K = o.matrix(o.Kernel(o.MATERNP, p=2), Xh.astype(np.float64), Xh.astype(np.float64))
    s2 = torch.from_numpy(rng.uniform(0.1, 0.5, n).astype(Xh.dtype)).cuda()
    dx = torch.from_numpy(rng.uniform(0.5, 1.5, n).astype(Xh.dtype)).cuda(); dy = torch.from_numpy(rng.uniform(0.5, 1.5, n).astype(Xh.dtype)).cuda()
    s2h, dxh, dyh = (t.cpu().numpy().astype(np.float64) for t in (s2, dx, dy))
    ops = [("G+s2I", G + s2, K + np.diag(s2h)), ("s2I+G", s2 + G, K + np.diag(s2h)),
           ("G+0.3+s2I", G + torch.full((n,), 0.3, dtype=dtype, device="cuda") + s2, K + np.diag(0.3 + s2h)),
           ("scaled", cg.ScaledOperator(dx, G, dy), dxh[:, None] * K * dyh[None, :]),
           ("fill", cg.Fill(0.7, n, n, dtype, X.device), np.full((n, n), 0.7)),
           ("fill+G", cg.Fill(0.7, n, n, dtype, X.device) + G, K + 0.7)]
    for name, A, M in ops:
        for alpha, beta in ((1.0, 0.0), (0.6, -1.4)):
            a0 = torch.from_numpy(rng.standard_normal(n).astype(Xh.dtype)).cuda()
            what = f"{name} beta={beta}"
            x, _, e = three_way(lambda a, y: cg.mul_(y, A, a, alpha, beta), a0, what)
            errs += e
            ah = a0.cpu().numpy().astype(np.float64)
            errs += oracle_errors(what, x.cpu().numpy(), alpha * (M @ ah) + beta * ah, abs(alpha) * (np.abs(M) @ np.abs(ah)) + abs(beta) * np.abs(ah),
                                  tol_of(dtype))
    # block Gramian (covgram_grad_mvm) and Kronecker of two lazy Gramians (covgram_kron_mvm) through their Python mul_
    B = cg.gramian(cg.GradientKernel(cg.EQ()), X[:200])
    Mb = o.grad_matrix(o.Kernel(o.EQ), Xh[:200].astype(np.float64))
    g1 = torch.from_numpy(points(rng, 48, 2, dtype)).cuda(); g2 = torch.from_numpy(points(rng, 40, 2, dtype)).cuda()
    Kp = cg.KroneckerProduct(cg.gramian(cg.EQ(), g1), cg.gramian(cg.MaternP(1), g2))
    Mk = np.kron(o.matrix(o.Kernel(o.EQ), g1.cpu().numpy().astype(np.float64)), o.matrix(o.Kernel(o.MATERNP, p=1), g2.cpu().numpy().astype(np.float64)))
    for name, A, M, tl in (("block", B, Mb, tol_of(dtype, grad=True)), ("kron", Kp, Mk, tol_of(dtype))):
        for alpha, beta in ((1.0, 0.0), (0.6, -1.4)):
            a0 = torch.from_numpy(rng.standard_normal(M.shape[0]).astype(Xh.dtype)).cuda()
            what = f"{name} beta={beta}"
            x, _, e = three_way(lambda a, y: cg.mul_(y, A, a, alpha, beta), a0, what)
            errs += e
            ah = a0.cpu().numpy().astype(np.float64)
            ref = alpha * (M @ ah) + beta * ah
            err = np.linalg.norm(x.cpu().numpy() - ref) / np.linalg.norm(ref)
            if err > tl:
                errs.append(f"{what}: oracle rel-err {err:.3e}")
    assert not errs, "\n".join(errs)
