"""The raw batched CG step (covgram_bcg_step, and covgram_bcg_update + covgram_bcg_direction with a separate Z) on random X, R, P, AP, Z
against the restatement of tests/mbcg_ref.py — no MVM involved.

Shapes: n in {1, 3, 1023, 4097, the one-workgroup capacity, capacity + 1} plus 1024, 5000 and capacity + 8 (aligned columns below and
above the capacity: the one-launch kernel with 1, 2 and 4 register groups, and the 16-byte general path), nrhs in {1, 3, 33}, leading
dimension n and n + 5 (unaligned columns: the entry-by-entry general path; the padding must stay untouched), with and without diag,
Z = R and a separate Z.  Column 1 is inactive, columns 0 and 2 are equal, and with 33 columns column 5 is all zero and the odd columns
from 7 on carry a threshold that stops them.

Bounds, eps_T the vectors' machine epsilon: every vector entry is one fused multiply-add of T-valued operands with a scalar that is an
fp64 sum rounded to T, so |X - X_ref| <= 4 eps_T (|x| + |alpha p|) and the same form for R, P (and AP with diag), X_ref being the fp64
expression with the logged alpha (beta), which is itself held to the restatement's.  A scalar is an fp64 sum of
products of T values: relative error <= 8 eps_T sum|terms| / |value| for fp32 (the entries of the updated R may differ by an ulp from the
restatement's), 8 n 2^-53 sum|terms| / |value| for fp64."""
import ctypes as C

import numpy as np
import pytest
import torch

import mbcg_ref as mr

pytestmark = pytest.mark.gpu

CAP = {torch.float32: 16384, torch.float64: 8192}
NP = {torch.float32: np.float32, torch.float64: np.float64}


def _sizes(dt):
    c = CAP[dt]
    return [1, 3, 1023, 1024, 4097, 5000, c, c + 1, c + 8]


def _block(a, ld, dt, fill=7.5):
    """(n, p) numpy -> device (p, ld) buffer (column-major n x p with leading dimension ld), padding = fill."""
    n, p = a.shape
    buf = torch.full((p, ld), fill, dtype=dt, device="cuda")
    buf[:, :n] = torch.from_numpy(np.ascontiguousarray(a.T)).to(dt).cuda()
    return buf


def _inputs(n, p, dt, rng):
    f = NP[dt]
    X, R, P, AP, Z = (rng.standard_normal((n, p)).astype(f) for _ in range(5))
    diag = rng.uniform(0.5, 2.0, n).astype(f)
    rz = rng.uniform(0.5, 2.0, p) * n
    tol2 = np.zeros(p)
    active = np.ones(p)
    if p >= 3:
        active[1] = 0.0
        for a in (X, R, P, AP, Z):
            a[:, 2] = a[:, 0]
        rz[2] = rz[0]
    if p >= 33:
        for a in (X, R, P, AP, Z):
            a[:, 5] = 0.0
        rz[5] = 0.0
        tol2[7::2] = 1e30
    rr = np.einsum("ij,ij->j", R.astype(np.float64), R.astype(np.float64))
    iters = np.arange(p, dtype=np.float64)
    return X, R, P, AP, Z, diag, rz, tol2, rr, active, iters


def _run(cg, n, p, dt, ld, inp, use_diag, sep, it=2, rows=4):
    """One device step on fresh copies; returns the outputs as numpy."""
    X, R, P, AP, Z, diag, rz, tol2, rr, active, iters = inp
    f = cg._ffi
    lib, ctx = f.lib(), cg.get_ctx(torch.device("cuda", 0))
    bufs = {k: _block(v, ld, dt) for k, v in (("X", X), ("R", R), ("P", P), ("AP", AP), ("Z", Z))}
    d = torch.from_numpy(diag).cuda() if use_diag else None
    state = torch.zeros(p * (f.BCG_FIELDS + 2 * f.BCG_SLAB), dtype=torch.float64, device="cuda")
    for fld, v in ((f.BCG_RZ, rz), (f.BCG_TOL2, tol2), (f.BCG_RR, rr), (f.BCG_ACTIVE, active), (f.BCG_ITERS, iters)):
        state[fld * p:(fld + 1) * p] = torch.from_numpy(np.asarray(v, dtype=np.float64)).cuda()
    nact = torch.tensor([int(active.sum())], dtype=torch.int32, device="cuda")
    alog = torch.full((rows, p), -3.0, dtype=torch.float64, device="cuda")
    blog = torch.full((rows, p), -3.0, dtype=torch.float64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    code = f.F32 if dt == torch.float32 else f.F64
    if not sep:
        f.check(lib.covgram_bcg_step(ctx.bind_stream(), n, p, code, ptr(bufs["X"]), ld, ptr(bufs["R"]), ld, ptr(bufs["P"]), ld, ptr(bufs["AP"]), ld,
                                     ptr(d), ptr(state), ptr(nact), ptr(alog), ptr(blog), it))
    else:
        f.check(lib.covgram_bcg_update(ctx.bind_stream(), n, p, code, ptr(bufs["X"]), ld, ptr(bufs["R"]), ld, ptr(bufs["P"]), ld, ptr(bufs["AP"]), ld,
                                       ptr(d), ptr(state), ptr(alog), it))
        f.check(lib.covgram_bcg_direction(ctx.bind_stream(), n, p, code, ptr(bufs["R"]), ld, ptr(bufs["Z"]), ld, ptr(bufs["P"]), ld, ptr(state),
                                          ptr(nact), ptr(blog), it))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in bufs.items()}                     # (p, ld)
    st = state[:f.BCG_FIELDS * p].cpu().numpy().reshape(f.BCG_FIELDS, p)
    out.update(rz=st[f.BCG_RZ], tol2=st[f.BCG_TOL2], rr=st[f.BCG_RR], active=st[f.BCG_ACTIVE], iters=st[f.BCG_ITERS], n_active=int(nact),
               alog=alog.cpu().numpy(), blog=blog.cpu().numpy())
    return out


def _check(n, p, dt, ld, inp, use_diag, sep, out, it=2):
    X, R, P, AP, Z, diag, rz, tol2, rr, active, iters = inp
    f8 = np.float64
    eps = float(np.finfo(NP[dt]).eps)
    ref = mr.step(X, R, P, AP, Z if sep else None, diag if use_diag else None, rz, tol2, rr, active, iters, dtype=NP[dt])
    tag = f"n={n} p={p} {dt} ld={ld} diag={use_diag} sep={sep}"
    for k in ("X", "R", "P", "AP", "Z"):
        assert np.isfinite(out[k]).all(), f"{tag}: non-finite {k}"
        assert (out[k][:, n:] == 7.5).all(), f"{tag}: {k} written past n"
    got = {k: out[k][:, :n].T for k in ("X", "R", "P", "AP", "Z")}
    act = np.asarray(active, dtype=bool)
    APr = ref["AP"].astype(f8)
    # vectors: the fp64 expressions with the DEVICE's logged coefficients (which are held to the restatement's further down): an entry is a
    # fused multiply-add given its scalar, whereas the scalar itself may carry the summation-order error of a cancelling dot product
    al, be = out["alog"][it], out["blog"][it]
    x_ex = X.astype(f8) + al * P.astype(f8)
    r_ex = R.astype(f8) - al * APr
    z_in = Z.astype(f8) if sep else got["R"].astype(f8)          # (Z = R: the device's own updated R)
    p_ex = z_in + be * P.astype(f8)
    for k, ex, scale in (("X", x_ex, np.abs(X) + np.abs(al * P)), ("R", r_ex, np.abs(R) + np.abs(al * APr)),
                         ("P", p_ex, np.abs(z_in) + np.abs(be * P))):
        cols = act if k != "P" else np.ones(p, dtype=bool)
        err = np.abs(got[k].astype(f8) - ex)[:, cols]
        lim = 4 * eps * scale.astype(f8)[:, cols]
        assert (err <= lim).all(), f"{tag}: {k} off by {np.max(err / np.maximum(lim, 1e-300)):.3g} of the bound"
    if use_diag:
        ap_ex = AP.astype(f8) + diag.astype(f8)[:, None] * P.astype(f8)
        err = np.abs(got["AP"].astype(f8) - ap_ex)[:, act]
        assert (err <= 4 * eps * (np.abs(AP) + np.abs(diag[:, None] * P)).astype(f8)[:, act]).all(), f"{tag}: AP"
    else:
        assert np.array_equal(got["AP"], AP), f"{tag}: AP written without diag"
    assert np.array_equal(got["Z"], Z), f"{tag}: Z written"
    # scalars: alpha against the restatement (its gamma is a sum over the INPUTS); rr, rz and beta as sums over the device's own updated R,
    # which the lines above tie to the inputs — the restatement's R moves with its alpha, whose sum may cancel
    c = 8 * eps if dt == torch.float32 else 8 * n * 2.0 ** -53
    Rd = got["R"].astype(f8)
    Zd = Z.astype(f8) if sep else Rd
    rr_ex, rz_ex, arz_ex = (np.einsum("ij,ij->j", a, b) for a, b in ((Rd, Rd), (Rd, Zd), (np.abs(Rd), np.abs(Zd))))
    for j in range(p):
        if not act[j]:
            continue
        lim_rz = c * arz_ex[j] / max(abs(rz_ex[j]), 1e-300)
        for name, g, r, lim in (("alpha", out["alog"][it, j], ref["alpha"][j], c * ref["abs_gamma"][j] / max(abs(ref["gamma"][j]), 1e-300)),
                                ("rr", out["rr"][j], rr_ex[j], c),
                                ("rz", out["rz"][j], rz_ex[j], lim_rz),
                                ("beta", out["blog"][it, j], rz_ex[j] / rz[j] if rz[j] != 0 else 0.0, lim_rz + 2.0 ** -52)):
            if r == 0.0:
                assert g == 0.0, f"{tag}: column {j} {name} = {g}, expected 0"
            else:
                assert abs(g - r) <= lim * abs(r), f"{tag}: column {j} {name} = {g!r} against {r!r} (bound {lim:.3g})"
    assert np.array_equal(out["iters"], ref["iters"].astype(f8)), tag
    assert np.array_equal(out["active"] != 0, ref["active"]), tag
    assert out["n_active"] == int(ref["active"].sum()), tag
    assert np.array_equal(out["tol2"], tol2), tag
    rows = [r for r in range(out["alog"].shape[0]) if r != it]
    assert (out["alog"][rows] == -3.0).all() and (out["blog"][rows] == -3.0).all(), f"{tag}: a log row other than `it` was written"
    # column states
    if p >= 3:
        assert np.array_equal(got["X"][:, 1], X[:, 1]) and np.array_equal(got["R"][:, 1], R[:, 1]), f"{tag}: the inactive column moved"
        assert out["alog"][it, 1] == 0.0 and out["blog"][it, 1] == 0.0 and out["rz"][1] == rz[1] and out["rr"][1] == rr[1] and out["iters"][1] == 1.0
        for k in ("X", "R", "P"):
            assert np.array_equal(got[k][:, 0], got[k][:, 2]), f"{tag}: equal columns differ in {k}"
        for k in ("alog", "blog"):
            assert out[k][it, 0] == out[k][it, 2], tag
        assert out["rr"][0] == out["rr"][2] and out["rz"][0] == out["rz"][2]
    if p >= 33:
        for k in ("X", "R", "P"):
            assert (got[k][:, 5] == 0).all(), f"{tag}: the zero column moved in {k}"
        assert out["alog"][it, 5] == 0.0 and out["blog"][it, 5] == 0.0 and out["rr"][5] == 0.0 and out["active"][5] == 0.0
        assert (out["active"][7::2] == 0).all() and out["active"][6] == 1.0
    assert np.isfinite(out["alog"]).all() and np.isfinite(out["blog"]).all() and np.isfinite(out["rr"]).all() and np.isfinite(out["rz"]).all()


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("which", range(9))
def test_step(cg, dt, which):
    n = _sizes(dt)[which]
    rng = np.random.default_rng(4000 + n)
    for p in (1, 3, 33):
        inp = _inputs(n, p, dt, rng)
        for ld in (n, n + 5):
            for use_diag in (False, True):
                for sep in (False, True):
                    out = _run(cg, n, p, dt, ld, inp, use_diag, sep)
                    _check(n, p, dt, ld, inp, use_diag, sep, out)
                    if p == 33 and ld == n:                            # the call repeated on fresh copies: the same bits
                        again = _run(cg, n, p, dt, ld, inp, use_diag, sep)
                        for k, v in out.items():
                            assert np.array_equal(np.asarray(v), np.asarray(again[k])), f"n={n} {dt}: {k} differs between two runs"


def test_errors(cg):
    f = cg._ffi
    lib, ctx = f.lib(), cg.get_ctx(torch.device("cuda", 0))
    n, p = 10, 2
    t = torch.ones((p, n), dtype=torch.float64, device="cuda")
    state = torch.zeros(p * (f.BCG_FIELDS + 2 * f.BCG_SLAB), dtype=torch.float64, device="cuda")
    nact = torch.zeros(1, dtype=torch.int32, device="cuda")
    P = lambda x: C.c_void_p(x.data_ptr())

    def step(n_, p_, code, ld):
        return lib.covgram_bcg_step(ctx.bind_stream(), n_, p_, code, P(t), ld, P(t), ld, P(t), ld, P(t), ld, None, P(state), P(nact), None, None, 0)
    assert step(n, p, f.F64, n - 1) == f.EINVAL
    assert step(-1, p, f.F64, n) == f.EINVAL
    assert step(n, -1, f.F64, n) == f.EINVAL
    assert step(n, p, 7, n) == f.EINVAL
    assert lib.covgram_bcg_step(ctx.bind_stream(), n, p, f.F64, P(t), n, P(t), n, P(t), n, P(t), n, None, P(state), P(nact), None, None, -1) == f.EINVAL
    assert step(n, 0, f.F64, n) == f.OK and step(0, p, f.F64, 0) == f.OK
    assert lib.covgram_bcg_update(ctx.bind_stream(), n, p, f.F64, P(t), n, P(t), n - 1, P(t), n, P(t), n, None, P(state), None, 0) == f.EINVAL
    assert lib.covgram_bcg_update(ctx.bind_stream(), n, p, 2, P(t), n, P(t), n, P(t), n, P(t), n, None, P(state), None, 0) == f.EINVAL
    assert lib.covgram_bcg_update(ctx.bind_stream(), n, 0, f.F64, P(t), n, P(t), n, P(t), n, P(t), n, None, P(state), None, 0) == f.OK
    assert lib.covgram_bcg_direction(ctx.bind_stream(), n, p, f.F64, P(t), n, P(t), n, P(t), n - 1, P(state), P(nact), None, 0) == f.EINVAL
    assert lib.covgram_bcg_direction(ctx.bind_stream(), -2, p, f.F64, P(t), n, P(t), n, P(t), n, P(state), P(nact), None, 0) == f.EINVAL
    assert lib.covgram_bcg_direction(ctx.bind_stream(), n, 0, f.F64, P(t), n, P(t), n, P(t), n, P(state), P(nact), None, 0) == f.OK
    assert lib.covgram_bcg_init(ctx.bind_stream(), n, p, f.F64, P(t), n - 1, P(t), n, 1e-8, 0.0, P(state), P(nact)) == f.EINVAL
    assert lib.covgram_bcg_init(ctx.bind_stream(), n, p, 5, P(t), n, P(t), n, 1e-8, 0.0, P(state), P(nact)) == f.EINVAL
    assert lib.covgram_bcg_init(ctx.bind_stream(), n, 0, f.F64, P(t), n, P(t), n, 1e-8, 0.0, P(state), P(nact)) == f.OK
    torch.cuda.synchronize()
    assert bool((t == 1).all()) and bool((state == 0).all()) and int(nact) == 0          # nothing was launched


def test_init(cg):
    """covgram_bcg_init: rz, rr, the thresholds, the active flags and their count, fp32 vectors with fp64 scalars."""
    f = cg._ffi
    lib, ctx = f.lib(), cg.get_ctx(torch.device("cuda", 0))
    n, p, ld = 3001, 5, 3004
    rng = np.random.default_rng(77)
    R = rng.standard_normal((n, p)).astype(np.float32)
    Z = rng.standard_normal((n, p)).astype(np.float32)
    R[:, 2] = 0.0
    R[:, 3] *= 1e-3
    Rb, Zb = _block(R, ld, torch.float32), _block(Z, ld, torch.float32)
    state = torch.full((p * (f.BCG_FIELDS + 2 * f.BCG_SLAB),), -1.0, dtype=torch.float64, device="cuda")
    nact = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    f.check(lib.covgram_bcg_init(ctx.bind_stream(), n, p, f.F32, C.c_void_p(Rb.data_ptr()), ld, C.c_void_p(Zb.data_ptr()), ld, 1e-3, 0.5,
                                 C.c_void_p(state.data_ptr()), C.c_void_p(nact.data_ptr())))
    st = state[:f.BCG_FIELDS * p].cpu().numpy().reshape(f.BCG_FIELDS, p)
    R8, Z8 = R.astype(np.float64), Z.astype(np.float64)
    rr, rz = np.einsum("ij,ij->j", R8, R8), np.einsum("ij,ij->j", R8, Z8)
    arz = np.einsum("ij,ij->j", np.abs(R8), np.abs(Z8))
    tol2 = np.maximum(1e-6 * rr, 0.25)
    c = 8 * n * 2.0 ** -53
    assert np.all(np.abs(st[f.BCG_RR] - rr) <= c * rr) and np.all(np.abs(st[f.BCG_RZ] - rz) <= c * arz)
    assert np.all(np.abs(st[f.BCG_TOL2] - tol2) <= 2 * c * tol2)
    assert st[f.BCG_ACTIVE].tolist() == [1.0, 1.0, 0.0, 0.0, 1.0] and (st[f.BCG_ITERS] == 0).all()    # the zero column and one below abstol
    assert int(nact) == 3
