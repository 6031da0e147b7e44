"""Row-wise parity of the gradient and value-gradient block MVMs (covgram_grad_mvm / covgram_valgrad_mvm, csrc/block_mvm.hip:
grad_mvm_impl) on every kernel route, each pinned by the info keys last_grad_path / last_grad_jsplit / last_grad_expand /
last_grad_bcast before its numbers are checked.

Error measure.  For every checked entry (i, l) of the output,  e = |b - ref| / (|alpha| absref + |beta| |y0|)  with absref =
covgram_oracle.grad_absmul / valgrad_absmul: sum_j sum_k |block_ij[l, k]| |a_j[k]| bounded as the kernels form it (k1 a_l and
the rank-one term apart) — the condition denominator of that entry as a dot product.  A norm-wise check cannot see a wrong
block row whose entries are small (a test point far from the cloud) or an error confined to a ragged tail; this one can.
  * fp64: e <= 1e-12;  fp32: e <= 1e-5 (BASELINE.json's contracts).
  * Both are divided by max(1, L_i / 10), L_i = -ln(max_j k(x_i, y_j) / k(0)) (dot product: max_j |x_i . y_j|): the profile's
    exp has condition number L in its argument, as tests/test_gpu_parity.py: rowwise_err allows for the value kernels.
  * Expanded form (grad_mvm.hpp, "Expanded form"; only on the rows that ran it): s = |x'|^2 + |y'|^2 - 2 x'.y' is a difference of
    terms of up to P_i = gamma^2 max(|x_i - c|^2, max_j |y_j - c|^2) (c = the column side's centre, the quantity the radius gates
    GRAD_EXPAND_GATE = 1000 / GRAD_EXPAND_GATE_F32 = 128 bound), so it carries an ABSOLUTE error of a few roundings of P_i
    (csrc/common.hpp, the matrix-core gate's comment: ~3 u P per entry with every rounding aligned).  For EQ, d ln k1 / ds =
    d ln k2 / ds = -1/2 (scaled s), so the coefficients k1, k2 of every block carry a relative error <= (1/2) 6 u P_i = 3 u P_i;
    t = x'.a - y'.a and r_l = x'_l - y'_l are differences of the same kind, whose rounding scales with |x' - c| + |y' - c| instead
    of |r|: absref is then taken about the centre (grad_absmul(..., centre=c)).  Bound: tol + 3 u P_i, u = 2^-53 / 2^-24.
    (fp32 at its gate: 1e-5 + 3 * 6e-8 * 128 = 3.3e-5; fp64 at its gate: 1e-12 + 3.3e-13.)

References are computed on a ROW SUBSET (first and last block rows, the ragged tail, every row of one lane-per-row workgroup,
32 random rows, the far rows) with the C oracle (isotropic / dot-product gradient) or the numpy oracle; one seed per route."""
import math

import numpy as np
import pytest
import torch

import c_oracle

pytestmark = pytest.mark.gpu

TOL = {np.float32: 1e-5, np.float64: 1e-12}
UNIT = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
NANV = float("nan")


def centre(P, dt):
    """The column side's centre as the library computes it (csrc/dense_mfma.hip: points_max_norm2): the mean of up to 1024
    evenly spaced points, rounded to the data's precision."""
    n = P.shape[0]
    ns = min(n, 1024)
    return P[::n // ns][:ns].astype(np.float64).mean(axis=0).astype(dt).astype(np.float64)


def row_subset(n, wg, rng, extra=()):
    rows = {0, n - 1}
    rows.update(range(n - n % 64 if n % 64 else max(0, n - 64), n))                      # the ragged tail (or the last wave)
    w0 = wg if n >= 2 * wg else 0
    rows.update(range(w0, min(n, w0 + wg)))                                               # one full workgroup
    rows.update(int(r) for r in rng.choice(n, size=min(n, 32), replace=False))
    rows.update(extra)
    return np.array(sorted(rows), dtype=np.int64)


def add_far(X, rng, count, lscale=1.0):
    """`count` test points 6 to 10 lengthscales from the cloud (their every block entry is tiny)."""
    Xf = X.copy()
    d = X.shape[1]
    idx = rng.choice(X.shape[0], size=count, replace=False)
    for i, r in zip(idx, np.linspace(6.0, 10.0, count)):
        v = rng.standard_normal(d); v /= np.linalg.norm(v)
        Xf[i] = X.mean(axis=0) + (np.abs(X - X.mean(axis=0)).max() + r * lscale) * v
    return Xf, [int(i) for i in idx]


def cond_L(o, ko, Xs, Y):
    Xs = Xs.astype(np.float64); Y = Y.astype(np.float64)
    if ko.trait == o.ISOTROPIC:
        s = (Xs ** 2).sum(1)[:, None] + (Y ** 2).sum(1)[None, :] - 2 * Xs @ Y.T
        smin = np.maximum(s.min(axis=1), 0.0)
        with np.errstate(divide="ignore"):
            return np.maximum(0.0, -np.log(np.abs(o.profile(ko, smin)) / abs(float(o.profile(ko, np.zeros(1))[0]))))
    return np.abs(Xs @ Y.T).max(axis=1)


def references(o, ko, X, Y, a, rows, dt, vg, expanded):
    """(ref, absref) on the checked rows; absref about the column side's centre for the expanded form."""
    d = X.shape[1]; bd = d + vg
    Xs = X[rows].astype(np.float64); Yd = Y.astype(np.float64); ad = a.astype(np.float64)
    if not vg and isinstance(ko, o.Kernel):
        ref = c_oracle.grad_mvm(ko, Xs, Yd, ad)
    else:
        ref = (o.valgrad_mul if vg else o.grad_mul)(None, ko, Xs, Yd, ad, chunk=8)
    c = centre(Y, dt) if expanded else None
    absref = (o.valgrad_absmul if vg else o.grad_absmul)(ko, Xs, Yd, ad, centre=c, chunk=8)
    return ref.reshape(-1, bd), absref.reshape(-1, bd)


def rowwise(o, ko, X, Y, refs, b, y0, alpha, beta, rows, dt, vg, expanded=False, gamma2=1.0):
    """max over the checked entries of e / bound (<= 1 passes), the worst row and its error."""
    bd = X.shape[1] + vg
    ref, absref = refs
    Xs = X[rows].astype(np.float64); Yd = Y.astype(np.float64)
    got = b.reshape(-1, bd)[rows].astype(np.float64)
    yb = np.zeros_like(got) if beta == 0 else y0.reshape(-1, bd)[rows].astype(np.float64)
    want = alpha * ref + beta * yb
    den = abs(alpha) * absref + abs(beta) * np.abs(yb)
    if expanded:
        c = centre(Y, dt)
        P = gamma2 * np.maximum(((Xs - c) ** 2).sum(1), ((Yd - c) ** 2).sum(1).max())
        bound = TOL[dt] + 3 * UNIT[dt] * P
    else:
        bound = np.full(len(rows), TOL[dt])
    bound = bound * np.maximum(1.0, cond_L(o, ko, Xs, Yd) / 10.0)
    assert np.all(np.isfinite(got)), "non-finite output"
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(den > 0, np.abs(got - want) / den, np.abs(got - want))   # an all-zero entry must come out zero
    worst = (e / bound[:, None]).max(axis=1)
    i = int(np.argmax(worst))
    return float(worst[i]), int(rows[i]), float(e[i].max())


def run_route(cg, o, *, dt, k, ko, X, Y, opts, path, vg_forms=(0, 1), expand=0, bcast=0, jsplit=None, nrhs=1, wg=64,
              extra_rows=(), gamma2=1.0, seed=0):
    """Both products (alpha, beta != 0 on a random y; beta = 0 on a NaN-filled y) for gradient and value-gradient blocks."""
    rng = np.random.default_rng(seed)
    n, d = X.shape; m = Y.shape[0]
    Xt = torch.from_numpy(X).cuda(); Yt = torch.from_numpy(Y).cuda()
    rows = row_subset(n, wg, rng, extra_rows)
    try:
        for key, v in opts.items():
            cg.set_option(key, v)
        for vg in vg_forms:
            bd = d + vg
            G = cg.gramian((cg.ValueGradientKernel if vg else cg.GradientKernel)(k), Xt, Yt)
            shape = (m * bd,) if nrhs == 1 else (m * bd, nrhs)
            a = rng.standard_normal(shape).astype(dt)
            y0 = rng.standard_normal((n * bd,) + shape[1:]).astype(dt)
            refs = [references(o, ko, X, Y, a if nrhs == 1 else a[:, c], rows, dt, vg, bool(expand)) for c in range(nrhs)]
            for alpha, beta in ((-0.7, 1.3), (1.6, 0.0)):
                yt = torch.from_numpy(y0.copy()).cuda() if beta != 0 else torch.full((n * bd,) + shape[1:], NANV, dtype=Xt.dtype, device="cuda")
                G.mul_(yt, torch.from_numpy(a).cuda(), alpha, beta)
                got = {key: cg.get_info(key) for key in ("last_grad_path", "last_grad_expand", "last_grad_bcast", "last_grad_jsplit")}
                want = dict(last_grad_path=path, last_grad_expand=expand, last_grad_bcast=bcast)
                if jsplit is not None:
                    want["last_grad_jsplit"] = jsplit[vg] if isinstance(jsplit, tuple) else jsplit
                assert {kk: got[kk] for kk in want} == want, (vg, got, want)
                b = yt.cpu().numpy()
                for c in range(nrhs):
                    bc = b if nrhs == 1 else b[:, c]
                    yc = y0 if nrhs == 1 else y0[:, c]
                    worst, row, e = rowwise(o, ko, X, Y, refs[c], bc, yc, alpha, beta, rows, dt, vg, expanded=bool(expand), gamma2=gamma2)
                    assert worst <= 1.0, (vg, alpha, beta, c, "row", row, "error", e, "of its bound x", worst)
    finally:
        for key in opts:
            cg.set_option(key, -1 if key in ("grad_expand", "grad_bcast", "grad_keep_r") else 0)


def cloud(rng, n, d, dt, scale=1.0, shift=0.0):
    return (scale * rng.standard_normal((n, d)) + shift).astype(dt)


F32, F64 = np.float32, np.float64
DIRECT = dict(grad_expand=0, grad_bcast=0)


# ---------------------------------------------------------------------------------------------------------------- lane-per-row
@pytest.mark.parametrize("d", [1, 3, 17, 48])
def test_fp64_lane_per_row_direct_differences_with_far_rows(cg, oracle, d):
    """grad_expand = 0: direct differences; m = 211 < 4 x 64 columns: a column split of 3 and the slab reduce (bit 32)."""
    o = oracle
    rng = np.random.default_rng(100 + d)
    X, far = add_far(cloud(rng, 300, d, F64), rng, 4)
    Y = cloud(rng, 211, d, F64, 0.9, 0.1)
    k, ko = (cg.EQ(), o.Kernel(o.EQ)) if d != 17 else (cg.Lengthscale(cg.MaternP(2), 1.3), o.Kernel(o.MATERNP, p=2, lengthscale=1.3))
    run_route(cg, o, dt=F64, k=k, ko=ko, X=X, Y=Y, opts=DIRECT, path=1 | 32, wg=256 if d < 48 else 64, extra_rows=far, seed=d)


def test_fp64_expanded_scalar_stream(cg, oracle):
    o = oracle
    rng = np.random.default_rng(201)
    X, far = add_far(cloud(rng, 333, 12, F64), rng, 3)
    Y = cloud(rng, 190, 12, F64)
    run_route(cg, o, dt=F64, k=1.5 * cg.EQ(), ko=o.Kernel(o.EQ, scale=1.5), X=X, Y=Y, opts=dict(grad_expand=1, grad_bcast=0),
              path=1 | 32, expand=1, wg=256, extra_rows=far, seed=1)


@pytest.mark.parametrize("d,waves", [(16, 1), (41, 4)])
def test_fp64_broadcast_kernel_ragged_rows(cg, oracle, d, waves):
    """grad_bcast = 1 / 4 waves per workgroup; n = 333 is not a multiple of 64 or 256 rows."""
    o = oracle
    rng = np.random.default_rng(300 + d)
    X, far = add_far(cloud(rng, 333, d, F64), rng, 3)
    Y = cloud(rng, 201, d, F64, 1.0, 0.05)
    run_route(cg, o, dt=F64, k=cg.EQ(), ko=o.Kernel(o.EQ), X=X, Y=Y, opts=dict(grad_expand=1, grad_bcast=waves), path=1 | 32,
              expand=1, bcast=waves, wg=64 * waves, extra_rows=far, seed=d)


@pytest.mark.parametrize("d", [3, 64])
def test_fp32_lane_per_row_direct_with_far_rows(cg, oracle, d):
    o = oracle
    rng = np.random.default_rng(400 + d)
    X, far = add_far(cloud(rng, 300, d, F32), rng, 4)
    Y = cloud(rng, 230, d, F32, 1.0, 0.1)
    k, ko = (cg.EQ(), o.Kernel(o.EQ)) if d == 3 else (cg.RQ(1.5), o.Kernel(o.RQ, param=1.5))
    run_route(cg, o, dt=F32, k=k, ko=ko, X=X, Y=Y, opts=DIRECT, path=1 | 32, wg=256, extra_rows=far, seed=d)


@pytest.mark.parametrize("d", [8, 32])
def test_fp32_expanded_form(cg, oracle, d):
    """The fp32 expanded form inside its gate (x ~ N(0, I): gamma^2 R^2 well below 128)."""
    o = oracle
    rng = np.random.default_rng(500 + d)
    X = cloud(rng, 300, d, F32); Y = cloud(rng, 250, d, F32, 0.9)
    run_route(cg, o, dt=F32, k=cg.EQ(), ko=o.Kernel(o.EQ), X=X, Y=Y, opts=dict(grad_expand=1), path=1 | 32, expand=1, wg=256, seed=d)


@pytest.mark.parametrize("dt,d", [(F32, 8), (F64, 3)])
def test_two_column_pass_odd_right_hand_sides(cg, oracle, dt, d):
    """p = 3 columns, broadcast kernel off: one two-column pass (bit 2) and one single column; every column row-wise."""
    o = oracle
    rng = np.random.default_rng(600 + d)
    X, far = add_far(cloud(rng, 260, d, dt), rng, 2)
    Y = cloud(rng, 150, d, dt)
    run_route(cg, o, dt=dt, k=cg.Lengthscale(cg.MaternP(2), 0.9), ko=o.Kernel(o.MATERNP, p=2, lengthscale=0.9), X=X, Y=Y,
              opts=DIRECT, path=1 | 2 | 32, nrhs=3, wg=256, extra_rows=far, seed=d)


def test_lane_per_row_column_split_where_the_slab_cap_binds(cg, oracle):
    """fp64 d = 48, n = 8150, m = 8191, 64-row workgroups at 2 waves per SIMD (grad_mvm.hpp), num_cus = 256:
    64 splits per the ~64 waves per CU rule, capped at m / 64 = 127; the slab cap gcap = 256e6 / (8192 (48 + vg) 8) = 81 (gradient) /
    79 (value-gradient) binds and snaps down to whole rounds of the 2048 resident workgroups: 80 (5 rounds) / 64 (4 rounds); the
    8-aligned chunks of ceil(8191 / 80) -> 104 and 128 columns give 79 and 64 splits with a ragged last chunk."""
    o = oracle
    rng = np.random.default_rng(700)
    assert cg.get_info("num_cus") == 256
    X, far = add_far(cloud(rng, 8150, 48, F64), rng, 3)
    Y = cloud(rng, 8191, 48, F64)
    run_route(cg, o, dt=F64, k=cg.EQ(), ko=o.Kernel(o.EQ), X=X, Y=Y, opts=DIRECT, path=1 | 32, jsplit=(79, 64), wg=64,
              extra_rows=far, seed=7)


# ---------------------------------------------------------------------------------------------------------------- panel path
@pytest.mark.parametrize("dt,d,m", [(F64, 65, 13), (F32, 70, 29)])
def test_panel_path_one_panel_one_slice(cg, oracle, dt, d, m):
    """d beyond the lane-per-row kernels, one column block (m <= 16 fp64 / 32 fp32 columns): one panel, no z slices."""
    o = oracle
    rng = np.random.default_rng(800 + d)
    X, far = add_far(cloud(rng, 300, d, dt), rng, 3)
    Y = cloud(rng, m, d, dt, 0.8)
    run_route(cg, o, dt=dt, k=cg.Lengthscale(cg.EQ(), 2.0), ko=o.Kernel(o.EQ, lengthscale=2.0), X=X, Y=Y, opts={}, path=4,
              extra_rows=far, seed=d)


def test_panel_path_z_slices(cg, oracle):
    """fp64 d = 65, n = 8150: 128 row blocks x 3 dimension chunks = 384 waves -> ceil(256 x 16 / 384) = 11 z slices and the
    separate reduce; m = 1000: one panel."""
    o = oracle
    rng = np.random.default_rng(900)
    X, far = add_far(cloud(rng, 8150, 65, F64), rng, 3, 2.0)
    Y = cloud(rng, 1000, 65, F64)
    run_route(cg, o, dt=F64, k=2.0 * cg.Lengthscale(cg.EQ(), 2.0), ko=o.Kernel(o.EQ, lengthscale=2.0, scale=2.0), X=X, Y=Y, opts={},
              path=4 | 16, extra_rows=far, seed=9)


@pytest.mark.parametrize("dt,d,n,m", [(F64, 65, 4096, 4100), (F32, 70, 8192, 5000)])
def test_panel_path_several_panels(cg, oracle, dt, d, n, m):
    """panel = (256 MiB / (npad64 2 ts)) / BC BC columns: fp64 n = 4096 -> 4096 columns, m = 4100 leaves a second panel of one
    16-column block; fp32 n = 8192 -> 4096 columns of the 5024 padded ones.  Both split over z slices too."""
    o = oracle
    rng = np.random.default_rng(1000 + d)
    X, far = add_far(cloud(rng, n, d, dt), rng, 3, 1.5)
    Y = cloud(rng, m, d, dt, 1.0, 0.05)
    run_route(cg, o, dt=dt, k=1.3 * cg.Lengthscale(cg.MaternP(2), 1.5), ko=o.Kernel(o.MATERNP, p=2, lengthscale=1.5, scale=1.3), X=X,
              Y=Y, opts={}, path=4 | 8 | 16, extra_rows=far, seed=d)


def test_panel_path_forced_at_small_d(cg, oracle):
    """grad_keep_r = 2 sends d = 5 to the panel path (D = 32: 5 waves -> 16 slices, capped at the 14 column blocks)."""
    o = oracle
    rng = np.random.default_rng(1100)
    X, far = add_far(cloud(rng, 300, 5, F64), rng, 3)
    Y = cloud(rng, 211, 5, F64)
    run_route(cg, o, dt=F64, k=cg.EQ(), ko=o.Kernel(o.EQ), X=X, Y=Y, opts=dict(grad_keep_r=2), path=4 | 16, extra_rows=far, seed=11)


def test_composite_with_a_matern_factor_takes_the_panel_path(cg, oracle):
    """Matern(nu) * EQ: the lane-per-row interpreter is built without the Matern factor (block_mvm.hip: heavy_factor)."""
    o = oracle
    rng = np.random.default_rng(1200)
    X, far = add_far(cloud(rng, 300, 3, F64), rng, 3)
    Y = cloud(rng, 150, 3, F64)
    ko = o.Composite(((o.Kernel(o.MATERN, param=1.3), o.Kernel(o.EQ)),), o.ISOTROPIC, 1.0)
    run_route(cg, o, dt=F64, k=cg.Matern(1.3) * cg.EQ(), ko=ko, X=X, Y=Y, opts={}, path=4 | 16, extra_rows=far, seed=12)


# ---------------------------------------------------------------------------------------------------------------- traits, sums
@pytest.mark.parametrize("name", ["Dot^3", "ExponentialDot"])
@pytest.mark.parametrize("keep_r,path", [(-1, 1 | 32), (2, 4 | 16)])
def test_dot_product_trait(cg, oracle, name, keep_r, path):
    o = oracle
    rng = np.random.default_rng(1300 + keep_r)
    X = cloud(rng, 280, 8, F64, 0.3); Y = cloud(rng, 200, 8, F64, 0.3, 0.05)
    k, ko = (cg.Dot() ** 3, o.Kernel(o.DOT, power=3)) if name == "Dot^3" else (cg.ExponentialDot(), o.Kernel(o.EXPDOT))
    run_route(cg, o, dt=F64, k=k, ko=ko, X=X, Y=Y, opts=dict(grad_keep_r=keep_r), path=path, wg=256, seed=13)


@pytest.mark.parametrize("dt", [F64, F32])
def test_sum_with_a_constant_term_term_by_term(cg, oracle, dt):
    """A Sum is split term by term; its constant term has zero derivatives and reaches only the value entry of the value-gradient
    blocks.  The info keys report the last term's launch (the EQ term; direct differences)."""
    o = oracle
    rng = np.random.default_rng(1400)
    X, far = add_far(cloud(rng, 300, 4, dt), rng, 2)
    Y = cloud(rng, 211, 4, dt)
    k = 0.6 * cg.Lengthscale(cg.MaternP(1), 1.2) + cg.Constant(0.4) + 0.7 * cg.EQ()
    ko = o.Composite(((o.Kernel(o.MATERNP, p=1, lengthscale=1.2, scale=0.6),), (o.Kernel(o.CONSTANT, scale=0.4),), (o.Kernel(o.EQ, scale=0.7),)),
                     o.ISOTROPIC, 1.0)
    run_route(cg, o, dt=dt, k=k, ko=ko, X=X, Y=Y, opts=DIRECT, path=1 | 32, wg=256, extra_rows=far, seed=14)


def test_fused_sum_gradient_is_split_term_by_term(cg, oracle):
    """A three-term fp32 Sum inside the matrix-core gate takes the one-pass Sum kernels for its VALUE MVM (last_sum_fused = 1);
    those kernels have no gradient form, so its gradient MVM must still be split term by term: the last term (EQ, d = 8) runs its
    own expanded-form kernel (last_grad_expand = 1) instead of the whole Sum on the composite interpreter."""
    o = oracle
    rng = np.random.default_rng(1500)
    X = cloud(rng, 2048, 8, F32, 0.35)
    L = cg.Lengthscale
    k = 0.5 * cg.InverseMultiQuadratic(1.2) + L(cg.MaternP(2), 1.5) + 0.3 * L(cg.EQ(), 0.8)
    ko = o.Composite(((o.Kernel(o.IMQ, param=1.2, scale=0.5),), (o.Kernel(o.MATERNP, p=2, lengthscale=1.5),), (o.Kernel(o.EQ, lengthscale=0.8, scale=0.3),)),
                     o.ISOTROPIC, 1.0)
    Xt = torch.from_numpy(X).cuda()
    (cg.gramian(k, Xt, Xt) @ torch.from_numpy(rng.standard_normal(2048).astype(F32)).cuda())
    assert cg.get_info("last_sum_fused") == 1
    run_route(cg, o, dt=F32, k=k, ko=ko, X=X, Y=X, opts={}, path=1 | 32, expand=1, wg=256, gamma2=1 / 0.64, seed=15)


# ---------------------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("dt,d,path_n1,path_m1", [(F64, 3, 1, 1), (F32, 70, 4 | 16, 4)])
def test_single_row_and_single_column(cg, oracle, dt, d, path_n1, path_m1):
    """n = 1 (97 columns: one chunk on the lane-per-row kernel; 4 slices on the panel path) and m = 1 (one column block).
    Lengthscale sqrt(d): with a single column at |r|^2 ~ 2 d, unit-lengthscale EQ entries of d = 70 fall below fp32's normal range."""
    o = oracle
    rng = np.random.default_rng(1600 + d)
    ls = math.sqrt(d)
    k, ko = cg.Lengthscale(cg.EQ(), ls), o.Kernel(o.EQ, lengthscale=ls)
    X = cloud(rng, 1, d, dt); Y = cloud(rng, 97, d, dt)
    run_route(cg, o, dt=dt, k=k, ko=ko, X=X, Y=Y, opts=DIRECT if d < 64 else {}, path=path_n1, seed=1)
    X = cloud(rng, 130, d, dt); Y = cloud(rng, 1, d, dt)
    run_route(cg, o, dt=dt, k=k, ko=ko, X=X, Y=Y, opts=DIRECT if d < 64 else {}, path=path_m1, seed=2)


@pytest.mark.parametrize("dt,d", [(F64, 3), (F32, 70)])
def test_no_columns_scales_y(cg, oracle, dt, d):
    """m = 0: y <- beta y (and zeros for beta = 0 over NaN), no block kernel (last_grad_path = 0)."""
    rng = np.random.default_rng(1700)
    X = torch.from_numpy(cloud(rng, 77, d, dt)).cuda(); Y = torch.empty((0, d), dtype=X.dtype, device="cuda")
    for vg in (0, 1):
        G = cg.gramian((cg.ValueGradientKernel if vg else cg.GradientKernel)(cg.EQ()), X, Y)
        y0 = rng.standard_normal(77 * (d + vg)).astype(dt)
        yt = torch.from_numpy(y0.copy()).cuda()
        G.mul_(yt, torch.empty(0, dtype=X.dtype, device="cuda"), 0.9, -1.7)
        assert cg.get_info("last_grad_path") == 0
        np.testing.assert_allclose(yt.cpu().numpy(), (-1.7 * y0.astype(np.float64)).astype(dt), rtol=TOL[dt], atol=0)
        yn = torch.full((77 * (d + vg),), NANV, dtype=X.dtype, device="cuda")
        G.mul_(yn, torch.empty(0, dtype=X.dtype, device="cuda"), 0.9, 0.0)
        assert torch.all(yn == 0).item()
