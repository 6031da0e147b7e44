"""taylor! and minres on the device: covgram_bh_taylor_moments / covgram_bh_taylor_mvm, BarnesHutFactorization.taylor_ / taylor /
taylor_moments / solve, product="taylor", and solve.minres.

The method is that of tests/test_gpu_barneshut.py: the product is judged on the tree the DEVICE exported, with the device's own sums,
centres and centred first moments as the far-field data (exact T values, which test_moments has checked against extended-precision
moments over the exported ranges); tests/taylor_ref.py runs the reference's recursion (src/taylor.jl:33-57) in fp64 on top.  Row-wise,
    |got_i - want_i| <= |alpha| B_i + TOL (|alpha| (E_i + |D_i w_i|) + |beta| |y0_i|) + tiny,
where a leaf term contributes as in the existing test (tests/matrix_cases.py: reference_and_bound) and a far-field term
f0 sums - 2 f1 (ri . m1) contributes  bound(f0) |sums| + TOL max(1, L / 10) 2 |f1| sum_l |ri_l| |m1_l|  to B and
|f0| |sums| + 2 |f1| sum_l |ri_l| |m1_l|  to E, L = -ln(|f0| / phi(0)) (tests/test_bh_taylor_host.py shows that exactly rounded fp32
arithmetic in the device's order stays below half of it).  Rows whose criterion lies within 64 eps_T (h.r + theta (|x| + |c|)) of
equality are AMBIGUOUS and left out — at most 2 % of a case's rows, asserted on the CPU before the comparison (a cap: a shape that
exceeded it would get another seed) — and a case with theta > 0 and m > 4 leafsize must compress at least one node for at least a tenth
of its rows.

Clouds: those of tests/test_gpu_barneshut.py — N(0, I) on both sides, fewer than 8 targets moved by +4 in every coordinate.  In d = 5 a
ball tree over 500 points of N(0, I) has no node with radius < |x - c| / 4 for a target inside the cloud (the radii shrink like
m^(-1/d)), so theta = 1/4 would compress nothing there: every second target of the d > 4 shape is moved by +2 in every coordinate,
which leaves rows of both sorts.  (Not by +4: with EQ(l = 0.7) those rows' entries lie around 1e-37, where the fp32 hardware
exponential flushes the profile AND its derivative to zero.  The bound has the floor `tiny` for a flushed value, as everywhere in the
project, but by its definition none for a flushed derivative, so whole rows of order 1e-36 would be judged on flushed terms;
tests/test_bh_taylor_host.py counts the entries below the smallest normal number for both shifts.)"""
import numpy as np
import pytest
import torch

import barneshut_ref as br
import covgram_oracle as o
import matrix_cases as mc
import taylor_ref as tr

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TDT = {F32: torch.float32, F64: torch.float64}
NANV = float("nan")
THETAS = (0.0, 0.25, 0.45)
AB = ((1.0, 0.0), (-0.7, 1.3))
CG_MAXITER = 512           # the convention of tests/test_gpu_barneshut.py

# (n, m, d, leafsize, kind): kind "xy" two clouds, "xx" gramian(k, x) on one handle, "copies" m copies of one point
SHAPES = [(1, 40, 2, 4, "xy"), (63, 300, 1, 4, "xy"), (65, 300, 1, 4, "xy"), (130, 777, 3, 8, "xy"), (129, 500, 5, 8, "xy"),
          (257, 1024, 2, 16, "xy"), (1024, 1024, 2, 16, "xx"), (64, 12, 2, 16, "xy"), (33, 40, 2, 4, "copies")]
IDS = [f"n{n}-m{m}-d{d}-leaf{ls}-{kind}" for n, m, d, ls, kind in SHAPES]


def kernels(cg):
    return [
        ("Cauchy", cg.Cauchy(), o.Kernel(o.CAUCHY)),
        ("2.5 EQ(l=0.7)", 2.5 * cg.Lengthscale(cg.EQ(), 0.7), o.Kernel(o.EQ, lengthscale=0.7, scale=2.5)),
        ("MaternP(2)", cg.MaternP(2), o.Kernel(o.MATERNP, p=2)),
        ("RQ(1.5)", cg.RQ(1.5), o.Kernel(o.RQ, param=1.5)),
    ]


def other_kernels(cg):
    """the remaining profiles and the Power exponent: with kernels(), all eight isotropic families"""
    return [
        ("Cauchy(l=1.5)^2", cg.Lengthscale(cg.Cauchy(), 1.5) ** 2, o.Kernel(o.CAUCHY, lengthscale=1.5, power=2)),
        ("EQ^3", cg.EQ() ** 3, o.Kernel(o.EQ, power=3)),
        ("Exp", cg.Exp(), o.Kernel(o.EXP)),
        ("GammaExp(1.5)", cg.GammaExp(1.5), o.Kernel(o.GAMMAEXP, param=1.5)),
        ("IMQ(0.9)", cg.InverseMultiQuadratic(0.9), o.Kernel(o.IMQ, param=0.9)),
        ("Matern(1.3)", cg.Matern(1.3), o.Kernel(o.MATERN, param=1.3)),
    ]


def cloud(n, m, d, dt, kind):
    rng = np.random.default_rng(7 + 1000 * d + n + 31 * m)
    Y = rng.standard_normal((m, d))
    if kind == "copies":
        Y = np.repeat(rng.standard_normal((1, d)), m, axis=0)
    if kind == "xx":
        return Y.astype(dt), Y.astype(dt)
    X = rng.standard_normal((n, d)) + (4.0 if n < 8 else 0.0)
    if d > 4:
        X[::2] += 2.0
    return X.astype(dt), Y.astype(dt)


def make(cg, k, X, Y, kind, **kw):
    Xt = torch.from_numpy(X).cuda()
    return cg.BarnesHutFactorization(k, Xt, **kw) if kind == "xx" else cg.BarnesHutFactorization(k, Xt, torch.from_numpy(Y).cuda(), **kw)


def export(F):
    return {key: t.cpu().numpy() for key, t in F.tree().items()}


def entries_of(ko, X, dt):
    def entries(rows, P):
        return mc.reference_and_bound(o, ko, X[rows], np.ascontiguousarray(P).astype(dt), dt)
    return entries


def limit(want, babs, eabs, y0, alpha, beta, extra, dt):
    yb = np.zeros_like(want) if beta == 0 else y0.astype(F64)
    full = alpha * want + beta * yb + alpha * extra
    lim = abs(alpha) * babs + mc.TOL[dt] * (abs(alpha) * (eabs + np.abs(extra)) + abs(beta) * np.abs(yb)) + mc.tiny(dt)
    return full, lim


def judge(got, want, babs, eabs, y0, alpha, beta, extra, dt, keep):
    full, lim = limit(want, babs, eabs, y0, alpha, beta, extra, dt)
    g = got.astype(F64)
    with np.errstate(invalid="ignore"):
        r = np.where(np.isfinite(g), np.abs(g - full) / lim, np.inf)
    r = np.where(keep, r, 0.0)
    i = int(np.argmax(r))
    return float(r[i]), i, float(g[i]), float(full[i])


def device_moments(F, w, use_com):
    return tuple(a.cpu().numpy() for a in F.taylor_moments(torch.from_numpy(w).cuda(), use_com=use_com))


# ---- 1. moments -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_moments(cg, shape, dt):
    n, m, d, ls, kind = shape
    X, Y = cloud(n, m, d, dt, kind)
    F = make(cg, cg.Cauchy(), X, Y, kind, leafsize=ls)
    t = export(F)
    eps = float(np.finfo(dt).eps)
    rng = np.random.default_rng(5)
    ws = {"randn": rng.standard_normal(m), "positive part": np.maximum(rng.standard_normal(m), 0), "zeros": np.zeros(m), "ones": np.ones(m)}
    for name, w in ws.items():
        w = w.astype(dt)
        rs, rc, sabs, mabs = br.moments(t, Y, w, eps)
        for use_com in (True, False):
            sums, cen, m1 = device_moments(F, w, use_com)
            assert sums.dtype == dt and cen.shape == (F.nnodes, d) and m1.shape == (F.nnodes, d) and m1.dtype == dt
            es = np.abs(sums.astype(F64) - rs) - (4 * eps * sabs + mc.tiny(dt))
            if use_com:
                ec = np.abs(cen.astype(F64) - rc) - (4 * eps * mabs / np.maximum(sabs, mc.tiny(dt))[:, None] + mc.tiny(dt))
            else:
                assert cen.tobytes() == t["centers"].tobytes(), "the ball centres are not the exported ones"
                ec = np.zeros(1)
            ref = tr.moments(t, Y, w, eps, use_com, centers=cen)        # centred about the device's own centre, as rounded to T
            em = np.abs(m1.astype(F64) - ref["m1"]) - (mc.TOL[dt] * (ref["mabs"] + np.abs(ref["sums"])[:, None] * np.abs(cen.astype(F64))) + mc.tiny(dt))
            print(f"bh-taylor-moments {IDS[SHAPES.index(shape)]} {np.dtype(dt).name} {name} use_com={use_com}: sums {es.max():.2e} centres {ec.max():.2e} "
                  f"m1 {em.max():.2e} (<= 0 passes)")
            assert (es <= 0).all() and (ec <= 0).all() and (em <= 0).all(), (name, use_com, es.max(), ec.max(), em.max())
            if name == "zeros":
                assert not sums.any() and not m1.any() and (not use_com or not cen.any())
    # NULL output pointers skip that array
    wt = torch.from_numpy(ws["randn"].astype(dt)).cuda()
    only = torch.full((F.nnodes, d), NANV, dtype=TDT[dt], device="cuda")
    cg._ffi.check(cg._ffi.lib().covgram_bh_taylor_moments(F.handle, cg._ffi._P(wt.data_ptr()), 1, None, None, cg._ffi._P(only.data_ptr()), cg._ffi.DEVICE))
    assert only.cpu().numpy().tobytes() == device_moments(F, ws["randn"].astype(dt), True)[2].tobytes()


# ---- 2. the product on the exported tree ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_product_on_exported_tree(cg, shape, dt):
    n, m, d, ls, kind = shape
    X, Y = cloud(n, m, d, dt, kind)
    eps = float(np.finfo(dt).eps)
    rng = np.random.default_rng(11)
    w = rng.standard_normal(m).astype(dt)
    y0 = rng.standard_normal(n).astype(dt)
    wt = torch.from_numpy(w).cuda()
    fails = []
    for kname, k, ko in kernels(cg):
        F = make(cg, k, X, Y, kind, leafsize=ls)
        t = export(F)
        ent = entries_of(ko, X, dt)
        jet = tr.far_jet(o, mc, ko, dt)
        for use_com in (True, False):
            sums, cen, m1 = device_moments(F, w, use_com)
            for theta in THETAS:
                rec = tr.recursion(t, X, Y, w, cen, sums, m1, theta, ent, jet, band_eps=eps if theta > 0 else None)
                want, babs, eabs, amb, comp = (rec[key] for key in ("want", "babs", "eabs", "ambiguous", "compressed"))
                assert amb.sum() <= 0.02 * n, (kname, theta, use_com, int(amb.sum()))
                if theta > 0 and m > 4 * ls:
                    assert (comp > 0).sum() >= 0.1 * n, (kname, theta, use_com, int((comp > 0).sum()))
                if theta == 0:
                    assert not comp.any()
                for alpha, beta in AB:
                    yt = torch.full((n,), NANV, dtype=TDT[dt], device="cuda") if beta == 0 else torch.from_numpy(y0).cuda()
                    F.taylor_(yt, wt, alpha, beta, theta=theta, use_com=use_com)
                    r, i, g, f = judge(yt.cpu().numpy(), want, babs, eabs, y0, alpha, beta, np.zeros(n), dt, ~amb)
                    line = (f"bh-taylor-rowwise {IDS[SHAPES.index(shape)]} {np.dtype(dt).name} {kname} theta={theta} use_com={use_com} ab=({alpha},{beta}): "
                            f"worst err/bound {r:.3f} at row {i} got {g!r} want {f!r}; ambiguous {int(amb.sum())}, rows compressing {int((comp > 0).sum())}")
                    print(line)
                    if not r <= 1.0:
                        fails.append(line)
    assert not fails, "\n".join(fails)


# ---- 3. theta = 0 is the dense product, all eight profiles ------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
def test_theta_zero_is_dense(cg, dt):
    shape = SHAPES[3]
    n, m, d, ls, kind = shape
    X, Y = cloud(n, m, d, dt, kind)
    rng = np.random.default_rng(17)
    w = rng.standard_normal(m).astype(dt); y0 = rng.standard_normal(n).astype(dt)
    wt = torch.from_numpy(w).cuda()
    fails = []
    for kname, k, ko in kernels(cg) + other_kernels(cg):
        ref, bound = mc.reference_and_bound(o, ko, X, Y, dt)
        want = ref @ w.astype(F64); babs = bound @ np.abs(w.astype(F64)); eabs = np.abs(ref) @ np.abs(w.astype(F64))
        F = make(cg, k, X, Y, kind, leafsize=ls)
        for use_com in (True, False):
            for alpha, beta in AB:
                yt = torch.full((n,), NANV, dtype=TDT[dt], device="cuda") if beta == 0 else torch.from_numpy(y0).cuda()
                F.taylor_(yt, wt, alpha, beta, theta=0.0, use_com=use_com)
                r, i, g, f = judge(yt.cpu().numpy(), want, babs, eabs, y0, alpha, beta, np.zeros(n), dt, np.ones(n, dtype=bool))
                line = f"bh-taylor-dense {np.dtype(dt).name} {kname} use_com={use_com} ab=({alpha},{beta}): worst err/bound {r:.3f} at row {i}"
                print(line)
                if not r <= 1.0:
                    fails.append(line)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dt", [F32, F64])
def test_far_field_of_the_other_profiles(cg, dt):
    """The derivative branch of every profile that kernels() leaves out (Exponential, GammaExponential, IMQ, Matern(nu), Power), on the
    exported tree at theta = 0.45 about the ball centres."""
    shape = SHAPES[3]
    n, m, d, ls, kind = shape
    X, Y = cloud(n, m, d, dt, kind)
    eps = float(np.finfo(dt).eps)
    w = np.random.default_rng(19).standard_normal(m).astype(dt)
    wt = torch.from_numpy(w).cuda()
    fails = []
    for kname, k, ko in other_kernels(cg):
        F = make(cg, k, X, Y, kind, leafsize=ls)
        t = export(F)
        sums, cen, m1 = device_moments(F, w, False)
        rec = tr.recursion(t, X, Y, w, cen, sums, m1, 0.45, entries_of(ko, X, dt), tr.far_jet(o, mc, ko, dt), band_eps=eps)
        assert rec["ambiguous"].sum() <= 0.02 * n and (rec["compressed"] > 0).sum() >= 0.1 * n
        got = F.taylor(wt, theta=0.45, use_com=False).cpu().numpy()
        r, i, g, f = judge(got, rec["want"], rec["babs"], rec["eabs"], None, 1.0, 0.0, np.zeros(n), dt, ~rec["ambiguous"])
        line = f"bh-taylor-other {np.dtype(dt).name} {kname}: worst err/bound {r:.3f} at row {i} got {g!r} want {f!r}"
        print(line)
        if not r <= 1.0:
            fails.append(line)
    assert not fails, "\n".join(fails)


# ---- 4. nonnegative weights: the unsplit single pass ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[5]], ids=[IDS[3], IDS[5]])
def test_nonnegative_weights_match_the_unsplit_product(cg, shape, dt):
    n, m, d, ls, kind = shape
    X, Y = cloud(n, m, d, dt, kind)
    eps = float(np.finfo(dt).eps)
    w = np.abs(np.random.default_rng(23).standard_normal(m)).astype(dt)
    wt = torch.from_numpy(w).cuda()
    for kname, k, ko in kernels(cg):
        F = make(cg, k, X, Y, kind, leafsize=ls)
        t = export(F)
        ent = entries_of(ko, X, dt)
        sums, cen, m1 = device_moments(F, w, True)
        bs, bc = (a.cpu().numpy() for a in F.moments(wt))
        for theta in (0.25, 0.45):
            rt = tr.recursion(t, X, Y, w, cen, sums, m1, theta, ent, tr.far_jet(o, mc, ko, dt), band_eps=eps)
            rb = br.recursion(t, X, Y, w, bc, bs, theta, ent, band_eps=eps)
            keep = ~(rt["ambiguous"] | rb["ambiguous"])
            lim = limit(rt["want"], rt["babs"], rt["eabs"], None, 1.0, 0.0, np.zeros(n), dt)[1] + limit(rb["want"], rb["babs"], rb["eabs"], None, 1.0, 0.0, np.zeros(n), dt)[1]
            a = F.taylor(wt, theta=theta, use_com=True).cpu().numpy().astype(F64)
            b = torch.empty(n, dtype=TDT[dt], device="cuda")
            F.mul_(b, wt, theta=theta, split=False)
            r = np.where(keep, np.abs(a - b.cpu().numpy().astype(F64)) / lim, 0.0)
            print(f"bh-taylor-unsplit {IDS[SHAPES.index(shape)]} {np.dtype(dt).name} {kname} theta={theta}: worst difference / (sum of both bounds) {r.max():.3f}")
            assert (r <= 1.0).all(), (kname, theta, float(r.max()))


# ---- 5. the reference's accuracy pin ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pin():
    rng = np.random.default_rng(20260)
    n, d = 1024, 2
    X = rng.standard_normal((n, d))
    K = o.matrix(o.Kernel(o.CAUCHY), X, X, F64)
    weights = {"ones": np.ones(n), "rand": rng.random(n), "signed rand": rng.random(n) - 0.5, "randn": rng.standard_normal(n)}
    return X, K, weights


def pin_handle(cg, X, dt=F64, **kw):
    return cg.BarnesHutFactorization(cg.Cauchy(), torch.from_numpy(X.astype(dt)).cuda(), D=1e-2, theta=0.125, leafsize=16, **kw)


@pytest.mark.parametrize("dt", [F32, F64])
def test_accuracy_pin(cg, pin, dt):
    """test/barneshut.jl:80 with the product the reference's mul! runs: norm-wise relative error against the dense fp64 K w + D w < 1e-3."""
    X, K, weights = pin
    F = pin_handle(cg, X, dt)
    for name, w in weights.items():
        wt = torch.from_numpy(w.astype(dt)).cuda()
        want = K @ w + 1e-2 * w
        err = {key: float(np.linalg.norm(got.cpu().numpy().astype(F64) - want) / np.linalg.norm(want))
               for key, got in (("com", F.taylor(wt)), ("ball", F.taylor(wt, use_com=False)), ("split", F @ wt))}
        print(f"bh-taylor-pin {np.dtype(dt).name} {name}: taylor (centre of mass) {err['com']:.2e}, taylor (ball centres) {err['ball']:.2e}, split {err['split']:.2e}")
        assert err["com"] < 1e-3, (name, err)


# ---- 6. determinism, aliasing, options --------------------------------------------------------------------------------------------------
def test_determinism_aliasing_and_options(cg, pin):
    X, K, weights = pin
    n = X.shape[0]
    F = pin_handle(cg, X)
    w = torch.from_numpy(weights["randn"]).cuda()
    for use_com in (True, False):
        b1 = F.taylor(w, use_com=use_com)
        b2 = F.taylor(w, use_com=use_com)
        assert b1.cpu().numpy().tobytes() == b2.cpu().numpy().tobytes()
        for alpha, beta in AB:                                     # b aliasing w
            want = torch.from_numpy(weights["signed rand"]).cuda()
            wa = want.clone()
            F.taylor_(want, wa, alpha, beta, use_com=use_com)      # separate buffers
            F.taylor_(wa, wa, alpha, beta, use_com=use_com)        # in place
            assert wa.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (alpha, beta)
        W = torch.from_numpy(np.stack([weights["ones"], weights["randn"], weights["signed rand"]], axis=1)).cuda()
        B = F.taylor(W, use_com=use_com)
        assert B.shape == (n, 3)
        for c, name in enumerate(("ones", "randn", "signed rand")):
            assert torch.equal(B[:, c], F.taylor(torch.from_numpy(weights[name]).cuda(), use_com=use_com)), name
        Ft = pin_handle(cg, X, product="taylor", use_com=use_com)
        assert torch.equal(Ft @ w, b1) and torch.equal(Ft @ W, B)
        y = torch.full((n,), NANV, dtype=torch.float64, device="cuda")
        Ft.mul_(y, w, split=False)                                 # split is not consulted
        assert torch.equal(y, b1)
    # a vector diagonal equals the scalar one
    Fv = cg.BarnesHutFactorization(cg.Cauchy(), torch.from_numpy(X).cuda(), D=np.full(n, 1e-2), theta=0.125, leafsize=16)
    for use_com in (True, False):
        assert torch.equal(Fv.taylor(w, use_com=use_com), F.taylor(w, use_com=use_com))
        for alpha, beta in AB:
            ys, yv = (torch.from_numpy(weights["rand"]).cuda() for _ in range(2))
            F.taylor_(ys, w, alpha, beta, use_com=use_com); Fv.taylor_(yv, w, alpha, beta, use_com=use_com)
            assert torch.equal(ys, yv), (use_com, alpha, beta)
    with pytest.raises(ValueError):
        cg.minres(F, torch.zeros((n, 2), dtype=torch.float64, device="cuda"))
    Fs = pin_handle(cg, X, product="split")
    y = torch.full((n,), NANV, dtype=torch.float64, device="cuda")
    cg._ffi.check(cg._ffi.lib().covgram_bh_mvm(Fs.handle, cg._ffi._P(w.data_ptr()), cg._ffi._P(y.data_ptr()), 1.0, 0.0, -1.0, 1,
                                               cg._ffi._P(Fs.D.data_ptr()), 1, cg._ffi.DEVICE))
    assert torch.equal(Fs @ w, y) and torch.equal(F @ w, y), "product=\"split\" is not the split product of covgram_bh_mvm"


# ---- 7. MINRES --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
def test_minres_against_a_dense_solve(cg, dt):
    n = 257
    X = np.random.default_rng(29).standard_normal((n, 2)).astype(dt)
    F = cg.BarnesHutFactorization(cg.EQ(), torch.from_numpy(X).cuda(), D=1.0, theta=0.0)
    b = np.random.default_rng(31).standard_normal(n).astype(dt)
    A = torch.from_numpy(o.matrix(o.Kernel(o.EQ), X, X, dt) + np.eye(n))
    want = torch.linalg.solve(A, torch.from_numpy(b.astype(F64))).numpy()
    reltol = 1e-10 if dt == F64 else 1e-5
    x, info = cg.minres(F, torch.from_numpy(b).cuda(), reltol=reltol)
    err = float(np.linalg.norm(x.cpu().numpy().astype(F64) - want) / np.linalg.norm(want))
    print(f"bh-minres dense {np.dtype(dt).name}: {info['iterations']} iterations, recurrence {info['residual_norm']:.2e}, solution error {err:.2e}")
    assert set(info) == {"iterations", "residual_norm", "converged"} and info["converged"] and err <= 100 * reltol, (err, info)


def test_minres_on_an_indefinite_system(cg):
    """K - sigma I with four positive eigenvalues: a system where cg has no business."""
    n = 300
    X = np.random.default_rng(5).standard_normal((n, 2)).astype(F32).astype(F64)
    K = o.matrix(o.Kernel(o.CAUCHY), X, X, F64)
    ev = np.linalg.eigvalsh(K)
    sigma = 0.5 * (ev[-4] + ev[-5])
    es = ev - sigma
    assert (es > 0).sum() == 4 and np.abs(es).max() / np.abs(es).min() <= 100, (sigma, np.abs(es).max() / np.abs(es).min())
    F = cg.BarnesHutFactorization(cg.Cauchy(), torch.from_numpy(X).cuda(), D=-sigma, theta=0.0)
    b = torch.from_numpy(np.random.default_rng(6).standard_normal(n)).cuda()
    x, info = cg.minres(F, b, reltol=1e-8, maxiter=n)
    res = float(torch.linalg.vector_norm(F @ x - b) / torch.linalg.vector_norm(b))
    print(f"bh-minres indefinite: sigma {sigma:.4f}, {info['iterations']} iterations, residual {res:.2e}")
    assert info["converged"] and res <= 1e-6, (res, info)
    x8, info8 = cg.minres(F, b, reltol=1e-8, maxiter=n, check_every=8)           # the recurrence without a read-back per iteration
    assert info8["converged"] and info["iterations"] <= info8["iterations"] < info["iterations"] + 8
    assert float(torch.linalg.vector_norm(F @ x8 - b) / torch.linalg.vector_norm(b)) <= 1e-6


def test_solve_pin(cg, pin):
    """test/barneshut.jl:81-82: x = F \\ b with b = F w and at most 128 iterations leaves |F x - b| < 1e-3 |b|.  fp32 is printed only:
    how far an fp32 Lanczos recurrence drifts on this system has not been measured before."""
    X, K, weights = pin
    for dt in (F64, F32):
        F = pin_handle(cg, X, dt, product="taylor")
        for name, w in weights.items():
            b = F @ torch.from_numpy(w.astype(dt)).cuda()
            x, info = cg.minres(F, b, maxiter=128, reltol=1e-4)
            res = float(torch.linalg.vector_norm(F @ x - b) / torch.linalg.vector_norm(b))
            print(f"bh-solve-pin {np.dtype(dt).name} {name}: {info['iterations']} iterations, recurrence "
                  f"{info['residual_norm'] / float(torch.linalg.vector_norm(b)):.2e}, residual {res:.2e}")
            if dt == F64:
                assert torch.equal(F.solve(b, maxiter=128, reltol=1e-4), x)
                assert res < 1e-3, (name, res, info)


# ---- 8. cg in a captured graph ----------------------------------------------------------------------------------------------------------
def test_cg_in_a_captured_graph(cg, pin):
    """The Taylor product with device pointers allocates nothing and never synchronises, so cg(..., graph=True) captures it; about the
    ball centres it is a linear operator.  Same right-hand side, iteration cap and bound as the split product's test."""
    X, K, weights = pin
    F = pin_handle(cg, X, product="taylor", use_com=False)
    b = F @ torch.from_numpy(weights["randn"]).cuda()
    res = {}
    for graph in (False, True):
        x, info = cg.cg(F, b, reltol=1e-4, maxiter=CG_MAXITER, graph=graph)
        assert info.get("graph", False) is graph
        res[graph] = float(torch.linalg.vector_norm(F @ x - b) / torch.linalg.vector_norm(b))
        print(f"bh-taylor-cg graph={graph} randn: {info['iterations']} iterations, residual {res[graph]:.2e}")
        assert info["converged"] and res[graph] < 1e-3, (graph, res, info)


# ---- 9. empty products and refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, F64])
def test_empty_products_and_refusals(cg, dt):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((17, 2)).astype(dt)
    E = np.zeros((0, 2), dtype=dt)
    f, lib = cg._ffi, cg._ffi.lib()
    F = make(cg, cg.Cauchy(), X, E, "xy")                      # m = 0: y <- beta y
    y = torch.full((17,), NANV, dtype=TDT[dt], device="cuda")
    F.taylor_(y, torch.zeros(0, dtype=TDT[dt], device="cuda"))
    assert not y.cpu().numpy().any()
    y0 = rng.standard_normal(17).astype(dt)
    y = torch.from_numpy(y0).cuda()
    F.taylor_(y, torch.zeros(0, dtype=TDT[dt], device="cuda"), 2.0, 0.5, use_com=False)
    assert np.array_equal(y.cpu().numpy(), (dt(0.5) * y0).astype(dt))
    assert all(a.shape[0] == 0 for a in F.taylor_moments(torch.zeros(0, dtype=TDT[dt], device="cuda")))
    F = make(cg, cg.Cauchy(), E, X, "xy")                      # n = 0: nothing to write
    out = F.taylor(torch.from_numpy(rng.standard_normal(17).astype(dt)).cuda())
    assert out.shape == (0,)
    F = make(cg, cg.Cauchy(), X, X, "xx")
    w = torch.from_numpy(rng.standard_normal(17).astype(dt)).cuda()
    y = torch.empty(17, dtype=TDT[dt], device="cuda")
    P = f._P
    assert lib.covgram_bh_taylor_mvm(None, P(w.data_ptr()), P(y.data_ptr()), 1.0, 0.0, -1.0, 1, None, 0, f.DEVICE) == f.EINVAL
    assert lib.covgram_bh_taylor_mvm(F.handle, None, P(y.data_ptr()), 1.0, 0.0, -1.0, 1, None, 0, f.DEVICE) == f.EINVAL
    assert lib.covgram_bh_taylor_mvm(F.handle, P(w.data_ptr()), P(y.data_ptr()), 1.0, 0.0, NANV, 1, None, 0, f.DEVICE) == f.EINVAL
    assert lib.covgram_bh_taylor_mvm(F.handle, P(w.data_ptr()), P(y.data_ptr()), 1.0, 0.0, -1.0, 1, P(w.data_ptr()), 5, f.DEVICE) == f.EINVAL
    assert lib.covgram_bh_taylor_mvm(F.handle, P(w.data_ptr()), P(y.data_ptr()), 1.0, 0.0, -1.0, 1, None, 0, 7) == f.EINVAL
    assert lib.covgram_bh_taylor_moments(None, P(w.data_ptr()), 1, None, None, None, f.DEVICE) == f.EINVAL
    assert lib.covgram_bh_taylor_moments(F.handle, None, 1, None, None, None, f.DEVICE) == f.EINVAL
    for bad in (torch.zeros(16, dtype=TDT[dt], device="cuda"), torch.zeros(18, dtype=TDT[dt], device="cuda")):
        with pytest.raises(ValueError):
            F.taylor(bad)
        with pytest.raises(ValueError):
            F.taylor_moments(bad)
    with pytest.raises(ValueError):
        F.taylor_(torch.empty(16, dtype=TDT[dt], device="cuda"), w)
    with pytest.raises(ValueError):
        F.taylor(w, theta=-0.5)
