"""Toeplitz / SymmetricToeplitz / Circulant products on the device (csrc/toeplitz.hip, csrc/toeplitz_kernels.hpp) ENTRY BY ENTRY against
the references and the bound of tests/toeplitz_ref.py, on every route of covgram_toeplitz_create / fast_mvm:

    rocFFT path (N < 2^13; fp32: < 2^14; circulant lengths 1, 2, 3, 33, 1000, 4099, 16384), the four-step path with rocFFT row batches
    (M' = 4, 8, 16), the fused radix-4 row kernels (M' = 64, 256, 1024) and the radix-16 row kernel (M' = 4096), column lengths 512,
    1024 and 2048, both tile maps of the column kernels — each at a tall shape (n > N / 2: the upper half of every column FFT's stores),
    a wide and a full one (m > N / 2: the upper half of its loads), which no square case reaches —

and the option arms (rocFFT batches / radix-4 rows / the radix-4 column FFT / the complex spectrum copy / every persistent-grid setting of
the radix-16 kernel in both dtypes), the transpose, a matrix right-hand side and repeated calls.  Every case runs (alpha, beta) = (1, 0)
into a NaN-filled y and (-0.7, 1.3) into a random one; `worst err / bound` is printed per case (-s)."""
import math

import numpy as np
import pytest
import torch

import toeplitz_ref as tr

pytestmark = pytest.mark.gpu

F32, F64 = tr.F32, tr.F64
TDT = {F32: torch.float32, F64: torch.float64}
DTYPES = [F32, F64]
OPTION_DEFAULTS = {"toeplitz_fused": 1, "toeplitz_colfft": 16, "toeplitz_real_spectrum": 1, "toeplitz_persist": -1}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def rocfft_stays_up(cg, dev):
    """covgram_toeplitz_destroy of the last live handle tears rocFFT down (half a second per cycle, see tests/test_gpu_host_api.py): one
    tiny handle lives as long as the module."""
    keep = cg.Circulant(torch.ones(4, dtype=torch.float64, device=dev))
    yield
    del keep


def operator(cg, case, inp, dev):
    vc = torch.from_numpy(inp.vc).to(dev)
    if case.circulant:
        return cg.Circulant(vc)
    if case.symmetric:
        return cg.SymmetricToeplitz(vc)
    return cg.Toeplitz(vc, torch.from_numpy(inp.vr).to(dev))


def products(cg, op, inp, dev):
    """The device results of both (alpha, beta), as device tensors; the first product is run twice and must repeat bit for bit."""
    ad = torch.from_numpy(inp.a).to(dev)
    out = []
    for al, be in tr.ALPHA_BETA:
        if be == 0:
            y = torch.full((op.shape[0],), float("nan"), dtype=op.dtype, device=dev)
        else:
            y = torch.from_numpy(inp.y0).to(dev)
        cg.mul_(y, op, ad, al, be)
        out.append(y)
    again = torch.full((op.shape[0],), float("nan"), dtype=op.dtype, device=dev)
    cg.mul_(again, op, ad, *tr.ALPHA_BETA[0])
    assert torch.equal(again, out[0]), "two calls on one handle differ"
    return out


def judge(name, case, dt, inp, outs, dev):
    """Every row of both products against want and bound (compared on the device); returns the worst err / bound."""
    worst = 0.0
    for (al, be), y in zip(tr.ALPHA_BETA, outs):
        assert tuple(y.shape) == (case.n,) and bool(torch.isfinite(y).all()), (name, al, "not finite")
        want, bound = (torch.from_numpy(x).to(dev) for x in tr.want_and_bound(case, dt, inp, al, be))
        err = (y.double() - want).abs()
        r = torch.where(bound > 0, err / bound, torch.where(err == 0, 0.0, float("inf")))
        i = int(torch.argmax(r))
        worst = max(worst, float(r[i]))
        assert float(r[i]) <= 1, (name, dt.__name__, (al, be), "row", i, "got", float(y[i]), "want", float(want[i]), "err/bound", float(r[i]),
                                  "rows over", int((r > 1).sum()), tr.route(case.n, case.m, dt, case.circulant))
    return worst


def run_case(cg, dev, case, dt, kinds=None, variants=None, label=""):
    """All kinds (and shift variants) of one case under the options in force; {(kind, variant): device results}."""
    res = {}
    for kind in (kinds or case.kinds):
        vs = tr.kind_variants(case, kind, dt)
        if kind == "shift" and variants is not None:
            vs = [v for v in vs if v in variants] or vs[-1:]
        for v in vs:
            inp = tr.inputs(case, kind, dt, v)
            op = operator(cg, case, inp, dev)
            assert tuple(op.shape) == (case.n, case.m)
            outs = products(cg, op, inp, dev)
            name = f"{case.tag} {case.n}x{case.m} {kind}{'' if v is None else v}{label}"
            w = judge(name, case, dt, inp, outs, dev)
            print(f"toeplitz {dt.__name__} {name}: worst err/bound {w:.3f}")
            res[(kind, v)] = outs
            del op
    return res


ALL_CASES = [(dt, c) for dt in DTYPES for c in tr.cases(dt) + tr.circulant_cases()]


@pytest.mark.parametrize("dt,case", ALL_CASES, ids=[f"{dt.__name__}-{c.tag}" for dt, c in ALL_CASES])
def test_every_entry_on_every_route(cg, dev, dt, case):
    """The case list of tests/toeplitz_ref.py under the default options.  The route of the case — the rule of covgram_toeplitz_create as
    tests/toeplitz_ref.py restates it — is asserted against the table of sizes first: the table documents which kernel a case is here
    for.  Neither reads the library, so a change of the rule in csrc/toeplitz.hip has to be carried over to both by hand.  (2^24:
    n + m - 1 = 2^24 in fp32, the longest case: spikes and two-sided shifts only.)"""
    rt = tr.route(case.n, case.m, dt, case.circulant)
    assert rt == tr.expected_route(case.n, case.m, dt, case.circulant), (case, rt)
    run_case(cg, dev, case, dt)


def test_route_map_reaches_every_kernel_class():
    """What the parametrisation above runs, by (row kernel, column length, tile map), per dtype: every fused-kernel class (L = 3, 4, 5,
    radix 16), the unfused path, all column lengths that exist for the dtype, both tile maps, each with n > N / 2 and with m > N / 2."""
    for dt in DTYPES:
        rows, cols, maps, halves = set(), set(), set(), {}
        for c in tr.cases(dt):
            rt = tr.route(c.n, c.m, dt)
            print(f"route {dt.__name__} {c.tag} {c.n}x{c.m}: N=2^{int(math.log2(rt.N))} n1={rt.n1} M'={rt.Mp} {rt.row} swizzled={rt.swizzled}")
            if not rt.fast:
                continue
            rows.add(rt.row); cols.add(rt.n1); maps.add(rt.swizzled)
            h = halves.setdefault((rt.row, rt.n1), set())
            h |= ({"n"} if c.n > rt.N // 2 else set()) | ({"m"} if c.m > rt.N // 2 else set())
        assert rows == {"unfused", "radix4:3", "radix4:4", "radix4:5", "radix16"}
        assert cols == ({512, 1024, 2048} if dt == F32 else {512, 1024}) and maps == {False, True}
        for k, h in halves.items():
            assert h == {"n", "m"} or k == ("radix16", 2048), (k, h)


# ---- option arms -------------------------------------------------------------------------------------------------------------------
def arm_cases(N):
    """One tall non-symmetric case and the largest symmetric one of an embedding."""
    lg = int(math.log2(N))
    return [tr.Case("2^%d:tall" % lg, *tr.shapes(N)["tall"], ("spikes", "shift"), False, False), tr.symmetric_case(N)]


def arm_variants(case):
    """Of the shifts, the one that reaches past N / 2 (first column e_p: y_i = a_(i - p), symmetric: + a_(i + p))."""
    N = tr.embedding(case.n, case.m)
    return [("col", N // 2 + 1 if N // 2 + 1 < case.n else case.n - 1)]


def with_options(cg, opts, fn):
    try:
        for k, v in opts.items():
            cg.set_option(k, v)
        return fn()
    finally:
        for k, v in OPTION_DEFAULTS.items():
            cg.set_option(k, v)


# one embedding per row-kernel class with the column length 1024 (the only one the radix-4 column kernel serves), and 2^22: 512 x 4096
@pytest.mark.parametrize("lg", [15, 17, 19, 21, 22, 23])
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: d.__name__)
def test_option_arms(cg, dev, dt, lg):
    """rocFFT row batches (toeplitz_fused = 0), radix-4 rows everywhere (2), the radix-4 column FFT (toeplitz_colfft = 4, column length
    1024) and, at M' = 4096, a symmetric handle created with the complex spectrum copy (toeplitz_real_spectrum = 0: REALS = false on a real
    spectrum): each arm against the reference and the bound, on a non-symmetric tall case and through cg.SymmetricToeplitz."""
    N = 1 << lg
    for case in arm_cases(N):
        rt = tr.route(case.n, case.m, dt)
        assert rt == tr.expected_route(case.n, case.m, dt) and rt.fast
        arms = []                                            # only the arms that run other code than the default at this size
        if rt.row != "unfused":
            arms.append({"toeplitz_fused": 0})
        if rt.row == "radix16":
            arms.append({"toeplitz_fused": 2})
        if rt.n1 == 1024:
            arms.append({"toeplitz_colfft": 4})
            if rt.row != "unfused":
                arms.append({"toeplitz_colfft": 4, "toeplitz_fused": 0})
        if rt.Mp == 4096 and case.symmetric:
            arms.append({"toeplitz_real_spectrum": 0})
        for opts in arms:
            label = " " + ",".join(f"{k[9:]}={v}" for k, v in opts.items())
            with_options(cg, opts, lambda: run_case(cg, dev, case, dt, variants=arm_variants(case), label=label))


@pytest.mark.parametrize("lg", [22, 23])
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: d.__name__)
def test_radix16_persistent_grid_arms(cg, dev, dt, lg):
    """rowfft16_fused_kernel at M' = 4096 with column length 512 and 1024: toeplitz_persist = -1 (the default: PERSIST in fp64 only), 0 and 1
    (the two instantiations the default skips), 3 (three workgroups with unequal trip counts: 256 / 512 pairs over 3, the prefetch past the
    last pair must not happen) and 100000 (clipped to one pair per workgroup) — REALS = false on the tall case, REALS = true through
    cg.SymmetricToeplitz.  Each arm against reference and bound; and the arms agree bit for bit, as csrc/toeplitz.hip claims."""
    N = 1 << lg
    for case in arm_cases(N):
        rt = tr.route(case.n, case.m, dt)
        assert rt.row == "radix16" and rt.n1 == (512 if lg == 22 else 1024)
        res = {}
        for p in (-1, 0, 1, 3, 100000):
            res[p] = with_options(cg, {"toeplitz_persist": p},
                                  lambda: run_case(cg, dev, case, dt, variants=arm_variants(case), label=f" persist={p}"))
        for p, r in res.items():
            for key, outs in r.items():
                for y, y0 in zip(outs, res[-1][key]):
                    assert torch.equal(y, y0), ("persist arms differ", case.tag, key, p, int((y != y0).sum()))


# ---- transpose, matrix right-hand side ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: d.__name__)
def test_transpose_of_a_tall_case(cg, dev, oracle, dt):
    """Toeplitz(vc, vr).T @ u = the product with first column and first row exchanged (what gram_product's backward relies on), on the
    tall case of 2^16: the transpose is wide, so its input reaches the upper half of the column FFT."""
    case = [c for c in tr.cases(dt) if c.tag == "2^16:tall"][0]
    inp = tr.inputs(case, "dense", dt)
    T = operator(cg, case, inp, dev)
    Tt = T.T
    assert tuple(Tt.shape) == (case.m, case.n)
    tcase = tr.Case("2^16:tall'", case.m, case.n, ("dense",), False, False)
    rng = np.random.default_rng(tr.seed_of(tcase, "dense"))
    u = rng.standard_normal(case.n).astype(dt)
    y0 = rng.standard_normal(case.m).astype(dt)
    vc64, vr64, u64 = inp.vr.astype(F64), inp.vc.astype(F64), u.astype(F64)
    t = oracle.toeplitz_mul(None, vc64, vr64, u64)
    rows = tr.dense_check_rows(rng, tcase)
    direct = np.array([tr.dense_row(vc64, vr64, u64, i) for i in rows])
    assert np.max(np.abs(direct - t[rows])) <= 1e-11 * np.max(np.abs(direct))
    tinp = tr.Inputs(inp.vr, inp.vc, u, y0, t, inp.cnorm, float(np.linalg.norm(u64)))
    w = judge("transpose", tcase, dt, tinp, products(cg, Tt, tinp, dev), dev)
    print(f"toeplitz {dt.__name__} transpose of {case.tag}: worst err/bound {w:.3f}")


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: d.__name__)
def test_matrix_right_hand_side_equals_its_columns(cg, dev, dt):
    """Three columns on the wide case of 2^16: bit for bit the three vector products, at both (alpha, beta)."""
    case = [c for c in tr.cases(dt) if c.tag == "2^16:wide"][0]
    inp = tr.inputs(case, "dense", dt)
    T = operator(cg, case, inp, dev)
    g = torch.Generator(device="cpu").manual_seed(7)
    A = torch.randn((case.m, 3), dtype=TDT[dt], generator=g).to(dev)
    A[:, 0] = torch.from_numpy(inp.a).to(dev)
    Y0 = torch.randn((case.n, 3), dtype=TDT[dt], generator=g).to(dev)
    for al, be in tr.ALPHA_BETA:
        Y = Y0.clone() if be else torch.full_like(Y0, float("nan"))
        cg.mul_(Y, T, A, al, be)
        for k in range(3):
            y = Y0[:, k].clone() if be else torch.full((case.n,), float("nan"), dtype=TDT[dt], device=dev)
            cg.mul_(y, T, A[:, k].contiguous(), al, be)
            assert torch.equal(Y[:, k], y), (al, be, k)
    want, bound = tr.want_and_bound(case, dt, inp, 1.0, 0.0)
    got = (T @ A)[:, 0].cpu().numpy().astype(F64)
    assert np.all(np.abs(got - want) <= bound)
