"""tests/kron_ref.py checked on the host, without the library: the reference and the bound against an explicit Kronecker matrix, a plain
same-precision implementation against the bound on every case, and the case table against the planner — every template arm of the three
kernels, both library-GEMM rules, the multiplied-out pair and the pair-first order must have a case that selects it on 256 CUs."""
import functools

import numpy as np
import pytest

import kron_ref as kr

F32, F64 = kr.F32, kr.F64
NUM_CUS = 256           # csrc/common.hpp, covgram_ctx::num_cus: the MI355X


@functools.lru_cache(maxsize=None)
def reference(tag, dt):
    """Inputs and the two fp64 operator applications of one case, shared by the tests of this module and never modified."""
    case = kr.BY_TAG[tag]
    Fs, a, y0 = kr.inputs(case, dt)
    cache = {}
    kr.want_and_bound(Fs, a, y0, 1.0, 0.0, dt, cache)
    for x in Fs + [a, y0, cache["t"], cache["tabs"]]:
        x.setflags(write=False)
    return Fs, a, y0, cache


@pytest.mark.parametrize("dt", [F64, F32])
@pytest.mark.parametrize("shapes,nrhs", [([(3, 4), (2, 5), (4, 3)], 0), ([(5, 2)], 0), ([(1, 3), (4, 1)], 0), ([(3, 4), (2, 5)], 3), ([(2, 2)] * 4, 2)])
def test_want_and_bound_against_the_explicit_kronecker_matrix(dt, shapes, nrhs):
    """want and bound from np.kron of the factors, in extended precision where numpy has one (longdouble; plain fp64 elsewhere)."""
    ld = np.longdouble
    rng = np.random.default_rng(5)
    Fs = [rng.standard_normal(s).astype(dt) for s in shapes]
    nin = int(np.prod([s[1] for s in shapes])); nout = int(np.prod([s[0] for s in shapes]))
    a = rng.standard_normal((nin,) if nrhs == 0 else (nin, nrhs)).astype(dt)
    y0 = rng.standard_normal((nout,) if nrhs == 0 else (nout, nrhs)).astype(dt)
    K = functools.reduce(np.kron, [F.astype(ld) for F in Fs])
    assert K.shape == (nout, nin)
    u = kr.unit_roundoff(dt)
    n = sum(s[1] for s in shapes) + len(shapes) + 2
    assert kr.terms(Fs) == n
    if len(shapes) >= 2:      # the multiplied-out pair: one dot product of length c_{q-1} c_q in place of two
        assert kr.terms(Fs, merged=True) == n - shapes[-2][1] - shapes[-1][1] + shapes[-2][1] * shapes[-1][1]
        wm, bm = kr.want_and_bound(Fs, a, y0, 1.0, 0.0, dt, merged=True)
        w0, b0 = kr.want_and_bound(Fs, a, y0, 1.0, 0.0, dt)
        assert np.array_equal(wm, w0) and (np.all(bm >= b0) or shapes[-2][1] * shapes[-1][1] < shapes[-2][1] + shapes[-1][1])
    for al, be in kr.ALPHA_BETA:
        want, bound = kr.want_and_bound(Fs, a, y0, al, be, dt)
        assert want.shape == y0.shape and bound.shape == y0.shape and want.dtype == np.float64
        w = ld(al) * (K @ a.astype(ld)) + ld(be) * y0.astype(ld)
        tabs = np.abs(K) @ np.abs(a.astype(ld))
        assert np.all(np.abs(want - w) <= 8 * np.finfo(np.float64).eps * (abs(al) * tabs + np.abs(be * y0.astype(ld))))
        b = n * u / (1 - n * u) * abs(al) * tabs + u * (np.abs(w) + 2 * np.abs(ld(be) * y0.astype(ld)))
        assert np.allclose(bound, b.astype(np.float64), rtol=1e-9, atol=0)
        assert np.all(bound > 0)
    # beta == 0 never reads y0
    want, bound = kr.want_and_bound(Fs, a, np.full(y0.shape, np.nan), 1.0, 0.0, dt)
    assert np.isfinite(want).all() and np.isfinite(bound).all()


def test_coordinates():
    assert kr.coordinates(0, [(3, 4), (2, 5)], 0) == (0, 0)
    assert kr.coordinates(5, [(3, 4), (2, 5)], 0) == (2, 1)
    assert kr.coordinates(5 * 7 + 6, [(3, 4), (2, 5)], 7) == (2, 1, 6)


ALL = [(c.tag, dt) for c in kr.CASES for dt in c.dts]


@pytest.mark.parametrize("tag,dt", ALL, ids=["%s-%s" % (t, d.__name__) for t, d in ALL])
def test_same_precision_mode_products_stay_within_the_bound(tag, dt):
    """numpy's mode products with every intermediate rounded to the dtype: a correct implementation in another summation order,
    which the bound (a worst case over orders) must hold for."""
    Fs, a, y0, cache = reference(tag, dt)
    worst = 0.0
    for al, be in kr.ALPHA_BETA:
        want, bound = kr.want_and_bound(Fs, a, y0, al, be, dt, cache)
        got = kr.emulate(Fs, a, y0, al, be, dt).astype(np.float64)
        assert got.shape == want.shape
        r = np.abs(got - want) / bound
        worst = max(worst, float(r.max()))
        assert r.max() <= 1, (tag, dt.__name__, (al, be), float(r.max()), kr.coordinates(int(np.argmax(r)), kr.BY_TAG[tag].shapes, kr.BY_TAG[tag].nrhs))
        # ... and the norm-wise tolerance beside it
        e = float(np.linalg.norm(got - want) / max(np.linalg.norm(want), np.finfo(np.float64).tiny))
        assert e <= kr.norm_tol(kr.BY_TAG[tag].shapes, dt), (tag, dt.__name__, (al, be), e)
    print(f"kron host {dt.__name__} {tag}: worst err/bound {worst:.3f}")


def arms_of(dt, a_aligned=True):
    """{(kernel, arm): [tags]}, the library-GEMM rules, merged and pair-first cases of CASES for one dtype at 256 CUs."""
    seen, blas, merged, first = {}, set(), [], []
    for c in kr.CASES:
        if dt not in c.dts:
            continue
        pl = kr.plan(c.shapes, dt, c.nrhs, NUM_CUS, a_aligned=a_aligned)
        assert pl.passes and pl.path != 0
        assert sum(p.final for p in pl.passes) == 1 and pl.passes[-1].final        # alpha / beta are applied once, by the last pass
        for p in pl.passes:
            if p.arm is not None:
                seen.setdefault((p.kernel, p.arm), []).append(c.tag)
            if p.kernel == "blas":
                blas.add(kr.blas_rule(p, c.shapes, c.nrhs))
        if pl.path & kr.PATH_MERGED:
            merged.append(c.tag)
        if pl.pair_first:
            first.append(c.tag)
    return seen, blas, merged, first


@pytest.mark.parametrize("dt", [F64, F32])
def test_cases_cover_every_arm_on_256_cus(dt):
    seen, blas, merged, first = arms_of(dt)
    print(f"\narm coverage, {dt.__name__}, num_cus = {NUM_CUS}:")
    missing = []
    for kernel, arm in kr.ALL_ARMS:
        tags = seen.get((kernel, arm), [])
        name = "%s<%d,%d,%s>" % (kernel, arm[0], arm[1], "VEC" if arm[2] else "scalar")
        if (kernel, arm) in kr.EXEMPT:
            assert not tags, (name, "is exempt but", tags, "select it")
            print(f"  {name:24s} EXEMPT: {kr.EXEMPT[(kernel, arm)]}")
            continue
        print(f"  {name:24s} {', '.join(tags[:5])}{' ...' if len(tags) > 5 else ''}")
        if not tags:
            missing.append(name)
    print(f"  library GEMM rules: {sorted(blas)}; multiplied-out pair: {merged[:4]}; pair first: {first}")
    assert not missing, missing
    assert blas == {"min", "mid"} and merged and first            # (no case is a shape the kernels refuse: "refused" would show here)
    assert len(set(seen)) + len(kr.EXEMPT) == 28


def test_plan_details_the_cases_are_here_for():
    """The properties the table's comments claim, from plan(): which pass is final, what the fused pass sees, the two GEMM forms."""
    P = lambda tag, dt, **kw: kr.plan(kr.BY_TAG[tag].shapes, dt, kr.BY_TAG[tag].nrhs, NUM_CUS, **kw)
    for dt in (F64, F32):
        pl = P("128^3", dt)
        assert [p.kernel for p in pl.passes] == ["mode", "pair"] and pl.passes[1].arm == (8, 8, True) and pl.path == 3
        assert P("64^3", dt).path == 2 | 4 and P("300x200", dt).path == 4 and P("16^5", dt).path & 16
        for tag in ("20,36,52", "7,130,96", "9,33,200", "3,48,300", "2,120,16", "40,100"):       # what the old docstring took for pair cases
            assert P(tag, dt).path == 2 | 4, tag
        pl = P("pair-only", dt)
        assert len(pl.passes) == 1 and pl.passes[0].kernel == "pair" and pl.passes[0].final and pl.passes[0].pre == 160
        pl = P("pair-first-f64" if dt == F64 else "pair-first-f32", dt)
        assert [p.kernel for p in pl.passes] == ["pair", "mode"] and not pl.passes[0].final and pl.pair_first
        pl = P("blas-mid", dt)
        assert [p.kernel for p in pl.passes] == ["blas", "modet"] and pl.passes[0].post == 16 and pl.passes[1].pre == 262144 and pl.passes[1].arm[0] == 8
        assert [p.kernel for p in P("12,1100", dt).passes] == ["mode", "blas"] and P("12,1100", dt).passes[1].post == 1
        assert P("pair<8,8>-3chunks", dt).passes[1].M == (65, 257)
        # a misaligned input changes the first pass alone
        a, b = P("128^3", dt), P("128^3", dt, a_aligned=False)
        assert b.passes[0].arm == a.passes[0].arm[:2] + (False,) and b.passes[1:] == a.passes[1:]
        a, b = P("pair-only", dt), P("pair-only", dt, a_aligned=False)
        assert a.passes[0].arm == (8, 8, True) and b.passes[0].arm == (8, 8, False)
        # an odd leading dimension of the last factor alone switches the fused pass to scalar accesses
        c = kr.BY_TAG["pair-K2=128-N2=128"]
        assert kr.plan(c.shapes, dt, 0, NUM_CUS).passes[-1].arm == (8, 8, True)
        assert kr.plan(c.shapes, dt, 0, NUM_CUS, lds=[128, 70, 129]).passes[-1].arm == (8, 8, False)
    # the planner depends on the chip: fewer CUs take the fused pass earlier
    assert kr.plan([(64, 64)] * 3, F64, 0, 64).path == 1 | 2
    assert kr.plan([(64, 64)] * 3, F32, 0, 64).path == 2 | 4          # fp32 sides <= 64 never fuse
