"""No GPU: pins what tests/test_gpu_toeplitz.py relies on (tests/toeplitz_ref.py) — the three references against the dense matrix, the
route map against the table of sizes, KAPPA against the measured numpy ratios, the headroom of numpy's same-precision embedding under the
bound, and the bound's sharpness: seven planted defects, each of which must exceed 4 x bound wherever it changes the product at all."""
import math

import numpy as np
import pytest

import toeplitz_ref as tr

F32, F64 = tr.F32, tr.F64
DTYPES = [F32, F64]


def test_numpy_fft_keeps_single_precision():
    """emulate() is a same-precision emulation only if np.fft does not promote float32 (numpy >= 2.0)."""
    x = np.ones(16, dtype=F32)
    X = np.fft.rfft(x)
    assert X.dtype == np.complex64 and np.fft.irfft(X, 16).dtype == F32


SMALL = [tr.Case("5x7", 5, 7, tr.ALL3, False, False), tr.Case("7x5", 7, 5, tr.ALL3, False, False), tr.Case("1x6", 1, 6, tr.ALL3, False, False),
         tr.Case("6x1", 6, 1, tr.ALL3, False, False), tr.Case("1x1", 1, 1, tr.ALL3, False, False), tr.Case("2x1", 2, 1, tr.ALL3, False, False),
         tr.Case("33x20", 33, 20, tr.ALL3, False, False), tr.Case("sym9", 9, 9, tr.ALL3, False, True), tr.Case("sym1", 1, 1, tr.ALL3, False, True),
         tr.Case("c1", 1, 1, ("spikes", "shift"), True, False), tr.Case("c2", 2, 2, ("spikes", "shift"), True, False),
         tr.Case("c7", 7, 7, ("spikes", "shift"), True, False), tr.Case("c12", 12, 12, ("spikes", "shift"), True, False)]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.tag)
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: d.__name__)
def test_references_against_the_dense_matrix(oracle, case, dt):
    for kind in case.kinds:
        for v in tr.kind_variants(case, kind, dt):
            inp = tr.inputs(case, kind, dt, v)
            vr = inp.vc if case.symmetric else inp.vr
            D = oracle.toeplitz_dense(inp.vc, None if case.circulant else vr, circulant=case.circulant)
            assert D.shape == (case.n, case.m)
            ref = D @ inp.a.astype(F64)
            assert np.max(np.abs(ref - inp.t)) <= 1e-13 * max(1.0, np.max(np.abs(ref))), (case.tag, kind, v)
            # the same-precision embedding computes the same product (to the bound), and its norms are those of the embedding
            for al, be in tr.ALPHA_BETA:
                want, bound = tr.want_and_bound(case, dt, inp, al, be)
                assert np.allclose(want, al * ref + be * inp.y0.astype(F64), rtol=0, atol=1e-13 * max(1.0, np.max(np.abs(ref))))
            c = np.concatenate([inp.vc, vr[1:]]) if not case.circulant else inp.vc
            assert math.isclose(inp.cnorm, float(np.linalg.norm(c.astype(F64))), rel_tol=1e-14)


TABLE = tr.ROUTE_TABLE


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: d.__name__)
def test_route_map_of_the_case_list(dt):
    """Every case sits on the route the table gives its embedding; each fast class has a case with n > N / 2 and one with m > N / 2."""
    seen = {}
    for case in tr.cases(dt):
        rt = tr.route(case.n, case.m, dt)
        assert rt.N == tr.next_pow2(max(case.n + case.m - 1, 2))
        lg = int(math.log2(rt.N))
        if lg < 13 or (lg == 13 and dt == F32):
            assert not rt.fast and rt.row == "rocfft", case
            continue
        n1, Mp, row, swz = TABLE[lg]
        assert (rt.fast, rt.n1, rt.Mp, rt.row, rt.swizzled) == (True, n1, Mp, row, swz[0 if dt == F64 else 1]), (case, rt)
        assert rt == tr.expected_route(case.n, case.m, dt)
        assert rt.n1 * rt.Mp * 2 == rt.N
        s = seen.setdefault(lg, set())
        if case.n > rt.N // 2:
            s.add("n")
        if case.m > rt.N // 2:
            s.add("m")
    assert sorted(seen) == list(range(13 if dt == F64 else 14, 24 if dt == F64 else 25))
    for lg, s in seen.items():
        assert s == {"n", "m"} or (lg == 24 and s == {"m"}), (lg, s)       # 2^24: the full shape only
    assert {tr.route(c.n, c.m, dt).n1 for c in tr.cases(dt)} >= ({0, 512, 1024, 2048} if dt == F32 else {512, 1024})
    assert {tr.route(c.n, c.m, dt).swizzled for c in tr.cases(dt) if tr.route(c.n, c.m, dt).fast} == {False, True}
    c = [c for c in tr.cases(dt) if c.tag == "4097x4096"][0]
    assert tr.route(c.n, c.m, dt).N == 8192 and tr.route(c.n, c.m, dt).fast == (dt == F64)
    for c in tr.circulant_cases():
        assert tr.route(c.n, c.m, dt, True) == tr.Route(c.n, False, 0, 0, "rocfft", False)


def test_measured_kappa_is_32_times_the_recorded_ratio():
    for dt in DTYPES:
        assert sorted(tr.NUMPY_RATIO[dt]) == list(range(tr.fast_min_lg(dt), 24 if dt == F64 else 25))
        assert math.isclose(tr.KAPPA_MEASURED[dt], 32 * max(tr.NUMPY_RATIO[dt].values()), rel_tol=1e-3), (dt, tr.KAPPA_MEASURED[dt])
        # raised on device evidence (toeplitz_ref.py), fivefold at most and on the embeddings up to 2^17 only
        assert tr.KAPPA_MEASURED[dt] <= tr.KAPPA_RAISED[dt] <= 5 * tr.KAPPA_MEASURED[dt]
        N0 = 1 << tr.fast_min_lg(dt)
        assert tr.kappa_of(dt, N0) == tr.kappa_of(dt, 1 << 17) == tr.KAPPA_RAISED[dt]
        assert tr.kappa_of(dt, 1 << 18) == tr.kappa_of(dt, 1 << 24) == tr.KAPPA_MEASURED[dt]
        assert math.isclose(tr.kappa_of(dt, N0 // 4), 2 * tr.KAPPA_MEASURED[dt])


HOST_LG = list(range(13, 21))


def _host_cases(dt, lg):
    """The device cases with the embedding 2^lg; lg = 0: the ones below 2^13 and the circulants."""
    out = []
    for case in tr.cases(dt) + tr.circulant_cases():
        N = tr.embedding(case.n, case.m, case.circulant)
        small = case.circulant or N < 8192
        if (lg == 0 and small) or (lg and not small and N == 1 << lg):
            out.append(case)
    return out


@pytest.mark.parametrize("lg", [0] + HOST_LG)
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: d.__name__)
def test_numpy_embedding_has_headroom(dt, lg):
    """numpy's embedding in the precision of the case uses at most 1/16 of what kappa allows, at both (alpha, beta): the device may be
    sixteen times worse than pocketfft before a case fails.  On the shift kind, whose ||c|| = 1 leaves the norm-wise term no slack, it is
    1/4 (tests/toeplitz_ref.py says why those cases do not set KAPPA), and 1/8 at the circulant lengths that are no power of two, where
    pocketfft itself pays for mixed radices and, at the prime 4099, for Bluestein's three transforms (measured: 1/14 there).  The second term of the bound is the rounding of the result
    itself, which no implementation can undercut sixteen-fold: the headroom is on the measured term.  The recorded ratios are met."""
    u = tr.unit_roundoff(dt)
    worst = 0.0
    for case in _host_cases(dt, lg):
        N = tr.embedding(case.n, case.m, case.circulant)
        for kind in case.kinds:
            for v in tr.kind_variants(case, kind, dt):
                inp = tr.inputs(case, kind, dt, v)
                if lg >= tr.fast_min_lg(dt) and kind in tr.MEASURED_KINDS:
                    worst = max(worst, tr.net_ratio(case, dt, inp))
                for al, be in tr.ALPHA_BETA:
                    want, bound = tr.want_and_bound(case, dt, inp, al, be)
                    rounding = 2 * u * (np.abs(al * inp.t) + np.abs(be * inp.y0.astype(F64)))
                    err = np.abs(tr.emulate(case, dt, inp, al, be).astype(F64) - want)
                    room = 4 if kind == "shift" else (16 if N & (N - 1) == 0 else 8)
                    over = err - ((bound - rounding) / room + rounding)
                    assert np.all(over <= 0), (case.tag, kind, v, al, float(np.max(err / np.maximum(bound, 1e-300))))
    if lg >= tr.fast_min_lg(dt):
        print(f"numpy ratio {dt.__name__} 2^{lg}: {worst:.4g} (recorded {tr.NUMPY_RATIO[dt][lg]:.4g})")
        # pocketfft's roundings depend on how numpy was built for the host (vector width); the recorded ratio is met to a quarter
        assert worst <= tr.NUMPY_RATIO[dt][lg] * 1.25


# 0: every case below 2^13 and the circulants; then the tall, wide and full shapes of an embedding — 2^13 .. 2^17 carry KAPPA_RAISED, 2^18
# and 2^20 KAPPA_MEASURED; the largest is where the bound is loosest against a defect (2^22 .. 2^24: toeplitz_ref.SHARPNESS_ABOVE_2_20)
SHARP_LG = [0, 13, 14, 15, 16, 17, 18, 20]


@pytest.mark.parametrize("lg", SHARP_LG)
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: d.__name__)
def test_planted_defects_exceed_four_times_the_bound(dt, lg):
    """Sharpness, a condition on kappa: on the spikes and shift inputs, each defect planted into the same-precision emulation pushes at
    least one entry over 4 x bound — on EVERY case whose exact product the defect changes at all (the fp64 emulation with the defect
    tells; e.g. zeroing the upper half of the input is no defect when m <= N / 2).  Every defect must be live on a tall and on a wide or
    full shape of every embedding, conjugation and the n / m swap on these non-symmetric rectangular shapes in particular; among the
    small cases (rocFFT lengths, circulants; kappa sqrt(N0 / N) there) it must be live somewhere.  The zeroed bin and the swapped pair are
    the MOST visible of their kind (the bin with the largest |C_k A_k|, the pair that differs most): their margins are best cases."""
    live = {d: set() for d in tr.DEFECTS}
    for case in _host_cases(dt, lg):
        shape = case.tag.split(":")[-1]
        if lg and shape not in ("tall", "wide", "full"):
            continue
        assert lg == 0 or (case.n != case.m and not case.symmetric)
        for kind in ("spikes", "shift"):
            vs = tr.kind_variants(case, kind, dt)
            if kind == "shift" and lg >= 18:                 # the identity and, per side, the largest shift: the long transforms cost
                vs = [vs[0]] + [max(x for x in vs if x[0] == w) for w in ("col", "row")]
            for v in vs:
                inp = tr.inputs(case, kind, dt, v)
                want, bound = tr.want_and_bound(case, dt, inp, 1.0, 0.0)
                inp64 = inp._replace(vc=inp.vc.astype(F64), vr=None if inp.vr is None else inp.vr.astype(F64), a=inp.a.astype(F64))
                for d in tr.DEFECTS:
                    exact = np.abs(tr.emulate(case, F64, inp64, defect=d) - want)
                    if np.max(exact) <= 1e-9 * (1 + np.max(np.abs(want))):
                        continue                             # vacuous here: the defect does not change this product
                    got = exact if dt == F64 else np.abs(tr.emulate(case, dt, inp, defect=d).astype(F64) - want)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        ratio = float(np.max(np.where(bound > 0, got / bound, np.where(got > 0, np.inf, 0.0))))
                    assert ratio > 4, (case.tag, kind, v, d, ratio)
                    live[d].add((shape, kind))
    for d, s in live.items():
        shapes_seen = {x[0] for x in s}
        if lg:
            assert "tall" in shapes_seen or d == "upper_input_zeroed", (d, s)
            assert shapes_seen & {"wide", "full"} or d == "upper_output_from_lower", (d, s)
        assert {x[1] for x in s} == {"spikes", "shift"}, (d, s)
