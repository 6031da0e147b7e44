"""Shared by tests/test_gpu_toeplitz.py (device) and tests/test_toeplitz_ref_host.py (no GPU): the inputs, the fp64 references, the
ENTRYWISE error bound, the route map and the case list of the Toeplitz / SymmetricToeplitz / Circulant MVM (csrc/toeplitz.hip).

    T[i, j] = vc[i - j] (i >= j),  vr[j - i] (i < j);    circulant: C[i, j] = vc[(i - j) mod n];    want = alpha T a + beta y0

Three kinds of input; every operand is rounded to the case's dtype FIRST, everything after that is fp64:

    spikes  vc, vr of magnitude [0.5, 1] with random signs; a = 16 entries of magnitude [1, 2] at the ends of a, either side of N/2 and
            on the first elements of the second tile row, zero elsewhere.  Reference: the sum of 16 scaled columns of T — no FFT, every
            row; an absent, doubled or misplaced term is at least 0.5 in size.
    shift   the generating vector is a unit impulse (first column e_p, first row e_p, or p = 0: the identity), a standard normal.
            Reference: a shifted, zero-filled (circulant: wrapped) copy of a — no arithmetic.
    dense   vc, vr as in spikes, a standard normal.  Reference: the oracle's fp64 circulant embedding, itself pinned at 64 rows by
            explicit fp64 dot products (to 1e-11) before anything is compared with it.

Bound (u = eps / 2 of the dtype, c = [vc, vr[1:]], N = the embedding the library uses: next_pow2(max(n + m - 1, 2)), circulant: n):

    |got_i - want_i|  <=  |alpha| kappa u log2(N) ||c||_2 ||a||_2  +  2 u (|alpha t_i| + |beta y0_i|)
    kappa = KAPPA_MEASURED[dtype] sqrt(N0 / N)    for N < N0 = 2^13 (fp64), 2^14 (fp32): the smallest embedding of the hand-written kernels
          = KAPPA_RAISED[dtype]                   for N0 <= N <= 2^17
          = KAPPA_MEASURED[dtype]                 above

The first term has the form of the FFT rounding-error result (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 24.2, with
the convolution's two forward transforms, product and inverse); the second covers the rounding of alpha t + beta y0 itself.  A rigorous
entrywise constant is 1e5 .. 1e7 times the error anybody sees, so KAPPA_MEASURED is measured — against a reference, not against the
code under test: the worst ratio  max_i |err_i| / (u log2(N) ||c|| ||a||)  of numpy's pocketfft embedding in the SAME precision (emulate() below)
over the case list of this module, times 32.  The 32: the constant grows linearly with the error of the twiddle factors (Higham's mu),
and the device builds its twiddles by chained complex multiplication (up to 15 roundings in rowfft16_fused_kernel, a two-level table
product in colfft16_kernel) where pocketfft's are correct to about u — allow 4; the other 8 is for a different factorisation (radix 16
and a four-step split against pocketfft's radix 4 / 2) and for the fluctuation of a maximum over up to 2^24 entries.

Which cases the ratio is taken over.  Two restrictions, both forced: without them the "measured" KAPPA is one at which the planted defects
of test_toeplitz_ref_host.py pass, and sharpness is the condition that may not give.
  * Embeddings: the power-of-two N from the smallest the hand-written kernels serve (N0 = 2^13 in fp64, 2^14 in fp32).  The ratio falls
    with N, so the smallest N sets it — and it falls like 1 / sqrt(N), to two digits over the whole table below (fp32: 0.00504 at 2^14,
    0.00249 at 2^16, 0.00128 at 2^18, ...): the norm-wise error the theorem bounds is spread over N entries.  A constant KAPPA therefore
    stops being a bound BELOW N0 (the rocFFT lengths 1 .. 512 and the circulants of the case list): at N = 2 it would allow 0.16 u ||c||
    ||a||, less than the two roundings of c_0 a_0 + c_1 a_1 done directly, and numpy's own embedding exceeds it 2.3-fold.  There the
    measured law is continued upwards, kappa = KAPPA_MEASURED sqrt(N0 / N) (fp32: 0.91 at N = 512, 15 at N = 2), never downwards: from N0 on
    kappa is the constant, although the ratio keeps falling.  Against that kappa numpy keeps its headroom of 16 at every small N of the
    list (asserted).  At N = 1 log2(N) = 0 and the second term alone is the bound.
  * Kinds: spikes and dense, whose generating vectors have full support: the inputs the form of the bound is made for.  In the shift kind c is ONE unit
    entry, ||c|| ||a|| has no sqrt(N) to spare, and the same pocketfft error is a ratio of 0.018 .. 0.080 (worst: 65536 x 1, c = e_1, a
    a single number: 1.3 u |a_0| on the rows where the product is exactly zero), against 0.0050 / 0.0137 for spikes and dense.  32 times
    0.080 is a KAPPA of 2.6, at which a zeroed spectrum bin passes in fp32 from about N = 2^18 on.
  The ratio is NET of the bound's second term: max_i (|err_i| - 2 u |t_i|)_+ / (u log2(N) ||c|| ||a||), since the rounding of the result
  is not the FFT's error.  Every case, of either restriction, is HELD to the same KAPPA; numpy's headroom under it is 16 on the measured
  kinds and 4 on the shift kind, both asserted on the host.

kappa is a condition: tests/test_toeplitz_ref_host.py asserts the headroom above and that each of seven planted defects exceeds 4 x bound,
at every small case and at the embeddings 2^13 .. 2^18 and 2^20; 2^22 .. 2^24 were run once (SHARPNESS_ABOVE_2_20 below).  It may be raised
above KAPPA_MEASURED only where the device needs it, when the error that needs it is spread (no isolated rows, no defect of one position)
and the planted defects still exceed 4 x bound at the raised value; the device figures that required it are recorded below."""
import functools
import math
from collections import namedtuple

import numpy as np

F32, F64 = np.float32, np.float64

# worst numpy same-precision ratio per embedding (numpy 2.2.6, pocketfft), this module's cases, both (alpha, beta); see measure_ratios()
NUMPY_VERSION_MEASURED = "2.2.6"
NUMPY_RATIO = {F32: {14: 0.005044, 15: 0.003858, 16: 0.002493, 17: 0.001833, 18: 0.001276, 19: 0.0008778, 20: 0.0006537, 21: 0.0004594,
                     22: 0.0003438, 23: 0.0002477, 24: 0.00016},
               F64: {13: 0.01367, 14: 0.008585, 15: 0.006759, 16: 0.004269, 17: 0.00315, 18: 0.002194, 19: 0.001532, 20: 0.001163,
                     21: 0.0008125, 22: 0.0006055, 23: 0.0004354}}
# the same for the shift kind (not part of KAPPA, see above): worst over the embeddings, at 65536 x 1 in both dtypes
NUMPY_RATIO_SHIFT = {F32: 0.08022, F64: 0.04011}
KAPPA_MEASURED = {F32: 32 * 0.005044, F64: 32 * 0.01367}          # 0.1614, 0.4374
# RAISED on device evidence, as the rule above provides, for the embeddings up to 2^RAISED_MAX_LG only.  With KAPPA_MEASURED every spikes and dense case and every wide and full shift
# passed on the MI355X (worst err / bound 0.62); seven shift cases with a short a (m = 1 and m = 101), all at 2^14 .. 2^17, did not: worst fp32 16384 x 1,
# c = e_16383, err / bound 1.99 (needs KAPPA 0.46), worst fp64 65536 x 1, c = e_65535, err / bound 1.28 (needs 0.60).  The pattern is no
# isolated row: the device returns every transported entry a_j with a RELATIVE error of a few ulps — 0, 1, 3, 5, 6 or 7 ulps of a_0 on
# N x 1 impulses, growing with the number of set bits of p (p = 0: exact; 1 and N / 2 + 1: 1 ulp; 4095, N - 2, N - 1: 5 to 7 ulps =
# 8.1 .. 11.3 u |a_0|), the SAME count of ulps in fp32 and fp64 and at 2^14 and 2^16; on the rows where the product is zero the error
# stays below 0.05 u log2(N) ||a||.  That is the signature of the chained twiddle powers (pow_chain16, the w *= w1 loops of the row
# kernels: their moduli drift from 1 by a few ulps, and a drift does not average out over the bins), which Higham's constant is linear
# in; numpy's table twiddles give 1 ulp.  With dense a the same few-ulp perturbations sit far below u log2(N) ||c|| ||a||; with ||c|| = 1
# and one to a hundred entries of a they ARE the bound's scale, and its second term allows 2 u |t_i| only.  Worst needs over all p
# probed (also p = 4095, N - 2): (9.72 - 2) / 14 = 0.55 in fp32, (11.34 - 2) / 14 = 0.67 in fp64; raised to
KAPPA_RAISED = {F32: 0.65, F64: 0.80}
RAISED_MAX_LG = 17
# From 2^18 on every case passed with KAPPA_MEASURED (closest: 262044 x 101 shifts in fp32, 0.98), and there it stays: raised to 2^24 as
# well, a zeroed bin would pass (fp32, multiples of the bound: 3.8 on the spikes input at 2^22, 1.1 at 2^24, 0.5 .. 0.9 on shifts).
# Sharpness with these values, fp32 (fp64 bounds are 5e8 times smaller): up to 2^20 asserted on the host, tightest a zeroed bin on a shift
# input at 2^20, 19 x bound.  2^22 .. 2^24, run once with emulate(defect=...), smallest multiple of the bound over the cases where the
# defect is live: every defect but the zeroed bin >= 200; the zeroed bin as below.  Both the zeroed bin and the swapped pair are the MOST
# visible instance (largest |C_k A_k|, most different pair): these are best cases, a typical bin is several times closer and passes in
# fp32 from about 2^20 on.  On SHIFT inputs from 2^22 on even the best bin stays under 4 x bound at KAPPA_MEASURED — one bin of 2^21 and
# more is a relative change of the product near fp32's resolution; the device's own error on those cases (0.74 of the bound at 2^22 tall,
# 0.76 at 2^23 tall) leaves no kappa that does both.
SHARPNESS_ABOVE_2_20 = {"bin_zeroed": {"2^22:tall spikes": 17.3, "2^22:full spikes": 15.3, "2^23:tall spikes": 8.15, "2^23:full spikes": 8.17,
                                       "2^24:full spikes": 4.39, "2^22:tall shift": 3.42, "2^22:full shift": 8.68, "2^23:tall shift": 2.72,
                                       "2^23:full shift": 4.09, "2^24:full shift": 2.11},
                        "every other defect, where live": 227}
# Largest err / bound on the MI355X with these values, all of tests/test_gpu_toeplitz.py (it prints the figure per case with -s):
GPU_WORST = {F32: 0.980, F64: 0.780}          # 262044 x 101, c = e_131073 (2^18, KAPPA_MEASURED); 65536 x 1, c = e_65535 (KAPPA_RAISED)

ALPHA_BETA = ((1.0, 0.0), (-0.7, 1.3))


def unit_roundoff(dt):
    return float(np.finfo(dt).eps) / 2


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def embedding(n, m, circulant=False):
    return n if circulant else next_pow2(max(n + m - 1, 2))


# ---- the route map: the rule of covgram_toeplitz_create / fast_mvm restated -------------------------------------------------
Route = namedtuple("Route", "N fast n1 Mp row swizzled")     # row: 'rocfft' | 'unfused' | 'radix4:L' | 'radix16'


def colfft_tw(dt):
    return 4 if dt == F64 else 8


def route(n, m, dt, circulant=False):
    N = embedding(n, m, circulant)
    Mh = N // 2
    n1 = 1024
    for cand in (1024, 512, 2048):
        if Mh % cand == 0 and Mh // cand in (64, 256, 1024, 4096):
            n1 = cand
            break
    fast = (not circulant) and Mh > 0 and Mh % n1 == 0 and Mh // n1 >= colfft_tw(dt)
    if not fast:
        return Route(N, False, 0, 0, "rocfft", False)
    Mp = Mh // n1
    L = {64: 3, 256: 4, 1024: 5, 4096: 6}.get(Mp, 0)
    row = "unfused" if not L else ("radix16" if L == 6 else "radix4:%d" % L)
    return Route(N, True, n1, Mp, row, (Mp // colfft_tw(dt)) % 16 == 0)


# log2(embedding): column length, row length, row kernel, swizzled tile map (fp64, fp32) — the sizes as csrc/toeplitz.hip reads today
ROUTE_TABLE = {13: (1024, 4, "unfused", (False, None)), 14: (1024, 8, "unfused", (False, False)), 15: (1024, 16, "unfused", (False, False)),
               16: (512, 64, "radix4:3", (True, False)), 17: (1024, 64, "radix4:3", (True, False)), 18: (512, 256, "radix4:4", (True, True)),
               19: (1024, 256, "radix4:4", (True, True)), 20: (512, 1024, "radix4:5", (True, True)), 21: (1024, 1024, "radix4:5", (True, True)),
               22: (512, 4096, "radix16", (True, True)), 23: (1024, 4096, "radix16", (True, True)), 24: (2048, 4096, "radix16", (True, True))}


def expected_route(n, m, dt, circulant=False):
    """The route ROUTE_TABLE gives the case — what the tests assert route() (the restated rule) against."""
    N = embedding(n, m, circulant)
    lg = int(math.log2(N)) if N > 0 else 0
    if circulant or N != 1 << lg or lg not in ROUTE_TABLE or ROUTE_TABLE[lg][3][0 if dt == F64 else 1] is None:
        return Route(N, False, 0, 0, "rocfft", False)
    n1, Mp, row, swz = ROUTE_TABLE[lg]
    return Route(N, True, n1, Mp, row, swz[0 if dt == F64 else 1])


# ---- cases ------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "tag n m kinds circulant symmetric")
ALL3 = ("spikes", "shift", "dense")


def shapes(N):
    """(tall, wide, full) of the embedding N: n + m - 1 = N each; full has n odd and m > N / 2."""
    return {"tall": (N - 100, 101), "wide": (37, N - 36), "full": (N // 2 - 37, N // 2 + 38)}


def cases(dt):
    """The Toeplitz cases of one dtype, smallest first."""
    out = []
    for lg in range(13, 25):
        N = 1 << lg
        sh = shapes(N)
        if lg <= 17:
            for s in ("tall", "wide", "full"):
                out.append(Case("2^%d:%s" % (lg, s), *sh[s], ALL3, False, False))
            if lg == 16 or lg == (13 if dt == F64 else 14):
                out.append(Case("2^%d:row" % lg, 1, N, ALL3, False, False))
                out.append(Case("2^%d:column" % lg, N, 1, ALL3, False, False))
        elif lg <= 21:
            for s in ("tall", "wide"):
                out.append(Case("2^%d:%s" % (lg, s), *sh[s], ("spikes", "shift"), False, False))
            out.append(Case("2^%d:full" % lg, *sh["full"], ALL3, False, False))
        elif lg <= 23:
            out.append(Case("2^%d:tall" % lg, *sh["tall"], ("spikes", "shift"), False, False))
            out.append(Case("2^%d:full" % lg, *sh["full"], ALL3, False, False))
        elif dt == F32:
            out.append(Case("2^24:full", *sh["full"], ("spikes", "shift"), False, False))
    out.append(Case("2^15:square", 9001, 9001, ALL3, False, False))              # the control: n = m odd, as every earlier test
    for n, m in ((300, 200), (200, 300), (1, 500), (500, 1), (1, 1), (2, 1), (4097, 4096)):
        out.append(Case("%dx%d" % (n, m), n, m, ALL3, False, False))
    return out


CIRCULANT_N = (1, 2, 3, 33, 1000, 4099, 16384)


def circulant_cases():
    return [Case("circulant:%d" % n, n, n, ("spikes", "shift"), True, False) for n in CIRCULANT_N]


def symmetric_case(N):
    """The largest SymmetricToeplitz of the embedding N (2n - 1 = N - 1)."""
    return Case("2^%d:symmetric" % int(math.log2(N)), N // 2, N // 2, ("spikes", "shift"), False, True)


def seed_of(case, kind, variant=None):
    s = "%s|%d|%d|%s|%s" % (case.tag, case.n, case.m, kind, variant)
    return int.from_bytes(s.encode(), "little") % (2 ** 63)


# ---- inputs (rounded to dt, returned as arrays of dtype dt) ------------------------------------------------------------------
def _signed(rng, k, lo, hi):
    return rng.uniform(lo, hi, k) * rng.choice([-1.0, 1.0], size=k)


def generating_vectors(rng, case, dt):
    vc = _signed(rng, case.n, 0.5, 1.0).astype(dt)
    if case.circulant or case.symmetric:
        return vc, None
    vr = _signed(rng, case.m, 0.5, 1.0).astype(dt)
    vr[0] = vc[0]
    return vc, vr


def spike_positions(rng, case, dt):
    n, m = case.n, case.m
    rt = route(n, m, dt, case.circulant)
    N = rt.N
    pos = [0, 1, m - 2, m - 1]
    if m > N // 2:
        pos += [N // 2 - 1, N // 2, N // 2 + 1]
    if rt.fast:
        pos += [2 * colfft_tw(dt) * rt.Mp - 1, 2 * colfft_tw(dt) * rt.Mp]
    pos += list(rng.integers(0, m, 16))
    seen = []
    for p in pos:
        p = int(min(max(p, 0), m - 1))
        if p not in seen:
            seen.append(p)
    return np.array(sorted(seen[:16]), dtype=np.int64)


def shift_variants(case, dt):
    """(where, p): 'col' = first column e_p (first row 0), 'row' = first row e_p (first column 0), 'id' = p = 0.  p from 1, the last
    index and just past N / 2 as the shape allows; symmetric and circulant operators have a first column only."""
    n, m = case.n, case.m
    N = embedding(n, m, case.circulant)
    big = N >= 1 << 22                               # one p per side there: just past N / 2, or the last index
    out = [("id", 0)]
    ps = (N // 2 + 1 if N // 2 + 1 < n else n - 1,) if big else (1, n - 1, N // 2 + 1)
    out += [("col", p) for p in sorted({p for p in ps if 1 <= p < n})]
    if not (case.circulant or case.symmetric):
        ps = (N // 2 + 1 if N // 2 + 1 < m else m - 1,) if big else (1, m - 1, N // 2 + 1)
        out += [("row", p) for p in sorted({p for p in ps if 1 <= p < m})]
    return out


Inputs = namedtuple("Inputs", "vc vr a y0 t cnorm anorm")   # vc, vr (None: first column only), a, y0 of dtype dt; t = T a in fp64


def _norms(case, vc, vr, a):
    c2 = float(np.sum(vc.astype(F64) ** 2))
    if case.symmetric:
        c2 += float(np.sum(vc[1:].astype(F64) ** 2))
    elif vr is not None:
        c2 += float(np.sum(vr[1:].astype(F64) ** 2))
    return math.sqrt(c2), float(np.linalg.norm(a.astype(F64)))


def spikes_reference(case, vc, vr, a, pos):
    """sum_j a_j T[:, j] over the spike positions, fp64."""
    n = case.n
    vc = vc.astype(F64)
    vr = vc if vr is None else vr.astype(F64)
    t = np.zeros(n)
    for j in pos:
        aj = float(a[j])
        if case.circulant:
            t += aj * np.roll(vc, j)
            continue
        k = min(j, n)                                # rows i < j: vr[j - i]
        if k:
            t[:k] += aj * vr[j:j - k:-1]
        if j < n:
            t[j:] += aj * vc[:n - j]
    return t


def shift_reference(case, a, where, p):
    n, m = case.n, case.m
    a = a.astype(F64)
    t = np.zeros(n)
    if case.circulant:
        return np.roll(a, p)
    if where == "id":
        k = min(n, m)
        t[:k] = a[:k]
        return t
    if where == "col" or case.symmetric:             # y_i = a_(i - p)
        k = min(n - p, m)
        if k > 0:
            t[p:p + k] += a[:k]
    if where == "row" or case.symmetric:             # y_i = a_(i + p)
        k = min(n, m - p)
        if k > 0:
            t[:k] += a[p:p + k]
    return t


def dense_row(vc, vr, a, i):
    """T[i, :] . a by an explicit fp64 dot product."""
    m = a.shape[0]
    k = min(i, m - 1)
    s = float(np.dot(vc[i - k:i + 1][::-1], a[:k + 1]))
    if i + 1 < m:
        s += float(np.dot(vr[1:m - i], a[i + 1:]))
    return s


def dense_check_rows(rng, case):
    n = case.n
    N = embedding(case.n, case.m, case.circulant)
    rows = [0, n - 1] + [r for r in (N // 2 - 1, N // 2, N // 2 + 1) if r < n]
    rows += list(rng.integers(0, n, 64))
    seen = []
    for r in rows:
        if int(r) not in seen:
            seen.append(int(r))
    return seen[:64]


@functools.lru_cache(maxsize=4)
def inputs(case, kind, dt, variant=None):
    """The operands and the fp64 product of one case.  Cached (the host and the device tests of one case share it); callers must not
    write into the arrays."""
    import covgram_oracle as oracle
    rng = np.random.default_rng(seed_of(case, kind, variant))
    n, m = case.n, case.m
    y0 = rng.standard_normal(n).astype(dt)
    if kind == "shift":
        where, p = variant
        vc = np.zeros(n, dtype=dt)
        vr = None if (case.circulant or case.symmetric) else np.zeros(m, dtype=dt)
        if where == "id":
            vc[0] = 1
            if vr is not None:
                vr[0] = 1
        elif where == "col":
            vc[p] = 1
        else:
            vr[p] = 1
        a = rng.standard_normal(m).astype(dt)
        t = shift_reference(case, a, where, p)
    else:
        vc, vr = generating_vectors(rng, case, dt)
        if kind == "spikes":
            pos = spike_positions(rng, case, dt)
            a = np.zeros(m, dtype=dt)
            a[pos] = _signed(rng, pos.shape[0], 1.0, 2.0).astype(dt)
            t = spikes_reference(case, vc, vr, a, pos)
        else:
            a = rng.standard_normal(m).astype(dt)
            vc64, a64 = vc.astype(F64), a.astype(F64)
            vr64 = vc64 if vr is None else vr.astype(F64)
            t = oracle.toeplitz_mul(None, vc64, None if vr is None else vr64, a64, circulant=case.circulant)
            rows = dense_check_rows(rng, case)
            direct = np.array([dense_row(vc64, vr64, a64, i) for i in rows])
            worst = float(np.max(np.abs(direct - t[rows])) / np.max(np.abs(direct)))
            assert worst <= 1e-11, ("the embedding reference disagrees with explicit dot products", case.tag, worst)
    cn, an = _norms(case, vc, vr, a)
    return Inputs(vc, vr, a, y0, t, cn, an)


def want_and_bound(case, dt, inp, alpha, beta, kappa=None):
    """(want, bound), fp64, every row."""
    u = unit_roundoff(dt)
    N = embedding(case.n, case.m, case.circulant)
    kappa = kappa_of(dt, N) if kappa is None else kappa
    at = alpha * inp.t
    by = beta * inp.y0.astype(F64) if beta != 0 else np.zeros_like(at)
    bound = abs(alpha) * kappa * u * math.log2(N) * inp.cnorm * inp.anorm + 2 * u * (np.abs(at) + np.abs(by))
    return at + by, bound


def fast_min_lg(dt):
    return 13 if dt == F64 else 14


def kappa_of(dt, N):
    """KAPPA_MEASURED[dt] sqrt(N0 / N) below the smallest measured embedding N0, KAPPA_RAISED[dt] from N0 to 2^RAISED_MAX_LG, the
    embeddings at which the device needed it, KAPPA_MEASURED[dt] above (the module docstring says why)."""
    N0 = 1 << fast_min_lg(dt)
    if N < N0:
        return KAPPA_MEASURED[dt] * math.sqrt(N0 / N)
    return KAPPA_RAISED[dt] if N <= 1 << RAISED_MAX_LG else KAPPA_MEASURED[dt]


def fft_term(case, dt, inp):
    """u log2(N) ||c|| ||a||: what KAPPA multiplies (alpha = 1)."""
    return unit_roundoff(dt) * math.log2(embedding(case.n, case.m, case.circulant)) * inp.cnorm * inp.anorm


# ---- numpy's embedding in the precision of the case, and the planted defects -------------------------------------------------
DEFECTS = ("drop_last", "upper_input_zeroed", "upper_output_from_lower", "n_m_swapped", "spectrum_conjugated", "bin_zeroed", "packed_pair_swapped")


def emulate(case, dt, inp, alpha=1.0, beta=0.0, defect=None):
    """alpha T a + beta y0 by the circulant embedding with every array and every transform in dtype dt (np.fft keeps float32 / complex64
    since numpy 2.0), optionally with one planted defect.  Returns an array of dtype dt."""
    n, m = case.n, case.m
    N = embedding(n, m, case.circulant)
    vc = inp.vc
    vr = vc if inp.vr is None else inp.vr
    c = np.zeros(N, dtype=dt)
    ap = np.zeros(N, dtype=dt)
    if case.circulant:
        c[:] = vc
    elif defect == "n_m_swapped":                    # the column part gets m entries and the row part n - 1
        k = min(m, n)
        c[:k] = vc[:k]
        k = min(n, m) - 1
        if k > 0:
            c[N - k:] = vr[1:k + 1][::-1]
    else:
        c[:n] = vc
        if m > 1:
            c[N - (m - 1):] = vr[1:][::-1]
    ap[:m] = inp.a
    if defect == "drop_last":
        ap[m - 1] = 0
    if defect == "upper_input_zeroed":
        ap[N // 2:] = 0
    if defect == "packed_pair_swapped" and N >= 2:   # the pair whose two elements differ most
        k = (N // 2) * 2
        j = int(np.argmax(np.abs(ap[0:k:2] - ap[1:k:2])))
        ap[2 * j], ap[2 * j + 1] = ap[2 * j + 1], ap[2 * j]
    C = np.fft.rfft(c)
    A = np.fft.rfft(ap)
    assert C.dtype == (np.complex64 if dt == F32 else np.complex128), C.dtype
    if defect == "spectrum_conjugated":
        C = np.conj(C)
    if defect == "bin_zeroed":                       # the bin that carries most of the product
        C[int(np.argmax(np.abs(C) * np.abs(A)))] = 0
    t = np.fft.irfft(C * A, N)
    assert t.dtype == dt, t.dtype
    if defect == "upper_output_from_lower":
        t[N // 2:] = t[:N - N // 2]
    t = t[:n]
    out = (dt(alpha) * t).astype(dt)
    if beta != 0:
        out = (out.astype(F64) + float(dt(beta)) * inp.y0.astype(F64)).astype(dt)      # one rounding, as a fused multiply-add
    return out


def kind_variants(case, kind, dt):
    return shift_variants(case, dt) if kind == "shift" else [None]


def net_ratio(case, dt, inp):
    """max_i (|err_i| - 2 u |t_i|)_+ / (u log2(N) ||c|| ||a||) of emulate() at alpha = 1, beta = 0: the part of numpy's error that the
    second term of the bound does not already allow."""
    err = np.abs(emulate(case, dt, inp).astype(F64) - inp.t) - 2 * unit_roundoff(dt) * np.abs(inp.t)
    return max(float(np.max(err)), 0.0) / fft_term(case, dt, inp)


MEASURED_KINDS = ("spikes", "dense")


def measure_ratios(dt, max_lg=24, kinds=MEASURED_KINDS):
    """{log2 N: worst net_ratio} over the given kinds of cases(dt) with 2^fast_min_lg(dt) <= N <= 2^max_lg."""
    out = {}
    for case in cases(dt):
        lg = int(math.log2(embedding(case.n, case.m)))
        if not fast_min_lg(dt) <= lg <= max_lg:
            continue
        for kind in case.kinds:
            if kind not in kinds:
                continue
            for v in kind_variants(case, kind, dt):
                out[lg] = max(out.get(lg, 0.0), net_ratio(case, dt, inputs(case, kind, dt, v)))
    return out
