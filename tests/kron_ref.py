"""Shared by tests/test_gpu_kron.py (device) and tests/test_kron_ref_host.py (no GPU): the planner of the Kronecker MVM restated, the fp64
reference with its ENTRYWISE error bound, and the case table.

    y <- alpha (F_1 (x) ... (x) F_q) a + beta y0,        F_k: r_k x c_k, F_1 the slowest index        (csrc/kron.hip, csrc/kron_kernels.hpp)

plan() restates which kernels, in which order and with which template arguments, covgram_kron_mvm launches for a shape; the library
reports the same through the info keys "last_kron_path" and "last_kron_arms", and the device tests hold the two against each other for
every case — a planner change that is not carried over here fails there, it does not silently empty a case of its purpose.

Bound (u = eps / 2 of the dtype; |.| entrywise):

    |got - want|  <=  gamma_n |alpha| (|F_1| (x) ... (x) |F_q|) |a|  +  u (|want| + 2 |beta y0|),      gamma_n = n u / (1 - n u),
    n = sum_k c_k + q + 2

Each output entry is a sum of prod_k c_k terms alpha F_1[o1, i1] ... F_q[oq, iq] a[i]; computed mode by mode a term passes through one
dot product of length c_k per mode — at most c_k roundings whatever the order of that sum (Higham, Accuracy and Stability of Numerical
Algorithms, section 3.1: the multiplication and at most c_k - 1 additions; a fused multiply-add chain and the two partial sums of the
fused pass have fewer) —, one more rounding per mode for what is stored in between or for the multiplied-out pair of small trailing
factors (the q), and the multiplications by alpha and beta (the 2); (1 + u)^n - 1 <= gamma_n.  The second term is the rounding of the
result itself and of beta y0.  The order of the modes does not enter, nor does the summation order inside a mode: the library GEMM modes
are covered too.  One route changes n: two trailing factors multiplied out (path bit 16) run ONE dot product of length c_{q-1} c_q
<= 256 in place of two of lengths c_{q-1} and c_q; for a plan that does so terms(merged=True) counts that product instead of the sum.

NORM_TOL is the norm-wise tolerance the suite held these products to before the entrywise bound existed, || got - want || / || want || <=
NORM_TOL sqrt(max(1, max_k c_k / 16)) over the whole result: kept beside the bound, since a worst-case entrywise bound at c_k >= 256 leaves
room for a uniform loss of several bits that the norm does not.

Inputs: standard normal factors, a and y0, rounded to the case's dtype first; ASYMMETRIC factors (a transposed kernel, or one that
swaps rows and columns of a factor, fails).  Everything after the rounding is fp64 (oracle/covgram_oracle.py::kron_mul)."""
import math
import zlib
from collections import namedtuple

import numpy as np

import covgram_oracle as oracle

F32, F64 = np.float32, np.float64
ALPHA_BETA = ((1.0, 0.0), (-0.7, 1.3))
NORM_TOL = {F32: 2e-6, F64: 1e-13}


def norm_tol(shapes, dt):
    return NORM_TOL[dt] * max(1.0, math.sqrt(max(s[1] for s in shapes) / 16.0))


# ---- csrc/kron_limits.hpp:9-14, csrc/kron.hip:91,102-104 -----------------------------------------------------------------------------
PAIR_MAX_K2 = 128
PAIR_MIN_SIDE = 48
MERGE_MAX_SIDE = 256
BLAS_MIN_SIDE = 1024
BLAS_MID_SIDE = 256
BLAS_MID_FLOPS = 2.0e9

# "last_kron_path" bits (csrc/common.hpp, covgram_ctx::last_kron_path)
PATH_PAIR, PATH_MODE, PATH_MODET, PATH_BLAS, PATH_MERGED = 1, 2, 4, 8, 16


def span_ok(rows, stride):
    return rows * stride < (1 << 31)


def pair_ok(K1, K2, ld2, ld3):
    return K2 <= PAIR_MAX_K2 and span_ok(128, ld3) and span_ok(K1, ld2)


def mode_ok(K, post, ld):
    return span_ok(16, post) and span_ok(K, ld)


def modet_ok(K, ld):
    return span_ok(128, K) and span_ok(K, ld)


# ---- "last_kron_arms" bits (csrc/kron_kernels.hpp: arm_bit_pair / arm_bit_mode / arm_bit_modet) -------------------------------------
def arm_bit(kernel, arm):
    if arm is None:                            # the library GEMM and the multiplied-out pair have no arms
        return 0
    n, w, vec = arm
    if kernel == "pair":                       # (NB1, NB2, VEC)
        return 1 << ((4 if n == 8 else 0) + (2 if w == 8 else 0) + int(vec))
    if kernel == "mode":                       # (NBP, NW, VEC)
        return 1 << (8 + {2: 0, 4: 4, 8: 8}[n] + (2 if w == 8 else 0) + int(vec))
    if kernel == "modet":                      # (NBB, NW, VEC)
        return 1 << (20 + (4 if n == 8 else 0) + (2 if w == 8 else 0) + int(vec))
    return 0


ALL_ARMS = ([("pair", (a, b, v)) for a in (4, 8) for b in (4, 8) for v in (False, True)]
            + [("mode", (a, b, v)) for a in (2, 4, 8) for b in (4, 8) for v in (False, True)]
            + [("modet", (a, b, v)) for a in (2, 8) for b in (4, 8) for v in (False, True)])

Pass = namedtuple("Pass", "kernel arm k pre post M K final")      # pair: k = q - 2, post = 1, M = (M1, N2), K = (K1, K2)
Plan = namedtuple("Plan", "passes path arms pair_first")


def pick_nw(strips, units, num_cus, minnw=4, maxnw=8):
    """csrc/kron_kernels.hpp pick_nw."""
    nw = minnw
    while nw < maxnw and nw < strips:
        nw *= 2
    while nw > minnw and units * ((strips + nw - 1) // nw) < num_cus:
        nw //= 2
    return nw


def pair_arm(dt, K2, N2, ld3, in_aligned, f_aligned=True):
    """csrc/kron_kernels.hpp run_pair: NB1 by the slab's row blocks, NB2 by the width of the last factor, VEC by 16-byte alignment."""
    vw = 16 // np.dtype(dt).itemsize
    vec = in_aligned and K2 % vw == 0 and f_aligned and ld3 % vw == 0 and N2 % vw == 0
    return (4 if (K2 + 15) // 16 <= 4 else 8, 8 if N2 > 64 else 4, vec)


def mode_arm(dt, M, pre, post, num_cus, in_aligned):
    """csrc/kron_kernels.hpp run_mode (option kron_fill at its default 1)."""
    vw = 16 // np.dtype(dt).itemsize
    vec = in_aligned and post % vw == 0
    strips = (M + 15) // 16
    nbp = 8
    while nbp > 2 and (16 * nbp // 2 >= post or pre * ((post + 16 * nbp - 1) // (16 * nbp)) < num_cus):
        nbp //= 2
    ntiles = (post + 16 * nbp - 1) // (16 * nbp)
    return (nbp, pick_nw(strips, pre * ntiles, num_cus), vec)


def modet_arm(dt, M, K, pre, num_cus, in_aligned):
    """csrc/kron_kernels.hpp run_modet: accesses of 16 bytes in fp64, 8 in fp32 (modet_vb) — two elements either way."""
    vec = in_aligned and K % 2 == 0
    strips = (M + 15) // 16
    nbb = 8 if (pre >= 128 and (pre + 127) // 128 >= num_cus) else 2
    ntiles = (pre + 16 * nbb - 1) // (16 * nbb)
    return (nbb, pick_nw(strips, ntiles, num_cus), vec)


def plan(shapes, dt, nrhs, num_cus, lds=None, a_aligned=True):
    """kron_run (csrc/kron.hip:107-187) restated.  shapes: [(r_k, c_k)]; nrhs = 0: a vector (one tensor), else that many tensors one after
    the other; lds: leading dimensions of the column-major factors (default: their rows); a_aligned: whether the input tensor starts on
    a 16-byte boundary (False: one element past one — the intermediates live in the library's workspace and always are)."""
    rows = [int(s[0]) for s in shapes]
    cols = [int(s[1]) for s in shapes]
    lds = list(lds) if lds is not None else list(rows)
    return _plan(rows, cols, lds, dt, max(int(nrhs), 1), num_cus, a_aligned, True)


def _plan(rows, cols, lds, dt, batch, num_cus, a_aligned, may_merge):
    q = len(rows)
    fp32 = np.dtype(dt).itemsize == 4
    total_in = float(batch)
    for c in cols:
        total_in *= c

    def big(k):                                                                         # kron.hip:119-122
        side = max(rows[k], cols[k])
        return side >= BLAS_MIN_SIDE or (side >= BLAS_MID_SIDE and 2.0 * total_in * rows[k] >= BLAS_MID_FLOPS)

    pre2 = batch * math.prod(rows[:max(q - 2, 0)])                                      # :124-127
    pre2_first = batch * math.prod(cols[:max(q - 2, 0)])
    pair = q >= 2 and not big(q - 1) and not big(q - 2) and pair_ok(cols[q - 2], cols[q - 1], lds[q - 2], lds[q - 1])     # :128
    pair_first = pair and q > 2 and rows[q - 2] * rows[q - 1] < cols[q - 2] * cols[q - 1]                                  # :130
    if fp32 and q >= 2 and max(rows[q - 2], cols[q - 2], rows[q - 1], cols[q - 1]) <= 64:                                   # :134
        pair = False
    if pair:                                                                            # :135-140
        units = (pre2_first if pair_first else pre2) * ((rows[q - 2] + 63) // 64)
        if units < num_cus // 2:
            pair = False
        if rows[q - 2] < PAIR_MIN_SIDE or cols[q - 1] < PAIR_MIN_SIDE:
            pair = False
    if not pair and q >= 2 and rows[q - 2] * rows[q - 1] <= MERGE_MAX_SIDE and cols[q - 2] * cols[q - 1] <= MERGE_MAX_SIDE and may_merge:   # :143-153
        r, c = rows[q - 2] * rows[q - 1], cols[q - 2] * cols[q - 1]
        sub = _plan(rows[:q - 2] + [r], cols[:q - 2] + [c], lds[:q - 2] + [r], dt, batch, num_cus, a_aligned, False)
        return Plan([Pass("merged", None, q - 2, 1, 1, (rows[q - 2], rows[q - 1]), (cols[q - 2], cols[q - 1]), False)] + sub.passes,
                    sub.path | PATH_MERGED, sub.arms, False)
    passes, path, arms = [], 0, 0
    aligned = a_aligned
    cur = list(cols)
    nsingle = q - 2 if pair else q

    def pair_pass(pre, final):
        arm = pair_arm(dt, cols[q - 1], rows[q - 1], lds[q - 1], aligned)
        return Pass("pair", arm, q - 2, pre, 1, (rows[q - 2], rows[q - 1]), (cols[q - 2], cols[q - 1]), final)

    if pair:
        path |= PATH_PAIR
    if pair and pair_first:                                                             # :156-163
        passes.append(pair_pass(pre2_first, nsingle == 0))
        cur[q - 2], cur[q - 1] = rows[q - 2], rows[q - 1]
        aligned = True
    for k in range(nsingle):                                                            # :164-178
        pre = batch * math.prod(rows[:k])
        post = math.prod(cur[k + 1:])
        final = k == nsingle - 1 and not (pair and not pair_first)
        fits = modet_ok(cols[k], lds[k]) if post == 1 else mode_ok(cols[k], post, lds[k])
        if big(k) or not fits:
            passes.append(Pass("blas", None, k, pre, post, rows[k], cols[k], final))
            path |= PATH_BLAS
        elif post == 1:
            passes.append(Pass("modet", modet_arm(dt, rows[k], cols[k], pre, num_cus, aligned), k, pre, 1, rows[k], cols[k], final))
            path |= PATH_MODET
        else:
            passes.append(Pass("mode", mode_arm(dt, rows[k], pre, post, num_cus, aligned), k, pre, post, rows[k], cols[k], final))
            path |= PATH_MODE
        cur[k] = rows[k]
        aligned = True
    if pair and not pair_first:                                                         # :179-183
        passes.append(pair_pass(pre2, True))
    for p in passes:
        arms |= arm_bit(p.kernel, p.arm)
    return Plan(passes, path, arms, bool(pair and pair_first))


def blas_rule(p, shapes, nrhs):
    """Which rule sent a library-GEMM pass there, big() of kron.hip:119-122 recomputed: 'min' (a side >= 1024), 'mid' (a side >= 256 with
    >= 2e9 flops in the mode), or 'refused' (neither: a shape the kernels do not take, kron_limits.hpp)."""
    assert p.kernel == "blas"
    side = max(p.M, p.K)
    if side >= BLAS_MIN_SIDE:
        return "min"
    total_in = float(max(int(nrhs), 1)) * math.prod(float(s[1]) for s in shapes)
    if side >= BLAS_MID_SIDE and 2.0 * total_in * p.M >= BLAS_MID_FLOPS:
        return "mid"
    return "refused"


def describe(pl):
    out = []
    for p in pl.passes:
        out.append(p.kernel + ("" if p.arm is None else "<%d,%d,%s>" % (p.arm[0], p.arm[1], "V" if p.arm[2] else "s")) + "[k=%d pre=%d post=%d]" % (p.k, p.pre, p.post))
    return " -> ".join(out) + " path=%d" % pl.path


# ---- reference and bound -------------------------------------------------------------------------------------------------------------
def unit_roundoff(dt):
    return float(np.finfo(dt).eps) / 2


def gamma(n, u):
    return n * u / (1.0 - n * u)


def terms(Fs, merged=False):
    """n of the bound: one dot product of length c_k per mode, one rounding per intermediate / multiplied-out pair, alpha and beta.
    merged: the plan multiplies the two trailing factors out (path bit 16, kron.hip:143-153) — they then run as ONE dot product of length
    c_{q-1} c_q (<= 256), which is what a term passes through there, in place of c_{q-1} + c_q; the rounding of the product
    F_{q-1}[.,.] F_q[.,.] itself is one of the q."""
    cs = [int(F.shape[1]) for F in Fs]
    if merged and len(cs) >= 2:
        cs = cs[:-2] + [cs[-2] * cs[-1]]
    return sum(cs) + len(Fs) + 2


def _columns(x):
    x = np.asarray(x)
    return [x] if x.ndim == 1 else [x[:, c] for c in range(x.shape[1])]


def _apply(Fs, a):
    """(F_1 (x) ... (x) F_q) a in fp64 through the oracle, column by column."""
    out = np.stack([oracle.kron_mul(None, Fs, c) for c in _columns(a)], axis=-1)
    return out[:, 0] if np.asarray(a).ndim == 1 else out


def want_and_bound(Fs, a, y0, alpha, beta, dt, cache=None, merged=False):
    """(want, bound) per output entry, fp64, shaped like y0.  cache: a dict that keeps the two operator applications (K a, |K| |a|)
    between the (alpha, beta) of one case.  merged: see terms()."""
    cache = {} if cache is None else cache
    if "t" not in cache:
        cache["t"] = _apply(Fs, a)
        cache["tabs"] = _apply([np.abs(np.asarray(F, dtype=np.float64)) for F in Fs], np.abs(np.asarray(a, dtype=np.float64)))
    t, tabs = cache["t"], cache["tabs"]
    y0 = np.asarray(y0, dtype=np.float64)
    want = alpha * t                                      # oracle.kron_mul's own last two statements
    if beta != 0:
        want = want + beta * y0
    u = unit_roundoff(dt)
    by = np.abs(beta * y0) if beta != 0 else 0.0          # beta == 0: y0 is not read (it may be NaN)
    bound = gamma(terms(Fs, merged), u) * abs(alpha) * tabs + u * (np.abs(want) + 2.0 * by)
    return want, bound


def emulate(Fs, a, y0, alpha, beta, dt):
    """The product mode by mode with every operand, intermediate and the result in dt (numpy's own summation order): what a plain
    same-precision implementation gives.  The host test holds it to the bound."""
    a = np.asarray(a, dtype=dt)
    vec = a.ndim == 1
    cols = [F.shape[1] for F in Fs]
    t = (a.reshape(cols + [1]) if vec else a.reshape(cols + [a.shape[1]])).astype(dt)
    for ax, F in enumerate(Fs):
        t = np.moveaxis(np.tensordot(np.asarray(F, dtype=dt), t, axes=([1], [ax])), 0, ax).astype(dt)
    t = t.reshape(-1) if vec else t.reshape(-1, a.shape[1])
    out = (dt(alpha) * t).astype(dt)
    if beta != 0:
        out = (out + (dt(beta) * np.asarray(y0, dtype=dt)).astype(dt)).astype(dt)
    return out


def coordinates(index, shapes, nrhs):
    """(o_1, ..., o_q[, column]) of a flat row-major index into y of shape (prod r_k,) or (prod r_k, nrhs)."""
    dims = [s[0] for s in shapes] + ([nrhs] if nrhs else [])
    return tuple(int(v) for v in np.unravel_index(int(index), dims))


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "tag shapes nrhs dts why")
BOTH = (F64, F32)


def _c(tag, shapes, why, nrhs=0, dts=BOTH):
    return Case(tag, [tuple(s) for s in shapes], nrhs, tuple(dts), why)


def _pairk1(K1):
    """Stage 1 of the fused pass walks ceil(K1 / 32) chunks in rounds of D register sets; K2 = 48: NB1 = 4, D = 2."""
    why = {1: "one row: n1 = 1 < n1p = 2", 31: "less than one chunk", 32: "exactly one chunk", 33: "one row into the second chunk: n1 = n1p = 2",
           97: "four chunks, the last of one row", 129: "five chunks: n1 = 5 < n1p = 6"}[K1]
    return _c("pair-K1=%d" % K1, [(128, 2), (64, K1), (108, 48)], "fused pass <4,8>, K1 = %d — %s" % (K1, why))


CASES = [
    # ---- every case tests/test_gpu_kron.py had (what each reaches at 256 CUs is what plan() says; the host test prints it)
    _c("128^3", [(128, 128)] * 3, "README.md:205-210: one mode pass + pair<8,8,V>"),
    _c("64^3", [(64, 64)] * 3, "64 slabs are too few for the fused pass: mode by mode"),
    _c("32^3", [(32, 32)] * 3, "mode by mode"),
    _c("16^4", [(16, 16)] * 4, "two trailing 16 x 16 factors multiplied out"),
    _c("20,36,52", [(20, 24), (36, 40), (52, 56)], "r_{q-1} = 36 < 48: mode by mode, ragged strips"),
    _c("7,130,96", [(7, 5), (130, 100), (96, 112)], "21 units: mode by mode, M = 130 (9 strips)"),
    _c("9,33,200", [(9, 11), (33, 17), (200, 31)], "mode by mode, unaligned rows (post = 31)"),
    _c("3,48,300", [(3, 4), (48, 128), (300, 128)], "3 units: mode by mode, M = 300"),
    _c("40,100", [(40, 40), (100, 90)], "q = 2 with one slab: the separate-modes route (also swallowed by a comment in test_kron_paths_by_shape)"),
    _c("500,17,23", [(500, 3), (17, 19), (23, 29)], "pre = 500, small odd trailing factors"),
    _c("2,120,16", [(2, 300), (120, 16), (16, 120)], "4 units: mode by mode although the pair would shrink the tensor"),
    _c("37x41", [(37, 41)], "q = 1"), _c("200x513", [(200, 513)], "q = 1, K = 513"), _c("1x1", [(1, 1)], "q = 1, a scalar"), _c("16x4", [(16, 4)], "q = 1"),
    _c("30,50", [(30, 200), (50, 150)], "c_q = 150 > 128: mode + modet"),
    _c("129,129", [(129, 129), (129, 129)], "one past the tile everywhere"),
    _c("5,3x260", [(5, 7), (3, 260)], "K = 260 in the last mode"),
    _c("64,256", [(64, 64), (256, 256)], "c_q = 256 > 128"),
    _c("q5-tiny", [(6, 5), (4, 3), (2, 7), (3, 2), (5, 4)], "q = 5, tiny and odd everywhere"),
    _c("1,9,4", [(1, 9), (9, 1), (4, 4)], "sides of one"),
    _c("256,256", [(256, 256), (256, 256)], "c_q = 256: mode + modet"),
    _c("8^3-rhs3", [(8, 8)] * 3, "matrix right-hand side", nrhs=3),
    _c("20,36,52-rhs2", [(20, 24), (36, 40), (52, 56)], "matrix right-hand side, mode route", nrhs=2),
    _c("37x41-rhs5", [(37, 41)], "matrix right-hand side, q = 1", nrhs=5),
    _c("30,50-rhs4", [(30, 200), (50, 150)], "matrix right-hand side, mode + modet", nrhs=4),
    _c("5,33,40", [(5, 6), (33, 20), (40, 70)], "the raw-ABI shape"),
    _c("1024,24", [(1024, 1030), (24, 40)], "rocBLAS by the side >= 1024 rule, post > 1"),
    _c("12,1100", [(12, 10), (1100, 1024)], "rocBLAS by the side >= 1024 rule, post = 1"),
    _c("300x200", [(300, 200)], "q = 1: the last-mode kernel alone"),
    # ---- the two cases a comment swallowed besides (40, 40), (100, 90)
    _c("32^4", [(32, 32)] * 4, "swallowed by a comment in test_kron_paths_by_shape"),
    _c("16^5", [(16, 16)] * 5, "swallowed by a comment in test_kron_paths_by_shape"),
    # ---- the fused pass, arm by arm
    _c("pair<4,4,s>-f64", [(128, 3), (48, 20), (33, 50)], "NB1 = NB2 = 4, ld3 = 33: unaligned", dts=(F64,)),
    _c("pair<4,4,s>-f32", [(128, 3), (70, 20), (33, 50)], "fp32 needs a side above 64; M1 = 70: two strip groups, the second ragged", dts=(F32,)),
    _c("pair<4,8,V>", [(128, 2), (48, 40), (100, 64)], "NB1 = 4, NB2 = 8, aligned"),
    _c("pair<8,4,s>", [(128, 2), (50, 33), (48, 65)], "NB1 = 8, NB2 = 4, ragged last strip, K2 = 65"),
    _c("pair<8,8>-3chunks", [(64, 2), (65, 31), (257, 127)], "N2 = 257: three output chunks, the last one column wide; K2 = 127"),
    _pairk1(1), _pairk1(31), _pairk1(32), _pairk1(33), _pairk1(97), _pairk1(129),
    _c("pair<8,8>-K1=33", [(64, 2), (160, 33), (72, 80)], "NB1 = 8: D = 4 register sets, n1 = 2 < n1p = 4; M1 = 160: three strip groups, the last half empty"),
    _c("pair<8,8>-K1=129", [(64, 2), (160, 129), (72, 80)], "NB1 = 8: n1 = 5 < n1p = 8"),
    _c("pair<8,4,V>", [(128, 2), (56, 40), (64, 80)], "NB1 = 8, NB2 = 4, aligned (the only fp32 shape class of this arm: K2 > 64 >= N2)"),
    _c("pair-K2=48-N2=48", [(128, 2), (70, 40), (48, 48)], "K2 = 48, N2 = 48"),
    _c("pair-K2=64-N2=65", [(128, 2), (70, 40), (65, 64)], "K2 = 64, N2 = 65: NB2 = 8 with one column past 64"),
    _c("pair-K2=65-N2=64", [(128, 2), (70, 40), (64, 65)], "K2 = 65: NB1 = 8 with one row in the fifth block; N2 = 64"),
    _c("pair-K2=128-N2=128", [(128, 2), (70, 40), (128, 128)], "K2 = N2 = 128: exactly one full chunk of each"),
    _c("pair-N2=129", [(128, 2), (70, 40), (129, 128)], "N2 = 129: a second output chunk of one column"),
    _c("pair-slabs129-f64", [(48, 8), (48, 50)], "129 slabs: the last group of 8 workgroups has one (slab >= pre exit)", nrhs=129, dts=(F64,)),
    _c("pair-slabs129-f32", [(48, 8), (48, 70)], "the same in fp32 (a side above 64)", nrhs=129, dts=(F32,)),
    _c("pair-only", [(96, 96), (96, 96)], "q = 2, 160 slabs: the pair is the only pass and applies alpha / beta", nrhs=160),
    _c("pair-first-f64", [(2, 130), (50, 60), (50, 60)], "the pair first (it shrinks the tensor), then a mode pass", dts=(F64,)),
    _c("pair-first-f32", [(2, 130), (50, 70), (50, 70)], "the pair first, fp32 (a side above 64)", dts=(F32,)),
    _c("pair-first-aligned", [(2, 130), (50, 72), (52, 72)], "the pair first with K2, N2 and ld3 multiples of four: VEC unless the input itself is misaligned"),
    # ---- the single-mode kernels, arm by arm
    _c("mode-NBP8", [(256, 2), (20, 24), (80, 70)], "k = 1: pre = 256, post = 70 — NBP = 8"),
    _c("mode-NBP4", [(256, 2), (20, 24), (40, 40)], "k = 1: pre = 256, post = 40 — NBP = 4"),
    _c("mode-NW8", [(64, 2), (130, 24), (40, 40)], "k = 1: M = 130 (9 strips), 64 x 2 tiles of 32 columns: NBP = 2, NW = 8"),
    _c("mode<8,8>", [(130, 24), (8, 256), (8, 128)], "k = 0: post = 32768 (256 tiles of 128 columns), M = 130: NBP = 8, NW = 8; K = 256 in mode 1"),
    _c("mode<8,8,s>", [(130, 24), (9, 255), (8, 129)], "the same with post = 32895: unaligned; K2 = 129 > 128 keeps the last two modes apart"),
    _c("mode<8,4,s>", [(256, 2), (20, 24), (80, 71)], "mode-NBP8 with post = 71: unaligned in both dtypes"),
    _c("mode<4,4,s>", [(256, 2), (20, 24), (41, 41)], "mode-NBP4 with post = 41: unaligned"),
    _c("mode<4,8,s>", [(256, 2), (130, 24), (41, 41)], "the same with M = 130: NW = 8"),
    _c("mode-post2",[(30, 4), (130, 129), (2, 2)], "post = 2 (r_1 r_2 > 256: not multiplied out)"),
    _c("mode-post3", [(30, 4), (130, 129), (3, 3)], "post = 3: VEC false in both dtypes"),
    _c("mode-post17", [(300, 4), (33, 20), (17, 17)], "post = 17"),
    _c("modet-NBB8", [(33000, 3), (3, 2)], "pre = 33000 >= 32641: NBB = 8; mode 0 has a side >= 1024: rocBLAS with post = 2"),
    _c("modet<8,4,s>", [(200, 2), (170, 2), (3, 3)], "pre = 34000, K = 3: NBB = 8 unaligned, no library GEMM in front"),
    _c("modet<8,8,V>", [(200, 2), (170, 2), (70, 2)], "pre = 34000, M = 70 (5 strips): NBB = 8, NW = 8"),
    _c("modet<8,8,s>", [(200, 2), (170, 2), (70, 3)], "the same with K = 3: unaligned"),
    _c("modet<2,8,s>", [(130, 33)], "q = 1 with 4096 right-hand sides: 128 row tiles x 2 strip groups — NBB = 2, NW = 8, K = 33", nrhs=4096),
    _c("blas-mid", [(256, 256), (16, 16)], "2.1e9 flops in mode 0: rocBLAS by the mid rule; then modet with pre = 262144", nrhs=1024),
    _c("separable", [(200, 200), (3, 2)], "SeparableGramian-shaped: a Gramian (x) a small B"),
]
BY_TAG = {c.tag: c for c in CASES}
assert len(BY_TAG) == len(CASES)


def inputs(case, dt):
    """(Fs, a, y0) of a case, rounded to dt; the stream depends on the case's tag only."""
    rng = np.random.default_rng(zlib.crc32(case.tag.encode()))
    Fs = [rng.standard_normal(s).astype(dt) for s in case.shapes]
    nin = math.prod(s[1] for s in case.shapes)
    nout = math.prod(s[0] for s in case.shapes)
    a = rng.standard_normal((nin,) if case.nrhs == 0 else (nin, case.nrhs)).astype(dt)
    y0 = rng.standard_normal((nout,) if case.nrhs == 0 else (nout, case.nrhs)).astype(dt)
    return Fs, a, y0


# Template arms that NO shape selects on 256 CUs, {(kernel, arm): the inequality of the planner that rules it out}
# (tests/test_kron_ref_host.py asserts that CASES covers every other arm in both dtypes, and that none of these is covered).
# Empty: all 28 instantiated arms are reachable on 256 CUs, and CASES reaches each of them in fp64 and in fp32.
EXEMPT = {}
