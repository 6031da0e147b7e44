"""Shared by tests/test_sparse_host.py (no GPU) and tests/test_gpu_sparse.py: the decay radii in closed form, the seeded clouds, the
lengthscale that puts the decay radius into the widest gap of the cloud's pair distances, and the fp64 reference of sparse(G, delta).

Reference pattern: s_ij <= R^2 with s_ij = sum_l (x_il - y_jl)^2 in fp64 ON THE DATA AS ROUNDED TO THE DTYPE, R = l r0(delta / |c|).  The
device forms s in the points' own precision with one fused multiply-add per dimension: d + 1 roundings of the differences and the
sums, each <= eps_T / 2 relative to a partial sum <= s, so |s_dev / s - 1| <= (d + 1) eps_T to first order, and R^2 is rounded once
more.  A pair whose |s / R^2 - 1| exceeds BAND = 8 (d + 2) eps_T is therefore on the same side of the threshold in both arithmetics:
the pattern must then agree EXACTLY.  The clouds are built so that no pair lies inside that band (asserted on the CPU before the device
is touched): the lengthscale is chosen from the data, in the middle of the widest relative gap between consecutive pair distances whose
kept share lies in a window inside (1 %, 60 %): [2 %, 50 %] unless a case names its own, to steer nnz / n or, where the distances are
dense against the band (fp32 at d = 70 with 385 500 pairs), to reach the sparser tail of the distances.

Values: covgram_oracle.matrix with the entrywise bound of tests/matrix_cases.reference_and_bound (imported, not copied)."""
import math

import numpy as np

import covgram_oracle as o
import matrix_cases as mc

F32, F64 = np.float32, np.float64
DELTA = 1e-6


def base_radius(family, param, delta):
    """r0(delta) of src/sparse.jl:25-35."""
    if family == o.EQ:
        return math.sqrt(-2.0 * math.log(delta))
    if family == o.GAMMAEXP:
        return (-2.0 * math.log(delta)) ** (1.0 / param)
    assert family in (o.EXP, o.MATERNP, o.MATERN), family
    return -math.log(delta)


def radius(ko, delta):
    """l r0(delta / |c|) of an oracle kernel: the two corrections of the reference that include/covgram.h states."""
    return ko.lengthscale * base_radius(ko.family, ko.param, delta / abs(ko.scale))


def band(d, dt):
    return 8.0 * (d + 2) * float(np.finfo(dt).eps)


def pair_s(X, Y):
    """s_ij in fp64 by direct differences on the rounded data."""
    Xd, Yd = X.astype(F64), Y.astype(F64)
    s = np.zeros((X.shape[0], Y.shape[0]))
    for l in range(X.shape[1]):
        q = Xd[:, l][:, None] - Yd[:, l][None, :]
        s += q * q
    return s


def cloud(rng, n, m, d, dt, same):
    """Seeded Gaussian clouds, spread 0.8 (0.8 sqrt(8 / d) for d > 8, as matrix_cases.wide_cloud); X is Y itself for `same` (n == m),
    otherwise: one row of X moved far outside (it keeps nothing; n >= 2 only — the single row of n = 1 has to keep something) and up to
    three rows of X copied from Y (s = 0 exactly).  Returns X, Y, far row or None, copied rows."""
    spread = 0.8 * (math.sqrt(8.0 / d) if d > 8 else 1.0)
    Y = (spread * rng.standard_normal((m, d))).astype(dt)
    if same:
        assert n == m
        return Y, Y, None, []
    X = spread * rng.standard_normal((n, d)) + 0.25 * spread
    far = None
    if n >= 2:
        far = int(rng.integers(n))
        v = rng.standard_normal(d); v /= np.linalg.norm(v)
        X[far] = 1.0e3 * spread * math.sqrt(d) * v
    X = X.astype(dt)
    rows = [i for i in range(n) if i != far]
    copies = [int(i) for i in rng.choice(rows, size=min(3, max(0, len(rows) - 1), m), replace=False)] if len(rows) > 1 else []
    for t, i in enumerate(copies):
        X[i] = Y[(7 * t + 1) % m]
    return X, Y, far, copies


WINDOW = (0.02, 0.50)


def gap_radius2(s, d, dt, window=WINDOW):
    """(R^2, relative half-width of its gap): the geometric middle of the widest relative gap between consecutive distinct pair
    distances at which the kept share lies in `window`."""
    v = np.unique(s[np.isfinite(s)].ravel())
    v = v[v > 0]
    cnt = np.searchsorted(np.sort(s.ravel()), v, side="right")          # pairs kept when R^2 is just above v[i]
    share = cnt / s.size
    ok = np.nonzero((share[:-1] >= window[0]) & (share[:-1] <= window[1]))[0]
    assert len(ok), "no candidate gap"
    rel = v[ok + 1] / v[ok]
    b = ok[int(np.argmax(rel))]
    return math.sqrt(v[b] * v[b + 1]), math.sqrt(v[b + 1] / v[b]) - 1.0


def fit_kernel(make, X, Y, d, dt, delta=DELTA, window=WINDOW):
    """make(l) -> oracle kernel.  The lengthscale (rounded to 12 digits, so that the device library sees the same double) that puts R^2
    into the widest gap; asserts the conditions of the module docstring and returns (ko, s, keep mask, R)."""
    s = pair_s(X, Y)
    R2, half = gap_radius2(s, d, dt, window)
    k1 = make(1.0)
    l = float(f"{math.sqrt(R2) / radius(k1, delta):.12e}")
    ko = make(l)
    R = radius(ko, delta)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(s / (R * R) - 1.0)
    inband = int((rel <= band(d, dt)).sum())
    assert inband == 0, f"{inband} pairs inside the band {band(d, dt):.2e} (gap half-width {half:.2e})"
    keep = s <= R * R
    share = keep.mean()
    assert 0.01 < share < 0.6, share
    return ko, s, keep, R


def group_width(nnz, n):
    """Lanes per row of the product kernel, from nnz / n (covgram_sparse_create in csrc/sparse.hip): 1 below 4 entries per row, 4 below 32,
    16 below 256, 64 from there."""
    avg = nnz / n
    return 1 if avg < 4 else 4 if avg < 32 else 16 if avg < 256 else 64


def csr_of(keep):
    rowptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    colind = np.nonzero(keep)[1].astype(np.int32)            # row-major order: ascending within every row
    return rowptr, colind


def reference_and_bound(ko, X, Y, dt):
    return mc.reference_and_bound(o, ko, X, Y, dt)
