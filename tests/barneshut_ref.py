"""Reference restatement of src/barneshut.jl:76-190 in numpy / fp64, shared by tests/test_barneshut_host.py (no GPU) and
tests/test_gpu_barneshut.py (device).

A tree is a dict of arrays: indices (a permutation of 0 .. m-1), and per node lo, hi, left, right (-1 at a leaf; root = node 0),
centers (nnodes x d), radii.  build_tree makes one of its own (median split by position along the widest dimension, stable); the
device tests pass the tree the library exported instead.  `recursion` is bh_recursion (:123-143) for all targets at once: the rows
that reach a node are carried as an index set, so every row receives exactly the terms of its own recursion."""
import numpy as np

F64 = np.float64


def build_tree(Y, leafsize):
    Y = np.asarray(Y, dtype=F64)
    m, d = Y.shape
    perm = np.arange(m)
    lo_, hi_, left, right = [], [], [], []

    def rec(lo, hi):
        v = len(lo_)
        lo_.append(lo); hi_.append(hi); left.append(-1); right.append(-1)
        if hi - lo > leafsize:
            P = Y[perm[lo:hi]]
            dim = int(np.argmax(P.max(0) - P.min(0)))
            perm[lo:hi] = perm[lo:hi][np.argsort(P[:, dim], kind="stable")]
            mid = lo + (hi - lo + 1) // 2
            left[v] = rec(lo, mid); right[v] = rec(mid, hi)
        return v

    if m:
        rec(0, m)
    nn = len(lo_)
    cen = np.zeros((nn, d)); rad = np.zeros(nn)
    for v in range(nn):
        P = Y[perm[lo_[v]:hi_[v]]]
        cen[v] = 0.5 * (P.max(0) + P.min(0))
        rad[v] = np.sqrt(((P - cen[v]) ** 2).sum(1).max())
    return {"indices": perm.astype(np.int32), "lo": np.array(lo_, np.int32), "hi": np.array(hi_, np.int32), "left": np.array(left, np.int32),
            "right": np.array(right, np.int32), "centers": cen, "radii": rad}


def depth_of(tree):
    """depth of every node (root 0)"""
    nn = len(tree["lo"])
    dep = np.zeros(nn, dtype=np.int64)
    stack = [(0, 0)] if nn else []
    while stack:
        v, k = stack.pop()
        dep[v] = k
        if tree["left"][v] >= 0:
            stack.append((int(tree["left"][v]), k + 1)); stack.append((int(tree["right"][v]), k + 1))
    return dep


def moments(tree, Y, w, eps):
    """(sums, com, sum |w|, sum |w| |y|) per node over the tree's ranges; com = sum |w| y / (sum |w| + eps) (:157-163).  Accumulated in
    extended precision (np.longdouble) and rounded to fp64 at the end: the device accumulates in fp64, so an fp64 sum here would carry an
    error of the size the fp64 comparison allows."""
    LD = np.longdouble
    Yl = np.asarray(Y, dtype=F64).astype(LD); wl = np.asarray(w, dtype=F64).astype(LD)
    idx = tree["indices"].astype(np.int64)
    nn = len(tree["lo"])
    sums = np.zeros(nn); sabs = np.zeros(nn); com = np.zeros((nn, Yl.shape[1])); mabs = np.zeros((nn, Yl.shape[1]))
    for v in range(nn):
        j = idx[tree["lo"][v]:tree["hi"][v]]
        aw = np.abs(wl[j])
        sa = aw.sum()
        sums[v] = F64(wl[j].sum()); sabs[v] = F64(sa)
        com[v] = ((aw[:, None] * Yl[j]).sum(0) / (sa + LD(eps))).astype(F64)
        mabs[v] = (aw[:, None] * np.abs(Yl[j])).sum(0).astype(F64)
    return sums, com, sabs, mabs


def recursion(tree, X, Y, w, com, sums, theta, entries, band_eps=None):
    """bh_recursion for every row of X.  entries(rows, P) -> (ref, bound): the fp64 Gramian entries k(X[rows], P) and their entrywise
    error bound.  com, sums: the far-field points and weights per node.  Returns a dict:
      want      sum of the recursion's terms                    babs   sum bound |weight|        eabs   sum |entry| |weight|
      ambiguous rows that visit a node with |h.r - theta |x - c|| <= 64 band_eps (h.r + theta (|x| + |c|))   (band_eps given)
      compressed number of nodes each row compressed            visits number of (row, node) visits."""
    X = np.asarray(X); Y = np.asarray(Y)
    X64 = X.astype(F64)
    n = X.shape[0]
    idx = tree["indices"].astype(np.int64)
    w64 = np.asarray(w, dtype=F64)
    com = np.asarray(com); sums64 = np.asarray(sums, dtype=F64)
    out = {"want": np.zeros(n), "babs": np.zeros(n), "eabs": np.zeros(n), "ambiguous": np.zeros(n, dtype=bool),
           "compressed": np.zeros(n, dtype=np.int64), "visits": 0}
    if len(tree["lo"]) == 0 or n == 0:
        return out
    stack = [(0, np.arange(n))]
    while stack:
        v, act = stack.pop()
        if act.size == 0:
            continue
        out["visits"] += act.size
        lo, hi, l, r = int(tree["lo"][v]), int(tree["hi"][v]), int(tree["left"][v]), int(tree["right"][v])
        if l < 0:
            j = idx[lo:hi]
            ref, bnd = entries(act, Y[j])
            out["want"][act] += ref @ w64[j]; out["babs"][act] += bnd @ np.abs(w64[j]); out["eabs"][act] += np.abs(ref) @ np.abs(w64[j])
            continue
        c = com[v].astype(F64)
        dist = np.sqrt(((X64[act] - c) ** 2).sum(1))
        hr = float(tree["radii"][v])
        if band_eps is not None:
            band = 64 * band_eps * (hr + theta * (np.linalg.norm(X64[act], axis=1) + np.linalg.norm(c)))
            out["ambiguous"][act] |= np.abs(hr - theta * dist) <= band
        far = hr < theta * dist
        if far.any():
            rows = act[far]
            ref, bnd = entries(rows, com[v][None, :])
            out["want"][rows] += ref[:, 0] * sums64[v]; out["babs"][rows] += bnd[:, 0] * abs(sums64[v]); out["eabs"][rows] += np.abs(ref[:, 0]) * abs(sums64[v])
            out["compressed"][rows] += 1
        stack.append((r, act[~far])); stack.append((l, act[~far]))
    return out


def barneshut(tree, X, Y, w, theta, entries, eps, split=True):
    """barneshut!(b, F, w, 1, 0, theta; split) of :76-112 in fp64 with fp64 moments: the product alone (no alpha, beta, D)."""
    w = np.asarray(w, dtype=F64)

    def one(wc):
        s, c, _, _ = moments(tree, Y, wc, eps)
        return recursion(tree, X, Y, wc, c, s, theta, entries)["want"]

    if split and (w < 0).any():
        return one(np.where(w > 0, w, 0.0)) - one(np.where(w < 0, -w, 0.0))
    return one(w)
