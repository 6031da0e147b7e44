// barneshut.hip — BarnesHutFactorization: a ball tree over the column points and the tree-based approximate product of a scalar isotropic
// Gramian (include/covgram.h: covgram_bh_*).  Replaces BarnesHutFactorization / barneshut! of src/barneshut.jl:25-190.
//
// TREE.  A binary tree over a permutation `indices` of the columns; a node owns the contiguous range [lo, hi) and splits it BY POSITION
// at lo + ceil((hi - lo) / 2) after a stable sort of the range along its dimension of widest extent, until a range holds at most
// `leafsize` points.  Duplicated points therefore split like any others, and the SHAPE of the tree (ranges, children, numbering) is a
// function of (m, leafsize) alone: the host lays it out, in pre-order, so that the left child of v is v + 1 and skip[v] is the first node
// behind v's subtree.  Everything that depends on the data runs on the device, level by level: the extents and sort keys of a level's
// nodes (bh_keys_kernel), rocPRIM's stable radix sort of the level's ranges, then per node the bounding-box centre and the radius
// (fp64 distances, rounded UP to the points' precision, so that containment holds without slack).  Minima, maxima and a stable sort
// do not depend on the order in which workgroups run: the tree is bit-identical from run to run.
//
// PRODUCT (src/barneshut.jl:76-143).  Per product the node moments sum w_j and sum |w_j| y_j / (sum |w_j| + eps(T)) are accumulated in
// fp64, leaves first, then parents from children level by level (no floating-point atomics), and rounded to T once.  The walk gives one
// lane one target and one wave 64 targets that are neighbours along a tree ordering of the targets; the wave walks the union of its
// lanes' paths in pre-order (v + 1 descends, skip[v] passes over a subtree), and a lane that has compressed a subtree sits out until the
// wave reaches that subtree's skip link.  The node under the wave is wave-uniform, so its record, a leaf's points and their weights are
// the same addresses in all 64 lanes.  The criterion h.r < theta |x_i - com[v]| is per lane: the terms a
// target receives are exactly those of the reference's recursion, in pre-order.  With split on, the positive and the negative part of
// w carry their own moments and their own masks and share one walk (a leaf's pair is evaluated once for both).
//
// TAYLOR PRODUCT (src/taylor.jl:7-57; covgram_bh_taylor_*).  One pass for weights of any sign: a compressed node adds the first-order
// expansion f0(s) sum w_j - 2 f1(s) (x_i - c) . m1 about a centre c, s = |x_i - c|^2, with m1 = sum w_j (y_j - c) the centred signed first
// moment.  c is the |w|-weighted centre of mass (use_com) or the ball centre, which does not depend on w: the product is then an exactly
// linear map of w.  The moments ride in ONE channel of 2 + 2 DM doubles per node, { sum w, sum |w|, sum |w| y, sum w y }, through the same
// leaf-then-parents schedule; the walk is the single-channel walk with the jet (f0, f1) in place of the value at internal nodes.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "driver.hpp"
#include "profiles.hpp"

namespace covgram {

constexpr int BH_MAX_D = 8;          // points in registers; beyond, a ball tree compresses nothing ("Barnes-Hut")
constexpr int BH_XLEAF = 64;         // the targets are ordered along a tree with leaves of one wave
constexpr int BH_TOP_DEPTH = 12;     // the moments of the levels 0 .. 12 (at most 4096 nodes each) are summed by ONE workgroup
constexpr int64_t BH_BIG_SEGMENT = 32768;   // ranges from this size on are sorted by the device-wide radix sort, one call each

static const char* bh_family_name(int family) {
    switch (family) {
        case COVGRAM_DOT: return "Dot";
        case COVGRAM_EXPDOT: return "ExponentialDot";
        case COVGRAM_ASINDOT: return "AsinDot (NeuralNetwork)";
        default: return "unknown";
    }
}

// ------------------------------------------------------------------------------------------------
// shape (host): pre-order numbering
// ------------------------------------------------------------------------------------------------
struct BhShape {
    std::vector<int32_t> lo, hi, left, right, skip, depth;
    int maxdepth = 0;
    int64_t size() const { return (int64_t)lo.size(); }
};

static int32_t bh_shape_node(BhShape& s, int64_t lo, int64_t hi, int depth, int64_t leafsize) {
    const int32_t v = (int32_t)s.lo.size();
    s.lo.push_back((int32_t)lo); s.hi.push_back((int32_t)hi); s.left.push_back(-1); s.right.push_back(-1); s.skip.push_back(0);
    s.depth.push_back(depth);
    s.maxdepth = std::max(s.maxdepth, depth);
    if (hi - lo > leafsize) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        const int32_t l = bh_shape_node(s, lo, mid, depth + 1, leafsize);
        const int32_t r = bh_shape_node(s, mid, hi, depth + 1, leafsize);
        s.left[v] = l; s.right[v] = r;
    }
    s.skip[v] = (int32_t)s.lo.size();
    return v;
}

// ------------------------------------------------------------------------------------------------
// build kernels
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bh_iota_kernel(int32_t* __restrict__ idx, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) idx[i] = (int32_t)i;
}

// One workgroup per range [begin[b], end[b]): the dimension of widest extent (the lowest one among equals), then keys[i] = that
// coordinate of point idx[i].  Minima and maxima are exact, so the choice does not depend on the order of the reduction.
template <typename T>
__global__ __launch_bounds__(256) void bh_keys_kernel(const T* __restrict__ P, int d, const int32_t* __restrict__ idx, const int32_t* __restrict__ begin,
                                                      const int32_t* __restrict__ end, T* __restrict__ keys) {
    __shared__ T smin[BH_MAX_D][256];
    __shared__ T smax[BH_MAX_D][256];
    __shared__ int sdim;
    const int lo = begin[blockIdx.x], hi = end[blockIdx.x];
    const int t = threadIdx.x;
    T mn[BH_MAX_D], mx[BH_MAX_D];
#pragma unroll
    for (int l = 0; l < BH_MAX_D; ++l) { mn[l] = (T)INFINITY; mx[l] = -(T)INFINITY; }
    for (int i = lo + t; i < hi; i += 256) {
        const T* p = P + (int64_t)idx[i] * d;
#pragma unroll
        for (int l = 0; l < BH_MAX_D; ++l)
            if (l < d) { const T c = p[l]; mn[l] = c < mn[l] ? c : mn[l]; mx[l] = c > mx[l] ? c : mx[l]; }
    }
#pragma unroll
    for (int l = 0; l < BH_MAX_D; ++l) { smin[l][t] = mn[l]; smax[l][t] = mx[l]; }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int l = 0; l < BH_MAX_D; ++l) {
                const T a = smin[l][t + o], b = smax[l][t + o];
                if (a < smin[l][t]) smin[l][t] = a;
                if (b > smax[l][t]) smax[l][t] = b;
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        int best = 0;
        T ext = smax[0][0] - smin[0][0];
        for (int l = 1; l < d; ++l) {
            const T e = smax[l][0] - smin[l][0];
            if (e > ext) { ext = e; best = l; }
        }
        sdim = best;
    }
    __syncthreads();
    const int dim = sdim;
    for (int i = lo + t; i < hi; i += 256) keys[i] = P[(int64_t)idx[i] * d + dim];
}

__device__ __forceinline__ float bh_round_up(double v, float) {
    float r = (float)v;
    if ((double)r < v) r = nextafterf(r, INFINITY);
    return r;
}
__device__ __forceinline__ double bh_round_up(double v, double) { return v; }

// One wave per node: centre = midpoint of the bounding box (in T), radius = max |y - centre| over the node's points, distances in fp64
// and rounded up to T: every point of the node lies within the radius of the centre.
template <typename T>
__global__ __launch_bounds__(64) void bh_balls_kernel(const T* __restrict__ P, int d, const int32_t* __restrict__ idx, const int32_t* __restrict__ nlo,
                                                      const int32_t* __restrict__ nhi, T* __restrict__ centers, T* __restrict__ rad) {
    const int v = blockIdx.x;
    const int lo = nlo[v], hi = nhi[v];
    const int t = threadIdx.x;
    T mn[BH_MAX_D], mx[BH_MAX_D];
#pragma unroll
    for (int l = 0; l < BH_MAX_D; ++l) { mn[l] = (T)INFINITY; mx[l] = -(T)INFINITY; }
    for (int i = lo + t; i < hi; i += 64) {
        const T* p = P + (int64_t)idx[i] * d;
#pragma unroll
        for (int l = 0; l < BH_MAX_D; ++l)
            if (l < d) { const T c = p[l]; mn[l] = c < mn[l] ? c : mn[l]; mx[l] = c > mx[l] ? c : mx[l]; }
    }
    T c[BH_MAX_D];
#pragma unroll
    for (int l = 0; l < BH_MAX_D; ++l) {
        for (int o = 32; o > 0; o >>= 1) {
            const T a = __shfl_xor(mn[l], o, 64), b = __shfl_xor(mx[l], o, 64);
            mn[l] = a < mn[l] ? a : mn[l]; mx[l] = b > mx[l] ? b : mx[l];
        }
        c[l] = (T)0.5 * mn[l] + (T)0.5 * mx[l];
    }
    double r2 = 0;
    for (int i = lo + t; i < hi; i += 64) {
        const T* p = P + (int64_t)idx[i] * d;
        double s = 0;
#pragma unroll
        for (int l = 0; l < BH_MAX_D; ++l)
            if (l < d) { const double q = (double)p[l] - (double)c[l]; s = fma(q, q, s); }
        r2 = s > r2 ? s : r2;
    }
    for (int o = 32; o > 0; o >>= 1) { const double a = __shfl_xor(r2, o, 64); r2 = a > r2 ? a : r2; }
    if (t == 0) {
        for (int l = 0; l < d; ++l) centers[(int64_t)v * d + l] = c[l];
        // sqrt is correctly rounded: one more ulp covers it, the conversion to T rounds up
        rad[v] = bh_round_up(sqrt(r2) * (1.0 + 4.440892098500626e-16), (T)0);
    }
}

// out[j][0 .. DM) = P[idx[j]][0 .. d), padded with zeros (they add exact zeros to every squared distance)
template <typename T>
__global__ __launch_bounds__(256) void bh_gather_kernel(const T* __restrict__ P, int d, int DM, const int32_t* __restrict__ idx, int64_t count,
                                                        T* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count * DM) return;
    const int64_t j = e / DM;
    const int l = (int)(e - j * DM);
    out[e] = l < d ? P[(int64_t)idx[j] * d + l] : (T)0;
}

// ------------------------------------------------------------------------------------------------
// moments: mom[(c nnodes + v) (2 + DM)] = { sum w, sum |w|, sum |w| y_0 .. }, fp64; channel c of NS: NS == 1: w itself; NS == 2: the
// positive part (c = 0) and the negated negative part (c = 1) of w
// ------------------------------------------------------------------------------------------------
template <typename T, int NS>
__device__ __forceinline__ T bh_channel(T w, int c) {
    if constexpr (NS == 1) return w;
    else return c == 0 ? (w > (T)0 ? w : (T)0) : (w < (T)0 ? -w : (T)0);
}

// one thread per leaf, its points in tree order; also ws[j] = w[indices[j]], the weights in tree order for the walk
template <typename T, int DM, int NS>
__global__ __launch_bounds__(256) void bh_leaf_moments_kernel(const int32_t* __restrict__ leaves, int64_t nleaves, const int32_t* __restrict__ nlo,
                                                              const int32_t* __restrict__ nhi, const int32_t* __restrict__ idx, const T* __restrict__ Ys,
                                                              const T* __restrict__ w, T* __restrict__ ws, double* __restrict__ mom, int64_t nnodes) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nleaves) return;
    const int v = leaves[q];
    const int lo = nlo[v], hi = nhi[v];
    double S[NS], A[NS], M[NS][DM];
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        S[c] = 0; A[c] = 0;
#pragma unroll
        for (int l = 0; l < DM; ++l) M[c][l] = 0;
    }
    for (int j = lo; j < hi; ++j) {
        const T wj = w[idx[j]];
        ws[j] = wj;
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            const double wc = (double)bh_channel<T, NS>(wj, c);
            const double aw = fabs(wc);
            S[c] += wc; A[c] += aw;
#pragma unroll
            for (int l = 0; l < DM; ++l) M[c][l] = fma(aw, (double)Ys[(int64_t)j * DM + l], M[c][l]);
        }
    }
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        double* o = mom + ((int64_t)c * nnodes + v) * (2 + DM);
        o[0] = S[c]; o[1] = A[c];
#pragma unroll
        for (int l = 0; l < DM; ++l) o[2 + l] = M[c][l];
    }
}

template <int DM, int NS>
__device__ __forceinline__ void bh_add_children(double* __restrict__ mom, int64_t nnodes, int v, int r) {
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        double* o = mom + ((int64_t)c * nnodes + v) * (2 + DM);
        const double* a = mom + ((int64_t)c * nnodes + v + 1) * (2 + DM);      // the left child is v + 1
        const double* b = mom + ((int64_t)c * nnodes + r) * (2 + DM);
#pragma unroll
        for (int e = 0; e < 2 + DM; ++e) o[e] = a[e] + b[e];
    }
}

// the internal nodes order[first .. first + count) of ONE level: parent = left child + right child
template <int DM, int NS>
__global__ __launch_bounds__(256) void bh_up_level_kernel(const int32_t* __restrict__ order, int64_t first, int64_t count, const int32_t* __restrict__ right,
                                                          double* __restrict__ mom, int64_t nnodes) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= count) return;
    const int v = order[first + q];
    bh_add_children<DM, NS>(mom, nnodes, v, right[v]);
}

// the levels top, top - 1, ..., 0 in ONE workgroup (level L's internal nodes: order[off[L] .. off[L + 1]))
template <int DM, int NS>
__global__ __launch_bounds__(256) void bh_up_top_kernel(const int32_t* __restrict__ order, const int64_t* __restrict__ off, int top,
                                                        const int32_t* __restrict__ right, double* __restrict__ mom, int64_t nnodes) {
    for (int L = top; L >= 0; --L) {
        const int64_t q0 = off[L], q1 = off[L + 1];
        for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) {
            const int v = order[q];
            bh_add_children<DM, NS>(mom, nnodes, v, right[v]);
        }
        __threadfence();
        __syncthreads();
    }
}

// rounded to T once: sums[v NS + c], com[(v NS + c) DM + l] = M_l / (A + eps(T))   (src/barneshut.jl:157-163)
template <typename T, int DM, int NS>
__global__ __launch_bounds__(256) void bh_finalize_kernel(const double* __restrict__ mom, int64_t nnodes, T* __restrict__ sums, T* __restrict__ com) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nnodes) return;
    const double eps = sizeof(T) == 4 ? 1.1920928955078125e-07 : 2.220446049250313e-16;
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        const double* o = mom + ((int64_t)c * nnodes + v) * (2 + DM);
        sums[v * NS + c] = (T)o[0];
        const double den = o[1] + eps;
#pragma unroll
        for (int l = 0; l < DM; ++l) com[(v * NS + c) * DM + l] = (T)(o[2 + l] / den);
    }
}

// ------------------------------------------------------------------------------------------------
// the walk
// ------------------------------------------------------------------------------------------------
template <typename T>
struct BhWalk {
    const T* Xs;            // [n][DM] targets in their tree order
    const int32_t* xperm;   // target t is row xperm[t]
    int64_t n;
    const T* Ys;            // [m][DM] columns in tree order
    const T* ws;            // [m] weights in tree order
    const int32_t *lo, *hi, *skip;
    const T* rad;
    const T* sums;          // [nnodes][NS]
    const T* com;           // [nnodes][NS][DM]
    int32_t nnodes;
    int32_t family;
    T theta;
    T alpha_k;              // alpha times the kernel's Constant factor
    T alpha, beta;
    const T* w;             // the caller's weights (diagonal term only)
    const T* diag;          // nullptr, one value, or n values
    int64_t diag_len;
    T* b;
};

template <typename T, int DM, int NS>
__global__ __launch_bounds__(64) void bh_walk_kernel(const BhWalk<T> g, const KParams<T> kp) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = t < g.n;
    T x[DM];
    {
        const T* xp = g.Xs + (live ? t : 0) * DM;
#pragma unroll
        for (int l = 0; l < DM; ++l) x[l] = xp[l];
    }
    // a lane takes part in channel c at node v when v >= resume[c]; lanes beyond n never do
    int resume0 = live ? 0 : 0x7fffffff, resume1 = resume0;
    T acc = (T)0;
    int v = 0;
    while (v < g.nnodes) {
        v = __builtin_amdgcn_readfirstlane(v);
        const int lo = g.lo[v], hi = g.hi[v], skip = g.skip[v];
        const bool leaf = skip == v + 1;
        const bool act0 = v >= resume0, act1 = NS == 2 && v >= resume1;
        const int cnt = leaf ? hi - lo : NS;
        const T* src = leaf ? g.Ys + (int64_t)lo * DM : g.com + (int64_t)v * NS * DM;
        const T* wsrc = leaf ? g.ws + lo : g.sums + (int64_t)v * NS;
        const T r = g.rad[v];
        bool descend = false;
        for (int j = 0; j < cnt; ++j) {
            const T* y = src + j * DM;
            T s = (T)0;
#pragma unroll
            for (int l = 0; l < DM; ++l) { const T q = x[l] - y[l]; s = fma_t(q, q, s); }
            const T wj = wsrc[j];
            T wgt;
            bool take;
            if (leaf) {
                if constexpr (NS == 1) wgt = wj;
                else wgt = (act0 && wj > (T)0) || (act1 && wj < (T)0) ? wj : (T)0;
                take = NS == 1 ? act0 : (act0 || act1);
            } else {
                const bool act = j == 0 ? act0 : act1;
                const bool far = r < g.theta * cg_sqrt(s);                  // src/barneshut.jl:135, per target
                take = act && far;
                descend = descend || (act && !far);
                if (take) { if (j == 0) resume0 = skip; else resume1 = skip; }
                wgt = j == 0 ? wj : -wj;
            }
            if (__any(take)) {
                const T kv = phi_any<T>(g.family, s * kp.gamma2, kp);
                if (take) acc = fma_t(kv, wgt, acc);
            }
        }
        v = leaf ? v + 1 : (__any(descend) ? v + 1 : skip);
    }
    if (live) {
        const int64_t i = g.xperm[t];
        T res = g.alpha_k * acc;
        if (g.diag_len > 0) res = fma_t(g.alpha * g.diag[g.diag_len == 1 ? 0 : i], g.w[i], res);
        g.b[i] = (g.beta == (T)0) ? res : fma_t(g.beta, g.b[i], res);       // beta == 0: b is never read
    }
}

// ------------------------------------------------------------------------------------------------
// taylor! (src/taylor.jl:7-57): moments and walk
// ------------------------------------------------------------------------------------------------
// one thread per leaf: mom[v (2 + 2 DM)] = { sum w, sum |w|, sum |w| y_0 .., sum w y_0 .. }, fp64, and ws[j] = w[indices[j]].  The record
// is 2 + DM' doubles wide with DM' = 2 DM, so the parents are summed by bh_up_level_kernel<2 DM, 1> / bh_up_top_kernel<2 DM, 1> as they are.
template <typename T, int DM>
__global__ __launch_bounds__(256) void bh_taylor_leaf_moments_kernel(const int32_t* __restrict__ leaves, int64_t nleaves, const int32_t* __restrict__ nlo,
                                                                     const int32_t* __restrict__ nhi, const int32_t* __restrict__ idx,
                                                                     const T* __restrict__ Ys, const T* __restrict__ w, T* __restrict__ ws,
                                                                     double* __restrict__ mom) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nleaves) return;
    const int v = leaves[q];
    const int lo = nlo[v], hi = nhi[v];
    double S = 0, A = 0, M[DM], R[DM];
#pragma unroll
    for (int l = 0; l < DM; ++l) { M[l] = 0; R[l] = 0; }
    for (int j = lo; j < hi; ++j) {
        const T wj = w[idx[j]];
        ws[j] = wj;
        const double wc = (double)wj, aw = fabs(wc);
        S += wc; A += aw;
#pragma unroll
        for (int l = 0; l < DM; ++l) {
            const double y = (double)Ys[(int64_t)j * DM + l];
            M[l] = fma(aw, y, M[l]);
            R[l] = fma(wc, y, R[l]);
        }
    }
    double* o = mom + (int64_t)v * (2 + 2 * DM);
    o[0] = S; o[1] = A;
#pragma unroll
    for (int l = 0; l < DM; ++l) { o[2 + l] = M[l]; o[2 + DM + l] = R[l]; }
}

// rounded to T once: sums[v], cm[(2 v) DM + l] = the centre c (use_com: M_l / (A + eps(T)), src/barneshut.jl:157-163; otherwise the ball
// centre, padded with zeros) and cm[(2 v + 1) DM + l] = m1 = R_l - S c_l (src/taylor.jl:15-18), centred in fp64 about c AS ROUNDED TO T
template <typename T, int DM>
__global__ __launch_bounds__(256) void bh_taylor_finalize_kernel(const double* __restrict__ mom, int64_t nnodes, int use_com, const T* __restrict__ centers,
                                                                 int d, T* __restrict__ sums, T* __restrict__ cm) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nnodes) return;
    const double eps = sizeof(T) == 4 ? 1.1920928955078125e-07 : 2.220446049250313e-16;
    const double* o = mom + v * (2 + 2 * DM);
    sums[v] = (T)o[0];
    const double den = o[1] + eps;
#pragma unroll
    for (int l = 0; l < DM; ++l) {
        const T c = use_com ? (T)(o[2 + l] / den) : (l < d ? centers[v * d + l] : (T)0);
        cm[(2 * v) * DM + l] = c;
        cm[(2 * v + 1) * DM + l] = (T)fma(-o[0], (double)c, o[2 + DM + l]);
    }
}

// The walk of bh_walk_kernel<T, DM, 1> with g.com = cm above.  Leaves: the direct sums, through the same evaluation site.  An internal
// node that a lane compresses adds f0(s) sums[v] - 2 f1(s) (x - c) . m1 (src/taylor.jl:43-50), f0 = phi(s / l^2)^p and f1 = d f0 / d s
// (jet_any carries the Power chain rule; the Lengthscale's is the factor gamma2; the Constant is in alpha_k).  The criterion is strict
// and h.r >= 0, so a lane that takes the term has s > 0: the derivative of Exponential, GammaExponential and Matern(nu < 1), singular
// at s = 0, is never USED there (a lane that does not take the term may evaluate it at 0 and discards the result).
template <typename T, int DM>
__global__ __launch_bounds__(64) void bh_taylor_walk_kernel(const BhWalk<T> g, const KParams<T> kp) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = t < g.n;
    T x[DM];
    {
        const T* xp = g.Xs + (live ? t : 0) * DM;
#pragma unroll
        for (int l = 0; l < DM; ++l) x[l] = xp[l];
    }
    int resume = live ? 0 : 0x7fffffff;      // a lane takes part at node v when v >= resume; lanes beyond n never do
    T acc = (T)0;
    int v = 0;
    while (v < g.nnodes) {
        v = __builtin_amdgcn_readfirstlane(v);
        const int lo = g.lo[v], hi = g.hi[v], skip = g.skip[v];
        const bool act = v >= resume;
        if (skip == v + 1) {                 // a leaf
            if (__any(act)) {
                for (int j = lo; j < hi; ++j) {
                    const T* y = g.Ys + (int64_t)j * DM;
                    T s = (T)0;
#pragma unroll
                    for (int l = 0; l < DM; ++l) { const T q = x[l] - y[l]; s = fma_t(q, q, s); }
                    const T kv = phi_any<T>(g.family, s * kp.gamma2, kp);
                    if (act) acc = fma_t(kv, g.ws[j], acc);
                }
            }
            v = v + 1;
            continue;
        }
        const T* c = g.com + (int64_t)v * 2 * DM;
        const T* m1 = c + DM;
        T s = (T)0, dot = (T)0;
#pragma unroll
        for (int l = 0; l < DM; ++l) { const T q = x[l] - c[l]; s = fma_t(q, q, s); dot = fma_t(q, m1[l], dot); }
        const bool far = g.rad[v] < g.theta * cg_sqrt(s);                   // src/taylor.jl:43, per target
        const bool take = act && far;
        if (take) resume = skip;
        if (__any(take)) {                                                  // value and derivative once; skipped wave-wide otherwise
            T f0, f1, f2;
            jet_any<T>(g.family, s * kp.gamma2, kp, f0, f1, f2);
            if (take) {
                acc = fma_t(f0, g.sums[v], acc);
                acc = fma_t((T)-2 * (f1 * kp.gamma2), dot, acc);
            }
        }
        v = __any(act && !far) ? v + 1 : skip;
    }
    if (live) {
        const int64_t i = g.xperm[t];
        T res = g.alpha_k * acc;
        if (g.diag_len > 0) res = fma_t(g.alpha * g.diag[g.diag_len == 1 ? 0 : i], g.w[i], res);
        g.b[i] = (g.beta == (T)0) ? res : fma_t(g.beta, g.b[i], res);       // beta == 0: b is never read
    }
}

}  // namespace covgram

struct covgram_bh {
    covgram_ctx* ctx = nullptr;
    int64_t n = 0, m = 0, nnodes = 0, nleaves = 0;
    int32_t d = 0, DM = 0, dtype = 0, leafsize = 0, maxdepth = 0;
    double theta = 0;
    covgram::HostKernel hk;
    // tree
    int32_t* indices = nullptr;      // m
    int32_t* nodes = nullptr;        // lo, hi, left, right, skip: nnodes each
    void* centers = nullptr;         // nnodes d
    void* rad = nullptr;             // nnodes
    void* Ys = nullptr;              // m DM
    void* Xs = nullptr;              // n DM
    int32_t* xperm = nullptr;        // n
    // moments schedule
    int32_t* leaves = nullptr;       // nleaves
    int32_t* order = nullptr;        // internal nodes by level
    int64_t* off_dev = nullptr;      // maxdepth + 2 level offsets into order
    std::vector<int64_t> off;
    // per-product storage (allocated once: a product allocates nothing)
    void* ws = nullptr;              // m
    double* mom = nullptr;           // 2 nnodes (2 + DM); taylor: nnodes (2 + 2 DM)
    void* sums = nullptr;            // nnodes 2;          taylor: nnodes
    void* com = nullptr;             // nnodes 2 DM;       taylor: per node the centre and m1
    const int32_t* lo() const { return nodes; }
    const int32_t* hi() const { return nodes + nnodes; }
    const int32_t* left() const { return nodes + 2 * nnodes; }
    const int32_t* right() const { return nodes + 3 * nnodes; }
    const int32_t* skip() const { return nodes + 4 * nnodes; }
};

namespace covgram {

static void bh_free(covgram_bh* F) {
    void* p[] = {F->indices, F->nodes, F->centers, F->rad, F->Ys, F->Xs, F->xperm, F->leaves, F->order, F->off_dev, F->ws, F->mom, F->sums, F->com};
    for (void* q : p) if (q) (void)hipFree(q);
    F->indices = nullptr; F->nodes = nullptr; F->centers = nullptr; F->rad = nullptr; F->Ys = nullptr; F->Xs = nullptr; F->xperm = nullptr;
    F->leaves = nullptr; F->order = nullptr; F->off_dev = nullptr; F->ws = nullptr; F->mom = nullptr; F->sums = nullptr; F->com = nullptr;
}

// temporaries of one create call
struct BhTemp {
    std::vector<void*> p;
    ~BhTemp() { for (void* q : p) if (q) (void)hipFree(q); }
    int alloc(void** out, size_t bytes) {
        *out = nullptr;
        if (hipMalloc(out, std::max<size_t>(bytes, 16)) != hipSuccess) { (void)hipGetLastError(); return COVGRAM_ENOMEM; }
        p.push_back(*out);
        return COVGRAM_OK;
    }
};

#define CG_BH_MALLOC(ptr, bytes)                                                                                                   \
    do {                                                                                                                           \
        if (hipMalloc((void**)&(ptr), std::max<size_t>((size_t)(bytes), 16)) != hipSuccess) {                                      \
            (void)hipGetLastError();                                                                                               \
            set_error("barneshut: hipMalloc of %zu bytes failed (%s)", (size_t)(bytes), #ptr);                                     \
            return COVGRAM_ENOMEM;                                                                                                 \
        }                                                                                                                          \
    } while (0)

// idx <- the permutation of 0 .. count-1 that orders the points P along the tree of `shape`: level by level, the ranges of the level's
// internal nodes are sorted (stable) along their widest dimension.  The result is written to idx (device, count entries).
template <typename T>
static int bh_order_points(covgram_ctx* ctx, const T* P, int64_t count, int d, const BhShape& shape, int32_t* idx) {
    hipStream_t st = ctx->stream;
    BhTemp tmp;
    int32_t *idx_alt = nullptr, *seg = nullptr;
    T *keys = nullptr, *keys_alt = nullptr;
    void* sort_tmp = nullptr;
    size_t sort_cap = 0;
    int rc;
    if ((rc = tmp.alloc((void**)&idx_alt, (size_t)count * 4)) || (rc = tmp.alloc((void**)&keys, (size_t)count * sizeof(T))) ||
        (rc = tmp.alloc((void**)&keys_alt, (size_t)count * sizeof(T)))) {
        set_error("barneshut: hipMalloc of the sort buffers (%lld points) failed", (long long)count);
        return rc;
    }
    hipLaunchKernelGGL(bh_iota_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, idx, count);
    // the internal nodes by level, in pre-order (ascending ranges)
    std::vector<std::vector<int32_t>> beg(shape.maxdepth + 1), end(shape.maxdepth + 1);
    int64_t nint = 0;
    for (int64_t v = 0; v < shape.size(); ++v)
        if (shape.left[v] >= 0) { beg[shape.depth[v]].push_back(shape.lo[v]); end[shape.depth[v]].push_back(shape.hi[v]); ++nint; }
    if (nint == 0) { CG_CHECK_HIP(hipGetLastError()); return COVGRAM_OK; }
    std::vector<int32_t> flat;
    flat.reserve((size_t)(2 * nint));
    std::vector<int64_t> lvl(shape.maxdepth + 2, 0);
    for (int L = 0; L <= shape.maxdepth; ++L) {
        lvl[L] = (int64_t)flat.size();
        flat.insert(flat.end(), beg[L].begin(), beg[L].end());
        flat.insert(flat.end(), end[L].begin(), end[L].end());
    }
    if ((rc = tmp.alloc((void**)&seg, flat.size() * 4))) { set_error("barneshut: hipMalloc of the level ranges failed"); return rc; }
    CG_CHECK_HIP(hipMemcpyAsync(seg, flat.data(), flat.size() * 4, hipMemcpyHostToDevice, st));
    CG_CHECK_HIP(hipStreamSynchronize(st));        // `flat` is pageable host memory: the copy has read it when this returns
    int32_t *cur = idx, *alt = idx_alt;
    for (int L = 0; L <= shape.maxdepth; ++L) {
        const int64_t ns = (int64_t)beg[L].size();
        if (ns == 0) continue;
        const int32_t* sb = seg + lvl[L];
        const int32_t* se = sb + ns;
        hipLaunchKernelGGL((bh_keys_kernel<T>), dim3((unsigned)ns), dim3(256), 0, st, P, d, cur, sb, se, keys);
        CG_CHECK_HIP(hipMemcpyAsync(alt, cur, (size_t)count * 4, hipMemcpyDeviceToDevice, st));   // the ranges of this level's leaves stay as they are
        int64_t biggest = 0;
        for (int64_t q = 0; q < ns; ++q) biggest = std::max<int64_t>(biggest, end[L][q] - beg[L][q]);
        const bool big = biggest >= BH_BIG_SEGMENT;
        size_t need = 0;
        if (big) CG_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, need, keys, keys_alt, cur, alt, (unsigned)biggest, 0, 8 * sizeof(T), st));
        else CG_CHECK_HIP(rocprim::segmented_radix_sort_pairs(nullptr, need, keys, keys_alt, cur, alt, (unsigned)count, (unsigned)ns, sb, se, 0, 8 * sizeof(T), st));
        if (need > sort_cap) {
            CG_CHECK_HIP(hipStreamSynchronize(st));
            sort_cap = need + need / 4;
            if ((rc = tmp.alloc(&sort_tmp, sort_cap))) { set_error("barneshut: hipMalloc of %zu bytes of sort storage failed", sort_cap); return rc; }
        }
        if (big) {
            for (int64_t q = 0; q < ns; ++q) {
                const int64_t a = beg[L][q], sz = end[L][q] - a;
                size_t bytes = sort_cap;
                CG_CHECK_HIP(rocprim::radix_sort_pairs(sort_tmp, bytes, keys + a, keys_alt + a, cur + a, alt + a, (unsigned)sz, 0, 8 * sizeof(T), st));
            }
        } else {
            size_t bytes = sort_cap;
            CG_CHECK_HIP(rocprim::segmented_radix_sort_pairs(sort_tmp, bytes, keys, keys_alt, cur, alt, (unsigned)count, (unsigned)ns, sb, se, 0, 8 * sizeof(T), st));
        }
        std::swap(cur, alt);
    }
    if (cur != idx) CG_CHECK_HIP(hipMemcpyAsync(idx, cur, (size_t)count * 4, hipMemcpyDeviceToDevice, st));
    CG_CHECK_HIP(hipGetLastError());
    CG_CHECK_HIP(hipStreamSynchronize(st));        // the temporaries are freed when this returns
    return COVGRAM_OK;
}

template <typename T>
static int bh_build(covgram_bh* F, const covgram_points* X, const covgram_points* Y) {
    covgram_ctx* ctx = F->ctx;
    hipStream_t st = ctx->stream;
    const int64_t n = F->n, m = F->m;
    const int d = F->d, DM = F->DM;
    int rc;
    if (m > 0) {
        BhShape shape;
        bh_shape_node(shape, 0, m, 0, F->leafsize);
        const int64_t nn = shape.size();
        F->nnodes = nn; F->maxdepth = shape.maxdepth;
        CG_BH_MALLOC(F->indices, (size_t)m * 4);
        CG_BH_MALLOC(F->nodes, (size_t)nn * 5 * 4);
        CG_BH_MALLOC(F->centers, (size_t)nn * d * sizeof(T));
        CG_BH_MALLOC(F->rad, (size_t)nn * sizeof(T));
        CG_BH_MALLOC(F->Ys, (size_t)m * DM * sizeof(T));
        CG_BH_MALLOC(F->ws, (size_t)m * sizeof(T));
        CG_BH_MALLOC(F->mom, (size_t)nn * 2 * (2 + DM) * sizeof(double));
        CG_BH_MALLOC(F->sums, (size_t)nn * 2 * sizeof(T));
        CG_BH_MALLOC(F->com, (size_t)nn * 2 * DM * sizeof(T));
        // node arrays and the bottom-up schedule
        std::vector<int32_t> flat((size_t)nn * 5);
        for (int64_t v = 0; v < nn; ++v) {
            flat[v] = shape.lo[v]; flat[nn + v] = shape.hi[v]; flat[2 * nn + v] = shape.left[v]; flat[3 * nn + v] = shape.right[v];
            flat[4 * nn + v] = shape.skip[v];
        }
        std::vector<int32_t> leaves, order;
        std::vector<std::vector<int32_t>> by_level(shape.maxdepth + 1);
        for (int64_t v = 0; v < nn; ++v) {
            if (shape.left[v] < 0) leaves.push_back((int32_t)v);
            else by_level[shape.depth[v]].push_back((int32_t)v);
        }
        F->off.assign(shape.maxdepth + 2, 0);
        for (int L = 0; L <= shape.maxdepth; ++L) {
            F->off[L] = (int64_t)order.size();
            order.insert(order.end(), by_level[L].begin(), by_level[L].end());
        }
        F->off[shape.maxdepth + 1] = (int64_t)order.size();
        F->nleaves = (int64_t)leaves.size();
        CG_BH_MALLOC(F->leaves, leaves.size() * 4);
        CG_BH_MALLOC(F->order, order.size() * 4);
        CG_BH_MALLOC(F->off_dev, F->off.size() * 8);
        CG_CHECK_HIP(hipMemcpyAsync(F->nodes, flat.data(), flat.size() * 4, hipMemcpyHostToDevice, st));
        CG_CHECK_HIP(hipMemcpyAsync(F->leaves, leaves.data(), leaves.size() * 4, hipMemcpyHostToDevice, st));
        if (!order.empty()) CG_CHECK_HIP(hipMemcpyAsync(F->order, order.data(), order.size() * 4, hipMemcpyHostToDevice, st));
        CG_CHECK_HIP(hipMemcpyAsync(F->off_dev, F->off.data(), F->off.size() * 8, hipMemcpyHostToDevice, st));
        CG_CHECK_HIP(hipStreamSynchronize(st));    // the host vectors go out of scope below
        rc = bh_order_points<T>(ctx, (const T*)Y->dptr, m, d, shape, F->indices);
        if (rc) return rc;
        hipLaunchKernelGGL((bh_balls_kernel<T>), dim3((unsigned)nn), dim3(64), 0, st, (const T*)Y->dptr, d, F->indices, F->lo(), F->hi(), (T*)F->centers,
                           (T*)F->rad);
        hipLaunchKernelGGL((bh_gather_kernel<T>), dim3((unsigned)((m * DM + 255) / 256)), dim3(256), 0, st, (const T*)Y->dptr, d, DM, F->indices, m,
                           (T*)F->Ys);
    }
    if (n > 0) {
        CG_BH_MALLOC(F->Xs, (size_t)n * DM * sizeof(T));
        CG_BH_MALLOC(F->xperm, (size_t)n * 4);
        if (X->dptr == Y->dptr && n == m) {        // gramian(k, x): the targets follow the tree itself
            CG_CHECK_HIP(hipMemcpyAsync(F->xperm, F->indices, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
        } else {                                   // otherwise a tree of their own, with leaves of one wave; only its ordering is kept
            BhShape xs;
            bh_shape_node(xs, 0, n, 0, BH_XLEAF);
            rc = bh_order_points<T>(ctx, (const T*)X->dptr, n, d, xs, F->xperm);
            if (rc) return rc;
        }
        hipLaunchKernelGGL((bh_gather_kernel<T>), dim3((unsigned)((n * DM + 255) / 256)), dim3(256), 0, st, (const T*)X->dptr, d, DM, F->xperm, n,
                           (T*)F->Xs);
    }
    CG_CHECK_HIP(hipGetLastError());
    CG_CHECK_HIP(hipStreamSynchronize(st));        // the handle keeps no reference to X or Y
    return COVGRAM_OK;
}

// parents from children, level by level: the moments of a node are CH values per channel, NS channels
template <int CH, int NS>
static void bh_up_sweep(covgram_bh* F) {
    hipStream_t st = F->ctx->stream;
    const int64_t nn = F->nnodes;
    for (int L = F->maxdepth; L > BH_TOP_DEPTH; --L) {
        const int64_t cnt = F->off[L + 1] - F->off[L];
        if (cnt > 0)
            hipLaunchKernelGGL((bh_up_level_kernel<CH, NS>), dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, F->order, F->off[L], cnt, F->right(),
                               F->mom, nn);
    }
    const int top = std::min<int>(F->maxdepth, BH_TOP_DEPTH);
    if (F->off[top + 1] > 0)
        hipLaunchKernelGGL((bh_up_top_kernel<CH, NS>), dim3(1), dim3(256), 0, st, F->order, F->off_dev, top, F->right(), F->mom, nn);
}

// the first stage of a product on the ctx stream: ws, then sums and com of NS channels
template <typename T, int DM, int NS>
static void bh_launch_moments(covgram_bh* F, const T* w) {
    hipStream_t st = F->ctx->stream;
    const int64_t nn = F->nnodes;
    hipLaunchKernelGGL((bh_leaf_moments_kernel<T, DM, NS>), dim3((unsigned)((F->nleaves + 255) / 256)), dim3(256), 0, st, F->leaves, F->nleaves, F->lo(),
                       F->hi(), F->indices, (const T*)F->Ys, w, (T*)F->ws, F->mom, nn);
    bh_up_sweep<DM, NS>(F);
    hipLaunchKernelGGL((bh_finalize_kernel<T, DM, NS>), dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, F->mom, nn, (T*)F->sums, (T*)F->com);
}

// taylor!: ws, then sums, centres and centred first moments (one channel; the storage of the split product holds it: nnodes (2 + 2 DM)
// doubles <= 2 nnodes (2 + DM), and centre + m1 are the 2 DM values per node of com)
template <typename T, int DM>
static void bh_launch_taylor_moments(covgram_bh* F, const T* w, int use_com) {
    hipStream_t st = F->ctx->stream;
    const int64_t nn = F->nnodes;
    hipLaunchKernelGGL((bh_taylor_leaf_moments_kernel<T, DM>), dim3((unsigned)((F->nleaves + 255) / 256)), dim3(256), 0, st, F->leaves, F->nleaves,
                       F->lo(), F->hi(), F->indices, (const T*)F->Ys, w, (T*)F->ws, F->mom);
    bh_up_sweep<2 * DM, 1>(F);
    hipLaunchKernelGGL((bh_taylor_finalize_kernel<T, DM>), dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, F->mom, nn, use_com,
                       (const T*)F->centers, (int)F->d, (T*)F->sums, (T*)F->com);
}

// what either walk kernel reads: the handle's arrays and the arguments of this product
template <typename T>
static BhWalk<T> bh_walk_args(const covgram_bh* F, const T* w, T* b, double alpha, double beta, double theta, const T* diag, int64_t diag_len) {
    BhWalk<T> g;
    g.Xs = (const T*)F->Xs; g.xperm = F->xperm; g.n = F->n; g.Ys = (const T*)F->Ys; g.ws = (const T*)F->ws;
    g.lo = F->lo(); g.hi = F->hi(); g.skip = F->skip(); g.rad = (const T*)F->rad; g.sums = (const T*)F->sums; g.com = (const T*)F->com;
    g.nnodes = (int32_t)F->nnodes; g.family = F->hk.k.family; g.theta = (T)theta;
    g.alpha_k = (T)(alpha * F->hk.kp.scale); g.alpha = (T)alpha; g.beta = (T)beta;
    g.w = w; g.diag = diag; g.diag_len = diag_len; g.b = b;
    return g;
}

// the moments of g.w, then the walk (the timed kernel), one lane per target
template <typename T, int DM, int NS>
static void bh_launch_product(covgram_bh* F, const BhWalk<T>& g) {
    if (F->nnodes > 0) bh_launch_moments<T, DM, NS>(F, g.w);
    TimerScope timed(F->ctx);
    hipLaunchKernelGGL((bh_walk_kernel<T, DM, NS>), dim3((unsigned)((F->n + 63) / 64)), dim3(64), 0, F->ctx->stream, g, cast_params<T>(F->hk.kp));
}

template <typename T, int DM>
static void bh_launch_taylor(covgram_bh* F, const BhWalk<T>& g, int use_com) {
    if (F->nnodes > 0) bh_launch_taylor_moments<T, DM>(F, g.w, use_com);
    TimerScope timed(F->ctx);
    hipLaunchKernelGGL((bh_taylor_walk_kernel<T, DM>), dim3((unsigned)((F->n + 63) / 64)), dim3(64), 0, F->ctx->stream, g, cast_params<T>(F->hk.kp));
}

// f(T{}, integral_constant<int, DM>{}): the handle's element type and padded dimension (2, 4, 8) as compile-time values
template <typename Fn>
static void bh_dispatch(const covgram_bh* F, Fn&& f) {
    using std::integral_constant;
    by_dtype(F->dtype, [&](auto t0) {
        switch (F->DM) {
            case 2: f(t0, integral_constant<int, 2>{}); break;
            case 4: f(t0, integral_constant<int, 4>{}); break;
            default: f(t0, integral_constant<int, 8>{}); break;
        }
    });
}

}  // namespace covgram

using namespace covgram;

// What covgram_bh_mvm and covgram_bh_taylor_mvm share: the argument checks, theta < 0 = the handle's, the staging of host buffers and
// the copy back.  launch(a_dev, y_dev, theta, diag_dev, diag_len) enqueues the product itself.
template <typename Launch>
static int bh_product_call(covgram_bh* F, const void* a, void* y, double beta, double theta, const void* diag, int64_t diag_len, int32_t loc,
                           Launch launch) {
    CG_REQUIRE(F != nullptr, COVGRAM_EINVAL, "Barnes-Hut handle is NULL");
    CG_REQUIRE(loc == COVGRAM_HOST || loc == COVGRAM_DEVICE, COVGRAM_EINVAL, "unknown loc %d", loc);
    const int64_t n = F->n, m = F->m;
    CG_REQUIRE((a != nullptr || m == 0) && (y != nullptr || n == 0), COVGRAM_EINVAL, "a or y is NULL");
    CG_REQUIRE(!(theta != theta), COVGRAM_EINVAL, "BarnesHutFactorization: theta is NaN");
    if (theta < 0) theta = F->theta;
    if (diag == nullptr) diag_len = 0;
    CG_REQUIRE(diag_len == 0 || (n == m && (diag_len == 1 || diag_len == n)), COVGRAM_EINVAL,
               "DimensionMismatch: a diagonal of length %lld on a %lld x %lld factorization (square, one value or n values)", (long long)diag_len,
               (long long)n, (long long)m);
    if (n == 0) return COVGRAM_OK;
    covgram_ctx* ctx = F->ctx;
    const size_t ts = dtype_size(F->dtype);
    CG_DEVICE(ctx);
    // Staged serves HOST pointers only.  DEVICE pointers go through as they are, y may be a itself: the walk reads the weights from the
    // handle's tree-ordered copy, which the moments stage has completed before the walk starts, and a lane reads a[i] for the diagonal term
    // before it writes y[i] — Staged's private copy of an overlapping a would be a device-to-device copy that nothing needs
    Staged st;
    st.a = a; st.y = y;
    const void* d_dev = diag;
    if (loc == COVGRAM_HOST) {
        int rc = st.begin(ctx, loc, ts, a, m, m, y, n, n, 1, beta); if (rc) return rc;
        void* sd = nullptr; int64_t ld;
        if (diag_len > 0) { rc = ws_reserve(ctx, 4, staged_bytes(diag_len, 1, ts), &sd); if (rc) return rc; }
        char* cur = (char*)sd;
        rc = stage_operand(ctx, loc, ts, cur, diag, diag_len, diag_len, 1, &d_dev, &ld); if (rc) return rc;
    }
    launch(st.a, st.y, theta, d_dev, diag_len);
    CG_CHECK_HIP(hipGetLastError());
    return st.finish();
}

// What covgram_bh_moments and covgram_bh_taylor_moments share.  The weights as the moment kernels see them: HOST: a copy in workspace slot 2
static int bh_stage_w(covgram_bh* F, const void* w, int32_t loc, const void** w_dev) {
    const size_t ts = dtype_size(F->dtype);
    void* sw = nullptr;
    if (loc == COVGRAM_HOST) { int rc = ws_reserve(F->ctx, 2, staged_bytes(F->m, 1, ts), &sw); if (rc) return rc; }
    char* cur = (char*)sw;
    int64_t ld;
    return stage_operand(F->ctx, loc, ts, cur, w, F->m, F->m, 1, w_dev, &ld);
}
// `rows` rows of `row` bytes, `pitch` bytes apart in the handle, to the caller's packed array of loc (dst == NULL: not asked for)
static int bh_copy_rows(covgram_ctx* ctx, void* dst, const void* src, size_t row, size_t pitch, size_t rows, int32_t loc) {
    if (!dst) return COVGRAM_OK;
    const hipMemcpyKind kind = loc == COVGRAM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (pitch == row) CG_CHECK_HIP(hipMemcpyAsync(dst, src, row * rows, kind, ctx->stream));
    else CG_CHECK_HIP(hipMemcpy2DAsync(dst, row, src, pitch, row, rows, kind, ctx->stream));
    return COVGRAM_OK;
}

extern "C" {

int covgram_bh_create(covgram_ctx* ctx, covgram_bh** out, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, double theta,
                      int32_t leafsize) {
    CG_REQUIRE(ctx && out && k && X && Y, COVGRAM_EINVAL, "NULL argument");
    CG_REQUIRE(X->ctx == ctx && Y->ctx == ctx, COVGRAM_EINVAL, "points belong to a different ctx");
    CG_REQUIRE(X->dtype == Y->dtype, COVGRAM_EINVAL, "x and y have different dtypes");
    CG_REQUIRE(X->d == Y->d, COVGRAM_EINVAL, "DimensionMismatch: inputs have to have the same length: %d, %d", X->d, Y->d);
    CG_REQUIRE(theta >= 0, COVGRAM_EINVAL, "BarnesHutFactorization: theta = %g is negative (0 = the exact product)", theta);
    CG_REQUIRE(leafsize >= 1, COVGRAM_EINVAL, "BarnesHutFactorization: leafsize = %d is smaller than 1", leafsize);
    // refusals by name, before any launch
    if (k->family == COVGRAM_COMPOSITE) {
        const covgram_kernel_composite* c = (const covgram_kernel_composite*)k;
        set_error("BarnesHutFactorization: a %s of profiles is not supported (single isotropic profiles under Lengthscale, Constant and Power only)",
                  c->nterms > 1 ? "Sum" : "Product");
        return COVGRAM_EUNSUPPORTED;
    }
    CG_REQUIRE(k->family != COVGRAM_DOT && k->family != COVGRAM_EXPDOT && k->family != COVGRAM_ASINDOT && k->trait == COVGRAM_ISOTROPIC,
               COVGRAM_EUNSUPPORTED, "BarnesHutFactorization: %s is a dot-product kernel; the far field of a ball tree needs an isotropic profile",
               bh_family_name(k->family));
    CG_REQUIRE(X->d >= 1 && X->d <= BH_MAX_D, COVGRAM_EUNSUPPORTED,
               "BarnesHutFactorization: d = %d exceeds the limit of %d dimensions (a ball tree compresses nothing beyond)", X->d, BH_MAX_D);
    const int dtype = X->dtype;
    HostKernel hk;
    int rc = make_host_kernel(k, dtype, true, &hk);      // gamma = 1 / l, unfolded profiles: the evaluation of covgram_matrix
    if (rc) return rc;
    CG_REQUIRE(X->n < ((int64_t)1 << 31) && Y->n < ((int64_t)1 << 31), COVGRAM_EINVAL, "BarnesHutFactorization: more than 2^31 - 1 points");
    CG_DEVICE(ctx);
    covgram_bh* F = new covgram_bh();
    F->ctx = ctx; F->n = X->n; F->m = Y->n; F->d = X->d; F->dtype = dtype; F->leafsize = leafsize; F->theta = theta; F->hk = hk;
    F->DM = X->d <= 2 ? 2 : (X->d <= 4 ? 4 : 8);
    rc = by_dtype(dtype, [&](auto t0) { return bh_build<decltype(t0)>(F, X, Y); });
    if (rc) { bh_free(F); delete F; return rc; }
    ctx->live_handles++;
    *out = F;
    return COVGRAM_OK;
}

int covgram_bh_info(const covgram_bh* F, int64_t* n, int64_t* m, int32_t* d, int32_t* dtype, int64_t* nnodes, int32_t* leafsize, double* theta) {
    CG_REQUIRE(F != nullptr, COVGRAM_EINVAL, "Barnes-Hut handle is NULL");
    if (n) *n = F->n;
    if (m) *m = F->m;
    if (d) *d = F->d;
    if (dtype) *dtype = F->dtype;
    if (nnodes) *nnodes = F->nnodes;
    if (leafsize) *leafsize = F->leafsize;
    if (theta) *theta = F->theta;
    return COVGRAM_OK;
}

int covgram_bh_export(const covgram_bh* F, int32_t* indices, int32_t* lo, int32_t* hi, int32_t* left, int32_t* right, void* centers, void* radii,
                      int32_t loc) {
    CG_REQUIRE(F != nullptr, COVGRAM_EINVAL, "Barnes-Hut handle is NULL");
    CG_REQUIRE(loc == COVGRAM_HOST || loc == COVGRAM_DEVICE, COVGRAM_EINVAL, "unknown loc %d", loc);
    covgram_ctx* ctx = F->ctx;
    CG_DEVICE(ctx);
    const hipMemcpyKind kind = loc == COVGRAM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const size_t ts = dtype_size(F->dtype), nb = (size_t)F->nnodes * 4;
    if (F->nnodes > 0) {
        if (indices) CG_CHECK_HIP(hipMemcpyAsync(indices, F->indices, (size_t)F->m * 4, kind, ctx->stream));
        if (lo) CG_CHECK_HIP(hipMemcpyAsync(lo, F->lo(), nb, kind, ctx->stream));
        if (hi) CG_CHECK_HIP(hipMemcpyAsync(hi, F->hi(), nb, kind, ctx->stream));
        if (left) CG_CHECK_HIP(hipMemcpyAsync(left, F->left(), nb, kind, ctx->stream));
        if (right) CG_CHECK_HIP(hipMemcpyAsync(right, F->right(), nb, kind, ctx->stream));
        if (centers) CG_CHECK_HIP(hipMemcpyAsync(centers, F->centers, (size_t)F->nnodes * F->d * ts, kind, ctx->stream));
        if (radii) CG_CHECK_HIP(hipMemcpyAsync(radii, F->rad, (size_t)F->nnodes * ts, kind, ctx->stream));
    }
    if (loc == COVGRAM_HOST) CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return COVGRAM_OK;
}

int covgram_bh_moments(covgram_bh* F, const void* w, void* sums, void* com, int32_t loc) {
    CG_REQUIRE(F != nullptr, COVGRAM_EINVAL, "Barnes-Hut handle is NULL");
    CG_REQUIRE(loc == COVGRAM_HOST || loc == COVGRAM_DEVICE, COVGRAM_EINVAL, "unknown loc %d", loc);
    if (F->nnodes == 0) return COVGRAM_OK;
    CG_REQUIRE(w != nullptr, COVGRAM_EINVAL, "w is NULL");
    covgram_ctx* ctx = F->ctx;
    const size_t ts = dtype_size(F->dtype), nn = (size_t)F->nnodes;
    CG_DEVICE(ctx);
    const void* w_dev;
    int rc = bh_stage_w(F, w, loc, &w_dev); if (rc) return rc;
    bh_dispatch(F, [&](auto t0, auto dm) { bh_launch_moments<decltype(t0), decltype(dm)::value, 1>(F, (const decltype(t0)*)w_dev); });
    CG_CHECK_HIP(hipGetLastError());
    rc = bh_copy_rows(ctx, sums, F->sums, nn * ts, nn * ts, 1, loc); if (rc) return rc;             // one channel: [nnodes]
    rc = bh_copy_rows(ctx, com, F->com, (size_t)F->d * ts, (size_t)F->DM * ts, nn, loc); if (rc) return rc;
    if (loc == COVGRAM_HOST) CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return COVGRAM_OK;
}

int covgram_bh_mvm(covgram_bh* F, const void* a, void* y, double alpha, double beta, double theta, int32_t split, const void* diag, int64_t diag_len,
                   int32_t loc) {
    return bh_product_call(F, a, y, beta, theta, diag, diag_len, loc, [&](const void* a_dev, void* y_dev, double th, const void* d_dev, int64_t dl) {
        bh_dispatch(F, [&](auto t0, auto dm) {
            using T = decltype(t0);
            const BhWalk<T> g = bh_walk_args<T>(F, (const T*)a_dev, (T*)y_dev, alpha, beta, th, (const T*)d_dev, dl);
            if (split) bh_launch_product<T, decltype(dm)::value, 2>(F, g);
            else bh_launch_product<T, decltype(dm)::value, 1>(F, g);
        });
    });
}

int covgram_bh_taylor_moments(covgram_bh* F, const void* w, int32_t use_com, void* sums, void* centers, void* m1, int32_t loc) {
    CG_REQUIRE(F != nullptr, COVGRAM_EINVAL, "Barnes-Hut handle is NULL");
    CG_REQUIRE(loc == COVGRAM_HOST || loc == COVGRAM_DEVICE, COVGRAM_EINVAL, "unknown loc %d", loc);
    if (F->nnodes == 0) return COVGRAM_OK;
    CG_REQUIRE(w != nullptr, COVGRAM_EINVAL, "w is NULL");
    covgram_ctx* ctx = F->ctx;
    const size_t ts = dtype_size(F->dtype), nn = (size_t)F->nnodes;
    CG_DEVICE(ctx);
    const void* w_dev;
    int rc = bh_stage_w(F, w, loc, &w_dev); if (rc) return rc;
    bh_dispatch(F, [&](auto t0, auto dm) { bh_launch_taylor_moments<decltype(t0), decltype(dm)::value>(F, (const decltype(t0)*)w_dev, use_com != 0); });
    CG_CHECK_HIP(hipGetLastError());
    const size_t row = (size_t)F->d * ts, pitch = (size_t)2 * F->DM * ts;       // per node: the centre, then m1, DM values each
    rc = bh_copy_rows(ctx, sums, F->sums, nn * ts, nn * ts, 1, loc); if (rc) return rc;
    rc = bh_copy_rows(ctx, centers, F->com, row, pitch, nn, loc); if (rc) return rc;
    rc = bh_copy_rows(ctx, m1, (const char*)F->com + (size_t)F->DM * ts, row, pitch, nn, loc); if (rc) return rc;
    if (loc == COVGRAM_HOST) CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return COVGRAM_OK;
}

int covgram_bh_taylor_mvm(covgram_bh* F, const void* a, void* y, double alpha, double beta, double theta, int32_t use_com, const void* diag,
                          int64_t diag_len, int32_t loc) {
    return bh_product_call(F, a, y, beta, theta, diag, diag_len, loc, [&](const void* a_dev, void* y_dev, double th, const void* d_dev, int64_t dl) {
        bh_dispatch(F, [&](auto t0, auto dm) {
            using T = decltype(t0);
            bh_launch_taylor<T, decltype(dm)::value>(F, bh_walk_args<T>(F, (const T*)a_dev, (T*)y_dev, alpha, beta, th, (const T*)d_dev, dl), use_com != 0);
        });
    });
}

int covgram_bh_destroy(covgram_bh* F) {
    if (!F) return COVGRAM_OK;
    {
        ::covgram::DeviceGuard _cg_dev(F->ctx->device);           // (a finalizer may call this from any thread state)
        (void)hipStreamSynchronize(F->ctx->stream);               // products that still read the arrays
        bh_free(F);
    }
    F->ctx->live_handles--;
    delete F;
    return COVGRAM_OK;
}

}  // extern "C"
