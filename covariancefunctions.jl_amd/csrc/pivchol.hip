// pivchol.hip — covgram_pivoted_cholesky: the diagonally pivoted Cholesky factor P' G P ~= L L' of a symmetric Gramian G = k(X, X) of one
// isotropic profile, on the device from the first pivot to the last (include/covgram.h).  The reference instantiates Matrix(G) and calls
// LAPACK pstrf (src/gramian.jl:192-199) and asks for "a special cholesky implementation to avoid instantiating G in the low rank case"
// (:191); covgram/factorize.py has that as a Python loop with one host synchronisation and about ten launches per pivot.  Here a pivot is ONE
// launch and the host is never asked anything: a rank-r factor is r launches enqueued back to back.
//
// Launch k (k = 0 .. max_rank - 1), every workgroup:
//   1. returns if an earlier launch has set `done`;
//   2. reduces the previous launch's per-workgroup (value, index) partials (<= PC_MAX_WGS of them) to the global pivot (dmax, p) — every
//      workgroup does the same reduction of the same words under a TOTAL order (larger value first, then smaller index), so all agree;
//      launch 0 has no partials: the isotropic diagonal is the constant scale phi(0), an n-way tie that goes to index 0;
//   3. stops when !(dmax > tol): workgroup 0 records rank = k and done = 1, nobody writes anything else;
//   4. loads x_p and the pivot row L[p, 0:k] into LDS and sweeps its rows i (consecutive lanes = consecutive i: the reads of L[:, j]
//      are coalesced): col = k(x_i, x_p) - sum_j L[i,j] L[p,j], L[i,k] = col / sqrt(dmax), dres[i] -= L[i,k]^2, dres[p] = 0;
//   5. leaves its own (max, argmin index among the maxima) of the new residual diagonal for launch k + 1.
// The partials are read by all workgroups and written by each: two buffers, used alternately, so a launch never reads what it writes.
// Progress from step to step comes from the launch order alone: no grid barrier, no workgroup waits for another.
#include <math.h>

#include <algorithm>

#include "driver.hpp"
#include "profiles.hpp"

namespace covgram {

constexpr int PC_THREADS = 256;
constexpr int PC_MAX_WGS = 1024;      // partials per buffer; beyond PC_MAX_WGS * PC_THREADS rows a workgroup walks several row blocks

// scratch of one call, at the start of workspace slot 1: [done][pad] then per buffer PC_MAX_WGS values (8 bytes each) and indices
struct PivcholWs {
    int32_t* done;
    void* val[2];
    int32_t* idx[2];
};
constexpr size_t PC_WS_HEAD = 256;
constexpr size_t PC_WS_BYTES = PC_WS_HEAD + 2 * PC_MAX_WGS * (sizeof(double) + sizeof(int32_t));

// the total order of the arg max: a NaN first (numpy's argmax; the stopping test then ends the factorisation), then the larger value,
// then the smaller index
template <typename T>
__device__ __forceinline__ bool pc_before(T va, int32_t ia, T vb, int32_t ib) {
    const bool na = va != va, nb = vb != vb;
    if (na != nb) return na;
    if (!na && va != vb) return va > vb;
    return ia < ib;
}

__device__ __forceinline__ float pc_sqrt(float x) { return __builtin_sqrtf(x); }      // correctly rounded, like numpy's
__device__ __forceinline__ double pc_sqrt(double x) { return __builtin_sqrt(x); }

// (v, i) <- the first of the workgroup's PC_THREADS candidates in that order, in every thread
template <typename T>
__device__ __forceinline__ void pc_block_first(T& v, int32_t& i, T* __restrict__ shv, int32_t* __restrict__ shi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T ov = __shfl_xor(v, o, 64);
        const int32_t oi = __shfl_xor(i, o, 64);
        if (pc_before(ov, oi, v, i)) { v = ov; i = oi; }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();                                            // shv / shi of an earlier call have been read
    if (lane == 0) { shv[wv] = v; shi[wv] = i; }
    __syncthreads();
    v = shv[0]; i = shi[0];
#pragma unroll
    for (int w = 1; w < PC_THREADS / 64; ++w)
        if (pc_before(shv[w], shi[w], v, i)) { v = shv[w]; i = shi[w]; }
}

template <typename T, int FAM>
__global__ __launch_bounds__(PC_THREADS) void pivchol_step_kernel(const T* __restrict__ X, int64_t n, int32_t d, T* __restrict__ L, int64_t ldl,
                                                                  int32_t* __restrict__ piv, T* __restrict__ dres, int32_t* __restrict__ rank,
                                                                  int32_t* __restrict__ done, const T* __restrict__ pin_v,
                                                                  const int32_t* __restrict__ pin_i, T* __restrict__ pout_v,
                                                                  int32_t* __restrict__ pout_i, int32_t k, T tol, T scale, const KParams<T> kp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pc_smem[];
    T* lp = reinterpret_cast<T*>(pc_smem);                     // L[p, 0:k]
    T* xp = lp + k;                                             // x_p, d scalars
    __shared__ T shv[PC_THREADS / 64];
    __shared__ int32_t shi[PC_THREADS / 64];
    if (k > 0 && *done != 0) return;                            // (launch 0 follows the memset of the word)

    auto value = [&](T s) {
        T w = Phi<FAM, T, false>::eval(s, kp);
        if (kp.power != 1) w = ipow(w, kp.power);
        return scale * w;
    };
    // 2. the pivot
    T dmax;
    int32_t p;
    if (k == 0) {
        dmax = value((T)0);
        p = 0;
    } else {
        dmax = -INFINITY;
        p = INT32_MAX;
        for (int q = threadIdx.x; q < (int)gridDim.x; q += PC_THREADS) {
            const T v = pin_v[q];
            const int32_t i = pin_i[q];
            if (pc_before(v, i, dmax, p)) { dmax = v; p = i; }
        }
        pc_block_first(dmax, p, shv, shi);
    }
    // 3. stop?  (uniform over the grid: every workgroup holds the same dmax)
    if (!(dmax > tol)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { *rank = k; *done = 1; }
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { piv[k] = p; *rank = k + 1; }
    // 4. pivot row and pivot point
    for (int j = threadIdx.x; j < k; j += PC_THREADS) lp[j] = L[(int64_t)p + (int64_t)j * ldl];
    for (int l = threadIdx.x; l < d; l += PC_THREADS) xp[l] = X[(int64_t)p * d + l];
    __syncthreads();
    const T rs = pc_sqrt(dmax);
    const T gam = kp.gamma;
    T bv = -INFINITY;
    int32_t bi = INT32_MAX;
    T* __restrict__ Lk = L + (int64_t)k * ldl;
    for (int64_t i = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PC_THREADS) {
        const T* __restrict__ xi = X + i * (int64_t)d;
        T s = (T)0;
        for (int l = 0; l < d; ++l) { const T q = (xi[l] - xp[l]) * gam; s = fma_t(q, q, s); }     // covgram_matrix's entry
        const T kv = value(s);
        T acc = (T)0;
        const T* __restrict__ Li = L + i;
        int j = 0;
        for (; j + 4 <= k; j += 4) {                            // four loads in flight, the sum in the order j = 0 .. k - 1
            const T l0 = Li[(int64_t)j * ldl], l1 = Li[(int64_t)(j + 1) * ldl], l2 = Li[(int64_t)(j + 2) * ldl], l3 = Li[(int64_t)(j + 3) * ldl];
            acc = fma_t(l0, lp[j], acc); acc = fma_t(l1, lp[j + 1], acc); acc = fma_t(l2, lp[j + 2], acc); acc = fma_t(l3, lp[j + 3], acc);
        }
        for (; j < k; ++j) acc = fma_t(Li[(int64_t)j * ldl], lp[j], acc);
        const T lik = (kv - acc) / rs;
        Lk[i] = lik;
        const T dold = (k == 0) ? dmax : dres[i];
        // the pivot is retired by its exact zero, and a zero stays zero (the oracle's d[piv[:k+1]] = 0): rounding in the later columns of
        // a retired row must not move it; a live entry that is exactly zero (a copy of a pivot point) could never be chosen anyway
        const T dnew = (i == (int64_t)p || dold == (T)0) ? (T)0 : fma_t(-lik, lik, dold);
        dres[i] = dnew;
        if (pc_before(dnew, (int32_t)i, bv, bi)) { bv = dnew; bi = (int32_t)i; }
    }
    // 5. this workgroup's partial
    pc_block_first(bv, bi, shv, shi);
    if (threadIdx.x == 0) { pout_v[blockIdx.x] = bv; pout_i[blockIdx.x] = bi; }
}

static const char* pivchol_family_name(int family) {
    switch (family) {
        case COVGRAM_DOT: return "Dot";
        case COVGRAM_EXPDOT: return "ExponentialDot";
        case COVGRAM_ASINDOT: return "AsinDot (NeuralNetwork)";
        case COVGRAM_CONSTANT: return "Constant";
        default: return "unknown";
    }
}

template <typename T>
static void pivchol_launch(const covgram_points* X, const HostKernel& hk, int32_t max_rank, double tol, void* L, int64_t ldl, int32_t* piv,
                           void* dres, int32_t* rank, const PivcholWs& w, unsigned nwg, hipStream_t stream) {
    const KParams<T> kp = cast_params<T>(hk.kp);
    for (int32_t k = 0; k < max_rank; ++k) {
        const size_t lds = (size_t)(k + X->d) * sizeof(T);
        const int in = (k + 1) & 1, out = k & 1;
#define CG_PC(F)                                                                                                                              \
        case F:                                                                                                                               \
            hipLaunchKernelGGL((pivchol_step_kernel<T, F>), dim3(nwg), dim3(PC_THREADS), lds, stream, (const T*)X->dptr, X->n, X->d, (T*)L, ldl, \
                               piv, (T*)dres, rank, w.done, (const T*)w.val[in], (const int32_t*)w.idx[in], (T*)w.val[out], w.idx[out], k, (T)tol, \
                               (T)hk.kp.scale, kp);                                                                                           \
            break;
        switch (hk.k.family) {
            CG_PC(COVGRAM_EQ) CG_PC(COVGRAM_EXP) CG_PC(COVGRAM_RQ) CG_PC(COVGRAM_GAMMAEXP) CG_PC(COVGRAM_CAUCHY) CG_PC(COVGRAM_IMQ)
            CG_PC(COVGRAM_MATERNP) CG_PC(COVGRAM_MATERN)
            default: break;
        }
#undef CG_PC
    }
}

}  // namespace covgram

using namespace covgram;

extern "C" {

int covgram_pivoted_cholesky(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, int32_t max_rank, double tol, void* L,
                             int64_t ldl, int32_t* piv, void* dres, int32_t* rank) {
    // everything that can be refused is refused here, before any device call
    CG_REQUIRE(k != nullptr, COVGRAM_EINVAL, "pivoted_cholesky: kernel is NULL");
    if (k->family == COVGRAM_COMPOSITE) {
        const covgram_kernel_composite* c = (const covgram_kernel_composite*)k;
        if (c->nterms > 1) set_error("pivoted_cholesky: a Sum of %d terms is not supported (single isotropic profiles only)", c->nterms);
        else set_error("pivoted_cholesky: a Product of profiles is not supported (single isotropic profiles only)");
        return COVGRAM_EUNSUPPORTED;
    }
    const bool ok = k->family == COVGRAM_EQ || k->family == COVGRAM_EXP || k->family == COVGRAM_RQ || k->family == COVGRAM_GAMMAEXP ||
                    k->family == COVGRAM_CAUCHY || k->family == COVGRAM_IMQ || k->family == COVGRAM_MATERNP || k->family == COVGRAM_MATERN;
    CG_REQUIRE(ok, COVGRAM_EUNSUPPORTED, "pivoted_cholesky: %s (family %d) is not an isotropic profile (supported: EQ, Exponential, RQ, "
               "GammaExponential, Cauchy, InverseMultiQuadratic, MaternP, Matern)", pivchol_family_name(k->family), k->family);
    CG_REQUIRE(tol >= 0, COVGRAM_EINVAL, "pivoted_cholesky: tol = %g must be >= 0", tol);
    CG_REQUIRE(max_rank >= 0, COVGRAM_EINVAL, "pivoted_cholesky: max_rank = %d is negative", max_rank);
    CG_REQUIRE(max_rank <= COVGRAM_PIVCHOL_MAX_RANK, COVGRAM_EUNSUPPORTED, "pivoted_cholesky: max_rank = %d exceeds COVGRAM_PIVCHOL_MAX_RANK = %d",
               max_rank, COVGRAM_PIVCHOL_MAX_RANK);
    CG_REQUIRE(ctx && X && rank, COVGRAM_EINVAL, "pivoted_cholesky: NULL argument (ctx, X or rank)");
    CG_REQUIRE(X->ctx == ctx, COVGRAM_EINVAL, "points belong to a different ctx");
    const int64_t n = X->n;
    CG_REQUIRE(max_rank <= n, COVGRAM_EINVAL, "pivoted_cholesky: max_rank = %d exceeds n = %lld", max_rank, (long long)n);
    CG_REQUIRE(n < ((int64_t)1 << 31), COVGRAM_EINVAL, "pivoted_cholesky: n = %lld rows do not fit 32-bit pivots", (long long)n);
    CG_REQUIRE(ldl >= n, COVGRAM_EINVAL, "DimensionMismatch: pivoted_cholesky: ldl=%lld < n=%lld", (long long)ldl, (long long)n);
    const bool empty = n == 0 || max_rank == 0;
    CG_REQUIRE(empty || (L && piv && dres), COVGRAM_EINVAL, "pivoted_cholesky: L, piv or dres is NULL");
    const int dtype = X->dtype;
    const size_t ts = dtype_size(dtype);
    CG_REQUIRE(((size_t)max_rank + (size_t)X->d) * ts <= 65536, COVGRAM_EUNSUPPORTED,
               "pivoted_cholesky: the pivot row and point (max_rank + d = %lld scalars) exceed the 64 KB of LDS", (long long)max_rank + X->d);
    HostKernel hk;
    int rc = make_host_kernel(k, dtype, true, &hk);            // gamma = 1 / l, unfolded profiles: the evaluation of covgram_matrix
    if (rc) return rc;
    CG_DEVICE(ctx);
    if (empty) {
        CG_CHECK_HIP(hipMemsetAsync(rank, 0, sizeof(int32_t), ctx->stream));
        return COVGRAM_OK;
    }
    void* wsp;
    rc = ws_reserve(ctx, 1, PC_WS_BYTES, &wsp);                // sized on first use (the slot never shrinks: a capture finds it in place)
    if (rc) return rc;
    PivcholWs w;
    char* base = (char*)wsp;
    w.done = (int32_t*)base;
    w.val[0] = base + PC_WS_HEAD;
    w.val[1] = base + PC_WS_HEAD + PC_MAX_WGS * sizeof(double);
    w.idx[0] = (int32_t*)(base + PC_WS_HEAD + 2 * PC_MAX_WGS * sizeof(double));
    w.idx[1] = w.idx[0] + PC_MAX_WGS;
    CG_CHECK_HIP(hipMemsetAsync(w.done, 0, PC_WS_HEAD, ctx->stream));
    const unsigned nwg = (unsigned)std::min<int64_t>((n + PC_THREADS - 1) / PC_THREADS, PC_MAX_WGS);
    { TimerScope tm(ctx); by_dtype(dtype, [&](auto t) { pivchol_launch<decltype(t)>(X, hk, max_rank, tol, L, ldl, piv, dres, rank, w, nwg, ctx->stream); }); }
    CG_CHECK_HIP(hipGetLastError());
    return COVGRAM_OK;
}

}  // extern "C"
