// covgram — batched CG: the vector recurrences of ONE iteration of nrhs independent conjugate-gradient solves that share a matrix
// right-hand-side MVM (covgram/solve.py: mbcg).  Per column the iteration of krylov.hip (IterativeSolvers.cg! 0.9.2, the reference's
// caller of mul! for `G \ b`, src/gramian.jl:229-238), with a preconditioned form split in two phases around the caller's Z = M^-1 R:
//     update:     AP += diag .* P;  gamma = P . AP;  alpha = rz / gamma;  X += alpha P;  R -= alpha AP;  rr = R . R
//     direction:  rz' = R . Z;  beta = rz' / rz;  P = Z + beta P;  rz <- rz';  active &= rr > tol2
// As library vector operations that is a dozen launches plus `where` masks for the columns that have stopped.  Here every per-column
// scalar (fp64 whatever the vectors' type) stays on the device, a stopped column is skipped, and the sums run in a fixed order: wave
// shuffles, LDS, then a per-column slab of workgroup partials that the NEXT launch reduces (no floating-point atomic, no workgroup waits
// for another).  The only atomic is the integer count of active columns.
#include <algorithm>
#include <cstdint>

#include "profiles.hpp"

namespace covgram {

constexpr int BCG_THREADS = 256, BCG_GROUPS = 2, BCG_SLAB = COVGRAM_BCG_SLAB, BCG1_THREADS = 1024;
static_assert(BCG_SLAB == 64, "a slab is reduced by one wave");
// private fields of the state: the (rz, active) the running step works with — committed from the public fields by the step's first
// launch, so that no launch reads a word another workgroup of the same launch writes
constexpr int BCG_RZ_CUR = 5, BCG_ACT_CUR = 6, BCG_GAMMA = 7;

template <typename T> struct BcgVec { static constexpr int V = 16 / sizeof(T); typedef T type __attribute__((ext_vector_type(16 / sizeof(T)))); };

// V consecutive entries from i: one 16-byte access where the column is aligned (vec) and the group is inside it, else entry by entry
template <typename T> __device__ __forceinline__ void bcg_load(const T* __restrict__ v, int64_t i, int64_t n, bool vec, T (&out)[BcgVec<T>::V]) {
    constexpr int V = BcgVec<T>::V;
    if (vec && i + V <= n) { const typename BcgVec<T>::type q = *reinterpret_cast<const typename BcgVec<T>::type*>(v + i); for (int c = 0; c < V; ++c) out[c] = q[c]; }
    else for (int c = 0; c < V; ++c) out[c] = i + c < n ? v[i + c] : (T)0;
}
template <typename T> __device__ __forceinline__ void bcg_store(T* __restrict__ v, int64_t i, int64_t n, bool vec, const T (&in)[BcgVec<T>::V]) {
    constexpr int V = BcgVec<T>::V;
    if (vec && i + V <= n) { typename BcgVec<T>::type q; for (int c = 0; c < V; ++c) q[c] = in[c]; *reinterpret_cast<typename BcgVec<T>::type*>(v + i) = q; }
    else for (int c = 0; c < V; ++c) if (i + c < n) v[i + c] = in[c];
}
__device__ __forceinline__ bool bcg_aligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 15) == 0;
}

__device__ __forceinline__ double bcg_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// fixed-order workgroup sum, the same value in every thread (sh: THREADS / 64 doubles, free again on return)
template <int THREADS>
__device__ __forceinline__ double bcg_block_sum(double v, double* sh) {
    v = bcg_wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < THREADS / 64; ++i) t += sh[i];
    __syncthreads();
    return t;
}
// the sum of a column's nb <= 64 workgroup partials: every wave reduces them with the same shuffles, so every thread of every workgroup
// holds the same bits
__device__ __forceinline__ double bcg_slab_sum(const double* __restrict__ slab, int nb) {
    const int l = threadIdx.x & 63;
    return bcg_wave_sum(l < nb ? slab[l] : 0.0);
}
__device__ __forceinline__ double* bcg_slab(double* state, int64_t nrhs, int which, int64_t j) {
    return state + (COVGRAM_BCG_FIELDS + (int64_t)which * BCG_SLAB) * nrhs + j * BCG_SLAB;
}

// ---- set-up: one workgroup per column -------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(BCG1_THREADS) void bcg_init_kernel(int64_t n, int64_t nrhs, const T* __restrict__ R, int64_t ldr, const T* __restrict__ Z, int64_t ldz,
                                                                double reltol, double abstol, double* __restrict__ state, int32_t* __restrict__ n_active) {
    __shared__ double sh[BCG1_THREADS / 64];
    for (int64_t j = blockIdx.x; j < nrhs; j += gridDim.x) {
        const T* r = R + j * ldr;
        const T* z = Z + j * ldz;
        double srr = 0.0, srz = 0.0;
        for (int64_t i = threadIdx.x; i < n; i += BCG1_THREADS) {
            const double ri = (double)r[i];
            srr += ri * ri;
            srz += ri * (double)z[i];
        }
        const double rr = bcg_block_sum<BCG1_THREADS>(srr, sh), rz = bcg_block_sum<BCG1_THREADS>(srz, sh);
        if (threadIdx.x == 0) {
            const double tol2 = fmax(reltol * reltol * rr, abstol * abstol);
            const bool act = rr > tol2;
            state[COVGRAM_BCG_RZ * nrhs + j] = rz;
            state[COVGRAM_BCG_TOL2 * nrhs + j] = tol2;
            state[COVGRAM_BCG_RR * nrhs + j] = rr;
            state[COVGRAM_BCG_ACTIVE * nrhs + j] = act ? 1.0 : 0.0;
            state[COVGRAM_BCG_ITERS * nrhs + j] = 0.0;
            state[BCG_RZ_CUR * nrhs + j] = rz;
            state[BCG_ACT_CUR * nrhs + j] = act ? 1.0 : 0.0;
            state[BCG_GAMMA * nrhs + j] = 0.0;
            if (act) atomicAdd(n_active, 1);
        }
    }
}

// what the last launch of a step leaves for column j (one thread): the logged beta, and for an active column rz, rr, iters, active
__device__ __forceinline__ void bcg_commit(double* __restrict__ state, int64_t nrhs, int64_t j, bool act, double rz_new, double rr, double beta,
                                           int32_t* __restrict__ n_active, double* __restrict__ blog) {
    if (blog) blog[j] = beta;
    if (!act) return;
    state[COVGRAM_BCG_RZ * nrhs + j] = rz_new;
    state[COVGRAM_BCG_RR * nrhs + j] = rr;
    state[COVGRAM_BCG_ITERS * nrhs + j] += 1.0;
    if (!(rr > state[COVGRAM_BCG_TOL2 * nrhs + j])) {
        state[COVGRAM_BCG_ACTIVE * nrhs + j] = 0.0;
        atomicSub(n_active, 1);
    }
}

// ---- the general path: a (row blocks x columns) grid; workgroup (b, j) walks the groups b, b + nb, ... of column j ----------------
// slab A[j][b] = the workgroup's part of P_j . AP_j, with AP_j <- AP_j + diag .* P_j on the way (SHIFT); commits (rz, active)
template <typename T, bool SHIFT>
__global__ __launch_bounds__(BCG_THREADS) void bcg_dot_kernel(int64_t n, int64_t nrhs, const T* __restrict__ P, int64_t ldp, T* __restrict__ AP, int64_t ldap,
                                                              const T* __restrict__ diag, double* __restrict__ state) {
    constexpr int V = BcgVec<T>::V;
    __shared__ double sh[BCG_THREADS / 64];
    const int b = blockIdx.x, nb = gridDim.x;
    for (int64_t j = blockIdx.y; j < nrhs; j += gridDim.y) {
        const bool act = state[COVGRAM_BCG_ACTIVE * nrhs + j] != 0.0;
        if (b == 0 && threadIdx.x == 0) {
            state[BCG_RZ_CUR * nrhs + j] = state[COVGRAM_BCG_RZ * nrhs + j];
            state[BCG_ACT_CUR * nrhs + j] = act ? 1.0 : 0.0;
        }
        if (!act) continue;                                        // (uniform over the workgroup)
        const T* p = P + j * ldp;
        T* ap = AP + j * ldap;
        const bool vec = bcg_aligned(p, ap, diag);
        double s = 0.0;
        for (int64_t i = ((int64_t)b * BCG_THREADS + threadIdx.x) * V; i < n; i += (int64_t)nb * BCG_THREADS * V) {
            T pv[V], av[V];
            bcg_load(p, i, n, vec, pv); bcg_load(ap, i, n, vec, av);
            if (SHIFT) {
                T dv[V];
                bcg_load(diag, i, n, vec, dv);
#pragma unroll
                for (int c = 0; c < V; ++c) av[c] = cg_fma(dv[c], pv[c], av[c]);
                bcg_store(ap, i, n, vec, av);
            }
#pragma unroll
            for (int c = 0; c < V; ++c) s += (double)pv[c] * (double)av[c];
        }
        const double t = bcg_block_sum<BCG_THREADS>(s, sh);
        if (threadIdx.x == 0) bcg_slab(state, nrhs, 0, j)[b] = t;
    }
}

// gamma = sum(slab A);  alpha;  X += alpha P;  R -= alpha AP;  slab B[j][b] = the workgroup's part of R_j . R_j
template <typename T>
__global__ __launch_bounds__(BCG_THREADS) void bcg_update_kernel(int64_t n, int64_t nrhs, T* __restrict__ X, int64_t ldx, T* __restrict__ R, int64_t ldr,
                                                                 const T* __restrict__ P, int64_t ldp, const T* __restrict__ AP, int64_t ldap,
                                                                 double* __restrict__ state, double* __restrict__ alog) {
    constexpr int V = BcgVec<T>::V;
    __shared__ double sh[BCG_THREADS / 64];
    const int b = blockIdx.x, nb = gridDim.x;
    for (int64_t j = blockIdx.y; j < nrhs; j += gridDim.y) {
        const bool act = state[BCG_ACT_CUR * nrhs + j] != 0.0;
        if (!act) {                                                // frozen: X_j, R_j and the column's partials are not touched
            if (alog && b == 0 && threadIdx.x == 0) alog[j] = 0.0;
            continue;
        }
        const double rz = state[BCG_RZ_CUR * nrhs + j];
        const double gamma = bcg_slab_sum(bcg_slab(state, nrhs, 0, j), nb);
        const double alpha_d = (rz != 0.0 && gamma != 0.0) ? rz / gamma : 0.0;     // 0 / 0 must not reach X
        if (b == 0 && threadIdx.x == 0) { if (alog) alog[j] = alpha_d; state[BCG_GAMMA * nrhs + j] = gamma; }
        const T alpha = (T)alpha_d;
        T* x = X + j * ldx;
        T* r = R + j * ldr;
        const T* p = P + j * ldp;
        const T* ap = AP + j * ldap;
        const bool vec = bcg_aligned(x, r, p, ap);
        double s = 0.0;
        for (int64_t i = ((int64_t)b * BCG_THREADS + threadIdx.x) * V; i < n; i += (int64_t)nb * BCG_THREADS * V) {
            T xv[V], rv[V], pv[V], av[V];
            bcg_load(x, i, n, vec, xv); bcg_load(r, i, n, vec, rv); bcg_load(p, i, n, vec, pv); bcg_load(ap, i, n, vec, av);
#pragma unroll
            for (int c = 0; c < V; ++c) {
                xv[c] = cg_fma(alpha, pv[c], xv[c]);
                rv[c] = cg_fma(-alpha, av[c], rv[c]);
                s += (double)rv[c] * (double)rv[c];
            }
            bcg_store(x, i, n, vec, xv); bcg_store(r, i, n, vec, rv);
        }
        const double t = bcg_block_sum<BCG_THREADS>(s, sh);
        if (threadIdx.x == 0) bcg_slab(state, nrhs, 1, j)[b] = t;
    }
}

// a preconditioned direction phase's first launch: slab A[j][b] = the workgroup's part of R_j . Z_j
template <typename T>
__global__ __launch_bounds__(BCG_THREADS) void bcg_rz_kernel(int64_t n, int64_t nrhs, const T* __restrict__ R, int64_t ldr, const T* __restrict__ Z, int64_t ldz,
                                                             double* __restrict__ state) {
    constexpr int V = BcgVec<T>::V;
    __shared__ double sh[BCG_THREADS / 64];
    const int b = blockIdx.x, nb = gridDim.x;
    for (int64_t j = blockIdx.y; j < nrhs; j += gridDim.y) {
        if (state[BCG_ACT_CUR * nrhs + j] == 0.0) continue;
        const T* r = R + j * ldr;
        const T* z = Z + j * ldz;
        const bool vec = bcg_aligned(r, z);
        double s = 0.0;
        for (int64_t i = ((int64_t)b * BCG_THREADS + threadIdx.x) * V; i < n; i += (int64_t)nb * BCG_THREADS * V) {
            T rv[V], zv[V];
            bcg_load(r, i, n, vec, rv); bcg_load(z, i, n, vec, zv);
#pragma unroll
            for (int c = 0; c < V; ++c) s += (double)rv[c] * (double)zv[c];
        }
        const double t = bcg_block_sum<BCG_THREADS>(s, sh);
        if (threadIdx.x == 0) bcg_slab(state, nrhs, 0, j)[b] = t;
    }
}

// rr = sum(slab B);  rz' = rr (Z = R) or sum(slab A) (SEPZ);  beta;  P = Z + beta P;  the column's state
template <typename T, bool SEPZ>
__global__ __launch_bounds__(BCG_THREADS) void bcg_direction_kernel(int64_t n, int64_t nrhs, const T* __restrict__ Z, int64_t ldz, T* __restrict__ P, int64_t ldp,
                                                                    double* __restrict__ state, int32_t* __restrict__ n_active, double* __restrict__ blog) {
    constexpr int V = BcgVec<T>::V;
    const int b = blockIdx.x, nb = gridDim.x;
    for (int64_t j = blockIdx.y; j < nrhs; j += gridDim.y) {
        const bool act = state[BCG_ACT_CUR * nrhs + j] != 0.0;
        const double rz = state[BCG_RZ_CUR * nrhs + j];
        double rr = 0.0, rz_new = 0.0;
        if (act) {
            rr = bcg_slab_sum(bcg_slab(state, nrhs, 1, j), nb);
            rz_new = SEPZ ? bcg_slab_sum(bcg_slab(state, nrhs, 0, j), nb) : rr;
        }
        const double beta_d = (act && rz != 0.0) ? rz_new / rz : 0.0;
        const T beta = (T)beta_d;
        const T* z = Z + j * ldz;
        T* p = P + j * ldp;
        const bool vec = bcg_aligned(z, p);
        for (int64_t i = ((int64_t)b * BCG_THREADS + threadIdx.x) * V; i < n; i += (int64_t)nb * BCG_THREADS * V) {
            T zv[V], pv[V];
            bcg_load(z, i, n, vec, zv); bcg_load(p, i, n, vec, pv);
#pragma unroll
            for (int c = 0; c < V; ++c) pv[c] = beta == (T)0 ? zv[c] : cg_fma(beta, pv[c], zv[c]);   // (beta = 0: P = Z whatever P held)
            bcg_store(p, i, n, vec, pv);
        }
        if (b == 0 && threadIdx.x == 0) bcg_commit(state, nrhs, j, act, rz_new, rr, beta_d, n_active, blog);
    }
}

// ---- small columns: the whole unpreconditioned step of column j in workgroup j, ONE launch -----------------------------------------
// G groups of V entries per thread, group g of thread t at (t + 1024 g) V (n <= 1024 G V; every column 16-byte aligned): P, AP and R
// stay in registers between the two sums (the design of cg_step_one_kernel, krylov.hip)
template <typename T, int G, bool SHIFT>
__global__ __launch_bounds__(BCG1_THREADS) void bcg_step_one_kernel(int n, int64_t nrhs, T* __restrict__ X, int64_t ldx, T* __restrict__ R, int64_t ldr,
                                                                    T* __restrict__ P, int64_t ldp, T* __restrict__ AP, int64_t ldap, const T* __restrict__ diag,
                                                                    double* __restrict__ state, int32_t* __restrict__ n_active,
                                                                    double* __restrict__ alog, double* __restrict__ blog) {
    constexpr int V = BcgVec<T>::V;
    __shared__ double sh[BCG1_THREADS / 64];
    const int t = threadIdx.x;
    const int64_t j = blockIdx.x;                              // (a grid of nrhs workgroups)
    T* x = X + j * ldx;
    T* r = R + j * ldr;
    T* p = P + j * ldp;
    T* ap = AP + j * ldap;
    const bool act = state[COVGRAM_BCG_ACTIVE * nrhs + j] != 0.0;
    if (!act) {                                                // frozen: P_j = R_j (beta = 0), the logs 0, nothing else
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int i = (t + g * BCG1_THREADS) * V;
            if (i >= n) continue;
            T rv[V];
            bcg_load<T>(r, i, n, true, rv); bcg_store<T>(p, i, n, true, rv);
        }
        if (t == 0) { if (alog) alog[j] = 0.0; if (blog) blog[j] = 0.0; }
        return;
    }
    const double rz = state[COVGRAM_BCG_RZ * nrhs + j];
    T pv[G][V], av[G][V], rv[G][V];
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int i = (t + g * BCG1_THREADS) * V;
        bcg_load<T>(p, i, n, true, pv[g]); bcg_load<T>(ap, i, n, true, av[g]); bcg_load<T>(r, i, n, true, rv[g]);
        if (SHIFT) {
            T dv[V];
            bcg_load<T>(diag, i, n, true, dv);
#pragma unroll
            for (int c = 0; c < V; ++c) av[g][c] = cg_fma(dv[c], pv[g][c], av[g][c]);
        }
#pragma unroll
        for (int c = 0; c < V; ++c) s += (double)pv[g][c] * (double)av[g][c];
    }
    const double gamma = bcg_block_sum<BCG1_THREADS>(s, sh);
    const double alpha_d = (rz != 0.0 && gamma != 0.0) ? rz / gamma : 0.0;
    const T alpha = (T)alpha_d;
    s = 0.0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int i = (t + g * BCG1_THREADS) * V;
        T xv[V];
        bcg_load<T>(x, i, n, true, xv);
#pragma unroll
        for (int c = 0; c < V; ++c) {
            rv[g][c] = cg_fma(-alpha, av[g][c], rv[g][c]);
            s += (double)rv[g][c] * (double)rv[g][c];
            xv[c] = cg_fma(alpha, pv[g][c], xv[c]);
        }
        bcg_store<T>(x, i, n, true, xv); bcg_store<T>(r, i, n, true, rv[g]);
        if (SHIFT) bcg_store<T>(ap, i, n, true, av[g]);
    }
    const double rr = bcg_block_sum<BCG1_THREADS>(s, sh);
    const double beta_d = rz != 0.0 ? rr / rz : 0.0;
    const T beta = (T)beta_d;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int i = (t + g * BCG1_THREADS) * V;
#pragma unroll
        for (int c = 0; c < V; ++c) pv[g][c] = beta == (T)0 ? rv[g][c] : cg_fma(beta, pv[g][c], rv[g][c]);
        bcg_store<T>(p, i, n, true, pv[g]);
    }
    if (t == 0) {
        if (alog) alog[j] = alpha_d;
        state[BCG_GAMMA * nrhs + j] = gamma;
        bcg_commit(state, nrhs, j, true, rr, rr, beta_d, n_active, blog);
    }
}

constexpr int BCG_MAX_GRID_Y = 65535;

static dim3 bcg_grid(int64_t n, int64_t nrhs, int V) {
    const int64_t per = (int64_t)BCG_THREADS * V * BCG_GROUPS;
    return dim3((unsigned)std::min<int64_t>(BCG_SLAB, std::max<int64_t>(1, (n + per - 1) / per)), (unsigned)std::min<int64_t>(nrhs, BCG_MAX_GRID_Y));
}

template <typename T>
static void bcg_update_T(hipStream_t st, int64_t n, int64_t nrhs, T* X, int64_t ldx, T* R, int64_t ldr, const T* P, int64_t ldp, T* AP, int64_t ldap,
                         const T* diag, double* state, double* alog) {
    const dim3 grid = bcg_grid(n, nrhs, BcgVec<T>::V);
    if (diag) hipLaunchKernelGGL((bcg_dot_kernel<T, true>), grid, dim3(BCG_THREADS), 0, st, n, nrhs, P, ldp, AP, ldap, diag, state);
    else hipLaunchKernelGGL((bcg_dot_kernel<T, false>), grid, dim3(BCG_THREADS), 0, st, n, nrhs, P, ldp, AP, ldap, diag, state);
    hipLaunchKernelGGL(bcg_update_kernel<T>, grid, dim3(BCG_THREADS), 0, st, n, nrhs, X, ldx, R, ldr, P, ldp, (const T*)AP, ldap, state, alog);
}

template <typename T>
static void bcg_direction_T(hipStream_t st, int64_t n, int64_t nrhs, const T* R, int64_t ldr, const T* Z, int64_t ldz, T* P, int64_t ldp, double* state,
                            int32_t* n_active, double* blog) {
    const dim3 grid = bcg_grid(n, nrhs, BcgVec<T>::V);
    hipLaunchKernelGGL(bcg_rz_kernel<T>, grid, dim3(BCG_THREADS), 0, st, n, nrhs, R, ldr, Z, ldz, state);
    hipLaunchKernelGGL((bcg_direction_kernel<T, true>), grid, dim3(BCG_THREADS), 0, st, n, nrhs, Z, ldz, P, ldp, state, n_active, blog);
}

template <typename T, int G>
static void bcg_step_one(hipStream_t st, int64_t n, int64_t nrhs, T* X, int64_t ldx, T* R, int64_t ldr, T* P, int64_t ldp, T* AP, int64_t ldap, const T* diag,
                         double* state, int32_t* n_active, double* alog, double* blog) {
    const dim3 grid((unsigned)nrhs);
    if (diag) hipLaunchKernelGGL((bcg_step_one_kernel<T, G, true>), grid, dim3(BCG1_THREADS), 0, st, (int)n, nrhs, X, ldx, R, ldr, P, ldp, AP, ldap, diag, state, n_active, alog, blog);
    else hipLaunchKernelGGL((bcg_step_one_kernel<T, G, false>), grid, dim3(BCG1_THREADS), 0, st, (int)n, nrhs, X, ldx, R, ldr, P, ldp, AP, ldap, diag, state, n_active, alog, blog);
}

template <typename T>
static void bcg_step_T(hipStream_t st, int64_t n, int64_t nrhs, T* X, int64_t ldx, T* R, int64_t ldr, T* P, int64_t ldp, T* AP, int64_t ldap, const T* diag,
                       double* state, int32_t* n_active, double* alog, double* blog) {
    constexpr int V = BcgVec<T>::V;
    // every column of every array starts on a 16-byte boundary: the bases do, and with more than one column the leading dimensions
    const bool lds = nrhs == 1 || ((ldx | ldr | ldp | ldap) % V) == 0;
    const bool aligned = lds && (((uintptr_t)X | (uintptr_t)R | (uintptr_t)P | (uintptr_t)AP | (uintptr_t)diag) & 15) == 0;
    if (aligned && n <= (int64_t)1 * BCG1_THREADS * V) return bcg_step_one<T, 1>(st, n, nrhs, X, ldx, R, ldr, P, ldp, AP, ldap, diag, state, n_active, alog, blog);
    if (aligned && n <= (int64_t)2 * BCG1_THREADS * V) return bcg_step_one<T, 2>(st, n, nrhs, X, ldx, R, ldr, P, ldp, AP, ldap, diag, state, n_active, alog, blog);
    if (aligned && n <= (int64_t)4 * BCG1_THREADS * V) return bcg_step_one<T, 4>(st, n, nrhs, X, ldx, R, ldr, P, ldp, AP, ldap, diag, state, n_active, alog, blog);
    bcg_update_T<T>(st, n, nrhs, X, ldx, R, ldr, P, ldp, AP, ldap, diag, state, alog);
    hipLaunchKernelGGL((bcg_direction_kernel<T, false>), bcg_grid(n, nrhs, V), dim3(BCG_THREADS), 0, st, n, nrhs, (const T*)R, ldr, P, ldp, state, n_active, blog);
}

}  // namespace covgram

using namespace covgram;

// the checks every entry point makes before any device call; 1 = nothing to do
static int bcg_check(covgram_ctx* ctx, int64_t n, int64_t nrhs, int32_t dtype, int64_t it, std::initializer_list<int64_t> lds) {
    CG_REQUIRE(ctx != nullptr, COVGRAM_EINVAL, "ctx is NULL");
    CG_REQUIRE(dtype == COVGRAM_F32 || dtype == COVGRAM_F64, COVGRAM_EINVAL, "dtype must be COVGRAM_F32 or COVGRAM_F64");
    CG_REQUIRE(n >= 0 && nrhs >= 0, COVGRAM_EINVAL, "DimensionMismatch: n = %lld and nrhs = %lld must be >= 0", (long long)n, (long long)nrhs);
    CG_REQUIRE(it >= 0, COVGRAM_EINVAL, "the iteration number it = %lld must be >= 0", (long long)it);
    for (int64_t ld : lds) CG_REQUIRE(ld >= n, COVGRAM_EINVAL, "DimensionMismatch: a leading dimension %lld is below n = %lld", (long long)ld, (long long)n);
    return (n == 0 || nrhs == 0) ? 1 : COVGRAM_OK;
}
#define BCG_CHECK(...)                                \
    do {                                              \
        const int _s = bcg_check(__VA_ARGS__);        \
        if (_s != COVGRAM_OK) return _s < 0 ? _s : COVGRAM_OK; \
    } while (0)

extern "C" int covgram_bcg_init(covgram_ctx* ctx, int64_t n, int64_t nrhs, int32_t dtype, const void* R, int64_t ldr, const void* Z, int64_t ldz,
                                double reltol, double abstol, double* state, int32_t* n_active) {
    CG_REQUIRE(ctx != nullptr, COVGRAM_EINVAL, "ctx is NULL");
    CG_REQUIRE(dtype == COVGRAM_F32 || dtype == COVGRAM_F64, COVGRAM_EINVAL, "dtype must be COVGRAM_F32 or COVGRAM_F64");
    CG_REQUIRE(n >= 0 && nrhs >= 0, COVGRAM_EINVAL, "DimensionMismatch: n = %lld and nrhs = %lld must be >= 0", (long long)n, (long long)nrhs);
    CG_REQUIRE(ldr >= n && ldz >= n, COVGRAM_EINVAL, "DimensionMismatch: a leading dimension (%lld, %lld) is below n = %lld", (long long)ldr, (long long)ldz, (long long)n);
    CG_REQUIRE(reltol >= 0.0 && abstol >= 0.0, COVGRAM_EINVAL, "reltol = %g and abstol = %g must be >= 0", reltol, abstol);
    if (nrhs == 0) return COVGRAM_OK;                              // (n = 0: every column starts inactive with rr = 0)
    CG_REQUIRE(state && n_active && (n == 0 || (R && Z)), COVGRAM_EINVAL, "NULL array");
    CG_DEVICE(ctx);
    CG_CHECK_HIP(hipMemsetAsync(n_active, 0, sizeof(int32_t), ctx->stream));
    const dim3 grid((unsigned)std::min<int64_t>(nrhs, 1 << 20));
    if (dtype == COVGRAM_F32) hipLaunchKernelGGL(bcg_init_kernel<float>, grid, dim3(BCG1_THREADS), 0, ctx->stream, n, nrhs, (const float*)R, ldr, (const float*)Z, ldz, reltol, abstol, state, n_active);
    else hipLaunchKernelGGL(bcg_init_kernel<double>, grid, dim3(BCG1_THREADS), 0, ctx->stream, n, nrhs, (const double*)R, ldr, (const double*)Z, ldz, reltol, abstol, state, n_active);
    CG_CHECK_HIP(hipGetLastError());
    return COVGRAM_OK;
}

extern "C" int covgram_bcg_step(covgram_ctx* ctx, int64_t n, int64_t nrhs, int32_t dtype, void* X, int64_t ldx, void* R, int64_t ldr, void* P, int64_t ldp,
                                void* AP, int64_t ldap, const void* diag, double* state, int32_t* n_active, double* alpha_log, double* beta_log, int64_t it) {
    BCG_CHECK(ctx, n, nrhs, dtype, it, {ldx, ldr, ldp, ldap});
    CG_REQUIRE(X && R && P && AP && state && n_active, COVGRAM_EINVAL, "NULL array");
    CG_DEVICE(ctx);
    double* const al = alpha_log ? alpha_log + it * nrhs : nullptr;
    double* const bl = beta_log ? beta_log + it * nrhs : nullptr;
    if (dtype == COVGRAM_F32) bcg_step_T<float>(ctx->stream, n, nrhs, (float*)X, ldx, (float*)R, ldr, (float*)P, ldp, (float*)AP, ldap, (const float*)diag, state, n_active, al, bl);
    else bcg_step_T<double>(ctx->stream, n, nrhs, (double*)X, ldx, (double*)R, ldr, (double*)P, ldp, (double*)AP, ldap, (const double*)diag, state, n_active, al, bl);
    CG_CHECK_HIP(hipGetLastError());
    return COVGRAM_OK;
}

extern "C" int covgram_bcg_update(covgram_ctx* ctx, int64_t n, int64_t nrhs, int32_t dtype, void* X, int64_t ldx, void* R, int64_t ldr, const void* P, int64_t ldp,
                                  void* AP, int64_t ldap, const void* diag, double* state, double* alpha_log, int64_t it) {
    BCG_CHECK(ctx, n, nrhs, dtype, it, {ldx, ldr, ldp, ldap});
    CG_REQUIRE(X && R && P && AP && state, COVGRAM_EINVAL, "NULL array");
    CG_DEVICE(ctx);
    double* const al = alpha_log ? alpha_log + it * nrhs : nullptr;
    if (dtype == COVGRAM_F32) bcg_update_T<float>(ctx->stream, n, nrhs, (float*)X, ldx, (float*)R, ldr, (const float*)P, ldp, (float*)AP, ldap, (const float*)diag, state, al);
    else bcg_update_T<double>(ctx->stream, n, nrhs, (double*)X, ldx, (double*)R, ldr, (const double*)P, ldp, (double*)AP, ldap, (const double*)diag, state, al);
    CG_CHECK_HIP(hipGetLastError());
    return COVGRAM_OK;
}

extern "C" int covgram_bcg_direction(covgram_ctx* ctx, int64_t n, int64_t nrhs, int32_t dtype, const void* R, int64_t ldr, const void* Z, int64_t ldz,
                                     void* P, int64_t ldp, double* state, int32_t* n_active, double* beta_log, int64_t it) {
    BCG_CHECK(ctx, n, nrhs, dtype, it, {ldr, ldz, ldp});
    CG_REQUIRE(R && Z && P && state && n_active, COVGRAM_EINVAL, "NULL array");
    CG_DEVICE(ctx);
    double* const bl = beta_log ? beta_log + it * nrhs : nullptr;
    if (dtype == COVGRAM_F32) bcg_direction_T<float>(ctx->stream, n, nrhs, (const float*)R, ldr, (const float*)Z, ldz, (float*)P, ldp, state, n_active, bl);
    else bcg_direction_T<double>(ctx->stream, n, nrhs, (const double*)R, ldr, (const double*)Z, ldz, (double*)P, ldp, state, n_active, bl);
    CG_CHECK_HIP(hipGetLastError());
    return COVGRAM_OK;
}
