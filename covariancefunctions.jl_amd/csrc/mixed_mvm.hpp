// mixed_mvm.hpp — the SCALAR Gramian of a Sum / Product / Power whose factors do NOT share one input trait (GenericInput in the
// reference's terms: its threaded loop src/gramian.jl:78-87 over k(x_i, y_j), trait rule src/properties.jl:47-63), e.g. EQ() + Dot(),
// EQ() * (Dot()^2 + 1), MaternP(2) + Dot()^2 + NN(): y <- alpha G a + beta y in ONE fused pass, and Matrix(G).
//
// Every entry is F(p, q, s) of p = x.y, q = |x|^2, s = |y|^2; isotropic leaves see g_f^2 |x - y|^2 with the distance formed by DIRECT
// differences of the stored coordinates (src/util.jl:40-47): a mixed kernel has no common centre to subtract and the expanded form's
// cancellation is not acceptable (grad_mixed.hpp).  Only the VALUE of each leaf is needed, so the leaves the gradient kernels refuse
// (Exponential, GammaExponential, MaternP(0), Matern(nu)) are taken.  Each factor picks its argument by its own trait:
//     isotropic       r^2 g_f^2
//     dot product     p
//     NeuralNetwork   (p + sigma) rsqrt((1 + q + sigma)(1 + s + sigma)), then (2/pi) asin            (src/mercer.jl:82-85)
//
// MI355X mapping, the shape of dense_mvm_kernel (dense_mvm.hpp):
//   lane per row (padded d <= 32): the raw x_i and q_i in VGPRs; the column stream is wave-uniform and arrives through the scalar data
//     cache; fp32 is pair-interleaved (Pk<float>: two columns per instruction).  A record per column group: (y coordinates, s_j,
//     a_j[NR]).  Per pair and dimension one subtract and two FMAs (r^2 and p).  The interpreter is factor-outer over blocks of
//     MIXV_BG column groups (parameter reads and the family branch once per block: expr_accumulate_block's form).  NR in {1, 4}
//     right-hand sides share every kernel evaluation.  Two-level accumulation (512-column inner chunks, then the split partials);
//     grid = (row blocks) x (column splits), slab [split][NR][npad], dense_reduce_kernel: fixed order, no float atomics.
//   chunked (wider d): a wave owns 64 rows and walks the columns in blocks of MIXV_CB; per block it sweeps the dimension in chunks
//     of MIXV_CH, the lane's x chunk loaded once per (block, chunk) and used against all columns of the block; r^2 and p per column
//     stay in registers; interpreter, accumulation and split as above.  Any d.
//   Matrix(G): lane per row, the columns of a 64-column strip walked inside the kernel, x_i in registers for d <= 32 and re-read in
//     chunks beyond; the same r^2, p chains and interpreter order as the product; stores coalesced along rows.
#pragma once
#include "profiles.hpp"

namespace covgram {

constexpr int MIXV_THREADS = 64;      // one wave per workgroup (no LDS, no barriers), as dense_mvm_kernel
constexpr int MIXV_INNER = 512;       // inner accumulation chunk (columns)
constexpr int MIXV_BG = 4;            // column groups per interpreter block, lane-per-row route
constexpr int MIXV_CB = 8;            // columns per block, chunked route
constexpr int MIXV_CH = 16;           // dimensions per chunk, chunked route

__host__ __device__ constexpr bool mixv_dot_family(int fam) { return fam == COVGRAM_DOT || fam == COVGRAM_EXPDOT || fam == COVGRAM_ASINDOT; }

// ---- the interpreter --------------------------------------------------------------------------------------------------------------------
// one pair (Matrix(G)): sum over the terms of coef_t prod_f phi_f(argument of f's own trait)^power_f
template <typename T>
__device__ __forceinline__ T mixed_value(const ExprParams<T>& ep, T r2, T p, T q, T s) {
    T total = (T)0;
    int fi = 0;
    for (int t = 0; t < ep.nterms; ++t) {
        T prod = ep.coef[t];
        for (int f = 0; f < ep.nfac[t]; ++f, ++fi) {
            const KParams<T>& kq = ep.f[fi];
            const int fam = ep.fam[fi];
            if (fam == COVGRAM_NEURALNETWORK) {
                const T sg = kq.param;
                const T u = (p + sg) * cg_rsqrt(((T)1 + q + sg) * ((T)1 + s + sg));
                prod *= phi_any<T>(COVGRAM_ASINDOT, u, kq);
            } else {
                prod *= phi_any<T>(fam, mixv_dot_family(fam) ? p : r2 * kq.gamma2, kq);
            }
        }
        total += prod;
    }
    return total;
}

// BG column groups at once, factor-outer: the factor's parameters are read and its family dispatched once per block; each finished
// term goes into the NR accumulators, acc[c] += wts[g * wstride + c] * term[g]
template <typename T, int BG, int NR>
__device__ __forceinline__ void mixed_accumulate_block(const typename Pk<T>::V (&r2)[BG], const typename Pk<T>::V (&p)[BG], T q,
                                                       const typename Pk<T>::V (&s)[BG], const ExprParams<T>& ep,
                                                       const typename Pk<T>::V* __restrict__ wts, int wstride, typename Pk<T>::V (&acc)[NR]) {
    using PK = Pk<T>;
    using V = typename PK::V;
    int fi = 0;
    for (int t = 0; t < ep.nterms; ++t) {
        V prod[BG];
        const V coef = PK::splat(ep.coef[t]);
#pragma unroll
        for (int g = 0; g < BG; ++g) prod[g] = coef;
        for (int f = 0; f < ep.nfac[t]; ++f, ++fi) {
            const KParams<T>& kq = ep.f[fi];
            const int pw = kq.power;
            int fam = ep.fam[fi];
            V arg[BG];
            if (fam == COVGRAM_NEURALNETWORK) {
                const T sg = kq.param;
                const V A = PK::splat((T)1 + q + sg), one = PK::splat((T)1 + sg), sgv = PK::splat(sg);
#pragma unroll
                for (int g = 0; g < BG; ++g) arg[g] = (p[g] + sgv) * PK::map(A * (one + s[g]), [](T v) { return cg_rsqrt(v); });
                fam = COVGRAM_ASINDOT;
            } else if (mixv_dot_family(fam)) {
#pragma unroll
                for (int g = 0; g < BG; ++g) arg[g] = p[g];
            } else {
                const V g2 = PK::splat(kq.gamma2);
#pragma unroll
                for (int g = 0; g < BG; ++g) arg[g] = r2[g] * g2;
            }
#define CG_MIXV_CASE(F)                                                                                                     \
    case F:                                                                                                                 \
        if (pw == 1) {                                                                                                      \
            _Pragma("unroll") for (int g = 0; g < BG; ++g)                                                                  \
                prod[g] = prod[g] * PK::map(arg[g], [&](T sv) { return Phi<F, T, false>::eval(sv, kq); });                  \
        } else {                                                                                                            \
            _Pragma("unroll") for (int g = 0; g < BG; ++g)                                                                  \
                prod[g] = prod[g] * PK::map(arg[g], [&](T sv) { return ipow(Phi<F, T, false>::eval(sv, kq), pw); });        \
        }                                                                                                                   \
        break;
            switch (fam) {
                CG_MIXV_CASE(COVGRAM_EQ)
                CG_MIXV_CASE(COVGRAM_EXP)
                CG_MIXV_CASE(COVGRAM_RQ)
                CG_MIXV_CASE(COVGRAM_GAMMAEXP)
                CG_MIXV_CASE(COVGRAM_CAUCHY)
                CG_MIXV_CASE(COVGRAM_IMQ)
                CG_MIXV_CASE(COVGRAM_MATERNP)
                CG_MIXV_CASE(COVGRAM_MATERN)
                CG_MIXV_CASE(COVGRAM_ASINDOT)
                CG_MIXV_CASE(COVGRAM_EXPDOT)
                default:                                           // COVGRAM_DOT
                    CG_MIXV_CASE(COVGRAM_DOT)
            }
#undef CG_MIXV_CASE
        }
#pragma unroll
        for (int g = 0; g < BG; ++g)
#pragma unroll
            for (int c = 0; c < NR; ++c) acc[c] = PK::fma(wts[g * wstride + c], prod[g], acc[c]);
    }
}

// ---- lane per row -----------------------------------------------------------------------------------------------------------------------
// registers (dwords per lane): x_i; per column group of the block r^2, p, the product and the argument; NR accumulators and totals;
// beside the profile's own temporaries (the Bessel series of Matern(nu) is the widest)
template <typename T, int D, int NR>
constexpr int mixv_min_waves() {
    constexpr int w = (int)(sizeof(T) / 4), pk = sizeof(T) == 4 ? 2 : 1;
    const int state = D * w + 4 * MIXV_BG * w * pk + NR * w * (pk + 1);
    const int waves = 512 / (state + (sizeof(T) == 8 ? 176 : 72));
    return waves < 1 ? 1 : (waves > 8 ? 8 : waves);
}

// the stream of the lane-per-row route: per column group (PKN columns, interleaved) D coordinates, s_j = |y_j|^2 (an ascending-l FMA
// chain), NR weights; the columns m .. mpad - 1 repeat the last point with weight 0
template <typename T>
__global__ __launch_bounds__(256) void mixed_pack_kernel(const T* __restrict__ Y, int64_t m, int32_t d, const T* __restrict__ A, int64_t lda, int32_t nr,
                                                         T* __restrict__ P, int32_t D, int32_t NR, int32_t PKN, int64_t mpad) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= mpad) return;
    const int64_t src = j < m ? j : m - 1;
    const T* yr = Y + src * (int64_t)d;
    const int64_t g = j / PKN;
    const int h = (int)(j - g * PKN);
    T* rec = P + g * (int64_t)(D + 1 + NR) * PKN + h;
    T s = (T)0;
    for (int l = 0; l < D; ++l) {
        const T yl = l < d ? yr[l] : (T)0;
        rec[(int64_t)l * PKN] = yl;
        s = cg_fma(yl, yl, s);
    }
    rec[(int64_t)D * PKN] = s;
    for (int c = 0; c < NR; ++c) rec[(int64_t)(D + 1 + c) * PKN] = (j < m && c < nr) ? A[j + (int64_t)c * lda] : (T)0;
}

// m: the PADDED column count (a multiple of MIXV_BG column groups); jchunk a multiple of 64 columns
template <typename T, int D, int NR>
__global__ __launch_bounds__(MIXV_THREADS, (mixv_min_waves<T, D, NR>())) void mixed_lane_kernel(
    const T* __restrict__ X, int64_t n, int32_t d, const typename Pk<T>::V* __restrict__ P, int64_t m, T* __restrict__ out, int64_t npad, int64_t ldy,
    int32_t nrhs, int64_t jchunk, T alpha, T beta, int32_t final_store, const ExprParams<T> ep) {
    using PK = Pk<T>;
    using V = typename PK::V;
    constexpr int S = D + 1 + NR;                            // stream elements per column group
    constexpr int DC = 64 / (int)sizeof(V);                  // dimensions per 64-byte scalar load
    constexpr int GINNER = MIXV_INNER / PK::N;
    int64_t row = (int64_t)blockIdx.x * MIXV_THREADS + threadIdx.x;
    const bool live = row < n;
    if (!live) row = n - 1;                                  // clamp: computed but never stored
    const int64_t j0 = (int64_t)blockIdx.y * jchunk;
    const int64_t j1 = (j0 + jchunk < m) ? (j0 + jchunk) : m;
    const int64_t g0 = j0 / PK::N, g1 = j1 / PK::N;

    T x[D];
    T q = (T)0;
    {
        const T* xr = X + row * (int64_t)d;
#pragma unroll
        for (int l = 0; l < D; ++l) {
            x[l] = (l < d) ? xr[l] : (T)0;
            q = cg_fma(x[l], x[l], q);
        }
    }
    T tot[NR];
#pragma unroll
    for (int c = 0; c < NR; ++c) tot[c] = (T)0;

    for (int64_t gb = g0; gb < g1; gb += GINNER) {
        const int cnt = (int)(((gb + GINNER < g1) ? (gb + GINNER) : g1) - gb);
        V acc[NR];
#pragma unroll
        for (int c = 0; c < NR; ++c) acc[c] = PK::splat((T)0);
        const V* __restrict__ p = P + gb * S;                // uniform address: the records arrive as scalar operands
        for (int g = 0; g < cnt; g += MIXV_BG, p += MIXV_BG * S) {
            V r2[MIXV_BG], pp[MIXV_BG], sv[MIXV_BG];
#pragma unroll
            for (int u = 0; u < MIXV_BG; ++u) {
                const V* __restrict__ rec = p + u * S;
                V ru = PK::splat((T)0), pu = PK::splat((T)0);
#pragma unroll
                for (int c0 = 0; c0 < D; c0 += DC) {
#pragma unroll
                    for (int l = c0; l < ((c0 + DC < D) ? c0 + DC : D); ++l) {
                        const V yl = rec[l];
                        const V xl = PK::splat(x[l]);
                        const V dl = xl - yl;
                        ru = PK::fma(dl, dl, ru);
                        pu = PK::fma(xl, yl, pu);
                    }
                    if constexpr (D > DC) __builtin_amdgcn_sched_barrier(0);
                }
                r2[u] = ru; pp[u] = pu; sv[u] = rec[D];
            }
            mixed_accumulate_block<T, MIXV_BG, NR>(r2, pp, q, sv, ep, p + D + 1, S, acc);
        }
#pragma unroll
        for (int c = 0; c < NR; ++c) tot[c] += PK::hsum(acc[c]);
    }

    if (!live) return;
    if (final_store) {                                       // one split: alpha / beta here (beta == 0 never reads y)
#pragma unroll
        for (int c = 0; c < NR; ++c) {
            if (c < nrhs) {
                T* yp = out + row + (int64_t)c * ldy;
                T v = alpha * tot[c];
                if (beta != (T)0) v = cg_fma(beta, *yp, v);
                *yp = v;
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < NR; ++c) out[((int64_t)blockIdx.y * NR + c) * npad + row] = tot[c];
    }
}

// ---- chunked route ----------------------------------------------------------------------------------------------------------------------
// the stream: per block of MIXV_CB columns (BGW = MIXV_CB / PKN column groups), nch chunks of [BGW][MIXV_CH] coordinates, then s[BGW] and
// a[BGW][NR]; the columns m .. mpad - 1 repeat the last point with weight 0
template <typename T>
__global__ __launch_bounds__(256) void mixed_chunk_pack_kernel(const T* __restrict__ Y, int64_t m, int32_t d, int32_t nch, const T* __restrict__ A, int64_t lda,
                                                               int32_t nr, T* __restrict__ P, int32_t NR, int32_t PKN, int64_t mpad) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= mpad) return;
    const int64_t src = j < m ? j : m - 1;
    const T* yr = Y + src * (int64_t)d;
    const int BGW = MIXV_CB / PKN;
    const int64_t b = j / MIXV_CB;
    const int within = (int)(j - b * MIXV_CB);
    const int g = within / PKN, h = within - g * PKN;
    T* base = P + b * ((int64_t)nch * BGW * MIXV_CH + (int64_t)BGW * (1 + NR)) * PKN;
    T s = (T)0;
    for (int l = 0; l < nch * MIXV_CH; ++l) {
        const T yl = l < d ? yr[l] : (T)0;
        const int ch = l / MIXV_CH, ll = l - ch * MIXV_CH;
        base[((int64_t)(ch * BGW + g) * MIXV_CH + ll) * PKN + h] = yl;
        s = cg_fma(yl, yl, s);
    }
    T* tail = base + (int64_t)nch * BGW * MIXV_CH * PKN;
    tail[g * PKN + h] = s;
    for (int c = 0; c < NR; ++c) tail[(BGW + g * NR + c) * PKN + h] = (j < m && c < nr) ? A[j + (int64_t)c * lda] : (T)0;
}

template <typename T, int NR>
constexpr int mixv_chunk_min_waves() {
    constexpr int w = (int)(sizeof(T) / 4);
    const int state = MIXV_CH * w + 4 * MIXV_CB * w + 3 * NR * w;
    const int waves = 512 / (state + (sizeof(T) == 8 ? 176 : 72));
    return waves < 1 ? 1 : (waves > 8 ? 8 : waves);
}

// m: the PADDED column count (a multiple of MIXV_CB); jchunk a multiple of 64 columns
template <typename T, int NR>
__global__ __launch_bounds__(MIXV_THREADS, (mixv_chunk_min_waves<T, NR>())) void mixed_chunk_kernel(
    const T* __restrict__ X, int64_t n, int32_t d, int32_t nch, const typename Pk<T>::V* __restrict__ P, int64_t m, T* __restrict__ out, int64_t npad,
    int64_t ldy, int32_t nrhs, int64_t jchunk, T alpha, T beta, int32_t final_store, const ExprParams<T> ep) {
    using PK = Pk<T>;
    using V = typename PK::V;
    constexpr int BGW = MIXV_CB / PK::N;
    constexpr int BINNER = MIXV_INNER / MIXV_CB;
    int64_t row = (int64_t)blockIdx.x * MIXV_THREADS + threadIdx.x;
    const bool live = row < n;
    if (!live) row = n - 1;
    const T* __restrict__ xr = X + row * (int64_t)d;
    const int64_t j0 = (int64_t)blockIdx.y * jchunk;
    const int64_t j1 = (j0 + jchunk < m) ? (j0 + jchunk) : m;
    const int64_t b0 = j0 / MIXV_CB, b1 = j1 / MIXV_CB;
    const int64_t bstride = (int64_t)nch * BGW * MIXV_CH + BGW * (1 + NR);

    T q = (T)0;
    for (int l = 0; l < d; ++l) q = cg_fma(xr[l], xr[l], q);
    T tot[NR];
#pragma unroll
    for (int c = 0; c < NR; ++c) tot[c] = (T)0;

    for (int64_t bb = b0; bb < b1; bb += BINNER) {
        const int64_t be = (bb + BINNER < b1) ? (bb + BINNER) : b1;
        V acc[NR];
#pragma unroll
        for (int c = 0; c < NR; ++c) acc[c] = PK::splat((T)0);
        for (int64_t b = bb; b < be; ++b) {
            const V* __restrict__ pb = P + b * bstride;      // uniform address
            V r2[BGW], pp[BGW], sv[BGW];
#pragma unroll
            for (int g = 0; g < BGW; ++g) { r2[g] = PK::splat((T)0); pp[g] = PK::splat((T)0); }
            for (int ch = 0; ch < nch; ++ch) {
                T x[MIXV_CH];
                const int l0 = ch * MIXV_CH;
#pragma unroll
                for (int l = 0; l < MIXV_CH; ++l) x[l] = (l0 + l < d) ? xr[l0 + l] : (T)0;
                const V* __restrict__ py = pb + (int64_t)ch * BGW * MIXV_CH;
#pragma unroll
                for (int g = 0; g < BGW; ++g) {
                    V rg = r2[g], pg = pp[g];
#pragma unroll
                    for (int l = 0; l < MIXV_CH; ++l) {
                        const V yl = py[g * MIXV_CH + l];
                        const V xl = PK::splat(x[l]);
                        const V dl = xl - yl;
                        rg = PK::fma(dl, dl, rg);
                        pg = PK::fma(xl, yl, pg);
                    }
                    r2[g] = rg; pp[g] = pg;
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            const V* __restrict__ tail = pb + (int64_t)nch * BGW * MIXV_CH;
#pragma unroll
            for (int g = 0; g < BGW; ++g) sv[g] = tail[g];
            mixed_accumulate_block<T, BGW, NR>(r2, pp, q, sv, ep, tail + BGW, NR, acc);
        }
#pragma unroll
        for (int c = 0; c < NR; ++c) tot[c] += PK::hsum(acc[c]);
    }

    if (!live) return;
    if (final_store) {
#pragma unroll
        for (int c = 0; c < NR; ++c) {
            if (c < nrhs) {
                T* yp = out + row + (int64_t)c * ldy;
                T v = alpha * tot[c];
                if (beta != (T)0) v = cg_fma(beta, *yp, v);
                *yp = v;
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < NR; ++c) out[((int64_t)blockIdx.y * NR + c) * npad + row] = tot[c];
    }
}

// ---- Matrix(G) --------------------------------------------------------------------------------------------------------------------------
// grid = (row blocks of 256, strips of 64 columns — several per workgroup beyond the grid's y extent); D > 0: x_i in registers
// (d <= D), D = 0: x_i re-read in chunks of MIXV_CH against MIXV_CB columns at a time.  Only rows i < n of each column are written.
template <typename T, int D>
__global__ __launch_bounds__(256) void mixed_matrix_kernel(const T* __restrict__ X, int64_t n, const T* __restrict__ Y, int64_t m, int32_t d,
                                                           T* __restrict__ out, int64_t ldo, T scale, const ExprParams<T> ep) {
    int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = row < n;
    if (!live) row = n - 1;
    const T* __restrict__ xr = X + row * (int64_t)d;
    const int64_t nstrips = (m + 63) / 64;
    if constexpr (D > 0) {
        T x[D];
        T q = (T)0;
#pragma unroll
        for (int l = 0; l < D; ++l) {
            x[l] = (l < d) ? xr[l] : (T)0;
            q = cg_fma(x[l], x[l], q);
        }
        for (int64_t st = blockIdx.y; st < nstrips; st += gridDim.y) {
            const int64_t je = (st * 64 + 64 < m) ? (st * 64 + 64) : m;
            for (int64_t j = st * 64; j < je; ++j) {
                const T* __restrict__ yr = Y + j * (int64_t)d;   // uniform address
                T r2 = (T)0, p = (T)0, s = (T)0;
#pragma unroll
                for (int l = 0; l < D; ++l) {
                    const T yl = (l < d) ? yr[l] : (T)0;
                    const T dl = x[l] - yl;
                    r2 = cg_fma(dl, dl, r2);
                    p = cg_fma(x[l], yl, p);
                    s = cg_fma(yl, yl, s);
                }
                const T v = scale * mixed_value<T>(ep, r2, p, q, s);
                if (live) out[row + j * ldo] = v;
            }
        }
    } else {
        T q = (T)0;
        for (int l = 0; l < d; ++l) q = cg_fma(xr[l], xr[l], q);
        const int nch = (d + MIXV_CH - 1) / MIXV_CH;
        for (int64_t st = blockIdx.y; st < nstrips; st += gridDim.y) {
            const int64_t je = (st * 64 + 64 < m) ? (st * 64 + 64) : m;
            for (int64_t jb = st * 64; jb < je; jb += MIXV_CB) {
                T r2[MIXV_CB], p[MIXV_CB], s[MIXV_CB];
#pragma unroll
                for (int c = 0; c < MIXV_CB; ++c) { r2[c] = (T)0; p[c] = (T)0; s[c] = (T)0; }
                for (int ch = 0; ch < nch; ++ch) {
                    T x[MIXV_CH];
                    const int l0 = ch * MIXV_CH;
#pragma unroll
                    for (int l = 0; l < MIXV_CH; ++l) x[l] = (l0 + l < d) ? xr[l0 + l] : (T)0;
#pragma unroll
                    for (int c = 0; c < MIXV_CB; ++c) {
                        const int64_t j = (jb + c < je) ? (jb + c) : (je - 1);
                        const T* __restrict__ yr = Y + j * (int64_t)d + l0;   // uniform address
#pragma unroll
                        for (int l = 0; l < MIXV_CH; ++l) {
                            const T yl = (l0 + l < d) ? yr[l] : (T)0;
                            const T dl = x[l] - yl;
                            r2[c] = cg_fma(dl, dl, r2[c]);
                            p[c] = cg_fma(x[l], yl, p[c]);
                            s[c] = cg_fma(yl, yl, s[c]);
                        }
                    }
                }
                // ONE copy of the interpreter: the column's scalars picked by a uniform index (the arrays are never indexed dynamically)
#pragma unroll 1
                for (int c = 0; c < MIXV_CB; ++c) {
                    T r2c = r2[0], pc = p[0], sc = s[0];
#pragma unroll
                    for (int e = 1; e < MIXV_CB; ++e)
                        if (c == e) { r2c = r2[e]; pc = p[e]; sc = s[e]; }
                    const T v = scale * mixed_value<T>(ep, r2c, pc, q, sc);
                    if (live && jb + c < je) out[row + (jb + c) * ldo] = v;
                }
            }
        }
    }
}

}  // namespace covgram
