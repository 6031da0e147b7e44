// sm_grad.hip — hyper-parameter gradients of the bilinear forms sum_t u_t' G a_t of a SpectralMixture Gramian in ONE pass over the n m
// pairs.  With W = U A' (rank nvec, formed per pair in registers, never stored), r = x_i - y_j by direct differences,
// phi_q = 2 pi mu_q . r and e_q = exp(-1/2 sum_k (r_k inv_l_qk)^2), per component q:
//     out[q (1 + 2 d)]             = sum_ij W_ij cos phi_q e_q                      dF/dw_q (not multiplied by w_q)
//     out[q (1 + 2 d) + 1 + k]     = sum_ij W_ij (-2 pi w_q) r_k sin phi_q e_q      dF/dmu_qk
//     out[q (1 + 2 d) + 1 + d + k] = sum_ij W_ij w_q cos phi_q e_q r_k^2            E_qk: dF/d(inv_l_qk^2) = -1/2 E_qk
// fp32 and fp64; the results are always fp64.
//
// Shape of the computation:
//   * sm_phase_kernel (sm_common.hpp) once per point set: (cos, sin) of 2 pi mu_q . x_i and of 2 pi mu_q . y_j, phases reduced in fp64.  Both
//     sides are kept unweighted: cos phi = cu cv + su sv, sin phi = su cv - cu sv, and the factors w_q and -2 pi w_q multiply the finished
//     fp64 sums in smg_reduce_kernel.  The pair loop has no trigonometric instruction;
//   * the tiling of bilin_grad.hip: a workgroup (4 waves) owns BG_TI = 64 rows and a chunk of column tiles, lane r of every wave is row r,
//     wave w takes a quarter of each tile's columns (JPL = 16 pairs per lane and tile in fp32, 8 in fp64).  The row's point is in registers;
//     LDS: the row tile's weights (staged once), the column tile's points, weights and the phase factors and exponent coefficients of the
//     current component chunk.  A lane works on 4 (fp32) or 2 (fp64) pairs at a time: W_ij as nvec fmas, the exponents by direct
//     differences, exp2, then W e cos phi and W e sin phi per component, which multiply r_k^2 and r_k into the per-dimension sums;
//   * the accumulators are bounded whatever Q and d are: the components are walked in chunks of smg_qc = 4 (fp32) or 2 (fp64), the chunk
//     loop OUTSIDE the column loop (a mixture that fits one chunk — the shapes the family is used at — is one pass, compiled for its own
//     count QN); the dimensions in chunks of four within a pass that serves at most 8 of them (d = 16: two passes per component chunk).  A
//     lane holds 2 min(DM, 8) QN <= 64 per-dimension sums and QN sums of W e cos phi;
//   * reduction: a lane adds at most BG_L = 128 pairs in the working precision.  Then its <= 64 sums are added over the 64 lanes by a
//     butterfly that halves the number of values a lane holds at every step (wave_fold: N - 1 exchanges instead of 6 per value; each
//     value still passes through exactly 6 additions) and lane l adds the one value it ends with to an fp64 total; the QN sums of
//     W e cos phi take the plain butterfly.  At the end of a pass the four waves' fp64 totals are added in wave order and written to a
//     slab; smg_reduce_kernel adds the slab in a fixed order.  No atomics: bit-identical from run to run;
//   * a pair with r = 0 adds exactly W_ij to the first output of each component (cos phi is replaced by 1 there, e_q = exp2(-0) = 1) and
//     exactly 0 to the others (r_k = 0).  Rows and columns beyond the sets have zero weights and finite points: they add exactly 0.
#include "bilin_common.hpp"
#include "sm_common.hpp"

namespace covgram {

template <typename T>
struct SmgArgs {
    const T* X; const T* Y;          // points, point-major, stride d
    int64_t n, m;
    int32_t d, ncomp, nch, nout;     // nout = ncomp (1 + 2 d)
    const T* U; int64_t ldu;         // n x nvec
    const T* A; int64_t lda;         // m x nvec
    int32_t nvec;
    const T* RX;                     // row phases    [nch][2 SM_QC][n]: cos then sin of the chunk's components
    const T* RY;                     // column phases [nch][2 SM_QC][m]
    const T* coef;                   // [nch SM_QC][SM_CST]: log2(e) / (2 l_qk^2), zero beyond d and beyond ncomp
    double* slab;                    // [gridDim.y][gridDim.x][nout]
    int64_t jchunk;                  // columns per blockIdx.y (a multiple of the tile width)
};

constexpr int smg_pow2(int v) { int p = 1; while (p < v) p *= 2; return p; }
constexpr int smg_log2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// Sum over the 64 lanes of each of the N = 2^k <= 64 values a lane holds: at every step a lane keeps one half of its values and sends
// the other half to the lane it is paired with, so that after k steps one value is left, which takes the remaining 6 - k plain
// butterfly steps.  Lane l ends with the sum of value (l >> (6 - k)) & (N - 1) in v[0].
template <typename T, int H, int N>
__device__ __forceinline__ void wave_fold_step(T (&v)[N], int lane, int o) {
    if constexpr (H >= 1) {
        const bool up = (lane & o) != 0;
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const T keep = up ? v[i + H] : v[i];
            const T send = up ? v[i] : v[i + H];
            v[i] = keep + __shfl_xor(send, o, 64);
        }
        wave_fold_step<T, H / 2, N>(v, lane, o >> 1);
    } else {
        for (; o >= 1; o >>= 1) v[0] += __shfl_xor(v[0], o, 64);
    }
}
template <typename T, int N>
__device__ __forceinline__ void wave_fold(T (&v)[N], int lane) { wave_fold_step<T, N / 2, N>(v, lane, 32); }

template <typename T>
__device__ __forceinline__ T smg_wave_sum(T x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// components per chunk of the gradient pass: the 2 DMC QN sums a lane holds are at most 64 registers in fp32 and, with half the components, 128 in fp64
template <typename T> constexpr int smg_qc = sizeof(T) == 4 ? SM_QC : SM_QC / 2;
// pairs a lane works on at a time: one 128-bit broadcast read of their weights per column of A
template <typename T> constexpr int smg_pg = sizeof(T) == 4 ? 4 : 2;
constexpr int SMG_DC = 8;        // dimensions per pass over the pairs

// DM: the dimensions, padded to 4, 8 or 16; QN: components evaluated per chunk — the mixture's own count when it has at most smg_qc<T>,
// otherwise smg_qc<T> (the last chunk's padding has zero phase factors and zero coefficients; its sums are not stored).  A pass over the
// column chunk serves one chunk of components and DMC = min(DM, 8) dimensions: d = 16 takes two passes per chunk, the second without the
// dF/dw sums.
template <typename T, int DM, int QN>
__global__ __launch_bounds__(BG_TI * BG_WAVES) __attribute__((amdgpu_waves_per_eu(2))) void smg_pair_kernel(const SmgArgs<T> g) {
    constexpr int JPL = bg_jpl<T>, TJ = JPL * BG_WAVES, KT = BG_L / JPL, QG = smg_qc<T>, SMG_PG = smg_pg<T>;
    constexpr int DMC = DM < SMG_DC ? DM : SMG_DC, NDP = DM / DMC;
    constexpr int NV = 2 * DMC * QN, NP = smg_pow2(NV);          // sums a lane holds; padded to a power of two for the fold
    constexpr int FOLD_SHIFT = 6 - smg_log2(NP);
    constexpr int NRED = NP + QN;
    static_assert(JPL % SMG_PG == 0 && BG_L % JPL == 0 && NP <= 64, "whole pair groups per tile; whole tiles per hand-off; one value per lane after the fold");
    extern __shared__ __align__(32) unsigned char smg_lds[];
    __shared__ double red[BG_WAVES][NRED];
    using V4 = T __attribute__((ext_vector_type(4)));
    T* ys = (T*)smg_lds;                                           // [TJ][DM]
    T* cs = ys + TJ * DM;                                          // [2 QN][TJ]: cos then sin of the chunk's components
    T* cfs = cs + 2 * QN * TJ;                                     // [QN][DM]: the chunk's coefficients
    T* us = cfs + QN * DM;                                         // [nvec][BG_TI]
    T* as = us + g.nvec * BG_TI;                                   // [nvec][TJ]
    const int tid = threadIdx.x, r = tid & 63, wv = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * BG_TI;
    const int64_t j0 = (int64_t)blockIdx.y * g.jchunk;
    const int64_t j1 = j0 + g.jchunk < g.m ? j0 + g.jchunk : g.m;
    const int64_t ic = i0 + r < g.n ? i0 + r : g.n - 1;
    double* __restrict__ slab = g.slab + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * g.nout;

    // the row tile: weights of rows beyond the set are zeros (their points are those of the last row: finite)
    for (int e = tid; e < g.nvec * BG_TI; e += BG_TI * BG_WAVES) {
        const int vv = e / BG_TI, rr = e % BG_TI;
        us[e] = i0 + rr < g.n ? g.U[(i0 + rr) + (int64_t)vv * g.ldu] : (T)0;
    }
    T x[DMC], xh[DMC];                                             // dimensions 0 .. DMC - 1 and, for d = 16, DMC .. 2 DMC - 1
#pragma unroll
    for (int k = 0; k < DMC; ++k) {
        x[k] = k < g.d ? g.X[ic * g.d + k] : (T)0;
        xh[k] = (NDP == 2 && DMC + k < g.d) ? g.X[ic * g.d + DMC + k] : (T)0;
    }

    const int nchunk = (g.ncomp + QG - 1) / QG;
    for (int pass = 0; pass < nchunk * NDP; ++pass) {
        const int c = pass / NDP, dp = pass % NDP;                 // component chunk, dimension pass
        T cu[QN], su[QN];
        int slot[QN];                                              // of the component's cosine in the phase tables; its sine: + SM_QC
#pragma unroll
        for (int q = 0; q < QN; ++q) {
            const int qg = c * QG + q;
            slot[q] = (qg / SM_QC) * 2 * SM_QC + qg % SM_QC;
            cu[q] = g.RX[(int64_t)slot[q] * g.n + ic];
            su[q] = g.RX[(int64_t)(slot[q] + SM_QC) * g.n + ic];
        }
        __syncthreads();                                           // the previous pass has read cfs and red
        for (int e = tid; e < QN * DM; e += BG_TI * BG_WAVES) cfs[e] = g.coef[(c * QG + e / DM) * SM_CST + e % DM];
        double totd = 0.0, totw = 0.0;                             // lane l: sum l >> FOLD_SHIFT of v; lane q: sum W e cos phi of component q
        T v[NP], accw[QN];
#pragma unroll
        for (int e = 0; e < NP; ++e) v[e] = (T)0;
#pragma unroll
        for (int q = 0; q < QN; ++q) accw[q] = (T)0;
        T xp[DMC];                                                 // the pass's dimensions of the row
#pragma unroll
        for (int k = 0; k < DMC; ++k) xp[k] = (NDP == 2 && dp) ? xh[k] : x[k];
        int held = 0;                                              // tiles in v and accw

        for (int64_t jt = j0; jt < j1; jt += TJ) {
            __syncthreads();                                       // the previous tile has been consumed
            for (int e = tid; e < g.nvec * TJ; e += BG_TI * BG_WAVES) {
                const int vv = e / TJ, jj = e % TJ;
                as[e] = jt + jj < j1 ? g.A[(jt + jj) + (int64_t)vv * g.lda] : (T)0;
            }
            for (int e = tid; e < TJ * DM; e += BG_TI * BG_WAVES) {
                const int jj = e / DM, k = e % DM;
                ys[e] = (jt + jj < j1 && k < g.d) ? g.Y[(jt + jj) * g.d + k] : (T)0;
            }
            for (int e = tid; e < 2 * QN * TJ; e += BG_TI * BG_WAVES) {
                const int f = e / TJ, jj = e % TJ;                 // f < QN: cos of component f; otherwise sin of component f - QN
                const int qg = c * QG + (f < QN ? f : f - QN);
                const int sl = (qg / SM_QC) * 2 * SM_QC + qg % SM_QC + (f < QN ? 0 : SM_QC);
                cs[e] = jt + jj < j1 ? g.RY[(int64_t)sl * g.m + jt + jj] : (T)0;
            }
            __syncthreads();
#pragma unroll 1
            for (int jg = 0; jg < JPL; jg += SMG_PG) {
                const int col = wv * JPL + jg;                     // the group's first column in the tile
                // W_ij = sum_v u_iv a_jv, v ascending
                using VP = T __attribute__((ext_vector_type(SMG_PG)));
                T w[SMG_PG];
#pragma unroll
                for (int p = 0; p < SMG_PG; ++p) w[p] = (T)0;
                for (int vv = 0; vv < g.nvec; ++vv) {
                    const T uv = us[vv * BG_TI + r];
                    const VP av = *(const VP*)(as + vv * TJ + col);
#pragma unroll
                    for (int p = 0; p < SMG_PG; ++p) w[p] = fma_t(uv, av[p], w[p]);
                }
                // the exponents t_q = sum_k c_qk r_k^2 (in gc) and |r|^2 (only its being zero is used), dimensions ascending
                T gc[SMG_PG][QN], gs[SMG_PG][QN], s[SMG_PG];
#pragma unroll
                for (int p = 0; p < SMG_PG; ++p) {
                    s[p] = (T)0;
#pragma unroll
                    for (int q = 0; q < QN; ++q) gc[p][q] = (T)0;
                }
#pragma unroll
                for (int kc = 0; kc < DM / 4; ++kc) {
                    V4 cf[QN];
#pragma unroll
                    for (int q = 0; q < QN; ++q) cf[q] = *(const V4*)(cfs + q * DM + 4 * kc);
#pragma unroll
                    for (int p = 0; p < SMG_PG; ++p) {
                        const V4 yv = *(const V4*)(ys + (col + p) * DM + 4 * kc);
                        const T* xk = 4 * kc < DMC ? x + 4 * kc : xh + (4 * kc - DMC);
                        const T dx = xk[0] - yv.x, dy = xk[1] - yv.y, dz = xk[2] - yv.z, dw = xk[3] - yv.w;
                        const T d2x = dx * dx, d2y = dy * dy, d2z = dz * dz, d2w = dw * dw;
                        s[p] += (d2x + d2y) + (d2z + d2w);
#pragma unroll
                        for (int q = 0; q < QN; ++q) gc[p][q] = fma_t(cf[q].w, d2w, fma_t(cf[q].z, d2z, fma_t(cf[q].y, d2y, fma_t(cf[q].x, d2x, gc[p][q]))));
                    }
                }
                // per pair and component: W e cos phi (kept in gc) and W e sin phi
#pragma unroll
                for (int p = 0; p < SMG_PG; ++p) {
                    const bool zero = s[p] == (T)0;
#pragma unroll
                    for (int q = 0; q < QN; ++q) {
                        const T cv = cs[q * TJ + col + p], sv = cs[(QN + q) * TJ + col + p];
                        const T we = w[p] * exp2_neg_tab(gc[p][q]);
                        const T cosv = zero ? (T)1 : fma_t(cu[q], cv, su[q] * sv);
                        const T sinv = fma_t(su[q], cv, -(cu[q] * sv));
                        gc[p][q] = we * cosv;
                        gs[p][q] = we * sinv;
                        if (dp == 0) accw[q] += gc[p][q];
                    }
                }
                // the pass's dimensions: sum (W e sin phi) r_k and sum (W e cos phi) r_k^2
#pragma unroll
                for (int kc = 0; kc < DMC / 4; ++kc) {
#pragma unroll
                    for (int p = 0; p < SMG_PG; ++p) {
                        const int k0 = NDP == 1 ? 4 * kc : 4 * kc + dp * DMC;
                        const V4 yv = *(const V4*)(ys + (col + p) * DM + k0);
                        const T df[4] = {xp[4 * kc] - yv.x, xp[4 * kc + 1] - yv.y, xp[4 * kc + 2] - yv.z, xp[4 * kc + 3] - yv.w};
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const T d2 = df[t] * df[t];
#pragma unroll
                            for (int q = 0; q < QN; ++q) {
                                v[q * 2 * DMC + 4 * kc + t] = fma_t(gs[p][q], df[t], v[q * 2 * DMC + 4 * kc + t]);
                                v[q * 2 * DMC + DMC + 4 * kc + t] = fma_t(gc[p][q], d2, v[q * 2 * DMC + DMC + 4 * kc + t]);
                            }
                        }
                    }
                }
            }
            if (++held == KT || jt + TJ >= j1) {                   // hand-off: at most BG_L pairs per lane
                wave_fold<T, NP>(v, r);
                totd += (double)v[0];
#pragma unroll
                for (int e = 0; e < NP; ++e) v[e] = (T)0;
#pragma unroll
                for (int q = 0; q < QN; ++q) {
                    const T sum = smg_wave_sum(accw[q]);
                    if (r == q) totw += (double)sum;
                    accw[q] = (T)0;
                }
                held = 0;
            }
        }
        // the pass's totals: the four waves in wave order
        if ((r & ((1 << FOLD_SHIFT) - 1)) == 0) red[wv][r >> FOLD_SHIFT] = totd;
        if (r < QN) red[wv][NP + r] = totw;
        __syncthreads();
        if (tid < NRED) {
            double t = red[0][tid];
#pragma unroll
            for (int q = 1; q < BG_WAVES; ++q) t += red[q][tid];
            int q, k, off;                                         // component of the chunk, dimension, offset of the output in the component's block
            if (tid >= NP) { q = tid - NP; k = dp == 0 ? 0 : g.d; off = 0; }   // (k = d: not stored by the second dimension pass)
            else {
                q = tid / (2 * DMC);
                const int e = tid % (2 * DMC);
                k = dp * DMC + e % DMC;
                off = 1 + k + (e >= DMC ? g.d : 0);
            }
            const int qg = c * QG + q;
            if (q < QN && qg < g.ncomp && k < g.d) slab[qg * (1 + 2 * g.d) + off] = t;
        }
    }
}

// out[k] <- factor_k sum over the slab's nblk rows: 256 strided partial sums per output, then a tree in LDS — a fixed order.
// factor: 1 for dF/dw_q, -2 pi w_q for dF/dmu_qk, w_q for E_qk
template <typename T>
__global__ __launch_bounds__(256) void smg_reduce_kernel(const double* __restrict__ slab, int64_t nblk, int nout, int d, const T* __restrict__ w,
                                                         double* __restrict__ out) {
    __shared__ double part[256];
    const int k = blockIdx.x, t = threadIdx.x;
    double sum = 0.0;
    for (int64_t b = t; b < nblk; b += 256) sum += slab[b * nout + k];
    part[t] = sum;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) part[t] += part[t + h];
        __syncthreads();
    }
    if (t == 0) {
        const int q = k / (1 + 2 * d), off = k % (1 + 2 * d);
        const double wq = (double)w[q];
        const double f = off == 0 ? 1.0 : (off <= d ? -6.283185307179586476925 * wq : wq);
        out[k] = f * part[0];
    }
}

template <typename T, int QN>
static void smg_launch_q(int dm, dim3 grid, size_t lds_tail, hipStream_t stream, const SmgArgs<T>& g) {
    constexpr int TJ = bg_jpl<T> * BG_WAVES;
    auto lds = [&](int DM) { return ((size_t)TJ * DM + (size_t)2 * QN * TJ + (size_t)QN * DM) * sizeof(T) + lds_tail; };
    if (dm == 4) hipLaunchKernelGGL((smg_pair_kernel<T, 4, QN>), grid, dim3(BG_TI * BG_WAVES), lds(4), stream, g);
    else if (dm == 8) hipLaunchKernelGGL((smg_pair_kernel<T, 8, QN>), grid, dim3(BG_TI * BG_WAVES), lds(8), stream, g);
    else hipLaunchKernelGGL((smg_pair_kernel<T, 16, QN>), grid, dim3(BG_TI * BG_WAVES), lds(16), stream, g);
}

template <typename T>
static int smg_run(covgram_sm* S, const covgram_points* X, const covgram_points* Y, const void* U, int64_t ldu, const void* A, int64_t lda, int nvec,
                   int nout, double* out_dev) {
    covgram_ctx* ctx = S->ctx;
    const int64_t n = X->n, m = Y->n;
    const int qpad = S->nch * SM_QC;
    const T* prm = (const T*)S->prm;
    // the phase tables of both point sets in workspace slot 0, both in the row layout (no weights)
    const size_t rx_bytes = (((size_t)n * 2 * qpad * sizeof(T)) + 255) & ~(size_t)255;
    void* ph;
    int rc = ws_reserve(ctx, 0, rx_bytes + (size_t)m * 2 * qpad * sizeof(T), &ph);
    if (rc) return rc;
    T* RX = (T*)ph; T* RY = (T*)((char*)ph + rx_bytes);
    SmgArgs<T> g;
    memset(&g, 0, sizeof(g));
    g.X = (const T*)X->dptr; g.Y = (const T*)Y->dptr; g.n = n; g.m = m;
    g.d = S->d; g.ncomp = S->ncomp; g.nch = S->nch; g.nout = nout;
    g.U = (const T*)U; g.ldu = ldu; g.A = (const T*)A; g.lda = lda; g.nvec = nvec;
    g.RX = RX; g.RY = RY;
    g.coef = prm + qpad + (size_t)qpad * S->d;
    constexpr int TJ = bg_jpl<T> * BG_WAVES;
    const int64_t rowtiles = (n + BG_TI - 1) / BG_TI;
    CG_REQUIRE(rowtiles <= 0x7fffffff, COVGRAM_EUNSUPPORTED, "bilinear_grad_sm: n = %lld exceeds the grid", (long long)n);
    const int64_t jsplit = bg_column_split<T>(ctx, rowtiles, m, &g.jchunk);
    const int64_t nblk = rowtiles * jsplit;
    void* slab;
    rc = ws_reserve(ctx, 1, (size_t)nblk * nout * sizeof(double), &slab);
    if (rc) return rc;
    g.slab = (double*)slab;
    const int dm = S->d <= 4 ? 4 : (S->d <= 8 ? 8 : 16);
    const size_t lds_tail = (size_t)nvec * (BG_TI + TJ) * sizeof(T);
    const dim3 grid((unsigned)rowtiles, (unsigned)jsplit);
    TimerScope tm(ctx);
    for (int side = 0; side < 2; ++side) {
        const covgram_points* P = side ? Y : X;
        const int64_t threads = P->n * qpad;
        hipLaunchKernelGGL((sm_phase_kernel<T>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)P->dptr, P->n, (const T*)nullptr,
                           (int64_t)0, (int)S->d, (int)S->ncomp, (int)S->nch, prm, prm + qpad, side ? RY : RX, (T*)nullptr);
    }
    if constexpr (sizeof(T) == 4) {                                // up to smg_qc<T> components: exactly one chunk of that many
        switch (S->ncomp) {
            case 1: smg_launch_q<T, 1>(dm, grid, lds_tail, ctx->stream, g); break;
            case 2: smg_launch_q<T, 2>(dm, grid, lds_tail, ctx->stream, g); break;
            case 3: smg_launch_q<T, 3>(dm, grid, lds_tail, ctx->stream, g); break;
            default: smg_launch_q<T, 4>(dm, grid, lds_tail, ctx->stream, g); break;
        }
    } else {
        if (S->ncomp == 1) smg_launch_q<T, 1>(dm, grid, lds_tail, ctx->stream, g);
        else smg_launch_q<T, 2>(dm, grid, lds_tail, ctx->stream, g);
    }
    hipLaunchKernelGGL((smg_reduce_kernel<T>), dim3((unsigned)nout), dim3(256), 0, ctx->stream, (const double*)slab, nblk, nout, (int)S->d, prm, out_dev);
    return COVGRAM_OK;
}

}  // namespace covgram

using namespace covgram;

extern "C" int covgram_bilinear_grad_sm(covgram_sm* S, const covgram_points* X, const covgram_points* Y, const void* U, int64_t ldu, const void* A,
                                        int64_t lda, int32_t nvec, double* out, int32_t loc) {
    CG_REQUIRE(S != nullptr, COVGRAM_EINVAL, "spectral-mixture handle is NULL");
    CG_REQUIRE(X != nullptr, COVGRAM_EINVAL, "NULL argument");
    if (!Y) Y = X;
    int rc = sm_check_points(S, X, Y);
    if (rc) return rc;
    CG_REQUIRE(loc == COVGRAM_HOST || loc == COVGRAM_DEVICE, COVGRAM_EINVAL, "unknown loc %d", loc);
    CG_REQUIRE(nvec >= 1 && nvec <= BG_MAX_NVEC, COVGRAM_EINVAL, "bilinear_grad_sm: nvec = %d is outside 1 .. %d", nvec, BG_MAX_NVEC);
    CG_REQUIRE(out != nullptr, COVGRAM_EINVAL, "out is NULL");
    const int64_t n = X->n, m = Y->n;
    CG_REQUIRE(ldu >= n && lda >= m, COVGRAM_EINVAL, "DimensionMismatch: ldu=%lld < n=%lld or lda=%lld < m=%lld", (long long)ldu, (long long)n,
               (long long)lda, (long long)m);
    CG_REQUIRE((U != nullptr || n == 0) && (A != nullptr || m == 0), COVGRAM_EINVAL, "U or A is NULL");
    covgram_ctx* ctx = S->ctx;
    const int nout = S->ncomp * (1 + 2 * S->d);
    const size_t ts = dtype_size(S->dtype);
    CG_DEVICE(ctx);
    if (n == 0 || m == 0) {                                        // an empty sum
        if (loc == COVGRAM_HOST) memset(out, 0, nout * sizeof(double));
        else CG_CHECK_HIP(hipMemsetAsync(out, 0, nout * sizeof(double), ctx->stream));
        return COVGRAM_OK;
    }
    const void* u_dev = U; const void* a_dev = A;
    double* o_dev = out;
    int64_t ldu_d = ldu, lda_d = lda;
    if (loc == COVGRAM_HOST) {
        void* so;
        rc = bg_stage_weights(ctx, n, m, nvec, ts, &u_dev, &ldu_d, &a_dev, &lda_d); if (rc) return rc;
        rc = ws_reserve(ctx, 3, (size_t)nout * sizeof(double), &so); if (rc) return rc;
        o_dev = (double*)so;
    }
    rc = by_dtype(S->dtype, [&](auto t) { return smg_run<decltype(t)>(S, X, Y, u_dev, ldu_d, a_dev, lda_d, nvec, nout, o_dev); });
    if (rc) return rc;
    CG_CHECK_HIP(hipGetLastError());
    if (loc == COVGRAM_HOST) {
        CG_CHECK_HIP(hipMemcpyAsync(out, o_dev, nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return COVGRAM_OK;
}
