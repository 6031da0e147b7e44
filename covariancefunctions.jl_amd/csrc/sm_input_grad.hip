// sm_input_grad.hip — the gradient of the bilinear forms sum_t u_t' G a_t of a SpectralMixture Gramian with respect to the ROW points in
// ONE pass over the n m pairs.  With W = U A' (rank nvec, formed per pair in registers, never stored), r = x_i - y_j by
// direct differences, phi_q = 2 pi mu_q . r and e_q = exp(-1/2 sum_k (r_k inv_l_qk)^2):
//     dX[i d + c] = sum_j W_ij sum_q w_q e_q (-2 pi mu_qc sin phi_q - inv_l_qc^2 r_c cos phi_q)
// the partial derivative of F(X, Y) = sum_ij W_ij k(x_i, y_j) in x_ic with the column side held fixed (also when Y = X: the host adds the
// call with U and A swapped; the mixture is symmetric in its arguments).  fp32 and fp64 points; the results are always fp64.
//
// Shape of the computation:
//   * sm_phase_kernel (sm_common.hpp) once per point set, both sides unweighted as in sm_grad.hip: cos phi = cu cv + su sv,
//     sin phi = su cv - cu sv.  The pair loop has no trigonometric instruction;
//   * the tiling of input_grad.hip: a workgroup (4 waves) owns BG_TI = 64 rows and a chunk of column tiles, lane r of every wave is row r,
//     wave w takes a quarter of each tile's columns (JPL = 16 pairs per lane and tile in fp32, 8 in fp64).  The row's point, its d sums in
//     the working precision and their d fp64 totals are in registers.  LDS: the row tile's weights (staged once), the column tile's
//     points, weights and phase factors.  The coefficient rows of the current component chunk — the exponent's log2(e) / (2 l_qk^2),
//     gsin_qk = -2 pi w_q mu_qk and gcos_qk = w_q inv_l_qk^2 (the handle's, each rounded once) — are wave-uniform: an isotropic handle
//     reads gsin and its two numbers per component through uniform addresses (scalar loads); with per-dimension lengthscales the three
//     tables are staged in LDS per chunk and read as 128-bit broadcasts once per group of pairs (scalar loads of that many values in
//     the pair loop share the LDS reads' wait counter: an earlier build that did so was 30-50 % slower in fp64);
//   * a lane works on 4 (fp32) or 2 (fp64) pairs at a time: W_ij as nvec fmas, the exponents by direct differences, exp2, then
//     gc_q = W e_q cos phi_q and gs_q = W e_q sin phi_q per component, and per dimension two fma chains over the chunk's components,
//     S_c = sum_q gsin_qc gs_q and C_c = sum_q gcos_qc gc_q, which join the lane's sum as acc_c += fma(-r_c, C_c, S_c).  An isotropic
//     handle (one lengthscale per component) has one exponent multiply per component and ONE chain C = sum_q gcos_q gc_q per pair: the
//     cosine half costs d fmas per pair instead of Q d;
//   * the components are walked in chunks of SM_QC = 4, the chunk loop OUTSIDE the column loop (a mixture that fits one chunk — the
//     shapes the family is used at — is one pass, compiled for its own count QN).  The sums are over the components, so the d
//     accumulators simply persist from chunk to chunk: no butterfly, no dimension passes;
//   * reduction: the row is the lane's own.  A lane adds at most BG_L = 128 pairs in the working precision, then its d sums join its fp64
//     totals.  At the end the four waves' totals of a row are added in wave order and written to the slab [jsplit][n][d];
//     smi_reduce_kernel adds the column chunks in ascending order.  No atomics: two calls agree bit for bit;
//   * a pair with sum_k r_k^2 == 0, the sum as evaluated in the points' precision (in fp32 r_k^2 underflows below |r_k| ~ 1e-23: such a
//     pair counts as coincident), adds exactly 0: cos phi is replaced by 1 and sin phi by 0 there (fma(su, cv, -(cu sv)) of identical phases is
//     not exactly 0), so gs_q = 0, S_c = 0, and C_c meets r_c = 0.  Rows and columns beyond the sets have zero weights and finite points.
#include "bilin_common.hpp"
#include "sm_common.hpp"

namespace covgram {

template <typename T>
struct SmiArgs {
    const T* X; const T* Y;          // points, point-major, stride d
    int64_t n, m;
    int32_t d, nch;
    const T* U; int64_t ldu;         // n x nvec
    const T* A; int64_t lda;         // m x nvec
    int32_t nvec;
    const T* RX;                     // row phases    [nch][2 SM_QC][n]: cos then sin of the chunk's components
    const T* RY;                     // column phases [nch][2 SM_QC][m]
    const T* coef;                   // [nch SM_QC][SM_CST]: log2(e) / (2 l_qk^2), zero beyond d and beyond ncomp
    const T* ciso;                   // [nch SM_QC]: the same for one lengthscale per component (ISO)
    const T* gsin;                   // [nch SM_QC][SM_CST]: -2 pi w_q mu_qk
    const T* gcos;                   // [nch SM_QC][SM_CST]: w_q inv_l_qk^2
    const T* gciso;                  // [nch SM_QC]: w_q inv_l_q^2 (ISO)
    double* slab;                    // [gridDim.y][n][d]
    int64_t jchunk;                  // columns per blockIdx.y (a multiple of the tile width)
};

// pairs a lane works on at a time: one 128-bit broadcast read of their weights per column of A
template <typename T> constexpr int smi_pg = sizeof(T) == 4 ? 4 : 2;

// DM: the dimensions, padded to 4, 8 or 16; QN: components evaluated per chunk — the mixture's own count when it has at most SM_QC,
// otherwise SM_QC (the last chunk's padding has zero phase factors and zero coefficients: it adds exact zeros); ISO: one lengthscale
// per component.
template <typename T, int DM, int QN, bool ISO>
__global__ __launch_bounds__(BG_TI * BG_WAVES) __attribute__((amdgpu_waves_per_eu(2))) void smi_pair_kernel(const SmiArgs<T> g) {
    constexpr int JPL = bg_jpl<T>, TJ = JPL * BG_WAVES, KT = BG_L / JPL, PG = smi_pg<T>;
    // keep the scheduler from lifting every dimension group's loads to the top of a pair group: at many dimensions times components
    // that alone exceeds the register file
    constexpr bool FENCE = DM * QN * (int)(sizeof(T) / 4) > 16;
    // fp32: v_exp_f32 flushes a denormal result, and a far row's whole sum can lie there.  The exponent's coefficients are halved where
    // they are loaded (exact: the half exponent has the bits of t / 2), h = exp2(-t / 2) stays normal down to e = 2^-252, and
    // W e = (W h) h leaves the denormal range to one product.  The price is one multiplication per pair and component and the
    // error of h twice in e (about two units of the last place of e instead of one).  fp64 is not split: ldexp produces denormals.
    constexpr bool SPLIT = sizeof(T) == 4;
    constexpr T EH = SPLIT ? (T)0.5 : (T)1;
    static_assert(JPL % PG == 0 && BG_L % JPL == 0 && DM % 4 == 0, "whole pair groups per tile; whole tiles per hand-off; 128-bit rows");
    extern __shared__ __align__(32) unsigned char smi_lds[];
    __shared__ double red[DM][BG_TI];
    __shared__ __align__(32) T cfl[ISO ? 1 : 3][SM_QC][SM_CST];    // per-dimension lengthscales: the chunk's three coefficient tables
    using V4 = T __attribute__((ext_vector_type(4)));
    using VP = T __attribute__((ext_vector_type(PG)));
    T* ys = (T*)smi_lds;                                           // [TJ][DM]
    T* cs = ys + TJ * DM;                                          // [2 QN][TJ]: cos then sin of the chunk's components
    T* us = cs + 2 * QN * TJ;                                      // [nvec][BG_TI]
    T* as = us + g.nvec * BG_TI;                                   // [nvec][TJ]
    const int tid = threadIdx.x, r = tid & 63, wv = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * BG_TI;
    const int64_t j0 = (int64_t)blockIdx.y * g.jchunk;
    const int64_t j1 = j0 + g.jchunk < g.m ? j0 + g.jchunk : g.m;
    const int64_t ic = i0 + r < g.n ? i0 + r : g.n - 1;

    // the row tile: weights of rows beyond the set are zeros (their points are those of the last row: finite)
    for (int e = tid; e < g.nvec * BG_TI; e += BG_TI * BG_WAVES) {
        const int vv = e / BG_TI, rr = e % BG_TI;
        us[e] = i0 + rr < g.n ? g.U[(i0 + rr) + (int64_t)vv * g.ldu] : (T)0;
    }
    T x[DM], acc[DM];
    double tot[DM];
#pragma unroll
    for (int k = 0; k < DM; ++k) {
        x[k] = k < g.d ? g.X[ic * g.d + k] : (T)0;
        acc[k] = (T)0;
        tot[k] = 0.0;
    }

    for (int c = 0; c < g.nch; ++c) {                              // component chunks; acc and tot persist: the sums are over the components
        T cu[QN], su[QN];
#pragma unroll
        for (int q = 0; q < QN; ++q) {
            cu[q] = g.RX[(int64_t)(c * 2 * SM_QC + q) * g.n + ic];
            su[q] = g.RX[(int64_t)(c * 2 * SM_QC + SM_QC + q) * g.n + ic];
        }
        // the chunk's coefficient rows: uniform addresses (scalar loads), or the three tables in LDS
        const T* cfe; const T* cfc; const T* cfs;
        T ce[QN];                                                  // ISO: the components' exponent coefficients (fp32: halved)
        if constexpr (ISO) {
            cfe = g.ciso + c * SM_QC; cfc = g.gciso + c * SM_QC; cfs = g.gsin + c * SM_QC * SM_CST;
#pragma unroll
            for (int q = 0; q < QN; ++q) ce[q] = EH * cfe[q];
        } else {
            __syncthreads();                                       // the previous chunk has read its rows
            T* cl = &cfl[0][0][0];
            for (int e = tid; e < SM_QC * SM_CST; e += BG_TI * BG_WAVES) {
                cl[e] = EH * g.coef[c * SM_QC * SM_CST + e];
                cl[SM_QC * SM_CST + e] = g.gcos[c * SM_QC * SM_CST + e];
                cl[2 * SM_QC * SM_CST + e] = g.gsin[c * SM_QC * SM_CST + e];
            }
            cfe = cl; cfc = cl + SM_QC * SM_CST; cfs = cl + 2 * SM_QC * SM_CST;
        }
        int held = 0;                                              // tiles in acc

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
                const int sl = c * 2 * SM_QC + (f < QN ? f : f - QN + SM_QC);
                cs[e] = jt + jj < j1 ? g.RY[(int64_t)sl * g.m + jt + jj] : (T)0;
            }
            __syncthreads();
#pragma unroll 1
            for (int jg = 0; jg < JPL; jg += PG) {
                const int col = wv * JPL + jg;                     // the group's first column in the tile
                // W_ij = sum_v u_iv a_jv, v ascending
                T w[PG];
#pragma unroll
                for (int p = 0; p < PG; ++p) w[p] = (T)0;
                for (int vv = 0; vv < g.nvec; ++vv) {
                    const T uv = us[vv * BG_TI + r];
                    const VP av = *(const VP*)(as + vv * TJ + col);
#pragma unroll
                    for (int p = 0; p < PG; ++p) w[p] = fma_t(uv, av[p], w[p]);
                }
                // |r|^2 (evaluated in the points' precision) and the exponents t_q = sum_k c_qk r_k^2 (in gc), dimensions ascending; ISO: t_q = c_q |r|^2
                T gc[PG][QN], gs[PG][QN], s[PG];
#pragma unroll
                for (int p = 0; p < PG; ++p) {
                    s[p] = (T)0;
#pragma unroll
                    for (int q = 0; q < QN; ++q) gc[p][q] = (T)0;
                }
#pragma unroll
                for (int kc = 0; kc < DM / 4; ++kc) {
                    V4 cf[QN];
                    if constexpr (!ISO) {
#pragma unroll
                        for (int q = 0; q < QN; ++q) cf[q] = *(const V4*)(cfe + q * SM_CST + 4 * kc);
                    }
#pragma unroll
                    for (int p = 0; p < PG; ++p) {
                        const V4 yv = *(const V4*)(ys + (col + p) * DM + 4 * kc);
                        const T dx = x[4 * kc] - yv.x, dy = x[4 * kc + 1] - yv.y, dz = x[4 * kc + 2] - yv.z, dw = x[4 * kc + 3] - yv.w;
                        if constexpr (ISO) {
                            s[p] = fma_t(dw, dw, fma_t(dz, dz, fma_t(dy, dy, fma_t(dx, dx, s[p]))));
                        } else {
                            const T d2x = dx * dx, d2y = dy * dy, d2z = dz * dz, d2w = dw * dw;
                            s[p] += (d2x + d2y) + (d2z + d2w);
#pragma unroll
                            for (int q = 0; q < QN; ++q) gc[p][q] = fma_t(cf[q].w, d2w, fma_t(cf[q].z, d2z, fma_t(cf[q].y, d2y, fma_t(cf[q].x, d2x, gc[p][q]))));
                        }
                    }
                    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
                }
                // per pair and component: W e cos phi and W e sin phi; at r = 0 cos phi := 1 and sin phi := 0
                T ci[PG];                                          // ISO: the one cosine chain of the pair
#pragma unroll
                for (int p = 0; p < PG; ++p) {
                    const bool zero = s[p] == (T)0;
                    ci[p] = (T)0;
#pragma unroll
                    for (int q = 0; q < QN; ++q) {
                        const T cv = cs[q * TJ + col + p], sv = cs[(QN + q) * TJ + col + p];
                        const T t = ISO ? ce[q] * s[p] : gc[p][q];
                        const T h = exp2_neg_tab(t);                   // fp32: exp2(-t / 2)
                        const T we = SPLIT ? (w[p] * h) * h : w[p] * h;
                        const T cosv = zero ? (T)1 : fma_t(cu[q], cv, su[q] * sv);
                        const T sinv = zero ? (T)0 : fma_t(su[q], cv, -(cu[q] * sv));
                        gc[p][q] = we * cosv;
                        gs[p][q] = we * sinv;
                        if constexpr (ISO) ci[p] = fma_t(cfc[q], gc[p][q], ci[p]);
                    }
                }
                // per dimension: the two chains over the chunk's components, then acc_c += S_c - r_c C_c
#pragma unroll
                for (int kc = 0; kc < DM / 4; ++kc) {
                    V4 a4[QN], b4[QN];
#pragma unroll
                    for (int q = 0; q < QN; ++q) {
                        a4[q] = *(const V4*)(cfs + q * SM_CST + 4 * kc);
                        if constexpr (!ISO) b4[q] = *(const V4*)(cfc + q * SM_CST + 4 * kc);
                    }
#pragma unroll
                    for (int p = 0; p < PG; ++p) {
                        const V4 yv = *(const V4*)(ys + (col + p) * DM + 4 * kc);
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const T df = x[4 * kc + t] - yv[t];
                            T sc = (T)0, cc = (T)0;
#pragma unroll
                            for (int q = 0; q < QN; ++q) {
                                sc = fma_t(a4[q][t], gs[p][q], sc);
                                if constexpr (!ISO) cc = fma_t(b4[q][t], gc[p][q], cc);
                            }
                            if constexpr (ISO) cc = ci[p];
                            acc[4 * kc + t] += fma_t(-df, cc, sc);
                        }
                    }
                    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (++held == KT || jt + TJ >= j1) {                   // hand-off: at most BG_L pairs per lane
#pragma unroll
                for (int k = 0; k < DM; ++k) {
                    tot[k] += (double)acc[k];
                    acc[k] = (T)0;
                }
                held = 0;
            }
        }
    }
    // the four waves' totals of a row in wave order; only rows of the set and dimensions below d are written
#pragma unroll
    for (int q = 0; q < BG_WAVES; ++q) {
        if (wv == q) {
#pragma unroll
            for (int k = 0; k < DM; ++k) red[k][r] = q == 0 ? tot[k] : red[k][r] + tot[k];
        }
        __syncthreads();
    }
    for (int e = tid; e < BG_TI * g.d; e += BG_TI * BG_WAVES) {
        const int rr = e / g.d, k = e % g.d;
        if (i0 + rr < g.n) g.slab[((int64_t)blockIdx.y * g.n + i0 + rr) * g.d + k] = red[k][rr];
    }
}

// out[e] <- sum_js slab[js][e], js ascending: a fixed order
__global__ __launch_bounds__(256) void smi_reduce_kernel(const double* __restrict__ slab, int64_t total, int64_t jsplit, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    double sum = slab[e];
    for (int64_t js = 1; js < jsplit; ++js) sum += slab[js * total + e];
    out[e] = sum;
}

template <typename T, int DM, int QN>
static void smi_launch_iso(bool iso, dim3 grid, size_t lds_tail, hipStream_t stream, const SmiArgs<T>& g) {
    constexpr int TJ = bg_jpl<T> * BG_WAVES;
    const size_t lds = ((size_t)TJ * DM + (size_t)2 * QN * TJ) * sizeof(T) + lds_tail;
    if (iso) hipLaunchKernelGGL((smi_pair_kernel<T, DM, QN, true>), grid, dim3(BG_TI * BG_WAVES), lds, stream, g);
    else hipLaunchKernelGGL((smi_pair_kernel<T, DM, QN, false>), grid, dim3(BG_TI * BG_WAVES), lds, stream, g);
}

template <typename T, int QN>
static void smi_launch_q(int dm, bool iso, dim3 grid, size_t lds_tail, hipStream_t stream, const SmiArgs<T>& g) {
    if (dm == 4) smi_launch_iso<T, 4, QN>(iso, grid, lds_tail, stream, g);
    else if (dm == 8) smi_launch_iso<T, 8, QN>(iso, grid, lds_tail, stream, g);
    else smi_launch_iso<T, 16, QN>(iso, grid, lds_tail, stream, g);
}

template <typename T>
static int smi_run(covgram_sm* S, const covgram_points* X, const covgram_points* Y, const void* U, int64_t ldu, const void* A, int64_t lda, int nvec,
                   double* out_dev) {
    covgram_ctx* ctx = S->ctx;
    const int64_t n = X->n, m = Y->n;
    const int d = S->d;
    const int qpad = S->nch * SM_QC;
    const T* prm = (const T*)S->prm;
    // the phase tables of both point sets in workspace slot 0, both in the row layout (no weights)
    const size_t rx_bytes = (((size_t)n * 2 * qpad * sizeof(T)) + 255) & ~(size_t)255;
    void* ph;
    int rc = ws_reserve(ctx, 0, rx_bytes + (size_t)m * 2 * qpad * sizeof(T), &ph);
    if (rc) return rc;
    T* RX = (T*)ph; T* RY = (T*)((char*)ph + rx_bytes);
    SmiArgs<T> g;
    memset(&g, 0, sizeof(g));
    g.X = (const T*)X->dptr; g.Y = (const T*)Y->dptr; g.n = n; g.m = m;
    g.d = d; g.nch = S->nch;
    g.U = (const T*)U; g.ldu = ldu; g.A = (const T*)A; g.lda = lda; g.nvec = nvec;
    g.RX = RX; g.RY = RY;
    g.coef = prm + qpad + (size_t)qpad * d;
    g.ciso = g.coef + (size_t)qpad * SM_CST;
    g.gsin = g.ciso + qpad;
    g.gcos = g.gsin + (size_t)qpad * SM_CST;
    g.gciso = g.gcos + (size_t)qpad * SM_CST;
    constexpr int TJ = bg_jpl<T> * BG_WAVES;
    const int64_t rowtiles = (n + BG_TI - 1) / BG_TI;
    const int64_t total = n * d;
    CG_REQUIRE(rowtiles <= 0x7fffffff && (total + 255) / 256 <= 0x7fffffff, COVGRAM_EUNSUPPORTED, "bilinear_input_grad_sm: n = %lld exceeds the grid",
               (long long)n);
    const int64_t jsplit = bg_column_split<T>(ctx, rowtiles, m, &g.jchunk);
    void* slab;
    rc = ws_reserve(ctx, 1, (size_t)jsplit * total * sizeof(double), &slab);
    if (rc) return rc;
    g.slab = (double*)slab;
    const int dm = d <= 4 ? 4 : (d <= 8 ? 8 : 16);
    const bool iso = S->isotropic != 0;
    const size_t lds_tail = (size_t)nvec * (BG_TI + TJ) * sizeof(T);
    const dim3 grid((unsigned)rowtiles, (unsigned)jsplit);
    TimerScope tm(ctx);
    for (int side = 0; side < 2; ++side) {
        const covgram_points* P = side ? Y : X;
        const int64_t threads = P->n * qpad;
        hipLaunchKernelGGL((sm_phase_kernel<T>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)P->dptr, P->n, (const T*)nullptr,
                           (int64_t)0, (int)d, (int)S->ncomp, (int)S->nch, prm, prm + qpad, side ? RY : RX, (T*)nullptr);
    }
    switch (S->ncomp) {                                            // up to SM_QC components: exactly one chunk of that many
        case 1: smi_launch_q<T, 1>(dm, iso, grid, lds_tail, ctx->stream, g); break;
        case 2: smi_launch_q<T, 2>(dm, iso, grid, lds_tail, ctx->stream, g); break;
        case 3: smi_launch_q<T, 3>(dm, iso, grid, lds_tail, ctx->stream, g); break;
        default: smi_launch_q<T, 4>(dm, iso, grid, lds_tail, ctx->stream, g); break;
    }
    hipLaunchKernelGGL(smi_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)slab, total, jsplit, out_dev);
    return COVGRAM_OK;
}

}  // namespace covgram

using namespace covgram;

extern "C" int covgram_bilinear_input_grad_sm(covgram_sm* S, const covgram_points* X, const covgram_points* Y, const void* U, int64_t ldu, const void* A,
                                              int64_t lda, int32_t nvec, double* dX, int32_t loc) {
    CG_REQUIRE(S != nullptr, COVGRAM_EINVAL, "spectral-mixture handle is NULL");
    CG_REQUIRE(X != nullptr, COVGRAM_EINVAL, "NULL argument");
    if (!Y) Y = X;
    int rc = sm_check_points(S, X, Y);
    if (rc) return rc;
    CG_REQUIRE(loc == COVGRAM_HOST || loc == COVGRAM_DEVICE, COVGRAM_EINVAL, "unknown loc %d", loc);
    CG_REQUIRE(nvec >= 1 && nvec <= BG_MAX_NVEC, COVGRAM_EINVAL, "bilinear_input_grad_sm: nvec = %d is outside 1 .. %d", nvec, BG_MAX_NVEC);
    CG_REQUIRE(dX != nullptr, COVGRAM_EINVAL, "dX is NULL");
    const int64_t n = X->n, m = Y->n;
    CG_REQUIRE(ldu >= n && lda >= m, COVGRAM_EINVAL, "DimensionMismatch: ldu=%lld < n=%lld or lda=%lld < m=%lld", (long long)ldu, (long long)n,
               (long long)lda, (long long)m);
    CG_REQUIRE((U != nullptr || n == 0) && (A != nullptr || m == 0), COVGRAM_EINVAL, "U or A is NULL");
    if (n == 0) return COVGRAM_OK;
    covgram_ctx* ctx = S->ctx;
    const size_t ts = dtype_size(S->dtype);
    const size_t obytes = (size_t)n * S->d * sizeof(double);
    CG_DEVICE(ctx);
    if (m == 0) {                                                  // an empty sum per row
        if (loc == COVGRAM_HOST) memset(dX, 0, obytes);
        else CG_CHECK_HIP(hipMemsetAsync(dX, 0, obytes, ctx->stream));
        return COVGRAM_OK;
    }
    const void* u_dev = U; const void* a_dev = A;
    double* o_dev = dX;
    int64_t ldu_d = ldu, lda_d = lda;
    if (loc == COVGRAM_HOST) {
        void* so;
        rc = bg_stage_weights(ctx, n, m, nvec, ts, &u_dev, &ldu_d, &a_dev, &lda_d); if (rc) return rc;
        rc = ws_reserve(ctx, 3, obytes, &so); if (rc) return rc;
        o_dev = (double*)so;
    }
    rc = by_dtype(S->dtype, [&](auto t) { return smi_run<decltype(t)>(S, X, Y, u_dev, ldu_d, a_dev, lda_d, nvec, o_dev); });
    if (rc) return rc;
    CG_CHECK_HIP(hipGetLastError());
    if (loc == COVGRAM_HOST) {
        CG_CHECK_HIP(hipMemcpyAsync(dX, o_dev, obytes, hipMemcpyDeviceToHost, ctx->stream));
        CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return COVGRAM_OK;
}
