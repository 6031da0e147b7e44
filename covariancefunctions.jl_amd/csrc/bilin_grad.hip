// bilin_grad.hip — hyper-parameter gradients of the bilinear forms sum_t u_t' G a_t in ONE pass over the n m pairs:
//     out[0]     = sum_ij W_ij k_ij                       W = U A' (rank nvec), formed per pair in registers, never stored
//     out[1]     = sum_ij W_ij dk_ij / dparam             RQ alpha | gamma-exponential gamma | IMQ c; 0 for the other families
//     out[2 + c] = sum_ij W_ij (dk/ds)_ij (x_ic - y_jc)^2  per_dim; otherwise out[2] = sum_ij W_ij (dk/ds)_ij s_ij
// with s the RAW squared distance (dk/ds carries scale, power and lengthscale).  fp32 and fp64; the results are always fp64.
//
// Shape of the computation:
//   * a workgroup (4 waves) owns BG_TI = 64 rows and a chunk of column tiles of 64 (fp32) or 32 (fp64) columns.  Lane r of every wave is
//     row r, wave w takes a quarter of each tile's columns: JPL = 16 (fp32) or 8 (fp64) pairs per lane and tile;
//   * LDS: the row tile's points xs and weights us (staged once: the row tile never changes), the column tile's points ys and
//     weights as (per tile).  Points wider than BG_DS = 16 dimensions pass through xs / ys in slabs of 16 (twice per tile: once for s,
//     once for the per-dimension sums), so that the footprint does not grow with d: <= 50 KB in fp64 at nvec = 32;
//   * per tile: W_ij as nvec fmas (one lane read of us and JPL / 4 four-wide broadcast reads of as per JPL fmas); s_ij by direct differences;
//     the jet (k, dk/ds, dk/dparam) by a wave-uniform switch on the family; the per-dimension sums in chunks of four dimensions whose
//     four accumulators are the only registers that depend on d — nothing spills at d = 64;
//   * reduction: a lane adds at most BG_L = 128 pairs in the working precision; then the 64 lanes are added by a butterfly in the working
//     precision and the wave's sum joins an fp64 total that lane (k mod 64) keeps for output k.  At the end the four waves' totals are
//     added in fp64 in wave order and written to a slab; bg_reduce_kernel adds the slab in a fixed order.  No atomics.
//   * a pair with s = 0 adds exactly 0 to out[2 ..]: dk/ds is replaced by 0 there (never 0 * inf), and to out[1] its finite limit.
#include "bilin_common.hpp"

namespace covgram {

constexpr int BG_MAX_OUT = 2 + BG_MAX_D;

template <typename T>
struct BgArgs {
    const T* X; const T* Y;          // points, point-major, stride d
    int64_t n, m;
    int32_t d, dpad;                 // dpad: d rounded up to a multiple of 4
    const T* U; int64_t ldu;         // n x nvec
    const T* A; int64_t lda;         // m x nvec
    int32_t nvec, family, per_dim, nout;
    T cpar;                          // the struct's own param (IMQ: c; kp.param holds c^2)
    KParams<T> kp;                   // gradient form: gamma = 1 / l, natural tables
    double* slab;                    // [gridDim.y][gridDim.x][nout]
    int64_t jchunk;                  // columns per blockIdx.y (a multiple of the tile width)
};

template <typename T>
__device__ __forceinline__ T bg_wave_sum(T x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

template <typename T>
__global__ __launch_bounds__(BG_TI * BG_WAVES) void bg_pair_kernel(const BgArgs<T> g) {
    constexpr int BG_JPL = bg_jpl<T>, BG_TJ = BG_JPL * BG_WAVES, BG_KT = BG_L / BG_JPL;
    extern __shared__ __align__(32) unsigned char bg_lds[];
    __shared__ double red[BG_WAVES][BG_MAX_OUT];
    using V4 = T __attribute__((ext_vector_type(4)));
    const int ds_w = g.dpad < BG_DS ? g.dpad : BG_DS;              // slab width in LDS (a multiple of 4)
    const int xs_w = ((ds_w >> 2) & 1) ? ds_w : ds_w + 4;         // row stride: an odd number of 16-byte groups
    const int nslab = (g.dpad + BG_DS - 1) / BG_DS;
    T* xs = (T*)bg_lds;                                            // [BG_TI][xs_w]
    T* ys = xs + BG_TI * xs_w;                                     // [BG_TJ][ds_w]
    T* us = ys + BG_TJ * ds_w;                                     // [nvec][BG_TI]
    T* as = us + g.nvec * BG_TI;                                   // [nvec][BG_TJ]
    static_assert(BG_JPL % 4 == 0 && BG_L % BG_JPL == 0, "128-bit broadcast reads of as; whole tiles per hand-off");
    const int tid = threadIdx.x, r = tid & 63, wv = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * BG_TI;
    const int64_t j0 = (int64_t)blockIdx.y * g.jchunk;
    const int64_t j1 = j0 + g.jchunk < g.m ? j0 + g.jchunk : g.m;
    double tot0 = 0.0, tot1 = 0.0;                                 // lane k of a wave: outputs k and 64 + k
    auto wave_add = [&](int k, T x) {
        const T w = bg_wave_sum(x);
        if (r == (k & 63)) { if (k < 64) tot0 += (double)w; else tot1 += (double)w; }
    };
    // one slab of a point tile: rows beyond the set and dimensions beyond d are zeros
    auto stage_points = [&](T* dst, int stride, int rows, const T* P, int64_t p0, int64_t pn, int c0) {
        for (int e = tid; e < rows * ds_w; e += BG_TI * BG_WAVES) {
            const int pp = e / ds_w, k = e % ds_w;
            const int64_t p = p0 + pp;
            dst[pp * stride + k] = (p < pn && c0 + k < g.d) ? P[p * g.d + c0 + k] : (T)0;
        }
    };
    for (int e = tid; e < g.nvec * BG_TI; e += BG_TI * BG_WAVES) {
        const int vv = e / BG_TI, rr = e % BG_TI;
        us[e] = i0 + rr < g.n ? g.U[(i0 + rr) + (int64_t)vv * g.ldu] : (T)0;
    }
    if (nslab == 1) stage_points(xs, xs_w, BG_TI, g.X, i0, g.n, 0);

    T acc0 = (T)0, acc1 = (T)0, acc2 = (T)0;
    int held = 0;                                                  // tiles in acc0 .. acc2
    for (int64_t jt = j0; jt < j1; jt += BG_TJ) {
        __syncthreads();                                           // the previous tile has been consumed
        for (int e = tid; e < g.nvec * BG_TJ; e += BG_TI * BG_WAVES) {
            const int vv = e / BG_TJ, jj = e % BG_TJ;
            as[e] = jt + jj < j1 ? g.A[(jt + jj) + (int64_t)vv * g.lda] : (T)0;
        }
        if (nslab == 1) stage_points(ys, ds_w, BG_TJ, g.Y, jt, j1, 0);
        __syncthreads();
        // W_ij = sum_v u_iv a_jv, v ascending
        T w[BG_JPL];
#pragma unroll
        for (int jj = 0; jj < BG_JPL; ++jj) w[jj] = (T)0;
        for (int vv = 0; vv < g.nvec; ++vv) {
            const T uv = us[vv * BG_TI + r];
            const V4* a4 = (const V4*)(as + vv * BG_TJ + wv * BG_JPL);
#pragma unroll
            for (int q = 0; q < BG_JPL / 4; ++q) {
                const V4 av = a4[q];
                w[4 * q + 0] = fma_t(uv, av.x, w[4 * q + 0]);
                w[4 * q + 1] = fma_t(uv, av.y, w[4 * q + 1]);
                w[4 * q + 2] = fma_t(uv, av.z, w[4 * q + 2]);
                w[4 * q + 3] = fma_t(uv, av.w, w[4 * q + 3]);
            }
        }
        // s_ij by direct differences, dimensions ascending
        T s[BG_JPL];
#pragma unroll
        for (int jj = 0; jj < BG_JPL; ++jj) s[jj] = (T)0;
        for (int sl = 0; sl < nslab; ++sl) {
            if (nslab > 1) {
                __syncthreads();
                stage_points(xs, xs_w, BG_TI, g.X, i0, g.n, sl * BG_DS);
                stage_points(ys, ds_w, BG_TJ, g.Y, jt, j1, sl * BG_DS);
                __syncthreads();
            }
            for (int c0 = 0; c0 < ds_w; c0 += 4) {
                const V4 xv = *(const V4*)(xs + r * xs_w + c0);
#pragma unroll
                for (int jj = 0; jj < BG_JPL; ++jj) {
                    const V4 yv = *(const V4*)(ys + (wv * BG_JPL + jj) * ds_w + c0);
                    const V4 df = xv - yv;
                    s[jj] = fma_t(df.w, df.w, fma_t(df.z, df.z, fma_t(df.y, df.y, fma_t(df.x, df.x, s[jj]))));
                }
            }
        }
        // the jet; gw = W dk/ds
        T gw[BG_JPL];
#pragma unroll 2
        for (int jj = 0; jj < BG_JPL; ++jj) {
            T v, dsv, dp;
            bg_jet<T>(g.family, s[jj], g.kp, g.cpar, v, dsv, dp);
            const T wij = w[jj];
            const bool zero = wij == (T)0;                         // rows / columns beyond the sets: nothing, whatever the jet gave
            acc0 = fma_t(wij, zero ? (T)0 : v, acc0);
            acc1 = fma_t(wij, zero ? (T)0 : dp, acc1);
            gw[jj] = zero ? (T)0 : wij * dsv;
            if (!g.per_dim) acc2 = fma_t(gw[jj], s[jj], acc2);
        }
        if (g.per_dim) {
            for (int sl = 0; sl < nslab; ++sl) {
                if (nslab > 1) {
                    __syncthreads();
                    stage_points(xs, xs_w, BG_TI, g.X, i0, g.n, sl * BG_DS);
                    stage_points(ys, ds_w, BG_TJ, g.Y, jt, j1, sl * BG_DS);
                    __syncthreads();
                }
                for (int c0 = 0; c0 < ds_w; c0 += 4) {
                    const V4 xv = *(const V4*)(xs + r * xs_w + c0);
                    V4 a4 = {(T)0, (T)0, (T)0, (T)0};
#pragma unroll
                    for (int jj = 0; jj < BG_JPL; ++jj) {
                        const V4 yv = *(const V4*)(ys + (wv * BG_JPL + jj) * ds_w + c0);
                        const V4 df = xv - yv;
                        const V4 d2 = df * df;
                        a4.x = fma_t(gw[jj], d2.x, a4.x);
                        a4.y = fma_t(gw[jj], d2.y, a4.y);
                        a4.z = fma_t(gw[jj], d2.z, a4.z);
                        a4.w = fma_t(gw[jj], d2.w, a4.w);
                    }
                    const int c = sl * BG_DS + c0;
                    if (c + 0 < g.d) wave_add(2 + c + 0, a4.x);
                    if (c + 1 < g.d) wave_add(2 + c + 1, a4.y);
                    if (c + 2 < g.d) wave_add(2 + c + 2, a4.z);
                    if (c + 3 < g.d) wave_add(2 + c + 3, a4.w);
                }
            }
        }
        if (++held == BG_KT || jt + BG_TJ >= j1) {                 // hand-off: at most BG_L pairs per lane
            wave_add(0, acc0);
            wave_add(1, acc1);
            if (!g.per_dim) wave_add(2, acc2);
            acc0 = (T)0; acc1 = (T)0; acc2 = (T)0; held = 0;
        }
    }
    if (r < 64) { red[wv][r] = tot0; if (r < BG_MAX_OUT - 64) red[wv][64 + r] = tot1; }
    __syncthreads();
    if (tid < g.nout) {
        double t = red[0][tid];
#pragma unroll
        for (int q = 1; q < BG_WAVES; ++q) t += red[q][tid];
        g.slab[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * g.nout + tid] = t;
    }
}

// out[k] <- sum over the slab's nblk rows: 256 strided partial sums per output, then a tree in LDS — a fixed order
__global__ __launch_bounds__(256) void bg_reduce_kernel(const double* __restrict__ slab, int64_t nblk, int nout, double* __restrict__ out) {
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
    if (t == 0) out[k] = part[0];
}

template <typename T>
static int bg_run(covgram_ctx* ctx, const HostKernel& hk, const covgram_points* X, const covgram_points* Y, const void* U, int64_t ldu, const void* A,
                  int64_t lda, int nvec, int per_dim, int nout, double* out_dev) {
    const int64_t n = X->n, m = Y->n;
    const int d = X->d;
    BgArgs<T> g;
    memset(&g, 0, sizeof(g));
    g.X = (const T*)X->dptr; g.Y = (const T*)Y->dptr; g.n = n; g.m = m; g.d = d; g.dpad = (d + 3) & ~3;
    g.U = (const T*)U; g.ldu = ldu; g.A = (const T*)A; g.lda = lda;
    g.nvec = nvec; g.family = hk.k.family; g.per_dim = per_dim; g.nout = nout;
    g.cpar = (T)hk.k.param;
    g.kp = cast_params<T>(hk.kp);
    constexpr int BG_TJ = bg_jpl<T> * BG_WAVES;
    const int64_t rowtiles = (n + BG_TI - 1) / BG_TI;
    const int64_t jsplit = bg_column_split<T>(ctx, rowtiles, m, &g.jchunk);
    CG_REQUIRE(rowtiles <= 0x7fffffff, COVGRAM_EUNSUPPORTED, "bilinear_grad: n = %lld exceeds the grid", (long long)n);
    const int64_t nblk = rowtiles * jsplit;
    void* slab;
    int rc = ws_reserve(ctx, 1, (size_t)nblk * nout * sizeof(double), &slab);
    if (rc) return rc;
    g.slab = (double*)slab;
    const int ds_w = std::min<int>(g.dpad, BG_DS);
    const int xs_w = ((ds_w >> 2) & 1) ? ds_w : ds_w + 4;
    const size_t lds = ((size_t)BG_TI * xs_w + (size_t)BG_TJ * ds_w + (size_t)nvec * (BG_TI + BG_TJ)) * sizeof(T);
    TimerScope tm(ctx);
    hipLaunchKernelGGL((bg_pair_kernel<T>), dim3((unsigned)rowtiles, (unsigned)jsplit), dim3(BG_TI * BG_WAVES), lds, ctx->stream, g);
    hipLaunchKernelGGL(bg_reduce_kernel, dim3((unsigned)nout), dim3(256), 0, ctx->stream, (const double*)slab, nblk, nout, out_dev);
    return COVGRAM_OK;
}

}  // namespace covgram

using namespace covgram;

extern "C" int covgram_bilinear_grad(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* U, int64_t ldu,
                                     const void* A, int64_t lda, int32_t nvec, int32_t per_dim, double* out, int32_t loc) {
    int rc = bg_check_args("bilinear_grad", ctx, k, X, &Y, U, ldu, A, lda, nvec, out, loc);
    if (rc) return rc;
    const int64_t n = X->n, m = Y->n;
    HostKernel hk;
    rc = make_host_kernel(k, X->dtype, true, &hk);
    if (rc) return rc;
    const int nout = 2 + (per_dim ? X->d : 1);
    const size_t ts = dtype_size(X->dtype);
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
    rc = X->dtype == COVGRAM_F32 ? bg_run<float>(ctx, hk, X, Y, u_dev, ldu_d, a_dev, lda_d, nvec, per_dim ? 1 : 0, nout, o_dev)
                                 : bg_run<double>(ctx, hk, X, Y, u_dev, ldu_d, a_dev, lda_d, nvec, per_dim ? 1 : 0, nout, o_dev);
    if (rc) return rc;
    CG_CHECK_HIP(hipGetLastError());
    if (loc == COVGRAM_HOST) {
        CG_CHECK_HIP(hipMemcpyAsync(out, o_dev, nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return COVGRAM_OK;
}
