// input_grad.hip — the gradient of the bilinear forms sum_t u_t' G a_t with respect to the ROW points in ONE pass over the n m pairs
// (DESIGN.md 3.16).  With W = U A' (rank nvec, formed per pair in registers, never stored) and s_ij = |x_i - y_j|^2 (raw):
//     dX[i d + c] = sum_j W_ij 2 (dk/ds)_ij (x_ic - y_jc)
// the partial derivative of F(X, Y) = sum_ij W_ij k(x_i, y_j) in x_ic with the column side held fixed (also when Y = X: the host adds the
// call with U and A swapped).  fp32 and fp64 points; the results are always fp64.
//
// Shape of the computation (bg_pair_kernel's, bilin_grad.hip; the jet and the constants come from bilin_common.hpp):
//   * a workgroup (4 waves) owns BG_TI = 64 rows, a chunk of column tiles of 64 (fp32) or 32 (fp64) columns (blockIdx.y) and a group of at
//     most BG_DS = 16 output dimensions (blockIdx.z).  Lane r of every wave is row r, wave w takes a quarter of each tile's columns;
//   * per tile: W_ij as nvec fmas (v ascending); s_ij by direct differences over ALL d dimensions (ascending, through the 16-dimension LDS
//     slabs); the jet by a wave-uniform switch on the family, dk/ds replaced by 0 where the scaled s is 0; gw_ij = W_ij (dk/ds)_ij, 0 for
//     rows and columns beyond the sets (W_ij = 0 there); then for the group's dimensions acc_c = fma(gw_ij, x_ic - y_jc, acc_c), the
//     difference recomputed from LDS.  The accumulators are addressed statically (four unrolled chunks of four): registers, not scratch;
//   * reduction: the row is the lane's own, there is no cross-lane step.  A lane adds at most BG_L = 128 pairs in the working precision,
//     then its <= 16 partial sums join fp64 totals it keeps in LDS ([wave][dimension][row]: lane-private, conflict-free addresses).  At the
//     end the four waves' totals of a row are added in fp64 in wave order and written to the slab [jsplit][n][d]; ig_reduce_kernel adds
//     the column chunks in ascending order and applies the factor 2 (exact).  No atomics: two calls agree bit for bit, and since every
//     group forms s, the jet and gw identically, the result does not depend on the grouping.
#include "bilin_common.hpp"

namespace covgram {

template <typename T>
struct IgArgs {
    const T* X; const T* Y;          // points, point-major, stride d
    int64_t n, m;
    int32_t d, dpad;                 // dpad: d rounded up to a multiple of 4
    const T* U; int64_t ldu;         // n x nvec
    const T* A; int64_t lda;         // m x nvec
    int32_t nvec, family;
    int32_t dg;                      // output dimensions per blockIdx.z: 16, or 8 where 16 would not fit the LDS (a divisor of BG_DS)
    T cpar;
    KParams<T> kp;                   // gradient form: gamma = 1 / l, natural tables
    double* slab;                    // [gridDim.y][n][d]
    int64_t jchunk;                  // columns per blockIdx.y (a multiple of the tile width)
};

template <typename T>
__global__ __launch_bounds__(BG_TI * BG_WAVES) void ig_pair_kernel(const IgArgs<T> g) {
    constexpr int JPL = bg_jpl<T>, TJ = JPL * BG_WAVES, KT = BG_L / JPL;
    extern __shared__ __align__(32) unsigned char ig_lds[];
    using V4 = T __attribute__((ext_vector_type(4)));
    const int ds_w = g.dpad < BG_DS ? g.dpad : BG_DS;              // slab width in LDS (a multiple of 4)
    const int xs_w = ((ds_w >> 2) & 1) ? ds_w : ds_w + 4;         // row stride: an odd number of 16-byte groups
    const int nslab = (g.dpad + BG_DS - 1) / BG_DS;
    const int c_lo = blockIdx.z * g.dg;                            // this workgroup's output dimensions: c_lo .. c_lo + dg
    const int gsl = c_lo / BG_DS, goff = c_lo % BG_DS;             // the slab that holds them and their offset in it
    const int gdim4 = g.dpad - c_lo < g.dg ? g.dpad - c_lo : g.dg; // how many, rounded up to a multiple of 4
    const int tw = g.dg < ds_w ? g.dg : ds_w;
    double* tot = (double*)ig_lds;                                 // [BG_WAVES][tw][BG_TI]
    T* xs = (T*)(tot + BG_WAVES * tw * BG_TI);                     // [BG_TI][xs_w]
    T* ys = xs + BG_TI * xs_w;                                     // [TJ][ds_w]
    T* us = ys + TJ * ds_w;                                        // [nvec][BG_TI]
    T* as = us + g.nvec * BG_TI;                                   // [nvec][TJ]
    static_assert(JPL % 4 == 0 && BG_L % JPL == 0, "128-bit broadcast reads of as; whole tiles per hand-off");
    const int tid = threadIdx.x, r = tid & 63, wv = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * BG_TI;
    const int64_t j0 = (int64_t)blockIdx.y * g.jchunk;
    const int64_t j1 = j0 + g.jchunk < g.m ? j0 + g.jchunk : g.m;
    double* mytot = tot + wv * tw * BG_TI + r;                     // dimension c_lo + c of this lane: mytot[c * BG_TI]
    for (int c = 0; c < tw; ++c) mytot[c * BG_TI] = 0.0;
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

    T acc[BG_DS];
#pragma unroll
    for (int c = 0; c < BG_DS; ++c) acc[c] = (T)0;
    int held = 0;                                                  // tiles in acc
    for (int64_t jt = j0; jt < j1; jt += TJ) {
        __syncthreads();                                           // the previous tile has been consumed
        for (int e = tid; e < g.nvec * TJ; e += BG_TI * BG_WAVES) {
            const int vv = e / TJ, jj = e % TJ;
            as[e] = jt + jj < j1 ? g.A[(jt + jj) + (int64_t)vv * g.lda] : (T)0;
        }
        if (nslab == 1) stage_points(ys, ds_w, TJ, g.Y, jt, j1, 0);
        __syncthreads();
        // W_ij = sum_v u_iv a_jv, v ascending
        T w[JPL];
#pragma unroll
        for (int jj = 0; jj < JPL; ++jj) w[jj] = (T)0;
        for (int vv = 0; vv < g.nvec; ++vv) {
            const T uv = us[vv * BG_TI + r];
            const V4* a4 = (const V4*)(as + vv * TJ + wv * JPL);
#pragma unroll
            for (int q = 0; q < JPL / 4; ++q) {
                const V4 av = a4[q];
                w[4 * q + 0] = fma_t(uv, av.x, w[4 * q + 0]);
                w[4 * q + 1] = fma_t(uv, av.y, w[4 * q + 1]);
                w[4 * q + 2] = fma_t(uv, av.z, w[4 * q + 2]);
                w[4 * q + 3] = fma_t(uv, av.w, w[4 * q + 3]);
            }
        }
        // s_ij by direct differences, dimensions ascending
        T s[JPL];
#pragma unroll
        for (int jj = 0; jj < JPL; ++jj) s[jj] = (T)0;
        for (int sl = 0; sl < nslab; ++sl) {
            if (nslab > 1) {
                __syncthreads();
                stage_points(xs, xs_w, BG_TI, g.X, i0, g.n, sl * BG_DS);
                stage_points(ys, ds_w, TJ, g.Y, jt, j1, sl * BG_DS);
                __syncthreads();
            }
            for (int c0 = 0; c0 < ds_w; c0 += 4) {
                const V4 xv = *(const V4*)(xs + r * xs_w + c0);
#pragma unroll
                for (int jj = 0; jj < JPL; ++jj) {
                    const V4 yv = *(const V4*)(ys + (wv * JPL + jj) * ds_w + c0);
                    const V4 df = xv - yv;
                    s[jj] = fma_t(df.w, df.w, fma_t(df.z, df.z, fma_t(df.y, df.y, fma_t(df.x, df.x, s[jj]))));
                }
            }
        }
        // gw = W dk/ds; rows / columns beyond the sets have W = 0: nothing, whatever the jet gave
        T gw[JPL];
#pragma unroll 2
        for (int jj = 0; jj < JPL; ++jj) {
            T v, dsv, dp;
            bg_jet<T>(g.family, s[jj], g.kp, g.cpar, v, dsv, dp);
            const T wij = w[jj];
            gw[jj] = wij == (T)0 ? (T)0 : wij * dsv;
        }
        // the group's dimensions: its slab is in LDS already unless another one was staged last
        if (nslab > 1 && gsl != nslab - 1) {
            __syncthreads();
            stage_points(xs, xs_w, BG_TI, g.X, i0, g.n, gsl * BG_DS);
            stage_points(ys, ds_w, TJ, g.Y, jt, j1, gsl * BG_DS);
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < BG_DS / 4; ++q) {
            if (4 * q < gdim4) {
                const V4 xv = *(const V4*)(xs + r * xs_w + goff + 4 * q);
#pragma unroll
                for (int jj = 0; jj < JPL; ++jj) {
                    const V4 yv = *(const V4*)(ys + (wv * JPL + jj) * ds_w + goff + 4 * q);
                    const V4 df = xv - yv;
                    acc[4 * q + 0] = fma_t(gw[jj], df.x, acc[4 * q + 0]);
                    acc[4 * q + 1] = fma_t(gw[jj], df.y, acc[4 * q + 1]);
                    acc[4 * q + 2] = fma_t(gw[jj], df.z, acc[4 * q + 2]);
                    acc[4 * q + 3] = fma_t(gw[jj], df.w, acc[4 * q + 3]);
                }
            }
        }
        if (++held == KT || jt + TJ >= j1) {                       // hand-off: at most BG_L pairs per lane
#pragma unroll
            for (int c = 0; c < BG_DS; ++c) {
                if (c < gdim4) mytot[c * BG_TI] += (double)acc[c];
                acc[c] = (T)0;
            }
            held = 0;
        }
    }
    __syncthreads();
    // the four waves' totals of a row in wave order; only rows of the set and dimensions below d are written
    const int gd = g.d - c_lo < g.dg ? g.d - c_lo : g.dg;
    for (int e = tid; e < BG_TI * gd; e += BG_TI * BG_WAVES) {
        const int rr = e / gd, c = e % gd;
        if (i0 + rr < g.n) {
            double t = tot[c * BG_TI + rr];
#pragma unroll
            for (int q = 1; q < BG_WAVES; ++q) t += tot[(q * tw + c) * BG_TI + rr];
            g.slab[((int64_t)blockIdx.y * g.n + i0 + rr) * g.d + c_lo + c] = t;
        }
    }
}

// out[e] <- 2 sum_js slab[js][e], js ascending: a fixed order
__global__ __launch_bounds__(256) void ig_reduce_kernel(const double* __restrict__ slab, int64_t total, int64_t jsplit, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    double sum = slab[e];
    for (int64_t js = 1; js < jsplit; ++js) sum += slab[js * total + e];
    out[e] = 2.0 * sum;
}

template <typename T>
static int ig_run(covgram_ctx* ctx, const HostKernel& hk, const covgram_points* X, const covgram_points* Y, const void* U, int64_t ldu, const void* A,
                  int64_t lda, int nvec, double* out_dev) {
    const int64_t n = X->n, m = Y->n;
    const int d = X->d;
    IgArgs<T> g;
    memset(&g, 0, sizeof(g));
    g.X = (const T*)X->dptr; g.Y = (const T*)Y->dptr; g.n = n; g.m = m; g.d = d; g.dpad = (d + 3) & ~3;
    g.U = (const T*)U; g.ldu = ldu; g.A = (const T*)A; g.lda = lda;
    g.nvec = nvec; g.family = hk.k.family;
    g.cpar = (T)hk.k.param;
    g.kp = cast_params<T>(hk.kp);
    constexpr int TJ = bg_jpl<T> * BG_WAVES;
    const int64_t rowtiles = (n + BG_TI - 1) / BG_TI;
    // LDS: the fp64 totals of one dimension group beside the tiles; 16 dimensions per group unless that passes 64 KB (fp64, nvec > 24)
    const int ds_w = std::min<int>(g.dpad, BG_DS);
    const int xs_w = ((ds_w >> 2) & 1) ? ds_w : ds_w + 4;
    const size_t tiles = ((size_t)BG_TI * xs_w + (size_t)TJ * ds_w + (size_t)nvec * (BG_TI + TJ)) * sizeof(T);
    auto lds_of = [&](int dg) { return (size_t)BG_WAVES * std::min(dg, ds_w) * BG_TI * sizeof(double) + tiles; };
    g.dg = lds_of(BG_DS) <= 65536 ? BG_DS : BG_DS / 2;
    const size_t lds = lds_of(g.dg);
    const int ngroups = (d + g.dg - 1) / g.dg;
    const int64_t jsplit = bg_column_split<T>(ctx, rowtiles * ngroups, m, &g.jchunk);
    const int64_t total = n * d;
    CG_REQUIRE(rowtiles <= 0x7fffffff && (total + 255) / 256 <= 0x7fffffff, COVGRAM_EUNSUPPORTED, "bilinear_input_grad: n = %lld exceeds the grid",
               (long long)n);
    void* slab;
    int rc = ws_reserve(ctx, 1, (size_t)jsplit * total * sizeof(double), &slab);
    if (rc) return rc;
    g.slab = (double*)slab;
    TimerScope tm(ctx);
    hipLaunchKernelGGL((ig_pair_kernel<T>), dim3((unsigned)rowtiles, (unsigned)jsplit, (unsigned)ngroups), dim3(BG_TI * BG_WAVES), lds, ctx->stream, g);
    hipLaunchKernelGGL(ig_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)slab, total, jsplit, out_dev);
    return COVGRAM_OK;
}

}  // namespace covgram

using namespace covgram;

extern "C" int covgram_bilinear_input_grad(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* U,
                                           int64_t ldu, const void* A, int64_t lda, int32_t nvec, double* dX, int32_t loc) {
    int rc = bg_check_args("bilinear_input_grad", ctx, k, X, &Y, U, ldu, A, lda, nvec, dX, loc);
    if (rc) return rc;
    const int64_t n = X->n, m = Y->n;
    HostKernel hk;
    rc = make_host_kernel(k, X->dtype, true, &hk);
    if (rc) return rc;
    if (n == 0) return COVGRAM_OK;
    const size_t ts = dtype_size(X->dtype);
    const size_t obytes = (size_t)n * X->d * sizeof(double);
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
    rc = X->dtype == COVGRAM_F32 ? ig_run<float>(ctx, hk, X, Y, u_dev, ldu_d, a_dev, lda_d, nvec, o_dev)
                                 : ig_run<double>(ctx, hk, X, Y, u_dev, ldu_d, a_dev, lda_d, nvec, o_dev);
    if (rc) return rc;
    CG_CHECK_HIP(hipGetLastError());
    if (loc == COVGRAM_HOST) {
        CG_CHECK_HIP(hipMemcpyAsync(dX, o_dev, obytes, hipMemcpyDeviceToHost, ctx->stream));
        CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return COVGRAM_OK;
}
