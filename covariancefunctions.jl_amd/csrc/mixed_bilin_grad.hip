// mixed_bilin_grad.hip — covgram_bilinear_grad_mixed: every hyper-parameter derivative of the bilinear forms sum_t u_t' G a_t of a MIXED-TRAIT
// composite (the composite of covgram_mvm_mixed: a Sum of Products of factors psi_f = phi_f(z_f)^power_f, each on the argument of its own
// trait) in ONE fused pass over the n m pairs.  With W = U A' (rank nvec) formed per pair in registers:
//     out[t]      = sum_ij W_ij prod_{f in t} psi_f                              term t WITHOUT its coefficient c_t
//     out[8 + f]  = c_t sum_ij W_ij z_f dpsi_f/dz_f prod_{g != f} psi_g          isotropic factors, z_f = r^2 / l_f^2
//     out[16 + f] = c_t sum_ij W_ij dpsi_f/dtheta_f prod_{g != f} psi_g          RQ alpha, gamma-exponential gamma, IMQ c, NeuralNetwork sigma
// f: the flat index of the factor in the descriptor.  Every other entry is exactly 0.  fp32 and fp64 points; the results are fp64.
//
// Shape of the computation — the tiling of bg_pair_kernel (bilin_grad.hip):
//   * a workgroup (4 waves) owns BG_TI = 64 rows and a chunk of column tiles of 64 (fp32) or 32 (fp64) columns; lane r of every wave is row
//     r, wave w takes a quarter of each tile's columns: a GROUP of JPL = 16 (fp32) or 8 (fp64) pairs per lane and tile;
//   * LDS: the row tile's U (staged once), per column tile the points, the A-tile and s_j = |y_j|^2; q_i = |x_i|^2 is one register per lane.
//     Points wider than BG_DS = 16 dimensions pass through LDS in slabs of 16.  Per pair and dimension one subtract and two fmas (r^2, p);
//   * the interpreter is factor-outer over the group: for the factor f of a term that carries live outputs, L = prod_{g != f} psi_g is
//     multiplied up factor by factor (never a division: a Dot factor can be 0 or negative), then f's jet (psi, z dpsi/dz, dpsi/dtheta) is
//     evaluated once and serves up to three outputs.  Each factor's family is dispatched ONCE per group, its code unrolled over the group;
//   * only LIVE outputs have accumulators, one LDS word per lane and live output: the group's JPL products are added in registers and join
//     the lane's accumulator; after at most BG_L = 128 pairs the accumulators are added over the 64 lanes by a butterfly in the working
//     precision and lane k keeps the fp64 total of live output k.  At the end the four waves' totals are added in fp64 in wave order and
//     written to a slab; mbg_reduce_kernel adds the slab in a fixed order, multiplies by c_t in fp64 and writes out.  No atomics;
//   * where the live outputs' accumulators would not fit 64 KB of LDS beside the tiles (fp64, many columns of U), the live outputs are walked
//     in bounded chunks, one pass of the same kernel per chunk: W and the factors are recomputed identically.
#include "mixed_bilin_grad.hpp"

namespace covgram {

constexpr int MBG_THREADS = BG_TI * BG_WAVES;
constexpr size_t MBG_LDS_BUDGET = 64 * 1024 - BG_WAVES * MBG_NOUT * sizeof(double);   // dynamic LDS beside the static fp64 exchange

template <typename T>
struct MbgArgs {
    const T* X; const T* Y;          // points, point-major, stride d
    int64_t n, m;
    int32_t d, dpad;                 // dpad: d rounded up to a multiple of 4
    const T* U; int64_t ldu;         // n x nvec
    const T* A; int64_t lda;         // m x nvec
    int32_t nvec, nlive;             // nlive: accumulators of this pass
    int32_t slot_v[EXPR_MAXT];       // accumulator of out[t], -1: not in this pass
    int32_t slot_z[EXPR_MAXF];       // accumulator of the factor's z dpsi/dz output (index: the factor as the device keeps it), -1: none
    int32_t slot_p[EXPR_MAXF];       // accumulator of the factor's dpsi/dtheta output, -1: none
    T cpar[EXPR_MAXF];               // the factor's own param as the descriptor holds it (IMQ: c; f.param holds c^2)
    ExprParams<T> ep;                // families and parameter blocks (coef is applied by the reduction)
    double* slab;                    // [gridDim.y][gridDim.x][nlive]
    int64_t jchunk;                  // columns per blockIdx.y (a multiple of the tile width)
};

struct MbgMap {
    int32_t idx[MBG_NOUT];           // accumulator -> entry of out
    double scale[MBG_NOUT];          // 1 for out[t], c_t for the derivative outputs
};

template <typename T>
__device__ __forceinline__ T mbg_wave_sum(T x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// L[jj] *= psi_f on the group
template <int F, typename T, int JPL>
__device__ __forceinline__ void mbg_group_values(const KParams<T>& kq, const T (&r2)[JPL], const T (&p)[JPL], T q, const T* __restrict__ sj, T (&L)[JPL]) {
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) {
        const T s = F == COVGRAM_NEURALNETWORK ? sj[jj] : (T)0;
        L[jj] *= mbg_value<F, T>(mbg_argument<F, T>(kq, r2[jj], p[jj], q, s), kq);
        if ((jj & 3) == 3) __builtin_amdgcn_sched_barrier(0);     // four pairs in flight: the profile's temporaries stay bounded
    }
}

// the group's three sums of W L (psi, z dpsi/dz, dpsi/dtheta); a pair with W == 0 (rows / columns beyond the sets) adds nothing
template <int F, typename T, int JPL>
__device__ __forceinline__ void mbg_group_jet(const KParams<T>& kq, T cpar, const T (&r2)[JPL], const T (&p)[JPL], T q, const T* __restrict__ sj,
                                              const T (&w)[JPL], const T (&L)[JPL], T& av, T& az, T& ap) {
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) {
        const T s = F == COVGRAM_NEURALNETWORK ? sj[jj] : (T)0;
        T v, zd, dp;
        mbg_jet<F, T>(mbg_argument<F, T>(kq, r2[jj], p[jj], q, s), kq, cpar, p[jj], q, s, v, zd, dp);
        const bool zero = w[jj] == (T)0;
        const T wl = w[jj] * L[jj];
        av = cg_fma(wl, zero ? (T)0 : v, av);
        az = cg_fma(wl, zero ? (T)0 : zd, az);
        ap = cg_fma(wl, zero ? (T)0 : dp, ap);
        if ((jj & 3) == 3) __builtin_amdgcn_sched_barrier(0);     // four pairs in flight: the jet's temporaries stay bounded
    }
}

#define CG_MBG_FAMILIES(X)                                                                                                                   \
    X(COVGRAM_EQ) X(COVGRAM_EXP) X(COVGRAM_RQ) X(COVGRAM_GAMMAEXP) X(COVGRAM_CAUCHY) X(COVGRAM_IMQ) X(COVGRAM_MATERNP) X(COVGRAM_DOT)        \
    X(COVGRAM_EXPDOT) X(COVGRAM_ASINDOT) X(COVGRAM_NEURALNETWORK)

template <typename T>
__global__ __launch_bounds__(MBG_THREADS) void mbg_pair_kernel(const MbgArgs<T> g) {
    constexpr int JPL = bg_jpl<T>, TJ = JPL * BG_WAVES, KT = BG_L / JPL;
    extern __shared__ __align__(32) unsigned char mbg_lds[];
    __shared__ double red[BG_WAVES][MBG_NOUT];
    using V4 = T __attribute__((ext_vector_type(4)));
    const int ds_w = g.dpad < BG_DS ? g.dpad : BG_DS;              // slab width in LDS (a multiple of 4)
    const int xs_w = ((ds_w >> 2) & 1) ? ds_w : ds_w + 4;         // row stride: an odd number of 16-byte groups
    const int nslab = (g.dpad + BG_DS - 1) / BG_DS;
    T* xs = (T*)mbg_lds;                                           // [BG_TI][xs_w]
    T* ys = xs + BG_TI * xs_w;                                     // [TJ][ds_w]
    T* us = ys + TJ * ds_w;                                        // [nvec][BG_TI]
    T* as = us + g.nvec * BG_TI;                                   // [nvec][TJ]
    T* ss = as + g.nvec * TJ;                                      // [TJ]: |y_j|^2
    T* acc = ss + TJ;                                              // [nlive][MBG_THREADS]
    static_assert(JPL % 4 == 0 && BG_L % JPL == 0, "128-bit broadcast reads of as; whole tiles per hand-off");
    const int tid = threadIdx.x, r = tid & 63, wv = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * BG_TI;
    const int64_t j0 = (int64_t)blockIdx.y * g.jchunk;
    const int64_t j1 = j0 + g.jchunk < g.m ? j0 + g.jchunk : g.m;
    double tot = 0.0;                                              // lane k of a wave: live output k
    // one slab of a point tile: rows beyond the set and dimensions beyond d are zeros
    auto stage_points = [&](T* dst, int stride, int rows, const T* P, int64_t p0, int64_t pn, int c0) {
        for (int e = tid; e < rows * ds_w; e += MBG_THREADS) {
            const int pp = e / ds_w, k = e % ds_w;
            const int64_t pt = p0 + pp;
            dst[pp * stride + k] = (pt < pn && c0 + k < g.d) ? P[pt * g.d + c0 + k] : (T)0;
        }
    };
    for (int e = tid; e < g.nvec * BG_TI; e += MBG_THREADS) {
        const int vv = e / BG_TI, rr = e % BG_TI;
        us[e] = i0 + rr < g.n ? g.U[(i0 + rr) + (int64_t)vv * g.ldu] : (T)0;
    }
    for (int k = 0; k < g.nlive; ++k) acc[k * MBG_THREADS + tid] = (T)0;
    if (nslab == 1) stage_points(xs, xs_w, BG_TI, g.X, i0, g.n, 0);
    T q = (T)0;                                                    // |x_i|^2, dimensions ascending; 0 beyond the set
    if (i0 + r < g.n) {
        const T* xr = g.X + (i0 + r) * (int64_t)g.d;
        for (int c = 0; c < g.d; ++c) q = cg_fma(xr[c], xr[c], q);
    }

    int held = 0;                                                  // tiles in the lane's accumulators
    for (int64_t jt = j0; jt < j1; jt += TJ) {
        __syncthreads();                                           // the previous tile has been consumed
        for (int e = tid; e < g.nvec * TJ; e += MBG_THREADS) {
            const int vv = e / TJ, jj = e % TJ;
            as[e] = jt + jj < j1 ? g.A[(jt + jj) + (int64_t)vv * g.lda] : (T)0;
        }
        if (tid < TJ) {
            T s = (T)0;
            if (jt + tid < j1) {
                const T* yr = g.Y + (jt + tid) * (int64_t)g.d;
                for (int c = 0; c < g.d; ++c) s = cg_fma(yr[c], yr[c], s);
            }
            ss[tid] = s;
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
            for (int c = 0; c < JPL / 4; ++c) {
                const V4 av = a4[c];
                w[4 * c + 0] = cg_fma(uv, av.x, w[4 * c + 0]);
                w[4 * c + 1] = cg_fma(uv, av.y, w[4 * c + 1]);
                w[4 * c + 2] = cg_fma(uv, av.z, w[4 * c + 2]);
                w[4 * c + 3] = cg_fma(uv, av.w, w[4 * c + 3]);
            }
        }
        // r^2 by direct differences and p = x . y, dimensions ascending
        T r2[JPL], p[JPL];
#pragma unroll
        for (int jj = 0; jj < JPL; ++jj) { r2[jj] = (T)0; p[jj] = (T)0; }
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
                    r2[jj] = cg_fma(df.w, df.w, cg_fma(df.z, df.z, cg_fma(df.y, df.y, cg_fma(df.x, df.x, r2[jj]))));
                    p[jj] = cg_fma(xv.w, yv.w, cg_fma(xv.z, yv.z, cg_fma(xv.y, yv.y, cg_fma(xv.x, yv.x, p[jj]))));
                }
            }
        }
        // the interpreter: terms, then the factors that carry live outputs
        const T* sj = ss + wv * JPL;
        T* mine = acc + tid;
        int fi0 = 0;
        for (int t = 0; t < g.ep.nterms; ++t) {
            const int nf = g.ep.nfac[t];
            const int sv = g.slot_v[t];
            if (nf == 0 && sv >= 0) {                              // a term of constants only: sum W
                T a = (T)0;
#pragma unroll
                for (int jj = 0; jj < JPL; ++jj) a += w[jj];
                mine[sv * MBG_THREADS] += a;
            }
            for (int f = 0; f < nf; ++f) {
                const int fi = fi0 + f;
                const int svf = f == 0 ? sv : -1, sz = g.slot_z[fi], sp = g.slot_p[fi];
                if (svf < 0 && sz < 0 && sp < 0) continue;
                T L[JPL];
#pragma unroll
                for (int jj = 0; jj < JPL; ++jj) L[jj] = (T)1;
                for (int o = 0; o < nf; ++o) {
                    if (o == f) continue;
                    const KParams<T>& kq = g.ep.f[fi0 + o];
                    switch (g.ep.fam[fi0 + o]) {
#define CG_MBG_CASE(F) case F: mbg_group_values<F, T, JPL>(kq, r2, p, q, sj, L); break;
                        CG_MBG_FAMILIES(CG_MBG_CASE)
#undef CG_MBG_CASE
                        default: break;
                    }
                }
                T av = (T)0, az = (T)0, ap = (T)0;
                const KParams<T>& kq = g.ep.f[fi];
                const T cpar = g.cpar[fi];
                switch (g.ep.fam[fi]) {
#define CG_MBG_CASE(F) case F: mbg_group_jet<F, T, JPL>(kq, cpar, r2, p, q, sj, w, L, av, az, ap); break;
                    CG_MBG_FAMILIES(CG_MBG_CASE)
#undef CG_MBG_CASE
                    default: break;
                }
                if (svf >= 0) mine[svf * MBG_THREADS] += av;
                if (sz >= 0) mine[sz * MBG_THREADS] += az;
                if (sp >= 0) mine[sp * MBG_THREADS] += ap;
            }
            fi0 += nf;
        }
        if (++held == KT || jt + TJ >= j1) {                       // hand-off: at most BG_L pairs per lane
            for (int k = 0; k < g.nlive; ++k) {
                const T sum = mbg_wave_sum(mine[k * MBG_THREADS]);
                mine[k * MBG_THREADS] = (T)0;
                if (r == k) tot += (double)sum;
            }
            held = 0;
        }
    }
    if (r < MBG_NOUT) red[wv][r] = tot;
    __syncthreads();
    if (tid < g.nlive) {
        double t = red[0][tid];
#pragma unroll
        for (int c = 1; c < BG_WAVES; ++c) t += red[c][tid];
        g.slab[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * g.nlive + tid] = t;
    }
}

// out[idx[k]] <- scale[k] * (sum over the slab's nblk rows): 256 strided partial sums per output, then a tree in LDS — a fixed order
__global__ __launch_bounds__(256) void mbg_reduce_kernel(const double* __restrict__ slab, int64_t nblk, int nlive, const MbgMap map, double* __restrict__ out) {
    __shared__ double part[256];
    const int k = blockIdx.x, t = threadIdx.x;
    double sum = 0.0;
    for (int64_t b = t; b < nblk; b += 256) sum += slab[b * nlive + k];
    part[t] = sum;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) part[t] += part[t + h];
        __syncthreads();
    }
    if (t == 0) out[map.idx[k]] = map.scale[k] * part[0];
}

// option "jsplit" > 0 fixes the number of column chunks (tests); otherwise bg_column_split
template <typename T>
static int64_t mbg_column_split(const covgram_ctx* ctx, int64_t rowtiles, int64_t m, int64_t* jchunk) {
    if (ctx->jsplit <= 0) return bg_column_split<T>(ctx, rowtiles, m, jchunk);
    constexpr int TJ = bg_jpl<T> * BG_WAVES;
    const int64_t ntiles = (m + TJ - 1) / TJ;
    int64_t jsplit = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(ctx->jsplit, ntiles), 65535));
    const int64_t tiles_per = (ntiles + jsplit - 1) / jsplit;
    jsplit = (ntiles + tiles_per - 1) / tiles_per;
    *jchunk = tiles_per * TJ;
    return jsplit;
}

// one live output: its entry of out, its scale, and where the kernel finds its accumulator index
struct MbgLive { int idx; double scale; int kind, which; };      // kind 0: slot_v[which], 1: slot_z[which], 2: slot_p[which]

template <typename T>
static int mbg_run(covgram_ctx* ctx, const HostKernel& hk, const double* cpar, const MbgLive* live, int nlive, const covgram_points* X,
                   const covgram_points* Y, const void* U, int64_t ldu, const void* A, int64_t lda, int nvec, double* out_dev) {
    const int64_t n = X->n, m = Y->n;
    const int d = X->d;
    MbgArgs<T> g;
    memset(&g, 0, sizeof(g));
    g.X = (const T*)X->dptr; g.Y = (const T*)Y->dptr; g.n = n; g.m = m; g.d = d; g.dpad = (d + 3) & ~3;
    g.U = (const T*)U; g.ldu = ldu; g.A = (const T*)A; g.lda = lda; g.nvec = nvec;
    g.ep = make_params<FAM_EXPR_DOT, T>(hk);
    for (int f = 0; f < EXPR_MAXF; ++f) g.cpar[f] = (T)cpar[f];
    constexpr int TJ = bg_jpl<T> * BG_WAVES;
    const int64_t rowtiles = (n + BG_TI - 1) / BG_TI;
    const int64_t jsplit = mbg_column_split<T>(ctx, rowtiles, m, &g.jchunk);
    CG_REQUIRE(rowtiles <= 0x7fffffff, COVGRAM_EUNSUPPORTED, "bilinear_grad_mixed: n = %lld exceeds the grid", (long long)n);
    const int64_t nblk = rowtiles * jsplit;
    const int ds_w = std::min<int>(g.dpad, BG_DS);
    const int xs_w = ((ds_w >> 2) & 1) ? ds_w : ds_w + 4;
    const size_t base = ((size_t)BG_TI * xs_w + (size_t)TJ * ds_w + (size_t)nvec * (BG_TI + TJ) + TJ) * sizeof(T);
    const int per_pass = (int)std::min<size_t>((MBG_LDS_BUDGET - base) / (MBG_THREADS * sizeof(T)), (size_t)MBG_NOUT);
    CG_REQUIRE(per_pass >= 1, COVGRAM_EUNSUPPORTED, "bilinear_grad_mixed: the tiles leave no LDS for an accumulator");
    void* slab;
    int rc = ws_reserve(ctx, 1, (size_t)nblk * std::min(nlive, per_pass) * sizeof(double), &slab);
    if (rc) return rc;
    g.slab = (double*)slab;
    TimerScope tm(ctx);
    for (int l0 = 0; l0 < nlive; l0 += per_pass) {                // the live outputs in bounded chunks: one pass each
        const int nl = std::min(per_pass, nlive - l0);
        MbgMap map;
        memset(&map, 0, sizeof(map));
        for (int t = 0; t < EXPR_MAXT; ++t) g.slot_v[t] = -1;
        for (int f = 0; f < EXPR_MAXF; ++f) { g.slot_z[f] = -1; g.slot_p[f] = -1; }
        for (int k = 0; k < nl; ++k) {
            const MbgLive& lv = live[l0 + k];
            (lv.kind == 0 ? g.slot_v : (lv.kind == 1 ? g.slot_z : g.slot_p))[lv.which] = k;
            map.idx[k] = lv.idx; map.scale[k] = lv.scale;
        }
        g.nlive = nl;
        const size_t lds = base + (size_t)nl * MBG_THREADS * sizeof(T);
        hipLaunchKernelGGL((mbg_pair_kernel<T>), dim3((unsigned)rowtiles, (unsigned)jsplit), dim3(MBG_THREADS), lds, ctx->stream, g);
        hipLaunchKernelGGL(mbg_reduce_kernel, dim3((unsigned)nl), dim3(256), 0, ctx->stream, (const double*)slab, nblk, nl, map, out_dev);
    }
    return COVGRAM_OK;
}

}  // namespace covgram

using namespace covgram;

extern "C" int covgram_bilinear_grad_mixed(covgram_ctx* ctx, const covgram_kernel_composite* k, const covgram_points* X, const covgram_points* Y, const void* U,
                                           int64_t ldu, const void* A, int64_t lda, int32_t nvec, double* out, int32_t loc) {
    const char* fn = "bilinear_grad_mixed";
    CG_REQUIRE(ctx && k && X, COVGRAM_EINVAL, "NULL argument");
    HostKernel hk;                                                 // the kernel's own refusals come first (host work only)
    int rc = make_composite_kernel(k, X->dtype, COMPOSITE_MIXED_PARAMETERS, &hk);
    if (rc) return rc;
    if (!Y) Y = X;
    CG_REQUIRE(X->ctx == ctx && Y->ctx == ctx, COVGRAM_EINVAL, "points belong to a different ctx");
    CG_REQUIRE(X->dtype == Y->dtype, COVGRAM_EINVAL, "X and Y have different dtypes");
    CG_REQUIRE(X->d == Y->d, COVGRAM_EINVAL, "DimensionMismatch: inputs have to have the same length (%d and %d)", X->d, Y->d);
    CG_REQUIRE(loc == COVGRAM_HOST || loc == COVGRAM_DEVICE, COVGRAM_EINVAL, "unknown loc %d", loc);
    CG_REQUIRE(nvec >= 1 && nvec <= BG_MAX_NVEC, COVGRAM_EINVAL, "%s: nvec = %d is outside 1 .. %d", fn, nvec, BG_MAX_NVEC);
    CG_REQUIRE(X->d >= 1 && X->d <= BG_MAX_D, COVGRAM_EINVAL, "%s: d = %d is outside 1 .. %d", fn, X->d, BG_MAX_D);
    CG_REQUIRE(out != nullptr, COVGRAM_EINVAL, "out is NULL");
    const int64_t n = X->n, m = Y->n;
    CG_REQUIRE(ldu >= n && lda >= m, COVGRAM_EINVAL, "DimensionMismatch: ldu=%lld < n=%lld or lda=%lld < m=%lld", (long long)ldu, (long long)n,
               (long long)lda, (long long)m);
    CG_REQUIRE((U != nullptr || n == 0) && (A != nullptr || m == 0), COVGRAM_EINVAL, "U or A is NULL");

    // the live outputs, from the families: out[t] of every term; z dpsi/dz of the isotropic factors; dpsi/dtheta of the factors with a parameter
    MbgLive live[MBG_NOUT];
    double cpar[EXPR_MAXF] = {0};
    int nlive = 0, nin = 0, nf = 0;
    for (int t = 0; t < k->nterms; ++t) {
        const double ct = k->head.scale * hk.coef[t];
        live[nlive++] = {t, 1.0, 0, t};
        for (int f = 0; f < k->nfactors[t]; ++f, ++nin) {
            const covgram_kernel& fk = k->factors[nin];
            if (fk.family == COVGRAM_CONSTANT) continue;           // folded into c_t; make_composite_kernel keeps no block for it
            cpar[nf] = fk.param;
            if (fk.family != COVGRAM_NEURALNETWORK && !mbg_dot_family(fk.family)) live[nlive++] = {MBG_Z0 + nin, ct, 1, nf};
            if (mbg_has_param(fk.family)) live[nlive++] = {MBG_P0 + nin, ct, 2, nf};
            ++nf;
        }
    }
    CG_DEVICE(ctx);
    const size_t ts = dtype_size(X->dtype);
    if (n == 0 || m == 0) {                                        // an empty sum
        if (loc == COVGRAM_HOST) memset(out, 0, MBG_NOUT * sizeof(double));
        else CG_CHECK_HIP(hipMemsetAsync(out, 0, MBG_NOUT * sizeof(double), ctx->stream));
        return COVGRAM_OK;
    }
    const void* u_dev = U; const void* a_dev = A;
    double* o_dev = out;
    int64_t ldu_d = ldu, lda_d = lda;
    if (loc == COVGRAM_HOST) {
        void* so;
        rc = bg_stage_weights(ctx, n, m, nvec, ts, &u_dev, &ldu_d, &a_dev, &lda_d); if (rc) return rc;
        rc = ws_reserve(ctx, 3, (size_t)MBG_NOUT * sizeof(double), &so); if (rc) return rc;
        o_dev = (double*)so;
    }
    CG_CHECK_HIP(hipMemsetAsync(o_dev, 0, MBG_NOUT * sizeof(double), ctx->stream));   // the dead outputs: exact zeros
    rc = X->dtype == COVGRAM_F32 ? mbg_run<float>(ctx, hk, cpar, live, nlive, X, Y, u_dev, ldu_d, a_dev, lda_d, nvec, o_dev)
                                 : mbg_run<double>(ctx, hk, cpar, live, nlive, X, Y, u_dev, ldu_d, a_dev, lda_d, nvec, o_dev);
    if (rc) return rc;
    CG_CHECK_HIP(hipGetLastError());
    if (loc == COVGRAM_HOST) {
        CG_CHECK_HIP(hipMemcpyAsync(out, o_dev, MBG_NOUT * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return COVGRAM_OK;
}
