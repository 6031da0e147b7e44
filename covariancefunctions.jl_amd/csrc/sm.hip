// sm.hip — SpectralMixture Gramians (src/stationary.jl:213-217): one fused pass for
//     G_ij = sum_q w_q cos(2 pi mu_q . (x_i - y_j)) exp(-1/2 sum_k ((x_ik - y_jk) / l_qk)^2)
// behind the covgram_sm_* handle of include/covgram.h: the product y <- alpha G a + beta y and Matrix(G), fp32 and fp64.
//
// Shape of the computation ("SpectralMixture"):
//   * sm_phase_kernel (O((n + m) Q d), once per call): the phases in revolutions u_qi = mu_q . x_i, v_qj = mu_q . y_j, accumulated in fp64
//     for both dtypes, reduced to [-1/2, 1/2] exactly (u - rint(u)) and turned into cos / sin by sincospi.  The row side keeps
//     (cos u, sin u), the column side (w_q cos v, w_q sin v), so that cos(2 pi (u - v)) w_q = cos u (w cos v) + sin u (w sin v) costs the
//     pair loop one multiplication and one fma and no trigonometric instruction;
//   * sm_pair_kernel: one thread per row, x_i in registers; the columns go through LDS in tiles of SM_TJ (coordinates, the column's
//     2 Q phase factors and, for a product, its right-hand sides).  The Q components are walked in chunks of SM_QC = 4, the chunk loop
//     OUTSIDE the column loop: a thread holds the row phases of one chunk (8 registers) whatever Q is, and Q <= 4 — the shapes the family
//     is used at — is exactly one chunk, compiled for its own count (QN = 1 .. 4).  Per pair the squared coordinate differences are formed once (direct differences, never the
//     expanded |x|^2 + |y|^2 - 2 x.y) and shared by the chunk's components; per component: t = sum_k c_qk d2_k with
//     c_qk = log2(e) / (2 l_qk^2) (ISO: one multiplication of the shared |x - y|^2), e = exp2(-t), and the two fmas above.
//     The value sum_q ... is then multiplied into up to four right-hand sides (NR) or stored (NR == 0: Matrix(G));
//   * small n: the columns are split over blockIdx.y, the partial sums go to a slab that sm_reduce_kernel adds in a fixed order
//     (no atomics: bit-identical from run to run).
#include <algorithm>
#include <cmath>

#include "profiles.hpp"
#include "sm_common.hpp"

// the column loop asks for two pairs per trip; where the body is too large for that (wide points) the request is dropped, silently
#pragma clang diagnostic ignored "-Wpass-failed"

namespace covgram {

constexpr int SM_ROWS = 256;   // rows (threads) per workgroup
constexpr int SM_TJ = 32;      // columns per LDS tile

template <typename T>
struct SmArgs {
    const T* X; const T* Y;          // points, point-major, stride d
    int64_t n, m;
    int32_t d, ncomp, nch;           // nch = ceil(ncomp / SM_QC)
    const T* RS;                     // row phases   [nch][2 SM_QC][n]: cos u then sin u of the chunk's components
    const T* CS;                     // column phases [m][nch][2 SM_QC]: w cos v then w sin v
    const T* coef;                   // [nch SM_QC][SM_CST]: log2(e) / (2 l_qk^2), zero beyond d and beyond ncomp
    const T* ciso;                   // [nch SM_QC]: the same for one lengthscale per component (ISO)
    const T* a; int64_t lda; int32_t nr;   // right-hand sides of this launch (nr <= NR)
    T* out; int64_t ldo;             // product: y (direct) or the slab [jsplit][nr][n]; Matrix(G): the n x m matrix
    int64_t jchunk;                  // columns per blockIdx.y (a multiple of SM_TJ)
    int32_t direct;                  // product: 1 = one column chunk, y written here with alpha and beta
    T alpha, beta;
};

// NR >= 1: out <- the product's rows (direct) or partial sums (slab); NR == 0: Matrix(G).  QN: components evaluated per chunk — the
// mixture's own count when it has at most SM_QC (one chunk, nothing padded), otherwise SM_QC (the last chunk's padding has zero phase
// factors and zero coefficients: exp2(-0) * 0 adds an exact zero).  No branch and no load from global memory inside the column loop.
template <typename T, int DM, bool ISO, int NR, int QN>
__global__ __launch_bounds__(SM_ROWS) void sm_pair_kernel(const SmArgs<T> g) {
    extern __shared__ __align__(16) unsigned char sm_lds[];
    constexpr int NRS = NR > 0 ? NR : 1;
    constexpr int NCF = ISO ? 1 : DM;                             // coefficients per component
    const int csw = g.nch * 2 * SM_QC;                            // phase factors per column
    T* ys = (T*)sm_lds;                                            // [SM_TJ][DM]
    T* cs = ys + SM_TJ * DM;                                       // [SM_TJ][csw]
    T* as = cs + SM_TJ * csw;                                      // [SM_TJ][NR]
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * SM_ROWS + tid;
    const bool live = i < g.n;
    const int64_t ic = live ? i : g.n - 1;
    T x[DM];
#pragma unroll
    for (int k = 0; k < DM; ++k) x[k] = k < g.d ? g.X[ic * g.d + k] : (T)0;
    T acc[NRS];
#pragma unroll
    for (int r = 0; r < NRS; ++r) acc[r] = (T)0;
    const int64_t j0 = (int64_t)blockIdx.y * g.jchunk;
    const int64_t j1 = j0 + g.jchunk < g.m ? j0 + g.jchunk : g.m;

    for (int64_t jt = j0; jt < j1; jt += SM_TJ) {
        const int jn = (int)(j1 - jt < SM_TJ ? j1 - jt : SM_TJ);
        __syncthreads();                                           // the previous tile has been consumed
        for (int e = tid; e < jn * DM; e += SM_ROWS) {
            const int jj = e / DM, k = e % DM;
            ys[e] = k < g.d ? g.Y[(jt + jj) * g.d + k] : (T)0;
        }
        for (int e = tid; e < jn * csw; e += SM_ROWS) cs[e] = g.CS[jt * csw + e];
        if constexpr (NR > 0) {
            for (int e = tid; e < jn * NR; e += SM_ROWS) {
                const int jj = e / NR, r = e % NR;
                as[e] = r < g.nr ? g.a[(jt + jj) + (int64_t)r * g.lda] : (T)0;
            }
        }
        __syncthreads();
        for (int c = 0; c < g.nch; ++c) {
            // the chunk's row phases and coefficients, in registers for the whole tile
            T cx[QN], sx[QN], cf[QN][NCF];
#pragma unroll
            for (int q = 0; q < QN; ++q) {
                cx[q] = g.RS[(int64_t)(c * 2 * SM_QC + q) * g.n + ic];
                sx[q] = g.RS[(int64_t)(c * 2 * SM_QC + SM_QC + q) * g.n + ic];
                if constexpr (ISO) {
                    cf[q][0] = g.ciso[c * SM_QC + q];             // uniform addresses
                } else {
#pragma unroll
                    for (int k = 0; k < DM; ++k) cf[q][k] = g.coef[(c * SM_QC + q) * SM_CST + k];
                }
            }
            const T* __restrict__ cc = cs + c * 2 * SM_QC;
#pragma unroll 2
            for (int jj = 0; jj < jn; ++jj) {
                T d2[DM];
                T s = (T)0;
#pragma unroll
                for (int k = 0; k < DM; ++k) {
                    const T r = x[k] - ys[jj * DM + k];
                    d2[k] = r * r;
                    if constexpr (ISO) s = fma_t(r, r, s);
                }
                T cw[QN], sw[QN];
#pragma unroll
                for (int q = 0; q < QN; ++q) { cw[q] = cc[jj * csw + q]; sw[q] = cc[jj * csw + SM_QC + q]; }
                // fp32: v_exp_f32 flushes results below 2^-126, but w cos(..) may lift such a term back into the normal range: the
                // exponent is biased by 32 (inside the first fma, free) and the pair's sum scaled back once
                constexpr T bias = sizeof(T) == 4 ? (T)-32 : (T)0;
                T v = (T)0;
#pragma unroll
                for (int q = 0; q < QN; ++q) {
                    T t;
                    if constexpr (ISO) {
                        t = fma_t(cf[q][0], s, bias);
                    } else {
                        t = fma_t(cf[q][0], d2[0], bias);
#pragma unroll
                        for (int k = 1; k < DM; ++k) t = fma_t(cf[q][k], d2[k], t);
                    }
                    const T e = exp2_neg_tab(t);
                    const T ph = fma_t(cx[q], cw[q], sx[q] * sw[q]);
                    v = fma_t(e, ph, v);
                }
                if constexpr (sizeof(T) == 4) v *= (T)0x1p-32;
                if constexpr (NR > 0) {
#pragma unroll
                    for (int r = 0; r < NR; ++r) acc[r] = fma_t(v, as[jj * NR + r], acc[r]);
                } else {
                    if (live) {
                        T* o = g.out + i + (jt + jj) * g.ldo;
                        *o = c == 0 ? v : *o + v;                  // later chunks add to what this thread stored
                    }
                }
            }
        }
    }
    if constexpr (NR > 0) {
        if (live) {
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if (r < g.nr) {
                    if (g.direct) {
                        T* yp = g.out + i + (int64_t)r * g.ldo;
                        *yp = (g.beta == (T)0) ? g.alpha * acc[r] : fma_t(g.alpha, acc[r], g.beta * *yp);   // beta == 0: y is never read
                    } else {
                        g.out[((int64_t)blockIdx.y * g.nr + r) * g.n + i] = acc[r];
                    }
                }
        }
    }
}

// y[i + r ldy] <- alpha sum_s slab[s][r][i] + beta y[i + r ldy], s ascending
template <typename T>
__global__ __launch_bounds__(256) void sm_reduce_kernel(const T* __restrict__ slab, int jsplit, int nr, int64_t n, T* __restrict__ y, int64_t ldy, T alpha,
                                                        T beta) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y;
    if (i >= n) return;
    T sum = (T)0;
    for (int s = 0; s < jsplit; ++s) sum += slab[((int64_t)s * nr + r) * n + i];
    T* yp = y + i + (int64_t)r * ldy;
    *yp = (beta == (T)0) ? alpha * sum : fma_t(alpha, sum, beta * *yp);
}

// y <- beta y (an empty column set)
template <typename T>
__global__ __launch_bounds__(256) void sm_scale_kernel(T* __restrict__ y, int64_t n, int64_t ldy, T beta) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    T* yp = y + i + (int64_t)blockIdx.y * ldy;
    *yp = (beta == (T)0) ? (T)0 : beta * *yp;
}

}  // namespace covgram

namespace covgram {

static int sm_dm(int d) { return d <= 1 ? 1 : (d <= 4 ? 4 : (d <= 8 ? 8 : 16)); }

template <typename T, int NR, int QN>
static void sm_launch_pairs_q(const covgram_sm* S, const SmArgs<T>& g, dim3 grid, hipStream_t stream) {
    const int dm = sm_dm(S->d);
    const size_t lds = (size_t)SM_TJ * (dm + g.nch * 2 * SM_QC + NR) * sizeof(T);
#define CG_SM(DMV, ISOV) hipLaunchKernelGGL((sm_pair_kernel<T, DMV, ISOV, NR, QN>), grid, dim3(SM_ROWS), lds, stream, g)
    if (dm == 1) CG_SM(1, false);                                  // one dimension: the two forms coincide
    else if (S->isotropic) { if (dm == 4) CG_SM(4, true); else if (dm == 8) CG_SM(8, true); else CG_SM(16, true); }
    else { if (dm == 4) CG_SM(4, false); else if (dm == 8) CG_SM(8, false); else CG_SM(16, false); }
#undef CG_SM
}

template <typename T, int NR>
static void sm_launch_pairs(const covgram_sm* S, const SmArgs<T>& g, dim3 grid, hipStream_t stream) {
    switch (S->ncomp) {                                            // up to SM_QC components: exactly one chunk of that many
        case 1: sm_launch_pairs_q<T, NR, 1>(S, g, grid, stream); break;
        case 2: sm_launch_pairs_q<T, NR, 2>(S, g, grid, stream); break;
        case 3: sm_launch_pairs_q<T, NR, 3>(S, g, grid, stream); break;
        default: sm_launch_pairs_q<T, NR, SM_QC>(S, g, grid, stream); break;
    }
}

template <typename T>
static SmArgs<T> sm_args(const covgram_sm* S, const covgram_points* X, const covgram_points* Y, const void* RS, const void* CS) {
    SmArgs<T> g;
    memset(&g, 0, sizeof(g));
    const int qpad = S->nch * SM_QC;
    const T* prm = (const T*)S->prm;
    g.X = (const T*)X->dptr; g.Y = (const T*)Y->dptr; g.n = X->n; g.m = Y->n;
    g.d = S->d; g.ncomp = S->ncomp; g.nch = S->nch;
    g.RS = (const T*)RS; g.CS = (const T*)CS;
    g.coef = prm + qpad + (size_t)qpad * S->d;
    g.ciso = g.coef + (size_t)qpad * SM_CST;
    return g;
}

// the phase tables of (X, Y) in workspace slot 0
template <typename T>
static int sm_phases(const covgram_sm* S, const covgram_points* X, const covgram_points* Y, void** RS, void** CS) {
    covgram_ctx* ctx = S->ctx;
    const int64_t n = X->n, m = Y->n;
    const int qpad = S->nch * SM_QC;
    const size_t rs_bytes = (((size_t)n * 2 * qpad * sizeof(T)) + 255) & ~(size_t)255;
    void* w;
    int rc = ws_reserve(ctx, 0, rs_bytes + (size_t)m * 2 * qpad * sizeof(T), &w);
    if (rc) return rc;
    *RS = w; *CS = (char*)w + rs_bytes;
    const T* prm = (const T*)S->prm;
    const int64_t threads = (n + m) * qpad;
    hipLaunchKernelGGL((sm_phase_kernel<T>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)X->dptr, n, (const T*)Y->dptr, m,
                       (int)S->d, (int)S->ncomp, (int)S->nch, prm, prm + qpad, (T*)*RS, (T*)*CS);
    return COVGRAM_OK;
}

template <typename T>
static int sm_mvm_t(covgram_sm* S, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda, void* y, int64_t ldy, int nrhs, double alpha,
                    double beta) {
    covgram_ctx* ctx = S->ctx;
    const int64_t n = X->n, m = Y->n;
    void *RS, *CS;
    int rc = sm_phases<T>(S, X, Y, &RS, &CS);
    if (rc) return rc;
    // column split: enough workgroups for every CU, chunks of at least four tiles
    const int64_t rowblocks = (n + SM_ROWS - 1) / SM_ROWS;
    const int64_t ntiles = (m + SM_TJ - 1) / SM_TJ;
    const int64_t target = (int64_t)ctx->num_cus * 4;
    int64_t jsplit = std::min<int64_t>((target + rowblocks - 1) / rowblocks, std::max<int64_t>(1, ntiles / 4));
    jsplit = std::max<int64_t>(1, std::min<int64_t>(jsplit, 64));
    const int64_t jchunk = ((ntiles + jsplit - 1) / jsplit) * SM_TJ;
    jsplit = (m + jchunk - 1) / jchunk;
    void* slab = nullptr;
    if (jsplit > 1) {
        rc = ws_reserve(ctx, 1, (size_t)jsplit * std::min(nrhs, 4) * n * sizeof(T), &slab);
        if (rc) return rc;
    }
    SmArgs<T> g = sm_args<T>(S, X, Y, RS, CS);
    g.jchunk = jchunk; g.direct = jsplit == 1 ? 1 : 0;
    g.alpha = (T)alpha; g.beta = (T)beta;
    const dim3 grid((unsigned)rowblocks, (unsigned)jsplit);
    TimerScope tm(ctx);
    for (int c0 = 0; c0 < nrhs; c0 += 4) {                        // four right-hand sides share one pass over the pairs
        const int nr = std::min(4, nrhs - c0);
        T* yc = (T*)y + (size_t)c0 * ldy;
        g.a = (const T*)a + (size_t)c0 * lda; g.lda = lda; g.nr = nr;
        g.out = jsplit == 1 ? yc : (T*)slab; g.ldo = ldy;
        if (nr == 1) sm_launch_pairs<T, 1>(S, g, grid, ctx->stream);
        else sm_launch_pairs<T, 4>(S, g, grid, ctx->stream);
        if (jsplit > 1)
            hipLaunchKernelGGL((sm_reduce_kernel<T>), dim3((unsigned)((n + 255) / 256), (unsigned)nr), dim3(256), 0, ctx->stream, (const T*)slab, (int)jsplit, nr, n,
                               yc, ldy, (T)alpha, (T)beta);
    }
    return COVGRAM_OK;
}

template <typename T>
static int sm_matrix_t(covgram_sm* S, const covgram_points* X, const covgram_points* Y, void* out, int64_t ldo) {
    covgram_ctx* ctx = S->ctx;
    const int64_t n = X->n, m = Y->n;
    void *RS, *CS;
    int rc = sm_phases<T>(S, X, Y, &RS, &CS);
    if (rc) return rc;
    SmArgs<T> g = sm_args<T>(S, X, Y, RS, CS);
    int64_t jchunk = 8 * SM_TJ;                                    // 256-column strips; longer ones when the grid's y extent would not hold them
    while ((m + jchunk - 1) / jchunk > 65535) jchunk *= 2;
    g.jchunk = jchunk; g.out = (T*)out; g.ldo = ldo;
    const dim3 grid((unsigned)((n + SM_ROWS - 1) / SM_ROWS), (unsigned)((m + jchunk - 1) / jchunk));
    TimerScope tm(ctx);
    sm_launch_pairs<T, 0>(S, g, grid, ctx->stream);
    return COVGRAM_OK;
}

}  // namespace covgram

using namespace covgram;

extern "C" {

int covgram_sm_create(covgram_ctx* ctx, covgram_sm** out, int32_t ncomp, int32_t d, const double* w, const double* mu, const double* inv_l,
                      int32_t dtype) {
    CG_REQUIRE(ctx && out, COVGRAM_EINVAL, "NULL argument");
    CG_REQUIRE(dtype == COVGRAM_F32 || dtype == COVGRAM_F64, COVGRAM_EINVAL, "unknown dtype %d", dtype);
    CG_REQUIRE(ncomp >= 1 && d >= 1, COVGRAM_EINVAL, "SpectralMixture: ncomp = %d and d = %d must be >= 1", ncomp, d);
    CG_REQUIRE(ncomp <= COVGRAM_SM_MAX_COMPONENTS && d <= COVGRAM_SM_MAX_D, COVGRAM_EUNSUPPORTED,
               "SpectralMixture: ncomp = %d, d = %d exceed the compiled limits of %d components and %d dimensions", ncomp, d,
               COVGRAM_SM_MAX_COMPONENTS, COVGRAM_SM_MAX_D);
    CG_REQUIRE(w && mu && inv_l, COVGRAM_EINVAL, "NULL parameter array");
    for (int q = 0; q < ncomp; ++q) {
        CG_REQUIRE(std::isfinite(w[q]), COVGRAM_EINVAL, "SpectralMixture: weight %d is not finite", q);
        for (int k = 0; k < d; ++k) {
            CG_REQUIRE(std::isfinite(mu[q * d + k]) && std::isfinite(inv_l[q * d + k]), COVGRAM_EINVAL, "SpectralMixture: parameter (%d, %d) is not finite", q, k);
            CG_REQUIRE(inv_l[q * d + k] >= 0, COVGRAM_EINVAL, "SpectralMixture: inverse lengthscale (%d, %d) = %g is negative", q, k, inv_l[q * d + k]);
        }
    }
    // rounded ONCE to the points' precision; the exponent's coefficients log2(e) / (2 l^2) are formed in fp64 from the rounded values
    const bool f32 = dtype == COVGRAM_F32;
    auto rnd = [f32](double v) { return f32 ? (double)(float)v : v; };
    const int nch = (ncomp + SM_QC - 1) / SM_QC, qpad = nch * SM_QC;
    const size_t count = sm_prm_count(qpad, d);
    std::vector<double> h(count, 0.0);
    double* hw = h.data(); double* hmu = hw + qpad; double* hc = hmu + (size_t)qpad * d; double* hi = hc + (size_t)qpad * SM_CST;
    double* hgs = hi + qpad; double* hgc = hgs + (size_t)qpad * SM_CST; double* hgi = hgc + (size_t)qpad * SM_CST;
    bool iso = true;
    for (int q = 0; q < ncomp; ++q) {
        hw[q] = rnd(w[q]);
        for (int k = 0; k < d; ++k) {
            hmu[q * d + k] = rnd(mu[q * d + k]);
            const double il = rnd(inv_l[q * d + k]);
            hc[q * SM_CST + k] = rnd(0.72134752044448170368 * il * il);
            hgs[q * SM_CST + k] = rnd(-6.283185307179586476925 * hw[q] * hmu[q * d + k]);
            hgc[q * SM_CST + k] = rnd(hw[q] * il * il);
            if (il != rnd(inv_l[q * d])) iso = false;
        }
        hi[q] = hc[q * SM_CST];
        hgi[q] = hgc[q * SM_CST];
    }
    CG_DEVICE(ctx);
    covgram_sm* S = new covgram_sm();
    S->ctx = ctx; S->ncomp = ncomp; S->d = d; S->dtype = dtype; S->isotropic = iso ? 1 : 0; S->nch = nch;
    const size_t ts = dtype_size(dtype);
    if (hipMalloc(&S->prm, count * ts) != hipSuccess) {
        (void)hipGetLastError();
        delete S;
        set_error("SpectralMixture: hipMalloc of %zu parameter bytes failed", count * ts);
        return COVGRAM_ENOMEM;
    }
    std::vector<float> hf;
    const void* src = h.data();
    if (f32) { hf.assign(h.begin(), h.end()); src = hf.data(); }
    hipError_t e = hipMemcpyAsync(S->prm, src, count * ts, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // the host arrays go out of scope
    if (e != hipSuccess) {
        set_error("SpectralMixture: copying the parameters failed: %s", hipGetErrorString(e));
        (void)hipFree(S->prm);
        delete S;
        return COVGRAM_EHIP;
    }
    ctx->live_handles++;
    *out = S;
    return COVGRAM_OK;
}

int covgram_sm_info(const covgram_sm* S, int32_t* ncomp, int32_t* d, int32_t* dtype, int32_t* isotropic) {
    CG_REQUIRE(S != nullptr, COVGRAM_EINVAL, "spectral-mixture handle is NULL");
    if (ncomp) *ncomp = S->ncomp;
    if (d) *d = S->d;
    if (dtype) *dtype = S->dtype;
    if (isotropic) *isotropic = S->isotropic;
    return COVGRAM_OK;
}

int covgram_sm_mvm(covgram_sm* S, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda, void* y, int64_t ldy, int32_t nrhs,
                   double alpha, double beta, int32_t loc) {
    int rc = sm_check_points(S, X, Y);
    if (rc) return rc;
    CG_REQUIRE(nrhs >= 1, COVGRAM_EINVAL, "nrhs must be >= 1");
    CG_REQUIRE(loc == COVGRAM_HOST || loc == COVGRAM_DEVICE, COVGRAM_EINVAL, "unknown loc %d", loc);
    const int64_t n = X->n, m = Y->n;
    CG_REQUIRE(lda >= m && ldy >= n, COVGRAM_EINVAL, "DimensionMismatch: lda=%lld < m=%lld or ldy=%lld < n=%lld", (long long)lda, (long long)m,
               (long long)ldy, (long long)n);
    CG_REQUIRE((a != nullptr || m == 0) && (y != nullptr || n == 0), COVGRAM_EINVAL, "a or y is NULL");
    if (n == 0) return COVGRAM_OK;
    covgram_ctx* ctx = S->ctx;
    const size_t ts = dtype_size(S->dtype);
    CG_DEVICE(ctx);
    Staged st;
    rc = st.begin(ctx, loc, ts, a, lda, m, y, ldy, n, nrhs, beta);
    if (rc) return rc;
    if (m == 0) {                                // an empty sum: y <- beta y
        const dim3 grid((unsigned)((n + 255) / 256), (unsigned)nrhs);
        by_dtype(S->dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((sm_scale_kernel<T>), grid, dim3(256), 0, ctx->stream, (T*)st.y, n, st.ldy, (T)beta);
        });
    } else
        rc = by_dtype(S->dtype, [&](auto t) { return sm_mvm_t<decltype(t)>(S, X, Y, st.a, st.lda, st.y, st.ldy, nrhs, alpha, beta); });
    if (rc) return rc;
    CG_CHECK_HIP(hipGetLastError());
    return st.finish();
}

int covgram_sm_matrix(covgram_sm* S, const covgram_points* X, const covgram_points* Y, void* out, int64_t ldo, int32_t loc) {
    int rc = sm_check_points(S, X, Y);
    if (rc) return rc;
    CG_REQUIRE(loc == COVGRAM_HOST || loc == COVGRAM_DEVICE, COVGRAM_EINVAL, "unknown loc %d", loc);
    const int64_t n = X->n, m = Y->n;
    CG_REQUIRE(ldo >= n, COVGRAM_EINVAL, "DimensionMismatch: ldo=%lld < n=%lld", (long long)ldo, (long long)n);
    if (n == 0 || m == 0) return COVGRAM_OK;
    CG_REQUIRE(out != nullptr, COVGRAM_EINVAL, "out is NULL");
    covgram_ctx* ctx = S->ctx;
    const size_t ts = dtype_size(S->dtype);
    CG_DEVICE(ctx);
    Staged st;
    rc = st.begin_tile(ctx, loc, ts, out, ldo, n, m);
    if (rc) return rc;
    rc = by_dtype(S->dtype, [&](auto t) { return sm_matrix_t<decltype(t)>(S, X, Y, st.y, st.ldy); });
    if (rc) return rc;
    CG_CHECK_HIP(hipGetLastError());
    return st.finish();
}

int covgram_sm_destroy(covgram_sm* S) {
    if (!S) return COVGRAM_OK;
    {
        ::covgram::DeviceGuard _cg_dev(S->ctx->device);           // (a finalizer may call this from any thread state)
        (void)hipStreamSynchronize(S->ctx->stream);               // products that still read the parameters
        if (S->prm) (void)hipFree(S->prm);
    }
    S->ctx->live_handles--;
    delete S;
    return COVGRAM_OK;
}

}  // extern "C"
