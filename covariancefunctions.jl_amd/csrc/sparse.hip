// sparse.hip — sparse(G, delta): the radius-thresholded CSR Gramian of an exponentially decaying isotropic kernel and its product
// (include/covgram.h: covgram_decay_radius, covgram_sparse_*).  Replaces SparseArrays.sparse(G::Gramian, delta) of src/sparse.jl:5-38.
//
// The reference finds the pairs inside the decay radius with a ball-tree range search and inserts them one by one into a
// SparseMatrixCSC.  Here every pair's s_ij = |x_i - y_j|^2 is evaluated by direct differences, as everywhere else in this library,
// in three steps: COUNT the kept pairs per (row, column chunk), SCAN the counts in (row, chunk) order, FILL the column indices and
// values at the scanned offsets.  A lane owns one row and walks its columns in ascending order, so the indices of a row come out
// sorted; the counts are integers, so nothing depends on the order in which workgroups run: the result is bit-identical from run to run.
//
// Two deliberate corrections of src/sparse.jl ("sparse(G, delta)"):
//   * Lengthscale: sparse.jl:38 drops its delta argument and DIVIDES by l; Lengthscale(k, l) evaluates k(r / l), so the radius is
//     l r0(delta);
//   * a Constant factor c (the spec's `scale`): c k(r) < delta  <=>  k(r) < delta / |c|, so r0 is taken at delta / |c|.
#include <math.h>

#include <algorithm>

#include "driver.hpp"
#include "profiles.hpp"

namespace covgram {

// ------------------------------------------------------------------------------------------------
// decay radius (host)
// ------------------------------------------------------------------------------------------------
static const char* sparse_family_name(int family) {
    switch (family) {
        case COVGRAM_EQ: return "ExponentiatedQuadratic";
        case COVGRAM_EXP: return "Exponential";
        case COVGRAM_RQ: return "RationalQuadratic";
        case COVGRAM_GAMMAEXP: return "GammaExponential";
        case COVGRAM_CAUCHY: return "Cauchy";
        case COVGRAM_IMQ: return "InverseMultiQuadratic";
        case COVGRAM_MATERNP: return "MaternP";
        case COVGRAM_DOT: return "Dot";
        case COVGRAM_EXPDOT: return "ExponentialDot";
        case COVGRAM_MATERN: return "Matern";
        case COVGRAM_ASINDOT: return "AsinDot (NeuralNetwork)";
        case COVGRAM_CONSTANT: return "Constant";
        default: return "unknown";
    }
}

static int decay_radius_of(const covgram_kernel* k, double delta, double* radius) {
    CG_REQUIRE(k != nullptr && radius != nullptr, COVGRAM_EINVAL, "NULL argument");
    if (k->family == COVGRAM_COMPOSITE) {
        const covgram_kernel_composite* c = (const covgram_kernel_composite*)k;
        if (c->nterms > 1) set_error("decay_radius: a Sum of %d terms has no single decay radius (single isotropic profiles only)", c->nterms);
        else set_error("decay_radius: a Product of profiles has no single decay radius (single isotropic profiles only)");
        return COVGRAM_EUNSUPPORTED;
    }
    const bool ok = k->family == COVGRAM_EQ || k->family == COVGRAM_EXP || k->family == COVGRAM_GAMMAEXP || k->family == COVGRAM_MATERNP ||
                    k->family == COVGRAM_MATERN;
    CG_REQUIRE(ok, COVGRAM_EUNSUPPORTED, "decay_radius: %s does not decay exponentially (defined for EQ, Exponential, GammaExponential, MaternP, Matern)",
               sparse_family_name(k->family));
    CG_REQUIRE(k->power == 1, COVGRAM_EUNSUPPORTED, "decay_radius: Power(%s, %d) is not supported (single profiles without a Power wrapper)",
               sparse_family_name(k->family), k->power);
    CG_REQUIRE(k->lengthscale > 0, COVGRAM_EINVAL, "DomainError: l = %g is non-positive", k->lengthscale);
    const double c = fabs(k->scale);
    const double de = delta / c;
    CG_REQUIRE(c > 0 && de > 0 && de < 1, COVGRAM_EINVAL, "decay_radius: need 0 < delta / |c| < 1 (delta = %g, Constant factor c = %g)", delta, k->scale);
    double r0 = 0;
    switch (k->family) {
        case COVGRAM_EQ: r0 = sqrt(-2.0 * log(de)); break;                                   // src/sparse.jl:25
        case COVGRAM_EXP: r0 = -log(de); break;                                              // :26
        case COVGRAM_GAMMAEXP:
            CG_REQUIRE(k->param > 0 && k->param <= 2, COVGRAM_EINVAL, "DomainError: gamma = %g not in (0, 2]", k->param);
            r0 = pow(-2.0 * log(de), 1.0 / k->param);                                        // :27
            break;
        case COVGRAM_MATERNP: r0 = -log(de); break;                                          // :35 (conservative)
        default:                                                                             // Matern(nu), :28-34
            CG_REQUIRE(k->param >= 0.5, COVGRAM_EINVAL, "DomainError: decay_radius not defined for Matern kernel with nu = %g < 1/2", k->param);
            r0 = -log(de);
            break;
    }
    *radius = k->lengthscale * r0;
    return COVGRAM_OK;
}

// ------------------------------------------------------------------------------------------------
// build: count / scan / fill
// ------------------------------------------------------------------------------------------------
constexpr int SP_ROWS = 256;    // rows of a workgroup, one per lane
constexpr int SP_TJ = 64;       // columns of an LDS tile
constexpr int SP_LDS = 4096;    // scalars of the tile: 64 columns of the widest register bucket
constexpr int SP_STEP = 8;      // dimensions between two tests of the partial sum

// THE predicate of both passes: s = sum_l (x_l - y_l)^2 by one fused multiply-add per dimension in ascending l, in the points' own
// precision; kept exactly when s <= R2 (inclusive, as the ball tree's inrange; a NaN is not kept).  The partial sums never decrease
// (q^2 >= 0 and rounding is monotone), so a lane stops once its partial sum exceeds R2: the predicate is unchanged, and a kept pair
// always carries its complete sum.  DM > 0: x in registers, padded with zeros like the tile's columns (they add exact zeros);
// DM == 0: any d, x read through the pointer.
template <typename T, int DM, typename XT>
__device__ __forceinline__ bool sparse_keep(const XT& x, const T* __restrict__ y, int d, T R2, T& s_out) {
    T s = (T)0;
    if constexpr (DM > 0) {
#pragma unroll
        for (int l0 = 0; l0 < DM; l0 += SP_STEP) {
#pragma unroll
            for (int l = l0; l < l0 + SP_STEP && l < DM; ++l) { const T q = x[l] - y[l]; s = fma_t(q, q, s); }
            if (DM > SP_STEP && s > R2) break;
        }
    } else {
        for (int l0 = 0; l0 < d; l0 += SP_STEP) {
            const int l1 = l0 + SP_STEP < d ? l0 + SP_STEP : d;
            for (int l = l0; l < l1; ++l) { const T q = x[l] - y[l]; s = fma_t(q, q, s); }
            if (s > R2) break;
        }
    }
    s_out = s;
    return s <= R2;
}

// the profiles that have a decay radius, on the library's usual (unfolded) evaluation
template <typename T>
__device__ __forceinline__ T sparse_phi(int family, T s, const KParams<T>& kp) {
    switch (family) {
        case COVGRAM_EQ: return Phi<COVGRAM_EQ, T, false>::eval(s, kp);
        case COVGRAM_EXP: return Phi<COVGRAM_EXP, T, false>::eval(s, kp);
        case COVGRAM_GAMMAEXP: return Phi<COVGRAM_GAMMAEXP, T, false>::eval(s, kp);
        case COVGRAM_MATERNP: return Phi<COVGRAM_MATERNP, T, false>::eval(s, kp);
        default: return Phi<COVGRAM_MATERN, T, false>::eval(s, kp);
    }
}

struct SparseSweep {
    int64_t n, m;
    int32_t d;
    int32_t tj;         // columns per tile
    int32_t use_lds;    // generic kernel only: 0 = a point does not fit the tile, columns are read from memory
    int64_t jchunk;     // columns per chunk (a multiple of tj)
    int32_t nchunks;
};

// One workgroup = 256 rows x one column chunk; the chunk's columns pass through LDS tile by tile, shared by the rows.
// FILL = false: counts[row nchunks + chunk] = kept pairs.  FILL = true: indices and values at off[row nchunks + chunk] ...; never at or
// beyond the next offset, and *flag is raised when a (row, chunk) fills another number than it counted.
template <typename T, int DM, bool FILL>
__global__ __launch_bounds__(SP_ROWS) void sparse_sweep_kernel(const T* __restrict__ X, const T* __restrict__ Y, const SparseSweep g, T R2,
                                                               uint32_t* __restrict__ counts, const int64_t* __restrict__ off,
                                                               int32_t* __restrict__ colind, T* __restrict__ vals, unsigned* __restrict__ flag,
                                                               int family, T scale, const KParams<T> kp) {
    __shared__ T tile[SP_LDS];
    const int64_t i = (int64_t)blockIdx.x * SP_ROWS + threadIdx.x;
    const bool active = i < g.n;
    const int chunk = blockIdx.y;
    const int d = g.d;
    const int64_t j0 = (int64_t)chunk * g.jchunk;
    const int64_t j1 = j0 + g.jchunk < g.m ? j0 + g.jchunk : g.m;
    const T* xg = X + (active ? i : 0) * (int64_t)d;           // (inactive lanes read row 0: they only help to stage the tiles)
    constexpr int XN = DM > 0 ? DM : 1;
    T xr[XN];
    if constexpr (DM > 0) {
#pragma unroll
        for (int l = 0; l < DM; ++l) xr[l] = (l < d) ? xg[l] : (T)0;
    }
    const int W = DM > 0 ? DM : d;                             // scalars per column of the tile
    const bool lds = DM > 0 ? true : (g.use_lds != 0);
    const int64_t slot = i * g.nchunks + chunk;
    int64_t pos = 0, end = 0;
    uint32_t cnt = 0;
    if (FILL && active) { pos = off[slot]; end = off[slot + 1]; }
    for (int64_t jb = j0; jb < j1; jb += g.tj) {
        const int nj = (int)(jb + g.tj < j1 ? g.tj : j1 - jb);
        if (lds) {
            __syncthreads();                                    // the previous tile has been read by every lane
            for (int e = threadIdx.x; e < nj * W; e += SP_ROWS) {
                const int c = e / W, l = e - c * W;
                tile[e] = (l < d) ? Y[(jb + c) * (int64_t)d + l] : (T)0;
            }
            __syncthreads();
        }
        if (!active) continue;
        for (int c = 0; c < nj; ++c) {
            T s;
            bool keep;
            if constexpr (DM > 0) keep = sparse_keep<T, DM>(xr, tile + c * DM, d, R2, s);
            else keep = lds ? sparse_keep<T, 0>(xg, tile + c * d, d, R2, s) : sparse_keep<T, 0>(xg, Y + (jb + c) * (int64_t)d, d, R2, s);
            if (keep) {
                if constexpr (FILL) {
                    if (pos < end) {
                        colind[pos] = (int32_t)(jb + c);
                        vals[pos] = scale * sparse_phi<T>(family, s * kp.gamma2, kp);
                    }
                    ++pos;
                } else {
                    ++cnt;
                }
            }
        }
    }
    if (active) {
        if constexpr (FILL) { if (pos != end) atomicOr(flag, 1u); }
        else counts[slot] = cnt;
    }
}

// exclusive scan of `count` 32-bit counts into 64-bit offsets, off[count] = the total: block sums, one workgroup over the block sums, apply
constexpr int SCAN_ITEMS = 16;
constexpr int SCAN_BLOCK = 256 * SCAN_ITEMS;

__device__ __forceinline__ int64_t block_inclusive_scan_256(int64_t v, int64_t* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int64_t u = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += u;
        __syncthreads();
    }
    return sh[t];
}

__global__ __launch_bounds__(256) void sparse_scan_sums_kernel(const uint32_t* __restrict__ counts, int64_t count, int64_t* __restrict__ bsum) {
    __shared__ int64_t sh[256];
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)threadIdx.x * SCAN_ITEMS;
    int64_t s = 0;
    for (int q = 0; q < SCAN_ITEMS; ++q) s += (base + q < count) ? (int64_t)counts[base + q] : 0;
    const int64_t incl = block_inclusive_scan_256(s, sh);
    if (threadIdx.x == 255) bsum[blockIdx.x] = incl;
}

__global__ __launch_bounds__(256) void sparse_scan_top_kernel(int64_t* __restrict__ bsum, int64_t nb) {
    __shared__ int64_t sh[256];
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += 256) {
        const int64_t idx = b0 + threadIdx.x;
        const int64_t v = idx < nb ? bsum[idx] : 0;
        const int64_t incl = block_inclusive_scan_256(v, sh);
        if (idx < nb) bsum[idx] = carry + incl - v;
        carry += sh[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[nb] = carry;
}

__global__ __launch_bounds__(256) void sparse_scan_apply_kernel(const uint32_t* __restrict__ counts, int64_t count, const int64_t* __restrict__ bsum,
                                                                int64_t nb, int64_t* __restrict__ off) {
    __shared__ int64_t sh[256];
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t c[SCAN_ITEMS];
    int64_t s = 0;
#pragma unroll
    for (int q = 0; q < SCAN_ITEMS; ++q) { c[q] = (base + q < count) ? counts[base + q] : 0u; s += c[q]; }
    const int64_t incl = block_inclusive_scan_256(s, sh);
    int64_t run = bsum[blockIdx.x] + incl - s;
#pragma unroll
    for (int q = 0; q < SCAN_ITEMS; ++q) {
        if (base + q < count) off[base + q] = run;
        run += c[q];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) off[count] = bsum[nb];
}

__global__ __launch_bounds__(256) void sparse_rowptr_kernel(const int64_t* __restrict__ off, int64_t n, int32_t nchunks, int64_t* __restrict__ rowptr) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= n) rowptr[i] = off[i * nchunks];
}

// ------------------------------------------------------------------------------------------------
// product: CSR gather, G lanes per row, no atomics
// ------------------------------------------------------------------------------------------------
// y[row + r ldy] = alpha sum_p vals[p] a[colind[p] + r lda] + beta y[..] for r < nr <= NR.  Lane q of a row's group adds the entries
// p0 + q, p0 + q + G, ... in ascending order; the G partial sums are then folded by an xor butterfly (G / 2, ..., 1): a fixed order.
template <typename T, int G, int NR>
__global__ __launch_bounds__(256) void sparse_mvm_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                         const T* __restrict__ vals, int64_t n, const T* __restrict__ a, int64_t lda,
                                                         T* __restrict__ y, int64_t ldy, int nr, T alpha, T beta) {
    const int64_t gt = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gt / G;
    const int q = (int)(gt % G);
    T acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = (T)0;
    if (row < n) {
        const int64_t p1 = rowptr[row + 1];
        for (int64_t p = rowptr[row] + q; p < p1; p += G) {
            const T v = vals[p];
            const int64_t c = colind[p];
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if (r < nr) acc[r] = fma_t(v, a[c + r * lda], acc[r]);
        }
    }
    // (no lane has left: groups never straddle a wave, and the rows beyond n carry zeros)
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1)
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[r] += __shfl_xor(acc[r], o, 64);
    if (row < n && q == 0) {
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (r < nr) {
                T* yp = y + row + r * ldy;
                *yp = (beta == (T)0) ? alpha * acc[r] : fma_t(alpha, acc[r], beta * *yp);     // beta == 0: y is never read
            }
    }
}

}  // namespace covgram

struct covgram_sparse {
    covgram_ctx* ctx = nullptr;
    int64_t n = 0, m = 0, nnz = 0;
    int32_t dtype = 0;
    double radius = 0;
    int64_t* rowptr = nullptr;   // n + 1
    int32_t* colind = nullptr;   // nnz
    void* vals = nullptr;        // nnz scalars
    int group = 1;               // lanes per row of the product kernel: 1, 4, 16 or 64 from nnz / n
};

namespace covgram {

template <typename T, int G>
static void launch_sparse_mvm(const covgram_sparse* S, const void* a, int64_t lda, void* y, int64_t ldy, int nrhs, double alpha, double beta,
                              hipStream_t stream) {
    const int64_t threads = S->n * G;
    const dim3 grid((unsigned)((threads + 255) / 256));
    for (int c0 = 0; c0 < nrhs; c0 += 4) {                        // four right-hand sides share one pass over the entries
        const int nr = std::min(4, nrhs - c0);
        const T* ac = (const T*)a + (size_t)c0 * lda;
        T* yc = (T*)y + (size_t)c0 * ldy;
        if (nr == 1)
            hipLaunchKernelGGL((sparse_mvm_kernel<T, G, 1>), grid, dim3(256), 0, stream, S->rowptr, S->colind, (const T*)S->vals, S->n, ac, lda, yc,
                               ldy, nr, (T)alpha, (T)beta);
        else
            hipLaunchKernelGGL((sparse_mvm_kernel<T, G, 4>), grid, dim3(256), 0, stream, S->rowptr, S->colind, (const T*)S->vals, S->n, ac, lda, yc,
                               ldy, nr, (T)alpha, (T)beta);
    }
}

template <typename T>
static void launch_sparse_mvm_t(const covgram_sparse* S, const void* a, int64_t lda, void* y, int64_t ldy, int nrhs, double alpha, double beta,
                                hipStream_t stream) {
    auto launch = [&](auto G) { launch_sparse_mvm<T, decltype(G)::value>(S, a, lda, y, ldy, nrhs, alpha, beta, stream); };
    if (!try_dim(Dims<1, 4, 16>{}, S->group, launch)) launch(std::integral_constant<int, 64>{});
}

template <typename T, bool FILL>
static void launch_sparse_sweep(const covgram_points* X, const covgram_points* Y, const SparseSweep& g, double R2, uint32_t* counts, const int64_t* off,
                                int32_t* colind, void* vals, unsigned* flag, const HostKernel& hk, hipStream_t stream) {
    const dim3 grid((unsigned)((g.n + SP_ROWS - 1) / SP_ROWS), (unsigned)g.nchunks);
#define CG_SWEEP(DMV)                                                                                                                        \
    hipLaunchKernelGGL((sparse_sweep_kernel<T, DMV, FILL>), grid, dim3(SP_ROWS), 0, stream, (const T*)X->dptr, (const T*)Y->dptr, g, (T)R2, counts, \
                       off, colind, (T*)vals, flag, (int)hk.k.family, (T)hk.kp.scale, cast_params<T>(hk.kp))
    const int d = g.d;
    if (d <= 4) CG_SWEEP(4); else if (d <= 8) CG_SWEEP(8); else if (d <= 16) CG_SWEEP(16); else if (d <= 32) CG_SWEEP(32);
    else if (d <= 64) CG_SWEEP(64); else CG_SWEEP(0);
#undef CG_SWEEP
}

// temporaries of one create call
struct SparseTemp {
    void* p[4] = {nullptr, nullptr, nullptr, nullptr};
    ~SparseTemp() { for (void* q : p) if (q) (void)hipFree(q); }
};

static void sparse_free(covgram_sparse* S) {
    if (S->rowptr) (void)hipFree(S->rowptr);
    if (S->colind) (void)hipFree(S->colind);
    if (S->vals) (void)hipFree(S->vals);
    S->rowptr = nullptr; S->colind = nullptr; S->vals = nullptr;
}

}  // namespace covgram

using namespace covgram;

extern "C" {

int covgram_decay_radius(const covgram_kernel* k, double delta, double* radius) { return decay_radius_of(k, delta, radius); }

int covgram_sparse_create(covgram_ctx* ctx, covgram_sparse** out, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y,
                          double delta) {
    CG_REQUIRE(ctx && out && X && Y, COVGRAM_EINVAL, "NULL argument");
    CG_REQUIRE(X->ctx == ctx && Y->ctx == ctx, COVGRAM_EINVAL, "points belong to a different ctx");
    CG_REQUIRE(X->dtype == Y->dtype, COVGRAM_EINVAL, "x and y have different dtypes");
    CG_REQUIRE(X->d == Y->d, COVGRAM_EINVAL, "DimensionMismatch: inputs have to have the same length: %d, %d", X->d, Y->d);
    double R = 0;
    int rc = decay_radius_of(k, delta, &R);
    if (rc) return rc;
    const int dtype = X->dtype;
    HostKernel hk;
    rc = make_host_kernel(k, dtype, true, &hk);   // gamma = 1 / l, unfolded profiles: the evaluation of covgram_matrix
    if (rc) return rc;
    const int64_t n = X->n, m = Y->n;
    CG_REQUIRE(m < ((int64_t)1 << 31), COVGRAM_EINVAL, "sparse: m = %lld columns do not fit 32-bit column indices", (long long)m);
    const size_t ts = dtype_size(dtype);
    CG_DEVICE(ctx);

    covgram_sparse* S = new covgram_sparse();
    S->ctx = ctx; S->n = n; S->m = m; S->dtype = dtype; S->radius = R;
    auto fail = [&](int code) { sparse_free(S); delete S; return code; };
#define CG_SP_HIP(expr)                                                                                          \
    do {                                                                                                         \
        hipError_t _e = (expr);                                                                                  \
        if (_e != hipSuccess) { set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); return fail(COVGRAM_EHIP); } \
    } while (0)
    if (hipMalloc((void**)&S->rowptr, (size_t)(n + 1) * sizeof(int64_t)) != hipSuccess) {
        set_error("sparse: hipMalloc of the %lld row offsets failed", (long long)(n + 1));
        return fail(COVGRAM_ENOMEM);
    }
    if (n == 0 || m == 0) {                       // an empty product: a valid handle with nnz = 0
        CG_SP_HIP(hipMemsetAsync(S->rowptr, 0, (size_t)(n + 1) * sizeof(int64_t), ctx->stream));
        CG_SP_HIP(hipStreamSynchronize(ctx->stream));
        ctx->live_handles++;
        *out = S;
        return COVGRAM_OK;
    }

    // tiles and chunks: 64-column tiles; small n splits the columns over workgroups, chunks of at least four tiles
    SparseSweep g;
    g.n = n; g.m = m; g.d = X->d;
    g.tj = SP_TJ; g.use_lds = 1;
    if (X->d > 64) {
        if (X->d > SP_LDS) g.use_lds = 0;
        else g.tj = std::max(1, std::min(SP_TJ, SP_LDS / X->d));
    }
    const int64_t rowblocks = (n + SP_ROWS - 1) / SP_ROWS;
    const int64_t ntiles = (m + g.tj - 1) / g.tj;
    const int64_t target = (int64_t)ctx->num_cus * 4;
    int64_t nchunks = std::min<int64_t>((target + rowblocks - 1) / rowblocks, std::max<int64_t>(1, ntiles / 4));
    nchunks = std::max<int64_t>(1, std::min<int64_t>(nchunks, 1024));
    const int64_t tiles_per = (ntiles + nchunks - 1) / nchunks;
    g.jchunk = tiles_per * g.tj;
    g.nchunks = (int32_t)((m + g.jchunk - 1) / g.jchunk);

    const int64_t slots = n * g.nchunks;
    const int64_t nb = (slots + SCAN_BLOCK - 1) / SCAN_BLOCK;
    SparseTemp tmp;
    uint32_t* counts = nullptr; int64_t* off = nullptr; int64_t* bsum = nullptr; unsigned* flag = nullptr;
    if (hipMalloc(&tmp.p[0], (size_t)slots * sizeof(uint32_t)) != hipSuccess || hipMalloc(&tmp.p[1], (size_t)(slots + 1) * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&tmp.p[2], (size_t)(nb + 1) * sizeof(int64_t)) != hipSuccess || hipMalloc(&tmp.p[3], sizeof(unsigned)) != hipSuccess) {
        set_error("sparse: hipMalloc of the count / offset arrays (%lld slots) failed", (long long)slots);
        return fail(COVGRAM_ENOMEM);
    }
    counts = (uint32_t*)tmp.p[0]; off = (int64_t*)tmp.p[1]; bsum = (int64_t*)tmp.p[2]; flag = (unsigned*)tmp.p[3];
    const double R2 = R * R;

    // 1. count
    by_dtype(dtype, [&](auto t) { launch_sparse_sweep<decltype(t), false>(X, Y, g, R2, counts, nullptr, nullptr, nullptr, nullptr, hk, ctx->stream); });
    // 2. scan in (row, chunk) order
    hipLaunchKernelGGL(sparse_scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, counts, slots, bsum);
    hipLaunchKernelGGL(sparse_scan_top_kernel, dim3(1), dim3(256), 0, ctx->stream, bsum, nb);
    hipLaunchKernelGGL(sparse_scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, counts, slots, bsum, nb, off);
    hipLaunchKernelGGL(sparse_rowptr_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, ctx->stream, off, n, g.nchunks, S->rowptr);
    CG_SP_HIP(hipMemsetAsync(flag, 0, sizeof(unsigned), ctx->stream));
    CG_SP_HIP(hipGetLastError());
    // the ONE synchronisation before the allocation: nnz
    int64_t nnz = 0;
    CG_SP_HIP(hipMemcpyAsync(&nnz, bsum + nb, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    CG_SP_HIP(hipStreamSynchronize(ctx->stream));
    S->nnz = nnz;
    if (nnz > 0) {
        if (hipMalloc((void**)&S->colind, (size_t)nnz * sizeof(int32_t)) != hipSuccess || hipMalloc(&S->vals, (size_t)nnz * ts) != hipSuccess) {
            (void)hipGetLastError();
            set_error("sparse: nnz = %lld entries (%.3g %% of %lld x %lld) need %zu bytes, which hipMalloc refused: raise delta or shorten the lengthscale",
                      (long long)nnz, 100.0 * (double)nnz / ((double)n * (double)m), (long long)n, (long long)m, (size_t)nnz * (sizeof(int32_t) + ts));
            return fail(COVGRAM_ENOMEM);
        }
        // 3. fill
        { TimerScope tm(ctx); by_dtype(dtype, [&](auto t) { launch_sparse_sweep<decltype(t), true>(X, Y, g, R2, nullptr, off, S->colind, S->vals, flag, hk, ctx->stream); }); }
        CG_SP_HIP(hipGetLastError());
    }
    // the fill has read X and Y for the last time when this returns (the handle keeps no reference to them), and its flag is known
    unsigned mismatch = 0;
    CG_SP_HIP(hipMemcpyAsync(&mismatch, flag, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    CG_SP_HIP(hipStreamSynchronize(ctx->stream));
    if (mismatch) { set_error("internal: count/fill mismatch"); return fail(COVGRAM_EHIP); }
#undef CG_SP_HIP
    const double avg = (double)nnz / (double)n;
    S->group = avg < 4 ? 1 : (avg < 32 ? 4 : (avg < 256 ? 16 : 64));
    ctx->live_handles++;
    *out = S;
    return COVGRAM_OK;
}

int covgram_sparse_info(const covgram_sparse* S, int64_t* n, int64_t* m, int64_t* nnz, int32_t* dtype, double* radius) {
    CG_REQUIRE(S != nullptr, COVGRAM_EINVAL, "sparse handle is NULL");
    if (n) *n = S->n;
    if (m) *m = S->m;
    if (nnz) *nnz = S->nnz;
    if (dtype) *dtype = S->dtype;
    if (radius) *radius = S->radius;
    return COVGRAM_OK;
}

int covgram_sparse_export(const covgram_sparse* S, int64_t* rowptr, int32_t* colind, void* vals, int32_t loc) {
    CG_REQUIRE(S != nullptr, COVGRAM_EINVAL, "sparse handle is NULL");
    CG_REQUIRE(loc == COVGRAM_HOST || loc == COVGRAM_DEVICE, COVGRAM_EINVAL, "unknown loc %d", loc);
    covgram_ctx* ctx = S->ctx;
    CG_DEVICE(ctx);
    const hipMemcpyKind kind = loc == COVGRAM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (rowptr) CG_CHECK_HIP(hipMemcpyAsync(rowptr, S->rowptr, (size_t)(S->n + 1) * sizeof(int64_t), kind, ctx->stream));
    if (colind && S->nnz) CG_CHECK_HIP(hipMemcpyAsync(colind, S->colind, (size_t)S->nnz * sizeof(int32_t), kind, ctx->stream));
    if (vals && S->nnz) CG_CHECK_HIP(hipMemcpyAsync(vals, S->vals, (size_t)S->nnz * dtype_size(S->dtype), kind, ctx->stream));
    if (loc == COVGRAM_HOST) CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return COVGRAM_OK;
}

int covgram_sparse_mvm(covgram_sparse* S, const void* a, int64_t lda, void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t loc) {
    CG_REQUIRE(S != nullptr, COVGRAM_EINVAL, "sparse handle is NULL");
    CG_REQUIRE(nrhs >= 1, COVGRAM_EINVAL, "nrhs must be >= 1");
    CG_REQUIRE(loc == COVGRAM_HOST || loc == COVGRAM_DEVICE, COVGRAM_EINVAL, "unknown loc %d", loc);
    const int64_t n = S->n, m = S->m;
    CG_REQUIRE(lda >= m && ldy >= n, COVGRAM_EINVAL, "DimensionMismatch: lda=%lld < m=%lld or ldy=%lld < n=%lld", (long long)lda, (long long)m,
               (long long)ldy, (long long)n);
    CG_REQUIRE((a != nullptr || m == 0) && (y != nullptr || n == 0), COVGRAM_EINVAL, "a or y is NULL");
    if (n == 0) return COVGRAM_OK;
    covgram_ctx* ctx = S->ctx;
    const size_t ts = dtype_size(S->dtype);
    CG_DEVICE(ctx);
    Staged st;
    int rc = st.begin(ctx, loc, ts, a, lda, m, y, ldy, n, nrhs, beta);
    if (rc) return rc;
    { TimerScope tm(ctx); by_dtype(S->dtype, [&](auto t) { launch_sparse_mvm_t<decltype(t)>(S, st.a, st.lda, st.y, st.ldy, nrhs, alpha, beta, ctx->stream); }); }
    CG_CHECK_HIP(hipGetLastError());
    return st.finish();
}

int covgram_sparse_destroy(covgram_sparse* S) {
    if (!S) return COVGRAM_OK;
    {
        ::covgram::DeviceGuard _cg_dev(S->ctx->device);           // (a finalizer may call this from any thread state)
        (void)hipStreamSynchronize(S->ctx->stream);               // products that still read the arrays
        sparse_free(S);
    }
    S->ctx->live_handles--;
    delete S;
    return COVGRAM_OK;
}

}  // extern "C"
