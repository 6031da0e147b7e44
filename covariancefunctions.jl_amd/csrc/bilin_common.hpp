// bilin_common.hpp — what the two fused passes over the pairs of a bilinear form sum_t u_t' G a_t share: bilin_grad.hip (hyper-parameter
// gradients) and input_grad.hip (gradients with respect to the row points).  The tile constants, the jet
// of one pair, the argument checks of the two C entries, the staging of host weights and the column split.
#pragma once
#include <algorithm>
#include <cmath>

#include "driver.hpp"
#include "profiles.hpp"

namespace covgram {

constexpr int BG_TI = 64;       // rows per workgroup = lanes per wave
constexpr int BG_WAVES = 4;
constexpr int BG_L = 128;       // pairs a lane adds in the working precision before the hand-off to fp64 (tests/bilin_grad_ref.py: HANDOFF)
// columns per lane and tile: 16 in fp32 (64-column tiles, a hand-off every 8 tiles), 8 in fp64 (32-column tiles, every 16): the three
// per-pair arrays (W, s, W dk/ds) are 3 JPL registers, twice that in fp64
template <typename T> constexpr int bg_jpl = sizeof(T) == 4 ? 16 : 8;
constexpr int BG_DS = 16;       // dimensions per LDS slab
constexpr int BG_MAX_D = 64, BG_MAX_NVEC = 32;

__device__ __forceinline__ float bg_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double bg_log1p(double x) { return log1p(x); }

// k, dk/ds (s raw; 0 where the scaled s is 0) and dk/dparam of one pair
template <typename T>
__device__ __forceinline__ void bg_jet(int family, T sr, const KParams<T>& kp, T cpar, T& v, T& ds, T& dp) {
    const T s = sr * kp.gamma2;
    T f, f1, f2, fp = (T)0;
    switch (family) {
        case COVGRAM_EQ: DPhi<COVGRAM_EQ, T>::eval(s, kp, f, f1, f2); break;
        case COVGRAM_EXP: DPhi<COVGRAM_EXP, T>::eval(s, kp, f, f1, f2); break;
        case COVGRAM_RQ: {
            DPhi<COVGRAM_RQ, T>::eval(s, kp, f, f1, f2);
            const T x = s * kp.c0;                                  // s / (2 alpha)
            fp = f * (x * cg_rcp((T)1 + x) - bg_log1p(x));          // phi (s / (2 alpha + s) - log1p(s / (2 alpha)))
            break;
        }
        case COVGRAM_GAMMAEXP: {
            DPhi<COVGRAM_GAMMAEXP, T>::eval(s, kp, f, f1, f2);
            const T sg = (kp.param == (T)0) ? (T)1 : pow_pos(s, kp.param);
            fp = s == (T)0 ? (T)0 : (T)-0.25 * f * sg * cg_log(s);  // -1/4 phi s^(gamma/2) log s; 0 at s = 0
            break;
        }
        case COVGRAM_CAUCHY: DPhi<COVGRAM_CAUCHY, T>::eval(s, kp, f, f1, f2); break;
        case COVGRAM_IMQ: {
            DPhi<COVGRAM_IMQ, T>::eval(s, kp, f, f1, f2);
            fp = -cpar * f * cg_rcp(s + kp.param);                  // -c (s + c^2)^(-3/2)
            break;
        }
        default: DPhi<COVGRAM_MATERNP, T>::eval(s, kp, f, f1, f2); break;
    }
    v = f;
    if (kp.power != 1) {                                            // (phi^q)' = q phi^(q-1) phi', in s and in the parameter alike
        const T fq1 = ipow(f, kp.power - 1);
        const T mult = (T)kp.power * fq1;
        v = fq1 * f; f1 *= mult; fp *= mult;
    }
    v *= kp.scale;
    dp = fp * kp.scale;
    ds = s == (T)0 ? (T)0 : f1 * kp.gamma2 * kp.scale;             // s = 0: the pair's differences are all 0 (NaN still propagates)
}

// The argument checks of covgram_bilinear_grad and covgram_bilinear_input_grad (`fn`: the name in the messages); *Y becomes X when NULL
inline int bg_check_args(const char* fn, covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points** Y, const void* U,
                         int64_t ldu, const void* A, int64_t lda, int32_t nvec, const double* out, int32_t loc) {
    CG_REQUIRE(ctx && k && X, COVGRAM_EINVAL, "NULL argument");
    if (!*Y) *Y = X;
    CG_REQUIRE(X->ctx == ctx && (*Y)->ctx == ctx, COVGRAM_EINVAL, "points belong to a different ctx");
    CG_REQUIRE(X->dtype == (*Y)->dtype, COVGRAM_EINVAL, "X and Y have different dtypes");
    CG_REQUIRE(X->d == (*Y)->d, COVGRAM_EINVAL, "DimensionMismatch: inputs have to have the same length (%d and %d)", X->d, (*Y)->d);
    CG_REQUIRE(loc == COVGRAM_HOST || loc == COVGRAM_DEVICE, COVGRAM_EINVAL, "unknown loc %d", loc);
    CG_REQUIRE(k->family != COVGRAM_COMPOSITE, COVGRAM_EUNSUPPORTED, "%s: composite kernels are handled term by term on the host", fn);
    CG_REQUIRE(k->family >= 0 && k->family < COVGRAM_NFAMILY, COVGRAM_EUNSUPPORTED, "unknown kernel family %d", k->family);
    CG_REQUIRE(k->family != COVGRAM_DOT && k->family != COVGRAM_EXPDOT && k->family != COVGRAM_ASINDOT, COVGRAM_EUNSUPPORTED,
               "%s: dot-product kernels have no bilinear gradient path", fn);
    CG_REQUIRE(k->family != COVGRAM_MATERN, COVGRAM_EUNSUPPORTED, "%s: Matern with real nu is not supported (half-integer nu: MaternP)", fn);
    CG_REQUIRE(nvec >= 1 && nvec <= BG_MAX_NVEC, COVGRAM_EINVAL, "%s: nvec = %d is outside 1 .. %d", fn, nvec, BG_MAX_NVEC);
    CG_REQUIRE(X->d >= 1 && X->d <= BG_MAX_D, COVGRAM_EINVAL, "%s: d = %d is outside 1 .. %d", fn, X->d, BG_MAX_D);
    CG_REQUIRE(out != nullptr, COVGRAM_EINVAL, "out is NULL");
    const int64_t n = X->n, m = (*Y)->n;
    CG_REQUIRE(ldu >= n && lda >= m, COVGRAM_EINVAL, "DimensionMismatch: ldu=%lld < n=%lld or lda=%lld < m=%lld", (long long)ldu, (long long)n,
               (long long)lda, (long long)m);
    CG_REQUIRE((U != nullptr || n == 0) && (A != nullptr || m == 0), COVGRAM_EINVAL, "U or A is NULL");
    return COVGRAM_OK;
}

// Host weights: U (n x nvec) and A (m x nvec) packed into workspace slot 2, stream-ordered; *U, *A and the leading dimensions then name the copies
inline int bg_stage_weights(covgram_ctx* ctx, int64_t n, int64_t m, int nvec, size_t ts, const void** U, int64_t* ldu, const void** A, int64_t* lda) {
    void* su;
    const size_t ub = (((size_t)n * nvec * ts) + 255) & ~(size_t)255;
    int rc = ws_reserve(ctx, 2, ub + (size_t)m * nvec * ts, &su); if (rc) return rc;
    void* sa = (char*)su + ub;
    CG_CHECK_HIP(hipMemcpy2DAsync(su, (size_t)n * ts, *U, (size_t)*ldu * ts, (size_t)n * ts, nvec, hipMemcpyHostToDevice, ctx->stream));
    CG_CHECK_HIP(hipMemcpy2DAsync(sa, (size_t)m * ts, *A, (size_t)*lda * ts, (size_t)m * ts, nvec, hipMemcpyHostToDevice, ctx->stream));
    *U = su; *A = sa; *ldu = n; *lda = m;
    return COVGRAM_OK;
}

// Column split of a launch with `rowblocks` workgroups per column chunk: enough workgroups for every CU, chunks of at least one hand-off
// interval.  *jchunk: columns per chunk (a multiple of the tile width)
template <typename T>
inline int64_t bg_column_split(const covgram_ctx* ctx, int64_t rowblocks, int64_t m, int64_t* jchunk) {
    constexpr int BG_TJ = bg_jpl<T> * BG_WAVES, BG_KT = BG_L / bg_jpl<T>;
    const int64_t ntiles = (m + BG_TJ - 1) / BG_TJ;
    int64_t jsplit = std::min<int64_t>(((int64_t)ctx->num_cus * 8 + rowblocks - 1) / rowblocks, std::max<int64_t>(1, ntiles / BG_KT));
    jsplit = std::max<int64_t>(1, std::min<int64_t>(jsplit, 65535));
    const int64_t tiles_per = (ntiles + jsplit - 1) / jsplit;
    jsplit = (ntiles + tiles_per - 1) / tiles_per;
    *jchunk = tiles_per * BG_TJ;
    return jsplit;
}

}  // namespace covgram
