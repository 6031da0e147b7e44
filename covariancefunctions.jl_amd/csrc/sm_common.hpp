// sm_common.hpp — what the units behind the covgram_sm handle share: sm.hip (product and Matrix(G)) and sm_grad.hip
// (hyper-parameter gradients of a bilinear form) and sm_input_grad.hip (its gradients in the row points).  The handle, the chunking of the components, the per-point phase kernel
// and the check of the points against the handle.
#pragma once
#include <cmath>

#include "driver.hpp"

struct covgram_sm {
    covgram_ctx* ctx = nullptr;
    int32_t ncomp = 0, d = 0, dtype = 0, isotropic = 0, nch = 0;
    // device, scalars of dtype: w [qpad] | mu [qpad d] | coef [qpad SM_CST] | ciso [qpad] | gsin [qpad SM_CST] | gcos [qpad SM_CST] | gciso [qpad]
    // (the last three: the input gradient's coefficients -2 pi w_q mu_qk and w_q inv_l_qk^2, formed in fp64 from the rounded parameters)
    void* prm = nullptr;
};

namespace covgram {

constexpr int SM_QC = 4;       // components per chunk
constexpr int SM_CST = COVGRAM_SM_MAX_D;   // stride of a component's coefficient row
inline size_t sm_prm_count(int qpad, int d) { return (size_t)qpad * (2 + d) + (size_t)qpad * SM_CST + (size_t)qpad * (2 * SM_CST + 1); }

// phases of both point sets: thread = (point, component slot)
template <typename T>
__global__ __launch_bounds__(256) void sm_phase_kernel(const T* __restrict__ X, int64_t n, const T* __restrict__ Y, int64_t m, int d, int ncomp, int nch,
                                                       const T* __restrict__ w, const T* __restrict__ mu, T* __restrict__ RS, T* __restrict__ CS) {
    const int qpad = nch * SM_QC;
    const int64_t gt = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gt >= (n + m) * qpad) return;
    int64_t pt = gt / qpad;
    const int q = (int)(gt % qpad);
    const bool row = pt < n;
    if (!row) pt -= n;
    const T* __restrict__ p = (row ? X : Y) + pt * d;
    double c = 0.0, s = 0.0;
    if (q < ncomp) {
        double u = 0.0;
        for (int k = 0; k < d; ++k) u = __builtin_fma((double)mu[q * d + k], (double)p[k], u);
        const double f = u - __builtin_rint(u);                  // exact; a non-finite u gives NaN
        sincospi(2.0 * f, &s, &c);
    }
    const int ch = q / SM_QC, ql = q % SM_QC;
    if (row) {
        RS[((int64_t)(ch * 2 * SM_QC + ql)) * n + pt] = (T)c;
        RS[((int64_t)(ch * 2 * SM_QC + SM_QC + ql)) * n + pt] = (T)s;
    } else {
        const double wq = q < ncomp ? (double)w[q] : 0.0;
        T* o = CS + (pt * nch + ch) * (2 * SM_QC);
        o[ql] = (T)(wq * c);
        o[SM_QC + ql] = (T)(wq * s);
    }
}

inline int sm_check_points(const covgram_sm* S, const covgram_points* X, const covgram_points* Y) {
    CG_REQUIRE(S != nullptr, COVGRAM_EINVAL, "spectral-mixture handle is NULL");
    CG_REQUIRE(X && Y, COVGRAM_EINVAL, "NULL argument");
    CG_REQUIRE(X->ctx == S->ctx && Y->ctx == S->ctx, COVGRAM_EINVAL, "points belong to a different ctx");
    CG_REQUIRE(X->dtype == S->dtype && Y->dtype == S->dtype, COVGRAM_EINVAL, "points and mixture have different dtypes");
    CG_REQUIRE(X->d == S->d && Y->d == S->d, COVGRAM_EINVAL, "DimensionMismatch: the mixture has d = %d, the points %d and %d", S->d, X->d, Y->d);
    return COVGRAM_OK;
}

}  // namespace covgram
