// mixed_bilin_grad.hpp — the per-pair jets of covgram_bilinear_grad_mixed (mixed_bilin_grad.hip): for one factor
// psi = phi(z)^power of a mixed-trait composite, on the argument of its own trait,
//     v  = psi
//     zd = z dpsi/dz          isotropic factors only (z = r^2 / l^2; 0 where z == 0, never 0 * inf)
//     dp = dpsi/dtheta        RQ alpha, gamma-exponential gamma, IMQ c (bg_jet's forms), NeuralNetwork sigma; 0 otherwise
// and the layout of the entry's 24 outputs.  The family is a template argument: the kernel dispatches once per group of pairs.
#pragma once
#include "bilin_common.hpp"

namespace covgram {

constexpr int MBG_NOUT = COVGRAM_MIXED_GRAD_NOUT;       // 24 = EXPR_MAXT + 2 EXPR_MAXF
constexpr int MBG_Z0 = EXPR_MAXT;                        // out[8 + f]
constexpr int MBG_P0 = EXPR_MAXT + EXPR_MAXF;            // out[16 + f]
static_assert(MBG_NOUT == EXPR_MAXT + 2 * EXPR_MAXF, "layout of out");

__host__ __device__ constexpr bool mbg_dot_family(int fam) { return fam == COVGRAM_DOT || fam == COVGRAM_EXPDOT || fam == COVGRAM_ASINDOT; }
__host__ __device__ constexpr bool mbg_has_param(int fam) {
    return fam == COVGRAM_RQ || fam == COVGRAM_GAMMAEXP || fam == COVGRAM_IMQ || fam == COVGRAM_NEURALNETWORK;
}

// the argument of a factor's own trait, exactly as mixed_value (mixed_mvm.hpp) forms it
template <int F, typename T>
__device__ __forceinline__ T mbg_argument(const KParams<T>& kq, T r2, T p, T q, T s) {
    if constexpr (F == COVGRAM_NEURALNETWORK) {
        const T sg = kq.param;
        return (p + sg) * cg_rsqrt(((T)1 + q + sg) * ((T)1 + s + sg));
    } else if constexpr (mbg_dot_family(F)) {
        return p;
    } else {
        return r2 * kq.gamma2;
    }
}

// psi of one factor on its argument
template <int F, typename T>
__device__ __forceinline__ T mbg_value(T z, const KParams<T>& kq) {
    constexpr int PF = F == COVGRAM_NEURALNETWORK ? COVGRAM_ASINDOT : F;
    const T v = Phi<PF, T, false>::eval(z, kq);
    return kq.power == 1 ? v : ipow(v, kq.power);
}

// (v, zd, dp) of one factor; cpar: IMQ's c as the struct holds it (kq.param is c^2); p, q, s: NeuralNetwork only
template <int F, typename T>
__device__ __forceinline__ void mbg_jet(T z, const KParams<T>& kq, T cpar, T p, T q, T s, T& v, T& zd, T& dp) {
    T f, f1 = (T)0, f2, fp = (T)0;
    if constexpr (F == COVGRAM_NEURALNETWORK) {
        // d/dsigma of (2/pi) asin((p + sigma) / sqrt(A B)), A = 1 + q + sigma, B = 1 + s + sigma:
        //     (2/pi) [1 - (p + sigma)(A + B) / (2 A B)] / sqrt(A B - (p + sigma)^2),   A B - (p + sigma)^2 >= 1 + |x~|^2 + |y~|^2
        const T sg = kq.param;
        const T A = (T)1 + q + sg, B = (T)1 + s + sg;
        const T AB = A * B, num = p + sg;
        f = (T)0.63661977236758134308 * asin(z);
        const T rad = cg_fma(-num, num, AB);
        const T br = cg_fma((T)-0.5 * num * (A + B), cg_rcp(AB), (T)1);
        fp = (T)0.63661977236758134308 * br * cg_rsqrt(rad);
    } else if constexpr (F == COVGRAM_DOT || F == COVGRAM_EXPDOT || F == COVGRAM_ASINDOT) {
        f = Phi<F, T, false>::eval(z, kq);                          // no lengthscale, no parameter: the value alone
    } else {
        DPhi<F, T>::eval(z, kq, f, f1, f2);
        if constexpr (F == COVGRAM_RQ) {
            const T x = z * kq.c0;                                  // z / (2 alpha)
            fp = f * (x * cg_rcp((T)1 + x) - bg_log1p(x));
        } else if constexpr (F == COVGRAM_GAMMAEXP) {
            const T sg = (kq.param == (T)0) ? (T)1 : pow_pos(z, kq.param);
            fp = z == (T)0 ? (T)0 : (T)-0.25 * f * sg * cg_log(z);  // the finite limit 0 at z = 0
        } else if constexpr (F == COVGRAM_IMQ) {
            fp = -cpar * f * cg_rcp(z + kq.param);
        }
    }
    v = f;
    if (kq.power != 1) {                                            // (phi^q)' = q phi^(q - 1) phi', in z and in the parameter alike
        const T fq1 = ipow(f, kq.power - 1);
        const T mult = (T)kq.power * fq1;
        v = fq1 * f; f1 *= mult; fp *= mult;
    }
    zd = z == (T)0 ? (T)0 : z * f1;                                 // z = 0: Exponential, GammaExponential and MaternP(0) have unbounded phi' there
    dp = fp;
}

}  // namespace covgram
