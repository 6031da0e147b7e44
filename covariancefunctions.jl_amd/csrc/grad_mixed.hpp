// grad_mixed.hpp — GradientKernel / ValueGradientKernel Gramian MVM of a Sum / Product / Power whose factors do NOT share one input
// trait (the reference's gradient algebra, src/gradient_algebra.jl:6-36 Sum, :47-89 Product; its README example
// MaternP(2) + Dot()^2 + NN()), in ONE pass of the shape of the single-trait gradient MVM (grad_mvm.hpp / grad_wide.hpp).
//
// Every supported leaf is a function of three scalars of the pair, p = x.y, q = |x|^2, s = |y|^2, and so are their sums, products and
// integer powers.  With k(x, y) = F(p, q, s):
//     grad_x k = F_p y + 2 F_q x        grad_y k = F_p x + 2 F_s y
//     d_x d_y' k = F_p I + y (F_pp x + 2 F_ps y)' + 2 x (F_qp x + 2 F_qs y)'
// so the block product with t = x_i.a_j (per pair) and w = y_j.a_j (per column) is
//     b_i += F_p a_j + (F_pp t + 2 F_ps w) y_j + 2 (F_qp t + 2 F_qs w) x_i                                   O(d) per pair
// and the value-gradient blocks (value row = grad_y k, value column = grad_x k) add
//     b0 += F a0 + F_p t + 2 F_s w,     F_p a0 on the y_j coefficient,     2 F_q a0 on the x_i coefficient.
// The x_i coefficient is a scalar per pair: it is summed over the columns and multiplies x_i ONCE per row.
// A node of the expression carries the jet (F, F_p, F_q, F_s, F_pp, F_ps, F_qp, F_qs): a Sum adds jets, a Product combines them by
// the Leibniz rules (the set is closed under both), Power(n) is the chain rule on the leaf's profile.  Leaves, as phi(u):
//     isotropic       u = g^2 |x - y|^2 by DIRECT differences (src/util.jl:40-47; a mixed kernel has no common centre to subtract, so the
//                     expanded form's cancellation is not acceptable here), u_p = -2 g^2, u_q = u_s = g^2; every leaf its own g = 1 / l
//     dot product     u = p
//     NeuralNetwork   phi = (2/pi) asin, A = 1 + q + sigma, B = 1 + s + sigma, D = (A B)^(-1/2), u = (p + sigma) D   (src/mercer.jl:82-85)
//                     u_p = D, u_q = -u / 2A, u_s = -u / 2B, u_ps = -D / 2B, u_qp = -D / 2A, u_qs = u / 4AB
// A product that vanishes at a pair is an ordinary number (the reference needs a Woodbury object per pair and throws there).
//
// MI355X mapping, as the single-trait siblings':
//   lane per block row (padded d <= 32): x_i, b_i and q_i in VGPRs; the column record (y_j, a_j, s_j, w_j, a0_j) is wave-uniform and
//     arrives through the scalar data cache; sweep 1 accumulates r^2, p, t, the interpreter walks the factors with wave-uniform control
//     flow, sweep 2 is two FMAs per dimension; grid = (row blocks) x (column splits) with the slab reduce of grad_reduce_kernel;
//   panel route (wider d): grad_mixed_coef_kernel walks 32-wide chunks for 4 column groups at a time and stores two coefficients per
//     block (F_p and the y_j coefficient) plus, per column block, the partial sums of the x_i coefficient and of the value row;
//     grad_mixed_apply_kernel keeps 32 coordinates of b_i over the panel and adds x_i times the summed coefficient once.
#pragma once
#include "grad_mvm.hpp"
#include "grad_wide.hpp"

namespace covgram {

constexpr int MIX_THREADS = 256;
constexpr int MIX_EXTRA = 4;          // scalars behind (y_j, a_j) in a column record: s_j, w_j, a0_j, one of padding
constexpr int MIX_CG = 4;             // column groups the coefficient kernel carries through one walk of the dimension

template <typename T>
struct MixJet { T v, p, q, s, pp, ps, qp, qs; };

// the jet of ONE leaf (its Power applied to the profile's own jet first)
template <typename T>
__device__ __forceinline__ void mixed_leaf(int fam, const KParams<T>& kp, T r2, T p, T q, T s, MixJet<T>& L) {
    if (fam == COVGRAM_NEURALNETWORK) {
        const T sg = kp.param;
        const T A = (T)1 + q + sg, B = (T)1 + s + sg, AB = A * B;
        const T D = cg_rsqrt(AB), iA = cg_rcp(A), iB = cg_rcp(B);
        const T w = p + sg;
        const T u = w * D;
        const T c = (T)0.63661977236758134308;
        const T iq = cg_rsqrt(cg_fma(-w, w, AB) * (D * D));         // 1 - u^2 = (A B - (p + sigma)^2) / (A B)
        T f0 = c * asin(u), f1 = c * iq, f2 = c * u * iq * iq * iq;
        if (kp.power != 1) power_jet(kp.power, f0, f1, f2);
        const T hu = (T)-0.5 * u, hD = (T)-0.5 * D;
        const T uq = hu * iA, us = hu * iB;
        L.v = f0; L.p = f1 * D; L.q = f1 * uq; L.s = f1 * us;
        L.pp = f2 * D * D;
        L.ps = cg_fma(f2 * D, us, f1 * hD * iB);
        L.qp = cg_fma(f2 * D, uq, f1 * hD * iA);
        L.qs = cg_fma(f2 * uq, us, f1 * (T)0.25 * u * iA * iB);
    } else if (fam == COVGRAM_DOT || fam == COVGRAM_EXPDOT || fam == COVGRAM_ASINDOT) {
        T f0, f1, f2;
        jet_any<T, true>(fam, p, kp, f0, f1, f2);
        L.v = f0; L.p = f1; L.q = (T)0; L.s = (T)0; L.pp = f2; L.ps = (T)0; L.qp = (T)0; L.qs = (T)0;
    } else {
        const T g2 = kp.gamma2;
        T f0, f1, f2;
        jet_any<T, true>(fam, r2 * g2, kp, f0, f1, f2);
        const T a1 = f1 * g2, a2 = f2 * g2 * g2;
        L.v = f0; L.p = (T)-2 * a1; L.q = a1; L.s = a1; L.pp = (T)4 * a2; L.ps = (T)-2 * a2; L.qp = (T)-2 * a2; L.qs = a2;
    }
}

// the composite's jet: sum over the terms of the Leibniz product of the term's leaves (coef[t]: the term's folded constants)
template <typename T>
__device__ __forceinline__ void mixed_jet(const ExprParams<T>& ep, T r2, T p, T q, T s, MixJet<T>& F) {
    F.v = F.p = F.q = F.s = F.pp = F.ps = F.qp = F.qs = (T)0;
    int fi = 0;
    for (int t = 0; t < ep.nterms; ++t) {
        MixJet<T> P;
        P.v = ep.coef[t];
        P.p = P.q = P.s = P.pp = P.ps = P.qp = P.qs = (T)0;
        for (int f = 0; f < ep.nfac[t]; ++f, ++fi) {
            MixJet<T> L, N;
            mixed_leaf<T>(ep.fam[fi], ep.f[fi], r2, p, q, s, L);
            N.pp = cg_fma(P.pp, L.v, cg_fma((T)2 * P.p, L.p, P.v * L.pp));
            N.ps = cg_fma(P.ps, L.v, cg_fma(P.p, L.s, cg_fma(P.s, L.p, P.v * L.ps)));
            N.qp = cg_fma(P.qp, L.v, cg_fma(P.q, L.p, cg_fma(P.p, L.q, P.v * L.qp)));
            N.qs = cg_fma(P.qs, L.v, cg_fma(P.q, L.s, cg_fma(P.s, L.q, P.v * L.qs)));
            N.p = cg_fma(P.p, L.v, P.v * L.p);
            N.q = cg_fma(P.q, L.v, P.v * L.q);
            N.s = cg_fma(P.s, L.v, P.v * L.s);
            N.v = P.v * L.v;
            P = N;
        }
        F.v += P.v; F.p += P.p; F.q += P.q; F.s += P.s; F.pp += P.pp; F.ps += P.ps; F.qp += P.qp; F.qs += P.qs;
    }
}

// what one pair contributes beside F_p a_j: the y_j coefficient, HALF the x_i coefficient and the value row's term
template <typename T, bool VG>
__device__ __forceinline__ void mixed_coefs(const MixJet<T>& F, T t, T w, T a0, T& cy, T& cx, T& b0) {
    const T w2 = (T)2 * w;
    cy = cg_fma(F.pp, t, F.ps * w2);
    cx = cg_fma(F.qp, t, F.qs * w2);
    b0 = (T)0;
    if constexpr (VG) {
        cy = cg_fma(F.p, a0, cy);
        cx = cg_fma(F.q, a0, cx);
        b0 = cg_fma(F.v, a0, cg_fma(F.p, t, F.s * w2));
    }
}

// ---- lane per block row -------------------------------------------------------------------------------------------------------------
// registers: x_i and b_i are 2 d-vectors; the interpreter keeps three jets live (24 scalars) beside the profile's own temporaries
template <typename T, int D>
constexpr int mixed_min_waves() {
    const int state = 2 * D * (int)(sizeof(T) / 4);
    const int w = 512 / (state + (sizeof(T) == 8 ? 120 : 72));
    return w < 1 ? 1 : (w > 8 ? 8 : w);
}

// P[j] = (y_j[0..D), a_j[0..D), s_j = |y_j|^2, w_j = y_j . a_j, a0_j, 0), zero padded; vg = 1: A holds blocks of d + 1, value weight first
template <typename T>
__global__ __launch_bounds__(256) void grad_mixed_pack_kernel(const T* __restrict__ Y, int64_t m, int32_t d, const T* __restrict__ A, T* __restrict__ P,
                                                              int32_t D, int32_t vg) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * (int64_t)D) return;
    const int64_t j = e / D;
    const int l = (int)(e - j * D);
    T* p = P + j * (int64_t)(2 * D + MIX_EXTRA);
    const T* yr = Y + j * (int64_t)d;
    const T* ar = A + j * (int64_t)(d + vg) + vg;
    p[l] = l < d ? yr[l] : (T)0;
    p[D + l] = l < d ? ar[l] : (T)0;
    if (l == 0) {
        T s = (T)0, w = (T)0;
        for (int c = 0; c < d; ++c) { s = cg_fma(yr[c], yr[c], s); w = cg_fma(yr[c], ar[c], w); }
        p[2 * D] = s; p[2 * D + 1] = w; p[2 * D + 2] = vg ? ar[-1] : (T)0; p[2 * D + 3] = (T)0;
    }
}

template <typename T, int D, bool VG>
__global__ __launch_bounds__(MIX_THREADS, (mixed_min_waves<T, D>())) void grad_mixed_lane_kernel(const T* __restrict__ X, int64_t n, int32_t d,
                                                                                                 const T* __restrict__ P, int64_t m, T* __restrict__ out,
                                                                                                 int64_t npad, int64_t jchunk, T alpha, T beta,
                                                                                                 int32_t final_store, const ExprParams<T> kp) {
    constexpr int RS = 2 * D + MIX_EXTRA;
    int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = row < n;
    if (!live) row = n - 1;
    const int64_t j0 = (int64_t)blockIdx.y * jchunk;
    const int64_t j1 = (j0 + jchunk < m) ? (j0 + jchunk) : m;

    T x[D], b[D];
    T q = (T)0;
    {
        const T* xr = X + row * (int64_t)d;
#pragma unroll
        for (int l = 0; l < D; ++l) {
            x[l] = (l < d) ? xr[l] : (T)0;
            b[l] = (T)0;
            q = cg_fma(x[l], x[l], q);
        }
    }
    T csum = (T)0, b0 = (T)0;
    const T* __restrict__ rec = P + j0 * RS;          // uniform addresses: the record arrives as scalar operands
    for (int64_t j = j0; j < j1; ++j, rec += RS) {
        T r2 = (T)0, p = (T)0, t = (T)0;
#pragma unroll
        for (int l = 0; l < D; ++l) {
            const T yl = rec[l];
            const T rl = x[l] - yl;
            r2 = cg_fma(rl, rl, r2);
            p = cg_fma(x[l], yl, p);
            t = cg_fma(x[l], rec[D + l], t);
        }
        MixJet<T> F;
        mixed_jet<T>(kp, r2, p, q, rec[2 * D], F);
        T cy, cx, v0;
        mixed_coefs<T, VG>(F, t, rec[2 * D + 1], VG ? rec[2 * D + 2] : (T)0, cy, cx, v0);
        csum += cx;
        b0 += v0;
        const T c1 = F.p;
#pragma unroll
        for (int l = 0; l < D; ++l) b[l] = cg_fma(cy, rec[l], cg_fma(c1, rec[D + l], b[l]));
    }
    csum *= (T)2;
#pragma unroll
    for (int l = 0; l < D; ++l) b[l] = cg_fma(x[l], csum, b[l]);

    if (!live) return;
    constexpr int VGI = VG ? 1 : 0;
    if (final_store) {
        T* yp = out + row * (int64_t)(d + VGI);
        if constexpr (VG) {
            T v = alpha * b0;
            if (beta != (T)0) v = cg_fma(beta, yp[0], v);
            yp[0] = v;
        }
#pragma unroll
        for (int l = 0; l < D; ++l) {
            if (l < d) {
                T v = alpha * b[l];
                if (beta != (T)0) v = cg_fma(beta, yp[VGI + l], v);
                yp[VGI + l] = v;
            }
        }
    } else {
        // partial slab [jsplit][D (+1: the value row)][npad], the layout grad_reduce_kernel sums
        T* op = out + (int64_t)blockIdx.y * (D + VGI) * npad + row;
#pragma unroll
        for (int l = 0; l < D; ++l) op[(int64_t)l * npad] = b[l];
        if constexpr (VG) op[(int64_t)D * npad] = b0;
    }
}

struct GradMixedArgs {
    const void* X; int64_t n; int32_t d; int32_t Dpad;
    const void* P; int64_t m;
    void* out; int64_t npad; int64_t jchunk; int32_t jsplit;
    int32_t vg;
    double alpha, beta;
    const HostKernel* hk;
    hipStream_t stream;
};

template <typename T, int D>
static int launch_grad_mixed_one(const GradMixedArgs& a) {
    const ExprParams<T> kp = make_params<FAM_EXPR_DOT, T>(*a.hk);
    const dim3 grid((unsigned)((a.n + MIX_THREADS - 1) / MIX_THREADS), (unsigned)a.jsplit);
    const int final_store = a.jsplit == 1 ? 1 : 0;
    by_bool(a.vg != 0, [&](auto vg) {
        hipLaunchKernelGGL((grad_mixed_lane_kernel<T, D, decltype(vg)::value>), grid, dim3(MIX_THREADS), 0, a.stream, (const T*)a.X, a.n, a.d, (const T*)a.P,
                           a.m, (T*)a.out, a.npad, a.jchunk, (T)a.alpha, (T)a.beta, final_store, kp);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("grad_mixed launch failed: %s", hipGetErrorString(e)); return COVGRAM_EHIP; }
    return COVGRAM_OK;
}

template <typename T>
static int launch_grad_mixed_T(const GradMixedArgs& a) {
    return by_dim(Dims<1, 2, 3, 4, 6, 8, 12, 16, 24, 32>{}, a.Dpad, "grad_mixed: padded dimension %d not compiled for the lane-per-row route",
                  [&](auto D) { return launch_grad_mixed_one<T, decltype(D)::value>(a); });
}

// ---- panel route ------------------------------------------------------------------------------------------------------------------------
// The blocked panel stream is grad_wide_pack_kernel's (gamma = 1, no centre); the column scalars go beside it in the same
// [block][group][packed column] order: SW[((block GJG + group) 2 + k) PKN + h], k = 0: s_j, 1: w_j (padding columns: the last point's s, w = 0)
template <typename T>
__global__ __launch_bounds__(256) void grad_mixed_panel_scalars_kernel(const T* __restrict__ Y, int64_t m, int32_t d, const T* __restrict__ A, int64_t col0,
                                                                       int64_t pcols, T* __restrict__ SW, int32_t PKN, int32_t vg) {
    const int64_t jp = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (jp >= pcols) return;
    const int64_t jj = col0 + jp;
    const bool pad = jj >= m;
    const int64_t j = pad ? (m - 1) : jj;
    const T* yr = Y + j * (int64_t)d;
    const T* ar = A + j * (int64_t)(d + vg) + vg;
    T s = (T)0, w = (T)0;
    for (int c = 0; c < d; ++c) { s = cg_fma(yr[c], yr[c], s); w = cg_fma(yr[c], ar[c], w); }
    const int64_t bc = (int64_t)GJG * PKN;
    const int64_t blk = jp / bc;
    const int within = (int)(jp - blk * bc);
    const int g = within / PKN, h = within - g * PKN;
    SW[((blk * GJG + g) * 2 + 0) * PKN + h] = s;
    SW[((blk * GJG + g) * 2 + 1) * PKN + h] = pad ? (T)0 : w;
}

// one of four values by a uniform index (the register arrays below are never indexed dynamically)
template <typename V>
__device__ __forceinline__ V mixed_pick(const V (&a)[MIX_CG], int g) { return g == 0 ? a[0] : (g == 1 ? a[1] : (g == 2 ? a[2] : a[3])); }
__device__ __forceinline__ float mixed_comp(v2f v, int h) { return h == 0 ? v.x : v.y; }
__device__ __forceinline__ double mixed_comp(double v, int) { return v; }

// grid = (row blocks of 64, column blocks).  C1 / C2: [column group][row] slabs of packed columns, as grad_wide_coef_kernel's; CX / C0:
// [column block][row], the block's sums of HALF the x_i coefficient and of the value row
template <typename T, bool VG>
__global__ __launch_bounds__(64) void grad_mixed_coef_kernel(const T* __restrict__ X, int64_t n, int32_t d, int32_t dpad,
                                                             const typename Pk<T>::V* __restrict__ P, const T* __restrict__ SW, const T* __restrict__ A0P,
                                                             T* __restrict__ C1, T* __restrict__ C2, T* __restrict__ CX, T* __restrict__ C0, int64_t npad,
                                                             const ExprParams<T> kp) {
    using PK = Pk<T>;
    using V = typename PK::V;
    constexpr int PKN = PK::N;
    int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int64_t srow = row;
    if (row >= n) row = n - 1;
    const T* __restrict__ xr = X + row * (int64_t)d;
    const int nch = dpad / WIDE_CH;
    const int64_t b = blockIdx.y;
    const V* __restrict__ pb = P + b * (int64_t)nch * 2 * GJG * WIDE_CH;
    T q = (T)0, cxs = (T)0, b0s = (T)0;
#pragma unroll 1
    for (int g0 = 0; g0 < GJG; g0 += MIX_CG) {
        V r2[MIX_CG], pp[MIX_CG], tt[MIX_CG];
#pragma unroll
        for (int g = 0; g < MIX_CG; ++g) { r2[g] = PK::splat((T)0); pp[g] = PK::splat((T)0); tt[g] = PK::splat((T)0); }
        for (int ch = 0; ch < nch; ++ch) {
            T x[WIDE_CH];
            const int l0 = ch * WIDE_CH;
#pragma unroll
            for (int l = 0; l < WIDE_CH; ++l) x[l] = (l0 + l < d) ? xr[l0 + l] : (T)0;
            if (g0 == 0) {
#pragma unroll
                for (int l = 0; l < WIDE_CH; ++l) q = cg_fma(x[l], x[l], q);
            }
            const V* __restrict__ py = pb + (int64_t)ch * (2 * GJG * WIDE_CH) + g0 * WIDE_CH;
            const V* __restrict__ pa = py + GJG * WIDE_CH;
#pragma unroll
            for (int g = 0; g < MIX_CG; ++g) {
                V rg = r2[g], pg = pp[g], tg = tt[g];
#pragma unroll
                for (int q0 = 0; q0 < WIDE_CH; q0 += WIDE_SB) {
#pragma unroll
                    for (int l = q0; l < q0 + WIDE_SB; ++l) {
                        const V xl = PK::splat(x[l]);
                        const V yl = py[g * WIDE_CH + l];
                        const V rl = xl - yl;
                        rg = PK::fma(rl, rl, rg);
                        pg = PK::fma(xl, yl, pg);
                        tg = PK::fma(xl, pa[g * WIDE_CH + l], tg);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                r2[g] = rg; pp[g] = pg; tt[g] = tg;
            }
        }
        // the jets, one packed column at a time: ONE copy of the interpreter in the kernel
#pragma unroll 1
        for (int e = 0; e < MIX_CG * PKN; ++e) {
            const int g = e / PKN, h = e - g * PKN;
            const T r2e = mixed_comp(mixed_pick(r2, g), h), pe = mixed_comp(mixed_pick(pp, g), h), te = mixed_comp(mixed_pick(tt, g), h);
            const int64_t cg = b * GJG + g0 + g;
            const T sj = SW[(cg * 2 + 0) * PKN + h], wj = SW[(cg * 2 + 1) * PKN + h];
            const T a0 = VG ? A0P[cg * PKN + h] : (T)0;
            MixJet<T> F;
            mixed_jet<T>(kp, r2e, pe, q, sj, F);
            T cy, cx, v0;
            mixed_coefs<T, VG>(F, te, wj, a0, cy, cx, v0);
            cxs += cx;
            b0s += v0;
            if (srow < n) {
                C1[(cg * npad + srow) * PKN + h] = F.p;
                C2[(cg * npad + srow) * PKN + h] = cy;
            }
        }
    }
    if (srow >= n) return;
    CX[b * npad + srow] = cxs;
    if constexpr (VG) C0[b * npad + srow] = b0s;
}

// grid = (row blocks of 64, dimension chunks, z slices): 32 coordinates of b_i over the column blocks of the slice,
// b_l += c1 a_jl + c2 y_jl, then + x_il (2 sum of CX) once; alpha / beta / accumulate / z slices as grad_wide_apply_kernel
template <typename T>
__global__ __launch_bounds__(64) void grad_mixed_apply_kernel(const T* __restrict__ X, int64_t n, int32_t d, int32_t dpad,
                                                              const typename Pk<T>::V* __restrict__ P, const typename Pk<T>::V* __restrict__ C1,
                                                              const typename Pk<T>::V* __restrict__ C2, const T* __restrict__ CX,
                                                              const T* __restrict__ C0, int64_t npad, int64_t nblocks, T* __restrict__ y, T alpha, T beta,
                                                              int32_t accumulate, int32_t vg, int64_t zstride) {
    using PK = Pk<T>;
    using V = typename PK::V;
    const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (row >= n) return;                                   // no barriers, no cross-lane traffic below
    const int64_t b_begin = nblocks * blockIdx.z / gridDim.z, b_end = nblocks * (blockIdx.z + 1) / gridDim.z;
    y += (int64_t)blockIdx.z * zstride;
    const int ch = blockIdx.y;
    const int l0 = ch * WIDE_CH;
    const int nch = dpad / WIDE_CH;
    const T* __restrict__ xr = X + row * (int64_t)d;
    V bv[WIDE_CH];
#pragma unroll
    for (int l = 0; l < WIDE_CH; ++l) bv[l] = PK::splat((T)0);
    T cs = (T)0, b0 = (T)0;
    for (int64_t b = b_begin; b < b_end; ++b) {
        const V* __restrict__ py = P + (b * nch + ch) * (int64_t)(2 * GJG * WIDE_CH);
        const V* __restrict__ pa = py + GJG * WIDE_CH;
#pragma unroll 1
        for (int g = 0; g < GJG; ++g) {
            const V c1 = C1[(b * GJG + g) * npad + row];
            const V c2 = C2[(b * GJG + g) * npad + row];
#pragma unroll
            for (int q0 = 0; q0 < WIDE_CH; q0 += WIDE_SB) {
#pragma unroll
                for (int l = q0; l < q0 + WIDE_SB; ++l) bv[l] = PK::fma(c2, py[g * WIDE_CH + l], PK::fma(c1, pa[g * WIDE_CH + l], bv[l]));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        cs += CX[b * npad + row];
        if (vg && ch == 0) b0 += C0[b * npad + row];
    }
    cs *= (T)2;
    if (vg && ch == 0) {
        T* y0 = y + row * (int64_t)(d + 1);
        T v = alpha * b0;
        if (accumulate) v += *y0;
        else if (beta != (T)0) v = cg_fma(beta, *y0, v);
        *y0 = v;
    }
    T* yp = y + row * (int64_t)(d + vg) + vg + l0;
#pragma unroll
    for (int l = 0; l < WIDE_CH; ++l) {
        if (l0 + l < d) {
            T v = alpha * cg_fma(xr[l0 + l], cs, PK::hsum(bv[l]));
            if (accumulate) v += yp[l];
            else if (beta != (T)0) v = cg_fma(beta, yp[l], v);
            yp[l] = v;
        }
    }
}

}  // namespace covgram
