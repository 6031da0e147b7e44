// block_matrix.hpp — dense instantiation of the matrix-valued ("block") Gramians (covgram_block_matrix): the (n B) x (m B) matrix whose
// B x B block (i, j) is what covgram_grad_mvm / covgram_valgrad_mvm / covgram_hess_mvm / covgram_valgradhess_mvm apply, column-major,
// point-major blocks (B = d, d + 1, d^2, 1 + d + d^2).
//
// One formula for every kind.  A row of a block is a functional on x_i of order o in {0: value, 1: d/dx_a, 2: d^2/dx_a dx_b}, a column one on
// y_j of order oc with indices (c, e); an entry is the derivative of k of total order n = o + oc.  With "empty" index slots (rho = kappa = 1,
// every Kronecker delta that touches an empty slot = 0):
//   isotropic  k = f(s), s = |r|^2, r = gamma (x_i - y_j), h_t = 2^t f^(t)(s); rho = (r_a, r_b), kappa = (r_c, r_e); sign (-1)^oc
//   dot prod.  k = f(s), s = x . y,                         h_t =     f^(t)(s); rho = (y_a, y_b), kappa = (x_c, x_e); deltas of one side (ab, ce) dropped
//       T = h_(n-2) (d_ab d_ce + d_ac d_be + d_ae d_bc)
//         + h_(n-1) (d_ab k_c k_e + d_ce r_a r_b + d_ac r_b k_e + d_ae r_b k_c + d_bc r_a k_e + d_be r_a k_c) + h_n r_a r_b k_c k_e,
// times scale gamma^n: -2 k' I - 4 k'' r r' for the gradient block, DESIGN.md §3.8 / §3.9 for the Hessian ones.  Per pair the thread groups it as
//   T = k_c (k_e A2 + A3) + d_ce A1 + d_ac A4 + d_bc A5     (A1, A2 per pair; A3, A4, A5 per pair and e):   one multiply and three selects per entry.
//
// Lane map (the kernel is bound by its stores: one jet feeds B^2 entries).  Lanes run along the flat row index I = i B + p, VR consecutive rows
// per thread (VR | B, so they belong to one point): consecutive lanes write consecutive addresses of a column, one streaming store of VR
// scalars per column and thread.  A thread keeps x_i in registers, walks the block columns j of its strip, reads y_j through wave-uniform
// (scalar) loads (and y_j[a], y_j[b] of its own rows through per-lane loads), evaluates r, s and the jet ONCE per (i, j) and then emits the B columns of that block column.  r is a direct difference
// (x - y) gamma; the entries do not depend on VR, ldo or the alignment of out.  No LDS, no atomics, no scratch.
#pragma once
#include "dispatch.hpp"
#include "profiles.hpp"
#include "hess_mvm.hpp"   // COVGRAM_HESS_FAMILIES: the families of the Hessian kinds
#include <type_traits>

namespace covgram {

constexpr int BM_THREADS = 256;
constexpr int BM_MAX_GRID_Y = 65535;

struct BlockMatArgs {
    const void* X; int64_t n;
    const void* Y; int64_t m;
    int32_t d, parts;                 // parts of a block besides the Hessian one: bit 0 the value row / column, bit 1 the d gradient ones
    void* out; int64_t ldo;
    int32_t Dpad, vr, hess;           // compiled dimension bucket; scalars per store; hess: blocks with Hessian rows / columns
    int32_t W;                        // block columns per strip
    const HostKernel* hk;
    hipStream_t stream;
};
typedef int (*bm_launch_fn)(const BlockMatArgs&, int dtype);
bm_launch_fn block_matrix_launcher(int tu_family);        // gradient kinds: every family
bm_launch_fn block_matrix_hess_launcher(int tu_family);   // Hessian kinds: nullptr where the family has no fourth derivative compiled

inline int bm_pad_dim(int d, bool hess) {
    int D = 4;
    while (D < d) D *= 2;
    return (D <= (hess ? 32 : 64)) ? D : -1;
}

template <typename T> __device__ __forceinline__ T bm_pick(const T (&h)[5], int t) {
    T v = (T)0;                        // t < 0: the term does not exist (its deltas are zero anyway)
#pragma unroll
    for (int q = 0; q < 5; ++q) v = (t == q) ? h[q] : v;
    return v;
}

// HO = false: gradient / value-gradient blocks (jets up to phi''), HO = true: Hessian / value-gradient-Hessian blocks (DPhi5).
// JT: the type the jet is evaluated in.  The gradient kinds take every family, and the fp32 closed forms of phi', phi'' of the Matern
// profiles lose up to 1e-4 of a single pair's value next to their Taylor switch — invisible in an MVM row, a miss of the entrywise 1e-5
// here — so their fp32 instances evaluate the jet of s in fp64 (JT = double): once per pair for B^2 stores, it stays hidden.
template <int FAM, typename T, int D, int VR, bool HO, typename JT>
__global__ __launch_bounds__(BM_THREADS) void block_matrix_kernel(const T* __restrict__ X, int64_t n, const T* __restrict__ Y, int64_t m, int32_t d,
                                                                  int32_t parts, T* __restrict__ out, int64_t ldo, int32_t W, T scale,
                                                                  const typename ParamsOf<FAM, JT>::type kp) {
    constexpr bool ISO = fam_is_iso<FAM>;
    const int vflag = parts & 1, gd = (parts & 2) ? d : 0;     // gradient rows / columns: all kinds but the Hessian alone
    const int B = vflag + gd + (HO ? d * d : 0);
    const int64_t NB = n * (int64_t)B;
    const int64_t I0 = ((int64_t)blockIdx.x * BM_THREADS + threadIdx.x) * VR;
    if (I0 >= NB) return;
    const int64_t i = I0 / B;
    const int p0 = (int)(I0 - i * B);
    const T gam = (T)kp.gamma;
    const T* xi = X + i * (int64_t)d;

    T x[D];
#pragma unroll
    for (int l = 0; l < D; ++l) x[l] = (l < d) ? xi[l] : (T)0;

    // the thread's VR row functionals: order, indices (a, b; -1 = empty), its own coordinates at them, d_ab, scale gamma^order
    int ro[VR], ra[VR], rb[VR];
    T xa[VR], xb[VR], dab[VR], wr[VR];
#pragma unroll
    for (int r = 0; r < VR; ++r) {
        int p = p0 + r, o, a = -1, b = -1;
        if (vflag && p == 0) o = 0;
        else {
            p -= vflag;
            if (p < gd) { o = 1; a = p; }
            else { p -= gd; o = 2; b = p / d; a = p - b * d; }
        }
        ro[r] = o; ra[r] = a; rb[r] = b;
        xa[r] = a >= 0 ? xi[a] : (T)0;
        xb[r] = b >= 0 ? xi[b] : (T)0;
        dab[r] = (ISO && o == 2 && a == b) ? (T)1 : (T)0;
        wr[r] = scale * (o == 0 ? (T)1 : (o == 1 ? gam : gam * gam));
    }
    typedef T VT __attribute__((ext_vector_type(VR)));
    auto store = [&](T* __restrict__ col, const T (&v)[VR]) {
        if constexpr (VR == 1) __builtin_nontemporal_store(v[0], col);
        else {
            VT vv;
#pragma unroll
            for (int r = 0; r < VR; ++r) vv[r] = v[r];
            __builtin_nontemporal_store(vv, reinterpret_cast<VT*>(col));
        }
    };

    for (int64_t jb = (int64_t)blockIdx.y * W; jb < m; jb += (int64_t)gridDim.y * W) {
        const int64_t jend = (jb + W < m) ? jb + W : m;
        for (int64_t j = jb; j < jend; ++j) {
            const T* __restrict__ yj = Y + j * (int64_t)d;
            // kappa: the column side's vector (r, or x), s, and the jet — once per (i, j)
            // (dot product with the jet in fp64: x . y is summed in fp64 too — its fp32 sum cancels, and phi'' of a Power of Dot is linear in it)
            constexpr bool WIDE_S = !ISO && !std::is_same<JT, T>::value;
            T kap[D];
            T s = (T)0;
            [[maybe_unused]] JT sw = (JT)0;
#pragma unroll
            for (int l = 0; l < D; ++l) {
                const int lc = l < d ? l : d - 1;                   // in-bounds (clamped) uniform load, then a select
                const T yv = yj[lc];
                const T yl = l < d ? yv : (T)0;
                if constexpr (ISO) { kap[l] = (x[l] - yl) * gam; s = cg_fma(kap[l], kap[l], s); }
                else {
                    kap[l] = x[l] * gam;
                    if constexpr (WIDE_S) sw = cg_fma((JT)kap[l], (JT)(yl * gam), sw);
                    else s = cg_fma(kap[l], yl * gam, s);
                }
            }
            JT sj;
            if constexpr (WIDE_S) sj = sw; else sj = (JT)s;
            T h[5];
            if constexpr (HO) {
                DPhi5<FAM, T>::eval(s, kp, h[0], h[1], h[2], h[3], h[4]);
                if constexpr (ISO) { h[1] *= (T)2; h[2] *= (T)4; h[3] *= (T)8; h[4] *= (T)16; }
            } else {
                JT j0, j1, j2;
                if constexpr (FAM == FAM_EXPR_ISO) expr_jet<JT, true, false>(sj, kp, j0, j1, j2);
                else if constexpr (FAM == FAM_EXPR_DOT) expr_jet<JT, false, false>(sj, kp, j0, j1, j2);
                else {
                    phi_jet<FAM, JT, false>(sj, kp, j0, j1, j2);
                    if (kp.power != 1) power_jet(kp.power, j0, j1, j2);
                }
                h[0] = (T)j0; h[1] = (T)j1; h[2] = (T)j2;
                if constexpr (ISO) { h[1] *= (T)2; h[2] *= (T)4; }
                h[3] = (T)0; h[4] = (T)0;
            }
            T rhoa[VR], rhob[VR];
#pragma unroll
            for (int r = 0; r < VR; ++r) {
                const T ya = ra[r] >= 0 ? yj[ra[r]] : (T)0, yb = rb[r] >= 0 ? yj[rb[r]] : (T)0;
                rhoa[r] = ra[r] >= 0 ? (ISO ? (xa[r] - ya) * gam : ya * gam) : (T)1;
                rhob[r] = rb[r] >= 0 ? (ISO ? (xb[r] - yb) * gam : yb * gam) : (T)1;
            }
            T* __restrict__ oc = out + I0 + (j * (int64_t)B) * ldo;
            // G0, G1, G2 = w h_n, w h_(n-1), w h_(n-2) for a column section of order OC
            auto coefs = [&](int r, int OC, T& G0, T& G1, T& G2) {
                const int nn = ro[r] + OC;
                T w = wr[r] * (OC == 0 ? (T)1 : (OC == 1 ? gam : gam * gam));
                if (ISO && OC == 1) w = -w;
                G0 = w * bm_pick(h, nn); G1 = w * bm_pick(h, nn - 1); G2 = w * bm_pick(h, nn - 2);
            };
            // ---- the value column --------------------------------------------------------------------------------
            if (vflag) {
                T v[VR];
#pragma unroll
                for (int r = 0; r < VR; ++r) {
                    T G0, G1, G2;
                    coefs(r, 0, G0, G1, G2);
                    v[r] = cg_fma(G0, rhoa[r] * rhob[r], G1 * dab[r]);
                }
                store(oc, v);
            }
            // ---- the d gradient columns ---------------------------------------------------------------------------
            if (gd) {
                T A2[VR], A4[VR], A5[VR];
#pragma unroll
                for (int r = 0; r < VR; ++r) {
                    T G0, G1, G2;
                    coefs(r, 1, G0, G1, G2);
                    A2[r] = cg_fma(G0, rhoa[r] * rhob[r], G1 * dab[r]);
                    A4[r] = G1 * rhob[r];
                    A5[r] = G1 * rhoa[r];
                }
                T* __restrict__ og = oc + (int64_t)vflag * ldo;
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    if (c < d) {
                        T v[VR];
#pragma unroll
                        for (int r = 0; r < VR; ++r) {
                            T t = kap[c] * A2[r];
                            t += (ra[r] == c) ? A4[r] : (T)0;
                            t += (rb[r] == c) ? A5[r] : (T)0;
                            v[r] = t;
                        }
                        store(og + (int64_t)c * ldo, v);
                    }
                }
            }
            // ---- the d^2 Hessian columns, component (c, e) at c + e d ----------------------------------------------
            if constexpr (HO) {
                T G0[VR], G1[VR], G2[VR], A1[VR], A2[VR];
#pragma unroll
                for (int r = 0; r < VR; ++r) {
                    coefs(r, 2, G0[r], G1[r], G2[r]);
                    const T pr = rhoa[r] * rhob[r];
                    A1[r] = ISO ? cg_fma(G1[r], pr, G2[r] * dab[r]) : (T)0;
                    A2[r] = cg_fma(G0[r], pr, G1[r] * dab[r]);
                }
                T* __restrict__ oh = oc + (int64_t)(vflag + gd) * ldo;
                for (int e = 0; e < d; ++e) {
                    T ke = kap[0];                                   // kappa_e: e is wave-uniform, a select chain over the registers
#pragma unroll
                    for (int c = 1; c < D; ++c) ke = (e == c) ? kap[c] : ke;
                    T Ce[VR], A4[VR], A5[VR], A1e[VR];
#pragma unroll
                    for (int r = 0; r < VR; ++r) {
                        const T dae = (ra[r] == e) ? (T)1 : (T)0, dbe = (rb[r] == e) ? (T)1 : (T)0;
                        Ce[r] = cg_fma(ke, A2[r], G1[r] * (dae * rhob[r] + dbe * rhoa[r]));
                        A4[r] = cg_fma(G1[r] * rhob[r], ke, G2[r] * dbe);
                        A5[r] = cg_fma(G1[r] * rhoa[r], ke, G2[r] * dae);
                    }
                    T* __restrict__ oe = oh + (int64_t)e * d * ldo;
#pragma unroll
                    for (int c = 0; c < D; ++c) {
                        if (c < d) {
                            T v[VR];
#pragma unroll
                            for (int r = 0; r < VR; ++r) {
                                T t = kap[c] * Ce[r];
                                t += (c == e) ? A1[r] : (T)0;
                                t += (ra[r] == c) ? A4[r] : (T)0;
                                t += (rb[r] == c) ? A5[r] : (T)0;
                                v[r] = t;
                            }
                            store(oe + (int64_t)c * ldo, v);
                        }
                    }
                }
            }
        }
    }
}

template <int FAM, typename T, int D, bool HO>
inline int launch_bm_one(const BlockMatArgs& a) {
    constexpr int VRW = 16 / (int)sizeof(T);
    const int B = (a.parts & 1) + ((a.parts & 2) ? a.d : 0) + (HO ? a.d * a.d : 0);
    const int64_t NB = a.n * (int64_t)B;
    const int vr = a.vr;
    const int64_t strips = (a.m + a.W - 1) / a.W;
    const dim3 grid((unsigned)((NB / vr + BM_THREADS - 1) / BM_THREADS), (unsigned)(strips < BM_MAX_GRID_Y ? strips : BM_MAX_GRID_Y));
    using JT = std::conditional_t<(!HO && sizeof(T) == 4), double, T>;
    const typename ParamsOf<FAM, JT>::type kp = make_params<FAM, JT>(*a.hk);
    if (vr == VRW)
        hipLaunchKernelGGL((block_matrix_kernel<FAM, T, D, VRW, HO, JT>), grid, dim3(BM_THREADS), 0, a.stream, (const T*)a.X, a.n, (const T*)a.Y, a.m, a.d,
                           a.parts, (T*)a.out, a.ldo, a.W, (T)a.hk->kp.scale, kp);
    else
        hipLaunchKernelGGL((block_matrix_kernel<FAM, T, D, 1, HO, JT>), grid, dim3(BM_THREADS), 0, a.stream, (const T*)a.X, a.n, (const T*)a.Y, a.m, a.d,
                           a.parts, (T*)a.out, a.ldo, a.W, (T)a.hk->kp.scale, kp);
    return COVGRAM_OK;
}

template <int FAM, typename T, bool HO>
inline int launch_bm_typed(const BlockMatArgs& a) {
    using Buckets = std::conditional_t<HO, Dims<4, 8, 16, 32>, Dims<4, 8, 16, 32, 64>>;
    return by_dim(Buckets{}, a.Dpad, "block matrix: no kernel for padded d = %d", [&](auto D) { return launch_bm_one<FAM, T, decltype(D)::value, HO>(a); });
}

template <int FAM, bool HO>
inline int launch_bm_family(const BlockMatArgs& a, int dtype) {
    return dtype == COVGRAM_F64 ? launch_bm_typed<FAM, double, HO>(a) : launch_bm_typed<FAM, float, HO>(a);
}

}  // namespace covgram
