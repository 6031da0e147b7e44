// hess_mvm.hpp — Y <- alpha G A + beta Y for the Hessian-kernel Gramian (covgram_hess_mvm) and the value-gradient-Hessian-kernel
// Gramian (covgram_valgradhess_mvm, VGH below).  Hessian: block (i, j) is the d^2 x d^2 matrix
//     T[(a,b),(c,e)] = d^4 k(x_i, y_j) / dx_a dx_b dy_c dy_e                                  (src/hessian.jl:33-41)
// applied in O(d^2) per pair through its data-sparse form (src/hessian.jl:125-190, 227-275).  With the block input as a d x d matrix
// A, Abar = A + A', t = tr A, and the block output as a d x d matrix B:
//   isotropic  k = f(|r|^2), r = x_i - y_j, g_m = 2^m f^(m):   u = Abar r, q = r'u / 2
//       B = g2 (t I + Abar) + g3 (q I + t r r' + u r' + r u') + g4 q r r'
//   dot product  k = f(x . y), g_m = f^(m), x = x_i, y = y_j:   w = Abar x, q = x'w / 2
//       B = g2 Abar + g3 (y w' + w y') + g4 q y y'
// Both are  B = W + W' + S + c I  with  W[a,:] = coef_a v[:]  (v = r or y), S = g2 Abar, so a lane that owns ROW a of the block
// accumulates W[a,:] and S[a,:] over the columns j and the transpose is taken once, in the epilogue.
//
// Lane map.  D = d rounded up to a power of two (<= 32).  Lane (i, a), a < D, owns row a of the output block of row point i:
// HESS_THREADS / D points per workgroup.  The columns' records — Abar_j (D x D, zero padded), the pre-scaled y_j and tr A_j, formed
// once per MVM by hess_pack_kernel — are staged through LDS in chunks and shared by all points of the workgroup.  Per pair a lane
// forms r (D subtractions of direct differences, src/util.jl:40-47), u_a = Abar[a,:] . r (D fma; the lanes of a point read D
// consecutive LDS words, lanes of different points the same ones), reduces q over the D lanes of its point with DPP moves, and
// updates its 2 D accumulators.  Padded dimensions carry zeros; rows beyond n and lanes a >= d compute and never store.
//
// VGH = true: the value-gradient-Hessian-kernel Gramian (covgram_valgradhess_mvm).  Block (i, j) is the (1 + d + d^2) x (1 + d + d^2)
// joint covariance of [f, grad f, vec hess f] (src/hessian.jl:301-325): entry (row functional on x_i, column functional on y_j) of k,
// the functionals being id, d/d._a and d^2/d._a d._b.  Block input (a_v, a_g, A), A[a, b] = flat entry 1 + d + a + b d, Abar = A + A',
// t = tr A; block output (b_v, b_g, B):
//   isotropic  k = f(|r|^2), r = x_i - y_j, g_m = 2^m f^(m):   u = Abar r, q = r'u / 2, rho = r . a_g,
//       c1 = g1 a_v - g2 rho + g2 t + g3 q,   c2 = g2 a_v - g3 rho + g3 t + g4 q
//       b_v = g0 a_v - g1 rho + g1 t + g2 q
//       b_g = c1 r - g1 a_g + g2 u
//       B   = c1 I + c2 r r' - g2 (a_g r' + r a_g') + g2 Abar + g3 (u r' + r u')
//   dot product  k = f(x . y), g_m = f^(m), x = x_i, y = y_j:   w = Abar x, q = x'w / 2, rho = x . a_g,
//       b_v = g0 a_v + g1 rho + g2 q
//       b_g = (g1 a_v + g2 rho + g3 q) y + g1 a_g + g2 w
//       B   = (g2 a_v + g3 rho + g4 q) y y' + g2 (a_g y' + y a_g') + g2 Abar + g3 (y w' + w y')
// The Hessian part is again  B = W + W' + S + c I, so the lane map, the LDS staging, the column split and the transpose epilogue are
// shared: one kernel template, and `if constexpr (VGH)` selects the per-pair scalars and the stores.  Lane (i, a) also owns b_g[a];
// b_v is the same in the D lanes of a point and stored by lane a = 0.  Per pair: one more group reduction (rho) and the full jet
// g0 ... g4 (DPhi5 instead of DPhi4).
//
// Lengthscale.  The kernels work in the pre-scaled coordinates gamma (x - c); a block entry that differentiates p times on the x side
// and q times on the y side carries gamma^(p+q).  Hessian alone: every entry carries gamma^4, folded into alpha on the host.  VGH:
// the pack kernel scales a_g by gamma and A by gamma^2, the epilogue b_g by gamma and B by gamma^2 (the constant factor of the kernel
// goes into alpha on the host).
#pragma once
#include "dispatch.hpp"
#include "profiles.hpp"

namespace covgram {

constexpr int HESS_THREADS = 256;
constexpr int HESS_MAX_D = 32;

// The families with a Hessian / value-gradient-Hessian MVM and Hessian block matrices (single profiles with closed-form derivatives up
// to the fourth), written once: X(covgram_family, its number as the suffix of the per-family launchers, arg).  The Makefile's HFAMS and
// covgram/kernels.py's _HESSIAN_FAMILIES repeat the numbers.
#define COVGRAM_HESS_FAMILIES(X, arg) \
    X(COVGRAM_EQ, 0, arg) X(COVGRAM_RQ, 2, arg) X(COVGRAM_CAUCHY, 4, arg) X(COVGRAM_IMQ, 5, arg) X(COVGRAM_DOT, 7, arg) X(COVGRAM_EXPDOT, 8, arg)

struct HessArgs {
    const void* X; int64_t n; int32_t d;
    const void* P; int64_t m;              // packed column records [m][hess_rec(D, vgh)]
    void* out;                             // y (jsplit == 1) or the partial slab [jsplit][n bd], bd = d^2 or 1 + d + d^2
    int32_t Dpad; int64_t jchunk; int32_t jsplit;
    const void* C = nullptr;               // common centre of the isotropic kernels (d scalars on the device)
    double alpha, beta;
    const HostKernel* hk;
    hipStream_t stream;
};
typedef int (*hess_launch_fn)(const HessArgs&, int dtype);
hess_launch_fn hess_launcher(int family);   // nullptr: the family has no Hessian kernel
hess_launch_fn vgh_launcher(int family);    // the same families

// does the Hessian (and value-gradient-Hessian) MVM exist for this kernel?
inline bool hess_family_ok(int family) {
#define CG_X(name, n, arg) if (family == name) return true;
    COVGRAM_HESS_FAMILIES(CG_X, )
#undef CG_X
    return false;
}
inline int hess_pad_dim(int d) { int D = 1; while (D < d) D *= 2; return D; }
// scalars per column record.  Hessian: Abar (D x D), y' (D), tr A, one pad scalar.  VGH: Abar, y', a_g (D), tr A, a_v, padded to a
// multiple of 4 scalars: records stay 16-byte aligned in both precisions
constexpr int hess_rec(int D, bool vgh) { return vgh ? (D * D + 2 * D + 2 + 3) & ~3 : D * D + D + 2; }
constexpr int hess_tr(int D, bool vgh) { return D * D + (vgh ? 2 : 1) * D; }          // offset of tr A in a record (VGH: a_v follows it)
// columns staged per chunk: about 16 KiB of records, at least 4
constexpr int hess_jc(int D, int ts, bool vgh) {
    const int jc = 16384 / (hess_rec(D, vgh) * ts);
    return jc < 4 ? 4 : (jc > 32 ? 32 : jc);
}
constexpr int hess_bc(int D) { return D < 8 ? D : 8; }           // block rows transposed per epilogue pass
constexpr int hess_lds_elems(int D, int ts, bool vgh) {
    const int stage = hess_jc(D, ts, vgh) * hess_rec(D, vgh);
    const int epi = (HESS_THREADS / D) * hess_bc(D) * (D + 1);
    return stage > epi ? stage : epi;
}

// record j of P: [c * D + a] = Abar_j[a, c] (symmetric), then y'_j = gamma (y_j - centre), then tr A_j.  a: block vectors, entry
// j d^2 + a + b d of column A (the reference's vec of a d x d matrix).  VGH: gamma^2 Abar_j, y'_j, gamma a_g, gamma^2 tr A_j, a_v; block j of
// a at offset j (1 + d + d^2): value, gradient, then entry a + b d of A
template <typename T, bool VGH>
__global__ __launch_bounds__(256) void hess_pack_kernel(const T* __restrict__ Y, int64_t m, int32_t d, const T* __restrict__ A, T* __restrict__ P,
                                                        int32_t D, T gamma, const T* __restrict__ Cn) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int rec = hess_rec(D, VGH), tr = hess_tr(D, VGH);
    if (e >= m * (int64_t)rec) return;
    const int64_t j = e / rec;
    const int l = (int)(e - j * rec);
    const T* aj = A + j * (int64_t)(VGH ? 1 + d + d * d : d * d);
    const T* Aj = aj + (VGH ? 1 + d : 0);
    const T g2 = gamma * gamma;
    T v = (T)0;
    if (l < D * D) {
        const int c = l / D, a = l - c * D;
        if (a < d && c < d) {
            v = Aj[a + c * d] + Aj[c + a * d];
            if constexpr (VGH) v *= g2;
        }
    } else if (l < D * D + D) {
        const int c = l - D * D;
        if (c < d) v = (Y[j * (int64_t)d + c] - (Cn ? Cn[c] : (T)0)) * gamma;
    } else if (VGH && l < tr) {
        const int c = l - D * D - D;
        if (c < d) v = aj[1 + c] * gamma;
    } else if (l == tr) {
        for (int a = 0; a < d; ++a) v += Aj[a + a * d];
        if constexpr (VGH) v *= g2;
    } else if (VGH && l == tr + 1) {
        v = aj[0];
    }
    P[e] = v;
}

template <int CTRL> __device__ __forceinline__ float hess_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <int CTRL> __device__ __forceinline__ double hess_dpp(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// sum over the D aligned lanes of a point, the same value in all of them (every lane of the wave takes part: no divergence around it)
template <int D, typename T> __device__ __forceinline__ T hess_group_sum(T v) {
    if constexpr (D >= 2) v += hess_dpp<0xB1>(v);      // quad_perm [1,0,3,2]: lane ^ 1
    if constexpr (D >= 4) v += hess_dpp<0x4E>(v);      // quad_perm [2,3,0,1]: lane ^ 2
    if constexpr (D >= 8) v += hess_dpp<0x141>(v);     // row_half_mirror: the other quad of the 8 (the lanes of a quad agree)
    if constexpr (D >= 16) v += hess_dpp<0x140>(v);    // row_mirror: the other half of the row of 16
    if constexpr (D >= 32) v += __shfl_xor(v, 16);
    return v;
}

// out: y itself (SLAB = false: alpha, beta applied here; beta == 0 never reads y) or this column chunk's slab (raw sums)
template <int FAM, typename T, int D, bool VGH, bool SLAB>
__global__ __launch_bounds__(HESS_THREADS) void hess_mvm_kernel(const T* __restrict__ X, int64_t n, int32_t d, const T* __restrict__ P, int64_t m,
                                                                T* __restrict__ out, int64_t jchunk, const T* __restrict__ Cn, KParams<T> kp,
                                                                T alpha, T beta) {
    constexpr bool ISO = fam_is_iso<FAM>;
    constexpr int REC = hess_rec(D, VGH), TR = hess_tr(D, VGH), JC = hess_jc(D, (int)sizeof(T), VGH), PPW = HESS_THREADS / D;
    constexpr int BC = hess_bc(D), LDW = D + 1;
    __shared__ __attribute__((aligned(16))) T lds[hess_lds_elems(D, (int)sizeof(T), VGH)];

    const int tid = (int)threadIdx.x;
    const int a = tid % D, ip = tid / D;
    const int64_t i = (int64_t)blockIdx.x * PPW + ip;
    const bool rowok = i < n;

    T x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = (rowok && c < d) ? (X[i * (int64_t)d + c] - (ISO ? Cn[c] : (T)0)) * kp.gamma : (T)0;
    const T xa = (rowok && a < d) ? (X[i * (int64_t)d + a] - (ISO ? Cn[a] : (T)0)) * kp.gamma : (T)0;

    T W[D], S[D];
#pragma unroll
    for (int c = 0; c < D; ++c) { W[c] = (T)0; S[c] = (T)0; }
    T diag = (T)0, bv = (T)0, bg = (T)0;                             // bv, bg: VGH only

    const int64_t j0 = (int64_t)blockIdx.y * jchunk;
    const int64_t j1 = (j0 + jchunk < m) ? j0 + jchunk : m;
    for (int64_t jb = j0; jb < j1; jb += JC) {
        const int nc = (int)((j1 - jb < JC) ? j1 - jb : JC);
        __syncthreads();                                              // the previous chunk has been consumed
        for (int e = tid; e < nc * REC; e += HESS_THREADS) lds[e] = P[jb * (int64_t)REC + e];
        __syncthreads();
        for (int jj = 0; jj < nc; ++jj) {
            const T* rec = lds + jj * REC;
            T Ar[D], v[D];                                            // Abar_j[a, :];  r (isotropic) or y_j (dot product)
#pragma unroll
            for (int c = 0; c < D; ++c) Ar[c] = rec[c * D + a];
            T s = (T)0, ua = (T)0;
#pragma unroll
            for (int c = 0; c < D; ++c) {
                const T yc = rec[D * D + c];
                if constexpr (ISO) {
                    v[c] = x[c] - yc;
                    s = fma_t(v[c], v[c], s);
                    ua = fma_t(Ar[c], v[c], ua);
                } else {
                    v[c] = yc;
                    s = fma_t(x[c], yc, s);
                    ua = fma_t(Ar[c], x[c], ua);
                }
            }
            const T ya = rec[D * D + a];
            const T va = ISO ? xa - ya : ya;                         // v[a]
            const T za = ISO ? va : xa;                               // entry a of the vector that u, q and rho are formed with: r or x
            const T aga = VGH ? rec[D * D + D + a] : (T)0;            // a_g,j[a] (VGH only; its LDS read is issued ahead of q's reduction)
            const T q = (T)0.5 * hess_group_sum<D>(za * ua);
            T g2, coef;
            if constexpr (VGH) {
                const T rho = hess_group_sum<D>(za * aga);
                const T t = rec[TR], av = rec[TR + 1];
                T g0, g1, g3, g4;
                DPhi5<FAM, T>::eval(s, kp, g0, g1, g2, g3, g4);
                if constexpr (ISO) {
                    g1 *= (T)2; g2 *= (T)4; g3 *= (T)8; g4 *= (T)16;
                    const T tr = t - rho;
                    const T c1 = fma_t(g1, av, fma_t(g2, tr, g3 * q));
                    const T c2 = fma_t(g2, av, fma_t(g3, tr, g4 * q));
                    bv += fma_t(g0, av, fma_t(g1, tr, g2 * q));
                    bg += fma_t(c1, va, fma_t(g2, ua, -g1 * aga));
                    coef = fma_t(g3, ua, fma_t((T)0.5 * c2, va, -g2 * aga));
                    diag += c1;
                } else {
                    const T c1 = fma_t(g1, av, fma_t(g2, rho, g3 * q));
                    const T c2 = fma_t(g2, av, fma_t(g3, rho, g4 * q));
                    bv += fma_t(g0, av, fma_t(g1, rho, g2 * q));
                    bg += fma_t(c1, va, fma_t(g2, ua, g1 * aga));
                    coef = fma_t(g3, ua, fma_t((T)0.5 * c2, va, g2 * aga));
                }
            } else {
                T g3, g4;
                DPhi4<FAM, T>::eval(s, kp, g2, g3, g4);
                if constexpr (ISO) {
                    g2 *= (T)4; g3 *= (T)8; g4 *= (T)16;
                    const T t = rec[TR];
                    coef = fma_t(g3, ua, (T)0.5 * fma_t(g3, t, g4 * q) * va);
                    diag += fma_t(g2, t, g3 * q);
                } else {
                    coef = fma_t(g3, ua, (T)0.5 * g4 * q * va);
                }
            }
#pragma unroll
            for (int c = 0; c < D; ++c) {
                W[c] = fma_t(coef, v[c], W[c]);
                S[c] = fma_t(g2, Ar[c], S[c]);
            }
        }
    }

    // B[a, b] = W[a, b] + W[b, a] + S[a, b] + (a == b) diag: BC rows of every point's W at a time through LDS
    T res[D];
    T* ep = lds + ip * (BC * LDW);
#pragma unroll
    for (int p = 0; p < D / BC; ++p) {
        __syncthreads();
        if (a >= p * BC && a < (p + 1) * BC) {
#pragma unroll
            for (int c = 0; c < D; ++c) ep[(a - p * BC) * LDW + c] = W[c];
        }
        __syncthreads();
#pragma unroll
        for (int bl = 0; bl < BC; ++bl) {
            const int b = p * BC + bl;
            res[b] = W[b] + ep[bl * LDW + a] + S[b];
        }
    }
    // the stores are written per operator as they were in its own kernel: another form of the same assignment compiles to other code
    if (rowok && a < d) {
        if constexpr (VGH) {
            const int64_t bd = 1 + (int64_t)d + (int64_t)d * d;
            T* o = out + (SLAB ? (int64_t)blockIdx.y * (n * bd) : (int64_t)0) + i * bd;
            const T gam = kp.gamma, gam2 = kp.gamma * kp.gamma;
            auto put = [&](T* p, T r) {
                if constexpr (SLAB) *p = r;
                else *p = (beta == (T)0) ? alpha * r : fma_t(alpha, r, beta * *p);
            };
            if (a == 0) put(o, bv);
            put(o + 1 + a, gam * bg);
            T* oh = o + 1 + d + a;
#pragma unroll
            for (int b = 0; b < D; ++b) {
                if (b < d) put(oh + b * d, gam2 * (res[b] + (b == a ? diag : (T)0)));
            }
        } else {
            T* o = out + (SLAB ? (int64_t)blockIdx.y * (n * (int64_t)d * d) : (int64_t)0) + i * (int64_t)d * d + a;
#pragma unroll
            for (int b = 0; b < D; ++b) {
                if (b < d) {
                    const T r = res[b] + (b == a ? diag : (T)0);
                    if constexpr (SLAB) o[b * d] = r;
                    else o[b * d] = (beta == (T)0) ? alpha * r : fma_t(alpha, r, beta * o[b * d]);
                }
            }
        }
    }
}

// y <- alpha (sum of the jsplit slabs) + beta y, fixed order; jsplit == 0 (no columns): y <- beta y
template <typename T>
__global__ __launch_bounds__(256) void hess_reduce_kernel(const T* __restrict__ slab, int32_t jsplit, int64_t total, T* __restrict__ y, T alpha, T beta) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    T s = (T)0;
    for (int k = 0; k < jsplit; ++k) s += slab[k * total + e];
    y[e] = (beta == (T)0) ? alpha * s : fma_t(alpha, s, beta * y[e]);
}

template <int FAM, typename T, int D, bool VGH>
inline int launch_hess_one(const HessArgs& a) {
    const int ppw = HESS_THREADS / D;
    const dim3 grid((unsigned)((a.n + ppw - 1) / ppw), (unsigned)a.jsplit);
    const KParams<T> kp = cast_params<T>(a.hk->kp);
    if (a.jsplit > 1)
        hipLaunchKernelGGL((hess_mvm_kernel<FAM, T, D, VGH, true>), grid, dim3(HESS_THREADS), 0, a.stream, (const T*)a.X, a.n, a.d, (const T*)a.P, a.m,
                           (T*)a.out, a.jchunk, (const T*)a.C, kp, (T)a.alpha, (T)a.beta);
    else
        hipLaunchKernelGGL((hess_mvm_kernel<FAM, T, D, VGH, false>), grid, dim3(HESS_THREADS), 0, a.stream, (const T*)a.X, a.n, a.d, (const T*)a.P, a.m,
                           (T*)a.out, a.jchunk, (const T*)a.C, kp, (T)a.alpha, (T)a.beta);
    return COVGRAM_OK;
}

template <int FAM, typename T, bool VGH>
inline int launch_hess_typed(const HessArgs& a) {
    return by_dim(Dims<1, 2, 4, 8, 16, 32>{}, a.Dpad, VGH ? "value-gradient-Hessian MVM: no kernel for padded d = %d" : "Hessian MVM: no kernel for padded d = %d",
                  [&](auto D) { return launch_hess_one<FAM, T, decltype(D)::value, VGH>(a); });
}

template <int FAM, bool VGH>
inline int launch_hess_family(const HessArgs& a, int dtype) {
    return dtype == COVGRAM_F64 ? launch_hess_typed<FAM, double, VGH>(a) : launch_hess_typed<FAM, float, VGH>(a);
}

}  // namespace covgram
