// vgh_mvm.hpp — Y <- alpha G A + beta Y for the value-gradient-Hessian-kernel Gramian (covgram_valgradhess_mvm): block (i, j) is the
// (1 + d + d^2) x (1 + d + d^2) joint covariance of [f, grad f, vec hess f] (src/hessian.jl:301-325): entry (row functional on x_i,
// column functional on y_j) of k, the functionals being id, d/d._a and d^2/d._a d._b.  Applied in O(d^2) per pair.  Block input
// (a_v, a_g, A), A[a, b] = flat entry 1 + d + a + b d, Abar = A + A', t = tr A; block output (b_v, b_g, B):
//   isotropic  k = f(|r|^2), r = x_i - y_j, g_m = 2^m f^(m):   u = Abar r, q = r'u / 2, rho = r . a_g,
//       c1 = g1 a_v - g2 rho + g2 t + g3 q,   c2 = g2 a_v - g3 rho + g3 t + g4 q
//       b_v = g0 a_v - g1 rho + g1 t + g2 q
//       b_g = c1 r - g1 a_g + g2 u
//       B   = c1 I + c2 r r' - g2 (a_g r' + r a_g') + g2 Abar + g3 (u r' + r u')
//   dot product  k = f(x . y), g_m = f^(m), x = x_i, y = y_j:   w = Abar x, q = x'w / 2, rho = x . a_g,
//       b_v = g0 a_v + g1 rho + g2 q
//       b_g = (g1 a_v + g2 rho + g3 q) y + g1 a_g + g2 w
//       B   = (g2 a_v + g3 rho + g4 q) y y' + g2 (a_g y' + y a_g') + g2 Abar + g3 (y w' + w y')
// The Hessian part is again  B = W + W' + S + c I  with  W[a,:] = coef_a v[:]  (v = r or y), S = g2 Abar: the lane map, the LDS
// staging, the column split and the transpose epilogue are those of hess_mvm.hpp.  Lane (i, a) owns row a of B of row point i and
// b_g[a]; b_v is the same in the D lanes of a point and stored by lane a = 0.  Per pair: one more group reduction (rho) and the
// full jet g0 ... g4 (DPhi5).
//
// Lengthscale.  The kernel works in the pre-scaled coordinates gamma (x - c); a block entry that differentiates p times on the x
// side and q times on the y side carries gamma^(p+q): vgh_pack_kernel scales a_g by gamma and A by gamma^2, the epilogue b_g by
// gamma and B by gamma^2 (the constant factor of the kernel goes into alpha on the host).
#pragma once
#include "hess_mvm.hpp"

namespace covgram {

struct VghArgs {
    const void* X; int64_t n; int32_t d;
    const void* P; int64_t m;              // packed column records [m][vgh_rec(D)]
    void* out;                             // y (jsplit == 1) or the partial slab [jsplit][n (1 + d + d^2)]
    int32_t Dpad; int64_t jchunk; int32_t jsplit;
    const void* C = nullptr;               // common centre of the isotropic kernels (d scalars on the device)
    double alpha, beta;
    const HostKernel* hk;
    hipStream_t stream;
};
typedef int (*vgh_launch_fn)(const VghArgs&, int dtype);
vgh_launch_fn vgh_launcher(int family);     // nullptr: the family has no value-gradient-Hessian kernel (hess_family_ok)

// Abar (D x D), y' (D), a_g (D), tr A, a_v, padded to a multiple of 4 scalars: records stay 16-byte aligned in both precisions
constexpr int vgh_rec(int D) { return (D * D + 2 * D + 2 + 3) & ~3; }
// columns staged per chunk: about 16 KiB of records, at least 4
constexpr int vgh_jc(int D, int ts) { return (16384 / (vgh_rec(D) * ts)) < 4 ? 4 : ((16384 / (vgh_rec(D) * ts)) > 32 ? 32 : (16384 / (vgh_rec(D) * ts))); }
constexpr int vgh_lds_elems(int D, int ts) {
    const int stage = vgh_jc(D, ts) * vgh_rec(D);
    const int epi = (HESS_THREADS / D) * hess_bc(D) * (D + 1);
    return stage > epi ? stage : epi;
}

// record j of P: [c * D + a] = gamma^2 Abar_j[a, c] (symmetric), then y'_j = gamma (y_j - centre), then gamma a_g, gamma^2 tr A_j, a_v.
// a: block vectors, block j at offset j (1 + d + d^2): value, gradient, then entry a + b d of A (the reference's vec of a d x d matrix)
template <typename T>
__global__ __launch_bounds__(256) void vgh_pack_kernel(const T* __restrict__ Y, int64_t m, int32_t d, const T* __restrict__ A, T* __restrict__ P,
                                                       int32_t D, T gamma, const T* __restrict__ Cn) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int rec = vgh_rec(D);
    if (e >= m * (int64_t)rec) return;
    const int64_t j = e / rec;
    const int l = (int)(e - j * rec);
    const T* aj = A + j * (int64_t)(1 + d + d * d);
    const T* Aj = aj + 1 + d;
    const T g2 = gamma * gamma;
    T v = (T)0;
    if (l < D * D) {
        const int c = l / D, a = l - c * D;
        if (a < d && c < d) v = (Aj[a + c * d] + Aj[c + a * d]) * g2;
    } else if (l < D * D + D) {
        const int c = l - D * D;
        if (c < d) v = (Y[j * (int64_t)d + c] - (Cn ? Cn[c] : (T)0)) * gamma;
    } else if (l < D * D + 2 * D) {
        const int c = l - D * D - D;
        if (c < d) v = aj[1 + c] * gamma;
    } else if (l == D * D + 2 * D) {
        for (int a = 0; a < d; ++a) v += Aj[a + a * d];
        v *= g2;
    } else if (l == D * D + 2 * D + 1) {
        v = aj[0];
    }
    P[e] = v;
}

// out: y itself (SLAB = false: alpha, beta applied here; beta == 0 never reads y) or this column chunk's slab (raw sums)
template <int FAM, typename T, int D, bool SLAB>
__global__ __launch_bounds__(HESS_THREADS) void vgh_mvm_kernel(const T* __restrict__ X, int64_t n, int32_t d, const T* __restrict__ P, int64_t m,
                                                               T* __restrict__ out, int64_t jchunk, const T* __restrict__ Cn, KParams<T> kp,
                                                               T alpha, T beta) {
    constexpr bool ISO = fam_is_iso<FAM>;
    constexpr int REC = vgh_rec(D), JC = vgh_jc(D, (int)sizeof(T)), PPW = HESS_THREADS / D;
    constexpr int BC = hess_bc(D), LDW = D + 1;
    __shared__ __attribute__((aligned(16))) T lds[vgh_lds_elems(D, (int)sizeof(T))];

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
    T diag = (T)0, bv = (T)0, bg = (T)0;

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
            const T aga = rec[D * D + D + a];
            const T q = (T)0.5 * hess_group_sum<D>(za * ua);
            const T rho = hess_group_sum<D>(za * aga);
            const T t = rec[D * D + 2 * D], av = rec[D * D + 2 * D + 1];
            T g0, g1, g2, g3, g4;
            DPhi5<FAM, T>::eval(s, kp, g0, g1, g2, g3, g4);
            T coef;
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
    if (rowok && a < d) {
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
    }
}

template <int FAM, typename T, int D>
inline int launch_vgh_one(const VghArgs& a) {
    const int ppw = HESS_THREADS / D;
    const dim3 grid((unsigned)((a.n + ppw - 1) / ppw), (unsigned)a.jsplit);
    const KParams<T> kp = cast_params<T>(a.hk->kp);
    if (a.jsplit > 1)
        hipLaunchKernelGGL((vgh_mvm_kernel<FAM, T, D, true>), grid, dim3(HESS_THREADS), 0, a.stream, (const T*)a.X, a.n, a.d, (const T*)a.P, a.m,
                           (T*)a.out, a.jchunk, (const T*)a.C, kp, (T)a.alpha, (T)a.beta);
    else
        hipLaunchKernelGGL((vgh_mvm_kernel<FAM, T, D, false>), grid, dim3(HESS_THREADS), 0, a.stream, (const T*)a.X, a.n, a.d, (const T*)a.P, a.m,
                           (T*)a.out, a.jchunk, (const T*)a.C, kp, (T)a.alpha, (T)a.beta);
    return COVGRAM_OK;
}

template <int FAM, typename T>
inline int launch_vgh_typed(const VghArgs& a) {
    switch (a.Dpad) {
        case 1: return launch_vgh_one<FAM, T, 1>(a);
        case 2: return launch_vgh_one<FAM, T, 2>(a);
        case 4: return launch_vgh_one<FAM, T, 4>(a);
        case 8: return launch_vgh_one<FAM, T, 8>(a);
        case 16: return launch_vgh_one<FAM, T, 16>(a);
        case 32: return launch_vgh_one<FAM, T, 32>(a);
        default: set_error("value-gradient-Hessian MVM: no kernel for padded d = %d", a.Dpad); return COVGRAM_EUNSUPPORTED;
    }
}

template <int FAM>
inline int launch_vgh_family(const VghArgs& a, int dtype) {
    return dtype == COVGRAM_F64 ? launch_vgh_typed<FAM, double>(a) : launch_vgh_typed<FAM, float>(a);
}

}  // namespace covgram
