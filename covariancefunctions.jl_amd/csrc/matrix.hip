// matrix.hip — dense instantiation: covgram_matrix (Matrix(G), HBM-write-bound: n * m * sizeof(T) out) and covgram_block_matrix (the block
// Gramians of the derivative kernels, block_matrix.hpp).
#include <algorithm>

#include "driver.hpp"
#include "dense_mvm.hpp"
#include "hess_mvm.hpp"
#include "block_matrix.hpp"

namespace covgram {

// One entry per (row, column): block = 256 rows x 1 column strip of 16 columns; lanes along rows -> coalesced column-major stores
// (the grid's y extent is capped at MATRIX_MAX_GRID_Y: with more strips than that a block walks several).
// EXPR: composite kernels (PT = ExprParams<T>, fam_or_iso != 0: isotropic factors, each scaling s by its own gamma2), else one profile
// through phi_any (PT = KParams<T>, fam_or_iso = the family, the rows pre-scaled by gamma).
template <typename T, bool EXPR, typename PT>
__global__ __launch_bounds__(256) void matrix_kernel(const T* __restrict__ X, int64_t n, const T* __restrict__ Y, int64_t m,
                                                     int32_t d, T* __restrict__ out, int64_t ldo, int fam_or_iso, T scale, const PT kp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool iso = EXPR ? (fam_or_iso != 0)
                          : (fam_or_iso != COVGRAM_DOT && fam_or_iso != COVGRAM_EXPDOT && fam_or_iso != COVGRAM_ASINDOT);
    const T* xi = X + i * (int64_t)d;
    for (int64_t jb = (int64_t)blockIdx.y * 16; jb < m; jb += (int64_t)gridDim.y * 16)
    for (int64_t j = jb; j < jb + 16 && j < m; ++j) {
        const T* yj = Y + j * (int64_t)d;
        T s = (T)0;
        for (int l = 0; l < d; ++l) {
            if (iso) { T r = xi[l] - yj[l]; if constexpr (!EXPR) r *= kp.gamma; s = cg_fma(r, r, s); }
            else s = cg_fma(xi[l], yj[l], s);
        }
        if constexpr (EXPR) out[i + j * ldo] = scale * (iso ? expr_value<T, true>(s, kp) : expr_value<T, false>(s, kp));
        else out[i + j * ldo] = scale * phi_any<T>(fam_or_iso, s, kp);
    }
}

// The same entries with the row x_i held in registers (d <= DM) and a strip of 64 columns per thread: the generic kernel above re-reads
// x_i from memory for every entry — at d = 32 that is 32 vector loads per entry (62 GB/s written for a 16384^2 fp32 tile, against
// 1.8 TB/s at d = 3).  Same arithmetic in the same order (entries are bit-identical); y_j is wave-uniform (scalar loads).
// EXPR: composite kernels (ExprParams), else one profile through phi_any.
template <typename T, int DM, bool EXPR, typename PT, int VR = 1>
__global__ __launch_bounds__(256) void matrix_reg_kernel(const T* __restrict__ X, int64_t n, const T* __restrict__ Y, int64_t m,
                                                         int32_t d, T* __restrict__ out, int64_t ldo, int family_or_iso, T scale, const PT kp) {
    // VR consecutive rows per thread (round 5): one 16-byte streaming store per column instead of VR narrow ones — Matrix(G) is a gigabyte written once
    // (fp32, n = 16384: 3.7 -> TB/s figures in profiles/r05_matrix_bench.txt); VR > 1 needs n, ldo multiples of VR and a 16-byte aligned out
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VR;
    if (i >= n) return;
    const bool iso = EXPR ? (family_or_iso != 0)
                          : (family_or_iso != COVGRAM_DOT && family_or_iso != COVGRAM_EXPDOT && family_or_iso != COVGRAM_ASINDOT);
    T x[VR][DM];
#pragma unroll
    for (int r = 0; r < VR; ++r)
#pragma unroll
        for (int l = 0; l < DM; ++l) x[r][l] = (l < d) ? X[(i + r) * (int64_t)d + l] : (T)0;
    int64_t jb = (int64_t)blockIdx.y * 64, jend = 0;          // the strip at hand (set per strip below)
    T gam = (T)1;
    if constexpr (!EXPR) gam = kp.gamma;
    // the padded dimensions l >= d contribute exact zeros (x = y = 0: r = 0, fma(0, 0, s) = s): no branch inside the entry loop;
    // their y is a scalar select after an in-bounds (clamped) load
    auto entry = [&](const T* __restrict__ yj, auto full, T (&s)[VR]) {
#pragma unroll
        for (int r = 0; r < VR; ++r) s[r] = (T)0;
#pragma unroll
        for (int l = 0; l < DM; ++l) {
            T yl;
            if constexpr (decltype(full)::value) yl = yj[l];
            else { const int lc = l < d ? l : d - 1; const T yv = yj[lc]; yl = l < d ? yv : (T)0; }
#pragma unroll
            for (int r = 0; r < VR; ++r) {
                if (iso) { T q = x[r][l] - yl; if constexpr (!EXPR) q *= gam; s[r] = cg_fma(q, q, s[r]); }
                else s[r] = cg_fma(x[r][l], yl, s[r]);
            }
        }
    };
    typedef T VT __attribute__((ext_vector_type(VR)));
    // the family switch sits OUTSIDE the column loop: each case is a short loop with one profile inlined (the switch inside — phi_any per
    // entry — put every profile, the Bessel series included, into one loop body: 180 SGPR spills, y fetched a dword at a time)
    auto strip = [&](auto famc, auto full) {
        constexpr int F = decltype(famc)::value;
        for (int64_t j = jb; j < jend; ++j) {
            T s[VR], v[VR];
            entry(Y + j * (int64_t)d, full, s);
#pragma unroll
            for (int r = 0; r < VR; ++r) {
                if constexpr (EXPR) v[r] = scale * (iso ? expr_value<T, true>(s[r], kp) : expr_value<T, false>(s[r], kp));
                else {
                    T w;
                    if constexpr (F == COVGRAM_DOT) w = s[r];
                    else if constexpr (F == COVGRAM_CONSTANT) w = (T)1;
                    else w = Phi<F, T, false>::eval(s[r], kp);
                    if (kp.power != 1) w = ipow(w, kp.power);
                    v[r] = scale * w;
                }
            }
            if constexpr (VR == 1) __builtin_nontemporal_store(v[0], out + i + j * ldo);
            else {
                VT vv;
#pragma unroll
                for (int r = 0; r < VR; ++r) vv[r] = v[r];
                __builtin_nontemporal_store(vv, reinterpret_cast<VT*>(out + i + j * ldo));
            }
        }
    };
    auto run = [&](auto famc) { if (d == DM) strip(famc, std::true_type()); else strip(famc, std::false_type()); };
    // one strip per block, unless there are more strips than the grid's y extent may hold (MATRIX_MAX_GRID_Y): then a block walks several
    for (; jb < m; jb += (int64_t)gridDim.y * 64) {
        jend = (jb + 64 < m) ? jb + 64 : m;
        if constexpr (EXPR) run(std::integral_constant<int, 0>());
        else switch (family_or_iso) {
#define CG_FAMCASE(F) case F: run(std::integral_constant<int, F>()); break;
            CG_FAMCASE(COVGRAM_EQ) CG_FAMCASE(COVGRAM_EXP) CG_FAMCASE(COVGRAM_RQ) CG_FAMCASE(COVGRAM_GAMMAEXP) CG_FAMCASE(COVGRAM_CAUCHY)
            CG_FAMCASE(COVGRAM_IMQ) CG_FAMCASE(COVGRAM_MATERNP) CG_FAMCASE(COVGRAM_DOT) CG_FAMCASE(COVGRAM_EXPDOT) CG_FAMCASE(COVGRAM_MATERN)
            CG_FAMCASE(COVGRAM_ASINDOT)
#undef CG_FAMCASE
        }
    }
}


}  // namespace covgram

using namespace covgram;

extern "C" {

int covgram_matrix(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, void* out,
                   int64_t ldo, int32_t loc) {
    int rc = check_pair(ctx, X, Y);
    if (rc) return rc;
    const int64_t n = X->n, m = Y->n;
    CG_REQUIRE(ldo >= n, COVGRAM_EINVAL, "ldo=%lld < n=%lld", (long long)ldo, (long long)n);
    CG_REQUIRE(out != nullptr || n * m == 0, COVGRAM_EINVAL, "out is NULL");
    const int dtype = X->dtype;
    const size_t ts = dtype_size(dtype);
    HostKernel hk;
    rc = make_host_kernel(k, dtype, true, &hk);   // gamma = 1/l, unfolded EQ
    if (rc) return rc;
    CG_DEVICE(ctx);
    ctx->last_matrix_path = 0;
    if (n == 0 || m == 0) return COVGRAM_OK;
    Staged st;
    rc = st.begin_tile(ctx, loc, ts, out, ldo, n, m);
    if (rc) return rc;
    void* const o = st.y;
    const int64_t ld = st.ldy;
    // a grid's y extent is limited (65535 is what every HIP device accepts): beyond it the kernels walk several strips per block
    constexpr int64_t MATRIX_MAX_GRID_Y = 65535;
    auto strips = [](int64_t mm, int64_t w) { const int64_t c = (mm + w - 1) / w; return (unsigned)(c < MATRIX_MAX_GRID_Y ? c : MATRIX_MAX_GRID_Y); };
    const bool expr = hk.tu_family >= COVGRAM_NFAMILY;             // composite: the interpreter
    const int fam_or_iso = expr ? (hk.tu_family == FAM_EXPR_ISO ? 1 : 0) : k->family;
    const int dd = X->d;
    ctx->last_matrix_path = expr ? 1002 : 1001;                    // route + 10 DM + 1000 VR (include/covgram.h); the register routes set theirs below
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const T* xp = (const T*)X->dptr;
        const T* yp = (const T*)Y->dptr;
        const T scale = (T)hk.kp.scale;
        if (dd <= 64 && ctx->matrix_variant != 1) {                // x_i in registers, 64-column strips (option matrix_variant = 1: the generic kernel)
            const dim3 g2((unsigned)((n + 255) / 256), strips(m, 64));
            // rows per thread: 16-byte streaming stores (4 fp32 / 2 fp64 rows) when the points are short (registers), n and the leading dimension are
            // multiples of it and the output is 16-byte aligned; a single profile only (the composite interpreter keeps one row per thread)
            constexpr int VRV = 16 / (int)sizeof(T);
#define CG_MAT(DMV)                                                                                                                            \
            do {                                                                                                                               \
                const bool vr = !expr && DMV <= 16 && n % VRV == 0 && ld % VRV == 0 && ((uintptr_t)o % 16) == 0;                                 \
                const dim3 g3((unsigned)((n / VRV + 255) / 256), strips(m, 64));                                                               \
                ctx->last_matrix_path = (expr ? 4 : 3) + 10 * DMV + 1000 * (vr ? VRV : 1);                                                     \
                if (expr) hipLaunchKernelGGL((matrix_reg_kernel<T, DMV, true, ExprParams<T>>), g2, dim3(256), 0, ctx->stream, xp, n, yp, m, dd, \
                                             (T*)o, ld, fam_or_iso, scale, make_params<FAM_EXPR_ISO, T>(hk));                                  \
                else if (vr) hipLaunchKernelGGL((matrix_reg_kernel<T, (DMV <= 16 ? DMV : 16), false, KParams<T>, VRV>), g3, dim3(256), 0,      \
                                                ctx->stream, xp, n, yp, m, dd, (T*)o, ld, fam_or_iso, scale, cast_params<T>(hk.kp));           \
                else hipLaunchKernelGGL((matrix_reg_kernel<T, DMV, false, KParams<T>>), g2, dim3(256), 0, ctx->stream, xp, n, yp, m, dd,       \
                                        (T*)o, ld, fam_or_iso, scale, cast_params<T>(hk.kp));                                                  \
            } while (0)
            if (dd <= 4) CG_MAT(4); else if (dd <= 8) CG_MAT(8); else if (dd <= 16) CG_MAT(16); else if (dd <= 32) CG_MAT(32); else CG_MAT(64);
#undef CG_MAT
        } else {
            const dim3 grid((unsigned)((n + 255) / 256), strips(m, 16));
            if (expr) hipLaunchKernelGGL((matrix_kernel<T, true, ExprParams<T>>), grid, dim3(256), 0, ctx->stream, xp, n, yp, m, dd, (T*)o, ld, fam_or_iso,
                                         scale, make_params<FAM_EXPR_ISO, T>(hk));
            else hipLaunchKernelGGL((matrix_kernel<T, false, KParams<T>>), grid, dim3(256), 0, ctx->stream, xp, n, yp, m, dd, (T*)o, ld, fam_or_iso, scale,
                                    cast_params<T>(hk.kp));
        }
    });
    CG_CHECK_HIP(hipGetLastError());
    return st.finish();
}

// Dense instantiation of a block Gramian (block_matrix.hpp): the matrix covgram_grad_mvm / covgram_valgrad_mvm / covgram_hess_mvm /
// covgram_valgradhess_mvm apply.  The kernels each MVM accepts, with its refusals.
int covgram_block_matrix(covgram_ctx* ctx, int32_t kind, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, void* out,
                         int64_t ldo, int32_t loc) {
    int rc = check_pair(ctx, X, Y);
    if (rc) return rc;
    CG_REQUIRE(k != nullptr, COVGRAM_EINVAL, "kernel is NULL");
    CG_REQUIRE(kind >= COVGRAM_BLOCK_GRADIENT && kind <= COVGRAM_BLOCK_VALUE_GRADIENT_HESSIAN, COVGRAM_EINVAL, "unknown block kind %d", kind);
    const bool hess = kind == COVGRAM_BLOCK_HESSIAN || kind == COVGRAM_BLOCK_VALUE_GRADIENT_HESSIAN;
    const int vflag = (kind == COVGRAM_BLOCK_VALUE_GRADIENT || kind == COVGRAM_BLOCK_VALUE_GRADIENT_HESSIAN) ? 1 : 0;
    const int d = X->d;
    if (hess) {
        rc = hess_refusal(vflag ? "ValueGradientHessianKernel" : "HessianKernel", k, d);
        if (rc) return rc;
    }
    const int64_t n = X->n, m = Y->n;
    const int64_t B = vflag + (kind == COVGRAM_BLOCK_HESSIAN ? 0 : (int64_t)d) + (hess ? (int64_t)d * d : 0);
    const int64_t NB = n * B, MB = m * B;
    CG_REQUIRE(ldo >= NB, COVGRAM_EINVAL, "ldo=%lld < n B=%lld", (long long)ldo, (long long)NB);
    CG_REQUIRE(out != nullptr || NB * MB == 0, COVGRAM_EINVAL, "out is NULL");
    const int dtype = X->dtype;
    const size_t ts = dtype_size(dtype);
    HostKernel hk;
    // gamma = 1 / l, unfolded EQ: the parameter block of the block MVMs.  The gradient kinds evaluate their jets in fp64 whatever the
    // dtype of the points (block_matrix.hpp: JT), so they take the fp64 block: the Taylor switches of the Matern profiles sit at
    // eps(T)^(1/p), and the fp32 ones leave 5e-5 of a single pair's phi'' next to the switch
    rc = make_host_kernel(k, hess ? dtype : COVGRAM_F64, true, &hk);
    if (rc) return rc;
    bm_launch_fn launch = hess ? block_matrix_hess_launcher(hk.tu_family) : block_matrix_launcher(hk.tu_family);
    CG_REQUIRE(launch != nullptr, COVGRAM_EUNSUPPORTED, "block matrix: no kernel for family %d", hk.tu_family);
    const int D = bm_pad_dim(d, hess);
    CG_REQUIRE(D > 0, COVGRAM_EUNSUPPORTED, "block matrix: d = %d exceeds the compiled maximum %d (rows in registers)", d, hess ? 32 : 64);
    CG_DEVICE(ctx);
    ctx->last_block_matrix_path = 0;
    if (n == 0 || m == 0) return COVGRAM_OK;
    Staged st;
    rc = st.begin_tile(ctx, loc, ts, out, ldo, NB, MB);
    if (rc) return rc;
    void* const o = st.y;
    const int64_t ld = st.ldy;
    // 16-byte streaming stores (4 fp32 / 2 fp64 consecutive rows per thread) when a thread's rows stay inside one point (VR | B), the
    // leading dimension is a multiple of VR and out is 16-byte aligned: the rule of covgram_matrix.  One arithmetic either way.
    const int VRW = 16 / (int)ts;
    const bool wide = B % VRW == 0 && ld % VRW == 0 && ((uintptr_t)o % 16) == 0;
    BlockMatArgs a;
    a.X = X->dptr; a.n = n; a.Y = Y->dptr; a.m = m; a.d = d; a.parts = vflag | (kind == COVGRAM_BLOCK_HESSIAN ? 0 : 2); a.out = o; a.ldo = ld; a.Dpad = D; a.vr = wide ? VRW : 1;
    a.hess = hess ? 1 : 0; a.hk = &hk; a.stream = ctx->stream;
    a.W = (int32_t)std::max<int64_t>(1, 64 / B);        // a strip of about 64 columns per workgroup, as covgram_matrix
    { TimerScope tm(ctx); rc = launch(a, dtype); }
    if (rc) return rc;
    ctx->last_block_matrix_path = (kind + 1) + 10 * a.vr;
    CG_CHECK_HIP(hipGetLastError());
    return st.finish();
}

}  // extern "C"
