// grad_mixed.hip — covgram_grad_mvm_mixed: the gradient / value-gradient block MVM of a composite whose factors carry their own input
// traits (grad_mixed.hpp), on the lane-per-row route (padded d <= 32) or the two-kernel panel route.
#include <math.h>

#include <algorithm>

#include "grad_driver.hpp"
#include "grad_mixed.hpp"

using namespace covgram;

// on device-resident a and y that do not overlap
static int grad_mixed_device(covgram_ctx* ctx, const HostKernel& hk, const covgram_points* X, const covgram_points* Y, const void* a_all, int64_t lda_d,
                             void* y_all, int64_t ldy_d, int32_t nrhs, double alpha, double beta, int vg) {
    int rc;
    const int64_t n = X->n, m = Y->n;
    const int d = X->d;
    const int bd = d + vg;
    const int dtype = X->dtype;
    const size_t ts = dtype_size(dtype);
    const int Dl = pad_dim(d);
    const bool wide = Dl < 0 || Dl > 32;
    const int D = wide ? ((d + 31) / 32) * 32 : Dl;
    const double alpha_eff = alpha * hk.kp.scale;
    const int64_t npad = (n + MIX_THREADS - 1) / MIX_THREADS * MIX_THREADS;
    for (int c0 = 0; c0 < nrhs; ++c0) {
        const void* a_dev = (const char*)a_all + (size_t)c0 * lda_d * ts;
        void* y_dev = (char*)y_all + (size_t)c0 * ldy_d * ts;
        if (m == 0) {                                           // no columns: y <- beta y
            grad_reduce(ctx, dtype, nullptr, npad, D, 0, y_dev, n, d, vg, 1, 0, 0.0, 0.0, beta);
        } else if (wide) {
            GradPanelPlan pp;
            rc = grad_panel_plan(ctx, dtype, n, m, D, bd, ctx->grad_mixed_panel, &pp); if (rc) return rc;
            ctx->last_grad_mixed_path |= 2 | (pp.several() ? 4 : 0) | (pp.zs > 1 ? 8 : 0);
            const int64_t npad64 = pp.npad64;
            const int zs = pp.zs;
            rc = grad_panel_route(ctx, pp, dtype, n, bd, vg, y_dev, alpha_eff, alpha_eff, beta, [&](int64_t col0, int64_t pc, int accumulate) -> int {
                const int64_t nb = pc / pp.BC;
                void *P, *C;
                // stream, the value weights, the column scalars (s_j, w_j); coefficient slabs C1, C2 and the per-block sums CX, C0
                int prc = ws_reserve(ctx, 0, (size_t)pc * (D * 2 + 3) * ts, &P); if (prc) return prc;
                prc = ws_reserve(ctx, 1, ((size_t)pc * 2 + (size_t)nb * 2) * npad64 * ts, &C); if (prc) return prc;
                void* A0P = (char*)P + (size_t)pc * D * 2 * ts;
                void* SW = (char*)A0P + (size_t)pc * ts;
                void* C2 = (char*)C + (size_t)pc * npad64 * ts;
                void* CX = (char*)C2 + (size_t)pc * npad64 * ts;
                void* C0 = (char*)CX + (size_t)nb * npad64 * ts;
                const int64_t pe = pc * (int64_t)D;
                const unsigned rb = (unsigned)(npad64 / 64);
                by_dtype(dtype, [&](auto t) {
                    using T = decltype(t);
                    using V = typename Pk<T>::V;
                    hipLaunchKernelGGL(grad_wide_pack_kernel<T>, dim3((unsigned)((pe + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)Y->dptr, m, d, D,
                                       (const T*)a_dev, col0, pc, (T*)P, pp.PKN, (T)1, vg, (T*)A0P, (const T*)nullptr);
                    hipLaunchKernelGGL(grad_mixed_panel_scalars_kernel<T>, dim3((unsigned)((pc + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)Y->dptr, m, d,
                                       (const T*)a_dev, col0, pc, (T*)SW, pp.PKN, vg);
                    const ExprParams<T> kp = make_params<FAM_EXPR_DOT, T>(hk);
                    TimerScope tm(ctx);
                    by_bool(vg != 0, [&](auto vgt) {
                        hipLaunchKernelGGL((grad_mixed_coef_kernel<T, decltype(vgt)::value>), dim3(rb, (unsigned)nb), dim3(64), 0, ctx->stream, (const T*)X->dptr, n,
                                           d, D, (const V*)P, (const T*)SW, (const T*)A0P, (T*)C, (T*)C2, (T*)CX, (T*)C0, npad64, kp);
                    });
                    hipLaunchKernelGGL(grad_mixed_apply_kernel<T>, dim3(rb, (unsigned)(D / WIDE_CH), (unsigned)zs), dim3(64), 0, ctx->stream, (const T*)X->dptr, n,
                                       d, D, (const V*)P, (const V*)C, (const V*)C2, (const T*)CX, (const T*)C0, npad64, nb,
                                       (T*)(zs > 1 ? pp.zslab : y_dev), (T)(zs > 1 ? 1.0 : alpha_eff), (T)(zs > 1 ? 0.0 : beta), accumulate, vg,
                                       (int64_t)(zs > 1 ? pp.total : 0));
                });
                CG_CHECK_HIP(hipGetLastError());
                return COVGRAM_OK;
            });
            if (rc) return rc;
        } else {
            void* P;
            rc = ws_reserve(ctx, 0, (size_t)m * (2 * D + MIX_EXTRA) * ts, &P); if (rc) return rc;
            const int64_t pe = m * (int64_t)D;
            by_dtype(dtype, [&](auto t) {
                using T = decltype(t);
                hipLaunchKernelGGL(grad_mixed_pack_kernel<T>, dim3((unsigned)((pe + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)Y->dptr, m, d, (const T*)a_dev,
                                   (T*)P, D, vg);
            });
            // column split as the single-trait lane-per-row kernel's, the slab cap as it stands (no snap to resident rounds)
            rc = grad_lane_route(ctx, dtype, n, m, d, D, vg, 1, MIX_THREADS, 0, npad, y_dev, 0, alpha_eff, alpha_eff, beta, [&](int64_t jchunk, int jsplit, void* out) -> int {
                GradMixedArgs ga;
                ga.X = X->dptr; ga.n = n; ga.d = d; ga.Dpad = D; ga.P = P; ga.m = m; ga.npad = npad; ga.jchunk = jchunk; ga.jsplit = jsplit; ga.vg = vg;
                ga.alpha = alpha_eff; ga.beta = beta; ga.hk = &hk; ga.stream = ctx->stream; ga.out = out;
                ctx->last_grad_mixed_jsplit = jsplit;
                ctx->last_grad_mixed_path |= 1 | (jsplit > 1 ? 16 : 0);
                TimerScope tm(ctx);
                return by_dtype(dtype, [&](auto t) { return launch_grad_mixed_T<decltype(t)>(ga); });
            });
            if (rc) return rc;
        }
    }
    return COVGRAM_OK;
}

extern "C" {

int covgram_grad_mvm_mixed(covgram_ctx* ctx, const covgram_kernel_composite* k, const covgram_points* X, const covgram_points* Y, const void* a,
                           int64_t lda, void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t value, int32_t loc) {
    HostKernel hk;
    return block_mvm_entry(
        ctx, X, Y, a, lda, y, ldy, nrhs, beta, loc, false,
        [&](int d, int64_t* B) -> int {
            CG_REQUIRE(k != nullptr, COVGRAM_EINVAL, "kernel is NULL");
            CG_REQUIRE(value == 0 || value == 1, COVGRAM_EINVAL, "value = %d: 0 (GradientKernel) or 1 (ValueGradientKernel)", value);
            *B = d + value;
            return COVGRAM_OK;
        },
        [&]() -> int {
            const int rc = make_composite_kernel(k, X->dtype, COMPOSITE_MIXED_GRADIENT, &hk);
            if (rc == COVGRAM_OK) { ctx->last_grad_mixed_path = 0; ctx->last_grad_mixed_jsplit = 0; }
            return rc;
        },
        [&](const Staged& st) { return grad_mixed_device(ctx, hk, X, Y, st.a, st.lda, st.y, st.ldy, nrhs, alpha, beta, value); });
}

}  // extern "C"

