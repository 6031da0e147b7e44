// grad_mixed.hip — covgram_grad_mvm_mixed: the gradient / value-gradient block MVM of a composite whose factors carry their own input
// traits (grad_mixed.hpp), on the lane-per-row route (padded d <= 32) or the two-kernel panel route.
#include <math.h>

#include <algorithm>

#include "driver.hpp"
#include "grad_mixed.hpp"

using namespace covgram;

// the composite as the kernels read it: HostKernel's composite fields (nterms, nfac, coef, ffam, fkp), every factor validated on its OWN
// trait; a NeuralNetwork factor keeps sigma in fkp.param
static int make_mixed_kernel(const covgram_kernel_composite* c, int dtype, HostKernel* out) {
    const covgram_kernel& h = c->head;
    CG_REQUIRE(h.family == COVGRAM_COMPOSITE, COVGRAM_EINVAL, "covgram_grad_mvm_mixed takes a covgram_kernel_composite (head.family = %d)", h.family);
    CG_REQUIRE(h.power == 1 && h.lengthscale == 1.0, COVGRAM_EINVAL, "composite head must have power == 1 and lengthscale == 1");
    CG_REQUIRE(c->nterms >= 1 && c->nterms <= EXPR_MAXT, COVGRAM_EUNSUPPORTED, "composite: %d terms (1..%d supported)", c->nterms, EXPR_MAXT);
    memset(out, 0, sizeof(*out));
    out->k = h;
    out->kp.gamma = 1.0; out->kp.gamma2 = 1.0; out->kp.scale = h.scale; out->kp.power = 1;
    out->tu_family = FAM_EXPR_DOT;
    out->nterms = c->nterms;
    int nin = 0, nf = 0;
    for (int t = 0; t < c->nterms; ++t) {
        CG_REQUIRE(c->nfactors[t] >= 1, COVGRAM_EINVAL, "composite: term %d has no factors", t);
        out->coef[t] = 1.0;
        for (int f = 0; f < c->nfactors[t]; ++f, ++nin) {
            CG_REQUIRE(nin < EXPR_MAXF, COVGRAM_EUNSUPPORTED, "composite: more than %d factors", EXPR_MAXF);
            const covgram_kernel& fk = c->factors[nin];
            if (fk.family == COVGRAM_CONSTANT) { out->coef[t] *= fk.scale; continue; }
            if (fk.family == COVGRAM_NEURALNETWORK) {
                CG_REQUIRE(fk.param >= 0, COVGRAM_EINVAL, "DomainError: NeuralNetwork sigma = %g is negative", fk.param);
                CG_REQUIRE(fk.power >= 1, COVGRAM_EINVAL, "Power exponent must be >= 1 (got %d)", fk.power);
                CG_REQUIRE(fk.lengthscale == 1.0, COVGRAM_EINVAL, "Lengthscale applies to isotropic kernels only");
                KParams<double>& kp = out->fkp[nf];
                kp.gamma = 1.0; kp.gamma2 = 1.0; kp.scale = 1.0; kp.param = fk.param; kp.power = fk.power;
            } else {
                CG_REQUIRE(fk.family >= 0 && fk.family < COVGRAM_NFAMILY, COVGRAM_EUNSUPPORTED, "unknown kernel family %d", fk.family);
                const char* name = kFamilyNames[fk.family];
                CG_REQUIRE(fk.family != COVGRAM_EXP && fk.family != COVGRAM_GAMMAEXP && !(fk.family == COVGRAM_MATERNP && fk.p == 0), COVGRAM_EUNSUPPORTED,
                           "mixed gradient kernel: the leaf %s%s is singular at zero distance and has no device path here", name,
                           fk.family == COVGRAM_MATERNP ? "(0)" : "");
                CG_REQUIRE(fk.family != COVGRAM_MATERN, COVGRAM_EUNSUPPORTED, "mixed gradient kernel: the leaf %s(nu) has no device path here (MaternP does)", name);
                HostKernel one;
                const int rc = make_host_kernel(&fk, dtype, true, &one);   // the factor's own trait against its family, its parameters
                if (rc) return rc;
                out->fkp[nf] = one.kp;
                out->fkp[nf].scale = 1.0;
            }
            out->coef[t] *= fk.scale;
            out->ffam[nf] = fk.family;
            ++out->nfac[t]; ++nf;
        }
    }
    return COVGRAM_OK;
}

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
    const int64_t rowblocks = (n + MIX_THREADS - 1) / MIX_THREADS;
    const int64_t npad = rowblocks * MIX_THREADS;
    for (int c0 = 0; c0 < nrhs; ++c0) {
        const void* a_dev = (const char*)a_all + (size_t)c0 * lda_d * ts;
        void* y_dev = (char*)y_all + (size_t)c0 * ldy_d * ts;
        const dim3 rgrid((unsigned)((n + 255) / 256), (unsigned)bd, 1);
        if (m == 0) {                                           // no columns: y <- beta y
            by_dtype(dtype, [&](auto t) {
                using T = decltype(t);
                hipLaunchKernelGGL(grad_reduce_kernel<T>, rgrid, dim3(256), 0, ctx->stream, (const T*)nullptr, npad, D, 0, (T*)y_dev, n, d, (T)0, (T)beta, vg, (T)0,
                                   (int64_t)0);
            });
        } else if (wide) {
            const int PKN = (dtype == COVGRAM_F32) ? 2 : 1;
            const int64_t BC = (int64_t)GJG * PKN;
            const int64_t mpad = ((m + BC - 1) / BC) * BC;
            const int64_t npad64 = ((n + 63) / 64) * 64;
            int64_t panel = (((int64_t)256 << 20) / (npad64 * 2 * (int64_t)ts)) / BC * BC;   // coefficient slabs <= 256 MB
            if (ctx->grad_mixed_panel > 0) panel = std::min<int64_t>(panel, ((ctx->grad_mixed_panel + BC - 1) / BC) * BC);
            panel = std::max<int64_t>(BC, std::min<int64_t>(panel, mpad));
            // (row blocks x dimension chunks) waves may not fill the chip: z slices over the panel's column blocks, as grad_wide's
            const int64_t waves = (npad64 / 64) * (D / 32);
            int zs = (int)std::min<int64_t>(16, std::max<int64_t>(1, ((int64_t)ctx->num_cus * 16 + waves - 1) / waves));
            zs = (int)std::min<int64_t>(zs, std::max<int64_t>(1, panel / BC));
            void* zslab = nullptr;
            const int64_t total = n * (int64_t)bd;
            if (zs > 1) { rc = ws_reserve(ctx, 4, (size_t)zs * total * ts, &zslab); if (rc) return rc; }
            ctx->last_grad_mixed_path |= 2 | (mpad > panel ? 4 : 0) | (zs > 1 ? 8 : 0);
            for (int64_t col0 = 0; col0 < mpad; col0 += panel) {
                const int64_t pc = std::min<int64_t>(panel, mpad - col0);
                const int64_t nb = pc / BC;
                void *P, *C;
                // stream, the value weights, the column scalars (s_j, w_j); coefficient slabs C1, C2 and the per-block sums CX, C0
                rc = ws_reserve(ctx, 0, (size_t)pc * (D * 2 + 3) * ts, &P); if (rc) return rc;
                rc = ws_reserve(ctx, 1, ((size_t)pc * 2 + (size_t)nb * 2) * npad64 * ts, &C); if (rc) return rc;
                void* A0P = (char*)P + (size_t)pc * D * 2 * ts;
                void* SW = (char*)A0P + (size_t)pc * ts;
                void* C2 = (char*)C + (size_t)pc * npad64 * ts;
                void* CX = (char*)C2 + (size_t)pc * npad64 * ts;
                void* C0 = (char*)CX + (size_t)nb * npad64 * ts;
                const int64_t pe = pc * (int64_t)D;
                const unsigned rb = (unsigned)(npad64 / 64);
                const int accumulate = col0 > 0 ? 1 : 0;
                by_dtype(dtype, [&](auto t) {
                    using T = decltype(t);
                    using V = typename Pk<T>::V;
                    hipLaunchKernelGGL(grad_wide_pack_kernel<T>, dim3((unsigned)((pe + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)Y->dptr, m, d, D,
                                       (const T*)a_dev, col0, pc, (T*)P, PKN, (T)1, vg, (T*)A0P, (const T*)nullptr);
                    hipLaunchKernelGGL(grad_mixed_panel_scalars_kernel<T>, dim3((unsigned)((pc + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)Y->dptr, m, d,
                                       (const T*)a_dev, col0, pc, (T*)SW, PKN, vg);
                    const ExprParams<T> kp = make_params<FAM_EXPR_DOT, T>(hk);
                    TimerScope tm(ctx);
                    by_bool(vg != 0, [&](auto vgt) {
                        hipLaunchKernelGGL((grad_mixed_coef_kernel<T, decltype(vgt)::value>), dim3(rb, (unsigned)nb), dim3(64), 0, ctx->stream, (const T*)X->dptr, n,
                                           d, D, (const V*)P, (const T*)SW, (const T*)A0P, (T*)C, (T*)C2, (T*)CX, (T*)C0, npad64, kp);
                    });
                    hipLaunchKernelGGL(grad_mixed_apply_kernel<T>, dim3(rb, (unsigned)(D / WIDE_CH), (unsigned)zs), dim3(64), 0, ctx->stream, (const T*)X->dptr, n,
                                       d, D, (const V*)P, (const V*)C, (const V*)C2, (const T*)CX, (const T*)C0, npad64, nb,
                                       (T*)(zs > 1 ? zslab : y_dev), (T)(zs > 1 ? 1.0 : alpha_eff), (T)(zs > 1 ? 0.0 : beta), accumulate, vg,
                                       (int64_t)(zs > 1 ? total : 0));
                });
                CG_CHECK_HIP(hipGetLastError());
            }
            if (zs > 1) {
                const dim3 zg((unsigned)((n + 255) / 256), (unsigned)bd);
                by_dtype(dtype, [&](auto t) {
                    using T = decltype(t);
                    hipLaunchKernelGGL(grad_wide_reduce_kernel<T>, zg, dim3(256), 0, ctx->stream, (const T*)zslab, zs, total, n, (T*)y_dev, (T)alpha_eff, (T)beta,
                                       vg, bd, (T)alpha_eff);
                });
            }
        } else {
            void* P;
            rc = ws_reserve(ctx, 0, (size_t)m * (2 * D + MIX_EXTRA) * ts, &P); if (rc) return rc;
            const int64_t pe = m * (int64_t)D;
            by_dtype(dtype, [&](auto t) {
                using T = decltype(t);
                hipLaunchKernelGGL(grad_mixed_pack_kernel<T>, dim3((unsigned)((pe + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)Y->dptr, m, d, (const T*)a_dev,
                                   (T*)P, D, vg);
            });
            // column split as the single-trait lane-per-row kernel's: about 64 waves per CU over the launch, at least 64 columns per
            // workgroup, the partial slabs within 256 MB
            int64_t gsplit = std::max<int64_t>(1, ((int64_t)ctx->num_cus * 64 * 64 / MIX_THREADS + rowblocks - 1) / rowblocks);
            gsplit = std::min(gsplit, std::max<int64_t>(1, m / 64));
            gsplit = std::min(gsplit, std::max<int64_t>(1, (int64_t)(256.0e6 / ((double)npad * (D + vg) * ts))));
            int64_t jchunk; int jsplit;
            choose_split(ctx, rowblocks, m, 8, &jchunk, &jsplit, gsplit * rowblocks);
            GradMixedArgs ga;
            ga.X = X->dptr; ga.n = n; ga.d = d; ga.Dpad = D; ga.P = P; ga.m = m; ga.npad = npad; ga.jchunk = jchunk; ga.jsplit = jsplit; ga.vg = vg;
            ga.alpha = alpha_eff; ga.beta = beta; ga.hk = &hk; ga.stream = ctx->stream;
            ctx->last_grad_mixed_jsplit = jsplit;
            ctx->last_grad_mixed_path |= 1 | (jsplit > 1 ? 16 : 0);
            if (jsplit == 1) ga.out = y_dev;
            else { rc = ws_reserve(ctx, 1, (size_t)jsplit * (D + vg) * npad * ts, &ga.out); if (rc) return rc; }
            { TimerScope tm(ctx); rc = by_dtype(dtype, [&](auto t) { return launch_grad_mixed_T<decltype(t)>(ga); }); }
            if (rc) return rc;
            if (jsplit > 1)
                by_dtype(dtype, [&](auto t) {
                    using T = decltype(t);
                    hipLaunchKernelGGL(grad_reduce_kernel<T>, rgrid, dim3(256), 0, ctx->stream, (const T*)ga.out, npad, D, jsplit, (T*)y_dev, n, d, (T)alpha_eff,
                                       (T)beta, vg, (T)alpha_eff, (int64_t)0);
                });
        }
    }
    return COVGRAM_OK;
}

extern "C" {

int covgram_grad_mvm_mixed(covgram_ctx* ctx, const covgram_kernel_composite* k, const covgram_points* X, const covgram_points* Y, const void* a,
                           int64_t lda, void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t value, int32_t loc) {
    int rc = check_pair(ctx, X, Y);
    if (rc) return rc;
    CG_REQUIRE(k != nullptr, COVGRAM_EINVAL, "kernel is NULL");
    CG_REQUIRE(nrhs >= 1, COVGRAM_EINVAL, "nrhs must be >= 1");
    CG_REQUIRE(value == 0 || value == 1, COVGRAM_EINVAL, "value = %d: 0 (GradientKernel) or 1 (ValueGradientKernel)", value);
    const int vg = value;
    const int64_t ma = Y->n * (int64_t)(Y->d + vg), ny = X->n * (int64_t)(X->d + vg);
    CG_REQUIRE(lda >= ma && ldy >= ny, COVGRAM_EINVAL, "lda / ldy smaller than the block vectors (%lld, %lld)", (long long)ma, (long long)ny);
    CG_REQUIRE((a != nullptr || ma == 0) && (y != nullptr || ny == 0), COVGRAM_EINVAL, "a or y is NULL");
    HostKernel hk;
    rc = make_mixed_kernel(k, X->dtype, &hk);
    if (rc) return rc;
    CG_DEVICE(ctx);
    ctx->last_grad_mixed_path = 0; ctx->last_grad_mixed_jsplit = 0;
    if (X->n == 0) return COVGRAM_OK;
    Staged st;
    rc = st.begin(ctx, loc, dtype_size(X->dtype), a, lda, ma, y, ldy, ny, nrhs, beta);
    if (rc) return rc;
    rc = grad_mixed_device(ctx, hk, X, Y, st.a, st.lda, st.y, st.ldy, nrhs, alpha, beta, vg);
    if (rc) return rc;
    CG_CHECK_HIP(hipGetLastError());
    return st.finish();
}

}  // extern "C"
