// mixed_mvm.hip — covgram_mvm_mixed and covgram_matrix_mixed: the scalar Gramian of a composite whose factors carry their own input traits
// (mixed_mvm.hpp).  The product's driver sends the plain terms of the composite — one trait, no NeuralNetwork factor — to the kernels behind
// covgram_mvm (dense_mvm_on_device: matrix cores, factored dot product, the Sum split) and runs the rest in the fused kernel, on the
// lane-per-row route (padded d <= 32) or the chunked route.  The column split, the partial slabs and the reduction of the fused kernel are
// dense_lane_route / dense_reduce (dense_driver.hpp), as covgram_mvm's lane-per-row kernels use them.
#include <math.h>

#include <algorithm>

#include "dense_driver.hpp"
#include "mixed_mvm.hpp"

using namespace covgram;

namespace {

// the padded dimension of the kernels that hold a row in registers (d <= 32); 0: the chunked kernels
static int mixv_bucket(int d) { return d <= 4 ? 4 : (d <= 8 ? 8 : (d <= 16 ? 16 : (d <= 32 ? 32 : 0))); }

// ---- the partition of the composite's terms ---------------------------------------------------------------------------------------------
enum MixedPart { PART_ISO = 0, PART_DOT = 1, PART_FUSED = 2, PART_CONST = 3 };

struct MixedGroup {
    bool present = false, simple = false;
    covgram_kernel k;                     // simple: one term of one factor
    covgram_kernel_composite c;
    const covgram_kernel* ptr() const { return simple ? &k : &c.head; }
};

struct MixedPlan {
    MixedGroup iso, dot;                  // single-trait groups for the kernels behind covgram_mvm
    bool fused = false;
    HostKernel fused_hk;                  // the terms of the fused kernel (head.scale in kp.scale)
    double constant = 0.0;                // sum of the constant-only terms (head.scale folded in)
};

// the terms of `k` whose part[t] == want as one composite under the head trait `trait`
static int gather_terms(const covgram_kernel_composite* k, const int* part, int want, int trait, covgram_kernel_composite* out) {
    memset(out, 0, sizeof(*out));
    out->head = k->head;
    out->head.trait = trait;
    int nin = 0, nout = 0;
    for (int t = 0; t < k->nterms; ++t) {
        if (part[t] == want) {
            out->nfactors[out->nterms++] = k->nfactors[t];
            for (int f = 0; f < k->nfactors[t]; ++f) out->factors[nout++] = k->factors[nin + f];
        }
        nin += k->nfactors[t];
    }
    return out->nterms;
}

// A term is PLAIN when all its profile factors share one trait and none is NeuralNetwork; a term of Constants only is the constant part;
// every other term — a Product across traits, anything with a NeuralNetwork factor — is fused.  The plain terms of a trait form one group
// for the kernels behind covgram_mvm unless the fused terms evaluate leaves of that trait themselves: there the plain term rides along
// in the fused pass, one more factor on an argument that pass has formed anyway, instead of a second pass over all pairs.  A group that
// make_host_kernel refuses stays fused.  Option "mixed_fuse" = 1, or nothing to delegate: every term, constants included, in the fused kernel.
static int mixed_partition(const covgram_ctx* ctx, const covgram_kernel_composite* k, int dtype, MixedPlan* plan) {
    int part[COVGRAM_COMPOSITE_MAX_TERMS];
    bool fused_has[2] = {false, false};
    int nin = 0;
    for (int t = 0; t < k->nterms; ++t) {
        bool has[2] = {false, false}, nn = false;
        for (int f = 0; f < k->nfactors[t]; ++f, ++nin) {
            const int fam = k->factors[nin].family;
            if (fam == COVGRAM_CONSTANT) continue;
            if (fam == COVGRAM_NEURALNETWORK) nn = true;
            else has[mixv_dot_family(fam) ? 1 : 0] = true;
        }
        if (nn || (has[0] && has[1])) {
            part[t] = PART_FUSED;
            fused_has[0] |= has[0]; fused_has[1] |= has[1];
        } else part[t] = has[0] ? PART_ISO : (has[1] ? PART_DOT : PART_CONST);
    }
    for (int t = 0; t < k->nterms; ++t)
        if ((part[t] == PART_ISO || part[t] == PART_DOT) && (ctx->mixed_fuse == 1 || fused_has[part[t]])) part[t] = PART_FUSED;
    // the two groups, each as covgram_mvm takes it
    for (int tr = 0; tr < 2; ++tr) {
        MixedGroup& g = tr == 0 ? plan->iso : plan->dot;
        if (gather_terms(k, part, tr, tr == 0 ? COVGRAM_ISOTROPIC : COVGRAM_DOTPRODUCT, &g.c) == 0) continue;
        int profiles = 0;
        for (int f = 0; f < g.c.nfactors[0]; ++f) profiles += g.c.factors[f].family != COVGRAM_CONSTANT;
        if (g.c.nterms == 1 && profiles == 1) {              // one term of one factor: a plain covgram_kernel
            double coef = g.c.head.scale;
            for (int f = 0; f < g.c.nfactors[0]; ++f) {
                if (g.c.factors[f].family == COVGRAM_CONSTANT) coef *= g.c.factors[f].scale;
                else g.k = g.c.factors[f];
            }
            g.k.scale *= coef;
            g.simple = true;
        }
        HostKernel probe;
        if (make_host_kernel(g.ptr(), dtype, false, &probe) == COVGRAM_OK) g.present = true;
        else
            for (int t = 0; t < k->nterms; ++t)
                if (part[t] == tr) part[t] = PART_FUSED;
    }
    const bool delegated = plan->iso.present || plan->dot.present;
    bool any_fused = false, any_const = false;
    for (int t = 0; t < k->nterms; ++t) { any_fused |= part[t] == PART_FUSED; any_const |= part[t] == PART_CONST; }
    if (any_fused && any_const && (!delegated || ctx->mixed_fuse == 1))
        for (int t = 0; t < k->nterms; ++t)
            if (part[t] == PART_CONST) part[t] = PART_FUSED;
    covgram_kernel_composite sub;
    if (gather_terms(k, part, PART_FUSED, k->head.trait, &sub) > 0) {
        const int rc = make_composite_kernel(&sub, dtype, COMPOSITE_MIXED_VALUES, &plan->fused_hk);
        if (rc) return rc;
        plan->fused = true;
    }
    nin = 0;
    for (int t = 0; t < k->nterms; ++t) {
        double coef = k->head.scale;
        for (int f = 0; f < k->nfactors[t]; ++f, ++nin) coef *= k->factors[nin].scale;
        if (part[t] == PART_CONST) plan->constant += coef;
    }
    return COVGRAM_OK;
}

// ---- the fused kernel on device-resident a and y that do not overlap: the route of dense_driver.hpp over its own column stream ----------------
static int mixed_fused_device(covgram_ctx* ctx, const HostKernel& hk, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda, void* y,
                              int64_t ldy, int32_t nrhs, double alpha, double beta) {
    const int64_t n = X->n, m = Y->n;
    const int d = X->d;
    const int dtype = X->dtype;
    const size_t ts = dtype_size(dtype);
    const int PKN = dtype == COVGRAM_F32 ? 2 : 1;
    const int D = mixv_bucket(d);
    const int nch = (d + MIXV_CH - 1) / MIXV_CH;
    const int64_t mpad = ((m + MIXV_CB - 1) / MIXV_CB) * MIXV_CB;                      // whole interpreter blocks on either route
    const int64_t rowblocks = (n + MIXV_THREADS - 1) / MIXV_THREADS, npad = rowblocks * MIXV_THREADS;
    const double alpha_eff = alpha * hk.kp.scale;
    int rc;
    for (int c0 = 0; c0 < nrhs;) {
        const int nr = nrhs - c0 >= 4 ? 4 : 1;                   // groups of four right-hand sides, the remainder one by one
        const char* a_c = (const char*)a + (size_t)c0 * lda * ts;
        char* y_c = (char*)y + (size_t)c0 * ldy * ts;
        void* P;
        const size_t rec = D ? (size_t)(D + 1 + nr) : (size_t)nch * MIXV_CH + 1 + nr;   // scalars per column
        rc = ws_reserve(ctx, 0, (size_t)mpad * rec * ts, &P); if (rc) return rc;
        by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            const dim3 pg((unsigned)((mpad + 255) / 256));
            if (D) hipLaunchKernelGGL(mixed_pack_kernel<T>, pg, dim3(256), 0, ctx->stream, (const T*)Y->dptr, m, d, (const T*)a_c, lda, nr, (T*)P, D, nr, PKN, mpad);
            else hipLaunchKernelGGL(mixed_chunk_pack_kernel<T>, pg, dim3(256), 0, ctx->stream, (const T*)Y->dptr, m, d, nch, (const T*)a_c, lda, nr, (T*)P, nr, PKN, mpad);
        });
        rc = dense_lane_route(ctx, dtype, rowblocks, npad, n, m, nr, nr, 0, false, y_c, ldy, alpha_eff, beta, [&](int64_t jchunk, int jsplit, void* out, unsigned*) {
            ctx->last_mixed_jsplit = jsplit;
            ctx->last_mixed_path |= (D ? 1 : 2) | (jsplit > 1 ? 16 : 0);
            const dim3 grid((unsigned)rowblocks, (unsigned)jsplit);
            const int fs = jsplit == 1 ? 1 : 0;
            by_dtype(dtype, [&](auto t) {
                by_bool(nr == 4, [&](auto four) {
                    using T = decltype(t);
                    using V = typename Pk<T>::V;
                    constexpr int NR = decltype(four)::value ? 4 : 1;
                    const ExprParams<T> ep = make_params<FAM_EXPR_DOT, T>(hk);
                    if (!try_dim(Dims<4, 8, 16, 32>{}, D, [&](auto DV) {
                            hipLaunchKernelGGL((mixed_lane_kernel<T, decltype(DV)::value, NR>), grid, dim3(MIXV_THREADS), 0, ctx->stream, (const T*)X->dptr, n, d,
                                               (const V*)P, mpad, (T*)out, npad, ldy, nr, jchunk, (T)alpha_eff, (T)beta, fs, ep);
                        }))
                        hipLaunchKernelGGL((mixed_chunk_kernel<T, NR>), grid, dim3(MIXV_THREADS), 0, ctx->stream, (const T*)X->dptr, n, d, nch, (const V*)P, mpad,
                                           (T*)out, npad, ldy, nr, jchunk, (T)alpha_eff, (T)beta, fs, ep);
                });
            });
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) { set_error("mixed_mvm launch failed: %s", hipGetErrorString(e)); return (int)COVGRAM_EHIP; }
            return (int)COVGRAM_OK;
        });
        if (rc) return rc;
        c0 += nr;
    }
    return COVGRAM_OK;
}

// the parts in the order iso, dot, fused, constant: the first applies the caller's beta, the others add (sum_split_run's rule)
static int mixed_device(covgram_ctx* ctx, const MixedPlan& plan, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda, void* y,
                        int64_t ldy, int32_t nrhs, double alpha, double beta) {
    const int64_t n = X->n, m = Y->n;
    const int dtype = X->dtype;
    if (m == 0) {                                                // no columns: y <- beta y
        dense_reduce(ctx, dtype, nullptr, n, 1, 0, y, n, ldy, nrhs, 0.0, beta);
        return COVGRAM_OK;
    }
    int rc;
    bool first = true;
    auto part_beta = [&] { const double b = first ? beta : 1.0; first = false; return b; };
    if (plan.iso.present) {
        rc = dense_mvm_on_device(ctx, plan.iso.ptr(), X, Y, a, lda, y, ldy, nrhs, alpha, part_beta()); if (rc) return rc;
        ctx->last_mixed_path |= 4;
    }
    if (plan.dot.present) {
        rc = dense_mvm_on_device(ctx, plan.dot.ptr(), X, Y, a, lda, y, ldy, nrhs, alpha, part_beta()); if (rc) return rc;
        ctx->last_mixed_path |= 8;
    }
    if (plan.fused) {
        rc = mixed_fused_device(ctx, plan.fused_hk, X, Y, a, lda, y, ldy, nrhs, alpha, part_beta()); if (rc) return rc;
    }
    if (first) dense_reduce(ctx, dtype, nullptr, n, 1, 0, y, n, ldy, nrhs, 0.0, beta);   // constant terms only
    if (plan.constant != 0.0) {
        rc = constant_term_mvm(ctx, dtype, a, m, lda, 1, y, n, ldy, 1, nrhs, alpha * plan.constant); if (rc) return rc;
        ctx->last_mixed_path |= 32;
    }
    return COVGRAM_OK;
}

}  // namespace

extern "C" {

int covgram_mvm_mixed(covgram_ctx* ctx, const covgram_kernel_composite* k, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda,
                      void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t loc) {
    // the kernel's own refusals come first (host work only; the points' dtype only sizes the Taylor guards)
    CG_REQUIRE(k != nullptr, COVGRAM_EINVAL, "kernel is NULL");
    HostKernel whole;
    int rc = make_composite_kernel(k, X ? X->dtype : COVGRAM_F64, COMPOSITE_MIXED_VALUES, &whole);
    if (rc) return rc;
    MixedPlan plan;
    return block_mvm_entry(
        ctx, X, Y, a, lda, y, ldy, nrhs, beta, loc, false,
        [&](int, int64_t* B) -> int { *B = 1; return COVGRAM_OK; },
        [&]() -> int {
            const int prc = mixed_partition(ctx, k, X->dtype, &plan);
            if (prc == COVGRAM_OK) { ctx->last_mixed_path = 0; ctx->last_mixed_jsplit = 0; }
            return prc;
        },
        [&](const Staged& st) { return mixed_device(ctx, plan, X, Y, st.a, st.lda, st.y, st.ldy, nrhs, alpha, beta); });
}

int covgram_matrix_mixed(covgram_ctx* ctx, const covgram_kernel_composite* k, const covgram_points* X, const covgram_points* Y, void* out, int64_t ldo,
                         int32_t loc) {
    CG_REQUIRE(k != nullptr, COVGRAM_EINVAL, "kernel is NULL");
    HostKernel hk;
    int rc = make_composite_kernel(k, X ? X->dtype : COVGRAM_F64, COMPOSITE_MIXED_VALUES, &hk);
    if (rc) return rc;
    rc = check_pair(ctx, X, Y);
    if (rc) return rc;
    const int64_t n = X->n, m = Y->n;
    CG_REQUIRE(ldo >= n, COVGRAM_EINVAL, "ldo=%lld < n=%lld", (long long)ldo, (long long)n);
    CG_REQUIRE(out != nullptr || n * m == 0, COVGRAM_EINVAL, "out is NULL");
    const int dtype = X->dtype;
    CG_DEVICE(ctx);
    ctx->last_mixed_matrix_path = 0;
    if (n == 0 || m == 0) return COVGRAM_OK;
    Staged st;
    rc = st.begin_tile(ctx, loc, dtype_size(dtype), out, ldo, n, m);
    if (rc) return rc;
    const int d = X->d;
    const int64_t strips = (m + 63) / 64;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)std::min<int64_t>(strips, 65535));
    ctx->last_mixed_matrix_path = d <= 32 ? 1 : 2;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const ExprParams<T> ep = make_params<FAM_EXPR_DOT, T>(hk);
        TimerScope tm(ctx);
        // (the bucket is one of the list: nothing to refuse)
        try_dim(Dims<0, 4, 8, 16, 32>{}, mixv_bucket(d), [&](auto D) {
            hipLaunchKernelGGL((mixed_matrix_kernel<T, decltype(D)::value>), grid, dim3(256), 0, ctx->stream, (const T*)X->dptr, n, (const T*)Y->dptr, m, d,
                               (T*)st.y, st.ldy, (T)hk.kp.scale, ep);
        });
    });
    CG_CHECK_HIP(hipGetLastError());
    return st.finish();
}

}  // extern "C"
