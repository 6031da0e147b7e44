// block_mvm.hip — the block MVM drivers of the derivative kernels: covgram_grad_mvm / covgram_valgrad_mvm (grad_mvm.hpp, grad_bcast.hpp,
// grad_wide.hpp; the column split, the panel plan and the reductions: grad_driver.hpp, shared with grad_mixed.hip) and covgram_hess_mvm /
// covgram_valgradhess_mvm (hess_mvm.hpp).
#include <math.h>

#include <algorithm>

#include "grad_driver.hpp"
#include "dense_mvm.hpp"
#include "grad_bcast.hpp"
#include "hess_mvm.hpp"

using namespace covgram;

// the automatic choice of the broadcast kernel by padded dimension (tools/c4_bcast_ab.py, profiles/r04_c4_bcast_ab.txt: n = 16384, EQ,
// scalar stream -> broadcast, four waves per workgroup: d = 8 x0.91, 16 x0.95, 24 x1.23, 32 (C4) x1.25, 48 x1.83)
#ifndef GRAD_BCAST_AUTO
#define GRAD_BCAST_AUTO(D) ((D) >= 24 ? 4 : 0)
#endif


extern "C" {

// on device-resident a and y that do not overlap, one kernel (a Sum arrives term by term)
static int grad_mvm_device(covgram_ctx* ctx, const covgram_kernel* k, const HostKernel& hk, const covgram_points* X, const covgram_points* Y,
                           const void* a_all, int64_t lda_d, void* y_all, int64_t ldy_d, int32_t nrhs, double alpha, double beta, int vg) {
    int rc;
    const int64_t n = X->n, m = Y->n;
    const int d = X->d;
    const int bd = d + vg;                                  // entries per block of a and y
    const int dtype = X->dtype;
    const size_t ts = dtype_size(dtype);
    // lane-owned rows up to d = 64 (fp32) / 48 (fp64) (grad_mvm.hpp); wider rows take the two-kernel panel path (grad_wide.hpp)
    // (Round 1 sent composites with d >= 8 to the panel path too: the lane-per-row kernel, interpreting their jets once per pair
    // at 3 waves per SIMD, spilled — C4-shaped EQ*RQ 16.1 ms against 8.9.  With the registers the interpreter needs — two waves per
    // SIMD for fp64, grad_temp_regs — it is the faster one at every d it reaches: tools/compgrad_ab.py, panel / lane-per-row:
    // fp64 EQ*RQ d = 32 12.2 / 10.5 ms, d = 48 17.9 / 13.1, MaternP(2)*EQ d = 8 10.1 / 4.1; fp32 d = 32 3.9 / 1.7, d = 8 3.5 / 1.2.)
    bool heavy_factor = false;                                       // a composite with a Matern(nu) factor: the lane-per-row interpreter is built without it
    if (hk.tu_family >= COVGRAM_NFAMILY) {
        int nf = 0;
        for (int t = 0; t < hk.nterms; ++t) nf += hk.nfac[t];
        for (int f = 0; f < nf; ++f) heavy_factor = heavy_factor || hk.ffam[f] == COVGRAM_MATERN;
    }
    const bool wide = d > (dtype == COVGRAM_F64 ? 48 : 64) || ctx->grad_keep_r == 2 || heavy_factor;
    const int D = wide ? ((d + 31) / 32) * 32 : pad_dim(d);
    grad_launch_fn launch = grad_launcher(hk.tu_family);
    ctx->last_grad_path = 0; ctx->last_grad_jsplit = 0; ctx->last_grad_expand = 0; ctx->last_grad_bcast = 0;
    if (n == 0) return COVGRAM_OK;
    const bool iso = (k->trait == COVGRAM_ISOTROPIC);
    const void* Cn = iso ? Y->center : nullptr;
    const double alpha0 = alpha * hk.kp.scale;              // value row of the value-gradient blocks
    // isotropic: b = -2 gamma^2 (psi' a + 2 psi'' r'(r'.a));  dot product: b = k1 a + k2 y (x.a)
    const double alpha_eff = alpha * hk.kp.scale * (iso ? -2.0 * hk.kp.gamma2 : 1.0);
    const int64_t rowblocks = (n + GRAD_THREADS - 1) / GRAD_THREADS;
    const int64_t npad = rowblocks * GRAD_THREADS;
    // two right-hand sides per pass where the lane-per-row kernel is compiled for it (grad_mvm.hpp: r, s, phi', phi'' once per pair)
    const bool two_ok = !wide && m > 0 && hk.k.power == 1 && grad_two_rhs_ok(ts, D, hk.tu_family);
    // expanded form (grad_mvm.hpp): fp64 isotropic simple profiles whose pre-scaled clouds lie within the radius gate
    // fp32 (round 5): the same form inside GRAD_EXPAND_GATE_F32 — there the absolute error of s is a few fp32 roundings of R^2, what the fp32
    // matrix-core dense kernels carry inside their gate of the same size (dense_mfma.hip), measured at the gate in tests/test_gpu_grad_expand32.py
    const double expand_gate = dtype == COVGRAM_F64 ? GRAD_EXPAND_GATE : GRAD_EXPAND_GATE_F32;
    const bool expd = !wide && m > 0 && iso && hk.tu_family < COVGRAM_NFAMILY && ctx->grad_keep_r != 1 && !(dtype == COVGRAM_F32 && hk.k.power != 1) &&
                          (ctx->grad_expand == 1 ||
                           // measured (tools/c4_expand_ab.py, profiles/r02_c4_expand_ab.txt): pays from d = 8 (C4 0.86x, d = 8 0.95x,
                           // d = 3 +4 %); MaternP(p >= 1) 0.89x since its exp(-r) is the library's own (it was +3 % with the
                           // 34-instruction one).  Never by default for the profiles that are singular at s = 0 (exponential,
                           // gamma-exponential, MaternP(0)): their diagonal blocks are NaN in the reference (inf * 0), which the
                           // exact zero of a direct difference reproduces and the rounded zero of the expanded form would not
                           // fp32 (tools/grad32_expand_ab.py, profiles/r05_grad32_expand_ab.txt, n = 16384): EQ d = 32 994 -> 828 us, d = 48 (n = 8192) 523 -> 391,
                           // d = 16 552 -> 457; RQ 0.85-0.94x; MaternP only from d = 32 (d = 8, 16: 1.12-1.19x — its jet's square root and the
                           // expanded form's clamp sit in front of a shorter dimension loop)
                           (ctx->grad_expand < 0 && D >= 8 && !(dtype == COVGRAM_F32 && hk.tu_family == COVGRAM_MATERNP && D < 32) &&
                            hk.tu_family != COVGRAM_MATERN && hk.tu_family != COVGRAM_EXP &&
                            hk.tu_family != COVGRAM_GAMMAEXP && !(hk.tu_family == COVGRAM_MATERNP && hk.k.p == 0) &&
                            hk.kp.gamma2 * gate_radius2(X, Y) <= expand_gate));
    // round 4: the expanded form with the column records in VGPRs (grad_bcast.hpp; option "grad_bcast": -1 auto, 0 never, 1 / 4 = with
    // that many waves per workgroup).  One right-hand side per pass: where it applies, matrix right-hand sides run column by column on it
    // (C4 shape: 2 x 1.36 ms against 3.30 ms for the scalar-stream kernel's two-column pass)
    int bcast = 0;
    if (expd && dtype == COVGRAM_F64 && hk.k.power == 1 && grad_bcast_ok(D) && hk.tu_family != COVGRAM_MATERN && ctx->grad_bcast != 0)
        bcast = ctx->grad_bcast == 1 ? 1 : (ctx->grad_bcast == 4 ? 4 : GRAD_BCAST_AUTO(D));
    for (int c0 = 0; c0 < nrhs;) {
        const int nr = (two_ok && !bcast && c0 + 1 < nrhs) ? 2 : 1;
        const void* a_dev = (const char*)a_all + (size_t)c0 * lda_d * ts;
        void* y_dev = (char*)y_all + (size_t)c0 * ldy_d * ts;
        if (m == 0) {                                           // no columns: y <- beta y
            grad_reduce(ctx, dtype, nullptr, npad, D, 0, y_dev, n, d, vg, nr, 0, 0.0, 0.0, beta);
        } else if (wide) {
            GradPanelPlan pp;
            rc = grad_panel_plan(ctx, dtype, n, m, D, bd, 0, &pp); if (rc) return rc;
            grad_wide_launch_fn wlaunch = grad_wide_launcher(hk.tu_family);
            ctx->last_grad_path |= 4 | (pp.several() ? 8 : 0) | (pp.zs > 1 ? 16 : 0);
            rc = grad_panel_route(ctx, pp, dtype, n, bd, vg, y_dev, alpha_eff, alpha0, beta, [&](int64_t col0, int64_t pc, int accumulate) -> int {
                const int64_t npad64 = pp.npad64;
                void *P, *C;
                // stream + (value-gradient) the columns' value weights; coefficient slabs C1, C2 + the value row's block partials C0
                int prc = ws_reserve(ctx, 0, (size_t)pc * (D * 2 + vg) * ts, &P); if (prc) return prc;
                prc = ws_reserve(ctx, 1, ((size_t)pc * 2 + (vg ? (size_t)(pc / pp.BC) : 0)) * npad64 * ts, &C); if (prc) return prc;
                void* A0P = vg ? (void*)((char*)P + (size_t)pc * D * 2 * ts) : nullptr;
                void* C0 = vg ? (void*)((char*)C + (size_t)pc * 2 * npad64 * ts) : nullptr;
                const int64_t pe = pc * (int64_t)D;
                by_dtype(dtype, [&](auto t) {
                    using T = decltype(t);
                    hipLaunchKernelGGL(grad_wide_pack_kernel<T>, dim3((unsigned)((pe + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)Y->dptr, m, d, D,
                                       (const T*)a_dev, col0, pc, (T*)P, pp.PKN, (T)hk.kp.gamma, vg, (T*)A0P, (const T*)Cn);
                });
                GradWideArgs wa;
                wa.Cn = Cn;
                wa.vg = vg; wa.A0P = A0P; wa.C0 = C0; wa.alpha0 = pp.zs > 1 ? 1.0 : alpha0;
                wa.vg_c = (iso ? -1.0 : 1.0) / hk.kp.gamma; wa.vg_b = iso ? -2.0 * hk.kp.gamma : hk.kp.gamma;
                wa.X = X->dptr; wa.n = n; wa.d = d; wa.dpad = D; wa.P = P; wa.C1 = C; wa.C2 = (char*)C + (size_t)pc * npad64 * ts;
                wa.npad = npad64; wa.nblocks = pc / pp.BC; wa.y = y_dev; wa.alpha = alpha_eff; wa.beta = beta; wa.accumulate = accumulate;
                if (pp.zs > 1) { wa.zs = pp.zs; wa.zstride = pp.total; wa.y = pp.zslab; wa.alpha = 1.0; wa.beta = 0.0; }
                wa.hk = &hk; wa.stream = ctx->stream;
                TimerScope tm(ctx);
                return wlaunch(wa, dtype);
            });
            if (rc) return rc;
        } else {
            void* P;
            // + 1 prefetch-only record; the value weights A0[0..m] of the value-gradient variant follow the stream
            rc = ws_reserve(ctx, 0, (size_t)(m + 1) * ((1 + nr) * D + nr * vg + (expd ? 1 + nr : 0)) * ts, &P); if (rc) return rc;
            void* A0 = vg ? (void*)((char*)P + (size_t)(m + 1) * (1 + nr) * D * ts) : nullptr;
            void* Ex = expd ? (void*)((char*)P + (size_t)(m + 1) * ((1 + nr) * D + nr * vg) * ts) : nullptr;
            const int64_t pe = (m + 1) * (int64_t)D;
            by_dtype(dtype, [&](auto t) {
                using T = decltype(t);
                hipLaunchKernelGGL(grad_pack_kernel<T>, dim3((unsigned)((pe + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)Y->dptr, m, d, (const T*)a_dev, (T*)P,
                                   D, (T)hk.kp.gamma, vg, (T*)A0, (const T*)Cn, nr, lda_d);
                if (!expd) return;
#define CG_PEL(DLV) hipLaunchKernelGGL((grad_pack_extra_lanes_kernel<T, DLV>), dim3((unsigned)(((m + 1) * DLV + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)Y->dptr, m, \
                                       (const T*)a_dev, (T)hk.kp.gamma, vg, (const T*)Cn, (T*)Ex, nr, lda_d)
                if (d == 8) CG_PEL(8); else if (d == 16) CG_PEL(16); else if (d == 32) CG_PEL(32); else if (d == 64) CG_PEL(64);
                else hipLaunchKernelGGL(grad_pack_extra_kernel<T>, dim3((unsigned)((m + 256) / 256)), dim3(256), 0, ctx->stream, (const T*)Y->dptr, m, d,
                                        (const T*)a_dev, (T)hk.kp.gamma, vg, (const T*)Cn, (T*)Ex, nr, lda_d);
#undef CG_PEL
            });
            ctx->last_grad_bcast = bcast;
            const int bwaves = std::max(1, std::min(4, 512 / (4 * D + 4 * ((2 * D + 15) / 16) + 44)));   // grad_bcast_waves<D>()
            const int gthreads = bcast ? 64 * bcast : grad_block_threads((int)ts, D, hk.tu_family);          // 64 or 256 threads per workgroup (grad_mvm.hpp)
            // the workgroups resident at once: where the slab cap binds, the column split snaps to whole rounds of them (grad_driver.hpp)
            const int64_t gslots = (int64_t)ctx->num_cus * 4 * (bcast ? bwaves : grad_waves_per_simd((int)ts, D, hk.tu_family)) / (gthreads / 64);
            rc = grad_lane_route(ctx, dtype, n, m, d, D, vg, nr, gthreads, gslots, npad, y_dev, ldy_d, alpha_eff, alpha0, beta, [&](int64_t jchunk, int jsplit, void* out) -> int {
                GradArgs ga;
                ga.C = Cn;
                ga.X = X->dptr; ga.n = n; ga.d = d; ga.P = P; ga.m = m; ga.npad = npad; ga.Dpad = D; ga.jchunk = jchunk; ga.jsplit = jsplit; ga.keep_r = (int)ctx->grad_keep_r;
                ga.alpha = alpha_eff; ga.beta = beta; ga.hk = &hk; ga.stream = ctx->stream; ga.out = out;
                ga.vg = vg; ga.A0 = A0; ga.alpha0 = alpha0;
                ga.expd = expd ? 1 : 0; ga.Ex = Ex; ga.bcast = bcast;
                ga.nr = nr; ga.ldy = ldy_d;
                ctx->last_grad_expand = ga.expd;
                ctx->last_grad_jsplit = jsplit;
                ctx->last_grad_path |= 1 | (nr == 2 ? 2 : 0) | (jsplit > 1 ? 32 : 0);
                ga.vg_c = (iso ? -1.0 : 1.0) / hk.kp.gamma;
                ga.vg_b = iso ? -2.0 * hk.kp.gamma : hk.kp.gamma;
                TimerScope tm(ctx);
                return launch(ga, dtype);
            });
            if (rc) return rc;
        }
        c0 += nr;
    }   // right-hand sides
    return COVGRAM_OK;
}

// vg = 0: GradientKernel blocks (d × d); vg = 1: ValueGradientKernel blocks ((d+1) × (d+1))
// a: (m bd) x nrhs, y: (n bd) x nrhs, column-major (lda, ldy), bd = d + vg entries per block (src/gramian.jl:241-257: blockmul! takes
// vectors OF MATRICES too, and the block mul! of src/gradient.jl:86-92 broadcasts over their columns)
static int grad_mvm_impl(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda,
                         void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t loc, int vg) {
    // derivatives are linear in the kernel: a Sum runs term by term as well
    // (always split: the one-pass Sum kernels of covgram_mvm (dense_mfma.hip: sum_fused_applies) are value kernels only — there is no
    //  one-pass gradient form, and the unsplit Sum would run the composite interpreter instead of each term's own kernel)
    SumSplit split;
    bool sum = false;
    HostKernel hk;
    return block_mvm_entry(
        ctx, X, Y, a, lda, y, ldy, nrhs, beta, loc, true,
        [&](int d, int64_t* B) -> int { *B = d + vg; return COVGRAM_OK; },
        [&]() -> int {
            sum = composite_sum_terms(ctx, k, loc, &split);
            return make_host_kernel(k, X->dtype, true, &hk);     // (a split Sum: the composite's own validation still applies)
        },
        [&](const Staged& st) -> int {
            if (!sum) return grad_mvm_device(ctx, k, hk, X, Y, st.a, st.lda, st.y, st.ldy, nrhs, alpha, beta, vg);
            return sum_split_run(
                split, beta,
                [&](const covgram_kernel* tk, double tbeta) {
                    HostKernel thk;
                    const int trc = make_host_kernel(tk, X->dtype, true, &thk);
                    return trc ? trc : grad_mvm_device(ctx, tk, thk, X, Y, st.a, st.lda, st.y, st.ldy, nrhs, alpha, tbeta, vg);
                },
                [&] {   // a constant has zero derivatives: only the value-value entry of the value-gradient blocks sees it
                    return vg ? constant_term_mvm(ctx, X->dtype, st.a, Y->n, st.lda, X->d + 1, st.y, X->n, st.ldy, X->d + 1, nrhs, alpha * split.constant) : COVGRAM_OK;
                });
        });
}

int covgram_grad_mvm(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda,
                     void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t loc) {
    return grad_mvm_impl(ctx, k, X, Y, a, lda, y, ldy, nrhs, alpha, beta, loc, 0);
}

int covgram_valgrad_mvm(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda,
                        void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t loc) {
    return grad_mvm_impl(ctx, k, X, Y, a, lda, y, ldy, nrhs, alpha, beta, loc, 1);
}

// Hessian-kernel Gramian (vgh = 0: n d^2 x m d^2) and value-gradient-Hessian-kernel Gramian (vgh = 1: n (1 + d + d^2) x m (1 + d + d^2)):
// hess_mvm.hpp.  One driver: the two differ in the block size, the column record, the launcher, the info key and in where the powers of
// gamma go (Hessian: gamma^4 into alpha here; VGH: per part of the block in the pack launch and the kernel's epilogue, so only the
// constant factor goes into alpha).
static int hess_mvm_impl(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda,
                         void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t loc, int vgh) {
    int rc = check_pair(ctx, X, Y);
    if (rc) return rc;
    CG_REQUIRE(k != nullptr, COVGRAM_EINVAL, "kernel is NULL");
    const char* w = vgh ? "ValueGradientHessianKernel" : "HessianKernel";
    const int d = X->d;
    rc = hess_refusal(w, k, d);
    if (rc) return rc;
    CG_REQUIRE(nrhs >= 1, COVGRAM_EINVAL, "nrhs must be >= 1");
    const int64_t n = X->n, m = Y->n, bd = (vgh ? 1 + (int64_t)d : 0) + (int64_t)d * d;
    CG_REQUIRE(lda >= m * bd && ldy >= n * bd, COVGRAM_EINVAL, "lda / ldy smaller than the block vectors (%lld, %lld)", (long long)(m * bd), (long long)(n * bd));
    CG_REQUIRE((a != nullptr || m == 0) && (y != nullptr || n == 0), COVGRAM_EINVAL, "a or y is NULL");
    const int dtype = X->dtype;
    const size_t ts = dtype_size(dtype);
    HostKernel hk;
    rc = make_host_kernel(k, dtype, true, &hk);
    if (rc) return rc;
    hess_launch_fn launch = vgh ? vgh_launcher(hk.tu_family) : hess_launcher(hk.tu_family);
    CG_REQUIRE(launch != nullptr, COVGRAM_EUNSUPPORTED, "%s(%s) has no device path", w, kFamilyNames[k->family]);
    CG_DEVICE(ctx);
    int64_t& last_path = vgh ? ctx->last_vgh_path : ctx->last_hess_path;
    last_path = 0;
    if (n == 0) return COVGRAM_OK;
    Staged st;
    rc = st.begin(ctx, loc, ts, a, lda, m * bd, y, ldy, n * bd, nrhs, beta);
    if (rc) return rc;
    const bool iso = (k->trait == COVGRAM_ISOTROPIC);
    const int D = hess_pad_dim(d);
    const int rec = hess_rec(D, vgh != 0);
    // Hessian: d^4 k / dx dx dy dy in the pre-scaled coordinates gamma (x - c): gamma^4 by the chain rule (dot product: gamma = 1)
    const double alpha_eff = vgh ? alpha * hk.kp.scale : alpha * hk.kp.scale * (iso ? hk.kp.gamma2 * hk.kp.gamma2 : 1.0);
    const int64_t total = n * bd;
    // Column split: a workgroup holds 256 / D row points, so small n leaves most of the chip idle; split the columns over up to
    // ~8 workgroups per CU, at least 4 staged chunks each, with the partial slabs (split x n bd scalars) within 256 MB
    const int ppw = HESS_THREADS / D;
    const int64_t rowwgs = (n + ppw - 1) / ppw;
    const int64_t minchunk = 4 * (int64_t)hess_jc(D, (int)ts, vgh != 0);
    int64_t split = std::max<int64_t>(1, ((int64_t)ctx->num_cus * 8 + rowwgs - 1) / rowwgs);
    split = std::min(split, std::max<int64_t>(1, m / minchunk));
    split = std::min(split, std::max<int64_t>(1, (int64_t)(256.0e6 / ((double)total * ts))));
    if (ctx->jsplit > 0) split = std::min<int64_t>(ctx->jsplit, std::max<int64_t>(1, m));
    int64_t jchunk = std::max<int64_t>(1, (m + split - 1) / split);
    const int jsplit = m > 0 ? (int)((m + jchunk - 1) / jchunk) : 0;
    void *P = nullptr, *slab = nullptr;
    if (m > 0) { rc = ws_reserve(ctx, 0, (size_t)m * rec * ts, &P); if (rc) return rc; }
    if (jsplit > 1) { rc = ws_reserve(ctx, 1, (size_t)jsplit * total * ts, &slab); if (rc) return rc; }
    const void* Cn = iso ? Y->center : nullptr;
    for (int c0 = 0; c0 < nrhs; ++c0) {
        const void* a_dev = (const char*)st.a + (size_t)c0 * st.lda * ts;
        void* y_dev = (char*)st.y + (size_t)c0 * st.ldy * ts;
        if (m > 0) {
            const int64_t pe = m * (int64_t)rec;
            by_dtype(dtype, [&](auto t) {
                using T = decltype(t);
                auto kern = vgh ? hess_pack_kernel<T, true> : hess_pack_kernel<T, false>;
                hipLaunchKernelGGL(kern, dim3((unsigned)((pe + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)Y->dptr, m, d, (const T*)a_dev, (T*)P, D,
                                   (T)hk.kp.gamma, (const T*)Cn);
            });
            HessArgs ha;
            ha.X = X->dptr; ha.n = n; ha.d = d; ha.P = P; ha.m = m; ha.out = jsplit > 1 ? slab : y_dev; ha.Dpad = D; ha.jchunk = jchunk; ha.jsplit = jsplit;
            ha.C = Cn; ha.alpha = alpha_eff; ha.beta = beta; ha.hk = &hk; ha.stream = ctx->stream;
            { TimerScope tm(ctx); rc = launch(ha, dtype); }
            if (rc) return rc;
            last_path = 1;
        }
        if (jsplit != 1) {   // several column chunks: fixed-order sum of their slabs; no columns: y <- beta y
            const dim3 rg((unsigned)((total + 255) / 256));
            by_dtype(dtype, [&](auto t) {
                using T = decltype(t);
                hipLaunchKernelGGL(hess_reduce_kernel<T>, rg, dim3(256), 0, ctx->stream, (const T*)slab, jsplit, total, (T*)y_dev, (T)alpha_eff, (T)beta);
            });
        }
    }
    CG_CHECK_HIP(hipGetLastError());
    return st.finish();
}

int covgram_hess_mvm(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda,
                     void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t loc) {
    return hess_mvm_impl(ctx, k, X, Y, a, lda, y, ldy, nrhs, alpha, beta, loc, 0);
}

int covgram_valgradhess_mvm(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda,
                            void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t loc) {
    return hess_mvm_impl(ctx, k, X, Y, a, lda, y, ldy, nrhs, alpha, beta, loc, 1);
}

}  // extern "C"
