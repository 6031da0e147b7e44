// dense_driver.hpp — the host plan of the scalar lane-per-row routes (covgram_mvm's lane-per-row and broadcast kernels in api.hip, the fused kernel
// of covgram_mvm_mixed in mixed_mvm.hip): the column split, the partial slabs and the fixed-order reduction behind them, which the matrix-core
// drivers (dense_mfma.hip) share.  The scalar mirror of grad_driver.hpp.  The split rule and the slab layout are the summation
// order of a product: they stand here once.  The kernels in between and the column streams they read are the drivers' own.  Host code only.
#pragma once
#include "driver.hpp"
#include "dense_mvm.hpp"

namespace covgram {

// y <- alpha * (sum of the jsplit partial slabs, [split][NRpad][npad]) + beta y over nr right-hand sides, in fixed order; with no slab (jsplit = 0:
// the product has no columns, or nothing but constant terms) y <- beta y.  The only launch site of dense_reduce_kernel.  A unit of one element type
// (dense_mfma.hip) calls the typed form; the form by dtype is a template so that such a unit does not get the other type's kernel instance from it.
template <typename T>
inline void dense_reduce(covgram_ctx* ctx, const T* slab, int64_t npad, int NRpad, int jsplit, T* y, int64_t n, int64_t ldy, int nr, double alpha, double beta) {
    hipLaunchKernelGGL(dense_reduce_kernel<T>, dim3((unsigned)((n + 63) / 64), (unsigned)nr), dim3(256), 0, ctx->stream, slab, npad, NRpad, jsplit, y, n, ldy, nr,
                       (T)alpha, (T)beta);
}
template <typename Ctx>
inline void dense_reduce(Ctx* ctx, int dtype, const void* slab, int64_t npad, int NRpad, int jsplit, void* y, int64_t n, int64_t ldy, int nr, double alpha,
                         double beta) {
    by_dtype(dtype, [&](auto t) { dense_reduce(ctx, (const decltype(t)*)slab, npad, NRpad, jsplit, (decltype(t)*)y, n, ldy, nr, alpha, beta); });
}

// The lane-per-row route of one pass over m > 0 columns (nr right-hand sides in NRpad slots, `rowblocks` workgroups of rows padded to npad):
// splits the columns into chunks of whole 64-column blocks (default_target: the caller's measured workgroup target, 0 for choose_split's own),
// reserves the partial slabs (workspace slot 1), has launch(jchunk, jsplit, out, tickets) run the kernel into them under the timer — into y
// itself when one workgroup per row block walks every column — and sums the slabs into y.  inkernel: the kernel can sum its own slabs (the
// last-arriving workgroup of each row block, pack.hpp); where option "inkernel_reduce" asks for that, `tickets` are its zeroed counters and
// no reduction is launched, else `tickets` is NULL.  The caller packs its column stream first and records its own info keys in launch.
template <typename Launch>
inline int dense_lane_route(covgram_ctx* ctx, int dtype, int64_t rowblocks, int64_t npad, int64_t n, int64_t m, int nr, int NRpad, int64_t default_target,
                            bool inkernel, void* y, int64_t ldy, double alpha, double beta, Launch launch) {
    int64_t jchunk; int jsplit;
    choose_split(ctx, rowblocks, m, 64, &jchunk, &jsplit, default_target);
    void* out = y;
    unsigned* tickets = nullptr;
    int rc;
    if (jsplit > 1) { rc = ws_reserve(ctx, 1, (size_t)jsplit * NRpad * npad * dtype_size(dtype), &out); if (rc) return rc; }
    if (inkernel && inkernel_reduce_on(ctx, false, n, jsplit)) { rc = tickets_reserve(ctx, (size_t)rowblocks, &tickets); if (rc) return rc; }
    { TimerScope tm(ctx); rc = launch(jchunk, jsplit, out, tickets); }
    if (rc) return rc;
    if (jsplit > 1 && !tickets) dense_reduce(ctx, dtype, out, npad, NRpad, jsplit, y, n, ldy, nr, alpha, beta);
    return COVGRAM_OK;
}

}  // namespace covgram
