// grad_driver.hpp — the host plans of the two gradient block-MVM drivers, grad_mvm_device (block_mvm.hip: one input trait) and grad_mixed_device
// (grad_mixed.hip: every factor its own trait): the column split of the lane-per-row route, the panel plan of the route for wide rows and the
// fixed-order reductions behind both.  The kernels in between and the workspace layouts of their operands are the drivers' own.  Host code only.
#pragma once
#include <math.h>

#include <algorithm>

#include "driver.hpp"
#include "grad_mvm.hpp"
#include "grad_wide.hpp"

namespace covgram {

// y <- alpha * (sum of the jsplit partial slabs) + beta y over the (d + vg)-entry blocks of nr right-hand sides, in fixed order; with no slab
// (jsplit = 0: the product has no columns) y <- beta y
inline void grad_reduce(covgram_ctx* ctx, int dtype, const void* slab, int64_t npad, int D, int jsplit, void* y, int64_t n, int d, int vg, int nr,
                        int64_t ldy, double alpha, double alpha0, double beta) {
    const dim3 rgrid((unsigned)((n + 255) / 256), (unsigned)(d + vg), (unsigned)nr);
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(grad_reduce_kernel<T>, rgrid, dim3(256), 0, ctx->stream, (const T*)slab, npad, D, jsplit, (T*)y, n, d, (T)alpha, (T)beta, vg, (T)alpha0,
                           ldy);
    });
}

// The lane-per-row route of one pass (nr right-hand sides, workgroups of `gthreads` threads, rows padded to npad): splits the m columns,
// reserves the partial slabs (workspace slot 1), has launch(jchunk, jsplit, out) run the kernel into them — into y itself when one
// workgroup per row block walks every column — and sums the slabs into y.
// gslots > 0, the workgroups resident on the chip at once: the slab cap binds only where neither "jsplit" nor "target_wgs" is set, and then
// snaps down to a whole number of resident rounds; gslots = 0: the cap always binds, as it stands.  (The column split is the summation order:
// each driver keeps the rule it was measured and tested with.)
template <typename Launch>
inline int grad_lane_route(covgram_ctx* ctx, int dtype, int64_t n, int64_t m, int d, int D, int vg, int nr, int gthreads, int64_t gslots, int64_t npad,
                           void* y, int64_t ldy, double alpha, double alpha0, double beta, Launch launch) {
    const size_t ts = dtype_size(dtype);
    // partial slabs cost jsplit * n * d * sizeof(T) bytes, but several rounds of workgroups balance the tail
    // (C4: 2.47 ms at CUs*8, 2.08 at CUs*32, 2.01 at CUs*64, 2.05 at CUs*96, 2.15 at CUs*128 — interleaved A/B, tools/c4_ab.py)
    // Column split: about 64 waves per CU over the launch (round 1's sweep), then (round 2, tools/c4_jsplit_sweep.py)
    //  * capped so that the partial slabs (split x n x d results, written here and read back by the reduction) stay inside the
    //    256 MB Infinity Cache — C4 at 64 splits writes 268 MB, d = 48 403 MB: 3.86 ms against 3.61 at 48 splits —
    //  * and, when that cap binds, snapped DOWN to a whole number of rounds of resident workgroups if one lies within reach (the
    //    waves of the EQ kernel all take the same time, so a ragged last round idles most of the chip: C4 at 64 row workgroups x
    //    {36, 42, 48, 54, 60} splits = {3.0, 3.5, 4.0, 4.5, 5.0} rounds: 1.744, 1.853, 1.748, 1.809, 1.770 ms).
    //  Old and new library alternating on one box: C4 1.79 -> 1.77 ms, value-gradient -2 %, d = 48 3.85 -> 3.65; the heavier
    //  profiles at the C4 shape lose 1.5 % (MaternP(2) 2.33 -> 2.37, RQ 3.60 -> 3.66): their slab is the same 268 MB but a
    //  smaller share of a longer kernel.
    const int64_t growwgs = (n + gthreads - 1) / gthreads;
    int64_t gsplit = std::max<int64_t>(1, ((int64_t)ctx->num_cus * 64 * 64 / gthreads + growwgs - 1) / growwgs);
    gsplit = std::min(gsplit, std::max<int64_t>(1, m / 64));   // >= 64 columns per workgroup: below that its prologue and slab rows dominate
                                                                // (tools/c4_jsplit_sweep.py small: n = 4096, d = 8: 16-column chunks 0.109 ms, 64-column 0.059)
    const int64_t width = (int64_t)(D + vg) * nr;              // slab entries per row
    const int64_t gcap = std::max<int64_t>(1, (int64_t)(256.0e6 / ((double)npad * width * ts)));
    if (gslots <= 0) gsplit = std::min(gsplit, gcap);
    else if (ctx->jsplit <= 0 && ctx->target_wgs <= 0 && gsplit > gcap) {
        gsplit = gcap;
        for (int64_t js = gsplit; js >= std::max<int64_t>(1, gsplit / 2); --js) {
            const double rounds = (double)(js * growwgs) / (double)gslots;
            const double ragged = std::ceil(rounds) - rounds;
            if (rounds >= 1.0 && ragged <= 0.04) { gsplit = js; break; }
        }
    }
    int64_t jchunk; int jsplit;
    choose_split(ctx, growwgs, m, 8, &jchunk, &jsplit, gsplit * growwgs);
    void* out = y;
    int rc;
    if (jsplit > 1) { rc = ws_reserve(ctx, 1, (size_t)jsplit * width * npad * ts, &out); if (rc) return rc; }
    rc = launch(jchunk, jsplit, out);
    if (rc) return rc;
    if (jsplit > 1) grad_reduce(ctx, dtype, out, npad, D, jsplit, y, n, d, vg, nr, ldy, alpha, alpha0, beta);
    return COVGRAM_OK;
}

// The panel route of one right-hand side: the columns go through in panels of whole column blocks (BC = GJG groups of PKN packed columns),
// each panel's pair coefficients in slabs of npad64 rows that a second kernel applies.
struct GradPanelPlan {
    int PKN;                  // columns per packed value: 2 (fp32) or 1
    int64_t BC, mpad, npad64;
    int64_t panel;            // columns per panel, a multiple of BC
    int zs;                   // z slices over a panel's column blocks
    void* zslab;              // zs > 1: their output slabs, `total` entries each (workspace slot 4)
    int64_t total;
    bool several() const { return mpad > panel; }
};

// panel_cap > 0: at most that many columns per panel (rounded up to whole blocks)
inline int grad_panel_plan(covgram_ctx* ctx, int dtype, int64_t n, int64_t m, int D, int bd, int64_t panel_cap, GradPanelPlan* p) {
    const size_t ts = dtype_size(dtype);
    p->PKN = (dtype == COVGRAM_F32) ? 2 : 1;
    const int64_t BC = p->BC = (int64_t)GJG * p->PKN;
    p->mpad = ((m + BC - 1) / BC) * BC;
    p->npad64 = ((n + 63) / 64) * 64;
    p->panel = (((int64_t)256 << 20) / (p->npad64 * 2 * (int64_t)ts)) / BC * BC;   // coefficient slabs C1, C2 <= 256 MB
    if (panel_cap > 0) p->panel = std::min<int64_t>(p->panel, ((panel_cap + BC - 1) / BC) * BC);
    p->panel = std::max<int64_t>(BC, std::min<int64_t>(p->panel, p->mpad));
    // (row blocks x dimension chunks) waves may not fill the chip: split each panel's column blocks over z slices that
    // accumulate raw sums into their own output slabs, reduced in fixed order after the last panel
    const int64_t waves = (p->npad64 / 64) * (D / 32);
    p->zs = (int)std::min<int64_t>(16, std::max<int64_t>(1, ((int64_t)ctx->num_cus * 16 + waves - 1) / waves));
    p->zs = (int)std::min<int64_t>(p->zs, std::max<int64_t>(1, p->panel / BC));
    p->zslab = nullptr;
    p->total = n * (int64_t)bd;
    return p->zs > 1 ? ws_reserve(ctx, 4, (size_t)p->zs * p->total * ts, &p->zslab) : COVGRAM_OK;
}

// panel(col0, pc, accumulate) packs and runs the pc columns from col0 on — into y (accumulate: on top of the panels before), or, with z slices,
// raw sums into the plan's slabs —; the slabs are then summed into y <- alpha (.) + beta y (alpha0: the value row of value-gradient blocks)
template <typename Panel>
inline int grad_panel_route(covgram_ctx* ctx, const GradPanelPlan& p, int dtype, int64_t n, int bd, int vg, void* y, double alpha, double alpha0, double beta,
                            Panel panel) {
    for (int64_t col0 = 0; col0 < p.mpad; col0 += p.panel) {
        const int rc = panel(col0, std::min<int64_t>(p.panel, p.mpad - col0), col0 > 0 ? 1 : 0);
        if (rc) return rc;
    }
    if (p.zs > 1) {
        const dim3 zg((unsigned)((n + 255) / 256), (unsigned)bd);
        by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(grad_wide_reduce_kernel<T>, zg, dim3(256), 0, ctx->stream, (const T*)p.zslab, p.zs, p.total, n, (T*)y, (T)alpha, (T)beta, vg, bd,
                               (T)alpha0);
        });
    }
    return COVGRAM_OK;
}

}  // namespace covgram
