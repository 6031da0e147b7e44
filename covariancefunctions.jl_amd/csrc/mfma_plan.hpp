// mfma_plan.hpp — the planning of the matrix-core MVM drivers (dense_mfma.hip) that is plain arithmetic: the column split of the all-entries kernels and the
// (panel, chunk) work list of the symmetric kernels.  No HIP, no library types: tests/mfma_plan_check.cpp checks it with the host compiler alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace covgram {

// ---- column split of the all-entries kernels: grid = rowtiles x js; wave (i, c) walks the column tiles [c tchunk, min((c + 1) tchunk, ntile)) and leaves its
// partial sums in row c of a slab of npad floats per row (js == 1: straight into y)
struct ColumnPlan { int64_t rowtiles, npad, js, tchunk; };

// n rows in blocks of `rows` (32 x the row tiles per wave), ntile column tiles; the grid aims at `target` waves, or option "jsplit" > 0 asks for
// that many chunks.  A wave keeps >= min_tiles column tiles (8: 256 columns).
// The EQ kernel's two extra clamps (stop_tiles > 0; not applied to a forced jsplit) — GP-sized problems (n = 8k ... 32k): a wave's prologue (row
// fragments), pipeline fill and epilogue (shuffles, slab row) are worth ~40 column tiles of work, so the split stops at stop_tiles = 64 tiles per
// wave — as long as the grid still holds >= floor_waves = 2048 waves, half of the chip's wave slots (tools/eq_small_sweep.py: d = 3, n = 16384
// 45.9 -> 37.9 us, n = 32768 118.8 -> 113.1; d = 8, n = 16384 60.9 -> 47.4, n = 32768 175 -> 152; n = 8192 17.7 -> 16.9 / 25.3 -> 21.8 us)
// (few rows — prediction shapes —: the 2048-wave floor itself stops at floor_tiles = 16 tiles per wave: 256 x 65536, d = 3: 26.8 -> 22.2 us)
inline ColumnPlan plan_columns(int64_t n, int64_t ntile, int rows, int64_t target, int64_t jsplit, int64_t min_tiles, int64_t stop_tiles = 0,
                               int64_t floor_waves = 0, int64_t floor_tiles = 1) {
    ColumnPlan pl;
    pl.rowtiles = (n + rows - 1) / rows;
    pl.npad = pl.rowtiles * rows;
    int64_t js = jsplit > 0 ? jsplit : std::max<int64_t>(1, (target + pl.rowtiles / 2) / pl.rowtiles);
    if (jsplit <= 0 && stop_tiles > 0)
        js = std::max<int64_t>(std::min<int64_t>((floor_waves + pl.rowtiles - 1) / pl.rowtiles, std::max<int64_t>(1, ntile / floor_tiles)),
                               std::min<int64_t>(js, std::max<int64_t>(1, ntile / stop_tiles)));
    js = std::max<int64_t>(1, std::min<int64_t>(js, std::max<int64_t>(1, ntile / min_tiles)));
    pl.tchunk = (ntile + js - 1) / js;
    pl.js = (ntile + pl.tchunk - 1) / pl.tchunk;
    return pl;
}

// ---- graded column split (dense_mfma_eq_kernel) --------------------------------------------------------------------------------------------
// A uniform split hands the chip equal workgroups: a slot that finishes its last one early finds nothing left to take, and the kernel drains at
// the granularity of one workgroup's life (C2: a quarter of the kernel).  The graded split keeps plan_columns' chunk length for the body and cuts
// the LAST portion of the column range — `tail_halfrounds` half rounds of the `slots` resident workgroups, at most half of the chunks — into shorter
// chunks of non-increasing length: each level takes half of what is left in chunks half as long as the level before, down to `floor_tiles`,
// which takes the rest.  Every graded chunk is a multiple of `stage` tiles (what a workgroup of the LDS-shared form fetches at once) except
// possibly the last one, the remainder.  The grid is dispatched chunk-major, so the short chunks start last and fill the slots that free up first.
//   start[0 .. js]: tile offsets of the chunk boundaries (chunk c walks [start[c], start[c + 1])), js <= GRADED_MAX_CHUNKS
//   graded == false: the shape does not admit it (too few chunks or rounds, chunks under the floor, more than 64 chunks) — the uniform plan `base`
//   stands, js = base.js, and start[] holds its equal steps where they fit the table
constexpr int GRADED_MAX_CHUNKS = 64;
struct GradedPlan { bool graded; int64_t js; int32_t start[GRADED_MAX_CHUNKS + 1]; };

// base: the uniform plan; rblocks: workgroups along the rows (grid x); slots: resident workgroups of the instance that will launch, whole chip;
// force: skip the "pays only from two rounds of resident workgroups on" condition (option "mfma_graded" = 1)
inline GradedPlan plan_columns_graded(const ColumnPlan& base, int64_t ntile, int64_t rblocks, int64_t slots, int64_t stage, int64_t floor_tiles,
                                      bool force, int64_t tail_halfrounds = 2) {
    GradedPlan g;
    g.graded = false; g.js = base.js;
    for (int64_t c = 0; c <= GRADED_MAX_CHUNKS; ++c) g.start[c] = (int32_t)std::min<int64_t>(c * base.tchunk, ntile);
    if (base.js < 2 || rblocks < 1 || slots < 1 || stage < 1 || ntile > INT32_MAX) return g;
    if (!force && (rblocks * base.js < 2 * slots || base.tchunk < floor_tiles)) return g;
    const int64_t tail_chunks = std::max<int64_t>(1, std::min<int64_t>((tail_halfrounds * slots + rblocks) / (2 * rblocks), base.js / 2));
    const int64_t body = base.js - tail_chunks;
    for (int64_t floor = (std::max<int64_t>(floor_tiles, 1) + stage - 1) / stage * stage;; floor *= 2) {
        int64_t len = base.tchunk / 2 / stage * stage;
        if (len < floor || body > GRADED_MAX_CHUNKS) return g;        // nothing to grade: the first level would fall under the floor
        int64_t js = body, at = body * base.tchunk, left = ntile - at;
        int32_t start[GRADED_MAX_CHUNKS + 1];
        for (int64_t c = 0; c <= body; ++c) start[c] = (int32_t)(c * base.tchunk);
        bool fits = true;
        while (left > 0 && fits) {
            // chunks of this level: half of what is left (at least one), everything at the floor; the remainder under a chunk goes last
            int64_t k = len > floor ? std::min<int64_t>((left / 2 + len - 1) / len, left / len) : left / len;
            if (len == floor && k == 0) k = 1;
            for (; k > 0 && fits; --k) {
                const int64_t take = std::min(len, left);
                if (js >= GRADED_MAX_CHUNKS) { fits = false; break; }
                at += take; left -= take; start[++js] = (int32_t)at;
            }
            if (len > floor) len = std::max(floor, len / 2 / stage * stage);
            else if (left > 0 && left < len) len = left;               // (the remainder: one last, shorter chunk)
        }
        if (!fits) continue;                                           // more than 64 chunks: a coarser floor
        g.graded = true; g.js = js;
        for (int64_t c = 0; c <= js; ++c) g.start[c] = start[c];
        for (int64_t c = js + 1; c <= GRADED_MAX_CHUNKS; ++c) g.start[c] = (int32_t)ntile;
        return g;
    }
}

// ---- work list of the symmetric kernels ----------------------------------------------------------------------------------------------------
// A panel = tpp row tiles; this call owns the panels pfirst, pfirst + pstride, ... (local numbers 0, 1, ...).  Workgroup (lp, c) walks the column
// tiles [max(c tchunk, first tile of its panel), min((c + 1) tchunk, ntile)): chunks sit at absolute multiples of tchunk, a panel's first one is
// cut at the panel's own first tile.  An entry packs (lp << SYM_CHUNK_BITS) | c; the caller checks sym_list_in_range first.
constexpr int SYM_CHUNK_BITS = 12, SYM_PANEL_BITS = 19;
inline int64_t sym_panels(int64_t ntile, int tpp) { return (ntile + tpp - 1) / tpp; }
inline int64_t sym_local_panels(int64_t ntile, int tpp, int64_t pfirst, int64_t pstride) {
    const int64_t panels = sym_panels(ntile, tpp);
    return panels > pfirst ? (panels - pfirst + pstride - 1) / pstride : 0;
}
inline int64_t sym_chunks(int64_t ntile, int64_t tchunk) { return (ntile + tchunk - 1) / tchunk; }
inline bool sym_list_in_range(int64_t ntile, int tpp, int64_t tchunk, int64_t pfirst, int64_t pstride) {
    return sym_chunks(ntile, tchunk) <= ((int64_t)1 << SYM_CHUNK_BITS) && sym_local_panels(ntile, tpp, pfirst, pstride) < ((int64_t)1 << SYM_PANEL_BITS);
}

// the (local panel, absolute chunk) pairs that exist, chunk-major (the workgroups in flight share a chunk's fragments in L2): whole chunks
// first, then the cut ones (a panel's first chunk, the last chunk of the row), longer ones first: the short workgroups fill the last round
// instead of leaving most of the chip idle behind a few long ones
inline std::vector<int32_t> sym_worklist(int64_t ntile, int tpp, int64_t tchunk, int64_t pfirst, int64_t pstride) {
    const int64_t maxc = sym_chunks(ntile, tchunk), lpanels = sym_local_panels(ntile, tpp, pfirst, pstride);
    const auto len = [&](int64_t lp, int64_t c) {                  // tiles of workgroup (lp, c); <= 0: the panel starts right of chunk c
        return std::min((c + 1) * tchunk, ntile) - std::max(c * tchunk, tpp * (pfirst + pstride * lp));
    };
    std::vector<int32_t> list, tail;
    for (int64_t c = 0; c < maxc; ++c)
        for (int64_t lp = 0; lp < lpanels && len(lp, c) > 0; ++lp)   // panels are ascending: the rest start right of this chunk too
            (len(lp, c) == tchunk ? list : tail).push_back((int32_t)((lp << SYM_CHUNK_BITS) | c));
    std::sort(tail.begin(), tail.end(), [&](int32_t u, int32_t v) {   // longer cut chunks first
        const int64_t lu = len(u >> SYM_CHUNK_BITS, u & ((1 << SYM_CHUNK_BITS) - 1)), lv = len(v >> SYM_CHUNK_BITS, v & ((1 << SYM_CHUNK_BITS) - 1));
        return lu != lv ? lu > lv : u < v;
    });
    list.insert(list.end(), tail.begin(), tail.end());
    return list;
}

}  // namespace covgram
