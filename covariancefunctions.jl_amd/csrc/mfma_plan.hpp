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
