// mfma_plan_check.cpp — compiled (host compiler, -fsanitize=address,undefined) and run by tests/test_host.py (CPU): the properties the matrix-core
// kernels rely on in csrc/mfma_plan.hpp, the planning header of csrc/dense_mfma.hip.  Prints one line per failed property and exits non-zero.
#include <cstdio>
#include <utility>

#include "../covariancefunctions.jl_amd/csrc/mfma_plan.hpp"

using namespace covgram;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// the tiles workgroup (lp, c) walks — dense_mfma_sym_kernel: T0 = max(c tchunk, first tile of the panel), T1 = min((c + 1) tchunk, ntile)
static std::pair<int64_t, int64_t> range_of(int32_t w, int64_t ntile, int tpp, int64_t tchunk, int64_t pfirst, int64_t pstride) {
    const int64_t lp = w >> SYM_CHUNK_BITS, c = w & ((1 << SYM_CHUNK_BITS) - 1), p8 = tpp * (pfirst + pstride * lp);
    return {std::max(c * tchunk, p8), std::min((c + 1) * tchunk, ntile)};
}

static void check_worklist(int64_t ntile, int tpp, int64_t tchunk, int64_t pfirst, int64_t pstride) {
    const auto tag = [&] { static char b[128]; std::snprintf(b, sizeof b, "ntile %lld tpp %d tchunk %lld panels (%lld, %lld)", (long long)ntile, tpp, (long long)tchunk, (long long)pfirst, (long long)pstride); return b; };
    CHECK(sym_list_in_range(ntile, tpp, tchunk, pfirst, pstride), "%s", tag());
    const std::vector<int32_t> list = sym_worklist(ntile, tpp, tchunk, pfirst, pstride);
    const int64_t lpanels = sym_local_panels(ntile, tpp, pfirst, pstride), maxc = sym_chunks(ntile, tchunk);
    std::vector<unsigned char> covered((size_t)(lpanels * ntile), 0);   // [local panel][tile]: entries that walk it
    size_t walked = 0;
    bool cut_seen = false;
    int64_t last_cut = tchunk;
    for (const int32_t w : list) {
        const int64_t lp = w >> SYM_CHUNK_BITS, c = w & ((1 << SYM_CHUNK_BITS) - 1);
        CHECK(w >= 0 && lp < lpanels && lp < ((int64_t)1 << SYM_PANEL_BITS) && c < maxc && c < ((int64_t)1 << SYM_CHUNK_BITS), "%s: entry %d outside the packing", tag(), w);
        const auto r = range_of(w, ntile, tpp, tchunk, pfirst, pstride);
        const int64_t len = r.second - r.first;
        CHECK(len > 0, "%s: entry (%lld, %lld) is empty", tag(), (long long)lp, (long long)c);
        if (len == tchunk) CHECK(!cut_seen, "%s: whole chunk (%lld, %lld) behind a cut one", tag(), (long long)lp, (long long)c);
        else {
            CHECK(len <= last_cut, "%s: cut chunks not in non-increasing length (%lld after %lld)", tag(), (long long)len, (long long)last_cut);
            cut_seen = true; last_cut = len;
        }
        for (int64_t t = r.first; t < r.second && lp < lpanels; ++t, ++walked) ++covered[(size_t)(lp * ntile + t)];
    }
    // every (panel of this rank, tile >= the panel's first tile) exactly once, and nothing else
    size_t want = 0;
    for (int64_t lp = 0; lp < lpanels; ++lp)
        for (int64_t t = tpp * (pfirst + pstride * lp); t < ntile; ++t) {
            ++want;
            CHECK(covered[(size_t)(lp * ntile + t)] == 1, "%s: panel %lld tile %lld covered %d times", tag(), (long long)lp, (long long)t, (int)covered[(size_t)(lp * ntile + t)]);
        }
    CHECK(walked == want, "%s: %zu (panel, tile) pairs walked, %zu exist", tag(), walked, want);
}

static void check_columns(int64_t n, int64_t ntile, int rows, int64_t target, int64_t jsplit, bool eq) {
    const ColumnPlan pl = eq ? plan_columns(n, ntile, rows, target, jsplit, 8, 64, 2048, 16) : plan_columns(n, ntile, rows, target, jsplit, 8);
    const auto tag = [&] { static char b[160]; std::snprintf(b, sizeof b, "n %lld ntile %lld rows %d target %lld jsplit %lld eq %d -> js %lld tchunk %lld", (long long)n, (long long)ntile, rows, (long long)target, (long long)jsplit, (int)eq, (long long)pl.js, (long long)pl.tchunk); return b; };
    CHECK(pl.js >= 1 && pl.js * pl.tchunk >= ntile && ntile > (pl.js - 1) * pl.tchunk, "%s", tag());
    CHECK(pl.tchunk >= std::min<int64_t>(8, ntile), "%s", tag());
    CHECK(pl.npad % rows == 0 && pl.npad >= n && pl.npad - n < rows && pl.rowtiles * rows == pl.npad, "%s: npad %lld", tag(), (long long)pl.npad);
    if (jsplit > 0) {   // a forced split is honoured up to the 8-tile clamp (and the rounding of the chunk length to whole tiles)
        const int64_t js = std::max<int64_t>(1, std::min<int64_t>(jsplit, std::max<int64_t>(1, ntile / 8))), tchunk = (ntile + js - 1) / js;
        CHECK(pl.tchunk == tchunk && pl.js == (ntile + tchunk - 1) / tchunk && pl.js <= jsplit, "%s", tag());
    }
}

int main() {
    for (const int64_t ntile : {1, 7, 8, 9, 64, 257, 4096})
        for (const int tpp : {4, 8})
            for (const int64_t tchunk : {64, 128, 1024})
                for (const auto& ps : {std::pair<int64_t, int64_t>{0, 1}, {0, 2}, {1, 2}, {3, 8}}) check_worklist(ntile, tpp, tchunk, ps.first, ps.second);
    for (const int64_t n : {1, 31, 32, 33, 301, 4096, 65600, 1000003})
        for (const int64_t ntile : {1, 4, 7, 8, 9, 63, 64, 129, 257, 4096, 16385})
            for (const int rows : {32, 64, 128})
                for (const int64_t target : {1, 256, 8192, 131072})
                    for (const int64_t jsplit : {0, 1, 3, 4, 100, 100000})
                        for (const bool eq : {false, true}) check_columns(n, ntile, rows, target, jsplit, eq);
    std::printf(failures ? "%d properties failed\n" : "mfma_plan ok\n", failures);
    return failures ? 1 : 0;
}
