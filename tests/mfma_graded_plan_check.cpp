// mfma_graded_plan_check.cpp — compiled (host compiler, -fsanitize=address,undefined) and run by tests/test_host_graded_plan.py (CPU): the properties
// dense_mfma_eq_kernel relies on in the chunk table of csrc/mfma_plan.hpp: plan_columns_graded.  Prints one line per failed property and exits non-zero.
#include <cstdio>

#include "../covariancefunctions.jl_amd/csrc/mfma_plan.hpp"

using namespace covgram;

static int failures = 0, graded_cases = 0, uniform_cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void check_graded(int64_t n, int64_t ntile, int rows, int64_t slots, int64_t stage, int64_t floor_tiles, bool force, int64_t tail_halfrounds) {
    const ColumnPlan base = plan_columns(n, ntile, rows, 16384, 0, 8, 64, 2048, 16);     // the EQ driver's uniform plan (256 CUs x 16 x 4 waves)
    const int64_t rblocks = (base.rowtiles + stage - 1) / stage;
    const GradedPlan g = plan_columns_graded(base, ntile, rblocks, slots, stage, floor_tiles, force, tail_halfrounds);
    const auto tag = [&] { static char b[200]; std::snprintf(b, sizeof b, "n %lld ntile %lld slots %lld stage %lld floor %lld force %d tail %lld -> base js %lld tchunk %lld, js %lld", (long long)n, (long long)ntile, (long long)slots, (long long)stage, (long long)floor_tiles, (int)force, (long long)tail_halfrounds, (long long)base.js, (long long)base.tchunk, (long long)g.js); return b; };
    const bool too_small = base.js < 2 || base.tchunk / 2 / stage * stage < (floor_tiles + stage - 1) / stage * stage ||
                           (!force && (rblocks * base.js < 2 * slots || base.tchunk < floor_tiles));
    if (too_small) CHECK(!g.graded, "%s: a graded plan for a shape that is too small", tag());
    if (!g.graded) {   // the uniform plan stands
        ++uniform_cases;
        CHECK(g.js == base.js, "%s", tag());
        for (int64_t c = 0; c <= std::min<int64_t>(base.js, GRADED_MAX_CHUNKS); ++c)
            CHECK(g.start[c] == std::min(c * base.tchunk, ntile), "%s: start[%lld] = %d", tag(), (long long)c, g.start[c]);
        return;
    }
    ++graded_cases;
    const int64_t js = g.js, floor = (floor_tiles + stage - 1) / stage * stage;
    CHECK(js >= 2 && js <= GRADED_MAX_CHUNKS && js > base.js - 1, "%s", tag());
    CHECK(g.start[0] == 0 && g.start[js] == ntile, "%s: ends %d .. %d", tag(), g.start[0], g.start[js]);
    std::vector<unsigned char> covered((size_t)ntile, 0);
    int64_t body = 0, prev = base.tchunk;
    for (int64_t c = 0; c < js; ++c) {
        const int64_t len = (int64_t)g.start[c + 1] - g.start[c];
        CHECK(len > 0, "%s: chunk %lld is empty or runs backwards", tag(), (long long)c);
        if (len <= 0) return;
        for (int64_t t = g.start[c]; t < g.start[c + 1] && t < ntile; ++t) ++covered[(size_t)t];
        if (len == base.tchunk && body == c) { ++body; continue; }                      // the body keeps the uniform plan's chunk length
        CHECK(len <= prev, "%s: chunk %lld of %lld tiles after one of %lld", tag(), (long long)c, (long long)len, (long long)prev);
        CHECK(len < base.tchunk, "%s: chunk %lld behind the body is a whole one", tag(), (long long)c);
        if (c + 1 < js) {
            CHECK(len >= floor, "%s: chunk %lld of %lld tiles under the floor", tag(), (long long)c, (long long)len);
            CHECK(len % stage == 0, "%s: chunk %lld of %lld tiles is no multiple of the stage", tag(), (long long)c, (long long)len);
        }
        prev = len;
    }
    CHECK(body >= 1 && body >= base.js - base.js / 2 && body < js, "%s: body of %lld chunks", tag(), (long long)body);
    for (int64_t t = 0; t < ntile; ++t) CHECK(covered[(size_t)t] == 1, "%s: tile %lld covered %d times", tag(), (long long)t, (int)covered[(size_t)t]);
    for (int64_t c = js; c <= GRADED_MAX_CHUNKS; ++c) CHECK(g.start[c] == ntile, "%s: start[%lld] past the table's end", tag(), (long long)c);
}

int main() {
    for (const int64_t n : {1, 33, 4096, 131072, 1000003})
        for (const int64_t ntile : {1, 8, 9, 63, 64, 129, 257, 4096, 16385})
            for (const int64_t slots : {1, 512, 1024})
                for (const int64_t stage : {1, 2, 4, 8})
                    for (const int64_t floor_tiles : {4, 8, 32, 64})
                        for (const bool force : {false, true})
                            for (const int64_t tail_halfrounds : {1, 2, 4}) check_graded(n, ntile, 64, slots, stage, floor_tiles, force, tail_halfrounds);
    // the contract shape (EQ, d = 3, n = 131072: 256 row blocks of 8 waves on 512 resident slots): 6 x 512 + 2 x 256 + 2 x 128 + 4 x 64 tiles
    {
        const ColumnPlan base = plan_columns(131072, 4096, 64, 16384, 0, 8, 64, 2048, 16);
        const GradedPlan g = plan_columns_graded(base, 4096, 256, 512, 8, 64, false);
        const int32_t want[15] = {0, 512, 1024, 1536, 2048, 2560, 3072, 3328, 3584, 3712, 3840, 3904, 3968, 4032, 4096};
        CHECK(base.js == 8 && base.tchunk == 512 && g.graded && g.js == 14, "contract shape: base js %lld, graded %d js %lld", (long long)base.js, (int)g.graded, (long long)g.js);
        for (int c = 0; c < 15; ++c) CHECK(g.start[c] == want[c], "contract shape: start[%d] = %d", c, g.start[c]);
        CHECK(!plan_columns_graded(base, 4096, 256, 1100, 8, 64, false).graded, "contract shape on 1100 slots: fewer than two rounds");
        // ... and the driver's half-round tail: 7 x 512 + 256 + 128 + 2 x 64 tiles
        const GradedPlan h = plan_columns_graded(base, 4096, 256, 512, 8, 64, false, 1);
        const int32_t half[12] = {0, 512, 1024, 1536, 2048, 2560, 3072, 3584, 3840, 3968, 4032, 4096};
        CHECK(h.graded && h.js == 11, "contract shape, half-round tail: graded %d js %lld", (int)h.graded, (long long)h.js);
        for (int c = 0; c < 12; ++c) CHECK(h.start[c] == half[c], "contract shape, half-round tail: start[%d] = %d", c, h.start[c]);
    }
    CHECK(graded_cases >= 100 && uniform_cases >= 100, "%d graded and %d uniform cases", graded_cases, uniform_cases);
    if (failures) std::printf("%d properties failed\n", failures);
    else std::printf("mfma_graded_plan ok (%d graded, %d uniform cases)\n", graded_cases, uniform_cases);
    return failures ? 1 : 0;
}
