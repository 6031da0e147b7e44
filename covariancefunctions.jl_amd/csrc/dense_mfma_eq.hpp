// dense_mfma_eq.hpp — device code of the fp32 EQ matrix-core MVM (design notes: dense_mfma.hip, which alone includes this): the contract kernel
// dense_mfma_eq_kernel, its cached column fragments and per-MVM weights (mfma_pack_kernel, mfma_pack_w_kernel), and the generic kernels' packs.
#pragma once
#include "dense_mfma.hpp"

namespace covgram {

// B fragments of every column tile in MFMA lane order + the fraction factors of the column norms (both depend on the points
// and g only: cached in the points handle).  Lane (r, h) of MFMA mm of tile T holds, for coordinate c = 2 mm + h of column
// j = 32 T + r, the eight K-slots  [y1, y2, y1, y3, y2, y1, y3, y2]  (16 bytes) of y~_c, which meet the row side's
// [x1, x1, x2, x1, x2, x3, x2, x3]; the integer part k_j of -|y~_j|^2/2 sits in the idle coordinate c = d as [1, k_j, 0, ...]
// (d odd) or replaces the last two slots of coordinate 0, [.., 1, k_j] (d even) — dense_mfma.hpp: norm_split.
//   PB[(T * K2 + mm) * 64 + l] = that fragment (zero outside the point set / dimension)
//   EF[32 T + r]               = exp2(f_j) in (1/2, 1]                          (0 for padding columns)
__global__ __launch_bounds__(256) void mfma_pack_kernel(const float* __restrict__ Y, int64_t m, int32_t d, uint4* __restrict__ PB,
                                                        float* __restrict__ EF, int32_t K2, float g, const float* __restrict__ Cn, int32_t fmt) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // (tile, mm, lane)
    const int64_t ntile = (m + 31) / 32;
    if (e >= ntile * K2 * 64) return;
    const int l = (int)(e & 63);
    const int64_t q = e >> 6;
    const int mm = (int)(q % K2);
    const int64_t T = q / K2;
    const int64_t j = 32 * T + (l & 31);
    if (fmt == 1) {
        // fp16 two-way split: lane (r, h) of MFMA mm holds coordinates c0 = 4 mm + 2 h and c0 + 1 of column j as
        // [y1, y2, y1 | y1, y2, y1 | 1, k_j] — the last two slots in lane half 0 of MFMA 0 only (dense_mfma.hpp: eq_row_fragments_h)
        const int c0 = 4 * mm + 2 * (l >> 5);
        const bool nl = mm == 0 && (l >> 5) == 0;
        uint4 frag = make_uint4(0, 0, 0, 0);
        if (j < m) {
            const float ya = c0 < d ? g * (Y[j * (int64_t)d + c0] - Cn[c0]) : 0.0f;
            const float yb = c0 + 1 < d ? g * (Y[j * (int64_t)d + c0 + 1] - Cn[c0 + 1]) : 0.0f;
            unsigned a1, a2, b1, b2;
            split2h(ya, a1, a2);
            split2h(yb, b1, b2);
            frag = make_uint4(a1 | (a2 << 16), a1 | (b1 << 16), b2 | (b1 << 16), 0u);
            if (nl) {
                double ny = 0.0;
                for (int cc = 0; cc < d; ++cc) { const double yc = (double)(g * (Y[j * (int64_t)d + cc] - Cn[cc])); ny = __builtin_fma(yc, yc, ny); }
                const double hn = -0.5 * ny, k = __builtin_ceil(hn);
                frag.w = F16_ONE | (f16_bits((float)k) << 16);
                EF[j] = __builtin_amdgcn_exp2f((float)(hn - k));
            }
        } else if (nl) {
            EF[j] = 0.0f;
        }
        PB[e] = frag;
        return;
    }
    const int c = 2 * mm + (l >> 5);
    uint4 frag = make_uint4(0, 0, 0, 0);
    const bool norm_lane = (d & 1) ? (c == d) : (c == 0);          // the lane that carries k_j (one per column)
    if (j < m) {
        if (c < d) {
            const float yt = g * (Y[j * (int64_t)d + c] - Cn[c]);
            unsigned y1, y2, y3;
            split3(yt, y1, y2, y3);
            frag = make_uint4(y1 | (y2 << 16), y1 | (y3 << 16), y2 | (y1 << 16), y3 | (y2 << 16));
        }
        if (norm_lane) {
            double ny = 0.0;
            for (int cc = 0; cc < d; ++cc) { const double yc = (double)(g * (Y[j * (int64_t)d + cc] - Cn[cc])); ny = __builtin_fma(yc, yc, ny); }
            const NormSplit sp = norm_split(ny);
            if (d & 1) frag = make_uint4(BF16_ONE | (sp.kbits << 16), 0, 0, 0);
            else frag.w = BF16_ONE | (sp.kbits << 16);
            EF[j] = sp.ef;
        }
    } else if (norm_lane) {
        EF[j] = 0.0f;
    }
    PB[e] = frag;
}

// the per-MVM part of the pack: W[j] = a_j * exp2(f_j) (the cached fraction factor, in (1/2, 1]), 0 for padding columns
__global__ __launch_bounds__(256) void mfma_pack_w_kernel(const float* __restrict__ A, const float* __restrict__ EF, float* __restrict__ W,
                                                          int64_t m, int64_t mpad) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < mpad) W[j] = j < m ? A[j] * EF[j] : 0.0f;
}

// LDS: 0 = every wave loads its own column tiles; 1 = stages of WPB tiles shared through LDS (K2 <= 4, RT = 2);
//      2 = ONE tile per stage, its K2 fragment slices fetched by the WPB waves in turn (K2 > 4, RT = 1)
// STAMP = 1: the diagnostic build of the SAME loop that reads the shader clock (s_memtime) and the constant 100 MHz counter
// (s_memrealtime) around the column loop of every workgroup — clock = d(memtime) / d(memrealtime) x 100 MHz (MI355X_MICROARCH.md,
// DVFS give-back item 6).  The stamps go to a buffer of their own; no product launch ever runs this instantiation.
template <int K2, int RT, int WPB = 1, int LDS = 0, int STAMP = 0, int FMT = 0>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(LDS == 1 ? (RT == 4 ? 2 : K2 <= 2 ? 4 : 3) : 1, LDS == 1 ? (RT == 4 ? 2 : K2 <= 2 ? 4 : 3) : 8))) void dense_mfma_eq_kernel(const float* __restrict__ X, int64_t n, int32_t d,
                                                           const uint4* __restrict__ PB, const float* __restrict__ W, int64_t ntile,
                                                           float* __restrict__ out, int64_t npad, int64_t tchunk, float g,
                                                           float alpha, float beta, int32_t final_store, const float* __restrict__ Cn,
                                                           unsigned long long* __restrict__ stamps, unsigned* __restrict__ tickets,
                                                           float* __restrict__ yfinal, const float* __restrict__ EF, int64_t mcols,
                                                           const ChunkTable chunks) {
    // WPB waves per workgroup take consecutive row tiles and walk the SAME column tiles at the same pace (no barrier,
    // nothing shared explicitly): their fragment loads coalesce in the CU's vector L1 instead of each going to L2
    const int l = threadIdx.x & 63, t = l & 31, h = l >> 5;
    const int64_t i0 = ((int64_t)blockIdx.x * WPB + (threadIdx.x >> 6)) * (32 * RT);
    // A fragments: lane (t, h) holds the split of x~[row][c = 2 mm + h] (+ the integer part of the row's half-norm)
    Frag a[RT][K2];
    float er[RT];                                                // exp2 of the fraction of the row's half-norm, in (1/2, 1]
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        int64_t row = i0 + 32 * r + t;
        if (row >= n) row = n - 1;                               // clamp: computed, never stored
        er[r] = eq_row_fragments_fmt<K2, FMT>(X + row * (int64_t)d, Cn, d, g, h, a[r]);
    }

    unsigned long long st_c0 = 0, st_r0 = 0;
    if constexpr (STAMP) { st_c0 = __builtin_amdgcn_s_memtime(); st_r0 = __builtin_amdgcn_s_memrealtime(); }
    // this workgroup's column tiles [T0, T1): equal steps of tchunk, or the boundaries of a graded split (chunks.n > 0: shorter chunks towards the end of
    // the grid, mfma_plan.hpp) — two scalar loads from the kernel arguments
    int64_t T0 = (int64_t)blockIdx.y * tchunk;
    int64_t T1 = (T0 + tchunk < ntile) ? (T0 + tchunk) : ntile;
    if (chunks.n > 0) { T0 = chunks.start[blockIdx.y]; T1 = chunks.start[blockIdx.y + 1]; }
    // the accumulators live as register PAIRS: with one or two MFMAs per tile the weighted sums are v_pk_fma_f32 (two fmas per instruction — nearly twice
    // the rate while no MFMA executes, slower than two v_fma_f32 beside one: tools/pkfma_probe.hip; C2-shaped 1.44 -> 1.33 ms, four MFMAs per tile +2-3 %)
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 acc2[RT][8];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int v = 0; v < 8; ++v) acc2[r][v] = (f32x2){0.0f, 0.0f};

    // Column tiles in pairs with two operand buffers (no register copies); the prefetch of a tile past the chunk is clamped
    // to the last tile (a harmless re-read) instead of branching.  Uniform base + 32-bit lane offset -> saddr loads.
    const uint4* __restrict__ pbase = PB + (T0 * K2) * 64;
    // column weights w_j = a_j exp2(f_j) (0 for padding columns).  EF != nullptr (round 4): W is the caller's a itself and the product with the cached
    // fraction factors is formed here, where a tile's weights are fetched: no weight-pack launch in front of the MVM (mvm_eq_mfma)
    const float* __restrict__ wbase = W + T0 * 32;
    const int nt = (int)(T1 - T0);
    auto weight = [&](int tc) {
        if (EF == nullptr) return wbase[tc * 32 + t];
        const int64_t j = (T0 + tc) * 32 + t;
        return j < mcols ? W[j] * EF[j] : 0.0f;
    };
    auto load_tile = [&](int ti, Frag (&f)[K2], float& w) {
        const int tc = ti < nt ? ti : nt - 1;
#pragma unroll
        for (int mm = 0; mm < K2; ++mm) f[mm].u = pbase[(tc * K2 + mm) * 64 + l];
        w = weight(tc);
    };
    auto process = [&](const Frag (&f)[K2], float w) {
        f32x16 D[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            D[r] = (f32x16){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int mm = 0; mm < K2; ++mm) D[r] = eq_mma<FMT>(a[r][mm], f[mm], D[r]);
        }
        // all exponentials of the tile first, then the weighted accumulation: no exp -> fma wait states in between
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int v = 0; v < 16; ++v) D[r][v] = __builtin_amdgcn_exp2f(D[r][v]);
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                if constexpr (K2 <= 2) acc2[r][v] = __builtin_elementwise_fma((f32x2){w, w}, (f32x2){D[r][2 * v], D[r][2 * v + 1]}, acc2[r][v]);
                else { acc2[r][v][0] = __builtin_fmaf(w, D[r][2 * v], acc2[r][v][0]); acc2[r][v][1] = __builtin_fmaf(w, D[r][2 * v + 1], acc2[r][v][1]); }
            }
    };
    if constexpr (LDS == 2) {
        // Long fragments (K2 KB per tile): the workgroup stages ONE tile at a time, wave w fetching the fragment slices
        // mm = w, w + WPB, ... of the NEXT tile (global_load_lds_dwordx4) while all waves stream the CURRENT tile's slices
        // from the other buffer into their MFMA chain; one barrier per tile (a tile is >= 32 K2 matrix-pipe cycles).
        static_assert(RT == 1, "split-tile staging is built for one row tile per wave");
        __shared__ uint4 tfA[K2][64], tfB[K2][64];
        __shared__ float twA[32], twB[32];
        typedef __attribute__((address_space(1))) const void* gptr_t;
        typedef __attribute__((address_space(3))) void* lptr_t;
        const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        // (gw, ge): loaded with the tile's LDS-DMA, multiplied only where the weight is stored after the tile's arithmetic (as in the LDS == 1 form
        // below; round 5: here the product sat right behind the loads — one exposed memory round trip per TILE for wave 0, and the barrier passes it on)
        float gw = 0.0f, ge = 1.0f;
#define CG_DMA2(tile, TF)                                                                       \
        {                                                                                       \
            const int ti_ = (tile);                                                             \
            const int tc_ = ti_ < nt ? ti_ : nt - 1;                                            \
            _Pragma("unroll") for (int q = 0; q < (K2 + WPB - 1) / WPB; ++q) {                  \
                const int mm = wv + q * WPB;                                                    \
                if (mm < K2) __builtin_amdgcn_global_load_lds((gptr_t)(pbase + (tc_ * K2 + mm) * 64 + l), (lptr_t)&TF[mm][0], 16, 0, 0); \
            }                                                                                   \
            if (wv == 0) {                                                                      \
                if (EF == nullptr) gw = ti_ < nt ? wbase[tc_ * 32 + t] : 0.0f;                  \
                else {                                                                          \
                    const int64_t j_ = (T0 + tc_) * 32 + t;                                     \
                    const bool in_ = ti_ < nt && j_ < mcols;                                    \
                    gw = in_ ? W[j_] : 0.0f; ge = in_ ? EF[j_] : 0.0f;                          \
                }                                                                               \
            }                                                                                   \
        }
#define CG_TILE2(TF, TW)                                                                        \
        {                                                                                       \
            f32x16 D = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};                        \
            Frag f_[K2];                                                                        \
            _Pragma("unroll") for (int mm = 0; mm < K2; ++mm) f_[mm].u = TF[mm][l];             \
            const float w = TW[t];                                                              \
            _Pragma("unroll") for (int mm = 0; mm < K2; ++mm) D = eq_mma<FMT>(a[0][mm], f_[mm], D); \
            _Pragma("unroll") for (int v = 0; v < 16; ++v) D[v] = __builtin_amdgcn_exp2f(D[v]); \
            _Pragma("unroll") for (int v = 0; v < 8; ++v) { acc2[0][v][0] = __builtin_fmaf(w, D[2 * v], acc2[0][v][0]); acc2[0][v][1] = __builtin_fmaf(w, D[2 * v + 1], acc2[0][v][1]); } \
        }
        CG_DMA2(0, tfA)
        if (wv == 0 && h == 0) twA[t] = gw * ge;
        __syncthreads();
        for (int ti = 0; ti < nt; ti += 2) {
            CG_DMA2(ti + 1, tfB)                                    // past the chunk: a re-fetch nobody reads
            CG_TILE2(tfA, twA)
            if (wv == 0 && h == 0) twB[t] = gw * ge;
            __syncthreads();
            if (ti + 1 >= nt) break;
            CG_DMA2(ti + 2, tfA)
            CG_TILE2(tfB, twB)
            if (wv == 0 && h == 0) twA[t] = gw * ge;
            __syncthreads();
        }
#undef CG_DMA2
#undef CG_TILE2
    } else if constexpr (LDS == 1) {
        // The WPB waves of the workgroup walk the same column tiles: each stage of WPB tiles is fetched ONCE — wave w moves
        // tile w of the NEXT stage straight from global memory into LDS (global_load_lds_dwordx4: no staging registers; lane
        // order in LDS = lane order of the packed fragments) while the current stage is read by all waves from the other
        // buffer — which cuts the L2 -> L1 fragment traffic by WPB.  Two buffers as two distinct arrays (the compiler's
        // LDS-DMA wait tracking tells them apart), the stage loop unrolled by two, one barrier per stage.
        __shared__ uint4 sfA[WPB][K2][64], sfB[WPB][K2][64];
        __shared__ float swA[WPB][32], swB[WPB][32];
        typedef __attribute__((address_space(1))) const void* gptr_t;
        typedef __attribute__((address_space(3))) void* lptr_t;
        const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int nstage = (nt + WPB - 1) / WPB;
        // (gw, ge): the weight's two factors a_j and exp2(f_j) when the kernel forms the product itself (EF != nullptr) — loaded here, multiplied
        // only where the weight goes to LDS at the end of the stage: a product right behind the loads would hold this wave until the LDS-DMA
        // it has just issued lands (the same counter); ge = 1 when W holds packed weights
        float gw, ge = 1.0f;
#define CG_DMA(stage, SF)                                                                       \
        {                                                                                       \
            const int ti_ = (stage) * WPB + wv;                                                 \
            const int tc_ = ti_ < nt ? ti_ : nt - 1;                                            \
            _Pragma("unroll") for (int mm = 0; mm < K2; ++mm)                                   \
                __builtin_amdgcn_global_load_lds((gptr_t)(pbase + (tc_ * K2 + mm) * 64 + l), (lptr_t)&SF[wv][mm][0], 16, 0, 0); \
            if (EF == nullptr) gw = ti_ < nt ? wbase[tc_ * 32 + t] : 0.0f;   /* tiles past the chunk: weight 0 */ \
            else {                                                                              \
                const int64_t j_ = (T0 + tc_) * 32 + t;                                         \
                const bool in_ = ti_ < nt && j_ < mcols;                                        \
                gw = in_ ? W[j_] : 0.0f; ge = in_ ? EF[j_] : 0.0f;                              \
            }                                                                                   \
        }
#define CG_STAGE(SF, SW)                                                                        \
        _Pragma("unroll 1") for (int k = 0; k < WPB; k += 2) {                                  \
            Frag f0[K2], f1[K2];                                                                \
            _Pragma("unroll") for (int mm = 0; mm < K2; ++mm) f0[mm].u = SF[k][mm][l];          \
            const float w0 = SW[k][t];                                                          \
            _Pragma("unroll") for (int mm = 0; mm < K2; ++mm) f1[mm].u = SF[k + 1][mm][l];      \
            const float w1 = SW[k + 1][t];                                                      \
            process(f0, w0);                                                                    \
            process(f1, w1);                                                                    \
        }
        CG_DMA(0, sfA)
        if (h == 0) swA[wv][t] = gw * ge;
        __syncthreads();
        for (int st = 0; st < nstage; st += 2) {
            CG_DMA(st + 1 < nstage ? st + 1 : st, sfB)              // past the last stage: a re-fetch nobody reads
            CG_STAGE(sfA, swA)
            if (h == 0) swB[wv][t] = gw * ge;
            __syncthreads();
            if (st + 1 >= nstage) break;
            CG_DMA(st + 2 < nstage ? st + 2 : st + 1, sfA)
            CG_STAGE(sfB, swB)
            if (h == 0) swA[wv][t] = gw * ge;
            __syncthreads();
        }
#undef CG_DMA
#undef CG_STAGE
    } else {
    Frag f0[K2], f1[K2];
    float w0, w1;
    load_tile(0, f0, w0);
    for (int ti = 0; ti < nt; ti += 2) {
        load_tile(ti + 1, f1, w1);
        process(f0, w0);
        load_tile(ti + 2, f0, w0);
        if (ti + 1 < nt) process(f1, w1);
    }
    }

    if constexpr (STAMP) {
        const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x == 0) {
            unsigned long long* o = stamps + 4 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
            o[0] = st_c0; o[1] = st_r0; o[2] = c1; o[3] = r1;
        }
    }
    // lane (t, h) owns output row t of each row tile iff bit 2 of t equals h; its register is v = (t & 3) + 4 (t >> 3)
    const int vsel = (t & 3) + 4 * (t >> 3);
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        // sum over the 32 column lanes of each half: afterwards every lane of half h holds the totals of rows i(v, h)
        float tot = 0.0f;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            float s = acc2[r][v >> 1][v & 1];
            s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8); s += __shfl_xor(s, 16);
            tot = (vsel == v) ? s : tot;
        }
        const int64_t i = i0 + 32 * r + t;
        if (((t >> 2) & 1) != h || i >= n) continue;
        const float res = er[r] * tot;
        if (final_store) {
            float v = alpha * res;
            if (beta != 0.0f) v = __builtin_fmaf(beta, out[i], v);
            out[i] = v;
        } else {
            slab_store(out + (int64_t)blockIdx.y * npad + i, res, tickets != nullptr);
        }
    }
    // column split with tickets: the LAST workgroup of this row block to arrive adds the block's partials in dense_reduce_kernel's
    // order and applies alpha / beta (pack.hpp: last_arrival) — no reduce launch, no dependent-launch gap behind the kernel
    if (!final_store && tickets != nullptr) {
        if (!last_arrival(tickets + blockIdx.x, gridDim.y)) return;
        const int64_t r0 = (int64_t)blockIdx.x * (WPB * 32 * RT);
        for (int idx = threadIdx.x; idx < WPB * 32 * RT; idx += 64 * WPB) {
            const int64_t i = r0 + idx;
            if (i >= n) continue;
            float v = alpha * ordered_split_sum<float>(out + i, npad, (int)gridDim.y);
            if (beta != 0.0f) v = __builtin_fmaf(beta, yfinal[i], v);
            yfinal[i] = v;
        }
    }
}

// Column tiles for the generic kernel.  Lane (r, h) of MFMA mm of tile T holds coordinate c = 2 mm + h of column
// j = 32 T + r:  c < d: the split of (iso ? -2 g y_c : g y_c) as [y1, y2, y1, y3, y2, y1, y3, y2];  c == d (iso): the norm
// slots [1, 1, 1, n1, n2, n3, 0, 0] with n = |g y|^2;  beyond: zeros.   W[(T * NR + c) * 32 + r] = A[j + c lda].
__global__ __launch_bounds__(256) void mfma_pack_gen_kernel(const float* __restrict__ Y, int64_t m, int32_t d, const float* __restrict__ A,
                                                            int64_t lda, int32_t nrhs, int32_t c0, uint4* __restrict__ PB,
                                                            float* __restrict__ W, int32_t K2, int32_t NR, float g, int32_t iso,
                                                            const float* __restrict__ Cn, int32_t fmt) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // (tile, mm, lane)
    const int64_t ntile = (m + 31) / 32;
    if (e >= ntile * K2 * 64) return;
    const int l = (int)(e & 63);
    const int64_t q = e >> 6;
    const int mm = (int)(q % K2);
    const int64_t T = q / K2;
    const int64_t j = 32 * T + (l & 31);
    const int c = 2 * mm + (l >> 5);
    uint4 frag = make_uint4(0, 0, 0, 0);
    if (fmt == 1) {
        // fp16 two-way split (dense_mfma.hpp: gen_row_fragments, GFMT = 1): positions q0 = 4 mm + 2 h and q0 + 1, three slots each — a coordinate
        // [y1, y2, y1] of -2 g (y - c), the row norm's position d as [1, 1, 1], the column norm at d + 1 as [k, f1, f2]
        if (j < m) {
            float ny = 0.0f;
            for (int cc = 0; cc < d; ++cc) { const float yc = g * (Y[j * (int64_t)d + cc] - Cn[cc]); ny = __builtin_fmaf(yc, yc, ny); }
            unsigned sl[6] = {0, 0, 0, 0, 0, 0};
            for (int w = 0; w < 2; ++w) {
                const int qq = 4 * mm + 2 * (l >> 5) + w;
                if (qq < d) { unsigned y1, y2; split2h(-2.0f * (g * (Y[j * (int64_t)d + qq] - Cn[qq])), y1, y2); sl[3 * w] = y1; sl[3 * w + 1] = y2; sl[3 * w + 2] = y1; }
                else if (qq == d) { sl[3 * w] = sl[3 * w + 1] = sl[3 * w + 2] = F16_ONE; }
                else if (qq == d + 1) { const Norm16 nn = norm16(ny); sl[3 * w] = nn.k; sl[3 * w + 1] = nn.f1; sl[3 * w + 2] = nn.f2; }
            }
            frag = make_uint4(sl[0] | (sl[1] << 16), sl[2] | (sl[3] << 16), sl[4] | (sl[5] << 16), 0u);
        }
    } else
    if (j < m) {
        if (c < d) {
            const float yt = iso ? -2.0f * (g * (Y[j * (int64_t)d + c] - Cn[c])) : g * Y[j * (int64_t)d + c];
            unsigned y1, y2, y3;
            split3(yt, y1, y2, y3);
            frag = make_uint4(y1 | (y2 << 16), y1 | (y3 << 16), y2 | (y1 << 16), y3 | (y2 << 16));
        } else if (iso && c == d) {
            float ny = 0.0f;
            for (int cc = 0; cc < d; ++cc) { const float yc = g * (Y[j * (int64_t)d + cc] - Cn[cc]); ny = __builtin_fmaf(yc, yc, ny); }
            unsigned n1, n2, n3;
            split3(ny, n1, n2, n3);
            frag = make_uint4(BF16_ONE | (BF16_ONE << 16), BF16_ONE | (n1 << 16), n2 | (n3 << 16), 0);
        }
    }
    PB[e] = frag;
    if (mm == 0 && l < 32)
        for (int cr = 0; cr < NR; ++cr) W[(T * NR + cr) * 32 + l] = (j < m && c0 + cr < nrhs) ? A[j + (int64_t)(c0 + cr) * lda] : 0.0f;
}

// A operands of dense_mfma_mrhs_kernel: AP[((T * NB + b) * 64 + l) * 16 + v] = a[j][c0 + 32 b + (l & 31)] with
// j = 32 T + 8 (v / 4) + 4 (l >> 5) + v % 4 (zero outside the matrix): lane l's sixteen values of one tile are contiguous
__global__ __launch_bounds__(256) void mfma_pack_rhs_kernel(const float* __restrict__ A, int64_t lda, int32_t nrhs, int32_t c0, int64_t m,
                                                            float* __restrict__ AP, int32_t NB) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // (tile, block, lane, v)
    const int64_t ntile = (m + 31) / 32;
    if (e >= ntile * NB * 64 * 16) return;
    const int v = (int)(e & 15), l = (int)((e >> 4) & 63);
    const int64_t q = e >> 10;
    const int b = (int)(q % NB);
    const int64_t T = q / NB;
    const int64_t j = 32 * T + 8 * (v >> 2) + 4 * (l >> 5) + (v & 3);
    const int c = c0 + 32 * b + (l & 31);
    AP[e] = (j < m && c < nrhs) ? A[j + (int64_t)c * lda] : 0.0f;
}

}  // namespace covgram
