// dense_mfma.hip — the fp32 ExponentiatedQuadratic Gramian MVM on the matrix cores.
//
// The lane-per-row kernel of dense_mvm.hpp spends 23 issue cycles per 64 pairs, two thirds of them on the distance
// (3 d packed VALU ops per column pair): it sits on the VALU issue ceiling.  For the EQ profile the
// distance can leave the VALU altogether:
//     exp(-|x-y|^2 / (2 l^2)) = exp2(-|x~|^2/2) * exp2(x~ . y~) * exp2(-|y~|^2/2),      x~ = sqrt(log2 e) x / l
// so that   b_i = alpha * e_i * sum_j w_j exp2(x~_i . y~_j),   e_i = exp2(-|x~_i|^2/2),  w_j = a_j exp2(-|y~_j|^2/2):
// a 32 x 32 GEMM tile per wave and 32 rows, then ONE v_exp_f32 and ONE v_fma_f32 per pair.
//
// Which MFMA.  v_mfma_f32_32x32x2_f32 is exact but shares the fp32 FMA datapath with the VALU: measured on C2 it added
// its full 64 cycles per instruction to the VALU time (2.66 ms, no gain; profiles/r01_mfma_eq_variants.txt).  The bf16
// matrix pipe does run beside the VALU (it holds vector issue for 8 of its 32 cycles), so the fp32 dot product is
// rebuilt on it from a three-way bf16 split of every coordinate, x~ = x1 + x2 + x3 (8 + 8 + 8 mantissa bits, bf16 keeps
// the fp32 exponent range): the eight products x1y1, x1y2, x2y1, x1y3, x2y2, x3y1, x2y3, x3y2 (everything down to
// 2^-24 |x~||y~|; only x3y3 ~ 2^-32 is dropped) are exact in the fp32 accumulator, and they fill exactly the 8 K-slots a
// lane owns in v_mfma_f32_32x32x16_bf16: one MFMA covers two coordinates (lane half h takes coordinate 2 mm + h).
//
// Which split (round 4).  Inside g^2 R^2 <= MFMA_F16_GATE (72) the coordinates are split into TWO fp16 pieces instead, x~ = h1 + h2, and only the
// three products h1 h1, h1 h2, h2 h1 are formed (v_mfma_f32_32x32x16_f16; a lane's 8 K-slots hold two coordinates + the norm slots, so one MFMA
// covers FOUR coordinates): what is dropped is ~2^-22 |x~_c y~_c| per coordinate — one fp32 rounding of the dot product, which the accumulator
// commits anyway — and the matrix-core work per pair halves.  The d = 5 ... 8 kernels were power-bound (2.0 GHz under them), so that is fewer cycles
// AND a higher clock: mvm_eq_mfma below ("Which split") has the measurements and the gate; everything after the MFMA is the same for both splits.
//
// Tile orientation: D = X~tile (32 rows i) * Y~tile^T (32 columns j).  A lane holds column j = lane & 31 and the 16 rows
// i = (v & 3) + 8 (v >> 2) + 4 (lane >> 5) of the result, so the column weight w_j is ONE per-lane register per tile and
// the 16 accumulators of a lane collect "row i, columns == lane (mod 32)" over all column tiles; the sum over the 32
// lanes happens once per wave, at the end (5 butterfly steps).  RT row tiles per wave share every B fragment.
//
// Numerics.  This is NOT the reference's direct-difference r^2 (src/util.jl:40-47): the exponent
//     x~ . y~ - |x~|^2/2 - |y~|^2/2  =  -|x~ - y~|^2 / 2
// is formed in the MFMA's fp32 accumulator from the split products plus the INTEGER parts of the two half-norms (two extra
// K-slots); their fractions are fp32 factors in (1/2, 1] (dense_mfma.hpp: norm_split) — so every exponential is <= 4: it can
// neither overflow nor lose a row or a column to an underflowing norm factor (round 1 kept e_i = exp2(-|x~_i|^2/2) and
// a_j e_j whole, which flushed every row of an X cluster > ~16 scaled units from the column centre to 0), and the weights
// stay within a factor 2 of the caller's a_j.  What remains is the cancellation: the partial sums reach max(|x~|^2, |y~|^2),
// so the exponent carries an absolute error of a few fp32 roundings of that size.  The path is therefore taken only when BOTH
// point sets lie within
//     g^2 max_i |x_i - c|^2 <= MFMA_GATE  and  g^2 max_j |y_j - c|^2 <= MFMA_GATE      (c = the column side's centre)
// (= 126: measured contribution to the MVM's relative error ~4e-9 per unit of the bound, i.e. <= 5e-7 against the 1e-5
// fp32 tolerance of BASELINE.json; common.hpp) — the radii are computed once when the covgram_points handle is created —
// and otherwise the exact direct-difference kernel runs.
// Option "dense_variant": 0 = this rule, 1 = always direct differences, 2 = MFMA whenever the shape allows (tests).
//
//
// This file is the HOST side of the matrix-core paths; the kernels live in headers (one path each, chosen on the host in covgram_mvm):
//   dense_mfma_eq.hpp  dense_mfma_eq_kernel<K2, RT, WPB, LDS>: EQ, any X / Y.  LDS = 0: one wave per workgroup with its own fragment loads; LDS = 1 (d <= 8) /
//                      2 (d > 8): four waves share the column tiles through LDS (global_load_lds DMA, double buffered) when the column chunks are long; the pack kernels
//   dense_mfma.hpp     dense_mfma_gen_kernel<FAM, ...>: RQ, Cauchy, IMQ, MaternP, Dot^p, ExponentialDot, EQ^p, several right-hand sides (the MFMA yields the profile
//                      argument s); dense_mfma_sym_kernel / _sym_wide_kernel / _sym2_kernel (dense_mfma_sym2.hpp): gramian(k, x), the upper triangle once, row AND
//                      column sums ("Symmetric Gramian" below), also rank r of P's share for the multi-GPU form; the launchers, one argument list per kernel family
//   mfma_plan.hpp      the column split and the symmetric work list as plain arithmetic (no HIP; tests/mfma_plan_check.cpp)
// Sections: the points handle's radii (device code: their reduction kernel) | the rules, each written once | shared steps | the three drivers.
#include "dense_driver.hpp"
#include "mfma_plan.hpp"
#include "dense_mfma_eq.hpp"

namespace covgram {
static_assert(GRADED_MAX_CHUNKS == MFMA_MAX_CHUNKS, "the planner's table and the kernel argument hold the same number of chunks");

// ---- The points handle's radii: max |x|^2 and max |x - c|^2 about a sampled centre, computed once at handle creation (covgram_points_create, --------------------
// api.hip), and the gate quantity the rules below derive from them
// max_i |x_i|^2 of a point set (fp32 or fp64 points), via atomicMax on the bit pattern of a non-negative float
// DL > 1 (d == DL, a power of two 8 .. 64): DL lanes share a point, one coordinate each — consecutive lanes read consecutive memory (round 5: a thread per
// point put every lane of a load on its own cache line once rows were long: 373 us for n = 2^20, d = 32 fp64 at handle creation)
template <typename T, int DL = 1>
__global__ __launch_bounds__(256) void max_norm2_kernel(const T* __restrict__ X, int64_t n, int32_t d, unsigned* __restrict__ outbits,
                                                        const T* __restrict__ Cn) {
    // outbits[0]: max |x_i|^2 (dot-product kernels), outbits[1]: max |x_i - c|^2 (isotropic kernels, c = the handle's centre)
    float v = 0.0f, vc = 0.0f;
    const int64_t g0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gs = (int64_t)gridDim.x * blockDim.x;
    const int cl = (int)(g0 % DL);                               // (DL divides the block: a lane keeps its coordinate across the stride)
    for (int64_t i = g0 / DL; i < (n + 63) / 64 * 64; i += gs / DL) {   // grid-stride; whole waves stay in the loop for the shuffles below
        double s = 0, sc = 0;
        if constexpr (DL == 1) {
            if (i >= n) continue;
            for (int c = 0; c < d; ++c) {
                const double xc = (double)X[i * (int64_t)d + c], xd = xc - (double)Cn[c];
                s += xc * xc; sc += xd * xd;
            }
        } else {
            if (i < n) { const double xc = (double)X[i * (int64_t)DL + cl], xd = xc - (double)Cn[cl]; s = xc * xc; sc = xd * xd; }
#pragma unroll
            for (int o = DL / 2; o > 0; o >>= 1) { s += __shfl_xor(s, o); sc += __shfl_xor(sc, o); }
        }
        float f = (float)s, fc = (float)sc;
        if (!(f >= 0.0f)) f = __builtin_inff();                  // NaN / overflow: never eligible
        if (!(fc >= 0.0f)) fc = __builtin_inff();
        v = fmaxf(v, f * 1.000001f);                             // round up: the bound must not under-estimate
        vc = fmaxf(vc, fc * 1.000001f);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { v = fmaxf(v, __shfl_xor(v, o)); vc = fmaxf(vc, __shfl_xor(vc, o)); }
    __shared__ float wmax[4], wcmax[4];
    if ((threadIdx.x & 63) == 0) { wmax[threadIdx.x >> 6] = v; wcmax[threadIdx.x >> 6] = vc; }
    __syncthreads();
    if (threadIdx.x == 0) {                                      // one pair of atomics per workgroup
        atomicMax(outbits, __float_as_uint(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))));
        atomicMax(outbits + 1, __float_as_uint(fmaxf(fmaxf(wcmax[0], wcmax[1]), fmaxf(wcmax[2], wcmax[3]))));
    }
}

int points_max_norm2(covgram_points* p) {
    p->max_norm2 = 0.0; p->max_cnorm2 = 0.0;
    p->center = nullptr; p->center_host.assign((size_t)p->d, 0.0);
    if (p->n == 0) return COVGRAM_OK;
    // The centre: the mean of up to 1024 evenly spaced points (one strided 2-D copy, averaged on the host, written to a small
    // device buffer the handle owns).  ANY common point keeps the isotropic kernels exact; one near the middle of the cloud also
    // keeps max |x - c| — and with it the matrix-core gate and the rounding of the pre-scaled coordinates — as small as the
    // cloud allows (C3: the first point sat 2.8 from the middle of a cloud of radius 6.5 and pushed the gate value to 127).
    const size_t ts = dtype_size(p->dtype);
    const int64_t ns = std::min<int64_t>(p->n, 1024), stride = p->n / ns;
    std::vector<char> samp((size_t)ns * p->d * ts);
    hipStream_t st = p->ctx->stream;
    hipError_t e = hipMemcpy2DAsync(samp.data(), (size_t)p->d * ts, p->dptr, (size_t)stride * p->d * ts, (size_t)p->d * ts, (size_t)ns,
                                    hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { set_error("centre sample copy failed: %s", hipGetErrorString(e)); return COVGRAM_EHIP; }
    std::vector<char> cdev((size_t)p->d * ts);
    for (int c = 0; c < p->d; ++c) {
        double s = 0;
        for (int64_t i = 0; i < ns; ++i)
            s += p->dtype == COVGRAM_F32 ? (double)((const float*)samp.data())[i * p->d + c] : ((const double*)samp.data())[i * p->d + c];
        s /= (double)ns;
        if (!(s - s == 0.0)) s = 0.0;                            // NaN / inf in the sample: that coordinate is not centred
        if (p->dtype == COVGRAM_F32) { ((float*)cdev.data())[c] = (float)s; p->center_host[c] = (double)(float)s; }
        else { ((double*)cdev.data())[c] = s; p->center_host[c] = s; }
    }
    e = hipMalloc(&p->center_buf, cdev.size());
    if (e != hipSuccess) { p->center_buf = nullptr; set_error("hipMalloc(%zu) failed: %s", cdev.size(), hipGetErrorString(e)); return COVGRAM_ENOMEM; }
    p->center = p->center_buf;
    p->owns_center = true;
    unsigned* dbits = nullptr;
    e = hipMemcpyAsync(p->center_buf, cdev.data(), cdev.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);           // cdev is a local
    if (e == hipSuccess) e = hipMalloc(&dbits, 2 * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemsetAsync(dbits, 0, 2 * sizeof(unsigned), st);
    if (e == hipSuccess) {
        const unsigned grid = (unsigned)std::min<int64_t>((p->n + 255) / 256, 2048);
#define CG_MN(TT, DLV) hipLaunchKernelGGL((max_norm2_kernel<TT, DLV>), dim3((unsigned)std::min<int64_t>((p->n * DLV + 255) / 256, 512)), dim3(256), 0, st, (const TT*)p->dptr, p->n, p->d, dbits, (const TT*)p->center)
#define CG_MND(TT) do { const bool big = p->n * (int64_t)p->d >= ((int64_t)1 << 22);   /* (small sets: the thread-per-point form's 64 atomics beat 512) */ \
                        if (big && p->d == 8) CG_MN(TT, 8); else if (big && p->d == 16) CG_MN(TT, 16); else if (big && p->d == 32) CG_MN(TT, 32); else if (big && p->d == 64) CG_MN(TT, 64); \
                        else hipLaunchKernelGGL((max_norm2_kernel<TT, 1>), dim3(grid), dim3(256), 0, st, (const TT*)p->dptr, p->n, p->d, dbits, (const TT*)p->center); } while (0)
        if (p->dtype == COVGRAM_F32) CG_MND(float); else CG_MND(double);
#undef CG_MND
#undef CG_MN
        e = hipGetLastError();
    }
    unsigned bits[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(bits, dbits, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (dbits) (void)hipFree(dbits);
    if (e != hipSuccess) {
        (void)hipFree(p->center_buf); p->center_buf = nullptr; p->center = nullptr; p->owns_center = false;
        set_error("max-norm reduction failed: %s", hipGetErrorString(e)); return COVGRAM_EHIP;
    }
    float f[2];
    memcpy(f, bits, sizeof(f));
    p->max_norm2 = (double)f[0];
    p->max_cnorm2 = (double)f[1];
    return COVGRAM_OK;
}

// bound on max_i |x_i - c_Y| from the per-handle quantities: |x - c_Y| <= |x - c_X| + |c_X - c_Y|
static double centred_radius(const covgram_points* X, const covgram_points* Y) {
    double s = 0;
    for (int c = 0; c < X->d; ++c) { const double t = X->center_host[c] - Y->center_host[c]; s += t * t; }
    if (!(s >= 0)) return INFINITY;
    return sqrt(X->max_cnorm2) + sqrt(s) * 1.000001;
}

// the larger of the two squared radii about the column side's centre: every partial sum of the cancellation
// |x~|^2 + |y~|^2 - 2 x~.y~ (and of the EQ exponent) is bounded by it, so the absolute rounding error of s scales with it
double gate_radius2(const covgram_points* X, const covgram_points* Y) {
    const double rx = centred_radius(X, Y), ry = sqrt(Y->max_cnorm2);
    const double r = rx > ry ? rx : ry;
    return r * r;
}

// ---- Rules: which kernel serves a call.  Each is written once; covgram_mvm (api.hip) and the drivers below only ask. --------------------
constexpr double LOG2E = 1.4426950408889634074;   // the pre-scaled coordinates: |x~|^2 = LOG2E |x|^2 / l^2

static int mfma_k2_for(int dims) {   // MFMAs per tile for `dims` (pseudo-)coordinates (two each), from the compiled set (dense_mfma.hpp: mfma_for_k2)
    static const int ks[] = {1, 2, 3, 4, 6, 8, 12, 16};
    const int need = (dims + 1) / 2;
    for (int k : ks) if (k >= need) return k;
    return -1;
}

bool mfma_eq_eligible(const covgram_ctx* ctx, const HostKernel& hk, const covgram_points* X, const covgram_points* Y, int nrhs) {
    if (ctx->dense_variant == 1) return false;
    if (hk.tu_family != COVGRAM_EQ || hk.k.power != 1 || X->dtype != COVGRAM_F32 || nrhs != 1) return false;
    if (X->d > 32 || Y->n == 0) return false;                   // beyond d = 32 the fragments leave one wave per SIMD
    if (ctx->dense_variant == 2) return true;
    const double g2 = LOG2E / (hk.k.lengthscale * hk.k.lengthscale);   // |x~|^2 = g2 |x|^2
    return g2 * gate_radius2(X, Y) <= mfma_gate_of(ctx);                 // BOTH sides: a far X cluster must not ride on a compact Y
}

// Which split (round 4) of the EQ forms' coordinates, and with it the MFMAs per tile.  The bf16 three-way split is exact to 2^-24 |x~_c y~_c| per
// coordinate and costs one MFMA per TWO coordinates.  The fp16 two-way split (x~ = h1 + h2, 11 + 11 bits; products h1 h1, h1 h2, h2 h1) drops terms
// of ~2^-22 |x~_c y~_c| — the size of ONE fp32 rounding of the dot product itself, which the accumulator commits anyway — and covers FOUR coordinates
// per MFMA: half the matrix-core work per pair.  The d = 5 ... 8 kernels are power-bound (2.0 GHz under C3's shard kernel,
// profiles/r04_c3_power_bound.txt), so that is both fewer cycles and a higher clock.  Taken while BOTH clouds lie within g^2 R^2 <= MFMA_F16_GATE
// (the added exponent error grows with the radius like the accumulator's own: common.hpp); beyond it, up to MFMA_GATE, the bf16 split serves as
// before.  Option "mfma_f16": -1 / 1 = this rule, 0 = never, 2 = wherever the matrix-core gate admits the cloud (measurements: tools/f16_split_ab.py).
// (gramian(k, x): every rank of a multi-GPU call sees the same cloud and lengthscale, hence the same split and the same panel size)
struct EqSplit { int fmt, K2; };
static EqSplit eq_split(const covgram_ctx* ctx, const HostKernel& hk, const covgram_points* X, const covgram_points* Y) {
    const double g2r2 = LOG2E / (hk.k.lengthscale * hk.k.lengthscale) * gate_radius2(X, Y);
    const int fmt = (ctx->mfma_f16 != 0 && g2r2 <= (ctx->mfma_f16 == 2 ? mfma_gate_of(ctx) : mfma_f16_gate_of(ctx))) ? 1 : 0;
    return {fmt, fmt ? mfma_k2_for(2 * ((X->d + 3) / 4)) : mfma_k2_for(X->d)};      // fp16: one MFMA per four coordinates
}

#define CG_DECL(n) int launch_mfma_family_##n(const MfmaArgs&, bool query);   // one translation unit per launcher family (mfma_fam.hip)
CG_DECL(0) CG_DECL(2) CG_DECL(4) CG_DECL(5) CG_DECL(6) CG_DECL(7) CG_DECL(8) CG_DECL(11) CG_DECL(12) CG_DECL(13)
#undef CG_DECL

mfma_launch_fn mfma_launcher(int family) {
    switch (family) {
        case COVGRAM_EQ: return launch_mfma_family_0;
        case COVGRAM_RQ: return launch_mfma_family_2;
        case COVGRAM_CAUCHY: return launch_mfma_family_4;
        case COVGRAM_IMQ: return launch_mfma_family_5;
        case COVGRAM_MATERNP: return launch_mfma_family_6;
        case COVGRAM_DOT: return launch_mfma_family_7;
        case COVGRAM_EXPDOT: return launch_mfma_family_8;
        case FAM_EXPR_ISO: return launch_mfma_family_11;          // Sum / Product / Power composites of the profiles above
        case FAM_EXPR_DOT: return launch_mfma_family_12;
        case FAM_SUM_ISO: return launch_mfma_family_13;           // a Sum of 2-3 single-profile isotropic terms in one pass (common.hpp: SumParams)
        default: return nullptr;
    }
}

// relative sensitivity of a profile to an absolute error in s (natural units): |phi'/phi| at its maximum.  0: a dot-product factor (x.y itself:
// no cancellation to gate); infinity: no matrix-core form (Exp = MaternP(0), gammaExp, Matern(nu), asin: not differentiable in s at 0 — direct
// differences only)
static double mfma_profile_sens(int fam, const KParams<double>& q) {
    switch (fam) {
        case COVGRAM_EQ: case COVGRAM_RQ: return 0.5;
        case COVGRAM_CAUCHY: return 1.0;
        case COVGRAM_IMQ: return 0.5 / q.param;                      // 1/sqrt(s + c^2) at s = 0 (param holds c^2)
        case COVGRAM_MATERNP: return q.p < 1 ? INFINITY : (fabs(q.mp_d1) > 0.5 ? fabs(q.mp_d1) : 0.5);
        case COVGRAM_DOT: case COVGRAM_EXPDOT: return 0.0;
        default: return INFINITY;
    }
}
// sensitivity x Power of a kernel.  A composite: every factor must be one of the smooth matrix-core profiles, and the relative errors of a product
// add up: the largest sum over a term's factors of (sensitivity x power / l^2) takes the place of the single profile's (whose 1 / l^2 the caller applies)
static double mfma_kernel_sens(const HostKernel& hk) {
    if (hk.tu_family < COVGRAM_NFAMILY) return mfma_profile_sens(hk.tu_family, hk.kp) * hk.k.power;
    double worst = 0.0;
    int fi = 0;
    for (int t = 0; t < hk.nterms; ++t) {
        double sum = 0.0;
        for (int f = 0; f < hk.nfac[t]; ++f, ++fi) {
            const double s = mfma_profile_sens(hk.ffam[fi], hk.fkp[fi]);
            if (!(s < INFINITY)) return INFINITY;
            sum += s * hk.fkp[fi].power * hk.fkp[fi].gamma2;
        }
        worst = std::max(worst, sum);
    }
    return worst;
}
// (radius-gate quantity of an ISOTROPIC generic matrix-core MVM) / (what mfma_gen_eligible admits at mfma_gate_pct = 100): sensitivity x Power x
// g^2 R^2 over 0.5 MFMA_GATE / log2(e) — the EQ gate in natural units —, single profiles and composites alike; infinity where a profile has no
// matrix-core form
static double mfma_gen_gate_frac(const HostKernel& hk, const covgram_points* X, const covgram_points* Y) {
    const double limit = 0.5 * MFMA_GATE / LOG2E;
    const double Pn = gate_radius2(X, Y);                                  // natural units: every factor of a composite has its own 1 / l^2
    if (!(Pn < 1e30)) return INFINITY;
    const double l2 = hk.tu_family < COVGRAM_NFAMILY ? hk.k.lengthscale * hk.k.lengthscale : 1.0;
    return mfma_kernel_sens(hk) * Pn / l2 / limit;
}

bool mfma_gen_eligible(const covgram_ctx* ctx, const HostKernel& hk, const covgram_points* X, const covgram_points* Y, int nrhs) {
    if (ctx->dense_variant == 1 || X->dtype != COVGRAM_F32 || Y->n == 0) return false;
    if (mfma_launcher(hk.tu_family) == nullptr) return false;
    // MaternP(p >= 1): up to round 4 the lane-per-row kernels (packed fp32 profile) beat the matrix-core ones (profile entry by entry) at d <= 4.
    // Round 5: the profile arithmetic runs on register pairs (dense_mfma.hpp: mfma_profile_pairs) and the order is a compile-time constant of the
    // instance: the general kernel is ahead at every d (16384 x 131072, d = 3: 428 against 543 us lane-per-row; d = 8: 631 against 862;
    // profiles/r05_sum_fused_ab.txt), the symmetric one too (n = 131072, d = 3: 2.0 against 2.6 ms) — MaternP(p >= 1) no longer has an exception here.
    if (!(mfma_kernel_sens(hk) < INFINITY)) return false;                      // some profile has no matrix-core form
    const bool iso = hk.k.trait == COVGRAM_ISOTROPIC;
    if (mfma_k2_for(X->d + (iso ? 1 : 0)) < 0) return false;
    if (ctx->dense_variant == 2) return true;
    if (!iso) {                                                                // x.y itself: no cancellation to gate, only the range
        const double P = sqrt(X->max_norm2) * sqrt(Y->max_norm2);
        return (hk.tu_family < COVGRAM_NFAMILY ? P / (hk.k.lengthscale * hk.k.lengthscale) : P) < 1e30;
    }
    return mfma_gen_gate_frac(hk, X, Y) <= 0.01 * (double)ctx->mfma_gate_pct;
}

// The generic kernels' split of the coordinates (round 5): the fp16 two-way split (dense_mfma.hpp: gen_row_fragments) for the isotropic single
// profiles and one-pass Sums while (a) its instance exists — d + 2 positions in at most `maxk2` MFMAs of four —, and (b) the cloud lies inside
// MFMA_F16_GATE / MFMA_GATE of the generic radius gate (mfma_gen_gate_frac: the quantity mfma_gen_eligible admits up to 1), the EQ kernel's rule
// (option "mfma_f16": 0 never, 2 wherever the matrix-core gate admits the cloud).  Returns the format and sets the MFMAs per tile.
static int mfma_gen_fmt(const covgram_ctx* ctx, const HostKernel& hk, int lfam, const covgram_points* X, const covgram_points* Y, int maxk2, int* K2) {
    const bool iso = hk.k.trait == COVGRAM_ISOTROPIC;
    const int d = X->d;
    *K2 = mfma_k2_for(d + (iso ? 1 : 0));
    if (ctx->mfma_f16 == 0 || !iso || lfam == FAM_EXPR_ISO || lfam == FAM_EXPR_DOT) return 0;
    int k2h = (d + 2 + 3) / 4;                                   // d + 2 positions, four per MFMA; compiled: 1, 2, 3, 4, 6, 8 (d <= 30)
    if (k2h == 5) k2h = 6; else if (k2h == 7) k2h = 8;
    if (k2h > maxk2 || k2h > 8) return 0;
    const double frac = mfma_gen_gate_frac(hk, X, Y);
    if (!(frac <= 0.01 * (double)ctx->mfma_gate_pct * (ctx->mfma_f16 == 2 ? 1.0 : MFMA_F16_GATE / MFMA_GATE))) return 0;
    *K2 = k2h;
    return 1;
}

// The launcher family and coordinate pre-scale of a generic matrix-core MVM: a Sum of single-profile terms runs its one-pass form
// (FAM_SUM_ISO: the pre-scale carries the first term's argument scale) unless option "sum_fused" = 0 keeps the composite interpreter.
static int mfma_family_of(const covgram_ctx* ctx, const HostKernel& hk, float* gamma) {
    if (ctx->sum_fused != 0 && sum_fusable(hk)) { *gamma = (float)make_sum_params(hk).gamma; return FAM_SUM_ISO; }
    *gamma = (float)hk.kp.gamma;
    return hk.tu_family;
}

// gramian(k, x) on a symmetric (upper-triangle) matrix-core form: the same point set on both sides and one right-hand side (option "mfma_sym" = 0:
// never), the column-sum slab — one row of the padded n per panel of `tpp` row tiles; tpp = 0: not asked — within 16 GiB of the 288, and n from
// `min_n` on, the size from which the form pays (option "mfma_sym" = 1: at any n)
static bool mfma_sym_admits(const covgram_ctx* ctx, const covgram_points* X, const covgram_points* Y, int nrhs, int tpp, int64_t min_n) {
    if (ctx->mfma_sym == 0 || nrhs != 1 || X->dptr != Y->dptr || X->n != Y->n) return false;
    if (tpp > 0) {
        const int64_t panels = sym_panels((X->n + 31) / 32, tpp);
        if ((size_t)panels * (size_t)(panels * 32 * tpp) * sizeof(float) > ((size_t)16 << 30)) return false;
    }
    return ctx->mfma_sym == 1 || X->n >= min_n;
}
// ... of the generic profiles.  heavy: the profile costs several exponentials (at d > 4: the all-entries kernel's cost grows with the fragment length,
// the symmetric kernel's floor does not — tools/sym_threshold_sweep.py, MaternP(2) d = 8: n = 10000 60.0 / 59.8 us, 12000 77.4 / 66.7)
static int64_t mfma_gen_sym_min_n(const HostKernel& hk, int d) {
    const bool heavy = hk.tu_family == COVGRAM_MATERNP || hk.tu_family == COVGRAM_RQ || hk.tu_family >= COVGRAM_NFAMILY;
    return heavy ? (d > 4 ? 10000 : MFMA_SYM_MIN_N_HEAVY) : MFMA_SYM_MIN_N_EQ_WIDE;
}

bool mfma_eq_sym_eligible(const covgram_ctx* ctx, const HostKernel& hk, const covgram_points* X, const covgram_points* Y, int nrhs) {
    if (!mfma_eq_eligible(ctx, hk, X, Y, nrhs)) return false;
    const int tpp = mfma_k2_for(X->d) > MFMA_NARROW_MAXK2 ? 4 : 8;                  // row tiles per panel (dense_mfma_sym_wide_kernel: 4)
    return mfma_sym_admits(ctx, X, Y, nrhs, tpp, X->d <= 4 ? MFMA_SYM_MIN_N_EQ : MFMA_SYM_MIN_N_EQ_WIDE);
}

// the generic profiles' symmetric form: same conditions on top of the generic matrix-core gate (hk: gamma = 1/l parameter block)
bool mfma_gen_sym_eligible(const covgram_ctx* ctx, const HostKernel& hk, const covgram_points* X, const covgram_points* Y, int nrhs) {
    if (!mfma_sym_admits(ctx, X, Y, nrhs, 0, 0) || !mfma_gen_eligible(ctx, hk, X, Y, nrhs)) return false;
    const int k2 = mfma_k2_for(X->d + (hk.k.trait == COVGRAM_ISOTROPIC ? 1 : 0));
    float gam_unused;
    const int lfam = mfma_family_of(ctx, hk, &gam_unused);
    if (lfam == FAM_SUM_ISO && k2 > 8) return false;                              // no one-pass symmetric instance: one (symmetric) MVM per term instead
    // (tiles per panel of the one-row-tile form: an upper bound of the slab whichever form runs — fewer tiles per panel = more panels)
    return mfma_sym_admits(ctx, X, Y, nrhs, mfma_sym_tiles_per_panel(lfam, k2), mfma_gen_sym_min_n(hk, X->d));
}

// covgram_mvm: does this composite take the one-pass Sum kernels (instead of one MVM per term)?
bool sum_fused_applies(const covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, int nrhs) {
    if (ctx->sum_fused == 0 || k == nullptr || k->family != COVGRAM_COMPOSITE || X->dtype != COVGRAM_F32 || Y->n == 0) return false;
    HostKernel hk;
    if (make_host_kernel(k, COVGRAM_F32, false, &hk) != COVGRAM_OK) return false;
    if (!sum_fusable(hk) || !mfma_gen_eligible(ctx, hk, X, Y, nrhs)) return false;
    // gramian(k, x) at d >= 16: the one-pass symmetric kernel has no instance (K2 > 8), and one symmetric MVM per term evaluates half the pairs
    // of the one-pass general kernel
    if (mfma_sym_admits(ctx, X, Y, nrhs, 0, mfma_gen_sym_min_n(hk, X->d)) && mfma_k2_for(X->d + 1) > 8) return false;
    // Measured (d = 3, n = 131072; profiles/r05_sum_fused_ab.txt, r05_sum_general_ab.txt): what one pass shares is the matrix-core work, the weighted
    // sums and the slabs — every term's transcendentals remain, and they are what the kernels are bound by.  Three terms: 4.07 against 4.83 ms for one
    // symmetric MVM per term, 0.95 / 1.01 against 0.98 / 1.09 on a 16384-row shard.  Two terms: one MVM per term wins or ties on both forms (symmetric
    // 3.05 against 3.32; shard, MaternP(2) + EQ: 0.62 against 0.71 — the EQ term costs 0.15 on its own kernel —, MaternP + MaternP 0.83 against 0.87,
    // RQ + MaternP 0.79 against 0.78): the one-pass kernel's wave-uniform family switches and its one-tile loop cost more than the second pass saves.
    // Option "sum_fused" = 1 takes the one-pass kernels wherever they exist (tests).
    if (ctx->sum_fused == 1) return true;
    return hk.nterms >= 3;
}

// ---- Steps the drivers share --------------------
// where a launch of plan `pl` leaves its sums: y itself, or (js > 1) the split-J slab of workspace slot 1, `nrpad` columns per chunk
static int split_out(covgram_ctx* ctx, const ColumnPlan& pl, int nrpad, float* y, float** out) {
    *out = y;
    return pl.js == 1 ? COVGRAM_OK : ws_reserve(ctx, 1, (size_t)pl.js * nrpad * pl.npad * sizeof(float), (void**)out);
}
// y[:, 0..nr) <- alpha (the js slab rows added in fixed order) + beta y
static void reduce_split(covgram_ctx* ctx, const float* slab, const ColumnPlan& pl, int nrpad, float* y, int64_t n, int64_t ldy, int nr, double alpha,
                         double beta) {
    dense_reduce(ctx, slab, pl.npad, nrpad, (int)pl.js, y, n, ldy, nr, alpha, beta);
}

// the generic kernels' column fragments (norm pseudo-coordinate) and the weights of `nr` right-hand sides in NR slots per tile, packed per MVM into
// workspace slot 0, with `extra` bytes behind them for the caller (*W + ntile NR 32)
static int gen_fragments(covgram_ctx* ctx, const covgram_points* Y, const float* a, int64_t lda, int nr, int NR, int K2, float gam, bool iso, int fmt,
                         size_t extra, const uint4** PB, float** W) {
    const int64_t ntile = (Y->n + 31) / 32, pe = ntile * K2 * 64;
    void* P;
    int rc = ws_reserve(ctx, 0, (size_t)ntile * ((size_t)K2 * 64 * sizeof(uint4) + (size_t)NR * 32 * sizeof(float)) + extra, &P);
    if (rc) return rc;
    *PB = (const uint4*)P;
    *W = (float*)((uint4*)P + pe);
    hipLaunchKernelGGL(mfma_pack_gen_kernel, dim3((unsigned)((pe + 255) / 256)), dim3(256), 0, ctx->stream, (const float*)Y->dptr, Y->n, Y->d, a, lda, nr, 0,
                       (uint4*)P, *W, K2, NR, gam, iso ? 1 : 0, (const float*)Y->center, fmt);
    return COVGRAM_OK;
}

// ---- EQ, all n m entries: dense_mfma_eq_kernel --------------------
// resident single-wave workgroups per CU of the kernel instance (register-limited), for the grid sizing below
template <int K2, int RT>
static int mfma_blocks_per_cu() {
    static int cached = 0;
    if (!cached) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, dense_mfma_eq_kernel<K2, RT>, 64, 0) != hipSuccess || nb <= 0) nb = 16;
        cached = nb;
    }
    return cached;
}
// the one place that spells dense_mfma_eq_kernel's argument list; a.grid counts WAVES (x: row blocks of 32 RT rows)
template <int K2, int RT, int WPB, int LDS, int STAMP, int FMT>
static void eq_launch(covgram_ctx* ctx, const MfmaArgs& a, dim3* launched) {
    *launched = dim3((a.grid.x + WPB - 1) / WPB, a.grid.y);
    if (a.occupancy) {   // the graded plan's question: how many workgroups of THIS instance a CU holds (asked once per instance), and its waves per workgroup
        static int cached = 0;
        if (!cached) {
            int nb = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, dense_mfma_eq_kernel<K2, RT, WPB, LDS, STAMP, FMT>, 64 * WPB, 0) != hipSuccess || nb <= 0) nb = std::max(1, 16 / WPB);
            cached = nb;
        }
        a.occupancy[0] = cached; a.occupancy[1] = WPB;
        return;
    }
    ctx->last_mfma_instance = (int64_t)K2 * 100000 + RT * 10000 + WPB * 1000 + LDS * 100 + STAMP * 10 + FMT;
    hipLaunchKernelGGL((dense_mfma_eq_kernel<K2, RT, WPB, LDS, STAMP, FMT>), *launched, dim3(64 * WPB), 0, a.stream, a.X, a.n, a.d, a.PB, a.W, a.ntile, a.out,
                       a.npad, a.tchunk, a.g, a.alpha, a.beta, a.final_store, a.Cn, STAMP ? a.stamps : nullptr, a.tickets, a.yfinal, a.EF, a.mcols, a.chunks);
}
// the instance of (K2, split) for this plan: row tiles per wave a.RT, the LDS-shared form (a.lds), the diagnostic build (a.stamps)
template <int K2, int FMT>
static void eq_launch_instance(covgram_ctx* ctx, const MfmaArgs& a, dim3* launched) {
    constexpr bool NARROW = K2 <= MFMA_NARROW_MAXK2;
    const bool stamp = a.stamps != nullptr;
    if (a.lds) {
        if constexpr (K2 <= 2) {   // d <= 4 and many row tiles: eight waves share each column tile (C2: 1.569 -> 1.550 ms; not for a 16384-row shard)
            if (a.grid.x >= 1024) return stamp ? eq_launch<K2, 2, 8, 1, 1, FMT>(ctx, a, launched) : eq_launch<K2, 2, 8, 1, 0, FMT>(ctx, a, launched);
        }
        // 256-thread workgroups: four waves on consecutive row tiles share the column tiles through LDS
        if constexpr (K2 == 3 || K2 == 4) { if (a.RT == 4) return eq_launch<K2, 4, 4, 1, 0, FMT>(ctx, a, launched); }
        if constexpr (K2 == 1 || K2 == 2 || K2 == 4) { if (stamp) return eq_launch<K2, 2, 4, 1, 1, FMT>(ctx, a, launched); }
        constexpr int LDSF = (NARROW || K2 == 6) ? 1 : 2;   // six MFMAs per tile: stages of four tiles too (round 5; one tile per stage before, as the longer fragments still are)
        return eq_launch<K2, (NARROW ? 2 : 1), 4, LDSF, 0, FMT>(ctx, a, launched);
    }
    if constexpr (K2 <= 8) { if (a.RT == 2) return eq_launch<K2, 2, 1, 0, 0, FMT>(ctx, a, launched); }
    eq_launch<K2, 1, 1, 0, 0, FMT>(ctx, a, launched);
}

// the column fragments and norm fraction factors of point set Y for (g, K2): packed once into the handle and reused by every
// later MVM (they depend on the points and the lengthscale only; the kernels form the weights a_j EF[j] themselves)
static int eq_fragments(covgram_ctx* ctx, const covgram_points* Y, int K2, float g, const float* Cn, const uint4** PB, const float** EF, int fmt = 0) {
    const int64_t m = Y->n, ntile = (m + 31) / 32;
    const size_t fbytes = (size_t)ntile * K2 * 64 * sizeof(uint4);
    const size_t total = fbytes + (size_t)ntile * 32 * sizeof(float);   // fragments + EF
    covgram_points::FragSlot* hit = nullptr;
    covgram_points::FragSlot* victim = nullptr;
    // a captured graph replays the kernels with the slot's ADDRESS baked in: a slot handed out during a capture is pinned — later eager
    // MVMs with other lengthscales evict the other slots only (the LRU re-pack silently changed what a replay reads)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = ctx->stream && hipStreamIsCapturing(ctx->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
    for (auto& f : Y->frag) {
        if (f.ptr && f.bytes == total && f.g == g && f.k2 == K2 && f.fmt == fmt) { hit = &f; break; }
        if (f.pinned) continue;
        // reuse order: an empty slot first, then a slot of another size (its buffer is replaced), then the least recently used
        const auto rank = [&](const covgram_points::FragSlot& s) { return !s.ptr ? 0 : (s.bytes != total ? 1 : 2); };
        if (!victim || rank(f) < rank(*victim) || (rank(f) == rank(*victim) && f.used < victim->used)) victim = &f;
    }
    if (!hit) {
        CG_REQUIRE(victim != nullptr, COVGRAM_EUNSUPPORTED, "all %d fragment slots of this point set are pinned by captured graphs (one per (lengthscale, d) used "
                   "inside a capture): destroy the handle, or keep to %d lengthscales per point set in graphs", covgram_points::FRAG_SLOTS, covgram_points::FRAG_SLOTS);
        // ANY miss during capture is refused: a re-pack captured into the graph would leave the slot's key naming fragments that do not exist
        // until the first replay (an eager MVM in between would read the previous lengthscale's), and it would pin a slot per captured lengthscale
        CG_REQUIRE(!capturing, COVGRAM_EUNSUPPORTED,
                   "the fragments of this (point set, lengthscale) must be packed once OUTSIDE stream capture: run one eager MVM with this lengthscale first");
        if (victim->ptr && victim->bytes != total) {   // only when the handle is re-used at another K2: off the steady-state path
            CG_CHECK_HIP(hipStreamSynchronize(ctx->stream)); (void)hipFree(victim->ptr); victim->ptr = nullptr;
        }
        if (!victim->ptr) {
            hipError_t me = hipMalloc(&victim->ptr, total);
            if (me != hipSuccess) { victim->ptr = nullptr; set_error("hipMalloc(%zu) failed: %s", total, hipGetErrorString(me)); return COVGRAM_ENOMEM; }
            victim->bytes = total;
        }
        // in place, stream-ordered behind every MVM that still reads this slot
        victim->g = g; victim->k2 = K2; victim->fmt = fmt;
        const int64_t pe = ntile * K2 * 64;
        hipLaunchKernelGGL(mfma_pack_kernel, dim3((unsigned)((pe + 255) / 256)), dim3(256), 0, ctx->stream, (const float*)Y->dptr, m, Y->d,
                           (uint4*)victim->ptr, (float*)((char*)victim->ptr + fbytes), K2, g, Cn, fmt);
        hit = victim;
    }
    if (capturing) hit->pinned = true;
    hit->used = ++Y->frag_clock;
    *PB = (const uint4*)hit->ptr;
    *EF = (const float*)((const char*)hit->ptr + fbytes);
    return COVGRAM_OK;
}

// y <- alpha * scale * G a + beta * y for ONE right-hand side (device pointers)
int mvm_eq_mfma(covgram_ctx* ctx, const HostKernel& hk, const covgram_points* X, const covgram_points* Y, const float* a, float* y,
                double alpha, double beta) {
    const int64_t n = X->n, m = Y->n;
    const EqSplit sp = eq_split(ctx, hk, X, Y);
    const int fmt = sp.fmt, K2 = sp.K2;
    ctx->last_mfma_f16 = fmt;
    CG_REQUIRE(K2 > 0, COVGRAM_EUNSUPPORTED, "dense_mfma: d = %d has no matrix-core instance", X->d);
    MfmaArgs ma;
    ma.X = (const float*)X->dptr; ma.n = n; ma.d = X->d; ma.ntile = (m + 31) / 32; ma.mcols = m; ma.K2 = K2; ma.fmt = fmt; ma.stream = ctx->stream;
    ma.g = (float)(sqrt(LOG2E) / hk.k.lengthscale);
    ma.Cn = (const float*)Y->center;                              // both sides are taken relative to the column side's centre
    ma.alpha = (float)(alpha * hk.kp.scale); ma.beta = (float)beta; ma.yfinal = y;
    const int64_t ntile = ma.ntile;
    const float* EF;
    int rc = eq_fragments(ctx, Y, K2, ma.g, ma.Cn, &ma.PB, &EF, fmt);
    if (rc) return rc;
    // the weights a_j exp2(f_j) of THIS right-hand side: formed inside the kernel (round 4) — the wave that fetches a tile loads a_j and the cached
    // exp2(f_j) with it and multiplies where the weight goes to LDS at the end of the stage.  (Rounds 1-2 had measured the in-kernel product 3 %
    // SLOWER than the pack launch: the product stood right behind its two loads and so behind the LDS-DMA the wave had just issued — one counter.
    // Deferred: C2-shaped 1359 -> 1340 us, a 16384-row shard 190.1 -> 186.5, n = 16384 35.1 -> 33.2, n = 2048 12.1 -> 10.8;
    // profiles/r04_fuse_w_ab.txt.)  Option "mfma_fuse_w" = 0 restores the pack launch; results are bit-identical either way.
    // ... unless a and y overlap (an in-place MVM, y == a): the workgroups of a final-store or ticketed launch write y while others still read
    // a — the pack launch copies the weights first, as every dense path did before round 4 (include/covgram.h: aliasing)
    const bool overlap = (const char*)a < (const char*)(y + n) && (const char*)y < (const char*)(a + m);
    const bool fuse_w = ctx->mfma_fuse_w != 0 && !overlap;
    ma.W = a; ma.EF = EF;
    if (!fuse_w) {
        void* Wp;
        rc = ws_reserve(ctx, 0, (size_t)ntile * 32 * sizeof(float), &Wp);
        if (rc) return rc;
        hipLaunchKernelGGL(mfma_pack_w_kernel, dim3((unsigned)((ntile * 32 + 255) / 256)), dim3(256), 0, ctx->stream, a, EF, (float*)Wp, m, ntile * 32);
        ma.W = (const float*)Wp; ma.EF = nullptr;
    }
    // split the column tiles so that the grid holds ~CUs * 128 waves (as the lane-per-row kernel, profiles/r01_quickbench_wg64.txt)
    // row tiles per wave: two share every B fragment while the state fits (d <= 8); option "rows_per_lane" = 1 / 2 forces it
    int rt = ctx->rows_per_lane == 1 ? 1 : (ctx->rows_per_lane == 2 ? 2 : (K2 <= MFMA_NARROW_MAXK2 ? 2 : 1));
    if (K2 > 8) rt = 1;
    // the uniform plan aims at 4 rounds of resident one-wave workgroups (nb per CU); where the LDS-shared form then runs at least two rounds of ITS resident
    // workgroups, the end of the column range is cut finer below ("graded split"): equal workgroups do not finish together, and the chip drains in their length
    int nb = 16;
    mfma_for_k2(K2, [&](auto k) {
        constexpr int K = decltype(k)::value;
        if constexpr (K <= 8) { if (rt == 2) { nb = mfma_blocks_per_cu<K, 2>(); return; } }
        nb = mfma_blocks_per_cu<K, 1>();
    });
    struct Plan { ColumnPlan col; int rt; bool lds4; };
    auto plan_for = [&](int r) {
        Plan pl; pl.rt = r;
        const int64_t target = ctx->target_wgs > 0 ? ctx->target_wgs : (int64_t)ctx->num_cus * nb * 4;
        pl.col = plan_columns(n, ntile, 32 * r, target, ctx->jsplit, 8, 64, 2048, 16);     // (the 64-tile stop and its 2048-wave floor: mfma_plan.hpp)
        // long column chunks: four waves of a workgroup share every column tile through LDS; short chunks would only pay its
        // prologue and barriers (tools/mfma_lds_ab.py)
        pl.lds4 = ((r >= 2 && K2 <= MFMA_NARROW_MAXK2) || (r == 1 && K2 > MFMA_NARROW_MAXK2)) &&
                  (ctx->mfma_lds == 1 || (ctx->mfma_lds < 0 && pl.col.tchunk >= MFMA_LDS_MIN_TILES && pl.col.rowtiles >= 64));
        return pl;
    };
    Plan pl = plan_for(rt);
    // d = 7, 8 (four MFMAs per tile) on the LDS-shared form: FOUR row tiles per wave, two waves per SIMD (round 4) — every column fragment
    // read from LDS, every LDS-DMA issue and every stage barrier serves twice the pairs: C3's row shard 4.31 -> 4.13 ms, a 16384-row shard
    // of 131072 columns 313 -> 305 us, 131072^2 at d = 7 1.565 -> 1.516 ms (tools/c3_rt_ab.py; d = 5, 6: 3.67 -> 3.66, left alone).
    // Option "rows_per_lane" = 4 asks for it wherever the instance exists (K2 = 3, 4), 2 keeps two row tiles.
    if ((K2 == 3 || K2 == 4) && pl.lds4 && pl.rt == 2 && (ctx->rows_per_lane == 4 || (ctx->rows_per_lane == 0 && K2 == 4 && !ctx->mfma_stamp))) {
        const Plan p4 = plan_for(4);
        if (p4.lds4) pl = p4;
    }
    ColumnPlan col = pl.col;
    ma.RT = pl.rt; ma.lds = pl.lds4 ? 1 : 0;
    ma.grid = dim3((unsigned)col.rowtiles, (unsigned)col.js);
    // The graded split (mfma_plan.hpp: plan_columns_graded).  Equal chunks fill the resident slots in whole rounds only on paper: the workgroups of a
    // round do not finish together, a slot that is done with its last one has nothing left to take, and the chip drains at the granularity of a
    // workgroup's life — C2's 8 x 256 workgroups on 512 slots live a quarter of the kernel each (tools/c2_drain_probe.py, profiles/c2_graded_split.txt).
    // The last half round's worth of columns is cut into chunks that halve down to MFMA_LDS_MIN_TILES, dispatched last: the slots that free up first
    // take them.  Automatic only where it can pay — shapes of the LDS-shared form, at least two rounds of the instance's resident workgroups, chunks at or above
    // the LDS form's minimum —; a forced "jsplit" / "target_wgs" and the GP-sized shapes under plan_columns' stop / floor clamps keep the uniform split.
    // Option "mfma_graded": -1 this rule, 0 never, 1 wherever the shape admits a graded table (tests), 100 h + f = 1 with a tail of h half rounds and a
    // floor of 16 * 2^f tiles (measurements: tools/c2_graded_ab.py).  The slab keeps one row per chunk, summed in chunk order: deterministic, as before.
    ctx->last_mfma_graded = 0;
    if (ctx->mfma_graded != 0 && ctx->jsplit <= 0 && ctx->target_wgs <= 0 && col.js > 1) {
        // The rule looks at the SHAPE — would the automatic "mfma_lds" share its column tiles through LDS? — and plans for that LDS-shared instance
        // even when option "mfma_lds" = 0 / 1 picks the form by hand: the table, and with it every bit of the result, is the same for both forms
        // (tests/test_gpu_parity.py compares them bit for bit)
        const bool lds_shape = ((pl.rt >= 2 && K2 <= MFMA_NARROW_MAXK2) || (pl.rt == 1 && K2 > MFMA_NARROW_MAXK2)) && col.tchunk >= MFMA_LDS_MIN_TILES &&
                               col.rowtiles >= 64;
        int occ[2] = {0, 1};                                             // resident workgroups per CU and waves per workgroup of the instance planned for
        dim3 unused;
        MfmaArgs q = ma;
        q.lds = lds_shape ? 1 : ma.lds; q.occupancy = occ;
        mfma_for_k2(K2, [&](auto k) {
            constexpr int K = decltype(k)::value;
            if (!fmt) eq_launch_instance<K, 0>(ctx, q, &unused);
            else if constexpr (K <= 8) eq_launch_instance<K, 1>(ctx, q, &unused);
        });
        const bool force = ctx->mfma_graded > 0;
        const int64_t wpb = occ[1], rblocks = (col.rowtiles + wpb - 1) / wpb, slots = (int64_t)ctx->num_cus * occ[0];
        // (GP-sized shapes: the split plan_columns' stop / floor clamps changed stays as measured there)
        const bool clamped = plan_columns(n, ntile, 32 * pl.rt, (int64_t)ctx->num_cus * nb * 4, 0, 8).js != col.js;
        // the floor: the LDS form's minimum; forced on a shape whose chunks are shorter than two of those, a wave's minimum of 8 tiles
        int64_t floor_tiles = col.tchunk >= 2 * MFMA_LDS_MIN_TILES ? MFMA_LDS_MIN_TILES : 8, halfrounds = MFMA_GRADED_TAIL_HALFROUNDS;
        if (ctx->mfma_graded >= 100) { halfrounds = ctx->mfma_graded / 100; floor_tiles = (int64_t)16 << (ctx->mfma_graded % 10); }   // (measurements)
        if (force || (lds_shape && !clamped)) {
            const GradedPlan gp = plan_columns_graded(col, ntile, rblocks, slots, q.lds ? wpb : 2 /* (that loop walks tile pairs) */, floor_tiles, force, halfrounds);
            if (gp.graded) {
                col.js = gp.js;
                ma.chunks.n = (int32_t)gp.js;
                for (int c = 0; c <= GRADED_MAX_CHUNKS; ++c) ma.chunks.start[c] = gp.start[c];
                ma.grid.y = (unsigned)gp.js;
                ctx->last_mfma_graded = gp.js;
            }
        }
    }
    ma.npad = col.npad; ma.tchunk = col.tchunk; ma.final_store = col.js == 1 ? 1 : 0;
    rc = split_out(ctx, col, 1, y, &ma.out);
    if (rc) return rc;
    // option "mfma_stamp": the clock-stamping diagnostic build of the two LDS-shared instances (C2's and C3's kernels)
    ctx->stamp_count = 0;
    if (ctx->mfma_stamp && pl.lds4 && (K2 == 1 || K2 == 2 || K2 == 4)) {
        const size_t need = (size_t)col.rowtiles * col.js * 4 * sizeof(unsigned long long);
        if (need > ctx->stamp_cap) {
            if (ctx->stamp_buf) { CG_CHECK_HIP(hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->stamp_buf); ctx->stamp_buf = nullptr; ctx->stamp_cap = 0; }
            CG_CHECK_HIP(hipMalloc(&ctx->stamp_buf, need));
            ctx->stamp_cap = need;
        }
        CG_CHECK_HIP(hipMemsetAsync(ctx->stamp_buf, 0, need, ctx->stream));
        ma.stamps = (unsigned long long*)ctx->stamp_buf;
    }
    // js > 1: the kernel can sum its own split-J slab (the last workgroup of each row block to arrive, fixed order; pack.hpp).  Measured
    // (profiles/r04_inkernel_reduce_ab.txt, separate launch -> in-kernel): n = 2048 16.2 -> 13.2 us, 4096 16.3 -> 14.9, 8192 17.2 -> 18.8,
    // 16384 37.9 -> 37.2, rank 0 of 8's shard of C2 214.4 -> 213.5, of 16 116.3 -> 115.0: it pays where the whole MVM is launch latency
    // and is noise elsewhere, so the automatic rule takes it up to n = 4096 (option "inkernel_reduce" = 1 / 0 forces it on / off)
    const bool ikr = inkernel_reduce_on(ctx, true, n, col.js);
    ctx->last_inkernel_reduce = ikr ? 1 : 0;
    if (ikr) { rc = tickets_reserve(ctx, (size_t)col.rowtiles, &ma.tickets); if (rc) return rc; }
    ctx->last_mfma_lds = ma.lds;
    dim3 launched;
    {
        TimerScope tm(ctx);
        const bool compiled = mfma_for_k2(K2, [&](auto k) {
            constexpr int K = decltype(k)::value;
            if (!fmt) eq_launch_instance<K, 0>(ctx, ma, &launched);
            else if constexpr (K <= 8) eq_launch_instance<K, 1>(ctx, ma, &launched);   // (the fp16 split: d <= 32 in at most eight MFMAs)
        });
        CG_REQUIRE(compiled, COVGRAM_EUNSUPPORTED, "dense_mfma: K2 = %d not compiled", K2);
    }
    if (ma.stamps) ctx->stamp_count = (size_t)launched.x * launched.y;
    if (col.js > 1 && !ikr) reduce_split(ctx, ma.out, col, 1, y, n, n, 1, alpha * hk.kp.scale, beta);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("dense_mfma launch failed: %s", hipGetErrorString(e)); return COVGRAM_EHIP; }
    return COVGRAM_OK;
}

// ---- Symmetric Gramian (gramian(k, x): y IS x) ----: every tile on or above the diagonal is evaluated ONCE and used twice,
//     b_i += e_i sum_j (a_j e_j) E_ij          (row sums, as dense_mfma_eq_kernel)
//     b_j += e_j sum_i (a_i e_i) E_ij          (column sums of the same exponentials, tiles strictly above the diagonal)
// with E_ij = exp2(x~_i . x~_j + k_i + k_j) from the MFMA and e = exp2(f) in (1/2, 1] the fraction factors of the half-norms
// (dense_mfma.hpp: norm_split): one v_exp_f32 and TWO v_fma_f32 per evaluated pair, i.e. 6 VALU
// issue cycles per Gramian entry instead of 10, and half the MFMAs.  The reference evaluates all n^2 entries
// (src/gramian.jl:78-87 does not look at issymmetric); the sums are the same numbers in a different order.
//
// Work decomposition: a workgroup = 8 waves x 1 row tile = a PANEL of 256 rows; workgroup (p, c) walks the column tiles
// [max(8 p, c tchunk), (c + 1) tchunk) — everything from the panel's own first tile to the right — with the LDS staging
// of the non-symmetric kernel.  Inside the panel's diagonal block the tiles below the diagonal are masked (weight 0 for
// the row sums of tiles J < I, for the column sums of tiles J <= I): < 0.5 % wasted work.  Row sums leave through the
// per-chunk slab R[c][i]; the column sums of a tile are added over the 8 waves in LDS in fixed order and stored to
// S[p][j] (each (p, tile) exactly once); dense_mfma_sym_reduce_kernel adds R over the panel's chunks and S over the panels
// p <= panel(j) in fixed order: deterministic, no float atomics.
//
// b_i = alpha (sum_{chunks c the panel of i visited} R[c][i] + e_i sum_{p <= panel(i)} S[p][i]) + beta b_i, fixed order
// (EF = the fraction factors e_i the EQ form's column sums still lack; nullptr: generic form).
// 64 rows per workgroup, the panel index strided over the 4 waves (as dense_reduce_kernel).
__global__ __launch_bounds__(1024) void dense_mfma_sym_reduce_kernel(int64_t n, const float* __restrict__ R, const float* __restrict__ S, int64_t npad,
                                                                    int64_t ntile, int32_t tchunk, const float* __restrict__ EF, float* __restrict__ y,
                                                                    float alpha, float beta, int32_t pfirst, int32_t pstride, int32_t tpp) {
    // 256 rows per workgroup — FOUR consecutive rows per lane (16-byte loads: the slab is hundreds of MB read once; round 5, 4-byte loads before:
    // 3.1 TB/s) —, the panel index strided over 16 waves (hundreds of panels per row: many independent loads in flight).  Per row the sums are formed
    // in the same order as before (panels part, part + 16, ...; then the 16 parts; then the chunks): bit-identical results.
    // (npad is a multiple of 4 and the slabs are 256-byte aligned; rows >= n of a lane's four are read — the slabs are padded — and not stored)
    typedef float f4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int64_t i = ((int64_t)blockIdx.x * 64 + lane) * 4;
    __shared__ f4 red[16][64];
    f4 s = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i < n) {
        const int64_t pi = i / (32 * tpp);                                           // the rows' panel (tpp row tiles: 256 or 128 rows — four rows share it)
        // local panels lp (global pfirst + pstride lp) up to the row's own panel
        const int64_t nlp = pi >= pfirst ? (pi - pfirst) / pstride + 1 : 0;
#pragma unroll 4
        for (int64_t lp = part; lp < nlp; lp += 16) s += *reinterpret_cast<const f4*>(S + lp * npad + i);
    }
    red[part][lane] = s;
    __syncthreads();
    if (part != 0 || i >= n) return;
    f4 cs = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < 16; ++q) cs += red[q][lane];                                  // fixed order
    const int64_t pi = i / (32 * tpp);
    const int64_t cfirst = (tpp * pi) / tchunk, cend = (ntile + tchunk - 1) / tchunk;   // the absolute chunks the row's panel visited
    f4 rs = {0.0f, 0.0f, 0.0f, 0.0f};
    if (pi >= pfirst && (pi - pfirst) % pstride == 0)                                 // the row sums exist only where this rank owns the panel
        for (int64_t c = cfirst; c < cend; ++c) rs += *reinterpret_cast<const f4*>(R + c * npad + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (i + e >= n) break;
        float v = alpha * (EF ? __builtin_fmaf(EF[i + e], cs[e], rs[e]) : cs[e] + rs[e]);
        if (beta != 0.0f) v = __builtin_fmaf(beta, y[i + e], v);
        y[i + e] = v;
    }
}

// the symmetric kernel of this call, resolved from the kernel, the cloud and the options: launcher family and its coordinate pre-scale (generic form), split of
// the coordinates and MFMAs per tile, row tiles per wave (2: dense_mfma_sym2_kernel) and per panel, EQ form at K2 > 4: the staged 8-wave kernel
struct SymForm { int lfam = COVGRAM_EQ; float gam = 0.0f; int fmt = 0, K2 = 0, rt = 1, tpp = 8; bool staged_wide = false; };
static SymForm sym_form(covgram_ctx* ctx, const HostKernel& hk, const covgram_points* X, bool fast) {
    SymForm f;
    if (fast) {
        const EqSplit sp = eq_split(ctx, hk, X, X);
        f.fmt = sp.fmt; f.K2 = sp.K2;
        // the EQ forms up to four MFMAs per tile: two row tiles per wave, 4-wave workgroups (dense_mfma_sym2.hpp) — option "mfma_sym_rt": 2 = that,
        // -1 = that up to two MFMAs per tile, 1 = the 8-wave one-row-tile kernel
        f.rt = (f.K2 <= (ctx->mfma_sym_rt == 2 ? MFMA_NARROW_MAXK2 : 2) && ctx->mfma_sym_rt != 1) ? 2 : 1;
        // Six MFMAs per tile (d = 17 .. 24 with the fp16 split, 11 .. 12 with bf16): the STAGED 8-wave kernel (four column tiles per stage and barrier, one
        // tile at a time in registers) instead of the one-tile-per-stage 4-wave kernel — round 5, tools/wide_staged_ab.py: n = 131072, d = 24 2.19 -> 1.89 ms,
        // d = 20 2.16 -> 1.82.  Eight MFMAs per tile need 169 registers there (two waves per SIMD): 2.55 -> 2.60 ms, so they keep the 4-wave kernel
        // (option "mfma_sym_st" = 16 forces the staged form for measurements).
        f.staged_wide = f.K2 == 6 || (f.K2 == 8 && f.fmt == 1 && ctx->mfma_sym_st == 16);
        // row tiles per panel: 8 waves x 1 tile (or 4 x 2), or 4 x 1 for long fragments (dense_mfma.hpp)
        f.tpp = (f.K2 > MFMA_NARROW_MAXK2 && !f.staged_wide) ? 4 : 8;
        return f;
    }
    const bool iso = hk.k.trait == COVGRAM_ISOTROPIC;
    f.lfam = mfma_family_of(ctx, hk, &f.gam);
    ctx->last_sum_fused = f.lfam == FAM_SUM_ISO ? 1 : 0;
    // the fp16 split where the staged (narrow) symmetric kernel of the family has the instance (dense_mfma.hpp: mfma_sym_narrow_maxk2)
    f.fmt = mfma_gen_fmt(ctx, hk, f.lfam, X, X, f.lfam == FAM_SUM_ISO ? 2 : 8, &f.K2);   // (the Sum: its staged kernel only)
    // at one or two MFMAs per tile: two row tiles per wave as the EQ form (dense_mfma_sym2.hpp; option "mfma_sym_rt" = 1: the one-row-tile panels)
    f.rt = (ctx->mfma_sym_rt != 1 && mfma_sym2_has(f.lfam, f.K2)) ? 2 : 1;
    f.tpp = mfma_sym_tiles_per_panel(f.lfam, f.K2, f.rt);   // 8 waves x 1 tile, 4 for the heavy profiles' 3-waves-per-SIMD form and for long fragments
    return f;
}

// column chunk of the symmetric kernels: a multiple of the 4-tile stage; ~8 rounds of the resident workgroups (2 per CU) over the triangle,
// ~4 for one rank's share of a multi-GPU MVM (the work list puts the cut, shorter chunks last, so the last round balances); >= 64 tiles —
// shorter chunks do not amortise a workgroup's prologue (rows, row weights, first stage) —, >= 128 for a rank's share (tools/sym_tchunk_sweep.py,
// tools/sym_shard_probe.py: rank r of 8 at C2 size 170-185 us with 128-tile chunks, 183-201 with 64).
// (4-wave workgroups: three per CU.  The two-row-tile kernels — heavier prologue: two sets of row fragments and weights per wave — take ~5 rounds:
//  tools/sym_rounds_ab.py, interleaved, n = 131072: EQ d = 3 980 / 962 / 958 us at 8 / 5 / 4 rounds, d = 8 1154 / 1131 / 1117; n = 262144 level)
static int64_t sym_tchunk(const covgram_ctx* ctx, const SymForm& f, int64_t ntile, int pstride) {
    const int64_t panels = sym_panels(ntile, f.tpp);
    const int64_t tileops = (panels * ntile / 2 + panels * 4) / pstride;         // (panel, tile) visits
    const bool two_row = f.rt == 2;
    const int64_t target = ctx->target_wgs > 0 ? ctx->target_wgs : (int64_t)ctx->num_cus * ((f.tpp == 4 || two_row) ? 3 : 2) * (pstride > 1 ? 4 : (two_row ? 5 : 8));
    const int64_t tchunk = ctx->jsplit > 0 ? (ntile + ctx->jsplit - 1) / ctx->jsplit : (tileops + target - 1) / target;
    return std::max<int64_t>(pstride > 1 ? 128 : 64, std::min<int64_t>(((tchunk + 3) / 4) * 4, 1024));
}

// the device copy of the work list (mfma_plan.hpp: sym_worklist), cached in the context by its key
static int sym_worklist_cached(covgram_ctx* ctx, int64_t ntile, int tpp, int64_t tchunk, int pfirst, int pstride) {
    CG_REQUIRE(sym_list_in_range(ntile, tpp, tchunk, pfirst, pstride), COVGRAM_EUNSUPPORTED, "dense_mfma_sym: work list out of range");
    const int64_t key[4] = {ntile, tchunk * 16 + tpp, pfirst, pstride};
    if (ctx->sym_map != nullptr && memcmp(ctx->sym_key, key, sizeof(key)) == 0) return COVGRAM_OK;
    const std::vector<int32_t> list = sym_worklist(ntile, tpp, tchunk, pfirst, pstride);
    if (list.size() > ctx->sym_map_cap) {
        if (ctx->sym_map) { CG_CHECK_HIP(hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->sym_map); ctx->sym_map = nullptr; }
        ctx->sym_map_cap = std::max<size_t>(list.size(), 4096);
        CG_CHECK_HIP(hipMalloc((void**)&ctx->sym_map, ctx->sym_map_cap * sizeof(int32_t)));
    } else if (ctx->sym_map) {
        CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));       // a launch in flight may still read the old list
    }
    if (!list.empty()) CG_CHECK_HIP(hipMemcpy(ctx->sym_map, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    memcpy(ctx->sym_key, key, sizeof(key));
    ctx->sym_map_len = list.size();
    return COVGRAM_OK;
}

// the EQ form's instance of (split, K2): FAM = FAM_EQFAST / FAM_EQFAST_H; false: not compiled
template <int FAM, int K2>
static bool eq_sym_launch(const covgram_ctx* ctx, const MfmaArgs& a, const SymForm& f) {
    constexpr bool H = FAM == FAM_EQFAST_H;
    const KParams<float> kp{};
    if constexpr (K2 <= MFMA_NARROW_MAXK2) {
        if (f.rt == 2) {   // 8-tile stages at K2 <= 2 (option "mfma_sym_st" = 4: four)
            if constexpr (K2 <= 2) { if (ctx->mfma_sym_st != 4) { mfma_sym_launch<dense_mfma_sym2_kernel<FAM, K2, 8>, 256>(a, kp); return true; } }
            mfma_sym_launch<dense_mfma_sym2_kernel<FAM, K2, 4>, 256>(a, kp);
        } else mfma_sym_launch<dense_mfma_sym_kernel<FAM, K2>, 512>(a, kp);
    } else if constexpr (H && (K2 == 6 || K2 == 8)) {
        if (f.staged_wide) mfma_sym_launch<dense_mfma_sym_kernel<FAM, K2>, 512>(a, kp);
        else mfma_sym_launch<dense_mfma_sym_wide_kernel<FAM, K2>, 256>(a, kp);
    } else if constexpr (!H && K2 == 6) mfma_sym_launch<dense_mfma_sym_kernel<FAM, K2>, 512>(a, kp);
    else if constexpr (!H) mfma_sym_launch<dense_mfma_sym_wide_kernel<FAM, K2>, 256>(a, kp);
    else return false;
    return true;
}

// y <- alpha * scale * G_part a + beta * y for the symmetric Gramian of ONE point set and one right-hand side, where G_part
// holds the entries (i, j), (j, i) whose upper-triangle tile lies in the panels pfirst, pfirst + pstride, ... — all of G
// for (0, 1); the partial products of the ranks (g, P), g < P, add up to G a (covgram_mvm_sym_partial).
// kgen == nullptr: the EQ form (hk is the dense EQ parameter block); else the generic form for kernel *kgen.  The two differ in where the
// fragments come from, in the EF pointer and in the launcher.
int mvm_eq_mfma_sym(covgram_ctx* ctx, const HostKernel& hk, const covgram_points* X, const float* a, float* y, double alpha, double beta,
                    int pfirst, int pstride, const covgram_kernel* kgen) {
    const bool fast = kgen == nullptr;
    HostKernel hkg;
    if (!fast) {   // gamma = 1/l and the profile sees s / l^2 — EQ / MaternP: the folded block (dense_mfma.hpp: mfma_folded)
        int rcg = make_host_kernel(kgen, COVGRAM_F32, !(kgen->family == COVGRAM_EQ || kgen->family == COVGRAM_MATERNP), &hkg);
        if (rcg) return rcg;
    }
    const HostKernel& hku = fast ? hk : hkg;
    const int64_t n = X->n, ntile = (n + 31) / 32;
    // 1. kernel and split
    const SymForm f = sym_form(ctx, hku, X, fast);
    ctx->last_mfma_f16 = f.fmt;
    CG_REQUIRE(f.K2 > 0, COVGRAM_EUNSUPPORTED, "dense_mfma_sym: d = %d has no matrix-core instance", X->d);
    MfmaArgs ma{};
    ma.X = (const float*)X->dptr; ma.n = n; ma.d = X->d; ma.ntile = ntile; ma.ldy = n; ma.nrhs = 1; ma.alpha = 1.0f; ma.beta = 0.0f; ma.final_store = 0;
    ma.K2 = f.K2; ma.RT = 1; ma.NR = 1; ma.hk = &hku; ma.stream = ctx->stream; ma.Cn = (const float*)X->center;
    ma.sym = 1; ma.pfirst = pfirst; ma.pstride = pstride; ma.fmt = f.fmt; ma.sym_rt = f.rt;
    // slab row stride: rows of R / S one panel apart must not sit a power of two apart (n = 49152: 192 KB stride, every panel's
    // stores to the same columns hit the same memory channel: 1.46 ms instead of 0.25); + 4.25 KB staggers them
    ma.npad = sym_panels(ntile, f.tpp) * 32 * f.tpp + 1088;
    // 2. fragments and weights
    int rc;
    if (fast) {
        // the fragments AND the fraction factors e_j are cached in the points handle; the kernel forms a_j e_j itself, so a
        // steady-state MVM launches no pack kernel
        ma.g = (float)(sqrt(LOG2E) / hk.k.lengthscale);
        rc = eq_fragments(ctx, X, f.K2, ma.g, ma.Cn, &ma.PB, &ma.EF, f.fmt);
        ma.W = a;
    } else {
        float* Wg = nullptr;
        rc = gen_fragments(ctx, X, a, n, 1, 1, f.K2, f.gam, hku.k.trait == COVGRAM_ISOTROPIC, f.fmt, 0, &ma.PB, &Wg);
        ma.W = Wg;
    }
    if (rc) return rc;
    // 3. column chunks, the row-sum slab R (one row per chunk) and the column-sum slab S (one row per local panel)
    ma.tchunk = sym_tchunk(ctx, f, ntile, pstride);
    void *Rp, *Sp;
    rc = ws_reserve(ctx, 1, (size_t)sym_chunks(ntile, ma.tchunk) * ma.npad * sizeof(float), &Rp); if (rc) return rc;
    rc = ws_reserve(ctx, 4, (size_t)std::max<int64_t>(sym_local_panels(ntile, f.tpp, pfirst, pstride), 1) * ma.npad * sizeof(float), &Sp); if (rc) return rc;
    ma.R = (float*)Rp; ma.S = (float*)Sp;
    // 4. work list
    rc = sym_worklist_cached(ctx, ntile, f.tpp, ma.tchunk, pfirst, pstride);
    if (rc) return rc;
    ma.wgmap = ctx->sym_map;
    ma.grid = dim3((unsigned)std::max<size_t>(ctx->sym_map_len, 1));
    // 5. launch
    {
        TimerScope tm(ctx);
        ctx->last_mfma_instance = fast ? -(int64_t)(f.K2 * 10 + f.fmt) : 0;
        ctx->last_mfma_sym_rt = f.rt;
        if (fast) {
            bool compiled = false;
            mfma_for_k2(f.K2, [&](auto k) {
                constexpr int K = decltype(k)::value;
                compiled = f.fmt ? eq_sym_launch<FAM_EQFAST_H, K>(ctx, ma, f) : eq_sym_launch<FAM_EQFAST, K>(ctx, ma, f);
            });
            CG_REQUIRE(compiled, COVGRAM_EUNSUPPORTED, f.fmt ? "dense_mfma_sym: K2 = %d not compiled for the fp16 split" : "dense_mfma_sym: K2 = %d not compiled", f.K2);
        } else {
            mfma_launch_fn launch = mfma_launcher(f.lfam);
            CG_REQUIRE(launch != nullptr, COVGRAM_EUNSUPPORTED, "dense_mfma_sym: family %d has no matrix-core path", f.lfam);
            rc = launch(ma, false);
            if (rc) return rc;
        }
    }
    // 6. reduce
    hipLaunchKernelGGL(dense_mfma_sym_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(1024), 0, ctx->stream, n, (const float*)Rp,
                       (const float*)Sp, ma.npad, ntile, (int)ma.tchunk, ma.EF, y, (float)(alpha * hku.kp.scale), (float)beta, pfirst, pstride, f.tpp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("dense_mfma_sym launch failed: %s", hipGetErrorString(e)); return COVGRAM_EHIP; }
    return COVGRAM_OK;
}

// ---- generic profiles / several right-hand sides (dense_mfma.hpp) --------------------
// y[:, 0..nrhs) <- alpha * scale * G a + beta * y (device pointers, column-major with lda / ldy)
int mvm_mfma_gen(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const float* a, int64_t lda,
                 float* y, int64_t ldy, int32_t nrhs, double alpha, double beta) {
    HostKernel hk;
    // gamma = 1/l and the profile sees s / l^2 — EQ / MaternP: the folded block (dense_mfma.hpp: mfma_folded)
    int rc = make_host_kernel(k, COVGRAM_F32, !(k->family == COVGRAM_EQ || k->family == COVGRAM_MATERNP), &hk);
    if (rc) return rc;
    const int64_t n = X->n, m = Y->n;
    const bool iso = hk.k.trait == COVGRAM_ISOTROPIC;
    const int64_t ntile = (m + 31) / 32;
    float gam;
    const int lfam = mfma_family_of(ctx, hk, &gam);
    int K2h = 0;
    const int gfmt = mfma_gen_fmt(ctx, hk, lfam, X, Y, 8, &K2h);        // the VALU forms (up to four right-hand sides): their split and MFMAs per tile
    const int K2m = mfma_k2_for(X->d + (iso ? 1 : 0));                   // the many-column GEMM form keeps bf16, with this many MFMAs per tile
    ctx->last_sum_fused = lfam == FAM_SUM_ISO ? 1 : 0;
    mfma_launch_fn launch = mfma_launcher(lfam);
    const double alpha_eff = alpha * hk.kp.scale;
    MfmaArgs ma{};
    ma.X = (const float*)X->dptr; ma.n = n; ma.d = X->d; ma.ntile = ntile; ma.ldy = ldy; ma.alpha = (float)alpha_eff; ma.beta = (float)beta;
    ma.hk = &hk; ma.stream = ctx->stream; ma.Cn = (const float*)Y->center;
    // plan, slab and grid of one launch over `rows` rows per wave and `nrpad` output columns per chunk
    auto plan = [&](int rows, int64_t target, int nrpad, float* y_c, ColumnPlan* pl) {
        *pl = plan_columns(n, ntile, rows, ctx->target_wgs > 0 ? ctx->target_wgs : target, ctx->jsplit, 8);
        ma.npad = pl->npad; ma.tchunk = pl->tchunk; ma.final_store = pl->js == 1 ? 1 : 0;
        ma.grid = dim3((unsigned)pl->rowtiles, (unsigned)pl->js);
        return split_out(ctx, *pl, nrpad, y_c, &ma.out);
    };
    int cdone = 0;
    // many right-hand sides: blocks of up to 64 on the fp32 matrix cores (dense_mfma_mrhs_kernel).  Its time is flat up to 32 columns
    // (n = 32768: 0.76 ms EQ, 0.86 ms MaternP(2)); the VALU form steps up every four columns (EQ d = 3: 0.29 / 0.56 / 0.81 ms at 4 / 8 /
    // 12; MaternP(2): 0.48 / 0.94 / 1.40): the crossover is 9 columns for the cheap profiles at d <= 3, 5 otherwise —
    // option "mfma_mrhs": -1 this rule, 0 never, 1 from 2 columns (tests)
    const bool cheap = K2m <= 2 && (hk.tu_family == COVGRAM_EQ || hk.tu_family == COVGRAM_CAUCHY || hk.tu_family == COVGRAM_IMQ ||
                                    hk.tu_family == COVGRAM_DOT || hk.tu_family == COVGRAM_EXPDOT);
    const int mrhs_min = ctx->mfma_mrhs == 1 ? 2 : (cheap ? 9 : 5);
    while (nrhs - cdone >= mrhs_min && ctx->mfma_mrhs != 0) {
        const int c0 = cdone;
        const int nr = std::min(64, nrhs - c0);
        const int NB = nr > 32 ? 2 : 1;
        float* y_c = y + (size_t)c0 * ldy;
        float* Wd;                                                   // the pack kernel's weight output: unused here; the A operands sit behind it
        rc = gen_fragments(ctx, Y, a, lda, 0, 1, K2m, gam, iso, 0, (size_t)ntile * NB * 64 * 16 * sizeof(float), &ma.PB, &Wd);
        if (rc) return rc;
        float* AP = Wd + ntile * 32;
        const int64_t ae = ntile * NB * 64 * 16;
        hipLaunchKernelGGL(mfma_pack_rhs_kernel, dim3((unsigned)((ae + 255) / 256)), dim3(256), 0, ctx->stream, a, lda, c0 + nr, c0, m, AP, NB);
        ColumnPlan pl;
        rc = plan(32, (int64_t)ctx->num_cus * 32, 32 * NB, y_c, &pl);   // the fp32 MFMAs bound this kernel: 2 rounds of 4 waves per SIMD
        if (rc) return rc;
        ma.K2 = K2m; ma.NR = 32 * NB; ma.RT = 1; ma.mrhs = NB; ma.fmt = 0; ma.lds = 0; ma.W = AP; ma.nrhs = nr;
        { TimerScope tm(ctx); rc = launch(ma, false); }
        if (rc) return rc;
        if (pl.js > 1) reduce_split(ctx, ma.out, pl, 32 * NB, y_c, n, ldy, nr, alpha_eff, beta);
        cdone += nr;
    }
    const int K2 = gfmt ? K2h : K2m;                                     // (mfma_gen_fmt returned the fp16 split's MFMAs per tile)
    ctx->last_mfma_f16 = gfmt;
    for (int c0 = cdone; c0 < nrhs; c0 += 4) {
        const int nr = std::min(4, nrhs - c0);
        const int NR = nr == 1 ? 1 : 4;
        float* y_c = y + (size_t)c0 * ldy;
        float* W;
        rc = gen_fragments(ctx, Y, a + (size_t)c0 * lda, lda, nr, NR, K2, gam, iso, gfmt, 0, &ma.PB, &W);
        if (rc) return rc;
        ma.K2 = K2; ma.NR = NR; ma.fmt = gfmt; ma.mrhs = 0; ma.lds = 0; ma.W = W; ma.nrhs = nr;
        ma.RT = (NR == 1 && K2 <= 4 && ctx->rows_per_lane != 1) ? 2 : 1;
        const int nb = launch(ma, true);
        // (the 64-tiles-per-wave stop of mvm_eq_mfma does not carry over: these profiles cost several times EQ's per tile, so a wave's fixed
        //  costs amortise over far fewer tiles — tools/rect_sweep.py, MaternP(2) 4096 x 65536: 32 splits 156 us, 128-256 splits 120-127 us)
        ColumnPlan pl;
        rc = plan(32 * ma.RT, (int64_t)ctx->num_cus * nb * 4, NR, y_c, &pl);
        if (rc) return rc;
        // long fragments (d > 8) and long column chunks: four waves share every column tile through LDS, one tile per stage
        // (tools/mfma_lds_ab.py <kernel>: 11-28 % faster at d = 12 .. 24; at d <= 8 the barrier per tile costs 5-18 %, so not there)
        ma.lds = (ctx->mfma_lds == 1 || (ctx->mfma_lds < 0 && K2 > 4 && pl.tchunk >= MFMA_LDS_MIN_TILES && pl.rowtiles >= 64)) ? 1 : 0;
        ctx->last_mfma_lds = ma.lds;
        { TimerScope tm(ctx); rc = launch(ma, false); }
        if (rc) return rc;
        if (pl.js > 1) reduce_split(ctx, ma.out, pl, NR, y_c, n, ldy, nr, alpha_eff, beta);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("dense_mfma launch failed: %s", hipGetErrorString(e)); return COVGRAM_EHIP; }
    return COVGRAM_OK;
}

}  // namespace covgram
