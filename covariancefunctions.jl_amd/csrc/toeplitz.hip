// toeplitz.hip — O(N log N) MVM with SymmetricToeplitz / Toeplitz / Circulant Gramians.
//
// Reference: gramian(k, x::StepRangeLen, y::StepRangeLen) builds SymmetricToeplitz(k.(x[1], x)),
// Toeplitz(k.(x, y[1]), k.(x[1], y)) or Circulant(k.(x[1], x)) (src/gramian.jl:167-189); the MVM itself
// is ToeplitzMatrices 0.7.1 (+ FFTW 1.5.0), a third-party dependency whose source is not part of the
// reference tree.  Its published algorithm is restated here: embed T (n×m) in an N×N circulant
// C with first column  c = [vc_0 .. vc_{n-1}, 0 .., vr_{m-1} .. vr_1], then  T a = (C [a; 0])_{0..n-1}
// = irfft(rfft(c) ⊙ rfft([a; 0])).  Any N >= n+m-1 gives the identical product, so N is the next
// power of two (real-to-complex rocFFT, half the traffic of the complex transform the reference uses),
// and — unlike the reference, which re-plans and re-transforms c on every mul! — the plan and the
// spectrum of c (pre-divided by N) are cached in the handle.
//
// HBM-bound: per MVM one pad pass, R2C, one pointwise pass, C2R, one epilogue pass.
#include <rocfft/rocfft.h>

#include <algorithm>
#include <vector>

#include "driver.hpp"
#include "toeplitz_kernels.hpp"

namespace covgram {

static int g_rocfft_users = 0;

#define CG_CHECK_FFT(expr)                                                                     \
    do {                                                                                       \
        rocfft_status _s = (expr);                                                             \
        if (_s != rocfft_status_success) {                                                     \
            ::covgram::set_error("%s failed: rocfft_status %d (%s:%d)", #expr, (int)_s, __FILE__, __LINE__); \
            return COVGRAM_EHIP;                                                               \
        }                                                                                      \
    } while (0)

}  // namespace covgram

using namespace covgram;

struct covgram_toeplitz {
    covgram_ctx* ctx = nullptr;
    int64_t n = 0, m = 0, N = 0;
    int32_t dtype = 0;
    bool circulant = false;
    rocfft_plan fwd = nullptr, inv = nullptr;
    rocfft_execution_info info = nullptr;
    void* work = nullptr; size_t work_bytes = 0;
    void* spec = nullptr;   // (N/2+1) complex, cached, pre-divided by N
    void* rbuf = nullptr;   // N reals
    void* cbuf = nullptr;   // (N/2+1) complex
    // fast path (four-step FFT without transposes): M = N/2 = 1024 * Mp
    bool fast = false;
    int64_t Mp = 0;
    rocfft_plan bfwd = nullptr, binv = nullptr;   // 1024 contiguous length-Mp complex transforms, in place
    void* zbuf = nullptr;    // M complex
    void* sperm = nullptr;   // M + 1 complex: permuted half spectrum of the embedding / M, Nyquist bin last
    int n1 = 1024;             // column length of the four-step split: M = n1 x Mp (512, 1024 or 2048 — whichever makes Mp a power of four <= 4096)
    bool sperm16_real = false; // sperm16 holds real parts only (symmetric matrix)
    void* sperm16 = nullptr; // M' = 4096: the same rows with their entries at the base-16 digit-reversed index (rowfft16_fused_kernel)
    void* tables = nullptr;  // tw1024 | tlo(2048) | thi(M/2048) | tA(1024) | tB(Mp)   (complex)
};


namespace covgram {

// Columns per tile.  64-byte row segments (half a cache line) so that a tile + the stage twiddles take 80 KiB of LDS and TWO
// workgroups share a CU: one tile's HBM phases overlap the other's LDS butterfly stages.  The two tiles that split each
// 128-byte line are mapped to workgroups b and b+8, which the dispatcher places on the same XCD (same L2) back to back.
template <typename T> constexpr int colfft_tw() { return sizeof(T) == 8 ? 4 : 8; }

// complex tables for the fast path, computed in long double on the host
template <typename T>
static void fill_tables(std::vector<T>& h, int64_t M, int64_t Mp, int n1) {
    const long double PI = 3.14159265358979323846264338327950288L;
    const int64_t nhi = M >> TWID_LB;
    h.resize(2 * (size_t)(n1 + (1 << TWID_LB) + nhi + n1 + Mp + Mp / 4 + Mp));
    size_t o = 0;
    auto put = [&](long double ang) { h[o++] = (T)cosl(ang); h[o++] = (T)sinl(ang); };
    for (int t = 0; t < n1; ++t) put(-2 * PI * t / n1);                               // tw[t]     = W_n1^t (n1 = column length)
    for (int l = 0; l < (1 << TWID_LB); ++l) put(-2 * PI * l / (long double)M);        // tlo[l]    = W_M^l
    for (int64_t q = 0; q < nhi; ++q) put(-2 * PI * q / (long double)nhi);             // thi[q]    = W_M^(2048 q)
    for (int k1 = 0; k1 < n1; ++k1) put(-PI * k1 / (long double)M);                    // tA[k1]    = exp(-i pi k1 / M)
    for (int64_t kp = 0; kp < Mp; ++kp) put(-PI * kp / (long double)Mp);               // tB[k']    = exp(-i pi 1024 k' / M)
    for (int64_t r = 0; r < Mp / 4; ++r) put(-2 * PI * r / (long double)Mp);           // twr[r]    = W_M'^r (quarter table)
    for (int64_t p = 0; p < Mp; ++p) {                                                 // tB16[p]   = tB[rev16(p)] (M' = 4096 only)
        const int64_t kp = (Mp == 4096) ? (((p & 0xF) << 8) | (p & 0xF0) | ((p >> 8) & 0xF)) : p;
        put(-PI * kp / (long double)Mp);
    }
}

struct FastTables { const void *tw, *tlo, *thi, *tA, *tB, *twr, *tB16; };
static FastTables table_ptrs(const covgram_toeplitz* Tz) {
    const size_t cs = 2 * dtype_size(Tz->dtype);
    const char* b = (const char*)Tz->tables;
    const int64_t M = Tz->N / 2, nhi = M >> TWID_LB;
    FastTables t;
    t.tw = b; b += cs * Tz->n1;
    t.tlo = b; b += cs * (1 << TWID_LB);
    t.thi = b; b += cs * nhi;
    t.tA = b; b += cs * Tz->n1;
    t.tB = b; b += cs * Tz->Mp;
    t.twr = b; b += cs * (Tz->Mp / 4);
    t.tB16 = b;
    return t;
}

// the column FFT of the fast path, either direction (option toeplitz_colfft: 16 = colfft16_kernel, default; 4 = colfft_kernel)
template <typename T, bool INV>
static void launch_colfft(covgram_toeplitz* Tz, const FastTables& t, const T* src, int64_t len, T* y, int64_t n, T alpha, T beta) {
    using V = typename V2T<T>::type;
    using std::integral_constant;
    constexpr int TW = colfft_tw<T>();
    hipStream_t st = Tz->ctx->stream;
    const dim3 grid((unsigned)(Tz->Mp / TW));
    auto col16 = [&](auto rr) {
        constexpr int R = decltype(rr)::value;
        hipLaunchKernelGGL((colfft16_kernel<T, TW, INV, R>), grid, dim3(16 * R * TW), 0, st, src, len, (V*)Tz->zbuf, Tz->Mp, (const V*)t.tw, (const V*)t.tlo,
                           (const V*)t.thi, y, n, alpha, beta);
    };
    if (Tz->n1 == 512) col16(integral_constant<int, 2>{});
    else if (Tz->n1 == 2048) col16(integral_constant<int, 8>{});
    else if (Tz->ctx->toeplitz_colfft != 4) col16(integral_constant<int, 4>{});
    else
        hipLaunchKernelGGL((colfft_kernel<T, TW, INV>), grid, dim3(COLFFT_THREADS), 0, st, src, len, (V*)Tz->zbuf, Tz->Mp,
                           (const V*)t.tw, (const V*)t.tlo, (const V*)t.thi, y, n, alpha, beta);
}

// zbuf <- permuted packed spectrum of the real signal src[0..len) (zero beyond), length N
template <typename T>
static int fast_forward(covgram_toeplitz* Tz, const T* src, int64_t len) {
    const FastTables t = table_ptrs(Tz);
    launch_colfft<T, false>(Tz, t, src, len, (T*)nullptr, (int64_t)0, (T)0, (T)0);
    void* io[1] = {Tz->zbuf};
    CG_CHECK_FFT(rocfft_execute(Tz->bfwd, io, nullptr, Tz->info));
    return COVGRAM_OK;
}

template <typename T>
static int fast_mvm(covgram_toeplitz* Tz, const T* a, T* y, double alpha, double beta) {
    using V = typename V2T<T>::type;
    using std::integral_constant;
    const FastTables t = table_ptrs(Tz);
    hipStream_t st = Tz->ctx->stream;
    int L = 0;
    for (int l = 3; l <= 6; ++l) if (Tz->Mp == ((int64_t)1 << (2 * l))) L = l;
    const bool fused = L && Tz->ctx->toeplitz_fused;
    if (fused) {
        // column FFT -> [row FFT, spectral step, inverse row FFT] in one kernel -> inverse column FFT: three passes over zbuf
        launch_colfft<T, false>(Tz, t, a, Tz->m, (T*)nullptr, (int64_t)0, (T)0, (T)0);
        const dim3 fg(Tz->n1 / 2);
        if (L == 6 && Tz->ctx->toeplitz_fused != 2)   // M' = 4096: radix-16 stages (option toeplitz_fused = 2 keeps the radix-4 kernel: A/B)
        {
            // round 4: persistent workgroups (one per CU) with the next row pair prefetched into registers (option toeplitz_persist: -1 = fp64
            // only, 0 = never, 1 = always, k > 1 = with k workgroups).  tools/c5_persist_ab.py / c5_stagger_ab.py, profiles/r04_c5_persist_ab.txt:
            // fp64 87.6 -> 85.3 us, results bit-identical; fp32 61.2 -> 65.3 (at 177 VGPRs the kernel loses its second workgroup per CU).  The
            // pass is NOT short of load / compute / store overlap between workgroups: a late start of half the grid only adds its delay, and
            // the fp32 kernel takes as long as the fp64 one on half the bytes — a workgroup's own chain (one round trip in, six butterfly stages
            // of ~2900 DP instructions per thread at two waves per SIMD, twelve barriers, one round trip out) is what a pair costs.
            const bool persist = Tz->ctx->toeplitz_persist > 0 || (Tz->ctx->toeplitz_persist < 0 && sizeof(T) == 8);
            const dim3 pg((unsigned)std::min<int64_t>(Tz->n1 / 2, Tz->ctx->toeplitz_persist > 1 ? Tz->ctx->toeplitz_persist : Tz->ctx->num_cus));
            by_bool(Tz->sperm16_real, [&](auto reals) {
                by_bool(persist, [&](auto pers) {
                    hipLaunchKernelGGL((rowfft16_fused_kernel<T, decltype(reals)::value, decltype(pers)::value>), decltype(pers)::value ? pg : fg, dim3(512), 0,
                                       st, (V*)Tz->zbuf, (const V*)Tz->sperm, (const V*)t.tA, (const V*)t.tB, (const V*)t.twr, (const void*)Tz->sperm16,
                                       (const V*)t.tB16, Tz->n1);
                });
            });
        } else {
            auto row4 = [&](auto ll) {
                constexpr int LL = decltype(ll)::value;
                hipLaunchKernelGGL((rowfft_fused_kernel<T, LL>), fg, dim3((1 << (2 * LL)) / 4), 0, st, (V*)Tz->zbuf, (const V*)Tz->sperm, (const V*)t.tA,
                                   (const V*)t.tB, (const V*)t.twr, Tz->n1);
            };
            switch (L) {
                case 3: row4(integral_constant<int, 3>{}); break;
                case 4: row4(integral_constant<int, 4>{}); break;
                case 5: row4(integral_constant<int, 5>{}); break;
                default: row4(integral_constant<int, 6>{}); break;
            }
        }
    } else {
        int rc = fast_forward<T>(Tz, a, Tz->m);
        if (rc) return rc;
        const int64_t pairs = (int64_t)(Tz->n1 / 2 + 1) * Tz->Mp;
        hipLaunchKernelGGL(spectral_kernel<T>, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, (V*)Tz->zbuf, Tz->Mp, (const V*)Tz->sperm,
                           (const V*)t.tA, (const V*)t.tB, Tz->n1);
        void* io[1] = {Tz->zbuf};
        CG_CHECK_FFT(rocfft_execute(Tz->binv, io, nullptr, Tz->info));
    }
    launch_colfft<T, true>(Tz, t, (const T*)nullptr, (int64_t)0, y, Tz->n, (T)alpha, (T)beta);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("toeplitz %s path launch failed: %s", fused ? "fused" : "fast", hipGetErrorString(e)); return COVGRAM_EHIP; }
    return COVGRAM_OK;
}

// the fast path's tables on the device; a failure reports the HIP call as covgram_toeplitz_create always named it
template <typename T>
static int upload_tables(covgram_toeplitz* Tz, int64_t Mh) {
    std::vector<T> h;
    fill_tables<T>(h, Mh, Tz->Mp, Tz->n1);
    const char* tn = sizeof(T) == 8 ? "double" : "float";
    hipError_t e = hipMalloc(&Tz->tables, h.size() * sizeof(T));
    if (e != hipSuccess) { set_error("hipMalloc(&T->tables, h.size() * sizeof(%s)) failed: %s", tn, hipGetErrorString(e)); return COVGRAM_EHIP; }
    e = hipMemcpy(Tz->tables, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_error("hipMemcpy(T->tables, h.data(), h.size() * sizeof(%s), hipMemcpyHostToDevice) failed: %s", tn, hipGetErrorString(e)); return COVGRAM_EHIP; }
    return COVGRAM_OK;
}

}  // namespace covgram

static int64_t next_pow2(int64_t v) { int64_t p = 1; while (p < v) p <<= 1; return p; }

extern "C" {

int covgram_toeplitz_destroy(covgram_toeplitz* T) {
    if (!T) return COVGRAM_OK;
    ::covgram::DeviceGuard _cg_dev(T->ctx->device);
    (void)hipStreamSynchronize(T->ctx->stream);
    if (T->fwd) rocfft_plan_destroy(T->fwd);
    if (T->inv) rocfft_plan_destroy(T->inv);
    if (T->bfwd) rocfft_plan_destroy(T->bfwd);
    if (T->binv) rocfft_plan_destroy(T->binv);
    if (T->info) rocfft_execution_info_destroy(T->info);
    void* bufs[] = {T->work, T->spec, T->rbuf, T->cbuf, T->zbuf, T->sperm, T->sperm16, T->tables};
    for (void* b : bufs) if (b) (void)hipFree(b);
    T->ctx->live_handles--;
    if (--g_rocfft_users == 0) rocfft_cleanup();
    delete T;
    return COVGRAM_OK;
}

int covgram_toeplitz_create(covgram_ctx* ctx, covgram_toeplitz** out, const void* vc, const void* vr, int64_t n, int64_t m,
                            int32_t dtype, int32_t loc, int32_t circulant) {
    CG_REQUIRE(ctx && out && vc, COVGRAM_EINVAL, "NULL argument");
    CG_REQUIRE(n >= 1, COVGRAM_EINVAL, "toeplitz: n must be >= 1");
    CG_REQUIRE(dtype == COVGRAM_F32 || dtype == COVGRAM_F64, COVGRAM_EINVAL, "unknown dtype %d", dtype);
    if (!vr) m = n;
    CG_REQUIRE(m >= 1, COVGRAM_EINVAL, "toeplitz: m must be >= 1");
    CG_REQUIRE(!(circulant && vr), COVGRAM_EINVAL, "circulant takes a first column only");
    CG_DEVICE(ctx);
    const size_t ts = dtype_size(dtype);
    if (g_rocfft_users++ == 0) rocfft_setup();
    covgram_toeplitz* T = new covgram_toeplitz();
    T->ctx = ctx; T->n = n; T->m = m; T->dtype = dtype; T->circulant = circulant != 0;
    T->N = circulant ? n : next_pow2(std::max<int64_t>(n + m - 1, 2));
    ctx->live_handles++;
    const int64_t N = T->N, NC = N / 2 + 1;
    auto fail = [&](int code) { covgram_toeplitz_destroy(T); return code; };
#define TRY_HIP(e) do { hipError_t _e = (e); if (_e != hipSuccess) { set_error("%s failed: %s", #e, hipGetErrorString(_e)); return fail(COVGRAM_EHIP); } } while (0)
#define TRY_FFT(e) do { rocfft_status _s = (e); if (_s != rocfft_status_success) { set_error("%s failed: rocfft_status %d", #e, (int)_s); return fail(COVGRAM_EHIP); } } while (0)
    const int64_t Mh = N / 2;
    // column length of the four-step split: 1024, or 512 / 2048 when that makes the row length a power of four <= 4096 (the sizes
    // the fused row kernels exist for: N = 2^20, 2^22 take 512 x 1024, 512 x 4096; N = 2^24 takes 2048 x 4096)
    const int64_t twmin = (dtype == COVGRAM_F64 ? colfft_tw<double>() : colfft_tw<float>());
    auto fused_len = [](int64_t mp) { return mp == 64 || mp == 256 || mp == 1024 || mp == 4096; };
    T->n1 = 1024;
    for (int cand : {1024, 512, 2048})
        if (Mh % cand == 0 && fused_len(Mh / cand)) { T->n1 = cand; break; }
    T->fast = !T->circulant && (Mh % T->n1 == 0) && (Mh / T->n1 >= twmin);
    T->Mp = T->fast ? Mh / T->n1 : 0;
    const rocfft_precision prec = (dtype == COVGRAM_F64) ? rocfft_precision_double : rocfft_precision_single;
    TRY_HIP(hipMalloc(&T->rbuf, (size_t)N * ts));
    size_t w1 = 0, w2 = 0;
    if (T->fast) {
        TRY_HIP(hipMalloc(&T->zbuf, (size_t)Mh * 2 * ts));
        TRY_HIP(hipMalloc(&T->sperm, (size_t)(Mh + 1) * 2 * ts));
        size_t blen[1] = {(size_t)T->Mp};
        TRY_FFT(rocfft_plan_create(&T->bfwd, rocfft_placement_inplace, rocfft_transform_type_complex_forward, prec, 1, blen, (size_t)T->n1, nullptr));
        TRY_FFT(rocfft_plan_create(&T->binv, rocfft_placement_inplace, rocfft_transform_type_complex_inverse, prec, 1, blen, (size_t)T->n1, nullptr));
        TRY_FFT(rocfft_plan_get_work_buffer_size(T->bfwd, &w1));
        TRY_FFT(rocfft_plan_get_work_buffer_size(T->binv, &w2));
        if (by_dtype(dtype, [&](auto t0) { return upload_tables<decltype(t0)>(T, Mh); })) return fail(COVGRAM_EHIP);
    } else {
        TRY_HIP(hipMalloc(&T->spec, (size_t)NC * 2 * ts));
        TRY_HIP(hipMalloc(&T->cbuf, (size_t)NC * 2 * ts));
        size_t len[1] = {(size_t)N};
        TRY_FFT(rocfft_plan_create(&T->fwd, rocfft_placement_notinplace, rocfft_transform_type_real_forward, prec, 1, len, 1, nullptr));
        TRY_FFT(rocfft_plan_create(&T->inv, rocfft_placement_notinplace, rocfft_transform_type_real_inverse, prec, 1, len, 1, nullptr));
        TRY_FFT(rocfft_plan_get_work_buffer_size(T->fwd, &w1));
        TRY_FFT(rocfft_plan_get_work_buffer_size(T->inv, &w2));
    }
    T->work_bytes = std::max(w1, w2);
    TRY_FFT(rocfft_execution_info_create(&T->info));
    if (T->work_bytes) {
        TRY_HIP(hipMalloc(&T->work, T->work_bytes));
        TRY_FFT(rocfft_execution_info_set_work_buffer(T->info, T->work, T->work_bytes));
    }
    TRY_FFT(rocfft_execution_info_set_stream(T->info, ctx->stream));

    // first column / row to the device (HOST: copies in workspace slot 1, read by the embedding before this returns)
    void* w = nullptr;
    int rc = ws_reserve(ctx, 1, loc == COVGRAM_HOST ? staged_bytes(n, 1, ts) + staged_bytes(vr ? m : 0, 1, ts) : 0, &w);
    if (rc) return fail(rc);
    char* cur = (char*)w;
    const void *dvc = vc, *dvr = vr;
    int64_t ldv;
    if ((rc = stage_operand(ctx, loc, ts, cur, vc, n, n, 1, &dvc, &ldv))) return fail(rc);
    if (vr && (rc = stage_operand(ctx, loc, ts, cur, vr, m, m, 1, &dvr, &ldv))) return fail(rc);
    if (!dvr) dvr = dvc;   // symmetric: vr = vc
    const unsigned gN = (unsigned)((N + 255) / 256), gC = (unsigned)((NC + 255) / 256);
    const int64_t me = T->circulant ? 1 : m;   // circulant: plain copy of vc (no wrapped row part)
    rc = by_dtype(dtype, [&](auto t0) -> int {
        using S = decltype(t0);
        using V = typename V2T<S>::type;
        hipLaunchKernelGGL(embed_kernel<S>, dim3(gN), dim3(256), 0, ctx->stream, (const S*)dvc, (const S*)dvr, n, me, N, (S*)T->rbuf);
        if (!T->fast) return COVGRAM_OK;
        // permuted half spectrum of the embedding, pre-divided by M (the unnormalised inverse transforms return M * signal)
        const int64_t tot = (int64_t)T->n1 * T->Mp;
        const FastTables ft = table_ptrs(T);
        if (fast_forward<S>(T, (const S*)T->rbuf, N)) return COVGRAM_EHIP;
        hipLaunchKernelGGL(half_spectrum_kernel<S>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, (const V*)T->zbuf, T->Mp, (const V*)ft.tA,
                           (const V*)ft.tB, (V*)T->sperm, (S)1 / (S)Mh, T->n1);
        return COVGRAM_OK;
    });
    if (rc) return fail(rc);
    if (T->fast) {
        if (T->Mp == 4096) {
            const int64_t tot = (int64_t)T->n1 * T->Mp;
            T->sperm16_real = (vr == nullptr) && ctx->toeplitz_real_spectrum != 0;       // c_j = c_(N-j): the spectrum has no imaginary part
            TRY_HIP(hipMalloc(&T->sperm16, (size_t)tot * (T->sperm16_real ? 1 : 2) * ts));
            by_dtype(dtype, [&](auto t0) {
                using S = decltype(t0);
                by_bool(T->sperm16_real, [&](auto reals) {
                    hipLaunchKernelGGL((permute16_kernel<S, decltype(reals)::value>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream,
                                       (const typename V2T<S>::type*)T->sperm, T->sperm16, tot);
                });
            });
        }
        TRY_HIP(hipStreamSynchronize(ctx->stream));
        (void)hipFree(T->rbuf); T->rbuf = nullptr;      // the fast path needs no real scratch buffer per MVM
    } else {
        void* in[1] = {T->rbuf}; void* outb[1] = {T->spec};
        TRY_FFT(rocfft_execute(T->fwd, in, outb, T->info));
        by_dtype(dtype, [&](auto t0) {
            using S = decltype(t0);
            hipLaunchKernelGGL(cmul_kernel<S>, dim3(gC), dim3(256), 0, ctx->stream, (S*)T->spec, (const S*)nullptr, NC, (S)1 / (S)N);
        });
    }
    TRY_HIP(hipStreamSynchronize(ctx->stream));
#undef TRY_HIP
#undef TRY_FFT
    *out = T;
    return COVGRAM_OK;
}

int covgram_toeplitz_mvm(covgram_toeplitz* T, const void* a, void* y, double alpha, double beta, int32_t loc) {
    CG_REQUIRE(T && a && y, COVGRAM_EINVAL, "NULL argument");
    covgram_ctx* ctx = T->ctx;
    CG_DEVICE(ctx);
    const size_t ts = dtype_size(T->dtype);
    const int64_t n = T->n, m = T->m, N = T->N, NC = N / 2 + 1;
    Staged st;
    int rc = st.begin(ctx, loc, ts, a, m, m, y, n, n, 1, beta);
    if (rc) return rc;
    CG_CHECK_FFT(rocfft_execution_info_set_stream(T->info, ctx->stream));
    rc = by_dtype(T->dtype, [&](auto t0) -> int {
        using S = decltype(t0);
        if (T->fast) return fast_mvm<S>(T, (const S*)st.a, (S*)st.y, alpha, beta);
        const unsigned gN = (unsigned)((N + 255) / 256), gC = (unsigned)((NC + 255) / 256), gn = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(pad_kernel<S>, dim3(gN), dim3(256), 0, ctx->stream, (const S*)st.a, m, N, (S*)T->rbuf);
        { void* in[1] = {T->rbuf}; void* ob[1] = {T->cbuf}; CG_CHECK_FFT(rocfft_execute(T->fwd, in, ob, T->info)); }
        hipLaunchKernelGGL(cmul_kernel<S>, dim3(gC), dim3(256), 0, ctx->stream, (S*)T->cbuf, (const S*)T->spec, NC, (S)1);
        { void* in[1] = {T->cbuf}; void* ob[1] = {T->rbuf}; CG_CHECK_FFT(rocfft_execute(T->inv, in, ob, T->info)); }
        hipLaunchKernelGGL(toep_epilogue_kernel<S>, dim3(gn), dim3(256), 0, ctx->stream, (const S*)T->rbuf, (S*)st.y, n, (S)alpha, (S)beta);
        CG_CHECK_HIP(hipGetLastError());
        return COVGRAM_OK;
    });
    return rc ? rc : st.finish();
}

}  // extern "C"
