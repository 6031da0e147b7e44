// api.hip — C-ABI entry points of libcovgram.so (include/covgram.h): errors, context / points handles, options, workspaces, the helpers
// every driver shares (driver.hpp) and the dense MVM driver.  Kernel parameters: kernel_params.hip; Matrix(G) and the block matrices:
// matrix.hip; gradient and Hessian block MVMs: block_mvm.hip.
// Structured MVMs live in toeplitz.hip (Toeplitz / Circulant), kron.hip (Kronecker) and lowrank.hip (low rank).
#include <math.h>
#include <stdarg.h>

#include <algorithm>
#include <vector>

#include "dense_driver.hpp"
#include "dense_sym32.hpp"
#include "dense_bcast.hpp"
#include "dense_wide.hpp"
#include "grad_wide.hpp"
#include "hess_mvm.hpp"
#include "block_matrix.hpp"

namespace covgram {

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ------------------------------------------------------------------------------------------------
// compiled dimension set
// ------------------------------------------------------------------------------------------------
const int kDims[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64};
const int kNumDims = (int)(sizeof(kDims) / sizeof(kDims[0]));

int pad_dim(int d) {
    for (int i = 0; i < kNumDims; ++i)
        if (kDims[i] >= d) return kDims[i];
    return -1;
}

// per-family launchers: one translation unit per family of FAMS (Makefile) and kernel kind — dense_fam.hip (lane-per-row, wide rows),
// grad_fam.hip (lane-per-row, panel path), block_fam.hip (block matrices).  ONE list: declarations and tables are generated from it.
#define COVGRAM_TU_FAMILIES(X, arg) \
    X(0, arg) X(1, arg) X(2, arg) X(3, arg) X(4, arg) X(5, arg) X(6, arg) X(7, arg) X(8, arg) X(9, arg) X(10, arg) X(11, arg) X(12, arg)
#define CG_DECL(n, arg)                                              \
    int launch_dense_family_##n(const DenseArgs&, int dtype);        \
    int launch_dense_wide_family_##n(const DenseArgs&, int dtype);   \
    int launch_grad_family_##n(const GradArgs&, int dtype);          \
    int launch_grad_wide_family_##n(const GradWideArgs&, int dtype); \
    int launch_bm_family_##n(const BlockMatArgs&, int dtype);
COVGRAM_TU_FAMILIES(CG_DECL, )
#undef CG_DECL
#define CG_ENTRY(n, stem) launch_##stem##_family_##n,
#define CG_LAUNCHER(fn_t, fn, stem)                                                  \
    fn_t fn(int family) {                                                            \
        static const fn_t t[] = {COVGRAM_TU_FAMILIES(CG_ENTRY, stem)};               \
        static_assert(sizeof(t) / sizeof(t[0]) == NUM_TU_FAMILIES, "family list");   \
        return (family >= 0 && family < NUM_TU_FAMILIES) ? t[family] : nullptr;      \
    }
CG_LAUNCHER(dense_launch_fn, dense_launcher, dense)
CG_LAUNCHER(dense_launch_fn, dense_wide_launcher, dense_wide)
CG_LAUNCHER(grad_launch_fn, grad_launcher, grad)
CG_LAUNCHER(grad_wide_launch_fn, grad_wide_launcher, grad_wide)
CG_LAUNCHER(bm_launch_fn, block_matrix_launcher, bm)
#undef CG_LAUNCHER
#undef CG_ENTRY
// Hessian and value-gradient-Hessian MVMs (hess_fam.hip) and the Hessian kinds of the block matrix (block_fam.hip): one translation
// unit per family of COVGRAM_HESS_FAMILIES (hess_mvm.hpp); every other family has no launcher
#define CG_DECL(name, n, arg)                                \
    int launch_hess_family_##n(const HessArgs&, int dtype);  \
    int launch_vgh_family_##n(const HessArgs&, int dtype);   \
    int launch_bmh_family_##n(const BlockMatArgs&, int dtype);
COVGRAM_HESS_FAMILIES(CG_DECL, )
#undef CG_DECL
#define CG_CASE(name, n, stem) case name: return launch_##stem##_family_##n;
#define CG_HESS_LAUNCHER(fn_t, fn, stem)                                                  \
    fn_t fn(int family) {                                                                 \
        switch (family) { COVGRAM_HESS_FAMILIES(CG_CASE, stem) default: return nullptr; } \
    }
CG_HESS_LAUNCHER(hess_launch_fn, hess_launcher, hess)
CG_HESS_LAUNCHER(hess_launch_fn, vgh_launcher, vgh)
CG_HESS_LAUNCHER(bm_launch_fn, block_matrix_hess_launcher, bmh)
#undef CG_HESS_LAUNCHER
#undef CG_CASE

int ws_reserve(covgram_ctx* ctx, int slot, size_t bytes, void** out) {
    Workspace& w = ctx->ws[slot];
    if (w.bytes < bytes) {
        if (w.ptr) {
            CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
            CG_CHECK_HIP(hipFree(w.ptr));
            w.ptr = nullptr; w.bytes = 0;
        }
        size_t want = std::max(bytes, (size_t)1 << 20);
        want = (want + 255) & ~(size_t)255;
        hipError_t e = hipMalloc(&w.ptr, want);
        if (e != hipSuccess) { set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e)); return COVGRAM_ENOMEM; }
        w.bytes = want;
    }
    *out = w.ptr;
    return COVGRAM_OK;
}

int unalias_input(covgram_ctx* ctx, const void** a, int64_t* lda, int64_t rows_a, int64_t cols, const void* y, int64_t ldy, int64_t rows_y, size_t ts) {
    if (*a == nullptr || y == nullptr || rows_a <= 0 || rows_y <= 0 || cols <= 0) return COVGRAM_OK;
    const char* a0 = (const char*)*a;
    const char* a1 = a0 + ((size_t)(cols - 1) * (size_t)*lda + (size_t)rows_a) * ts;
    const char* y0 = (const char*)y;
    const char* y1 = y0 + ((size_t)(cols - 1) * (size_t)ldy + (size_t)rows_y) * ts;
    if (!(a0 < y1 && y0 < a1)) return COVGRAM_OK;
    CG_DEVICE(ctx);
    void* w;
    int rc = ws_reserve(ctx, 5, (size_t)rows_a * (size_t)cols * ts, &w);
    if (rc) return rc;
    CG_CHECK_HIP(hipMemcpy2DAsync(w, (size_t)rows_a * ts, *a, (size_t)*lda * ts, (size_t)rows_a * ts, (size_t)cols, hipMemcpyDeviceToDevice, ctx->stream));
    *a = w; *lda = rows_a;
    return COVGRAM_OK;
}

int tickets_reserve(covgram_ctx* ctx, size_t count, unsigned** out) {
    if (ctx->tickets_cap < count) {
        if (ctx->tickets) {
            CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
            CG_CHECK_HIP(hipFree(ctx->tickets));
            ctx->tickets = nullptr; ctx->tickets_cap = 0;
        }
        const size_t want = std::max<size_t>(count, 16384);
        hipError_t e = hipMalloc((void**)&ctx->tickets, want * sizeof(unsigned));
        if (e != hipSuccess) { ctx->tickets = nullptr; set_error("hipMalloc(%zu) failed: %s", want * sizeof(unsigned), hipGetErrorString(e)); return COVGRAM_ENOMEM; }
        CG_CHECK_HIP(hipMemsetAsync(ctx->tickets, 0, want * sizeof(unsigned), ctx->stream));
        ctx->tickets_cap = want;
    }
    *out = ctx->tickets;
    return COVGRAM_OK;
}

std::pair<hipEvent_t, hipEvent_t>* timer_next(covgram_ctx* ctx) {
    if (!ctx->time_kernels) return nullptr;
    if (ctx->timers_used == ctx->timers.size()) {
        if (ctx->timers.size() >= 8192) return nullptr;
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return nullptr;
        ctx->timers.emplace_back(a, b);
    }
    return &ctx->timers[ctx->timers_used++];
}

// staging (driver.hpp) -----------------------------------------------------------------------------
int Staged::begin(covgram_ctx* ctx, int loc, size_t ts, const void* a_in, int64_t lda_in, int64_t rows_a, void* y_in, int64_t ldy_in, int64_t rows_y, int nrhs,
                  double beta) {
    ctx_ = ctx; a = a_in; y = y_in; lda = lda_in; ldy = ldy_in; host_ = nullptr;
    if (loc == COVGRAM_DEVICE) return unalias_input(ctx, &a, &lda, rows_a, nrhs, y_in, ldy_in, rows_y, ts);
    if (loc != COVGRAM_HOST || rows_y <= 0) return COVGRAM_OK;
    void *sa, *sy;
    int rc = ws_reserve(ctx, 2, (size_t)std::max<int64_t>(rows_a, 1) * nrhs * ts, &sa); if (rc) return rc;
    rc = ws_reserve(ctx, 3, (size_t)rows_y * nrhs * ts, &sy); if (rc) return rc;
    if (rows_a > 0)
        CG_CHECK_HIP(hipMemcpy2DAsync(sa, (size_t)rows_a * ts, a_in, (size_t)lda_in * ts, (size_t)rows_a * ts, nrhs, hipMemcpyHostToDevice, ctx->stream));
    if (beta != 0.0)
        CG_CHECK_HIP(hipMemcpy2DAsync(sy, (size_t)rows_y * ts, y_in, (size_t)ldy_in * ts, (size_t)rows_y * ts, nrhs, hipMemcpyHostToDevice, ctx->stream));
    a = sa; y = sy; lda = std::max<int64_t>(rows_a, 1); ldy = rows_y;
    host_ = y_in; host_ld_ = ldy_in; rows_ = rows_y; cols_ = nrhs; ts_ = ts;
    return COVGRAM_OK;
}

int Staged::begin_tile(covgram_ctx* ctx, int loc, size_t ts, void* out, int64_t ldo, int64_t rows, int64_t cols) {
    ctx_ = ctx; y = out; ldy = ldo; host_ = nullptr;
    if (loc != COVGRAM_HOST) return COVGRAM_OK;
    int rc = ws_reserve(ctx, 3, (size_t)rows * cols * ts, &y); if (rc) return rc;
    ldy = rows;
    host_ = out; host_ld_ = ldo; rows_ = rows; cols_ = cols; ts_ = ts;
    return COVGRAM_OK;
}

int Staged::finish() {
    if (!host_) return COVGRAM_OK;
    CG_CHECK_HIP(hipMemcpy2DAsync(host_, (size_t)host_ld_ * ts_, y, (size_t)rows_ * ts_, (size_t)rows_ * ts_, cols_, hipMemcpyDeviceToHost, ctx_->stream));
    CG_CHECK_HIP(hipStreamSynchronize(ctx_->stream));
    return COVGRAM_OK;
}

// ------------------------------------------------------------------------------------------------
int check_pair(const covgram_ctx* ctx, const covgram_points* X, const covgram_points* Y) {
    CG_REQUIRE(ctx && X && Y, COVGRAM_EINVAL, "NULL argument");
    CG_REQUIRE(X->ctx == ctx && Y->ctx == ctx, COVGRAM_EINVAL, "points belong to a different ctx");
    CG_REQUIRE(X->dtype == Y->dtype, COVGRAM_EINVAL, "x and y have different dtypes");
    CG_REQUIRE(X->d == Y->d, COVGRAM_EINVAL, "DimensionMismatch: inputs have to have the same length: %d, %d", X->d, Y->d);
    return COVGRAM_OK;
}

// The direct-difference symmetric kernels (dense_sym_kernel: fp64, 64-row blocks; dense_sym32_kernel: fp32, 64 R-row blocks) on
// gramian(k, x) for `world` ranks (1: the whole triangle in one launch): a single profile without a Power wrapper, d <= 64, and the
// column-sum slab — ceil(row blocks / world) x npad scalars, held in workspace slot 4 for the life of the ctx — within `cap_gib` GiB.
// ONE predicate for covgram_mvm, covgram_mvm_sym_supported and covgram_mvm_sym_partial (the three disagreed on the cap).
struct DenseSymShape { int64_t blk, blocks, mine, npad; size_t slab_bytes; };
static bool dense_sym_shape(const HostKernel& hk, const covgram_points* X, int world, int cap_gib, DenseSymShape* out) {
    if (X->n <= 0 || hk.tu_family >= COVGRAM_NFAMILY || hk.k.power != 1 || world < 1) return false;
    if (X->d > kDims[kNumDims - 1]) return false;
    const int D = pad_dim(X->d);
    if (D < 0 || rows_per_lane_for(D) != 1) return false;
    DenseSymShape sh;
    const bool f64 = X->dtype == COVGRAM_F64;
    sh.blk = f64 ? 64 : 64 * dense_sym32_rows(D);
    sh.blocks = (X->n + sh.blk - 1) / sh.blk;
    sh.mine = (sh.blocks + world - 1) / world;
    sh.npad = f64 ? ((X->n + 63) / 64) * 64 : ((X->n + 511) / 512) * 512;
    sh.slab_bytes = (size_t)sh.mine * (size_t)sh.npad * dtype_size(X->dtype);
    if (sh.slab_bytes > ((size_t)cap_gib << 30)) return false;
    if (out) *out = sh;
    return true;
}

// choose the J split: enough workgroups to fill the chip, chunks aligned to the inner accumulation block
void choose_split(const covgram_ctx* ctx, int64_t rowblocks, int64_t m, int64_t align, int64_t* jchunk, int* jsplit,
                  int64_t default_target) {
    // ~128 single-wave workgroups per CU = 4 rounds of resident waves: measured on C2 (profiles/r01_quickbench_wg64.txt)
    // 3.63 ms at 8 waves per CU, 2.76 ms at 32, 2.63 ms at 64, 2.56 ms at 128 — dynamic rounds even out per-CU speed
    int64_t target = ctx->target_wgs > 0 ? ctx->target_wgs : (default_target > 0 ? default_target : (int64_t)ctx->num_cus * 128);
    int64_t js = ctx->jsplit > 0 ? ctx->jsplit : (target + rowblocks - 1) / std::max<int64_t>(rowblocks, 1);
    const int64_t maxsplit = std::max<int64_t>(1, m / align);
    js = std::max<int64_t>(1, std::min(js, maxsplit));
    int64_t jc = (m + js - 1) / js;
    jc = ((jc + align - 1) / align) * align;
    if (jc <= 0) jc = align;
    js = std::max<int64_t>(1, (m + jc - 1) / jc);
    *jchunk = jc;
    *jsplit = (int)js;
}


// (the conditions are spelled out at SumTerm, driver.hpp)
bool composite_sum_terms(const covgram_ctx* ctx, const covgram_kernel* k, int32_t loc, SumSplit* split) {
    SumTerm* const terms = split->terms;
    double* const constant = &split->constant;
    if (k == nullptr || k->family != COVGRAM_COMPOSITE || ctx->composite_termwise == 0) return false;
    const covgram_kernel_composite* c = (const covgram_kernel_composite*)k;
    if (c->nterms < 1 || c->nterms > COVGRAM_COMPOSITE_MAX_TERMS) return false;
    int nin = 0, nt = 0, nsimple = 0;
    *constant = 0.0;
    for (int t = 0; t < c->nterms; ++t) {
        double coef = c->head.scale;
        int profiles = 0;
        SumTerm& st = terms[nt];
        memset(&st.c, 0, sizeof(st.c));
        for (int f = 0; f < c->nfactors[t]; ++f, ++nin) {
            if (nin >= COVGRAM_COMPOSITE_MAX_FACTORS) return false;
            const covgram_kernel& fk = c->factors[nin];
            if (fk.family == COVGRAM_CONSTANT) { coef *= fk.scale; continue; }
            st.c.factors[profiles++] = fk;
        }
        if (profiles == 0) { *constant += coef; continue; }
        st.simple = profiles == 1;
        if (st.simple) { st.k = st.c.factors[0]; st.k.scale *= coef; ++nsimple; }
        else {
            st.c.head = c->head; st.c.head.scale = coef;
            st.c.nterms = 1; st.c.nfactors[0] = profiles;
        }
        ++nt;
    }
    if (nt == 0) return false;                                 // a profile term goes first: it applies beta
    if (nsimple == 0 && *constant == 0.0) return false;        // products only: one interpreter pass
    if (nsimple == 0 && nt > 1) return false;
    if (*constant != 0.0 && loc != COVGRAM_DEVICE) return false;   // the constant term works on device vectors only
    split->nterms = nt;
    return true;
}

// y[i * ys + r * ldy] += coef * sum_j a[j * as + r * lda]   (as = ys = 1: dense; d + 1: the value row of value-gradient blocks)
template <typename T>
__global__ __launch_bounds__(1024) void const_sum_kernel(const T* __restrict__ a, int64_t m, int64_t lda, int64_t as, T* __restrict__ S) {
    const T* __restrict__ ar = a + (int64_t)blockIdx.x * lda;
    T s = 0;
    for (int64_t j = threadIdx.x; j < m; j += 1024) s += ar[j * as];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    __shared__ T part[16];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        T tot = 0;
        for (int w = 0; w < 16; ++w) tot += part[w];           // fixed order: deterministic
        S[blockIdx.x] = tot;
    }
}
template <typename T>
__global__ __launch_bounds__(256) void const_add_kernel(T* __restrict__ y, int64_t n, int64_t ldy, int64_t ys, const T* __restrict__ S, T coef) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[(int64_t)blockIdx.y * ldy + i * ys] += coef * S[blockIdx.y];
}
int constant_term_mvm(covgram_ctx* ctx, int dtype, const void* a, int64_t m, int64_t lda, int64_t as, void* y, int64_t n, int64_t ldy,
                             int64_t ys, int nrhs, double coef) {
    if (n == 0 || m == 0 || coef == 0.0) return COVGRAM_OK;
    void* S;
    int rc = ws_reserve(ctx, 0, (size_t)nrhs * 8, &S);
    if (rc) return rc;
    const dim3 ag((unsigned)((n + 255) / 256), (unsigned)nrhs);
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(const_sum_kernel<T>, dim3(nrhs), dim3(1024), 0, ctx->stream, (const T*)a, m, lda, as, (T*)S);
        hipLaunchKernelGGL(const_add_kernel<T>, ag, dim3(256), 0, ctx->stream, (T*)y, n, ldy, ys, (const T*)S, (T)coef);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("constant-term kernels failed: %s", hipGetErrorString(e)); return COVGRAM_EHIP; }
    return COVGRAM_OK;
}

const char* const kFamilyNames[COVGRAM_NFAMILY] = {"ExponentiatedQuadratic", "Exponential", "RationalQuadratic", "GammaExponential", "Cauchy",
                                                          "InverseMultiQuadratic", "MaternP", "Dot", "ExponentialDot", "Matern", "AsinDot"};
int hess_refusal(const char* w, const covgram_kernel* k, int d) {
    CG_REQUIRE(k->family != COVGRAM_COMPOSITE, COVGRAM_EUNSUPPORTED, "%s of a composite kernel (Sum / Product / Power) has no device path", w);
    CG_REQUIRE(k->family >= 0 && k->family < COVGRAM_NFAMILY, COVGRAM_EUNSUPPORTED, "unknown kernel family %d", k->family);
    CG_REQUIRE(hess_family_ok(k->family), COVGRAM_EUNSUPPORTED, "%s(%s) has no device path (no closed-form fourth derivative compiled)", w, kFamilyNames[k->family]);
    CG_REQUIRE(k->power == 1, COVGRAM_EUNSUPPORTED, "%s(%s^%d): Power wrappers have no device path", w, kFamilyNames[k->family], k->power);
    CG_REQUIRE(d <= HESS_MAX_D, COVGRAM_EUNSUPPORTED, "%s(%s): d = %d exceeds the compiled maximum %d", w, kFamilyNames[k->family], d, HESS_MAX_D);
    return COVGRAM_OK;
}

// ------------------------------------------------------------------------------------------------
// the dense MVM driver: y <- alpha G a + beta y for ONE kernel (a split Sum arrives term by term) on device-resident a and y that do
// not overlap.  route() decides; one function per route launches it.
// ------------------------------------------------------------------------------------------------
enum DenseKind {
    DENSE_DOT_FACTORED,                   // X (Y' a): lowrank.hip
    DENSE_MFMA_EQ_SYM, DENSE_MFMA_EQ, DENSE_MFMA_GEN_SYM, DENSE_MFMA_GEN,   // fp32 matrix cores: dense_mfma.hip
    DENSE_BCAST,                          // fp64 wide points, expanded distance: dense_bcast.hpp
    DENSE_LANES                           // lane-per-row (dense_mvm.hpp, dense_sym32.hpp) / wide rows (dense_wide.hpp); m = 0: y <- beta y
};
struct DenseMvm {
    // the call
    covgram_ctx* ctx; const covgram_kernel* k; const HostKernel& hk; const covgram_points* X; const covgram_points* Y;
    const void* a; int64_t lda; void* y; int64_t ldy; int nrhs; double alpha, beta;
    int rank, world;                      // covgram_mvm_sym_partial (world > 0): the row blocks rank, rank + world, ... of the symmetric kernel only
    // the decision (route)
    DenseKind kind = DENSE_LANES;
    bool wide = false;                    // d > 64: the chunked kernel
    bool dsym = false;                    // direct-difference symmetric form (DENSE_BCAST, DENSE_LANES): the upper triangle once
    DenseSymShape symsh{};                // dsym: blocks and column-sum slab
    int D = 0;                            // padded dimension
    int64_t rowblocks = 0, npad = 0;      // 64-row blocks of the lane-per-row launches
    const void* Cn = nullptr;             // the column side's centre (isotropic kernels)
    double alpha_eff = 0;
    dense_launch_fn launch = nullptr;

    const int64_t n = X->n, m = Y->n;
    const int dtype = X->dtype;
    const size_t ts = dtype_size(dtype);

    int route();
    int launch_sym(DenseArgs& da, void* y_c, int js0);
    int run_mfma();
    int run_bcast();
    int run_lanes();
    int run() {
        int rc = route();
        if (rc) return rc;
        switch (kind) {
            case DENSE_DOT_FACTORED:
                rc = mvm_dot_factored(ctx, hk, X, Y, a, lda, y, ldy, nrhs, alpha, beta);
                if (rc == COVGRAM_OK) ctx->last_dense_path = 4;
                return rc;
            case DENSE_BCAST: return run_bcast();
            case DENSE_LANES: return run_lanes();
            default: return run_mfma();
        }
    }
};

int DenseMvm::route() {
    // d <= 64: x_i lives in registers (dense_mvm.hpp); beyond that the chunked kernel of dense_wide.hpp (any d)
    wide = X->d > kDims[kNumDims - 1];
    D = wide ? ((X->d + 31) / 32) * 32 : pad_dim(X->d);
    launch = wide ? dense_wide_launcher(hk.tu_family) : dense_launcher(hk.tu_family);
    alpha_eff = alpha * hk.kp.scale;
    const int R = rows_per_lane_for(D);
    const int64_t rows_per_wg = (int64_t)DENSE_THREADS * R;
    rowblocks = (n + rows_per_wg - 1) / rows_per_wg;
    npad = rowblocks * rows_per_wg;
    // isotropic kernels work relative to the column side's centre (common.hpp: covgram_points::center)
    Cn = (hk.k.trait == COVGRAM_ISOTROPIC) ? Y->center : nullptr;
    ctx->last_mfma_sym = 0; ctx->last_dense_bcast = 0; ctx->last_dense_sym = 0;
    // Gramian(Dot(), x, y) = X Y' (src/gramian.jl:23,150-151): the reference goes entry by entry through the generic loop; the
    // product is X (Y' a), two O((n + m) d) streaming passes (lowrank.hip).  dense_variant = 1 / 2 keep the entry-by-entry kernels.
    if (m > 0 && hk.tu_family == COVGRAM_DOT && hk.k.power == 1 && ctx->dense_variant == 0 && world == 0 && (size_t)X->d * (size_t)nrhs * ts <= 65536) {
        kind = DENSE_DOT_FACTORED;
        return COVGRAM_OK;
    }
    bool mfma = true;
    if (m > 0 && mfma_eq_eligible(ctx, hk, X, Y, nrhs)) kind = mfma_eq_sym_eligible(ctx, hk, X, Y, nrhs) ? DENSE_MFMA_EQ_SYM : DENSE_MFMA_EQ;
    else if (m > 0 && mfma_gen_eligible(ctx, hk, X, Y, nrhs))
        kind = mfma_gen_sym_eligible(ctx, hk, X, Y, nrhs) ? DENSE_MFMA_GEN_SYM : DENSE_MFMA_GEN;   // gramian(k, x): upper triangle once, any matrix-core profile
    else mfma = false;
    ctx->last_mfma_sym = (kind == DENSE_MFMA_EQ_SYM || kind == DENSE_MFMA_GEN_SYM) ? 1 : 0;
    if (m > 0) ctx->last_dense_path = mfma ? 2 : (wide ? 3 : 1);
    // fp64 gramian(k, x) * a on the direct-difference path: the upper triangle once (dense_sym_kernel, dense_mvm.hpp).  The same point
    // set on both sides, one right-hand side, a single (non-composite) profile without a Power wrapper, d <= 64; from n = 6144 (16384 for
    // the profiles that cost a reciprocal or less: below that the launch is latency and the triangle's imbalance, not arithmetic —
    // tools/fp64_sym_sweep.py: break-even at n ~ 6000, x1.1-1.25 at 8192, x1.3-1.5 at 16384, x1.5-1.75 from 32768) while the column-sum
    // slab n^2 / 8 bytes — held in workspace slot 4 for the life of the ctx — stays within 1 GiB (n <= 92681) when the choice is automatic,
    // 2 GiB (n <= 131072) when option "dense_sym" = 1 asks for it; R = 1 row per lane (64-row blocks) is what the kernel is written for.
    const bool cheap_profile = hk.tu_family == COVGRAM_CAUCHY || hk.tu_family == COVGRAM_IMQ || hk.tu_family == COVGRAM_DOT;
    // covgram_mvm_sym_partial (direct-difference form): rank r of P evaluates the row blocks r, r + P, ... only (world > 0)
    // fp32 (dense_sym32_kernel, round 4): the same form for what the matrix-core path refuses — Exponential, gamma-exponential, MaternP(0),
    // clouds that fail its radius gate, dense_variant = 1 — from n = 24576 (32768 for the cheap profiles).
    const bool sym_forced = ctx->dense_sym == 1 || world > 0;
    // fp32 break-even measured at n ~ 22000 (profiles/r04_sym32_sweep.txt: x0.85-0.9 at 16384, x1.2-1.5 at 32768, x1.5-1.85 from 65536)
    const int64_t sym_min_n = dtype == COVGRAM_F64 ? (cheap_profile ? 16384 : 6144) : (cheap_profile ? 32768 : 24576);   // fp64, d = 3 (tools/c1_sym_ab.py): n = 4096 31 against 29 us, 6144 42 against 48, 8192 62 against 77
    dsym = !mfma && !wide && m > 0 && nrhs == 1 && (ctx->dense_sym != 0 || world > 0) && X->dptr == Y->dptr && n == m &&
           (sym_forced || n >= sym_min_n) && R == 1 &&
           dense_sym_shape(hk, X, world > 0 ? world : 1, sym_forced ? 2 : 1, &symsh);
    if (world > 0 && !dsym) { set_error("the symmetric direct-difference kernel does not apply to this kernel / point set"); return COVGRAM_EUNSUPPORTED; }
    ctx->last_dense_sym = dsym ? 1 : 0;
    if (mfma) return COVGRAM_OK;
    // fp64, wide points (round 4, dense_bcast.hpp): |x - y|^2 expanded around cached norms — one v_fmac_f64 per dimension and pair instead of
    // a subtraction and an fma, the column records in VGPRs (DPP broadcast) instead of the scalar stream — for the profiles that are smooth
    // in s at 0, one right-hand side, no Power wrapper, inside the expanded form's radius gate (as the gradient kernel's: grad_mvm.hpp).
    // Where the symmetric form applies too (gramian(k, x), n from 6144 / 16384, or covgram_mvm_sym_partial's cyclic row blocks) the two
    // combine: dense_bcast_sym_kernel evaluates the upper triangle once WITH the one-fmac distance (profiles/r04_fp64_dense_d_sweep.txt).
    const bool bc_family = hk.tu_family == COVGRAM_EQ || hk.tu_family == COVGRAM_RQ || hk.tu_family == COVGRAM_CAUCHY || hk.tu_family == COVGRAM_IMQ ||
                           (hk.tu_family == COVGRAM_MATERNP && hk.k.p >= 1);
    const bool dbc = !wide && m > 0 && dtype == COVGRAM_F64 && nrhs == 1 && bc_family && hk.k.power == 1 && dense_bcast_ok(D) &&
                     ctx->dense_bcast != 0 && ctx->dense_variant != 1 &&
                     (ctx->dense_bcast == 1 || (D >= 16 && gate_radius2(X, Y) / (hk.k.lengthscale * hk.k.lengthscale) <= GRAD_EXPAND_GATE));
    ctx->last_dense_bcast = dbc ? 1 : 0;
    kind = dbc ? DENSE_BCAST : DENSE_LANES;
    return COVGRAM_OK;
}

int DenseMvm::run_mfma() {
    const float* af = (const float*)a;
    float* yf = (float*)y;
    switch (kind) {
        case DENSE_MFMA_EQ_SYM: return mvm_eq_mfma_sym(ctx, hk, X, af, yf, alpha, beta);
        case DENSE_MFMA_EQ: return mvm_eq_mfma(ctx, hk, X, Y, af, yf, alpha, beta);
        case DENSE_MFMA_GEN_SYM: return mvm_eq_mfma_sym(ctx, hk, X, af, yf, alpha, beta, 0, 1, k);
        default: return mvm_mfma_gen(ctx, k, X, Y, af, lda, yf, ldy, nrhs, alpha, beta);
    }
}

// gramian(k, x) on the direct-difference symmetric kernels (dense_sym_kernel / dense_bcast_sym_kernel: fp64, dense_sym32_kernel: fp32; the
// cyclic blocks of covgram_mvm_sym_partial included): `da` is the all-entries launch, js0 its column split.  The upper triangle once, the
// column sums into the slab of workspace slot 4, then the kernel's reduce.
int DenseMvm::launch_sym(DenseArgs& da, void* y_c, int js0) {
    const bool f32 = dtype == COVGRAM_F32;
    // fp64: chunks of whole 64-column blocks; about twice the workgroups of the all-entries launch, half of them (left of the diagonal) leave
    // at once.  fp32: 64 R-row blocks (R rows per lane), chunks of whole 512-column inner blocks; ~64 k workgroups, half of them (left of
    // the diagonal) leave at once, so that the triangle's long and short rows even out over several rounds of resident waves
    const int64_t cb = f32 ? 512 : 64;
    const int64_t blocks = (m + cb - 1) / cb;
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(blocks, f32 ? (65536 + symsh.mine - 1) / symsh.mine : 2 * (int64_t)js0));
    const int64_t per = (blocks + want - 1) / want;
    da.jchunk = per * cb;
    da.jsplit = (int)((m + da.jchunk - 1) / da.jchunk);
    da.npad = symsh.npad;
    da.sym = 1;
    if (world > 0) { da.sym_first = rank; da.sym_stride = world; }
    int rc = ws_reserve(ctx, 1, (size_t)da.jsplit * da.npad * ts, &da.out); if (rc) return rc;
    rc = ws_reserve(ctx, 4, symsh.slab_bytes, &da.colslab); if (rc) return rc;
    { TimerScope tm(ctx); rc = launch(da, dtype); }
    if (rc) return rc;
    if (f32)
        hipLaunchKernelGGL(dense_sym32_reduce_kernel<float>, dim3((unsigned)((n + 63) / 64)), dim3(1024), 0, ctx->stream, (const float*)da.out,
                           (const float*)da.colslab, da.npad, da.jsplit, (float*)y_c, n, (float)alpha_eff, (float)beta, da.sym_first, da.sym_stride,
                           (int32_t)symsh.blk);
    else
        hipLaunchKernelGGL(dense_sym_reduce_kernel<double>, dim3((unsigned)rowblocks), dim3(1024), 0, ctx->stream, (const double*)da.out,
                           (const double*)da.colslab, da.npad, da.jsplit, (double*)y_c, n, alpha_eff, beta, da.sym_first, da.sym_stride);
    return COVGRAM_OK;
}

int DenseMvm::run_bcast() {
    const int64_t CB = DENSE_BCAST_CB;
    const int64_t mpad = ((m + CB - 1) / CB) * CB + CB;               // whole blocks + one prefetch-only block
    void* Pb;
    int rc = ws_reserve(ctx, 0, (size_t)mpad * (D + 2) * ts, &Pb); if (rc) return rc;
    double* Exb = (double*)Pb + (size_t)mpad * D;
    // D a power of two: D lanes per column record; else a thread per column
    if (!try_dim(Dims<16, 32, 64>{}, D, [&](auto DL) {
            hipLaunchKernelGGL((dense_bcast_pack_lanes_kernel<decltype(DL)::value>), dim3((unsigned)((mpad * DL() + 255) / 256)), dim3(256), 0, ctx->stream,
                               (const double*)Y->dptr, m, Y->d, (const double*)a, (double*)Pb, Exb, hk.kp.gamma, (const double*)Cn, mpad);
        }))
        hipLaunchKernelGGL(dense_bcast_pack_kernel<double>, dim3((unsigned)((mpad + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)Y->dptr, m, Y->d,
                           (const double*)a, (double*)Pb, Exb, D, hk.kp.gamma, (const double*)Cn, mpad);
    DenseArgs da;
    da.C = Cn; da.X = X->dptr; da.n = n; da.d = X->d; da.P = Pb; da.Ex = Exb; da.m = m; da.ldy = ldy; da.nrhs = 1;
    da.Dpad = D; da.NRpad = 1; da.rows_per_lane = 1; da.variant = 0; da.bcast = 1;
    da.alpha = alpha_eff; da.beta = beta; da.hk = &hk; da.stream = ctx->stream;
    ctx->last_dense_path = 1;
    if (dsym) {
        // gramian(k, x): the upper triangle once on dense_bcast_sym_kernel — 64-row blocks, chunks of whole 64-column blocks, the column-sum
        // slab and the reduce kernel of dense_sym_kernel (covgram_mvm_sym_partial's cyclic blocks included)
        int64_t jchunk; int jsplit;
        choose_split(ctx, rowblocks, m, 64, &jchunk, &jsplit);
        rc = launch_sym(da, y, jsplit);
    } else {
        const int64_t rb256 = (n + 255) / 256;                        // 256-row blocks, about 32 workgroups per CU
        da.npad = rb256 * 256;
        rc = dense_lane_route(ctx, dtype, rb256, da.npad, n, m, 1, 1, (int64_t)ctx->num_cus * 32, false, y, ldy, alpha_eff, beta,
                              [&](int64_t jchunk, int jsplit, void* out, unsigned*) {
                                  da.jchunk = jchunk; da.jsplit = jsplit; da.out = out;
                                  return launch(da, dtype);
                              });
    }
    if (rc) return rc;
    ctx->last_jsplit = da.jsplit;
    return COVGRAM_OK;
}

// up to four right-hand sides per pass
int DenseMvm::run_lanes() {
    const int PKN = (dtype == COVGRAM_F32) ? 2 : 1;      // fp32 packs two columns per stream element
    const bool dsym32 = dsym && dtype == COVGRAM_F32;
    int rc;
    for (int c0 = 0; c0 < nrhs; c0 += 4) {
        const int nr = std::min(4, nrhs - c0);
        const int NRpad = (nr == 1) ? 1 : 4;
        const char* a_c = (const char*)a + (size_t)c0 * lda * ts;
        char* y_c = (char*)y + (size_t)c0 * ldy * ts;
        if (m == 0) { dense_reduce(ctx, dtype, nullptr, npad, NRpad, 0, y_c, n, ldy, nr, 0.0, beta); continue; }   // empty sum: y <- beta * y
        void* P;
        const int PADTO = dsym32 ? 8 : PKN;                 // dense_sym32_kernel reduces eight columns at a time
        int64_t mp = ((m + PADTO - 1) / PADTO) * PADTO;     // stream padded to whole column groups
        if (wide) {                                         // ... or to whole column blocks of the wide kernel
            const int64_t bc = 32 * PKN;
            mp = ((m + bc - 1) / bc) * bc;
        }
        rc = ws_reserve(ctx, 0, (size_t)mp * (D + NRpad) * ts, &P); if (rc) return rc;
        by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            if (wide) {
                const int64_t tot = mp * (int64_t)(D + NRpad);
                hipLaunchKernelGGL(dense_wide_pack_kernel<T>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)Y->dptr, m, Y->d, D,
                                   (const T*)a_c, lda, nr, 0, (T*)P, NRpad, PKN, 32, (T)hk.kp.gamma, (const T*)Cn);
            } else
                hipLaunchKernelGGL(dense_pack_kernel<T>, dim3((unsigned)((mp + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)Y->dptr, m, Y->d, (const T*)a_c,
                                   lda, nr, 0, (T*)P, D, NRpad, PKN, (T)hk.kp.gamma, (const T*)Cn, PADTO);
        });
        DenseArgs da;
        da.C = Cn;
        da.X = X->dptr; da.n = n; da.d = X->d; da.P = P; da.m = m; da.npad = npad; da.ldy = ldy; da.nrhs = nr;
        da.Dpad = D; da.NRpad = NRpad; da.rows_per_lane = rows_per_lane_for(D);
        da.variant = (int)ctx->dense_variant; da.alpha = alpha_eff; da.beta = beta; da.hk = &hk; da.stream = ctx->stream;
        if (dsym) {
            int64_t jchunk; int jsplit;
            choose_split(ctx, rowblocks, m, 64, &jchunk, &jsplit);
            rc = launch_sym(da, y_c, jsplit); if (rc) return rc;
            ctx->last_jsplit = dsym32 ? da.jsplit : jsplit;   // (the fp64 kernel reports the all-entries split it started from)
            continue;
        }
        // chunks are multiples of 64 columns (whole packed pairs); small problems split finer than the 512-column
        // inner accumulation block so that they still expose thousands of waves.
        // The lane-per-row kernel can sum its own split-J slab (last-arriving workgroup of each 64-row block, fixed order: pack.hpp) — only
        // on request: its column splits are fine (64 at C1's size), and 64 tickets on one counter plus the uncached re-read cost more than
        // the launch they save (profiles/r04_inkernel_reduce_ab.txt: C1 27.1 -> 39.0 us, n = 16384 259 -> 262)
        rc = dense_lane_route(ctx, dtype, rowblocks, npad, n, m, nr, NRpad, 0, !wide, y_c, ldy, alpha_eff, beta,
                              [&](int64_t jchunk, int jsplit, void* out, unsigned* tickets) {
                                  ctx->last_jsplit = jsplit;
                                  ctx->last_inkernel_reduce = tickets ? 1 : 0;
                                  da.jchunk = jchunk; da.jsplit = jsplit; da.out = out; da.tickets = tickets; da.yfinal = tickets ? y_c : nullptr;
                                  return launch(da, dtype);
                              });
        if (rc) return rc;
    }
    return COVGRAM_OK;
}

// the product of ONE kernel on device-resident a and y that do not overlap: by the route of DenseMvm, or (split: its Sum split) term by term
static int dense_mvm_run(covgram_ctx* ctx, const covgram_kernel* k, const HostKernel& hk, const SumSplit* split, const covgram_points* X,
                         const covgram_points* Y, const void* a, int64_t lda, void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int rank, int world) {
    if (!split) return DenseMvm{ctx, k, hk, X, Y, a, lda, y, ldy, nrhs, alpha, beta, rank, world}.run();
    return sum_split_run(
        *split, beta,
        [&](const covgram_kernel* tk, double tbeta) {
            HostKernel thk;
            const int trc = make_host_kernel(tk, X->dtype, false, &thk);
            return trc ? trc : DenseMvm{ctx, tk, thk, X, Y, a, lda, y, ldy, nrhs, alpha, tbeta, rank, world}.run();
        },
        [&] { return constant_term_mvm(ctx, X->dtype, a, Y->n, lda, 1, y, X->n, ldy, 1, nrhs, alpha * split->constant); });
}

// covgram_mvm, and (world > 0) the direct-difference form of covgram_mvm_sym_partial: validation, the Sum split, staging
static int dense_mvm(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda, void* y,
                     int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t loc, int rank, int world) {
    int rc = check_pair(ctx, X, Y);
    if (rc) return rc;
    ctx->last_sum_fused = 0;
    CG_REQUIRE(nrhs >= 1, COVGRAM_EINVAL, "nrhs must be >= 1");
    const int64_t n = X->n, m = Y->n;
    CG_REQUIRE(lda >= m && ldy >= n, COVGRAM_EINVAL, "DimensionMismatch: lda=%lld < m=%lld or ldy=%lld < n=%lld",
               (long long)lda, (long long)m, (long long)ldy, (long long)n);
    CG_REQUIRE((a != nullptr || m == 0) && (y != nullptr || n == 0), COVGRAM_EINVAL, "a or y is NULL");
    // (a Sum the one-pass matrix-core kernels take is NOT split: every term shares the pair's distance, as in the reference's
    //  per-pair evaluation src/algebra.jl:27-47 — dense_mfma.hip: sum_fused_applies)
    SumSplit split;
    const bool sum = !sum_fused_applies(ctx, k, X, Y, nrhs) && composite_sum_terms(ctx, k, loc, &split);
    HostKernel hk;
    rc = make_host_kernel(k, X->dtype, false, &hk);     // (a split Sum: the composite's own validation — traits, limits — still applies)
    if (rc) return rc;
    CG_DEVICE(ctx);
    if (n == 0) return COVGRAM_OK;
    // a and y may overlap (include/covgram.h): the kernels below, and every term of a split Sum, read a private copy of a
    Staged st;
    rc = st.begin(ctx, loc, dtype_size(X->dtype), a, lda, m, y, ldy, n, nrhs, beta);
    if (rc) return rc;
    rc = dense_mvm_run(ctx, k, hk, sum ? &split : nullptr, X, Y, st.a, st.lda, st.y, st.ldy, nrhs, alpha, beta, rank, world);
    if (rc) return rc;
    CG_CHECK_HIP(hipGetLastError());
    return st.finish();
}

// (driver.hpp) covgram_mvm's product behind its staging, for a driver that has staged a and y itself (mixed_mvm.hip)
int dense_mvm_on_device(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda, void* y,
                        int64_t ldy, int32_t nrhs, double alpha, double beta) {
    ctx->last_sum_fused = 0;
    SumSplit split;
    const bool sum = !sum_fused_applies(ctx, k, X, Y, nrhs) && composite_sum_terms(ctx, k, COVGRAM_DEVICE, &split);
    HostKernel hk;
    const int rc = make_host_kernel(k, X->dtype, false, &hk);
    if (rc) return rc;
    return dense_mvm_run(ctx, k, hk, sum ? &split : nullptr, X, Y, a, lda, y, ldy, nrhs, alpha, beta, 0, 0);
}

}  // namespace covgram

using namespace covgram;

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

int covgram_version(void) { return COVGRAM_VERSION; }
int covgram_sizeof_kernel(void) { return (int)sizeof(covgram_kernel); }
int covgram_sizeof_composite(void) { return (int)sizeof(covgram_kernel_composite); }
const char* covgram_last_error(void) { return g_err; }

int covgram_device_count(int* count) {
    CG_REQUIRE(count != nullptr, COVGRAM_EINVAL, "count is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { c = 0; (void)hipGetLastError(); }
    *count = c;
    return COVGRAM_OK;
}

int covgram_ctx_create(covgram_ctx** out, int device_id, void* hip_stream) {
    CG_REQUIRE(out != nullptr, COVGRAM_EINVAL, "ctx out pointer is NULL");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        set_error("no HIP device visible (hipGetDeviceCount: %s) — libcovgram has no CPU fallback",
                  e == hipSuccess ? "0 devices" : hipGetErrorString(e));
        return COVGRAM_ENODEVICE;
    }
    CG_REQUIRE(device_id >= 0 && device_id < count, COVGRAM_EINVAL, "device_id %d out of range [0,%d)", device_id, count);
    ::covgram::DeviceGuard _cg_dev(device_id);
    CG_REQUIRE(_cg_dev.ok(), COVGRAM_EHIP, "hipSetDevice(%d) failed", device_id);
    hipDeviceProp_t prop;
    CG_CHECK_HIP(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; libcovgram is built for gfx950 (MI355X) only", device_id, prop.gcnArchName);
        return COVGRAM_ENODEVICE;
    }
    covgram_ctx* c = new covgram_ctx();
    c->device = device_id;
    c->num_cus = prop.multiProcessorCount;
    c->stream = (hipStream_t)hip_stream;   // NULL = the device's default (null) stream, like any HIP API
    c->own_stream = false;
    *out = c;
    return COVGRAM_OK;
}

int covgram_ctx_destroy(covgram_ctx* ctx) {
    if (!ctx) return COVGRAM_OK;
    CG_REQUIRE(ctx->live_handles == 0, COVGRAM_EINVAL, "ctx destroyed with %d live handles", ctx->live_handles);
    ::covgram::DeviceGuard _cg_dev(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx_blas_destroy(ctx);
    (void)comm_destroy(ctx);
    for (auto& w : ctx->ws) if (w.ptr) (void)hipFree(w.ptr);
    if (ctx->sym_map) (void)hipFree(ctx->sym_map);
    if (ctx->stamp_buf) (void)hipFree(ctx->stamp_buf);
    if (ctx->tickets) (void)hipFree(ctx->tickets);
    for (auto& t : ctx->timers) { (void)hipEventDestroy(t.first); (void)hipEventDestroy(t.second); }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return COVGRAM_OK;
}

int covgram_ctx_set_stream(covgram_ctx* ctx, void* hip_stream) {
    CG_REQUIRE(ctx != nullptr, COVGRAM_EINVAL, "ctx is NULL");
    // workspaces are reused across calls: order the new stream after everything queued on the old one
    if ((hipStream_t)hip_stream != ctx->stream) CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->stream = (hipStream_t)hip_stream;
    return COVGRAM_OK;
}

int covgram_ctx_get_stream(covgram_ctx* ctx, void** hip_stream) {
    CG_REQUIRE(ctx && hip_stream, COVGRAM_EINVAL, "NULL argument");
    *hip_stream = (void*)ctx->stream;
    return COVGRAM_OK;
}

// options and info keys: name -> member of covgram_ctx
struct CtxField { const char* key; int64_t covgram_ctx::*member; };
#define CG_FIELD(name) {#name, &covgram_ctx::name}
static const CtxField kOptions[] = {
    CG_FIELD(dense_variant), CG_FIELD(toeplitz_fused), CG_FIELD(toeplitz_colfft), CG_FIELD(toeplitz_persist), CG_FIELD(kron_fill), CG_FIELD(mfma_f16),
    CG_FIELD(mfma_gate_pct), CG_FIELD(mfma_fuse_w), CG_FIELD(toeplitz_real_spectrum), CG_FIELD(rows_per_lane), CG_FIELD(jsplit), CG_FIELD(target_wgs),
    CG_FIELD(grad_keep_r), CG_FIELD(grad_expand), CG_FIELD(grad_bcast), CG_FIELD(mfma_lds), CG_FIELD(mfma_sym), CG_FIELD(dense_sym), CG_FIELD(dense_bcast),
    CG_FIELD(mfma_stamp), CG_FIELD(mfma_graded), CG_FIELD(inkernel_reduce), CG_FIELD(matrix_variant), CG_FIELD(mfma_mrhs), CG_FIELD(composite_termwise), CG_FIELD(sum_fused),
    CG_FIELD(lowrank_reverse), CG_FIELD(mfma_sym_rt), CG_FIELD(mfma_sym_st), CG_FIELD(lowrank_wgs), CG_FIELD(grad_mixed_panel), CG_FIELD(mixed_fuse), CG_FIELD(time_kernels)};
static const CtxField kInfo[] = {
    CG_FIELD(last_dense_path), CG_FIELD(last_jsplit), CG_FIELD(last_kron_path), CG_FIELD(last_mfma_lds), CG_FIELD(last_mfma_sym), CG_FIELD(last_dense_sym),
    CG_FIELD(last_dense_bcast), CG_FIELD(last_mfma_f16), CG_FIELD(last_inkernel_reduce), CG_FIELD(last_grad_expand), CG_FIELD(last_grad_bcast),
    CG_FIELD(last_grad_path), CG_FIELD(last_grad_jsplit), CG_FIELD(last_hess_path), CG_FIELD(last_vgh_path), CG_FIELD(last_matrix_path),
    CG_FIELD(last_block_matrix_path), CG_FIELD(last_sum_fused), CG_FIELD(last_mfma_instance), CG_FIELD(last_mfma_graded), CG_FIELD(last_mfma_sym_rt), CG_FIELD(last_grad_mixed_path),
    CG_FIELD(last_grad_mixed_jsplit), CG_FIELD(last_kron_arms), CG_FIELD(last_mixed_path), CG_FIELD(last_mixed_jsplit),
    CG_FIELD(last_mixed_matrix_path), CG_FIELD(num_cus)};
#undef CG_FIELD

int covgram_ctx_set_option(covgram_ctx* ctx, const char* key, int64_t value) {
    CG_REQUIRE(ctx && key, COVGRAM_EINVAL, "NULL argument");
    for (const CtxField& f : kOptions) {
        if (strcmp(key, f.key)) continue;
        if (!strcmp(key, "mfma_gate_pct")) CG_REQUIRE(value >= 1 && value <= 100, COVGRAM_EINVAL, "mfma_gate_pct = %lld: 1..100", (long long)value);
        if (!strcmp(key, "time_kernels")) ctx->timers_used = 0;
        ctx->*f.member = value;
        return COVGRAM_OK;
    }
    set_error("unknown option '%s'", key);
    return COVGRAM_EINVAL;
}

int covgram_ctx_get_info(covgram_ctx* ctx, const char* key, int64_t* value) {
    CG_REQUIRE(ctx && key && value, COVGRAM_EINVAL, "NULL argument");
    for (const CtxField& f : kInfo)
        if (!strcmp(key, f.key)) { *value = ctx->*f.member; return COVGRAM_OK; }
    if (!strcmp(key, "last_clock_khz")) {
        // median over the workgroups of the last stamped launch of (shader cycles) / (100 MHz ticks) x 100 MHz, in kHz; 0: none
        *value = 0;
        if (ctx->stamp_count > 0 && ctx->stamp_buf) {
            CG_DEVICE(ctx);
            CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
            std::vector<unsigned long long> h(ctx->stamp_count * 4);
            CG_CHECK_HIP(hipMemcpy(h.data(), ctx->stamp_buf, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            std::vector<double> khz;
            for (size_t w = 0; w < ctx->stamp_count; ++w) {
                const double dc = (double)(h[4 * w + 2] - h[4 * w]), dr = (double)(h[4 * w + 3] - h[4 * w + 1]);
                if (h[4 * w + 3] > h[4 * w + 1] && dr >= 100.0) khz.push_back(dc / dr * 1.0e5);   // >= 1 us of work
            }
            if (!khz.empty()) { std::nth_element(khz.begin(), khz.begin() + khz.size() / 2, khz.end()); *value = (int64_t)khz[khz.size() / 2]; }
        }
        return COVGRAM_OK;
    }
    set_error("unknown info key '%s'", key);
    return COVGRAM_EINVAL;
}

int covgram_ctx_read_stamps(covgram_ctx* ctx, uint64_t* out, int64_t cap, int64_t* count) {
    CG_REQUIRE(ctx && count && cap >= 0 && (out || cap == 0), COVGRAM_EINVAL, "NULL argument");
    *count = ctx->stamp_buf ? (int64_t)ctx->stamp_count : 0;
    const size_t take = (size_t)std::min<int64_t>(*count, cap);
    if (take == 0) return COVGRAM_OK;
    CG_DEVICE(ctx);
    CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    CG_CHECK_HIP(hipMemcpy(out, ctx->stamp_buf, take * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return COVGRAM_OK;
}

int covgram_ctx_kernel_time(covgram_ctx* ctx, double* total_ms, int64_t* launches, int32_t reset) {
    CG_REQUIRE(ctx && total_ms && launches, COVGRAM_EINVAL, "NULL argument");
    CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    double tot = 0;
    for (size_t i = 0; i < ctx->timers_used; ++i) {
        float ms = 0;
        CG_CHECK_HIP(hipEventElapsedTime(&ms, ctx->timers[i].first, ctx->timers[i].second));
        tot += ms;
    }
    *total_ms = tot;
    *launches = (int64_t)ctx->timers_used;
    if (reset) ctx->timers_used = 0;
    return COVGRAM_OK;
}

int covgram_sync(covgram_ctx* ctx) {
    CG_REQUIRE(ctx != nullptr, COVGRAM_EINVAL, "ctx is NULL");
    CG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return COVGRAM_OK;
}

int covgram_points_create(covgram_ctx* ctx, covgram_points** out, const void* x, int64_t n, int32_t d, int32_t dtype,
                          int32_t loc) {
    CG_REQUIRE(ctx && out, COVGRAM_EINVAL, "NULL argument");
    CG_REQUIRE(n >= 0 && d >= 1, COVGRAM_EINVAL, "points: need n >= 0 and d >= 1 (got n=%lld d=%d)", (long long)n, d);
    CG_REQUIRE(dtype == COVGRAM_F32 || dtype == COVGRAM_F64, COVGRAM_EINVAL, "unknown dtype %d", dtype);
    CG_REQUIRE(x != nullptr || n == 0, COVGRAM_EINVAL, "points pointer is NULL");
    CG_DEVICE(ctx);
    covgram_points* p = new covgram_points();
    p->ctx = ctx; p->n = n; p->d = d; p->dtype = dtype;
    if (loc == COVGRAM_DEVICE) { p->dptr = const_cast<void*>(x); p->owns = false; }
    else {
        const size_t bytes = (size_t)n * d * dtype_size(dtype);
        if (bytes) {
            hipError_t e = hipMalloc(&p->dptr, bytes);
            if (e != hipSuccess) { delete p; set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); return COVGRAM_ENOMEM; }
            e = hipMemcpyAsync(p->dptr, x, bytes, hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) { (void)hipFree(p->dptr); delete p; set_error("H2D copy failed: %s", hipGetErrorString(e)); return COVGRAM_EHIP; }
        }
        p->owns = true;
    }
    int rc = points_max_norm2(p);      // one reduction + 4-byte read-back: gates the matrix-core EQ path (dense_mfma.hip)
    if (rc) { if (p->owns && p->dptr) (void)hipFree(p->dptr); delete p; return rc; }
    ctx->live_handles++;
    *out = p;
    return COVGRAM_OK;
}

int covgram_points_slice(const covgram_points* parent, int64_t first, int64_t count, covgram_points** out) {
    CG_REQUIRE(parent && out, COVGRAM_EINVAL, "NULL argument");
    CG_REQUIRE(first >= 0 && count >= 0 && first + count <= parent->n, COVGRAM_EINVAL,
               "slice [%lld, %lld) outside [0, %lld)", (long long)first, (long long)(first + count), (long long)parent->n);
    covgram_points* p = new covgram_points(*parent);
    p->owns = false;
    p->owns_center = false;            // the centre buffer stays the parent's
    for (auto& f : p->frag) f = covgram_points::FragSlot{};   // a slice packs its own fragments
    p->frag_clock = 0;
    p->n = count;
    p->dptr = (char*)parent->dptr + (size_t)first * parent->d * dtype_size(parent->dtype);
    parent->ctx->live_handles++;
    *out = p;
    return COVGRAM_OK;
}

int covgram_points_destroy(covgram_points* p) {
    if (!p) return COVGRAM_OK;
    {
        ::covgram::DeviceGuard _cg_dev(p->ctx->device);            // (a finalizer may call this from any thread state)
        bool frags = false;
        for (const auto& f : p->frag) frags = frags || f.ptr;
        if (frags || (p->owns && p->dptr) || (p->owns_center && p->center_buf)) (void)hipStreamSynchronize(p->ctx->stream);
        for (auto& f : p->frag) if (f.ptr) (void)hipFree(f.ptr);
        if (p->owns && p->dptr) (void)hipFree(p->dptr);
        if (p->owns_center && p->center_buf) (void)hipFree(p->center_buf);
    }
    p->ctx->live_handles--;
    delete p;
    return COVGRAM_OK;
}

int covgram_points_info(const covgram_points* p, int64_t* n, int32_t* d, int32_t* dtype) {
    CG_REQUIRE(p != nullptr, COVGRAM_EINVAL, "points is NULL");
    if (n) *n = p->n;
    if (d) *d = p->d;
    if (dtype) *dtype = p->dtype;
    return COVGRAM_OK;
}

int covgram_mvm(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* a,
                int64_t lda, void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t loc) {
    return dense_mvm(ctx, k, X, Y, a, lda, y, ldy, nrhs, alpha, beta, loc, 0, 0);
}

int covgram_mvm_sym_supported(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, int32_t world, int32_t* supported) {
    CG_REQUIRE(supported != nullptr, COVGRAM_EINVAL, "NULL argument");
    *supported = 0;
    CG_REQUIRE(world >= 1, COVGRAM_EINVAL, "world = %d", world);
    int rc = check_pair(ctx, X, X);
    if (rc) return rc;
    if (k == nullptr || k->family == COVGRAM_COMPOSITE) return COVGRAM_OK;
    HostKernel hk;
    rc = make_host_kernel(k, X->dtype, false, &hk);
    if (rc) return rc;
    if (X->n <= 0) return COVGRAM_OK;
    // fp64 (the reference's default element type), and fp32 where no matrix-core kernel takes the pair (profile, cloud): the direct-
    // difference symmetric kernels over cyclic row blocks, with the SAME shape / slab predicate covgram_mvm applies to the partial call
    // (it depends on world: a rank's column-sum slab is ceil(row blocks / world) x n scalars, capped at 2 GiB)
    if (X->dtype == COVGRAM_F64) { *supported = dense_sym_shape(hk, X, world, 2, nullptr) ? 1 : 0; return COVGRAM_OK; }
    if (mfma_eq_sym_eligible(ctx, hk, X, X, 1) || mfma_gen_sym_eligible(ctx, hk, X, X, 1)) { *supported = 1; return COVGRAM_OK; }
    if (mfma_eq_eligible(ctx, hk, X, X, 1) || mfma_gen_eligible(ctx, hk, X, X)) return COVGRAM_OK;   // the general matrix-core kernel is the better row shard
    *supported = dense_sym_shape(hk, X, world, 2, nullptr) ? 1 : 0;
    return COVGRAM_OK;
}

int covgram_mvm_sym_partial(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const void* a, void* y,
                            int32_t rank, int32_t world) {
    CG_REQUIRE(world >= 1 && rank >= 0 && rank < world, COVGRAM_EINVAL, "rank %d outside [0, %d)", rank, world);
    CG_REQUIRE(a != nullptr && y != nullptr, COVGRAM_EINVAL, "a or y is NULL");
    int32_t ok = 0;
    int rc = covgram_mvm_sym_supported(ctx, k, X, world, &ok);
    if (rc) return rc;
    if (!ok) { set_error("no symmetric kernel applies to this kernel / point set / world size"); return COVGRAM_EUNSUPPORTED; }
    int64_t lda = X->n;
    rc = unalias_input(ctx, &a, &lda, X->n, 1, y, X->n, X->n, dtype_size(X->dtype));   // a and y may overlap: a private copy of a
    if (rc) return rc;
    HostKernel hk;
    rc = make_host_kernel(k, X->dtype, false, &hk);
    if (rc) return rc;
    const bool mc = X->dtype == COVGRAM_F32 && (mfma_eq_sym_eligible(ctx, hk, X, X, 1) || mfma_gen_sym_eligible(ctx, hk, X, X, 1));
    if (!mc) {
        // rank r takes the row blocks r, r + P, ... of the upper triangle on the direct-difference kernel of the data's precision;
        // the partials of all ranks add up to G a
        return dense_mvm(ctx, k, X, X, a, X->n, y, X->n, 1, 1.0, 0.0, COVGRAM_DEVICE, rank, world);
    }
    CG_DEVICE(ctx);
    ctx->last_dense_path = 2; ctx->last_mfma_sym = 1;
    const bool fast = mfma_eq_sym_eligible(ctx, hk, X, X, 1);
    return mvm_eq_mfma_sym(ctx, hk, X, (const float*)a, (float*)y, 1.0, 0.0, rank, world, fast ? nullptr : k);
}

}  // extern "C"
