// driver.hpp — what the C-ABI drivers share: staging of host pointers, dtype dispatch, the timer bracket, the bracket of a block MVM entry, the
// Sum split.  Served units: the point-pair entries (api.hip, matrix.hip, mixed_mvm.hip, block_mvm.hip, grad_mixed.hip — these two through grad_driver.hpp —,
// sm.hip, sparse.hip, bilin_grad.hip, input_grad.hip, dense_mfma.hip, pivchol.hip), kernel_params.hip (the family names of its refusals) and the
// structured operators (toeplitz.hip, toeplitz_direct.hip, kron.hip, lowrank.hip, barneshut.hip).  Host code only; the per-family kernel units
// include common.hpp and dispatch.hpp (by_dtype, by_bool, by_dim), not this.
#pragma once
#include "dispatch.hpp"

namespace covgram {

// HIP-event bracket around the dominant kernel of a product (option "time_kernels"): the first event is recorded here, the second on EVERY way
// out of the scope — a refused launch too, so that covgram_ctx_kernel_time never meets a counted pair whose second event was not recorded
struct TimerScope {
    explicit TimerScope(covgram_ctx* ctx) : stream(ctx->stream), tm(timer_next(ctx)) {
        if (tm) (void)hipEventRecord(tm->first, stream);
    }
    ~TimerScope() { if (tm) (void)hipEventRecord(tm->second, stream); }
    TimerScope(const TimerScope&) = delete;
    TimerScope& operator=(const TimerScope&) = delete;
    hipStream_t stream;
    std::pair<hipEvent_t, hipEvent_t>* tm;
};

// a (rows_a x nrhs, leading dimension lda) and y (rows_y x nrhs, ldy) of one product as its kernels see them: device memory, a not overlapping y.
//   HOST:   copies in workspace slots 2 / 3 (y goes in only when beta != 0: nothing reads it otherwise); a is staged before anything is written
//           back, so any overlap of the host arrays is harmless.  finish() copies y back and waits for it.
//   DEVICE: the caller's arrays; an a that overlaps y is replaced by a private copy (unalias_input, workspace slot 5).
// begin() enqueues its copies at once: call it in front of every launch of the product (a split Sum: once, in front of the first term).
// begin_tile() is the mirror for an output tile (rows x cols, ldo) in y / ldy.  HOST: the kernels write a packed tile in slot 3 (ldy = rows) and
// finish() copies it back column by column — the rows beyond `rows` of the caller's array stay untouched — and waits.
struct Staged {
    const void* a = nullptr;
    void* y = nullptr;
    int64_t lda = 0, ldy = 0;
    int begin(covgram_ctx* ctx, int loc, size_t ts, const void* a_in, int64_t lda_in, int64_t rows_a, void* y_in, int64_t ldy_in, int64_t rows_y, int nrhs,
              double beta);
    int begin_tile(covgram_ctx* ctx, int loc, size_t ts, void* out, int64_t ldo, int64_t rows, int64_t cols);
    int finish();
private:
    covgram_ctx* ctx_ = nullptr;
    void* host_ = nullptr;        // set while a device copy (rows_ x cols_) has to go back to the caller's array (leading dimension host_ld_)
    int64_t host_ld_ = 0, rows_ = 0, cols_ = 0;
    size_t ts_ = 0;
};

// One further operand of a call (rows x cols, column-major, leading dimension ld: a factor, a first column, a right-hand side) as the kernels
// see it.  HOST: a packed device copy (*ldd = rows) at the cursor `cur` into a workspace the caller reserved — staged_bytes() of it per
// operand — which moves on to the next 256-byte boundary; the copy is enqueued on the ctx stream.  DEVICE: the caller's array.
inline size_t staged_bytes(int64_t rows, int64_t cols, size_t ts) { return ((size_t)rows * (size_t)cols * ts + 255) & ~(size_t)255; }
inline int stage_operand(covgram_ctx* ctx, int loc, size_t ts, char*& cur, const void* src, int64_t ld, int64_t rows, int64_t cols, const void** dev,
                         int64_t* ldd) {
    *dev = src; *ldd = ld;
    if (loc != COVGRAM_HOST || rows <= 0 || cols <= 0) return COVGRAM_OK;
    CG_CHECK_HIP(hipMemcpy2DAsync(cur, (size_t)rows * ts, src, (size_t)ld * ts, (size_t)rows * ts, (size_t)cols, hipMemcpyHostToDevice, ctx->stream));
    *dev = cur; *ldd = rows;
    cur += staged_bytes(rows, cols, ts);
    return COVGRAM_OK;
}

int check_pair(const covgram_ctx* ctx, const covgram_points* X, const covgram_points* Y);

// The bracket of a block MVM entry, y <- alpha G a + beta y on block vectors with B entries per point (a: m B x nrhs, y: n B x nrhs,
// column-major): the argument checks, the ctx's device, the staging of a and y around run(st), which enqueues the product on st.a / st.y.
//   block(d, &B): the entry's own checks that come first, and its block size;
//   lower():      the kernel's validation, host work only — nothing has touched the device before it returns COVGRAM_OK;
//   stage_empty:  whether a product without rows (n = 0) is still staged and run, or returns at once.
template <typename Block, typename Lower, typename Run>
inline int block_mvm_entry(covgram_ctx* ctx, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda, void* y, int64_t ldy, int32_t nrhs,
                           double beta, int32_t loc, bool stage_empty, Block block, Lower lower, Run run) {
    int rc = check_pair(ctx, X, Y);
    if (rc) return rc;
    int64_t B = 0;
    rc = block(X->d, &B);
    if (rc) return rc;
    CG_REQUIRE(nrhs >= 1, COVGRAM_EINVAL, "nrhs must be >= 1");
    const int64_t ma = Y->n * B, ny = X->n * B;
    CG_REQUIRE(lda >= ma && ldy >= ny, COVGRAM_EINVAL, "lda / ldy smaller than the block vectors (%lld, %lld)", (long long)ma, (long long)ny);
    CG_REQUIRE((a != nullptr || ma == 0) && (y != nullptr || ny == 0), COVGRAM_EINVAL, "a or y is NULL");
    rc = lower();
    if (rc) return rc;
    CG_DEVICE(ctx);
    if (X->n == 0 && !stage_empty) return COVGRAM_OK;
    Staged st;
    rc = st.begin(ctx, loc, dtype_size(X->dtype), a, lda, ma, y, ldy, ny, nrhs, beta);
    if (rc) return rc;
    rc = run(st);
    if (rc) return rc;
    CG_CHECK_HIP(hipGetLastError());
    return st.finish();
}

// choose the J split: enough workgroups to fill the chip, chunks aligned to the inner accumulation block
void choose_split(const covgram_ctx* ctx, int64_t rowblocks, int64_t m, int64_t align, int64_t* jchunk, int* jsplit, int64_t default_target = 0);

// A composite whose every term is ONE profile (times constants) is a plain Sum (src/algebra.jl:5-14): G = sum_t c_t G_t, so
// every MVM is the sum of the terms' MVMs, each on its own single-profile path (matrix cores, folded constants, lane-per-row
// gradient kernel) instead of the per-block interpreter of the composite kernels.  Fills the terms; false = not such a sum.
// Constant-only terms (k = c: G = c 1 1', src/stationary.jl:27-34) add up in *constant: their MVM is c * sum(a) on every row.
// Product terms (several profiles) stay composite, one single-term composite each, and run on the interpreter by themselves;
// when EVERY term is a product the whole composite stays on the interpreter (one pass shares the distances).
struct SumTerm {
    bool simple;
    covgram_kernel k;                     // simple
    covgram_kernel_composite c;           // product term
    const covgram_kernel* ptr() const { return simple ? &k : &c.head; }
};
struct SumSplit {
    SumTerm terms[COVGRAM_COMPOSITE_MAX_TERMS];
    int nterms = 0;
    double constant = 0.0;
};
bool composite_sum_terms(const covgram_ctx* ctx, const covgram_kernel* k, int32_t loc, SumSplit* split);
// y[i * ys + r * ldy] += coef * sum_j a[j * as + r * lda]   (as = ys = 1: dense; d + 1: the value row of value-gradient blocks)
int constant_term_mvm(covgram_ctx* ctx, int dtype, const void* a, int64_t m, int64_t lda, int64_t as, void* y, int64_t n, int64_t ldy, int64_t ys,
                      int nrhs, double coef);
// the split Sum on device-resident a and y: run_term(kernel, beta) once per profile term — the first applies the caller's beta, the others add —
// and then add_constant()
template <typename RunTerm, typename AddConstant>
inline int sum_split_run(const SumSplit& s, double beta, RunTerm run_term, AddConstant add_constant) {
    for (int t = 0; t < s.nterms; ++t) {
        const int rc = run_term(s.terms[t].ptr(), t == 0 ? beta : 1.0);
        if (rc) return rc;
    }
    return add_constant();
}

// covgram_mvm's product behind its staging (api.hip): y <- alpha G a + beta y for one covgram_kernel — a single profile or a one-trait
// composite, a Sum split per term — on device-resident a and y that do not overlap, by the routes of the dense driver (matrix cores,
// factored dot product, lane per row, ...).  For a driver that has staged a and y itself and sends parts of its kernel there (mixed_mvm.hip).
int dense_mvm_on_device(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda, void* y,
                        int64_t ldy, int32_t nrhs, double alpha, double beta);

// The kernels that HessianKernel(k) / ValueGradientHessianKernel(k) (w: the wrapper's name) have a device path for: single profiles with
// closed-form derivatives up to the fourth, no Power wrapper, d <= HESS_MAX_D.  The refusals of covgram_hess_mvm,
// covgram_valgradhess_mvm and the Hessian kinds of covgram_block_matrix.
extern const char* const kFamilyNames[COVGRAM_NFAMILY];
int hess_refusal(const char* w, const covgram_kernel* k, int d);

}  // namespace covgram
