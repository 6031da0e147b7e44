/* covgram.h — C ABI of libcovgram.so, the MI355X (gfx950) lazy-Gramian MVM engine.
 *
 * Drop-in boundary for ONE hot path of SebastianAment/CovarianceFunctions.jl (v0.3.5):
 *     mul!(b, gramian(k, x[, y]), a, α, β)
 * and its structured siblings.  The reference is pure Julia with no FFI of its own, so the
 * boundary is the set of Julia methods listed below; a Julia shim (`ccall`) or the Python
 * `ctypes` binding in covariancefunctions.jl_amd/covgram/_ffi.py binds exactly these symbols.
 * Citations are file:line relative to the reference repository root.
 *
 *   covgram_mvm            replaces  LinearAlgebra.mul!(y::AbstractVector, G::Gramian, x, α, β)   src/gramian.jl:78-87
 *                          and       LinearAlgebra.mul!(Y::AbstractMatrix, G::Gramian, X, α, β)   src/gramian.jl:89-99
 *                          and       Base.:*(G::Gramian, a)                                       src/gramian.jl:66-75
 *   covgram_matrix         replaces  Base.Matrix(G::Gramian) / Matrix!                            src/gramian.jl:102-114
 *   covgram_grad_mvm       replaces  BlockFactorizations.blockmul!(y, G::Gramian, x, α, β)        src/gramian.jl:241-257
 *                          with the  GradientKernelElement mul! (isotropic / dot-product)         src/gradient.jl:86-92, 109-115
 *   covgram_valgrad_mvm    the same  blockmul! with the ValueGradientKernel element                       src/gradient.jl:319-351, 400-474
 *   covgram_hess_mvm       the same  blockmul! with the HessianKernel elements' O(d^2) mul!             src/hessian.jl:125-190, 227-275
 *   covgram_valgradhess_mvm the same blockmul! with the ValueGradientHessianKernel elements, in O(d^2)           src/hessian.jl:279-325, 392-479
 *   covgram_block_matrix   replaces  Base.Matrix(G) of those four block Gramians (gramian(k, x, y, Val(false)))   src/gramian.jl:125-130, 192-199
 *   covgram_sparse_create  replaces  SparseArrays.sparse(G::Gramian, delta) and decay_radius(k, delta)         src/sparse.jl:5-38
 *   covgram_sparse_mvm     replaces  mul!(y, ::SparseMatrixCSC, a, alpha, beta) on its result
 *   covgram_bh_create      replaces  BarnesHutFactorization(k, x, y, D; theta, leafsize)                 src/barneshut.jl:25-39
 *   covgram_bh_mvm         replaces  barneshut!(b, F, w, alpha, beta, theta; split) and mul!(b, F, w, alpha, beta)   src/barneshut.jl:45-143
 *   covgram_bh_moments     replaces  node_sums / compute_centers_of_mass                                 src/barneshut.jl:145-190
 *   covgram_bh_taylor_mvm  replaces  taylor!(b, F, w, alpha, beta, theta; use_com), the signed branch of mul!      src/taylor.jl:7-57
 *   covgram_bh_taylor_moments  replaces  its node_sums / weighted_node_sums / centring of the first moments      src/taylor.jl:15-18
 *   (covgram_bh_taylor_mvm under a binding's MINRES replaces ldiv!(x, F, b) and F \ b               src/barneshut.jl:64-72)
 *   covgram_toeplitz_*     replaces  mul!(y, ::SymmetricToeplitz/Toeplitz/Circulant, a, α, β) of ToeplitzMatrices 0.7.1 as
 *                          constructed by gramian(k, x::StepRangeLen, y::StepRangeLen)            src/gramian.jl:167-189
 *   covgram_toeplitz_durbin / _levinson / _trench  replace durbin! / levinson! / trench!             src/toeplitz.jl:12-111
 *   covgram_kron_mvm       replaces  mul!(y, ::KroneckerProduct, a) of KroneckerProducts 1.1.1 as constructed at
 *                                                                                                 src/algebra.jl:91-95, src/separable.jl:33-42
 *   covgram_lowrank_mvm    replaces  mul!(y, L::LazyMatrixProduct(U, V'), a, α, β)                src/lazy_linear_algebra.jl:78-85
 *                          as built by gramian(k::FiniteBasis, x, y)                              src/mercer.jl:61-70
 *   covgram_pivoted_cholesky  replaces  cholesky(G::Gramian, Val(true); tol) without instantiating G (the reference's own TODO)   src/gramian.jl:191-199
 *   covgram_kernel         encodes   the kernel value k together with input_trait(k)              src/properties.jl:31-45
 *   covgram_kernel_composite encodes Sum / Product / Power of same-trait kernels                  src/algebra.jl:5-63, src/properties.jl:47-63
 *
 * Conventions (same as the reference's at that boundary):
 *   - the caller owns every buffer it passes; handles own only what the library allocated;
 *   - points are point-major: d contiguous scalars per point (Julia d×n column-major matrix ==
 *     Vector of d-vectors, src/gramian.jl:2,154-155);
 *   - flat block vectors of the gradient Gramian are point-major (block i = entries i*d..i*d+d-1);
 *   - matrices (right-hand sides, dense factors) are column-major with an explicit leading dimension;
 *   - beta == 0 means the previous contents of y are NOT read (NaN-safe, src/gramian.jl:80,90,245);
 *   - every function returns 0 on success and a negative covgram_status on failure; no exception
 *     crosses the ABI; covgram_last_error() gives a thread-local message;
 *   - unlike the reference (which runs @inbounds), dimension mismatches are reported as errors;
 *   - there is NO CPU fallback: every compute entry point needs a gfx950 device.
 */
#ifndef COVGRAM_H
#define COVGRAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COVGRAM_VERSION 113 /* 0.1.1: covgram_kron_mvm, covgram_grad_mvm and covgram_valgrad_mvm take (lda, ldy, nrhs); 111 adds
                               covgram_cg_step_shifted; 112: covgram_mvm_sym_supported takes `world` (the symmetric partial form's
                               column-sum slab depends on it), fp32 direct-difference symmetric partials; 113: the communicator
                               (covgram_comm_*), covgram_mvm_sharded, covgram_mvm_sym_allreduce.  Added since, backward
                               compatibly (no version step): covgram_hess_mvm and the info key "last_hess_path";
                               covgram_valgradhess_mvm and the info key "last_vgh_path";
                               the info key "last_matrix_path";
                               covgram_block_matrix, the COVGRAM_BLOCK_* kinds and the info key "last_block_matrix_path";
                               covgram_decay_radius and the covgram_sparse_* handle (sparse(G, delta));
                               the covgram_bh_* handle (BarnesHutFactorization);
                               covgram_bh_taylor_moments and covgram_bh_taylor_mvm (taylor! on that handle);
                               covgram_pivoted_cholesky and COVGRAM_PIVCHOL_MAX_RANK;
                               covgram_bcg_init, covgram_bcg_step, covgram_bcg_update, covgram_bcg_direction and the
                               COVGRAM_BCG_* layout of their state (batched CG on a block of right-hand sides);
                               the covgram_sm_* handle (SpectralMixture Gramians: one fused product and Matrix(G));
                               covgram_bilinear_grad (hyper-parameter gradients of bilinear forms in one pass);
                               covgram_bilinear_input_grad (their gradients with respect to the row points in one pass);
                               covgram_bilinear_grad_sm (the hyper-parameter gradients of a SpectralMixture Gramian's bilinear forms);
                               covgram_bilinear_input_grad_sm (their gradients with respect to the row points in one pass);
                               covgram_grad_mvm_mixed, the factor family COVGRAM_NEURALNETWORK, the option "grad_mixed_panel" and the
                               info keys "last_grad_mixed_path" / "last_grad_mixed_jsplit" (gradient Gramians of mixed-trait composites);
                               the info key "last_kron_arms" (template arms of the last covgram_kron_mvm's kernels);
                               covgram_mvm_mixed and covgram_matrix_mixed, the option "mixed_fuse" and the info keys "last_mixed_path" /
                               "last_mixed_jsplit" / "last_mixed_matrix_path" (scalar Gramians of mixed-trait composites).
                               A binding checks covgram_version() against the header it mirrors at load time */

typedef enum covgram_status {
    COVGRAM_OK = 0,
    COVGRAM_EINVAL = -1,       /* bad argument / dimension mismatch */
    COVGRAM_EUNSUPPORTED = -2, /* kernel family / dimension / dtype outside the compiled set */
    COVGRAM_EHIP = -3,         /* HIP / rocFFT runtime failure (message in covgram_last_error) */
    COVGRAM_ENODEVICE = -4,    /* no gfx950 device visible: the product path fails loudly */
    COVGRAM_ENOMEM = -5
} covgram_status;

/* Scalar profile phi(s); s = |x-y|^2 (isotropic) or x.y (dot product). */
typedef enum covgram_family {
    COVGRAM_EQ = 0,       /* exp(-s/2)                         src/stationary.jl:37-42   */
    COVGRAM_EXP = 1,      /* exp(-sqrt(s))                     src/stationary.jl:56-60   */
    COVGRAM_RQ = 2,       /* (1 + s/(2 alpha))^-alpha          src/stationary.jl:45-53   */
    COVGRAM_GAMMAEXP = 3, /* exp(-s^(gamma/2)/2)               src/stationary.jl:63-71   */
    COVGRAM_CAUCHY = 4,   /* 1/(1+s)                           src/stationary.jl:221-224 */
    COVGRAM_IMQ = 5,      /* 1/sqrt(s + c^2)                   src/stationary.jl:231-235 */
    COVGRAM_MATERNP = 6,  /* Matern nu = p + 1/2, 0 <= p <= 8  src/stationary.jl:117-158 */
    COVGRAM_DOT = 7,      /* s                                 src/mercer.jl:6-9         */
    COVGRAM_EXPDOT = 8,   /* exp(s)                            src/mercer.jl:19-22       */
    COVGRAM_MATERN = 9,   /* Matern, real nu > 0: 2^(1-nu)/Gamma(nu) r^nu K_nu(r), r = sqrt(2 nu s); Taylor guard near 0
                             (param = nu)                                        src/stationary.jl:87-114  */
    COVGRAM_ASINDOT = 10, /* (2/pi) asin(s): the NeuralNetwork kernel on its normalised augmented inputs x^ = [x, sqrt(sigma)] /
                             sqrt(1 + |x|^2 + sigma), for which x^.y^ is the argument of asin   src/mercer.jl:73-85 */
    COVGRAM_NFAMILY = 11,
    /* only inside / as the head of a covgram_kernel_composite: */
    COVGRAM_CONSTANT = 100, /* factor: the constant `scale`            src/stationary.jl:27-34   */
    COVGRAM_COMPOSITE = 101, /* head of a covgram_kernel_composite      src/algebra.jl:5-63       */
    /* only as a factor of the composite passed to covgram_grad_mvm_mixed, covgram_mvm_mixed or covgram_matrix_mixed: */
    COVGRAM_NEURALNETWORK = 102 /* factor: NeuralNetwork(sigma) on the RAW points, (2/pi) asin((x.y + sigma) / sqrt((1 + |x|^2 + sigma)
                                   (1 + |y|^2 + sigma))); param = sigma >= 0, trait = 0 (neither trait), lengthscale = 1   src/mercer.jl:73-85 */
} covgram_family;

/* input_trait(k), src/properties.jl:31-45.  Only the two traits with a device path are encoded;
 * GenericInput kernels never reach the library (the host falls back exactly as gramian.jl:78-87). */
typedef enum covgram_trait { COVGRAM_ISOTROPIC = 1, COVGRAM_DOTPRODUCT = 2 } covgram_trait;

typedef enum covgram_dtype { COVGRAM_F32 = 0, COVGRAM_F64 = 1 } covgram_dtype;
typedef enum covgram_loc { COVGRAM_HOST = 0, COVGRAM_DEVICE = 1 } covgram_loc;

#define COVGRAM_MATERNP_MAX_P 8

typedef struct covgram_kernel {
    int32_t family;     /* covgram_family */
    int32_t trait;      /* covgram_trait; must agree with the family (checked) */
    int32_t p;          /* MaternP order */
    int32_t power;      /* Power(k, p) exponent, >= 1 (src/algebra.jl:50-63); 1 = none */
    double param;       /* RQ alpha | gammaExp gamma | IMQ c | Matern nu */
    double lengthscale; /* Lengthscale(k, l): s <- s/l^2, isotropic only (src/transformation.jl:6-19); 1 = none */
    double scale;       /* Constant(c) * k (src/algebra.jl:23-25); 1 = none */
} covgram_kernel;

/* Sum / Product / Power of kernels that share one input trait (src/algebra.jl:5-63; the common trait is what
 * src/properties.jl:47-63 computes, Constant arguments do not count):
 *     k(x, y) = head.scale * sum_{t < nterms}  prod_{f < nfactors[t]}  factor(x, y)
 * with the factors of term 0 first in `factors`, then term 1's, ...  Each factor is a simple covgram_kernel with its
 * own scale, lengthscale and power (or family COVGRAM_CONSTANT: just `scale`).  Every entry point that takes a
 * `const covgram_kernel*` accepts `&composite.head` (head.family == COVGRAM_COMPOSITE, head.trait = the common trait,
 * head.power == 1, head.lengthscale == 1). */
#define COVGRAM_COMPOSITE_MAX_TERMS 8
#define COVGRAM_COMPOSITE_MAX_FACTORS 8
typedef struct covgram_kernel_composite {
    covgram_kernel head;
    int32_t nterms;
    int32_t nfactors[COVGRAM_COMPOSITE_MAX_TERMS];
    covgram_kernel factors[COVGRAM_COMPOSITE_MAX_FACTORS];
} covgram_kernel_composite;

typedef struct covgram_ctx covgram_ctx;           /* one device + one stream + workspace + rocFFT plans */
typedef struct covgram_points covgram_points;     /* device-resident point set (stays resident across MVMs) */
typedef struct covgram_toeplitz covgram_toeplitz; /* cached circulant spectrum + plans */
typedef struct covgram_sparse covgram_sparse;     /* radius-thresholded CSR Gramian: owns its three arrays */
typedef struct covgram_bh covgram_bh;             /* Barnes-Hut factorization: ball tree over the columns, tree-ordered copies of both point sets */

int covgram_version(void);
/* sizeof() of the two structs that cross the ABI by pointer, as THIS build of the library sees them: a binding asserts its
 * own mirror against these at load time (julia/CovGram.jl does; tests/abi_layout.c checks every field offset). */
int covgram_sizeof_kernel(void);
int covgram_sizeof_composite(void);
const char* covgram_last_error(void);
int covgram_device_count(int* count);

/* hip_stream: the hipStream_t every kernel of this ctx is launched on (e.g. torch's current stream); NULL is the
 * device's default (null) stream.  The library never creates streams of its own. */
int covgram_ctx_create(covgram_ctx** ctx, int device_id, void* hip_stream);
int covgram_ctx_destroy(covgram_ctx* ctx);
int covgram_ctx_set_stream(covgram_ctx* ctx, void* hip_stream);
int covgram_ctx_get_stream(covgram_ctx* ctx, void** hip_stream);
/* tuning / A-B knobs: "dense_variant" (0 = auto: fp32 EQ runs on the matrix cores when the norm bound of dense_mfma.hip
 * holds and the plain dot-product Gramian is applied as X (Y' a), 1 = always the entry-by-entry direct kernel, 2 = matrix
 * cores whenever the shape allows), "rows_per_lane", "jsplit",
 * "target_wgs", "grad_keep_r", "time_kernels", "toeplitz_fused" (1 = fused row-FFT kernels, radix-16 stages at M' = 4096; 0 = rocFFT
 * batches; 2 = radix-4 stages everywhere), "toeplitz_colfft" (column FFT of the Toeplitz fast path: 16 = radix-16 register
 * butterflies, the default; 4 = the radix-4 LDS kernel), "toeplitz_persist" (fused radix-16 row kernel: persistent workgroups that prefetch the next row pair into registers; -1 = fp64 only, 0 = never, 1 = always), "toeplitz_real_spectrum" (read when a handle is created: 1 = a symmetric
 * matrix keeps the row kernel's spectrum copy as reals, 0 = always complex), "mfma_lds" (matrix-core EQ path: four waves share the
 * column tiles through LDS; -1 = when the column chunks are long enough, 0 = never, 1 = whenever compiled: d <= 8),
 * "matrix_variant" (covgram_matrix: 0 = rows in registers, 64-column strips — d <= 64 —, 1 = the generic entry-by-entry kernel),
 * "mfma_mrhs" (matrix right-hand sides on the fp32 matrix cores, dense_mfma_mrhs_kernel: -1 = from 5 columns (9 for the cheap profiles at d <= 3), 0 = never — four
 * columns at a time on the VALU —, 1 = from 2 columns),
 * "mfma_sym" (matrix-core EQ path on gramian(k, x), both sides the SAME device points: evaluate the upper triangle once;
 * -1 = from n = 12500 ... 18000 by the profile's cost, 0 = never, 1 = always),
 * "dense_sym" (the same for fp64 on the direct-difference path — the reference's default element type: gramian(k, x) with one
 * right-hand side evaluates every entry on or above the diagonal blocks once, dense_sym_kernel; -1 = from n = 6144 (16384 for
 * Cauchy / IMQ / Dot) while its column-sum slab of n^2 / 8 bytes stays within 1 GiB, 0 = never, 1 = always, up to a 2 GiB slab — the
 * slab lives in the ctx's workspace until the ctx is destroyed: 512 MiB at n = 65536, once per ctx),
 * "composite_termwise" (1 = a Sum runs one MVM per term on the term's own path, 0 = one pass of the composite kernels),
 * "sum_fused" (fp32 Sum of two or three single-profile isotropic terms — EQ, RQ, Cauchy, IMQ, MaternP(1..3), no Power wrapper — in ONE pass of
 * the matrix-core kernels, every term evaluated on the pair's shared distance as the reference does, src/algebra.jl:27-47: -1 = where it
 * measured faster than one MVM per term (three terms), 0 = never, 1 = wherever the one-pass kernels exist),
 * "mfma_sym_rt" (the symmetric fp32 matrix-core kernels at one or two MFMAs per tile — EQ, MaternP, RQ, Cauchy, IMQ: -1 / 2 = two row tiles per
 * wave in 4-wave workgroups, dense_mfma_sym2.hpp; 1 = one row tile per wave),
 * "grad_expand" (fp64 isotropic gradient / value-gradient Gramians in the expanded form — |x - y|^2 = |x|^2 + |y|^2 - 2 x.y with
 * cached norms, 4 instead of 6 fp64 instructions per dimension and pair: -1 = while the pre-scaled clouds lie within
 * gamma^2 R^2 <= 1000 of their common centre, 0 = never, 1 = always),
 * "inkernel_reduce" (the dense kernels' column-split partials: 1 = summed inside the kernel by the last workgroup of each row block
 * to arrive — fixed order, bit-identical to the separate launch, one launch and one dependent-launch gap less per MVM —, 0 = the separate
 * reduce launch, -1 = in the kernel only where it measured faster: the matrix-core EQ kernel up to n = 4096),
 * "grad_bcast" (fp64 expanded-form gradient / value-gradient MVM with the column records in vector registers, read by
 * v_fmac_f64_dpp row_newbcast — counted vector loads instead of the scalar stream: -1 = from padded d = 24, 0 = never, 1 / 4 = always,
 * with that many waves per workgroup),
 * "dense_bcast" (the same register-broadcast scheme for the fp64 dense value MVM of the isotropic kernels, one right-hand side:
 * |x - y|^2 expanded around cached norms, one v_fmac_f64_dpp per dimension and pair, all-entries and upper-triangle-once kernels:
 * -1 = from padded d = 16 up to d = 64 inside the gamma^2 R^2 <= 1000 gate of "grad_expand", 0 = never, 1 = wherever it applies, d >= 8),
 * "mfma_f16" (the fp32 matrix-core kernels' split of the coordinates: -1 / 1 = the fp16 two-way split — 3 products per coordinate, one MFMA per
 * FOUR coordinates, half the matrix-core work of the bf16 three-way split — while both clouds lie within g^2 R^2 <= 72 and the bf16 split beyond,
 * 0 = always the bf16 split, 2 = the fp16 split up to the matrix-core gate of 126: measurements only.  EQ kernels (general and symmetric) and,
 * since round 5, the generic ones — MaternP(p >= 1), RQ, Cauchy, IMQ, EQ^p, one-pass Sums; isotropic, d <= 30 — inside the same 72 / 126 of their gate),
 * "kron_fill" (1 / 2: workgroups per CU the Kronecker mode kernel's column tiling aims at; 2 measured slower, profiles/r05_kron_fill_ab.txt; 3 = never
 * fuse the last two modes: measurements, profiles/r05_kron_nopair_ab.txt),
 * "mfma_gate_pct" (1..100, default 100: both radius gates in percent.  BASELINE's 1e-5 is held NORM-wise at the full gates (<= 7.3e-6 measured);
 * the ROW-wise error |err_i| / (|K| |a|)_i of an adversarial cloud — points ON the gate's sphere, isolated rows, d >= 5 — reaches 1.5e-5 (bf16) /
 * 2.5e-5 (fp16) at the edge and scales with the gate: 40 holds 1e-5 row-wise on it.  Clouds outside run the direct-difference kernels),
 * "mfma_fuse_w" (the general matrix-core EQ kernel's column weights a_j exp2(f_j): -1 / 1 = formed inside the kernel, 0 = by a pack launch in front of
 * it — bit-identical results),
 * "mfma_graded" (the general matrix-core EQ kernel's column split: -1 = graded — the last half round's worth of columns cut into chunks that halve down to 64
 * tiles, so that the chip drains in short workgroups — on the LDS-shared form from two rounds of resident workgroups on, 0 = always equal chunks, 1 = graded
 * wherever the shape admits it (tests), 100 h + f = 1 with a tail of h half rounds and a floor of 16 * 2^f tiles: measurements only, tools/c2_graded_ab.py.  A forced "jsplit" or "target_wgs" keeps equal
 * chunks.  Results differ between the two splits by the fp32 summation order of the chunks' partial sums; each is deterministic),
 * "mfma_stamp" (1 = the general matrix-core EQ kernel runs its clock-stamping DIAGNOSTIC build — s_memtime / s_memrealtime
 * around every workgroup's column loop, for bench.py's sustained-clock figure; never set in production). */
int covgram_ctx_set_option(covgram_ctx* ctx, const char* key, int64_t value);
/* read-only facts: "last_dense_path" (which kernel the last covgram_mvm ran: 0 none yet, 1 lane-per-row direct differences,
 * 2 matrix cores, 3 wide rows, 4 Gramian(Dot(), x, y) factored as X (Y' a)), "last_matrix_path" (which kernel the last covgram_matrix
 * ran: 0 none yet or n m == 0, otherwise route + 10 DM + 1000 VR with route 1 = generic single profile, 2 = generic composite,
 * 3 = registers single profile, 4 = registers composite; DM the compiled dimension bucket, 0 for the generic kernels; VR rows per
 * thread, 1 where not applicable), "last_mfma_lds" (1: that matrix-core MVM shared its column tiles through LDS), "last_mfma_sym" (1: the last dense
 * MVM ran the symmetric upper-triangle kernel), "last_dense_sym" (1: it ran a direct-difference symmetric kernel, fp64 or fp32), "last_inkernel_reduce" (1: the last dense kernel summed its own split-J slab), "last_grad_expand" (1: the last gradient MVM ran the expanded form), "last_grad_bcast" (waves per workgroup of the broadcast kernel if the last gradient MVM ran it, else 0), "last_grad_path" (which kernels the last gradient or value-gradient MVM ran, as bits: 1 = the lane-per-row kernel, 2 = its two-column pass, 4 = the panel path (grad_wide), 8 = more than one panel, 16 = the panel path split over z slices with the separate reduce, 32 = the lane-per-row kernel with a column split > 1 and the slab reduce; 0 = no block kernel (n = 0 or m = 0); a Sum split term by term reports its last term), "last_grad_jsplit" (the column split of the last gradient MVM's lane-per-row launch, 0 if it did not run one), "last_hess_path" (0 = no Hessian MVM yet or one without rows / columns, 1 = the last covgram_hess_mvm ran its block kernel, csrc/hess_mvm.hpp), "last_block_matrix_path" (0 = no covgram_block_matrix yet or an empty product, otherwise (kind + 1) + 10 VR, VR = scalars per store instruction of the launch that ran: 1, or 2 for fp64 / 4 for fp32 on the 16-byte route), "last_sum_fused" (1: the last covgram_mvm ran a Sum on the one-pass kernels), "last_mfma_instance" (which instance of the matrix-core EQ kernels the last launch was: the template arguments of dense_mfma_eq_kernel as K2 1e5 + RT 1e4 + WPB 1e3 + LDS 100 + STAMP 10 + FMT, -(K2 10 + FMT) for the symmetric kernel, 0 otherwise — bench.py checks its recorded PMC pass against it), "last_dense_bcast" (1: the last fp64 dense MVM ran a register-broadcast kernel), "last_mfma_graded" (the number of column chunks if the last general matrix-core EQ MVM ran the graded split of "mfma_graded", else 0), "last_mfma_f16" (1: the last general matrix-core EQ MVM ran the fp16 two-way split), "last_jsplit" (the column split of the last lane-per-row dense launch), "last_kron_path" (which kernels the last covgram_kron_mvm ran, as bits: 1 = the fused last-two-modes pass, 2 = the single-mode kernel, 4 = the last-mode kernel, 8 = a rocBLAS GEMM (a factor side >= 1024, >= 256 with >= 2 GFLOP, or a shape the kernels refuse), 16 = two small trailing factors multiplied out first), "last_kron_arms" (which template arms of those kernels it launched, one bit each, cleared together with "last_kron_path": the fused pass <NB1, NB2, VEC> is bit 4 [NB1 == 8] + 2 [NB2 == 8] + VEC, the single-mode kernel <NBP, NW, VEC> bit 8 + 4 log2(NBP / 2) + 2 [NW == 8] + VEC, the last-mode kernel <NBB, NW, VEC> bit 20 + 4 [NBB == 8] + 2 [NW == 8] + VEC; a rocBLAS mode sets none), "num_cus", "last_clock_khz" (median shader clock over the workgroups of the last
 * launch made with "mfma_stamp" = 1; synchronises the stream; 0 = no stamped launch yet). */
int covgram_ctx_get_info(covgram_ctx* ctx, const char* key, int64_t* value);
int covgram_sync(covgram_ctx* ctx);
/* With option "time_kernels" = 1 every dense / gradient MVM brackets its dominant kernel with HIP events on the
 * ctx stream; this returns the summed device time and the number of launches since the last reset. */
int covgram_ctx_kernel_time(covgram_ctx* ctx, double* total_ms, int64_t* launches, int32_t reset);
/* The clock stamps of the last launch made with "mfma_stamp" = 1 (diagnostics: tools/c2_drain_probe.py): *count = its workgroups (0: none
 * yet), and up to cap of them are copied to out as four values each — shader clock and 100 MHz counter at the start of the workgroup's column
 * loop, the same two at its end — in launch order (chunk-major: workgroup = chunk * row blocks + row block).  Synchronises the stream. */
int covgram_ctx_read_stamps(covgram_ctx* ctx, uint64_t* out, int64_t cap, int64_t* count);

/* x: n points of dimension d, point-major.  loc == HOST: copied to the device; loc == DEVICE: borrowed
 * (the caller keeps it alive and unchanged while the handle lives: creation caches a sample mean c of the set as the
 * common centre of the isotropic kernels and the extent max |x_i - c|^2 that gates the matrix-core path; after an
 * in-place update destroy and re-create the handle, as the Python Gramian does from the tensor's version counter). */
int covgram_points_create(covgram_ctx* ctx, covgram_points** out, const void* x, int64_t n, int32_t d,
                          int32_t dtype, int32_t loc);
/* rows [first, first+count) of an existing handle (row shard for multi-GPU); borrows the parent's memory. */
int covgram_points_slice(const covgram_points* parent, int64_t first, int64_t count, covgram_points** out);
int covgram_points_destroy(covgram_points* pts);
int covgram_points_info(const covgram_points* pts, int64_t* n, int32_t* d, int32_t* dtype);

/* y <- alpha * G(k; X, Y) * a + beta * y.   G is n×m (n = |X|, m = |Y|); a is m×nrhs (lda >= m),
 * y is n×nrhs (ldy >= n), column-major; dtype is that of the points.  loc applies to a and y.
 * Aliasing: a and y may overlap in any way — y may be a itself (an in-place MVM, n == m), or any part of it, with any lda / ldy; the
 * library then reads a from a private copy (loc == DEVICE: one device-to-device copy at entry; loc == HOST: a is staged to the device
 * before anything is written back).  Separate ranges cost nothing. */
int covgram_mvm(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y,
                const void* a, int64_t lda, void* y, int64_t ldy, int32_t nrhs, double alpha, double beta,
                int32_t loc);

/* out[i + j*ldo] = k(x_i, y_j): dense instantiation of the n×m Gramian (column-major), for any n and m (more column strips than a
 * grid's y extent holds are walked inside the kernels).  Only the entries i < n of every column are written: rows n <= i < ldo of out
 * are never touched, with loc == HOST (the staged tile is copied back column by column) as with loc == DEVICE.
 * Routes (info key "last_matrix_path"): d <= 64 keeps x_i in registers (compiled buckets DM = 4, 8, 16, 32, 64; option
 * "matrix_variant" = 1 or d > 64: the generic kernels).  A single profile with d <= 16 writes VR = 4 (fp32) / 2 (fp64) consecutive
 * rows per thread with one 16-byte streaming store per column when n and the leading dimension are multiples of VR and out is
 * 16-byte aligned (loc == HOST: the staged tile has leading dimension n, so only n counts); otherwise one row per thread (VR = 1)
 * with the same arithmetic — the entries do not depend on ldo or on the alignment of out. */
int covgram_matrix(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y,
                   void* out, int64_t ldo, int32_t loc);

/* Multi-GPU form of the symmetric dense MVM (one process per GPU, every rank holds all of x and a): rank r of `world`
 * evaluates the upper-triangle tiles of gramian(k, x) whose 256-row panel p satisfies p % world == r — cyclic, so every rank
 * gets the same share of the triangle — and returns in y (n scalars, device) the partial product of those entries AND their
 * mirror images; the partials of all ranks add up to G a, so ONE all-reduce (RCCL) completes b on every rank
 * (the rows of src/gramian.jl:81 are independent, and so are the unordered pairs {i, j}).
 * fp32: the symmetric matrix-core kernels where they apply (EQ / RQ / Cauchy / IMQ / MaternP(p >= 1) / Dot^p / ExponentialDot, d <= 32, norm
 * gate, n from 12500 ... 18000 by profile or option "mfma_sym" = 1).  Where NO matrix-core kernel takes the pair (Exponential,
 * gamma-exponential, MaternP(0), clouds outside the norm gate) and in fp64 (the reference's default element type): the direct-difference
 * symmetric kernels over the cyclic row blocks p % world == rank (64 rows in fp64, 64 R rows in fp32, R = 4 / 2 / 1 for d <= 8 / 32 / 64) —
 * any single profile without a Power wrapper, d <= 64, as long as one rank's column-sum slab, ceil(row blocks / world) x n scalars, stays
 * within 2 GiB (it lives in the ctx's workspace).  `*supported` of covgram_mvm_sym_supported says so for the given `world` (identically on
 * every rank: it depends on k, x and world only), and covgram_mvm_sym_partial returns COVGRAM_EUNSUPPORTED exactly when it says 0 —
 * callers then shard rows and all-gather (covgram_mvm). */
int covgram_mvm_sym_supported(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, int32_t world, int32_t* supported);
/* Aliasing (covgram_mvm_sym_partial): a and y may overlap in any way; a is then read from a private copy. */
int covgram_mvm_sym_partial(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const void* a, void* y,
                            int32_t rank, int32_t world);

/* ---- the collective behind the ABI (round 5) ------------------------------------------------------------------------------
 * One process per GPU; a ctx can own ONE RCCL communicator, and the multi-GPU MVMs below enqueue their single collective on the
 * ctx stream right behind the kernels (no second stream, no host synchronisation): the GPU analogue of the reference's only
 * parallel axis, `@threads for i in 1:n` over the output rows of mul! (src/gramian.jl:78-87).
 *   covgram_comm_unique_id   rank 0 calls it once and hands the COVGRAM_COMM_ID_BYTES bytes to the other ranks by any means of the
 *                            caller's (MPI.jl's bcast, a torch.distributed store, a file): nothing else crosses processes outside RCCL.
 *   covgram_comm_create      collective over all `world` ranks (ncclCommInitRank on the ctx's device).  RCCL is resolved at this first
 *                            use (dlopen of librccl.so.1 — in a PyTorch process the copy torch has loaded): single-GPU callers never load it.
 *   covgram_comm_destroy     also done by covgram_ctx_destroy.      covgram_comm_info: rank and world (world = 0: no communicator).
 *   covgram_comm_all_gather / covgram_comm_all_reduce_sum   the two collectives themselves on device buffers, stream-ordered (a block
 *                            Gramian's shards, a caller's own vectors); all_gather may run in place (send == recv + rank * count).
 *   covgram_mvm_sharded      y <- alpha G(k; X, Y) a + beta y with y COMPLETE ON EVERY RANK.  X (all n row points), Y, a and y are
 *                            replicated device data; rank r evaluates the rows [r per, (r + 1) per), per = ceil(n / world), with the
 *                            single-GPU kernels — straight into its slice of y when world divides n, the all-gather then in place — and
 *                            ONE ncclAllGather completes y, which is the replicated `a` of the next Krylov iteration.  One right-hand side.
 *                            Aliasing: a and y may overlap in any way; a is then read from a private copy.
 *   covgram_mvm_sym_allreduce  the same product of gramian(k, x) in the symmetric form: covgram_mvm_sym_partial(rank, world) + ONE
 *                            ncclAllReduce; COVGRAM_EUNSUPPORTED exactly when covgram_mvm_sym_supported says 0 (then: covgram_mvm_sharded). */
#define COVGRAM_COMM_ID_BYTES 128
int covgram_comm_unique_id(void* id, int64_t bytes);
int covgram_comm_create(covgram_ctx* ctx, const void* unique_id, int32_t rank, int32_t world);
int covgram_comm_destroy(covgram_ctx* ctx);
int covgram_comm_info(const covgram_ctx* ctx, int32_t* rank, int32_t* world);
int covgram_comm_all_gather(covgram_ctx* ctx, const void* send, void* recv, int64_t count, int32_t dtype);
int covgram_comm_all_reduce_sum(covgram_ctx* ctx, void* buf, int64_t count, int32_t dtype);
int covgram_mvm_sharded(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* a,
                        void* y, double alpha, double beta);
int covgram_mvm_sym_allreduce(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const void* a, void* y, double alpha,
                              double beta);

/* Gradient-kernel Gramian (nd × md): Y <- alpha * G A + beta * Y with flat point-major block vectors as the columns of
 * A (m*d × nrhs, lda >= m*d) and Y (n*d × nrhs, ldy >= n*d), column-major; a vector is nrhs = 1 (lda, ldy then unused beyond the check).
 * blockmul! takes vectors of matrices and the block mul! broadcasts over their columns (src/gramian.jl:241-257, src/gradient.jl:86-92):
 * two right-hand sides share one pass over the pairs (r, phi', phi'' evaluated once) where the lane-per-row kernel holds two
 * accumulators (fp64 d <= 32, fp32 d <= 64, single profiles without a Power wrapper); otherwise one pass per column. */
int covgram_grad_mvm(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* a,
                     int64_t lda, void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t loc);

/* Value-and-gradient Gramian (n(d+1) × m(d+1)), src/gradient.jl:400-474 with the block mul! of :319-351: block (i,j) is
 *     [ k(x_i,y_j)        (d/dy k)^T      ]
 *     [ d/dx k            d/dx d/dy^T k   ]
 * flat point-major block vectors: entry i*(d+1) is the value component, i*(d+1)+1+l the l-th gradient component; right-hand sides
 * as for covgram_grad_mvm (lda >= m*(d+1), ldy >= n*(d+1)).
 * Aliasing (covgram_grad_mvm and covgram_valgrad_mvm): a and y may overlap in any way; a is then read from a private copy. */
int covgram_valgrad_mvm(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* a,
                        int64_t lda, void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t loc);

/* The same two block Gramians for a Sum / Product / Power whose factors do NOT share one input trait — GenericInput in the reference's
 * terms, its gradient algebra of src/gradient_algebra.jl:6-36 (Sum) and :47-89 (Product) — in ONE fused pass over the pairs.
 * value = 0: the blocks and vectors of covgram_grad_mvm; value = 1: those of covgram_valgrad_mvm (blocks of d + 1, the value first).
 * k is the composite of covgram_kernel_composite, k(x, y) = head.scale sum_t prod_f factor(x, y); this entry is the one that reads the
 * `trait` of every factor instead of the head's (head.trait is not read; head.power = 1 and head.lengthscale = 1 as everywhere).
 * Factors: COVGRAM_CONSTANT; the isotropic profiles that are smooth at zero distance — EQ, RQ, Cauchy, IMQ, MaternP(p >= 1) —, each
 * with its own lengthscale, on |x - y|^2 formed by direct differences of the stored coordinates (no centring, no expanded form); the
 * dot-product profiles Dot, ExponentialDot, AsinDot on x.y; COVGRAM_NEURALNETWORK (param = sigma) on the raw points; every one with
 * its own power >= 1 and scale.  Exponential, GammaExponential, MaternP(0) (singular at zero distance) and Matern(nu) are
 * COVGRAM_EUNSUPPORTED with a message that names the leaf.  Every factor is a function F(p, q, s) of p = x.y, q = |x|^2, s = |y|^2; the
 * composite's first and second partial derivatives follow from the factors' by the sum and Leibniz rules, and block (i, j) applied to
 * a_j costs O(d):  b_i += F_p a_j + (F_pp t + 2 F_ps w) y_j + 2 (F_qp t + 2 F_qs w) x_i,  t = x_i.a_j, w = y_j.a_j.  A product that is
 * zero at a pair is an ordinary number here (the reference throws DomainError there, src/gradient_algebra.jl:74-76).
 * Routes (info key "last_grad_mixed_path", bits: 1 = lane per block row, padded d <= 32; 2 = the two-kernel panel route for wider
 * points; 4 = more than one panel; 8 = the panel's column blocks split over z slices with a fixed-order reduce; 16 = the lane-per-row
 * launch split over the columns with the slab reduce — "last_grad_mixed_jsplit" is that split, 0 if the route did not run; 0 = no block
 * kernel ran: n = 0 or m = 0).  Option "grad_mixed_panel" (0 = automatic: the coefficient slabs within 256 MB) caps the columns of a
 * panel, rounded up to whole column blocks; options "jsplit" and "target_wgs" act on the lane-per-row route as on covgram_grad_mvm.
 * y <- alpha G a + beta y; beta == 0 never reads y; m = 0 gives beta y; nrhs columns run one after the other.  Option "time_kernels"
 * brackets the lane-per-row kernel and the panel route's two kernels.
 * Aliasing: a and y may overlap in any way; a is then read from a private copy. */
int covgram_grad_mvm_mixed(covgram_ctx* ctx, const covgram_kernel_composite* k, const covgram_points* X, const covgram_points* Y,
                           const void* a, int64_t lda, void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t value,
                           int32_t loc);

/* The SCALAR Gramian (n x m) of such a composite — EQ() + Dot(), EQ() * (Dot()^2 + 1), MaternP(2) + Dot()^2 + NN(): GenericInput in the
 * reference's terms, its threaded loop src/gramian.jl:78-87 — with the semantics of covgram_mvm: y <- alpha G a + beta y on nrhs columns
 * (lda >= m, ldy >= n); beta == 0 never reads y; m = 0 gives beta y; n = 0 returns at once; a and y may overlap in any way (a is then read
 * from a private copy).  k is the composite covgram_grad_mvm_mixed takes: head.trait is not read, every factor is validated on its own
 * trait.  Factors: COVGRAM_CONSTANT; every isotropic family — EQ, Exponential, RQ, GammaExponential, Cauchy, IMQ, MaternP(p >= 0),
 * Matern(nu): only the VALUE of a leaf is needed, so the leaves the gradient entry refuses are taken —, each with its own lengthscale, on
 * |x - y|^2 formed by direct differences of the stored coordinates (no centring, no expanded form); Dot, ExponentialDot, AsinDot on x.y;
 * COVGRAM_NEURALNETWORK (param = sigma >= 0) on the raw points; every one with its own power >= 1 and scale.
 * The driver partitions the terms (option "mixed_fuse" = 0, the default).  A term is PLAIN when all its profile factors share one trait
 * and none is NeuralNetwork.  The plain isotropic terms form one single-trait composite and the plain dot-product terms another (one term
 * of one factor: a plain covgram_kernel); each runs on the device-resident a and y through the path behind covgram_mvm — matrix cores,
 * the factored dot product, its own Sum split.  A trait's plain terms stay in the fused kernel where the fused terms evaluate leaves of
 * that trait themselves (EQ * Dot^2 + EQ: one pass), and where covgram_mvm's validation refuses the group.  Terms of Constants only add
 * c sum(a) to every row.  The remaining terms — Products across traits, anything with a NeuralNetwork factor — run in ONE fused kernel:
 * lane per row for padded d <= 32 (buckets 4, 8, 16, 32), chunked beyond (any d); right-hand sides in groups of four accumulators per
 * kernel evaluation, the remainder one by one; a fixed-order column split with a slab reduce (deterministic run to run).  Parts run in
 * the order isotropic, dot product, fused, constant; the first applies beta, the others add.  With nothing to delegate, or with
 * "mixed_fuse" = 1, every term, constants included, runs in the fused kernel.
 * Info key "last_mixed_path", bits: 1 = fused lane-per-row route, 2 = fused chunked route, 4 = isotropic group delegated, 8 = dot-product
 * group delegated, 16 = fused launch split over the columns, 32 = constant term added; 0 = no kernel ran.  "last_mixed_jsplit": the
 * fused split, 0 if the fused kernel did not run.  Options "jsplit", "target_wgs" and "time_kernels" act on the fused kernel as on the
 * dense route (and on the delegated parts as in covgram_mvm). */
int covgram_mvm_mixed(covgram_ctx* ctx, const covgram_kernel_composite* k, const covgram_points* X, const covgram_points* Y, const void* a,
                      int64_t lda, void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t loc);

/* Matrix(G) of the same composite, the semantics of covgram_matrix: out[i + j * ldo] = k(x_i, y_j), column-major, ldo >= n; only the
 * rows i < n of each column are written.  ONE kernel for any d with the per-pair arithmetic of the product (the same r^2, p and
 * interpreter order): lane per row, the columns walked inside the kernel, x_i in registers for d <= 32 and re-read in chunks beyond
 * (info key "last_mixed_matrix_path": 1 = in registers, 2 = chunked; 0 = none yet, or n m == 0). */
int covgram_matrix_mixed(covgram_ctx* ctx, const covgram_kernel_composite* k, const covgram_points* X, const covgram_points* Y, void* out,
                         int64_t ldo, int32_t loc);

/* Hessian-kernel Gramian (n d^2 × m d^2), src/hessian.jl:33-41: block (i,j) is the d^2 × d^2 matrix
 *     T[(a,b),(c,e)] = d^4 k(x_i, y_j) / dx_a dx_b dy_c dy_e,
 * applied in O(d^2) per pair (src/hessian.jl:125-190 isotropic, :227-275 dot product), never formed.  Flat point-major block vectors:
 * entry i*d^2 + a + b*d is component (a, b) of point i (the reference's vec of a d × d matrix); right-hand sides as for covgram_grad_mvm
 * (lda >= m*d^2, ldy >= n*d^2, nrhs columns).  Device path: single profiles whose derivatives up to the fourth have closed forms —
 * EQ, RQ, Cauchy, IMQ with lengthscale and scale; ExponentialDot and Dot (a zero matrix: y <- beta y) — and d <= 32.  A Power wrapper,
 * composites and every other family return COVGRAM_EUNSUPPORTED with a message that names the kernel.  Option "time_kernels" brackets
 * the block kernel; info key "last_hess_path" reports it.
 * Aliasing: a and y may overlap in any way; a is then read from a private copy. */
int covgram_hess_mvm(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* a,
                     int64_t lda, void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t loc);

/* Value-gradient-Hessian-kernel Gramian (n(1+d+d^2) × m(1+d+d^2)), src/hessian.jl:279-325: block (i,j) is the joint covariance of
 * [f, grad f, vec hess f], entry (row functional on x_i, column functional on y_j) of k(x_i, y_j) with the functionals id, d/d._a,
 * d^2/d._a d._b; applied in O(d^2) per pair for isotropic AND dot-product kernels (the reference: :392-479, isotropic only), never
 * formed.  Flat point-major block vectors, block of point i at offset i*(1+d+d^2): entry 0 the value, entries 1..d the gradient, entry
 * 1 + d + a + b*d the Hessian component (a, b) (the order of covgram_hess_mvm); right-hand sides as for covgram_grad_mvm
 * (lda >= m*(1+d+d^2), ldy >= n*(1+d+d^2), nrhs columns).  Device path: the kernels of covgram_hess_mvm — EQ, RQ, Cauchy, IMQ with
 * lengthscale and scale; ExponentialDot and Dot (NOT a zero matrix here: its value and gradient rows and columns are non-zero) — and
 * d <= 32; a Power wrapper, composites and every other family return COVGRAM_EUNSUPPORTED with a message that names the kernel.
 * Option "time_kernels" brackets the block kernel; info key "last_vgh_path" reports it ("last_hess_path" is left alone).
 * Aliasing: a and y may overlap in any way; a is then read from a private copy. */
int covgram_valgradhess_mvm(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* a,
                            int64_t lda, void* y, int64_t ldy, int32_t nrhs, double alpha, double beta, int32_t loc);

/* Dense instantiation of a block Gramian: out[(i B + p) + (j B + q) ldo] = entry (p, q) of block (i, j), the (n B) x (m B) matrix the MVM
 * of the same kind applies (column c is that MVM applied to the unit vector e_c), column-major, point-major blocks, with the ordering
 * inside a block that the MVM's comment above fixes: the value first, then the gradient, then Hessian component (a, b) at a + b d.
 * Any n and m (0: nothing is written); ldo >= n B, else COVGRAM_EINVAL; only the rows < n B of each column are written, with loc == HOST
 * as with loc == DEVICE.  r = x_i - y_j is a direct difference (no expanded form, no radius gate).  Kernels: those of the MVM of the
 * same kind with the same refusals — gradient / value-gradient: single profiles of both traits, Power wrappers, MaternP, Matern(nu),
 * Sum / Product composites, with the rows in registers (d <= 64); Hessian / value-gradient-Hessian: EQ, RQ, Cauchy, IMQ, ExponentialDot
 * and Dot (under COVGRAM_BLOCK_HESSIAN a matrix of zeros, which IS written), d <= 32, everything else COVGRAM_EUNSUPPORTED with a message
 * that names the kernel.  A thread writes VR = 4 (fp32) / 2 (fp64) consecutive rows with one 16-byte streaming store per column when
 * B and ldo are multiples of VR and out is 16-byte aligned (loc == HOST: the staged tile has leading dimension n B), otherwise one row
 * (VR = 1) with the same arithmetic: the entries do not depend on ldo or on the alignment of out.  Info key "last_block_matrix_path";
 * option "time_kernels" brackets the kernel. */
#define COVGRAM_BLOCK_GRADIENT 0               /* B = d            blocks of covgram_grad_mvm        */
#define COVGRAM_BLOCK_VALUE_GRADIENT 1         /* B = d + 1        blocks of covgram_valgrad_mvm     */
#define COVGRAM_BLOCK_HESSIAN 2                /* B = d*d          blocks of covgram_hess_mvm        */
#define COVGRAM_BLOCK_VALUE_GRADIENT_HESSIAN 3 /* B = 1 + d + d*d  blocks of covgram_valgradhess_mvm */
int covgram_block_matrix(covgram_ctx* ctx, int32_t kind, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, void* out,
                         int64_t ldo, int32_t loc);

/* ---- sparse(G, delta): the Gramian of an exponentially decaying isotropic kernel thresholded at its decay radius (src/sparse.jl:5-38) ----
 * covgram_decay_radius: the distance R beyond which |k| < delta, for ONE isotropic profile (needs no device), src/sparse.jl:25-38:
 *     EQ  sqrt(-2 ln de)    Exponential  -ln de    GammaExponential(g)  (-2 ln de)^(1/g)    MaternP(p), Matern(nu >= 1/2)  -ln de (conservative)
 * times the lengthscale, with de = delta / |scale|.  Two deliberate corrections of the reference: (1) src/sparse.jl:38 drops its delta
 * argument and DIVIDES by l, but Lengthscale(k, l) evaluates k(r / l), so R = l r0; (2) a Constant factor c (the spec's `scale`) is
 * honoured: c k(r) < delta exactly when k(r) < delta / |c|.  0 < delta / |scale| < 1 is required (COVGRAM_EINVAL), Matern(nu < 1/2) is the
 * reference's DomainError (COVGRAM_EINVAL, "DomainError: ..."); RQ, Cauchy, IMQ, the dot-product families, a Power wrapper and composites
 * have no decay radius: COVGRAM_EUNSUPPORTED with a message that names the kernel (the reference's TypeError branch).
 *
 * covgram_sparse_create builds S = sparse(gramian(k, X, Y), delta) on the device:
 *   - pattern: entry (i, j) is kept exactly when s_ij <= R^2, R = the decay radius above (R^2 rounded to the points' precision),
 *     s_ij = sum_l (x_il - y_jl)^2 formed from the STORED coordinates by direct differences (src/util.jl:40-47), one explicit fused
 *     multiply-add per dimension in ascending l, in the points' own precision; the comparison is inclusive, as the ball tree's inrange is;
 *     no centring, no expanded form and no radius gate on this path;
 *   - value: k(x_i, y_j) of that s_ij, with the library's usual profile evaluation (that of covgram_matrix: scale phi(s / l^2));
 *   - layout: CSR, 0-based: rowptr n + 1 int64, colind nnz int32 ascending within every row, vals nnz scalars of the points' dtype;
 *     m >= 2^31 is COVGRAM_EINVAL;
 *   - n = 0 or m = 0: a valid handle with nnz = 0;
 *   - deterministic: count, scan, fill — integer counts scanned in a fixed order, every lane walks its row's columns in ascending order — the
 *     three arrays are bit-identical from run to run;
 *   - memory: the stream is synchronised once to learn nnz before colind and vals are allocated; if they do not fit: COVGRAM_ENOMEM with a
 *     message that states nnz.  It is synchronised again before returning: the handle keeps no reference to X or Y, which may be
 *     destroyed (or, if borrowed, changed) at once;
 *   - any d >= 1 (rows in registers up to d = 64), fp32 and fp64; X and Y follow the rules of covgram_mvm: one ctx, one dtype, one d;
 *   - a row's fill count that differs from its count is COVGRAM_EHIP "internal: count/fill mismatch" (both passes run ONE predicate, and
 *     the fill never writes at or beyond the next row's offset).
 * covgram_sparse_info: any output pointer may be NULL.  covgram_sparse_export copies the three arrays to caller memory (loc: host or
 * device; a NULL pointer skips that array).
 * covgram_sparse_mvm: y <- alpha S a + beta y for nrhs columns, column-major (lda >= m, ldy >= n), loc applies to a and y; beta == 0 never
 * reads y; 1, 4, 16 or 64 lanes per row (from nnz / n), partial sums folded in a fixed order, no atomics: bit-identical from run to run.
 * Aliasing: a and y may overlap in any way; a is then read from a private copy.
 * Option "time_kernels" brackets the fill kernel of covgram_sparse_create and the product kernel. */
int covgram_decay_radius(const covgram_kernel* k, double delta, double* radius);
int covgram_sparse_create(covgram_ctx* ctx, covgram_sparse** out, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y,
                          double delta);
int covgram_sparse_info(const covgram_sparse* S, int64_t* n, int64_t* m, int64_t* nnz, int32_t* dtype, double* radius);
int covgram_sparse_export(const covgram_sparse* S, int64_t* rowptr, int32_t* colind, void* vals, int32_t loc);
int covgram_sparse_mvm(covgram_sparse* S, const void* a, int64_t lda, void* y, int64_t ldy, int32_t nrhs, double alpha, double beta,
                       int32_t loc);
int covgram_sparse_destroy(covgram_sparse* S);

/* ---- BarnesHutFactorization: the tree-based approximate product of a scalar isotropic Gramian (src/barneshut.jl:25-190) ----
 * covgram_bh_create builds, once per (k, X, Y), a binary ball tree over the COLUMN points Y on the device:
 *   - a node owns the range [lo, hi) of a permutation `indices` of 0 .. m-1; a range of more than `leafsize` points (reference default 16)
 *     is sorted along its dimension of widest extent and split BY POSITION at lo + ceil((hi - lo) / 2), so duplicated points split like
 *     any others and the depth is at most ceil(log2(m / leafsize)) + 1; the shape of the tree therefore depends on (m, leafsize) only;
 *   - nodes are numbered in pre-order: the root is node 0 and the left child of v is v + 1; a leaf has left = right = -1;
 *   - every node has a centre (the midpoint of its bounding box) and a radius such that each of its points lies within the radius of
 *     the centre (distances in fp64, rounded up to the points' precision);
 *   - deterministic: exact minima / maxima and a radix sort whose result depends on its input alone — bit-identical from run to run;
 *   - the handle keeps tree-ordered COPIES of both point sets (the targets X are ordered along the tree when X and Y are the same
 *     device points, otherwise along a tree of their own): X and Y may be destroyed, or changed, when create returns;
 *   - kernels: ONE isotropic profile (EQ, Exponential, RQ, GammaExponential, Cauchy, IMQ, MaternP, Matern) under lengthscale, scale and
 *     power.  Dot-product families and composites are COVGRAM_EUNSUPPORTED by name, before any launch; 1 <= d <= 8 (points in registers),
 *     larger d is COVGRAM_EUNSUPPORTED naming the limit; theta < 0 or leafsize < 1 is COVGRAM_EINVAL; fp32 and fp64;
 *   - n = 0 or m = 0 give a valid handle (m = 0: no nodes).
 * covgram_bh_info: any output pointer may be NULL.  covgram_bh_export copies indices[m], per node lo, hi, left, right (int32), the
 * centres (nnodes x d, node-major) and the radii (nnodes) in the points' dtype to caller memory (host or device; NULL skips an array).
 * covgram_bh_moments: the first stage of a product for the weights w (m scalars): sums[v] = sum of w_j over node v and
 * com[v] = sum |w_j| y_j / (sum |w_j| + eps(T)) (nnodes x d), src/barneshut.jl:157-163 — accumulated in fp64 for both dtypes, leaves
 * first, then every parent from its two children (no floating-point atomics), rounded to T once.  A node whose weights are all zero
 * has com = 0 and sums = 0.
 * covgram_bh_mvm: y <- alpha (F a) + beta y [+ alpha D a], one right-hand side; beta == 0 never reads y; a and y may be the same memory.
 *   For every target x_i the tree is walked from the root: a leaf adds sum_j k(x_i, y_j) a_j by direct differences; an internal node
 *   with radius < theta |x_i - com[v]| adds k(x_i, com[v]) sums[v]; otherwise both children are visited (src/barneshut.jl:123-143).  The
 *   criterion is evaluated per target; the terms a target receives are exactly the recursion's, added in pre-order.
 *   theta < 0: the handle's; theta = 0: the exact product.  split != 0: BH(a+) - BH(a-) with a+ = max(a, 0), a- = max(-a, 0)
 *   (src/barneshut.jl:101-112): both signs carry their own moments and share one walk; an empty sign adds exact zeros, so the weights are
 *   never inspected on the host.  split == 0: the single pass on a as it is.  (The reference's mul! sends signed weights to taylor!:
 *   that product is covgram_bh_taylor_mvm below.)
 *   diag: NULL, or diag_len = 1 or n scalars of the points' dtype (n == m): the diagonal D of src/barneshut.jl:92-94.
 *   With loc == DEVICE the product is stream-ordered, allocates nothing and never synchronises: a captured graph may contain it.
 *   m = 0: y <- beta y.  n = 0: returns at once.  Option "time_kernels" brackets the walk kernel. */
int covgram_bh_create(covgram_ctx* ctx, covgram_bh** out, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, double theta,
                      int32_t leafsize);
int covgram_bh_info(const covgram_bh* F, int64_t* n, int64_t* m, int32_t* d, int32_t* dtype, int64_t* nnodes, int32_t* leafsize, double* theta);
int covgram_bh_export(const covgram_bh* F, int32_t* indices, int32_t* lo, int32_t* hi, int32_t* left, int32_t* right, void* centers, void* radii,
                      int32_t loc);
int covgram_bh_moments(covgram_bh* F, const void* w, void* sums, void* com, int32_t loc);
int covgram_bh_mvm(covgram_bh* F, const void* a, void* y, double alpha, double beta, double theta, int32_t split, const void* diag, int64_t diag_len,
                   int32_t loc);
/* taylor! (src/taylor.jl:7-57): the first-order expansion of the far field, one pass for weights of any sign.
 * covgram_bh_taylor_moments: per node sums[v] = sum w_j (signed), the expansion centre centers[v] (nnodes x d) — use_com != 0: the
 *   |w|-weighted centre of mass of covgram_bh_moments; use_com == 0: the ball centre of covgram_bh_export, which does not depend on w —
 *   and the centred signed first moment m1[v] = sum w_j y_j - sums[v] centers[v] (nnodes x d).  sum w_j y_j is accumulated in fp64 in the
 *   schedule of covgram_bh_moments; m1 is centred in fp64 about the centre AS ROUNDED TO T and then rounded to T once.  A NULL output
 *   pointer skips that array.
 * covgram_bh_taylor_mvm: y <- alpha (T a) + beta y [+ alpha D a] with the walk, the arguments, the status codes and the m = 0 / n = 0
 *   behaviour of covgram_bh_mvm.  A leaf adds its direct sum; an internal node with radius < theta |x_i - centers[v]| adds
 *   f0(s) sums[v] - 2 f1(s) (x_i - centers[v]) . m1[v], s = |x_i - centers[v]|^2, f0 the kernel as a function of the squared distance
 *   and f1 = d f0 / d s (src/taylor.jl:43-50).  The criterion is strict, so s > 0 wherever f1 is evaluated.  With use_com == 0 the
 *   product is an exactly linear map of a (the centres and the set of compressed nodes do not depend on a); with use_com != 0 and
 *   a >= 0 it is the single pass of covgram_bh_mvm up to rounding (m1 is then rounding-level). */
int covgram_bh_taylor_moments(covgram_bh* F, const void* w, int32_t use_com, void* sums, void* centers, void* m1, int32_t loc);
int covgram_bh_taylor_mvm(covgram_bh* F, const void* a, void* y, double alpha, double beta, double theta, int32_t use_com, const void* diag,
                          int64_t diag_len, int32_t loc);
int covgram_bh_destroy(covgram_bh* F);

/* Toeplitz T[i,j] = vc[i-j] (i >= j), vr[j-i] (i < j); vr == NULL: symmetric (vr = vc, m = n).
 * circulant != 0: T[i,j] = vc[(i-j) mod n] (vr must be NULL).  The spectrum of the circulant embedding
 * (N = next power of two >= n+m-1, real-to-complex rocFFT) is computed once here and cached.
 * Aliasing (covgram_toeplitz_mvm): a and y may overlap in any way; a is then read from a private copy. */
int covgram_toeplitz_create(covgram_ctx* ctx, covgram_toeplitz** out, const void* vc, const void* vr, int64_t n,
                            int64_t m, int32_t dtype, int32_t loc, int32_t circulant);
int covgram_toeplitz_mvm(covgram_toeplitz* T, const void* a, void* y, double alpha, double beta, int32_t loc);
int covgram_toeplitz_destroy(covgram_toeplitz* T);

/* Direct solvers of src/toeplitz.jl for the symmetric positive definite Toeplitz matrix K = SymmetricToeplitz([1; r])
 * (UNIT diagonal; r = the first column without its leading 1 — callers with T.vc[0] = r_0 != 1 pass vc[1:] / r_0 and scale the
 * result by 1 / r_0, src/toeplitz.jl:100-111 with its inverted `r_0 == 1` test put right):
 *   covgram_toeplitz_durbin    replaces durbin!(y, r)        src/toeplitz.jl:12-27    y = K_n \ (-r), K_n = SymmetricToeplitz([1, r[1:n-1]]), n = length(r)
 *   covgram_toeplitz_levinson  replaces levinson!(x, r, b)   src/toeplitz.jl:75-98    x = K \ b, n = length(b) = length(r) + 1
 *   covgram_toeplitz_trench    replaces trench!(B, r)        src/toeplitz.jl:52-71    B = inv(K), n x n column-major (ldb), BOTH triangles filled
 * Durbin / Levinson are chains of n - 1 dependent steps: one workgroup walks them in ONE launch that cannot be interrupted (n <= 16384: state
 * in registers and LDS, 28 ms at n = 16384 fp64; above: vectors in global memory, ~8 us a step — n = 65536: 0.5 s; it grows with n^2), so all
 * three return COVGRAM_EUNSUPPORTED above COVGRAM_TOEPLITZ_DIRECT_MAX_N: larger systems are
 * for the circulant-preconditioned CG over covgram_toeplitz_mvm (covgram/solve.py: toeplitz_solve; julia/CovGram.jl: `\`). */
#define COVGRAM_TOEPLITZ_DIRECT_MAX_N 65536
int covgram_toeplitz_durbin(covgram_ctx* ctx, const void* r, int64_t n, void* y, int32_t dtype, int32_t loc);
int covgram_toeplitz_levinson(covgram_ctx* ctx, const void* r, const void* b, int64_t n, void* x, int32_t dtype, int32_t loc);
int covgram_toeplitz_trench(covgram_ctx* ctx, const void* r, int64_t n, void* B, int64_t ldb, int32_t dtype, int32_t loc);

/* The vector work of ONE conjugate-gradient iteration, after the caller's Ap = A p (covgram_mvm & co.) — the recurrences of
 * IterativeSolvers.cg! 0.9.2, the reference's caller of mul! for `G \ b` (src/gramian.jl:229-238, src/lazy_linear_algebra.jl:135-144),
 * without preconditioner:   alpha = rho / (p . Ap);  x += alpha p;  r -= alpha Ap;  rho' = r . r;  p = r + (rho' / rho) p.
 * Three launches, all scalars on the device, sums in a fixed order.  Device pointers only.  scal: 2 + 512 elements of the vectors'
 * type; the caller sets scal[1] = r . r before the first step; after a step scal[1] = rho' (= |r|^2: the residual test) and
 * scal[0] = the rho it divided by.  The rest of scal is scratch. */
int covgram_cg_step(covgram_ctx* ctx, int64_t n, int32_t dtype, void* x, void* r, void* p, const void* Ap, void* scal);
/* The same step for A = G + Diagonal(diag) (the reference's G + sigma^2 I, kept lazy: src/gramian.jl:55-60, src/lazy_linear_algebra.jl:126-133)
 * after the caller's Ap = G p of the Gramian ALONE: the first launch completes Ap <- Ap + diag .* p in the pass that takes p . Ap, and the
 * last one leaves |r| = sqrt(rho') in scal[2 + 512] — the diagonal term and the residual norm cost no launch of their own (a graph-replayed
 * iteration at n = 16384 is launch-bound: tools/cg_rate.py).  diag: n device entries, or NULL (no shift).  scal: 2 + 512 + 1 elements. */
int covgram_cg_step_shifted(covgram_ctx* ctx, int64_t n, int32_t dtype, void* x, void* r, void* p, void* Ap, void* scal, const void* diag);

/* Batched CG: the vector work of ONE iteration of nrhs INDEPENDENT conjugate-gradient recurrences that share the caller's matrix
 * right-hand-side product AP = G P (covgram_mvm & co. with nrhs columns) and stop column by column (covgram/solve.py: mbcg).  The
 * recurrences are those of covgram_cg_step per column; their coefficients are the Lanczos coefficients of stochastic Lanczos
 * quadrature (covgram/solve.py: cg_tridiagonals, logdet).  X, R, P, AP, Z: column-major n x nrhs DEVICE arrays of `dtype` with leading
 * dimensions >= n (the layout of covgram_mvm); diag: n entries or NULL.
 * state: COVGRAM_BCG_STATE_DOUBLES(nrhs) DEVICE doubles, fp64 whatever the vectors' type; field f of column j is
 * state[f * nrhs + j]:
 *   COVGRAM_BCG_RZ      rz_j = R_j . Z_j of the current direction          COVGRAM_BCG_TOL2    the absolute threshold on |r_j|^2
 *   COVGRAM_BCG_RR      rr_j = R_j . R_j                                    COVGRAM_BCG_ACTIVE  1 while column j iterates, else 0
 *   COVGRAM_BCG_ITERS   the iterations column j has taken
 * and the rest (three more fields and two slabs of COVGRAM_BCG_SLAB workgroup partials per column) is scratch.
 * n_active: ONE device int32, the number of active columns — the only word a caller needs to read back.
 * alpha_log, beta_log: DEVICE doubles, row-major (iterations x nrhs), or NULL; a step writes row `it` (it >= 0).
 *
 * Update phase, after AP = G P:   AP_j += diag .* P_j (diag != NULL);  gamma_j = P_j . AP_j;
 *     alpha_j = (active_j && rz_j != 0 && gamma_j != 0) ? rz_j / gamma_j : 0;  X_j += alpha_j P_j;  R_j -= alpha_j AP_j;  rr_j = R_j . R_j.
 * Direction phase, Z = R without a preconditioner, else the caller's Z = M^-1 R:   rz'_j = R_j . Z_j;
 *     beta_j = (active_j && rz_j != 0) ? rz'_j / rz_j : 0;  P_j = Z_j + beta_j P_j;  alpha_j, beta_j logged at row `it`;
 *     for active columns rz_j <- rz'_j and iters_j += 1;  active_j &= rr_j > tol2_j;  n_active = the number of active columns.
 * An inactive column is frozen: X_j, R_j, rr_j, rz_j are not written (bitwise unchanged), its logged coefficients are 0 and P_j = Z_j;
 * the 0 / 0 guards are covgram_cg_step's, per column, so no NaN reaches X and a column with R = P = 0 stays exactly 0.
 * Every sum runs in a fixed order (wave shuffles, LDS, then a per-column slab of workgroup partials that the NEXT launch reduces; no
 * floating-point atomic), column j's outputs depend on column j's inputs alone: equal columns and repeated calls give equal bits.
 *
 *   covgram_bcg_init       rz_j = R_j . Z_j, rr_j = R_j . R_j, tol2_j = max(reltol^2 rr_j, abstol^2), active_j = rr_j > tol2_j,
 *                          iters_j = 0, n_active (Z = R without a preconditioner).  One launch, one workgroup per column.
 *   covgram_bcg_step       both phases with Z = R (rz' = rr: the second dot is free).  Columns of at most 16384 fp32 / 8192 fp64 entries
 *                          whose addresses are all multiples of 16 bytes: ONE launch of nrhs workgroups, each holding its column of P, AP
 *                          and R in registers.  Otherwise three launches on a (row blocks x columns) grid.
 *   covgram_bcg_update     the update phase alone (two launches); rr_j is committed by the direction phase that follows.
 *   covgram_bcg_direction  the direction phase alone with the caller's Z (two launches).
 * n, nrhs >= 0, every leading dimension >= n, it >= 0, dtype F32 / F64 — else COVGRAM_EINVAL, checked before any device call.  n = 0 or
 * nrhs = 0: nothing is done.  Nothing synchronises with the host. */
#define COVGRAM_BCG_SLAB 64
#define COVGRAM_BCG_RZ 0
#define COVGRAM_BCG_TOL2 1
#define COVGRAM_BCG_RR 2
#define COVGRAM_BCG_ACTIVE 3
#define COVGRAM_BCG_ITERS 4
#define COVGRAM_BCG_FIELDS 8
#define COVGRAM_BCG_STATE_DOUBLES(nrhs) ((int64_t)(nrhs) * (COVGRAM_BCG_FIELDS + 2 * COVGRAM_BCG_SLAB))
int covgram_bcg_init(covgram_ctx* ctx, int64_t n, int64_t nrhs, int32_t dtype, const void* R, int64_t ldr, const void* Z, int64_t ldz,
                     double reltol, double abstol, double* state, int32_t* n_active);
int covgram_bcg_step(covgram_ctx* ctx, int64_t n, int64_t nrhs, int32_t dtype, void* X, int64_t ldx, void* R, int64_t ldr, void* P,
                     int64_t ldp, void* AP, int64_t ldap, const void* diag, double* state, int32_t* n_active, double* alpha_log,
                     double* beta_log, int64_t it);
int covgram_bcg_update(covgram_ctx* ctx, int64_t n, int64_t nrhs, int32_t dtype, void* X, int64_t ldx, void* R, int64_t ldr, const void* P,
                       int64_t ldp, void* AP, int64_t ldap, const void* diag, double* state, double* alpha_log, int64_t it);
int covgram_bcg_direction(covgram_ctx* ctx, int64_t n, int64_t nrhs, int32_t dtype, const void* R, int64_t ldr, const void* Z, int64_t ldz,
                          void* P, int64_t ldp, double* state, int32_t* n_active, double* beta_log, int64_t it);

/* Y <- alpha * (F_1 ⊗ F_2 ⊗ ... ⊗ F_q) A + beta * Y, standard Kronecker order (F_1 = slowest index).
 * factors[i]: dense rows[i]×cols[i] column-major matrix with leading dimension lds[i] (device or host per loc).
 * A: (prod cols)×nrhs (lda), Y: (prod rows)×nrhs (ldy), column-major; a vector is nrhs = 1.  Hand-written mode-product kernels on the
 * matrix cores of the data's own precision (csrc/kron.hip): the last two modes in ONE pass when cols[q-1] <= 128, so q = 3 costs two
 * passes over the tensor; a mode whose factor has a side >= 1024 (a compute-bound dense GEMM) goes to rocBLAS.
 * Aliasing: A and Y may overlap in any way (Y = A: an in-place product of a square operator); A is then read from a private copy. */
int covgram_kron_mvm(covgram_ctx* ctx, const void* const* factors, const int64_t* rows, const int64_t* cols,
                     const int64_t* lds, int32_t q, int32_t dtype, const void* a, int64_t lda, void* y, int64_t ldy,
                     int32_t nrhs, double alpha, double beta, int32_t loc);

/* Y <- alpha * U (V' A) + beta * Y;  U: n×r (ldu), V: m×r (ldv), A: m×nrhs (lda >= m), Y: n×nrhs (ldy >= n), column-major.
 * nrhs >= 8: both tall-skinny products run on the matrix cores in the data's own precision (v_mfma_f32_32x32x2_f32 /
 * v_mfma_f64_16x16x4_f64); fewer right-hand sides: streaming GEMV kernels, one pair per column.
 * Aliasing: A and Y may overlap in any way; A is then read from a private copy. */
int covgram_lowrank_mvm(covgram_ctx* ctx, const void* U, int64_t ldu, const void* V, int64_t ldv, int64_t n, int64_t m,
                        int64_t r, int32_t dtype, const void* a, int64_t lda, void* y, int64_t ldy, int32_t nrhs,
                        double alpha, double beta, int32_t loc);

/* P' G P ~= L L' by diagonal pivoting for the symmetric Gramian G = k(X, X) of ONE isotropic profile, never forming G: the set-up of a
 * low-rank preconditioner for CG on G + D (covgram/factorize.py: PivotedCholeskyPreconditioner), entirely on the device.  The
 * semantics are LAPACK pstrf's, as oracle.pivoted_cholesky restates them:
 *   the residual diagonal starts at k(x_i, x_i) = scale phi(0);  step k: p = argmax of the residual diagonal, TIES TO THE SMALLEST
 *   INDEX (inside a workgroup and across workgroups: results are reproducible), stop when !(dmax > tol) (a NaN stops too);
 *   col_i = k(x_i, x_p) - sum_{j<k} L[i,j] L[p,j] (the sum in the order j = 0 .. k-1, fused multiply-adds of the data's type);
 *   L[i,k] = col_i / sqrt(dmax);  dres[i] -= L[i,k]^2;  dres[p] = 0 exactly, and an entry that is exactly zero stays zero (p is retired:
 *   with tol >= 0 a zero is never chosen).
 * k(x_i, x_p) is evaluated with the arithmetic of covgram_matrix (direct differences, unfolded profiles).
 * All outputs are DEVICE pointers: L column-major n x max_rank (ldl >= n, rows in the original order), piv max_rank entries, dres n
 * entries of the points' type (the residual diagonal on return), rank ONE int32.  On return (stream order) rank = the number of columns
 * written, piv[0:rank] = the pivots in order; columns >= rank of L and piv[rank:] are left untouched.
 * One launch per pivot, max_rank launches enqueued back to back on the ctx stream; NOTHING in the call synchronises with the host (the
 * caller reads rank when it needs it), and no workgroup ever waits for another: a launch starts by reducing the previous launch's <= 1024
 * per-workgroup (value, index) partials, and once a launch has decided to stop, every later one returns on a `done` word.
 * Supported: EQ, Exponential, RQ, GammaExponential, Cauchy, IMQ, MaternP, Matern(nu) with Lengthscale, Constant and Power wrappers.
 * Composites and dot-product kernels: COVGRAM_EUNSUPPORTED; max_rank > COVGRAM_PIVCHOL_MAX_RANK: COVGRAM_EUNSUPPORTED; tol < 0 (or NaN),
 * max_rank < 0, max_rank > n, ldl < n: COVGRAM_EINVAL — all checked before any device call.  n = 0 or max_rank = 0 writes rank = 0. */
#define COVGRAM_PIVCHOL_MAX_RANK 1024
int covgram_pivoted_cholesky(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, int32_t max_rank, double tol,
                             void* L, int64_t ldl, int32_t* piv, void* dres, int32_t* rank);

/* ---- SpectralMixture(w, mu, l) = sum_q w_q Cosine(mu_q) ARD(EQ(), l_q) (src/stationary.jl:213-217): the Gramian
 *     G_ij = sum_q w_q cos(2 pi mu_q . (x_i - y_j)) exp(-1/2 sum_k ((x_ik - y_jk) inv_l_qk)^2)
 * in ONE pass over the pairs (csrc/sm.hip).  The kernel mixes two input traits (c . r and |r|^2) and is GenericInput in the reference's
 * terms, so it has no covgram_kernel encoding: a handle carries its parameters instead.
 * covgram_sm_create: w[ncomp], mu and inv_l ncomp x d row-major, HOST arrays of doubles (the only copy from the host on this path);
 *   they are rounded ONCE to `dtype` here.  inv_l = 0 is a component without an EQ factor, mu = 0 one without a Cosine; weights may
 *   have either sign.  ncomp < 1, d < 1, a negative inv_l or a non-finite parameter: COVGRAM_EINVAL; ncomp > COVGRAM_SM_MAX_COMPONENTS
 *   or d > COVGRAM_SM_MAX_D: COVGRAM_EUNSUPPORTED naming the limits.  No kernel is launched.
 * covgram_sm_info: any output pointer may be NULL; isotropic = 1 when every component has one inverse lengthscale over all dimensions
 *   (what Spectral(w, mu, l::Real) gives): the kernels then scale the pair's shared |x - y|^2 instead of its d squared differences.
 * covgram_sm_mvm: y <- alpha G a + beta y with the semantics of covgram_mvm: column-major a (m x nrhs, lda >= m) and y (n x nrhs,
 *   ldy >= n), loc applies to both; beta == 0 never reads y; m == 0 gives y <- beta y, n == 0 returns at once; a and y may overlap in
 *   any way (a is then read from a private copy); any nrhs >= 1 (four right-hand sides share one pass over the pairs).  X and Y must
 *   belong to the handle's ctx and have its dtype and its d (COVGRAM_EINVAL otherwise).  Differences are direct, x_ik - y_jk in the
 *   points' precision: no centring, no expanded form, no radius gate.  With loc == DEVICE the product is stream-ordered, allocates
 *   nothing after the first call of a shape (workspace of the ctx) and never synchronises: a captured graph may contain it.
 *   Column-split partial sums are added in a fixed order, no atomics: bit-identical from run to run.
 * covgram_sm_matrix: out[i + j ldo] = G_ij with the same per-pair arithmetic, column-major, ldo >= n; rows n <= i < ldo of out are
 *   never touched, with loc == HOST (a staged tile copied back column by column) as with loc == DEVICE.  n m == 0: nothing is written.
 * Option "time_kernels" brackets the pair kernel(s) of a call. */
typedef struct covgram_sm covgram_sm;   /* device-resident parameters of one mixture */
#define COVGRAM_SM_MAX_COMPONENTS 32
#define COVGRAM_SM_MAX_D 16
int covgram_sm_create(covgram_ctx* ctx, covgram_sm** out, int32_t ncomp, int32_t d, const double* w, const double* mu, const double* inv_l,
                      int32_t dtype);
int covgram_sm_info(const covgram_sm* S, int32_t* ncomp, int32_t* d, int32_t* dtype, int32_t* isotropic);
int covgram_sm_mvm(covgram_sm* S, const covgram_points* X, const covgram_points* Y, const void* a, int64_t lda, void* y, int64_t ldy,
                   int32_t nrhs, double alpha, double beta, int32_t loc);
int covgram_sm_matrix(covgram_sm* S, const covgram_points* X, const covgram_points* Y, void* out, int64_t ldo, int32_t loc);
int covgram_sm_destroy(covgram_sm* S);

/* ---- Hyper-parameter gradients of the bilinear forms sum_t u_t' G a_t in ONE pass over the pairs (csrc/bilin_grad.hip), with
 * W = U A' (n x m, rank nvec) formed per pair in registers and never stored:
 *     out[0]     = sum_ij W_ij k_ij                          the value: d/dscale = out[0] / scale
 *     out[1]     = sum_ij W_ij dk_ij / dparam                param = the struct's `param`: RQ alpha, gamma-exponential gamma, IMQ c;
 *                                                            0 for the families without one
 *     out[2 + c] = sum_ij W_ij (dk/ds)_ij (x_ic - y_jc)^2     c < d, per_dim != 0; per_dim == 0: the one number out[2] = sum_ij W_ij (dk/ds)_ij s_ij
 * s is the RAW squared distance, formed by direct differences: dk/ds includes scale, power and lengthscale (d/dl = -(2 / l) sum_c out[2 + c]).
 * `out` holds 2 + (per_dim ? d : 1) DOUBLES whatever the points' dtype (host or device memory, `loc`, which also applies to U and A).
 * U is n x nvec (ldu >= n), A is m x nvec (lda >= m), column-major, in the points' dtype; Y == NULL means Y = X.
 * k: a simple isotropic kernel of any family except COVGRAM_MATERN, any power >= 1, scale and lengthscale.  Composites, dot-product
 *   families and COVGRAM_MATERN: COVGRAM_EUNSUPPORTED.  nvec outside 1 .. 32 or d outside 1 .. 64: COVGRAM_EINVAL.
 * A pair at distance 0 (with Y == NULL the whole diagonal) adds exactly 0 to out[2 ..] for every family, also those whose dk/ds is
 *   unbounded at 0, and the finite limit of dk/dparam to out[1].
 * A lane adds at most 128 pairs in the points' precision before the sum continues in fp64; partial sums are added in a fixed order, no
 *   atomics: two calls with the same arguments agree bit for bit.  n m == 0 gives zeros.  With loc == DEVICE the call is stream-ordered
 *   and never synchronises.  Option "time_kernels" brackets the pair kernel and its reduction. */
int covgram_bilinear_grad(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* U, int64_t ldu,
                          const void* A, int64_t lda, int32_t nvec, int32_t per_dim, double* out, int32_t loc);

/* ---- Gradients of the bilinear forms sum_t u_t' G a_t with respect to the ROW points in ONE pass over the pairs (csrc/input_grad.hip),
 * W = U A' as in covgram_bilinear_grad:
 *     dX[i d + c] = sum_j W_ij 2 (dk/ds)_ij (x_ic - y_jc)        i < n, c < d
 * the partial derivative of F(X, Y) = sum_ij W_ij k(x_i, y_j) in x_ic with the column side held FIXED, also when Y == NULL (Y = X): an
 *   isotropic k is symmetric in its arguments, so the derivative in the column points is the call with (X, U) and (Y, A) swapped, and the
 *   full derivative of the symmetric case is call(X, NULL, U, A) + call(X, NULL, A, U).
 * `dX` holds n d DOUBLES, point-major like the points, whatever the points' dtype (host or device memory, `loc`, which also applies to U
 *   and A); nothing outside them is written.  s is the RAW squared distance by direct differences: dk/ds includes scale, power and lengthscale.
 * U, A, k, nvec and d: exactly as covgram_bilinear_grad, with the same status codes.
 * A pair at distance 0 (with Y == NULL the whole diagonal) adds exactly 0 for every family, also those whose dk/ds is unbounded at 0.
 * A lane owns a row: it adds at most 128 pairs in the points' precision before the sum continues in fp64, and partial sums are added in a
 *   fixed order, no atomics: two calls with the same arguments agree bit for bit.  m == 0 gives zeros, n == 0 returns at once.  With
 *   loc == DEVICE the call is stream-ordered and never synchronises.  Option "time_kernels" brackets the pair kernel and its reduction. */
int covgram_bilinear_input_grad(covgram_ctx* ctx, const covgram_kernel* k, const covgram_points* X, const covgram_points* Y, const void* U, int64_t ldu,
                                const void* A, int64_t lda, int32_t nvec, double* dX, int32_t loc);

/* ---- Hyper-parameter gradients of the bilinear forms sum_t u_t' G a_t of a SpectralMixture Gramian in ONE pass over the pairs
 * (csrc/sm_grad.hip), W = U A' as in covgram_bilinear_grad.  With r = x_i - y_j by direct differences, phi_q = 2 pi mu_q . r and
 * e_q = exp(-1/2 sum_k (r_k inv_l_qk)^2), `out` holds ncomp (1 + 2 d) DOUBLES whatever the points' dtype, component-major:
 *     out[q (1 + 2 d)]             = sum_ij W_ij cos phi_q e_q                     dF/dw_q (NOT multiplied by w_q)
 *     out[q (1 + 2 d) + 1 + k]     = sum_ij W_ij (-2 pi w_q) r_k sin phi_q e_q     dF/dmu_qk
 *     out[q (1 + 2 d) + 1 + d + k] = sum_ij W_ij w_q cos phi_q e_q r_k^2           E_qk: dF/d(inv_l_qk^2) = -1/2 E_qk
 * so that the value is sum_q w_q out[q (1 + 2 d)].  w, mu and inv_l are the handle's parameters as covgram_sm_create rounded them.
 * U is n x nvec (ldu >= n), A is m x nvec (lda >= m), column-major, in the points' dtype; `loc` applies to U, A and out; Y == NULL
 *   means Y = X.  X, Y and S must agree in ctx, dtype and d (COVGRAM_EINVAL, as covgram_sm_mvm); nvec outside 1 .. 32 or a NULL out:
 *   COVGRAM_EINVAL.
 * The phases mu_q . x_i and mu_q . y_j are formed per point and reduced in fp64 (as covgram_sm_mvm does); the pair loop has no
 *   trigonometric instruction.  A pair with r = 0 (with Y == NULL the whole diagonal) adds exactly W_ij to the first output of every
 *   component and exactly 0 to the others; rows and columns beyond the sets add exactly 0.
 * A lane adds at most 128 pairs in the points' precision before the sum continues in fp64; partial sums are added in a fixed order, no
 *   atomics: two calls with the same arguments agree bit for bit.  n m == 0 gives zeros.  With loc == DEVICE the call is stream-ordered
 *   and never synchronises.  Option "time_kernels" brackets the phase kernels, the pair kernel and its reduction. */
int covgram_bilinear_grad_sm(covgram_sm* S, const covgram_points* X, const covgram_points* Y, const void* U, int64_t ldu, const void* A,
                             int64_t lda, int32_t nvec, double* out, int32_t loc);

/* ---- Gradients of the bilinear forms sum_t u_t' G a_t of a SpectralMixture Gramian with respect to the ROW points in ONE pass over the
 * pairs (csrc/sm_input_grad.hip), W = U A', r, phi_q and e_q as in covgram_bilinear_grad_sm:
 *     dX[i d + c] = sum_j W_ij sum_q w_q e_q (-2 pi mu_qc sin phi_q - inv_l_qc^2 r_c cos phi_q)        i < n, c < d
 * the partial derivative of F(X, Y) = sum_ij W_ij sum_q w_q cos phi_q e_q in x_ic with the column side held FIXED, also when Y == NULL
 *   (Y = X): the mixture is symmetric in its arguments (cos is even), so the derivative in the column points is the call with
 *   (Y, X, A, U), and the full derivative of the one-point-set case is call(X, NULL, U, A) + call(X, NULL, A, U) — the conventions of
 *   covgram_bilinear_input_grad.
 * `dX` holds n d DOUBLES, point-major like the points, whatever the points' dtype; nothing outside them is written.  U is n x nvec
 *   (ldu >= n), A is m x nvec (lda >= m), column-major, in the points' dtype; `loc` applies to U, A and dX.  w, mu and inv_l are the
 *   handle's parameters as covgram_sm_create rounded them, once, to the points' dtype.
 * X, Y and S must agree in ctx, dtype and d (COVGRAM_EINVAL, as covgram_sm_mvm); nvec outside 1 .. 32 or a NULL dX: COVGRAM_EINVAL.
 * The phases mu_q . x_i and mu_q . y_j are formed per point and reduced in fp64; the pair loop has no trigonometric instruction
 *   (cos phi = cu cv + su sv, sin phi = su cv - cu sv).  A pair with sum_k r_k^2 == 0 (with Y == NULL the whole diagonal) adds exactly 0
 *   to every output: sin phi is replaced by 0 there by a select, next to cos phi := 1.  Rows and columns beyond the sets add exactly 0.
 * A lane owns a row: it adds at most 128 pairs in the points' precision before the sum continues in fp64; the four waves' totals and the
 *   column chunks are added in a fixed order, no atomics: two calls with the same arguments agree bit for bit.  m == 0 gives zeros,
 *   n == 0 returns at once.  With loc == DEVICE the call is stream-ordered, never synchronises, uses the ctx workspace and allocates
 *   nothing after the first call of a shape.  Option "time_kernels" brackets the phase kernels, the pair kernel and its reduction. */
int covgram_bilinear_input_grad_sm(covgram_sm* S, const covgram_points* X, const covgram_points* Y, const void* U, int64_t ldu, const void* A,
                                   int64_t lda, int32_t nvec, double* dX, int32_t loc);

/* ---- Hyper-parameter gradients of the bilinear forms sum_t u_t' G a_t of a MIXED-TRAIT composite in ONE pass over the pairs
 * (csrc/mixed_bilin_grad.hip), W = U A' as in covgram_bilinear_grad.  `k` is the composite of covgram_mvm_mixed: a Sum of terms
 * c_t prod_f psi_f with psi_f = phi_f(z_f)^power_f on the argument of the factor's own trait (isotropic: z = r^2 / l_f^2 with r^2 by direct
 * differences; dot product: p = x.y; COVGRAM_NEURALNETWORK: sigma in `param`), the coefficient c_t = head.scale times the scales of the
 * term's factors.  `out` holds COVGRAM_MIXED_GRAD_NOUT = 24 DOUBLES whatever the points' dtype; f is the FLAT index of a factor in
 * k->factors:
 *     out[t]      = sum_ij W_ij prod_{f in t} psi_f                                t < nterms: term t WITHOUT c_t (constants only: sum W),
 *                                                                                  so that the value is sum_t c_t out[t]
 *     out[8 + f]  = sum_ij W_ij c_t z_f dpsi_f/dz_f prod_{g != f} psi_g            isotropic factors: d/dl_f = -(2 / l_f) out[8 + f]
 *     out[16 + f] = sum_ij W_ij c_t dpsi_f/dtheta_f prod_{g != f} psi_g            theta: RQ alpha, gamma-exponential gamma, IMQ c,
 *                                                                                  NeuralNetwork sigma
 * and every other entry is written as exact 0.0.  The products over the other factors are multiplied up, never divided out.
 * Leaves: EQ, Exponential, RQ, GammaExponential, Cauchy, IMQ, MaternP(p >= 0), each with its own lengthscale; Dot, ExponentialDot,
 *   AsinDot; NeuralNetwork(sigma); Constant.  A COVGRAM_MATERN factor: COVGRAM_EUNSUPPORTED naming the leaf.
 * U, A, ldu, lda, nvec (1 .. 32), d (1 .. 64), Y == NULL, loc and the status codes: as covgram_bilinear_grad.
 * A pair whose scaled z_f is 0 (with Y == NULL the whole diagonal) adds exactly 0 to out[8 + f], also for the leaves whose derivative
 *   is unbounded there, and the finite limit to out[16 + f]; rows and columns beyond the sets add nothing.
 * A lane adds at most 128 pairs in the points' precision before the sum continues in fp64; partial sums are added in a fixed order, no
 *   atomics: two calls with the same arguments agree bit for bit.  n m == 0 gives 24 zeros.  With loc == DEVICE the call is
 *   stream-ordered and never synchronises.  Options: "time_kernels" brackets the pair kernel and its reduction; "jsplit" > 0 fixes the
 *   number of column chunks. */
#define COVGRAM_MIXED_GRAD_NOUT 24 /* COVGRAM_COMPOSITE_MAX_TERMS + 2 * COVGRAM_COMPOSITE_MAX_FACTORS */
int covgram_bilinear_grad_mixed(covgram_ctx* ctx, const covgram_kernel_composite* k, const covgram_points* X, const covgram_points* Y, const void* U,
                                int64_t ldu, const void* A, int64_t lda, int32_t nvec, double* out, int32_t loc);

/* Test hook: the double-precision parameter block handed to the device kernels for `k`
 * (out45[0..8] = gamma, gamma^2, scale, param, c0, 2p+1, Taylor bound, d1, d2; then the MaternP tables
 * H_p, H_{p-1}, H_{p-2} and Taylor coefficients, 9 doubles each).  Needs no device. */
int covgram_debug_kernel_params(const covgram_kernel* k, int32_t dtype, int32_t for_gradient, double* out45);

#ifdef __cplusplus
}
#endif
#endif /* COVGRAM_H */
