# CovGram.jl — the reference-side binding a maintainer would add: `ccall` stubs for libcovgram.so and the methods that route
# the hot path of CovarianceFunctions.jl (v0.3.5) — `gramian` dispatch, `mul!`, `Matrix` — to the MI355X engine.
#
# WRITTEN BLIND: Julia is not installed in the build image, so this file has never been executed.  All logic lives in the C
# library; this shim is declarative (struct mirrors, kernel lowering, ccall).  What CAN be checked without Julia is checked:
# tests/test_host.py::test_julia_shim_mirrors_the_header parses the `struct` blocks and the `ccall` argument-type tuples below
# and compares them with include/covgram.h (tests/abi_layout.c compiles the header and prints sizeof / offsetof of every
# field), so a drift between this file and the header fails the CPU test suite.  At load time the module additionally
# asserts sizeof(CKernel) / sizeof(CComposite) against the library's own covgram_sizeof_*().
# The executed and tested host mirror is the Python package next to it (covgram/).
#
# Usage:   using CovarianceFunctions, CovGram
#          CovGram.enable!()                    # from here on the methods below take the device path where input_trait allows
#          G = gramian(EQ(), X)                 # unchanged, lazy, O(1)
#          mul!(b, G, a)                        # covgram_mvm
#          T = gramian(Exp(), range(-1, 1, length = 2^22))     # DeviceToeplitz (covgram_toeplitz_*)
#
# One context = one device + one stream (include/covgram.h: covgram_ctx_create(ctx, device_id, stream)); a multi-GPU job is
# one Julia process per GPU (MPI.jl), each with its own context — the library holds no multi-device state.
module CovGram

using LinearAlgebra
using SparseArrays
using CovarianceFunctions
using CovarianceFunctions: Gramian, GradientKernel, ValueGradientKernel, HessianKernel, ValueGradientHessianKernel, IsotropicInput, DotProductInput, StationaryInput,
                           GenericInput, input_trait, EQ, RQ, Exp, γExp, Cauchy, InverseMultiQuadratic, MaternP, Dot,
                           ExponentialDot, Lengthscale, Power, Product, Sum, Constant, SeparableProduct, SeparableKernel, LazyGrid, FiniteBasis
import CovarianceFunctions: gramian
import BlockFactorizations

const libcovgram = get(ENV, "COVGRAM_LIB", joinpath(@__DIR__, "..", "lib", "libcovgram.so"))

# ---- struct mirrors of include/covgram.h (field order and types are ABI; checked by tests/test_host.py) ------------------
const COMPOSITE_MAX_TERMS = 8        # COVGRAM_COMPOSITE_MAX_TERMS
const COMPOSITE_MAX_FACTORS = 8      # COVGRAM_COMPOSITE_MAX_FACTORS

# mirrors `covgram_kernel`
struct CKernel
    family::Int32
    trait::Int32
    p::Int32
    power::Int32
    param::Float64
    lengthscale::Float64
    scale::Float64
end

# mirrors `covgram_kernel_composite`: k = head.scale * sum_t prod_f factors; every entry point accepts a pointer to its first
# member (`head`, family = 101) in place of a CKernel
struct CComposite
    head::CKernel
    nterms::Int32
    nfactors::NTuple{8, Int32}
    factors::NTuple{8, CKernel}
end

const F_EQ, F_EXP, F_RQ, F_GAMMAEXP, F_CAUCHY, F_IMQ, F_MATERNP, F_DOT, F_EXPDOT = Int32.(0:8)
const F_CONSTANT, F_COMPOSITE = Int32(100), Int32(101)
const ISO, DOTP = Int32(1), Int32(2)
const HOST, DEVICE = Int32(0), Int32(1)
const ABI_VERSION = 113              # COVGRAM_VERSION of the header these ccall signatures mirror
dtype_code(::Type{Float32}) = Int32(0); dtype_code(::Type{Float64}) = Int32(1)
const DevFloat = Union{Float32, Float64}

function __init__()
    isfile(libcovgram) || return          # enable!() reports the missing library
    v = ccall((:covgram_version, libcovgram), Cint, ())
    v == ABI_VERSION || error("libcovgram.so is ABI version $v, CovGram.jl binds version $ABI_VERSION (include/covgram.h COVGRAM_VERSION): rebuild the library")
    sk = ccall((:covgram_sizeof_kernel, libcovgram), Cint, ())
    sc = ccall((:covgram_sizeof_composite, libcovgram), Cint, ())
    (sk == sizeof(CKernel) && sc == sizeof(CComposite)) ||
        error("CovGram.jl and libcovgram.so disagree on the ABI: covgram_kernel $(sizeof(CKernel)) vs $sk bytes, covgram_kernel_composite $(sizeof(CComposite)) vs $sc")
end

check(rc) = rc == 0 ? nothing :
    (msg = unsafe_string(ccall((:covgram_last_error, libcovgram), Cstring, ()));
     rc == -1 ? throw(DimensionMismatch(msg)) : error("libcovgram status $rc: $msg"))

# ---- lowering: the same closed set `covgram.kernels.device_spec` handles; anything else -> nothing (GenericInput path) ----
lower(k; scale = 1.0, power = 1, l = 1.0) = nothing
lower(::EQ; kw...)            = ckernel(F_EQ, ISO; kw...)
lower(::Exp; kw...)           = ckernel(F_EXP, ISO; kw...)
lower(k::RQ; kw...)           = ckernel(F_RQ, ISO; param = k.α, kw...)
lower(k::γExp; kw...)         = ckernel(F_GAMMAEXP, ISO; param = k.γ, kw...)
lower(::Cauchy; kw...)        = ckernel(F_CAUCHY, ISO; kw...)
lower(k::InverseMultiQuadratic; kw...) = ckernel(F_IMQ, ISO; param = k.c, kw...)
lower(k::MaternP; kw...)      = k.p ≤ 8 ? ckernel(F_MATERNP, ISO; p = k.p, kw...) : nothing
lower(::Dot; kw...)           = ckernel(F_DOT, DOTP; kw...)
lower(::ExponentialDot; kw...) = ckernel(F_EXPDOT, DOTP; kw...)
lower(k::Lengthscale; scale = 1.0, power = 1, l = 1.0) = lower(k.k; scale = scale, power = power, l = l * k.l)
lower(k::Power; scale = 1.0, power = 1, l = 1.0) = k.p ≥ 1 ? lower(k.k; scale = scale, power = power * k.p, l = l) : nothing
function lower(k::Product; scale = 1.0, power = 1, l = 1.0)
    rest = [a for a in k.args if !(a isa Constant)]
    length(rest) == 1 || return nothing
    c = prod(Float64[a.c for a in k.args if a isa Constant]; init = 1.0)
    lower(rest[1]; scale = scale * c^power, power = power, l = l)
end
ckernel(f, t; p = 0, param = 0.0, scale = 1.0, power = 1, l = 1.0) =
    (t == DOTP && l != 1.0) ? nothing : CKernel(f, t, Int32(p), Int32(power), Float64(param), Float64(l), Float64(scale))

# Sum / Product / Power with a common trait (src/algebra.jl:5-63, src/properties.jl:47-63) -> CComposite, or nothing.
# A term is a Product (or a single kernel); each of its non-Constant factors must lower to a CKernel of the common trait.
# (covgram/kernels.py::device_spec is the executed version of this flattening, including the merge of like factors.)
const NOKERNEL = CKernel(F_CONSTANT, Int32(0), Int32(0), Int32(1), 0.0, 1.0, 0.0)
function lower_composite(k)
    terms = k isa Sum ? collect(k.args) : [k]
    length(terms) ≤ COMPOSITE_MAX_TERMS || return nothing
    nfac = zeros(Int32, COMPOSITE_MAX_TERMS); facs = CKernel[]; trait = Int32(0)
    for (t, term) in enumerate(terms)
        parts = term isa Product ? collect(term.args) : [term]
        for part in parts
            f = part isa Constant ? CKernel(F_CONSTANT, Int32(0), Int32(0), Int32(1), 0.0, 1.0, Float64(part.c)) : lower(part)
            f === nothing && return nothing
            if f.family != F_CONSTANT
                trait == 0 && (trait = f.trait)
                trait == f.trait || return nothing                       # mixed traits: GenericInput (src/properties.jl:47-63)
            end
            push!(facs, f); nfac[t] += 1
        end
    end
    (trait != 0 && length(facs) ≤ COMPOSITE_MAX_FACTORS) || return nothing
    while length(facs) < COMPOSITE_MAX_FACTORS; push!(facs, NOKERNEL); end
    CComposite(CKernel(F_COMPOSITE, trait, Int32(0), Int32(1), 0.0, 1.0, 1.0), Int32(length(terms)), Tuple(nfac), Tuple(facs))
end
# what the entry points take: Ref{CKernel}, or Ref{CComposite} (same address as its head)
device_kernel(k) = (s = lower(k); s === nothing ? lower_composite(k) : s)
device_kernel_for(k) = ENABLED[] && input_trait(k) isa Union{IsotropicInput, DotProductInput} ? device_kernel(k) : nothing
kref(s::CKernel) = Ref(s)
kref(s::CComposite) = Ref(s)

# ---- context: one per process = one device + its default stream ---------------------------------------------------------
const CTX = Ref{Ptr{Cvoid}}(C_NULL)
const DEVICE_ID = Ref{Cint}(0)           # set before the first call (e.g. from the MPI local rank): one process per GPU
function ctx()
    if CTX[] == C_NULL
        check(ccall((:covgram_ctx_create, libcovgram), Cint, (Ref{Ptr{Cvoid}}, Cint, Ptr{Cvoid}), CTX, DEVICE_ID[], C_NULL))
    end
    CTX[]
end

# ---- device-resident copy of a point set ---------------------------------------------------------------------------------
# Cached per (input object, element type) so Krylov solvers upload x once.  The library's contract for a handle is "unchanged
# while the handle lives" (include/covgram.h: covgram_points_create), whereas the reference's lazy Gramian follows in-place
# updates of x; the cache therefore keeps a fingerprint (length, dimension, a hash of ≤ 4096 strided scalars) and re-uploads
# when it changes; `CovGram.refresh!(x)` forces it after an update the sample might miss.  Keys are weak: the Points
# finalizer runs (and frees the HBM copy) once x itself is garbage.
mutable struct Points
    handle::Ptr{Cvoid}
    fingerprint::UInt
    function Points(x::AbstractVector, ::Type{T}) where {T}
        d = length(x[1]); n = length(x)
        X = Matrix{T}(undef, d, n)                      # d×n column-major == point-major, as gramian.jl:2,154-155
        for (j, xj) in enumerate(x); X[:, j] .= xj; end
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:covgram_points_create, libcovgram), Cint,
                    (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Int64, Int32, Int32, Int32), ctx(), h, X, n, d, dtype_code(T), HOST))
        p = new(h[], fingerprint(x))
        finalizer(q -> ccall((:covgram_points_destroy, libcovgram), Cint, (Ptr{Cvoid},), q.handle), p)
        p
    end
end
function fingerprint(x::AbstractVector)
    n = length(x); n == 0 && return UInt(0)
    d = length(x[1]); h = hash((n, d))
    for j in 1:max(1, n ÷ 1024):n
        xj = x[j]
        for c in 1:max(1, d ÷ 4):d; h = hash(xj[c], h); end
    end
    h
end
const POINTS = WeakKeyDict{Any, Dict{DataType, Points}}()
function points(x, ::Type{T}) where {T}
    per = get!(() -> Dict{DataType, Points}(), POINTS, x)
    p = get(per, T, nothing)
    if p === nothing || p.fingerprint != fingerprint(x)
        p = Points(x, T); per[T] = p                   # the old handle is freed by its finalizer
    end
    p
end
refresh!(x) = (delete!(POINTS, x); nothing)

const ENABLED = Ref(false)
function enable!()
    isfile(libcovgram) || error("$libcovgram not found: build it with `make -C covariancefunctions.jl_amd -j8`; there is no CPU fallback inside the library")
    ENABLED[] = true
end
disable!() = (ENABLED[] = false)

# --- src/gramian.jl:78-87 / 89-99 --------------------------------------------------------------------------------
function device_mul!(y::StridedVecOrMat{T}, G::Gramian, a::StridedVecOrMat{T}, α, β, spec) where {T <: DevFloat}
    n, m = size(G)
    size(a, 1) == m && size(y, 1) == n && size(y, 2) == size(a, 2) || throw(DimensionMismatch("mul!: size mismatch"))
    X = points(G.x, T); Y = G.x === G.y ? X : points(G.y, T)
    check(ccall((:covgram_mvm, libcovgram), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Float64, Float64, Int32),
                ctx(), kref(spec), X.handle, Y.handle, a, stride(a, 2) == 0 ? m : max(stride(a, 2), m), y, max(stride(y, 2), n),
                size(a, 2), Float64(α), Float64(β), HOST))
    return y
end

function LinearAlgebra.mul!(y::StridedVector{T}, G::Gramian{T}, a::StridedVector{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    spec = device_kernel_for(G.k)
    spec === nothing ? invoke(mul!, Tuple{AbstractVector, Gramian, AbstractVector, Real, Real}, y, G, a, α, β) :
                       device_mul!(y, G, a, α, β, spec)
end
function LinearAlgebra.mul!(Y::StridedMatrix{T}, G::Gramian{T}, A::StridedMatrix{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    spec = device_kernel_for(G.k)
    spec === nothing ? invoke(mul!, Tuple{AbstractMatrix, Gramian, AbstractMatrix, Real, Real}, Y, G, A, α, β) :
                       device_mul!(Y, G, A, α, β, spec)
end

# --- src/gramian.jl:102-114: Matrix(G) -> covgram_matrix (HBM-write-bound tile instantiation, copied back) ----------------
function Base.Matrix(G::Gramian{T}) where {T <: DevFloat}
    spec = device_kernel_for(G.k)
    spec === nothing && return invoke(Matrix, Tuple{Gramian}, G)
    n, m = size(G)
    M = Matrix{T}(undef, n, m)
    X = points(G.x, T); Y = G.x === G.y ? X : points(G.y, T)
    check(ccall((:covgram_matrix, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32),
                ctx(), kref(spec), X.handle, Y.handle, M, n, HOST))
    return M
end

# --- src/gramian.jl:241-257 with src/gradient.jl:86-115: flat point-major block vectors ---------------------------
function device_blockmul!(sym::Symbol, y::StridedVecOrMat{T}, G::Gramian, a::StridedVecOrMat{T}, α, β, spec) where {T}
    X = points(G.x, T); Y = G.x === G.y ? X : points(G.y, T)
    size(y, 2) == size(a, 2) || throw(DimensionMismatch("mul!: y has $(size(y, 2)) columns, a has $(size(a, 2))"))
    lda = max(stride(a, 2), size(a, 1)); ldy = max(stride(y, 2), size(y, 1)); nrhs = Int32(size(a, 2))
    if sym === :grad
        check(ccall((:covgram_grad_mvm, libcovgram), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Float64, Float64, Int32),
                    ctx(), kref(spec), X.handle, Y.handle, a, lda, y, ldy, nrhs, Float64(α), Float64(β), HOST))
    elseif sym === :hess   # src/hessian.jl:33-41, element mul! :125-190 / :227-275: blocks of d^2, entry a + b d (vec of a d x d matrix)
        check(ccall((:covgram_hess_mvm, libcovgram), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Float64, Float64, Int32),
                    ctx(), kref(spec), X.handle, Y.handle, a, lda, y, ldy, nrhs, Float64(α), Float64(β), HOST))
    elseif sym === :valgradhess   # src/hessian.jl:301-325: blocks of 1 + d + d^2: value, gradient, then entry a + b d of the Hessian
        check(ccall((:covgram_valgradhess_mvm, libcovgram), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Float64, Float64, Int32),
                    ctx(), kref(spec), X.handle, Y.handle, a, lda, y, ldy, nrhs, Float64(α), Float64(β), HOST))
    else   # src/gradient.jl:400-474 (ValueGradientKernel), block mul! :319-351: blocks of d+1, value component first
        check(ccall((:covgram_valgrad_mvm, libcovgram), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Float64, Float64, Int32),
                    ctx(), kref(spec), X.handle, Y.handle, a, lda, y, ldy, nrhs, Float64(α), Float64(β), HOST))
    end
    return y
end

# --- src/gradient_algebra.jl:6-89: GradientKernel / ValueGradientKernel of a Sum / Product whose factors do NOT share one trait
# (input_trait = GenericInput, e.g. MaternP(2) + Dot()^2 + NN()) -> covgram_grad_mvm_mixed, the entry that reads every factor's own
# trait.  Leaves: the profiles of `lower` that are smooth at zero distance, and NeuralNetwork(σ) as family 102 with σ in param.
# (covgram/kernels.py::mixed_gradient_spec is the executed version of this flattening, including Power over sums.)
const F_NEURALNETWORK = Int32(102)
lower_mixed_leaf(k) = (f = lower(k); (f === nothing || f.family in (F_EXP, F_GAMMAEXP) || (f.family == F_MATERNP && f.p == 0)) ? nothing : f)
lower_mixed_leaf(k::CovarianceFunctions.NeuralNetwork) = CKernel(F_NEURALNETWORK, Int32(0), Int32(0), Int32(1), Float64(k.σ), 1.0, 1.0)
lower_mixed_leaf(k::Constant) = CKernel(F_CONSTANT, Int32(0), Int32(0), Int32(1), 0.0, 1.0, Float64(k.c))
function lower_mixed(k)
    terms = k isa Sum ? collect(k.args) : [k]
    length(terms) ≤ COMPOSITE_MAX_TERMS || return nothing
    nfac = zeros(Int32, COMPOSITE_MAX_TERMS); facs = CKernel[]
    for (t, term) in enumerate(terms)
        for part in (term isa Product ? collect(term.args) : [term])
            f = lower_mixed_leaf(part)
            f === nothing && return nothing
            push!(facs, f); nfac[t] += 1
        end
    end
    length(facs) ≤ COMPOSITE_MAX_FACTORS || return nothing
    while length(facs) < COMPOSITE_MAX_FACTORS; push!(facs, NOKERNEL); end
    CComposite(CKernel(F_COMPOSITE, Int32(0), Int32(0), Int32(1), 0.0, 1.0, 1.0), Int32(length(terms)), Tuple(nfac), Tuple(facs))
end
# the hook of the block mul! methods below: the mixed composite where the kernel has one, else the reference's own blockmul!
function mixed_or(G::Gramian, value::Integer, y::StridedVecOrMat{T}, a::StridedVecOrMat{T}, α, β, fallback) where {T <: DevFloat}
    spec = ENABLED[] && input_trait(G.k.k) isa GenericInput ? lower_mixed(G.k.k) : nothing
    spec === nothing && return fallback()
    X = points(G.x, T); Y = G.x === G.y ? X : points(G.y, T)
    size(y, 2) == size(a, 2) || throw(DimensionMismatch("mul!: y has $(size(y, 2)) columns, a has $(size(a, 2))"))
    check(ccall((:covgram_grad_mvm_mixed, libcovgram), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Float64, Float64, Int32, Int32),
                ctx(), Ref(spec), X.handle, Y.handle, a, max(stride(a, 2), size(a, 1)), y, max(stride(y, 2), size(y, 1)), Int32(size(a, 2)),
                Float64(α), Float64(β), Int32(value), HOST))
    return y
end
# --- the SCALAR Gramian of such a composite (src/gramian.jl:78-87 on a GenericInput kernel): plain wrappers of covgram_mvm_mixed and
# covgram_matrix_mixed on a CComposite the caller has built (every factor with its own trait; no lowering on this side)
function mixed_mul!(y::StridedVecOrMat{T}, spec::CComposite, X::Points, Y::Points, a::StridedVecOrMat{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    size(y, 2) == size(a, 2) || throw(DimensionMismatch("mixed_mul!: y has $(size(y, 2)) columns, a has $(size(a, 2))"))
    check(ccall((:covgram_mvm_mixed, libcovgram), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Float64, Float64, Int32),
                ctx(), Ref(spec), X.handle, Y.handle, a, max(stride(a, 2), size(a, 1)), y, max(stride(y, 2), size(y, 1)), Int32(size(a, 2)),
                Float64(α), Float64(β), HOST))
    return y
end
# every hyper-parameter derivative of Σ_t U[:, t]' G A[:, t] of such a composite in one pass (covgram_bilinear_grad_mixed): the 24 Float64 of
# include/covgram.h — out[t] per term without its coefficient, out[8 + f] = Σ W c_t z ∂ψ_f/∂z Π ψ_g, out[16 + f] = Σ W c_t ∂ψ_f/∂θ_f Π ψ_g
const MIXED_GRAD_NOUT = 24           # COVGRAM_MIXED_GRAD_NOUT
function mixed_bilinear_grad(spec::CComposite, X::Points, Y::Points, U::StridedVecOrMat{T}, A::StridedVecOrMat{T}) where {T <: DevFloat}
    size(U, 2) == size(A, 2) || throw(DimensionMismatch("mixed_bilinear_grad: U is n × nvec, A is m × nvec"))
    out = zeros(Float64, MIXED_GRAD_NOUT)
    check(ccall((:covgram_bilinear_grad_mixed, libcovgram), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Int32),
                ctx(), Ref(spec), X.handle, Y.handle, U, max(stride(U, 2), size(U, 1)), A, max(stride(A, 2), size(A, 1)), Int32(size(U, 2)), out, HOST))
    return out
end
function mixed_matrix!(out::StridedMatrix{T}, spec::CComposite, X::Points, Y::Points) where {T <: DevFloat}
    check(ccall((:covgram_matrix_mixed, libcovgram), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32),
                ctx(), Ref(spec), X.handle, Y.handle, out, max(stride(out, 2), size(out, 1)), HOST))
    return out
end

function LinearAlgebra.mul!(y::StridedVector{T}, B::BlockFactorizations.BlockFactorization{T, <:Gramian{<:Any, <:GradientKernel}},
                            a::StridedVector{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    G = B.A
    spec = device_kernel_for(G.k.k)
    spec === nothing ? mixed_or(G, 0, y, a, α, β, () -> invoke(mul!, Tuple{AbstractVector, BlockFactorizations.BlockFactorization, AbstractVector, Real, Real}, y, B, a, α, β)) :
                       device_blockmul!(:grad, y, G, a, α, β, spec)
end
# matrix right-hand sides (src/gramian.jl:241-257: AbstractVecOfVecOrMat): one library call for all columns
function LinearAlgebra.mul!(Y::StridedMatrix{T}, B::BlockFactorizations.BlockFactorization{T, <:Gramian{<:Any, <:GradientKernel}},
                            A::StridedMatrix{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    G = B.A
    spec = device_kernel_for(G.k.k)
    spec === nothing ? mixed_or(G, 0, Y, A, α, β, () -> invoke(mul!, Tuple{AbstractMatrix, BlockFactorizations.BlockFactorization, AbstractMatrix, Real, Real}, Y, B, A, α, β)) :
                       device_blockmul!(:grad, Y, G, A, α, β, spec)
end
function LinearAlgebra.mul!(y::StridedVector{T}, B::BlockFactorizations.BlockFactorization{T, <:Gramian{<:Any, <:ValueGradientKernel}},
                            a::StridedVector{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    G = B.A
    spec = device_kernel_for(G.k.k)
    spec === nothing ? mixed_or(G, 1, y, a, α, β, () -> invoke(mul!, Tuple{AbstractVector, BlockFactorizations.BlockFactorization, AbstractVector, Real, Real}, y, B, a, α, β)) :
                       device_blockmul!(:valgrad, y, G, a, α, β, spec)
end
function LinearAlgebra.mul!(Y::StridedMatrix{T}, B::BlockFactorizations.BlockFactorization{T, <:Gramian{<:Any, <:ValueGradientKernel}},
                            A::StridedMatrix{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    G = B.A
    spec = device_kernel_for(G.k.k)
    spec === nothing ? mixed_or(G, 1, Y, A, α, β, () -> invoke(mul!, Tuple{AbstractMatrix, BlockFactorizations.BlockFactorization, AbstractMatrix, Real, Real}, Y, B, A, α, β)) :
                       device_blockmul!(:valgrad, Y, G, A, α, β, spec)
end

# --- src/hessian.jl: HessianKernel Gramians -> covgram_hess_mvm.  Device path: ONE profile of EQ / RQ / Cauchy / IMQ / Dot / ExponentialDot
# without a Power wrapper and d <= 32 (include/covgram.h); everything else keeps the reference's own blockmul!
hessian_spec(k, d::Integer) = begin
    spec = device_kernel_for(k)
    (spec isa CKernel && spec.family in (Int32(0), Int32(2), Int32(4), Int32(5), Int32(7), Int32(8)) && spec.power == 1 && d <= 32) ? spec : nothing
end
function LinearAlgebra.mul!(y::StridedVector{T}, B::BlockFactorizations.BlockFactorization{T, <:Gramian{<:Any, <:HessianKernel}},
                            a::StridedVector{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    G = B.A
    spec = hessian_spec(G.k.k, length(first(G.x)))
    spec === nothing ? invoke(mul!, Tuple{AbstractVector, BlockFactorizations.BlockFactorization, AbstractVector, Real, Real}, y, B, a, α, β) :
                       device_blockmul!(:hess, y, G, a, α, β, spec)
end
function LinearAlgebra.mul!(Y::StridedMatrix{T}, B::BlockFactorizations.BlockFactorization{T, <:Gramian{<:Any, <:HessianKernel}},
                            A::StridedMatrix{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    G = B.A
    spec = hessian_spec(G.k.k, length(first(G.x)))
    spec === nothing ? invoke(mul!, Tuple{AbstractMatrix, BlockFactorizations.BlockFactorization, AbstractMatrix, Real, Real}, Y, B, A, α, β) :
                       device_blockmul!(:hess, Y, G, A, α, β, spec)
end

# --- src/hessian.jl:279-479: ValueGradientHessianKernel Gramians -> covgram_valgradhess_mvm; the kernels and the bound on d of hessian_spec
function LinearAlgebra.mul!(y::StridedVector{T}, B::BlockFactorizations.BlockFactorization{T, <:Gramian{<:Any, <:ValueGradientHessianKernel}},
                            a::StridedVector{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    G = B.A
    spec = hessian_spec(G.k.k, length(first(G.x)))
    spec === nothing ? invoke(mul!, Tuple{AbstractVector, BlockFactorizations.BlockFactorization, AbstractVector, Real, Real}, y, B, a, α, β) :
                       device_blockmul!(:valgradhess, y, G, a, α, β, spec)
end
function LinearAlgebra.mul!(Y::StridedMatrix{T}, B::BlockFactorizations.BlockFactorization{T, <:Gramian{<:Any, <:ValueGradientHessianKernel}},
                            A::StridedMatrix{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    G = B.A
    spec = hessian_spec(G.k.k, length(first(G.x)))
    spec === nothing ? invoke(mul!, Tuple{AbstractMatrix, BlockFactorizations.BlockFactorization, AbstractMatrix, Real, Real}, Y, B, A, α, β) :
                       device_blockmul!(:valgradhess, Y, G, A, α, β, spec)
end

# --- src/gramian.jl:125-130, 192-199: Matrix of the four block Gramians -> covgram_block_matrix (one store-bound pass; the jet of a pair
# evaluated once for its whole block).  Blocks are point-major with the ordering of the block mul!s above.
const BLOCK_GRADIENT, BLOCK_VALUE_GRADIENT, BLOCK_HESSIAN, BLOCK_VALUE_GRADIENT_HESSIAN = Int32(0), Int32(1), Int32(2), Int32(3)
function device_blockmatrix(kind::Int32, G::Gramian, ::Type{T}, bd::Integer, spec) where {T}
    X = points(G.x, T); Y = G.x === G.y ? X : points(G.y, T)
    n, m = size(G)
    M = Matrix{T}(undef, n * bd, m * bd)
    check(ccall((:covgram_block_matrix, libcovgram), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32),
                ctx(), kind, kref(spec), X.handle, Y.handle, M, Int64(n * bd), HOST))
    return M
end
function Base.Matrix(B::BlockFactorizations.BlockFactorization{T, <:Gramian{<:Any, <:GradientKernel}}) where {T <: DevFloat}
    G = B.A; spec = device_kernel_for(G.k.k); d = length(first(G.x))
    (spec === nothing || d > 64) ? invoke(Matrix, Tuple{BlockFactorizations.BlockFactorization}, B) : device_blockmatrix(BLOCK_GRADIENT, G, T, d, spec)
end
function Base.Matrix(B::BlockFactorizations.BlockFactorization{T, <:Gramian{<:Any, <:ValueGradientKernel}}) where {T <: DevFloat}
    G = B.A; spec = device_kernel_for(G.k.k); d = length(first(G.x))
    (spec === nothing || d > 64) ? invoke(Matrix, Tuple{BlockFactorizations.BlockFactorization}, B) : device_blockmatrix(BLOCK_VALUE_GRADIENT, G, T, d + 1, spec)
end
function Base.Matrix(B::BlockFactorizations.BlockFactorization{T, <:Gramian{<:Any, <:HessianKernel}}) where {T <: DevFloat}
    G = B.A; d = length(first(G.x)); spec = hessian_spec(G.k.k, d)
    spec === nothing ? invoke(Matrix, Tuple{BlockFactorizations.BlockFactorization}, B) : device_blockmatrix(BLOCK_HESSIAN, G, T, d * d, spec)
end
function Base.Matrix(B::BlockFactorizations.BlockFactorization{T, <:Gramian{<:Any, <:ValueGradientHessianKernel}}) where {T <: DevFloat}
    G = B.A; d = length(first(G.x)); spec = hessian_spec(G.k.k, d)
    spec === nothing ? invoke(Matrix, Tuple{BlockFactorizations.BlockFactorization}, B) :
                       device_blockmatrix(BLOCK_VALUE_GRADIENT_HESSIAN, G, T, 1 + d + d * d, spec)
end

# --- src/separable.jl:38-42: mul!(y, G::Gramian{<:AbstractMatrix, <:SeparableKernel}, x) on vectors of vectors -----------------
# The reference multiplies by kronecker(G) = gramian(k.k, x, y) ⊗ k.B (:33-35): block i of the result is B Σ_j k(x_i, y_j) a_j.  With
# the blocks of `a` as the ROWS of an m × q matrix that is (G_scalar A) Bᵀ: ONE covgram_mvm with q right-hand sides (every entry of
# the scalar Gramian evaluated once, O(n) memory — the Kronecker factor is never densified) and an n × q by q × p host product.
function LinearAlgebra.mul!(y::AbstractVector{<:AbstractVector{T}}, G::Gramian{<:AbstractMatrix, <:SeparableKernel},
                            a::AbstractVector{<:AbstractVector{T}}) where {T <: DevFloat}
    spec = device_kernel_for(G.k.k)
    spec === nothing && return invoke(mul!, Tuple{CovarianceFunctions.AbstractVecOfVec, Gramian{<:AbstractMatrix, <:SeparableKernel}, CovarianceFunctions.AbstractVecOfVec}, y, G, a)
    n, m = length(G.x), length(G.y); Bm = G.k.B; p, q = size(Bm)
    (length(a) == m && length(y) == n) || throw(DimensionMismatch("mul!: $(length(y)) / $(length(a)) blocks for a $n × $m block Gramian"))
    A = Matrix{T}(undef, m, q)
    for j in 1:m
        length(a[j]) == q || throw(DimensionMismatch("mul!: block $j of a has length $(length(a[j])) ≠ $q"))
        A[j, :] .= a[j]
    end
    GA = Matrix{T}(undef, n, q)
    device_mul!(GA, Gramian(G.k.k, G.x, G.y), A, 1, 0, spec)
    for i in 1:n
        mul!(y[i], Bm, view(GA, i, :))
    end
    return y
end

# --- multi-GPU symmetric form (one Julia process per GPU, e.g. under MPI.jl; x and a replicated) -----------------------
# rank r of `world` evaluates its cyclic share of the upper triangle of gramian(k, x) — 256-row panels on the symmetric matrix-core
# kernels (Float32), 64-row / 64 R-row blocks on the direct-difference symmetric kernels (Float64, and Float32 where the matrix cores
# do not apply) — and returns the partial product of those entries and their mirror images in `part` (device memory); an all-reduce
# (sum) of `part` over the ranks is G * a.  `covgram_mvm_sym_supported` tells whether a symmetric kernel serves (k, x) at this world
# size — it depends on k, x and world only, so all ranks take the same branch; otherwise shard rows and all-gather (covgram_mvm on
# X[lo:hi] × X).  The element type is the Gramian's own (src/gramian.jl:27-33).
function sym_partial!(part::Ptr{Cvoid}, G::Gramian{T}, a::Ptr{Cvoid}, rank::Integer, world::Integer) where {T <: DevFloat}
    spec = device_kernel(G.k); spec === nothing && return false
    X = points(G.x, T)
    ok = Ref{Int32}(0)
    check(ccall((:covgram_mvm_sym_supported, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{Int32}),
                ctx(), kref(spec), X.handle, Int32(world), ok))
    ok[] == 1 || return false
    check(ccall((:covgram_mvm_sym_partial, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32),
                ctx(), kref(spec), X.handle, a, part, Int32(rank), Int32(world)))
    return true
end

# --- the collective behind the ABI (include/covgram.h, "the collective behind the ABI"): mul! on a Gramian sharded over the GPUs of a node ------
# One Julia process per GPU.  `comm_unique_id()` on rank 0, its 128 bytes broadcast by whatever the job already has (MPI.bcast!, a shared
# file), then `comm_create!(id, rank, world)` on every rank: the library owns the RCCL communicator from there on, and
#     mul!(y, ShardedGramian(G), a, α, β)
# is the reference's mul!(y, G, a, α, β) (src/gramian.jl:78-87) with its `@threads for i in 1:n` spread over the ranks: each evaluates its
# rows (or, for gramian(k, x), its cyclic panels of the upper triangle) and ONE all-gather (all-reduce) on the library's stream completes y
# on every rank.  x, a and y are device pointers here (replicated data stays resident between Krylov iterations).
const COMM_ID_BYTES = 128
function comm_unique_id()
    id = zeros(UInt8, COMM_ID_BYTES)
    check(ccall((:covgram_comm_unique_id, libcovgram), Cint, (Ptr{Cvoid}, Int64), id, Int64(COMM_ID_BYTES)))
    return id
end
comm_create!(id::Vector{UInt8}, rank::Integer, world::Integer) =
    check(ccall((:covgram_comm_create, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32), ctx(), id, Int32(rank), Int32(world)))
comm_destroy!() = check(ccall((:covgram_comm_destroy, libcovgram), Cint, (Ptr{Cvoid},), ctx()))
function comm_info()
    r = Ref{Int32}(0); w = Ref{Int32}(0)
    check(ccall((:covgram_comm_info, libcovgram), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}), ctx(), r, w))
    return Int(r[]), Int(w[])
end
all_gather!(recv::Ptr{Cvoid}, send::Ptr{Cvoid}, count::Integer, ::Type{T}) where {T <: DevFloat} =
    check(ccall((:covgram_comm_all_gather, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32), ctx(), send, recv, Int64(count), dtype_code(T)))
all_reduce_sum!(buf::Ptr{Cvoid}, count::Integer, ::Type{T}) where {T <: DevFloat} =
    check(ccall((:covgram_comm_all_reduce_sum, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32), ctx(), buf, Int64(count), dtype_code(T)))

struct ShardedGramian{T, GT <: Gramian{T}} <: AbstractMatrix{T}
    G::GT
end
Base.size(S::ShardedGramian) = size(S.G)
# y, a: device pointers to n resp. m replicated scalars of the Gramian's element type
function LinearAlgebra.mul!(y::Ptr{Cvoid}, S::ShardedGramian{T}, a::Ptr{Cvoid}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    G = S.G
    spec = device_kernel(G.k); spec === nothing && error("ShardedGramian: the kernel has no device path (GenericInput)")
    X = points(G.x, T)
    if G.x === G.y                                          # gramian(k, x): the symmetric form where a symmetric kernel serves it
        rc = ccall((:covgram_mvm_sym_allreduce, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64),
                   ctx(), kref(spec), X.handle, a, y, Float64(α), Float64(β))
        rc == 0 && return y
        rc == -2 || check(rc)                               # COVGRAM_EUNSUPPORTED: row shards below
    end
    Y = G.x === G.y ? X : points(G.y, T)
    check(ccall((:covgram_mvm_sharded, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64),
                ctx(), kref(spec), X.handle, Y.handle, a, y, Float64(α), Float64(β)))
    return y
end

# --- Toeplitz (src/gramian.jl:167-189): the handle caches the plans and the spectrum of the circulant embedding ----------
mutable struct DeviceToeplitz{T} <: AbstractMatrix{T}
    handle::Ptr{Cvoid}
    n::Int
    m::Int
    vc::Vector{T}
    vr::Union{Nothing, Vector{T}}
    circulant::Bool
end
function DeviceToeplitz(vc::Vector{T}, vr::Union{Nothing, Vector{T}} = nothing; circulant = false) where {T <: DevFloat}
    h = Ref{Ptr{Cvoid}}(C_NULL); n = length(vc); m = vr === nothing ? n : length(vr)
    check(ccall((:covgram_toeplitz_create, libcovgram), Cint,
                (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int32, Int32, Int32),
                ctx(), h, vc, vr === nothing ? C_NULL : vr, n, m, dtype_code(T), HOST, circulant ? 1 : 0))
    t = DeviceToeplitz{T}(h[], n, m, vc, vr, circulant)
    finalizer(q -> ccall((:covgram_toeplitz_destroy, libcovgram), Cint, (Ptr{Cvoid},), q.handle), t); t
end
function LinearAlgebra.mul!(y::StridedVector{T}, A::DeviceToeplitz{T}, a::StridedVector{T}, α::Real = 1, β::Real = 0) where {T}
    check(ccall((:covgram_toeplitz_mvm, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Int32),
                A.handle, a, y, Float64(α), Float64(β), HOST)); y
end
Base.size(A::DeviceToeplitz) = (A.n, A.m)
function Base.getindex(A::DeviceToeplitz, i::Integer, j::Integer)   # T[i,j] = vc[i-j+1] (i ≥ j), vr[j-i+1] (i < j)
    A.circulant && return A.vc[mod(i - j, A.n) + 1]
    i ≥ j ? A.vc[i - j + 1] : (A.vr === nothing ? A.vc[j - i + 1] : A.vr[j - i + 1])
end
LinearAlgebra.issymmetric(A::DeviceToeplitz) = A.vr === nothing && !A.circulant

# gramian(k, x::StepRangeLen, y::StepRangeLen, trait): same three cases as src/gramian.jl:172-183; floating-point ranges only
# (more specific than the reference's method, which stays the fallback)
function gramian(k, x::StepRangeLen{T}, y::StepRangeLen{T}, t::Union{IsotropicInput, StationaryInput}) where {T <: DevFloat}
    ENABLED[] || return invoke(gramian, Tuple{Any, StepRangeLen, StepRangeLen, Union{IsotropicInput, StationaryInput}}, k, x, y, t)
    if x === y
        DeviceToeplitz(T.(k.(x[1], x)))                                   # SymmetricToeplitz(k1), src/gramian.jl:174-175
    elseif x.step == y.step
        DeviceToeplitz(T.(k.(x, y[1])), T.(k.(x[1], y)))                  # Toeplitz(k1, k2), :177-179
    else
        Gramian(k, x, y)                                                  # :181
    end
end
# periodic boundary conditions: Circulant(k1), src/gramian.jl:186-189
function gramian(k::CovarianceFunctions.StationaryKernel, x::StepRangeLen{T}, p::CovarianceFunctions.PeriodicInput) where {T <: DevFloat}
    ENABLED[] || return invoke(gramian, Tuple{CovarianceFunctions.StationaryKernel, StepRangeLen, CovarianceFunctions.PeriodicInput}, k, x, p)
    DeviceToeplitz(T.(k.(x[1], x)); circulant = true)
end

# --- direct Toeplitz solvers (src/toeplitz.jl:12-111): the O(n²) chains on one workgroup of the device --------------------
# unit-diagonal forms, as the reference's vector methods; `levinson(T, b)` / `trench(T)` normalise by T.vc[1] (the reference's
# `r_0 == 1` test is inverted, src/toeplitz.jl:40-42,103-105; done right here)
function device_durbin(r::Vector{T}) where {T <: DevFloat}
    y = similar(r)
    check(ccall((:covgram_toeplitz_durbin, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int32, Int32),
                ctx(), r, length(r), y, dtype_code(T), HOST)); y
end
function device_levinson(r::Vector{T}, b::Vector{T}) where {T <: DevFloat}
    length(b) == length(r) + 1 || throw(DimensionMismatch("length(b) = $(length(b)) ≠ $(length(r) + 1) = length(r) + 1"))
    x = similar(b)
    check(ccall((:covgram_toeplitz_levinson, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int32, Int32),
                ctx(), r, b, length(b), x, dtype_code(T), HOST)); x
end
function device_trench(r::Vector{T}) where {T <: DevFloat}
    n = length(r) + 1; B = Matrix{T}(undef, n, n)
    check(ccall((:covgram_toeplitz_trench, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Int32),
                ctx(), r, n, B, n, dtype_code(T), HOST)); Symmetric(B)
end
device_levinson(A::DeviceToeplitz{T}, b::Vector{T}) where {T} = device_levinson(A.vc[2:end] ./ A.vc[1], b) ./ A.vc[1]
device_trench(A::DeviceToeplitz) = Symmetric(parent(device_trench(A.vc[2:end] ./ A.vc[1])) ./ A.vc[1])
# `\`: the reference's `\` on a SymmetricToeplitz is a DIRECT solve, and so is this one wherever the library serves it: Levinson is ONE
# launch of n - 1 dependent O(n) steps on one workgroup (n <= 16384: state in registers and LDS, 28 ms at n = 16384 fp64; above that the
# vectors live in global memory, ~8 us a step), up to COVGRAM_TOEPLITZ_DIRECT_MAX_N = 65536.  Beyond it the library returns
# COVGRAM_EUNSUPPORTED and the solve is conjugate gradients over the FFT MVM (`mul!` above: covgram_toeplitz_mvm; the reference's own
# solver for lazy operators, src/gramian.jl:229-238) with an explicit tolerance, and it ERRORS when CG did not converge — noise-free
# Gramians are ill-conditioned, and IterativeSolvers.cg returns its last iterate silently (ADVICE r3).
const TOEPLITZ_DIRECT_MAX_N = 65536          # COVGRAM_TOEPLITZ_DIRECT_MAX_N
function LinearAlgebra.:\(A::DeviceToeplitz{T}, b::Vector{T}) where {T}
    issymmetric(A) || error("only symmetric Toeplitz solves are served")
    length(b) <= TOEPLITZ_DIRECT_MAX_N && return device_levinson(A, b)
    x, hist = CovarianceFunctions.IterativeSolvers.cg(A, b; reltol = eps(T)^(2 / 3), maxiter = 4 * ceil(Int, sqrt(length(b))) + 200, log = true)
    hist.isconverged || error("Toeplitz solve of order $(length(b)): CG over the FFT MVM did not converge in $(hist.iters) iterations " *
                              "(relative tolerance $(eps(T)^(2 / 3))); add a noise term or use a preconditioned solver")
    x
end

# --- Kronecker (src/algebra.jl:91-95, src/separable.jl:33-42): dense factors, mode products on the matrix cores (csrc/kron.hip) --
struct DeviceKronecker{T} <: AbstractMatrix{T}
    factors::Vector{Matrix{T}}          # F_1 ⊗ F_2 ⊗ … ⊗ F_q in the reference's order (kronecker(G_1, …, G_q))
end
Base.size(K::DeviceKronecker) = (prod(size(F, 1) for F in K.factors), prod(size(F, 2) for F in K.factors))
function Base.getindex(K::DeviceKronecker, i::Integer, j::Integer)
    v = one(eltype(K)); i -= 1; j -= 1
    for F in reverse(K.factors)                                           # the LAST factor's index varies fastest
        r, c = size(F); v *= F[i % r + 1, j % c + 1]; i ÷= r; j ÷= c
    end
    v
end
function LinearAlgebra.mul!(y::StridedVecOrMat{T}, K::DeviceKronecker{T}, a::StridedVecOrMat{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    q = length(K.factors)
    n, m = size(K)
    size(a, 1) == m && size(y, 1) == n && size(y, 2) == size(a, 2) || throw(DimensionMismatch("mul!: size mismatch"))
    ptrs = Ptr{Cvoid}[pointer(F) for F in K.factors]
    rows = Int64[size(F, 1) for F in K.factors]; cols = Int64[size(F, 2) for F in K.factors]
    GC.@preserve K check(ccall((:covgram_kron_mvm, libcovgram), Cint,
        (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int32, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Float64, Float64, Int32),
        ctx(), ptrs, rows, cols, rows, Int32(q), dtype_code(T), a, max(stride(a, 2), m), y, max(stride(y, 2), n), Int32(size(a, 2)),
        Float64(α), Float64(β), HOST))
    y
end
function gramian(k::SeparableProduct, X::LazyGrid{T}, Y::LazyGrid{T}) where {T <: DevFloat}
    ENABLED[] || return invoke(gramian, Tuple{SeparableProduct, LazyGrid, LazyGrid}, k, X, Y)
    length(X.args) == length(Y.args) || throw(DimensionMismatch("length(X.args) = $(length(X.args)) ≠ $(length(Y.args)) = length(Y.args)"))
    length(k.args) == length(X.args) || throw(DimensionMismatch("SeparableProduct needs d = $(length(X.args)) kernels but has r = $(length(k.args))"))
    DeviceKronecker{T}([Matrix{T}(Matrix(gramian(ki, xi, yi))) for (ki, xi, yi) in zip(k.args, X.args, Y.args)])
end

# --- low rank (src/mercer.jl:53-70, src/lazy_linear_algebra.jl:78-85): U (V' a), vector or matrix right-hand sides -------
struct DeviceLowRank{T} <: AbstractMatrix{T}
    U::Matrix{T}
    V::Matrix{T}
end
Base.size(L::DeviceLowRank) = (size(L.U, 1), size(L.V, 1))
Base.getindex(L::DeviceLowRank, i::Integer, j::Integer) = dot(view(L.U, i, :), view(L.V, j, :))
function LinearAlgebra.mul!(y::StridedVecOrMat{T}, L::DeviceLowRank{T}, a::StridedVecOrMat{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    n, m = size(L); r = size(L.U, 2)
    size(a, 1) == m && size(y, 1) == n && size(y, 2) == size(a, 2) || throw(DimensionMismatch("mul!: size mismatch"))
    check(ccall((:covgram_lowrank_mvm, libcovgram), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int64, Int64, Int64, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Float64, Float64, Int32),
                ctx(), L.U, n, L.V, m, n, m, r, dtype_code(T), a, max(stride(a, 2), m), y, max(stride(y, 2), n), Int32(size(a, 2)),
                Float64(α), Float64(β), HOST))
    y
end
function gramian(k::FiniteBasis{T}, x::AbstractVector, y::AbstractVector) where {T <: DevFloat}
    r = length(k.basis)
    (ENABLED[] && length(x) > r && length(y) > r) || return invoke(gramian, Tuple{FiniteBasis, AbstractVector, AbstractVector}, k, x, y)
    U = CovarianceFunctions.basis(k, x)
    V = x === y ? U : CovarianceFunctions.basis(k, y)
    DeviceLowRank{T}(U, V)
end

# --- src/gramian.jl:191 ("a special cholesky implementation to avoid instantiating G in the low rank case") -> covgram_pivoted_cholesky ----
# The diagonally pivoted Cholesky factor of gramian(k, x) for one isotropic profile, on the device: one launch per pivot, nothing
# synchronises with the host.  L (n × max_rank, column-major, leading dimension ldl), piv (max_rank Int32), dres (n entries of T) and
# rank (one Int32) are DEVICE pointers; the caller reads `rank` when it needs it.  Returns false when the kernel has no device factorisation.
const PIVCHOL_MAX_RANK = 1024                # COVGRAM_PIVCHOL_MAX_RANK
function pivoted_cholesky!(L::Ptr{Cvoid}, ldl::Integer, piv::Ptr{Cvoid}, dres::Ptr{Cvoid}, rank::Ptr{Cvoid}, G::Gramian{T}, max_rank::Integer;
                           tol::Real = 0.0) where {T <: DevFloat}
    spec = device_kernel(G.k); (spec === nothing || !(spec isa CKernel) || spec.trait != ISO) && return false
    G.x === G.y || throw(ArgumentError("pivoted_cholesky!: a symmetric Gramian gramian(k, x) is expected"))
    X = points(G.x, T)
    check(ccall((:covgram_pivoted_cholesky, libcovgram), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                ctx(), kref(spec), X.handle, Int32(max_rank), Float64(tol), L, Int64(ldl), piv, dres, rank))
    return true
end

# --- src/sparse.jl:5-38: sparse(G, δ) -> covgram_sparse_*(count / scan / fill on the device instead of the ball-tree range search) ------
# decay_radius as the LIBRARY defines it (include/covgram.h): l r0(δ / |c|) — src/sparse.jl:38 divides by l and drops δ, and ignores
# Constant factors; both are put right there.
function device_decay_radius(spec, δ::Real)
    r = Ref{Float64}(0.0)
    check(ccall((:covgram_decay_radius, libcovgram), Cint, (Ptr{Cvoid}, Float64, Ref{Float64}), kref(spec), Float64(δ), r))
    r[]
end
# the device-resident CSR matrix itself, for callers that keep multiplying on the GPU (host vectors are staged per call)
mutable struct DeviceSparse{T} <: AbstractMatrix{T}
    handle::Ptr{Cvoid}
    n::Int; m::Int; nnz::Int; radius::Float64
    function DeviceSparse(k, x, y, ::Type{T}, δ::Real, spec) where {T <: DevFloat}
        X = points(x, T); Y = x === y ? X : points(y, T)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:covgram_sparse_create, libcovgram), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64),
                    ctx(), h, kref(spec), X.handle, Y.handle, Float64(δ)))
        n = Ref{Int64}(0); m = Ref{Int64}(0); nnz = Ref{Int64}(0); dt = Ref{Int32}(0); r = Ref{Float64}(0.0)
        check(ccall((:covgram_sparse_info, libcovgram), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int32}, Ref{Float64}),
                    h[], n, m, nnz, dt, r))
        S = new{T}(h[], n[], m[], nnz[], r[])
        finalizer(q -> ccall((:covgram_sparse_destroy, libcovgram), Cint, (Ptr{Cvoid},), q.handle), S)
        S
    end
end
Base.size(S::DeviceSparse) = (S.n, S.m)
# (rowptr, colind, vals) of the CSR arrays, 0-based as the library stores them
function csr(S::DeviceSparse{T}) where {T}
    rowptr = Vector{Int64}(undef, S.n + 1); colind = Vector{Int32}(undef, S.nnz); vals = Vector{T}(undef, S.nnz)
    check(ccall((:covgram_sparse_export, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Cvoid}, Int32),
                S.handle, rowptr, colind, vals, HOST))
    rowptr, colind, vals
end
function LinearAlgebra.mul!(y::StridedVecOrMat{T}, S::DeviceSparse{T}, a::StridedVecOrMat{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    size(a, 1) == S.m && size(y, 1) == S.n && size(y, 2) == size(a, 2) || throw(DimensionMismatch("mul!: size mismatch"))
    size(a, 2) == 0 && return y                        # no columns: nothing to do (the ABI requires nrhs >= 1)
    check(ccall((:covgram_sparse_mvm, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Float64, Float64, Int32),
                S.handle, a, max(stride(a, 2), S.m), y, max(stride(y, 2), S.n), size(a, 2), Float64(α), Float64(β), HOST))
    return y
end
function Base.getindex(S::DeviceSparse{T}, i::Integer, j::Integer) where {T}   # (for show and tests; not a hot path)
    rowptr, colind, vals = csr(S)
    for p in rowptr[i] + 1:rowptr[i + 1]
        colind[p] == j - 1 && return vals[p]
    end
    zero(T)
end
# sparse(G, δ): the reference's SparseMatrixCSC.  An isotropic kernel is symmetric in its arguments, so the handle is built with X and Y
# EXCHANGED: the CSR arrays of the m × n matrix sparse(gramian(k, y, x)) are, plus 1, the colptr / rowval / nzval of the n × m CSC matrix.
# Only a kernel without a device spec goes to the reference's method (its signature as of src/sparse.jl:5); a kernel that has a spec but
# no decay radius (RQ, a Sum, a Power, ...) is refused by the library, by name, through check(...): INTEGRATION.md.
function SparseArrays.sparse(G::Gramian{T}, δ::Real = 1e-6; leafsize::Int = 16) where {T <: DevFloat}
    spec = device_kernel_for(G.k)
    spec === nothing && return invoke(SparseArrays.sparse, Tuple{Gramian, Real}, G, δ; leafsize = leafsize)
    n, m = size(G)
    St = DeviceSparse(G.k, G.y, G.x, T, δ, spec)
    rowptr, colind, vals = csr(St)
    SparseArrays.SparseMatrixCSC{T, Int64}(n, m, rowptr .+ 1, Int64.(colind) .+ 1, vals)
end

# --- src/barneshut.jl:8-143: BarnesHutFactorization -> covgram_bh_* (ball tree over y built on the device, tree-based approximate product) ---
# Deviation from the reference (DESIGN.md, "Barnes-Hut"): its mul! sends signed weights to taylor!; here mul! and * stay the SPLIT Barnes-Hut
# product BH(w+) - BH(w-), the default of the reference's own barneshut!, and taylor!(b, F, w, alpha, beta, theta; use_com) is a method of its
# own (src/taylor.jl:7-57 -> covgram_bh_taylor_mvm).  ldiv! / `\` run IterativeSolvers.minres! on the Taylor product (src/barneshut.jl:64-72).
mutable struct DeviceBarnesHut{T} <: AbstractMatrix{T}
    handle::Ptr{Cvoid}
    k::Any; x::Any; y::Any
    D::Union{Nothing, Vector{T}}
    n::Int; m::Int; d::Int; nnodes::Int; leafsize::Int; θ::Float64
    function DeviceBarnesHut(k, x, y, D, ::Type{T}, θ::Real, leafsize::Integer, spec) where {T <: DevFloat}
        X = points(x, T); Y = x === y ? X : points(y, T)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:covgram_bh_create, libcovgram), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Int32),
                    ctx(), h, kref(spec), X.handle, Y.handle, Float64(θ), Int32(leafsize)))
        n = Ref{Int64}(0); m = Ref{Int64}(0); d = Ref{Int32}(0); dt = Ref{Int32}(0); nn = Ref{Int64}(0); ls = Ref{Int32}(0); th = Ref{Float64}(0.0)
        check(ccall((:covgram_bh_info, libcovgram), Cint,
                    (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int32}, Ref{Int32}, Ref{Int64}, Ref{Int32}, Ref{Float64}), h[], n, m, d, dt, nn, ls, th))
        Dv = D === nothing ? nothing : (D isa Number ? T[D] : Vector{T}(diag(D)))
        F = new{T}(h[], k, x, y, Dv, n[], m[], d[], nn[], ls[], th[])
        finalizer(q -> ccall((:covgram_bh_destroy, libcovgram), Cint, (Ptr{Cvoid},), q.handle), F)
        F
    end
end
Base.size(F::DeviceBarnesHut) = (F.n, F.m)
Base.getindex(F::DeviceBarnesHut, i::Integer, j::Integer) = F.k(F.x[i], F.y[j])                 # src/barneshut.jl:42
# the export: indices (0-based permutation of the columns), per node lo, hi, left, right (-1 at a leaf, root = node 0), centres d × nnodes, radii
function tree(F::DeviceBarnesHut{T}) where {T}
    indices = Vector{Int32}(undef, F.nnodes > 0 ? F.m : 0)
    lo = Vector{Int32}(undef, F.nnodes); hi = similar(lo); left = similar(lo); right = similar(lo)
    centers = Matrix{T}(undef, F.d, F.nnodes); radii = Vector{T}(undef, F.nnodes)
    check(ccall((:covgram_bh_export, libcovgram), Cint,
                (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Cvoid}, Ptr{Cvoid}, Int32),
                F.handle, indices, lo, hi, left, right, centers, radii, HOST))
    (; indices, lo, hi, left, right, centers, radii)
end
# node_sums / compute_centers_of_mass of src/barneshut.jl:145-190 in one call: (sums, centers_of_mass d × nnodes)
function moments(F::DeviceBarnesHut{T}, w::StridedVector{T}) where {T}
    length(w) == F.m || throw(DimensionMismatch("length of w does not match second dimension of F: $(length(w)) ≠ $(F.m)"))
    sums = Vector{T}(undef, F.nnodes); com = Matrix{T}(undef, F.d, F.nnodes)
    check(ccall((:covgram_bh_moments, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32), F.handle, w, sums, com, HOST))
    sums, com
end
function barneshut!(b::StridedVector{T}, F::DeviceBarnesHut{T}, w::StridedVector{T}, α::Real = 1, β::Real = 0, θ::Real = F.θ;
                    split::Bool = true) where {T <: DevFloat}
    length(w) == F.m || throw(DimensionMismatch("length of w does not match second dimension of F: $(length(w)) ≠ $(F.m)"))
    length(b) == F.n || throw(DimensionMismatch("length of b does not match first dimension of F: $(length(b)) ≠ $(F.n)"))
    stride(b, 1) == 1 && stride(w, 1) == 1 || throw(ArgumentError("barneshut!: contiguous vectors expected"))
    Dp = F.D === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(pointer(F.D))
    GC.@preserve F check(ccall((:covgram_bh_mvm, libcovgram), Cint,
                               (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Int32, Ptr{Cvoid}, Int64, Int32),
                               F.handle, w, b, Float64(α), Float64(β), Float64(θ), Int32(split), Dp, Int64(F.D === nothing ? 0 : length(F.D)), HOST))
    b
end
# node_sums, the expansion centres and the centred first moments of src/taylor.jl:14-18 in one call: (sums, centers d × nnodes, m1 d × nnodes)
function taylor_moments(F::DeviceBarnesHut{T}, w::StridedVector{T}; use_com::Bool = true) where {T}
    length(w) == F.m || throw(DimensionMismatch("length of w does not match second dimension of F: $(length(w)) ≠ $(F.m)"))
    sums = Vector{T}(undef, F.nnodes); centers = Matrix{T}(undef, F.d, F.nnodes); m1 = Matrix{T}(undef, F.d, F.nnodes)
    check(ccall((:covgram_bh_taylor_moments, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32),
                F.handle, w, Int32(use_com), sums, centers, m1, HOST))
    sums, centers, m1
end
function taylor!(b::StridedVector{T}, F::DeviceBarnesHut{T}, w::StridedVector{T}, α::Real = 1, β::Real = 0, θ::Real = F.θ;
                 use_com::Bool = true) where {T <: DevFloat}
    length(w) == F.m || throw(DimensionMismatch("length of w does not match second dimension of F: $(length(w)) ≠ $(F.m)"))
    length(b) == F.n || throw(DimensionMismatch("length of b does not match first dimension of F: $(length(b)) ≠ $(F.n)"))
    stride(b, 1) == 1 && stride(w, 1) == 1 || throw(ArgumentError("taylor!: contiguous vectors expected"))
    Dp = F.D === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(pointer(F.D))
    GC.@preserve F check(ccall((:covgram_bh_taylor_mvm, libcovgram), Cint,
                               (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Int32, Ptr{Cvoid}, Int64, Int32),
                               F.handle, w, b, Float64(α), Float64(β), Float64(θ), Int32(use_com), Dp, Int64(F.D === nothing ? 0 : length(F.D)), HOST))
    b
end
# the operator minres! sees: the Taylor product of F (use_com = false: an exactly linear map)
struct TaylorProduct{T} <: AbstractMatrix{T}
    F::DeviceBarnesHut{T}
    use_com::Bool
end
Base.size(A::TaylorProduct) = size(A.F)
Base.getindex(A::TaylorProduct, i::Integer, j::Integer) = A.F[i, j]
LinearAlgebra.mul!(b::StridedVector{T}, A::TaylorProduct{T}, w::StridedVector{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat} =
    taylor!(b, A.F, w, α, β; use_com = A.use_com)
function LinearAlgebra.ldiv!(x::StridedVector{T}, F::DeviceBarnesHut{T}, b::StridedVector{T}; use_com::Bool = true, kwargs...) where {T <: DevFloat}
    CovarianceFunctions.IterativeSolvers.minres!(x, TaylorProduct{T}(F, use_com), b; kwargs...)
end
Base.:\(F::DeviceBarnesHut{T}, b::StridedVector{T}; kwargs...) where {T <: DevFloat} = ldiv!(zeros(T, F.m), F, b; initially_zero = true, kwargs...)
LinearAlgebra.mul!(b::StridedVector{T}, F::DeviceBarnesHut{T}, w::StridedVector{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat} =
    barneshut!(b, F, w, α, β)
function LinearAlgebra.mul!(B::StridedMatrix{T}, F::DeviceBarnesHut{T}, W::StridedMatrix{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    size(B, 2) == size(W, 2) || throw(DimensionMismatch("mul!: size mismatch"))
    for c in 1:size(W, 2)
        barneshut!(view(B, :, c), F, view(W, :, c), α, β)
    end
    B
end
Base.:*(F::DeviceBarnesHut{T}, w::StridedVector{T}) where {T <: DevFloat} = mul!(zeros(T, F.n), F, w)
# CovGram.BarnesHutFactorization: the signatures of the reference's constructors (src/barneshut.jl:25-39) as a function of THIS module (the
# reference's own type and constructors stay as they are).  A kernel without a device spec gets the reference's factorization; a kernel
# that has one but is refused (composites, dot-product kernels, d > 8) is refused by the library, by name, through check(...)
function BarnesHutFactorization(k, x, y = x, D = nothing; θ::Real = 1 / 4, leafsize::Int = 16)
    spec = ENABLED[] ? device_kernel_for(k) : nothing
    T = CovarianceFunctions.gramian_eltype(k, x[1], y[1])
    (spec === nothing || !(T <: DevFloat)) && return CovarianceFunctions.BarnesHutFactorization(k, x, y, D; θ = θ, leafsize = leafsize)
    DeviceBarnesHut(k, x, y, D, T, θ, leafsize, spec)
end
BarnesHutFactorization(G::Gramian; θ::Real = 1 / 4, leafsize::Int = 16) = BarnesHutFactorization(G.k, G.x, G.y; θ = θ, leafsize = leafsize)

# --- src/stationary.jl:213-217: SpectralMixture(w, μ, l) = Σ_q w_q Cosine(μ_q) ARD(EQ(), l_q) -> covgram_sm_* (one fused pass) --------
# The kernel is GenericInput in the reference (its factors mix two traits), so it has no CKernel encoding: the handle carries the
# parameters.  w: Q weights, μ and invl: d × Q (column q = component q, which is the library's row-major Q × d), invl = 1 ./ l.
const SM_MAX_COMPONENTS, SM_MAX_D = 32, 16   # COVGRAM_SM_MAX_COMPONENTS, COVGRAM_SM_MAX_D
mutable struct DeviceSpectralMixture{T} <: AbstractMatrix{T}
    handle::Ptr{Cvoid}
    X::Points; Y::Points
    n::Int; m::Int
    w::Vector{Float64}; μ::Matrix{Float64}; invl::Matrix{Float64}
    function DeviceSpectralMixture(w::AbstractVector, μ::AbstractMatrix, invl::AbstractMatrix, x, y, ::Type{T}) where {T <: DevFloat}
        size(μ) == size(invl) && size(μ, 2) == length(w) || throw(DimensionMismatch("SpectralMixture: μ and invl must be d × Q"))
        wd = Vector{Float64}(w); μd = Matrix{Float64}(μ); ld = Matrix{Float64}(invl)
        X = points(x, T); Y = x === y ? X : points(y, T)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:covgram_sm_create, libcovgram), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32),
                    ctx(), h, length(wd), size(μd, 1), wd, μd, ld, T === Float32 ? Int32(0) : Int32(1)))
        S = new{T}(h[], X, Y, length(x), length(y), wd, μd, ld)
        finalizer(q -> ccall((:covgram_sm_destroy, libcovgram), Cint, (Ptr{Cvoid},), q.handle), S)
        S
    end
end
Base.size(S::DeviceSpectralMixture) = (S.n, S.m)
function sm_isotropic(S::DeviceSpectralMixture)
    q = Ref{Int32}(0); d = Ref{Int32}(0); dt = Ref{Int32}(0); iso = Ref{Int32}(0)
    check(ccall((:covgram_sm_info, libcovgram), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Int32}), S.handle, q, d, dt, iso))
    iso[] != 0
end
function LinearAlgebra.mul!(y::StridedVecOrMat{T}, S::DeviceSpectralMixture{T}, a::StridedVecOrMat{T}, α::Real = 1, β::Real = 0) where {T <: DevFloat}
    size(a, 1) == S.m && size(y, 1) == S.n && size(y, 2) == size(a, 2) || throw(DimensionMismatch("mul!: size mismatch"))
    size(a, 2) == 0 && return y                        # no columns: nothing to do (the ABI requires nrhs >= 1)
    check(ccall((:covgram_sm_mvm, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Float64, Float64, Int32),
                S.handle, S.X.handle, S.Y.handle, a, max(stride(a, 2), S.m), y, max(stride(y, 2), S.n), size(a, 2), Float64(α), Float64(β), HOST))
    return y
end
function Base.Matrix(S::DeviceSpectralMixture{T}) where {T <: DevFloat}
    out = Matrix{T}(undef, S.n, S.m)
    check(ccall((:covgram_sm_matrix, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32),
                S.handle, S.X.handle, S.Y.handle, out, max(S.n, 1), HOST))
    out
end
Base.getindex(S::DeviceSpectralMixture, i::Integer, j::Integer) = Matrix(S)[i, j]   # (for show and tests; not a hot path)

# --- hyper-parameter gradients of Σ_t U[:, t]' S A[:, t] in one pass (covgram_bilinear_grad_sm): a (1 + 2d) × Q Float64 matrix whose column q is
#     [∂F/∂w_q; ∂F/∂μ_q (d numbers); E_q (d numbers, ∂F/∂(invl_kq²) = −E_kq / 2)], W = U A' (include/covgram.h)
function sm_bilinear_grad(S::DeviceSpectralMixture{T}, U::StridedVecOrMat{T}, A::StridedVecOrMat{T}) where {T <: DevFloat}
    size(U, 1) == S.n && size(A, 1) == S.m && size(U, 2) == size(A, 2) || throw(DimensionMismatch("sm_bilinear_grad: U is n × nvec, A is m × nvec"))
    out = Matrix{Float64}(undef, 1 + 2 * size(S.μ, 1), length(S.w))
    check(ccall((:covgram_bilinear_grad_sm, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Int32),
                S.handle, S.X.handle, S.Y.handle, U, max(stride(U, 2), S.n), A, max(stride(A, 2), S.m), size(U, 2), out, HOST))
    return out
end

# --- hyper-parameter gradients of Σ_t U[:, t]' G A[:, t] in one pass (covgram_bilinear_grad): out = [Σ W k, Σ W ∂k/∂param, Σ W (∂k/∂s) Δ_c² ...]
#     (one number Σ W (∂k/∂s) s for per_dim = false) in Float64, W = U A'; simple isotropic kernels only (include/covgram.h)
function bilinear_grad(G::Gramian{T}, U::StridedVecOrMat{T}, A::StridedVecOrMat{T}; per_dim::Bool = false) where {T <: DevFloat}
    spec = device_kernel_for(G.k)
    spec isa CKernel || throw(ArgumentError("bilinear_grad: simple isotropic kernels only"))
    n, m = size(G)
    size(U, 1) == n && size(A, 1) == m && size(U, 2) == size(A, 2) || throw(DimensionMismatch("bilinear_grad: U is n × nvec, A is m × nvec"))
    X = points(G.x, T); Y = G.x === G.y ? X : points(G.y, T)
    out = Vector{Float64}(undef, 2 + (per_dim ? length(first(G.x)) : 1))
    check(ccall((:covgram_bilinear_grad, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Float64}, Int32),
                ctx(), kref(spec), X.handle, Y.handle, U, max(stride(U, 2), n), A, max(stride(A, 2), m), size(U, 2), Int32(per_dim), out, HOST))
    return out
end

# --- the gradient of the same bilinear form with respect to the ROW points in one pass (covgram_bilinear_input_grad): a d × n Float64 matrix
#     whose column i is Σ_j W_ij 2 (∂k/∂s)_ij (x_i − y_j), the column side held fixed (also for G.x === G.y: add the call with U and A swapped)
function bilinear_input_grad(G::Gramian{T}, U::StridedVecOrMat{T}, A::StridedVecOrMat{T}) where {T <: DevFloat}
    spec = device_kernel_for(G.k)
    spec isa CKernel || throw(ArgumentError("bilinear_input_grad: simple isotropic kernels only"))
    n, m = size(G)
    size(U, 1) == n && size(A, 1) == m && size(U, 2) == size(A, 2) || throw(DimensionMismatch("bilinear_input_grad: U is n × nvec, A is m × nvec"))
    X = points(G.x, T); Y = G.x === G.y ? X : points(G.y, T)
    dX = Matrix{Float64}(undef, length(first(G.x)), n)
    check(ccall((:covgram_bilinear_input_grad, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Int32),
                ctx(), kref(spec), X.handle, Y.handle, U, max(stride(U, 2), n), A, max(stride(A, 2), m), size(U, 2), dX, HOST))
    return dX
end

# --- the same for a spectral mixture (covgram_bilinear_input_grad_sm): column i is Σ_j W_ij Σ_q w_q e_q (−2π μ_q sin φ_q − invl_q² ∘ r cos φ_q),
#     r = x_i − y_j, the column side held fixed (also for one point set: add the call with U and A swapped)
function bilinear_input_grad(S::DeviceSpectralMixture{T}, U::StridedVecOrMat{T}, A::StridedVecOrMat{T}) where {T <: DevFloat}
    size(U, 1) == S.n && size(A, 1) == S.m && size(U, 2) == size(A, 2) || throw(DimensionMismatch("bilinear_input_grad: U is n × nvec, A is m × nvec"))
    dX = Matrix{Float64}(undef, size(S.μ, 1), S.n)
    check(ccall((:covgram_bilinear_input_grad_sm, libcovgram), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Int32),
                S.handle, S.X.handle, S.Y.handle, U, max(stride(U, 2), S.n), A, max(stride(A, 2), S.m), size(U, 2), dX, HOST))
    return dX
end

end # module
