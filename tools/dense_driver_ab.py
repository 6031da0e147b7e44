"""A/B of two builds of the library over the scalar MVM entries (covgram_mvm, covgram_mvm_mixed, covgram_matrix_mixed), on the library named
by COVGRAM_LIB (default: the in-tree build).  Run once per library, one process each, under a time limit of its own, and compare the outputs
line by line (profiles/dense_driver_ab.txt); the protocol of tools/grad_driver_ab.py.

    python3 tools/dense_driver_ab.py record OUT.txt    one line per call: sha256 of the result buffer, timed launch count, the last_* info keys of the two
                                                       drivers.  Calls: a few hundred points on every branch of the lane-per-row routes, the Sum split
                                                       and the mixed partition, with host and with device pointers, in place (y is a) where square,
                                                       alpha = -0.7, beta = 1.3 on a prefilled y, lda / ldy larger than the rows; seeded inputs.
    python3 tools/dense_driver_ab.py rate              launch-bound shape (n = m = 256, d = 3, fp64, device pointers): 5 warm-up calls, then 7 batches
                                                       of 200 back-to-back calls between one pair of HIP events each; median (min, max) batch time per
                                                       call in us.  The host-side cost of a call is what it measures."""
import ctypes as C, hashlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("covariancefunctions.jl_amd", "tests", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import covgram as cg
import mixed_ref as R
import test_gpu_mixed as M
KEYS = ["last_dense_path", "last_jsplit", "last_inkernel_reduce", "last_dense_sym", "last_dense_bcast", "last_mfma_sym", "last_sum_fused", "last_mixed_path",
        "last_mixed_jsplit", "last_mixed_matrix_path"]
OPTIONS = {"jsplit": 0, "inkernel_reduce": -1, "dense_sym": -1, "dense_bcast": -1, "dense_variant": 0, "mixed_fuse": 0}   # name: default
lib, f = cg._ffi.lib(), cg._ffi
P = lambda v: v.ctypes.data_as(C.c_void_p)
F32, F64 = np.float32, np.float64
HANDLES = []


def dense_cases():
    """(label, kernel, n, m, d, dtype, nrhs, options, x is y) of covgram_mvm"""
    eq, direct = cg.EQ(), dict(dense_variant=1)
    out = [(f"lanes nrhs {r}", eq, 333, 517, 3, F64, r, {}, False) for r in (1, 3, 4, 5)]
    out += [("lanes in place", eq, 130, 130, 3, F64, 5, {}, True), ("lanes jsplit 1", eq, 333, 517, 3, F64, 1, dict(jsplit=1), False),
            ("lanes f32 nrhs 5", cg.MaternP(2), 333, 517, 5, F32, 5, direct, False), ("lanes f32 jsplit 1", eq, 333, 517, 3, F32, 1, dict(direct, jsplit=1), False),
            ("in-kernel reduce", eq, 333, 517, 3, F64, 1, dict(inkernel_reduce=1), False), ("in-kernel reduce f32 nrhs 3", eq, 200, 300, 8, F32, 3, dict(direct, inkernel_reduce=1), False),
            ("wide d 65", cg.Lengthscale(eq, 2.0), 300, 200, 65, F64, 1, {}, False), ("wide d 65 f32 nrhs 5", cg.Lengthscale(eq, 2.0), 300, 200, 65, F32, 5, direct, False),
            ("wide d 65 in-kernel reduce asked", cg.Lengthscale(eq, 2.0), 300, 200, 65, F64, 1, dict(inkernel_reduce=1), False),
            ("symmetric f64", eq, 333, 333, 3, F64, 1, dict(dense_sym=1), True), ("symmetric f32", cg.Exponential(), 520, 520, 3, F32, 1, dict(direct, dense_sym=1), True),
            ("broadcast d 16", eq, 333, 517, 16, F64, 1, dict(dense_bcast=1), False), ("broadcast d 12 jsplit 1", eq, 333, 517, 12, F64, 1, dict(dense_bcast=1, jsplit=1), False),
            ("broadcast symmetric d 16", eq, 333, 333, 16, F64, 1, dict(dense_bcast=1, dense_sym=1), True),
            ("sum with a constant", cg.EQ() + cg.RQ(2.0) + 1.5, 130, 130, 3, F64, 2, {}, True), ("sum with a scaled product", 2.5 * cg.EQ() * cg.RQ(2.0) + cg.MaternP(1), 200, 300, 3, F64, 1, {}, False),
            ("composite product", cg.EQ() * cg.RQ(2.0), 130, 200, 8, F32, 1, {}, False), ("composite product f64 nrhs 4", 0.5 * cg.EQ() * cg.RQ(2.0), 130, 200, 8, F64, 4, {}, False),
            ("dot product factored", cg.Dot(), 333, 517, 3, F64, 1, {}, False), ("dot product squared", cg.Dot() ** 2, 333, 517, 3, F64, 1, {}, False),
            ("matrix cores nrhs 2", eq, 333, 517, 3, F32, 2, {}, False), ("matrix cores nrhs 2 jsplit 3", eq, 333, 517, 3, F32, 2, dict(jsplit=3), False),
            ("matrix cores eq", eq, 333, 517, 3, F32, 1, dict(jsplit=3), False),
            ("no columns", eq, 137, 0, 5, F64, 3, {}, False), ("no columns f32", eq, 137, 0, 5, F32, 1, {}, False), ("no rows", eq, 0, 137, 5, F64, 1, {}, False)]
    return out


def mixed_cases():
    """(label, name of mixed_ref.kernels, n, m, d, dtype, nrhs, options, x is y) of covgram_mvm_mixed: the rows of DEFAULT in tests/test_gpu_mixed.py"""
    out = [(f"{name} lane", name, 200, 333, 5, dt, 1, {}, False) for name in M.DEFAULT for dt in (F64, F32)]
    for dt in (F64, F32):
        big = "maternp2+dot^2+nn"
        out += [("sum3 chunked d 40", big, 200, 333, 40, dt, 1, {}, False), ("sum3 chunked d 40 nrhs 5", big, 130, 130, 40, dt, 5, {}, True),
                ("sum3 lane nrhs 4", big, 130, 130, 5, dt, 4, {}, True), ("sum3 lane nrhs 5 jsplit 1", big, 200, 333, 32, dt, 5, dict(jsplit=1), False),
                ("sum3 fused", big, 200, 333, 5, dt, 1, dict(mixed_fuse=1), False), ("constant term fused", "eq+(dot^2+1)", 200, 333, 5, dt, 1, dict(mixed_fuse=1), False),
                ("constant term nrhs 5", "eq+(dot^2+1)", 130, 130, 3, dt, 5, {}, True), ("product with a constant term", "eq*(dot^2+1)", 200, 333, 40, dt, 4, {}, False),
                ("no columns", big, 137, 0, 5, dt, 2, {}, False)]
    return out


def points(h, X):
    hp = f._P()
    f.check(lib.covgram_points_create(h, C.byref(hp), P(X), X.shape[0], X.shape[1], f.F64 if X.dtype == F64 else f.F32, f.HOST))
    HANDLES.append(hp)
    return hp


def close(h):
    while HANDLES:
        f.check(lib.covgram_points_destroy(HANDLES.pop()))
    f.check(lib.covgram_ctx_destroy(h))


def clouds(seed, n, m, d, dt, same):
    rng = np.random.default_rng(seed)
    s = 0.8 * min(1.0, (3.0 / d) ** 0.5)
    X = np.ascontiguousarray((s * rng.standard_normal((n, d))).astype(dt))
    return X, (X if same else np.ascontiguousarray((s * rng.standard_normal((m, d))).astype(dt)))


def calls(h, dt):
    """(label, square, call(pa, lda, py, ldy, loc) -> rc, n, m, nrhs, options, what to keep alive) for one element type"""
    out = []
    for i, (label, k, n, m, d, cdt, nrhs, opts, same) in enumerate(dense_cases()):
        if cdt != dt:
            continue
        X, Y = clouds(100 + i, n, m, d, dt, same)
        hx = points(h, X); hy = hx if same else points(h, Y)
        spec = cg.kernels.require_device_spec(k)
        out.append((f"covgram_mvm {label}", same, lambda pa, lda, py, ldy, loc, spec=spec, hx=hx, hy=hy, nrhs=nrhs:
                    lib.covgram_mvm(h, f.kref(spec), hx, hy, pa, lda, py, ldy, nrhs, -0.7, 1.3, loc), n, m, nrhs, opts, (X, Y, spec)))
    ks = R.kernels(cg)
    for label, name, n, m, d, cdt, nrhs, opts, same in mixed_cases():
        if cdt != dt:
            continue
        X, Y = (a.astype(dt) for a in R.clouds32(name, max(n, 1), max(m, 1), d, same))
        X, Y = np.ascontiguousarray(X[:n]), (None if same else np.ascontiguousarray(Y[:m]))
        hx = points(h, X); hy = hx if same else points(h, Y)
        spec = cg.kernels.require_mixed_spec(ks[name])
        out.append((f"covgram_mvm_mixed {label}", same, lambda pa, lda, py, ldy, loc, spec=spec, hx=hx, hy=hy, nrhs=nrhs:
                    lib.covgram_mvm_mixed(h, C.byref(spec), hx, hy, pa, lda, py, ldy, nrhs, -0.7, 1.3, loc), n, m, nrhs, opts, (X, Y, spec)))
    for d in (3, 40):   # covgram_matrix_mixed: the result tile (ldo > n) in the place of y, no a
        n, m = 200, 333
        X, Y = (np.ascontiguousarray(a.astype(dt)) for a in R.clouds32("maternp2+dot^2+nn", n, m, d, False))
        hx, hy = points(h, X), points(h, Y)
        spec = cg.kernels.require_mixed_spec(ks["maternp2+dot^2+nn"])
        out.append((f"covgram_matrix_mixed d {d}", False, lambda pa, lda, py, ldy, loc, spec=spec, hx=hx, hy=hy:
                    lib.covgram_matrix_mixed(h, C.byref(spec), hx, hy, py, ldy, loc), n, n, m, {}, (X, Y, spec)))
    return out


def record(path):
    out = open(path, "w") if path else sys.stdout
    out.write("keys: " + " ".join(k[5:] for k in KEYS) + "\n")
    ms, cnt, v = C.c_double(), C.c_int64(), C.c_int64()
    for dt in (F64, F32):
        h = f._P()
        f.check(lib.covgram_ctx_create(C.byref(h), 0, None))
        f.check(lib.covgram_ctx_set_option(h, b"time_kernels", 1))
        for ci, (name, square, call, n, m, nrhs, opts, keep) in enumerate(calls(h, dt)):
            for loc in (f.HOST, f.DEVICE):
                for inplace in ((False, True) if square else (False,)):
                    rng = np.random.default_rng(1000 + ci)
                    lda, ldy = (m + 3, m + 3) if inplace else (m + 5, n + 3)
                    a = rng.standard_normal((nrhs, lda)).astype(dt)
                    y = a if inplace else rng.standard_normal((nrhs, ldy)).astype(dt)
                    for key, val in {**OPTIONS, **opts}.items():
                        f.check(lib.covgram_ctx_set_option(h, key.encode(), val))
                    f.check(lib.covgram_ctx_kernel_time(h, C.byref(ms), C.byref(cnt), 1))
                    if loc == f.HOST:
                        rc = call(P(a), lda, P(y), ldy, loc)
                        res = y
                    else:
                        ta = torch.from_numpy(a).cuda()
                        ty = ta if inplace else torch.from_numpy(y).cuda()
                        rc = call(ta.data_ptr(), lda, ty.data_ptr(), ldy, loc)
                        torch.cuda.synchronize()
                        res = ty.cpu().numpy()
                    trc = lib.covgram_ctx_kernel_time(h, C.byref(ms), C.byref(cnt), 1)
                    keys = []
                    for k in KEYS:
                        f.check(lib.covgram_ctx_get_info(h, k.encode(), C.byref(v))); keys.append(v.value)
                    out.write("%s %s [%s%s]: rc %d sha256 %s launches %d timer_rc %d keys %s\n" % (
                        name, "f32" if dt == F32 else "f64", "host" if loc == f.HOST else "device", ", in place" if inplace else "", rc,
                        hashlib.sha256(res.tobytes()).hexdigest()[:32], cnt.value, trc, ",".join(map(str, keys))))
                    out.flush()
                    if rc not in (f.OK, f.EINVAL, f.EUNSUPPORTED):   # a HIP error: nothing more is started on the GPU
                        sys.exit("%s: rc %d: %s" % (name, rc, lib.covgram_last_error().decode()))
        close(h)


def rate():
    h = f._P()
    f.check(lib.covgram_ctx_create(C.byref(h), 0, None))
    n, d = 256, 3
    X, _ = clouds(7, n, n, d, F64, True)
    hx = points(h, X)
    eq = cg.kernels.require_device_spec(cg.EQ())
    sum2, sum3 = (cg.kernels.require_mixed_spec(k) for k in (cg.EQ() + cg.Dot(), cg.MaternP(2) + cg.Dot() ** 2 + cg.NeuralNetwork()))
    mvm = lambda nrhs: (lambda pa, py: lib.covgram_mvm(h, f.kref(eq), hx, hx, pa, n, py, n, nrhs, 1.0, 0.0, f.DEVICE))
    mixed = lambda spec: (lambda pa, py: lib.covgram_mvm_mixed(h, C.byref(spec), hx, hx, pa, n, py, n, 1, 1.0, 0.0, f.DEVICE))
    entries = [("covgram_mvm nrhs 1", 1, mvm(1)), ("covgram_mvm nrhs 4", 4, mvm(4)), ("covgram_mvm_mixed EQ+Dot", 1, mixed(sum2)),
               ("covgram_mvm_mixed MaternP(2)+Dot^2+NN", 1, mixed(sum3))]
    line = []
    for name, nrhs, call in entries:
        a = torch.randn(n * nrhs, dtype=torch.float64, device="cuda"); y = torch.empty_like(a)
        pa, py = a.data_ptr(), y.data_ptr()
        for _ in range(5):
            f.check(call(pa, py))
        torch.cuda.synchronize()
        ts = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                call(pa, py)
            e1.record(); e1.synchronize(); ts.append(e0.elapsed_time(e1) * 1e3 / 200)
        ts.sort()
        line.append(f"{name} n=m={n} d={d} f64: {ts[3]:.2f} us (min {ts[0]:.2f}, max {ts[-1]:.2f})")
    print("lib_ab " if os.environ.get("COVGRAM_LIB") else "in-tree", " | ".join(line), flush=True)
    close(h)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "rate":
        rate()
    else:
        record(sys.argv[2] if len(sys.argv) > 2 else None)
