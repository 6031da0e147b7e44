"""A/B of two builds of the library over the gradient block-MVM entries (covgram_grad_mvm, covgram_valgrad_mvm, covgram_grad_mvm_mixed), on the
library named by COVGRAM_LIB (default: the in-tree build).  Run once per library, one process each, under a time limit of its own, and compare the
outputs line by line (profiles/grad_driver_ab.txt); the protocol of tools/structured_ab.py.

    python3 tools/grad_driver_ab.py record OUT.txt     one line per call: sha256 of the result buffer, timed launch count, every last_* info key.
                                                       Calls: the smallest shape that reaches each branch of the two drivers, with host and with
                                                       device pointers, in place (y is a) where square; seeded inputs.
    python3 tools/grad_driver_ab.py rate               launch-bound shape per entry (n = m = 256, d = 3, fp64, device pointers): 5 warm-up calls,
                                                       then 7 batches of 200 back-to-back calls between one pair of HIP events each; median
                                                       (min, max) batch time per call in us.  The host-side cost of a call is what it measures."""
import ctypes as C, hashlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("covariancefunctions.jl_amd", "tests", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import covgram as cg
import grad_mixed_ref as R
import test_gpu_grad_mixed as M
KEYS = ["last_dense_path", "last_jsplit", "last_inkernel_reduce", "last_grad_expand", "last_grad_bcast", "last_grad_path", "last_grad_jsplit", "last_hess_path",
        "last_vgh_path", "last_matrix_path", "last_block_matrix_path", "last_sum_fused", "last_grad_mixed_path", "last_grad_mixed_jsplit"]
OPTIONS = {"jsplit": 0, "target_wgs": 0, "grad_keep_r": -1, "grad_expand": -1, "grad_bcast": -1, "grad_mixed_panel": 0}   # name: default
lib, f = cg._ffi.lib(), cg._ffi
P = lambda v: v.ctypes.data_as(C.c_void_p)
F32, F64 = np.float32, np.float64
DIRECT = dict(grad_expand=0, grad_bcast=0)
MIXED = "maternp2+dot^2+nn"
HANDLES = []


def single_cases():
    """(label, kernel, n, m, d, dtype, nrhs, options, x is y) of covgram_grad_mvm / covgram_valgrad_mvm"""
    eq = cg.EQ()
    return [("lane direct", eq, 333, 517, 3, F64, 1, {}, False), ("two-column pass", eq, 130, 130, 3, F64, 3, {}, True),
            ("expanded f64", eq, 200, 300, 8, F64, 1, {}, False), ("expanded f32", eq, 200, 300, 8, F32, 1, {}, False),
            ("broadcast 1 wave", eq, 200, 300, 32, F64, 1, dict(grad_bcast=1), False), ("broadcast 4 waves", eq, 200, 300, 32, F64, 1, dict(grad_bcast=4), False),
            ("slab cap and round snap", eq, 8150, 8191, 48, F64, 1, DIRECT, False),      # tests/test_gpu_grad_rowwise.py
            ("panel one panel", cg.Lengthscale(eq, 2.0), 300, 13, 65, F64, 1, {}, False), ("panel one panel f32", cg.Lengthscale(eq, 2.0), 300, 29, 70, F32, 1, {}, False),
            ("panel z slices", eq, 8150, 1000, 65, F64, 1, {}, False), ("panel several panels", eq, 4096, 4100, 65, F64, 1, {}, False),
            ("panel forced at d = 5", eq, 300, 220, 5, F64, 1, dict(grad_keep_r=2), False), ("dot product", cg.Dot() ** 2, 333, 517, 3, F64, 1, {}, False),
            ("sum with a constant", cg.EQ() + cg.RQ(2.0) + 1.5, 130, 130, 3, F64, 2, {}, True), ("composite product", cg.EQ() * cg.RQ(2.0), 130, 200, 8, F32, 1, {}, False),
            ("no columns", eq, 37, 0, 5, F64, 1, {}, False), ("no rows", eq, 0, 37, 5, F64, 1, {}, False)]


def mixed_cases():
    """the rows of ROUTES in tests/test_gpu_grad_mixed.py, both element types, and the empty products"""
    out = [(route, n, m, d, dt, 1, opts, same) for route, (n, m, d, same, opts, _) in M.ROUTES.items() for dt in (F64, F32)]
    return out + [("lane nrhs 3", 130, 130, 5, F64, 3, {}, True), ("no columns", 37, 0, 5, F64, 1, {}, False), ("no rows", 0, 37, 40, F64, 1, {}, False)]


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
    """(label, square, call(pa, lda, py, ldy, loc) -> rc, block size, n, m, nrhs, options) for one element type"""
    out = []
    for i, (label, k, n, m, d, cdt, nrhs, opts, same) in enumerate(single_cases()):
        if cdt != dt:
            continue
        X, Y = clouds(100 + i, n, m, d, dt, same)
        hx = points(h, X); hy = hx if same else points(h, Y)
        spec = cg.kernels.require_device_spec(k)
        for vg, fn in ((0, lib.covgram_grad_mvm), (1, lib.covgram_valgrad_mvm)):
            out.append((f"{fn.__name__} {label}", same, lambda pa, lda, py, ldy, loc, fn=fn, spec=spec, hx=hx, hy=hy, nrhs=nrhs:
                        fn(h, f.kref(spec), hx, hy, pa, lda, py, ldy, nrhs, -0.7, 1.3, loc), d + vg, X.shape[0], Y.shape[0], nrhs, opts, (X, Y, spec)))
    k = R.kernels(cg)[MIXED]
    spec = cg.kernels.require_mixed_gradient_spec(k)
    for label, n, m, d, cdt, nrhs, opts, same in mixed_cases():
        if cdt != dt:
            continue
        X, Y = (a.astype(dt) for a in R.clouds(MIXED, max(n, 1), max(m, 1), d, same))
        X, Y = np.ascontiguousarray(X[:n]), (None if same else np.ascontiguousarray(Y[:m]))
        hx = points(h, X); hy = hx if same else points(h, Y)
        for vg in (0, 1):
            out.append((f"covgram_grad_mvm_mixed value={vg} {label}", same, lambda pa, lda, py, ldy, loc, hx=hx, hy=hy, nrhs=nrhs, vg=vg:
                        lib.covgram_grad_mvm_mixed(h, C.byref(spec), hx, hy, pa, lda, py, ldy, nrhs, -0.7, 1.3, vg, loc), d + vg, n, m, nrhs, opts, (X, Y, spec)))
    return out


def record(path):
    out = open(path, "w") if path else sys.stdout
    out.write("keys: " + " ".join(k[5:] for k in KEYS) + "\n")
    ms, cnt, v = C.c_double(), C.c_int64(), C.c_int64()
    for dt in (F64, F32):
        h = f._P()
        f.check(lib.covgram_ctx_create(C.byref(h), 0, None))
        f.check(lib.covgram_ctx_set_option(h, b"time_kernels", 1))
        for ci, (name, square, call, B, n, m, nrhs, opts, keep) in enumerate(calls(h, dt)):
            for loc in (f.HOST, f.DEVICE):
                for inplace in ((False, True) if square else (False,)):
                    rng = np.random.default_rng(1000 + ci)
                    lda, ldy = (m * B + 3, m * B + 3) if inplace else (m * B + 5, n * B + 3)
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
    eq, mixed = cg.kernels.require_device_spec(cg.EQ()), cg.kernels.require_mixed_gradient_spec(R.kernels(cg)[MIXED])
    entries = [("covgram_grad_mvm", d, lambda pa, py, B: lib.covgram_grad_mvm(h, f.kref(eq), hx, hx, pa, n * B, py, n * B, 1, 1.0, 0.0, f.DEVICE)),
               ("covgram_valgrad_mvm", d + 1, lambda pa, py, B: lib.covgram_valgrad_mvm(h, f.kref(eq), hx, hx, pa, n * B, py, n * B, 1, 1.0, 0.0, f.DEVICE)),
               ("covgram_grad_mvm_mixed", d, lambda pa, py, B: lib.covgram_grad_mvm_mixed(h, C.byref(mixed), hx, hx, pa, n * B, py, n * B, 1, 1.0, 0.0, 0, f.DEVICE))]
    line = []
    for name, B, call in entries:
        a = torch.randn(n * B, dtype=torch.float64, device="cuda"); y = torch.empty_like(a)
        pa, py = a.data_ptr(), y.data_ptr()
        for _ in range(5):
            f.check(call(pa, py, B))
        torch.cuda.synchronize()
        ts = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                call(pa, py, B)
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
