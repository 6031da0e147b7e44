"""The structured-operator calls of tests/test_gpu_host_api._staged_entry_points (Toeplitz, Kronecker, low rank, Barnes-Hut, Levinson / Durbin /
Trench) on the library named by COVGRAM_LIB (default: the in-tree build), HOST and DEVICE and in place where square: one line per call with the
sha256 of the result bytes, the timed launch count and every last_* info key.  Run once per library, one process each, and compare the outputs
line by line (profiles/structured_driver_ab.txt): `python3 tools/structured_ab.py OUT.txt`."""
import ctypes as C, hashlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("covariancefunctions.jl_amd", "tests", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import covgram as cg
import test_gpu_host_api as t
KEYS = ["last_dense_path", "last_jsplit", "last_kron_path", "last_mfma_lds", "last_mfma_sym", "last_dense_sym", "last_dense_bcast", "last_mfma_f16",
        "last_inkernel_reduce", "last_grad_expand", "last_grad_bcast", "last_grad_path", "last_grad_jsplit", "last_hess_path", "last_vgh_path",
        "last_matrix_path", "last_block_matrix_path", "last_sum_fused", "last_mfma_instance", "last_mfma_sym_rt"]
STRUCT = ("covgram_toeplitz", "covgram_kron", "covgram_lowrank", "covgram_bh")
lib, f = cg._ffi.lib(), cg._ffi
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
out.write("keys: " + " ".join(k[5:] for k in KEYS) + "\n")
for dt in (np.float32, np.float64):
    h = f._P()
    f.check(lib.covgram_ctx_create(C.byref(h), 0, None))
    eps, close = t._staged_entry_points(cg, h, dt)
    f.check(lib.covgram_ctx_set_option(h, b"time_kernels", 1))
    ms, cnt, v = C.c_double(), C.c_int64(), C.c_int64()
    for name, (square_ok, run) in eps.items():
        if not name.startswith(STRUCT):
            continue
        for loc in (f.HOST, f.DEVICE):
            for inplace in ((False, True) if square_ok else (False,)):
                f.check(lib.covgram_ctx_kernel_time(h, C.byref(ms), C.byref(cnt), 1))
                res, _, rows = run(loc, inplace)
                rc = lib.covgram_ctx_kernel_time(h, C.byref(ms), C.byref(cnt), 1)
                keys = []
                for k in KEYS:
                    f.check(lib.covgram_ctx_get_info(h, k.encode(), C.byref(v))); keys.append(v.value)
                out.write("%s %s [%s%s]: sha256 %s launches %d timer_rc %d keys %s\n" % (
                    name, "f32" if dt == np.float32 else "f64", "host" if loc == f.HOST else "device", ", in place" if inplace else "",
                    hashlib.sha256(res.tobytes()).hexdigest()[:32], cnt.value, rc, ",".join(map(str, keys))))
                out.flush()
    f.check(lib.covgram_ctx_set_option(h, b"time_kernels", 0))
    close()
    assert lib.covgram_ctx_destroy(h) == 0
