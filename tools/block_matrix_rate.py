"""Bytes written per second by covgram_block_matrix (BlockGramian.to_dense()) for the four block Gramians, beside covgram_matrix of a
scalar Gramian with the same number of output bytes, written to profiles/block_matrix.txt.

Protocol (that of tools/hessian_rate.py / tools/vgh_rate.py): ONE child process (fresh GPU context, its own time limit).  In the child, per
shape: the block matrix and then the scalar Matrix(G) of side n B (same output bytes, d = 3), each into a buffer allocated once, 3 warm-up
calls, then 7 batches of back-to-back calls (as many as fill ~0.2 s, at least 3) bracketed by one pair of HIP events each; the figure is
the MEDIAN batch time per call (min and max beside it), the whole call through the C ABI.  Both kernels are bound by the same streaming
stores, so the scalar figure measured in the same process is the yardstick.  Last, the inherited LazyOperator.to_dense (an identity of
size m B through the block MVM: what to_dense() was before covgram_block_matrix) at one small shape, for the speed-up.

    python tools/block_matrix_rate.py              all shapes -> profiles/block_matrix.txt
    python tools/block_matrix_rate.py --child      what the child runs (lines on stdout)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (kind, d, n, precision): outputs of 0.25 ... 2 GiB
SHAPES = [("gradient", 8, 2048, "f32"), ("gradient", 8, 1024, "f64"), ("gradient", 32, 512, "f32"), ("gradient", 32, 256, "f64"),
          ("value-gradient", 7, 2048, "f32"), ("hessian", 8, 256, "f32"), ("hessian", 8, 128, "f64"), ("hessian", 16, 64, "f32"),
          ("hessian", 16, 32, "f64"), ("value-gradient-hessian", 8, 128, "f64")]


def child():
    sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
    import ctypes as C
    import numpy as np
    import torch
    import covgram as cg
    f, lib = cg._ffi, cg._ffi.lib()
    wraps = {"gradient": (cg.GradientKernel, lambda d: d), "value-gradient": (cg.ValueGradientKernel, lambda d: d + 1),
             "hessian": (cg.HessianKernel, lambda d: d * d), "value-gradient-hessian": (cg.ValueGradientHessianKernel, lambda d: 1 + d + d * d)}

    def timed(call):
        for _ in range(3):
            call()
        torch.cuda.synchronize()

        def batch(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / reps
        reps = max(3, int(200.0 / max(batch(2), 1e-3)))
        ms = sorted(batch(reps) for _ in range(7))
        return ms[3], ms[0], ms[-1], reps

    for kind, d, n, prec in SHAPES:
        dt = torch.float64 if prec == "f64" else torch.float32
        rng = np.random.default_rng(n + d)
        X = torch.from_numpy(rng.standard_normal((n, d))).to(device="cuda", dtype=dt)
        wrap, bs = wraps[kind]
        B = bs(d); N = n * B
        G = cg.gramian(wrap(cg.Lengthscale(cg.EQ(), float(np.sqrt(d)))), X)
        buf = torch.empty((N, N), dtype=dt, device="cuda")
        spec = G._lower(); ctx = G.inner._px.ctx.bind_stream()
        b = timed(lambda: f.check(lib.covgram_block_matrix(ctx, G._kind(), f.kref(spec), G.inner._px.handle, G.inner._py.handle,
                                                           f._P(buf.data_ptr()), N, f.DEVICE)))
        key = cg.get_info("last_block_matrix_path")
        S = cg.gramian(cg.Lengthscale(cg.EQ(), float(np.sqrt(3))), torch.from_numpy(rng.standard_normal((N, 3))).to(device="cuda", dtype=dt))
        sspec = S._spec()
        s = timed(lambda: f.check(lib.covgram_matrix(ctx, f.kref(sspec), S._px.handle, S._py.handle, f._P(buf.data_ptr()), N, f.DEVICE)))
        skey = cg.get_info("last_matrix_path")
        gb = N * N * buf.element_size() / 1e9
        print(f"{kind:22s} d={d:2d} n={n:5d} {prec} B={B:4d} {gb * 1e9 / 2 ** 30:5.2f} GiB key={key}: {b[0]:8.3f} ms (min {b[1]:.3f}, max {b[2]:.3f}; {b[3]} per batch) "
              f"= {gb / b[0]:6.3f} TB/s   scalar Matrix(G) {N} x {N} key={skey}: {s[0]:8.3f} ms (min {s[1]:.3f}, max {s[2]:.3f}) = {gb / s[0]:6.3f} TB/s   "
              f"ratio block / scalar rate {s[0] / b[0]:.3f}", flush=True)
        del buf, G, S
    # the inherited to_dense(): an m B x m B identity through the block MVM
    d, n = 8, 256
    X = torch.from_numpy(np.random.default_rng(1).standard_normal((n, d))).cuda()
    G = cg.gramian(cg.GradientKernel(cg.Lengthscale(cg.EQ(), float(np.sqrt(d)))), X)
    new = timed(G.to_dense)
    old = timed(lambda: cg.LazyOperator.to_dense(G))
    print(f"gradient d={d} n=m={n} f64 ({n * d} x {n * d}): to_dense() {new[0]:.4f} ms (min {new[1]:.4f}, max {new[2]:.4f})   inherited LazyOperator.to_dense "
          f"(identity through the MVM) {old[0]:.3f} ms (min {old[1]:.3f}, max {old[2]:.3f})   speed-up {old[0] / new[0]:.1f}x", flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child()
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        sys.exit(r.returncode)
    out = os.path.join(ROOT, "profiles", "block_matrix.txt")
    doc = __doc__.split("\n\n")[1]
    with open(out, "w") as fh:
        fh.write("Dense block Gramians (covgram_block_matrix) beside the scalar Matrix(G) (covgram_matrix) of the same output size, x = y ~ N(0, I), "
                 "EQ, lengthscale sqrt(d); tools/block_matrix_rate.py\n\n" + doc + "\n\n" + r.stdout)
    print("wrote", out)


if __name__ == "__main__":
    main()
