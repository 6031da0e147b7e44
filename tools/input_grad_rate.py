"""Time of the fused input-gradient pass (covgram_bilinear_input_grad) beside what the library needed for the same numbers before it
existed, and beside its sibling of comparable work, written to profiles/input_grad.txt.

The earlier route to dX[i] = sum_t u_it sum_j grad_x k(x_i, y_j) a_jt: ONE ValueGradientKernel product with an nvec-column right-hand side whose
value entries are the columns of A and whose gradient entries are zero (nvec products; the library shares the pair evaluations between two
columns at a time), then the gradient rows of the result scaled by u_it and summed over t.  The Gramian and its right-hand side are built
outside the timed region, in its favour.  The sibling: the per_dim pass of covgram_bilinear_grad at the same shape (d + 2 numbers out of
the same pairs instead of n d).

Protocol: ONE process.  Shapes: EQ and MaternP(2) under a lengthscale, d = 3 and 8, n = m = 16384 and 131072 (two point sets), nvec = 1 and
17, fp32 and fp64; standard normal points and weights.  Per shape warm-up calls of all three (2; 1 at the larger size), then REPS rounds
that ALTERNATE the three, each call between its own pair of HIP events; medians with (min .. max).  The pair kernel with its reduction
alone comes from option "time_kernels" in a separate batch.  Per shape also the largest difference between the fused result and the
ValueGradient route, relative to the largest entry.  Last: the worst err / bound of the GPU test's case (a) clouds, recomputed here with
tests/input_grad_ref.py.  Nothing here is a share of peak.

    python tools/input_grad_rate.py [--out profiles/input_grad.txt] [--quick]      (--quick: n = 2^11 only, to rehearse the script)"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "input_grad.txt")
    quick = "--quick" in sys.argv
    sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
    import numpy as np
    import torch
    import covgram as cg
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    f = cg._ffi
    lines = ["Input gradients of sum_t u_t' G a_t on one MI355X: the fused pass covgram_bilinear_input_grad (n d numbers) against ONE ValueGradientKernel",
             "product with nvec value-only columns (+ scaling its gradient rows by U) and beside the per_dim pass of covgram_bilinear_grad, one process,",
             "alternating calls, medians of HIP-event times in ms with (min .. max) (protocol: tools/input_grad_rate.py).", ""]
    slower = []

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def fmt(ts):
        return f"{statistics.median(ts):9.3f} ({min(ts):.3f} .. {max(ts):.3f})"

    sizes = (2048,) if quick else (16384, 131072)
    kernels = (("EQ", lambda l: cg.Lengthscale(cg.EQ(), l)), ("MaternP(2)", lambda l: cg.Lengthscale(cg.MaternP(2), l)))
    lib = f.lib()
    for tdt, tname in ((torch.float32, "fp32"), (torch.float64, "fp64")):
        for n in sizes:
            reps, warm = (3, 1) if n > 16384 else (9, 2)
            for kname, make in kernels:
                for d in (3, 8):
                    for nvec in (1, 17):
                        rng = np.random.default_rng([n, d, nvec])
                        l = 0.5 * np.sqrt(d)
                        X = torch.from_numpy(rng.standard_normal((n, d))).to(dev, tdt)
                        Y = torch.from_numpy(rng.standard_normal((n, d))).to(dev, tdt)
                        Ut = torch.from_numpy(rng.standard_normal((nvec, n))).to(dev, tdt)      # column-major n x nvec
                        At = torch.from_numpy(rng.standard_normal((nvec, n))).to(dev, tdt)
                        G = cg.gramian(make(l), X, Y)
                        V = cg.gramian(cg.ValueGradientKernel(make(l)), X, Y)
                        spec = G._spec()
                        dX = torch.empty((n, d), dtype=torch.float64, device=dev)
                        out = torch.empty(2 + d, dtype=torch.float64, device=dev)
                        rhs = torch.zeros((n, d + 1, nvec), dtype=tdt, device=dev)              # blocks of d + 1: value first
                        rhs[:, 0, :] = At.t()
                        rhs = rhs.reshape(n * (d + 1), nvec)
                        res = torch.empty((n * (d + 1), nvec), dtype=tdt, device=dev)
                        dV = torch.empty((n, d), dtype=tdt, device=dev)

                        def fused():
                            f.check(lib.covgram_bilinear_input_grad(G._px.ctx.bind_stream(), f.kref(spec), G._px.handle, G._py.handle, f._P(Ut.data_ptr()), n,
                                                                    f._P(At.data_ptr()), n, nvec, C.cast(dX.data_ptr(), C.POINTER(C.c_double)), f.DEVICE))

                        def valgrad():
                            V.mul_(res, rhs)
                            dV.copy_((res.reshape(n, d + 1, nvec)[:, 1:, :] * Ut.t()[:, None, :]).sum(dim=2))

                        def sibling():
                            f.check(lib.covgram_bilinear_grad(G._px.ctx.bind_stream(), f.kref(spec), G._px.handle, G._py.handle, f._P(Ut.data_ptr()), n,
                                                              f._P(At.data_ptr()), n, nvec, 1, C.cast(out.data_ptr(), C.POINTER(C.c_double)), f.DEVICE))

                        for _ in range(warm):
                            fused(); valgrad(); sibling()
                        torch.cuda.synchronize()
                        diff = float((dX - dV.double()).abs().max() / dX.abs().max())
                        tf, tv, ts = [], [], []
                        for _ in range(reps):
                            tf.append(timed(fused)); tv.append(timed(valgrad)); ts.append(timed(sibling))
                        cg.set_option("time_kernels", 1); cg.kernel_time()
                        for _ in range(3):
                            fused()
                        kms, cnt = cg.kernel_time()
                        cg.set_option("time_kernels", 0)
                        mf, mv, ms = statistics.median(tf), statistics.median(tv), statistics.median(ts)
                        tag = f"{tname} {kname:10s} n = {n:6d} d = {d} nvec = {nvec:2d}"
                        lines += [f"{tag}: fused {fmt(tf)}   ValueGradient product + scaling {fmt(tv)}   per_dim bilinear_grad {fmt(ts)}   "
                                  f"ValueGradient / fused {mv / mf:6.2f} x   fused / per_dim {mf / ms:5.2f} x",
                                  f"{'':{len(tag)}}  pair kernel + reduction alone {kms / max(cnt, 1):.3f} ms, {n * n / (mf * 1e-3):.3e} pairs / s; "
                                  f"largest |fused - ValueGradient route| / largest |entry|: {diff:.1e}"]
                        print("\n".join(lines[-2:]), flush=True)
                        if not mf < mv:
                            slower.append(f"{tag}: fused {mf:.3f} ms, ValueGradient route {mv:.3f} ms")
                        del G, V, rhs, res
    lines.append("")
    if slower:
        lines += ["Shapes at which the fused pass was NOT faster than the ValueGradient route:"] + ["  " + s for s in slower] + [""]
    else:
        lines += ["The fused pass was faster than the ValueGradient route at every shape above.", ""]

    # the worst err / bound of the GPU test's clouds (tests/test_gpu_input_grad.py, case (a)), dX and dY
    for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import covgram_oracle as o
    import input_grad_ref as ir
    import matrix_cases as mc
    import test_gpu_bilin_grad as tg
    import test_gpu_input_grad as ti
    lines += ["Worst err / bound over rows and dimensions on the GPU test's clouds (N = 257, M = 130, nvec in {1, 3, 17}, dX and dY; the bound of",
              "tests/input_grad_ref.py, the test's criterion is <= 1):"]
    for dt in (np.float32, np.float64):
        for d in ((3,) if quick else (1, 3, 8)):
            row = []
            for name, ko in tg.FAMILIES:
                rng = np.random.default_rng(1000 + d)
                X, Y = mc.iso_cloud(rng, tg.N, tg.M, d, dt, lscale=ko.lengthscale)[:2]
                worst = 0.0
                for nvec in (1, 3, 17):
                    U, A = tg.weights(rng, tg.N, tg.M, nvec, dt)
                    for P, Q, S, B in ((X, Y, U, A), (Y, X, A, U)):
                        ref, bound = ir.reference_and_bound(o, ko, P, Q, S, B, dt)
                        worst = max(worst, float((np.abs(ti.raw(cg, ko, P, Q, S, B) - ref) / bound).max()))
                row.append(f"{name} {worst:.3f}")
            lines.append(f"  {dt.__name__} d = {d}: " + ", ".join(row))
            print(lines[-1], flush=True)
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
