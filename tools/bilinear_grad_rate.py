"""Time of the fused hyper-parameter gradient pass (covgram_bilinear_grad) beside what the library needed for the same numbers before it
existed: one central difference per parameter out of its own products, written to profiles/bilinear_grad.txt.

The earlier route, per parameter: two `mul_` with an nvec-column right-hand side on Gramians of the perturbed kernel (built outside the
timed region, in its favour; a per-dimension lengthscale would also need two rescaled point sets) plus the nvec dot products with U and
the difference.  The file reports the fused pass (ALL parameters at once), the two products of ONE parameter, and that figure times
the number of parameters (scale + lengthscale: 2; per_dim: 1 + d).

Protocol: ONE process.  Shapes: EQ and MaternP(2) under a lengthscale, d = 3 and 8 with per_dim on and off, n = m = 16384 and 131072 (two
point sets), nvec = 1 and 17, fp32 and fp64; standard normal points and weights.  Per shape 2 warm-up calls of both, then REPS rounds
that ALTERNATE the two, each call between its own pair of HIP events; medians with (min .. max).  The pair kernel alone comes from option
"time_kernels" in a separate batch.  Last: inv_quad_logdet_gradient beside inv_quad_logdet alone at n = 16384 (fp64, d = 3, 16 probes),
host clock around calls that end in a device synchronise.  Nothing here is a share of peak.

    python tools/bilinear_grad_rate.py [--out profiles/bilinear_grad.txt] [--quick]      (--quick: n = 2^11 only, to rehearse the script)"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "bilinear_grad.txt")
    quick = "--quick" in sys.argv
    sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
    import numpy as np
    import torch
    import covgram as cg
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    f = cg._ffi
    lines = ["Hyper-parameter gradients of sum_t u_t' G a_t on one MI355X: the fused pass covgram_bilinear_grad (every parameter at once) against the",
             "central difference of ONE parameter from two products with an nvec-column right-hand side (+ dot products), one process, alternating",
             "calls, medians of HIP-event times in ms with (min .. max) (protocol: tools/bilinear_grad_rate.py).", ""]
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
            reps = 3 if n > 16384 else 9
            for kname, make in kernels:
                for d in (3, 8):
                    for per_dim in (0, 1):
                        for nvec in (1, 17):
                            rng = np.random.default_rng([n, d, nvec])
                            l = 0.5 * np.sqrt(d)
                            X = torch.from_numpy(rng.standard_normal((n, d))).to(dev, tdt)
                            Y = torch.from_numpy(rng.standard_normal((n, d))).to(dev, tdt)
                            Ut = torch.from_numpy(rng.standard_normal((nvec, n))).to(dev, tdt)      # column-major n x nvec
                            At = torch.from_numpy(rng.standard_normal((nvec, n))).to(dev, tdt)
                            G = cg.gramian(make(l), X, Y)
                            h = 1e-3 * l
                            Gp, Gm = cg.gramian(make(l + h), X, Y), cg.gramian(make(l - h), X, Y)
                            spec = G._spec()
                            nout = 2 + (d if per_dim else 1)
                            out = torch.empty(nout, dtype=torch.float64, device=dev)
                            yp = torch.empty((nvec, n), dtype=tdt, device=dev).t()
                            ym = torch.empty((nvec, n), dtype=tdt, device=dev).t()
                            fd = torch.empty((), dtype=tdt, device=dev)

                            def fused():
                                f.check(lib.covgram_bilinear_grad(G._px.ctx.bind_stream(), f.kref(spec), G._px.handle, G._py.handle, f._P(Ut.data_ptr()), n,
                                                                  f._P(At.data_ptr()), n, nvec, per_dim, C.cast(out.data_ptr(), C.POINTER(C.c_double)), f.DEVICE))

                            def pair():
                                Gp.mul_(yp, At.t()); Gm.mul_(ym, At.t())
                                fd.copy_(((yp - ym) * Ut.t()).sum() / (2 * h))

                            for _ in range(2):
                                fused(); pair()
                            torch.cuda.synchronize()
                            dl = -2.0 / l * float(out[2:].sum())
                            rel = abs(dl - float(fd)) / max(abs(dl), 1e-300)
                            tf, tp = [], []
                            for _ in range(reps):
                                tf.append(timed(fused)); tp.append(timed(pair))
                            cg.set_option("time_kernels", 1); cg.kernel_time()
                            for _ in range(3):
                                fused()
                            kms, cnt = cg.kernel_time()
                            cg.set_option("time_kernels", 0)
                            mf, mp = statistics.median(tf), statistics.median(tp)
                            npar = 1 + (d if per_dim else 1)
                            tag = f"{tname} {kname:10s} n = {n:6d} d = {d} per_dim = {per_dim} nvec = {nvec:2d}"
                            lines += [f"{tag}: fused {fmt(tf)}   two products of one parameter {fmt(tp)}   x {npar} parameters = {npar * mp:9.3f}   "
                                      f"one parameter / fused {mp / mf:6.2f} x",
                                      f"{'':{len(tag)}}  pair kernel + reduction alone {kms / max(cnt, 1):.3f} ms, {n * n / (mf * 1e-3):.3e} pairs / s; "
                                      f"d/dl fused against the central difference: {rel:.1e} relative"]
                            print("\n".join(lines[-2:]), flush=True)
                            if not mf < mp:
                                slower.append(f"{tag}: fused {mf:.3f} ms, two products {mp:.3f} ms")
                            del G, Gp, Gm
    lines.append("")
    if slower:
        lines += ["Shapes at which the fused pass was NOT faster than the two products of ONE parameter:"] + ["  " + s for s in slower] + [""]
    else:
        lines += ["The fused pass was faster than the two products of one parameter at every shape above.", ""]

    # the marginal likelihood's gradient beside its value
    n, d, p = (2048, 3, 16) if quick else (16384, 3, 16)
    rng = np.random.default_rng(n)
    X = torch.from_numpy(rng.standard_normal((n, d))).to(dev, torch.float64)
    b = torch.from_numpy(rng.standard_normal(n)).to(dev, torch.float64)
    Z = torch.from_numpy(2.0 * rng.integers(0, 2, size=(n, p)) - 1.0).to(dev, torch.float64)
    A = cg.gramian(2.0 * cg.Lengthscale(cg.MaternP(2), 0.8), X) + torch.full((n,), 0.1, dtype=torch.float64, device=dev)

    def clock(call):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    tv, tg = [], []
    for it in range(4):
        t1, r1 = clock(lambda: cg.inv_quad_logdet(A, b, probes=Z, reltol=1e-6))
        t2, r2 = clock(lambda: cg.inv_quad_logdet_gradient(A, b, probes=Z, reltol=1e-6))
        if it:
            tv.append(t1); tg.append(t2)
    lines += [f"inv_quad_logdet_gradient beside inv_quad_logdet, n = {n}, d = {d}, fp64, 2.0 Lengthscale(MaternP(2), 0.8) + 0.1 I, {p} fixed probes, reltol 1e-6,",
              f"  {r1[3]['iterations']} iterations, 3 alternating calls after a warm-up, host clock, ms:",
              f"  inv_quad_logdet {fmt(tv)}   inv_quad_logdet_gradient {fmt(tg)}   (the gradient adds {1 + p} fused passes with nvec = 1)",
              f"  grad_inv_quad = {[float(v) for v in r2[3]]}", f"  grad_logdet   = {[float(v) for v in r2[4]]} +- {[float(v) for v in r2[5]['grad_logdet_stderr']]}", ""]
    print("\n".join(lines[-6:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
