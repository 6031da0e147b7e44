"""Time of the fused input-gradient pass of a SpectralMixture Gramian (covgram_bilinear_input_grad_sm: the n d derivatives of
sum_t u_t' G a_t in the row points, ONE side per call) beside two references.  Written to profiles/sm_input_grad.txt.

  (a) covgram_bilinear_grad_sm on the same shape in the same process: the hyper-parameter pass runs the same pair arithmetic (W, the
      exponents, exp2, W e cos phi and W e sin phi) with more accumulators, Q (1 + 2d) sums instead of d;
  (b) torch autograd through a dense torch expression of F = sum_ij W_ij k(x_i, y_j) (forward and backward, the gradient in X) at
      N_DENSE points a side — the largest power of two at which the n x m x d differences and the per-component n x m intermediates
      autograd keeps fit comfortably in fp64 — compared through pairs per second.

Protocol: ONE process.  Shapes: fp32 and fp64, Q = 4, one lengthscale per component (scalar l) and per component and dimension, d = 3
and 8, n = m = 2^15 and 2^17 (two point sets), nvec = 1 and 17; standard normal points, w = exp(0.5 N), mu = exp(0.7 N) with mu_0 = 0,
l = 0.3 exp(0.5 N) sqrt(d / 3).  Both entries are called through the C ABI on device memory.  Per shape warm-up calls of both, then REPS
rounds that ALTERNATE the two, each call between its own pair of HIP events; the figures are the medians, with the spread (min .. max)
beside them.  The kernels alone come from option "time_kernels" in a separate batch.  No time was fixed in advance; nothing here is a
share of peak.

    python tools/sm_input_grad_rate.py [--out profiles/sm_input_grad.txt] [--quick]      (--quick: n = 2^12 only, to rehearse the script)"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_DENSE = 8192


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "sm_input_grad.txt")
    quick = "--quick" in sys.argv
    sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
    import numpy as np
    import torch
    import covgram as cg
    f = cg._ffi
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    Q = 4
    n_dense = 1024 if quick else N_DENSE
    lines = ["Input gradients of sum_t u_t' G a_t for SpectralMixture Gramians on one MI355X: the fused pass (covgram_bilinear_input_grad_sm, one side:",
             "n d derivatives) against (a) the fused hyper-parameter pass covgram_bilinear_grad_sm on the same shape and (b) torch autograd through a",
             f"dense expression of F at n = m = {n_dense}; one process, alternating calls, medians of HIP-event times in ms with (min .. max)",
             "(protocol: tools/sm_input_grad_rate.py).  Q = 4, two point sets.  'iso': one lengthscale per component; 'ard': one per dimension.", ""]
    not_faster = []

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def fmt(ts):
        return f"{statistics.median(ts):10.3f} ({min(ts):.3f} .. {max(ts):.3f})"

    def problem(n, d, nvec, scalar_l, tdt):
        rng = np.random.default_rng([n, d, nvec, int(scalar_l)])
        X = torch.from_numpy(rng.standard_normal((n, d))).to(dev, tdt)
        Y = torch.from_numpy(rng.standard_normal((n, d))).to(dev, tdt)
        w = np.exp(0.5 * rng.standard_normal(Q))
        mu = np.exp(0.7 * rng.standard_normal((Q, d))); mu[0] = 0.0
        l = 0.3 * np.exp(0.5 * rng.standard_normal(Q if scalar_l else (Q, d))) * np.sqrt(d / 3.0)
        Ut = torch.from_numpy(rng.standard_normal((nvec, n))).to(dev, tdt)            # (nvec, n) row-major == column-major n x nvec
        At = torch.from_numpy(rng.standard_normal((nvec, n))).to(dev, tdt)
        return X, Y, w, mu, l, Ut, At

    sizes = (4096,) if quick else (1 << 15, 1 << 17)
    for tdt, name in ((torch.float32, "fp32"), (torch.float64, "fp64")):
        for n in sizes:
            reps = 3 if n > (1 << 15) else 7
            for d in (3, 8):
                for scalar_l in (True, False):
                    for nvec in (1, 17):
                        X, Y, w, mu, l, Ut, At = problem(n, d, nvec, scalar_l, tdt)
                        G = cg.gramian(cg.SM(w, [m for m in mu], [lq for lq in l]), X, Y)
                        assert isinstance(G, cg.SpectralMixtureGramian) and G.isotropic() == scalar_l
                        dX = torch.empty((n, d), dtype=torch.float64, device=dev)
                        hyp = torch.empty(Q * (1 + 2 * d), dtype=torch.float64, device=dev)
                        lib = f.lib()
                        G._px.ctx.bind_stream()
                        pd = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_double))

                        def inputs():
                            f.check(lib.covgram_bilinear_input_grad_sm(G.handle, G._px.handle, G._py.handle, f._P(Ut.data_ptr()), n, f._P(At.data_ptr()), n,
                                                                       nvec, pd(dX), f.DEVICE))

                        def hypers():
                            f.check(lib.covgram_bilinear_grad_sm(G.handle, G._px.handle, G._py.handle, f._P(Ut.data_ptr()), n, f._P(At.data_ptr()), n, nvec,
                                                                 pd(hyp), f.DEVICE))

                        for _ in range(1 if n > (1 << 15) else 2):
                            inputs(); hypers()
                        torch.cuda.synchronize()
                        ti, th = [], []
                        for _ in range(reps):
                            ti.append(timed(inputs)); th.append(timed(hypers))
                        cg.set_option("time_kernels", 1); cg.kernel_time()
                        for _ in range(2):
                            inputs()
                        kms, cnt = cg.kernel_time()
                        cg.set_option("time_kernels", 0)
                        mi, mh = statistics.median(ti), statistics.median(th)
                        tag = f"{name} n = {n} d = {d} {'iso' if scalar_l else 'ard'} nvec = {nvec:2d}"
                        lines += [f"{tag}: input gradient, one side {fmt(ti)}   (a) hyper-parameter pass {fmt(th)}   (a) / input {mh / mi:5.2f} x   "
                                  f"kernels alone {kms / max(cnt, 1):.3f} ms, {n * n / (mi * 1e-3):.3e} pairs / s"]
                        print(lines[-1], flush=True)
                        if not mi < mh:
                            not_faster.append(f"{tag}: input gradient {mi:.3f} ms, hyper-parameter pass {mh:.3f} ms")
                        del G
    lines += ["", f"(b) torch autograd through the dense expression, forward and backward, n = m = {n_dense}, beside the fused pass at the same shape:"]
    for tdt, name in ((torch.float32, "fp32"), (torch.float64, "fp64")):
        for d in (3, 8):
            for scalar_l in (True, False):
                for nvec in (1, 17):
                    n = n_dense
                    X, Y, w, mu, l, Ut, At = problem(n, d, nvec, scalar_l, tdt)
                    G = cg.gramian(cg.SM(w, [m for m in mu], [lq for lq in l]), X, Y)
                    wt = torch.as_tensor(w).to(dev, tdt); mut = torch.as_tensor(mu).to(dev, tdt)
                    il2 = torch.as_tensor(np.broadcast_to((1.0 / np.asarray(l)).reshape(Q, -1), (Q, d)).copy() ** 2).to(dev, tdt)
                    dX = torch.empty((n, d), dtype=torch.float64, device=dev)
                    res = {}

                    def fused():
                        G._px.ctx.bind_stream()
                        f.check(f.lib().covgram_bilinear_input_grad_sm(G.handle, G._px.handle, G._py.handle, f._P(Ut.data_ptr()), n, f._P(At.data_ptr()), n, nvec,
                                                                       C.cast(dX.data_ptr(), C.POINTER(C.c_double)), f.DEVICE))

                    def dense():
                        x = X.detach().clone().requires_grad_()
                        D = x[:, None, :] - Y[None, :, :]
                        W = Ut.t() @ At
                        F = sum((W * wt[q] * torch.cos(2 * torch.pi * (D * mut[q]).sum(-1)) * torch.exp(-0.5 * (D * D * il2[q]).sum(-1))).sum() for q in range(Q))
                        F.backward()
                        res["dense"] = x.grad

                    fused(); dense()
                    torch.cuda.synchronize()
                    scale = float(dX.abs().max())
                    diff = float((dX - res["dense"].double()).abs().max()) / scale
                    tf, td = [], []
                    for _ in range(3):
                        tf.append(timed(fused)); td.append(timed(dense))
                    mf, md = statistics.median(tf), statistics.median(td)
                    tag = f"{name} n = {n} d = {d} {'iso' if scalar_l else 'ard'} nvec = {nvec:2d}"
                    lines += [f"{tag}: fused {fmt(tf)}   dense autograd {fmt(td)}   dense / fused {md / mf:7.1f} x   "
                              f"max |fused - dense| / max |fused| = {diff:.1e}"]
                    print(lines[-1], flush=True)
                    if not mf < md:
                        not_faster.append(f"{tag}: fused {mf:.3f} ms, dense autograd {md:.3f} ms")
                    del G, res
                    torch.cuda.empty_cache()
    lines.append("")
    if not_faster:
        lines += ["Shapes at which the input-gradient pass was NOT faster than a reference:"] + ["  " + s for s in not_faster] + [""]
    else:
        lines += ["The input-gradient pass was faster than both references at every shape above.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
