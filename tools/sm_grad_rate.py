"""Time of the fused hyper-parameter gradient pass of a SpectralMixture Gramian (covgram_bilinear_grad_sm through
spectral_mixture_gradient: all Q (1 + 2d) derivatives of sum_t u_t' G a_t at once) beside what the library offered for the same numbers
before it: central differences, two covgram_sm_mvm products with nvec columns per parameter.  Written to profiles/sm_grad.txt.

Protocol: ONE process.  Shapes: fp32 and fp64, Q = 4, d = 3 and 8, n = m = 2^15 and 2^17 (one point set on both sides), nvec = 1 and
17, one lengthscale per component and dimension; standard normal points, w = exp(0.5 N), mu = exp(0.7 N) with mu_0 = 0,
l = 0.3 exp(0.5 N) sqrt(d / 3).  The central difference is timed for ONE parameter (the first weight): its two mixtures (w_0 +- h) are
built outside the timed region, a timed call runs the two products and the two dot products with U; the time for all parameters is that
figure times Q (1 + 2d) and is printed as such.  Per shape 2 warm-up calls of both, then REPS rounds that ALTERNATE the two, each
call between its own pair of HIP events; the figures are the medians, with the spread (min .. max) beside them.  The fused kernels
alone come from option "time_kernels" in a separate batch.  No ratio was fixed in advance; nothing here is a share of peak.

    python tools/sm_grad_rate.py [--out profiles/sm_grad.txt] [--quick]      (--quick: n = 2^12 only, to rehearse the script)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "sm_grad.txt")
    quick = "--quick" in sys.argv
    sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
    import numpy as np
    import torch
    import covgram as cg
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    Q = 4
    lines = ["Hyper-parameter gradients of sum_t u_t' G a_t for SpectralMixture Gramians on one MI355X: the fused pass (spectral_mixture_gradient,",
             "all Q (1 + 2d) derivatives at once) against central differences from two covgram_sm_mvm products per parameter, one process,",
             "alternating calls, medians of HIP-event times in ms with (min .. max) (protocol: tools/sm_grad_rate.py).  Q = 4, per-dimension",
             "lengthscales, one point set on both sides.  'all' = the one-parameter figure times the Q (1 + 2d) parameters.", ""]
    slower_one, slower_all = [], []

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def fmt(ts):
        return f"{statistics.median(ts):10.3f} ({min(ts):.3f} .. {max(ts):.3f})"

    sizes = (4096,) if quick else (1 << 15, 1 << 17)
    for tdt, name in ((torch.float32, "fp32"), (torch.float64, "fp64")):
        for n in sizes:
            reps = 3 if n > (1 << 15) else 9
            for d in (3, 8):
                for nvec in (1, 17):
                    rng = np.random.default_rng([n, d, nvec])
                    X = torch.from_numpy(rng.standard_normal((n, d))).to(dev, tdt)
                    w = np.exp(0.5 * rng.standard_normal(Q))
                    mu = np.exp(0.7 * rng.standard_normal((Q, d))); mu[0] = 0.0
                    l = 0.3 * np.exp(0.5 * rng.standard_normal((Q, d))) * np.sqrt(d / 3.0)
                    make = lambda ww: cg.gramian(cg.SM(ww, [m for m in mu], [lq for lq in l]), X)
                    G = make(w)
                    assert isinstance(G, cg.SpectralMixtureGramian)
                    nparam = len(cg.hyperparameters(G.k))
                    assert nparam == Q * (1 + 2 * d)
                    U = torch.from_numpy(rng.standard_normal((nvec, n))).to(dev, tdt).t()        # column-major n x nvec
                    A = torch.from_numpy(rng.standard_normal((nvec, n))).to(dev, tdt).t()
                    h = 1e-2 if tdt == torch.float32 else 1e-5
                    wp, wm = w.copy(), w.copy()
                    wp[0] += h; wm[0] -= h
                    Gp, Gm = make(wp), make(wm)
                    Yb = torch.empty((nvec, n), dtype=tdt, device=dev).t()
                    res = {}

                    def fused():
                        res["fused"] = cg.spectral_mixture_gradient(G, U, A)

                    def central():
                        Gp.mul_(Yb, A)
                        fp = (U * Yb).sum(dtype=torch.float64)
                        Gm.mul_(Yb, A)
                        fm = (U * Yb).sum(dtype=torch.float64)
                        res["central"] = float(fp - fm) / (float(Gp.w[0]) - float(Gm.w[0]))

                    for _ in range(2):
                        fused(); central()
                    torch.cuda.synchronize()
                    g0 = float(res["fused"][1][0])
                    rel = abs(g0 - res["central"]) / max(abs(g0), 1e-300)
                    tf, tc = [], []
                    for _ in range(reps):
                        tf.append(timed(fused)); tc.append(timed(central))
                    cg.set_option("time_kernels", 1); cg.kernel_time()
                    for _ in range(3):
                        fused()
                    kms, cnt = cg.kernel_time()
                    cg.set_option("time_kernels", 0)
                    mf, mc_ = statistics.median(tf), statistics.median(tc)
                    tag = f"{name} n = {n} d = {d} nvec = {nvec:2d}"
                    lines += [f"{tag}: fused, {nparam} parameters {fmt(tf)}   central difference, 1 parameter {fmt(tc)}   all {mc_ * nparam:10.1f}",
                              f"{'':{len(tag)}}  1 parameter / fused {mc_ / mf:6.2f} x   all / fused {mc_ * nparam / mf:7.1f} x   fused kernels alone "
                              f"{kms / max(cnt, 1):.3f} ms, {n * n * Q / (mf * 1e-3):.3e} pair-components / s; |fused - central| / |fused| of dF/dw_0 = {rel:.1e}"]
                    print("\n".join(lines[-2:]), flush=True)
                    if not mf < mc_:
                        slower_one.append(f"{tag}: fused {mf:.3f} ms, two products {mc_:.3f} ms")
                    if not mf < mc_ * nparam:
                        slower_all.append(f"{tag}: fused {mf:.3f} ms, all central differences {mc_ * nparam:.3f} ms")
                    del G, Gp, Gm
    lines.append("")
    if slower_all:
        lines += ["Shapes at which the fused pass was NOT faster than central differences of ALL parameters:"] + ["  " + s for s in slower_all] + [""]
    else:
        lines += ["The fused pass was faster than central differences of all Q (1 + 2d) parameters at every shape above.", ""]
    if slower_one:
        lines += ["Shapes at which the fused pass (all parameters) took longer than the central difference of ONE parameter:"] + ["  " + s for s in slower_one] + [""]
    else:
        lines += ["The fused pass (all parameters) was faster than the central difference of even ONE parameter at every shape above.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
