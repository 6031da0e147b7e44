"""Time of the fused hyper-parameter gradient pass of a mixed-trait composite (covgram_bilinear_grad_mixed through
mixed_bilinear_gradient: every derivative of sum_t u_t' G a_t at once) beside the route the library offered for the same numbers before
it: central differences, two gramian(k, x) @ A products (covgram_mvm_mixed, default partition) with nvec columns per parameter.
Written to profiles/mixed_grad.txt.

Protocol: ONE process.  Kernels: 1.5 Lengthscale(EQ, 0.7) + 0.5 Dot (3 parameters) and Lengthscale(EQ, 0.8) * (Dot^2 + 1) (2 parameters);
fp32 and fp64, d = 3 and 8, n = m = 2^14 and 2^17 (one point set on both sides), nvec = 1 and 17; points N(0, 0.75^2 / d).  The
central difference is timed for ONE parameter (the first lengthscale): its two Gramians (l +- h) are built outside the timed region, a
timed call runs the two products and the two dot products with U; the time for all parameters is that figure times the parameter
count and is printed as such.  Per shape WARM warm-up calls of both, then REPS rounds that ALTERNATE the two, each call between its
own pair of HIP events; the figures are the medians, with the spread (min .. max) beside them.  The fused kernels alone come from
option "time_kernels" in a separate batch.  No ratio was fixed in advance; nothing here is a share of peak.

    python tools/mixed_grad_rate.py [--out profiles/mixed_grad.txt] [--dtypes fp32,fp64] [--append] [--quick]
    (--quick: n = 2^12 only, to rehearse the script; --append: add the chosen dtypes' lines to an existing file)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "mixed_grad.txt")
    dtypes = sys.argv[sys.argv.index("--dtypes") + 1].split(",") if "--dtypes" in sys.argv else ["fp32", "fp64"]
    quick, append = "--quick" in sys.argv, "--append" in sys.argv
    sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
    import numpy as np
    import torch
    import covgram as cg
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    head = ["Hyper-parameter gradients of sum_t u_t' G a_t for mixed-trait composites on one MI355X: the fused pass (mixed_bilinear_gradient, every",
            "derivative at once) against central differences from two gramian(k, x) @ A products per parameter (default partition), one process,",
            "alternating calls, medians of HIP-event times in ms with (min .. max) (protocol: tools/mixed_grad_rate.py).  One point set on both",
            "sides.  'all' = the one-parameter figure times the number of parameters.", ""]
    lines = []
    slower_one, slower_all = [], []
    kernels = (("1.5 ls(EQ, 0.7) + 0.5 Dot", lambda l: 1.5 * cg.Lengthscale(cg.EQ(), l) + 0.5 * cg.Dot(), 0.7),
               ("ls(EQ, 0.8) * (Dot^2 + 1)", lambda l: cg.Lengthscale(cg.EQ(), l) * (cg.Dot() ** 2 + 1), 0.8))

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def fmt(ts):
        return f"{statistics.median(ts):10.3f} ({min(ts):.3f} .. {max(ts):.3f})"

    sizes = (4096,) if quick else (1 << 14, 1 << 17)
    for name in dtypes:
        tdt = {"fp32": torch.float32, "fp64": torch.float64}[name]
        for kname, make, l0 in kernels:
            for n in sizes:
                warm, reps = (1, 3) if n > (1 << 14) else (2, 9)
                for d in (3, 8):
                    for nvec in (1, 17):
                        rng = np.random.default_rng([n, d, nvec])
                        X = torch.from_numpy(0.75 / np.sqrt(d) * rng.standard_normal((n, d))).to(dev, tdt)
                        G = cg.gramian(make(l0), X)
                        assert isinstance(G, cg.MixedGramian)
                        nparam = len(cg.hyperparameters(G.k))
                        li = [nm for _, nm, _ in cg.hyperparameters(G.k)].index("l")
                        U = torch.from_numpy(rng.standard_normal((nvec, n))).to(dev, tdt).t()        # column-major n x nvec
                        A = torch.from_numpy(rng.standard_normal((nvec, n))).to(dev, tdt).t()
                        h = 1e-2 if tdt == torch.float32 else 1e-5
                        Gp, Gm = cg.gramian(make(l0 + h), X), cg.gramian(make(l0 - h), X)
                        Yb = torch.empty((nvec, n), dtype=tdt, device=dev).t()
                        res = {}

                        def fused():
                            res["fused"] = cg.mixed_bilinear_gradient(G, U, A)

                        def central():
                            Gp.mul_(Yb, A)
                            fp = (U * Yb).sum(dtype=torch.float64)
                            Gm.mul_(Yb, A)
                            fm = (U * Yb).sum(dtype=torch.float64)
                            res["central"] = float(fp - fm) / (2 * h)

                        for _ in range(warm):
                            fused(); central()
                        torch.cuda.synchronize()
                        g0 = float(res["fused"][1][li])
                        rel = abs(g0 - res["central"]) / max(abs(g0), 1e-300)
                        tf, tc = [], []
                        for _ in range(reps):
                            tf.append(timed(fused)); tc.append(timed(central))
                        cg.set_option("time_kernels", 1); cg.kernel_time()
                        fused()
                        kms, cnt = cg.kernel_time()
                        cg.set_option("time_kernels", 0)
                        mf, mc_ = statistics.median(tf), statistics.median(tc)
                        tag = f"{name} {kname} n = {n} d = {d} nvec = {nvec:2d}"
                        lines += [f"{tag}: fused, {nparam} parameters {fmt(tf)}   central difference, 1 parameter {fmt(tc)}   all {mc_ * nparam:10.1f}",
                                  f"{'':{len(tag)}}  1 parameter / fused {mc_ / mf:6.2f} x   all / fused {mc_ * nparam / mf:7.2f} x   fused kernels alone "
                                  f"{kms / max(cnt, 1):.3f} ms, {n * n / (mf * 1e-3):.3e} pairs / s; |fused - central| / |fused| of dF/dl = {rel:.1e}"]
                        print("\n".join(lines[-2:]), flush=True)
                        if not mf < mc_:
                            slower_one.append(f"{tag}: fused {mf:.3f} ms, two products {mc_:.3f} ms")
                        if not mf < mc_ * nparam:
                            slower_all.append(f"{tag}: fused {mf:.3f} ms, all central differences {mc_ * nparam:.3f} ms")
                        del G, Gp, Gm
    lines.append("")
    which = " and ".join(dtypes)
    if slower_all:
        lines += [f"{which}: shapes at which the fused pass was NOT faster than central differences of ALL parameters:"] + ["  " + s for s in slower_all] + [""]
    else:
        lines += [f"{which}: the fused pass was faster than central differences of all parameters at every shape above.", ""]
    if slower_one:
        lines += [f"{which}: shapes at which the fused pass (all parameters) was NOT faster than the central difference of ONE parameter:"] + ["  " + s for s in slower_one] + [""]
    else:
        lines += [f"{which}: the fused pass (all parameters) was faster than the central difference of even ONE parameter at every shape above.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a" if append else "w") as fh:
        fh.write("\n".join(([] if append else head) + lines))


if __name__ == "__main__":
    main()
