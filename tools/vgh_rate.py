"""Time per value-gradient-Hessian-kernel Gramian MVM (covgram_valgradhess_mvm) beside the Hessian-kernel MVM (covgram_hess_mvm) of the
same shape, written to profiles/vgh_mvm.txt.

Protocol (that of tools/hessian_rate.py): per shape one child process (fresh GPU context, its own time limit; the steps are chained,
the first failure ends the run).  In the child, for each of the two operators in turn: 5 warm-up MVMs, then 7 batches of back-to-back
MVMs (as many as fill ~0.2 s, at least 5) bracketed by one pair of HIP events each; the figure is the MEDIAN batch time per MVM (min
and max beside it).  It is the whole call — pack launch, block kernel, slab reduce —, not the block kernel alone.  The yardstick is
the Hessian MVM timed in the same child: per pair the full block adds about 6 d fma, two jet values and one group reduction to the
Hessian block's 3 d^2 fma, so the flop model predicts a ratio VGH / Hessian of about 1 + 2 / d.

    python tools/vgh_rate.py            all shapes -> profiles/vgh_mvm.txt
    python tools/vgh_rate.py --one EQ 16 128 f64       one shape, one line on stdout (what the children run)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("EQ", 16, 128, "f64"), ("EQ", 16, 4096, "f64"), ("EQ", 8, 16384, "f32"), ("RQ", 16, 4096, "f64")]


def one(name, d, n, prec):
    sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
    import numpy as np
    import torch
    import covgram as cg
    dt = torch.float64 if prec == "f64" else torch.float32
    rng = np.random.default_rng(n + d)
    X = torch.from_numpy(rng.standard_normal((n, d))).to(device="cuda", dtype=dt)
    k = cg.Lengthscale(cg.EQ() if name == "EQ" else cg.RQ(1.5), float(np.sqrt(d)))

    def timed(G, block, key):
        a = torch.from_numpy(rng.standard_normal(n * block)).to(device="cuda", dtype=dt)
        y = torch.empty_like(a)
        for _ in range(5):
            G.mul_(y, a)
        torch.cuda.synchronize()
        assert cg.get_info(key) == 1

        def batch(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                G.mul_(y, a)
            e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / reps
        reps = max(5, int(200.0 / max(batch(3), 1e-3)))
        ms = sorted(batch(reps) for _ in range(7))
        return ms[3], ms[0], ms[-1], reps
    h = timed(cg.gramian(cg.HessianKernel(k), X), d * d, "last_hess_path")
    v = timed(cg.gramian(cg.ValueGradientHessianKernel(k), X), 1 + d + d * d, "last_vgh_path")
    print(f"{name:3s} d={d:3d} n={n:6d} {prec}: VGH {v[0]:9.4f} ms / MVM (min {v[1]:.4f}, max {v[2]:.4f}; {v[3]} per batch)   "
          f"Hessian {h[0]:9.4f} ms (min {h[1]:.4f}, max {h[2]:.4f}; {h[3]} per batch)   "
          f"ratio {v[0] / h[0]:.3f} (model 1 + 2/d = {1 + 2 / d:.3f})", flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        return one(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
    lines = []
    for name, d, n, prec in SHAPES:
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--one", name, str(d), str(n), prec],
                           capture_output=True, text=True)
        if r.returncode != 0:                      # nothing more is started on the GPU after a failure
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(r.returncode)
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    out = os.path.join(ROOT, "profiles", "vgh_mvm.txt")
    doc = __doc__.split("\n\n")[1]
    with open(out, "w") as f:
        f.write("Value-gradient-Hessian-kernel Gramian MVM (covgram_valgradhess_mvm) beside the Hessian-kernel MVM (covgram_hess_mvm), "
                "x = y ~ N(0, I), lengthscale sqrt(d); tools/vgh_rate.py\n\n" + doc + "\n\n")
        f.write("\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
