"""Time per Hessian-kernel Gramian MVM (covgram_hess_mvm) and its share of the vector peak, written to profiles/hessian_mvm.txt.

Protocol: per shape one child process (fresh GPU context, its own time limit; the steps are chained, the first failure ends the
run).  In the child: 5 warm-up MVMs, then 7 batches of back-to-back MVMs (as many as fill ~0.2 s, at least 5) bracketed by one pair of
HIP events each; the figure is the MEDIAN batch time per MVM (min and max beside it).  It is the whole call — pack launch, block
kernel, slab reduce —, not the block kernel alone.  flop = 6 d^2 n m (the block algebra's 3 d^2 fma per pair; the lane map of
csrc/hess_mvm.hpp issues about 5 d^2 + the profile per pair), peaks 78.6 (fp64) / 157.3 (fp32) TFLOP/s.

    python tools/hessian_rate.py            all shapes -> profiles/hessian_mvm.txt
    python tools/hessian_rate.py --one EQ 16 128 f64       one shape, one line on stdout (what the children run)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("EQ", 16, 128, "f64"), ("EQ", 16, 4096, "f64"), ("EQ", 8, 16384, "f32"), ("RQ", 16, 4096, "f64")]
PEAK = {"f64": 78.6, "f32": 157.3}
REFERENCE_MS = 76.744   # the reference's published mul! time at EQ, d = 16, n = 128 (its README, 12.81 M allocations)


def one(name, d, n, prec):
    sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
    import numpy as np
    import torch
    import covgram as cg
    dt = torch.float64 if prec == "f64" else torch.float32
    rng = np.random.default_rng(n + d)
    X = torch.from_numpy(rng.standard_normal((n, d))).to(device="cuda", dtype=dt)
    k = cg.Lengthscale(cg.EQ() if name == "EQ" else cg.RQ(1.5), float(np.sqrt(d)))
    G = cg.gramian(cg.HessianKernel(k), X)
    a = torch.from_numpy(rng.standard_normal(n * d * d)).to(device="cuda", dtype=dt)
    y = torch.empty_like(a)
    for _ in range(5):
        G.mul_(y, a)
    torch.cuda.synchronize()
    assert cg.get_info("last_hess_path") == 1

    def batch(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            G.mul_(y, a)
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / reps
    reps = max(5, int(200.0 / max(batch(3), 1e-3)))
    ms = sorted(batch(reps) for _ in range(7))
    med = ms[3]
    tf = 6.0 * d * d * n * n / (med * 1e-3) * 1e-12
    line = (f"{name:3s} d={d:3d} n={n:6d} {prec}: {med:9.4f} ms / MVM (min {ms[0]:.4f}, max {ms[-1]:.4f}; {reps} MVMs per batch)   "
            f"{tf:6.2f} TFLOP/s = {tf / PEAK[prec]:.3f} of the {prec} vector peak")
    if (name, d, n, prec) == SHAPES[0]:
        line += f"   [reference, published: {REFERENCE_MS:.1f} ms -> {REFERENCE_MS / med:.0f}x]"
    print(line, flush=True)


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
    out = os.path.join(ROOT, "profiles", "hessian_mvm.txt")
    doc = __doc__.split("\n\n")[1]
    with open(out, "w") as f:
        f.write("Hessian-kernel Gramian MVM (covgram_hess_mvm), x = y ~ N(0, I), lengthscale sqrt(d); tools/hessian_rate.py\n\n" + doc + "\n\n")
        f.write("\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
