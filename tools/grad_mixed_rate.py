"""Time per gradient-kernel Gramian MVM of a mixed-trait composite (covgram_grad_mvm_mixed, one fused pass) beside the term-by-term composition the library could already run, written to profiles/grad_mixed.txt.

Protocol (that of tools/hessian_rate.py): per shape one child process (fresh GPU context, its own time limit; the steps are chained,
the first failure ends the run).  In the child: 5 warm-up MVMs, then 7 batches of back-to-back MVMs (as many as fill ~0.2 s, at least
5) bracketed by one pair of HIP events each; the figure is the MEDIAN batch time per MVM (min and max beside it) of the whole call.
"sum" is the reference README's kernel MaternP(2) + Dot()^2 + NN(): the fused pass against LazyMatrixSum of the three gradient
operators of its terms (lane-per-row / panel MVM of MaternP(2) and of Dot()^2, the warped AsinDot operator of NN()) in the same process,
and at d = n = 1024 against the reference's published 3.139 s.  "prod" is EQ() * (Dot()^2 + 1): no other route exists, time and
pairs/s only.  Points ~ N(0, 0.64 * min(1, 3 / d) I), so that x.y and |x - y|^2 keep their size as d grows.

    python tools/grad_mixed_rate.py            all shapes -> profiles/grad_mixed.txt
    python tools/grad_mixed_rate.py --one sum 1024 1024 f64       one shape, one line on stdout (what the children run)"""
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ([(kind, 1024, 1024, prec) for kind in ("sum", "prod") for prec in ("f64", "f32")] +
          [(kind, d, 16384, prec) for kind in ("sum", "prod") for prec in ("f64", "f32") for d in (3, 8, 32, 128)])
REFERENCE_S = 3.139411   # the reference's published mul! time of GradientKernel(MaternP(2) + Dot()^2 + NN()) at d = n = 1024 (its README)


def one(kind, d, n, prec):
    sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
    import numpy as np
    import torch
    import covgram as cg
    dt = torch.float64 if prec == "f64" else torch.float32
    rng = np.random.default_rng(n + d)
    X = torch.from_numpy(0.8 * min(1.0, math.sqrt(3.0 / d)) * rng.standard_normal((n, d))).to(device="cuda", dtype=dt)
    a = torch.from_numpy(rng.standard_normal(n * d)).to(device="cuda", dtype=dt)
    terms = (cg.MaternP(2), cg.Dot() ** 2, cg.NeuralNetwork())
    k = (terms[0] + terms[1] + terms[2]) if kind == "sum" else cg.EQ() * (cg.Dot() ** 2 + 1)
    G = cg.gramian(cg.GradientKernel(k), X)
    assert type(G) is cg.MixedBlockGramian

    def timed(op):
        y = torch.empty_like(a)
        for _ in range(5):
            op.mul_(y, a)
        torch.cuda.synchronize()

        def batch(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                op.mul_(y, a)
            e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / reps
        reps = max(5, int(200.0 / max(batch(3), 1e-3)))
        ms = sorted(batch(reps) for _ in range(7))
        return ms[3], ms[0], ms[-1], reps, y

    med, lo, hi, reps, yf = timed(G)
    path = cg.get_info("last_grad_mixed_path")
    line = (f"{kind:4s} d={d:5d} n={n:6d} {prec}: fused {med:9.4f} ms / MVM (min {lo:.4f}, max {hi:.4f}; {reps} per batch; path bits {path})   "
            f"{n * n / (med * 1e-3) * 1e-9:8.3f} G pairs/s")
    if kind == "sum":
        T = cg.LazyMatrixSum(*[cg.gramian(cg.GradientKernel(t), X) for t in terms])
        tmed, tlo, thi, _, yt = timed(T)
        dev = float((yf - yt).abs().max() / yt.abs().max())
        line += f"   term by term {tmed:9.4f} ms (min {tlo:.4f}, max {thi:.4f}) -> fused / termwise = {med / tmed:.3f}; max |diff| / max |y| = {dev:.1e}"
        if d == 1024 and n == 1024:
            line += f"   [reference, published: {REFERENCE_S:.3f} s -> {REFERENCE_S * 1e3 / med:.0f}x]"
    print(line, flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        return one(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
    lines = []
    for kind, d, n, prec in SHAPES:
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--one", kind, str(d), str(n), prec],
                           capture_output=True, text=True)
        if r.returncode != 0:                      # nothing more is started on the GPU after a failure
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(r.returncode)
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    out = os.path.join(ROOT, "profiles", "grad_mixed.txt")
    doc = "\n\n".join(__doc__.split("\n\n")[1:2])
    with open(out, "w") as f:
        f.write("Gradient-kernel Gramian MVM of mixed-trait composites (covgram_grad_mvm_mixed), x = y; tools/grad_mixed_rate.py\n\n" + doc + "\n\n")
        f.write("\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
