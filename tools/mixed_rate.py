"""Time per SCALAR Gramian MVM of a mixed-trait composite (covgram_mvm_mixed) on its routes, beside what the library could run before, written to profiles/mixed.txt.

Protocol (that of tools/grad_mixed_rate.py, measuring-on-mi355x): per (n, d, element type) one child process (fresh GPU context, its own
time limit; the first failure ends the run).  In the child, per kernel, number of right-hand sides and route: 2 warm-up MVMs, one timed
MVM to size the batches, then 5 batches (3 when one MVM takes more than 0.3 s) of back-to-back MVMs (as many as fill ~0.15 s, 1 to 50)
bracketed by one pair of HIP events each; the figure is the MEDIAN batch time per whole call in ms.  x = y, points
~ N(0, 0.64 * min(1, 3 / d) I).  Kernels: "prod" EQ() * (Dot()^2 + 1), "sum2" EQ() + Dot(), "sum3" MaternP(2) + Dot()^2 + NN().  Routes:
  default   covgram_mvm_mixed as it routes by itself (path bits of last_mixed_path beside it)
  fused     option mixed_fuse = 1: every term in the fused kernel
  vg-rows   the value rows of MixedBlockGramian(ValueGradientKernel(k)) on value-only weights: the only route to this product before
            (skipped, "-", where its block vectors exceed 1 GiB or one MVM exceeds the child's remaining time)
  terms     for the two Sums, a hand-built LazyMatrixSum of the terms' own Gramians: what a user could do before
  eq        the plain dense EQ() product of the same process, for scale

    python tools/mixed_rate.py                      all shapes -> profiles/mixed.txt
    python tools/mixed_rate.py --n 16384 [--d 3]    only that n (and d); the file says which shapes ran, several runs append
    python tools/mixed_rate.py --one 16384 3 f32    one child, its lines on stdout"""
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS, DS, PRECS, NRHS = (16384, 131072), (3, 8, 32, 128), ("f32", "f64"), (1, 8)
CHILD_LIMIT = 280


def one(n, d, prec):
    sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
    import numpy as np
    import torch
    import covgram as cg
    t_start = time.time()
    dt = torch.float64 if prec == "f64" else torch.float32
    rng = np.random.default_rng(n + d)
    X = torch.from_numpy(0.8 * min(1.0, math.sqrt(3.0 / d)) * rng.standard_normal((n, d))).to(device="cuda", dtype=dt)
    kernels = {"prod": (cg.EQ() * (cg.Dot() ** 2 + 1), None), "sum2": (cg.EQ() + cg.Dot(), (cg.EQ(), cg.Dot())),
               "sum3": (cg.MaternP(2) + cg.Dot() ** 2 + cg.NeuralNetwork(), (cg.MaternP(2), cg.Dot() ** 2, cg.NeuralNetwork()))}

    def timed(mul):
        for _ in range(2):
            mul()
        torch.cuda.synchronize()

        def batch(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                mul()
            e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / reps
        t1 = batch(1)
        reps = max(1, min(50, int(150.0 / max(t1, 1e-3))))
        ms = sorted(batch(reps) for _ in range(5 if t1 < 300.0 else 3))
        return ms[len(ms) // 2]

    Geq = cg.gramian(cg.EQ(), X)
    for nrhs in NRHS:
        shape = (n,) if nrhs == 1 else (n, nrhs)
        a = torch.from_numpy(rng.standard_normal(shape)).to(device="cuda", dtype=dt)
        y = torch.empty_like(a)
        t_eq = timed(lambda: Geq.mul_(y, a))
        for kind, (k, terms) in kernels.items():
            G = cg.gramian(k, X)
            assert type(G) is cg.MixedGramian
            cg.set_option("mixed_fuse", 0)
            t_def = timed(lambda: G.mul_(y, a))
            path = cg.get_info("last_mixed_path")
            y_def = y.clone()
            cg.set_option("mixed_fuse", 1)
            t_fus = timed(lambda: G.mul_(y, a))
            dev = float((y - y_def).abs().max() / y_def.abs().max())
            cg.set_option("mixed_fuse", 0)
            t_terms = "-"
            if terms is not None:
                T = cg.LazyMatrixSum(*[cg.gramian(t, X) for t in terms])
                t_terms = f"{timed(lambda: T.mul_(y, a)):10.4f}"
            t_vg = "-"
            B = d + 1
            if n * B * nrhs * a.element_size() <= (1 << 30) and time.time() - t_start < 0.5 * CHILD_LIMIT:
                V = cg.gramian(cg.ValueGradientKernel(k), X)
                assert type(V) is cg.MixedBlockGramian
                av = torch.zeros((n * B,) + tuple(shape[1:]), dtype=dt, device="cuda")
                av[::B] = a
                yv = torch.empty_like(av)
                t_vg = f"{timed(lambda: V.mul_(yv, av)):10.4f}"
                del V, av, yv
            print(f"{kind:4s} n={n:6d} d={d:3d} {prec} nrhs={nrhs}: default {t_def:10.4f} (path {path:2d})  fused {t_fus:10.4f}  vg-rows {t_vg:>10s}  "
                  f"terms {t_terms:>10s}  eq {t_eq:10.4f} ms   default {n * n * nrhs / (t_def * 1e-3) * 1e-9:8.2f} G pair-columns/s; "
                  f"max |fused - default| / max |y| = {dev:.1e}", flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        return one(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
    ns = [int(sys.argv[sys.argv.index("--n") + 1])] if "--n" in sys.argv else list(NS)
    ds = [int(sys.argv[sys.argv.index("--d") + 1])] if "--d" in sys.argv else list(DS)
    lines = []
    for n in ns:
        for d in ds:
            for prec in PRECS:
                r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--one", str(n), str(d), prec],
                                   capture_output=True, text=True)
                if r.returncode != 0:              # nothing more is started on the GPU after a failure
                    sys.stderr.write(r.stdout + r.stderr)
                    sys.exit(r.returncode)
                lines += [ln for ln in r.stdout.splitlines() if " nrhs=" in ln]
                print("\n".join(r.stdout.splitlines()), flush=True)
    out = os.path.join(ROOT, "profiles", "mixed.txt")
    doc = __doc__.split("\n\n")[1]
    partial = "--n" in sys.argv and os.path.exists(out)     # a restricted run adds its shapes to the file
    with open(out, "a" if partial else "w") as f:
        if not partial:
            f.write("Scalar Gramian MVM of mixed-trait composites (covgram_mvm_mixed), x = y, whole calls in ms; tools/mixed_rate.py\n\n" + doc + "\n")
        f.write(f"\nShapes of this run: n in {ns}, d in {ds}, {list(PRECS)}, nrhs in {list(NRHS)}.\n\n")
        f.write("\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
