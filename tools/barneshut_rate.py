"""Time of BarnesHutFactorization (covgram_bh_create) and of its product (covgram_bh_mvm, split on) beside the dense covgram_mvm of
gramian(k, x) in the same process, written to profiles/barneshut.txt.

Shapes: Cauchy and EQ, d in {2, 3}, n in {2^14, 2^17, 2^20}, theta in {1/8, 1/4, 1/2}, fp32, leafsize 16, N(0, I) clouds, randn weights.
For n <= 2^17 the norm-wise relative error of the tree product against the dense product is recorded too.

Protocol: ONE process.  Per shape 2 warm-up calls of everything, then
  * create: REPS back-to-back constructions on device-resident points, host clock around them (the call ends in a stream synchronise):
    mean per call, through the Python class (it includes covgram_bh_info and the finalizer's covgram_bh_destroy);
  * tree product per theta (the per-product override on ONE handle) and dense product: REPS back-to-back calls between one pair of HIP
    events, mean per call (the tree product = moments kernels + walk); the walk kernel alone from option "time_kernels".
REPS = 10 (3 at n = 2^20, where one dense product takes tens of milliseconds).  The dense MVM of the same process is the comparison
that matters; nothing here is a share of peak.  The closing block of the file is written by this tool too: per (kernel, d, theta) the
first measured n at which the tree product beats the dense one, or that none does, and the sizes that --max-log2n left out.

    python tools/barneshut_rate.py [--out profiles/barneshut.txt] [--max-log2n 20]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "barneshut.txt")
    max_log2n = int(sys.argv[sys.argv.index("--max-log2n") + 1]) if "--max-log2n" in sys.argv else 20
    sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
    import numpy as np
    import torch
    import covgram as cg
    assert torch.cuda.is_available(), "needs an MI355X"
    lines = ["BarnesHutFactorization on one MI355X, fp32, leafsize 16, N(0, I), randn weights, split product: covgram_bh_create, covgram_bh_mvm and the dense",
             "covgram_mvm of gramian(k, x), one process, back-to-back calls after 2 warm-up calls (protocol: tools/barneshut_rate.py); times in ms per call.",
             "rel err = |F w - G w| / |G w| (n <= 2^17).", ""]

    def events(call, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def kernel_only(call, reps):
        cg.set_option("time_kernels", 1)
        cg.kernel_time()
        for _ in range(reps):
            call()
        ms, cnt = cg.kernel_time()
        cg.set_option("time_kernels", 0)
        return ms / max(cnt, 1)

    sizes = [log2n for log2n in (14, 17, 20) if log2n <= max_log2n]
    first_win = {}                      # (kernel, d, theta) -> (log2n, dense / tree, rel err text) of the first n at which the tree wins
    for kname, k in (("Cauchy", cg.Cauchy()), ("EQ", cg.EQ())):
        for d in (2, 3):
            for log2n in sizes:
                n = 1 << log2n
                reps = 3 if log2n >= 20 else 10
                rng = np.random.default_rng(log2n + d)
                Xt = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda()
                a = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
                y = torch.empty(n, dtype=torch.float32, device="cuda")
                G = cg.gramian(k, Xt)
                for _ in range(2):
                    F = cg.BarnesHutFactorization(G); F.mul_(y, a); G.mul_(y, a)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    cg.BarnesHutFactorization(G)
                torch.cuda.synchronize()
                create_ms = (time.perf_counter() - t0) * 1e3 / reps
                de_ms = events(lambda: G.mul_(y, a), reps)
                yd = (G @ a).double() if log2n <= 17 else None
                lines.append(f"{kname}, d = {d}, n = 2^{log2n}: {F.nnodes} nodes; create {create_ms:.3f}; dense product {de_ms:.4f}")
                for theta in (0.125, 0.25, 0.5):
                    bh_ms = events(lambda: F.mul_(y, a, theta=theta), reps)
                    walk_ms = kernel_only(lambda: F.mul_(y, a, theta=theta), reps)
                    err = ""
                    if yd is not None:
                        yb = torch.empty_like(y); F.mul_(yb, a, theta=theta)
                        err = f"   rel err {float(torch.linalg.vector_norm(yb.double() - yd) / torch.linalg.vector_norm(yd)):.2e}"
                    if de_ms > bh_ms:
                        first_win.setdefault((kname, d, theta), (log2n, de_ms / bh_ms, err.strip()))
                    lines.append(f"  theta = {theta:<5}  tree product {bh_ms:9.4f}  (walk kernel {walk_ms:9.4f})   dense / tree {de_ms / bh_ms:6.2f} x{err}")
                lines.append("")
                print("\n".join(lines[-5:]), flush=True)
                del F, G
    lines.append("First measured n at which the tree product is faster than the dense product of the same process (n in "
                 + ", ".join(f"2^{q}" for q in sizes) + "):")
    for kname in ("Cauchy", "EQ"):
        for d in (2, 3):
            for theta in (0.125, 0.25, 0.5):
                win = first_win.get((kname, d, theta))
                lines.append(f"  {kname}, d = {d}, theta = {theta:<5}  " + (f"n = 2^{win[0]} ({win[1]:.2f} x{', ' + win[2] if win[2] else ''})" if win
                                                                     else f"none up to n = 2^{sizes[-1]}"))
    left_out = [q for q in (14, 17, 20) if q > max_log2n]
    if left_out:
        lines.append("Not run (--max-log2n " + str(max_log2n) + "): n = " + ", ".join(f"2^{q}" for q in left_out) + ".")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
