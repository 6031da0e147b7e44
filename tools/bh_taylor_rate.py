"""Time and error of the Taylor product of BarnesHutFactorization (covgram_bh_taylor_mvm, about the centres of mass and about the ball
centres) beside the split product (covgram_bh_mvm) of the same process, written whole to profiles/bh_taylor.txt.

Shapes: those of profiles/barneshut.txt — Cauchy and EQ, d in {2, 3}, n in {2^14, 2^17, 2^20}, theta in {1/8, 1/4, 1/2}, fp32, leafsize 16,
N(0, I) clouds, randn weights (the same seeds, so the same points).  For n <= 2^17 the norm-wise relative error of each product against
the dense product is recorded.  The split product's time is set beside the one recorded in profiles/barneshut.txt (read before this tool
writes anything), to show that the existing kernel was not disturbed.  Then: the time per MINRES iteration at n = 2^17 (solve.minres on
product="taylor", use_com=False, 20 iterations between one pair of events, check_every = 20), and the asymmetry |T - T'|_F / |T|_F of the
ball-centre operator on the pin of the tests (Cauchy, n = 1024, d = 2, theta = 1/8, fp64).

Protocol (as tools/barneshut_rate.py): ONE process; per shape 2 warm-up calls of everything, then REPS back-to-back calls between one
pair of HIP events, mean per call (a product = moments kernels + walk).  REPS = 10 (3 at n = 2^20).

    python tools/bh_taylor_rate.py [--out profiles/bh_taylor.txt] [--max-log2n 20]"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def recorded_split_times(path):
    """{(kernel, d, log2n, theta): ms} of the tree product in profiles/barneshut.txt"""
    out, head = {}, None
    if not os.path.exists(path):
        return out
    for line in open(path):
        m = re.match(r"(\w+), d = (\d+), n = 2\^(\d+):", line)
        if m:
            head = (m.group(1), int(m.group(2)), int(m.group(3)))
        m = re.match(r"\s+theta = ([0-9.]+)\s+tree product\s+([0-9.]+)", line)
        if m and head:
            out[head + (float(m.group(1)),)] = float(m.group(2))
    return out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "bh_taylor.txt")
    max_log2n = int(sys.argv[sys.argv.index("--max-log2n") + 1]) if "--max-log2n" in sys.argv else 20
    sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
    import numpy as np
    import torch
    import covgram as cg
    assert torch.cuda.is_available(), "needs an MI355X"
    before = recorded_split_times(os.path.join(ROOT, "profiles", "barneshut.txt"))
    lines = ["taylor! on one MI355X, fp32, leafsize 16, N(0, I), randn weights: covgram_bh_taylor_mvm about the centres of mass (com) and about the ball",
             "centres (ball) beside the split product covgram_bh_mvm of the same process; back-to-back calls after 2 warm-up calls (protocol:",
             "tools/bh_taylor_rate.py); times in ms per product (moments + walk).  'recorded' = the split product in profiles/barneshut.txt.",
             "rel err = |F w - G w| / |G w| against the dense product (n <= 2^17).", ""]

    def events(call, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    sizes = [q for q in (14, 17, 20) if q <= max_log2n]
    ratios = []
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
                F = cg.BarnesHutFactorization(G)
                yd = (G @ a).double() if log2n <= 17 else None
                lines.append(f"{kname}, d = {d}, n = 2^{log2n}: {F.nnodes} nodes")
                for theta in (0.125, 0.25, 0.5):
                    calls = {"split": lambda: F.mul_(y, a, theta=theta), "com": lambda: F.taylor_(y, a, theta=theta, use_com=True),
                             "ball": lambda: F.taylor_(y, a, theta=theta, use_com=False)}
                    ms, err = {}, {}
                    for key, call in calls.items():
                        call(); call()
                        ms[key] = events(call, reps)
                        if yd is not None:
                            call()
                            err[key] = float(torch.linalg.vector_norm(y.double() - yd) / torch.linalg.vector_norm(yd))
                    rec = before.get((kname, d, log2n, theta))
                    ratios.append((ms["split"] / ms["com"], kname, d, log2n, theta))
                    text = (f"  theta = {theta:<5}  split {ms['split']:9.4f}" + (f" (recorded {rec:9.4f}, now / recorded {ms['split'] / rec:5.2f})" if rec else "")
                            + f"   taylor com {ms['com']:9.4f}  ball {ms['ball']:9.4f}   split / taylor com {ms['split'] / ms['com']:5.2f} x")
                    if err:
                        text += f"   rel err split {err['split']:.2e}  com {err['com']:.2e}  ball {err['ball']:.2e}"
                    lines.append(text)
                lines.append("")
                print("\n".join(lines[-5:]), flush=True)
                flush()
                del F, G
    if ratios:
        lo, hi = min(ratios), max(ratios)
        lines.append(f"split / taylor (com) over all shapes: {lo[0]:.2f} x ({lo[1]}, d = {lo[2]}, n = 2^{lo[3]}, theta = {lo[4]}) to "
                     f"{hi[0]:.2f} x ({hi[1]}, d = {hi[2]}, n = 2^{hi[3]}, theta = {hi[4]}).")
        lines.append("")
    if 17 in sizes:
        n, iters = 1 << 17, 20
        rng = np.random.default_rng(17 + 2)
        Xt = torch.from_numpy(rng.standard_normal((n, 2)).astype(np.float32)).cuda()
        b = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
        for theta in (0.25, 0.5):
            F = cg.BarnesHutFactorization(cg.Cauchy(), Xt, D=1e-2, theta=theta, product="taylor", use_com=False)
            y = torch.empty_like(b)
            solve = lambda: cg.minres(F, b, reltol=0.0, maxiter=iters, check_every=iters)
            solve()
            it_ms = events(solve, 3) / iters
            mv_ms = events(lambda: F.mul_(y, b), 10)
            lines.append(f"MINRES, Cauchy + 1e-2 I, d = 2, n = 2^17, theta = {theta}, ball centres: {it_ms:.4f} ms per iteration ({iters} iterations between the events, "
                         f"set-up included), of which the product {mv_ms:.4f}")
        lines.append("")
    # asymmetry on the tests' pin
    rng = np.random.default_rng(20260)
    X = torch.from_numpy(rng.standard_normal((1024, 2))).cuda()
    F = cg.BarnesHutFactorization(cg.Cauchy(), X, theta=0.125, leafsize=16)
    eye = torch.eye(1024, dtype=torch.float64, device="cuda")
    # (about the ball centres only: there the product is a linear map and T = its matrix; about the centres of mass a unit vector's
    #  centre of mass is its own point, so the "columns" T e_j would be exact and say nothing about the operator on other weights)
    T = F.taylor(eye, use_com=False)
    lines.append("asymmetry |T - T'|_F / |T|_F of the Taylor product about the ball centres on the pin (Cauchy, n = 1024, d = 2, theta = 1/8, fp64): "
                 f"{float(torch.linalg.matrix_norm(T - T.T) / torch.linalg.matrix_norm(T)):.2e}")
    left_out = [q for q in (14, 17, 20) if q > max_log2n]
    if left_out:
        lines.append("Not run (--max-log2n " + str(max_log2n) + "): n = " + ", ".join(f"2^{q}" for q in left_out) + ".")
    flush()


if __name__ == "__main__":
    main()
