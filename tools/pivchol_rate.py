"""The device pivoted Cholesky (covgram_pivoted_cholesky: one launch per pivot) against the lazy Python loop of
cholesky(G, pivoted=True, max_rank=r) of the same process, and what the rank-r preconditioner built on it does to CG on G + sigma^2 I.

Shapes: n = 2^14 and 2^17, d = 3, MaternP(2), fp32 and fp64, rank 32 and 128.  Both factorisations are timed with events around the
whole call (the best of REPS calls after a warm-up call each); CG: sigma^2 = 1e-2, reltol 1e-6, iteration count and wall time of the
whole solve without and with the preconditioner (its set-up timed separately).  Prints one line per shape; `--out FILE` also writes them."""
import argparse, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
import covgram as cg

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="*", default=[2 ** 14, 2 ** 17])
ap.add_argument("--rank", type=int, nargs="*", default=[32, 128])
ap.add_argument("--dtype", nargs="*", default=["float32", "float64"])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--no-cg", action="store_true")
ap.add_argument("--maxiter", type=int, default=3000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    """(best milliseconds by events around the whole call, the last result); one warm-up call first."""
    fn()
    best, res = float("inf"), None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        res = fn()
        e1.record(); e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best, res


def wall(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


say(f"# tools/pivchol_rate.py on {torch.cuda.get_device_name(0)}: MaternP(2), d = 3, N(0, I) points; times in ms")
for n in args.n:
    for dname in args.dtype:
        dt = getattr(torch, dname)
        rng = np.random.default_rng(n)
        X = torch.from_numpy(rng.standard_normal((n, 3))).to(dt).cuda()
        b = torch.from_numpy(rng.standard_normal(n)).to(dt).cuda()
        G = cg.gramian(cg.MaternP(2), X)
        sig = torch.full((n,), 1e-2, dtype=dt, device="cuda")
        A = G + sig
        plain = None
        for r in args.rank:
            t_dev, F = timed(lambda: cg.pivoted_cholesky(G, r), args.reps)
            t_lazy, Fl = timed(lambda: cg.cholesky(G, pivoted=True, max_rank=r), max(1, args.reps - 1))
            same = bool(torch.equal(F.piv[:F.rank].cpu(), Fl.piv[:Fl.rank].cpu()))
            dL = float((F.L - Fl.L).abs().max()) if same else float("nan")
            say(f"factor n={n} {dname} rank={r}: device {t_dev:.3f}  lazy {t_lazy:.3f}  lazy/device {t_lazy / t_dev:.1f}x  "
                f"(ranks {F.rank}/{Fl.rank}, same pivots {same}, max|dL| {dL:.2e}, max residual diagonal {float(F.residual_diagonal.max()):.3e})")
            if args.no_cg:
                continue
            if plain is None:
                plain = wall(lambda: cg.cg(A, b, reltol=1e-6, maxiter=args.maxiter))
            t_set, P = wall(lambda: cg.PivotedCholeskyPreconditioner(G, 1e-2, r))
            t_pcg, (xp, ip) = wall(lambda: cg.cg(A, b, reltol=1e-6, maxiter=args.maxiter, precond=P))
            t_cg, (x0, i0) = plain
            say(f"cg     n={n} {dname} rank={r}: plain {i0['iterations']} its {t_cg:.1f} (converged {i0['converged']})  "
                f"preconditioned {ip['iterations']} its {t_pcg:.1f} + set-up {t_set:.1f} (converged {ip['converged']})  "
                f"iterations x{ip['iterations'] / max(i0['iterations'], 1):.2f}  time x{(t_pcg + t_set) / t_cg:.2f}")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
