"""Batched CG on a block of right-hand sides (covgram.mbcg) at GP sizes: time per iteration for p in {8, 32}, n in {16384, 131072}, fp32 and
fp64, EQ d = 3, A = G + 0.1 I — against (a) p iterations of the single-vector cg of the same process (what p right-hand sides cost one at
a time), (b) the same batched iteration with the step written as torch ops, and the bare matrix right-hand-side MVM; the two steps also
over a DIAGONAL operator (its product is one elementwise launch, so the iteration's time is the step's: at n = 131072 the step is below
the run-to-run spread of a 6 to 90 ms Gramian product); then logdet at
n = 16384 with and without a rank-128 pivoted-Cholesky preconditioner.  Writes the table to profiles/mbcg.txt (or --out PATH).

Every time is a host clock around work that ends in a device synchronise, second run of each (the first warms the code objects and the
MVM's caches); tolerances are 0 so that no column stops and an iteration always carries all p columns."""
import argparse, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
import covgram as cg


def timed(fn, repeat=2):
    for _ in range(repeat):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(); el = time.perf_counter() - t0
    return el, out


def torch_mbcg(G, diag, B, iters):
    """The iteration of mbcg with its vector work as torch ops on (p, n) blocks: per-column dots, scalars and masks."""
    Rt = B.t().contiguous(); Xt = torch.zeros_like(Rt); Pt = Rt.clone(); APt = torch.empty_like(Rt)
    rz = (Rt.double() * Rt.double()).sum(1); tol2 = torch.zeros_like(rz); active = rz > tol2
    zero = torch.zeros_like(rz)
    for _ in range(iters):
        G.mul_(APt.t(), Pt.t())
        APt.addcmul_(Pt, diag)
        gamma = (Pt.double() * APt.double()).sum(1)
        alpha = torch.where(active & (rz != 0) & (gamma != 0), rz / gamma, zero)
        a = alpha.to(Rt.dtype)[:, None]
        Xt.addcmul_(Pt, a)
        Rt.addcmul_(APt, -a)
        rr = (Rt.double() * Rt.double()).sum(1)
        beta = torch.where(active & (rz != 0), rr / rz, zero)
        Pt.mul_(beta.to(Rt.dtype)[:, None]).add_(Rt)
        rz = torch.where(active, rr, rz)
        active = active & (rr > tol2)
    return Xt.t()


class DiagOp(cg.LazyOperator):
    """Diagonal(w): a product that costs one elementwise launch (eigenvalues spread over six decades: CG keeps iterating)."""
    def __init__(self, w):
        self.w, self.shape, self.dtype, self.device = w, (w.shape[0], w.shape[0]), w.dtype, w.device

    def mul_(self, y, a, alpha=1.0, beta=0.0):
        return torch.mul(a, self.w[:, None] if a.dim() == 2 else self.w, out=y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mbcg.txt"))
    ap.add_argument("--quick", action="store_true", help="n = 4096 only (a rehearsal of the script)")
    args = ap.parse_args()
    lines = ["mbcg: time per iteration, EQ d = 3, A = G + 0.1 I, MI355X (tools/mbcg_rate.py); us",
             "n dtype p | MVM (p columns) | mbcg iteration | step = mbcg - MVM | torch-op iteration | p x single-vector cg iteration | cg x p / mbcg | "
             "iteration over a diagonal operator: mbcg | torch ops"]
    sizes = (4096,) if args.quick else (16384, 131072)
    for dt in (torch.float32, torch.float64):
        for n in sizes:
            rng = np.random.default_rng(n)
            X = torch.from_numpy(rng.standard_normal((n, 3))).to(dt).cuda()
            G = cg.gramian(cg.EQ(), X)
            d = torch.full((n,), 0.1, dtype=dt, device="cuda")
            A = G + d
            iters = 400 if n <= 16384 else (40 if dt == torch.float32 else 12)     # windows of 0.07 to 1.1 s
            b = torch.from_numpy(rng.standard_normal(n)).to(dt).cuda()
            t1, (_, i1) = timed(lambda: cg.cg(A, b, reltol=0.0, maxiter=iters))
            single = t1 / i1["iterations"] * 1e6
            for p in (8, 32):
                B = torch.from_numpy(rng.standard_normal((n, p))).to(dt).cuda()
                Yt = torch.empty((p, n), dtype=dt, device="cuda")
                Bt = B.t().contiguous()
                tm, _ = timed(lambda: [G.mul_(Yt.t(), Bt.t()) for _ in range(iters)])
                tb, (_, ib) = timed(lambda: cg.mbcg(A, B, reltol=0.0, maxiter=iters, check_every=iters))
                assert ib["iterations"] == iters and ib["column_iterations"] == [iters] * p
                tt, _ = timed(lambda: torch_mbcg(G, d, B, iters))
                mvm, mb, to = (t / iters * 1e6 for t in (tm, tb, tt))
                D = DiagOp(torch.from_numpy(10.0 ** rng.uniform(-3, 3, n)).to(dt).cuda())
                td, (_, idg) = timed(lambda: cg.mbcg(D + d, B, reltol=0.0, maxiter=400, check_every=400))
                assert idg["column_iterations"] == [400] * p
                tdt, _ = timed(lambda: torch_mbcg(D, d, B, 400))
                lines.append(f"{n} {str(dt)[6:]} {p} | {mvm:.1f} | {mb:.1f} | {mb - mvm:.1f} | {to:.1f} | {p * single:.1f} | {p * single / mb:.2f} | "
                             f"{td / 400 * 1e6:.1f} | {tdt / 400 * 1e6:.1f}")
                print(lines[-1], flush=True)
    # logdet at n = 16384
    n = 4096 if args.quick else 16384
    lines += ["", f"logdet(A, probes=16), n = {n}, EQ d = 3, A = G + 0.1 I: seconds, iterations, estimate +- standard error"]
    for dt in (torch.float32, torch.float64):
        rng = np.random.default_rng(n)
        X = torch.from_numpy(rng.standard_normal((n, 3))).to(dt).cuda()
        G = cg.gramian(cg.EQ(), X)
        A = G + torch.full((n,), 0.1, dtype=dt, device="cuda")
        reltol = 1e-6 if dt == torch.float64 else 1e-4
        t0, (e0, i0) = timed(lambda: cg.logdet(A, probes=16, reltol=reltol, maxiter=2000, generator=torch.Generator(device="cuda").manual_seed(1)))
        ts, P = timed(lambda: cg.PivotedCholeskyPreconditioner(G, 0.1, 128))
        t1, (e1, i1) = timed(lambda: cg.logdet(A, probes=16, reltol=reltol, maxiter=2000, precond=P, generator=torch.Generator(device="cuda").manual_seed(1)))
        lines.append(f"{str(dt)[6:]} (reltol {reltol:g}) plain: {t0:.3f} s, {i0['iterations']} iterations, {e0:.2f} +- {i0['stderr']:.2f} | rank-128 preconditioner "
                     f"(set-up {ts:.3f} s): {t1:.3f} s, {i1['iterations']} iterations, {e1:.2f} +- {i1['stderr']:.2f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
