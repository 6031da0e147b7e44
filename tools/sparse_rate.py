"""Time of sparse(G, delta) (covgram_sparse_create) and of its product (covgram_sparse_mvm) beside the dense covgram_mvm of the same Gramian
in the same process, written to profiles/sparse.txt.

Shapes: the reference README's (EQ, d = 32, n = 16384, fp64, delta = 1e-6; there: 7.2 s to build on the CPU, 0.45 ms per sparse mul!) on a
standard normal cloud with the lengthscale chosen so that the kept share is near that README's 0.22 % (the 0.0022 quantile of the pair
distances of a 2048-point sample), and EQ, d = 3, n = 131072, fp64, l = 0.05.

Protocol: ONE process.  Per shape: 3 warm-up calls of everything, then
  * create: 20 back-to-back covgram_sparse_create / covgram_sparse_destroy pairs on device-resident points, host clock around them (the call
    ends in a stream synchronise): the figure is the mean per call; its fill kernel alone from option "time_kernels" (HIP events around the
    kernel, mean of the 20).  The pair goes through cg.sparse(), so the whole-call figure also holds Python's decay_radius, the
    covgram_sparse_info call and the finalizer's covgram_sparse_destroy with its stream synchronise and three hipFree;
  * sparse product and dense product, one right-hand side: 20 back-to-back calls between one pair of HIP events, mean per call; the
    kernels alone from "time_kernels" in a second batch of 20.
The dense MVM of the same process is the comparison that matters; nothing here is a share of peak.

    python tools/sparse_rate.py [--out profiles/sparse.txt]"""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "sparse.txt")
    sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
    import numpy as np
    import torch
    import covgram as cg
    assert torch.cuda.is_available(), "needs an MI355X"
    delta = 1e-6
    lines = [f"sparse(G, {delta:g}) on one MI355X: covgram_sparse_create, covgram_sparse_mvm and the dense covgram_mvm of the same Gramian, one process,",
             f"{REPS} back-to-back calls each after 3 warm-up calls (protocol: tools/sparse_rate.py); times in ms per call.  The whole call of",
             "covgram_sparse_create is timed through cg.sparse(): it includes Python's decay_radius, covgram_sparse_info and the finalizer's",
             "covgram_sparse_destroy (a stream synchronise and three hipFree).", ""]

    def events(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(REPS):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / REPS

    def kernel_only(call):
        cg.set_option("time_kernels", 1)
        cg.kernel_time()
        for _ in range(REPS):
            call()
        ms, cnt = cg.kernel_time()
        cg.set_option("time_kernels", 0)
        return ms / max(cnt, 1), cnt

    for d, n, l_fixed in ((32, 16384, None), (3, 131072, 0.05)):
        rng = np.random.default_rng(16384 + d)
        X = rng.standard_normal((n, d))
        r0 = math.sqrt(-2.0 * math.log(delta))
        if l_fixed is None:
            Xs = X[:2048]
            s = ((Xs[:, None, :] - Xs[None, :, :]) ** 2).sum(-1)[np.triu_indices(2048, 1)]
            l = math.sqrt(float(np.quantile(s, 0.0022))) / r0
        else:
            l = l_fixed
        k = cg.Lengthscale(cg.EQ(), l)
        Xt = torch.from_numpy(X).cuda()
        G = cg.gramian(k, Xt)
        a = torch.from_numpy(rng.standard_normal(n)).cuda()
        y = torch.empty(n, dtype=torch.float64, device="cuda")
        S = cg.sparse(G, delta)
        for _ in range(3):
            cg.sparse(G, delta); S.mul_(y, a); G.mul_(y, a)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            cg.sparse(G, delta)
        torch.cuda.synchronize()
        create_ms = (time.perf_counter() - t0) * 1e3 / REPS
        fill_ms, fill_cnt = kernel_only(lambda: cg.sparse(G, delta))
        sp_ms = events(lambda: S.mul_(y, a))
        sp_k, _ = kernel_only(lambda: S.mul_(y, a))
        de_ms = events(lambda: G.mul_(y, a))
        de_k, _ = kernel_only(lambda: G.mul_(y, a))
        ys, yd = S @ a, G @ a
        diff = float((ys - yd).abs().max())
        lines += [f"EQ, d = {d}, n = {n}, fp64, l = {l:.6g} (decay radius {S.radius:.6g}): nnz = {S.nnz} ({100.0 * S.nnz / (n * n):.4f} % of n^2, {S.nnz / n:.1f} per row)",
                  f"  covgram_sparse_create   whole call {create_ms:9.3f}   fill kernel {fill_ms:9.3f}  ({fill_cnt} timed launches; count, scan and the two synchronisations are the rest)",
                  f"  covgram_sparse_mvm      whole call {sp_ms:9.4f}   kernel {sp_k:9.4f}",
                  f"  covgram_mvm (dense)     whole call {de_ms:9.4f}   dominant kernel {de_k:9.4f}",
                  f"  dense / sparse product time {de_ms / sp_ms:.1f} x;  max |S a - G a| = {diff:.3e} for |a|_1 = {float(a.abs().sum()):.3e} (each dropped entry < {delta:g})", ""]
        print("\n".join(lines[-6:]), flush=True)
        del S, G
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
