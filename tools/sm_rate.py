"""Time of the fused SpectralMixture product (covgram_sm_mvm) beside the host composition of the same product from this library's existing
pieces, and of Matrix(G) (covgram_sm_matrix) beside covgram_matrix of EQ, written to profiles/sm.txt.

The host composition, for G = sum_q w_q Cosine(mu_q) ARD(EQ(), l_q):
    G a = sum_q w_q [ cos u_q .* (E_q (cos v_q .* a)) + sin u_q .* (E_q (sin v_q .* a)) ],   u_q = 2 pi X mu_q, v_q = 2 pi Y mu_q,
with E_q = gramian(EQ(), X ./ l_q, Y ./ l_q): per product Q dense EQ MVMs with 2 right-hand sides on rescaled points plus elementwise
vector work.  The Q rescaled point sets, their Gramian objects and the 4 Q cos / sin vectors are built ONCE outside the timed region (in
favour of the composition); a timed call forms the 2 Q weighted right-hand sides, runs the Q products and combines them.

Protocol: ONE process.  Shapes: fp32 and fp64, n = m = 2^15 and 2^17 (one point set on both sides), d = 1 and 3, Q = 4, one lengthscale
per component ("scalar") and one per component and dimension ("ard"); standard normal points, w = exp(0.5 N), mu = exp(0.7 N) with
mu_0 = 0, l = 0.3 exp(0.5 N).  Per shape 2 warm-up calls of both, then REPS rounds that ALTERNATE the two, each call between its own
pair of HIP events; the figures are the medians, with the spread (min .. max) beside them.  The fused kernel alone comes from option
"time_kernels" in a separate batch.  Matrix(G): n = m = 16384, d = 3, the fused kernel against covgram_matrix of EQ (one profile), both
into a preallocated buffer, pairs per second.  Nothing here is a share of peak.

    python tools/sm_rate.py [--out profiles/sm.txt] [--quick]      (--quick: n = 2^12 only, to rehearse the script)"""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIX = [
    "Per pair and component the fused kernel issues (fp32, from the gfx950 ISA of sm_pair_kernel, DESIGN.md \"SpectralMixture\"):",
    "  shared by the pair's components: d subtractions and d multiplications (scalar lengthscales: d fused multiply-adds instead of the",
    "  multiplications) and, for a product, one fused multiply-add per right-hand side; three LDS reads (coordinates, 8 phase factors);",
    "  per component: d fused multiply-adds (scalar lengthscales: one multiplication), one v_exp_f32, one multiplication and two fused",
    "  multiply-adds.  fp64 replaces v_exp_f32 by the 14-instruction table form of exp2 (csrc/profiles.hpp: exp2_neg_tab).",
]


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "sm.txt")
    quick = "--quick" in sys.argv
    sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
    import numpy as np
    import torch
    import covgram as cg
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    Q = 4
    lines = ["SpectralMixture Gramians on one MI355X: the fused product covgram_sm_mvm against the host composition (Q dense EQ products with 2",
             "right-hand sides on rescaled points + elementwise cos / sin work) from this library's own products, one process, alternating calls,",
             "medians of HIP-event times in ms per product with (min .. max) (protocol: tools/sm_rate.py).  Q = 4, one point set on both sides.", ""]
    slower = []

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def fmt(ts):
        return f"{statistics.median(ts):10.3f} ({min(ts):.3f} .. {max(ts):.3f})"

    sizes = (4096,) if quick else (1 << 15, 1 << 17)
    for tdt, name in ((torch.float32, "fp32"), (torch.float64, "fp64")):
        for n in sizes:
            reps = 5 if n > (1 << 15) else 15
            for d in (1, 3):
                for scalar in (True, False):
                    rng = np.random.default_rng([n, d, int(scalar)])
                    X = torch.from_numpy(rng.standard_normal((n, d))).to(dev, tdt)
                    w = np.exp(0.5 * rng.standard_normal(Q))
                    mu = np.exp(0.7 * rng.standard_normal((Q, d))); mu[0] = 0.0
                    l = 0.3 * np.exp(0.5 * rng.standard_normal(Q if scalar else (Q, d)))
                    k = cg.SM(w, [m for m in mu], [lq for lq in l])
                    G = cg.gramian(k, X)
                    assert isinstance(G, cg.SpectralMixtureGramian) and G.isotropic() == (scalar or d == 1)
                    a = torch.from_numpy(rng.standard_normal(n)).to(dev, tdt)
                    y = torch.empty(n, dtype=tdt, device=dev)
                    # the composition's resident pieces
                    inv_l = torch.from_numpy(G.inv_l).to(dev, tdt)
                    mut = torch.from_numpy(G.mu).to(dev, tdt)
                    wt = [float(v) for v in G.w]
                    E, cu, su = [], [], []
                    for q in range(Q):
                        E.append(cg.gramian(cg.EQ(), (X * inv_l[q]).contiguous()))
                        u = (2 * math.pi) * (X @ mut[q])
                        cu.append(torch.cos(u)); su.append(torch.sin(u))
                    rhs = torch.empty((2, n), dtype=tdt, device=dev).t()          # column-major n x 2
                    t = torch.empty((2, n), dtype=tdt, device=dev).t()
                    yh = torch.empty(n, dtype=tdt, device=dev)

                    def host():
                        yh.zero_()
                        for q in range(Q):
                            torch.mul(cu[q], a, out=rhs[:, 0]); torch.mul(su[q], a, out=rhs[:, 1])
                            E[q].mul_(t, rhs)
                            yh.addcmul_(cu[q], t[:, 0], value=wt[q]); yh.addcmul_(su[q], t[:, 1], value=wt[q])

                    def fused():
                        G.mul_(y, a)

                    for _ in range(2):
                        fused(); host()
                    torch.cuda.synchronize()
                    rel = float((y - yh).norm() / yh.norm())
                    tf, th = [], []
                    for _ in range(reps):
                        tf.append(timed(fused)); th.append(timed(host))
                    cg.set_option("time_kernels", 1); cg.kernel_time()
                    for _ in range(3):
                        fused()
                    kms, cnt = cg.kernel_time()
                    cg.set_option("time_kernels", 0)
                    mf, mh = statistics.median(tf), statistics.median(th)
                    tag = f"{name} n = {n} d = {d} {'scalar' if scalar else 'ard   '} l"
                    lines += [f"{tag}: fused {fmt(tf)}   host composition {fmt(th)}   host / fused {mh / mf:6.2f} x",
                              f"{'':{len(tag)}}  fused kernels alone {kms / max(cnt, 1):.3f} ms, {n * n * Q / (mf * 1e-3):.3e} pair-components / s; "
                              f"|fused - host| / |host| = {rel:.2e}"]
                    print("\n".join(lines[-2:]), flush=True)
                    if not mf < mh:
                        slower.append(f"{tag}: fused {mf:.3f} ms, host composition {mh:.3f} ms")
                    del G, E, cu, su
    lines.append("")
    if slower:
        lines += ["Shapes at which the fused product was NOT faster than the host composition:"] + ["  " + s for s in slower] + MIX + [""]
    else:
        lines += ["The fused product was faster than the host composition at every shape above.", ""]

    # Matrix(G) against covgram_matrix of one EQ profile
    n, d = (2048, 3) if quick else (16384, 3)
    lines += [f"Matrix(G), n = m = {n}, d = {d}, into a preallocated buffer, 10 alternating calls after 2 warm-ups; entries per second from the median:"]
    for tdt, name in ((torch.float32, "fp32"), (torch.float64, "fp64")):
        rng = np.random.default_rng(n)
        X = torch.from_numpy(rng.standard_normal((n, d))).to(dev, tdt)
        w = np.exp(0.5 * rng.standard_normal(Q)); mu = np.exp(0.7 * rng.standard_normal((Q, d))); mu[0] = 0.0
        G = cg.gramian(cg.SM(w, [m for m in mu], [lq for lq in 0.3 * np.exp(0.5 * rng.standard_normal((Q, d)))]), X)
        Ge = cg.gramian(cg.Lengthscale(cg.EQ(), 0.3), X)
        buf = torch.empty((n, n), dtype=tdt, device=dev)
        lib, P = cg._ffi.lib(), cg._ffi._P
        ctx = cg.get_ctx(dev).bind_stream()
        spec = Ge._spec()

        def m_sm():
            cg._ffi.check(lib.covgram_sm_matrix(G.handle, G._px.handle, G._py.handle, P(buf.data_ptr()), n, cg._ffi.DEVICE))

        def m_eq():
            cg._ffi.check(lib.covgram_matrix(ctx, cg._ffi.kref(spec), Ge._px.handle, Ge._py.handle, P(buf.data_ptr()), n, cg._ffi.DEVICE))

        for _ in range(2):
            m_sm(); m_eq()
        ts, te = [], []
        for _ in range(10):
            ts.append(timed(m_sm)); te.append(timed(m_eq))
        lines.append(f"  {name}: covgram_sm_matrix (Q = {Q}, ard) {fmt(ts)} ms = {n * n / (statistics.median(ts) * 1e-3):.3e} entries / s;   "
                     f"covgram_matrix EQ {fmt(te)} ms = {n * n / (statistics.median(te) * 1e-3):.3e} entries / s")
        print(lines[-1], flush=True)
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
