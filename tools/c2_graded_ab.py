"""The contract kernel (C2: EQ, d = 3, n = 131072, fp32, all entries), its row shards and C3's row shard (d = 8, 65536 rows x 524288 columns): the column
split (option mfma_graded), interleaved; us per MVM.
0 = equal chunks, -1 = the automatic rule, 1 = the rule's schedule wherever the shape admits it; 100 h + f = a tail of h half rounds of resident workgroups cut
into chunks halving down to a floor of 16 * 2^f tiles (102: half a round down to 64 tiles, 202: one round, 402: two rounds, 203: one round down to 128).
Per setting: the repetitions after a discarded first, their minimum and median, and the chunk count."""
import os, sys, numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "covariancefunctions.jl_amd"))
import covgram as cg
e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 4          # (the first is discarded)
CANDIDATES = (0, -1, 1, 101, 102, 103, 104, 201, 202, 203, 402)
cg.set_option("mfma_sym", 0)
for name, n, d, per, settings in (("C2", 131072, 3, 131072, CANDIDATES), ("C2, rank 0 of 8", 131072, 3, 16384, (0, -1, 1)), ("C2, rank 0 of 16", 131072, 3, 8192, (0, -1, 1)),
                                  ("C3, rank 0 of 8", 524288, 8, 65536, (0, -1, 102, 202))):
    rng = np.random.default_rng(0xC0F + 1)
    X = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda(); a = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    G = cg.gramian(cg.EQ(), X[:per], X); y = torch.empty(per, dtype=torch.float32, device="cuda")
    res, chunks = {}, {}
    for rep in range(REPS):
        for v in settings:
            cg.set_option("mfma_graded", v)
            for _ in range(4): G.mul_(y, a)
            torch.cuda.synchronize(); e0.record()
            for _ in range(40): G.mul_(y, a)
            e1.record(); e1.synchronize()
            if rep: res.setdefault(v, []).append(e0.elapsed_time(e1) / 40 * 1e3)
            chunks[v] = cg.get_info("last_mfma_graded")
    cg.set_option("mfma_graded", -1)
    print(f"{name}: rows {per} x cols {n}, d = {d}, instance {cg.get_info('last_mfma_instance')}")
    for v, ts in res.items():
        print(f"  mfma_graded = {v:3d} (graded chunks {chunks[v]:2d}): " + " ".join(f"{t:.1f}" for t in ts) + f"   min {min(ts):.1f}  median {np.median(ts):.1f} us", flush=True)
    del G, X, a, y
cg.set_option("mfma_sym", -1)
