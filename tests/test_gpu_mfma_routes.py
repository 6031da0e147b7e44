"""Route table of the fp32 matrix-core MVM drivers (csrc/dense_mfma.hip: mvm_eq_mfma, mvm_eq_mfma_sym, mvm_mfma_gen).

Every case below forces one kernel instance with the existing options, runs one MVM and compares
  * the info keys KEYS with tests/golden/mfma_routes.json — the values the library had BEFORE the drivers' planning and launching code was
    rewritten (one planner, one launch path): a refactor of those drivers must leave every routing decision where it was —, and
  * the result with the fp64 oracle at the tolerance tests/test_gpu_parity.py uses for these paths (1e-5, norm-wise).

The fixture is a record of an OLDER build and is never regenerated from the code under test.  To extend the case list: build the commit in front
of the change to the drivers into a directory of its own and run, on the GPU,
    COVGRAM_LIB=<that build>/lib/libcovgram.so python tests/test_gpu_mfma_routes.py --record
which rewrites the fixture from that library; `--hash` prints per case the sha256 of the result bytes, every last_* info key and the timed
launch count instead (one process per library: the A/B record of profiles/mfma_driver_ab.txt)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mfma_routes.json")
KEYS = ("last_dense_path", "last_mfma_sym", "last_mfma_sym_rt", "last_mfma_f16", "last_mfma_lds", "last_mfma_instance", "last_sum_fused",
        "last_inkernel_reduce", "last_jsplit")
ALL_LAST = ("last_dense_path", "last_jsplit", "last_kron_path", "last_mfma_lds", "last_mfma_sym", "last_dense_sym", "last_dense_bcast", "last_mfma_f16",
            "last_inkernel_reduce", "last_grad_expand", "last_grad_bcast", "last_grad_path", "last_grad_jsplit", "last_hess_path", "last_vgh_path",
            "last_matrix_path", "last_block_matrix_path", "last_sum_fused", "last_mfma_instance", "last_mfma_sym_rt")
DEFAULTS = {"dense_variant": 0, "rows_per_lane": 0, "mfma_lds": -1, "jsplit": 0, "mfma_f16": -1, "mfma_sym": -1, "mfma_sym_rt": -1, "mfma_sym_st": 0,
            "mfma_fuse_w": -1, "inkernel_reduce": -1, "sum_fused": -1}
TOL = 1e-5                       # tests/test_gpu_parity.py: every fp32 matrix-core path against the fp64 oracle
DS = (2, 3, 6, 8, 11, 16, 24, 32)   # bf16 split: K2 = 1, 2, 3, 4, 6, 8, 12, 16; fp16 split: K2 = 1, 1, 2, 2, 3, 4, 6, 8


def _generic(cg, o):
    """(name, covgram kernel, oracle kernel): one kernel per launcher family of the generic matrix-core kernels"""
    L = cg.Lengthscale
    return [
        ("RQ", L(cg.RQ(1.5), 1.3), o.Kernel(o.RQ, param=1.5, lengthscale=1.3)),
        ("Cauchy", 2.0 * cg.Cauchy(), o.Kernel(o.CAUCHY, scale=2.0)),
        ("IMQ", cg.InverseMultiQuadratic(1.2), o.Kernel(o.IMQ, param=1.2)),
        ("MaternP1", cg.MaternP(1), o.Kernel(o.MATERNP, p=1)),
        ("MaternP2", L(cg.MaternP(2), 1.5), o.Kernel(o.MATERNP, p=2, lengthscale=1.5)),
        ("MaternP3", cg.MaternP(3), o.Kernel(o.MATERNP, p=3)),
        ("Dot2", cg.Dot() ** 2, o.Kernel(o.DOT, power=2)),
        ("ExpDot", cg.ExponentialDot(), o.Kernel(o.EXPDOT)),
        ("Product", cg.EQ() * L(cg.Cauchy(), 1.5), o.Composite(((o.Kernel(o.EQ), o.Kernel(o.CAUCHY, lengthscale=1.5)),), o.ISOTROPIC, 1.0)),
        ("Sum2", 1.5 * L(cg.MaternP(2), 0.7) + 0.5 * L(cg.EQ(), 2.0),
         o.Composite(((o.Kernel(o.MATERNP, p=2, lengthscale=0.7, scale=1.5),), (o.Kernel(o.EQ, lengthscale=2.0, scale=0.5),)), o.ISOTROPIC, 1.0)),
        ("Sum3", 0.5 * cg.InverseMultiQuadratic(1.2) + L(cg.MaternP(2), 1.5) + 0.3 * L(cg.EQ(), 0.8),
         o.Composite(((o.Kernel(o.IMQ, param=1.2, scale=0.5),), (o.Kernel(o.MATERNP, p=2, lengthscale=1.5),), (o.Kernel(o.EQ, lengthscale=0.8, scale=0.3),)),
                     o.ISOTROPIC, 1.0)),
    ]


def cases(cg, o):
    """[(name, kernel, oracle kernel, n, m (0: gramian(k, x)), d, nrhs, options, mode)]; mode: "mul", "alias" (y and a share memory), "partial"
    (covgram_mvm_sym_partial, rank 1 of 2)"""
    eq = 1.7 * cg.Lengthscale(cg.EQ(), 0.9)
    eqo = o.Kernel(o.EQ, lengthscale=0.9, scale=1.7)
    out = []
    # the general EQ kernel: every compiled K2 of both splits
    for d in DS:
        for f16 in (0, 2):
            out.append((f"eq d={d} f16={f16}", eq, eqo, 301, 123, d, 1, {"dense_variant": 2, "mfma_f16": f16}, "mul"))
    # ... its instances at one K2 of each split (d = 3: fp16, K2 = 1; d = 7 under the bf16 split: K2 = 4, four row tiles per wave exist)
    for d, f16 in ((3, -1), (7, 0)):
        for rpl in (1, 2, 4):
            for lds in (0, 1):
                for fw in (0, 1):
                    out.append((f"eq d={d} rpl={rpl} lds={lds} fuse_w={fw}", eq, eqo, 301, 123, d, 1,
                                {"dense_variant": 2, "mfma_f16": f16, "rows_per_lane": rpl, "mfma_lds": lds, "mfma_fuse_w": fw}, "mul"))
        out.append((f"eq d={d} alias", eq, eqo, 301, 123, d, 1, {"dense_variant": 2, "mfma_f16": f16}, "alias"))
        # a column split: the slab, its reduce launch or the ticketed in-kernel sum
        for js in (1, 4):
            for ikr in (0, 1):
                for lds in (0, 1):
                    out.append((f"eq d={d} m=4099 jsplit={js} ikr={ikr} lds={lds}", eq, eqo, 301, 4099, d, 1,
                                {"dense_variant": 2, "mfma_f16": f16, "jsplit": js, "inkernel_reduce": ikr, "mfma_lds": lds}, "mul"))
    # >= 1024 row-tile pairs at K2 <= 2: eight waves per workgroup
    out.append(("eq d=3 n=65600 eight waves", eq, eqo, 65600, 320, 3, 1, {"dense_variant": 2, "mfma_lds": 1}, "mul"))
    # the symmetric EQ forms
    for d in DS:
        for f16 in (0, 2):
            out.append((f"eqsym d={d} f16={f16}", eq, eqo, 300, 0, d, 1, {"dense_variant": 2, "mfma_sym": 1, "mfma_f16": f16}, "mul"))
    for d, f16 in ((3, 2), (8, 0), (8, 2), (32, 2)):
        for rt in (1, 2):
            for st in (-1, 4, 16):
                out.append((f"eqsym d={d} f16={f16} rt={rt} st={st}", eq, eqo, 300, 0, d, 1,
                            {"dense_variant": 2, "mfma_sym": 1, "mfma_f16": f16, "mfma_sym_rt": rt, "mfma_sym_st": st}, "mul"))
    # the generic forms
    for name, k, ko in _generic(cg, o):
        for nrhs in (1, 4, 7, 40):
            out.append((f"gen {name} nrhs={nrhs}", k, ko, 301, 123, 3, nrhs, {"dense_variant": 2, "sum_fused": 1}, "mul"))
        for rt in (1, 2):
            out.append((f"gensym {name} rt={rt}", k, ko, 300, 0, 3, 1, {"dense_variant": 2, "sum_fused": 1, "mfma_sym": 1, "mfma_sym_rt": rt}, "mul"))
    # the automatic routing (no forced variant): the radius gates of mfma_eq_eligible / mfma_gen_eligible / the fp16 split on clouds of growing radius,
    # and what covgram_mvm makes of a Sum (one pass or one MVM per term) and of a dot-product kernel
    auto = [("EQ", eq, eqo)] + [c for c in _generic(cg, o) if c[0] in ("MaternP2", "IMQ", "Dot2", "Product", "Sum2", "Sum3")]
    for name, k, ko in auto:
        for scale in (1.0, 2.5, 6.0):
            for nrhs in (1, 7):
                out.append((f"auto {name} scale={scale} nrhs={nrhs}", k, ko, 301, 123, 3, nrhs, {"_scale": scale}, "mul"))
        out.append((f"auto {name} gramian", k, ko, 300, 0, 3, 1, {"mfma_sym": 1}, "mul"))
    # one rank's share of gramian(k, x)
    out.append(("partial eq d=3 rank 1 of 2", eq, eqo, 600, 0, 3, 1, {"dense_variant": 2, "mfma_sym": 1}, "partial"))
    out.append(("partial MaternP2 d=3 rank 1 of 2", cg.MaternP(2), o.Kernel(o.MATERNP, p=2), 600, 0, 3, 1, {"dense_variant": 2, "mfma_sym": 1}, "partial"))
    return out


def run_case(cg, o, idx, case, all_keys=False):
    """-> (result, fp64 oracle result, info keys, timed launches)"""
    name, k, ko, n, m, d, nrhs, opts, mode = case
    rng = np.random.default_rng(5000 + idx)
    opts = dict(opts)
    scale = opts.pop("_scale", 1.0)
    X = (scale * rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)
    Y = X if m == 0 else (scale * rng.standard_normal((m, d)) / np.sqrt(d)).astype(np.float32)
    mm = Y.shape[0]
    A = rng.standard_normal((mm, nrhs)).astype(np.float32)
    if nrhs == 1:
        A = A[:, 0]
    Xd = torch.from_numpy(X).cuda()
    G = cg.gramian(k, Xd) if m == 0 else cg.gramian(k, Xd, torch.from_numpy(Y).cuda())
    try:
        for key, v in opts.items():
            cg.set_option(key, v)
        cg.set_option("time_kernels", 1)
        if mode == "alias":                                   # a is the head of y's buffer
            buf = torch.zeros(max(n, mm), dtype=torch.float32, device="cuda")
            buf[:mm] = torch.from_numpy(A).cuda()
            cg.mul_(buf[:n], G, buf[:mm], -0.7, 0.0)
            got, ref = buf[:n].cpu().numpy(), o.mul(None, ko, X, Y, A, -0.7, 0.0, np.float32)
        elif mode == "partial":                               # rank 0's share completes the product; the keys are rank 1's
            ad = torch.from_numpy(A).cuda()
            p0 = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda"); p1 = p0.clone()
            G.sym_partial_(p0, ad, 0, 2)
            cg.kernel_time()
            G.sym_partial_(p1, ad, 1, 2)
            got, ref = np.stack([p1.cpu().numpy(), (p0 + p1).cpu().numpy()]), o.mul(None, ko, X, Y, A, dtype=np.float32)
        elif nrhs == 1:
            y0 = rng.standard_normal(n).astype(np.float32)
            yd = torch.from_numpy(y0.copy()).cuda()
            cg.mul_(yd, G, torch.from_numpy(A).cuda(), -0.7, 1.3)
            got, ref = yd.cpu().numpy(), o.mul(y0, ko, X, Y, A, -0.7, 1.3, np.float32)
        else:
            got, ref = (G @ torch.from_numpy(A).cuda()).cpu().numpy(), o.mul(None, ko, X, Y, A, dtype=np.float32)
        launches = cg.kernel_time()[1]
        info = {key: cg.get_info(key) for key in (ALL_LAST if all_keys else KEYS)}
    finally:
        cg.set_option("time_kernels", 0)
        for key, v in DEFAULTS.items():
            cg.set_option(key, v)
    return got, ref, info, launches


def relerr(b, ref):
    b = np.asarray(b, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    return np.linalg.norm(b - ref) / np.linalg.norm(ref)


def test_routes_match_the_recorded_table_and_the_oracle(cg, oracle, monkeypatch):
    # A route leaves the info keys it does not write as the call before left them, and the table records them as they stand after each case of
    # the fixed sequence below, started from a fresh context (the recording ran in a process of its own): the test takes a fresh context too,
    # whatever ran in this process before; monkeypatch puts the process's contexts back afterwards
    monkeypatch.setattr(sys.modules[cg.get_ctx.__module__], "_CTX", {})
    with open(FIXTURE) as f:
        want = json.load(f)
    cs = cases(cg, oracle)
    assert sorted(want) == sorted(c[0] for c in cs), "tests/golden/mfma_routes.json and cases() list different cases"
    bad = []
    for idx, case in enumerate(cs):
        got, ref, info, _ = run_case(cg, oracle, idx, case)
        if info != want[case[0]]:
            bad.append((case[0], {k: (info[k], want[case[0]][k]) for k in KEYS if info[k] != want[case[0]][k]}))
        e = relerr(got[1] if case[8] == "partial" else got, ref)
        if not e <= TOL:
            bad.append((case[0], "relative error", e))
    assert not bad, bad


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "covariancefunctions.jl_amd")); sys.path.insert(0, os.path.join(root, "oracle"))
    import covgram
    import covgram_oracle
    table = {}
    for idx, case in enumerate(cases(covgram, covgram_oracle)):
        got, ref, info, launches = run_case(covgram, covgram_oracle, idx, case, all_keys="--hash" in sys.argv)
        if "--hash" in sys.argv:
            e = relerr(got[1] if case[8] == "partial" else got, ref)
            print(f"{case[0]} | {hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()} | launches {launches} | relerr {e:.2e} | "
                  + " ".join(f"{k[5:]}={v}" for k, v in info.items()), flush=True)
        table[case[0]] = info
    if "--record" in sys.argv:
        with open(FIXTURE, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(name)}: {json.dumps(info)}" for name, info in table.items()) + "\n}\n")   # one case per line
        print(f"recorded {len(table)} cases from {covgram._ffi.LIB_PATH}")
