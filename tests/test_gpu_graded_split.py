"""The graded column split of the general matrix-core EQ kernel (option "mfma_graded"; csrc/mfma_plan.hpp: plan_columns_graded): the chunk boundaries
reach dense_mfma_eq_kernel as a table in its kernel arguments, one slab row per chunk, summed in chunk order.  Small shapes at which the table can go
wrong — a column count that is no multiple of the stage, a short last chunk, more than one row block — on every form of the kernel: the fp16 and bf16
splits, d = 3 and d = 8, one-wave and LDS-shared workgroups, the separate and the in-kernel slab sum, alpha / beta on a non-zero y, y aliasing a.
Each result is held to 1e-5 norm-wise AND row-wise against the fp64 oracle (the bound of the full-size tests and BASELINE.json), as is the uniform split
of the same shape; the graded result is bit-identical from run to run."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _errors(y, ref, absref):
    y = y.double().cpu().numpy()
    return float(np.linalg.norm(y - ref) / np.linalg.norm(ref)), float(np.max(np.abs(y - ref) / absref))


@pytest.mark.parametrize("kind", ["d3_f16", "d3_bf16", "d8"])
@pytest.mark.parametrize("n,m", [(1000, 4100), (2048, 2048)])
def test_graded_split_matches_the_oracle_and_itself(cg, oracle, n, m, kind):
    import c_oracle
    d = 8 if kind == "d8" else 3
    rng = np.random.default_rng(1000 * d + n)
    Yh = (rng.standard_normal((m, d)) * min(1.0, np.sqrt(3.0 / d))).astype(np.float32)
    Xh = Yh[:n] if n == m else (rng.standard_normal((n, d)) * min(1.0, np.sqrt(3.0 / d))).astype(np.float32)
    ah = rng.standard_normal(m).astype(np.float32); y0h = rng.standard_normal(n).astype(np.float32)
    X = torch.from_numpy(Xh).cuda(); Y = X if n == m else torch.from_numpy(Yh).cuda()
    a = torch.from_numpy(ah).cuda(); y0 = torch.from_numpy(y0h).cuda()
    # the fp64 references, once per case: G a and |G| |a| (EQ is positive: G |a|)
    K = oracle.Kernel(oracle.EQ)
    Ga = c_oracle.mvm(K, Xh.astype(np.float64), Yh.astype(np.float64), ah.astype(np.float64))
    Gabs = c_oracle.mvm(K, Xh.astype(np.float64), Yh.astype(np.float64), np.abs(ah).astype(np.float64))
    try:
        cg.set_option("mfma_sym", 0); cg.set_option("dense_variant", 2); cg.set_option("mfma_f16", 0 if kind == "d3_bf16" else -1)
        G = cg.gramian(cg.EQ(), X, Y)
        for lds in (0, 1):
            for ikr in (0, 1):
                cg.set_option("mfma_lds", lds); cg.set_option("inkernel_reduce", ikr)
                for alpha, beta in ((1.0, 0.0), (0.7, -0.3)):
                    ref = alpha * Ga + beta * y0h.astype(np.float64)
                    absref = abs(alpha) * Gabs + abs(beta) * np.abs(y0h).astype(np.float64)
                    tag = (n, m, kind, lds, ikr, alpha, beta)
                    outs = []
                    for graded in (1, 1, 0):
                        cg.set_option("mfma_graded", graded)
                        y = y0.clone(); G.mul_(y, a, alpha, beta)
                        chunks = cg.get_info("last_mfma_graded")
                        assert cg.get_info("last_dense_path") == 2 and cg.get_info("last_mfma_lds") == lds and cg.get_info("last_inkernel_reduce") == ikr, tag
                        assert cg.get_info("last_mfma_f16") == (0 if kind == "d3_bf16" else 1), tag
                        assert (chunks > 1) if graded else (chunks == 0), (tag, graded, chunks)
                        rel, roww = _errors(y, ref, absref)
                        print(f"{tag} graded {graded} chunks {chunks}: rel-err {rel:.3e} row-wise {roww:.3e}")
                        assert rel <= TOL and roww <= TOL, (tag, graded, rel, roww)
                        outs.append(y)
                    assert torch.equal(outs[0], outs[1]), tag                 # the same slab order on every run
                if n == m:                                                    # y aliasing a
                    for graded in (1, 0):
                        cg.set_option("mfma_graded", graded)
                        y = a.clone(); G.mul_(y, y, 0.7, -0.3)
                        assert (cg.get_info("last_mfma_graded") > 1) == bool(graded)
                        rel, roww = _errors(y, 0.7 * Ga - 0.3 * ah.astype(np.float64), 0.7 * Gabs + 0.3 * np.abs(ah).astype(np.float64))
                        print(f"{(n, m, kind, lds, ikr)} in place, graded {graded}: rel-err {rel:.3e} row-wise {roww:.3e}")
                        assert rel <= TOL and roww <= TOL, (n, m, kind, lds, ikr, graded, rel, roww)
    finally:
        for key in ("mfma_sym", "mfma_f16", "mfma_lds", "inkernel_reduce", "mfma_graded"):
            cg.set_option(key, -1)
        cg.set_option("dense_variant", 0)


def test_stamps_of_a_graded_launch_are_read_back(cg):
    """covgram_ctx_read_stamps (tools/c2_drain_probe.py): one record per workgroup of the stamped launch — row blocks x chunks of the graded table —, each
    ending after it started; a short buffer takes only what fits."""
    import ctypes as C
    rng = np.random.default_rng(11)
    X = torch.from_numpy(rng.standard_normal((2048, 3)).astype(np.float32)).cuda(); a = torch.from_numpy(rng.standard_normal(2048).astype(np.float32)).cuda()
    lib, h = cg._ffi.lib(), cg.get_ctx().handle
    try:
        cg.set_option("mfma_sym", 0); cg.set_option("dense_variant", 2); cg.set_option("mfma_lds", 1); cg.set_option("mfma_graded", 1)
        G = cg.gramian(cg.EQ(), X)
        y_plain = G @ a
        cg.set_option("mfma_stamp", 1)
        y_stamped = G @ a
        inst, chunks = cg.get_info("last_mfma_instance"), cg.get_info("last_mfma_graded")
        assert inst // 10 % 10 == 1 and chunks > 1, (inst, chunks)
        assert torch.equal(y_plain, y_stamped)                                    # the diagnostic build computes the same thing
        cnt = C.c_int64(-1)
        cg._ffi.check(lib.covgram_ctx_read_stamps(h, None, 0, C.byref(cnt)))
        wpb = inst // 1000 % 10
        assert cnt.value == (2048 // 64 // wpb) * chunks, (cnt.value, wpb, chunks)
        buf = (C.c_uint64 * (4 * cnt.value))()
        cg._ffi.check(lib.covgram_ctx_read_stamps(h, buf, cnt.value, C.byref(cnt)))
        s = np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4)
        assert (s[:, 2] > s[:, 0]).all() and (s[:, 3] >= s[:, 1]).all() and (s[:, 1] > 0).all()
        short = (C.c_uint64 * 12)(*([7] * 12))
        cg._ffi.check(lib.covgram_ctx_read_stamps(h, short, 2, C.byref(cnt)))
        assert list(short[:8]) == [int(v) for v in s[:2].ravel()] and list(short[8:]) == [7] * 4
    finally:
        cg.set_option("mfma_stamp", 0); cg.set_option("mfma_sym", -1); cg.set_option("dense_variant", 0); cg.set_option("mfma_lds", -1); cg.set_option("mfma_graded", -1)


def test_forced_split_and_small_shapes_keep_the_uniform_plan(cg):
    """A forced "jsplit" / "target_wgs" keeps equal chunks whatever "mfma_graded" says, and the automatic rule leaves a GP-sized problem alone."""
    rng = np.random.default_rng(9)
    X = torch.from_numpy(rng.standard_normal((4096, 3)).astype(np.float32)).cuda(); a = torch.from_numpy(rng.standard_normal(4096).astype(np.float32)).cuda()
    try:
        cg.set_option("mfma_sym", 0); cg.set_option("dense_variant", 2)
        G = cg.gramian(cg.EQ(), X)
        y_auto = G @ a
        assert cg.get_info("last_dense_path") == 2 and cg.get_info("last_mfma_graded") == 0
        cg.set_option("mfma_graded", 0)
        assert torch.equal(G @ a, y_auto)
        cg.set_option("mfma_graded", 1)
        for key in ("jsplit", "target_wgs"):
            cg.set_option(key, 4 if key == "jsplit" else 512)
            G @ a
            assert cg.get_info("last_mfma_graded") == 0, key
            cg.set_option(key, 0)
        G @ a
        assert cg.get_info("last_mfma_graded") > 1
    finally:
        cg.set_option("mfma_sym", -1); cg.set_option("dense_variant", 0); cg.set_option("mfma_graded", -1); cg.set_option("jsplit", 0); cg.set_option("target_wgs", 0)
