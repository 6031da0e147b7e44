"""The entrywise bound of tests/test_gpu_matrix.py is feasible: an exactly rounded fp32 evaluation in the matrix kernels' own order
of operations (matrix_cases.emulate_f32) stays inside it, on the clouds the GPU tests use and on tighter / wider ones.  No GPU: the
device's exp / log / Bessel evaluations are not part of this emulation — their headroom is what the GPU tests measure.  The bound is
a condition derived in matrix_cases.py; a ratio above 1 here means the bound asks more than fp32 arithmetic can give, and is a
finding about the bound, to be reasoned about, never a number to fit."""
import numpy as np
import pytest

import covgram_oracle as o
import matrix_cases as mc

F32 = np.float32

ISO = [("EQ l=0.7", o.Kernel(o.EQ, lengthscale=0.7)), ("Exp", o.Kernel(o.EXP)), ("RQ(0.37)", o.Kernel(o.RQ, param=0.37)),
       ("2.5*MaternP(2) l=1.3", o.Kernel(o.MATERNP, p=2, lengthscale=1.3, scale=2.5)), ("Matern(0.8)", o.Kernel(o.MATERN, param=0.8)),
       ("gammaExp(1.5)", o.Kernel(o.GAMMAEXP, param=1.5)),
       ("iso_product", o.Composite(((o.Kernel(o.EQ), o.Kernel(o.CAUCHY, lengthscale=1.5)),), o.ISOTROPIC, 1.0))]
DOT = [("Dot", o.Kernel(o.DOT)), ("Dot^3", o.Kernel(o.DOT, power=3)), ("ExponentialDot", o.Kernel(o.EXPDOT)),
       ("0.3*ExponentialDot", o.Kernel(o.EXPDOT, scale=0.3)), ("AsinDot", o.Kernel(o.ASINDOT)),
       ("dot_sum", o.Composite(((o.Kernel(o.DOT, power=2),), (o.Kernel(o.EXPDOT, scale=0.3),)), o.DOTPRODUCT, 1.0))]


def ratio(name, ko, X, Y, what):
    ref, bound = mc.reference_and_bound(o, ko, X, Y, F32)
    w, i, j = mc.worst_entry(mc.emulate_f32(o, ko, X, Y), ref, bound)
    print(f"matrix-bound-host {name:22s} d={X.shape[1]:3d} {what}: worst err/bound {w:.3f} at ({i}, {j}), ref {ref[i, j]:.3e}")
    return w


@pytest.mark.parametrize("d", [1, 3, 8, 12, 32, 40, 64])
def test_fp32_emulation_within_bound_isotropic(d):
    for name, ko in ISO:
        # the clouds of the GPU tests: far rows 6..10 lengthscales away, rows with s = 0 exactly
        X, Y, far, cop = mc.iso_cloud(np.random.default_rng(100 + d), 257, 130, d, F32, lscale=mc.lengthscale_of(ko))
        assert len(far) == 8 and len(cop) == 4
        assert ratio(name, ko, X, Y, "gpu-test cloud") <= 1.0, (name, d)
        for scale, shift in ((0.3, 0.0), (1.5, 0.0), (0.8, 8.0)):
            rng = np.random.default_rng(1)
            X = (scale * rng.standard_normal((257, d)) + 0.2).astype(F32); Y = (scale * rng.standard_normal((130, d))).astype(F32)
            X[:8] += F32(shift) / np.sqrt(d)
            assert ratio(name, ko, X, Y, f"scale {scale} shift {shift}") <= 1.0, (name, d, scale, shift)


@pytest.mark.parametrize("d", [65, 100, 256])
def test_fp32_emulation_within_bound_wide_clouds(d):
    """The clouds of the generic-kernel cases (d > 64), at the sizes the GPU test runs: see matrix_cases.wide_cloud for why d = 256
    carries no far rows."""
    for name, ko in [("EQ", o.Kernel(o.EQ)), ISO[1], ISO[2], ISO[3], ISO[6]]:           # unit-scale lengthscales, as the GPU cases
        for n, m in ((1028, 130), (255, 17)):
            X, Y = mc.wide_cloud(o, ko, np.random.default_rng(d + n), n, m, d, F32)
            assert ratio(name, ko, X, Y, f"wide cloud n={n}") <= 1.0, (name, d, n)


@pytest.mark.parametrize("d", [1, 3, 8, 12, 32, 40, 64, 256])
def test_fp32_emulation_within_bound_dot_product(d):
    for name, ko in DOT:
        X, Y = mc.dot_cloud(np.random.default_rng(200 + d), 257, 130, d, F32, unit_ball=name == "AsinDot")
        assert ratio(name, ko, X, Y, "gpu-test cloud") <= 1.0, (name, d)
        if name == "AsinDot":
            continue
        for scale in (0.3, 0.8):
            rng = np.random.default_rng(2)
            sc = scale if d == 1 else scale * (1.0 if "ExponentialDot" in name and d <= 8 else 1 / np.sqrt(d)) * (3 if "ExponentialDot" in name else 1)
            X = (sc * rng.standard_normal((257, d)) + 0.1).astype(F32); Y = (sc * rng.standard_normal((130, d))).astype(F32)
            assert ratio(name, ko, X, Y, f"scale {scale}") <= 1.0, (name, d, scale)


def test_bound_forms():
    """The bound is the documented condition: relative TOL where L <= 10, TOL L / 10 beyond, TOL (|phi| + |phi'| sum |x||y|) for dot
    products; the tiny term only matters below the normal range."""
    ko = o.Kernel(o.EQ)
    X = np.array([[0.0], [0.0], [0.0]], F32); Y = np.array([[0.0], [2.0], [10.0]], F32)
    ref, b = mc.reference_and_bound(o, ko, X, Y, F32)
    t = mc.tiny(F32)
    assert np.allclose(ref[0], [1.0, np.exp(-2.0), np.exp(-50.0)], rtol=1e-15)
    assert np.allclose(b[0] - t, [1e-5, 1e-5 * np.exp(-2.0), 1e-5 * 5.0 * np.exp(-50.0)], rtol=1e-12)
    kd = o.Kernel(o.DOT, power=3)
    X = np.array([[1.0, -2.0]]); Y = np.array([[3.0, 1.5]])
    ref, b = mc.reference_and_bound(o, kd, X, Y, np.float64)
    assert ref[0, 0] == 0.0 and np.isclose(b[0, 0], 1e-12 * 0.0 + mc.tiny(np.float64))      # phi' = 3 s^2 = 0 at s = 0
    kd = o.Kernel(o.DOT)
    ref, b = mc.reference_and_bound(o, kd, X, Y, np.float64)
    assert ref[0, 0] == 0.0 and np.isclose(b[0, 0], 1e-12 * 6.0)
