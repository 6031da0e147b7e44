"""The entrywise bound of tests/test_gpu_sm.py is feasible: exactly rounded fp32 arithmetic (sm_ref.emulate_f32), in the per-point-phase
form and in the per-pair-cosine form, stays within HALF of it on the clouds and parameters the device test uses.  No GPU: the device's
exp and the rounding of its phase tables are not part of this emulation — their headroom (the other half) is what the device test
measures.  A ratio above 0.5 here is a finding about the bound, to be reasoned about, never a number to fit."""
import numpy as np
import pytest

import sm_ref as sr

F32 = np.float32


@pytest.mark.parametrize("case", sr.CASES, ids=lambda c: sr.case_name(c, F32))
def test_fp32_emulation_within_half_the_bound(case):
    X, Y, w, mu, l, inv_l = sr.make_case(case, F32)
    ref, bound = sr.reference_and_bound(w, mu, inv_l, X, Y, F32)
    for form in ("phase", "pair"):
        r, i, j = sr.worst_entry(sr.emulate_f32(w, mu, inv_l, X, Y, form), ref, bound)
        print(f"sm-bound-host {sr.case_name(case, F32)} {form}: worst err/bound {r:.3f} at ({i}, {j}), ref {ref[i, j]:.3e}")
        assert r <= 0.5, (case, form, r)


def test_bound_form():
    """The bound is the documented condition: TOL |w| e (max(1, s / 20) + 2 pi sum |mu| (|x| + |y|)) + tiny, summed over the components."""
    w = np.array([2.0, -0.5]); mu = np.array([[0.0], [0.25]]); inv_l = np.array([[1.0], [0.5]])
    X = np.array([[1.0]]); Y = np.array([[-1.0], [9.0]])
    ref, b = sr.reference_and_bound(w, mu, inv_l, X, Y, np.float64)
    s0 = np.array([4.0, 64.0]); s1 = s0 / 4
    want = 2.0 * np.exp(-s0 / 2) - 0.5 * np.cos(2 * np.pi * 0.25 * np.array([2.0, -8.0])) * np.exp(-s1 / 2)
    assert np.allclose(ref[0], want, rtol=1e-14, atol=1e-300)
    ph = 2 * np.pi * 0.25 * (1.0 + np.array([1.0, 9.0]))
    lim = 1e-12 * (2.0 * np.exp(-s0 / 2) * np.maximum(1, s0 / 20) + 0.5 * np.exp(-s1 / 2) * (np.maximum(1, s1 / 20) + ph)) + sr.tiny(np.float64)
    assert np.allclose(b[0], lim, rtol=1e-13)
