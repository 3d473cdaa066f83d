"""log det C: the model's own checks (tests/logdet_model.py), the declared and exported entry points, and the operators' refusal to run
without a GPU.  The device side is tests/test_gpu_logdet.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import logdet_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gdca_last_logdet", "gdca_spd_inverse_logdet_dev", "gdca_spd_inverse_logdet", "gdca_run_loglik_dev", "gdca_run_loglik"]


def _matrices():
    """every SPD matrix of the GPU test: (name, C, Reference)"""
    out = [("spd n=%d" % n,) + lm.operator_case(n) for n in lm.OPERATOR_SIZES]
    out.append(("diag 2^e",) + lm.reference("pow2", lambda: lm.pow2_diagonal()[0]))
    out.append(("4 C, n=257",) + lm.reference("4C", lambda: 4.0 * lm.random_spd(257)))
    for N, M, q in lm.FAMILIES:
        for pc in lm.PSEUDOCOUNTS:
            out.append(("family N=%d M=%d q=%d pc=%g" % (N, M, q, pc),) + lm.family_case(N, M, q, pc))
    return out


def test_longdouble_is_extended_and_agrees_with_mpmath():
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    for n in (1, 15, 16, 17):
        C, ref = lm.operator_case(n)
        assert abs(lm.logdet_mp(C) - ref.logdet) <= 2 * lm.U * abs(ref.logdet)
    C, ref = lm.family_case(7, 200, 2, 0.5)  # (n = 7)
    assert abs(lm.logdet_mp(C) - ref.logdet) <= 2 * lm.U * abs(ref.logdet)


def test_numpy_f64_reference_is_inside_the_bar():
    """The reference alone stays inside the bar: numpy's f64 2 sum log diag(cholesky(C)) on every test matrix."""
    for name, C, ref in _matrices():
        frac = ref.fraction(lm.logdet_numpy(C))
        print("%-32s logdet %+.6e  bar %.3g (elimination %.3g, logarithms %.3g)  numpy uses %.3g of it" %
              (name, ref.logdet, ref.bar, lm.F_BLOCKED * ref.term_elim, ref.term_log, frac))
        assert frac <= 1.0, (name, frac)


def test_the_bar_is_not_slack():
    """One pivot off by 1e-9 relative is outside the bar.  The bar is a worst-case bound and grows like n S1 ~ n^2.5 on the random
    matrices: at n = 1300 it has reached 1.6e-9 and the perturbation sits at 0.6 of it (printed, not asserted); everywhere else the
    perturbation is outside, by a factor 2.8 at n = 640 and thousands at small n."""
    for name, C, ref in _matrices():
        d = ref.d.copy()
        d[ref.n // 2] *= np.longdouble(1.0) + np.longdouble(1e-9)
        frac = ref.fraction(float(np.log(d).sum(dtype=np.longdouble)))
        print("%-32s a pivot off by 1e-9: %.3g of the bar" % (name, frac))
        if name != "spd n=1300":
            assert frac > 1.0, (name, frac)


def test_exact_cases_of_the_model():
    C, e = lm.pow2_diagonal()
    _, ref = lm.reference("pow2", lambda: C)
    assert abs(ref.logdet - np.log(2.0) * float(e.sum())) <= (np.log2(300) + 2) * lm.U * np.abs(e).sum() * np.log(2.0)
    _, r1 = lm.operator_case(257)
    _, r4 = lm.reference("4C", lambda: 4.0 * lm.random_spd(257))
    assert abs((r4.logdet - r1.logdet) - 257 * np.log(4.0)) <= 4 * lm.U * abs(r4.logdet)
    with pytest.raises(ValueError):
        lm.cholesky_ld(np.array([[1.0, 2.0], [2.0, 1.0]]))


def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "gdca.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(r"gdca_status\s+%s\s*\(" % name, code), name
    assert re.search(r"#define\s+GDCA_LOG_2PI\s+1\.8378770664093453\b", src)
    assert float("1.8378770664093453") == float(np.log(2.0 * np.pi))
    # the header says what it must: the definition, the determinism contract, the branches; and the energies point here
    for phrase in ("log p(x) = -E(x) - 1/2 (n log 2 pi + log det C)", "MERGE_GROUP=1", "Newton-Schulz", "Cholesky fallback", "does not depend on K"):
        assert phrase in src, phrase
    assert "NOT included" not in src
    from gaussdca.jl_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS
    for m in ("last_logdet", "spd_inverse_logdet", "run_loglik"):
        assert callable(getattr(_lib.Context, m))
    from gaussdca.jl_amd import dcautils

    assert dcautils.LOG_2PI == float(np.log(2.0 * np.pi))
    assert dcautils.loglik_constant(3, 0.25) == 0.5 * (3 * dcautils.LOG_2PI + 0.25)


def test_operators_raise_without_a_gpu(refdata):
    import gaussdca.jl_amd as g

    if g.load().gdca_device_count() > 0:
        pytest.skip("a HIP device is present: the refusal is what a machine without one shows")
    with pytest.raises(g.GdcaError):
        g.gDCA_loglik(os.path.join(refdata, "small.fasta.gz"))
    with pytest.raises(g.GdcaError):
        g.inv_cholesky(np.eye(3), return_logdet=True)
    with pytest.raises(g.GdcaError):
        g.sequence_loglik(np.eye(4), np.full(4, 0.2), np.ones((1, 2), dtype=np.int8), 0.0, q=5)
