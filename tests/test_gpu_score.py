"""The score stage on the device (csrc/k_score.hip: k_fn, k_fn20, k_diag_chol, k_di_tridiag, k_di_ql, k_colsum, k_apc_apply) through
the operator entries compute_FN, compute_DI_gauss and correct_APC, against the extended-precision model of tests/score_model.py.

Every entry is held to its own scale, not to the largest score of the matrix (the bars and where they come from: score_model's
fn_bound, apc_bound, di_bound).  The inputs are not alignments: they are built to enter each branch by block size (s = 1, 2: no
Householder step; 12 / 13: a partial last k-step of the MFMA products; 16 / 17: one tile or four; 23 .. 29: the seven-unit FN
instance), the index arithmetic beyond one pass (the persistent FN list longer than its grid, APC beyond 256 rows) and the
cancellations (a Householder column whose tail is 1e-9 of its head, couplings of 1e-8, blocks that are an offset plus a small signal).
The DI expectations come from tests/golden/score_cases.npz (mpmath, 40 digits); FN and APC are recomputed here in np.longdouble."""
import os

import numpy as np
import pytest

import score_model as sm

pytestmark = pytest.mark.gpu

# c of the DI bar: 8 x the largest error of the f64 oracle against the model in the bar's unit (0.0185, tests/golden/README.md), at least 8
DI_C = sm.DI_C
assert DI_C == 8.0


@pytest.fixture(scope="module")
def g():
    import gaussdca.jl_amd as g

    assert os.path.exists(g._lib.LIB_PATH), "libgdca.so missing: the GPU tests never fall back to the CPU"
    assert g.load().gdca_device_count() > 0, "no HIP device"
    return g


@pytest.fixture(scope="module")
def ctx(g):
    c = g.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_cases.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", sm.DI_CASES)
def test_di_every_pair_within_its_own_bar(g, ctx, golden, name):
    c = sm.score_cases("di", name)
    q, N = c["q"], c["N"]
    s = q - 1
    assert sm.input_hash(c["mJ"], c["C"]) == str(golden[name + ".sha256"]), "inputs differ from those the golden file was made from"
    ref, B = golden[name + ".DI"], golden[name + ".B"]
    DI = g.compute_DI_gauss(c["mJ"], c["C"], q, ctx=ctx)
    # the status itself: GDCA_OK, so no eigenvalue iteration gave up (di_noconv == 0); and the same bits on a second call
    S2 = np.full((N, N), np.nan)
    rc = ctx.lib.gdca_di(ctx.h, g._lib._p(c["mJ"]), g._lib._p(c["C"]), N, q, g._lib._p(S2))
    assert rc == g._lib.GDCA_OK
    assert np.array_equal(S2, DI)
    assert np.array_equal(DI, DI.T) and np.all(np.diag(DI) == 0.0)
    err = np.abs(DI - ref)
    bound = sm.di_bound(s, B, DI_C)
    units = sm.di_units(s, B, err)
    w = tuple(int(v) for v in np.unravel_index(np.argmax(err / bound), err.shape))
    print("%s: worst pair %s err %.3g = %.3g of its bar (%.3g units of s^2 u B^2 beyond the log-sum term; largest %.3g units)"
          % (name, w, err[w], err[w] / bound[w], units[w], units.max()))
    assert np.all(err <= bound), [(int(i), int(j), float(err[i, j]), float(bound[i, j]), float(units[i, j]))
                                  for i, j in zip(*np.nonzero(err > bound)) if i < j]
    for i, j in c["exact_zero"]:  # X = 0: every gamma is 0 and the two halves of the formula cancel
        assert abs(DI[i, j]) <= s * sm.U, DI[i, j]


@pytest.mark.parametrize("name", sm.FN_CASES)
def test_fn_every_pair_within_its_own_bar(g, ctx, name):
    c = sm.score_cases("fn", name)
    q, N = c["q"], c["N"]
    s = q - 1
    ref, scale = sm.fn_model(c["mJ"], q)
    FN = g.compute_FN(c["mJ"], q, ctx=ctx)
    assert np.array_equal(FN, FN.T) and np.all(np.diag(FN) == 0.0)
    bound = sm.fn_bound(s, ref, scale)
    err = np.abs(FN - ref)
    off = ~np.eye(N, dtype=bool)
    print("%s: worst err / bound %.3g" % (name, float(np.max(err[off] / bound[off]))))
    assert np.all(err <= bound), float(np.max(err - bound))
    # every off-diagonal entry was written: the launcher zero-fills S, and these blocks have FN > 0 (but for s = 1, where the
    # centred 1 x 1 block is 0 identically and the bar above has said all there is to say)
    if s > 1:
        assert np.all(ref[off] > 10 * bound[off]) and np.all(FN[off] > 0.0)


@pytest.mark.parametrize("name", sm.APC_CASES)
def test_apc_every_entry_within_its_own_bar(g, ctx, name):
    S = sm.score_cases("apc", name)["S"]
    ref, corr, amp = sm.apc_model(S)
    out = g.correct_APC(S, ctx=ctx)
    bound = sm.apc_bound(S, corr, amp)
    err = np.abs(out - ref)
    print("%s: amp %.3g, worst err / bound %.3g" % (name, float(amp), float(np.max(err / bound))))
    assert np.all(bound > 0) and np.all(err <= bound), float(np.max(err - bound))
    assert np.array_equal(out, out.T)
