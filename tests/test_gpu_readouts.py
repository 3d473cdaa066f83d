"""The three read-outs of the fitted model (energies, pair energies, mutation scan) on ONE context, one after the other: they share
the pack kernel, the g pass and the grow-only buffers Xg, gpart, gvec and PX*, so a read-out must not see what an earlier, larger or
differently shaped one left there.  Every result is array_equal to the same call on a fresh context that ran nothing else, and within
the bound its CPU model states (the bounds of tests/test_gpu_energy.py, test_gpu_pair_energy.py and test_gpu_mutation.py).

Shapes: N = 9 (three site blocks, the last ragged), split = 5 (A: two dwords, the second ragged; B: one); q = 21 (the s = 20
instances; three row blocks of the scan) and q = 5 (the generic instances; one ragged row block); K = 300 (two pack workgroups)
before and after K = 2 and 3."""
import numpy as np
import pytest

import pair_energy_model as pm
from gdca_testutil import assert_within_order_bound, g, mutation_reference as reference, ratio  # noqa: F401 (g: fixture)

pytestmark = pytest.mark.gpu

N, SPLIT = 9, 5


def synthetic_model(q, seed):
    """mJ = B B' / n + I (symmetric positive definite), Pi uniform in (0, 1 / q): no fit"""
    rng = np.random.default_rng(seed)
    n = N * (q - 1)
    B = rng.standard_normal((n, n))
    return B @ B.T / n + np.eye(n), rng.uniform(0.0, 1.0 / q, size=n)


def sequences(rng, q, K, sites=N):
    """(sites, K) int8, uniform over the symbols and the gap; the first sequence starts with a gap"""
    X = rng.integers(1, q + 1, size=(sites, K)).astype(np.int8)
    X[0, 0] = q
    return np.asfortranarray(X)


@pytest.mark.parametrize("q", [21, 5])
def test_read_outs_share_one_context(g, q):  # noqa: F811
    mJ, Pi = synthetic_model(q, 77 + q)
    rng = np.random.default_rng(q)
    X300, X2, X3 = sequences(rng, q, 300), sequences(rng, q, 2), sequences(rng, q, 3)
    XA, XB = sequences(rng, q, 3, SPLIT), sequences(rng, q, 2, N - SPLIT)
    assert set(np.unique(X300)) == set(range(1, q + 1))  # every symbol, and the gap
    calls = [
        ("energies K = 300", lambda c: g.sequence_energies(mJ, Pi, X300, q, ctx=c)),
        ("mutation scan K = 2", lambda c: g.mutation_scan(mJ, Pi, X2, q, ctx=c)),
        ("pair energies 3 x 2", lambda c: g.pair_energies(mJ, Pi, XA, XB, q, what="energy", ctx=c)),
        ("energies K = 3", lambda c: g.sequence_energies(mJ, Pi, X3, q, ctx=c)),
        ("pair coupling 3 x 2", lambda c: g.pair_energies(mJ, None, XA, XB, q, what="coupling", ctx=c)),
        ("potentials K = 300", lambda c: g.mutation_scan(mJ, Pi, X300, q, what="potential", ctx=c)),
    ]
    shared = g.Context(0)
    got = [call(shared) for _, call in calls]
    shared.close()
    for (tag, call), out in zip(calls, got):
        fresh = g.Context(0)
        alone = call(fresh)
        fresh.close()
        assert np.array_equal(out, alone), tag

    E300, D2, Epair, E3, R, V300 = got
    assert_within_order_bound(E300, mJ, Pi, X300, q, "q %d, energies K = 300" % q)
    assert_within_order_bound(E3, mJ, Pi, X3, q, "q %d, energies K = 3" % q)
    _, _, dE_ref, bD = reference(mJ, Pi, X2, q)
    V_ref, bV, _, _ = reference(mJ, Pi, X300, q)
    rd, rv = ratio(D2, dE_ref, bD), ratio(V300, V_ref, bV)
    print("q %d: max |dE - dE_exact| / bound = %.3g, max |V - V_exact| / bound = %.3g" % (q, rd, rv))
    assert rd <= 1.0 and rv <= 1.0, (rd, rv)
    E_ref, bound, _, _, _ = pm.pair_energy(mJ, Pi, XA, XB, q)
    R_ref, BR = pm.coupling_gather(mJ, XA, XB, q)
    rb = pm.coupling_bound(SPLIT, N - SPLIT, BR)
    print("q %d: pair energy max err / bound %.3g, coupling max err %.3g (bound %.3g)" %
          (q, float((np.abs(Epair - E_ref) / bound).max()), float(np.abs(R - R_ref).max()), float(rb.max())))
    assert np.all(np.abs(Epair - E_ref) <= bound)
    assert np.all(np.abs(R - R_ref) <= rb)


def test_fused_read_outs_share_one_context(g):  # noqa: F811
    """The fused forms on the alignment's own sequences (the NULL forms: the halves as they lie in Z), then a plain run"""
    from gaussdca.jl_amd.synth import synth_family

    M, q = 40, 5
    Zf = np.asfortranarray(synth_family(N, M, q, seed=5).T.astype(np.int8))
    assert Zf.shape == (N, M)
    calls = [
        ("run_energies", lambda c: c.run_energies_ptr(Zf.ctypes.data, N, M, q, 0.5, -1.0)[0]),
        ("run_mutation_scan", lambda c: c.run_mutation_scan_ptr(Zf.ctypes.data, N, M, q, 0.5, -1.0)[0]),
        ("run_pair_energies", lambda c: c.run_pair_energies_ptr(Zf.ctypes.data, N, M, q, 0.5, -1.0, SPLIT)[0]),
        ("run", lambda c: c.run(Zf, q, 0.5, -1.0, g._lib.SCORE_FROB)[0]),
    ]
    shared = g.Context(0)
    got = [call(shared) for _, call in calls]
    shared.close()
    assert got[0].shape == (M,) and got[1].shape == (M, N, q) and got[2].shape == (M, M) and got[3].shape == (N, N)
    for (tag, call), out in zip(calls, got):
        fresh = g.Context(0)
        alone = call(fresh)
        fresh.close()
        assert np.all(np.isfinite(out)), tag
        assert np.array_equal(out, alone), tag
