"""The pair tally's skip-and-recover form (context option TALLY_SKIP, default 1): each column's most frequent symbol is left out of
the tally and its histogram row is recovered from the single-site sums.  The integer tallies are those of the full loop, so every
output must be bit for bit what TALLY_SKIP=0 gives: the fused path's scores (covariance built in the tally's epilogue, mode 1),
Pij_true of the operator path and of gdca_run_multi (mode 0), the wide TALLY_TJ=32 form and a phase batch's batched grids.
Kept small: one family per case."""
import ctypes as C
import os

import numpy as np
import pytest

from gdca_testutil import edge_family as _edge_family

pytestmark = pytest.mark.gpu

FROB, DI = 0, 1


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


def _frequencies(g, ctx, Zf, q, W):
    N, M = Zf.shape
    n = N * (q - 1)
    Pi = np.empty(n)
    Pij = np.empty((n, n), order="F")
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    ctx.check(ctx.lib.gdca_frequencies(ctx.h, ptr(Zf), N, M, q, ptr(W), float(W.sum()), ptr(Pi), ptr(Pij)))
    return Pi, Pij


def _both(ctx, fn, **opts):
    out = []
    for skip in (0, 1):
        ctx.set_options(TALLY_SKIP=skip, **opts)
        out.append(fn())
    ctx.set_options(TALLY_SKIP=1, TALLY_TJ=0)
    return out


@pytest.mark.parametrize("M,N,q,tj", [(2053, 37, 21, 0), (2053, 37, 21, 32), (1500, 29, 5, 0), (700, 45, 31, 0)],
                         ids=["q21", "q21-tj32", "q5", "q31"])
def test_pij_true_equals_full_loop(g, ctx, M, N, q, tj):
    """Operator path (gdca_frequencies: mode 0, caller-given weights): equal weights make the tie of column 3 a true tie; the
    second weight vector is random.  Also against a direct numpy tally."""
    Zf = _edge_family(M, N, q, 11 + N)
    rng = np.random.default_rng(5)
    for W in (np.ones(M), rng.random(M)):
        (Pi0, P0), (Pi1, P1) = _both(ctx, lambda: _frequencies(g, ctx, Zf, q, W), TALLY_TJ=tj)
        assert np.array_equal(Pi0, Pi1)
        assert np.array_equal(P0, P1), float(np.abs(P0 - P1).max())
        s = q - 1
        X = np.zeros((M, N * s))
        for i in range(N):
            a = Zf[i].astype(int) - 1
            ok = a < s
            X[np.nonzero(ok)[0], i * s + a[ok]] = 1.0
        ref = (X * W[:, None]).T @ X / W.sum()
        assert np.allclose(P1, ref, rtol=1e-12, atol=1e-14)


def test_fused_scores_equal_full_loop(g, ctx):
    """gdca_run (mode 1, the covariance in the tally's epilogue) at config B's shape and on the edge family, both scores, TJ 16
    and 32."""
    from gaussdca.jl_amd import synth

    fams = [(np.asfortranarray(synth.synth_family(128, 10000, 21, 0xB128).T), 0.2),
            (_edge_family(2053, 37, 21, 3), -1.0)]
    for Zf, theta in fams:
        for score, pc in ((FROB, 0.8), (DI, 0.2)):
            for tj in (0, 32):
                (S0, st0), (S1, st1) = _both(ctx, lambda: ctx.run(Zf, 21, pc, theta, score), TALLY_TJ=tj)
                assert np.array_equal(S0, S1), (Zf.shape, score, tj, float(np.abs(S0 - S1).max()))
                assert st0["Meff"] == st1["Meff"] and st0["refined"] == st1["refined"]


def test_multi_equals_full_loop(g, ctx):
    """gdca_run_multi builds every pseudocount's covariance from the stored Pij_true (mode 0)."""
    Zf = _edge_family(1200, 61, 21, 8)
    settings = [(0.8, FROB, 1), (0.2, DI, 1), (0.5, FROB, 0)]
    r0, r1 = _both(ctx, lambda: ctx.run_multi(Zf, 21, settings, -1.0))
    for (S0, _), (S1, _) in zip(r0, r1):
        assert np.array_equal(S0, S1)


def test_phase_batch_equals_full_loop(g):
    """A phase batch of mixed families (batched grids of k_tally_keep and k_pair_tally, members of different N, M and kept-list
    lengths): TALLY_SKIP=1 on every member against 0 on every member."""
    import torch

    from gaussdca.jl_amd import synth

    fams = [synth.synth_family(N, M, 21, 0xA00 + N) for N, M in ((40, 500), (130, 2000), (75, 900))]
    fams.append(np.ascontiguousarray(_edge_family(1100, 37, 21, 4).T))  # (M, N)
    Zd = [torch.from_numpy(z).cuda() for z in fams]
    cs = [g.Context(0) for _ in fams]
    res = []
    for skip in (0, 1):
        for c in cs:
            c.set_options(TALLY_SKIP=skip)
        outs = [torch.zeros((z.shape[1], z.shape[1]), dtype=torch.float64, device="cuda") for z in fams]
        g.run_dev_phased(cs, [zd.data_ptr() for zd in Zd], [z.shape[1] for z in fams], [z.shape[0] for z in fams],
                         [21] * len(fams), 0.8, -1.0, FROB, [x.data_ptr() for x in outs])
        for c in cs:
            c.collect()
        res.append([x.cpu() for x in outs])
    for k in range(len(fams)):
        assert torch.equal(res[0][k], res[1][k]), k
        assert bool(torch.isfinite(res[1][k]).all())
    for c in cs:
        c.close()
