"""The mutation scan on the device (gdca_mutation_scan*, gdca_run_mutation_scan*, mutation_scan, gDCA_mutation_scan) against
tests/mutation_model.py: the site potentials V(x; i, c) and the energy changes dE(x; i, b) = V(x; i, b) - V(x; i, x_i).

No tolerance is invented here.  Operator parity uses the bound of ANY summation order, |V - V_exact| <= 2 (N + 2 + n) u B_V
(mutation_model.bound_V) and bound_V(b) + bound_V(x_i) + 2 u |dE| for the changes; the cross-check against the explicit mutants adds the
two order_bounds of tests/energy_model.py; the fused form, whose inverse is the library's and not LAPACK's, is allowed on top of the
bound what tests/test_gpu_energy.py::test_fused_parity allows for the same reason (score_close's rtol = 1e-6, atol_frac = 1e-9);
everything about the order of the sums and the relation of the two modes is array_equal."""
import os

import numpy as np
import pytest

import energy_model as em
import mutation_model as mm
from gdca_testutil import ctx, g, golden_model, mixed_sequences, mutation_reference as reference, ratio, synth_model  # noqa: F401 (g, ctx: fixtures)

pytestmark = pytest.mark.gpu

GOLD = ["small.fasta.gz", "large.fasta.gz"]


def assert_both_modes(g, ctx, mJ, Pi, X, q, tag):
    V_ref, bV, dE_ref, bD = reference(mJ, Pi, X, q)
    V = g.mutation_scan(mJ, Pi, X, q, what="potential", ctx=ctx)
    D = g.mutation_scan(mJ, Pi, X, q, what="delta", ctx=ctx)
    assert V.shape == D.shape == (X.shape[1], X.shape[0], q)
    rv, rd = ratio(V, V_ref, bV), ratio(D, dE_ref, bD)
    print("%s: max |V - V_exact| / bound = %.3g, max |dE - dE_exact| / bound = %.3g" % (tag, rv, rd))
    assert rv <= 1.0 and rd <= 1.0, (tag, rv, rd)
    return V, D


# ---- 1. operator parity, derived bounds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLD)
@pytest.mark.parametrize("pc", [0.8, 0.2])
def test_operator_parity_goldens(g, ctx, refdata, name, pc):
    Zo, q, mJ, Pi = golden_model(refdata, name, pc)
    X = mixed_sequences(np.random.default_rng(11), Zo, q, 24)
    assert np.all(X[:, 0] == q)
    assert_both_modes(g, ctx, mJ, Pi, X, q, "%s pc %g" % (name, pc))


SYNTH = [(21, 53), (5, 30), (31, 41), (21, 200)]


@pytest.mark.parametrize("q,N", SYNTH, ids=["q%d-N%d" % c for c in SYNTH])
def test_operator_parity_synthetic(g, ctx, q, N):
    Zo, q, mJ, Pi = synth_model(q, N)
    X = mixed_sequences(np.random.default_rng(q * 1000 + N), Zo, q, 36, shift=1)
    assert_both_modes(g, ctx, mJ, Pi, X, q, "q %d N %d" % (q, N))


# ---- 2. against the independent kernel: every explicit mutant through gdca_energies -----------------------------------------------------------
def test_delta_matches_the_energies_of_the_explicit_mutants(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    N = Zo.shape[1]
    assert (N, q) == (53, 21)
    X = mixed_sequences(np.random.default_rng(2), Zo, q, 3, shift=1)  # no gaps, random with gaps, a member
    D = g.mutation_scan(mJ, Pi, X, q, ctx=ctx)
    _, _, dE_ref, bD = reference(mJ, Pi, X, q)
    E_wt = g.sequence_energies(mJ, Pi, X, q, ctx=ctx)
    _, B_wt, _ = em.energies_gather(mJ, Pi, X, q)
    worst = 0.0
    for k in range(3):
        Xm = mm.single_mutants(X[:, k], q)
        E_mut = g.sequence_energies(mJ, Pi, Xm, q, ctx=ctx)
        _, B_mut, _ = em.energies_gather(mJ, Pi, Xm, q)
        diff = (E_mut - E_wt[k]).reshape(N, q)
        tol = em.order_bound(N, q, B_mut).reshape(N, q) + em.order_bound(N, q, B_wt[k]) + bD[k]
        err = np.abs(D[k] - diff)
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), (k, float((err / tol).max()))
    print("scan vs explicit mutants: max error / tolerance = %.3g" % worst)


# ---- 3. exact relations ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,N", [(21, 53), (31, 41), (5, 30)])
def test_exact_relations_of_the_two_modes(g, ctx, q, N):
    Zo, q, mJ, Pi = synth_model(q, N)
    X = mixed_sequences(np.random.default_rng(N), Zo, q, 40)
    V = g.mutation_scan(mJ, Pi, X, q, what="potential", ctx=ctx)
    D = g.mutation_scan(mJ, Pi, X, q, what="delta", ctx=ctx)
    assert np.array_equal(D, V - mm.wild_type(V, X, q))
    own = mm.wild_type(D, X, q)
    assert np.all(own == 0.0) and not np.signbit(own).any()
    assert np.all(V[:, :, q - 1] == 0.0) and not np.signbit(V[:, :, q - 1]).any()


# ---- 4. order-fixed sums -----------------------------------------------------------------------------------------------------------------------
def test_order_fixed_sums(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    rng = np.random.default_rng(5)
    X = mixed_sequences(rng, Zo, q, 1000, shift=3)
    D = g.mutation_scan(mJ, Pi, X, q, ctx=ctx)
    assert np.array_equal(D, g.mutation_scan(mJ, Pi, X, q, ctx=ctx))  # run to run
    x = np.asfortranarray(X[:, 417:418])
    alone = g.mutation_scan(mJ, Pi, x, q, ctx=ctx)
    assert np.array_equal(D[417:418], alone)
    for K in (1000, 5000):
        big = np.asfortranarray(np.tile(X, (1, K // 1000)))
        for pos in (0, K - 1):
            Y = big.copy(order="F")
            Y[:, pos] = x[:, 0]
            assert np.array_equal(g.mutation_scan(mJ, Pi, Y, q, ctx=ctx)[pos:pos + 1], alone), (K, pos)


# ceil(K / 128) * ceil(N / sites per row block) >= 2 x 256 compute units selects the 32-sequences-per-wave instances (the s = 20 one and
# the generic one); fewer workgroups, the 4-sequences ones.  K is no multiple of 128 or 16: a ragged last workgroup.
@pytest.mark.parametrize("q", [21, 31])
def test_wide_and_narrow_instances_give_the_same_bits(g, ctx, q):
    N, K = 200, 1001
    Zo, q, mJ, Pi = synth_model(q, N, seed=4242 + q)
    rng = np.random.default_rng(q)
    X64 = mixed_sequences(rng, Zo, q, 64)
    spb = 64 // (q - 1)
    assert 1 * -(-N // spb) < 512 <= -(-K // 128) * -(-N // spb) and K % 128 and K % 16
    for what in ("delta", "potential"):
        D64 = g.mutation_scan(mJ, Pi, X64, q, what=what, ctx=ctx)          # the narrow instance
        idx = rng.integers(0, 64, size=K)
        idx[:64], idx[-64:] = np.arange(64), np.arange(64)[::-1]
        big = np.asfortranarray(X64[:, idx])
        assert np.array_equal(g.mutation_scan(mJ, Pi, big, q, what=what, ctx=ctx), D64[idx]), what   # the wide instance


# ---- 5. the fused forms --------------------------------------------------------------------------------------------------------------------------
def close_to_oracle(D, ref, bound):
    """the derived bound on the oracle's model, plus what tests/test_gpu_energy.py::test_fused_parity allows for the library's inverse
    differing from LAPACK's at rounding level (score_close: rtol = 1e-6, atol_frac = 1e-9)"""
    return bool(np.all(np.abs(D - ref) <= bound + 1e-6 * np.abs(ref) + 1e-9 * np.abs(ref).max()))


@pytest.mark.parametrize("name", GOLD)
@pytest.mark.parametrize("pc,theta,dedup", [(0.8, "auto", False), (0.2, 0.3, True), (0.2, "auto", False), (0.8, 0.3, True),
                                            (0.8, "auto", True), (0.2, 0.3, False)])
def test_fused_parity(g, ctx, refdata, name, pc, theta, dedup):
    Zo, q, mJ, Pi = golden_model(refdata, name, pc, theta, dedup)
    fasta = os.path.join(refdata, name)
    kw = dict(pseudocount=pc, theta=theta if theta != "auto" else ":auto", remove_dups=dedup, ctx=ctx)
    X = mixed_sequences(np.random.default_rng(3), Zo, q, 12)
    V_ref, bV, dE_ref, bD = reference(mJ, Pi, X, q)
    D = g.gDCA_mutation_scan(fasta, X, **kw)
    assert D.shape == (12, Zo.shape[1], q) and close_to_oracle(D, dE_ref, bD)
    assert g.gdca.last_stats["ms_fn"] == 0.0 and g.gdca.last_stats["ms_score"] > 0.0
    assert close_to_oracle(g.gDCA_mutation_scan(fasta, X, what="potential", **kw), V_ref, bV)
    # sequences = None: the alignment's own sequences after the gap filter (and the deduplication) == passing them
    D_none = g.gDCA_mutation_scan(fasta, **kw)
    assert D_none.shape == (Zo.shape[0], Zo.shape[1], q) and g.gdca.last_stats["M"] == Zo.shape[0]
    assert np.array_equal(D_none, g.gDCA_mutation_scan(fasta, np.asfortranarray(Zo.T), **kw))
    Xf = np.asfortranarray(Zo[:12].T)
    _, _, dF_ref, bF = reference(mJ, Pi, Xf, q)
    assert close_to_oracle(D_none[:12], dF_ref, bF)


@pytest.mark.parametrize("M,N,q,pc,theta", [(400, 53, 21, 0.8, -1.0), (300, 30, 5, 0.2, 0.2)])
def test_fused_is_the_operator_on_the_librarys_own_model(g, ctx, M, N, q, pc, theta):
    import torch
    from gaussdca.jl_amd.synth import synth_family

    Zo = synth_family(N, M, q, seed=77 + N)
    Zf = np.asfortranarray(Zo.T)
    X = mixed_sequences(np.random.default_rng(N), Zo, q, 50)
    dZ = torch.from_numpy(Zo).cuda()
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    Pi_true, Pij_true, _, _ = g.compute_weighted_frequencies(Zf, q, theta if theta >= 0 else ":auto", ctx=ctx)
    Pi, Pij = g.add_pseudocount(Pi_true, Pij_true, pc, q, ctx=ctx)
    mJ = g.inv_cholesky(g.compute_C(Pi, Pij, ctx=ctx), ctx=ctx)
    mJ = np.tril(mJ) + np.tril(mJ, -1).T
    for what in (g._lib.MUT_DELTA, g._lib.MUT_POTENTIAL):
        dD = torch.full((50, N, q), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        st = ctx.run_mutation_scan_dev(dZ.data_ptr(), N, M, q, pc, theta, dX.data_ptr(), 50, what, dD.data_ptr())
        D = dD.cpu().numpy()
        assert st["ms_fn"] == 0.0 and st["ms_score"] > 0.0 and st["ms_total"] >= st["ms_score"]
        D_op = g.mutation_scan(mJ, Pi, X, q, what="delta" if what == g._lib.MUT_DELTA else "potential", ctx=ctx)
        assert np.array_equal(D, D_op), float(np.abs(D - D_op).max())
    _, st_run = ctx.run(Zf, q, pc, theta, 0)
    for f in ("theta", "Meff", "thresh", "info", "refined", "cond_bound", "N", "M", "q", "n", "n_pad", "pair_identity_sum"):
        assert st[f] == st_run[f], (f, st[f], st_run[f])


@pytest.mark.parametrize("option,value,refined", [("CHOLESKY", 2, 2), ("REFINE", 1, 1), ("SWEEP_DEBUG", 32, 0)])
def test_fused_parity_through_the_collect_time_branches(g, refdata, option, value, refined):
    """The scan is run AGAIN at collect time after the blocked Cholesky fallback, after a Newton-Schulz step and after the sweep's
    second attempt, as the energy targets are."""
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    X = mixed_sequences(np.random.default_rng(8), Zo, q, 12)
    V_ref, bV, dE_ref, bD = reference(mJ, Pi, X, q)
    c = g.Context(0)
    try:
        c.set_option(option, value)
        fasta = os.path.join(refdata, "small.fasta.gz")
        D = g.gDCA_mutation_scan(fasta, X, ctx=c)
        st = g.gdca.last_stats
        assert st["refined"] == refined and (st["sweep_retries"] > 0) == (option == "SWEEP_DEBUG"), st
        assert close_to_oracle(D, dE_ref, bD)
        assert close_to_oracle(g.gDCA_mutation_scan(fasta, X, what="potential", ctx=c), V_ref, bV)
    finally:
        c.close()


def test_a_fused_scan_leaves_nothing_behind(g, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    Zf = np.asfortranarray(Zo.T)
    N, M = Zf.shape
    X = mixed_sequences(np.random.default_rng(21), Zo, q, 10)
    used, fresh = g.Context(0), g.Context(0)
    try:
        D, _ = used.run_mutation_scan_ptr(Zf.ctypes.data, N, M, q, 0.8, -1.0, X.ctypes.data, 10, g._lib.MUT_DELTA)
        assert D.shape == (10, N, q) and np.all(np.isfinite(D))
        S_used = used.run(Zf, q, 0.8, -1.0, 0)[0]
        S_fresh = fresh.run(Zf, q, 0.8, -1.0, 0)[0]
    finally:
        used.close()
        fresh.close()
    assert S_used.shape == (N, N) and np.array_equal(S_used, S_fresh)


# ---- 6. failure modes ----------------------------------------------------------------------------------------------------------------------------
def test_failure_modes(g, ctx, refdata):
    import ctypes as C

    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    X = mixed_sequences(np.random.default_rng(9), Zo, q, 10)
    good = g.mutation_scan(mJ, Pi, X, q, ctx=ctx)
    for byte in (0, q + 1):
        Y = X.copy(order="F")
        Y[7, 4] = byte
        with pytest.raises(g.ArgumentError):
            g.mutation_scan(mJ, Pi, Y, q, ctx=ctx)
        assert np.array_equal(g.mutation_scan(mJ, Pi, X, q, ctx=ctx), good)  # the context still works
        with pytest.raises(g.ArgumentError):
            g.gDCA_mutation_scan(os.path.join(refdata, "small.fasta.gz"), Y, ctx=ctx)
    # straight at the C-ABI: nothing is run
    lib, D = ctx.lib, np.full((10, X.shape[0], q), np.nan)
    p = g._lib._p
    N = X.shape[0]
    EINVAL = g._lib.GDCA_EINVAL
    assert lib.gdca_mutation_scan(ctx.h, p(mJ), p(Pi), N, q, p(X), 0, 0, p(D)) == EINVAL
    assert lib.gdca_mutation_scan(ctx.h, p(mJ), p(Pi), N, q, p(X), 10, 2, p(D)) == EINVAL
    assert lib.gdca_mutation_scan(ctx.h, p(mJ), p(Pi), N, q, p(X), 10, -1, p(D)) == EINVAL
    assert lib.gdca_mutation_scan(ctx.h, p(mJ), p(Pi), N, 32, p(X), 10, 0, p(D)) == EINVAL
    assert lib.gdca_mutation_scan(ctx.h, p(mJ), p(Pi), N, 1, p(X), 10, 0, p(D)) == EINVAL
    assert lib.gdca_mutation_scan(ctx.h, None, p(Pi), N, q, p(X), 10, 0, p(D)) == EINVAL
    assert lib.gdca_mutation_scan(ctx.h, p(mJ), None, N, q, p(X), 10, 0, p(D)) == EINVAL
    assert lib.gdca_mutation_scan(ctx.h, p(mJ), p(Pi), N, q, None, 10, 0, p(D)) == EINVAL
    assert lib.gdca_mutation_scan(ctx.h, p(mJ), p(Pi), N, q, p(X), 10, 0, None) == EINVAL
    prm, st = g._lib.Params(0.8, -1.0, 0, 1), g._lib.Stats()
    Zf = np.asfortranarray(Zo.T)
    M = Zf.shape[1]
    assert lib.gdca_run_mutation_scan(ctx.h, p(Zf), N, M, q, C.byref(prm), p(X), 0, 0, p(D), C.byref(st)) == EINVAL
    assert lib.gdca_run_mutation_scan(ctx.h, p(Zf), N, M, q, C.byref(prm), p(X), 10, 7, p(D), C.byref(st)) == EINVAL
    assert lib.gdca_run_mutation_scan(ctx.h, p(Zf), N, M, 32, C.byref(prm), p(X), 10, 0, p(D), C.byref(st)) == EINVAL
    assert lib.gdca_run_mutation_scan(ctx.h, None, N, M, q, C.byref(prm), p(X), 10, 0, p(D), C.byref(st)) == EINVAL
    assert lib.gdca_run_mutation_scan(ctx.h, p(Zf), N, M, q, C.byref(prm), p(X), 10, 0, None, C.byref(st)) == EINVAL
    assert np.all(np.isnan(D))
    assert np.array_equal(g.mutation_scan(mJ, Pi, X, q, ctx=ctx), good)


# ---- 7. sanity of meaning ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLD)
def test_native_residues_sit_in_minima(g, ctx, refdata, name):
    """The family's own sequences have a larger median dE over all substitutions than uniformly random sequences (whose median is 0:
    their own symbol is as arbitrary as the target).  Checked on the numpy model first: tests/test_mutation_cpu.py."""
    from oracle import gdca_oracle as o

    fasta = os.path.join(refdata, name)
    Zo = o.read_fasta_alignment(fasta, 0.9)
    q = int(Zo.max())
    R = np.asfortranarray(np.random.default_rng(1).integers(1, q + 1, size=(Zo.shape[1], 64)).astype(np.int8))
    med_fam = float(np.median(g.gDCA_mutation_scan(fasta, ctx=ctx)))
    med_rand = float(np.median(g.gDCA_mutation_scan(fasta, R, ctx=ctx)))
    print("%s: median dE over all substitutions: family %.4g, random %.4g" % (name, med_fam, med_rand))
    assert med_fam > med_rand
