"""Energies of sequences under the fitted Gaussian model on the device (gdca_energies*, gdca_run_energies*, sequence_energies,
gDCA_energies) against tests/energy_model.py: E(x) = 1/2 (x - Pi)' mJ (x - Pi).

No tolerance is invented here.  Operator parity uses the bound of ANY summation order of the T = N^2 + N + 1 terms,
|E - E_ref| <= 2 (T + n) u B (energy_model.order_bound; 1e-11 .. 7e-9 of |E| on the goldens, where the two CPU forms sit at 1e-14);
the fused form is held to the bar of every score comparison of this repository (score_close's rtol = 1e-6, atol_frac = 1e-9);
everything about the order of the sums is array_equal."""
import os

import numpy as np
import pytest

import energy_model as em
from gdca_testutil import assert_within_order_bound, ctx, g, golden_model, mixed_sequences  # noqa: F401 (g, ctx: fixtures)

pytestmark = pytest.mark.gpu

GOLD = ["small.fasta.gz", "large.fasta.gz"]


# ---- 1. operator parity, derived bound ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLD)
@pytest.mark.parametrize("pc", [0.8, 0.2])
def test_operator_parity_goldens(g, ctx, refdata, name, pc):
    Zo, q, mJ, Pi = golden_model(refdata, name, pc)
    rng = np.random.default_rng(11)
    X = mixed_sequences(rng, Zo, q, 64)
    E = g.sequence_energies(mJ, Pi, X, q, ctx=ctx)
    E_ref, c0, bound = assert_within_order_bound(E, mJ, Pi, X, q, "%s pc %g" % (name, pc))
    gaps = np.all(X == q, axis=0)
    assert gaps.any() and np.all(np.abs(E[gaps] - c0 / 2) <= bound[gaps])
    # the family's own sequences
    Xf = np.asfortranarray(Zo.T)
    assert_within_order_bound(g.sequence_energies(mJ, Pi, Xf, q, ctx=ctx), mJ, Pi, Xf, q, "%s pc %g, the family" % (name, pc))


# every q, N and K the issue names, none a multiple of a tile; n <= 6000
SYNTH = [(2, 1, 1), (2, 200, 64), (5, 7, 3), (5, 53, 1000), (21, 1, 3), (21, 7, 1000), (21, 53, 64), (21, 200, 1), (31, 1, 64),
         (31, 7, 1), (31, 53, 3), (31, 200, 1000)]


@pytest.mark.parametrize("q,N,K", SYNTH, ids=["q%d-N%d-K%d" % c for c in SYNTH])
def test_operator_parity_synthetic(g, ctx, q, N, K):
    from gaussdca.jl_amd.synth import synth_family

    Zo = synth_family(N, 300, q, seed=1000 * q + N)
    mJ, Pi = em.model_from_Z(Zo, q, 0.5)
    rng = np.random.default_rng(q * 1000 + N + K)
    for shift in ((0, 1, 2, 3) if K == 1 else (K % 4,)):  # (K = 1: each kind of sequence alone)
        X = mixed_sequences(rng, Zo, q, K, shift)
        E = g.sequence_energies(mJ, Pi, X, q, ctx=ctx)
        _, c0, bound = assert_within_order_bound(E, mJ, Pi, X, q, "q %d N %d K %d" % (q, N, K))
        gaps = np.all(X == q, axis=0)
        assert np.all(np.abs(E[gaps] - c0 / 2) <= bound[gaps])


# ---- 2. fused parity, the project's score bar ------------------------------------------------------------------------------------------
def energies_close(E, E_ref):
    """score_close (tests/gdca_testutil.py, rtol = 1e-6, atol_frac = 1e-9) on a vector: the helper compares the off-diagonal of a
    square matrix, so the K energies are repeated as the K rows of one -- every energy sits off the diagonal, the scale
    max |E_ref| is the vector's"""
    from gdca_testutil import score_close

    E, E_ref = np.asarray(E), np.asarray(E_ref)
    assert E.shape == E_ref.shape and E.ndim == 1 and E.size >= 2
    return score_close(np.tile(E, (E.size, 1)), np.tile(E_ref, (E.size, 1)), rtol=1e-6, atol_frac=1e-9)[0]


@pytest.mark.parametrize("name", GOLD)
@pytest.mark.parametrize("pc,theta,dedup", [(0.8, "auto", False), (0.2, 0.3, True), (0.2, "auto", False), (0.8, 0.3, True),
                                            (0.8, "auto", True), (0.2, 0.3, False)])
def test_fused_parity(g, ctx, refdata, tmp_path, name, pc, theta, dedup):
    Zo, q, mJ, Pi = golden_model(refdata, name, pc, theta, dedup)
    fasta = os.path.join(refdata, name)
    kw = dict(pseudocount=pc, theta=theta if theta != "auto" else ":auto", remove_dups=dedup, ctx=ctx)
    # sequences = None: the alignment's own sequences after the gap filter (and the deduplication)
    E = g.gDCA_energies(fasta, **kw)
    Xf = np.asfortranarray(Zo.T)
    E_ref, _, _ = em.energies_gather(mJ, Pi, Xf, q)
    print("%s: max rel %.3g" % (name, float((np.abs(E - E_ref) / np.abs(E_ref)).max())))
    assert E.shape == (Zo.shape[0],) and energies_close(E, E_ref)
    assert g.gdca.last_stats["M"] == Zo.shape[0] and g.gdca.last_stats["ms_fn"] == 0.0
    # an array
    rng = np.random.default_rng(3)
    X = mixed_sequences(rng, Zo, q, 40)
    X_ref, _, _ = em.energies_gather(mJ, Pi, X, q)
    assert energies_close(g.gDCA_energies(fasta, X, **kw), X_ref)
    # a second FASTA file: every record kept (an all-gap record too), so the energies line up with the records
    from gaussdca.jl_amd.synth import write_fasta

    path = str(tmp_path / "candidates.fasta")
    write_fasta(path, np.ascontiguousarray(X.T))
    E_file = g.gDCA_energies(fasta, path, **kw)
    assert E_file.shape == (40,) and energies_close(E_file, X_ref)


@pytest.mark.parametrize("option,value,refined", [("CHOLESKY", 2, 2), ("REFINE", 1, 1), ("SWEEP_DEBUG", 32, 0)])
def test_fused_parity_through_the_collect_time_branches(g, refdata, option, value, refined):
    """The energy stage is run AGAIN at collect time after the blocked Cholesky fallback, after a Newton-Schulz step and after the
    sweep's second attempt; each leaves -inverse in the lower triangle, and unlike FN and DI the energies see the sign."""
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    rng = np.random.default_rng(8)
    X = mixed_sequences(rng, Zo, q, 40)
    X_ref, _, _ = em.energies_gather(mJ, Pi, X, q)
    c = g.Context(0)
    try:
        c.set_option(option, value)
        fasta = os.path.join(refdata, "small.fasta.gz")
        E = g.gDCA_energies(fasta, X, ctx=c)
        st = g.gdca.last_stats
        assert st["refined"] == refined and (st["sweep_retries"] > 0) == (option == "SWEEP_DEBUG"), st
        assert energies_close(E, X_ref)
        E_own = g.gDCA_energies(fasta, ctx=c)
        assert energies_close(E_own, em.energies_gather(mJ, Pi, np.asfortranarray(Zo.T), q)[0])
    finally:
        c.close()


# ---- 3. the same model as gdca_run -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,q,pc,theta", [(400, 53, 21, 0.8, -1.0), (300, 30, 5, 0.2, 0.2)])
def test_same_model_as_gdca_run(g, ctx, M, N, q, pc, theta):
    import torch
    from gaussdca.jl_amd.synth import synth_family

    Zo = synth_family(N, M, q, seed=77 + N)
    Zf = np.asfortranarray(Zo.T)
    rng = np.random.default_rng(N)
    X = mixed_sequences(rng, Zo, q, 50)
    dZ = torch.from_numpy(Zo).cuda()
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    dE = torch.full((50,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    st = ctx.run_energies_dev(dZ.data_ptr(), N, M, q, pc, theta, dX.data_ptr(), 50, dE.data_ptr())
    E = dE.cpu().numpy()
    _, st_run = ctx.run(Zf, q, pc, theta, 0)
    for f in ("theta", "Meff", "thresh", "info", "refined", "cond_bound", "N", "M", "q", "n", "n_pad", "pair_identity_sum"):
        assert st[f] == st_run[f], (f, st[f], st_run[f])
    assert st["ms_fn"] == 0.0 and st["ms_score"] > 0.0 and st["ms_total"] >= st["ms_score"]
    # the operator chain through the library's own operators on the same Z
    Pi_true, Pij_true, _, _ = g.compute_weighted_frequencies(Zf, q, theta if theta >= 0 else ":auto", ctx=ctx)
    Pi, Pij = g.add_pseudocount(Pi_true, Pij_true, pc, q, ctx=ctx)
    mJ = g.inv_cholesky(g.compute_C(Pi, Pij, ctx=ctx), ctx=ctx)
    mJ = np.tril(mJ) + np.tril(mJ, -1).T
    E_op = g.sequence_energies(mJ, Pi, X, q, ctx=ctx)
    # they turned out bit-equal (the same inverse, the same Pi, the same order of every sum), so that is what is required
    assert np.array_equal(E, E_op), float(np.abs(E - E_op).max())


# ---- 4. order-fixed sums -----------------------------------------------------------------------------------------------------------------
def test_order_fixed_sums(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    rng = np.random.default_rng(5)
    X = mixed_sequences(rng, Zo, q, 1000, shift=3)
    E = g.sequence_energies(mJ, Pi, X, q, ctx=ctx)
    assert np.array_equal(E, g.sequence_energies(mJ, Pi, X, q, ctx=ctx))  # run to run
    x = np.asfortranarray(X[:, 417:418])
    alone = g.sequence_energies(mJ, Pi, x, q, ctx=ctx)
    for pos in (0, 999):
        Y = X.copy(order="F")
        Y[:, pos] = x[:, 0]
        assert np.array_equal(g.sequence_energies(mJ, Pi, Y, q, ctx=ctx)[pos:pos + 1], alone), pos
    assert np.array_equal(E[417:418], alone)
    # a batch beyond one workgroup's sequences: the same sequence at its two ends and in the middle
    big = np.asfortranarray(np.tile(X, (1, 5)))
    Eb = g.sequence_energies(mJ, Pi, big, q, ctx=ctx)
    assert np.array_equal(Eb, np.tile(E, 5))


# ceil(K / 2048) * ceil(N / 4) >= 2 x 256 compute units selects the eight-sequences-per-thread instances of the gather kernel (the
# s = 20 one and the generic one); fewer workgroups, the two-sequences ones.  K is no multiple of 2048: the last workgroup's tail.
@pytest.mark.parametrize("q", [21, 31])
def test_wide_and_narrow_instances_and_split_launches_give_the_same_bits(g, ctx, q):
    from gaussdca.jl_amd.synth import synth_family

    N, K = 200, 25001
    Zo = synth_family(N, 300, q, seed=4242 + q)
    mJ, Pi = em.model_from_Z(Zo, q, 0.5)
    rng = np.random.default_rng(q)
    X64 = mixed_sequences(rng, Zo, q, 64)
    E64 = g.sequence_energies(mJ, Pi, X64, q, ctx=ctx)                     # 1 x 50 workgroups: the narrow instance
    assert_within_order_bound(E64, mJ, Pi, X64, q, "q %d N %d, 64 alone" % (q, N))
    idx = rng.integers(0, 64, size=K)
    idx[:64], idx[-64:] = np.arange(64), np.arange(64)[::-1]
    big = np.asfortranarray(X64[:, idx])
    assert -(-K // 2048) * -(-N // 4) >= 512 and K % 2048
    E_big = g.sequence_energies(mJ, Pi, big, q, ctx=ctx)                   # 13 x 50 workgroups: the wide instance
    assert np.array_equal(E_big, E64[idx])
    # the same batch in several launches of the gather kernel (option ENERGY_CHUNK; by default only beyond ~2.7e5 sequences at N = 500)
    c = g.Context(0)
    try:
        for chunk in (10000, 2048 * 11 + 5, 333):                          # wide + narrow tail; wide + a 2468-sequence tail; 76 narrow launches
            c.set_option("ENERGY_CHUNK", chunk)
            assert np.array_equal(g.sequence_energies(mJ, Pi, big, q, ctx=c), E_big), chunk
    finally:
        c.close()


def test_a_wider_integer_type_is_not_wrapped_into_a_legal_symbol(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    X = np.asarray(Zo.T[:, :5], dtype=np.int64).copy()
    assert np.array_equal(g.sequence_energies(mJ, Pi, X, q, ctx=ctx), g.sequence_energies(mJ, Pi, X.astype(np.int8), q, ctx=ctx))
    X[3, 2] = 261  # (int8: 5)
    with pytest.raises(g.ArgumentError):
        g.sequence_energies(mJ, Pi, X, q, ctx=ctx)
    with pytest.raises(g.ArgumentError):
        g.gDCA_energies(os.path.join(refdata, "small.fasta.gz"), X, ctx=ctx)
    with pytest.raises(g.ArgumentError):
        g.sequence_energies(mJ, Pi, X.astype(np.float64), q, ctx=ctx)


@pytest.mark.parametrize("name", GOLD)
def test_sequences_none_equals_the_alignment_itself(g, ctx, refdata, name):
    from oracle import gdca_oracle as o

    fasta = os.path.join(refdata, name)
    Zo = o.read_fasta_alignment(fasta, 0.9)
    E_none = g.gDCA_energies(fasta, ctx=ctx)
    E_Z = g.gDCA_energies(fasta, np.asfortranarray(Zo.T), ctx=ctx)
    assert np.array_equal(E_none, E_Z)
    assert np.array_equal(E_none, g.gDCA_energies(fasta, ctx=ctx))


# ---- 5. failure modes: argument and arithmetic statuses ------------------------------------------------------------------------------
def test_failure_modes(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    rng = np.random.default_rng(9)
    X = mixed_sequences(rng, Zo, q, 10)
    good = g.sequence_energies(mJ, Pi, X, q, ctx=ctx)
    for byte in (0, q + 1, -3, 127):
        Y = X.copy(order="F")
        Y[7, 4] = byte
        with pytest.raises(g.ArgumentError):
            g.sequence_energies(mJ, Pi, Y, q, ctx=ctx)
        assert np.array_equal(g.sequence_energies(mJ, Pi, X, q, ctx=ctx), good)  # the context still works
        with pytest.raises(g.ArgumentError):
            g.gDCA_energies(os.path.join(refdata, "small.fasta.gz"), Y, ctx=ctx)
    with pytest.raises(g.ArgumentError):  # K = 0
        g.sequence_energies(mJ, Pi, X[:, :0], q, ctx=ctx)
    with pytest.raises(g.ArgumentError):  # N mismatch
        g.sequence_energies(mJ, Pi, X[:-1], q, ctx=ctx)
    with pytest.raises(g.ArgumentError):
        g.gDCA_energies(os.path.join(refdata, "small.fasta.gz"), X[:-1], ctx=ctx)
    with pytest.raises(g.ArgumentError):  # q = 32
        g.sequence_energies(np.eye(31 * 2), np.zeros(31 * 2), np.ones((2, 3), dtype=np.int8), 32, ctx=ctx)
    # straight at the C-ABI: nothing is run
    import ctypes as C

    lib, E = ctx.lib, np.full(10, np.nan)
    p = g._lib._p
    N = X.shape[0]
    assert lib.gdca_energies(ctx.h, p(mJ), p(Pi), N, q, p(X), 0, p(E)) == g._lib.GDCA_EINVAL
    assert lib.gdca_energies(ctx.h, p(mJ), p(Pi), N, 32, p(X), 10, p(E)) == g._lib.GDCA_EINVAL
    assert lib.gdca_energies(ctx.h, p(mJ), p(Pi), N, 1, p(X), 10, p(E)) == g._lib.GDCA_EINVAL
    prm = g._lib.Params(0.8, -1.0, 0, 1)
    st = g._lib.Stats()
    Zf = np.asfortranarray(Zo.T)
    assert lib.gdca_run_energies(ctx.h, p(Zf), N, Zf.shape[1], q, C.byref(prm), p(X), 0, p(E), C.byref(st)) == g._lib.GDCA_EINVAL
    assert lib.gdca_run_energies(ctx.h, p(Zf), N, Zf.shape[1], 32, C.byref(prm), p(X), 10, p(E), C.byref(st)) == g._lib.GDCA_EINVAL
    assert np.all(np.isnan(E))
    # pseudocount 0 on an alignment with a constant column: not positive definite, as gdca_run reports it
    Zc = Zf.copy(order="F")
    Zc[3, :] = 5
    with pytest.raises(g.PosDefException) as e_run:
        ctx.run(Zc, q, 0.0, -1.0, 0)
    with pytest.raises(g.PosDefException) as e_en:
        ctx.run_energies_ptr(Zc.ctypes.data, N, Zc.shape[1], q, 0.0, -1.0)
    assert e_en.value.info > 0 and e_en.value.info == e_run.value.info
    assert np.array_equal(g.sequence_energies(mJ, Pi, X, q, ctx=ctx), good)


def test_a_fused_energy_run_leaves_nothing_behind_for_the_next_score_stage(g, refdata):
    """What a score stage computes is an argument of that stage, not state an earlier run left in the context: after a
    gdca_run_energies that fails on an illegal byte of X and a good gdca_run_pair_energies, gdca_fn_dev on a known mJ and gdca_run on
    the same alignment give, on the same context, bit for bit what a fresh context gives."""
    import ctypes as C

    from gaussdca.jl_amd import devops

    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    Zf = np.asfortranarray(Zo.T)
    N, M = Zf.shape
    X = mixed_sequences(np.random.default_rng(21), Zo, q, 10)

    def fn_and_run(c):
        dmJ = g.DeviceBuffer.from_array(c, np.ascontiguousarray(mJ))
        dS = devops.compute_FN_dev(c, dmJ, N, q)
        S_fn = dS.download((N, N))
        dmJ.free()
        dS.free()
        return S_fn, c.run(Zf, q, 0.8, -1.0, 0)[0]

    used, fresh = g.Context(0), g.Context(0)
    try:
        bad = X.copy(order="F")
        bad[7, 4] = q + 1
        prm, st, E = g._lib.Params(0.8, -1.0, 0, 0), g._lib.Stats(), np.full(10, np.nan)
        p = g._lib._p
        assert used.lib.gdca_run_energies(used.h, p(Zf), N, M, q, C.byref(prm), p(bad), 10, p(E), C.byref(st)) == g._lib.GDCA_EINVAL
        split = N // 2
        XA, XB = np.asfortranarray(X[:split]), np.asfortranarray(X[split:])
        Ep, _ = used.run_pair_energies_ptr(Zf.ctypes.data, N, M, q, 0.8, -1.0, split, XA.ctypes.data, 10, XB.ctypes.data, 10)
        assert Ep.shape == (10, 10) and np.all(np.isfinite(Ep))
        S_fn, S_run = fn_and_run(used)
        S_fn0, S_run0 = fn_and_run(fresh)
    finally:
        used.close()
        fresh.close()
    assert S_fn.shape == (N, N) and np.array_equal(S_fn, S_fn0)
    assert S_run.shape == (N, N) and np.array_equal(S_run, S_run0)


# ---- 6. sanity of meaning ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLD)
def test_family_fits_better_than_random(g, ctx, refdata, name):
    from oracle import gdca_oracle as o

    fasta = os.path.join(refdata, name)
    Zo = o.read_fasta_alignment(fasta, 0.9)
    q = int(Zo.max())
    rng = np.random.default_rng(1)
    R = np.asfortranarray(rng.integers(1, q + 1, size=(Zo.shape[1], 64)).astype(np.int8))
    E_fam = g.gDCA_energies(fasta, ctx=ctx)
    E_rand = g.gDCA_energies(fasta, R, ctx=ctx)
    print("%s: family mean %.1f (%.1f .. %.1f), random min %.1f" % (name, E_fam.mean(), E_fam.min(), E_fam.max(), E_rand.min()))
    assert E_fam.mean() < E_rand.min()
