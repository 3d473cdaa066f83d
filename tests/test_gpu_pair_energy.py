"""All-pairs partner energies across a split alignment on the device (gdca_pair_energies*, gdca_run_pair_energies*, pair_energies,
gDCA_pair_energies) against tests/pair_energy_model.py:  E(a (+) b) = E(a (+) gaps) + E(gaps (+) b) - c0 / 2 + R(a, b).

No tolerance is invented here.  Operator parity uses the bounds of ANY summation order: |R - R_ref| <= 2 N_A N_B u B_R for the
coupling, energy_model.order_bound(N, q, B_cat + |c0|) for the energy; the fused form is held to the bar of every score comparison of
this repository (score_close's rtol = 1e-6, atol_frac = 1e-9); everything about the order of the sums is array_equal."""
import os

import numpy as np
import pytest

import energy_model as em
import pair_energy_model as pm
from gdca_testutil import ctx, g, golden_model  # noqa: F401 (g, ctx: fixtures)

pytestmark = pytest.mark.gpu

GOLD = ["small.fasta.gz", "large.fasta.gz"]
SPLITS = {"small.fasta.gz": (26, 1, 52), "large.fasta.gz": (20, 399)}


def assert_pair_parity(g, ctx, mJ, Pi, XA, XB, q, tag):
    """COUPLING and ENERGY of the operator form within the derived bounds; all-gap rows and columns exactly / within the marginal's"""
    NA, NB = XA.shape[0], XB.shape[0]
    R = g.pair_energies(mJ, None, XA, XB, q, what="coupling", ctx=ctx)
    E = g.pair_energies(mJ, Pi, XA, XB, q, what="energy", ctx=ctx)
    assert R.shape == E.shape == (XA.shape[1], XB.shape[1])
    R_ref, BR = pm.coupling_gather(mJ, XA, XB, q)
    E_ref, bound, c0, EA, EB = pm.pair_energy(mJ, Pi, XA, XB, q)
    rb = pm.coupling_bound(NA, NB, BR)
    errR, errE = np.abs(R - R_ref), np.abs(E - E_ref)
    print("%s: coupling max err / bound %.3g, energy max err / bound %.3g (bound / |E| <= %.3g)" %
          (tag, float((errR[rb > 0] / rb[rb > 0]).max()) if (rb > 0).any() else 0.0, float((errE / bound).max()),
           float((bound / np.abs(E_ref)).max())))
    assert np.all(errR <= rb), (tag, "coupling")
    assert np.all(errE <= bound), (tag, "energy")
    ga, gb = np.all(XA == q, axis=0), np.all(XB == q, axis=0)
    assert np.all(R[ga, :] == 0.0) and np.all(R[:, gb] == 0.0)  # B_R = 0: exactly zero
    assert np.all(np.abs(E[ga, :] - EB[None, :]) <= bound[ga, :]) and np.all(np.abs(E[:, gb] - EA[:, None]) <= bound[:, gb])
    return E, E_ref, bound


# ---- 1. operator parity, derived bounds -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLD)
@pytest.mark.parametrize("pc", [0.8, 0.2])
def test_operator_parity_goldens(g, ctx, refdata, name, pc):
    Zo, q, mJ, Pi = golden_model(refdata, name, pc)
    rng = np.random.default_rng(21)
    for split in SPLITS[name]:
        XA, XB = pm.mixed_halves(rng, Zo, q, split, 64, 3 if split != SPLITS[name][0] else 64, shift=split)
        assert_pair_parity(g, ctx, mJ, Pi, XA, XB, q, "%s pc %g split %d" % (name, pc, split))
    # the family's own halves
    split = SPLITS[name][0]
    XA, XB = np.asfortranarray(Zo[:, :split].T), np.asfortranarray(Zo[:, split:].T)
    assert_pair_parity(g, ctx, mJ, Pi, XA, XB, q, "%s pc %g, the family" % (name, pc))


# every q the issue names, N and split no multiples of any tile size (4, 64), K_A and K_B from {1, 3, 64, 1000}; n <= 6000
SYNTH = [(2, 9, 1, 1, 1), (2, 203, 101, 64, 3), (5, 7, 6, 3, 1000), (5, 53, 17, 1000, 64), (21, 2, 1, 3, 3), (21, 7, 3, 1000, 1),
         (21, 53, 52, 64, 64), (21, 201, 67, 1, 1000), (31, 2, 1, 64, 1), (31, 7, 5, 1, 3), (31, 53, 1, 3, 64), (31, 199, 90, 1000, 1000)]


@pytest.mark.parametrize("q,N,split,KA,KB", SYNTH, ids=["q%d-N%d-s%d-KA%d-KB%d" % c for c in SYNTH])
def test_operator_parity_synthetic(g, ctx, q, N, split, KA, KB):
    from gaussdca.jl_amd.synth import synth_family

    Zo = synth_family(N, 300, q, seed=2000 * q + N)
    mJ, Pi = em.model_from_Z(Zo, q, 0.5)
    rng = np.random.default_rng(q * 1000 + N + KA + KB)
    for shift in ((0, 1, 2, 3) if KA * KB == 1 else (KA % 4,)):  # (1 x 1: each kind of sequence alone)
        XA, XB = pm.mixed_halves(rng, Zo, q, split, KA, KB, shift)
        assert_pair_parity(g, ctx, mJ, Pi, XA, XB, q, "q %d N %d split %d %d x %d" % (q, N, split, KA, KB))


def test_consistency_with_sequence_energies(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    rng = np.random.default_rng(6)
    XA, XB = pm.mixed_halves(rng, Zo, q, 26, 12, 9)
    E = g.pair_energies(mJ, Pi, XA, XB, q, ctx=ctx)
    cat = pm.concatenations(XA, XB)
    E_cat = g.sequence_energies(mJ, Pi, cat, q, ctx=ctx).reshape(9, 12).T
    _, B_cat, c0 = em.energies_gather(mJ, Pi, cat, q)
    B_cat = B_cat.reshape(9, 12).T
    both = em.order_bound(53, q, B_cat + abs(c0)) + em.order_bound(53, q, B_cat)
    print("pair vs concatenation on the device: max err / (sum of bounds) %.3g" % float((np.abs(E - E_cat) / both).max()))
    assert np.all(np.abs(E - E_cat) <= both)


# ---- 2. fused parity, the project's score bar ------------------------------------------------------------------------------------------
def matrices_close(E, E_ref):
    """score_close (tests/gdca_testutil.py, rtol = 1e-6, atol_frac = 1e-9) on a K_A x K_B matrix: the helper compares the off-diagonal
    of a square matrix, so the entries are laid out as a vector repeated over the rows of one (as test_gpu_energy.energies_close)"""
    from gdca_testutil import score_close

    E, E_ref = np.asarray(E).ravel(), np.asarray(E_ref).ravel()
    assert E.shape == E_ref.shape and E.size >= 2
    return score_close(np.tile(E, (E.size, 1)), np.tile(E_ref, (E.size, 1)), rtol=1e-6, atol_frac=1e-9)[0]


@pytest.mark.parametrize("name", GOLD)
@pytest.mark.parametrize("pc,theta,dedup", [(0.8, "auto", False), (0.2, 0.3, True)])
def test_fused_parity(g, ctx, refdata, tmp_path, name, pc, theta, dedup):
    from gaussdca.jl_amd.synth import write_fasta

    Zo, q, mJ, Pi = golden_model(refdata, name, pc, theta, dedup)
    split = SPLITS[name][0]
    fasta = os.path.join(refdata, name)
    kw = dict(pseudocount=pc, theta=theta if theta != "auto" else ":auto", remove_dups=dedup, ctx=ctx)
    # seqs None: the halves of the alignment's own sequences after the gap filter (and the deduplication); only the first 40 x 40
    # block is compared with the numpy model
    E = g.gDCA_pair_energies(fasta, split, **kw)
    M = Zo.shape[0]
    assert E.shape == (M, M)
    ZA, ZB = np.asfortranarray(Zo[:40, :split].T), np.asfortranarray(Zo[:40, split:].T)
    assert matrices_close(E[:40, :40], pm.pair_energy(mJ, Pi, ZA, ZB, q)[0])
    assert g.gdca.last_stats["M"] == M and g.gdca.last_stats["ms_fn"] == 0.0
    # arrays, one half each and both; the coupling too
    rng = np.random.default_rng(3)
    XA, XB = pm.mixed_halves(rng, Zo, q, split, 20, 13)
    E_ref = pm.pair_energy(mJ, Pi, XA, XB, q)[0]
    assert matrices_close(g.gDCA_pair_energies(fasta, split, XA, XB, **kw), E_ref)
    assert matrices_close(g.gDCA_pair_energies(fasta, split, None, XB, **kw)[:40], pm.pair_energy(mJ, Pi, ZA, XB, q)[0])
    assert matrices_close(g.gDCA_pair_energies(fasta, split, XA, None, **kw)[:, :40], pm.pair_energy(mJ, Pi, XA, ZB, q)[0])
    R = g.gDCA_pair_energies(fasta, split, XA, XB, what="coupling", **kw)
    assert matrices_close(R, pm.coupling_gather(mJ, XA, XB, q)[0])
    # FASTA files of the halves: every record kept (an all-gap record too), so rows and columns line up with the records
    pa, pb = str(tmp_path / "a.fasta"), str(tmp_path / "b.fasta")
    write_fasta(pa, np.ascontiguousarray(XA.T))
    write_fasta(pb, np.ascontiguousarray(XB.T))
    E_file = g.gDCA_pair_energies(fasta, split, pa, pb, **kw)
    assert E_file.shape == (20, 13) and matrices_close(E_file, E_ref)


@pytest.mark.parametrize("option,value,refined", [("CHOLESKY", 2, 2), ("REFINE", 1, 1), ("SWEEP_DEBUG", 32, 0)])
def test_fused_parity_through_the_collect_time_branches(g, refdata, option, value, refined):
    """The pair stage is run AGAIN at collect time after the blocked Cholesky fallback, after a Newton-Schulz step and after the
    sweep's second attempt; each leaves -inverse in the lower triangle, and this stage sees the sign."""
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    rng = np.random.default_rng(8)
    XA, XB = pm.mixed_halves(rng, Zo, q, 26, 20, 13)
    E_ref = pm.pair_energy(mJ, Pi, XA, XB, q)[0]
    c = g.Context(0)
    try:
        c.set_option(option, value)
        fasta = os.path.join(refdata, "small.fasta.gz")
        E = g.gDCA_pair_energies(fasta, 26, XA, XB, ctx=c)
        st = g.gdca.last_stats
        assert st["refined"] == refined and (st["sweep_retries"] > 0) == (option == "SWEEP_DEBUG"), st
        assert matrices_close(E, E_ref)
        R = g.gDCA_pair_energies(fasta, 26, XA, XB, what="coupling", ctx=c)
        assert matrices_close(R, pm.coupling_gather(mJ, XA, XB, q)[0])
    finally:
        c.close()


# ---- 3. the same model as gdca_run -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,q,split,pc,theta", [(400, 53, 21, 26, 0.8, -1.0), (300, 30, 5, 11, 0.2, 0.2)])
def test_same_model_as_gdca_run(g, ctx, M, N, q, split, pc, theta):
    import torch
    from gaussdca.jl_amd.synth import synth_family

    Zo = synth_family(N, M, q, seed=78 + N)
    Zf = np.asfortranarray(Zo.T)
    rng = np.random.default_rng(N)
    XA, XB = pm.mixed_halves(rng, Zo, q, split, 50, 37)
    dZ = torch.from_numpy(Zo).cuda()
    dXA = torch.from_numpy(np.ascontiguousarray(XA.T)).cuda()
    dXB = torch.from_numpy(np.ascontiguousarray(XB.T)).cuda()
    # the library's own operators on the same Z
    Pi_true, Pij_true, _, _ = g.compute_weighted_frequencies(Zf, q, theta if theta >= 0 else ":auto", ctx=ctx)
    Pi, Pij = g.add_pseudocount(Pi_true, Pij_true, pc, q, ctx=ctx)
    mJ = g.inv_cholesky(g.compute_C(Pi, Pij, ctx=ctx), ctx=ctx)
    mJ = np.tril(mJ) + np.tril(mJ, -1).T
    _, st_run = ctx.run(Zf, q, pc, theta, 0)
    for what, name in ((g._lib.PAIR_ENERGY, "energy"), (g._lib.PAIR_COUPLING, "coupling")):
        dE = torch.full((37, 50), float("nan"), dtype=torch.float64, device="cuda")  # column-major 50 x 37
        torch.cuda.synchronize()
        st = ctx.run_pair_energies_dev(dZ.data_ptr(), N, M, q, pc, theta, split, dXA.data_ptr(), 50, dXB.data_ptr(), 37, what, dE.data_ptr())
        E = dE.cpu().numpy().T
        for f in ("theta", "Meff", "thresh", "info", "refined", "cond_bound", "N", "M", "q", "n", "n_pad", "pair_identity_sum"):
            assert st[f] == st_run[f], (f, st[f], st_run[f])
        assert st["ms_fn"] == 0.0 and st["ms_score"] > 0.0 and st["ms_total"] >= st["ms_score"]
        E_op = g.pair_energies(mJ, Pi, XA, XB, q, what=name, ctx=ctx)
        # the same inverse, the same Pi, the same order of every sum: bit-equal
        assert np.array_equal(E, E_op), (name, float(np.abs(E - E_op).max()))
    # Z's own halves (XA / XB NULL) against the same halves given as arrays
    dE = torch.full((M, M), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.run_pair_energies_dev(dZ.data_ptr(), N, M, q, pc, theta, split, None, 0, None, 0, g._lib.PAIR_ENERGY, dE.data_ptr())
    E_own = dE.cpu().numpy().T
    E_arr = g.pair_energies(mJ, Pi, np.asfortranarray(Zo[:, :split].T), np.asfortranarray(Zo[:, split:].T), q, ctx=ctx)
    assert np.array_equal(E_own, E_arr)


@pytest.mark.parametrize("name", GOLD)
def test_native_pairs_are_the_diagonal(g, ctx, refdata, name):
    Zo, q, mJ, Pi = golden_model(refdata, name, 0.8)
    fasta, split = os.path.join(refdata, name), SPLITS[name][0]
    N = Zo.shape[1]
    E = g.gDCA_pair_energies(fasta, split, ctx=ctx)
    E_seq = g.gDCA_energies(fasta, ctx=ctx)
    assert E.shape == (Zo.shape[0],) * 2
    _, B, c0 = em.energies_gather(mJ, Pi, np.asfortranarray(Zo.T), q)
    both = em.order_bound(N, q, B + abs(c0)) + em.order_bound(N, q, B)
    err = np.abs(np.diag(E) - E_seq)
    print("%s: diagonal vs gDCA_energies max err / (sum of bounds) %.3g" % (name, float((err / both).max())))
    assert np.all(err <= both)


# ---- 4. order-fixed sums -----------------------------------------------------------------------------------------------------------------
def test_order_fixed_sums(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    rng = np.random.default_rng(5)
    XA, XB = pm.mixed_halves(rng, Zo, q, 26, 1000, 1000, shift=3)
    for what in ("energy", "coupling"):
        E = g.pair_energies(mJ, Pi, XA, XB, q, what=what, ctx=ctx)
        assert np.array_equal(E, g.pair_energies(mJ, Pi, XA, XB, q, what=what, ctx=ctx))  # run to run
        xa, xb = np.asfortranarray(XA[:, 417:418]), np.asfortranarray(XB[:, 334:335])
        alone = g.pair_energies(mJ, Pi, xa, xb, q, what=what, ctx=ctx)
        assert alone.shape == (1, 1) and np.array_equal(E[417:418, 334:335], alone)
        for pa in (0, 999):
            for pb in (0, 999):
                YA, YB = XA.copy(order="F"), XB.copy(order="F")
                YA[:, pa], YB[:, pb] = xa[:, 0], xb[:, 0]
                got = g.pair_energies(mJ, Pi, YA, YB, q, what=what, ctx=ctx)
                assert np.array_equal(got[pa:pa + 1, pb:pb + 1], alone), (what, pa, pb)


# fold: ceil(K_A / 128) * ceil(n_B / 64) >= 2 x 256 compute units selects the 32-sequences-per-wave instance, fewer workgroups the
# 4-sequences one; gather: ceil(K_B / 512) * ceil(K_A / 8) >= 512 selects two sequences b per thread, fewer one.  Neither K is a
# multiple of a workgroup's share: the tails.
def test_wide_and_narrow_instances_and_chunks_give_the_same_bits(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    rng = np.random.default_rng(12)
    XA, XB = pm.mixed_halves(rng, Zo, q, 26, 64, 64)
    E64 = g.pair_energies(mJ, Pi, XA, XB, q, ctx=ctx)            # 1 x 9 and 8 x 1 workgroups: the narrow instances
    KA, KB = 7500, 2100
    nB = 27 * 20
    assert -(-KA // 128) * -(-nB // 64) >= 512 and -(-KB // 512) * -(-KA // 8) >= 512 and KA % 128 and KB % 512
    ia, ib = rng.integers(0, 64, size=KA), rng.integers(0, 64, size=KB)
    ia[:64], ia[-64:], ib[:64], ib[-64:] = np.arange(64), np.arange(64)[::-1], np.arange(64), np.arange(64)[::-1]
    bigA, bigB = np.asfortranarray(XA[:, ia]), np.asfortranarray(XB[:, ib])
    want = E64[np.ix_(ia, ib)]
    assert np.array_equal(g.pair_energies(mJ, Pi, bigA, bigB, q, ctx=ctx), want)   # the wide instances
    R64 = g.pair_energies(mJ, None, XA, XB, q, what="coupling", ctx=ctx)
    assert np.array_equal(g.pair_energies(mJ, None, bigA, bigB, q, what="coupling", ctx=ctx), R64[np.ix_(ia, ib)])
    # the same batch in several launches (option PAIR_CHUNK): chunks that split the batch unevenly, wide and narrow launches mixed
    c = g.Context(0)
    try:
        for chunk in (7296, 1000, 333):
            c.set_option("PAIR_CHUNK", chunk)
            assert np.array_equal(g.pair_energies(mJ, Pi, bigA, bigB, q, ctx=c), want), chunk
    finally:
        c.close()


# ---- 5. failure modes: argument and arithmetic statuses ------------------------------------------------------------------------------
def test_failure_modes(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    fasta = os.path.join(refdata, "small.fasta.gz")
    rng = np.random.default_rng(9)
    XA, XB = pm.mixed_halves(rng, Zo, q, 26, 10, 7)
    good = g.pair_energies(mJ, Pi, XA, XB, q, ctx=ctx)
    for byte in (0, q + 1, -3, 127):
        for which in ("A", "B"):
            YA, YB = XA.copy(order="F"), XB.copy(order="F")
            (YA if which == "A" else YB)[7, 4] = byte
            for what in ("energy", "coupling"):
                with pytest.raises(g.ArgumentError):
                    g.pair_energies(mJ, Pi, YA, YB, q, what=what, ctx=ctx)
            assert np.array_equal(g.pair_energies(mJ, Pi, XA, XB, q, ctx=ctx), good)  # the context still works
            with pytest.raises(g.ArgumentError):
                g.gDCA_pair_energies(fasta, 26, YA, YB, ctx=ctx)
    with pytest.raises(g.ArgumentError):  # K = 0
        g.pair_energies(mJ, Pi, XA[:, :0], XB, q, ctx=ctx)
    with pytest.raises(g.ArgumentError):
        g.pair_energies(mJ, Pi, XA, XB[:, :0], q, ctx=ctx)
    with pytest.raises(g.ArgumentError):  # widths that do not add up to the model's
        g.pair_energies(mJ, Pi, XA[:-1], XB, q, ctx=ctx)
    with pytest.raises(g.ArgumentError):
        g.gDCA_pair_energies(fasta, 26, XA[:-1], XB, ctx=ctx)
    for split in (0, 53):
        with pytest.raises(g.ArgumentError):
            g.gDCA_pair_energies(fasta, split, ctx=ctx)
    with pytest.raises(g.ArgumentError):  # q = 32
        g.pair_energies(np.eye(31 * 2), np.zeros(31 * 2), np.ones((1, 3), dtype=np.int8), np.ones((1, 3), dtype=np.int8), 32, ctx=ctx)
    # straight at the C-ABI: nothing is run, nothing is written
    import ctypes as C

    lib, E = ctx.lib, np.full(70, np.nan)
    p = g._lib._p
    N, EINVAL = 53, g._lib.GDCA_EINVAL

    def op(q_=q, split=26, KA=10, KB=7, what=1, pi=p(Pi), xa=p(XA), e=p(E)):
        return lib.gdca_pair_energies(ctx.h, p(mJ), pi, N, q_, split, xa, KA, p(XB), KB, what, e)

    assert op(KA=0) == EINVAL and op(KB=0) == EINVAL and op(split=0) == EINVAL and op(split=N) == EINVAL
    assert op(q_=32) == EINVAL and op(q_=1) == EINVAL and op(what=2) == EINVAL and op(what=-1) == EINVAL
    assert op(pi=None) == EINVAL and op(xa=None) == EINVAL and op(e=None) == EINVAL
    prm = g._lib.Params(0.8, -1.0, 0, 1)
    st = g._lib.Stats()
    Zf = np.asfortranarray(Zo.T)

    def fused(q_=q, split=26, KA=10, KB=7, what=1):
        return lib.gdca_run_pair_energies(ctx.h, p(Zf), N, Zf.shape[1], q_, C.byref(prm), split, p(XA), KA, p(XB), KB, what, p(E), C.byref(st))

    assert fused(KA=0) == EINVAL and fused(KB=0) == EINVAL and fused(split=0) == EINVAL and fused(split=N) == EINVAL
    assert fused(q_=32) == EINVAL and fused(what=2) == EINVAL
    assert np.all(np.isnan(E))
    assert op(what=0, pi=None) == 0 and not np.any(np.isnan(E))  # (the coupling needs no Pi)
    # pseudocount 0 on an alignment with a constant column: not positive definite, as gdca_run reports it
    Zc = Zf.copy(order="F")
    Zc[3, :] = 5
    with pytest.raises(g.PosDefException) as e_run:
        ctx.run(Zc, q, 0.0, -1.0, 0)
    with pytest.raises(g.PosDefException) as e_pair:
        ctx.run_pair_energies_ptr(Zc.ctypes.data, N, Zc.shape[1], q, 0.0, -1.0, 26)
    assert e_pair.value.info > 0 and e_pair.value.info == e_run.value.info
    assert np.array_equal(g.pair_energies(mJ, Pi, XA, XB, q, ctx=ctx), good)


# ---- 6. sanity of meaning ------------------------------------------------------------------------------------------------------------------
def test_native_partners_are_recovered_more_often_than_by_a_uniform_guess(g, ctx, tmp_path):
    """The paired family of test_pair_energy_cpu.test_partner_matching_on_the_numpy_model (there: 11 of 64 rows)."""
    from gaussdca.jl_amd.synth import write_fasta

    Zfit, Zheld = pm.paired_family(30, 1000, 64)
    path = str(tmp_path / "pairs.fasta")
    write_fasta(path, Zfit)
    XA, XB = np.asfortranarray(Zheld[:, :30].T), np.asfortranarray(Zheld[:, 30:].T)
    E = g.gDCA_pair_energies(path, 30, XA, XB, pseudocount=0.5, max_gap_fraction=1.0, ctx=ctx)
    rate = float((E.argmin(axis=1) == np.arange(64)).mean())
    print("native partner recovered in %.3f of 64 rows (uniform guess: %.3f)" % (rate, 1 / 64))
    assert rate > 1 / 64
