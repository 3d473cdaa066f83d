"""Partner matching per species on the device (gdca_pair_energies_blocked*, gdca_assign_blocks*, gdca_run_partner_match*,
pair_energies_blocked, assign_blocks, gDCA_partner_match) against tests/partner_model.py.

The blocked energies are held to the full matrix bit for bit (array_equal: the contract of include/gdca.h) and, like it, to the
bounds of any summation order; the solver to scipy's total EXACTLY on integer costs and to partner_model.solver_bar on energies;
the fused form to the operator form bit for bit and to the numpy model at the bar of every score comparison here (score_close)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import energy_model as em
import pair_energy_model as pm
import partner_model as pt
from gdca_testutil import ctx, g  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

# (kA, kB) of the species of one call: empty sides, single sequences, around the groups of 8 a, around the tile of 32 b, beyond any tile
SIZES = [(0, 3), (3, 0), (1, 1), (1, 9), (7, 8), (8, 8), (9, 7), (31, 33), (33, 31), (70, 40)]
OFFA, OFFB = pt.offsets([s[0] for s in SIZES]), pt.offsets([s[1] for s in SIZES])
SHAPES = [(q, N, split) for q in (2, 5, 21, 31) for N, split in ((7, 3), (53, 17), (121, 60))]


@functools.lru_cache(maxsize=None)
def model(q, N):
    from gaussdca.jl_amd.synth import synth_family

    Zo = synth_family(N, 300, q, seed=3000 * q + N)
    return (Zo,) + tuple(em.model_from_Z(Zo, q, 0.5))


def blocked(g, c, mJ, Pi, XA, XB, offA, offB, q, what="energy"):
    """gdca_pair_energies_blocked on species-sorted sequences: the packed array"""
    offA, offB = np.ascontiguousarray(offA, dtype=np.int32), np.ascontiguousarray(offB, dtype=np.int32)
    E = np.full(pt.blocks_length(offA, offB), np.nan)
    p = g._lib._p
    w = {"energy": 1, "coupling": 0}[what]
    c.check(c.lib.gdca_pair_energies_blocked(c.h, p(mJ), p(Pi) if w else None, XA.shape[0] + XB.shape[0], q, XA.shape[0], p(XA), XA.shape[1],
                                             p(XB), XB.shape[1], p(offA), p(offB), len(offA) - 1, w, p(E)))
    return E


@pytest.fixture(scope="module")
def chunked(g):
    """contexts whose fold / gather launches take at most 128 and 333 sequences a"""
    cs = [g.Context(0).set_options(PAIR_CHUNK=k) for k in (128, 333)]
    yield cs
    for c in cs:
        c.close()


# ---- 1. blocked = full, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,N,split", SHAPES, ids=["q%d-N%d-s%d" % s for s in SHAPES])
def test_blocked_equals_full(g, ctx, chunked, q, N, split):
    Zo, mJ, Pi = model(q, N)
    if (N, split) == (121, 60) and q in (21, 31):
        assert (N - split) * (q - 1) > 1020 and (N - split) % 4  # more than one LDS segment; a ragged last dword
    rng = np.random.default_rng(q * 100 + N)
    # the ten species; then 300 species of 1..3 sequences a side (the work list)
    many_a, many_b = pt.offsets(rng.integers(1, 4, size=300)), pt.offsets(rng.integers(1, 4, size=300))
    while not all(np.any((many_a[:-1] < k) & (many_a[1:] > k)) for k in (128, 333)):  # (drawn until a species lies across each chunk size)
        many_a = pt.offsets(rng.integers(1, 4, size=300))
    for offA, offB in ((OFFA, OFFB), (many_a, many_b)):
        KA, KB = int(offA[-1]), int(offB[-1])
        XA, XB = pm.mixed_halves(rng, Zo, q, split, KA, KB, shift=KA % 4)
        for what in ("energy", "coupling"):
            full = g.pair_energies(mJ, Pi, XA, XB, q, what=what, ctx=ctx)
            want = pt.pack(pt.cut_blocks(full, offA, offB))
            got = blocked(g, ctx, mJ, Pi, XA, XB, offA, offB, q, what)
            assert np.array_equal(got, want), (what, KA, KB)
            assert np.array_equal(blocked(g, ctx, mJ, Pi, XA, XB, offA, offB, q, what), got)  # run to run
            for c in chunked:  # (KA = 163: the last species lies across a = 128; KA ~ 600: species across 128, 256, 333, ...)
                assert np.array_equal(blocked(g, c, mJ, Pi, XA, XB, offA, offB, q, what), want), what
            if offA is OFFA:
                # one species that holds everything: the full matrix
                one = blocked(g, ctx, mJ, Pi, XA, XB, [0, KA], [0, KB], q, what)
                assert np.array_equal(one.reshape((KA, KB), order="F"), full)


def test_python_wrapper_takes_labels_in_any_order(g, ctx):
    q, N, split = 21, 53, 17
    Zo, mJ, Pi = model(q, N)
    rng = np.random.default_rng(77)
    la, lb = rng.integers(0, 12, size=90) * 3 - 7, rng.integers(1, 13, size=70) * 3 - 7   # (label -7 on A only, 29 on B only)
    XA, XB = pm.mixed_halves(rng, Zo, q, split, 90, 70)
    full = g.pair_energies(mJ, Pi, XA, XB, q, ctx=ctx)
    blocks = g.pair_energies_blocked(mJ, Pi, XA, XB, la, lb, q, ctx=ctx)
    labels = g.species_blocks(la, lb)[4]
    assert len(blocks) == len(labels)
    for lab, b in zip(labels, blocks):
        ia, ib = np.nonzero(la == lab)[0], np.nonzero(lb == lab)[0]
        assert b.shape == (len(ia), len(ib)) and np.array_equal(b, full[np.ix_(ia, ib)]), lab
    assert blocks[0].shape[1] == 0 and blocks[-1].shape[0] == 0
    assert all(b.base is not None for b in blocks if b.size)  # views of one packed array


# ---- 2. parity with the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,N,split", [(21, 53, 17), (31, 121, 60)])
def test_parity_with_the_model(g, ctx, q, N, split):
    Zo, mJ, Pi = model(q, N)
    rng = np.random.default_rng(5)
    KA, KB = int(OFFA[-1]), int(OFFB[-1])
    XA, XB = pm.mixed_halves(rng, Zo, q, split, KA, KB)
    XA[:, 40], XB[:, 45] = q, q   # an all-gap a in species (31, 33), an all-gap b in it too
    R_ref, BR = pm.coupling_gather(mJ, XA, XB, q)
    E_ref, bound = pm.pair_energy(mJ, Pi, XA, XB, q)[:2]
    rb = pm.coupling_bound(split, N - split, BR)
    cut = lambda M: pt.pack(pt.cut_blocks(np.asarray(M, dtype=np.float64), OFFA, OFFB))  # noqa: E731
    R, E = blocked(g, ctx, mJ, Pi, XA, XB, OFFA, OFFB, q, "coupling"), blocked(g, ctx, mJ, Pi, XA, XB, OFFA, OFFB, q, "energy")
    errR, errE = np.abs(R - cut(R_ref)), np.abs(E - cut(E_ref))
    print("q %d N %d: coupling max err / bound %.3g, energy max err / bound %.3g" %
          (q, N, float((errR[cut(rb) > 0] / cut(rb)[cut(rb) > 0]).max()), float((errE / cut(bound)).max())))
    assert np.all(errR <= cut(rb)) and np.all(errE <= cut(bound))
    Rb = pt.unpack(R, OFFA, OFFB)[7]
    assert np.all(Rb[40 - OFFA[7], :] == 0.0) and np.all(Rb[:, 45 - OFFB[7]] == 0.0)


# ---- 3. the solver on integer costs: every sum is exact -------------------------------------------------------------------------------
INT_SHAPES = [(1, 1), (2, 2), (3, 3), (5, 9), (9, 5), (63, 63), (64, 64), (65, 65), (130, 130), (130, 64), (0, 4)]


def test_solver_on_integer_costs(g, ctx):
    rng = np.random.default_rng(2)
    blocks = [rng.integers(-2**20, 2**20 + 1, size=s).astype(np.float64) for s in INT_SHAPES]
    match, gap = g.assign_blocks(blocks, ctx=ctx)
    for Cm, m, gp in zip(blocks, match, gap):
        assert pt.is_valid_matching(Cm, m), Cm.shape
        assert pt.total_of(Cm, m) == pt.assign_scipy(Cm)[1], Cm.shape   # exactly
        assert np.array_equal(gp, pt.gap_of(Cm, m)), Cm.shape
    assert np.all(match[-1] == -1) if len(match[-1]) else True
    assert np.all(match[9][np.argsort(match[9])[:66]] == -1) and np.all(gap[9][match[9] < 0] == 0.0)  # 130 x 64: 66 unmatched, +0.0
    assert not np.any(np.signbit(gap[9][match[9] < 0]))
    # run to run, and whatever other species share the call
    again = g.assign_blocks(blocks, ctx=ctx)
    other = g.assign_blocks(blocks[::-1], ctx=ctx)
    for k in range(len(blocks)):
        assert np.array_equal(again[0][k], match[k]) and np.array_equal(again[1][k], gap[k])
        assert np.array_equal(other[0][len(blocks) - 1 - k], match[k]) and np.array_equal(other[1][len(blocks) - 1 - k], gap[k])
    # one column: the gap is +inf
    m1, g1 = g.assign_blocks([np.array([[3.0], [1.0], [2.0]])], ctx=ctx)
    assert m1[0].tolist() == [-1, 0, -1] and g1[0].tolist() == [0.0, np.inf, 0.0]
    # the row's own minimum overridden: a negative gap
    m2, g2 = g.assign_blocks([np.array([[1.0, 2.0], [1.5, 9.0]])], ctx=ctx)
    assert m2[0].tolist() == [1, 0] and g2[0].tolist() == [-1.0, 7.5]


def test_solver_ties(g, ctx):
    for shape in ((7, 9), (9, 7), (64, 64), (1, 5)):
        Cm = np.full(shape, 3.0)
        m, gp = g.assign_blocks([Cm], ctx=ctx)
        assert pt.is_valid_matching(Cm, m[0]) and pt.total_of(Cm, m[0]) == 3.0 * min(shape)
        assert np.all(gp[0][m[0] >= 0] == 0.0)
        m_again, _ = g.assign_blocks([Cm], ctx=ctx)
        assert np.array_equal(m_again[0], m[0])


def test_a_species_without_finite_costs_comes_back_unmatched(g, ctx):
    """the search indexes nothing by an undefined minimum; the other species of the call are not touched"""
    bad, good = np.array([[np.nan, np.nan], [1.0, 2.0]]), np.array([[1.0, 2.0], [1.5, 9.0]])
    m, gp = g.assign_blocks([bad, good, np.full((3, 3), np.inf)], ctx=ctx)
    assert m[0].tolist() == [-1, -1] and gp[0].tolist() == [0.0, 0.0]
    assert m[1].tolist() == [1, 0] and gp[1].tolist() == [-1.0, 7.5]
    assert m[2].tolist() == [-1, -1, -1] and gp[2].tolist() == [0.0, 0.0, 0.0]


def test_a_species_beyond_assign_max_is_refused(g, ctx):
    p = g._lib._p
    for shape in ((513, 1), (1, 513)):
        E = np.zeros(513)
        offA, offB = np.array([0, shape[0]], dtype=np.int32), np.array([0, shape[1]], dtype=np.int32)
        match, gap = np.full(shape[0], 77, dtype=np.int32), np.full(shape[0], 7.5)
        assert ctx.lib.gdca_assign_blocks(ctx.h, p(E), p(offA), p(offB), 1, p(match), p(gap)) == g._lib.GDCA_EINVAL
        assert np.all(match == 77) and np.all(gap == 7.5)   # nothing written
    m, _ = g.assign_blocks([np.arange(512.0 * 2).reshape(512, 2)], ctx=ctx)  # 512 is accepted, and the context still works
    assert pt.is_valid_matching(np.zeros((512, 2)), m[0])


# ---- 4. the solver on energies ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def family():
    Zfit, Zheld = pm.paired_family(30, 1000, 64)
    XA, XB = np.asfortranarray(Zheld[:, :30].T), np.asfortranarray(Zheld[:, 30:].T)
    return Zfit, XA, XB, pt.species_labels(pt.SPECIES_CUT)


def test_solver_on_energies(g, ctx, family):
    Zfit, XA, XB, lab = family
    mJ, Pi = em.model_from_Z(Zfit, 21, 0.5)
    blocks = g.pair_energies_blocked(mJ, Pi, XA, XB, lab, lab, 21, ctx=ctx)   # the device's own blocks
    match, gap = g.assign_blocks(blocks, ctx=ctx)
    worst = 0.0
    for b, m, gp in zip(blocks, match, gap):
        ref, total = pt.assign_scipy(b)
        bar = pt.solver_bar(b)
        used = abs(pt.total_of(b, m) - total) / bar
        worst = max(worst, used)
        print("species %2d x %2d: |total - scipy's| / bar = %.3g" % (*b.shape, used))
        assert np.array_equal(m, ref), b.shape
        assert abs(pt.total_of(b, m) - total) <= bar
        assert np.array_equal(gp, pt.gap_of(b, m))
    print("largest fraction of the solver's bar used: %.3g" % worst)
    native, by_argmin = pt.native_recovered(match), pt.native_recovered([b.argmin(axis=1) for b in blocks])
    print("native partners of 64: assignment %d, row argmin inside the species %d" % (native, by_argmin))
    assert native >= 50 and native > by_argmin


# ---- 5. fused --------------------------------------------------------------------------------------------------------------------------
def blocks_close(blocks, ref_blocks):
    """score_close (rtol = 1e-6, atol_frac = 1e-9) on the packed entries, laid out as test_gpu_pair_energy.matrices_close does"""
    from gdca_testutil import score_close

    E, E_ref = pt.pack(blocks), pt.pack(ref_blocks)
    assert E.shape == E_ref.shape and E.size >= 2
    return score_close(np.tile(E, (E.size, 1)), np.tile(E_ref, (E.size, 1)), rtol=1e-6, atol_frac=1e-9)[0]


def library_model(g, ctx, Zfit, q, pc):
    Zf = np.asfortranarray(Zfit.T)
    Pi_true, Pij_true, _, _ = g.compute_weighted_frequencies(Zf, q, ":auto", ctx=ctx)
    Pi, Pij = g.add_pseudocount(Pi_true, Pij_true, pc, q, ctx=ctx)
    mJ = g.inv_cholesky(g.compute_C(Pi, Pij, ctx=ctx), ctx=ctx)
    return np.tril(mJ) + np.tril(mJ, -1).T, Pi


def expected_in_callers_order(la, lb, labels, match, gap):
    """per-species local results -> match (index into the caller's seqs_b) and gap in the caller's order"""
    m, gp = np.full(len(la), -2, dtype=np.int64), np.full(len(la), np.nan)
    for lab, ml, gl in zip(labels, match, gap):
        ia, ib = np.nonzero(la == lab)[0], np.nonzero(lb == lab)[0]
        m[ia] = np.where(ml >= 0, ib[np.maximum(ml, 0)] if len(ib) else -1, -1)
        gp[ia] = gl
    return m, gp


@pytest.fixture(scope="module")
def fitted(family, tmp_path_factory):
    from gaussdca.jl_amd.synth import write_fasta

    path = str(tmp_path_factory.mktemp("partner") / "pairs.fasta")
    write_fasta(path, family[0])
    return path


def test_fused_equals_the_operator_form(g, ctx, family, fitted):
    Zfit, XA, XB, lab = family
    rng = np.random.default_rng(31)
    sa, sb = rng.permutation(64), rng.permutation(64)   # the caller's order: unsorted, different on the two sides
    YA, YB, la, lb = np.asfortranarray(XA[:, sa]), np.asfortranarray(XB[:, sb]), lab[sa], lab[sb]
    kw = dict(pseudocount=0.5, max_gap_fraction=1.0, ctx=ctx)
    match, gap, blocks = g.gDCA_partner_match(fitted, 30, YA, YB, la, lb, return_blocks=True, **kw)
    st = g.gdca.last_stats
    assert st["ms_fn"] == 0.0 and st["ms_score"] > 0.0 and st["ms_total"] >= st["ms_score"]
    mJ, Pi = library_model(g, ctx, Zfit, 21, 0.5)
    op_blocks = g.pair_energies_blocked(mJ, Pi, YA, YB, la, lb, 21, ctx=ctx)
    assert len(blocks) == len(op_blocks) and all(np.array_equal(b, ob) for b, ob in zip(blocks, op_blocks))
    m_want, g_want = expected_in_callers_order(la, lb, np.unique(lab), *g.assign_blocks(op_blocks, ctx=ctx))
    assert np.array_equal(match, m_want) and np.array_equal(gap, g_want)
    # the caller's order: a's native partner is the b that came from the same held-out pair
    native = int(np.sum(sb[np.maximum(match, 0)] == sa))
    assert native >= 50
    # without the blocks (kept inside the context): the same matching
    m2, g2 = g.gDCA_partner_match(fitted, 30, YA, YB, la, lb, **kw)
    assert np.array_equal(m2, match) and np.array_equal(g2, gap)
    # against the numpy model, the bar of every score comparison here
    mJ_np, Pi_np = em.model_from_Z(Zfit, 21, 0.5)
    E_np = pm.pair_energy(mJ_np, Pi_np, YA, YB, 21)[0]
    ref = [E_np[np.ix_(np.nonzero(la == s)[0], np.nonzero(lb == s)[0])] for s in np.unique(lab)]
    assert blocks_close(blocks, ref)
    # the coupling
    mc, gc, bc = g.gDCA_partner_match(fitted, 30, YA, YB, la, lb, what="coupling", return_blocks=True, **kw)
    op_c = g.pair_energies_blocked(mJ, None, YA, YB, la, lb, 21, what="coupling", ctx=ctx)
    assert all(np.array_equal(b, ob) for b, ob in zip(bc, op_c))
    assert np.array_equal(mc, expected_in_callers_order(la, lb, np.unique(lab), *g.assign_blocks(op_c, ctx=ctx))[0])


def test_fused_on_the_alignments_own_sequences(g, ctx, family, fitted):
    Zfit = family[0]
    M = Zfit.shape[0]
    lab = np.arange(M) // 8   # 125 species of 8, as the sequences lie
    kw = dict(pseudocount=0.5, max_gap_fraction=1.0, ctx=ctx)
    match, gap = g.gDCA_partner_match(fitted, 30, None, None, lab, lab, **kw)
    ZA, ZB = np.asfortranarray(Zfit[:, :30].T), np.asfortranarray(Zfit[:, 30:].T)
    m_arr, g_arr = g.gDCA_partner_match(fitted, 30, ZA, ZB, lab, lab, **kw)
    assert match.shape == (M,) and np.array_equal(match, m_arr) and np.array_equal(gap, g_arr)
    assert np.all(match // 8 == lab)   # inside the species
    # one side the alignment's own, labels unsorted on it
    rng = np.random.default_rng(1)
    lab_u = lab[rng.permutation(M)]
    m_u, g_u = g.gDCA_partner_match(fitted, 30, None, ZB, lab_u, lab, **kw)
    m_u2, g_u2 = g.gDCA_partner_match(fitted, 30, ZA, ZB, lab_u, lab, **kw)
    assert np.array_equal(m_u, m_u2) and np.array_equal(g_u, g_u2) and np.all(m_u // 8 == lab_u)
    with pytest.raises(g.ArgumentError):
        g.gDCA_partner_match(fitted, 30, None, None, lab[:-1], lab, **kw)


@pytest.mark.parametrize("option,value,refined", [("CHOLESKY", 2, 2), ("REFINE", 1, 1)])
def test_fused_through_the_collect_time_branches(g, family, fitted, option, value, refined):
    Zfit, XA, XB, lab = family
    mJ_np, Pi_np = em.model_from_Z(Zfit, 21, 0.5)
    E_np = pm.pair_energy(mJ_np, Pi_np, XA, XB, 21)[0]
    off = pt.offsets(pt.SPECIES_CUT)
    c = g.Context(0)
    try:
        c.set_option(option, value)
        match, gap, blocks = g.gDCA_partner_match(fitted, 30, XA, XB, lab, lab, pseudocount=0.5, max_gap_fraction=1.0, return_blocks=True, ctx=c)
        assert g.gdca.last_stats["refined"] == refined, g.gdca.last_stats
        assert blocks_close(blocks, pt.cut_blocks(E_np, off, off))
        want = np.concatenate([pt.assign_scipy(b)[0] + o for b, o in zip(blocks, off[:-1])])   # scipy on the device's own blocks
        assert np.array_equal(match, want)
        assert np.array_equal(gap, np.concatenate([pt.gap_of(b, m - o) for b, m, o in zip(blocks, np.split(match, off[1:-1]), off[:-1])]))
    finally:
        c.close()


# ---- 6. argument checks ----------------------------------------------------------------------------------------------------------------
def test_argument_checks(g, ctx):
    q, N, split = 21, 53, 17
    Zo, mJ, Pi = model(q, N)
    rng = np.random.default_rng(9)
    KA, KB = int(OFFA[-1]), int(OFFB[-1])
    XA, XB = pm.mixed_halves(rng, Zo, q, split, KA, KB)
    good = blocked(g, ctx, mJ, Pi, XA, XB, OFFA, OFFB, q)
    p, lib, EINVAL = g._lib._p, ctx.lib, g._lib.GDCA_EINVAL
    E = np.full(good.size, np.nan)

    def op(offA=OFFA, offB=OFFB, S=len(SIZES), e=p(E), xb=XB, what=1, pi=p(Pi)):
        offA, offB = np.ascontiguousarray(offA, dtype=np.int32), np.ascontiguousarray(offB, dtype=np.int32)
        return lib.gdca_pair_energies_blocked(ctx.h, p(mJ), pi, N, q, split, p(XA), KA, p(xb), KB, p(offA), p(offB), S, what, e)

    bad = OFFA.copy()
    bad[4], bad[5] = bad[5], bad[4]   # non-monotone
    short = OFFA.copy()
    short[-1] -= 1                    # does not end at KA
    late = OFFB.copy()
    late[0] = 1                       # does not start at 0
    assert op(offA=bad) == EINVAL and op(offA=short) == EINVAL and op(offB=late) == EINVAL and op(S=0) == EINVAL
    assert op(e=None) == EINVAL and op(pi=None) == EINVAL and op(what=2) == EINVAL
    assert lib.gdca_pair_energies_blocked(ctx.h, p(mJ), p(Pi), N, q, split, p(XA), KA, p(XB), KB, None, p(OFFB), len(SIZES), 1, p(E)) == EINVAL
    assert np.all(np.isnan(E))   # nothing written
    YB = XB.copy(order="F")
    YB[5, 100] = q + 1            # a bad symbol: found on the device
    assert op(xb=YB) == EINVAL
    with pytest.raises(g.ArgumentError):
        g.pair_energies_blocked(mJ, Pi, XA, YB, np.zeros(KA, dtype=int), np.zeros(KB, dtype=int), q, ctx=ctx)
    with pytest.raises(g.ArgumentError):
        g.pair_energies_blocked(mJ, Pi, XA, XB, np.zeros(KA - 1, dtype=int), np.zeros(KB, dtype=int), q, ctx=ctx)
    # the assignment: offsets, a NULL that is needed
    match = np.full(KA, 77, dtype=np.int32)
    assert lib.gdca_assign_blocks(ctx.h, p(good), p(bad), p(OFFB), len(SIZES), p(match), None) == EINVAL
    assert lib.gdca_assign_blocks(ctx.h, p(good), p(OFFA), p(OFFB), 0, p(match), None) == EINVAL
    assert lib.gdca_assign_blocks(ctx.h, p(good), p(OFFA), p(OFFB), len(SIZES), None, None) == EINVAL
    assert lib.gdca_assign_blocks(ctx.h, None, p(OFFA), p(OFFB), len(SIZES), p(match), None) == EINVAL
    assert np.all(match == 77)
    # the fused form
    prm, st = g._lib.Params(0.5, -1.0, 0, 0), g._lib.Stats()
    Zf = np.asfortranarray(Zo.T)
    gap = np.full(KA, 7.5)

    def fused(offA=OFFA, S=len(SIZES), m=p(match), xb=XB):
        offA = np.ascontiguousarray(offA, dtype=np.int32)
        return lib.gdca_run_partner_match(ctx.h, p(Zf), N, Zf.shape[1], q, C.byref(prm), split, p(XA), KA, p(xb), KB, p(offA), p(OFFB), S, 1,
                                          None, m, p(gap), C.byref(st))

    assert fused(offA=bad) == EINVAL and fused(offA=short) == EINVAL and fused(S=0) == EINVAL and fused(m=None) == EINVAL
    assert np.all(match == 77) and np.all(gap == 7.5)
    assert fused(xb=YB) == EINVAL
    # the context is usable afterwards
    assert fused() == 0 and np.all(match[:3] == -1) and int(np.sum(match < 0)) == sum(max(a - b, 0) for a, b in SIZES)
    assert np.array_equal(blocked(g, ctx, mJ, Pi, XA, XB, OFFA, OFFB, q), good)
