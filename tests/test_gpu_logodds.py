"""Pair log-odds on the device (gdca_pair_logodds*, gdca_pair_logodds_blocked*, gdca_run_pair_logodds*, gdca_run_partner_logodds*,
pair_logodds, gDCA_pair_logodds, gDCA_partner_logodds) against tests/logodds_model.py:

    L[a, b] = ((EmA[a] + EmB[b]) - E[a, b]) + I,     I = -1/2 ((log det C - log det C_AA) - log det C_BB).

No tolerance is invented here.  The operator form is held to the model's bar -- the sum of the bars of its parts --, the fused parts to
the bar of every score comparison of this repository (score_close's rtol = 1e-6, atol_frac = 1e-9), the fused L to 1e-6 of the
magnitudes it is a difference of; everything about the combination and the order of the sums is array_equal.  The fractions of the
bars used are printed."""
import ctypes as C
import functools

import numpy as np
import pytest

import logodds_model as lo
import pair_energy_model as pm
import partner_model as pt
from gdca_testutil import ctx, g, score_close  # noqa: F401 (g, ctx: fixtures)

pytestmark = pytest.mark.gpu


# ---- 1. the contract, operator form --------------------------------------------------------------------------------------------------------
# (q, N, split, K_A, K_B): n_A = n_B = 1 first; the last has a ragged last dword and more than one LDS segment on the B side
SHAPES = [(2, 2, 1, 1, 1), (2, 9, 8, 3, 333), (5, 7, 6, 333, 3), (21, 7, 3, 64, 64), (21, 53, 17, 333, 64), (31, 121, 60, 64, 333)]


@functools.lru_cache(maxsize=None)
def operator_model(q, N, split):
    from gaussdca.jl_amd.synth import synth_family

    Zo = synth_family(N, 300, q, seed=5000 * q + N)
    return Zo, lo.Model(Zo, q, 0.5, split, reference_logdets=False)


@pytest.fixture(scope="module")
def chunked(g):
    """contexts whose fold / gather launches take at most 128 and 333 sequences a"""
    cs = [g.Context(0).set_options(PAIR_CHUNK=k) for k in (128, 333)]
    yield cs
    for c in cs:
        c.close()


def operator_L(g, c, m, XA, XB):
    return g.pair_logodds(m.mJ, m.mJA, m.mJB, m.Pi, XA, XB, m.I, m.q, ctx=c)


@pytest.mark.parametrize("q,N,split,KA,KB", SHAPES, ids=["q%d-N%d-s%d-KA%d-KB%d" % s for s in SHAPES])
def test_operator_form(g, ctx, chunked, q, N, split, KA, KB):
    Zo, m = operator_model(q, N, split)
    if (N, split) == (121, 60):
        assert (N - split) * (q - 1) > 1020 and (N - split) % 4
    rng = np.random.default_rng(q * 1000 + N + KA + KB)
    for shift in ((0, 1, 2, 3) if KA * KB == 1 else (KA % 4,)):  # (1 x 1: each kind of sequence alone)
        XA, XB = pm.mixed_halves(rng, Zo, q, split, KA, KB, shift)
        L = operator_L(g, ctx, m, XA, XB)
        p = m.parts(XA, XB)
        frac = np.abs(L - p["L"]) / p["bar"]
        print("q %d N %d split %d %d x %d: max |L - L_ref| / bar %.3g (max bar %.3g)" % (q, N, split, KA, KB, float(frac.max()), float(p["bar"].max())))
        assert L.shape == (KA, KB) and np.all(frac <= 1.0)
        # bit for bit the expression of the four values, each from the entry point that owns it
        E = g.pair_energies(m.mJ, m.Pi, XA, XB, q, ctx=ctx)
        EmA = g.sequence_energies(m.mJA, m.PiA, XA, q, ctx=ctx)
        EmB = g.sequence_energies(m.mJB, m.PiB, XB, q, ctx=ctx)
        assert np.array_equal(L, lo.combine_f64(EmA, EmB, E, m.I))
        assert np.array_equal(operator_L(g, ctx, m, XA, XB), L)  # run to run
        for c in chunked:
            assert np.array_equal(operator_L(g, c, m, XA, XB), L)
        # ... and not on where a and b stand in their batches
        a, b = KA // 2, KB - 1
        alone = operator_L(g, ctx, m, np.asfortranarray(XA[:, a:a + 1]), np.asfortranarray(XB[:, b:b + 1]))
        assert np.array_equal(alone, L[a:a + 1, b:b + 1])


# ---- 2. blocked = full, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,N,split", [(5, 7, 6), (21, 53, 17), (31, 121, 60)])
def test_blocked_equals_full(g, ctx, chunked, q, N, split):
    from test_gpu_partner import SIZES

    Zo, m = operator_model(q, N, split)
    rng = np.random.default_rng(q * 100 + N)
    ten = (pt.offsets([s[0] for s in SIZES]), pt.offsets([s[1] for s in SIZES]))
    many = (pt.offsets(rng.integers(1, 4, size=300)), pt.offsets(rng.integers(1, 4, size=300)))
    for offA, offB in (ten, many):
        KA, KB = int(offA[-1]), int(offB[-1])
        XA, XB = pm.mixed_halves(rng, Zo, q, split, KA, KB, shift=KA % 4)
        full = operator_L(g, ctx, m, XA, XB)
        la, lb = np.repeat(np.arange(len(offA) - 1), np.diff(offA)), np.repeat(np.arange(len(offB) - 1), np.diff(offB))
        for c in [ctx] + chunked:
            blocks = g.pair_logodds_blocked(m.mJ, m.mJA, m.mJB, m.Pi, XA, XB, la, lb, m.I, q, ctx=c)
            want = pt.cut_blocks(full, offA, offB)
            assert len(blocks) == len(want) and all(np.array_equal(b, w) for b, w in zip(blocks, want)), (KA, KB)
        if offA is ten[0]:
            one = g.pair_logodds_blocked(m.mJ, m.mJA, m.mJB, m.Pi, XA, XB, np.zeros(KA, dtype=int), np.zeros(KB, dtype=int), m.I, q, ctx=ctx)
            assert len(one) == 1 and np.array_equal(one[0], full)  # one species that holds everything: the full matrix


# ---- 3. fused --------------------------------------------------------------------------------------------------------------------------------
FAMILIES = {"first": (53, 300, 21, 17), "second": (7, 200, 2, 3)}  # (N, M, q, split) of synth_family
TIMING = ("ms_", "sweep_ghz")


@functools.lru_cache(maxsize=None)
def fused_case(name, pc=0.5):
    from gaussdca.jl_amd.synth import synth_family

    N, M, q, split = FAMILIES[name]
    Zo = synth_family(N, M, q, seed=6000 + 100 * q + N)
    m = lo.Model(Zo, q, pc, split)
    XA, XB = pm.mixed_halves(np.random.default_rng(N), Zo, q, split, 21, 13)
    return Zo, np.asfortranarray(Zo.T), m, XA, XB, m.parts(XA, XB)


def close(x, ref):
    """score_close (rtol = 1e-6, atol_frac = 1e-9) on a vector or matrix of two entries or more"""
    x, ref = np.asarray(x, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()
    assert x.shape == ref.shape and x.size >= 2
    return score_close(np.tile(x, (x.size, 1)), np.tile(ref, (ref.size, 1)), rtol=1e-6, atol_frac=1e-9)[0]


def run_fused(c, Zf, q, pc, split, XA=None, XB=None):
    N, M = Zf.shape
    args = [] if XA is None else [XA.ctypes.data, XA.shape[1]]
    args = args if XB is None else (args or [None, 0]) + [XB.ctypes.data, XB.shape[1]]
    return c.run_pair_logodds_ptr(Zf.ctypes.data, N, M, q, pc, -1.0, split, *args)


def untimed(info):
    return {k: v for k, v in info.items() if k != "ms_marginals"}


def assert_fused_parts(tag, m, p, L, EmA, EmB, E, info):
    """each part at the fused-parity bar, L at 1e-6 of the magnitudes it is a difference of; the fractions used, printed"""
    assert close(EmA, p["EmA"]) and close(EmB, p["EmB"]) and close(E, p["E"])
    lds = (info["logdet"], info["logdet_A"], info["logdet_B"])
    for v, ref in zip(lds, (m.ld, m.ldA, m.ldB)):
        assert abs(v - ref) <= 1e-6 * abs(ref) + 1e-9 * abs(m.ld)
    assert abs(info["information"] - m.I) <= (1e-6 + 1e-9) * abs(m.I)
    lbar = 1e-6 * p["mag"]
    print("%s: |dL| / (1e-6 mag) %.3g, |dL| / bar %.3g, log dets |d| / bar %.3g %.3g %.3g, |dI| / bar_I %.3g" %
          (tag, float((np.abs(L - p["L"]) / lbar).max()), float((np.abs(L - p["L"]) / p["bar"]).max()), m.ref.fraction(lds[0]),
           m.refA.fraction(lds[1]), m.refB.fraction(lds[2]), abs(info["information"] - m.I) / m.bar_I))
    assert np.all(np.abs(L - p["L"]) <= lbar)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_fused_form(g, ctx, name):
    Zo, Zf, m, XA, XB, p = fused_case(name)
    N, M, q, split = FAMILIES[name]
    (L, EmA, EmB, info), st = run_fused(ctx, Zf, q, 0.5, split, XA, XB)
    lds = [ctx.last_logdet(k) for k in range(3)]
    with pytest.raises(g.ArgumentError):
        ctx.last_logdet(3)
    E, st_e = ctx.run_pair_energies_ptr(Zf.ctypes.data, N, M, q, 0.5, -1.0, split, XA.ctypes.data, XA.shape[1], XB.ctypes.data, XB.shape[1])
    # the combination, bit for bit, of values the call itself and its neighbours return
    assert info["information"] == lo.information_f64(info["logdet"], info["logdet_A"], info["logdet_B"])
    assert np.array_equal(L, lo.combine_f64(EmA, EmB, E, info["information"]))
    assert lds == [info["logdet"], info["logdet_A"], info["logdet_B"]] and ctx.last_logdet(0) == lds[0]
    assert info["refined_A"] == info["refined_B"] == 0 and info["reserved"] == 0.0
    assert 0.0 < info["ms_marginals"] < st["ms_total"] and st["ms_fn"] == 0.0 and st["ms_score"] > 0.0  # (a context times its runs by default)
    for f in st:
        if not f.startswith(TIMING):
            assert st[f] == st_e[f], (f, st[f], st_e[f])
    assert_fused_parts(name, m, p, L, EmA, EmB, E, info)
    ctx.set_timing(False)
    try:
        (L2, _, _, info2), st2 = run_fused(ctx, Zf, q, 0.5, split, XA, XB)
    finally:
        ctx.set_timing(True)
    assert np.array_equal(L2, L) and info2["ms_marginals"] == 0.0 == st2["ms_total"]  # run to run; no timeline, no times
    assert untimed(info2) == untimed(info)
    # the marginal models are the inverses of the diagonal blocks of the JOINT covariance (the joint alignment's weights, not a refit on
    # half the columns): bit for bit the library's own operators on those blocks
    Pi_true, Pij_true, _, _ = g.compute_weighted_frequencies(Zf, q, ":auto", ctx=ctx)
    Pi, Pij = g.add_pseudocount(Pi_true, Pij_true, 0.5, q, ctx=ctx)
    Cd = g.compute_C(Pi, Pij, ctx=ctx)
    nA = split * (q - 1)
    sym = lambda X: np.tril(X) + np.tril(X, -1).T  # noqa: E731
    mJA, ldA = g.inv_cholesky(np.ascontiguousarray(Cd[:nA, :nA]), ctx=ctx, return_logdet=True)
    mJB, ldB = g.inv_cholesky(np.ascontiguousarray(Cd[nA:, nA:]), ctx=ctx, return_logdet=True)
    assert (ldA, ldB) == (info["logdet_A"], info["logdet_B"])
    assert np.array_equal(EmA, g.sequence_energies(sym(mJA), Pi[:nA], XA, q, ctx=ctx))
    assert np.array_equal(EmB, g.sequence_energies(sym(mJB), Pi[nA:], XB, q, ctx=ctx))


def test_fused_on_the_alignments_own_sequences(g, ctx):
    Zo, Zf, m, _, _, _ = fused_case("first")
    N, M, q, split = FAMILIES["first"]
    ZA, ZB = np.asfortranarray(Zo[:, :split].T), np.asfortranarray(Zo[:, split:].T)
    (L, EmA, EmB, info), _ = run_fused(ctx, Zf, q, 0.5, split)
    (L_arr, EmA_arr, EmB_arr, info_arr), _ = run_fused(ctx, Zf, q, 0.5, split, ZA, ZB)
    assert L.shape == (M, M) and np.array_equal(L, L_arr) and np.array_equal(EmA, EmA_arr) and np.array_equal(EmB, EmB_arr)
    assert untimed(info) == untimed(info_arr)
    (L_a, _, _, _), _ = run_fused(ctx, Zf, q, 0.5, split, None, ZB[:, :7].copy(order="F"))
    (L_b, _, _, _), _ = run_fused(ctx, Zf, q, 0.5, split, ZA[:, :5].copy(order="F"), None)
    assert np.array_equal(L_a, L[:, :7]) and np.array_equal(L_b, L[:5, :])
    rate_L = float((L.argmax(axis=1) == np.arange(M)).mean())
    print("the family's own pairs: the native partner is the row's best L in %.3f of %d rows; mean native L %.3f, I %.3f" %
          (rate_L, M, float(np.diag(L).mean()), info["information"]))


@pytest.mark.parametrize("option,value,refined", [("CHOLESKY", 2, 2), ("REFINE", 1, 1), ("SWEEP_DEBUG", 32, 0)])
def test_fused_through_the_collect_time_branches(g, option, value, refined):
    """every one of the three fits takes the branch: the marginal fits rebuild THEIR block of the covariance"""
    Zo, Zf, m, XA, XB, p = fused_case("first")
    N, M, q, split = FAMILIES["first"]
    c = g.Context(0)
    try:
        c.set_option(option, value)
        (L, EmA, EmB, info), st = run_fused(c, Zf, q, 0.5, split, XA, XB)
        assert st["refined"] == info["refined_A"] == info["refined_B"] == refined, (st, info)
        assert (st["sweep_retries"] > 0) == (option == "SWEEP_DEBUG")
        for k, key in enumerate(("logdet", "logdet_A", "logdet_B")):
            v, src = c.last_logdet(k, return_source=True)
            assert v == info[key] and src == (1 if option == "CHOLESKY" else 0)
        E, _ = c.run_pair_energies_ptr(Zf.ctypes.data, N, M, q, 0.5, -1.0, split, XA.ctypes.data, XA.shape[1], XB.ctypes.data, XB.shape[1])
        assert info["information"] == lo.information_f64(info["logdet"], info["logdet_A"], info["logdet_B"])
        assert np.array_equal(L, lo.combine_f64(EmA, EmB, E, info["information"]))
        assert_fused_parts("%s=%s" % (option, value), m, p, L, EmA, EmB, E, info)
    finally:
        c.close()


@pytest.mark.parametrize("name", list(FAMILIES))
def test_pseudocount_one(g, ctx, name):
    Zo, Zf, m, XA, XB, p = fused_case(name, 1.0)
    N, M, q, split = FAMILIES[name]
    (L, _, _, info), _ = run_fused(ctx, Zf, q, 1.0, split, XA, XB)
    print("%s, pseudocount 1: |I| / bar %.3g, max |L| / bar %.3g" % (name, abs(info["information"]) / m.bar_I, float((np.abs(L) / p["bar"]).max())))
    assert abs(info["information"]) <= m.bar_I
    assert np.all(np.abs(L) <= p["bar"])


# ---- 4. matching -----------------------------------------------------------------------------------------------------------------------------
def test_matching_on_the_golden_family(g, ctx, tmp_path):
    from gaussdca.jl_amd.synth import write_fasta

    m, XA, XB, p = lo.family_model()
    Zfit, _ = lo.family_alignment()
    Zf = np.asfortranarray(Zfit.T)
    N, M = Zf.shape
    q, split = lo.FAMILY["q"], lo.FAMILY["split"]
    off = pt.offsets(lo.SPECIES_SIZES)
    (Lp, match, gap, info), st = ctx.run_partner_logodds_ptr(Zf.ctypes.data, N, M, q, 0.5, -1.0, split, XA.ctypes.data, 40, XB.ctypes.data, 40, off, off)
    blocks = pt.unpack(Lp, off, off)
    # the blocks are the fused full form's entries, bit for bit
    (L, _, _, info_full), _ = run_fused(ctx, Zf, q, 0.5, split, XA, XB)
    assert untimed(info) == untimed(info_full) and all(np.array_equal(b, w) for b, w in zip(blocks, pt.cut_blocks(L, off, off)))
    assert np.all(np.abs(L - p["L"]) <= 1e-6 * p["mag"])
    # match = the assignment on -L; gap by its definition: one subtraction of two entries of L
    m_dev, g_dev = g.assign_blocks([-b for b in blocks], ctx=ctx)
    local = np.split(match - np.repeat(off[:-1], np.diff(off)), off[1:-1])
    for s, (b, ml, md, gd) in enumerate(zip(blocks, local, m_dev, g_dev)):
        assert np.array_equal(ml, md) and pt.is_valid_matching(b, ml)
        want = np.array([b[a, ml[a]] - (np.delete(b[a], ml[a]).max() if b.shape[1] > 1 else -np.inf) for a in range(len(ml))])
        assert np.array_equal(gap[off[s]:off[s + 1]], want) and np.array_equal(gd, want)
        # the natives recovered are the model's wherever its second-best margin exceeds twice the bar: every species of the fixture
        blk = slice(off[s], off[s + 1])
        ref, _ = pt.assign_scipy(-p["L"][blk, blk])
        margin = pt.second_best_margin(-p["L"][blk, blk])
        assert margin > 2.0 * lo.species_bar(p["bar"][blk, blk]) + pt.solver_bar(b)
        assert np.array_equal(ml, ref), s
    assert gap[0] == np.inf  # the species of one
    # without the blocks (kept inside the context): the same matching; and the Python entry on a FASTA file, labels in the caller's order
    (none, m2, g2, _), _ = ctx.run_partner_logodds_ptr(Zf.ctypes.data, N, M, q, 0.5, -1.0, split, XA.ctypes.data, 40, XB.ctypes.data, 40, off, off,
                                                      want_blocks=False)
    assert none is None and np.array_equal(m2, match) and np.array_equal(g2, gap)
    path = str(tmp_path / "pairs.fasta")
    write_fasta(path, Zfit)
    lab = pt.species_labels(lo.SPECIES_SIZES)
    sa, sb = np.random.default_rng(3).permutation(40), np.random.default_rng(4).permutation(40)
    YA, YB = np.asfortranarray(XA[:, sa]), np.asfortranarray(XB[:, sb])
    kw = dict(pseudocount=0.5, max_gap_fraction=1.0, ctx=ctx)
    mp, gp, info_p = g.gDCA_partner_logodds(path, split, YA, YB, lab[sa], lab[sb], return_info=True, **kw)
    assert np.array_equal(sb[mp], match[sa]) and np.array_equal(gp, gap[sa])  # (a = sa[i] in the fixture's order; every a is matched)
    assert info_p["information"] == info["information"]
    Lw, iw = g.gDCA_pair_logodds(path, split, XA, XB, return_info=True, **kw)
    assert np.array_equal(Lw, L) and np.array_equal(g.gDCA_pair_logodds(path, split, XA, XB, **kw), L) and iw["logdet"] == info["logdet"]
    # the record of the use: natives recovered by the assignment on L, on E and on R
    lab_s = pt.species_labels(lo.SPECIES_SIZES)
    nat = {"L": int(np.sum(match == np.arange(40)))}
    for what in ("energy", "coupling"):
        mw, _ = g.gDCA_partner_match(path, split, XA, XB, lab_s, lab_s, what=what, **kw)
        nat[what] = int(np.sum(mw == np.arange(40)))
    print("natives recovered of 40 by the assignment on L %d, on E %d, on R %d (the model on L: %d)" %
          (nat["L"], nat["energy"], nat["coupling"], sum(int(np.sum(pt.assign_scipy(-p["L"][off[s]:off[s + 1], off[s]:off[s + 1]])[0] ==
                                                                   np.arange(off[s + 1] - off[s]))) for s in range(len(off) - 1))))


def test_a_species_beyond_assign_max_is_refused(g, ctx):
    Zo, Zf, m, _, _, _ = fused_case("second")
    N, M, q, split = FAMILIES["second"]
    p, EINVAL = g._lib._p, g._lib.GDCA_EINVAL
    K = 513
    XA, XB = pm.mixed_halves(np.random.default_rng(1), Zo, q, split, K, K)
    one = np.array([0, K], dtype=np.int32)
    prm, st = g._lib.Params(0.5, -1.0, 0, 0), g._lib.Stats()
    match, gap = np.full(K, 77, dtype=np.int32), np.full(K, 7.5)
    rc = ctx.lib.gdca_run_partner_logodds(ctx.h, p(Zf), N, M, q, C.byref(prm), split, p(XA), K, p(XB), K, p(one), p(one), 1, None, p(match), p(gap),
                                          None, C.byref(st))
    assert rc == EINVAL and np.all(match == 77) and np.all(gap == 7.5)
    two = np.array([0, 512, K], dtype=np.int32)
    rc = ctx.lib.gdca_run_partner_logodds(ctx.h, p(Zf), N, M, q, C.byref(prm), split, p(XA), K, p(XB), K, p(two), p(two), 2, None, p(match), p(gap),
                                          None, C.byref(st))
    assert rc == 0 and sorted(match[:512].tolist()) == list(range(512)) and match[512] == 512


# ---- 5. argument checks ----------------------------------------------------------------------------------------------------------------------
def test_argument_checks(g, ctx):
    q, N, split = 21, 53, 17
    Zo, m = operator_model(q, N, split)
    rng = np.random.default_rng(9)
    KA, KB = 10, 7
    XA, XB = pm.mixed_halves(rng, Zo, q, split, KA, KB)
    good = operator_L(g, ctx, m, XA, XB)
    lib, p, EINVAL = ctx.lib, g._lib._p, g._lib.GDCA_EINVAL
    L = np.full(KA * KB, np.nan)
    offA, offB = np.array([0, 4, KA], dtype=np.int32), np.array([0, 3, KB], dtype=np.int32)
    I = C.c_double(m.I)

    def op(q_=q, split_=split, ka=KA, kb=KB, mj=p(m.mJ), mja=p(m.mJA), mjb=p(m.mJB), pi=p(m.Pi), xa=p(XA), xb=p(XB), out=p(L)):
        return lib.gdca_pair_logodds(ctx.h, mj, mja, mjb, pi, N, q_, split_, xa, ka, xb, kb, I, out)

    def blocked(oa=offA, ob=offB, S=2, out=p(L), mja=p(m.mJA)):
        oa, ob = np.ascontiguousarray(oa, dtype=np.int32), np.ascontiguousarray(ob, dtype=np.int32)
        return lib.gdca_pair_logodds_blocked(ctx.h, p(m.mJ), mja, p(m.mJB), p(m.Pi), N, q, split, p(XA), KA, p(XB), KB, p(oa), p(ob), S, I, out)

    for kw in (dict(mj=None), dict(mja=None), dict(mjb=None), dict(pi=None), dict(xa=None), dict(xb=None), dict(out=None), dict(split_=0),
               dict(split_=N), dict(q_=1), dict(q_=32), dict(ka=0), dict(kb=0), dict(ka=-1)):
        assert op(**kw) == EINVAL, kw
    bad, short, late = np.array([0, 5, 4]), np.array([0, 4, KA - 1]), np.array([1, 3, KB])
    assert blocked(oa=bad) == EINVAL and blocked(oa=short) == EINVAL and blocked(ob=late) == EINVAL and blocked(S=0) == EINVAL
    assert blocked(out=None) == EINVAL and blocked(mja=None) == EINVAL
    assert lib.gdca_pair_logodds_blocked(ctx.h, p(m.mJ), p(m.mJA), p(m.mJB), p(m.Pi), N, q, split, p(XA), KA, p(XB), KB, None, p(offB), 2, I,
                                         p(L)) == EINVAL
    assert np.all(np.isnan(L))  # nothing written
    # a bad symbol is found on the device, in XA alone and in XB alone; the context still works
    prm, st = g._lib.Params(0.5, -1.0, 0, 0), g._lib.Stats()
    Zf = np.asfortranarray(Zo.T)
    M = Zf.shape[1]

    def fused(xa=XA, xb=XB, q_=q, split_=split, ka=KA, kb=KB, z=p(Zf), out=p(L), prm_=C.byref(prm)):
        return lib.gdca_run_pair_logodds(ctx.h, z, N, M, q_, prm_, split_, p(xa) if xa is not None else None, ka,
                                         p(xb) if xb is not None else None, kb, out, None, None, None, C.byref(st))

    for which in ("A", "B"):
        for byte in (0, q + 1, -3):
            YA, YB = XA.copy(order="F"), XB.copy(order="F")
            (YA if which == "A" else YB)[7, 4] = byte
            assert op(xa=p(YA), xb=p(YB)) == EINVAL and fused(xa=YA, xb=YB) == EINVAL
            with pytest.raises(g.ArgumentError):
                g.pair_logodds(m.mJ, m.mJA, m.mJB, m.Pi, YA, YB, m.I, q, ctx=ctx)
        assert np.array_equal(operator_L(g, ctx, m, XA, XB), good)
    L[:] = np.nan
    for kw in (dict(z=None), dict(out=None), dict(prm_=None), dict(split_=0), dict(split_=N), dict(q_=1), dict(q_=32), dict(ka=0), dict(kb=-2)):
        assert fused(**kw) == EINVAL, kw
    match = np.full(KA, 77, dtype=np.int32)

    def partner(oa=offA, S=2, mt=p(match)):
        oa = np.ascontiguousarray(oa, dtype=np.int32)
        return lib.gdca_run_partner_logodds(ctx.h, p(Zf), N, M, q, C.byref(prm), split, p(XA), KA, p(XB), KB, p(oa), p(offB), S, None, mt, None, None,
                                            C.byref(st))

    assert partner(oa=bad) == EINVAL and partner(oa=short) == EINVAL and partner(S=0) == EINVAL and partner(mt=None) == EINVAL
    assert np.all(np.isnan(L)) and np.all(match == 77)
    # Python's own checks
    with pytest.raises(g.ArgumentError):
        g.pair_logodds(m.mJ, m.mJA[:-1, :-1], m.mJB, m.Pi, XA, XB, m.I, q, ctx=ctx)
    with pytest.raises(g.ArgumentError):
        g.pair_logodds(m.mJ, m.mJA, m.mJB, m.Pi, XA[:, :0], XB, m.I, q, ctx=ctx)
    # a run outstanding on the context
    S_dev = g.DeviceBuffer(ctx, N * N * 8)
    Z_dev = g.DeviceBuffer.from_array(ctx, Zf)
    prm_run = g._lib.Params(0.5, -1.0, 0, 1)
    assert lib.gdca_run_dev_async(ctx.h, Z_dev.ptr, N, M, q, C.byref(prm_run), S_dev.ptr) == 0
    try:
        assert fused() == EINVAL and op() == EINVAL and partner() == EINVAL and blocked() == EINVAL
    finally:
        assert lib.gdca_run_collect(ctx.h, C.byref(st)) == 0
        S_dev.free()
        Z_dev.free()
    # the existing entry points still refuse what = 2: the log-odds has entry points of its own
    E = np.full(KA * KB, np.nan)
    assert lib.gdca_pair_energies(ctx.h, p(m.mJ), p(m.Pi), N, q, split, p(XA), KA, p(XB), KB, 2, p(E)) == EINVAL
    assert lib.gdca_run_pair_energies(ctx.h, p(Zf), N, M, q, C.byref(prm), split, p(XA), KA, p(XB), KB, 2, p(E), C.byref(st)) == EINVAL
    assert lib.gdca_pair_energies_blocked(ctx.h, p(m.mJ), p(m.Pi), N, q, split, p(XA), KA, p(XB), KB, p(offA), p(offB), 2, 2, p(E)) == EINVAL
    assert lib.gdca_run_partner_match(ctx.h, p(Zf), N, M, q, C.byref(prm), split, p(XA), KA, p(XB), KB, p(offA), p(offB), 2, 2, None, p(match), None,
                                      C.byref(st)) == EINVAL
    assert np.all(np.isnan(E)) and np.all(match == 77)
    assert fused() == 0 and partner() == 0 and np.array_equal(operator_L(g, ctx, m, XA, XB), good)


# ---- 6. a plain score run afterwards ---------------------------------------------------------------------------------------------------------
def test_a_logodds_run_leaves_nothing_behind(g):
    """after a log-odds run (its collect-time branches taken too: they rebuild the BLOCKS' covariances from the stored Pij_true), gdca_run,
    gdca_run_pair_energies and gdca_run_partner_match give, on the same context, bit for bit what a fresh context gives; and the
    log-det record is the last run's"""
    Zo, Zf, m, XA, XB, _ = fused_case("first")
    N, M, q, split = FAMILIES["first"]
    off = pt.offsets([5, 16]), pt.offsets([6, 7])

    def after(c):
        S = c.run(Zf, q, 0.5, -1.0, 0)[0]
        ld_run = c.last_logdet(0)
        with pytest.raises(g.ArgumentError):
            c.last_logdet(1)
        E = c.run_pair_energies_ptr(Zf.ctypes.data, N, M, q, 0.5, -1.0, split, XA.ctypes.data, 21, XB.ctypes.data, 13)[0]
        pm_ = c.run_partner_match_ptr(Zf.ctypes.data, N, M, q, 0.5, -1.0, split, XA.ctypes.data, 21, XB.ctypes.data, 13, *off)[0]
        Ssmall = c.run(np.asfortranarray(Zf[:9]), q, 0.8, -1.0, 0)[0]  # (a smaller family: other leading dimensions)
        return S, ld_run, E, pm_, Ssmall

    used, fresh = g.Context(0), g.Context(0)
    try:
        used.set_option("REFINE", 1)
        run_fused(used, Zf, q, 0.5, split, XA, XB)
        used.set_option("REFINE", -1)
        used.run_partner_logodds_ptr(Zf.ctypes.data, N, M, q, 0.5, -1.0, split, XA.ctypes.data, 21, XB.ctypes.data, 13, *off)
        bad = XB.copy(order="F")
        bad[3, 2] = q + 1
        with pytest.raises(g.ArgumentError):
            run_fused(used, Zf, q, 0.5, split, XA, bad)
        got, want = after(used), after(fresh)
    finally:
        used.close()
        fresh.close()
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], want[2]) and np.array_equal(got[4], want[4])
    assert all(np.array_equal(a, b) for a, b in zip(got[3], want[3]))
