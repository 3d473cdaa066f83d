"""The pseudo-likelihood fit AT WIDTH: test_gpu_plm.py holds the kernels at M <= 40 (106 at file level), below every bound at which
they start iterating -- k_plm_tally's 16 sequences in flight and its blocks of GDCA_PLM_CHUNK_RULE = 512, plm_geometry's slabs of
whole default blocks, k_plm_nll's stride of 256, the grids of ceil(M / 256) of k_plm_nll_seq and k_plm_check_w.  Here the same
statements at M up to 1100 (the inputs and the conditions that make a case able to tell one order from another: test_plm_cpu.py), and
devops.plm_fit / gDCA_plm as the chain of their operators.  Everything is bit equality, an integer, or a bound derived where it
stands."""
import os

import numpy as np
import pytest

import bm_model as bm
import plm_model as pm
from gdca_testutil import ctx, g  # noqa: F401 (fixtures)
from test_gpu_plm import EINVAL, bits, dev_conditionals, dev_tallies, dev_tally, device_loop, same_bits, up, with_options
from test_plm_cpu import WIDTH_FIT_FAMILY, WIDTH_NLL_CASES, WIDTH_TALLY_CASES, softmax_case, width_case

pytestmark = pytest.mark.gpu
RULE = pm.CHUNK_RULE
WIDE = (5, 21, 1029)  # blocks of 512, 512, 5: the case of sections 3, 4 and 5


def chunked(g, chunk, **kv):
    return with_options(g, PLM_CHUNK=chunk, **kv)


# ---- 1. the tally at width, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q,M,chunk", WIDTH_TALLY_CASES)
def test_tally_at_width(g, N, q, M, chunk):
    """(5, 21, 1029, rule): blocks of 512, 512, 5 in the s = 20 instance, n = 100 in two row blocks.  (7, 5, 517): the generic instance,
    512 and a ragged 5.  (6, 2, 600): s = 1.  (3, 31, 100, 24): s = 30, a chunk that is no multiple of the 16 in flight -- a batch of
    16, then 8 --, a last block of 4.  (13, 21, 96, 32): chunk = 2 x 16 and M = 3 chunks exactly, the prefetch's condition at equality,
    four column groups the last with one site.  (4, 5, 49 | 48, 16): chunk = the 16 in flight, M one past whole blocks and whole blocks.
    (53, 21, 529): n = 1060, 17 row blocks the last with 36 live lanes, 512 + 17 = a batch of 16 and one."""
    W, Z, w, Meff = width_case(N, q, M)
    c = chunked(g, chunk)
    try:
        p, _ = dev_conditionals(g, c, W, Z, q)
        Pi, Pij = dev_tally(g, c, p, Z, w, Meff, q)
    finally:
        c.close()
    Pi_m, Pij_m = pm.tallies_ordered(p, Z, w, Meff, q, chunk or RULE)
    assert same_bits(Pi, Pi_m), int((bits(Pi) != bits(Pi_m)).sum())
    assert same_bits(Pij, Pij_m), int((bits(Pij) != bits(Pij_m)).sum())
    m = bm.multipliers(N, q)
    assert same_bits(Pij, Pij.T.copy()) and same_bits(np.diagonal(Pij).copy(), Pi)
    assert np.all(Pij[m == 0.0] == 0.0) and not np.signbit(Pij[m == 0.0]).any()
    # the case can tell an order from another with the device's p too (test_plm_cpu.py: with numpy's)
    Pij_1 = pm.tallies_ordered(p, Z, w, Meff, q, M)[1]
    d = int((bits(Pij_m) != bits(Pij_1)).sum())
    print("N=%d q=%d M=%d chunk=%d: %d entries of Pij are not the one-block sum's" % (N, q, M, chunk, d))
    assert d > 0


# ---- 2. nll beyond one stride ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q,M", WIDTH_NLL_CASES)
def test_nll_beyond_one_stride(g, ctx, N, q, M):
    """M = 1029 (four full trips and five threads with a fifth), 517, 257 (ONE thread with a second term) and 256 (none).  That the
    ordered sum is not the ascending one on these inputs: test_plm_cpu.py"""
    W, Z, w, Meff = width_case(N, q, M)
    _, nll_k = dev_conditionals(g, ctx, W, Z, q)
    nll = dev_tallies(g, ctx, W, Z, w, Meff, q)[2]
    want = float(pm.nll_ordered(w, nll_k, Meff))
    asc = np.float64(0.0)
    for v in w * nll_k:
        asc = asc + v
    print("M=%d: nll %.17g, the model's %.17g, k ascending %.17g" % (M, nll, want, float(asc / np.float64(Meff))))
    assert nll == want


# ---- 3. the conditionals do not depend on the batch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q", [(5, 21), (7, 5)])
def test_conditionals_do_not_depend_on_the_batch(g, ctx, N, q):
    """The 37 sequences of the softmax cases (potentials up to 700) drawn 1029 times: more than one workgroup of k_plm_nll_seq and,
    with PLM_SLAB = 512, three slabs -- nll_k + k0, the table's slab offsets --, in the q = 21 instance and the generic one.  A
    sequence's conditionals are its own whatever stands beside it: the bits of the batch of 37."""
    W, Z37 = softmax_case(N, q)
    rng = np.random.default_rng(1029 + N)
    idx = rng.integers(0, 37, WIDE[2])
    idx[:37], idx[-37:] = np.arange(37), np.arange(37)[::-1]
    Zbig = np.asfortranarray(Z37[:, idx])
    p37, nll37 = dev_conditionals(g, ctx, W, Z37, q)
    assert np.isfinite(p37).all() and np.isfinite(nll37).all()
    for slab in (0, 512):
        c = with_options(g, PLM_SLAB=slab)
        try:
            p, nll_k = dev_conditionals(g, c, W, Zbig, q)
        finally:
            c.close()
        assert same_bits(p, p37[idx]), slab
        assert same_bits(nll_k, nll37[idx]), slab


# ---- 4. the fused form, the slabs and the loop at the default chunk ------------------------------------------------------------------------------
def wide_problem():
    N, q, M = WIDE
    W0, Z, w, Meff = width_case(N, q, M)
    Pi_d, Pij_d = (x.astype(np.float64) for x in pm.frequencies(Z, w, Meff, q))
    return N, q, M, Z, w, Meff, Pi_d, Pij_d, W0


def test_fused_equals_seams_at_the_default_chunk(g):
    """PLM_SLAB 0 (one slab of 1029 rounded to 1536), 512 (three), 1024 (two), 100 (rounded up to 512: three)"""
    N, q, M = WIDE
    W, Z, w, Meff = width_case(N, q, M)
    first = None
    for slab in (0, 512, 1024, 100):
        c = with_options(g, PLM_SLAB=slab)
        try:
            p, nll_k = dev_conditionals(g, c, W, Z, q)
            Pi_s, Pij_s = dev_tally(g, c, p, Z, w, Meff, q)
            Pi_f, Pij_f, nll = dev_tallies(g, c, W, Z, w, Meff, q)
        finally:
            c.close()
        assert same_bits(Pi_s, Pi_f) and same_bits(Pij_s, Pij_f), slab
        assert nll == float(pm.nll_ordered(w, nll_k, Meff)), slab
        if first is None:
            first = (p, nll_k, Pi_f, Pij_f)
            Pi_m, Pij_m = pm.tallies_ordered(p, Z, w, Meff, q, RULE)
            assert same_bits(Pi_f, Pi_m) and same_bits(Pij_f, Pij_m)
        for a, b in zip(first, (p, nll_k, Pi_f, Pij_f)):
            assert same_bits(a, b), slab


@pytest.mark.parametrize("lam", [0.0, 0.01])
def test_loop_rule_at_the_default_chunk(g, lam):
    """test_gpu_plm.test_loop_rule (M = 27, PLM_CHUNK = 8) with PLM_CHUNK = 0 at M = 1029"""
    from gaussdca.jl_amd import devops

    prob = wide_problem()
    N, q, M, Z, w, Meff, Pi_d, Pij_d, W0 = prob
    n = N * (q - 1)
    eta = 1.0 / (N + 2 * lam)
    runs = {}
    for slab in (0, 512):
        c = chunked(g, 0, PLM_SLAB=slab)
        try:
            W, trace = device_loop(g, c, prob, W0, 3, eta, lam)
            Wa, ta = device_loop(g, c, prob, W0, 1, eta, lam)
            Wb, tb = device_loop(g, c, prob, Wa, 2, eta, lam)
            assert same_bits(W, Wb) and same_bits(trace, np.concatenate((ta, tb)))
            runs[slab] = (W, trace)
            if slab:
                continue
            # the first iteration's W is the model's step from the ordered tally of the device's own conditionals
            p, _ = dev_conditionals(g, c, W0, Z, q)
            assert same_bits(Wa, bm.update(W0, Pij_d, pm.tallies_ordered(p, Z, w, Meff, q, chunk=RULE)[1], N, q, eta, lam))
            # the caller's chain of the operator forms
            dW, dZ, dw = up(g, c, np.asfortranarray(W0)), up(g, c, Z), up(g, c, w)
            dPi_d, dPij_d = up(g, c, Pi_d), up(g, c, np.asfortranarray(Pij_d))
            rows = []
            for it in range(3):
                dPi_c, dPij_c, dnll = devops.plm_tallies_dev(c, dW, dZ, dw, Meff, N, M, q)
                out = devops.bm_readout_dev(c, dPi_d, dPij_d, dPi_c, dPij_c, N, q).download((4,))
                assert out[3] == 0.0
                out[3] = dnll.download((1,))[0]
                rows.append(out)
                devops.bm_update_dev(c, dW, dPij_d, dPij_c, N, q, eta, lam)
            assert same_bits(W, dW.download((n, n))) and same_bits(trace, np.stack(rows))
        finally:
            c.close()
    assert same_bits(runs[0][0], runs[512][0]) and same_bits(runs[0][1], runs[512][1])  # whatever the slab
    W, trace = runs[0]
    m = bm.multipliers(N, q)
    assert same_bits(W, W.T.copy()) and np.all(W[m == 0.0] == 0.0) and not np.signbit(W[m == 0.0]).any()
    assert not same_bits(W, W0) and np.isfinite(trace).all()


# ---- 5. the weights are checked past the first workgroup --------------------------------------------------------------------------------------------
def test_a_bad_weight_anywhere_is_refused(g, ctx):
    """1.5 at k = 700 (the third workgroup of k_plm_check_w), -1e-3 at k = 1028 (the fifth and last, its fifth thread), NaN at k = 256
    (the second's first thread): GDCA_EINVAL from the three entries that take weights, nothing written, the context still good"""
    from gaussdca.jl_amd import devops

    N, q, M, Z, w, Meff, Pi_d, Pij_d, W0 = wide_problem()
    n = N * (q - 1)
    rng = np.random.default_rng(5)
    mark_i, mark_ij, mark_t = rng.normal(size=n), np.asfortranarray(rng.normal(size=(n, n))), rng.normal(size=(3, 4))
    dW, dZ, dw = up(g, ctx, np.asfortranarray(W0)), up(g, ctx, Z), up(g, ctx, w)
    dPi_d, dPij_d = up(g, ctx, Pi_d), up(g, ctx, np.asfortranarray(Pij_d))
    dPi_c, dPij_c, dtrace, dnll = up(g, ctx, mark_i), up(g, ctx, mark_ij), up(g, ctx, mark_t), up(g, ctx, np.array([-7.0]))
    dp, dnll_k = devops.plm_conditionals_dev(ctx, dW, dZ, N, M, q)
    lib, h = ctx.lib, ctx.h

    def tally(w_):
        return lib.gdca_plm_tally_dev(h, dp.ptr, dZ.ptr, w_.ptr, Meff, N, M, q, dPi_c.ptr, dPij_c.ptr)

    def tallies(w_):
        return lib.gdca_plm_tallies_dev(h, dW.ptr, dZ.ptr, w_.ptr, Meff, N, M, q, dPi_c.ptr, dPij_c.ptr, dnll.ptr)

    def learn(w_):
        return lib.gdca_plm_learn_dev(h, dW.ptr, dZ.ptr, w_.ptr, Meff, dPi_d.ptr, dPij_d.ptr, N, M, q, 3, 0.1, 0.01, dtrace.ptr)

    for k, v in ((700, 1.5), (1028, -1e-3), (256, float("nan"))):
        bad = w.copy()
        bad[k] = v
        dbad = up(g, ctx, bad)
        assert [f(dbad) for f in (tally, tallies, learn)] == [EINVAL] * 3, (k, v)
        dbad.free()
    assert same_bits(dW.download((n, n)), np.asfortranarray(W0))
    assert same_bits(dPi_c.download((n,)), mark_i) and same_bits(dPij_c.download((n, n)), mark_ij)
    assert same_bits(dtrace.download((3, 4), order="C"), mark_t) and dnll.download((1,))[0] == -7.0
    # ... and the next good calls succeed
    assert [f(dw) for f in (tally, tallies, learn)] == [0] * 3
    assert not same_bits(dW.download((n, n)), np.asfortranarray(W0)) and not same_bits(dPij_c.download((n, n)), mark_ij)
    assert np.isfinite(dtrace.download((3, 4), order="C")).all()


# ---- 6. plm_fit / gDCA_plm is the chain of its operators ------------------------------------------------------------------------------------------
FASTA = "small.fasta.gz"  # N = 53, q = 21, M = 106 (98 without duplicates): one block of the rule
FIT_ITER = 3
FIT_CASES = [dict(), dict(init="gaussian"), dict(target_pseudocount=0.1), dict(eta=0.05), dict(theta=0.3), dict(remove_dups=True),
             dict(theta=0.2)]
FIT_IDS = ["default", "gaussian", "target-0.1", "eta-0.05", "theta-0.3", "dedup", "theta-0.2"]
FAMILIES = ["small", "synth"]
# remove_dups is the file level's alone.  theta = 0.2 on the synthetic family alone: there theta = 0.3 is a neighbourhood of
# floor(0.3 x 12) = 3 differing sites, and :auto's theta, 0.2967, is the same 3 -- the same weights, so that case must REPEAT the
# default's bits, and 0.2 (2 sites) is the case that has to differ (test_plm_cpu.test_width_fit_family_is_three_blocks_of_the_rule)
FIT_PARAMS = [(f, kw) for f in FAMILIES for kw in FIT_CASES if kw != (dict(theta=0.2) if f == "small" else dict(remove_dups=True))]
SAME_NEIGHBOURHOOD = ("synth", 0.3)
FIT_PARAM_IDS = ["%s-%s" % (f, FIT_IDS[FIT_CASES.index(kw)]) for f, kw in FIT_PARAMS]
_fits, _chains = {}, {}


def fit_family(g, refdata, which, remove_dups=False):
    """(Z (N, M), N, M, q): the golden family as gDCA_plm reads it, or synth_family(12, 1100, 5, 11) -- three blocks of the rule,
    reweighted weights below 1 (test_plm_cpu.test_width_fit_family_is_three_blocks_of_the_rule)"""
    if which == "small":
        Z = g.read_fasta_alignment(os.path.join(refdata, FASTA), 0.9)
        if remove_dups:
            Z, _ = g.remove_duplicate_sequences(Z)
    else:
        from gaussdca.jl_amd.synth import synth_family

        N, M, q, seed = WIDTH_FIT_FAMILY
        Z = np.asfortranarray(synth_family(N, M, q, seed).T)
    return (Z,) + Z.shape + (int(Z.max()),)


def fit_of(g, ctx, refdata, which, n_iter=FIT_ITER, **kw):
    """gDCA_plm on the golden family, devops.plm_fit on the synthetic one, once per set of arguments"""
    from gaussdca.jl_amd import devops

    key = (which, n_iter) + tuple(sorted(kw.items()))
    if key not in _fits:
        if which == "small":
            _fits[key] = g.gDCA_plm(os.path.join(refdata, FASTA), n_iter, ctx=ctx, **kw)
        else:
            Z, N, M, q = fit_family(g, refdata, which)
            _fits[key] = devops.plm_fit(Z, q, n_iter, ctx=ctx, **kw)
    return _fits[key]


def operator_chain(g, ctx, refdata, which, init="independent", target_pseudocount=0.0, eta=None, theta=":auto", remove_dups=False,
                   lam=0.01, pseudocount=0.8):
    """What devops.plm_fit documents, step by step with the HOST operator forms: the weighted frequencies, add_pseudocount twice from the
    same true tallies, the start (potts_independent in numpy, or compute_C, inv_cholesky, potts_from_gaussian), eta = 1 / (N + 2 lam),
    plm_learn -> a dict, made once per case"""
    key = (which, init, target_pseudocount, eta, theta, remove_dups)
    if key not in _chains:
        Z, N, M, q = fit_family(g, refdata, which, remove_dups)
        Pi_t, Pij_t, Meff, wts = g.compute_weighted_frequencies(Z, q, theta, ctx=ctx)
        Pi_d, Pij_d = g.add_pseudocount(Pi_t, Pij_t, target_pseudocount, q, ctx=ctx)
        Pi, Pij = g.add_pseudocount(Pi_t, Pij_t, pseudocount, q, ctx=ctx)
        if init == "gaussian":
            W0 = g.potts_from_gaussian(g.inv_cholesky(g.compute_C(Pi, Pij, ctx=ctx), ctx=ctx), Pi, q, ctx=ctx)
        else:
            W0 = bm.potts_independent(Pi, N, q)
        step = 1.0 / (N + 2 * lam) if eta is None else eta
        W, trace = g.plm_learn(W0, Z, wts, Meff, Pi_d, Pij_d, FIT_ITER, q, eta=step, lam=lam, ctx=ctx)
        _chains[key] = dict(Z=Z, N=N, M=M, q=q, Meff=Meff, wts=wts, Pi_d=Pi_d, Pij_d=Pij_d, W0=W0, W=W, trace=trace, eta=step, lam=lam)
    return _chains[key]


@pytest.mark.parametrize("which,kw", FIT_PARAMS, ids=FIT_PARAM_IDS)
def test_fit_is_the_chain_of_the_operators(g, ctx, refdata, which, kw):
    W, trace = fit_of(g, ctx, refdata, which, **kw)
    ref = operator_chain(g, ctx, refdata, which, **kw)
    N, q, M = ref["N"], ref["q"], ref["M"]
    n = N * (q - 1)
    if which == "small":
        assert (N, q, M) == (53, 21, 98 if kw.get("remove_dups") else 106)
    else:
        assert (N, q, M) == (12, 5, 1100) and M > 2 * RULE and ref["wts"].max() <= 1 and (ref["wts"] < 1).any() and ref["Meff"] < M
    assert W.shape == (n, n) and trace.shape == (FIT_ITER, 4)
    assert same_bits(trace, ref["trace"]), (trace, ref["trace"])
    assert same_bits(W, ref["W"]), int((bits(W) != bits(ref["W"])).sum())
    m = bm.multipliers(N, q)
    assert same_bits(W, W.T.copy()) and np.all(W[m == 0.0] == 0.0) and not np.signbit(W[m == 0.0]).any()
    assert np.isfinite(trace).all() and not same_bits(W, ref["W0"])
    print("%s %s: trace\n%s" % (which, kw, trace))
    if kw:  # the case's argument matters: other bits than the default's
        base, base_ref = fit_of(g, ctx, refdata, which), operator_chain(g, ctx, refdata, which)
        if (which, kw.get("theta")) == SAME_NEIGHBOURHOOD:  # theta reaches the fit through the neighbourhood's integer alone
            assert same_bits(ref["wts"], base_ref["wts"]) and ref["Meff"] == base_ref["Meff"]
            assert same_bits(W, base[0]) and same_bits(trace, base[1])
            return
        assert not same_bits(W, base[0]) and not same_bits(trace, base[1])
        if "theta" in kw:
            assert not same_bits(ref["wts"], base_ref["wts"]) and ref["Meff"] != base_ref["Meff"]
        if "target_pseudocount" in kw:  # ... and it moves the data's side alone: the same start
            assert same_bits(ref["W0"], base_ref["W0"]) and not same_bits(ref["Pij_d"], base_ref["Pij_d"])
        if "eta" in kw:
            assert same_bits(ref["W0"], base_ref["W0"]) and same_bits(ref["Pij_d"], base_ref["Pij_d"]) and ref["eta"] != base_ref["eta"]


@pytest.mark.parametrize("which", FAMILIES)
def test_scores_of_the_fit(g, ctx, refdata, which):
    """scores=True: the third entry of plm_fit is APC(FN(W)) of the host forms bit for bit, gDCA_plm's the ranking of it entry for entry"""
    from gaussdca.jl_amd import devops

    Z, N, M, q = fit_family(g, refdata, which)
    base = fit_of(g, ctx, refdata, which)
    W, trace, S = devops.plm_fit(Z, q, FIT_ITER, scores=True, ctx=ctx)
    assert same_bits(W, base[0]) and same_bits(trace, base[1])
    want = g.correct_APC(g.compute_FN(W, q, ctx=ctx), ctx=ctx)
    assert S.shape == (N, N) and same_bits(S, want) and np.isfinite(S).all()
    if which == "small":
        sep = 4
        Wf, tf, R = g.gDCA_plm(os.path.join(refdata, FASTA), FIT_ITER, scores=True, min_separation=sep, ctx=ctx)
        assert same_bits(Wf, W) and same_bits(tf, trace)
        rank = g.compute_ranking(want, sep)
        assert len(R) == len(rank) == (N - sep) * (N - sep + 1) // 2
        assert np.array_equal(R.i, rank.i) and np.array_equal(R.j, rank.j) and same_bits(R.score, rank.score)
        assert np.all(np.diff(R.score) <= 0)


ADAPT_ITER, ADAPT_ETA = 14, 4.0


@pytest.mark.parametrize("which", FAMILIES)
def test_adaptive_fit_is_the_adaptive_loop(g, ctx, refdata, which):
    """adapt=True: trace and W of the fit are those of devops.plm_learn_adaptive_dev from the chain's start.  On the synthetic family
    the etas are those of plm_model.learn_adaptive at the rule's blocks, restores included (its conditionals are numpy's exp, so only
    the decisions are compared)."""
    from gaussdca.jl_amd import devops

    ref = operator_chain(g, ctx, refdata, which)
    Z, N, M, q, lam = ref["Z"], ref["N"], ref["M"], ref["q"], ref["lam"]
    n = N * (q - 1)
    n_iter, eta0 = (4, ref["eta"]) if which == "small" else (ADAPT_ITER, ADAPT_ETA)
    if which == "small":
        W, trace = g.gDCA_plm(os.path.join(refdata, FASTA), n_iter, adapt=True, ctx=ctx)
    else:
        W, trace = devops.plm_fit(Z, q, n_iter, adapt=True, eta=eta0, ctx=ctx)
    dW = up(g, ctx, np.asfortranarray(ref["W0"]))
    args = (up(g, ctx, Z), up(g, ctx, ref["wts"]), ref["Meff"], up(g, ctx, ref["Pi_d"]), up(g, ctx, np.asfortranarray(ref["Pij_d"])), N, M, q)
    t2, etas, st = devops.plm_learn_adaptive_dev(ctx, dW, *args, n_iter, eta0, lam)
    assert same_bits(trace, t2), (trace, t2)
    assert same_bits(W, dW.download((n, n)))
    assert np.isfinite(trace).all() and trace[-1, 3] < trace[0, 3]
    if which == "small":
        assert (etas > 0).all()  # (from the default step the first iterations only grow it)
        return
    Wm, tm, em, log, _ = pm.learn_adaptive(ref["W0"], Z, ref["wts"], ref["Meff"], ref["Pi_d"], ref["Pij_d"], q, n_iter, eta0, lam, chunk=RULE)
    # Both runs decide by the sign of f - f_acc.  Where a point is a restored one the device evaluates the same bits twice and the gap
    # is an exact 0 in both runs.  Elsewhere the model's gap must stand clear of what the two runs can differ by: an evaluation is M N
    # terms (a log-sum-exp of q terms over potentials of N) at f64 rounding, and a step at eta <= ADAPT_ETA carries a difference of
    # the tallies of that size into W and from there into the next f, so the runs part by at most that a step, added over the steps
    ev = M * N * (N + q + 2) * 2.0 ** -52 * max(1.0, float(tm[:, 3].max()))
    f_acc, gaps = None, []
    for f, ok in log:
        if f_acc is not None and f != f_acc:
            gaps.append(abs(f - f_acc))
        f_acc = f if ok else f_acc
    print("adaptive: etas %s\nsmallest gap of f %.3e, evaluation bound %.3e" % (etas, min(gaps), ev))
    assert min(gaps) > 1e3 * ADAPT_ETA * n_iter * ev
    assert np.array_equal(etas, em) and (etas == 0).sum() >= 3 and (etas > 0).sum() >= 8
