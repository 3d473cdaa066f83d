"""The pseudo-likelihood fit on the device (gdca_plm_conditionals*, gdca_plm_tally*, gdca_plm_tallies*, gdca_plm_learn*) against
tests/plm_model.py: the conditionals within the bars measured on the CPU (test_plm_cpu.py), the tally bit for bit against the model's
ordered sums, the fused form against its seams, the gradient through the public route, the loop rule, learning on the exact toy
against the numpy loop, and the plumbing.  No tolerance is invented here: every bound is derived where it stands or measured on the
numpy model alone."""
import os

import numpy as np
import pytest

import bm_model as bm
import plm_model as pm
from gdca_testutil import ctx, g  # noqa: F401 (fixtures)
from test_plm_cpu import SOFTMAX_CASES, SOFTMAX_DEVICE_FACTOR, SOFTMAX_M, SOFTMAX_MEASURED, container, family, softmax_case

pytestmark = pytest.mark.gpu
LD = np.longdouble
EINVAL = 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def up(g, c, a):
    a = np.asarray(a)
    return g.DeviceBuffer.from_array(c, a if a.flags.c_contiguous or a.flags.f_contiguous else np.asfortranarray(a))


def dev_conditionals(g, c, W, Z, q):
    from gaussdca.jl_amd import devops

    N, M = Z.shape
    dp, dn = devops.plm_conditionals_dev(c, up(g, c, np.asfortranarray(W)), up(g, c, Z), N, M, q)
    return dp.download((M, N, q), order="C"), dn.download((M,))


def dev_tally(g, c, p, Z, w, Meff, q):
    from gaussdca.jl_amd import devops

    N, M = Z.shape
    n = N * (q - 1)
    dPi, dPij = devops.plm_tally_dev(c, up(g, c, np.ascontiguousarray(p)), up(g, c, Z), up(g, c, w), Meff, N, M, q)
    return dPi.download((n,)), dPij.download((n, n))


def dev_tallies(g, c, W, Z, w, Meff, q):
    from gaussdca.jl_amd import devops

    N, M = Z.shape
    n = N * (q - 1)
    dPi, dPij, dnll = devops.plm_tallies_dev(c, up(g, c, np.asfortranarray(W)), up(g, c, Z), up(g, c, w), Meff, N, M, q)
    return dPi.download((n,)), dPij.download((n, n)), float(dnll.download((1,))[0])


def with_options(g, **kv):
    c = g.Context(0)
    for k, v in kv.items():
        c.set_option(k, v)
    return c


# ---- 1. the softmax ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q", SOFTMAX_CASES)
def test_softmax_against_the_longdouble_model(g, ctx, N, q):
    """Bars: SOFTMAX_DEVICE_FACTOR x what test_plm_cpu measured for the f64 numpy model against longdouble on these inputs, in ulps of p
    and in ulps of l at max(|l|, 1).  l_ki itself is not an output: nll_k is its sum over i added one by one, so it is held to the
    sum of the sites' l bars plus the (N - 1) roundings of the additions, each below 2^-53 of the sum of |l|."""
    W, Z = softmax_case(N, q)
    M = SOFTMAX_M
    p, nll_k = dev_conditionals(g, ctx, W, Z, q)
    assert np.isfinite(p).all() and np.isfinite(nll_k).all() and (p >= 0).all()
    p_ld, l_ld, nll_ld = pm.conditionals(W, Z, q, LD)
    mp, ml = SOFTMAX_MEASURED[(N, q)]
    ep = float(pm.ulps(p, p_ld).max())
    l_abs = np.abs(l_ld).astype(np.float64)
    bound = SOFTMAX_DEVICE_FACTOR * ml * np.spacing(np.maximum(l_abs, 1.0)).sum(axis=1) + (N - 1) * 2.0 ** -53 * l_abs.sum(axis=1)
    en = np.abs(nll_k.astype(LD) - nll_ld).astype(np.float64)
    print("N=%d q=%d: p %.1f ulps (bar %.0f), nll_k error / bound %.3g" % (N, q, ep, SOFTMAX_DEVICE_FACTOR * mp, float((en / bound).max())))
    assert ep <= SOFTMAX_DEVICE_FACTOR * mp
    assert (en <= bound).all()
    assert np.abs(p.sum(axis=2) - 1).max() <= q * 2.0 ** -52
    assert float(nll_k[5]) >= 0 and (Z[:, 5] == q).all()  # the all-gap sequence: V = 0 at the wild type everywhere


# ---- 2. the tally, bit for bit ------------------------------------------------------------------------------------------------------------------
TALLY_CASES = [(3, 5, 8), (7, 5, 9), (5, 21, 27), (6, 31, 9), (10, 5, 27), (13, 21, 8)]


@pytest.mark.parametrize("N,q,M", TALLY_CASES)
def test_tally_bit_for_bit(g, N, q, M):
    """n = 12 and 28 (below one row block), 100 and 260 (not a multiple of 64), 180 (s = 30), 40; N = 3, 5, 6, 7, 10, 13: the packed dword's
    tail; PLM_CHUNK = 8 with M = 8 (one full block), 9 (a ragged last block of one), 27 (three full blocks and a ragged fourth)"""
    rng = np.random.default_rng(100 * N + q + M)
    W = container(rng, N, q, 0.7)
    Z, _, _ = family(rng, N, q, M)
    w = 0.5 + np.arange(M) * 2.0 ** -40  # weights 2^-40 apart: the order of the additions shows in the last bits
    w[1] = 0.0
    w[M - 1] = 1.0
    Meff = float(w.sum())
    c = with_options(g, PLM_CHUNK=8)
    try:
        p, _ = dev_conditionals(g, c, W, Z, q)
        Pi, Pij = dev_tally(g, c, p, Z, w, Meff, q)
        c.set_option("PLM_CHUNK", 0)
        Pi_r, Pij_r = dev_tally(g, c, p, Z, w, Meff, q)  # (the rule: one block here)
    finally:
        c.close()
    Pi_m, Pij_m = pm.tallies_ordered(p, Z, w, Meff, q, chunk=8)
    assert same_bits(Pi, Pi_m) and same_bits(Pij, Pij_m)
    Pi_1, Pij_1 = pm.tallies_ordered(p, Z, w, Meff, q, chunk=pm.CHUNK_RULE)
    assert same_bits(Pi_r, Pi_1) and same_bits(Pij_r, Pij_1)
    if M > 16:  # (a ragged block of ONE sequence, M = 9, adds in the sequential order)
        assert not same_bits(Pij_1, Pij_m)  # the option does change the bits: the case can tell an order from another
    m = bm.multipliers(N, q)
    assert same_bits(Pij, Pij.T.copy()) and same_bits(np.diagonal(Pij).copy(), Pi)
    assert np.all(Pij[m == 0.0] == 0.0) and not np.signbit(Pij[m == 0.0]).any()


# ---- 3. the fused form is its seams ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q,M", [(7, 5, 27), (5, 21, 21)])
def test_fused_equals_seams_at_two_slab_sizes(g, N, q, M):
    rng = np.random.default_rng(7 * N + q)
    W = container(rng, N, q, 0.7)
    Z, w, Meff = family(rng, N, q, M)
    out = {}
    for slab in (8, 16, 0):
        c = with_options(g, PLM_CHUNK=8, PLM_SLAB=slab)
        try:
            p, nll_k = dev_conditionals(g, c, W, Z, q)
            out[slab] = (p, nll_k) + dev_tally(g, c, p, Z, w, Meff, q) + dev_tallies(g, c, W, Z, w, Meff, q)
        finally:
            c.close()
    p, nll_k, Pi_s, Pij_s, Pi_f, Pij_f, nll = out[8]
    assert same_bits(Pi_s, Pi_f) and same_bits(Pij_s, Pij_f)
    assert nll == float(pm.nll_ordered(w, nll_k, Meff))
    for slab in (16, 0):
        for a, b in zip(out[8][:6], out[slab][:6]):
            assert same_bits(a, b), slab
        assert out[slab][6] == nll


# ---- 4. the gradient through the public route ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q,M", [(5, 4, 40), (9, 21, 33)])
def test_gradient_through_the_public_route(g, ctx, N, q, M):
    """2 (Pij_c - Pij_d) and 1/2 (Pi_c - Pi_d) from g.plm_tallies against plm_model's longdouble gradient.  An entry of Pij_c is a sum of
    at most M products w_k p_k below 1, divided once: (M + 8) 2^-52 covers its additions in any order; p itself carries the f64
    potentials' error, at most n max|W| 2^-51 relative (n terms, any order, then exp's argument).  The data's side is the model's own
    Pij_d rounded to f64 (2^-53).  Twice the sum for the couplings, half of it for the diagonal."""
    rng = np.random.default_rng(3 * N + q)
    W = container(rng, N, q, 0.5)
    Z, w, Meff = family(rng, N, q, M)
    Pi_d, Pij_d = pm.frequencies(Z, w, Meff, q)
    G = pm.gradient(W, Z, w, Meff, Pi_d, Pij_d, q)
    Pi_c, Pij_c, nll = g.plm_tallies(W, Z, w, Meff, q, ctx=ctx)
    n = N * (q - 1)
    m = bm.multipliers(N, q)
    e = (M + 8) * 2.0 ** -52 + n * float(np.abs(W).max()) * 2.0 ** -51 + 2.0 ** -53
    Gd = np.where(m == 1.0, 2 * (Pij_c - Pij_d.astype(np.float64)), 0.0)
    Gd[np.arange(n), np.arange(n)] = (Pi_c - Pi_d.astype(np.float64)) / 2
    err = float(np.abs(Gd.astype(LD) - G).max())
    print("N=%d q=%d: max |gradient error| %.2e, bound %.2e, max |gradient| %.2e" % (N, q, err, 2 * e, float(np.abs(G).max())))
    assert err <= 2 * e and float(np.abs(G).max()) > 1e3 * e
    ref = float(pm.nll_of(W, Z, w, Meff, q))
    assert abs(nll - ref) <= (M * N * (N + q + 2)) * 2.0 ** -52 * max(1.0, float(np.abs(pm.conditionals(W, Z, q)[1]).max()))


# ---- 5. the loop rule ---------------------------------------------------------------------------------------------------------------------------
def loop_problem(N=6, q=5, M=27, seed=11):
    rng = np.random.default_rng(seed)
    Z, w, Meff = family(rng, N, q, M)
    Pi_d, Pij_d = (x.astype(np.float64) for x in pm.frequencies(Z, w, Meff, q))
    return N, q, M, Z, w, Meff, Pi_d, Pij_d, container(rng, N, q, 0.3)


def device_loop(g, c, prob, W0, n_iter, eta, lam):
    from gaussdca.jl_amd import devops

    N, q, M, Z, w, Meff, Pi_d, Pij_d, _ = prob
    n = N * (q - 1)
    dW = up(g, c, np.asfortranarray(W0))
    dtrace = devops.plm_learn_dev(c, dW, up(g, c, Z), up(g, c, w), Meff, up(g, c, Pi_d), up(g, c, np.asfortranarray(Pij_d)), N, M, q,
                                  n_iter, eta, lam)
    return dW.download((n, n)), dtrace.download((n_iter, 4), order="C")


@pytest.mark.parametrize("lam", [0.0, 0.01])
def test_loop_rule(g, lam):
    from gaussdca.jl_amd import devops

    prob = loop_problem()
    N, q, M, Z, w, Meff, Pi_d, Pij_d, W0 = prob
    n = N * (q - 1)
    eta = 1.0 / (N + 2 * lam)
    runs = {}
    for slab in (0, 8):
        c = with_options(g, PLM_CHUNK=8, PLM_SLAB=slab)
        try:
            W, trace = device_loop(g, c, prob, W0, 7, eta, lam)
            Wa, ta = device_loop(g, c, prob, W0, 3, eta, lam)
            Wb, tb = device_loop(g, c, prob, Wa, 4, eta, lam)
            assert same_bits(W, Wb) and same_bits(trace, np.concatenate((ta, tb)))
            runs[slab] = (W, trace)
            if slab:
                continue
            # the caller's chain of the operator forms
            dW, dZ, dw = up(g, c, np.asfortranarray(W0)), up(g, c, Z), up(g, c, w)
            dPi_d, dPij_d = up(g, c, Pi_d), up(g, c, np.asfortranarray(Pij_d))
            rows = []
            for it in range(7):
                dPi_c, dPij_c, dnll = devops.plm_tallies_dev(c, dW, dZ, dw, Meff, N, M, q)
                out = devops.bm_readout_dev(c, dPi_d, dPij_d, dPi_c, dPij_c, N, q).download((4,))
                assert out[3] == 0.0
                out[3] = dnll.download((1,))[0]
                rows.append(out)
                devops.bm_update_dev(c, dW, dPij_d, dPij_c, N, q, eta, lam)
            assert same_bits(W, dW.download((n, n))) and same_bits(trace, np.stack(rows))
            # the host-pointer form
            Wh, th = g.plm_learn(W0, Z, w, Meff, Pi_d, Pij_d, 7, q, eta=eta, lam=lam, ctx=c)
            assert same_bits(W, Wh) and same_bits(trace, th)
        finally:
            c.close()
    assert same_bits(runs[0][0], runs[8][0]) and same_bits(runs[0][1], runs[8][1])  # whatever the slab
    # ... and the numpy statement in the device's order follows it: the same tallies from the device's own conditionals give the same
    # step, so the first iteration's W is the model's bit for bit once the model is fed the device's p
    c = with_options(g, PLM_CHUNK=8)
    try:
        p, _ = dev_conditionals(g, c, W0, Z, q)
        W1, _ = device_loop(g, c, prob, W0, 1, eta, lam)
    finally:
        c.close()
    assert same_bits(W1, bm.update(W0, Pij_d, pm.tallies_ordered(p, Z, w, Meff, q, chunk=8)[1], N, q, eta, lam))
    m = bm.multipliers(N, q)
    W = runs[0][0]
    assert same_bits(W, W.T.copy()) and np.all(W[m == 0.0] == 0.0) and not np.signbit(W[m == 0.0]).any()
    assert runs[0][1][-1, 3] < runs[0][1][0, 3]


# ---- 6. it learns -----------------------------------------------------------------------------------------------------------------------------------
LEARN_ITER = 800
# MEASURED 2026-10-21 with plm_model.learn (pure numpy, f64, eta = 1 / N = 0.25, lam = 0) on plm_model.consistency_toy(4, 3) from the
# independent-site start: max |W - W_true| 2.1229 at the start, 1.5958 after 100 iterations, 1.2510 after 200, 0.8560 after 400,
# 0.5562 after 800, 0.3752 after 1600.  800 iterations: the numpy loop is below half the start's distance, and the device's 800
# iterations take well under a second.
LEARN_NUMPY_END, LEARN_START = 0.5562, 2.1229


def test_it_learns_on_the_exact_toy(g, ctx):
    N, q = 4, 3
    mJ, Pi, Z, w, W_true = pm.consistency_toy(N, q)
    w64 = w.astype(np.float64)
    M = Z.shape[1]
    Pi_d, Pij_d = (x.astype(np.float64) for x in pm.frequencies(Z, w, 1.0, q))
    W0 = bm.potts_independent(Pi_d, N, q)
    eta = 1.0 / N
    W_np, trace_np = pm.learn(W0, Z, w64, 1.0, Pi_d, Pij_d, q, LEARN_ITER, eta, 0.0, ordered=False)
    end_np, start = float(np.abs(W_np - W_true).max()), float(np.abs(W0 - W_true).max())
    assert abs(end_np - LEARN_NUMPY_END) < 1e-4 and abs(start - LEARN_START) < 1e-4  # the recorded measurement is this run
    W, trace = device_loop(g, ctx, (N, q, M, Z, w64, 1.0, Pi_d, Pij_d, None), W0, LEARN_ITER, eta, 0.0)
    end = float(np.abs(W - W_true).max())
    print("max |W - W_true|: start %.4f, numpy loop %.4f, device loop %.4f" % (start, end_np, end))
    assert end <= 2 * end_np and end < start / 2
    # the device's nll against the numpy loop's: an evaluation is M N terms (log-sum-exp of q terms over potentials of N) at f64
    # rounding; a gradient step at eta <= 1 / L does not expand distances, so the two runs' roundings add at most linearly in t
    ev = M * N * (N + q + 2) * 2.0 ** -52 * max(1.0, float(trace_np[:, 3].max()))
    assert (np.abs(trace[:, 3] - trace_np[:, 3]) <= ev * (1 + np.arange(LEARN_ITER))).all()
    assert (np.diff(trace[:, 3]) <= ev).all()  # and it does not rise beyond an evaluation's rounding


# ---- 7. plumbing ------------------------------------------------------------------------------------------------------------------------------------
def test_gDCA_plm_feeds_the_readouts(g, ctx, refdata):
    fasta = os.path.join(refdata, "small.fasta.gz")
    W, trace, R = g.gDCA_plm(fasta, 3, scores=True, ctx=ctx)
    Z = g.read_fasta_alignment(fasta, 0.9)
    N, q = Z.shape[0], int(Z.max())
    n = N * (q - 1)
    assert W.shape == (n, n) and trace.shape == (3, 4) and np.isfinite(W).all() and np.isfinite(trace).all()
    assert trace[2, 3] < trace[0, 3]  # the default step lowers nll
    m = bm.multipliers(N, q)
    assert same_bits(W, W.T.copy()) and np.all(W[m == 0.0] == 0.0)
    zeros = np.zeros(n)
    X = np.asfortranarray(Z[:, :6])
    E = g.sequence_energies(W, zeros, X, q, ctx=ctx)
    D = g.mutation_scan(W, zeros, X, q, ctx=ctx)
    S = g.correct_APC(g.compute_FN(W, q, ctx=ctx), ctx=ctx)
    assert np.isfinite(E).all() and np.isfinite(D).all() and np.isfinite(S).all() and len(R) > 0
    assert [(i, j) for i, j, _ in R[:5]] == [(i, j) for i, j, _ in g.compute_ranking(S, 5)[:5]]
    # the adaptive loop and the plm start of the Boltzmann machine run through the same route
    Wa, ta = g.gDCA_plm(fasta, 4, adapt=True, ctx=ctx)
    assert np.isfinite(Wa).all() and ta.shape == (4, 4) and ta[-1, 3] < ta[0, 3]
    Wb, tb = g.gDCA_bm(fasta, 1, K=32, init="plm", plm_iter=2, ctx=ctx)
    assert np.isfinite(Wb).all() and tb.shape == (1, 4)


def test_adaptive_device_loop_is_the_model(g):
    from gaussdca.jl_amd import devops

    prob = loop_problem(N=4, q=5, M=20, seed=5)
    N, q, M, Z, w, Meff, Pi_d, Pij_d, W0 = prob
    n = N * (q - 1)
    lam, eta0 = 0.01, 4.0
    c = with_options(g, PLM_CHUNK=8)
    try:
        dW = up(g, c, np.asfortranarray(W0))
        args = (up(g, c, Z), up(g, c, w), Meff, up(g, c, Pi_d), up(g, c, np.asfortranarray(Pij_d)), N, M, q)
        ta, ea, st = devops.plm_learn_adaptive_dev(c, dW, *args, 9, eta0, lam)
        tb, eb, st = devops.plm_learn_adaptive_dev(c, dW, *args, 11, eta0, lam, state=st)
        W = dW.download((n, n))
        dW2 = up(g, c, np.asfortranarray(W0))
        t2, e2, st2 = devops.plm_learn_adaptive_dev(c, dW2, *args, 20, eta0, lam)
        assert same_bits(W, dW2.download((n, n))) and same_bits(np.vstack([ta, tb]), t2) and np.array_equal(np.concatenate([ea, eb]), e2)
    finally:
        c.close()
    # the numpy rule takes the same decisions: the same etas, restores included (its conditionals are numpy's exp, so the bits are not
    # compared).  The two runs differ by the conditionals' roundings alone -- a few ulps of p in sums of M N terms below 1, over 20
    # steps of at most eta0 = 4: below M N 20 eta0 2^-50 = 5.7e-12 had every term the same sign -- and a different decision anywhere
    # would move W by a step's size, 1e-2 and more: 1e-9 lies between the two
    Wm, tm_, em, log, _ = pm.learn_adaptive(W0, Z, w, Meff, Pi_d, Pij_d, q, 20, eta0, lam, chunk=8)
    assert np.array_equal(e2, em) and (e2 == 0).any() and (e2 > 0).sum() > 10
    assert np.abs(W - Wm).max() < 1e-9 and np.abs(t2[:, 3] - tm_[:, 3]).max() < 1e-9


def test_host_forms_equal_dev_forms(g, ctx):
    rng = np.random.default_rng(2)
    N, q, M = 7, 5, 27
    W = container(rng, N, q, 0.7)
    Z, w, Meff = family(rng, N, q, M)
    p, nll_k = dev_conditionals(g, ctx, W, Z, q)
    ph, nh = g.plm_conditionals(W, Z, q, ctx=ctx)
    assert same_bits(p, ph) and same_bits(nll_k, nh)
    Pi, Pij, nll = dev_tallies(g, ctx, W, Z, w, Meff, q)
    Pi_h, Pij_h, nll_h = g.plm_tallies(W, Z, w, Meff, q, ctx=ctx)
    assert same_bits(Pi, Pi_h) and same_bits(Pij, Pij_h) and nll == nll_h
    n = N * (q - 1)
    Pi_t, Pij_t = np.empty(n), np.empty((n, n), order="F")
    P = g._lib._p
    pc = np.ascontiguousarray(p)
    ctx.check(ctx.lib.gdca_plm_tally(ctx.h, P(pc), P(Z), P(w), Meff, N, M, q, P(Pi_t), P(Pij_t)))
    assert same_bits(Pi, Pi_t) and same_bits(Pij, Pij_t)


def test_refusals_leave_W_untouched(g, ctx):
    from gaussdca.jl_amd import devops

    prob = loop_problem()
    N, q, M, Z, w, Meff, Pi_d, Pij_d, W0 = prob
    n = N * (q - 1)
    dW, dZ, dw = up(g, ctx, np.asfortranarray(W0)), up(g, ctx, Z), up(g, ctx, w)
    dPi_d, dPij_d = up(g, ctx, Pi_d), up(g, ctx, np.asfortranarray(Pij_d))
    dtrace, dPi_c, dPij_c, dnll = (g.DeviceBuffer(ctx, b) for b in (32 * 3, 8 * n, 8 * n * n, 8))
    bad_w = w.copy()
    bad_w[3] = 1.5
    dbad, dneg = up(g, ctx, bad_w), up(g, ctx, np.where(np.arange(M) == 2, -1e-3, w))
    lib, h = ctx.lib, ctx.h
    V = lambda b: None if b is None else b.ptr  # noqa: E731

    def learn(W=dW, Z_=dZ, w_=dw, Meff_=Meff, Pi=dPi_d, Pij=dPij_d, N_=N, M_=M, q_=q, it=3, eta=0.1, lam=0.01, tr=dtrace):
        return lib.gdca_plm_learn_dev(h, V(W), V(Z_), V(w_), Meff_, V(Pi), V(Pij), N_, M_, q_, it, eta, lam, V(tr))

    def tallies(W=dW, Z_=dZ, w_=dw, Meff_=Meff, q_=q, Pi=dPi_c, Pij=dPij_c, nll=dnll):
        return lib.gdca_plm_tallies_dev(h, V(W), V(Z_), V(w_), Meff_, N, M, q_, V(Pi), V(Pij), V(nll))

    refused = [learn(W=None), learn(Z_=None), learn(w_=None), learn(Pi=None), learn(Pij=None), learn(tr=None), learn(q_=1), learn(q_=32),
               learn(w_=dbad), learn(w_=dneg), learn(eta=0.0), learn(eta=-1.0), learn(eta=float("nan")), learn(eta=float("inf")),
               learn(lam=-0.1), learn(lam=float("nan")), learn(lam=float("inf")), learn(it=0), learn(tr=dW), learn(Meff_=0.0), learn(N_=0), learn(M_=0),
               tallies(W=None), tallies(Pi=None), tallies(Pij=None), tallies(nll=None), tallies(Pij=dW), tallies(w_=dbad), tallies(q_=32),
               tallies(Meff_=float("nan")),
               lib.gdca_plm_conditionals_dev(h, V(dW), V(dZ), N, M, q, None, V(dnll)),
               lib.gdca_plm_conditionals_dev(h, V(dW), V(dZ), N, M, q, V(dW), V(dnll)),
               lib.gdca_plm_tally_dev(h, V(dPij_c), V(dZ), V(dbad), Meff, N, M, q, V(dPi_c), V(dPij_c)),
               lib.gdca_plm_tally_dev(h, V(dPij_c), V(dZ), V(dw), Meff, N, M, q, V(dPi_c), None)]
    assert refused == [EINVAL] * len(refused), refused
    assert same_bits(dW.download((n, n)), np.asfortranarray(W0))
    # the host form refuses the same and leaves the caller's array alone
    Wh = np.asfortranarray(W0.copy())
    tr = np.empty((3, 4))
    P = g._lib._p
    assert lib.gdca_plm_learn(h, P(Wh), P(Z), P(bad_w), Meff, P(Pi_d), P(np.asfortranarray(Pij_d)), N, M, q, 3, 0.1, 0.0, P(tr)) == EINVAL
    assert same_bits(Wh, W0)
    # a byte of Z outside 1 .. q: reported as the mutation stage reports it
    Zbad = Z.copy()
    Zbad[2, 4] = q + 1
    with pytest.raises(g.ArgumentError) as ei:
        devops.plm_tallies_dev(ctx, dW, up(g, ctx, Zbad), dw, Meff, N, M, q)
    with pytest.raises(g.ArgumentError) as em:
        devops.mutation_scan_dev(ctx, dW, up(g, ctx, np.zeros(n)), N, q, up(g, ctx, Zbad), M)
    assert type(ei.value) is type(em.value) and str(ei.value) == str(em.value)
    # and the context still works
    assert learn() == 0
    assert not same_bits(dW.download((n, n)), np.asfortranarray(W0))
