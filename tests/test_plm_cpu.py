"""The pseudo-likelihood fit without a GPU: tests/plm_model.py against finite differences, against the exact toy (the gradient
vanishes at the true parameters, L-BFGS lands on them), the loop's monotonicity at the default step, the adaptive rule, the measured
softmax bars the GPU test uses, the inputs of the GPU tests at width with the conditions under which they can tell one order of
summation from another, and the exported symbols and bindings."""
import ctypes
import os

import numpy as np
import pytest

import bm_model as bm
import plm_model as pm
from gdca_testutil import ROOT

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)

NEW_SYMBOLS = ("gdca_plm_conditionals_dev", "gdca_plm_conditionals", "gdca_plm_tally_dev", "gdca_plm_tally", "gdca_plm_tallies_dev",
               "gdca_plm_tallies", "gdca_plm_learn_dev", "gdca_plm_learn", "gdca_dbuf_copy")


def container(rng, N, q, scale=1.0):
    """a random model in the container's form"""
    n = N * (q - 1)
    A = rng.normal(size=(n, n)) * scale
    W = np.where(bm.multipliers(N, q) == 1.0, A + A.T, 0.0)
    W[np.arange(n), np.arange(n)] = rng.normal(size=n) * scale
    return W


def family(rng, N, q, M, gaps=0.15):
    """Z (N, M) int8 with gaps, sequence 5 (where there is one) all gaps; w (M,) unequal weights in (0, 1]; Meff = sum w"""
    Z = rng.integers(1, q, size=(N, M)).astype(np.int8)
    Z[rng.random((N, M)) < gaps] = q
    if M > 5:
        Z[:, 5] = q
    w = 1.0 / rng.integers(1, 6, size=M)
    return np.asfortranarray(Z), w, float(w.sum())


# ---- the softmax cases of the GPU test, and the bars measured here -------------------------------------------------------------------------
SOFTMAX_CASES = [(7, 5), (5, 21), (9, 31), (53, 21)]
SOFTMAX_M = 37
# MEASURED on the CPU (test_softmax_bars_are_the_measured_ones prints them): the largest error of plm_model's f64 conditionals against
# its np.longdouble ones on exactly these inputs, in ulps of p and in ulps of l taken at max(|l|, 1) -- l = (V[x] - m) + log(Zs) with Zs
# rounded at the ulp of 1, so below 1 its absolute error does not shrink with l.  V spans +-700 here: m - V_c is rounded at the ulp of
# 1400, which alone is 2^-43 relative in e_c = 1024 ulps of p, and the f64 potentials' own sums of N terms of that size add to it.
# The GPU test's bars are 4 x these (the device library's exp / log and its own order of the potentials' sums); both numbers of every
# case, and what the device reached, are recorded in tests/golden/plm_softmax_bars.md.
# (l: a small l is the difference of two potentials near 700, so the f64 potentials' absolute error, a few ulps of 700 = a few hundred
# ulps of 1, shows in it at N = 53.)  Measured 2026-10-21: 1212.2 / 15.53, 1095.4 / 8.12, 1572.0 / 23.34, 2216.6 / 255.96.
SOFTMAX_MEASURED = {(7, 5): (1250.0, 16.0), (5, 21): (1100.0, 9.0), (9, 31): (1600.0, 24.0), (53, 21): (2250.0, 260.0)}
SOFTMAX_DEVICE_FACTOR = 4.0


def softmax_case(N, q):
    """(W scaled so that max |V| = 700, Z (N, 37) with gaps and one all-gap sequence)"""
    rng = np.random.default_rng(1000 * N + q)
    W = container(rng, N, q)
    Z, _, _ = family(rng, N, q, SOFTMAX_M)
    W = W * (700.0 / float(np.abs(pm.potentials(W, Z, q)).max()))
    return W, Z


def softmax_errors(p, l, W, Z, q):
    """(max ulps of p, max ulps of l at max(|l|, 1)) against the longdouble model"""
    p_ld, l_ld, _ = pm.conditionals(W, Z, q, LD)
    return float(pm.ulps(p, p_ld).max()), float(pm.ulps(l, l_ld, floor=1.0).max())


@pytest.mark.parametrize("N,q", SOFTMAX_CASES)
def test_softmax_bars_are_the_measured_ones(N, q):
    W, Z = softmax_case(N, q)
    V = pm.potentials(W, Z, q)
    assert 699.0 < float(np.abs(V).max()) <= 700.5 and float(V.min()) < -300 and float(V.max()) > 300
    assert (Z[:, 5] == q).all() and (Z == q).sum() > N
    p, l, _ = pm.conditionals(W, Z, q, np.float64)
    assert np.isfinite(p).all() and np.isfinite(l).all()
    ep, el = softmax_errors(p, l, W, Z, q)
    print("softmax N=%d q=%d: f64 model against longdouble: %.1f ulps of p, %.2f ulps of l" % (N, q, ep, el))
    mp, ml = SOFTMAX_MEASURED[(N, q)]
    assert ep <= mp and el <= ml and mp < 2 * ep + 1 and ml < 2 * el + 1  # the recorded numbers are these measurements, rounded up


# ---- 1. the gradient identity against central finite differences -------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q", [(5, 4), (3, 21)])
def test_gradient_is_the_tallies_expression(N, q):
    rng = np.random.default_rng(10 * N + q)
    W = container(rng, N, q, 0.5)
    Z, w, Meff = family(rng, N, q, 23)
    Pi_d, Pij_d = pm.frequencies(Z, w, Meff, q)
    G = pm.gradient(W, Z, w, Meff, Pi_d, Pij_d, q)
    n = N * (q - 1)
    m = bm.multipliers(N, q)
    # central differences of nll in longdouble: h = 2^-20, truncation h^2 |f'''| / 6 ~ 1e-13 (third derivatives of a log-sum-exp of
    # unit coefficients are below 1), rounding eps_ld |nll| / h ~ 1e-19 * 50 * 1e6 ~ 5e-12 at the worst
    h = LD(2.0) ** -20
    Wl = W.astype(LD)
    picks = [(r, r) for r in range(n)] + [(int(r), int(c)) for r, c in zip(*np.nonzero(np.tril(m == 1.0))) if (r * 7 + c) % 5 == 0]
    worst = 0.0
    for r, c in picks:
        up, dn = Wl.copy(), Wl.copy()
        up[r, c] += h
        dn[r, c] -= h
        if r != c:
            up[c, r] += h
            dn[c, r] -= h
        fd = -(pm.nll_of(up, Z, w, Meff, q) - pm.nll_of(dn, Z, w, Meff, q)) / (2 * h)
        worst = max(worst, float(abs(fd - G[r, c])))
    print("N=%d q=%d: %d parameters, worst |finite difference - tallies' expression| = %.2e" % (N, q, len(picks), worst))
    assert worst < 2e-11
    # the ordered f64 tallies say the same to f64 rounding: sums of M terms below 1
    p64 = pm.conditionals(W, Z, q, np.float64)[0]
    Pi_o, Pij_o = pm.tallies_ordered(p64, Z, w, Meff, q, chunk=8)
    Pi_l, Pij_l = pm.tallies(pm.conditionals(W, Z, q, LD)[0], Z, w, Meff, q)
    bound = (Z.shape[1] + 8) * 2.0 ** -52 + n * np.abs(W).max() * 2.0 ** -51  # the sums' roundings + the f64 potentials' behind p
    assert float(np.abs(Pij_o - Pij_l).max()) < bound and float(np.abs(Pi_o - Pi_l).max()) < bound
    assert np.array_equal(Pij_o, Pij_o.T) and np.array_equal(np.diagonal(Pij_o), Pi_o)
    assert np.all(Pij_o[m == 0.0] == 0.0) and not np.signbit(Pij_o[m == 0.0]).any()


# ---- 2. consistency on the exact toy ------------------------------------------------------------------------------------------------------------
def test_gradient_vanishes_at_the_true_parameters():
    N, q = 4, 3
    mJ, Pi, Z, w, W_true = pm.consistency_toy(N, q)
    assert Z.shape == (N, 81) and abs(float(w.sum()) - 1) < 1e-15
    Pi_d, Pij_d = pm.frequencies(Z, w, 1.0, q)
    G = pm.gradient(W_true, Z, w, 1.0, Pi_d, Pij_d, q)
    # W_true is the exact model rounded to f64: a relative 2^-53 an entry, so every potential (at most n entries of it) and with it
    # every log-probability is off by at most n max|W| 2^-53; a probability-weighted average of differences of conditionals that are
    # each off by that relative amount, twice (the pair's two sites), plus the longdouble roundings (far below)
    n = N * (q - 1)
    bound = 4 * n * float(np.abs(W_true).max()) * 2.0 ** -53
    print("max |gradient| at the true parameters: %.2e (bound %.2e)" % (float(np.abs(G).max()), bound))
    assert float(np.abs(G).max()) < bound


def test_lbfgs_lands_on_the_true_parameters():
    from scipy.optimize import minimize

    N, q = 4, 3
    mJ, Pi, Z, w, W_true = pm.consistency_toy(N, q)
    w64 = w.astype(np.float64)
    Pi_d, Pij_d = (x.astype(np.float64) for x in pm.frequencies(Z, w, 1.0, q))
    n = N * (q - 1)

    def fg(theta):
        W = pm.from_parameters(theta, N, q)
        G = pm.gradient(W, Z, w64, 1.0, Pi_d, Pij_d, q, np.float64)
        return float(pm.nll_of(W, Z, w64, 1.0, q, np.float64)), -pm.parameters(G, N, q)

    th0 = pm.parameters(bm.potts_independent(Pi_d, N, q), N, q)
    gtol = 1e-9
    res = minimize(fg, th0, jac=True, method="L-BFGS-B", options=dict(gtol=gtol, ftol=0.0, maxiter=2000, maxcor=30))
    g_end = float(np.abs(res.jac).max())
    # the smallest eigenvalue mu of the Hessian at the optimum, by central differences of the gradient: for a strongly convex function
    # |theta - theta*|_2 <= |grad|_2 / mu near the optimum, so max |grad| <= gtol implies |theta - theta*|_inf <= sqrt(P) gtol / mu;
    # twice that for the Hessian's own variation over so short a way
    th_true = pm.parameters(W_true, N, q)
    P, h = len(th_true), 1e-5
    H = np.empty((P, P))
    for a in range(P):
        e = np.zeros(P)
        e[a] = h
        H[:, a] = (fg(th_true + e)[1] - fg(th_true - e)[1]) / (2 * h)
    mu = float(np.linalg.eigvalsh((H + H.T) / 2).min())
    tol = 2 * np.sqrt(P) * max(g_end, gtol) / mu
    err = float(np.abs(res.x - th_true).max())
    print("L-BFGS-B: %d iterations, max |grad| %.2e, mu %.3e, max |theta - theta_true| %.2e (tolerance %.2e)" % (res.nit, g_end, mu, err, tol))
    assert mu > 0 and g_end <= 10 * gtol  # (it stopped on the gradient, not on a failed line search far from the optimum)
    assert err < tol


# ---- 3. the default step never raises the penalised nll ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,N,q,M,lam", [(1, 5, 4, 30, 0.01), (2, 4, 6, 25, 0.0)])
def test_default_step_is_monotone(seed, N, q, M, lam):
    rng = np.random.default_rng(seed)
    Z, w, Meff = family(rng, N, q, M)
    Pi_d, Pij_d = (x.astype(np.float64) for x in pm.frequencies(Z, w, Meff, q))
    W0 = container(rng, N, q, 0.3)
    eta = 1.0 / (N + 2 * lam)
    n_iter = 200
    W, trace, Ws = pm.learn(W0, Z, w, Meff, Pi_d, Pij_d, q, n_iter, eta, lam, chunk=8, ordered=False, keep=True)
    f = [pm.nll_of(Wt, Z, w, Meff, q) + LD(lam) * pm.penalty(Wt, N, q, LD) for Wt in Ws + [W]]
    # a longdouble evaluation sums M N terms l_ki (each a log-sum-exp of q terms over potentials of N terms) and n^2 squares: its error
    # is below (M N (N + q + 2) + n^2) eps_ld times the largest term; twice that separates two evaluations
    n = N * (q - 1)
    big = max(float(np.abs(pm.conditionals(W0, Z, q)[1]).max()), float(np.abs(W).max()) ** 2, 1.0)
    bound = 2 * (M * N * (N + q + 2) + n * n) * EPS_LD * big
    rises = [(t, float(f[t + 1] - f[t])) for t in range(n_iter) if abs(f[t + 1] - f[t]) > bound and f[t + 1] > f[t]]
    checked = sum(1 for t in range(n_iter) if abs(f[t + 1] - f[t]) > bound)
    print("penalised nll %.6f -> %.6f over %d iterations, %d compared beyond the evaluation bound %.1e" % (f[0], f[-1], n_iter, checked, bound))
    assert checked > n_iter // 2 and not rises, rises[:3]
    assert float(f[-1]) < float(f[0])
    # the f64 trace's nll follows the longdouble one: M N terms at f64 rounding
    assert np.abs(trace[:, 3] - np.array([float(pm.nll_of(Wt, Z, w, Meff, q)) for Wt in Ws])).max() < M * N * (N + q + 2) * 2.0 ** -52 * big


# ---- 4. the adaptive rule ---------------------------------------------------------------------------------------------------------------------------
def test_adaptive_rule_splits_and_never_keeps_a_step_after_a_rise():
    rng = np.random.default_rng(5)
    N, q, M, lam = 4, 5, 20, 0.01
    Z, w, Meff = family(rng, N, q, M)
    Pi_d, Pij_d = (x.astype(np.float64) for x in pm.frequencies(Z, w, Meff, q))
    W0 = container(rng, N, q, 0.3)
    eta0 = 4.0  # far above 1 / (N + 2 lam): the rule has to halve
    W, trace, etas, log, state = pm.learn_adaptive(W0, Z, w, Meff, Pi_d, Pij_d, q, 40, eta0, lam, chunk=8)
    Wa, ta, ea, la, sa = pm.learn_adaptive(W0, Z, w, Meff, Pi_d, Pij_d, q, 17, eta0, lam, chunk=8)
    Wb, tb, eb, lb, sb = pm.learn_adaptive(Wa, Z, w, Meff, Pi_d, Pij_d, q, 23, eta0, lam, state=sa, chunk=8)
    assert np.array_equal(W, Wb) and np.array_equal(trace, np.vstack([ta, tb])) and np.array_equal(etas, np.concatenate([ea, eb]))
    assert state[0] == sb[0] and state[1] == sb[1]
    acc = [f for f, ok in log if ok]
    rej = [t for t, (f, ok) in enumerate(log) if not ok]
    assert rej and len(acc) > len(rej)  # both branches ran
    assert all(b <= a for a, b in zip(acc, acc[1:]))  # the accepted values never rise
    for t in rej:
        prev = [u for u in range(t) if log[u][1]][-1]
        assert etas[t] == 0.0 and log[t][0] > log[prev][0]  # a rise: no step is taken from the risen point
        if t + 1 < len(log):  # the restored point is evaluated again (the same bits) and left with half the step that rose
            assert log[t + 1][1] and log[t + 1][0] == log[prev][0] and etas[t + 1] == etas[prev] / 2
    assert acc[-1] < acc[0]


# ---- 5. the cases at width can tell one order from another (the GPU tests of test_gpu_plm_width.py run on these inputs) ----------------------------
# (N, q, M, PLM_CHUNK; 0: the rule, blocks of pm.CHUNK_RULE): what each one reaches stands at test_gpu_plm_width.test_tally_at_width
WIDTH_TALLY_CASES = [(5, 21, 1029, 0), (7, 5, 517, 0), (6, 2, 600, 0), (3, 31, 100, 24), (13, 21, 96, 32), (4, 5, 49, 16), (4, 5, 48, 16),
                     (53, 21, 529, 0)]
WIDTH_NLL_CASES = [(5, 21, 1029), (7, 5, 517), (5, 21, 257), (5, 21, 256)]
WIDTH_FIT_FAMILY = (12, 1100, 5, 11)  # synth_family's (N, M, q, seed): three blocks of the rule


def width_case(N, q, M):
    """(W, Z, w, Meff) as test_gpu_plm.test_tally_bit_for_bit builds them: seed 100 N + q + M, weights 2^-40 apart (the order of the
    additions shows in the last bits) with one zero and one 1"""
    rng = np.random.default_rng(100 * N + q + M)
    W = container(rng, N, q, 0.7)
    Z, _, _ = family(rng, N, q, M)
    w = 0.5 + np.arange(M) * 2.0 ** -40
    w[1] = 0.0
    w[M - 1] = 1.0
    return W, Z, w, float(w.sum())


def differing(a, b):
    return int((np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)).sum())


@pytest.mark.parametrize("N,q,M,chunk", WIDTH_TALLY_CASES)
def test_width_cases_tell_the_blocks_from_one_block(N, q, M, chunk):
    """With numpy's own p: the ordered tally cut into the case's blocks is not the bits of the same tally summed as ONE block, so a
    device that added the blocks' partials in another place, or took another block length, would show."""
    W, Z, w, Meff = width_case(N, q, M)
    assert Z.shape == (N, M) and int(Z.max()) <= q and w.min() == 0.0 and w.max() == 1.0
    p = pm.conditionals(W, Z, q, np.float64)[0]
    Pi_b, Pij_b = pm.tallies_ordered(p, Z, w, Meff, q, chunk or pm.CHUNK_RULE)
    Pi_1, Pij_1 = pm.tallies_ordered(p, Z, w, Meff, q, M)
    d = differing(Pij_b, Pij_1)
    print("N=%d q=%d M=%d chunk=%d: %d entries of Pij differ from the one-block sum's, %d of Pi" % (N, q, M, chunk, d, differing(Pi_b, Pi_1)))
    assert d > 0
    assert np.array_equal(Pij_b, Pij_b.T) and np.array_equal(np.diagonal(Pij_b), Pi_b)


@pytest.mark.parametrize("N,q,M", WIDTH_NLL_CASES)
def test_width_cases_tell_the_strided_sum_from_the_ascending_one(N, q, M):
    """nll in the device's order (256 strided partials, the halving tree) is not the bits of the products added one by one with k
    ascending: a wrong stride, start or tree would show."""
    W, Z, w, Meff = width_case(N, q, M)
    nll_k = pm.conditionals(W, Z, q, np.float64)[2]
    prod = w * nll_k
    asc = np.float64(0.0)
    for v in prod:
        asc = asc + v
    ordered = float(pm.nll_ordered(w, nll_k, Meff))
    print("M=%d: nll ordered %.17g, ascending %.17g" % (M, ordered, float(asc / np.float64(Meff))))
    assert ordered != float(asc / np.float64(Meff))


def test_width_fit_family_is_three_blocks_of_the_rule():
    """synth_family(12, 1100, 5, 11): every symbol of the alphabet occurs (q is read off Z.max()), the sequences number more than two
    blocks of the rule, plm_fit takes them as they are (it removes no duplicates: the chain of the operators gets the same M), and
    the reweighting has neighbours to count: weights below 1."""
    from gaussdca.jl_amd.dcautils import remove_duplicate_sequences
    from gaussdca.jl_amd.synth import synth_family
    from oracle import gdca_oracle as o

    N, M, q, seed = WIDTH_FIT_FAMILY
    Zo = synth_family(N, M, q, seed)
    Z = np.asfortranarray(Zo.T)
    assert Z.shape == (N, M) and int(Z.max()) == q and int(Z.min()) == 1 and M > 2 * pm.CHUNK_RULE
    Zu, _ = remove_duplicate_sequences(Z)
    wts, Meff, _, _ = o.compute_weights(np.ascontiguousarray(Zo), "auto")
    print("synth family: %d sequences, %d distinct, Meff %.2f, %d weights below 1" % (M, Zu.shape[1], Meff, int((wts < 1).sum())))
    assert Zu.shape[1] <= M and (wts < 1).any() and wts.max() <= 1 and Meff < M
    # theta reaches the weights through floor(theta N) alone: :auto's theta and 0.3 are the same neighbourhood of 3 sites here (a fit
    # at theta = 0.3 repeats the default's bits), 0.2 is another
    thr = {th: o.compute_weights(np.ascontiguousarray(Zo), th)[3] for th in ("auto", 0.3, 0.2)}
    assert thr == {"auto": 3, 0.3: 3, 0.2: 2}, thr


# ---- 6. exports and bindings ------------------------------------------------------------------------------------------------------------------------
def test_exports_and_bindings():
    import gaussdca.jl_amd as g
    from gaussdca.jl_amd import _lib, devops
    from test_cabi_cpu import _header_prototypes

    assert os.path.exists(_lib.LIB_PATH), "libgdca.so not built"
    raw = ctypes.CDLL(_lib.LIB_PATH)
    protos = _header_prototypes()
    for s in NEW_SYMBOLS:
        assert hasattr(raw, s), s
        assert len(_lib.SYMBOLS[s][1]) == len(protos[s][1]), s
    assert len(protos["gdca_plm_learn_dev"][1]) == 14 and len(protos["gdca_plm_tallies_dev"][1]) == 11
    assert protos["gdca_plm_learn"][1][4] == "double" and protos["gdca_plm_learn"][1][11:13] == ["double", "double"]
    assert _lib.SYMBOLS["gdca_plm_learn_dev"][1][4] == ctypes.c_double and _lib.SYMBOLS["gdca_plm_learn_dev"][1][11:13] == [ctypes.c_double] * 2
    hdr = open(os.path.join(ROOT, "include", "gdca.h")).read()
    assert "Pseudo-likelihood fit" in hdr and "PLM_CHUNK" in hdr and "PLM_SLAB" in hdr and "CONDITIONAL TALLIES" in hdr
    assert raw.gdca_version() == 6 and raw.gdca_stats_bytes() == ctypes.sizeof(_lib.Stats)  # the ABI stays 0.6
    for f in ("plm_conditionals_dev", "plm_tally_dev", "plm_tallies_dev", "plm_learn_dev"):
        assert callable(getattr(devops, f)) and hasattr(g.Context, f), f
    assert callable(devops.plm_fit) and callable(devops.plm_learn_adaptive_dev) and callable(g.gDCA_plm) and callable(g.plm_learn)
    assert "1 / (N + 2 lam)" in g.gDCA_plm.__doc__ and "halved" in g.gDCA_plm.__doc__
    assert devops.PLM_GROW == pm.GROW
    W = np.diag(np.arange(1.0, 7.0))
    W[0, 3] = W[3, 0] = 2.0
    W[0, 1] = 9.0  # (inside a diagonal block: not a coupling)
    assert devops.plm_penalty(W, 2, 4) == 4.0 == float(pm.penalty(W, 2, 4))
    # the Python layer refuses before the library is asked
    with pytest.raises(g.ArgumentError):
        devops.plm_fit(np.ones((3, 4), dtype=np.int8), 4, 0)
    with pytest.raises(g.ArgumentError):
        devops.plm_fit(np.ones((3, 4), dtype=np.int8), 4, 3, init="plm")
    with pytest.raises(g.ArgumentError):
        devops.plm_fit(np.ones((3, 4), dtype=np.int8), 4, 3, eta=0.0)
    with pytest.raises(g.ArgumentError):
        g.plm_learn(np.zeros((6, 6)), np.ones((3, 4), dtype=np.int8), np.ones(4), 4.0, np.zeros(9), np.zeros((9, 9)), 3, q=4)
