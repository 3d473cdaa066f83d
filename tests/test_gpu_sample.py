"""The Metropolis chains on the device (gdca_sample*, gdca_run_sample*, sample, gDCA_sample) against tests/sample_model.py: the rule
of include/gdca.h bit for bit (emulate, from the device's own initial table and the device's own thresholds), the thresholds against
-log(u) in np.longdouble, the mathematics of the accepted path (walk_model's exact replay and bounds), what the outputs may not depend
on -- K, the position in the batch, where the table lives, how the chain is cut into launches, fused or operator --, and the sampled
distribution against the exact one of a toy model.  No tolerance is invented here."""
import ctypes as C
import os

import numpy as np
import pytest

import energy_model as em
import sample_model as sm
from energy_model import U
from gdca_testutil import ctx, g, golden_model, mixed_sequences, synth_model  # noqa: F401 (g, ctx: fixtures)
from test_sample_cpu import P_PASS, P_POWER, TOY_BURN, TOY_CHAIN_SEED, toy_chains
from test_walk_cpu import tie_model

pytestmark = pytest.mark.gpu

NAMES = ("Xs", "dE_s", "accepted", "thr", "moves", "V")
INT_MIN = np.iinfo(np.int32).min


def chains(g, ctx, mJ, Pi, X, q, **kw):
    """sample with the trace and the table as a dict of NAMES"""
    return dict(zip(NAMES, g.sample(mJ, Pi, X, q, trace=True, table=True, ctx=ctx, **kw)))


def same(a, b, what=""):
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), (what, n)


def chain_of(d, k):
    """chain k of a batch, as a batch of one"""
    return {n: d[n][..., k:k + 1] if n == "Xs" else d[n][k:k + 1] for n in NAMES}


def assert_is_the_rule(g, ctx, mJ, Pi, X, q, V0, mask=None, flags=0, beta=1.0, seed=0, stream0=0, burn=0, stride=1, n_samples=1, tag=""):
    """every output of the device's chains == sample_model.emulate from the device's own initial table V0 and the device's own
    thresholds, chain by chain"""
    N, K = X.shape
    T = burn + n_samples * stride
    d = chains(g, ctx, mJ, Pi, X, q, mask=mask, gaps=bool(flags), beta=beta, seed=seed, stream0=stream0, burn=burn, stride=stride,
               n_samples=n_samples)
    assert d["Xs"].shape == (N, n_samples, K) and d["dE_s"].shape == (K, n_samples) and d["accepted"].shape == (K,)
    assert d["thr"].shape == (K, T) and d["moves"].shape == (K, T) and d["V"].shape == (K, N, q)
    for k in range(K):
        Xs, dE_s, acc, moves, V = sm.emulate(V0[k], mJ, X[:, k], q, d["thr"][k], mask, flags, beta, seed, stream0 + k, burn, stride, n_samples)
        what = (tag, k, int(d["accepted"][k]), acc)
        assert np.array_equal(d["moves"][k], moves), what
        assert d["accepted"][k] == acc, what
        assert np.array_equal(d["Xs"][:, :, k], Xs.T), what
        assert np.array_equal(d["dE_s"][k], dE_s) and np.array_equal(np.signbit(d["dE_s"][k]), np.signbit(dE_s)), what
        assert np.array_equal(d["V"][k], V), what
    return d


# ---- 1. the rule, bit for bit --------------------------------------------------------------------------------------------------------------
MODEL_IDS = ["small-0.8", "small-0.2", "ties", "q21-N200"]


def model(refdata, which):
    """(tag, Zo (M, N) family, q, mJ, Pi)"""
    if which < 2:
        pc = (0.8, 0.2)[which]
        return ("small pc %g" % pc,) + golden_model(refdata, "small.fasta.gz", pc)
    if which == 2:
        mJ, Pi, x, _ = tie_model()
        return "ties", np.repeat(x[None, :], 3, axis=0), 3, mJ, Pi
    return ("synth q 21 N 200",) + synth_model(21, 200)


# flags, masked, beta: both state spaces, with and without a mask, the three temperatures
RULE_CASES = [(0, False, 1.0), (sm.GAPS, False, 1.0), (0, True, 4.0), (sm.GAPS, True, 0.0), (sm.GAPS, False, 4.0), (0, False, 0.0)]


@pytest.mark.parametrize("which", range(4), ids=MODEL_IDS)
def test_the_rule_bit_for_bit(g, ctx, refdata, which):
    tag, Zo, q, mJ, Pi = model(refdata, which)
    N = Zo.shape[1]
    X = mixed_sequences(np.random.default_rng(100 + which), Zo, q, 7)  # all gaps, gap-free, random, a family member, ...
    V0 = g.mutation_scan(mJ, Pi, X, q, what="potential", ctx=ctx)
    mask = (np.arange(N) % 3 != 1).astype(np.int8)
    burn, stride = N, N // 2 + 1
    for flags, masked, beta in RULE_CASES:
        d = assert_is_the_rule(g, ctx, mJ, Pi, X, q, V0, mask if masked else None, flags, beta, seed=which, stream0=3, burn=burn, stride=stride,
                               n_samples=6, tag="%s flags %d mask %d beta %g" % (tag, flags, masked, beta))
        T = burn + 6 * stride
        assert 3.9 * N <= T <= 4.1 * N + 6
        rate = d["accepted"] / T
        print("%s flags %d mask %d beta %g: acceptance %s" % (tag, flags, masked, beta, np.round(rate, 3).tolist()))
        code = np.where(d["moves"] >= 0, d["moves"], -1 - d["moves"])
        live = d["moves"][:, 0] != INT_MIN
        if masked:
            assert np.all((code[live] // q) % 3 != 1) and np.array_equal(d["Xs"][mask == 0], np.repeat(X[mask == 0][:, None, :], 6, axis=1))
        if not flags:
            assert not live[0::4].any() and np.delete(live, [0, 4]).all()  # the all-gap starts have no site, every other start has some
            assert np.all(code[live] % q != q - 1) and np.array_equal(d["Xs"] == q, np.repeat((X == q)[:, None, :], 6, axis=1))
        else:
            assert live.all()
        if beta == 0.0:
            assert np.all(d["accepted"][live] == T)
        assert np.all(d["accepted"][~live] == 0)


# ---- 2. the thresholds ------------------------------------------------------------------------------------------------------------------------
def test_thresholds_are_within_two_ulp_of_minus_log_u(g, ctx, refdata):
    """thr as the device computed it against -log(u) in np.longdouble: HIP documents 1 ulp for the f64 log, the bar is one more.  The
    ends of u -- u = 1 (thr = 0) and u = 2^-53, the smallest -- are reached with counters constructed for them."""
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 7)
    worst = 0.0
    for seed in (0, 1, 2 ** 64 - 1):
        d = chains(g, ctx, mJ, Pi, X, q, seed=seed, stream0=2 ** 63 - 3, burn=0, stride=1000, n_samples=4)
        for k in range(7):
            ref = sm.thresholds_exact(seed, 2 ** 63 - 3 + k, 4000)
            ulps = np.abs((d["thr"][k].astype(np.longdouble) - ref).astype(np.float64)) / np.spacing(np.abs(ref).astype(np.float64))
            worst = max(worst, float(ulps.max()))
    x = np.asfortranarray(X[:, 1:2])
    for r1, want in ((2 ** 64 - 1, 0.0), (2 ** 64 - 2048, 0.0), (0, 53 * np.log(np.longdouble(2))), (2047, 53 * np.log(np.longdouble(2)))):
        seed = sm.seed_for_draw(r1, 11, 1)
        thr = chains(g, ctx, mJ, Pi, x, q, seed=seed, stream0=11, burn=0, stride=1, n_samples=1)["thr"][0, 0]
        assert sm.uniform53(r1) == (1.0 if want == 0.0 else 2.0 ** -53)
        if want == 0.0:
            assert thr == 0.0
        else:
            ulps = abs(float(np.longdouble(thr) - want)) / np.spacing(float(want))
            worst = max(worst, ulps)
    print("thresholds: largest distance from -log(u) in longdouble %.3f ulp over %d thresholds and the two ends of u" % (worst, 3 * 7 * 4000))
    assert worst <= 2.0, worst


# ---- 3. the mathematics ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", [0.8, 0.2])
def test_the_mathematics(g, ctx, refdata, pc):
    """The accepted moves are a walk's path: every partial sum of the recorded dE against the exact energy changes of the visited states
    (walk_model.replay_exact) within the summed step bounds of walk_bounds plus the summation's own rounding, 2 u sum_t |S_t| over the
    exact partial sums S_t (one rounding an addition, the 2 for the second order); the final table within e_T; and the energies of the
    samples minus the start's against dE_s within the walk test's bound."""
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", pc)
    N = Zo.shape[1]
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 7)
    T = 2 * N
    d = chains(g, ctx, mJ, Pi, X, q, gaps=True, seed=5, burn=0, stride=1, n_samples=T)  # a sample after every proposal
    E0 = g.sequence_energies(mJ, Pi, X, q, ctx=ctx)
    last = np.asfortranarray(d["Xs"][:, -1, :])
    E1 = g.sequence_energies(mJ, Pi, last, q, ctx=ctx)
    _, B0, _ = em.energies_gather(mJ, Pi, X, q)
    _, B1, _ = em.energies_gather(mJ, Pi, last, q)
    worst = 0.0
    for k in range(7):
        path = sm.accepted_path(d["moves"][k], q)
        n_acc = int(d["accepted"][k])
        assert len(path) == n_acc
        Xv, Vl, B, dEl = sm.replay_exact(mJ, Pi, X[:, k], path, q, n_acc)
        e, bD = sm.walk_bounds(mJ, Xv, path, q, Vl, B, dEl)
        assert np.array_equal(Xv[:, -1], d["Xs"][:, -1, k])
        exact = np.array([dEl[t, path[t, 0], path[t, 1] - 1] for t in range(n_acc)], dtype=np.longdouble)
        step_b = np.array([bD[t, path[t, 0], path[t, 1] - 1] for t in range(n_acc)])
        S = np.concatenate(([0], np.cumsum(exact)))
        bound = np.concatenate(([0.0], np.cumsum(step_b) + 2.0 * U * np.cumsum(np.abs(S[1:]).astype(np.float64))))
        at = np.cumsum(d["moves"][k] >= 0)  # accepted moves behind each sample
        err = np.abs((d["dE_s"][k].astype(np.longdouble) - S[at]).astype(np.float64))
        assert np.all(err <= bound[at]), (k, float((err[at > 0] / bound[at][at > 0]).max()))
        if n_acc == 0:
            continue
        errV = np.abs((d["V"][k].astype(np.longdouble) - Vl[n_acc]).astype(np.float64))
        assert np.all(errV <= e[n_acc]), (k, float((errV[:, :q - 1] / e[n_acc][:, :q - 1]).max()))
        assert np.all(d["V"][k][:, q - 1] == 0.0) and not np.signbit(d["V"][k][:, q - 1]).any()
        worst = max(worst, float((err[at > 0] / bound[at][at > 0]).max()), float((errV[:, :q - 1] / e[n_acc][:, :q - 1]).max()))
        tol = em.order_bound(N, q, B0[k]) + em.order_bound(N, q, B1[k]) + float(step_b.sum())
        gap = abs((E1[k] - E0[k]) - d["dE_s"][k, -1])
        print("k %d: %3d of %d accepted, dE_s %.6g, |energy difference - dE_s| = %.3g, tolerance %.3g" % (k, n_acc, T, d["dE_s"][k, -1], gap, tol))
        assert gap <= tol, (k, gap, tol)
    print("pc %g: largest error / bound %.3g" % (pc, worst))


# ---- 4. order fixed ----------------------------------------------------------------------------------------------------------------------------
def test_a_batch_is_its_chains_run_one_at_a_time_and_runs_repeat(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    N = Zo.shape[1]
    X = mixed_sequences(np.random.default_rng(5), Zo, q, 300, shift=1)
    kw = dict(gaps=True, beta=1.0, seed=9, burn=N, stride=7, n_samples=5)
    a = chains(g, ctx, mJ, Pi, X, q, stream0=40, **kw)
    same(a, chains(g, ctx, mJ, Pi, X, q, stream0=40, **kw), "run to run")
    for k in (0, 66, 257, 299):
        same(chain_of(a, k), chains(g, ctx, mJ, Pi, np.asfortranarray(X[:, k:k + 1]), q, stream0=40 + k, **kw), "alone %d" % k)
    # the same start on another stream is another chain; at another place with its stream it is the same chain
    Y = X.copy(order="F")
    Y[:, 3] = X[:, 257]
    b = chains(g, ctx, mJ, Pi, Y, q, stream0=40 + 257 - 3, **kw)
    same(chain_of(b, 3), chain_of(a, 257), "position")


@pytest.mark.parametrize("N", [53, 200])
def test_table_in_lds_and_in_hbm_give_the_same_bits(g, N):
    Zo, q, mJ, Pi = synth_model(21, N)
    X = mixed_sequences(np.random.default_rng(N), Zo, q, 9)
    kw = dict(gaps=True, seed=N, stream0=1, burn=N, stride=N, n_samples=2)
    out = {}
    for where in ("lds", "hbm", "auto"):
        c = g.Context(0)
        try:
            c.set_option("WALK_TABLE", where)
            out[where] = chains(g, c, mJ, Pi, X, q, **kw)
            Xs, dE_s, acc = g.sample(mJ, Pi, X, q, ctx=c, **kw)  # without the table and the trace: the tables live in the context's workspace
            assert np.array_equal(Xs, out[where]["Xs"]) and np.array_equal(dE_s, out[where]["dE_s"]) and np.array_equal(acc, out[where]["accepted"])
        finally:
            c.close()
    same(out["lds"], out["hbm"], "lds / hbm")
    same(out["lds"], out["auto"], "lds / auto")
    print("N %d: accepted %s of %d" % (N, out["lds"]["accepted"].tolist(), 3 * N))


@pytest.mark.parametrize("where", ["lds", "hbm"])
def test_the_cut_into_launches_does_not_matter(g, refdata, where):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 7)
    kw = dict(gaps=False, seed=3, stream0=2, burn=20, stride=13, n_samples=10, mask=(np.arange(53) % 5 != 0))
    out = {}
    for chunk in (1, 7, 64, 0):
        c = g.Context(0)
        try:
            c.set_option("WALK_TABLE", where)
            c.set_option("SAMPLE_CHUNK", chunk)
            out[chunk] = chains(g, c, mJ, Pi, X, q, **kw)
            short = g.sample(mJ, Pi, X, q, ctx=c, **kw)
            assert np.array_equal(short[0], out[chunk]["Xs"]) and np.array_equal(short[1], out[chunk]["dE_s"])
        finally:
            c.close()
    for chunk in (1, 7, 64):
        same(out[chunk], out[0], "SAMPLE_CHUNK %d" % chunk)
    print("accepted %s of 150" % out[0]["accepted"].tolist())
    c = g.Context(0)
    try:
        for bad in ("-1", "x", ""):
            with pytest.raises(g.ArgumentError):
                c.set_option("SAMPLE_CHUNK", bad)
        c.set_option("GDCA_SAMPLE_CHUNK", "4096")
    finally:
        c.close()


def test_only_the_lower_triangle_is_read(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 7)
    kw = dict(gaps=True, seed=1, burn=53, stride=53, n_samples=2)
    a = chains(g, ctx, mJ, Pi, X, q, **kw)
    bad = mJ.copy()
    bad[np.tril_indices_from(bad, -1)] = np.nan  # (numpy's strict lower triangle is the library's strict upper one: tests/test_gpu_walk.py)
    same(a, chains(g, ctx, bad, Pi, X, q, **kw), "NaN in the triangle that is not read")


# ---- 5. lengths ------------------------------------------------------------------------------------------------------------------------------
def test_lengths(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    N = Zo.shape[1]
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 7)
    kw = dict(gaps=False, seed=2, stream0=7)
    burn, stride = 17, 11
    five = chains(g, ctx, mJ, Pi, X, q, burn=burn, stride=stride, n_samples=5, **kw)
    three = chains(g, ctx, mJ, Pi, X, q, burn=burn, stride=stride, n_samples=3, **kw)
    T3 = burn + 3 * stride
    assert np.array_equal(three["Xs"], five["Xs"][:, :3]) and np.array_equal(three["dE_s"], five["dE_s"][:, :3])
    assert np.array_equal(three["thr"], five["thr"][:, :T3]) and np.array_equal(three["moves"], five["moves"][:, :T3])
    assert np.array_equal(three["accepted"], (five["moves"][:, :T3] >= 0).sum(axis=1))
    # sample j is the state after proposal burn + (j + 1) stride - 1: against the chain sampled after every proposal
    T5 = burn + 5 * stride
    every = chains(g, ctx, mJ, Pi, X, q, burn=0, stride=1, n_samples=T5, **kw)
    at = burn + (np.arange(5) + 1) * stride - 1
    assert np.array_equal(every["Xs"][:, at], five["Xs"]) and np.array_equal(every["dE_s"][:, at], five["dE_s"])
    assert np.array_equal(every["moves"], five["moves"]) and np.array_equal(every["V"], five["V"])
    zero = chains(g, ctx, mJ, Pi, X, q, burn=T5 - 1, stride=1, n_samples=1, **kw)  # one sample, behind the last proposal
    assert np.array_equal(zero["Xs"][:, 0], five["Xs"][:, 4]) and np.array_equal(zero["V"], five["V"])
    # beta = 0 accepts every proposal
    hot = chains(g, ctx, mJ, Pi, X, q, beta=0.0, burn=0, stride=N, n_samples=2, **kw)
    live = [1, 2, 3, 5, 6]  # (0 and 4 are the all-gap starts)
    assert np.all(hot["accepted"][live] == 2 * N) and np.all(hot["moves"][live] >= 0) and np.all(hot["accepted"][[0, 4]] == 0)
    # an empty site list: the all-gap start without GDCA_SAMPLE_GAPS, and a mask that lets nothing change
    for d, ks in ((five, [0, 4]), (chains(g, ctx, mJ, Pi, X, q, mask=np.zeros(N, dtype=np.int8), burn=3, stride=2, n_samples=5, **kw), range(7))):
        for k in ks:
            assert d["accepted"][k] == 0 and np.all(d["moves"][k] == INT_MIN) and np.all(d["dE_s"][k] == 0.0)
            assert np.array_equal(d["Xs"][:, :, k], np.repeat(X[:, k:k + 1], 5, axis=1))
            assert np.all(d["thr"][k] >= 0.0)
    V0 = g.mutation_scan(mJ, Pi, X, q, what="potential", ctx=ctx)
    assert np.array_equal(five["V"][0], V0[0])


# ---- 6. the distribution on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, sm.GAPS])
def test_the_device_samples_the_boltzmann_distribution(g, ctx, flags):
    """tests/test_sample_cpu.py's statistical test with the library in emulate's place: the same model, start, K, burn and chain seed"""
    def run(mJ, Pi, X, q, fl, beta, seed):
        return g.sample(mJ, Pi, X, q, beta=beta, burn=TOY_BURN, stride=1, n_samples=1, seed=seed, gaps=bool(fl), ctx=ctx)[0][:, 0, :].T

    Xs, states, p = toy_chains(flags, 1.0, TOY_CHAIN_SEED, run)
    pv, x2, df = sm.chi2_p(Xs, states, p, 4)
    Xw, _, _ = toy_chains(flags, 1.1, TOY_CHAIN_SEED, run)
    pw, x2w, _ = sm.chi2_p(Xw, states, p, 4)
    print("flags %d: chi2 %.1f on %d degrees of freedom, p = %.3g; beta x 1.1: chi2 %.1f, p = %.3g" % (flags, x2, df, pv, x2w, pw))
    assert pv >= P_PASS, pv
    assert pw < P_POWER, pw


# ---- 7. fused ----------------------------------------------------------------------------------------------------------------------------------
def test_fused_is_the_operator_on_the_librarys_own_model(g, ctx, refdata):
    Zo, q, _, _ = golden_model(refdata, "small.fasta.gz", 0.8)
    M, N = Zo.shape
    Zf = np.asfortranarray(Zo.T)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 7)
    pc = 0.8
    Pi_true, Pij_true, _, _ = g.compute_weighted_frequencies(Zf, q, ":auto", ctx=ctx)
    Pi, Pij = g.add_pseudocount(Pi_true, Pij_true, pc, q, ctx=ctx)
    mJ = g.inv_cholesky(g.compute_C(Pi, Pij, ctx=ctx), ctx=ctx)
    mJ = np.tril(mJ) + np.tril(mJ, -1).T
    kw = dict(beta=1.5, seed=4, stream0=9, burn=N, stride=N, n_samples=3)
    for flags in (0, 1):
        op = chains(g, ctx, mJ, Pi, X, q, gaps=bool(flags), **kw)
        res, st = ctx.run_sample_ptr(Zf.ctypes.data, N, M, q, pc, -1.0, X.ctypes.data, 7, flags=flags, trace=True, table=True, **kw)
        same(dict(zip(NAMES, res)), op, "fused / operator, flags %d" % flags)
        assert st["ms_fn"] == 0.0 and st["ms_score"] > 0.0 and st["ms_total"] >= st["ms_score"]
    print("accepted %s of %d" % (op["accepted"].tolist(), 4 * N))
    # X = None starts a chain from each of Z's own sequences
    own, st = ctx.run_sample_ptr(Zf.ctypes.data, N, M, q, pc, -1.0, burn=5, stride=3, n_samples=2, seed=1, trace=True)
    assert own[0].shape == (N, 2, M) and own[1].shape == (M, 2) and own[2].shape == (M,) and own[3].shape == (M, 11) and st["M"] == M
    given, _ = ctx.run_sample_ptr(Zf.ctypes.data, N, M, q, pc, -1.0, Zf.ctypes.data, M, burn=5, stride=3, n_samples=2, seed=1, trace=True)
    for a, b in zip(own, given):
        assert np.array_equal(a, b)
    # the file-level entry
    fasta = os.path.join(refdata, "small.fasta.gz")
    res, _ = ctx.run_sample_ptr(Zf.ctypes.data, N, M, q, pc, -1.0, X.ctypes.data, 7, trace=True, **kw)
    top = g.gDCA_sample(fasta, X, trace=True, ctx=ctx, **kw)
    assert len(top) == 5 and g.gdca.last_stats["ms_fn"] == 0.0
    for a, b in zip(top, res):
        assert np.array_equal(a, b)
    short = g.gDCA_sample(fasta, burn=5, stride=3, n_samples=2, seed=1, ctx=ctx)
    assert len(short) == 3 and all(np.array_equal(a, b) for a, b in zip(short, own[:3]))
    # the samples are an alignment as they lie
    E = g.sequence_energies(mJ, Pi, np.asfortranarray(top[0].reshape(N, -1, order="F")), q, ctx=ctx)
    assert E.shape == (21,) and np.all(np.isfinite(E))


def test_the_device_pointer_wrapper_is_the_host_form(g, ctx, refdata):
    from gaussdca.jl_amd import devops

    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    N, K = Zo.shape[1], 7
    X = mixed_sequences(np.random.default_rng(7), Zo, q, K)
    kw = dict(beta=1.0, burn=N, stride=N, n_samples=2, seed=6, stream0=1)
    host = chains(g, ctx, mJ, Pi, X, q, gaps=True, **kw)
    up = lambda a: g.DeviceBuffer.from_array(ctx, a)  # noqa: E731
    dXs, dacc, ddE, dthr, dmoves, dV = devops.sample_dev(ctx, up(mJ), up(Pi), N, q, up(X), K, flags=g._lib.SAMPLE_GAPS,
                                                         want=("dE_s", "thr", "moves", "V"), **kw)
    T = 3 * N
    dev = dict(Xs=dXs.download((N, 2, K), np.int8), dE_s=ddE.download((K, 2), order="C"), accepted=dacc.download((K,), np.int32),
               thr=dthr.download((K, T), order="C"), moves=dmoves.download((K, T), np.int32, order="C"), V=dV.download((K, N, q), order="C"))
    same(dev, host, "devops.sample_dev / sample")
    only = devops.sample_dev(ctx, up(mJ), up(Pi), N, q, up(X), K, flags=g._lib.SAMPLE_GAPS, want=(), **kw)
    assert only[2:] == (None, None, None, None) and np.array_equal(only[0].download((N, 2, K), np.int8), host["Xs"])


@pytest.mark.parametrize("option,value,refined", [("CHOLESKY", 2, 2), ("REFINE", 1, 1)])
def test_fused_chains_through_the_collect_time_branches(g, refdata, option, value, refined):
    """the stage runs AGAIN at collect time after the Cholesky fallback and after a Newton-Schulz step: the chains returned are chains
    on the model finally used, started anew -- the count agrees with the trace of the same run, and the state space is kept"""
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    N = Zo.shape[1]
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 7)
    c = g.Context(0)
    try:
        c.set_option(option, value)
        Xs, dE_s, acc, thr, moves = g.gDCA_sample(os.path.join(refdata, "small.fasta.gz"), X, burn=N, stride=N, n_samples=1, seed=2, trace=True, ctx=c)
        assert g.gdca.last_stats["refined"] == refined
    finally:
        c.close()
    assert np.array_equal(acc, (moves >= 0).sum(axis=1)) and np.all(acc[[0, 4]] == 0) and np.all(moves[[0, 4]] == INT_MIN)
    assert np.all(moves[[1, 2, 3, 5, 6]] != INT_MIN) and np.all(np.isfinite(dE_s)) and np.all(thr >= 0.0)
    assert np.array_equal(Xs[:, 0, :] == q, X == q)


def test_a_pending_context_refuses_the_host_forms(g, refdata):
    from gaussdca.jl_amd.synth import synth_family

    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 7)
    Z = np.ascontiguousarray(synth_family(12, 200, 5, 11))
    c = g.Context(0)
    try:
        c.run_ranked_async_ptr(Z.ctypes.data, 12, 200, 5, 0.5, 0.2, 0, 1)
        with pytest.raises(g.ArgumentError, match="still enqueued"):
            g.sample(mJ, Pi, X, q, burn=0, stride=1, n_samples=4, ctx=c)
        with pytest.raises(g.ArgumentError, match="still enqueued"):
            c.run_sample_ptr(np.asfortranarray(Zo.T).ctypes.data, Zo.shape[1], Zo.shape[0], q, 0.8, -1.0, X.ctypes.data, 7, n_samples=4)
        i1, j1, s1, st1 = c.run_ranked_collect()
        assert len(s1) > 0
        assert g.sample(mJ, Pi, X, q, beta=0.0, burn=0, stride=1, n_samples=4, ctx=c)[2].max() == 4
    finally:
        c.close()


def test_refusals(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    M, N = Zo.shape
    K, S = 7, 4
    X = mixed_sequences(np.random.default_rng(7), Zo, q, K)
    kw = dict(seed=1, burn=2, stride=3, n_samples=S)
    good = chains(g, ctx, mJ, Pi, X, q, **kw)
    Y = X.copy(order="F")
    Y[7, 5] = q + 1
    with pytest.raises(g.ArgumentError):
        g.sample(mJ, Pi, Y, q, ctx=ctx, **kw)
    with pytest.raises(g.ArgumentError):
        g.gDCA_sample(os.path.join(refdata, "small.fasta.gz"), Y, ctx=ctx, **kw)
    same(chains(g, ctx, mJ, Pi, X, q, **kw), good, "the context still works")

    # straight at the C-ABI: nothing is run, the outputs are untouched
    lib, p, EINVAL = ctx.lib, g._lib._p, g._lib.GDCA_EINVAL
    T = 2 + 3 * S
    Xs, dE_s, acc = np.full((N, S, K), 77, dtype=np.int8, order="F"), np.full((K, S), np.nan), np.full(K, -7, dtype=np.int32)
    thr, moves, V = np.full((K, T), np.nan), np.full((K, T), -7, dtype=np.int32), np.full((K, N, q), np.nan)
    outs = (p(Xs), p(dE_s), p(acc), p(thr), p(moves), p(V))

    def op(mJ_=p(mJ), Pi_=p(Pi), N_=N, q_=q, X_=p(X), K_=K, flags=0, beta=1.0, burn=2, stride=3, S_=S, outs_=outs):
        return lib.gdca_sample(ctx.h, mJ_, Pi_, N_, q_, X_, K_, None, flags, beta, 1, 0, burn, stride, S_, *outs_)

    assert op(K_=0) == EINVAL and op(K_=-1) == EINVAL and op(K_=2 ** 31 - 256) == EINVAL
    assert op(q_=1) == EINVAL and op(q_=32) == EINVAL and op(q_=2) == EINVAL  # (q = 2 without the flag: one target symbol)
    assert op(beta=-1e-300) == EINVAL and op(beta=float("nan")) == EINVAL and op(beta=float("inf")) == EINVAL
    assert op(burn=-1) == EINVAL and op(stride=0) == EINVAL and op(S_=0) == EINVAL and op(S_=-2) == EINVAL
    assert op(burn=2 ** 31 - 4, stride=1, S_=4) == EINVAL and op(burn=0, stride=2 ** 30, S_=2) == EINVAL  # n_steps = 2^31
    assert op(flags=2) == EINVAL and op(flags=3) == EINVAL and op(flags=-1) == EINVAL
    assert op(X_=None) == EINVAL and op(mJ_=None) == EINVAL and op(Pi_=None) == EINVAL
    assert op(outs_=(None,) + outs[1:]) == EINVAL and op(outs_=outs[:2] + (None,) + outs[3:]) == EINVAL
    prm, st = g._lib.Params(0.8, -1.0, 0, 1), g._lib.Stats()
    Zf = np.asfortranarray(Zo.T)

    def fused(Z_=p(Zf), q_=q, X_=p(X), K_=K, flags=0, beta=1.0, burn=2, stride=3, S_=S, outs_=outs, prm_=C.byref(prm)):
        return lib.gdca_run_sample(ctx.h, Z_, N, M, q_, prm_, X_, K_, None, flags, beta, 1, 0, burn, stride, S_, *outs_, C.byref(st))

    assert fused(K_=0) == EINVAL and fused(q_=32) == EINVAL and fused(beta=-1.0) == EINVAL and fused(beta=float("nan")) == EINVAL
    assert fused(burn=-1) == EINVAL and fused(stride=0) == EINVAL and fused(S_=0) == EINVAL and fused(flags=4) == EINVAL
    assert fused(Z_=None) == EINVAL and fused(prm_=None) == EINVAL
    assert fused(outs_=(None,) + outs[1:]) == EINVAL and fused(outs_=outs[:2] + (None,) + outs[3:]) == EINVAL
    assert np.all(Xs == 77) and np.all(acc == -7) and np.all(moves == -7)
    assert np.all(np.isnan(dE_s)) and np.all(np.isnan(thr)) and np.all(np.isnan(V))
    # a table that cannot live in LDS, asked into LDS
    c = g.Context(0)
    try:
        c.set_option("WALK_TABLE", "lds")
        big = np.ones((1000, 1), dtype=np.int8, order="F")
        rc = c.lib.gdca_sample(c.h, p(mJ), p(Pi), 1000, 21, p(big), 1, None, 0, 1.0, 1, 0, 2, 3, S, *outs)  # (refused before mJ is looked at)
        assert rc == EINVAL and b"LDS" in c.lib.gdca_last_error(c.h)
    finally:
        c.close()
    assert np.all(Xs == 77) and np.all(acc == -7)
    same(chains(g, ctx, mJ, Pi, X, q, **kw), good, "the context still works")


# ---- 8. a table too big for LDS ---------------------------------------------------------------------------------------------------------------
def test_a_big_table(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "large.fasta.gz", 0.8)
    N = Zo.shape[1]
    assert (N, q) == (400, 21) and N * q * 8 > 64 * 1024
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 4)
    V0 = g.mutation_scan(mJ, Pi, X, q, what="potential", ctx=ctx)
    d = assert_is_the_rule(g, ctx, mJ, Pi, X, q, V0, None, sm.GAPS, 1.0, seed=8, burn=100, stride=50, n_samples=2, tag="large")
    print("large: accepted", d["accepted"].tolist(), "of 200")
    assert d["accepted"].max() >= 100
    # the other instance and the other paths at this width (N > 256: every loop over the sites takes a second pass): the table asked
    # into LDS and into HBM (k_sample<true>, k_sample<false>), a mask, and the 200 proposals cut into launches of 97, 97 and 6 -- each
    # the rule from the same V0, and all of them the same bits
    mask = (np.arange(N) % 3 == 0).astype(np.int8)
    for m in (None, mask):
        runs = {}
        for where in ("lds", "hbm"):
            for chunk in (0, 97):
                c = g.Context(0)
                try:
                    c.set_option("WALK_TABLE", where)
                    c.set_option("SAMPLE_CHUNK", chunk)
                    runs[where, chunk] = assert_is_the_rule(g, c, mJ, Pi, X, q, V0, m, sm.GAPS, 1.0, seed=8, burn=100, stride=50, n_samples=2,
                                                            tag="large mask %d %s chunk %d" % (m is not None, where, chunk))
                finally:
                    c.close()
        for key, r in runs.items():
            same(r, runs["lds", 0], "mask %d: %s / lds in one launch" % (m is not None, key))
        a = runs["lds", 0]
        print("large mask %d: accepted %s of 200" % (m is not None, a["accepted"].tolist()))
        if m is None:
            same(a, d, "default placement")
        else:
            code = np.where(a["moves"] >= 0, a["moves"], -1 - a["moves"])
            assert np.all((code // q) % 3 == 0) and a["accepted"].max() >= 100
            assert np.array_equal(a["Xs"][mask == 0], np.repeat(X[mask == 0][:, None, :], 2, axis=1))
