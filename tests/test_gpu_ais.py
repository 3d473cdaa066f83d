"""Annealed importance sampling on the device (gdca_log_partition*, log_partition, potts_loglik) against tests/ais_model.py: the rule
of include/gdca.h bit for bit (emulate, from the device's own start tables, start energies and thresholds), the thresholds against
-log(u) in np.longdouble, what the outputs may not depend on -- the position in the batch, where the table lives, how the chain is
cut into launches, host or device pointers --, the reduction against np.longdouble, and the estimate against the exact partition
function of a toy model.  No tolerance is invented here."""
import numpy as np
import pytest

import ais_model as am
import sample_model as sm
from gdca_testutil import ctx, g, golden_model, synth_model  # noqa: F401 (g, ctx: fixtures)
from test_ais_cpu import TOY_K, assert_estimates_z, toy_log_z
from test_sample_cpu import TOY_MODEL_SEED
from test_walk_cpu import tie_model

pytestmark = pytest.mark.gpu

NAMES = ("out4", "logw", "E_end", "X0", "Xout", "accepted", "thr", "moves")
INT_MIN = np.iinfo(np.int32).min
LADDER = np.linspace(0.0, 1.0, 7)  # L = 6
U = 2.0 ** -53


def ais(g, ctx, mJ, Pi, q, betas, sweep, K, x=None, mask=None, flags=0, seed=0, stream0=0):
    """gdca_log_partition with every output, as a dict of NAMES"""
    mJ, Pi = np.ascontiguousarray(mJ, dtype=np.float64), np.ascontiguousarray(Pi, dtype=np.float64)
    N = Pi.shape[0] // (q - 1)
    b = np.ascontiguousarray(betas, dtype=np.float64)
    L = b.size - 1
    out = ctx.log_partition_outputs(N, K, L * sweep, True)
    p = g._lib._p
    xa, ma = (None if a is None else np.ascontiguousarray(a, dtype=np.int8) for a in (x, mask))
    ctx.check(ctx.lib.gdca_log_partition(ctx.h, p(mJ), p(Pi), N, q, None if xa is None else p(xa), None if ma is None else p(ma), flags, p(b), L,
                                         sweep, K, seed, stream0, *[p(a) for a in out]))
    return dict(zip(NAMES, out))


def same(a, b, what="", names=NAMES):
    for n in names:
        assert np.array_equal(a[n], b[n], equal_nan=True), (what, n)


def assert_is_the_rule(g, ctx, mJ, Pi, q, betas, sweep, K, x=None, mask=None, flags=0, seed=0, stream0=0, tag=""):
    """every output of the device's chains == ais_model: the starts, then emulate from the device's own V0 (mutation_scan of the
    returned X0), the device's own E0 (sequence_energies) and the device's own thresholds, chain by chain"""
    N = Pi.shape[0] // (q - 1)
    L = len(betas) - 1
    d = ais(g, ctx, mJ, Pi, q, betas, sweep, K, x, mask, flags, seed, stream0)
    assert np.array_equal(d["X0"], am.starts(x, q, mask, flags, seed, stream0, K, N=N)), tag
    V0 = g.mutation_scan(mJ, Pi, d["X0"], q, what="potential", ctx=ctx)
    E0 = g.sequence_energies(mJ, Pi, d["X0"], q, ctx=ctx)
    for k in range(K):
        moves, acc, xout, logw, E_end = am.emulate(V0[k], E0[k], mJ, d["X0"][:, k], q, betas, sweep, d["thr"][k], mask, flags, seed, stream0 + k)
        what = (tag, k, int(d["accepted"][k]), acc)
        assert np.array_equal(d["moves"][k], moves), what
        assert d["accepted"][k] == acc, what
        assert np.array_equal(d["Xout"][:, k], xout), what
        assert d["logw"][k] == logw and np.signbit(d["logw"][k]) == np.signbit(logw), what + (d["logw"][k], logw)
        assert d["E_end"][k] == E_end, what
    n_sites = len(sm.sites_of(am.template_of(x, q, N), q, mask, flags))
    if n_sites:
        assert (d["moves"] >= 0).any() and (d["moves"] < 0).any(), tag  # an accepted and a rejected proposal
        assert d["accepted"].sum() == (d["moves"] >= 0).sum()
    # out4 of these log-weights (test 4 holds it at width)
    ref = am.reduce_exact(d["logw"], n_sites, sm.targets(q, flags))
    assert abs(float(d["out4"][0] - ref[0])) <= (K + 16) * U * max(1.0, abs(float(ref[0]))), tag
    assert d["out4"][2] == d["logw"].max() and abs(float(d["out4"][3] - ref[3])) <= 2 * np.spacing(float(ref[3])), tag
    print("%s: accepted %s of %d, log Z %.4f, ess %.2f of %d" % (tag, d["accepted"].tolist(), L * sweep, d["out4"][0], d["out4"][1], K))
    return d, E0


# ---- 1. the rule, bit for bit --------------------------------------------------------------------------------------------------------------
def small_case(refdata):
    """the golden model (N = 53, q = 21, n = 1060 rows: several rows a thread), a template from the family, a mask"""
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    gaps = (Zo == q).sum(axis=1)
    x = np.ascontiguousarray(Zo[np.nonzero((gaps > 0) & (gaps < 20))[0][0]], dtype=np.int8)
    mask = (np.arange(Zo.shape[1]) % 3 != 1).astype(np.int8)
    return mJ, Pi, q, x, mask


def synth_case():
    """N = 70, q = 5 with gaps and no template: more than 64 free sites (the second ballot word of the list, starts at positions >= 64),
    n = 280 rows, no multiple of 256"""
    _, q, mJ, Pi = synth_model(5, 70)
    return mJ, Pi, q


def test_the_rule_small_model_mask_template(g, ctx, refdata):
    mJ, Pi, q, x, mask = small_case(refdata)
    assert (x == q).any() and (x[mask != 0] != q).any()
    d, _ = assert_is_the_rule(g, ctx, mJ, Pi, q, LADDER, 5, 5, x, mask, 0, seed=2, stream0=3, tag="small")
    fixed = (mask == 0) | (x == q)
    assert np.array_equal(d["Xout"][fixed], np.repeat(x[fixed, None], 5, axis=1)) and np.all(d["Xout"][~fixed] != q)


def test_the_rule_more_than_64_free_sites(g, ctx):
    mJ, Pi, q = synth_case()
    assert Pi.shape[0] == 280
    d, _ = assert_is_the_rule(g, ctx, mJ, Pi, q, LADDER, 5, 5, None, None, sm.GAPS, seed=1, stream0=0, tag="synth q 5 N 70")
    code = np.where(d["moves"] >= 0, d["moves"], -1 - d["moves"])
    assert (code // q >= 64).any() and (d["X0"][64:] != d["X0"][64:, :1]).any()


def test_the_rule_ties(g, ctx):
    mJ, Pi, x, _ = tie_model()
    assert_is_the_rule(g, ctx, mJ, Pi, 3, LADDER, 5, 5, x, None, 0, seed=4, stream0=1, tag="ties")
    assert_is_the_rule(g, ctx, mJ, Pi, 3, LADDER, 5, 5, x, None, sm.GAPS, seed=4, stream0=1, tag="ties, gaps")


def test_the_rule_no_free_site(g, ctx, refdata):
    mJ, Pi, q, _, _ = small_case(refdata)
    x = np.full(53, q, dtype=np.int8)
    d, E0 = assert_is_the_rule(g, ctx, mJ, Pi, q, LADDER, 5, 5, x, None, 0, seed=5, tag="all gaps")
    assert np.all(d["moves"] == INT_MIN) and np.all(d["accepted"] == 0) and np.array_equal(d["Xout"], d["X0"]) and np.all(d["X0"] == q)
    want = np.float64(0.0)
    for l in range(1, 7):
        want = want + (LADDER[l - 1] - LADDER[l]) * (E0[0] + 0.0)
    assert np.all(d["logw"] == want) and np.all(d["E_end"] == E0[0] + 0.0) and d["out4"][3] == 0.0
    assert d["out4"][1] == 5.0  # (equal weights: every e_k is exp(0))


def test_the_rule_one_stage_is_plain_importance_sampling(g, ctx, refdata):
    mJ, Pi, q, x, mask = small_case(refdata)
    d, E0 = assert_is_the_rule(g, ctx, mJ, Pi, q, np.array([0.0, 0.7]), 5, 5, x, mask, sm.GAPS, seed=6, tag="L = 1")
    assert np.array_equal(d["logw"], (0.0 - 0.7) * (E0 + 0.0))


def test_the_rule_non_monotonic_ladder(g, ctx, refdata):
    mJ, Pi, q, x, _ = small_case(refdata)
    assert_is_the_rule(g, ctx, mJ, Pi, q, np.array([0.0, 0.6, 0.3, 1.0]), 5, 5, x, None, 0, seed=7, tag="ladder 0, 0.6, 0.3, 1")


# ---- 2. the thresholds ------------------------------------------------------------------------------------------------------------------------
def test_thresholds_are_within_two_ulp_of_minus_log_u(g, ctx, refdata):
    """thr as the device computed it against -log(u) in np.longdouble: the bar of tests/test_gpu_sample.py's test of the same name (HIP
    documents 1 ulp for the f64 log, the bar is one more; that test states it as a literal in its body, so it is said again here)"""
    mJ, Pi, q, x, _ = small_case(refdata)
    worst = 0.0
    for seed in (0, 2 ** 64 - 1):
        d = ais(g, ctx, mJ, Pi, q, np.linspace(0, 1, 41), 50, 5, x, None, 0, seed, 2 ** 63 - 3)
        for k in range(5):
            ref = sm.thresholds_exact(seed, 2 ** 63 - 3 + k, 2000)
            ulps = np.abs((d["thr"][k].astype(np.longdouble) - ref).astype(np.float64)) / np.spacing(np.abs(ref).astype(np.float64))
            worst = max(worst, float(ulps.max()))
    print("thresholds: largest distance from -log(u) in longdouble %.3f ulp over %d thresholds" % (worst, 2 * 5 * 2000))
    assert worst <= 2.0, worst


# ---- 3. what the bits may not depend on ---------------------------------------------------------------------------------------------------------
PER_CHAIN = ("logw", "E_end", "X0", "Xout", "accepted", "thr", "moves")


def chain_of(d, k):
    return {n: d[n][:, k:k + 1] if n in ("X0", "Xout") else d[n][k:k + 1] for n in PER_CHAIN}


def test_a_chain_does_not_depend_on_its_place_in_the_batch(g, ctx, refdata):
    mJ, Pi, q, x, mask = small_case(refdata)
    d = ais(g, ctx, mJ, Pi, q, LADDER, 5, 5, x, mask, 0, 3, 10)
    for k in range(5):
        same(ais(g, ctx, mJ, Pi, q, LADDER, 5, 1, x, mask, 0, 3, 10 + k), chain_of(d, k), "chain %d alone" % k, PER_CHAIN)
    # two runs of the same call: out4 to the bit
    same(ais(g, ctx, mJ, Pi, q, LADDER, 5, 5, x, mask, 0, 3, 10), d, "the same call again")


@pytest.mark.parametrize("case", ["small", "synth"])
def test_where_the_table_lives_and_the_cut_into_launches_do_not_matter(g, refdata, case):
    if case == "small":
        mJ, Pi, q, x, mask = small_case(refdata)
        flags = 0
    else:
        (mJ, Pi, q), x, mask, flags = synth_case(), None, None, sm.GAPS
    out = {}
    for where, chunk in (("lds", 0), ("hbm", 0), ("lds", 7), ("hbm", 1), ("lds", 1)):  # sweep 5: cuts inside stages, and at every proposal
        c = g.Context(0)
        try:
            c.set_option("WALK_TABLE", where)
            c.set_option("SAMPLE_CHUNK", chunk)
            out[where, chunk] = ais(g, c, mJ, Pi, q, LADDER, 5, 5, x, mask, flags, 8, 2)
            short = g.log_partition(mJ, Pi, q, betas=LADDER, sweep=5, K=5, x=x, mask=mask, gaps=bool(flags), seed=8, stream0=2, ctx=c)
            assert short[0] == out[where, chunk]["out4"][0] and short[1] == out[where, chunk]["out4"][1]
            assert np.array_equal(short[2], out[where, chunk]["logw"])
        finally:
            c.close()
    for key, r in out.items():
        same(r, out["lds", 0], "%s / lds in one launch" % (key,))
    assert (out["lds", 0]["moves"] >= 0).any()


def test_host_and_device_pointers(g, ctx, refdata):
    from gaussdca.jl_amd import devops

    mJ, Pi, q, x, mask = small_case(refdata)
    N, K, sweep = 53, 5, 5
    T = 6 * sweep
    d = ais(g, ctx, mJ, Pi, q, LADDER, sweep, K, x, mask, 0, 9, 4)
    bufs = []
    for a in (np.asfortranarray(mJ), Pi, x, mask):
        b = g.DeviceBuffer(ctx, a.nbytes)
        b.upload(np.ascontiguousarray(a) if a.ndim == 1 else a)
        bufs.append(b)
    r = devops.log_partition_dev(ctx, bufs[0], bufs[1], N, q, LADDER, sweep, K, dx=bufs[2], dmask=bufs[3], seed=9, stream0=4,
                                 want=("E_end", "X0", "Xout", "accepted", "thr", "moves"))
    shapes = (((4,), np.float64), ((K,), np.float64), ((K,), np.float64), ((N, K), np.int8), ((N, K), np.int8), ((K,), np.int32),
              ((K, T), np.float64), ((K, T), np.int32))
    dev = {n: b.download(s, dtype=t, order="F" if len(s) == 2 and t == np.int8 else "C") for n, b, (s, t) in zip(NAMES, r, shapes)}
    same(dev, d, "_dev form / host-pointer form")
    # only the required outputs
    r2 = devops.log_partition_dev(ctx, bufs[0], bufs[1], N, q, LADDER, sweep, K, dx=bufs[2], dmask=bufs[3], seed=9, stream0=4)
    assert r2[2:] == (None,) * 6
    assert np.array_equal(r2[0].download((4,)), d["out4"]) and np.array_equal(r2[1].download((K,)), d["logw"])


# ---- 4. the reduction ---------------------------------------------------------------------------------------------------------------------------
def test_the_reduction(g, ctx):
    """out4 against ais_model.reduce_exact of the device's own log-weights, K = 1000 (no multiple of 256), a steep ladder on the toy
    model for a wide spread of the weights.  out[0]: all terms of S1 are positive, so the sum of K terms carries at most (K - 1) u
    relative error; exp and log are within 1 ulp each by the HIP math documentation; the rounding of exp's argument adds at most u / e
    a term; three more roundings come from the closing additions: (K + 16) u max(1, |out[0]|).  out[1]: twice that, relative."""
    q, K = 4, 1000
    mJ, Pi = sm.toy_model(TOY_MODEL_SEED)
    d = ais(g, ctx, mJ, Pi, q, np.array([0.0, 2.0, 4.0]), 2, K, None, None, sm.GAPS, 11, 0)
    lw = d["logw"]
    assert np.all(np.isfinite(lw)) and lw.max() - lw.min() > 10.0
    lz, ess, m, lo = am.reduce_exact(lw, 4, 4)
    bar = (K + 16) * U
    print("reduction: spread of logw %.1f, out %s, errors %.3g, %.3g of the bars" % (
        lw.max() - lw.min(), d["out4"].tolist(), abs(float(d["out4"][0] - lz)) / (bar * max(1.0, abs(float(lz)))), abs(float(d["out4"][1] - ess)) / (2 * bar * float(ess))))
    assert d["out4"][2] == lw.max() == float(m)
    assert abs(float(d["out4"][3] - lo)) <= 2 * np.spacing(float(lo)) and abs(d["out4"][3] - 4 * np.log(4.0)) <= 2 * np.spacing(4 * np.log(4.0))
    assert abs(float(d["out4"][0] - lz)) <= bar * max(1.0, abs(float(lz)))
    assert abs(float(d["out4"][1] - ess)) <= 2 * bar * float(ess)
    assert 1.0 <= d["out4"][1] <= K
    # a NaN among the log-weights, through a NaN entry of the model: out[0] and out[1] are NaN, and the call still returns
    bad = mJ.copy()
    bad[0, 0] = np.nan
    dn = ais(g, ctx, bad, Pi, q, np.array([0.0, 2.0, 4.0]), 2, K, None, None, sm.GAPS, 11, 0)
    assert np.isnan(dn["logw"]).any()
    assert np.isnan(dn["out4"][0]) and np.isnan(dn["out4"][1]) and dn["out4"][3] == d["out4"][3]
    same(ais(g, ctx, mJ, Pi, q, np.array([0.0, 2.0, 4.0]), 2, K, None, None, sm.GAPS, 11, 0), d, "the context still works")


# ---- 5. the device estimates Z ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, sm.GAPS])
def test_the_device_estimates_z(g, ctx, flags):
    seen = []

    def run(mJ, Pi, q, flags, betas, sweep, seed):
        logZ, ess, logw = g.log_partition(mJ, Pi, q, betas=betas, sweep=sweep, K=TOY_K, gaps=bool(flags), seed=seed, ctx=ctx)
        seen.append((logZ, ess, logw))
        return logw

    assert_estimates_z(flags, run, "device")
    assert len(seen) == 3
    T = sm.targets(4, flags)
    for logZ, ess, logw in seen:
        # out[0] is log(|Omega| mean(w)) of the returned log-weights, within the reduction's bar
        want = 4 * np.log(np.longdouble(T)) + np.log(np.exp(logw.astype(np.longdouble)).mean())
        assert abs(float(logZ - want)) <= (TOY_K + 16) * U * max(1.0, abs(float(want))), (logZ, float(want))
        assert 1.0 <= ess <= TOY_K


# ---- 6. potts_loglik ----------------------------------------------------------------------------------------------------------------------------
def test_potts_loglik_normalises_the_toy_model(g, ctx):
    """L = -E - logZ_hat over ALL 256 states: logsumexp(L) = log Z_exact - logZ_hat, which must lie within 4 / sqrt(ess), four standard
    errors of the estimator's own relative error 1 / sqrt(ess) (a looser sanity bar than the z test's)"""
    q = 4
    mJ, Pi = sm.toy_model(TOY_MODEL_SEED)
    states, n_sites, T = am.enumerate_states(q, sm.GAPS, None, None, N=4)
    X = np.asfortranarray(states.T)
    L, logZ, ess = g.potts_loglik(mJ, Pi, X, q, gaps=True, n_stages=16, sweep=4, K=4096, seed=3, ctx=ctx)
    assert L.shape == (256,) and np.array_equal(L, -g.sequence_energies(mJ, Pi, X, q, ctx=ctx) - logZ)
    lse = float(np.log(np.exp(L.astype(np.longdouble)).sum()))
    exact = float(toy_log_z(sm.GAPS))
    print("potts_loglik: logsumexp(L) = %.5f, log Z exact %.5f, estimate %.5f, ess %.0f, bar %.4f" % (lse, exact, logZ, ess, 4 / np.sqrt(ess)))
    assert abs(lse - (exact - logZ)) <= 1e-12 and abs(lse) <= 4 / np.sqrt(ess)
    with pytest.raises(g.ArgumentError, match="outside the state space"):
        g.potts_loglik(mJ, Pi, X, q, n_stages=16, K=64, ctx=ctx)  # (gaps among the sequences, none in the state space)
    x = np.array([1, 2, 3, 1], dtype=np.int8)
    with pytest.raises(g.ArgumentError, match="outside the state space"):
        g.potts_loglik(mJ, Pi, X, q, x=x, mask=np.array([1, 1, 0, 1]), gaps=True, n_stages=16, K=64, ctx=ctx)
    inside = np.asfortranarray(X[:, X[2] == 3])
    Lm, logZm, essm = g.potts_loglik(mJ, Pi, inside, q, x=x, mask=np.array([1, 1, 0, 1]), gaps=True, n_stages=16, K=4096, ctx=ctx)
    exact_m = float(am.log_z_exact(mJ, Pi, q, 1.0, sm.GAPS, x, np.array([1, 1, 0, 1])))
    assert inside.shape == (4, 64) and abs(logZm - exact_m) <= 4 / np.sqrt(essm) and abs(float(np.log(np.exp(Lm).sum())) - (exact_m - logZm)) <= 1e-12


# ---- 7. width -----------------------------------------------------------------------------------------------------------------------------------
def test_more_chains_than_compute_units(g, ctx, refdata):
    mJ, Pi, q, x, _ = small_case(refdata)
    K, betas = 300, np.linspace(0.0, 1.0, 21)
    out = g.log_partition(mJ, Pi, q, betas=betas, sweep=53, K=K, x=x, seed=12, trace=True, ctx=ctx)
    logZ, ess, logw, E_end, X0, Xout, accepted, thr, moves = out
    assert logw.shape == (K,) and X0.shape == Xout.shape == (53, K) and thr.shape == moves.shape == (K, 20 * 53)
    assert np.all(accepted > 0) and np.all(np.isfinite(logw)) and np.isfinite(logZ) and 1.0 <= ess <= K
    assert np.array_equal(accepted, (moves >= 0).sum(axis=1))
    for k in (0, 299):
        one = g.log_partition(mJ, Pi, q, betas=betas, sweep=53, K=1, x=x, seed=12, stream0=k, trace=True, ctx=ctx)
        assert one[2][0] == logw[k] and one[3][0] == E_end[k] and np.array_equal(one[5][:, 0], Xout[:, k]) and np.array_equal(one[8][0], moves[k])
    # the default sweep is one sweep of the free sites
    n_sites = int((x != q).sum())
    d = g.log_partition(mJ, Pi, q, n_stages=3, K=2, x=x, seed=12, trace=True, ctx=ctx)
    assert d[7].shape == (2, 3 * n_sites)
    print("width: log Z %.3f, ess %.1f of %d, accepted %d .. %d of %d" % (logZ, ess, K, accepted.min(), accepted.max(), 20 * 53))
