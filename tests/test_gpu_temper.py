"""Replica exchange over the Metropolis chains on the device (gdca_sample_tempered*, gdca_run_sample_tempered*, sample_tempered,
gDCA_sample_tempered) against tests/temper_model.py: the rule of include/gdca.h bit for bit (emulate, from the device's own start
tables, start energies, thresholds and swap thresholds), the swap thresholds against -log(u) in np.longdouble, R = 1 against the plain
chains, what the outputs may not depend on -- K, the position in the batch, where the table lives, how the replicas are cut into
launches, fused or operator --, and the sampled distribution of a toy model with a barrier against the exact one.  No tolerance is
invented here."""
import ctypes as C
import os

import numpy as np
import pytest

import sample_model as sm
import temper_model as tm
from gdca_testutil import ctx, g, golden_model, mixed_sequences, synth_model  # noqa: F401 (g, ctx: fixtures)
from test_sample_cpu import P_PASS, P_POWER
from test_temper_cpu import TOY_CHAIN_SEED
from test_walk_cpu import tie_model

pytestmark = pytest.mark.gpu

NAMES = ("Xs", "E_s", "accepted", "swaps", "Xr_out", "slot_out", "thr", "moves", "swap_thr", "slot_path")


def tempered(g, ctx, mJ, Pi, X, q, **kw):
    """sample_tempered with the traces as a dict of NAMES"""
    return dict(zip(NAMES, g.sample_tempered(mJ, Pi, X, q, trace=True, ctx=ctx, **kw)))


def same(a, b, what="", names=NAMES):
    for n in names:
        assert np.array_equal(a[n], b[n]), (what, n)


def chain_of(d, k):
    """chain k of a batch, as a batch of one"""
    return {n: d[n][..., k:k + 1] if n in ("Xs", "Xr_out") else d[n][k:k + 1] for n in NAMES}


def replicas(X, R):
    """(N, K) -> (N, R, K): every replica of a chain at its chain's start"""
    return np.asfortranarray(np.repeat(X[:, None, :], R, axis=1))


def assert_is_the_rule(g, ctx, mJ, Pi, Xr, q, betas, tag="", **kw):
    """every output of the device's tempered chains == temper_model.emulate from the device's own start tables and energies and the
    device's own thresholds, chain by chain -> the device's outputs"""
    N, R, K = Xr.shape
    flat = np.asfortranarray(Xr.reshape(N, R * K, order="F"))
    V0 = g.mutation_scan(mJ, Pi, flat, q, what="potential", ctx=ctx).reshape(K, R, N, q)
    E0 = g.sequence_energies(mJ, Pi, flat, q, ctx=ctx).reshape(K, R)
    d = tempered(g, ctx, mJ, Pi, Xr, q, betas=betas, **kw)
    S, every = kw["n_samples"], kw["swap_every"]
    T = kw["burn"] + S * kw["stride"]
    E = T // every
    assert d["Xs"].shape == (N, S, K) and d["E_s"].shape == (K, S) and d["accepted"].shape == (K, R) and d["swaps"].shape == (K, R - 1)
    assert d["Xr_out"].shape == (N, R, K) and d["slot_out"].shape == (K, R) and d["thr"].shape == (K, R, T) and d["moves"].shape == (K, R, T)
    assert d["swap_thr"].shape == (K, R - 1, E) and d["slot_path"].shape == (K, R, E)
    slot0 = kw.get("slot0")
    for k in range(K):
        ref = tm.emulate(V0[k], E0[k], mJ, Xr[:, :, k].T, q, betas, d["thr"][k], d["swap_thr"][k].T, mask=kw.get("mask"),
                         flags=sm.GAPS if kw.get("gaps") else 0, seed=kw.get("seed", 0), stream0=kw.get("stream0", 0) + k * R, swap_every=every,
                         burn=kw["burn"], stride=kw["stride"], n_samples=S, slot0=None if slot0 is None else slot0[k])
        what = (tag, k)
        assert np.array_equal(d["moves"][k], ref["moves"]), what
        assert np.array_equal(d["slot_path"][k], ref["slot_path"].T), what
        assert np.array_equal(d["accepted"][k], ref["accepted"]) and np.array_equal(d["swaps"][k], ref["swaps"]), what
        assert np.array_equal(d["Xs"][:, :, k], ref["Xs"].T) and np.array_equal(d["Xr_out"][:, :, k], ref["Xr_out"].T), what
        assert np.array_equal(d["E_s"][k], ref["E_s"]) and np.array_equal(d["slot_out"][k], ref["slot_out"]), what
        # a pair that is not attempted has the threshold +0.0
        idle = ~tm.attempted(R, E).T
        assert np.all(d["swap_thr"][k][idle] == 0.0) and not np.signbit(d["swap_thr"][k][idle]).any() and np.all(d["swap_thr"][k] >= 0.0)
    return d


# ---- 1. the rule, bit for bit --------------------------------------------------------------------------------------------------------------
# model, R, betas, gaps, masked, a slot0 that is not the identity, seed (chosen on the CPU with the numpy checker: every run holds an
# accepted swap, a rejected one and a sample right behind an accepted swap of pair 0 -- asserted below)
RULE_CASES = [("small", 3, (1.0, 0.8, 0.9), False, True, False, 0),
              ("small", 4, (1.0, 0.9, 0.8, 0.7), True, False, True, 0),
              ("synth", 3, (1.0, 0.6, 0.3), True, True, False, 0),
              ("ties", 4, (1.0, 0.7, 0.5, 0.2), False, False, False, 0)]
RULE_SHAPE = dict(swap_every=5, burn=10, stride=5, n_samples=6)


def rule_model(refdata, which):
    if which == "small":
        return golden_model(refdata, "small.fasta.gz", 0.8)
    if which == "synth":
        return synth_model(5, 7)
    mJ, Pi, x, _ = tie_model()
    return np.repeat(x[None, :], 3, axis=0), 3, mJ, Pi


def rule_inputs(refdata, case):
    """(mJ, Pi, Xr (N, R, K), q, keyword arguments) of a case: K = 5 chains whose replicas start at distinct sequences, chain 0 all gaps"""
    which, R, betas, gaps, masked, permuted, seed = case
    Zo, q, mJ, Pi = rule_model(refdata, which)
    N, K = Zo.shape[1], 5
    rng = np.random.default_rng(len(which) + R)
    if masked:  # every replica of a chain at its chain's start (the fused form's start) ...
        Xr = replicas(mixed_sequences(rng, Zo, q, K), R)
    else:       # ... or each replica at a sequence of its own: residues only, family members, random ones
        Xr = np.stack([mixed_sequences(rng, Zo, q, K, shift=r % 2 * 2 + 1) for r in range(R)], axis=1)
    Xr[:, :, 0] = q
    kw = dict(RULE_SHAPE, gaps=gaps, seed=seed, stream0=3)
    if masked:
        kw["mask"] = (np.arange(N) % 3 != 1).astype(np.int8)
    if permuted:
        kw["slot0"] = np.stack([np.roll(np.arange(R), k + 1) for k in range(K)]).astype(np.int32)
    return mJ, Pi, np.asfortranarray(Xr), q, betas, kw


def swap_coverage(d, R, n_samples, swap_every, burn, stride):
    """(accepted swaps, rejected swaps, samples taken right behind an accepted swap of pair 0) of a run's slot_path and swaps"""
    K, _, E = d["slot_path"].shape
    att = tm.attempts(R, E)
    after = 0
    for j in range(n_samples):
        e = (burn + (j + 1) * stride) // swap_every - 1
        if e % 2 == 0 and e > 0:  # pair 0 is attempted in the even rounds: accepted iff the holder of slot 0 changed
            after += int((np.argmin(d["slot_path"][:, :, e], axis=1) != np.argmin(d["slot_path"][:, :, e - 1], axis=1)).sum())
    return int(d["swaps"].sum()), int(K * att.sum() - d["swaps"].sum()), after


@pytest.mark.parametrize("case", RULE_CASES, ids=["%s-R%d" % c[:2] for c in RULE_CASES])
def test_the_rule_bit_for_bit(g, ctx, refdata, case):
    mJ, Pi, Xr, q, betas, kw = rule_inputs(refdata, case)
    d = assert_is_the_rule(g, ctx, mJ, Pi, Xr, q, betas, tag=str(case[:2]), **kw)
    R = len(betas)
    acc, rej, after = swap_coverage(d, R, 6, 5, 10, 5)
    print("%s R %d: accepted proposals by slot %s, swaps accepted %d rejected %d, samples behind a swap of pair 0: %d" %
          (case[0], R, d["accepted"].sum(axis=0).tolist(), acc, rej, after))
    assert acc >= 1 and rej >= 1 and after >= 1
    # the all-gap chain without the flag: nothing can change, its replicas still swap (equal energies: d = 0 <= thr_s)
    if not kw["gaps"]:
        assert np.all(d["accepted"][0] == 0) and np.all(d["moves"][0] == tm.INT_MIN) and np.array_equal(d["swaps"][0], tm.attempts(R, 8))
    # the counts by slot are the counts of the moves, looked up through the slot held at every proposal
    for k in range(5):
        held = np.concatenate((np.repeat((kw["slot0"][k] if "slot0" in kw else np.arange(R))[:, None], 5, axis=1),
                               np.repeat(d["slot_path"][k][:, :-1], 5, axis=1)), axis=1)
        assert np.array_equal(np.bincount(held[d["moves"][k] >= 0], minlength=R), d["accepted"][k])


# ---- 2. the swap thresholds --------------------------------------------------------------------------------------------------------------
def test_swap_thresholds_are_within_two_ulp_of_minus_log_u(g, ctx):
    """swap_thr as the device computed it against -log(u) in np.longdouble (HIP documents 1 ulp for the f64 log, the bar is one more,
    as for the chains' thresholds); the ends of u are reached with counters constructed for them"""
    Zo, q, mJ, Pi = synth_model(5, 7)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 6)
    R, E = 4, 400
    worst, n = 0.0, 0
    for seed in (0, 2 ** 64 - 1):
        d = tempered(g, ctx, mJ, Pi, X, q, betas=(1.0, 0.5, 0.25, 0.0), seed=seed, stream0=2 ** 62, swap_every=1, burn=0, stride=1, n_samples=E)
        for k in range(6):
            ref = tm.swap_thresholds_exact(seed, 2 ** 62, k, R, E)
            on = tm.attempted(R, E)
            got = d["swap_thr"][k].T
            ulps = np.abs((got.astype(np.longdouble) - ref).astype(np.float64))[on] / np.spacing(np.abs(ref).astype(np.float64))[on]
            worst, n = max(worst, float(ulps.max())), n + int(on.sum())
    x = np.asfortranarray(X[:, 1:2])
    for r1, want in ((2 ** 64 - 1, 0.0), (2 ** 64 - 2048, 0.0), (0, 53 * np.log(np.longdouble(2))), (2047, 53 * np.log(np.longdouble(2)))):
        # draw(skey, 0) == r1: skey = mix64(~key), so the chain key is ~unmix64(skey) and the seed is constructed as for a proposal draw
        sk = (sm.unmix64(r1) - sm.G) & sm.M64
        ky = ~sm.unmix64(sk) & sm.M64
        seed = (sm.unmix64((sm.unmix64(ky) - (11 + 1) * sm.G) & sm.M64) - sm.G) & sm.M64
        assert sm.draw(tm.skey(seed, 11, 0, 2), 0) == r1
        thr = tempered(g, ctx, mJ, Pi, x, q, betas=(1.0, 0.5), seed=seed, stream0=11, swap_every=1, burn=0, stride=1, n_samples=1)["swap_thr"][0, 0, 0]
        if want == 0.0:
            assert thr == 0.0
        else:
            worst = max(worst, abs(float(np.longdouble(thr) - want)) / np.spacing(float(want)))
    print("swap thresholds: largest distance from -log(u) in longdouble %.3f ulp over %d thresholds and the two ends of u" % (worst, n))
    assert worst <= 2.0, worst


# ---- 3. one replica is the plain chain ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap_every", [1, 5])
def test_one_replica_is_the_plain_chain(g, ctx, refdata, swap_every):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 7)
    kw = dict(seed=3, stream0=40, burn=10, stride=5, n_samples=6, mask=(np.arange(53) % 5 != 0))
    for gaps, beta in ((False, 1.0), (True, 0.5)):
        plain = g.sample(mJ, Pi, X, q, beta=beta, gaps=gaps, trace=True, ctx=ctx, **kw)
        E0 = g.sequence_energies(mJ, Pi, X, q, ctx=ctx)
        d = tempered(g, ctx, mJ, Pi, X, q, betas=(beta,), gaps=gaps, swap_every=swap_every, **kw)
        assert np.array_equal(d["Xs"], plain[0]) and np.array_equal(d["accepted"][:, 0], plain[2])
        assert np.array_equal(d["thr"][:, 0], plain[3]) and np.array_equal(d["moves"][:, 0], plain[4])
        assert np.array_equal(d["E_s"], E0[:, None] + plain[1])
        assert d["swaps"].shape == (7, 0) and np.all(d["slot_out"] == 0) and np.all(d["slot_path"] == 0)
        assert np.array_equal(d["Xr_out"][:, 0, :], d["Xs"][:, -1, :])


# ---- 4. equal betas ---------------------------------------------------------------------------------------------------------------------------
def test_equal_betas_accept_every_attempted_swap(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 5)
    for R, E in ((2, 7), (5, 8), (64, 6)):
        d = tempered(g, ctx, mJ, Pi, X, q, betas=(0.9,) * R, gaps=True, seed=R, swap_every=3, burn=3 * (E - 2), stride=3, n_samples=2)
        assert np.array_equal(d["swaps"], np.repeat(tm.attempts(R, E)[None], 5, axis=0))
        # the permutation the schedule implies: every even (odd) round exchanges the holders of the pairs (0, 1), (2, 3), .. ((1, 2), ..)
        holder = np.arange(R)
        for e in range(E):
            for p in range(e % 2, R - 1, 2):
                holder[p], holder[p + 1] = holder[p + 1], holder[p]
        slot = np.empty(R, dtype=np.int32)
        slot[holder] = np.arange(R)
        assert np.array_equal(d["slot_out"], np.repeat(slot[None], 5, axis=0)) and np.array_equal(d["slot_path"][:, :, -1], d["slot_out"])
        assert d["accepted"].sum() > 0


# ---- 5. order fixed ----------------------------------------------------------------------------------------------------------------------------
def test_a_batch_is_its_chains_run_one_at_a_time_and_runs_repeat(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    X = mixed_sequences(np.random.default_rng(5), Zo, q, 70, shift=1)
    R = 3
    kw = dict(betas=(1.0, 0.8, 0.6), gaps=True, seed=9, swap_every=5, burn=20, stride=10, n_samples=3)
    a = tempered(g, ctx, mJ, Pi, X, q, stream0=40, **kw)
    same(a, tempered(g, ctx, mJ, Pi, X, q, stream0=40, **kw), "run to run")
    assert a["swaps"].sum() > 0 and (a["swaps"] < tm.attempts(R, 10)[None]).any()
    for k in (0, 33, 69):
        same(chain_of(a, k), tempered(g, ctx, mJ, Pi, np.asfortranarray(X[:, k:k + 1]), q, stream0=40 + k * R, **kw), "alone %d" % k)
    # a run continues from Xr_out and slot_out?  The streams start anew, so it is another run -- but the hand-over is accepted as it lies
    b = tempered(g, ctx, mJ, Pi, a["Xr_out"], q, stream0=40, slot0=a["slot_out"], **kw)
    assert b["Xs"].shape == a["Xs"].shape and np.all(np.sort(b["slot_out"], axis=1) == np.arange(R))


# ---- 6. where the table lives, how the replicas are cut into launches ----------------------------------------------------------------------
@pytest.mark.parametrize("N", [53, 200])
def test_table_placement_and_the_cut_into_launches_do_not_matter(g, N):
    Zo, q, mJ, Pi = synth_model(21, N)
    X = mixed_sequences(np.random.default_rng(N), Zo, q, 5)
    kw = dict(betas=(1.0, 0.9, 0.8), gaps=True, seed=N, stream0=1, swap_every=5, burn=N // 5 * 5, stride=10, n_samples=2)
    out = {}
    for where, chunk in (("lds", 0), ("hbm", 0), ("auto", 0), ("lds", 1), ("hbm", 1), ("lds", 7), ("hbm", 7), ("auto", 7)):
        c = g.Context(0)
        try:
            c.set_option("WALK_TABLE", where)
            c.set_option("SAMPLE_CHUNK", chunk)
            out[where, chunk] = tempered(g, c, mJ, Pi, X, q, **kw)
        finally:
            c.close()
    for key, r in out.items():
        same(r, out["lds", 0], str(key))
    print("N %d: accepted by slot %s, swaps %s" % (N, out["lds", 0]["accepted"].sum(axis=0).tolist(), out["lds", 0]["swaps"].sum(axis=0).tolist()))


def test_only_the_lower_triangle_is_read(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 7)
    kw = dict(betas=(1.0, 0.7), gaps=True, seed=1, swap_every=53, burn=53, stride=53, n_samples=2)
    a = tempered(g, ctx, mJ, Pi, X, q, **kw)
    bad = mJ.copy()
    bad[np.tril_indices_from(bad, -1)] = np.nan  # (numpy's strict lower triangle is the library's strict upper one: tests/test_gpu_walk.py)
    same(a, tempered(g, ctx, bad, Pi, X, q, **kw), "NaN in the triangle that is not read")


# ---- 8. the barrier toy on the device ----------------------------------------------------------------------------------------------------------
def test_the_device_crosses_the_barrier_the_plain_chains_do_not(g, ctx):
    """tests/test_temper_cpu.py's statistical test with the library in emulate_chains' place: the same model, start, K, budget, ladder and
    chain seed.  Without the tempered entry points no call of the library passes it: the plain chains are seen."""
    def run(mJ, Pi, X, q, betas, seed):
        out = g.sample_tempered(mJ, Pi, X, q, betas=betas, swap_every=tm.TOY_SWAP_EVERY, burn=tm.TOY_STEPS - tm.TOY_SWAP_EVERY,
                                stride=tm.TOY_SWAP_EVERY, n_samples=1, seed=seed, gaps=True, ctx=ctx)
        return out[0][:, 0, :].T, out[3]

    def plain(mJ, Pi, X, q, betas, seed):
        return g.sample(mJ, Pi, X, q, beta=betas[0], burn=tm.TOY_STEPS - 1, stride=1, n_samples=1, seed=seed, gaps=True, ctx=ctx)[0][:, 0, :].T, None

    Xs, rates, states, p = tm.toy_chains(tm.TOY_LADDER, TOY_CHAIN_SEED, run)
    pv, x2, df = sm.chi2_p(Xs, states, p, tm.TOY_Q)
    Xp, _, _, _ = tm.toy_chains((1.0,), TOY_CHAIN_SEED, plain)
    pp, x2p, _ = sm.chi2_p(Xp, states, p, tm.TOY_Q)
    print("ladder: chi2 %.1f on %d degrees of freedom, p = %.3g, swap rates %s; plain: chi2 %.1f, p = %.3g" %
          (x2, df, pv, np.round(rates, 3).tolist(), x2p, pp))
    assert pv >= P_PASS, pv
    assert np.all((rates >= 0.3) & (rates <= 0.95)), rates
    assert pp < P_POWER, pp


# ---- 9. fused ----------------------------------------------------------------------------------------------------------------------------------
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
    kw = dict(betas=(1.5, 1.0, 0.5), seed=4, stream0=9, swap_every=N, burn=N, stride=N, n_samples=3)
    for flags in (0, 1):
        op = tempered(g, ctx, mJ, Pi, X, q, gaps=bool(flags), **kw)
        res, st = ctx.run_sample_tempered_ptr(Zf.ctypes.data, N, M, q, pc, -1.0, X.ctypes.data, 7, flags=flags, trace=True, **kw)
        same(dict(zip(NAMES, res)), op, "fused / operator, flags %d" % flags)
        assert st["ms_fn"] == 0.0 and st["ms_score"] > 0.0 and st["ms_total"] >= st["ms_score"]
    print("accepted by slot %s, swaps %s" % (op["accepted"].sum(axis=0).tolist(), op["swaps"].sum(axis=0).tolist()))
    # X = None starts a chain from each of Z's own sequences
    kw2 = dict(betas=(1.0, 0.5), swap_every=3, burn=6, stride=3, n_samples=2, seed=1)
    own, st = ctx.run_sample_tempered_ptr(Zf.ctypes.data, N, M, q, pc, -1.0, trace=True, **kw2)
    assert own[0].shape == (N, 2, M) and own[2].shape == (M, 2) and own[3].shape == (M, 1) and own[6].shape == (M, 2, 12) and st["M"] == M
    given, _ = ctx.run_sample_tempered_ptr(Zf.ctypes.data, N, M, q, pc, -1.0, Zf.ctypes.data, M, trace=True, **kw2)
    for a, b in zip(own, given):
        assert np.array_equal(a, b)
    # the file-level entry: burn and stride in sweeps
    fasta = os.path.join(refdata, "small.fasta.gz")
    top = g.gDCA_sample_tempered(fasta, X, betas=(1.5, 1.0, 0.5), seed=4, stream0=9, burn=1, stride=1, n_samples=3, ctx=ctx)
    res, _ = ctx.run_sample_tempered_ptr(Zf.ctypes.data, N, M, q, pc, -1.0, X.ctypes.data, 7, **kw)
    assert len(top) == 4 and g.gdca.last_stats["ms_fn"] == 0.0
    for a, b in zip(top, res[:4]):
        assert np.array_equal(a, b)
    E = g.sequence_energies(mJ, Pi, np.asfortranarray(top[0].reshape(N, -1, order="F")), q, ctx=ctx)
    assert E.shape == (21,) and np.all(np.isfinite(E))


def test_the_device_pointer_wrapper_is_the_host_form(g, ctx, refdata):
    from gaussdca.jl_amd import devops

    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    N, K, R = Zo.shape[1], 7, 3
    X = mixed_sequences(np.random.default_rng(7), Zo, q, K)
    Xr = replicas(X, R)
    slot0 = np.stack([np.roll(np.arange(R), k) for k in range(K)]).astype(np.int32)
    kw = dict(swap_every=N, burn=N, stride=N, n_samples=2, seed=6, stream0=1)
    betas = (1.0, 0.8, 0.5)
    host = tempered(g, ctx, mJ, Pi, Xr, q, betas=betas, gaps=True, slot0=slot0, **kw)
    up = lambda a: g.DeviceBuffer.from_array(ctx, a)  # noqa: E731
    out = devops.sample_tempered_dev(ctx, up(mJ), up(Pi), N, q, up(Xr), K, betas, dslot0=up(slot0), flags=g._lib.SAMPLE_GAPS,
                                     want=("E_s", "thr", "moves", "swap_thr", "slot_path"), **kw)
    dXs, dacc, dsw, dXo, dso, dE, dthr, dmv, dst, dsp = out
    T, E = 3 * N, 3
    dev = dict(Xs=dXs.download((N, 2, K), np.int8), E_s=dE.download((K, 2), order="C"), accepted=dacc.download((K, R), np.int32, order="C"),
               swaps=dsw.download((K, R - 1), np.int32, order="C"), Xr_out=dXo.download((N, R, K), np.int8),
               slot_out=dso.download((K, R), np.int32, order="C"), thr=dthr.download((K, R, T), order="C"),
               moves=dmv.download((K, R, T), np.int32, order="C"), swap_thr=dst.download((K, R - 1, E), order="C"),
               slot_path=dsp.download((K, R, E), np.int32, order="C"))
    same(dev, host, "devops.sample_tempered_dev / sample_tempered")
    only = devops.sample_tempered_dev(ctx, up(mJ), up(Pi), N, q, up(Xr), K, betas, dslot0=up(slot0), flags=g._lib.SAMPLE_GAPS, want=(), **kw)
    assert only[5:] == (None,) * 5 and np.array_equal(only[0].download((N, 2, K), np.int8), host["Xs"])


@pytest.mark.parametrize("option,value,refined", [("CHOLESKY", 2, 2), ("REFINE", 1, 1)])
def test_fused_chains_through_the_collect_time_branches(g, refdata, option, value, refined):
    """the stage runs AGAIN at collect time after the Cholesky fallback and after a Newton-Schulz step: what comes back is a whole run on
    the model finally used -- the counts agree with each other, the state space is kept"""
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    M, N = Zo.shape
    Zf = np.asfortranarray(Zo.T)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 7)
    c = g.Context(0)
    try:
        c.set_option(option, value)
        res, st = c.run_sample_tempered_ptr(Zf.ctypes.data, N, M, q, 0.8, -1.0, X.ctypes.data, 7, betas=(1.0, 0.6, 0.3), swap_every=N, burn=N,
                                            stride=N, n_samples=2, seed=2, trace=True)
        assert st["refined"] == refined
    finally:
        c.close()
    d = dict(zip(NAMES, res))
    assert d["accepted"].sum() == (d["moves"] >= 0).sum() and np.all(d["accepted"][[0, 4]] == 0) and np.all(d["moves"][[0, 4]] == tm.INT_MIN)
    assert np.all(d["moves"][[1, 2, 3, 5, 6]] != tm.INT_MIN) and np.all(np.isfinite(d["E_s"])) and np.all(d["thr"] >= 0.0)
    assert np.all(np.sort(d["slot_out"], axis=1) == np.arange(3)) and np.all(d["swaps"] <= tm.attempts(3, 3))
    assert np.array_equal(d["Xs"][:, 0, :] == q, X == q)


def test_a_pending_context_refuses_the_host_forms(g, refdata):
    from gaussdca.jl_amd.synth import synth_family

    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 7)
    Z = np.ascontiguousarray(synth_family(12, 200, 5, 11))
    kw = dict(betas=(1.0, 0.0), swap_every=1, burn=0, stride=1, n_samples=4)
    c = g.Context(0)
    try:
        c.run_ranked_async_ptr(Z.ctypes.data, 12, 200, 5, 0.5, 0.2, 0, 1)
        with pytest.raises(g.ArgumentError, match="still enqueued"):
            g.sample_tempered(mJ, Pi, X, q, ctx=c, **kw)
        with pytest.raises(g.ArgumentError, match="still enqueued"):
            c.run_sample_tempered_ptr(np.asfortranarray(Zo.T).ctypes.data, Zo.shape[1], Zo.shape[0], q, 0.8, -1.0, X.ctypes.data, 7, **kw)
        i1, j1, s1, st1 = c.run_ranked_collect()
        assert len(s1) > 0
        assert g.sample_tempered(mJ, Pi, X, q, gaps=True, ctx=c, **kw)[2].sum(axis=1).max() >= 4  # (the slot at beta = 0 accepts everything)
    finally:
        c.close()


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    M, N = Zo.shape
    K, S, R = 7, 4, 3
    X = mixed_sequences(np.random.default_rng(7), Zo, q, K)
    Xr = replicas(X, R)
    kw = dict(betas=(1.0, 0.8, 0.6), seed=1, swap_every=2, burn=2, stride=4, n_samples=S)
    good = tempered(g, ctx, mJ, Pi, Xr, q, **kw)
    Y = Xr.copy(order="F")
    Y[7, 1, 5] = q + 1
    with pytest.raises(g.ArgumentError):
        g.sample_tempered(mJ, Pi, Y, q, ctx=ctx, **kw)
    with pytest.raises(g.ArgumentError):
        g.gDCA_sample_tempered(os.path.join(refdata, "small.fasta.gz"), np.asfortranarray(Y[:, 1, :]), betas=(1.0, 0.5), ctx=ctx)
    same(tempered(g, ctx, mJ, Pi, Xr, q, **kw), good, "the context still works")

    # straight at the C-ABI: nothing is run, the outputs are untouched
    lib, p, EINVAL = ctx.lib, g._lib._p, g._lib.GDCA_EINVAL
    T = 2 + 4 * S
    b3 = np.array([1.0, 0.8, 0.6])
    Xs, E_s, acc = np.full((N, S, K), 77, dtype=np.int8, order="F"), np.full((K, S), np.nan), np.full((K, R), -7, dtype=np.int32)
    sw, Xo, so = np.full((K, R - 1), -7, dtype=np.int32), np.full((N, R, K), 77, dtype=np.int8, order="F"), np.full((K, R), -7, dtype=np.int32)
    thr, moves = np.full((K, R, T), np.nan), np.full((K, R, T), -7, dtype=np.int32)
    sthr, sp = np.full((K, R - 1, T // 2), np.nan), np.full((K, R, T // 2), -7, dtype=np.int32)
    outs = (p(Xs), p(E_s), p(acc), p(sw), p(Xo), p(so), p(thr), p(moves), p(sthr), p(sp))

    def op(mJ_=p(mJ), Pi_=p(Pi), N_=N, q_=q, X_=p(Xr), slot0=None, K_=K, R_=R, betas=b3, flags=0, every=2, burn=2, stride=4, S_=S, outs_=outs):
        return lib.gdca_sample_tempered(ctx.h, mJ_, Pi_, N_, q_, X_, slot0, K_, R_, None if betas is None else p(betas), None, flags, 1, 0, every,
                                        burn, stride, S_, *outs_)

    assert op() == 0
    same(dict(zip(NAMES, (Xs, E_s, acc, sw, Xo, so, thr, moves, sthr, sp))), good, "the C-ABI call")
    for a in (Xs, acc, sw, Xo, so, moves, sp):
        a[...] = 77 if a.dtype == np.int8 else -7
    for a in (E_s, thr, sthr):
        a[...] = np.nan
    assert op(K_=0) == EINVAL and op(K_=-1) == EINVAL and op(K_=(2 ** 31 - 256) // 3 + 1) == EINVAL  # (K R in the place of K)
    assert op(R_=0) == EINVAL and op(R_=-1) == EINVAL and op(R_=65, betas=np.ones(65)) == EINVAL
    assert op(q_=1) == EINVAL and op(q_=32) == EINVAL and op(q_=2) == EINVAL
    for bad in (-1e-300, float("nan"), float("inf")):
        for where in range(3):
            b = b3.copy()
            b[where] = bad
            assert op(betas=b) == EINVAL
    assert op(betas=None) == EINVAL
    assert op(every=0) == EINVAL and op(every=-2) == EINVAL and op(every=4) == EINVAL and op(every=3) == EINVAL  # (4 does not divide burn, 3 neither)
    assert op(every=4, burn=4, stride=6) == EINVAL
    assert op(burn=-2) == EINVAL and op(stride=0) == EINVAL and op(S_=0) == EINVAL and op(S_=-2) == EINVAL
    assert op(every=1, burn=2 ** 31 - 4, stride=1, S_=4) == EINVAL and op(burn=0, stride=2 ** 30, S_=2) == EINVAL  # n_steps = 2^31
    assert op(flags=2) == EINVAL and op(flags=3) == EINVAL and op(flags=-1) == EINVAL
    assert op(X_=None) == EINVAL and op(mJ_=None) == EINVAL and op(Pi_=None) == EINVAL
    for i in (0, 2, 3, 4, 5):  # Xs, accepted, swaps, Xr_out, slot_out
        assert op(outs_=outs[:i] + (None,) + outs[i + 1:]) == EINVAL, i
    prm, st = g._lib.Params(0.8, -1.0, 0, 1), g._lib.Stats()
    Zf = np.asfortranarray(Zo.T)

    def fused(Z_=p(Zf), q_=q, X_=p(X), K_=K, R_=R, betas=b3, flags=0, every=2, burn=2, stride=4, S_=S, outs_=outs, prm_=C.byref(prm)):
        return lib.gdca_run_sample_tempered(ctx.h, Z_, N, M, q_, prm_, X_, K_, R_, None if betas is None else p(betas), None, flags, 1, 0, every,
                                            burn, stride, S_, *outs_, C.byref(st))

    assert fused(K_=0) == EINVAL and fused(q_=32) == EINVAL and fused(R_=0) == EINVAL and fused(R_=65, betas=np.ones(65)) == EINVAL
    assert fused(betas=np.array([1.0, -1.0, 0.5])) == EINVAL and fused(betas=None) == EINVAL and fused(every=3) == EINVAL and fused(every=0) == EINVAL
    assert fused(burn=-2) == EINVAL and fused(stride=0) == EINVAL and fused(S_=0) == EINVAL and fused(flags=4) == EINVAL
    assert fused(Z_=None) == EINVAL and fused(prm_=None) == EINVAL
    for i in (0, 2, 3, 4, 5):
        assert fused(outs_=outs[:i] + (None,) + outs[i + 1:]) == EINVAL, i
    assert np.all(Xs == 77) and np.all(acc == -7) and np.all(moves == -7) and np.all(sw == -7) and np.all(Xo == 77) and np.all(so == -7)
    assert np.all(np.isnan(E_s)) and np.all(np.isnan(thr)) and np.all(np.isnan(sthr)) and np.all(sp == -7)
    # a slot0 that is no permutation: found on the device, GDCA_EINVAL -- a repeated slot, a slot out of range, in one chain of the batch
    for bad in ((0, 1, 1), (0, 1, 3), (-1, 0, 1)):
        s0 = np.repeat(np.arange(R, dtype=np.int32)[None], K, axis=0)
        s0[4] = bad
        assert op(slot0=p(s0)) == EINVAL and b"permutation" in lib.gdca_last_error(ctx.h)
    s0 = np.repeat(np.arange(R, dtype=np.int32)[None], K, axis=0)
    assert op(slot0=p(s0)) == 0
    # a bad symbol in Xr: found on the device
    assert op(X_=p(Y)) == EINVAL
    # a table that cannot live in LDS, asked into LDS
    c = g.Context(0)
    try:
        c.set_option("WALK_TABLE", "lds")
        big = np.ones((1000, R, 1), dtype=np.int8, order="F")
        rc = c.lib.gdca_sample_tempered(c.h, p(mJ), p(Pi), 1000, 21, p(big), None, 1, R, p(b3), None, 0, 1, 0, 2, 2, 4, S, *outs)
        assert rc == EINVAL and b"LDS" in c.lib.gdca_last_error(c.h)
    finally:
        c.close()
    same(tempered(g, ctx, mJ, Pi, Xr, q, **kw), good, "the context still works")


# ---- 11, 12. the Boltzmann-machine loop with a ladder ------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap_every", [1, 7])
def test_bm_loop_with_one_temperature_is_the_enqueued_loop(g, ctx, refdata, swap_every):
    """betas = (beta,): the loop driven from Python over the tempered operator form gives gdca_bm_learn_dev's W, X and trace bit for bit"""
    from test_gpu_bm import device_loop, loop_problem, same_bits

    N, q, W0, Pi_d, Pij_d, X0, mask, L = loop_problem(g, ctx)
    for flags, msk in ((0, None), (sm.GAPS, mask)):
        W, X, trace = device_loop(g, ctx, L, N, q, W0, Pi_d, Pij_d, X0, msk, flags, 3, 3)
        Wt, Xr, tt, slot, rates = g.bm_learn(W0, Pi_d, Pij_d, X0, 3, q, eta=L["eta"], lam=L["lam"], burn=L["burn"], stride=L["stride"],
                                             n_samples=L["n_samples"], seed=L["seed"], iter0=3, mask=msk, gaps=bool(flags), ctx=ctx,
                                             betas=(L["beta"],), swap_every=swap_every)
        assert same_bits(W, Wt) and np.array_equal(X, Xr[:, 0, :]) and same_bits(trace, tt)
        assert Xr.shape == (N, 1, L["K"]) and np.all(slot == 0) and rates.shape == (3, 0)
    # the file-level entry: one temperature is today's path, and a ladder returns the swap rates as a third result
    fasta = os.path.join(refdata, "small.fasta.gz")
    kw = dict(K=16, burn=53, stride=53, n_samples=2, seed=3, ctx=ctx)
    Wp, tp = g.gDCA_bm(fasta, 2, **kw)
    Wo, to, ro = g.gDCA_bm(fasta, 2, betas=(1.0,), **kw)
    assert same_bits(Wp, Wo) and same_bits(tp, to) and ro.shape == (2, 0)
    Wl, tl, rl = g.gDCA_bm(fasta, 2, betas=(1.0, 0.9, 0.8), **kw)
    assert Wl.shape == Wp.shape and tl.shape == (2, 4) and rl.shape == (2, 2) and np.all((rl >= 0) & (rl <= 1)) and np.all(np.isfinite(Wl))
    assert not same_bits(Wl, Wp)  # (other streams: another run)


# MEASURED with temper_model.bm_learn (pure numpy, thresholds -np.log(u)) on test_bm_cpu.py's learning problem at its settings, the
# ladder (1, 0.7), swap_every = 1 (burn = 16, stride = 1), seeds 0 .. 5: the exact pair-frequency deviation of the learned model was
# 0.00433, 0.00284, 0.00400, 0.00299, 0.00348, 0.00320 (acceptance at the target 0.18, swap rate 0.73).  The bar is twice the largest, as
# LEARN_BAR is; it is below half the start's 0.0371, so the test can tell learning from none.
LADDER_MEASURED = (0.00433, 0.00284, 0.00400, 0.00299, 0.00348, 0.00320)
LADDER_BAR = 2 * 0.004335


def test_learning_with_a_ladder_lowers_the_exact_deviation(g, ctx):
    import bm_model as bm
    from test_bm_cpu import LEARN as L, START_DEVIATION, learn_problem

    assert max(LADDER_MEASURED) * 2 <= LADDER_BAR + 1e-12 and LADDER_BAR < START_DEVIATION / 2
    N, q, P1, P2, W0, X0, start = learn_problem()
    W, Xr, trace, slot, rates = g.bm_learn(W0, P1, P2, X0, L["n_iter"], q, eta=L["eta"], burn=L["burn"], stride=L["stride"],
                                           n_samples=L["n_samples"], seed=L["seed"], gaps=True, ctx=ctx, betas=(1.0, 0.7), swap_every=1)
    dev = bm.pair_deviation(W, P2, q, N)
    first, last = float(trace[:10, 1].mean()), float(trace[-50:, 1].mean())
    print("exact pair deviation: start %.4f, learned %.5f, bar %.5f; trace[:, 1]: first 10 %.4f, last 50 %.4f; acceptance %.3f, swap rate %.3f" %
          (start, dev, LADDER_BAR, first, last, float(trace[:, 3].mean()), float(rates.mean())))
    assert dev < LADDER_BAR
    assert not start < LADDER_BAR  # the control: no learning does not pass
    assert last < first
    assert np.all(np.sort(slot, axis=1) == np.arange(2)) and Xr.shape == (N, 2, L["K"])
