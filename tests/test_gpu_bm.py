"""Boltzmann-machine refinement on the device (gdca_potts_from_gaussian*, gdca_bm_update*, gdca_bm_readout*, gdca_bm_learn*) against
tests/bm_model.py: the update and the read-out bit for bit, the loop against the chain of the operator forms and against the numpy
statement driven with the device's thresholds and start tables, the container (W, zeros) under the existing read-outs, and learning
itself: the exact marginals of the learned model on a toy against the target's.  No tolerance is invented here: the bounds are
bm_model's, mutation_model's and energy_model's, the learning bar is measured on the numpy loop alone (test_bm_cpu.py)."""
import numpy as np
import pytest

import bm_model as bm
import energy_model as em
import sample_model as sm
import tally_model as tm
from energy_model import U
from gdca_testutil import ctx, g, golden_model, mixed_sequences, mutation_reference, synth_model  # noqa: F401 (g, ctx: fixtures)
from test_bm_cpu import LEARN, LEARN_BAR, learn_problem

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def up(g, c, a):
    return g.DeviceBuffer.from_array(c, np.asfortranarray(a))


def tallies(rng, N, q, M, like=None):
    """(Pi, Pij) of a random alignment of M sequences through tally_model -- symmetric to the bit, zero off the diagonal inside a
    diagonal block, Pij[r, r] = Pi[r]; like: an alignment (N, M') whose first columns are kept, so that the two tallies correlate"""
    Z = rng.integers(1, q + 1, size=(N, M)).astype(np.int8)
    Z[:, ::3] = np.minimum(Z[:1, ::3] + (rng.random((N, Z[:, ::3].shape[1])) < 0.3), q)  # columns that resemble their first site
    if like is not None:
        keep = min(M, like.shape[1]) * 3 // 4
        Z[:, :keep] = like[:, :keep]
    Pi, Pij = tm.frequencies(Z, np.ones(M), float(M), q)
    return Z, Pi, Pij


def container(rng, N, q):
    """a random model in the container's form"""
    n = N * (q - 1)
    A = rng.normal(size=(n, n))
    W = np.where(bm.multipliers(N, q) == 1.0, A + A.T, 0.0)
    W[np.arange(n), np.arange(n)] = rng.normal(size=n)
    return W


def assert_container(W, N, q):
    m = bm.multipliers(N, q)
    assert same_bits(W, W.T.copy())
    assert np.all(W[m == 0.0] == 0.0) and not np.signbit(W[m == 0.0]).any()


def case(g, ctx, refdata, which):
    """(tag, N, q, W0): the models of the update and the read-out tests"""
    if which < 3:
        Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", (0.8, 0.2)[which]) if which < 2 else synth_model(5, 7)
        return ("small-0.8", "small-0.2", "N7-q5")[which], Zo.shape[1], q, g.potts_from_gaussian(mJ, Pi, q, ctx=ctx)
    N, q = ((301, 2), (5, 31), (7, 4))[which - 3]  # n = 301: odd and two row blocks of the narrow instance; n = 150; n = 21: odd
    return "N%d-q%d" % (N, q), N, q, container(np.random.default_rng(which), N, q)


CASES = ["small-0.8", "small-0.2", "N7-q5", "N301-q2", "N5-q31", "N7-q4"]


# ---- 1. the update, bit for bit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(6), ids=CASES)
def test_update_bit_for_bit(g, ctx, refdata, which):
    from gaussdca.jl_amd import devops

    tag, N, q, W0 = case(g, ctx, refdata, which)
    n = N * (q - 1)
    rng = np.random.default_rng(50 + which)
    Zd, _, Pd = tallies(rng, N, q, 96)
    for lam in (0.0, 0.01):
        W = W0.copy()
        dW, dPd = up(g, ctx, W), up(g, ctx, Pd)
        for step in range(3):
            _, _, Pm = tallies(rng, N, q, 64 + step, like=Zd)
            dPm = up(g, ctx, Pm)
            devops.bm_update_dev(ctx, dW, dPd, dPm, N, q, 0.5 + step, lam)
            W = bm.update(W, Pd, Pm, N, q, 0.5 + step, lam)
            got = dW.download((n, n))
            assert same_bits(got, W), (tag, lam, step, int((bits(got) != bits(W)).sum()))
            dPm.free()
        assert_container(got, N, q)
        assert not same_bits(got, W0)
        dW.free(), dPd.free()
    # the host-pointer form: the same bits
    Wh = np.asfortranarray(W0.copy())
    p = g._lib._p
    ctx.check(ctx.lib.gdca_bm_update(ctx.h, p(Wh), None, p(Pd), None, p(Pm), N, q, 1.0, 0.25))
    assert same_bits(Wh, bm.update(W0, Pd, Pm, N, q, 1.0, 0.25))


# ---- 2. the read-out ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(6), ids=CASES)
def test_readout(g, ctx, refdata, which):
    """out[0], out[1] bit for bit; out[2] within bm_model.readout's bound.  MEASURED on an MI355X: |out[2] - exact| at most 6.7e-16 (three
    ulp of a correlation of 0.67-0.87), the bound 5e-14 (T = 189) to 1.7e-10 (T = 45 150; 1e-10 at T = 551 200), the ratio at most 2.5e-3."""
    from gaussdca.jl_amd import devops

    tag, N, q, _ = case(g, ctx, refdata, which)
    rng = np.random.default_rng(70 + which)
    Zd, Pi_d, Pij_d = tallies(rng, N, q, 200)
    _, Pi_m, Pij_m = tallies(rng, N, q, 150, like=Zd)
    want, bound = bm.readout(Pi_d, Pij_d, Pi_m, Pij_m, N, q)
    bufs = [up(g, ctx, a) for a in (Pi_d, Pij_d, Pi_m, Pij_m)]
    dout = up(g, ctx, np.full(4, np.nan))
    devops.bm_readout_dev(ctx, *bufs, N, q, dout)
    out = dout.download((4,))
    again = devops.bm_readout_dev(ctx, *bufs, N, q).download((4,))
    assert same_bits(out, again)
    err = abs(out[2] - want[2])
    print("%s: out %s, |out[2] - exact| = %.3g, bound %.3g, ratio %.3g, T = %d" %
          (tag, out.tolist(), err, bound, err / bound, (q - 1) ** 2 * N * (N - 1) // 2))
    assert out[0] == want[0] and out[1] == want[1]
    assert np.isfinite(bound) and err <= bound and abs(want[2]) > 0.05
    assert out[3] == 0.0 and not np.signbit(out[3])
    host = np.full(4, np.nan)
    p = g._lib._p
    ctx.check(ctx.lib.gdca_bm_readout(ctx.h, p(Pi_d), p(Pij_d), p(Pi_m), p(Pij_m), N, q, p(host)))
    assert same_bits(host, out)
    for b in bufs:
        b.free()


# ---- 3. the loop against the chain of the operator forms, and against the numpy statement ---------------------------------------------------------
LOOP = dict(K=33, n_iter=5, burn=14, stride=7, n_samples=3, eta=0.75, lam=0.01, beta=1.0, seed=11)


def loop_problem(g, ctx):
    """N = 7, q = 5: (N, q, W0, Pi_d, Pij_d, X0 (N, K), mask)"""
    Zo, q, mJ, Pi = synth_model(5, 7)
    N = Zo.shape[1]
    Z = np.ascontiguousarray(Zo.T.astype(np.int8))
    Pi_d, Pij_d = tm.frequencies(Z, np.ones(Z.shape[1]), float(Z.shape[1]), q)
    X0 = np.asfortranarray(Z[:, :LOOP["K"]])
    return N, q, g.potts_from_gaussian(mJ, Pi, q, ctx=ctx), Pi_d, Pij_d, X0, (np.arange(N) % 3 != 1).astype(np.int8)


def device_loop(g, c, N, q, W, Pi_d, Pij_d, X, mask, flags, iter0, n_iter, want_last=False):
    from gaussdca.jl_amd import devops

    L = LOOP
    n = N * (q - 1)
    dW, dPi, dPij, dX = up(g, c, W), up(g, c, Pi_d), up(g, c, Pij_d), up(g, c, X)
    dmask = None if mask is None else up(g, c, mask)
    dXs = g.DeviceBuffer(c, N * L["n_samples"] * L["K"]) if want_last else None
    dtr = devops.bm_learn_dev(c, dW, dPi, dPij, N, q, dX, L["K"], n_iter, L["burn"], L["stride"], L["n_samples"], L["eta"], L["lam"],
                              L["beta"], L["seed"], iter0, dmask, flags, dXs_last=dXs)
    out = (dW.download((n, n)), dX.download((N, L["K"]), dtype=np.int8), dtr.download((n_iter, 4), order="C"))
    if want_last:
        out += (dXs.download((N, L["n_samples"], L["K"]), dtype=np.int8),)
    return out


def operator_iteration(g, c, N, q, W, Pi_d, Pij_d, X, mask, flags, t, model=False):
    """the steps 1 - 5 of iteration t with the operator forms -> (W, X, out (4,), Xs); model: bm_model.iteration driven with the
    device's thresholds and start tables must give the same W, X and out"""
    from gaussdca.jl_amd import devops

    L = LOOP
    K, S = L["K"], L["n_samples"]
    n, T = N * (q - 1), L["burn"] + L["n_samples"] * L["stride"]
    dW, dZero, dX = up(g, c, W), up(g, c, np.zeros(n)), up(g, c, X)
    dmask = None if mask is None else up(g, c, mask)
    dXs, dacc, _, dthr, _, _ = devops.sample_dev(c, dW, dZero, N, q, dX, K, L["beta"], L["burn"], L["stride"], S, L["seed"], t * K, dmask, flags,
                                                 want=("thr",))
    Xs = dXs.download((N, S, K), dtype=np.int8)
    acc = dacc.download((K,), dtype=np.int32)
    Xn = np.asfortranarray(Xs[:, -1, :])
    M = K * S
    dPi_m, dPij_m = devops.compute_weighted_frequencies_dev(c, dXs, N, M, q, up(g, c, np.ones(M)), float(M))
    dPi_d, dPij_d = up(g, c, Pi_d), up(g, c, Pij_d)
    out = devops.bm_readout_dev(c, dPi_d, dPij_d, dPi_m, dPij_m, N, q).download((4,))
    assert out[3] == 0.0
    out[3] = np.float64(int(acc.astype(np.int64).sum())) / np.float64(K * T)
    devops.bm_update_dev(c, dW, dPij_d, dPij_m, N, q, L["eta"], L["lam"])
    Wn = dW.download((n, n))
    if model:
        V0 = devops.mutation_scan_dev(c, up(g, c, W), dZero, N, q, dX, K, g._lib.MUT_POTENTIAL).download((K, N, q), order="C")
        thr = dthr.download((K, T), order="C")
        Wm, Xm, om, Xsm, Pi_m, Pij_m = bm.iteration(W, Pi_d, Pij_d, X, q, t, flags, L["beta"], L["seed"], L["burn"], L["stride"], S, L["eta"],
                                                    L["lam"], mask, thr=thr, V0=V0)
        assert np.array_equal(Xsm, np.transpose(Xs, (2, 1, 0))), t
        assert same_bits(dPij_m.download((n, n)), Pij_m) and same_bits(dPi_m.download((n,)), Pi_m), t
        assert same_bits(Wn, Wm), (t, int((bits(Wn) != bits(Wm)).sum()))
        assert np.array_equal(Xn, Xm) and out[0] == om[0] and out[1] == om[1] and out[3] == om[3], t
        _, bound = bm.readout(Pi_d, Pij_d, Pi_m, Pij_m, N, q)
        assert abs(out[2] - om[2]) <= bound, (t, out[2], om[2], bound)
    return Wn, Xn, out, Xs


STATE_SPACES = [(0, False), (sm.GAPS, False), (sm.GAPS, True)]


@pytest.mark.parametrize("flags,masked", STATE_SPACES, ids=["residues", "gaps", "gaps-masked"])
def test_loop_is_the_operator_chain(g, ctx, flags, masked):
    N, q, W0, Pi_d, Pij_d, X0, mask = loop_problem(g, ctx)
    mask = mask if masked else None
    n_iter = LOOP["n_iter"]
    W, X, trace, last = device_loop(g, ctx, N, q, W0, Pi_d, Pij_d, X0, mask, flags, 3, n_iter, want_last=True)
    assert_container(W, N, q)
    # the operator forms, iteration by iteration
    Wc, Xc, rows = W0, X0, []
    for it in range(n_iter):
        Wc, Xc, out, Xs = operator_iteration(g, ctx, N, q, Wc, Pi_d, Pij_d, Xc, mask, flags, 3 + it)
        rows.append(out)
    assert same_bits(W, Wc) and np.array_equal(X, Xc) and same_bits(trace, np.stack(rows)) and np.array_equal(last, Xs)
    assert not np.array_equal(X, X0) and np.all((trace[:, 3] > 0) & (trace[:, 3] <= 1)) and np.all(np.abs(trace[:, 2]) <= 1)
    print("trace:\n%s" % trace)
    # 5 = 2 + 3 through W, X and iter0
    Wa, Xa, ta = device_loop(g, ctx, N, q, W0, Pi_d, Pij_d, X0, mask, flags, 3, 2)
    Wb, Xb, tb = device_loop(g, ctx, N, q, Wa, Pi_d, Pij_d, Xa, mask, flags, 5, 3)
    assert same_bits(W, Wb) and np.array_equal(X, Xb) and same_bits(trace, np.concatenate((ta, tb)))
    # another iter0: other streams, another run
    assert not same_bits(device_loop(g, ctx, N, q, W0, Pi_d, Pij_d, X0, mask, flags, 4, n_iter)[0], W)
    # however the chains are cut into launches and wherever the tables live
    for chunk in (1, 7, 0):
        for where in ("lds", "hbm"):
            c = g.Context(0)
            try:
                c.set_option("SAMPLE_CHUNK", chunk)
                c.set_option("WALK_TABLE", where)
                Wo, Xo, to = device_loop(g, c, N, q, W0, Pi_d, Pij_d, X0, mask, flags, 3, n_iter)
            finally:
                c.close()
            assert same_bits(W, Wo) and np.array_equal(X, Xo) and same_bits(trace, to), (chunk, where)
    # the host-pointer form
    Wh, Xh, th = g.bm_learn(W0, Pi_d, Pij_d, X0, n_iter, q, eta=LOOP["eta"], lam=LOOP["lam"], burn=LOOP["burn"], stride=LOOP["stride"],
                            n_samples=LOOP["n_samples"], seed=LOOP["seed"], iter0=3, mask=mask, gaps=bool(flags), ctx=ctx)
    assert same_bits(W, Wh) and np.array_equal(X, Xh) and same_bits(trace, th)


@pytest.mark.parametrize("flags,masked", STATE_SPACES, ids=["residues", "gaps", "gaps-masked"])
def test_loop_is_the_numpy_statement(g, ctx, flags, masked):
    """the operator chain with the thresholds and the start tables asked from the device, fed to bm_model: W after EVERY iteration"""
    N, q, W0, Pi_d, Pij_d, X0, mask = loop_problem(g, ctx)
    mask = mask if masked else None
    W, X = W0, X0
    for it in range(LOOP["n_iter"]):
        W, X, _, _ = operator_iteration(g, ctx, N, q, W, Pi_d, Pij_d, X, mask, flags, it, model=True)
        Wl, Xl, _ = device_loop(g, ctx, N, q, W0, Pi_d, Pij_d, X0, mask, flags, 0, it + 1)
        assert same_bits(W, Wl) and np.array_equal(X, Xl), it


# ---- 4. the container -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(3), ids=CASES[:3])
def test_the_container_under_the_existing_readouts(g, ctx, refdata, which):
    """W = potts_from_gaussian(mJ, Pi): the couplings are mJ's bits, the diagonal is the header's rule bit for bit, and (W, zeros) gives
    the energy differences and the site potentials of (mJ, Pi).  Exactly, V under (W, 0) IS V under (mJ, Pi) and the energies differ by
    the constant c0 / 2, but for the rounding of W[r, r] = fl(mJ[r, r] - 2 g[r]): half of it enters a potential and an energy per
    non-gap site, e[r] = u |W[r, r]| / 2 + 2 (n + 1) u Gabs[r], Gabs[r] = sum_c |mJ[r, c]| |Pi[c]| (the rounding of the subtraction, and
    g's n products and n additions in any order as mutation_model.bound_V counts them).  So
        |V_W - V_G| <= bound_V(W) + bound_V(G) + e[r],
        |(E_W[k] - E_W[1]) - (E_G[k] - E_G[1])| <= the four order bounds + the e of both sequences' residues + 2 u (|dE_W| + |dE_G|).
    MEASURED on an MI355X, largest error / bound: energy differences 7.5e-6 (small, pseudocount 0.8; |dE| up to 494), 7.1e-6 (0.2; up to
    2380), 6.1e-4 (N = 7, q = 5; up to 8.3); site potentials 0 in all three: the two tables were the same bits."""
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", (0.8, 0.2)[which]) if which < 2 else synth_model(5, 7)
    N, s = Zo.shape[1], q - 1
    n = N * s
    A = bm.library_symmetric(mJ)
    W = g.potts_from_gaussian(mJ, Pi, q, ctx=ctx)
    m = bm.multipliers(N, q)
    assert_container(W, N, q)
    assert np.array_equal(bits(W)[m == 1.0], bits(A)[m == 1.0])
    assert same_bits(W, bm.potts_from_gaussian(mJ, Pi, q)), int((bits(W) != bits(bm.potts_from_gaussian(mJ, Pi, q))).sum())
    with pytest.raises(g.ArgumentError, match="alias"):
        d = up(g, ctx, mJ)
        ctx.potts_from_gaussian_dev(d.ptr, up(g, ctx, Pi).ptr, N, q, d.ptr)
    zeros = np.zeros(n)
    X = mixed_sequences(np.random.default_rng(9), Zo, q, 7)
    e = U * np.abs(np.diagonal(W)) / 2 + 2.0 * (n + 1) * U * (np.abs(A) @ np.abs(Pi))
    e_seq = em.one_hot(X, q) @ e  # (K,): the residues of each sequence
    EW, EG = g.sequence_energies(W, zeros, X, q, ctx=ctx), g.sequence_energies(mJ, Pi, X, q, ctx=ctx)
    bW = em.order_bound(N, q, em.energies_gather(W, zeros, X, q)[1])
    bG = em.order_bound(N, q, em.energies_gather(mJ, Pi, X, q)[1])
    dW_, dG_ = EW - EW[1], EG - EG[1]
    bound = bW + bW[1] + bG + bG[1] + e_seq + e_seq[1] + 2 * U * (np.abs(dW_) + np.abs(dG_))
    err = np.abs(dW_ - dG_)
    print("%s: energy differences: largest error / bound %.3g (|dE| up to %.3g)" % (CASES[which], float((err[bound > 0] / bound[bound > 0]).max()),
                                                                                   float(np.abs(dG_).max())))
    assert np.all(err <= bound) and np.abs(dG_).max() > 1.0
    VW = g.mutation_scan(W, zeros, X, q, what="potential", ctx=ctx)
    VG = g.mutation_scan(mJ, Pi, X, q, what="potential", ctx=ctx)
    bVW, bVG = mutation_reference(W, zeros, X, q)[1], mutation_reference(mJ, Pi, X, q)[1]
    bV = bVW + bVG
    bV[:, :, :s] += e.reshape(N, s)[None]
    errV = np.abs(VW - VG)
    assert np.all(errV[:, :, s] == 0.0)
    print("%s: site potentials: largest error / bound %.3g" % (CASES[which], float((errV[:, :, :s] / bV[:, :, :s]).max())))
    assert np.all(errV <= bV)


# ---- 5. learning works ------------------------------------------------------------------------------------------------------------------------
def test_learning_lowers_the_exact_deviation(g, ctx):
    """The toy of test_bm_cpu.py on the device: from the independent-site model, the exact pair-frequency deviation of the learned
    model from the target is below LEARN_BAR (measured there on the numpy loop alone; below half the start's), the start itself is
    not, and the sampled deviation of the trace falls.  MEASURED on an MI355X: start 0.0371, learned 0.0062, bar 0.0171; trace[:, 1]
    0.0331 over the first 10 iterations, 0.0073 over the last 50; mean acceptance 0.18."""
    N, q, P1, P2, W0, X0, start = learn_problem()
    L = LEARN
    W, X, trace = g.bm_learn(W0, P1, P2, X0, L["n_iter"], q, eta=L["eta"], burn=L["burn"], stride=L["stride"], n_samples=L["n_samples"],
                             seed=L["seed"], gaps=True, ctx=ctx)
    dev = bm.pair_deviation(W, P2, q, N)
    first, last = float(trace[:10, 1].mean()), float(trace[-50:, 1].mean())
    print("exact pair deviation: start %.4f, learned %.4f, bar %.4f; trace[:, 1]: first 10 %.4f, last 50 %.4f; acceptance %.3f" %
          (start, dev, LEARN_BAR, first, last, float(trace[:, 3].mean())))
    assert_container(W, N, q)
    assert dev < LEARN_BAR
    assert not start < LEARN_BAR  # the control: no learning does not pass
    assert last < first


# ---- 6. arguments -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_model_and_the_chains_untouched(g, ctx):
    N, q, W0, Pi_d, Pij_d, X0, _ = loop_problem(g, ctx)
    lib, p, EINVAL = ctx.lib, g._lib._p, g._lib.GDCA_EINVAL
    W, X = np.asfortranarray(W0.copy()), X0.copy(order="F")
    trace = np.full((5, 4), np.nan)
    K = X.shape[1]

    def op(W_=p(W), Pi_=p(Pi_d), Pij_=p(Pij_d), N_=N, q_=q, X_=p(X), K_=K, flags=1, beta=1.0, iter0=0, n_iter=5, burn=2, stride=3, S=2, eta=1.0,
           lam=0.0, trace_=p(trace)):
        return lib.gdca_bm_learn(ctx.h, W_, Pi_, Pij_, N_, q_, X_, K_, None, flags, beta, 1, iter0, n_iter, burn, stride, S, eta, lam, trace_, None)

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert op(eta=bad) == EINVAL, bad
    for bad in (-1e-300, float("nan"), float("inf")):
        assert op(lam=bad) == EINVAL, bad
    assert op(n_iter=0) == EINVAL and op(n_iter=-3) == EINVAL
    assert op(K_=0) == EINVAL and op(K_=-1) == EINVAL and op(q_=1) == EINVAL and op(q_=32) == EINVAL
    assert op(beta=-1.0) == EINVAL and op(beta=float("nan")) == EINVAL
    assert op(burn=-1) == EINVAL and op(stride=0) == EINVAL and op(S=0) == EINVAL and op(burn=2 ** 31 - 4, stride=1, S=4) == EINVAL
    assert op(flags=2) == EINVAL and op(flags=-1) == EINVAL
    assert op(iter0=2 ** 64 - 1) == EINVAL and op(iter0=(2 ** 64 - 1) // K - 3) == EINVAL  # t K past 2^64
    assert op(W_=None) == EINVAL and op(Pi_=None) == EINVAL and op(Pij_=None) == EINVAL and op(X_=None) == EINVAL and op(trace_=None) == EINVAL
    assert same_bits(W, W0) and np.array_equal(X, X0) and np.all(np.isnan(trace))
    # the _dev form: the same checks, the arrays in HBM as they were
    dW, dX, dP1, dP2, dtr = up(g, ctx, W0), up(g, ctx, X0), up(g, ctx, Pi_d), up(g, ctx, Pij_d), up(g, ctx, trace)

    def dev(iter0=0, n_iter=5, eta=1.0, lam=0.0, K_=K, S=2, W_=dW.ptr):
        return lib.gdca_bm_learn_dev(ctx.h, W_, dP1.ptr, dP2.ptr, N, q, dX.ptr, K_, None, 1, 1.0, 1, iter0, n_iter, 2, 3, S, eta, lam, dtr.ptr, None)

    assert dev(eta=0.0) == EINVAL and dev(lam=-1.0) == EINVAL and dev(n_iter=0) == EINVAL and dev(iter0=2 ** 64 - 5) == EINVAL
    assert dev(K_=0) == EINVAL and dev(S=0) == EINVAL and dev(W_=None) == EINVAL
    n = N * (q - 1)
    assert same_bits(dW.download((n, n)), W0) and np.array_equal(dX.download((N, K), dtype=np.int8), X0) and np.all(np.isnan(dtr.download((5, 4))))
    # q = 2 without the flag: one target symbol
    W2, P2 = np.zeros((3, 3), order="F"), np.full((3, 3), 0.25, order="F")
    X2 = np.ones((3, 4), dtype=np.int8, order="F")
    assert lib.gdca_bm_learn(ctx.h, p(W2), p(np.full(3, 0.5)), p(P2), 3, 2, p(X2), 4, None, 0, 1.0, 1, 0, 1, 2, 3, 1, 1.0, 0.0, p(trace), None) == EINVAL
    # the operators' own refusals
    assert lib.gdca_bm_update(ctx.h, p(W), None, p(Pij_d), None, p(Pij_d), N, q, 0.0, 0.0) == EINVAL
    assert lib.gdca_bm_update(ctx.h, p(W), None, p(Pij_d), None, p(Pij_d), N, q, 1.0, -1.0) == EINVAL
    assert lib.gdca_bm_update(ctx.h, p(W), None, None, None, p(Pij_d), N, q, 1.0, 0.0) == EINVAL
    assert lib.gdca_bm_readout(ctx.h, p(Pi_d), p(Pij_d), p(Pi_d), p(Pij_d), N, q, None) == EINVAL
    assert same_bits(W, W0)
    # a byte of X outside 1..q: reported as the chains report it
    Y = X0.copy(order="F")
    Y[3, 5] = q + 1
    with pytest.raises(g.ArgumentError):
        g.sample(W0, np.zeros(N * (q - 1)), Y, q, gaps=True, ctx=ctx)
    with pytest.raises(g.ArgumentError):
        g.bm_learn(W0, Pi_d, Pij_d, Y, 2, q, burn=2, stride=3, ctx=ctx)
    # the context still works
    Wn, Xn, tr = g.bm_learn(W0, Pi_d, Pij_d, X0, 1, q, burn=2, stride=3, ctx=ctx)
    assert np.all(np.isfinite(tr)) and not same_bits(Wn, W0)
