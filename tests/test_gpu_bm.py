"""Boltzmann-machine refinement on the device (gdca_potts_from_gaussian*, gdca_bm_update*, gdca_bm_readout*, gdca_bm_learn*) against
tests/bm_model.py: the update and the read-out bit for bit, the loop against the chain of the operator forms and against the numpy
statement driven with the device's thresholds and start tables, the container (W, zeros) under the existing read-outs, and learning
itself: the exact marginals of the learned model on a toy against the target's; then the whole fit (gDCA_bm, devops.bm_fit) on a
golden family against the chain of the operator forms and against bm_model.fit.  No tolerance is invented here: the bounds are
bm_model's, mutation_model's, energy_model's and score_model's, the learning bar is measured on the numpy loop alone (test_bm_cpu.py)."""
import os

import numpy as np
import pytest

import bm_model as bm
import energy_model as em
import sample_model as sm
import score_model
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
# (q, N) -> the settings.  Beyond the toy, burn = N and stride = N // 2 + 1:
#   q = 6, N = 257: n = 1285, odd -- the narrow update instance over six row blocks; the sampler's loops over sites one element into a
#                   second pass; N % 4 = 1 for the packed symbols; 256 % s != 0 and 256 % q != 0, so the incremental (site, symbol) wrap
#                   is taken; a tally of 99 sequences over 17 ragged column blocks
#   q = 3, N = 300: n = 600, even -- the wide update instance over two row blocks; 256 % s = 0
# Every clause of the two tests runs at every shape; only the number of iterations is smaller beyond the toy (2, split 1 + 1).
LOOPS = {(5, 7): LOOP, (6, 257): dict(LOOP, n_iter=2, burn=257, stride=129), (3, 300): dict(LOOP, n_iter=2, burn=300, stride=151)}
_loop_problems = {}


def loop_problem(g, ctx, q=5, N=7):
    """(N, q, W0, Pi_d, Pij_d, X0 (N, K), mask, the settings), made once per shape and never written to"""
    if (q, N) not in _loop_problems:
        L = LOOPS[q, N]
        Zo, q, mJ, Pi = synth_model(q, N)
        assert Zo.shape[1] == N
        Z = np.ascontiguousarray(Zo.T.astype(np.int8))
        Pi_d, Pij_d = tm.frequencies(Z, np.ones(Z.shape[1]), float(Z.shape[1]), q)
        X0 = np.asfortranarray(Z[:, :L["K"]])
        out = (g.potts_from_gaussian(mJ, Pi, q, ctx=ctx), Pi_d, Pij_d, X0, (np.arange(N) % 3 != 1).astype(np.int8))
        for a in out:
            a.setflags(write=False)
        _loop_problems[q, N] = (N, q) + out + (L,)
    return _loop_problems[q, N]


def device_loop(g, c, L, N, q, W, Pi_d, Pij_d, X, mask, flags, iter0, n_iter, want_last=False):
    from gaussdca.jl_amd import devops

    n = N * (q - 1)
    dW, dPi, dPij, dX = up(g, c, W), up(g, c, Pi_d), up(g, c, Pij_d), up(g, c, X)
    dmask = None if mask is None else up(g, c, mask)
    dXs = g.DeviceBuffer(c, N * L["n_samples"] * L["K"]) if want_last else None
    dtr = devops.bm_learn_dev(c, dW, dPi, dPij, N, q, dX, L["K"], n_iter, L["burn"], L["stride"], L["n_samples"], L["eta"], L["lam"],
                              L["beta"], L["seed"], iter0, dmask, flags, dXs_last=dXs)
    out = (dW.download((n, n)), dX.download((N, L["K"]), dtype=np.int8), dtr.download((n_iter, 4), order="C"))
    if want_last:
        out += (dXs.download((N, L["n_samples"], L["K"]), dtype=np.int8),)
        dXs.free()
    for b in (dW, dPi, dPij, dX, dtr) + (() if dmask is None else (dmask,)):
        b.free()
    return out


def operator_iteration(g, c, L, N, q, W, Pi_d, Pij_d, X, mask, flags, t, model=False):
    """the steps 1 - 5 of iteration t with the operator forms -> (W, X, out (4,), Xs); model: bm_model.iteration driven with the
    device's thresholds and start tables must give the same W, X and out"""
    from gaussdca.jl_amd import devops

    K, S = L["K"], L["n_samples"]
    n, T = N * (q - 1), L["burn"] + L["n_samples"] * L["stride"]
    M = K * S
    dW, dZero, dX, dOnes = up(g, c, W), up(g, c, np.zeros(n)), up(g, c, X), up(g, c, np.ones(M))
    dmask = None if mask is None else up(g, c, mask)
    dXs, dacc, _, dthr, _, _ = devops.sample_dev(c, dW, dZero, N, q, dX, K, L["beta"], L["burn"], L["stride"], S, L["seed"], t * K, dmask, flags,
                                                 want=("thr",))
    Xs = dXs.download((N, S, K), dtype=np.int8)
    acc = dacc.download((K,), dtype=np.int32)
    Xn = np.asfortranarray(Xs[:, -1, :])
    dPi_m, dPij_m = devops.compute_weighted_frequencies_dev(c, dXs, N, M, q, dOnes, float(M))
    dPi_d, dPij_d = up(g, c, Pi_d), up(g, c, Pij_d)
    dout = devops.bm_readout_dev(c, dPi_d, dPij_d, dPi_m, dPij_m, N, q)
    out = dout.download((4,))
    assert out[3] == 0.0
    out[3] = np.float64(int(acc.astype(np.int64).sum())) / np.float64(K * T)
    devops.bm_update_dev(c, dW, dPij_d, dPij_m, N, q, L["eta"], L["lam"])
    Wn = dW.download((n, n))
    if model:
        dW0 = up(g, c, W)
        dV0 = devops.mutation_scan_dev(c, dW0, dZero, N, q, dX, K, g._lib.MUT_POTENTIAL)
        V0 = dV0.download((K, N, q), order="C")
        dW0.free(), dV0.free()
        thr = dthr.download((K, T), order="C")
        Wm, Xm, om, Xsm, Pi_m, Pij_m, bound = bm.iteration(W, Pi_d, Pij_d, X, q, t, flags, L["beta"], L["seed"], L["burn"], L["stride"], S,
                                                           L["eta"], L["lam"], mask, thr=thr, V0=V0, with_bound=True)
        assert np.array_equal(Xsm, np.transpose(Xs, (2, 1, 0))), t
        assert same_bits(dPij_m.download((n, n)), Pij_m) and same_bits(dPi_m.download((n,)), Pi_m), t
        assert same_bits(Wn, Wm), (t, int((bits(Wn) != bits(Wm)).sum()))
        assert np.array_equal(Xn, Xm) and out[0] == om[0] and out[1] == om[1] and out[3] == om[3], t
        assert abs(out[2] - om[2]) <= bound, (t, out[2], om[2], bound)
    for b in (dW, dZero, dX, dOnes, dXs, dacc, dthr, dPi_m, dPij_m, dPi_d, dPij_d, dout) + (() if dmask is None else (dmask,)):
        b.free()
    return Wn, Xn, out, Xs


STATE_SPACES = [(0, False), (sm.GAPS, False), (sm.GAPS, True)]
# the toy keeps its three ids; the two wide shapes follow, each in the three state spaces
LOOP_CASES = [(q, N, flags, masked) for (q, N) in LOOPS for flags, masked in STATE_SPACES]
LOOP_IDS = [("" if (q, N) == (5, 7) else "q%d-N%d-" % (q, N)) + ("gaps-masked" if masked else "gaps" if flags else "residues")
            for q, N, flags, masked in LOOP_CASES]


@pytest.mark.parametrize("q,N,flags,masked", LOOP_CASES, ids=LOOP_IDS)
def test_loop_is_the_operator_chain(g, ctx, q, N, flags, masked):
    N, q, W0, Pi_d, Pij_d, X0, mask, L = loop_problem(g, ctx, q, N)
    mask = mask if masked else None
    n_iter = L["n_iter"]
    W, X, trace, last = device_loop(g, ctx, L, N, q, W0, Pi_d, Pij_d, X0, mask, flags, 3, n_iter, want_last=True)
    assert_container(W, N, q)
    # the operator forms, iteration by iteration
    Wc, Xc, rows = W0, X0, []
    for it in range(n_iter):
        Wc, Xc, out, Xs = operator_iteration(g, ctx, L, N, q, Wc, Pi_d, Pij_d, Xc, mask, flags, 3 + it)
        rows.append(out)
    assert same_bits(W, Wc) and np.array_equal(X, Xc) and same_bits(trace, np.stack(rows)) and np.array_equal(last, Xs)
    assert not np.array_equal(X, X0) and np.all((trace[:, 3] > 0) & (trace[:, 3] <= 1)) and np.all(np.abs(trace[:, 2]) <= 1)
    print("trace:\n%s" % trace)
    # n_iter = a + b through W, X and iter0: 5 = 2 + 3 on the toy, 2 = 1 + 1 beyond it
    a = max(1, 2 * n_iter // 5)
    Wa, Xa, ta = device_loop(g, ctx, L, N, q, W0, Pi_d, Pij_d, X0, mask, flags, 3, a)
    Wb, Xb, tb = device_loop(g, ctx, L, N, q, Wa, Pi_d, Pij_d, Xa, mask, flags, 3 + a, n_iter - a)
    assert same_bits(W, Wb) and np.array_equal(X, Xb) and same_bits(trace, np.concatenate((ta, tb)))
    # another iter0: other streams, another run
    assert not same_bits(device_loop(g, ctx, L, N, q, W0, Pi_d, Pij_d, X0, mask, flags, 4, n_iter)[0], W)
    # however the chains are cut into launches and wherever the tables live
    for chunk in (1, 7, 0):
        for where in ("lds", "hbm"):
            c = g.Context(0)
            try:
                c.set_option("SAMPLE_CHUNK", chunk)
                c.set_option("WALK_TABLE", where)
                Wo, Xo, to = device_loop(g, c, L, N, q, W0, Pi_d, Pij_d, X0, mask, flags, 3, n_iter)
            finally:
                c.close()
            assert same_bits(W, Wo) and np.array_equal(X, Xo) and same_bits(trace, to), (chunk, where)
    # the host-pointer form
    Wh, Xh, th = g.bm_learn(W0, Pi_d, Pij_d, X0, n_iter, q, eta=L["eta"], lam=L["lam"], burn=L["burn"], stride=L["stride"],
                            n_samples=L["n_samples"], seed=L["seed"], iter0=3, mask=mask, gaps=bool(flags), ctx=ctx)
    assert same_bits(W, Wh) and np.array_equal(X, Xh) and same_bits(trace, th)


@pytest.mark.parametrize("q,N,flags,masked", LOOP_CASES, ids=LOOP_IDS)
def test_loop_is_the_numpy_statement(g, ctx, q, N, flags, masked):
    """the operator chain with the thresholds and the start tables asked from the device, fed to bm_model: W after EVERY iteration"""
    N, q, W0, Pi_d, Pij_d, X0, mask, L = loop_problem(g, ctx, q, N)
    mask = mask if masked else None
    W, X = W0, X0
    for it in range(L["n_iter"]):
        W, X, _, _ = operator_iteration(g, ctx, L, N, q, W, Pi_d, Pij_d, X, mask, flags, it, model=True)
        Wl, Xl, _ = device_loop(g, ctx, L, N, q, W0, Pi_d, Pij_d, X0, mask, flags, 0, it + 1)
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
    N, q, W0, Pi_d, Pij_d, X0, _, _ = loop_problem(g, ctx)
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


# ---- 7. the whole fit: gDCA_bm and devops.bm_fit on a golden family ----------------------------------------------------------------------------
# small.fasta.gz: N = 53, q = 21, n = 1060, M = 106 (98 without duplicates).  burn and stride are the defaults, 10 N and N: 636 proposals
# a chain and iteration.  Every setting that has a default is given another value, so that one put into another's place shows.
# beta = 0.1 because the chains must move for the test to see anything: at beta = 0.9 the Gaussian start of this family of 106
# sequences accepts ONE of the first iteration's 10 176 proposals and none afterwards (MEASURED on an MI355X, and the same in
# bm_model.fit), so three iterations tally the start sequences three times; at 0.1 bm_model.fit accepts 35 % to 77 %.
FASTA = "small.fasta.gz"
FIT_ITER = 3
FIT = dict(K=16, n_samples=2, eta=0.5, lam=0.01, beta=0.1, seed=5, pseudocount=0.5)
FIT_CASES = [dict(), dict(init="independent"), dict(target_pseudocount=0.1), dict(gaps=False), dict(remove_dups=True)]
FIT_IDS = ["gaussian", "independent", "target-0.1", "residues", "dedup"]
_fits, _chains = {}, {}


def family(g, refdata, remove_dups=False):
    """(Z (N, M) as gDCA_bm reads it, N, M, q)"""
    Z = g.read_fasta_alignment(os.path.join(refdata, FASTA), 0.9)
    if remove_dups:
        Z, _ = g.remove_duplicate_sequences(Z)
    return (Z,) + Z.shape + (int(Z.max()),)


def fit_of(g, ctx, refdata, n_iter=FIT_ITER, **kw):
    """gDCA_bm on the family with FIT's settings and kw on the module's context, called once per set of arguments"""
    key = (n_iter,) + tuple(sorted(kw.items()))
    if key not in _fits:
        _fits[key] = g.gDCA_bm(os.path.join(refdata, FASTA), n_iter, ctx=ctx, **dict(FIT, **kw))
    return _fits[key]


def operator_chain(g, ctx, refdata, init="gaussian", target_pseudocount=0.0, gaps=True, remove_dups=False):
    """What devops.bm_fit documents, step by step with the HOST operator forms the suite pins one by one: the weighted frequencies at
    theta = :auto, add_pseudocount twice from the same true tallies, compute_C, inv_cholesky, potts_from_gaussian (or potts_independent
    in numpy), then bm_learn from the first K sequences with burn = 10 N, stride = N and iter0 = 0 -> a dict, made once per case"""
    key = (init, target_pseudocount, gaps, remove_dups)
    if key not in _chains:
        Z, N, M, q = family(g, refdata, remove_dups)
        Pi_t, Pij_t, Meff, wts = g.compute_weighted_frequencies(Z, q, ":auto", ctx=ctx)
        Pi_d, Pij_d = g.add_pseudocount(Pi_t, Pij_t, target_pseudocount, q, ctx=ctx)
        Pi, Pij = g.add_pseudocount(Pi_t, Pij_t, FIT["pseudocount"], q, ctx=ctx)
        mJ = g.inv_cholesky(g.compute_C(Pi, Pij, ctx=ctx), ctx=ctx) if init == "gaussian" else None
        W0 = g.potts_from_gaussian(mJ, Pi, q, ctx=ctx) if init == "gaussian" else bm.potts_independent(Pi, N, q)
        W, X, trace = g.bm_learn(W0, Pi_d, Pij_d, Z[:, :FIT["K"]], FIT_ITER, q, eta=FIT["eta"], lam=FIT["lam"], beta=FIT["beta"], burn=10 * N,
                                 stride=N, n_samples=FIT["n_samples"], seed=FIT["seed"], iter0=0, gaps=gaps, ctx=ctx)
        _chains[key] = dict(Z=Z, N=N, M=M, q=q, Meff=Meff, wts=wts, Pi_d=Pi_d, Pij_d=Pij_d, Pi=Pi, mJ=mJ, W0=W0, W=W, X=X, trace=trace)
    return _chains[key]


@pytest.mark.parametrize("kw", FIT_CASES, ids=FIT_IDS)
def test_fit_is_the_chain_of_the_operators(g, ctx, refdata, kw):
    """W and trace of gDCA_bm, and of devops.bm_fit on the alignment itself, are the bits of the chain of the host operator forms.
    (Every step of it is: the host forms and the _dev forms bm_fit calls gave the same bits on an MI355X, the inverse in place over
    the covariance included, so the reference is built from the host forms throughout.)"""
    from gaussdca.jl_amd import devops

    W, trace = fit_of(g, ctx, refdata, **kw)
    ref = operator_chain(g, ctx, refdata, **kw)
    Z, N, q = ref["Z"], ref["N"], ref["q"]
    n = N * (q - 1)
    assert (N, q, ref["M"]) == (53, 21, 98 if kw.get("remove_dups") else 106)
    assert W.shape == (n, n) and trace.shape == (FIT_ITER, 4)
    assert same_bits(trace, ref["trace"]), (trace, ref["trace"])
    assert same_bits(W, ref["W"]), int((bits(W) != bits(ref["W"])).sum())
    assert_container(W, N, q)
    assert np.all(np.isfinite(trace)) and np.all((trace[:, 3] > 0) & (trace[:, 3] <= 1)) and not same_bits(W, ref["W0"])
    print("%s: trace\n%s" % (kw, trace))
    direct = devops.bm_fit(Z, q, FIT_ITER, ctx=ctx, **dict(FIT, **{k: v for k, v in kw.items() if k != "remove_dups"}))
    assert len(direct) == 2 and same_bits(direct[0], W) and same_bits(direct[1], trace)
    if kw:  # the case's argument matters: another W than the first case's
        base = fit_of(g, ctx, refdata)
        assert not same_bits(W, base[0]) and not same_bits(trace, base[1])
    if "target_pseudocount" in kw:  # ... and it moves the targets alone: the same start
        assert same_bits(ref["W0"], operator_chain(g, ctx, refdata)["W0"]) and not same_bits(ref["Pij_d"], operator_chain(g, ctx, refdata)["Pij_d"])


@pytest.mark.parametrize("init,tpc", [("gaussian", 0.0), ("independent", 0.1)], ids=["gaussian", "independent-target-0.1"])
def test_fit_is_the_numpy_statement(g, ctx, refdata, init, tpc):
    """bm_model.fit with the oracle's weights, driven as operator_iteration(model=True) drives bm_model.iteration: the thresholds and
    the start tables (and, for the Gaussian start, the inverse) asked from the device.  The targets are the model's bit for bit and
    within test_operator_parity's bars of the oracle's; W after every iteration, the chains' last states and trace[:, (0, 1, 3)] are
    the model's bits, trace[:, 2] is within bm_model.readout's bound."""
    from oracle import gdca_oracle as o

    kw = dict(init=init, target_pseudocount=tpc)
    ref = operator_chain(g, ctx, refdata, **kw)
    Z, N, q = ref["Z"], ref["N"], ref["q"]
    K, S = FIT["K"], FIT["n_samples"]
    zeros = np.zeros(N * (q - 1))
    Zo = np.ascontiguousarray(Z.T)
    wts, Meff, _, _ = o.compute_weights(Zo, "auto")

    def thresholds(t):
        return g.sample(ref["W0"], zeros, Z[:, :K], q, beta=FIT["beta"], burn=10 * N, stride=N, n_samples=S, seed=FIT["seed"], stream0=t * K,
                        gaps=True, trace=True, ctx=ctx)[3]

    f = bm.fit(Z, q, FIT_ITER, wts, Meff, K, eta=FIT["eta"], lam=FIT["lam"], pseudocount=FIT["pseudocount"], target_pseudocount=tpc, init=init,
               n_samples=S, beta=FIT["beta"], seed=FIT["seed"], inverse=lambda C: ref["mJ"], thresholds=thresholds,
               tables=lambda W, X: g.mutation_scan(W, zeros, X, q, what="potential", ctx=ctx))
    # the targets: against the oracle's at the bars of test_operator_parity (frequencies 1e-12 of the largest, add_pseudocount the
    # same bits from the same input), and the device's own are the model's
    Pi_o, Pij_o = o.compute_frequencies(Zo, q, wts, Meff)
    Pi_do, Pij_do = o.add_pseudocount(Pi_o, Pij_o, tpc, q)
    assert np.max(np.abs(f["Pi_d"] - Pi_do)) <= 1e-12 * np.max(np.abs(Pi_do)) and np.max(np.abs(f["Pij_d"] - Pij_do)) <= 1e-12 * np.max(np.abs(Pij_do))
    again = bm.add_pseudocount(Pi_o, Pij_o, tpc, q)
    assert np.array_equal(again[0], Pi_do) and np.array_equal(again[1], Pij_do)
    assert same_bits(ref["Pi_d"], f["Pi_d"]) and same_bits(ref["Pij_d"], f["Pij_d"]) and same_bits(ref["Pi"], f["Pi"])
    assert same_bits(ref["W0"], f["W0"]), int((bits(ref["W0"]) != bits(f["W0"])).sum())
    # the loop
    for it in range(FIT_ITER):
        Wd = fit_of(g, ctx, refdata, n_iter=it + 1, **kw)[0]
        assert same_bits(Wd, f["Ws"][it]), (it, int((bits(Wd) != bits(f["Ws"][it])).sum()))
    W, trace = fit_of(g, ctx, refdata, **kw)
    assert same_bits(W, ref["W"]) and np.array_equal(ref["X"], f["X"])
    assert same_bits(trace[:, (0, 1, 3)], f["trace"][:, (0, 1, 3)]), (trace, f["trace"])
    err = np.abs(trace[:, 2] - f["trace"][:, 2])
    print("%s: trace\n%s\n|trace[:, 2] - exact| %s, bound %s" % (kw, trace, err, f["bounds"]))
    assert np.all(np.isfinite(f["bounds"])) and np.all(err <= f["bounds"])


def test_what_the_fit_may_not_depend_on(g, ctx, refdata):
    fasta = os.path.join(refdata, FASTA)
    W, trace = fit_of(g, ctx, refdata)
    M = family(g, refdata)[2]
    # K beyond the family is the whole family (and not the K = 16 of the other tests)
    every = g.gDCA_bm(fasta, 2, ctx=ctx, **dict(FIT, K=M))
    beyond = g.gDCA_bm(fasta, 2, ctx=ctx, **dict(FIT, K=10 ** 6))
    assert same_bits(every[0], beyond[0]) and same_bits(every[1], beyond[1]) and not same_bits(every[1], trace[:2])
    # a shorter fit is the beginning of a longer one
    two = fit_of(g, ctx, refdata, n_iter=2)
    assert same_bits(two[1], trace[:2]) and not same_bits(two[0], W)
    # a second call repeats the bits
    again = g.gDCA_bm(fasta, FIT_ITER, ctx=ctx, **FIT)
    assert same_bits(again[0], W) and same_bits(again[1], trace)
    # the tables in HBM and the chains cut into launches of 97 proposals (636 = 6 x 97 + 54)
    c = g.Context(0)
    try:
        c.set_option("WALK_TABLE", "hbm")
        c.set_option("SAMPLE_CHUNK", 97)
        other = g.gDCA_bm(fasta, FIT_ITER, ctx=c, **FIT)
    finally:
        c.close()
    assert same_bits(other[0], W) and same_bits(other[1], trace)


def test_scores_of_the_fit(g, ctx, refdata):
    """scores=True: the third entry is the ranking of APC(FN(W)) of the host forms entry for entry; FN(W) is within score_model.fn_bound of
    the extended-precision model; and the fields on W's diagonal blocks do not reach the contact score"""
    sep = 4
    W, trace, R = g.gDCA_bm(os.path.join(refdata, FASTA), FIT_ITER, scores=True, min_separation=sep, ctx=ctx, **FIT)
    base = fit_of(g, ctx, refdata)
    assert same_bits(W, base[0]) and same_bits(trace, base[1])
    _, N, _, q = family(g, refdata)
    s = q - 1
    FN = g.compute_FN(W, q, ctx=ctx)
    want = g.compute_ranking(g.correct_APC(FN, ctx=ctx), sep)
    assert len(R) == len(want) == (N - sep) * (N - sep + 1) // 2
    assert np.array_equal(R.i, want.i) and np.array_equal(R.j, want.j) and same_bits(R.score, want.score)
    assert np.all(np.isfinite(R.score)) and np.all(np.diff(R.score) <= 0)
    ref, scale = score_model.fn_model(W, q)
    bound = score_model.fn_bound(s, ref, scale)
    err = np.abs(FN - ref)
    off = ~np.eye(N, dtype=bool)
    print("FN(W): worst err / bound %.3g" % float(np.max(err[off] / bound[off])))
    assert np.all(err <= bound) and np.all(ref[off] > 10 * bound[off])
    junk = W.copy()
    inside = bm.multipliers(N, q) != 1.0
    junk[inside] = 1e3 * np.random.default_rng(1).normal(size=int(inside.sum()))
    assert same_bits(g.compute_FN(junk, q, ctx=ctx), FN)
    # and the other separation is another list of the same scores
    R5 = g.gDCA_bm(os.path.join(refdata, FASTA), FIT_ITER, scores=True, ctx=ctx, **FIT)[2]
    assert len(R5) == (N - 5) * (N - 4) // 2 and R5 == g.compute_ranking(g.correct_APC(FN, ctx=ctx), 5)


def test_a_fit_leaves_nothing_behind(g, refdata):
    fasta = os.path.join(refdata, FASTA)
    used, fresh = g.Context(0), g.Context(0)
    try:
        out = g.gDCA_bm(fasta, 2, scores=True, ctx=used, **FIT)
        assert np.all(np.isfinite(out[0])) and np.all(np.isfinite(out[1]))
        R_used, R_fresh = g.gDCA(fasta, ctx=used), g.gDCA(fasta, ctx=fresh)
    finally:
        used.close()
        fresh.close()
    assert len(R_used) == len(R_fresh) > 0
    assert np.array_equal(R_used.i, R_fresh.i) and np.array_equal(R_used.j, R_fresh.j) and same_bits(R_used.score, R_fresh.score)
