"""log det C from the pivots of the inverse, and the log-likelihoods built on it (gdca_last_logdet, gdca_spd_inverse_logdet*,
gdca_run_loglik*, inv_cholesky(return_logdet=True), sequence_loglik, gDCA_loglik) against tests/logdet_model.py.

The bar is the model's (stated from the backward error of the elimination, tests/logdet_model.py); every comparison of values prints
the fraction of it the device uses.  Everything about bits -- the inverse beside the value, run to run, the collect-time branches,
L against -(E + c) -- is array_equal / ==."""
import os

import numpy as np
import pytest

import energy_model as em
import logdet_model as lm
from gdca_testutil import ctx, g, mixed_sequences  # noqa: F401 (g, ctx: fixtures)

pytestmark = pytest.mark.gpu

LOG_2PI = float(np.log(2.0 * np.pi))


def constant(n, logdet):
    """c = 0.5 * (n * log(2 pi) + logdet) in numpy float64: one multiplication, one addition, one multiplication"""
    return np.float64(0.5) * (np.float64(n) * np.float64(LOG_2PI) + np.float64(logdet))


def dev_inverse(c, C, with_logdet=True, room=0, dirt=None):
    """The _dev forms on C (n x n): (inverse, logdet or None).  room / dirt: the matrix lies at the start of an allocation `room`
    doubles larger, filled with `dirt` behind it."""
    import torch

    n = C.shape[0]
    buf = np.empty(n * n + room)
    buf[:n * n] = np.asfortranarray(C).ravel(order="F")
    if room:
        buf[n * n:] = dirt
    d = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    if with_logdet:
        v = c.spd_inverse_logdet_dev(d.data_ptr(), n)
    else:
        import ctypes as C_

        info = C_.c_int32(0)
        c.check(c.lib.gdca_spd_inverse_dev(c.h, C_.c_void_p(d.data_ptr()), n, C_.byref(info)), info.value)
        v = None
    out = d.cpu().numpy()
    if room:
        assert np.array_equal(out[n * n:], buf[n * n:])  # (nothing behind the matrix is touched)
    return out[:n * n].reshape((n, n), order="F"), v


def held(name, ref, value, factor=1.0):
    frac = ref.fraction(value)
    print("%-40s logdet %+.12e  uses %.3g of the bar (%.3g)" % (name, value, frac, ref.bar))
    assert frac <= factor, (name, frac)
    return frac


# ---- 1. operator level against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", lm.OPERATOR_SIZES)
def test_operator_sizes(g, ctx, n):
    C, ref = lm.operator_case(n)
    X0, _ = dev_inverse(ctx, C, with_logdet=False)
    X1, v = dev_inverse(ctx, C)
    assert np.array_equal(X0, X1)  # the plain entry and the new entry: one inverse
    held("spd n=%d" % n, ref, v)
    assert ctx.last_logdet(return_source=True) == (v, 0)
    # the host forms: the same bits, inv_cholesky unchanged in type and value when the keyword is absent
    mJ = g.inv_cholesky(C, ctx=ctx)
    mJ2, v2 = g.inv_cholesky(C, ctx=ctx, return_logdet=True)
    assert isinstance(mJ, np.ndarray) and mJ.dtype == np.float64 and np.array_equal(mJ, mJ2) and np.array_equal(mJ, X1) and v2 == v
    assert np.allclose(mJ @ C, np.eye(n), atol=1e-9)


@pytest.mark.parametrize("option,value,n", [("GROUP", 1, 640), ("GROUP", 2, 640), ("GROUP", 3, 640), ("GROUP", 4, 640), ("RAGGED", 0, 129),
                                            ("RAGGED", 0, 640), ("RAGGED", 0, 17)])
def test_operator_groupings(g, option, value, n):
    """Pivots of multi-block groups run on the scratch matrix, the first of a group straight from A; RAGGED=0 sweeps the matrix padded
    to 128.  Every grouping is inside the bar, and its inverse is the plain entry's under the same option."""
    C, ref = lm.operator_case(n)
    c = g.Context(0)
    try:
        c.set_option(option, value)
        X0, _ = dev_inverse(c, C, with_logdet=False)
        X1, v = dev_inverse(c, C)
        assert np.array_equal(X0, X1)
        held("spd n=%d %s=%d" % (n, option, value), ref, v)
    finally:
        c.close()


# ---- 2. exact cases ------------------------------------------------------------------------------------------------------------------------
def test_powers_of_two_on_the_diagonal(ctx):
    C, e = lm.pow2_diagonal()
    _, v = dev_inverse(ctx, C)
    bound = (np.log2(300) + 2) * lm.U * float(np.abs(e).sum()) * np.log(2.0)
    err = abs(np.longdouble(v) - np.log(np.longdouble(2.0)) * int(e.sum()))
    print("diag(2^e): logdet %+.15e, |error| %.3g, bound %.3g" % (v, float(err), bound))
    assert err <= bound


def test_scaling_by_four_scales_every_pivot_exactly(ctx):
    C, _ = lm.operator_case(257)
    _, v1 = dev_inverse(ctx, C)
    _, v4 = dev_inverse(ctx, 4.0 * C)
    # the pivots of 4 C are exactly four times those of C: the two sums differ by n log 4 up to the roundings of the logarithms and
    # of the two trees
    bound = 2 * (np.log2(257) + 2) * lm.U * (abs(v1) + abs(v4) + 257 * np.log(4.0))
    print("logdet(4 C) - logdet(C) - n log 4 = %.3g (bound %.3g)" % (v4 - v1 - 257 * np.log(4.0), bound))
    assert abs((v4 - v1) - 257 * np.log(4.0)) <= bound


# ---- 3. padding ------------------------------------------------------------------------------------------------------------------------------
def test_padding_rows_are_not_summed(g):
    C, ref = lm.operator_case(129)
    c = g.Context(0)
    try:
        X0, v0 = dev_inverse(c, C)
        # the context's workspace dirty beyond n (a larger matrix before), the caller's allocation larger and dirty behind the matrix
        dev_inverse(c, 1e3 * lm.operator_case(257)[0])
        X1, v1 = dev_inverse(c, C, room=5000, dirt=-7.25e300)
        assert v1 == v0 and np.array_equal(X0, X1)
        held("spd n=129, dirty", ref, v1)
    finally:
        c.close()


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------------------
def test_same_bits_on_three_calls(ctx):
    C, _ = lm.operator_case(640)
    vals = [dev_inverse(ctx, C)[1] for _ in range(3)]
    assert vals[0] == vals[1] == vals[2], vals


def test_merged_members_keep_their_bits(g):
    import torch

    ns = [20, 77, 128, 129, 200, 256, 333, 500]
    cases = [lm.reference(("spd-batch", n), lambda n=n: lm.random_spd(n, seed=70 + n)) for n in ns]
    ctxs = [g.Context(0) for _ in ns]
    try:
        ctxs[0].set_option("MERGE_GROUP", 1)
        runs = []
        for _ in range(2):
            bufs = [torch.from_numpy(np.asfortranarray(C).ravel(order="F").copy()).cuda() for C, _ in cases]
            torch.cuda.synchronize()
            info = g.spd_inverse_batch_dev(ctxs, [b.data_ptr() for b in bufs], ns)
            assert info == [0] * len(ns)
            runs.append([c.last_logdet(return_source=True) for c in ctxs])
        assert runs[0] == runs[1]
        assert len({v for v, _ in runs[0]}) == len(ns)  # all distinct
        single = g.Context(0)
        try:
            for (C, ref), n, (v, src) in zip(cases, ns, runs[0]):
                _, vs = dev_inverse(single, C)  # the library's own grouping
                held("merged member n=%d" % n, ref, v)
                print("   against its single run: %.3g of the bar" % (abs(v - vs) / ref.bar))
                assert src == 0 and abs(v - vs) <= 2 * ref.bar
        finally:
            single.close()
    finally:
        for c in ctxs:
            c.close()


# ---- 5. branches ---------------------------------------------------------------------------------------------------------------------------
def test_cholesky_fallback_is_the_source(g):
    C, ref = lm.operator_case(257)
    c = g.Context(0)
    try:
        c.set_option("CHOLESKY", 2)
        _, v = dev_inverse(c, C)
        assert c.last_logdet(return_source=True) == (v, 1)
        held("spd n=257 CHOLESKY=2", ref, v)
    finally:
        c.close()


def test_collect_time_branches_of_a_fused_run(g, refdata):
    fasta = os.path.join(refdata, "small.fasta.gz")
    plain = g.Context(0)
    try:
        L0, ld0 = g.gDCA_loglik(fasta, ctx=plain)
        assert g.gdca.last_stats["refined"] == 0 and g.gdca.last_stats["sweep_retries"] == 0
        assert plain.last_logdet(return_source=True) == (ld0, 0)
    finally:
        plain.close()
    for option, value in (("SWEEP_DEBUG", 32), ("REFINE", 1), ("CHOLESKY", 2)):
        c = g.Context(0)
        try:
            c.set_option(option, value)
            L, ld = g.gDCA_loglik(fasta, ctx=c)
            st = g.gdca.last_stats
            v, src = c.last_logdet(return_source=True)
            assert v == ld and np.all(np.isfinite(L))
            if option == "SWEEP_DEBUG":  # the forced second attempt: the undisturbed run's bits, all of them
                assert st["sweep_retries"] > 0 and src == 0 and ld == ld0 and np.array_equal(L, L0)
            elif option == "REFINE":     # the value stays that of the sweep's pivots; the energies are the refined inverse's
                assert st["refined"] == 1 and src == 0 and ld == ld0
                assert np.allclose(L, L0, rtol=1e-9, atol=0)
            else:                        # the fallback's diagonal
                assert st["refined"] == 2 and src == 1
                print("CHOLESKY=2: logdet %+.15e against the sweep's %+.15e" % (ld, ld0))
                assert abs(ld - ld0) <= 1e-9 * abs(ld0) and np.allclose(L, L0, rtol=1e-9, atol=0)
        finally:
            c.close()


def test_not_positive_definite_and_the_getters_refusals(g):
    c = g.Context(0)
    try:
        with pytest.raises(g.ArgumentError):  # no inverse yet
            c.last_logdet()
        C, _ = lm.operator_case(129)
        w, V = np.linalg.eigh(C)
        w[40] = -1.0
        Cbad = (V * w) @ V.T
        Cbad = (Cbad + Cbad.T) * 0.5
        with pytest.raises(g.PosDefException):
            c.spd_inverse_logdet(Cbad)
        assert np.isnan(c.last_logdet())  # GDCA_OK, NaN
        c.spd_inverse_logdet(C)
        assert np.isfinite(c.last_logdet(0))
        with pytest.raises(g.ArgumentError):  # k = 1 after a single run
            c.last_logdet(1)
        with pytest.raises(g.ArgumentError):
            c.last_logdet(-1)
        # entry points without an inverse leave the record alone
        v = c.last_logdet()
        g.correct_APC(np.ones((4, 4)), ctx=c)
        assert c.last_logdet() == v
    finally:
        c.close()


# ---- 6. fused ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,q", lm.FAMILIES)
@pytest.mark.parametrize("pc", lm.PSEUDOCOUNTS)
def test_fused_loglik_is_the_energies_and_the_constant(g, ctx, N, M, q, pc):
    Zo = lm.family(N, M, q)
    Zf = np.asfortranarray(Zo.T)
    n = N * (q - 1)
    X = mixed_sequences(np.random.default_rng(N + q), Zo, q, 37)
    L, ld, st = ctx.run_loglik(Zf, q, pc, -1.0, X)
    assert ctx.last_logdet(return_source=True) == (ld, 0) and st["ms_score"] > 0.0 and st["ms_fn"] == 0.0
    E, st_e = ctx.run_energies_ptr(Zf.ctypes.data, N, M, q, pc, -1.0, X.ctypes.data, X.shape[1])
    assert ctx.last_logdet() == ld
    assert np.array_equal(L, -(E + constant(n, ld)))
    for f in ("theta", "Meff", "thresh", "info", "refined", "n", "n_pad"):
        assert st[f] == st_e[f], f
    # a plain gdca_run with the same parameters: the same inverse, the same bits
    ctx.run(Zf, q, pc, -1.0, 0)
    assert ctx.last_logdet() == ld
    # X = None scores Z; the value does not depend on X or K
    Lz, ldz, _ = ctx.run_loglik(Zf, q, pc, -1.0)
    Ez, _ = ctx.run_energies_ptr(Zf.ctypes.data, N, M, q, pc, -1.0)
    assert ldz == ld and Lz.shape == (M,) and np.array_equal(Lz, -(Ez + constant(n, ld)))
    # against the model, on the oracle's covariance
    _, ref = lm.family_case(N, M, q, pc)
    held("family N=%d M=%d q=%d pc=%g" % (N, M, q, pc), ref, ld)
    # an illegal byte of X
    Xbad = X.copy(order="F")
    Xbad[N // 2, 5] = q + 1
    with pytest.raises(g.ArgumentError):
        ctx.run_loglik(Zf, q, pc, -1.0, Xbad)


def test_against_an_independent_density(ctx):
    from scipy.stats import multivariate_normal

    N, M, q, pc = 30, 1000, 21, 0.5
    Zo = lm.family(N, M, q)
    Zf = np.asfortranarray(Zo.T)
    X = mixed_sequences(np.random.default_rng(99), Zo, q, 32)
    L, ld, _ = ctx.run_loglik(Zf, q, pc, -1.0, X)
    C, ref = lm.family_case(N, M, q, pc)
    want = multivariate_normal(mean=ref.Pi, cov=C).logpdf(em.one_hot(X, q))
    E_ref = -(want + constant(N * (q - 1), ref.logdet))
    # the fused energies' bar (rtol 1e-6, 1e-9 of the largest: tests/test_gpu_energy.py) plus half the logdet bar
    tol = 1e-6 * np.abs(E_ref) + 1e-9 * np.abs(E_ref).max() + 0.5 * ref.bar
    print("against scipy's logpdf: max |L - want| = %.3g, smallest tolerance %.3g" % (float(np.abs(L - want).max()), float(tol.min())))
    assert np.all(np.abs(L - want) <= tol)


def test_run_multi_members(ctx):
    N, M, q = 53, 500, 5
    Zf = np.asfortranarray(lm.family(N, M, q).T)
    singles = []
    for pc in (0.5, 0.8):
        ctx.run(Zf, q, pc, -1.0, 0)
        singles.append(ctx.last_logdet())
    ctx.run_multi(Zf, q, [(0.5, 0), (0.8, 0), (0.5, 1)], -1.0)
    assert [ctx.last_logdet(k) for k in range(3)] == [singles[0], singles[1], singles[0]]
    with pytest.raises(Exception):
        ctx.last_logdet(3)


# ---- 7. the Python surface -------------------------------------------------------------------------------------------------------------------
def test_gdca_loglik_on_a_golden_family(g, ctx, refdata):
    L, ld = g.gDCA_loglik(os.path.join(refdata, "small.fasta.gz"), ctx=ctx)
    assert L.shape == (g.gdca.last_stats["M"],) and np.all(np.isfinite(L)) and ld == ctx.last_logdet()
    # sequence_loglik: host arithmetic on sequence_energies
    Zo = lm.family(7, 200, 2)
    mJ, Pi = em.model_from_Z(Zo, 2, 0.5)
    X = np.asfortranarray(Zo[:9].T)
    Ls = g.sequence_loglik(mJ, Pi, X, 1.25, q=2, ctx=ctx)
    assert np.array_equal(Ls, -(g.sequence_energies(mJ, Pi, X, 2, ctx=ctx) + constant(7, 1.25)))


def test_held_out_likelihood_of_two_pseudocounts(ctx):
    N, M, q = 30, 1000, 21
    Zf = np.asfortranarray(lm.family(N, M, q).T)
    train, test = np.asfortranarray(Zf[:, :800]), np.asfortranarray(Zf[:, 800:])
    means = {pc: float(ctx.run_loglik(train, q, pc, -1.0, test)[0].mean()) for pc in (0.05, 0.8)}
    print("held-out mean log-likelihood of the last 200 sequences: pseudocount 0.05: %.6f, 0.8: %.6f -> %g generalises better" %
          (means[0.05], means[0.8], max(means, key=means.get)))
    assert np.isfinite(means[0.05]) and np.isfinite(means[0.8]) and means[0.05] != means[0.8]
