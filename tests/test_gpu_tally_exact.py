"""The weighted frequency tallies (k_tally.hip) against an exact integer model, bit for bit, at every boundary of the kernels.

The tally is 64-bit fixed point and order-independent, so Pi_true and Pij_true are promised exactly: the integer sum of
rint(W_k 2^shift), converted to f64 once, scaled, divided by Meff once (tests/tally_model.py restates that contract without
importing the library or the oracle).  Every case below asks `np.array_equal` against that model on Pi and on the whole Pij, and
the derived bound `tally_model.bound` against the true sums (`tally_model.exact_frequencies`); no tolerance here was tuned to what the
device gives.  Each case runs with TALLY_SKIP 0 and 1 and, for q <= 21 (where gdca_tally_tj grants it), TALLY_TJ 16 and 32.  The
families are tests/tally_cases.py's grid; tests/test_tally_model_cpu.py shows the model itself inside the bound on each of them.

Which alphabets run the skip form: by gdca_tally_skip's rule as written all of 2 .. 31 do at TALLY_TJ 16 (the [q][q][16] layout fits
and costs no occupancy), and q <= 21 at TALLY_TJ 32.  The tests do not depend on that: both settings must match the model.

Then the paths that consume the tally without exposing it -- the fused covariance epilogue (mode 1), the stored Pij_true of
gdca_run_multi, a phase batch's batched grids -- each tied bit for bit to the operator path that the model pins."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import tally_cases
import tally_model as tm

pytestmark = pytest.mark.gpu

FROB, DI = 0, 1


@pytest.fixture(scope="module")
def g():
    import gaussdca.jl_amd as g

    assert os.path.exists(g._lib.LIB_PATH), "libgdca.so missing: the GPU tests never fall back to the CPU"
    assert g.load().gdca_device_count() > 0, "no HIP device"
    return g


@pytest.fixture(scope="module")
def ctx(g):
    c = g.Context(0)
    yield c
    c.close()


def _frequencies(ctx, Zf, q, W, Meff):
    N, M = Zf.shape
    n = N * (q - 1)
    Pi = np.full(n, np.nan)
    Pij = np.full((n, n), np.nan, order="F")
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    ctx.check(ctx.lib.gdca_frequencies(ctx.h, ptr(Zf), N, M, q, ptr(W), float(Meff), ptr(Pi), ptr(Pij)))
    return Pi, Pij


def _settings(q):
    return [(skip, tj) for skip in (0, 1) for tj in ((0, 32) if q <= 21 else (0,))]


def _restore(ctx):
    ctx.set_options(TALLY_SKIP=1, TALLY_TJ=0)


def _assert_exact(label, Pi, Pij, Pi_m, Pij_m, Pifix, H, shift, Meff, q):
    s = q - 1
    msg = tm.first_mismatch(Pi, Pi_m, Pifix.reshape(-1), shift, Meff, s)
    assert msg is None, "%s Pi: %s" % (label, msg)
    msg = tm.first_mismatch(Pij, Pij_m, H, shift, Meff, s)
    assert msg is None, "%s Pij: %s" % (label, msg)
    assert np.array_equal(Pij, Pij.T), label


def _assert_bound(label, Pi, Pij, exact, shift, Meff):
    Pi_x, Pij_x, cnt_i, cnt_ij = exact
    for what, got, ref, cnt in (("Pi", Pi, Pi_x, cnt_i), ("Pij", Pij, Pij_x, cnt_ij)):
        err = np.abs(got.astype(np.longdouble) - ref)
        lim = tm.bound(cnt, shift, Meff, got)
        over = err > lim
        assert not over.any(), "%s %s: %d entries outside the derived bound, first at %s: error %.3g, bound %.3g" % (
            label, what, int(over.sum()), tuple(int(x) for x in np.argwhere(over)[0]), float(err[over][0]), float(lim[over][0]))


def _check_case(ctx, name, Z, q, W, Meff, frequencies):
    """frequencies(): the device's (Pi, Pij) under the current options."""
    N, M = Z.shape
    shift = tm.fix_shift(M)
    Pifix, H = tm.tallies(Z, tm.wfix(W, shift), q)
    Pi_m, Pij_m = tm.to_frequency(Pifix.reshape(-1), shift, Meff), tm.to_frequency(H, shift, Meff)
    exact = tm.exact_frequencies(Z, W, Meff, q)
    try:
        for skip, tj in _settings(q):
            ctx.set_options(TALLY_SKIP=skip, TALLY_TJ=tj)
            Pi, Pij = frequencies()
            label = "%s (N=%d M=%d q=%d TALLY_SKIP=%d TALLY_TJ=%d)" % (name, N, M, q, skip, tj or 16)
            _assert_exact(label, Pi, Pij, Pi_m, Pij_m, Pifix, H, shift, Meff, q)
            _assert_bound(label, Pi, Pij, exact, shift, Meff)
    finally:
        _restore(ctx)


@pytest.mark.parametrize("name", list(tally_cases.GRID))
def test_frequencies_equal_the_integer_model(g, ctx, name):
    """gdca_frequencies (operator path: caller-given weights through k_fix_weights, mode 0)."""
    Z, q, W, Meff = tally_cases.GRID[name]()
    _check_case(ctx, name, Z, q, W, Meff, lambda: _frequencies(ctx, Z, q, W, Meff))


@pytest.mark.parametrize("name", tally_cases.PIPELINE)
def test_pipeline_weights_equal_the_integer_model(g, ctx, name):
    """compute_weights on the device, then compute_weighted_frequencies(Z, q, theta): the weights the pipeline really makes (1/n_k),
    the model fed with the device's W and Meff."""
    from gaussdca.jl_amd import dcautils

    Z, q, _, _ = tally_cases.GRID[name]()
    W, Meff = dcautils.compute_weights(Z, q, 0.2, ctx=ctx)
    assert np.all((W > 0) & (W <= 1)) and np.array_equal(W, 1.0 / np.rint(1.0 / W))

    def freq():
        Pi, Pij, Meff2, W2 = dcautils.compute_weighted_frequencies(Z, q, 0.2, ctx=ctx)
        assert Meff2 == Meff and np.array_equal(W2, W)
        return Pi, Pij

    _check_case(ctx, name + " (device weights)", Z, q, W, Meff, freq)


@pytest.fixture(scope="module")
def consumers():
    return [(name,) + tally_cases.GRID[name]()[:2] for name in tally_cases.CONSUMERS]


def _both_skips(ctx, fn):
    out = []
    try:
        for skip in (0, 1):
            ctx.set_options(TALLY_SKIP=skip)
            out.append(fn())
    finally:
        _restore(ctx)
    return out


def test_fused_epilogue_equals_the_operator_chain(g, ctx, consumers):
    """gdca_run builds the covariance in the tally's epilogue (mode 1); the operator chain takes Pij_true from mode 0 -- which the
    model pins above -- through add_pseudocount and compute_C, which are bit-exact against the oracle.  Same scores bit for bit."""
    from gaussdca.jl_amd import devops

    for name, Z, q in consumers:
        for score, sname, pc in ((FROB, "frob", 0.8), (DI, "DI", 0.2)):
            runs = _both_skips(ctx, lambda: (ctx.run(Z, q, pc, -1.0, score), devops.scores_stepwise(Z, q, pc, "auto", sname, ctx=ctx)))
            for skip, ((S, st), (S2, info)) in enumerate(runs):
                assert np.isfinite(S).all(), (name, sname, skip)
                assert np.array_equal(S, S2), (name, sname, skip, float(np.abs(S - S2).max()))
                assert info["Meff"] == st["Meff"] and info["thresh"] == st["thresh"]
            assert np.array_equal(runs[0][0][0], runs[1][0][0]), (name, sname)


def test_multi_members_equal_single_runs(g, ctx, consumers):
    """gdca_run_multi: every pseudocount's covariance from the stored Pij_true (k_cov_from_pij)."""
    settings = [(0.8, FROB, 1), (0.2, DI, 1), (0.5, FROB, 0)]
    for name, Z, q in consumers:
        for skip, (multi, singles) in enumerate(_both_skips(ctx, lambda: (
                ctx.run_multi(Z, q, settings, -1.0), [ctx.run(Z, q, pc, -1.0, sc, bool(apc)) for pc, sc, apc in settings]))):
            for k, ((S, st), (S1, st1)) in enumerate(zip(multi, singles)):
                assert np.array_equal(S, S1), (name, skip, k, float(np.abs(S - S1).max()))
                assert st["Meff"] == st1["Meff"] and st["info"] == st1["info"] == 0


def test_phase_batch_members_equal_single_runs(g, ctx, consumers):
    """One phase batch of the eight families (one batched grid per kernel kind; members with their own N, M, q, kept-list strides
    and sigma): every member's scores are those of its single run.  MERGE_GROUP=1 as in test_phase_batched_runs_equal_single_runs:
    a merged sweep then pivots in the groups a launch of its own uses, so the comparison is bit for bit."""
    import torch

    Zd = [torch.from_numpy(np.ascontiguousarray(Z.T)).cuda() for _, Z, _ in consumers]   # (M, N) row-major == N x M column-major
    Ns, Ms, qs = [Z.shape[0] for _, Z, _ in consumers], [Z.shape[1] for _, Z, _ in consumers], [q for _, _, q in consumers]
    assert len(consumers) <= 16 and len(set(qs)) > 1
    cs = [g.Context(0) for _ in consumers]
    cs[0].set_options(MERGE_GROUP=1, PHASED_GRIDS=1)
    try:
        for skip in (0, 1):
            ctx.set_options(TALLY_SKIP=skip)
            want = [ctx.run(Z, q, 0.8, -1.0, FROB)[0] for _, Z, q in consumers]
            for c in cs:
                c.set_options(TALLY_SKIP=skip)
            outs = [torch.zeros((n, n), dtype=torch.float64, device="cuda") for n in Ns]
            torch.cuda.synchronize()
            g.run_dev_phased(cs, [z.data_ptr() for z in Zd], Ns, Ms, qs, 0.8, -1.0, FROB, [x.data_ptr() for x in outs])
            sts = [c.collect() for c in cs]
            for k, (name, _, _) in enumerate(consumers):
                assert sts[k]["info"] == 0
                assert np.array_equal(outs[k].cpu().numpy(), want[k]), (name, skip)
    finally:
        _restore(ctx)
        for c in cs:
            c.close()


@pytest.mark.slow
def test_config_C_family_on_a_sample_of_column_pairs(g, ctx):
    """N = 500, M = 50 000 (config C's family): all of Pi, and the s x s blocks of 64 column pairs drawn with a fixed seed plus the
    pairs at the corners and across the first column-block edges, each compared in full.  The sample caps the model's cost (no
    n x n model matrix); it is not a tolerance."""
    from gaussdca.jl_amd import synth

    N, M, q = 500, 50000, 21
    s = q - 1
    Z = np.asfortranarray(synth.synth_family(N, M, q, synth.SEEDS["C"]).T)
    W = 1.0 / np.random.default_rng(0xC).integers(1, 200, size=M)
    Meff = math.fsum(W)
    shift = tm.fix_shift(M)
    Wf = tm.wfix(W, shift)
    rng = np.random.default_rng(0xC500)
    pairs = [(0, 0), (0, N - 1), (N - 1, N - 1), (15, 16), (31, 32)] + [tuple(sorted(int(x) for x in rng.integers(0, N, size=2)))
                                                                        for _ in range(64)]
    blocks = {p: tm.pair_tally(Z, Wf, q, *p) for p in pairs}
    Pifix = tm.single_site(Z, Wf, q)
    Pi_m = tm.to_frequency(Pifix.reshape(-1), shift, Meff)
    try:
        for skip in (0, 1):
            ctx.set_options(TALLY_SKIP=skip)
            Pi, Pij = _frequencies(ctx, Z, q, W, Meff)
            msg = tm.first_mismatch(Pi, Pi_m, Pifix.reshape(-1), shift, Meff, s)
            assert msg is None, "TALLY_SKIP=%d Pi: %s" % (skip, msg)
            for (i, j), H in blocks.items():
                want = tm.to_frequency(H, shift, Meff)
                got = Pij[i * s:(i + 1) * s, j * s:(j + 1) * s]
                bad = np.argwhere(got != want)
                assert len(bad) == 0, "TALLY_SKIP=%d pair (%d, %d): %d cells differ, first (i=%d, a=%d, j=%d, b=%d): got %r, model %r, " \
                    "integer tally %d, difference %+.6g weight units" % (
                        skip, i, j, len(bad), i, bad[0][0] + 1, j, bad[0][1] + 1, got[tuple(bad[0])], want[tuple(bad[0])],
                        int(H[tuple(bad[0])]), (got[tuple(bad[0])] - want[tuple(bad[0])]) * Meff)
                assert np.array_equal(Pij[j * s:(j + 1) * s, i * s:(i + 1) * s], want.T), (skip, i, j)
    finally:
        _restore(ctx)
