"""The greedy walk on the device (gdca_greedy_walk*, gdca_run_greedy_walk*, greedy_walk, gDCA_greedy_walk) against
tests/walk_model.py: the rule of include/gdca.h bit for bit (emulate, from the device's own initial table), the mathematics (the
exact replay in np.longdouble within the bounds derived in walk_model.py), and what the outputs may not depend on -- K, the position
in the batch, where the table lives, fused or operator.  No tolerance is invented here."""
import ctypes as C
import os

import numpy as np
import pytest

import energy_model as em
import walk_model as wm
from gdca_testutil import ctx, g, golden_model, mixed_sequences, synth_model  # noqa: F401 (g, ctx: fixtures)
from test_walk_cpu import TIE_CASES, tie_model

pytestmark = pytest.mark.gpu

NAMES = ("Xout", "steps", "dE_sum", "path", "dE_path", "V")


def walk(g, ctx, mJ, Pi, X, q, **kw):
    """greedy_walk with path and table as a dict of NAMES"""
    return dict(zip(NAMES, g.greedy_walk(mJ, Pi, X, q, path=True, table=True, ctx=ctx, **kw)))


def same(a, b, what=""):
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), (what, n)
    assert not np.signbit(a["dE_path"][a["dE_path"] == 0]).any()


def assert_is_the_rule(g, ctx, mJ, Pi, X, q, V0, mask=None, flags=0, min_gain=0.0, max_steps=None, tag=""):
    """every output of the device's walk == walk_model.emulate from the device's own initial table V0, sequence by sequence"""
    N, K = X.shape
    T = max_steps or 4 * N
    d = walk(g, ctx, mJ, Pi, X, q, mask=mask, gap_target=bool(flags & 1), fill_gaps=bool(flags & 2), min_gain=min_gain, max_steps=T)
    assert d["Xout"].shape == (N, K) and d["path"].shape == (K, T, 2) and d["dE_path"].shape == (K, T) and d["V"].shape == (K, N, q)
    for k in range(K):
        xout, steps, path, dE_path, dE_sum, V = wm.emulate(V0[k], mJ, X[:, k], q, mask, flags, min_gain, T)
        what = (tag, k, int(d["steps"][k]), steps)
        assert d["steps"][k] == steps, what
        assert np.array_equal(d["path"][k], path), what
        assert np.array_equal(d["dE_path"][k], dE_path), what
        assert np.array_equal(d["Xout"][:, k], xout), what
        assert np.array_equal(d["V"][k], V), what
        assert d["dE_sum"][k] == dE_sum and np.signbit(d["dE_sum"][k]) == np.signbit(dE_sum), what
        # the unused rows
        assert np.all(d["path"][k, steps:] == -1) and np.all(d["dE_path"][k, steps:] == 0.0) and not np.signbit(d["dE_path"][k, steps:]).any()
    return d


# ---- 1. the rule, bit for bit --------------------------------------------------------------------------------------------------------------
MODELS = [("small", 0.8), ("small", 0.2), (21, 53), (5, 30), (31, 41), (21, 200)]
MODEL_IDS = ["small-0.8", "small-0.2", "q21-N53", "q5-N30", "q31-N41", "q21-N200"]


def model(refdata, which):
    """(tag, K, seed of the sequences, Zo, q, mJ, Pi)"""
    a, b = MODELS[which]
    if a == "small":
        return ("small pc %g" % b, 8, 7) + golden_model(refdata, "small.fasta.gz", b)
    return ("synth q %d N %d" % (a, b), 36, 1000 * a + b) + synth_model(a, b)


@pytest.mark.parametrize("which", range(6), ids=MODEL_IDS)
def test_the_rule_bit_for_bit(g, ctx, refdata, which):
    tag, K, seed, Zo, q, mJ, Pi = model(refdata, which)
    N = Zo.shape[1]
    X = mixed_sequences(np.random.default_rng(seed), Zo, q, K)
    V0 = g.mutation_scan(mJ, Pi, X, q, what="potential", ctx=ctx)
    d = assert_is_the_rule(g, ctx, mJ, Pi, X, q, V0, tag=tag)
    print("%s: walk lengths %d .. %d of at most %d" % (tag, d["steps"].min(), d["steps"].max(), 4 * N))
    assert d["steps"].max() < 4 * N
    assert np.all(d["steps"][0::4] == 0) and np.array_equal(d["Xout"][:, 0::4], X[:, 0::4])  # all gaps, flags = 0: nothing may move
    assert np.array_equal(d["Xout"] == q, X == q)                                              # gaps stay gaps, residues stay residues
    assert_is_the_rule(g, ctx, mJ, Pi, X, q, V0, flags=3, tag=tag + " flags 3")
    mask = (np.arange(N) % 3 == 0).astype(np.int8)
    for flags in (0, 3):
        dm = assert_is_the_rule(g, ctx, mJ, Pi, X, q, V0, mask=mask, flags=flags, tag=tag + " mask")
        used = dm["path"][:, :, 0]
        assert np.all(used[used >= 0] % 3 == 0)
        assert np.array_equal(dm["Xout"][mask == 0], X[mask == 0])
        if flags == 0:
            assert not np.any(dm["path"][:, :, 1] == q)
    dg = assert_is_the_rule(g, ctx, mJ, Pi, X, q, V0, min_gain=0.5, tag=tag + " min_gain")
    taken = dg["path"][:, :, 0] >= 0
    assert np.all(dg["dE_path"][taken] < -0.5) and np.all(dg["steps"] <= d["steps"].max())


# ---- 2. the mathematics ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", [0.8, 0.2])
def test_the_mathematics(g, ctx, refdata, pc):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", pc)
    N = Zo.shape[1]
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 8)
    T = 4 * N
    d = walk(g, ctx, mJ, Pi, X, q, max_steps=T)
    assert d["steps"].min() == 0 and d["steps"].max() >= N and d["steps"].max() < T  # (tests/test_walk_cpu.py saw this on the model)
    E0 = g.sequence_energies(mJ, Pi, X, q, ctx=ctx)
    E1 = g.sequence_energies(mJ, Pi, d["Xout"], q, ctx=ctx)
    _, B0, _ = em.energies_gather(mJ, Pi, X, q)
    _, B1, _ = em.energies_gather(mJ, Pi, d["Xout"], q)
    worst = 0.0
    for k in range(8):
        steps = int(d["steps"][k])
        total, w = wm.check_walk(mJ, Pi, X[:, k], q, None, 0, 0.0, T, steps, d["path"][k], d["dE_path"][k], d["V"][k], "pc %g k %d" % (pc, k))
        worst = max(worst, w)
        tol = em.order_bound(N, q, B0[k]) + em.order_bound(N, q, B1[k]) + total
        err = abs((E1[k] - E0[k]) - d["dE_sum"][k])
        print("k %d: %3d steps, dE_sum %.6g, |energy difference - dE_sum| = %.3g, tolerance %.3g" % (k, steps, d["dE_sum"][k], err, tol))
        assert err <= tol, (k, err, tol)
        assert d["dE_sum"][k] <= 0.0
    print("pc %g: largest error / bound %.3g" % (pc, worst))


# ---- 3. one step is the scan's argmin ----------------------------------------------------------------------------------------------------------
def test_one_step_is_the_scans_argmin_and_short_walks_are_prefixes(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    N = Zo.shape[1]
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 8)
    D = g.mutation_scan(mJ, Pi, X, q, what="delta", ctx=ctx)
    full = walk(g, ctx, mJ, Pi, X, q, max_steps=4 * N)
    for flags in (0, 3):
        one = walk(g, ctx, mJ, Pi, X, q, max_steps=1, gap_target=bool(flags & 1), fill_gaps=bool(flags & 2))
        for k in range(8):
            adm = wm.admissible(X[:, k], q, None, flags)
            code = int(np.argmin(np.where(adm, D[k], np.inf)))
            i, b = divmod(code, q)
            if adm.any() and D[k, i, b] < 0.0:
                assert one["steps"][k] == 1 and tuple(one["path"][k, 0]) == (i, b + 1) and one["dE_path"][k, 0] == D[k, i, b], (flags, k)
                assert one["dE_sum"][k] == D[k, i, b]
            else:
                assert one["steps"][k] == 0 and tuple(one["path"][k, 0]) == (-1, -1), (flags, k)
    for t in (1, 5, 16):
        short = walk(g, ctx, mJ, Pi, X, q, max_steps=t)
        assert np.array_equal(short["steps"], np.minimum(full["steps"], t))
        assert np.array_equal(short["path"], full["path"][:, :t]) and np.array_equal(short["dE_path"], full["dE_path"][:, :t])
    assert (walk(g, ctx, mJ, Pi, X, q, max_steps=16)["steps"] == 16).any()  # at least one walk is cut off


# ---- 4. order-fixed ------------------------------------------------------------------------------------------------------------------------------
def test_order_fixed(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    K = 1000
    X = mixed_sequences(np.random.default_rng(5), Zo, q, K, shift=3)
    a = walk(g, ctx, mJ, Pi, X, q, max_steps=16)
    same(a, walk(g, ctx, mJ, Pi, X, q, max_steps=16), "run to run")
    x = np.asfortranarray(X[:, 417:418])
    alone = walk(g, ctx, mJ, Pi, x, q, max_steps=16)
    for n in NAMES:
        assert np.array_equal(a[n][..., 417:418] if n == "Xout" else a[n][417:418], alone[n]), n
    for pos in (0, K - 1):
        Y = X.copy(order="F")
        Y[:, pos] = x[:, 0]
        b = walk(g, ctx, mJ, Pi, Y, q, max_steps=16)
        for n in NAMES:
            assert np.array_equal(b[n][..., pos:pos + 1] if n == "Xout" else b[n][pos:pos + 1], alone[n]), (pos, n)


def test_a_batch_is_its_sequences_walked_one_at_a_time(g, ctx):
    Zo, q, mJ, Pi = synth_model(21, 200)
    K = 257
    X = mixed_sequences(np.random.default_rng(257), Zo, q, K, shift=1)
    a = walk(g, ctx, mJ, Pi, X, q)
    for k in (0, 1, 66, 130, 256):
        alone = walk(g, ctx, mJ, Pi, np.asfortranarray(X[:, k:k + 1]), q)
        for n in NAMES:
            assert np.array_equal(a[n][..., k:k + 1] if n == "Xout" else a[n][k:k + 1], alone[n]), (k, n)


# ---- 5. table placement ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [53, 200])
def test_table_in_lds_and_in_hbm_give_the_same_bits(g, N):
    Zo, q, mJ, Pi = synth_model(21, N)
    X = mixed_sequences(np.random.default_rng(N), Zo, q, 36)
    out = {}
    for where in ("lds", "hbm", "auto"):
        c = g.Context(0)
        try:
            c.set_option("WALK_TABLE", where)
            out[where] = walk(g, c, mJ, Pi, X, q)
            Xo, st, ds = g.greedy_walk(mJ, Pi, X, q, ctx=c)   # without the table and the path: the tables live in the context's workspace
            assert np.array_equal(Xo, out[where]["Xout"]) and np.array_equal(st, out[where]["steps"]) and np.array_equal(ds, out[where]["dE_sum"])
        finally:
            c.close()
    same(out["lds"], out["hbm"], "lds / hbm")
    same(out["lds"], out["auto"], "lds / auto")
    assert out["lds"]["steps"].max() >= N // 2


def test_an_unknown_table_placement_is_refused(g):
    c = g.Context(0)
    try:
        for bad in ("sram", "", "1"):
            with pytest.raises(g.ArgumentError):
                c.set_option("WALK_TABLE", bad)
        c.set_option("GDCA_WALK_TABLE", "HBM")
    finally:
        c.close()


# ---- 6. a big table ----------------------------------------------------------------------------------------------------------------------------------
def test_a_big_table(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "large.fasta.gz", 0.8)
    N = Zo.shape[1]
    assert (N, q) == (400, 21) and N * q * 8 > 64 * 1024
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 8)
    V0 = g.mutation_scan(mJ, Pi, X, q, what="potential", ctx=ctx)
    d = assert_is_the_rule(g, ctx, mJ, Pi, X, q, V0, tag="large")
    print("large: walk lengths", d["steps"].tolist())
    assert 300 <= d["steps"].max() < 4 * N
    # the other instance and the other paths at this width (N > 256: every loop over the sites takes a second pass): the table asked
    # into LDS and into HBM (k_walk<true>, k_walk<false>), a mask, both flags -- each the rule from the same V0, and the same bits
    mask = (np.arange(N) % 3 == 0).astype(np.int8)
    lds, hbm = g.Context(0), g.Context(0)
    try:
        lds.set_option("WALK_TABLE", "lds")
        hbm.set_option("WALK_TABLE", "hbm")
        for m, flags in ((None, 0), (mask, 0), (None, 3), (mask, 3)):
            tag = "large mask %d flags %d" % (m is not None, flags)
            a = assert_is_the_rule(g, lds, mJ, Pi, X, q, V0, mask=m, flags=flags, tag=tag + " lds")
            b = assert_is_the_rule(g, hbm, mJ, Pi, X, q, V0, mask=m, flags=flags, tag=tag + " hbm")
            same(a, b, tag + ": lds / hbm")
            print("%s: walk lengths %s" % (tag, a["steps"].tolist()))
            assert a["steps"].max() >= N // 4
            if m is None and flags == 0:
                same(a, d, "default placement")
            if m is not None:
                used = a["path"][:, :, 0]
                assert np.all(used[used >= 0] % 3 == 0) and np.array_equal(a["Xout"][mask == 0], X[mask == 0])
    finally:
        lds.close()
        hbm.close()


# ---- 7. lower triangle only ------------------------------------------------------------------------------------------------------------------------
def test_only_the_lower_triangle_is_read(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 8)
    a = walk(g, ctx, mJ, Pi, X, q)
    bad = mJ.copy()
    # (the library reads element (row, col), row >= col, of the column-major matrix at [col * n + row]: of the row-major array the
    # wrapper hands it that is numpy's UPPER triangle, so the library's strict upper triangle is numpy's strict lower one)
    bad[np.tril_indices_from(bad, -1)] = np.nan
    same(a, walk(g, ctx, bad, Pi, X, q), "NaN in the triangle that is not read")
    V0 = g.mutation_scan(bad, Pi, X, q, what="potential", ctx=ctx)
    assert np.all(np.isfinite(V0))
    assert_is_the_rule(g, ctx, bad, Pi, X, q, V0, tag="NaN triangle")


# ---- 8. fused against operator ------------------------------------------------------------------------------------------------------------------------
def test_fused_is_the_operator_on_the_librarys_own_model(g, ctx, refdata):
    Zo, q, _, _ = golden_model(refdata, "small.fasta.gz", 0.8)
    M, N = Zo.shape
    Zf = np.asfortranarray(Zo.T)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 8)
    pc = 0.8
    Pi_true, Pij_true, _, _ = g.compute_weighted_frequencies(Zf, q, ":auto", ctx=ctx)
    Pi, Pij = g.add_pseudocount(Pi_true, Pij_true, pc, q, ctx=ctx)
    mJ = g.inv_cholesky(g.compute_C(Pi, Pij, ctx=ctx), ctx=ctx)
    mJ = np.tril(mJ) + np.tril(mJ, -1).T
    T = 4 * N
    for flags in (0, 3):
        op = walk(g, ctx, mJ, Pi, X, q, max_steps=T, gap_target=bool(flags & 1), fill_gaps=bool(flags & 2))
        res, st = ctx.run_greedy_walk_ptr(Zf.ctypes.data, N, M, q, pc, -1.0, X.ctypes.data, 8, flags=flags, max_steps=T, path=True, table=True)
        same(dict(zip(NAMES, res)), op, "fused / operator, flags %d" % flags)
        assert st["ms_fn"] == 0.0 and st["ms_score"] > 0.0 and st["ms_total"] >= st["ms_score"]
    assert op["steps"].max() >= N // 2
    # X = None walks Z itself
    own, st = ctx.run_greedy_walk_ptr(Zf.ctypes.data, N, M, q, pc, -1.0, max_steps=16, path=True)
    assert own[0].shape == (N, M) and own[1].shape == (M,) and own[3].shape == (M, 16, 2) and st["M"] == M
    given, _ = ctx.run_greedy_walk_ptr(Zf.ctypes.data, N, M, q, pc, -1.0, Zf.ctypes.data, M, max_steps=16, path=True)
    for a, b in zip(own, given):
        assert np.array_equal(a, b)
    # the file-level entry
    fasta = os.path.join(refdata, "small.fasta.gz")
    res, _ = ctx.run_greedy_walk_ptr(Zf.ctypes.data, N, M, q, pc, -1.0, X.ctypes.data, 8, max_steps=T, path=True, table=True)
    top = g.gDCA_greedy_walk(fasta, X, path=True, table=True, ctx=ctx)
    assert len(top) == 6 and g.gdca.last_stats["ms_fn"] == 0.0
    for a, b in zip(top, res):
        assert np.array_equal(a, b)
    short = g.gDCA_greedy_walk(fasta, max_steps=16, ctx=ctx)
    assert len(short) == 3 and np.array_equal(short[0], own[0]) and np.array_equal(short[1], own[1]) and np.array_equal(short[2], own[2])


@pytest.mark.parametrize("option,value,refined", [("CHOLESKY", 2, 2), ("REFINE", 1, 1)])
def test_fused_walk_through_the_collect_time_branches(g, refdata, option, value, refined):
    """the stage runs AGAIN at collect time after the Cholesky fallback and after a Newton-Schulz step, as the mutation stage does: the
    walk returned is the walk of the model finally used -- it ends in a local minimum of the oracle's model up to the bounds"""
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 8)
    c = g.Context(0)
    try:
        c.set_option(option, value)
        Xout, steps, dE_sum = g.gDCA_greedy_walk(os.path.join(refdata, "small.fasta.gz"), X, ctx=c)
        assert g.gdca.last_stats["refined"] == refined
    finally:
        c.close()
    assert steps.min() == 0 and steps.max() >= Zo.shape[1] // 2 and np.all(dE_sum <= 0)
    assert np.array_equal(Xout == q, X == q)


# ---- 9. the exact-tie model ------------------------------------------------------------------------------------------------------------------------------
def test_exact_ties_on_the_device(g, ctx):
    mJ, Pi, x, V = tie_model()
    X = np.asfortranarray(np.repeat(x[:, None], 3, axis=1))
    assert np.array_equal(g.mutation_scan(mJ, Pi, X, 3, what="potential", ctx=ctx), np.repeat(V[None], 3, axis=0))
    for flags, mask, min_gain, moves, dEs, final in TIE_CASES:
        d = walk(g, ctx, mJ, Pi, X, 3, mask=mask, gap_target=bool(flags & 1), fill_gaps=bool(flags & 2), min_gain=min_gain, max_steps=8)
        for k in range(3):
            n = len(moves)
            assert d["steps"][k] == n and [tuple(r) for r in d["path"][k, :n]] == moves, (flags, mask, min_gain, d["path"][k])
            assert list(d["dE_path"][k, :n]) == dEs and d["dE_sum"][k] == sum(dEs)
            assert list(d["Xout"][:, k]) == final and np.array_equal(d["V"][k], V)
            assert np.all(d["path"][k, n:] == -1) and np.all(d["dE_path"][k, n:] == 0.0)


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(g, ctx, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    M, N = Zo.shape
    K, T = 8, 16
    X = mixed_sequences(np.random.default_rng(7), Zo, q, K)
    good = walk(g, ctx, mJ, Pi, X, q, max_steps=T)
    Y = X.copy(order="F")
    Y[7, 5] = q + 1
    with pytest.raises(g.ArgumentError):
        g.greedy_walk(mJ, Pi, Y, q, max_steps=T, ctx=ctx)
    with pytest.raises(g.ArgumentError):
        g.gDCA_greedy_walk(os.path.join(refdata, "small.fasta.gz"), Y, max_steps=T, ctx=ctx)
    same(walk(g, ctx, mJ, Pi, X, q, max_steps=T), good, "the context still works")

    # straight at the C-ABI: nothing is run, the outputs are untouched
    lib, p, EINVAL = ctx.lib, g._lib._p, g._lib.GDCA_EINVAL
    Xout, steps = np.full((N, K), 77, dtype=np.int8, order="F"), np.full(K, -7, dtype=np.int32)
    dsum, path, dpath, V = np.full(K, np.nan), np.full((K, T, 2), -7, dtype=np.int32), np.full((K, T), np.nan), np.full((K, N, q), np.nan)
    outs = (p(Xout), p(steps), p(dsum), p(path), p(dpath), p(V))

    def op(mJ_=p(mJ), Pi_=p(Pi), N_=N, q_=q, X_=p(X), K_=K, flags=0, min_gain=0.0, T_=T, outs_=outs):
        return lib.gdca_greedy_walk(ctx.h, mJ_, Pi_, N_, q_, X_, K_, None, flags, min_gain, T_, *outs_)

    assert op(K_=0) == EINVAL and op(K_=-1) == EINVAL and op(K_=2 ** 31 - 256) == EINVAL
    assert op(q_=1) == EINVAL and op(q_=32) == EINVAL
    assert op(T_=0) == EINVAL and op(T_=65536) == EINVAL and op(T_=-1) == EINVAL
    assert op(min_gain=-1e-300) == EINVAL and op(min_gain=float("nan")) == EINVAL
    assert op(flags=4) == EINVAL and op(flags=-1) == EINVAL
    assert op(X_=None) == EINVAL and op(mJ_=None) == EINVAL and op(Pi_=None) == EINVAL
    assert op(outs_=(None,) + outs[1:]) == EINVAL and op(outs_=(outs[0], None) + outs[2:]) == EINVAL
    prm, st = g._lib.Params(0.8, -1.0, 0, 1), g._lib.Stats()
    Zf = np.asfortranarray(Zo.T)

    def fused(Z_=p(Zf), q_=q, X_=p(X), K_=K, flags=0, min_gain=0.0, T_=T, outs_=outs, prm_=C.byref(prm)):
        return lib.gdca_run_greedy_walk(ctx.h, Z_, N, M, q_, prm_, X_, K_, None, flags, min_gain, T_, *outs_, C.byref(st))

    assert fused(K_=0) == EINVAL and fused(q_=32) == EINVAL and fused(T_=0) == EINVAL and fused(T_=65536) == EINVAL
    assert fused(min_gain=-1.0) == EINVAL and fused(min_gain=float("nan")) == EINVAL and fused(flags=8) == EINVAL
    assert fused(Z_=None) == EINVAL and fused(prm_=None) == EINVAL
    assert fused(outs_=(None,) + outs[1:]) == EINVAL and fused(outs_=(outs[0], None) + outs[2:]) == EINVAL
    assert np.all(Xout == 77) and np.all(steps == -7) and np.all(path == -7)
    assert np.all(np.isnan(dsum)) and np.all(np.isnan(dpath)) and np.all(np.isnan(V))
    # a table that cannot live in LDS, asked into LDS: N q doubles beyond 160 KiB
    c = g.Context(0)
    try:
        c.set_option("WALK_TABLE", "lds")
        Nb, qb = 1000, 21
        big = np.ones((Nb, 1), dtype=np.int8, order="F")
        rc = c.lib.gdca_greedy_walk(c.h, p(mJ), p(Pi), Nb, qb, p(big), 1, None, 0, 0.0, T, *outs)   # (refused before mJ is looked at)
        assert rc == EINVAL and b"LDS" in c.lib.gdca_last_error(c.h)
    finally:
        c.close()
    assert np.all(Xout == 77) and np.all(steps == -7)
    same(walk(g, ctx, mJ, Pi, X, q, max_steps=T), good, "the context still works")


def test_a_pending_context_refuses_the_host_forms(g, refdata):
    from gaussdca.jl_amd.synth import synth_family

    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 8)
    Z = np.ascontiguousarray(synth_family(12, 200, 5, 11))
    c = g.Context(0)
    try:
        c.run_ranked_async_ptr(Z.ctypes.data, 12, 200, 5, 0.5, 0.2, 0, 1)
        with pytest.raises(g.ArgumentError, match="still enqueued"):
            g.greedy_walk(mJ, Pi, X, q, max_steps=4, ctx=c)
        with pytest.raises(g.ArgumentError, match="still enqueued"):
            c.run_greedy_walk_ptr(np.asfortranarray(Zo.T).ctypes.data, Zo.shape[1], Zo.shape[0], q, 0.8, -1.0, X.ctypes.data, 8, max_steps=4)
        i1, j1, s1, st1 = c.run_ranked_collect()
        assert len(s1) > 0
        assert g.greedy_walk(mJ, Pi, X, q, max_steps=4, ctx=c)[1].max() == 4
    finally:
        c.close()
