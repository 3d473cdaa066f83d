"""The double-mutant scan on the device (gdca_double_mutant_scan*, gdca_double_mutants*, their fused forms, double_mutant_scan,
double_mutant_energies, gDCA_double_mutant_scan, gDCA_double_mutants) against tests/epistasis_model.py.

No tolerance is invented here: the listed double mutants are held against the longdouble model within ddE_bound, the maps within the
same bound (robust to near-ties: the exact ddE at the returned code against the exact minimum) and epi_bound, both derived in the
model file; the cross-check against the explicit double mutants adds the two order_bounds of tests/energy_model.py; everything about
the order of the operations, the minimiser, the mirror entries and the relation to the single-substitution scan is array_equal --
including the whole list form against the header's fixed f64 expressions evaluated by numpy on the device's own dE.

The map kernel's site tile is T = 4 sites and its sequence chunk 64 sequences: the shapes sit below, at and above both."""
import ctypes as C
import os

import numpy as np
import pytest

import energy_model as em
import epistasis_model as ep
import mutation_model as mm
from gdca_testutil import ctx, g, golden_model, mixed_sequences, synth_model  # noqa: F401 (g, ctx: fixtures)

pytestmark = pytest.mark.gpu

T, CHUNK = 4, 64
# (q, N, K): N = T - 1, T, T + 1, 2 T + 1; K = 1, 3, one chunk, one chunk + 1; q = 21 is the compile-time instance, the others the generic one
SHAPES = [(2, 2, 1), (5, 3, 3), (5, 4, 3), (5, 5, CHUNK + 1), (5, 9, CHUNK), (21, 7, CHUNK + 1), (31, 6, 3)]
# at width: 65 tiles a side (2145 tiles) with a ragged last tile; the benchmarked width, 125 tiles a side (7875 tiles: the tile index
# is recovered from a square root); a second sequence chunk with one live lane at a ragged width (11 tiles a side)
SHAPES += [(6, 257, 3), (3, 500, 2), (6, 41, CHUNK + 1)]
GOLD = [("small.fasta.gz", 0.8), ("small.fasta.gz", 0.2)]
ALL = SHAPES + GOLD
IDS = ["q%d-N%d-K%d" % c for c in SHAPES] + ["small-pc%g" % pc for _, pc in GOLD]


def symmetric(mJ):
    """the lower triangle mirrored: the device reads the lower triangle, the numpy model whatever entry it is handed"""
    return np.tril(mJ) + np.tril(mJ, -1).T


def raw_scan(ctx, mJ, Pi, X, q, want=(True, True, True)):
    """gdca_double_mutant_scan itself -> (Emin, code, epi), each indexed [k, i, j] (or None where not wanted)"""
    N, K = X.shape
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    Emin = np.full((K, N, N), np.nan) if want[0] else None
    code = np.full((K, N, N), -7, dtype=np.int32) if want[1] else None
    epi = np.full((K, N, N), np.nan) if want[2] else None
    mJ, Pi = np.ascontiguousarray(mJ), np.ascontiguousarray(Pi)
    ctx.check(ctx.lib.gdca_double_mutant_scan(ctx.h, p(mJ), p(Pi), N, q, p(X), K, p(Emin), p(code), p(epi)))
    return tuple(None if a is None else a.transpose(0, 2, 1) for a in (Emin, code, epi))  # [k, j, i] in memory


_cases = {}


def case(g, ctx, refdata, c):
    """Everything the first three tests share of one shape, computed once: the model, the sequences, the device's list form of every
    target of every pair ([k, pair, c - 1, b - 1]), its maps, its single-substitution scan, and the longdouble model's tensors"""
    if c in _cases:
        return _cases[c]
    if isinstance(c[0], str):
        Zo, q, mJ, Pi = golden_model(refdata, c[0], c[1])
        K = 3
        X = mixed_sequences(np.random.default_rng(17), Zo, q, K, shift=1)  # no gaps, random with gaps, a member
    else:
        q, N, K = c
        Zo, q, mJ, Pi = synth_model(q, N)
        X = mixed_sequences(np.random.default_rng(100 * q + N), Zo, q, K, shift=0 if K > 1 else 2)
    mJ = symmetric(mJ)
    N = X.shape[0]
    rec, pairs = ep.all_records(X, q)
    out = g.double_mutant_energies(mJ, Pi, X, rec, q, ctx=ctx).reshape(K, len(pairs), q, q)
    maps = raw_scan(ctx, mJ, Pi, X, q)
    dE = g.mutation_scan(mJ, Pi, X, q, ctx=ctx)
    pot = mm.potentials_exact(mJ, Pi, X, q)
    I, J = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    ref, bound, epi, epi_b = [], [], [], []
    for k in range(K):
        x = X[:, k]
        ddE, eps, dEm, bD = ep.ddE_exact(mJ, Pi, x, q, pot=tuple(a[k:k + 1] for a in pot))
        b = ep.ddE_bound(mJ, x, q, bD, ddE)
        ref.append(ddE[I, :, J, :].transpose(0, 2, 1))       # [pair, c, b]
        bound.append(b[I, :, J, :].transpose(0, 2, 1))
        e = ep.epi_exact(eps)
        epi.append(e)
        epi_b.append(ep.epi_bound(mJ, x, q, e))
    adm = np.stack([ep.admissible(X[:, k], q)[I, :, J, :].transpose(0, 2, 1) for k in range(K)])
    _cases[c] = dict(q=q, N=N, K=K, mJ=mJ, Pi=Pi, X=X, rec=rec, pairs=pairs, I=I, J=J, out=out, maps=maps, dE=dE, ref=np.stack(ref),
                     bound=np.stack(bound), epi=np.stack(epi), epi_b=np.stack(epi_b), adm=adm)
    return _cases[c]


# ---- 1. the list form against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_listed_double_mutants_against_the_model(g, ctx, refdata, c):
    d = case(g, ctx, refdata, c)
    err = np.abs(d["out"] - d["ref"]).astype(np.float64)
    z = d["bound"] == 0
    assert np.all(err[z] == 0)
    ratio = float((err[~z] / d["bound"][~z]).max()) if (~z).any() else 0.0
    print("%s: %d listed double mutants, max |ddE - ddE_exact| / bound = %.3g" % (c, d["out"].size, ratio))
    assert ratio <= 1.0, ratio


# ---- 2. exact relations --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_exact_relations(g, ctx, refdata, c):
    d = case(g, ctx, refdata, c)
    q, N, K, X, out, I, J = d["q"], d["N"], d["K"], d["X"], d["out"], d["I"], d["J"]
    Emin, code, epi = d["maps"]
    # the list form IS the header's fixed f64 expressions on the device's own dE
    for k in range(K):
        fixed = ep.ddE_fixed(d["mJ"], d["dE"][k], X[:, k], q)
        assert np.array_equal(out[k], fixed[I, :, J, :].transpose(0, 2, 1)), k
    # Emin = the minimum of the list form over the admissible targets, code = its first argmin in ascending code order
    flat = np.where(d["adm"], out, np.inf).reshape(K, len(I), q * q)
    assert np.array_equal(Emin[:, I, J], flat.min(axis=2))
    assert np.array_equal(code[:, I, J], flat.argmin(axis=2))  # (numpy's argmin: the first of equal minima)
    # [j, i] mirrors [i, j], the code transposed
    assert np.array_equal(Emin[:, J, I], Emin[:, I, J]) and np.array_equal(epi[:, J, I], epi[:, I, J])
    assert np.array_equal(code[:, J, I], ep.transpose_code(code[:, I, J], q))
    # the diagonal: +0.0, -1, +0.0
    ii = np.arange(N)
    for a in (Emin[:, ii, ii], epi[:, ii, ii]):
        assert np.all(a == 0.0) and not np.signbit(a).any()
    assert np.all(code[:, ii, ii] == -1)
    # records with b = x_i are the single change of the other site bit for bit (c = x_j likewise; both: +0.0)
    a = X.T.astype(np.int64) - 1                                    # [k, site]
    kk = np.arange(K)[:, None]
    pp = np.arange(len(I))[None, :]
    assert np.array_equal(out[kk, pp, :, a[:, I]], d["dE"][:, J, :])       # [k, pair, c]
    assert np.array_equal(out[kk, pp, a[:, J], :], d["dE"][:, I, :])       # [k, pair, b]
    both = out[kk, pp, a[:, J], a[:, I]]
    assert np.all(both == 0.0) and not np.signbit(both).any()
    # a record and its swap (k, j, c, i, b) give the same bits
    swapped = np.ascontiguousarray(d["rec"][:, [0, 3, 4, 1, 2]])
    assert np.array_equal(g.double_mutant_energies(d["mJ"], d["Pi"], X, swapped, q, ctx=ctx), out.reshape(-1))
    # the decoded wrapper says the same
    Em, si, sj, ee = g.double_mutant_scan(d["mJ"], d["Pi"], X, q, ctx=ctx)
    assert np.array_equal(Em, Emin) and np.array_equal(ee, epi)
    assert si.dtype == sj.dtype == np.int8 and np.array_equal(si[:, I, J], code[:, I, J] % q + 1) and np.array_equal(sj[:, I, J], code[:, I, J] // q + 1)
    assert np.array_equal(si[:, J, I], sj[:, I, J]) and np.array_equal(sj[:, J, I], si[:, I, J])
    assert np.all(si[:, ii, ii] == 0) and np.all(sj[:, ii, ii] == 0)
    assert np.all(si[:, I, J] != X.T[:, I]) and np.all(sj[:, I, J] != X.T[:, J])  # a true double substitution


# ---- 3. the maps against the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_maps_against_the_model(g, ctx, refdata, c):
    d = case(g, ctx, refdata, c)
    q, K, I, J = d["q"], d["K"], d["I"], d["J"]
    Emin, code, epi = d["maps"]
    P = len(I)
    ref = np.where(d["adm"], d["ref"], np.inf).reshape(K, P, q * q)
    bound = d["bound"].reshape(K, P, q * q)
    c0 = ref.argmin(axis=2)[:, :, None]
    cs = code[:, I, J].astype(np.int64)[:, :, None]
    assert np.all(np.take_along_axis(d["adm"].reshape(K, P, q * q), cs, axis=2))
    at = lambda A, ix: np.take_along_axis(A, ix, axis=2)[:, :, 0]  # noqa: E731
    # computed(c*) <= computed(c0): exact(c*) - exact(c0) <= bound(c*) + bound(c0), whatever near-ties there are
    gap = (at(ref, cs) - at(ref, c0)).astype(np.float64)
    tol = at(bound, cs) + at(bound, c0)
    assert np.all(gap >= 0) and np.all(gap <= tol), float((gap / tol).max())
    err = np.abs(Emin[:, I, J] - at(ref, cs)).astype(np.float64)
    assert np.all(err <= at(bound, cs)), float((err / at(bound, cs)).max())
    e_err = np.abs(epi - d["epi"]).astype(np.float64)
    off = ~np.eye(d["N"], dtype=bool)[None].repeat(K, 0)
    zero = d["epi_b"] == 0
    assert np.all(e_err[zero] == 0)
    r = float((e_err[off & ~zero] / d["epi_b"][off & ~zero]).max()) if (off & ~zero).any() else 0.0
    print("%s: minimiser differs from the exact one at %d of %d pairs; max |epi - epi_exact| / bound = %.3g" %
          (c, int((cs != c0).sum()), K * P, r))
    assert r <= 1.0, r


# ---- 4. order-fixed ------------------------------------------------------------------------------------------------------------------------
def some_records(rng, X, q, L):
    N, K = X.shape
    i = rng.integers(0, N, size=L)
    j = (i + rng.integers(1, N, size=L)) % N
    return np.stack([rng.integers(0, K, size=L), i, rng.integers(1, q + 1, size=L), j, rng.integers(1, q + 1, size=L)], axis=1).astype(np.int32)


@pytest.mark.parametrize("q,N", [(21, 9), (5, 6)])
def test_order_fixed(g, ctx, q, N):
    Zo, q, mJ, Pi = synth_model(q, N)
    mJ = symmetric(mJ)
    rng = np.random.default_rng(q + N)
    K = CHUNK + 60  # two sequence chunks
    X = mixed_sequences(rng, Zo, q, K, shift=3)
    maps = raw_scan(ctx, mJ, Pi, X, q)
    again = raw_scan(ctx, mJ, Pi, X, q)
    assert all(np.array_equal(a, b) for a, b in zip(maps, again))  # run to run
    x = np.asfortranarray(X[:, 117:118])
    alone = raw_scan(ctx, mJ, Pi, x, q)
    rec1 = some_records(rng, x, q, 500)
    out1 = g.double_mutant_energies(mJ, Pi, x, rec1, q, ctx=ctx)
    assert all(np.array_equal(a[117:118], b) for a, b in zip(maps, alone))
    for pos in (0, K - 1):  # the same sequence at either end of the batch
        Y = X.copy(order="F")
        Y[:, pos] = x[:, 0]
        got = raw_scan(ctx, mJ, Pi, Y, q)
        assert all(np.array_equal(a[pos:pos + 1], b) for a, b in zip(got, alone)), pos
        rec = rec1.copy()
        rec[:, 0] = pos
        assert np.array_equal(g.double_mutant_energies(mJ, Pi, Y, rec, q, ctx=ctx), out1), pos
    # a map alone is the same map
    only = raw_scan(ctx, mJ, Pi, X, q, want=(False, True, False))
    assert only[0] is None and only[2] is None and np.array_equal(only[1], maps[1])


def test_compile_time_and_generic_instance_give_the_same_bits(g, ctx):
    """q = 21 runs the instance with s = 20 at compile time; option EPI_GENERIC = 1 sends the same model through the generic one"""
    Zo, q, mJ, Pi = synth_model(21, 9)
    mJ = symmetric(mJ)
    X = mixed_sequences(np.random.default_rng(5), Zo, q, CHUNK + 3)
    maps = raw_scan(ctx, mJ, Pi, X, q)
    c = g.Context(0)
    try:
        c.set_option("EPI_GENERIC", 1)
        generic = raw_scan(c, mJ, Pi, X, q)
    finally:
        c.close()
    assert all(np.array_equal(a, b) for a, b in zip(maps, generic))


# ---- 5. the fused forms ------------------------------------------------------------------------------------------------------------------
def fused(c, Zf, q, pc, theta, X, rec):
    N, M = Zf.shape
    (Emin, code, epi), st = c.run_double_mutant_scan_ptr(Zf.ctypes.data, N, M, q, pc, theta, X.ctypes.data, X.shape[1])
    assert st["ms_fn"] == 0.0 and st["ms_score"] > 0.0 and st["ms_total"] >= st["ms_score"]
    out, st2 = c.run_double_mutants_ptr(Zf.ctypes.data, N, M, q, pc, theta, X.ctypes.data, X.shape[1], rec.ctypes.data, rec.shape[0])
    assert st2["ms_fn"] == 0.0 and st2["ms_score"] > 0.0
    return tuple(a.transpose(0, 2, 1) for a in (Emin, code, epi)), out, st


@pytest.mark.parametrize("pc,theta,dedup", [(0.8, "auto", False), (0.2, 0.3, True)])
def test_fused_is_the_operator_on_the_librarys_own_model(g, ctx, refdata, pc, theta, dedup):
    Zo, q, _, _ = golden_model(refdata, "small.fasta.gz", pc, theta, dedup)
    Zf = np.asfortranarray(Zo.T)
    th = -1.0 if theta == "auto" else theta
    X = mixed_sequences(np.random.default_rng(31), Zo, q, 6)
    rec = some_records(np.random.default_rng(32), X, q, 4000)
    Pi_true, Pij_true, _, _ = g.compute_weighted_frequencies(Zf, q, ":auto" if theta == "auto" else theta, ctx=ctx)
    Pi, Pij = g.add_pseudocount(Pi_true, Pij_true, pc, q, ctx=ctx)
    mJ = symmetric(g.inv_cholesky(g.compute_C(Pi, Pij, ctx=ctx), ctx=ctx))
    maps_f, out_f, st = fused(ctx, Zf, q, pc, th, X, rec)
    assert st["refined"] == 0 and st["M"] == Zo.shape[0]
    maps_o = raw_scan(ctx, mJ, Pi, X, q)
    assert all(np.array_equal(a, b) for a, b in zip(maps_f, maps_o))
    assert np.array_equal(out_f, g.double_mutant_energies(mJ, Pi, X, rec, q, ctx=ctx))
    # the file-level wrappers run the same thing
    fasta = os.path.join(refdata, "small.fasta.gz")
    kw = dict(pseudocount=pc, theta=":auto" if theta == "auto" else theta, remove_dups=dedup, ctx=ctx)
    Em, si, sj, ee = g.gDCA_double_mutant_scan(fasta, X, **kw)
    assert np.array_equal(Em, maps_f[0]) and np.array_equal(ee, maps_f[2])
    di, dj = g.dcautils.decode_double_code(maps_f[1], q)
    assert np.array_equal(si, di) and np.array_equal(sj, dj)
    assert np.array_equal(g.gDCA_double_mutants(fasta, X, rec, **kw), out_f)


@pytest.mark.parametrize("option,value,refined", [("CHOLESKY", 2, 2), ("REFINE", 1, 1)])
def test_fused_through_the_collect_time_branches(g, refdata, option, value, refined):
    """The stage is run AGAIN at collect time after the blocked Cholesky fallback and after a Newton-Schulz step (new score_target kinds on
    the one re-score path); the result is held against the model on the oracle's mJ, Pi.  ddE: within ddE_bound, nothing added (its
    delta_bounds are bounds of ANY summation order over N terms and leave room).  epi: epi_bound is the rounding of q^2 squares of
    four-entry differences of ONE matrix and nothing else, and these branches' inverses are not LAPACK's bits -- so, as
    tests/test_gpu_mutation.py::close_to_oracle and tests/test_gpu_energy.py::test_fused_parity do for the same reason, the suite's
    allowance for the library's inverse (score_close: rtol = 1e-6, atol_frac = 1e-9) is added to it.  (Measured on an MI355X without the
    allowance: epi at 0.35 of epi_bound through CHOLESKY=2 and at 2.6 through REFINE=1; ddE at 0.0038 and 0.0091 of ddE_bound.)"""
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    mJ = symmetric(mJ)
    Zf = np.asfortranarray(Zo.T)
    N = Zf.shape[0]
    X = mixed_sequences(np.random.default_rng(8), Zo, q, 2, shift=2)  # random with gaps, a member
    pairs = [(0, 1), (3, 4), (7, 40), (20, 52), (51, 52)]
    rec, pairs = ep.all_records(X, q, pairs)
    c = g.Context(0)
    try:
        c.set_option(option, value)
        (Emin, code, epi), out, st = fused(c, Zf, q, 0.8, -1.0, X, rec)
    finally:
        c.close()
    assert st["refined"] == refined, st
    out = out.reshape(2, len(pairs), q, q)
    worst = worst_e = 0.0
    for k in range(2):
        x = X[:, k]
        ddE, eps, _, bD = ep.ddE_exact(mJ, Pi, x, q)
        b = ep.ddE_bound(mJ, x, q, bD, ddE)
        e, adm = ep.epi_exact(eps), ep.admissible(x, q)
        eb = ep.epi_bound(mJ, x, q, e) + 1e-6 * e.astype(np.float64) + 1e-9 * float(e.max())
        for p, (i, j) in enumerate(pairs):
            r, bb = ep.by_code(ddE, i, j), ep.by_code(b, i, j)
            worst = max(worst, float((np.abs(out[k, p].reshape(-1) - r).astype(np.float64) / bb).max()))
            cs = int(code[k, i, j])
            assert ep.by_code(adm, i, j)[cs]
            ra = np.where(ep.by_code(adm, i, j), r, np.inf)
            c0 = int(ra.argmin())
            assert 0 <= float(r[cs] - r[c0]) <= bb[cs] + bb[c0], (k, i, j)
            worst = max(worst, float(abs(Emin[k, i, j] - r[cs]) / bb[cs]))
            worst_e = max(worst_e, float(abs(epi[k, i, j] - e[i, j]) / eb[i, j]))
    print("%s=%s: max |ddE - ddE_exact| / bound = %.3g, max |epi - epi_exact| / (bound + inverse allowance) = %.3g" % (option, value, worst, worst_e))
    assert worst <= 1.0 and worst_e <= 1.0, (worst, worst_e)


# ---- 6. against the independent kernel: explicit double mutants through gdca_energies -----------------------------------------------------
def test_against_the_energies_of_the_explicit_double_mutants(g, ctx, refdata):
    d = case(g, ctx, refdata, GOLD[0])
    q, N, mJ, Pi, X = d["q"], d["N"], d["mJ"], d["Pi"], d["X"]
    k = 2  # the member of the family
    E_wt = g.sequence_energies(mJ, Pi, X[:, k:k + 1], q, ctx=ctx)[0]
    _, B_wt, _ = em.energies_gather(mJ, Pi, X[:, k:k + 1], q)
    worst = 0.0
    for (i, j) in [(0, 1), (3, 30), (25, 26), (10, 52)]:
        p = d["pairs"].index((i, j))
        Xm = ep.explicit_double_mutants(X[:, k], i, j, q)
        E_mut = g.sequence_energies(mJ, Pi, Xm, q, ctx=ctx)
        _, B_mut, _ = em.energies_gather(mJ, Pi, Xm, q)
        tol = em.order_bound(N, q, B_mut) + em.order_bound(N, q, B_wt[0]) + d["bound"][k, p].reshape(-1)
        err = np.abs(d["out"][k, p].reshape(-1) - (E_mut - E_wt))
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), (i, j, float((err / tol).max()))
    print("list form vs explicit double mutants: max error / tolerance = %.3g" % worst)


# ---- 7. failure modes ------------------------------------------------------------------------------------------------------------------------
def test_failure_modes(g, ctx, refdata):
    Zo, q, mJ, Pi = synth_model(5, 9)
    N, K = 9, 5
    X = mixed_sequences(np.random.default_rng(9), Zo, q, K)
    rec = some_records(np.random.default_rng(10), X, q, 64)
    good = g.double_mutant_energies(mJ, Pi, X, rec, q, ctx=ctx)
    good_maps = raw_scan(ctx, mJ, Pi, X, q)
    # detected on the device: a bad symbol, a bad record
    for byte in (0, q + 1):
        Y = X.copy(order="F")
        Y[7, 4] = byte
        with pytest.raises(g.ArgumentError, match="symbol"):
            g.double_mutant_scan(mJ, Pi, Y, q, ctx=ctx)
        with pytest.raises(g.ArgumentError, match="symbol"):
            g.double_mutant_energies(mJ, Pi, Y, rec, q, ctx=ctx)
    for col, value in ((3, None), (2, 0), (4, q + 1), (0, K), (0, -1), (1, N), (3, -1)):
        bad = rec.copy()
        bad[17, col] = bad[17, 1] if value is None else value  # (None: i == j)
        with pytest.raises(g.ArgumentError, match="record"):
            g.double_mutant_energies(mJ, Pi, X, bad, q, ctx=ctx)
        assert np.array_equal(g.double_mutant_energies(mJ, Pi, X, rec, q, ctx=ctx), good)  # the context still works
    # straight at the C-ABI: nothing is run
    lib, EINVAL = ctx.lib, g._lib.GDCA_EINVAL
    p = g._lib._p
    A, Cd, Ep, out = np.full((K, N, N), np.nan), np.full((K, N, N), -7, dtype=np.int32), np.full((K, N, N), np.nan), np.full(64, np.nan)
    scan = lambda mJ_, Pi_, N_, q_, X_, K_, a, b, c: lib.gdca_double_mutant_scan(ctx.h, mJ_, Pi_, N_, q_, X_, K_, a, b, c)  # noqa: E731
    assert scan(p(mJ), p(Pi), 1, q, p(X), K, p(A), p(Cd), p(Ep)) == EINVAL            # N = 1
    assert scan(p(mJ), p(Pi), N, q, p(X), K, None, None, None) == EINVAL              # all outputs NULL
    assert scan(p(mJ), p(Pi), N, q, None, K, p(A), p(Cd), p(Ep)) == EINVAL            # X = NULL: no "scan Z itself" here
    assert scan(p(mJ), p(Pi), N, q, p(X), 0, p(A), p(Cd), p(Ep)) == EINVAL
    assert scan(p(mJ), p(Pi), N, 32, p(X), K, p(A), p(Cd), p(Ep)) == EINVAL
    assert scan(p(mJ), p(Pi), N, 1, p(X), K, p(A), p(Cd), p(Ep)) == EINVAL
    assert scan(None, p(Pi), N, q, p(X), K, p(A), p(Cd), p(Ep)) == EINVAL
    assert scan(p(mJ), None, N, q, p(X), K, p(A), p(Cd), p(Ep)) == EINVAL
    lst = lambda N_, X_, K_, m_, L_, o_: lib.gdca_double_mutants(ctx.h, p(mJ), p(Pi), N_, q, X_, K_, m_, L_, o_)  # noqa: E731
    assert lst(N, p(X), K, p(rec), 0, p(out)) == EINVAL                               # L = 0
    assert lst(1, p(X), K, p(rec), 64, p(out)) == EINVAL
    assert lst(N, None, K, p(rec), 64, p(out)) == EINVAL
    assert lst(N, p(X), K, None, 64, p(out)) == EINVAL
    assert lst(N, p(X), K, p(rec), 64, None) == EINVAL
    prm, st = g._lib.Params(0.5, -1.0, 0, 1), g._lib.Stats()
    Zf = np.asfortranarray(Zo.T)
    M = Zf.shape[1]
    run = lib.gdca_run_double_mutant_scan
    assert run(ctx.h, p(Zf), N, M, q, C.byref(prm), None, K, p(A), p(Cd), p(Ep), C.byref(st)) == EINVAL
    assert run(ctx.h, p(Zf), N, M, q, C.byref(prm), p(X), K, None, None, None, C.byref(st)) == EINVAL
    assert run(ctx.h, p(Zf), N, M, q, C.byref(prm), p(X), 0, p(A), p(Cd), p(Ep), C.byref(st)) == EINVAL
    assert run(ctx.h, None, N, M, q, C.byref(prm), p(X), K, p(A), p(Cd), p(Ep), C.byref(st)) == EINVAL
    runl = lib.gdca_run_double_mutants
    assert runl(ctx.h, p(Zf), N, M, q, C.byref(prm), p(X), K, p(rec), 0, p(out), C.byref(st)) == EINVAL
    assert runl(ctx.h, p(Zf), N, M, q, C.byref(prm), None, K, p(rec), 64, p(out), C.byref(st)) == EINVAL
    assert runl(ctx.h, p(Zf), N, M, q, C.byref(prm), p(X), K, None, 64, p(out), C.byref(st)) == EINVAL
    assert np.all(np.isnan(A)) and np.all(Cd == -7) and np.all(np.isnan(Ep)) and np.all(np.isnan(out))
    # the fused form reports a bad record too, and the context works afterwards
    bad = rec.copy()
    bad[5, 3] = bad[5, 1]
    with pytest.raises(g.ArgumentError, match="record"):
        ctx.run_double_mutants_ptr(Zf.ctypes.data, N, M, q, 0.5, -1.0, X.ctypes.data, K, bad.ctypes.data, 64)
    assert np.array_equal(g.double_mutant_energies(mJ, Pi, X, rec, q, ctx=ctx), good)
    assert all(np.array_equal(a, b) for a, b in zip(raw_scan(ctx, mJ, Pi, X, q), good_maps))


# ---- 8. a fused scan leaves nothing behind ------------------------------------------------------------------------------------------------
def test_a_fused_double_mutant_scan_leaves_nothing_behind(g, refdata):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", 0.8)
    Zf = np.asfortranarray(Zo.T)
    N, M = Zf.shape
    X = mixed_sequences(np.random.default_rng(21), Zo, q, 10)
    rec = some_records(np.random.default_rng(22), X, q, 100)
    used, fresh = g.Context(0), g.Context(0)
    try:
        (Emin, code, epi), _ = used.run_double_mutant_scan_ptr(Zf.ctypes.data, N, M, q, 0.8, -1.0, X.ctypes.data, 10)
        assert Emin.shape == (10, N, N) and np.all(np.isfinite(Emin)) and np.all(np.isfinite(epi)) and code.min() == -1
        out, _ = used.run_double_mutants_ptr(Zf.ctypes.data, N, M, q, 0.8, -1.0, X.ctypes.data, 10, rec.ctypes.data, 100)
        assert np.all(np.isfinite(out))
        S_used = used.run(Zf, q, 0.8, -1.0, 0)[0]
        S_fresh = fresh.run(Zf, q, 0.8, -1.0, 0)[0]
    finally:
        used.close()
        fresh.close()
    assert S_used.shape == (N, N) and np.array_equal(S_used, S_fresh)
