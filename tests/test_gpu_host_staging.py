"""The host-pointer entry points of libgdca.so and the staging layer they share (host_stage in csrc/gdca_api.hip).

1. A context with an enqueued ranked run refuses a host-pointer call BEFORE anything is uploaded: the enqueued run still refines from
   its own alignment.  (A collect that rebuilt C from the other family's bytes is off by orders of magnitude: the families are
   independent.)
2. A host-pointer form is its `_dev` form plus copies: the same kernels on the same inputs, so every output is equal bit for bit --
   one entry of every family, with the optional-argument corners the wrappers branch on.
3. The staging buffers grow inside a call and across calls without an earlier pointer of the call going stale.

Toy shapes throughout: N = 5, q = 3, M = 40, K = 3, split = 2, S = 2 species, L = 4 listed double mutants."""
import ctypes as C

import numpy as np
import pytest

from gaussdca.jl_amd.synth import synth_family
from gdca_testutil import ctx, g, score_close  # noqa: F401 (g, ctx: fixtures)

pytestmark = pytest.mark.gpu

N, Q, M, K, SPLIT, S, L = 5, 3, 40, 3, 2, 2, 4
NN = N * (Q - 1)
PAIR_ENERGY, MUT_DELTA = 1, 0  # GDCA_PAIR_ENERGY, GDCA_MUT_DELTA
FILL, PAD = 0x5A, 16  # every staged buffer of a test is PAD bytes longer than its array; the tail must keep its FILL bytes


# ---- the guard ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option,refined", [(("REFINE", 1), 1), (("CHOLESKY", 2), 2)])
def test_pending_context_refuses_host_forms_before_it_uploads(g, option, refined):
    Z, Z2 = (np.ascontiguousarray(synth_family(12, 200, 5, seed)) for seed in (11, 12))   # (M, N): the 12 x 200 column-major alignment
    Nz, Mz, qz = 12, 200, 5
    assert not np.array_equal(Z, Z2)
    rng = np.random.default_rng(5)
    A48 = rng.standard_normal((48, 48))
    n = Nz * (qz - 1)
    mJ, Pi, X, E = rng.standard_normal((n, n)), rng.random(n), rng.integers(1, qz + 1, size=(3, Nz)).astype(np.int8), np.empty(3)
    c0, c1 = g.Context(0), g.Context(0)
    try:
        for c in (c0, c1):
            c.set_option(*option)
        i0, j0, s0, st0 = c0.run_ranked_ptr(Z.ctypes.data, Nz, Mz, qz, 0.5, 0.2, 0, 1)
        assert st0["refined"] == refined
        c1.run_ranked_async_ptr(Z.ctypes.data, Nz, Mz, qz, 0.5, 0.2, 0, 1)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        S12, out = np.empty((12, 12)), C.c_uint64()
        with pytest.raises(g.ArgumentError, match="still enqueued"):
            c1.run(np.asfortranarray(Z2.T), qz, 0.5, 0.2, 0)
        for rc in (lambda: c1.lib.gdca_pair_identity_sum(c1.h, p(Z2), Nz, Mz, C.byref(out)),
                   lambda: c1.lib.gdca_fn(c1.h, p(A48), 12, 5, p(S12)),   # (a 48 x 48 matrix: N = 12, q = 5)
                   lambda: c1.lib.gdca_energies(c1.h, p(mJ), p(Pi), Nz, qz, p(X), 3, p(E))):
            with pytest.raises(g.ArgumentError, match="still enqueued"):
                c1.check(rc())
        i1, j1, s1, st1 = c1.run_ranked_collect()
        assert st1["refined"] == refined
        assert np.array_equal(i1, i0) and np.array_equal(j1, j0)
        # the suite's bar for scores (score_close takes score matrices: the ranked pairs put back into one)
        S0, S1 = np.zeros((Nz + 1, Nz + 1)), np.zeros((Nz + 1, Nz + 1))
        S0[i0, j0], S1[i1, j1] = s0, s1
        ok, max_rel, max_abs = score_close(S1, S0, rtol=1e-6, atol_frac=1e-9)
        print("max_rel %.3g max_abs %.3g" % (max_rel, max_abs))
        assert ok, (max_rel, max_abs)
    finally:
        c0.close()
        c1.close()


# ---- host form == device form ---------------------------------------------------------------------------------------------------
class In:
    """an input array (None: an optional argument left out)"""
    def __init__(self, a):
        self.a = a


class Out:
    """an output array of `nbytes` (want=False: an optional output left out); `init`: what the buffer holds before the call"""
    def __init__(self, nbytes, want=True, init=None):
        self.nbytes, self.want, self.init = int(nbytes), want, init


class Ref:
    """a host scalar the call writes through a pointer (the same in both forms): compared by value"""
    def __init__(self, ctype):
        self.ctype = ctype


def _flat(a):
    return np.frombuffer(np.ascontiguousarray(a.reshape(-1, order="A")).tobytes(), dtype=np.uint8)


def _call(ctx, name, spec, dev):
    """one form of an entry: arrays on the host (numpy) or on the device (torch); -> the outputs as bytes / values, in order"""
    import torch

    keep, args, outs = [], [], []
    for s in spec:
        if isinstance(s, In) and s.a is None or isinstance(s, Out) and not s.want:
            args.append(None)
            continue
        if isinstance(s, (In, Out)):
            body = _flat(s.a) if isinstance(s, In) else (np.full(s.nbytes, FILL, np.uint8) if s.init is None else _flat(s.init))
            buf = np.concatenate([body, np.full(PAD, FILL, np.uint8)])
            if dev:
                buf = torch.from_numpy(buf).cuda()
            keep.append(buf)
            args.append(C.c_void_p(buf.data_ptr() if dev else buf.ctypes.data))
            if isinstance(s, Out):
                outs.append(buf)
        elif isinstance(s, Ref):
            v = s.ctype()
            args.append(C.byref(v))
            outs.append(v)
        else:
            args.append(s() if callable(s) else s)
    if dev:
        torch.cuda.synchronize()
    ctx.check(getattr(ctx.lib, name + ("_dev" if dev else ""))(ctx.h, *args))
    ctx.synchronize()  # (the elementwise `_dev` forms return right after the launch)
    res = []
    for o in outs:
        if isinstance(o, (C.c_double, C.c_int32, C.c_uint64)):
            res.append(o.value)
            continue
        b = o.cpu().numpy() if dev else o
        assert np.all(b[-PAD:] == FILL), name + ": wrote past the end of an array"
        res.append(b[:-PAD].copy())
    return res


def both(ctx, name, *spec):
    """the host-pointer form and the `_dev` form of an entry on the same inputs: equal bit for bit; -> the host form's outputs"""
    h, d = _call(ctx, name, spec, False), _call(ctx, name, spec, True)
    assert len(h) == len(d)
    for k, (a, b) in enumerate(zip(h, d)):
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, b), "%s: output %d differs between the host and the device form" % (name, k)
        else:
            assert a == b or (a != a and b != b), (name, k, a, b)
    return h


def f64(b):
    return b.view(np.float64)


def i32(b):
    return b.view(np.int32)


@pytest.fixture(scope="module")
def toy(g, ctx):
    """the alignment, sequences and species of the cases below, and a model of the alignment from the operator chain itself (each
    link host == device): everything is computed once and left unchanged"""
    from gaussdca.jl_amd._lib import Params, Stats

    rng = np.random.default_rng(2024)
    t = dict(Z=np.ascontiguousarray(synth_family(N, M, Q, 77)))
    t["prm"] = Params(0.5, 0.2, 0, 0)
    t["stats"] = lambda: C.byref(Stats())
    t["X"] = rng.integers(1, Q + 1, size=(K, N)).astype(np.int8)            # (K, N) == N x K column-major
    t["XA"], t["XB"] = np.ascontiguousarray(t["X"][:, :SPLIT]), np.ascontiguousarray(t["X"][:, SPLIT:])
    t["offA"], t["offB"] = np.array([0, 1, 3], np.int32), np.array([0, 2, 3], np.int32)    # blocks 1 x 2 and 2 x 1
    t["offA0"], t["offB0"] = np.array([0, 0, 3], np.int32), np.array([0, 3, 3], np.int32)  # one side of every species empty
    W, Meff, theta_used, thresh = both(ctx, "gdca_compute_weights", In(t["Z"]), N, M, C.c_double(0.2), Out(M * 8), Ref(C.c_double),
                                       Ref(C.c_double), Ref(C.c_int32))
    assert theta_used == 0.2 and 0 < Meff <= M
    Pi_t, Pij_t = both(ctx, "gdca_frequencies", In(t["Z"]), N, M, Q, In(W), C.c_double(Meff), Out(NN * 8), Out(NN * NN * 8))
    Pi, Pij = both(ctx, "gdca_add_pseudocount", In(Pi_t), In(Pij_t), N, Q, C.c_double(0.5), Out(NN * 8), Out(NN * NN * 8))
    Cm, = both(ctx, "gdca_covariance", In(Pi), In(Pij), NN, Out(NN * NN * 8))
    mJ, info, logdet = both(ctx, "gdca_spd_inverse_logdet", Out(NN * NN * 8, init=Cm), NN, Ref(C.c_int32), Ref(C.c_double))
    assert info == 0 and np.isfinite(logdet)
    assert np.allclose(f64(mJ).reshape(NN, NN) @ f64(Cm).reshape(NN, NN), np.eye(NN), atol=1e-9)
    t.update(Pi=Pi, C=Cm, mJ=mJ)
    sym = lambda n: (lambda a: a + a.T)(rng.standard_normal((n, n)))  # noqa: E731
    t["mJA"], t["mJB"] = sym(SPLIT * (Q - 1)), sym((N - SPLIT) * (Q - 1))
    return t


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def test_score_operators(ctx, toy):
    t = toy
    S_fn, = both(ctx, "gdca_fn", In(t["mJ"]), N, Q, Out(N * N * 8))
    S_di, = both(ctx, "gdca_di", In(t["mJ"]), In(t["C"]), N, Q, Out(N * N * 8))
    assert not np.array_equal(S_fn, S_di)
    S_apc, = both(ctx, "gdca_apc", Out(N * N * 8, init=S_fn), N)
    assert not np.array_equal(S_apc, S_fn)


def test_energies_and_fused_energies(ctx, toy):
    t = toy
    E, = both(ctx, "gdca_energies", In(t["mJ"]), In(t["Pi"]), N, Q, In(t["X"]), K, Out(K * 8))
    assert np.all(np.isfinite(f64(E)))
    run = lambda X, k: both(ctx, "gdca_run_energies", In(t["Z"]), N, M, Q, C.byref(t["prm"]), In(X), k, Out((K if X is not None else M) * 8),  # noqa: E731
                            t["stats"])
    assert np.all(np.isfinite(f64(run(t["X"], K)[0])))
    assert np.all(np.isfinite(f64(run(None, 0)[0])))           # X absent: the alignment's own M sequences
    Lk, logdet = both(ctx, "gdca_run_loglik", In(t["Z"]), N, M, Q, C.byref(t["prm"]), In(None), 0, Out(M * 8), Ref(C.c_double), t["stats"])
    assert np.isfinite(logdet) and np.all(np.isfinite(f64(Lk)))


def test_pair_energies_blocks_and_matching(g, ctx, toy):
    t = toy
    model = (In(t["mJ"]), In(t["Pi"]), N, Q, SPLIT, In(t["XA"]), K, In(t["XB"]), K)
    E, = both(ctx, "gdca_pair_energies", *model, PAIR_ENERGY, Out(K * K * 8))
    Eb, = both(ctx, "gdca_pair_energies_blocked", *model, ptr(t["offA"]), ptr(t["offB"]), S, PAIR_ENERGY, Out(4 * 8))
    full = f64(E).reshape(K, K)                                # [b, a]: KA x KB column-major
    assert np.array_equal(f64(Eb), np.concatenate([full[0:2, 0:1].ravel(), full[2:3, 1:3].ravel()]))
    E0, = both(ctx, "gdca_pair_energies_blocked", *model, ptr(t["offA0"]), ptr(t["offB0"]), S, PAIR_ENERGY, Out(0))   # packed length 0
    assert E0.size == 0
    match, gap = both(ctx, "gdca_assign_blocks", In(f64(Eb)), ptr(t["offA"]), ptr(t["offB"]), S, Out(K * 4), Out(K * 8))
    match2, = both(ctx, "gdca_assign_blocks", In(f64(Eb)), ptr(t["offA"]), ptr(t["offB"]), S, Out(K * 4), Out(0, want=False))   # gap null
    assert np.array_equal(match, match2)
    m0, g0 = both(ctx, "gdca_assign_blocks", In(np.empty(0)), ptr(t["offA0"]), ptr(t["offB0"]), S, Out(K * 4), Out(K * 8))
    assert np.all(i32(m0) == -1) and np.all(f64(g0) == 0.0)    # every species comes back unmatched as a whole
    fused = lambda offA, offB, ne, wantE, wantgap: both(  # noqa: E731
        ctx, "gdca_run_partner_match", In(t["Z"]), N, M, Q, C.byref(t["prm"]), SPLIT, In(t["XA"]), K, In(t["XB"]), K, ptr(offA), ptr(offB), S, PAIR_ENERGY,
        Out(ne * 8, want=wantE), Out(K * 4), Out(K * 8, want=wantgap), t["stats"])
    Ef, mf, gf = fused(t["offA"], t["offB"], 4, True, True)
    mf2, = fused(t["offA"], t["offB"], 4, False, False)        # E_host null, gap null
    assert np.array_equal(mf, mf2)
    assert np.all(i32(fused(t["offA0"], t["offB0"], 0, True, True)[1]) == -1)


def test_pair_logodds_and_matching(ctx, toy):
    t = toy
    Lb, = both(ctx, "gdca_pair_logodds_blocked", In(t["mJ"]), In(t["mJA"]), In(t["mJB"]), In(t["Pi"]), N, Q, SPLIT, In(t["XA"]), K, In(t["XB"]), K,
               ptr(t["offA"]), ptr(t["offB"]), S, C.c_double(0.25), Out(4 * 8))
    assert np.all(np.isfinite(f64(Lb)))
    Lf, mf, gf = both(ctx, "gdca_run_partner_logodds", In(t["Z"]), N, M, Q, C.byref(t["prm"]), SPLIT, In(t["XA"]), K, In(t["XB"]), K,
                      ptr(t["offA"]), ptr(t["offB"]), S, Out(4 * 8), Out(K * 4), Out(K * 8), None, t["stats"])
    assert np.all(np.isfinite(f64(Lf)))


def test_selection_concatenation_and_the_loop(ctx, toy):
    t = toy
    match, gap = np.array([1, -1, 0], np.int32), np.array([0.5, 0.0, 2.0])
    sel, n_sel = both(ctx, "gdca_select_confident", In(match), In(gap), K, 2, Out(K * 4), Ref(C.c_int32))
    assert n_sel == 2
    selA, selB, col0, cols = np.array([0, 2], np.int32), np.array([1, 0], np.int32), 3, 6
    cat = lambda sa, sb, n, c0: both(ctx, "gdca_concat_pairs", In(t["XA"]), K, In(t["XB"]), K, N, SPLIT, In(sa), In(sb), n, Out(N * cols), c0)[0]  # noqa: E731
    Zc = cat(selA, selB, 2, col0).reshape(cols, N)
    assert np.all(Zc[:col0] == FILL) and np.all(Zc[col0 + 2:] == FILL)      # bytes outside the written columns: untouched
    want = np.concatenate([t["XA"][selA], t["XB"][selB]], axis=1)
    assert np.array_equal(Zc[col0:col0 + 2].view(np.int8), want)
    assert np.all(cat(None, None, 0, col0) == FILL)                          # n_sel == 0: nothing is written
    rounds = np.zeros(2 * 12)
    m, gp, mt, gt, done = both(ctx, "gdca_run_partner_ipa", In(t["XA"]), K, In(t["XB"]), K, ptr(t["offA"]), ptr(t["offB"]), S, N, Q, SPLIT, PAIR_ENERGY,
                               C.byref(t["prm"]), In(t["Z"]), M, None, None, 0, 1, 2, Out(K * 4), Out(K * 8), Out(2 * K * 4), Out(2 * K * 8),
                               ptr(rounds), Ref(C.c_int32), t["stats"])
    assert 1 <= done <= 2
    assert np.array_equal(i32(mt)[(done - 1) * K:done * K], i32(m))          # the last completed round's row of the trace
    assert np.all(mt[done * K * 4:] == FILL)                                 # the rows of rounds that did not run: untouched


def test_mutation_and_double_mutant_scans(ctx, toy):
    t = toy
    model = (In(t["mJ"]), In(t["Pi"]), N, Q, In(t["X"]), K)
    fit = (In(t["Z"]), N, M, Q, C.byref(t["prm"]), In(t["X"]), K)
    D, = both(ctx, "gdca_mutation_scan", *model, MUT_DELTA, Out(Q * N * K * 8))
    assert np.all(np.isfinite(f64(D)))
    maps = N * N * K
    code, = both(ctx, "gdca_double_mutant_scan", *model, Out(0, want=False), Out(maps * 4), Out(0, want=False))   # two of the three maps null
    Emin, code3, epi = both(ctx, "gdca_double_mutant_scan", *model, Out(maps * 8), Out(maps * 4), Out(maps * 8))
    assert np.array_equal(code, code3)
    muts = np.array([[0, 0, 1, 1, 2], [1, 4, 3, 2, 1], [2, 3, 2, 0, 3], [0, 2, 1, 4, 1]], np.int32)     # L records (k, i, b, j, c)
    dd, = both(ctx, "gdca_double_mutants", *model, In(muts), L, Out(L * 8))
    assert np.all(np.isfinite(f64(dd)))
    Ef, = both(ctx, "gdca_run_double_mutant_scan", *fit, Out(maps * 8), Out(0, want=False), Out(0, want=False), t["stats"])
    ddf, = both(ctx, "gdca_run_double_mutants", *fit, In(muts), L, Out(L * 8), t["stats"])
    assert np.all(np.isfinite(f64(Ef))) and np.all(np.isfinite(f64(ddf)))


# ---- buffers that grow inside and across calls ----------------------------------------------------------------------------------
def test_staging_buffers_grow_without_stale_pointers(g, toy):
    t = toy
    rng = np.random.default_rng(9)
    c = g.Context(0)
    try:
        for k in (3, 3000, 3):
            X = rng.integers(1, Q + 1, size=(k, N)).astype(np.int8)
            E, = both(c, "gdca_energies", In(t["mJ"]), In(t["Pi"]), N, Q, In(X), k, Out(k * 8))
            assert np.all(np.isfinite(f64(E)))
        # seven staged arrays straight after: the later ones are larger than what their buffers held so far
        both(c, "gdca_pair_logodds_blocked", In(t["mJ"]), In(t["mJA"]), In(t["mJB"]), In(t["Pi"]), N, Q, SPLIT, In(t["XA"]), K, In(t["XB"]), K,
             ptr(t["offA"]), ptr(t["offB"]), S, C.c_double(0.25), Out(4 * 8))
    finally:
        c.close()
