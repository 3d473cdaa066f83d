"""Several pseudocount / score settings of one alignment in one call (gdca_run_multi, gdca_run_multi_dev, gdca_run_ranked_multi,
gDCA_multi).  The front end runs once, the covariance of every distinct pseudocount is built from the stored Pij_true, settings
with the same pseudocount share one inverse -- and every member's output must be bit for bit that of a single run with its setting:
the scores, the ranking, the conditioning decisions (Newton-Schulz step, Cholesky fallback, the sweep's second attempt) and the
failure status of a member whose covariance is not positive definite."""
import os

import numpy as np
import pytest

from gdca_testutil import compare_with_golden, random_msa

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


def _singles(ctx, Zf, q, settings, theta):
    return [ctx.run(Zf, q, pc, theta, score, bool(apc)) for pc, score, apc in settings]


def _assert_same_as_singles(multi, singles):
    for k, ((S, st), (S1, st1)) in enumerate(zip(multi, singles)):
        assert np.array_equal(S, S1), (k, float(np.abs(S - S1).max()))
        for f in ("theta", "Meff", "pair_identity_sum", "thresh", "info", "refined", "N", "M", "q", "n", "n_pad"):
            assert st[f] == st1[f], (k, f, st[f], st1[f])


# unsorted pseudocounts, one repeated with both scores, APC on and off
SETTINGS = [(0.5, DI, 1), (0.2, FROB, 1), (0.8, FROB, 0), (0.2, DI, 1), (0.5, FROB, 1), (0.8, DI, 0)]
SHAPES = [(700, 60, 21, -1.0), (1200, 250, 21, 0.2), (900, 131, 5, -1.0), (500, 97, 21, 0.2)]   # (M, N, q, theta)


@pytest.mark.parametrize("M,N,q,theta", SHAPES, ids=["M%d-N%d-q%d-th%g" % s for s in SHAPES])
def test_every_member_is_its_single_run_bit_for_bit(g, ctx, M, N, q, theta):
    rng = np.random.default_rng(N * 7 + q)
    Zf = np.asfortranarray(random_msa(rng, M, N, q).T)
    want = _singles(ctx, Zf, q, SETTINGS, theta)
    _assert_same_as_singles(ctx.run_multi(Zf, q, SETTINGS, theta), want)
    # K = 1 is the single run itself
    _assert_same_as_singles(ctx.run_multi(Zf, q, SETTINGS[1:2], theta), want[1:2])
    # the ranked form against gdca_run_ranked, member by member
    sep = 4
    got = ctx.run_ranked_multi_ptr(Zf.ctypes.data, N, M, q, SETTINGS, theta, sep)
    for k, (pc, score, apc) in enumerate(SETTINGS):
        ii, jj, sc, st = ctx.run_ranked_ptr(Zf.ctypes.data, N, M, q, pc, theta, score, sep, apc=bool(apc))
        assert np.array_equal(got[k][0], ii) and np.array_equal(got[k][1], jj) and np.array_equal(got[k][2], sc), k
        assert got[k][3]["info"] == st["info"] and got[k][3]["Meff"] == st["Meff"]


def test_device_resident_form(g, ctx):
    import torch

    rng = np.random.default_rng(5)
    M, N, q = 800, 110, 21
    Zo = random_msa(rng, M, N, q)
    Zf = np.asfortranarray(Zo.T)
    settings = [(0.8, FROB, 1), (0.2, DI, 1), (0.2, FROB, 1)]
    want = _singles(ctx, Zf, q, settings, -1.0)
    dZ = torch.from_numpy(Zo).cuda()                                       # (M, N) row-major == N x M column-major
    dS = torch.full((len(settings), N, N), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                                               # (torch's stream is not the context's)
    sts = ctx.run_multi_dev(dZ.data_ptr(), N, M, q, settings, -1.0, dS.data_ptr())
    S = dS.cpu().numpy()
    for k in range(len(settings)):
        assert np.array_equal(S[k].T, want[k][0]), k                    # block k: N x N column-major
        assert sts[k]["info"] == 0 and sts[k]["Meff"] == want[k][1]["Meff"]
    # shared front end: the same theta / Meff / front-end times in every entry
    assert len({(st["theta"], st["Meff"], st["ms_theta"], st["ms_weights"]) for st in sts}) == 1


# ---- the reference's goldens through gDCA_multi ----------------------------------------------------------------------------------
def _golden_ok(R, path, exact_order=True):
    rep = compare_with_golden(R, path)
    assert rep["keys_equal"] and rep["max_rel"] <= 1e-6, rep
    assert rep["string_mismatches"] <= max(3, len(R) // 2000), rep
    assert rep["order_equal_mod_ties"], rep
    if exact_order:
        assert rep["order_equal"], rep


def test_goldens_through_gDCA_multi(g, ctx, refdata):
    from oracle import gdca_oracle as o

    small = os.path.join(refdata, "small.fasta.gz")
    R = g.gDCA_multi(small, [(0.8, ":frob"), (0.2, ":DI")], ctx=ctx)
    _golden_ok(R[0], os.path.join(refdata, "small.FNRout.txt"))
    # member 1 (DI at 0.2, duplicates kept) against the oracle's score matrix, through the same ranking rule
    Zo = o.read_fasta_alignment(small, 0.9)
    S_o = o.scores_from_Z(Zo, int(Zo.max()), 0.2, "auto", "DI")
    scale = float(np.abs(S_o).max())
    assert len(R[1]) > 0
    for i, j, s in R[1]:                                  # score_close's bar, entry by entry of the ranking
        ref = S_o[j - 1, i - 1]
        assert abs(s - ref) <= 1e-6 * abs(ref) + 1e-9 * scale, (i, j, s, ref)
    assert len(g.gdca.last_multi_stats) == 2 and g.gdca.last_multi_stats[1]["info"] == 0
    R = g.gDCA_multi(small, [{"pseudocount": 0.2, "score": "DI"}, {"pseudocount": 0.8, "score": "frob"}], remove_dups=True, ctx=ctx)
    _golden_ok(R[0], os.path.join(refdata, "small.DIRout.txt"))
    R = g.gDCA_multi(os.path.join(refdata, "large.fasta.gz"), [(0.2, "DI"), (0.8, "frob")], remove_dups=True, ctx=ctx)
    _golden_ok(R[0], os.path.join(refdata, "large.DIRout.txt"), exact_order=False)
    R1 = g.gDCA(os.path.join(refdata, "large.fasta.gz"), pseudocount=0.8, remove_dups=True, ctx=ctx)
    assert np.array_equal(R[1].i, R1.i) and np.array_equal(R[1].j, R1.j) and np.array_equal(R[1].score, R1.score)


# ---- conditioning, per pseudocount group -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ill(g):
    from gaussdca.jl_amd import synth

    return np.asfortranarray(synth.synth_family(430, 600, 21, 0x1C0D).T)   # the family of test_gpu_conditioning.py


def test_newton_schulz_and_cholesky_groups(g, ctx, ill):
    # pc 1e-6: one Newton-Schulz step (refined 1); pc 1e-8: the sweep gives up, blocked Cholesky answers (refined 2)
    settings = [(0.8, FROB, 1), (1e-6, FROB, 1), (0.8, DI, 1), (1e-8, FROB, 1)]
    want = _singles(ctx, ill, 21, settings, -1.0)
    assert [st["refined"] for _, st in want] == [0, 1, 0, 2]
    got = ctx.run_multi(ill, 21, settings, -1.0)
    _assert_same_as_singles(got, want)
    assert got[0][1]["refined"] == got[2][1]["refined"] == 0 and got[0][1]["matrix_norm1"] == 0.0


def test_a_second_attempt_of_the_sweep_per_group(g):
    rng = np.random.default_rng(77)
    M, N, q = 700, 90, 21
    Zf = np.asfortranarray(random_msa(rng, M, N, q).T)
    settings = [(0.8, FROB, 1), (0.2, DI, 1), (0.2, FROB, 0)]
    ref, c = g.Context(0), g.Context(0)
    try:
        want = _singles(ref, Zf, q, settings, -1.0)
        c.set_options(SWEEP_DEBUG=32)                     # the watchdog ends the first attempt of every inverse
        got = c.run_multi(Zf, q, settings, -1.0)
        assert all(st["sweep_retries"] > 0 for _, st in got)
        _assert_same_as_singles(got, want)
        rk = c.run_ranked_multi_ptr(Zf.ctypes.data, N, M, q, settings, -1.0, 5)
        for k, (pc, score, apc) in enumerate(settings):
            ii, jj, sc, _ = ref.run_ranked_ptr(Zf.ctypes.data, N, M, q, pc, -1.0, score, 5, apc=bool(apc))
            assert rk[k][3]["sweep_retries"] > 0
            assert np.array_equal(rk[k][0], ii) and np.array_equal(rk[k][1], jj) and np.array_equal(rk[k][2], sc), k
    finally:
        c.close()
        ref.close()


# ---- failure semantics -----------------------------------------------------------------------------------------------------------
def test_a_failing_member_leaves_the_others_computed(g, ctx):
    rng = np.random.default_rng(404)
    M, N, q = 600, 70, 21
    Zo = random_msa(rng, M, N, q)
    Zo[:, 11] = 3                                         # a constant column: its covariance block is exactly 0 at pc = 0
    Zf = np.asfortranarray(Zo.T)
    with pytest.raises(g.PosDefException) as e1:
        ctx.run(Zf, q, 0.0, -1.0, FROB)
    info = e1.value.info
    assert info > 0
    settings = [(0.8, FROB, 1), (0.0, FROB, 1), (0.0, DI, 1), (0.5, DI, 1)]
    want0, want3 = ctx.run(Zf, q, 0.8, -1.0, FROB), ctx.run(Zf, q, 0.5, -1.0, DI)
    with pytest.raises(g.PosDefException) as e:
        ctx.run_multi(Zf, q, settings, -1.0)
    assert e.value.info == info
    assert e.value.statuses == [g._lib.GDCA_OK, g._lib.GDCA_ENOTPD, g._lib.GDCA_ENOTPD, g._lib.GDCA_OK]
    res = e.value.results
    assert res[1][1]["info"] == res[2][1]["info"] == info
    assert np.array_equal(res[0][0], want0[0]) and np.array_equal(res[3][0], want3[0])
    assert res[0][1]["info"] == res[3][1]["info"] == 0
    # the ranked form: same status, the good members ranked as single runs rank them
    with pytest.raises(g.PosDefException) as e:
        ctx.run_ranked_multi_ptr(Zf.ctypes.data, N, M, q, settings, -1.0, 5)
    ii, jj, sc, _ = ctx.run_ranked_ptr(Zf.ctypes.data, N, M, q, 0.8, -1.0, FROB, 5)
    r0 = e.value.results[0]
    assert np.array_equal(r0[0], ii) and np.array_equal(r0[1], jj) and np.array_equal(r0[2], sc)
    # and the context works on afterwards
    _assert_same_as_singles(ctx.run_multi(Zf, q, [(0.8, FROB, 1), (0.5, DI, 1)], -1.0), [want0, want3])


def test_invalid_calls_run_nothing(g, ctx):
    import ctypes as C

    lib, L = ctx.lib, g._lib
    rng = np.random.default_rng(9)
    M, N, q = 300, 40, 21
    Zf = np.asfortranarray(random_msa(rng, M, N, q).T)

    def call(prm, K):
        S = np.full((max(K, 1), N, N), 7.25)
        sts = (L.Stats * max(K, 1))()
        for st in sts:
            st.info = 12345
        rc = lib.gdca_run_multi(ctx.h, L._p(Zf), N, M, q, prm, K, L._p(S), sts)
        assert np.all(S == 7.25) and all(st.info == 12345 for st in sts), "an invalid call must not run"
        return rc

    prm, K = L._multi_params([(0.8, FROB), (0.2, DI)], -1.0, True)
    prm[1].theta = 0.3                                    # mismatched theta
    assert call(prm, K) == L.GDCA_EINVAL
    prm, _ = L._multi_params([(0.8, FROB)] * 17, 0.2, True)
    assert call(prm, 0) == L.GDCA_EINVAL
    assert call(prm, 17) == L.GDCA_EINVAL
    prm, K = L._multi_params([(0.8, FROB), (1.5, DI), (0.2, FROB)], 0.2, True)
    assert call(prm, K) == L.GDCA_EINVAL
    prm, K = L._multi_params([(0.8, FROB), (0.2, 7)], 0.2, True)
    assert call(prm, K) == L.GDCA_EINVAL
    with pytest.raises(g.ArgumentError):
        ctx.run_multi(Zf, q, [(0.8, FROB)] * 17, -1.0)
    # the context is untouched by them
    _assert_same_as_singles(ctx.run_multi(Zf, q, [(0.8, FROB, 1), (0.2, DI, 1)], -1.0), _singles(ctx, Zf, q, [(0.8, FROB, 1), (0.2, DI, 1)], -1.0))
    assert C.sizeof(L.Stats) == lib.gdca_stats_bytes()
