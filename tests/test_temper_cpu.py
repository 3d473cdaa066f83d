"""Replica exchange over the Metropolis chains without a GPU: the swap generator's known answers, the numpy statement of the rule
(tests/temper_model.py) against itself, against tests/sample_model.py at R = 1 and against the exact Boltzmann distribution of a toy
model with a barrier the plain chains do not cross, the exported symbols and bindings with their argument checks, and the compiler's
report on k_temper.hip."""
import ctypes
import os
import re

import numpy as np
import pytest

import mutation_model as mm
import sample_model as sm
import temper_model as tm
from gdca_testutil import CSRC, HIPCC, ROOT, compiler_report
from test_sample_cpu import P_PASS, P_POWER

NEW_SYMBOLS = ("gdca_sample_tempered_dev", "gdca_sample_tempered", "gdca_run_sample_tempered_dev", "gdca_run_sample_tempered")

TOY_CHAIN_SEED = 1  # with it the tempered checker passes and the two wrong runs are seen (asserted here); the GPU test runs under the same conditions


# ---- 1. known answers ---------------------------------------------------------------------------------------------------------------------------
def test_known_answers():
    table = [((0, 0, 0, 3), 0x1c44fab6a246bae2, {0: 0x3dc548297666b4b4, 4: 0xace4d333b149e3d1}),
             ((1, 5, 2, 4), 0x56a6a56ca201d633, {0: 0x9faf955cbe491e47, 5: 0xf81e54a1e15977ed})]
    for (seed, stream0, k, R), sk, draws in table:
        assert tm.skey(seed, stream0, k, R) == sk == sm.mix64(~sm.key(seed, stream0 + k * R) & sm.M64)
        u = tm.swap_uniforms(seed, stream0, k, R, 2)
        for c, v in draws.items():
            assert sm.draw(sk, c) == v
            assert u[c // R, c % R] == sm.uniform53(v)  # counter e R + p: the round and the pair
    assert tm.swap_uniforms(0, 0, 0, 3, 2)[0, 0] == 0.24129153263347802 and tm.swap_uniforms(1, 5, 2, 4, 2)[1, 1] == 0.9692128081527239
    ref = tm.swap_thresholds_exact(0, 0, 0, 3, 2)
    assert abs(float(ref[0, 0]) + np.log(0.24129153263347802)) <= np.spacing(1.5)
    # the swap key is not a proposal key of the chain's own streams
    assert tm.skey(0, 0, 0, 3) not in [sm.key(0, s) for s in range(8)]
    assert tm.attempts(3, 8).tolist() == [4, 4] and tm.attempts(4, 7).tolist() == [4, 3, 4] and tm.attempts(1, 5).tolist() == []
    assert tm.attempted(4, 2).tolist() == [[True, False, True], [False, True, False]]


# ---- 2. the checkers ----------------------------------------------------------------------------------------------------------------------------
def checker_case(R, K=5):
    q = 4
    mJ, Pi = sm.toy_model(7)
    rng = np.random.default_rng(R)
    Xr = rng.integers(1, q + 1, size=(K, R, 4)).astype(np.int8)
    Xr[K - 1] = q
    V0 = mm.potentials_dense(mJ, Pi, np.asfortranarray(Xr.reshape(K * R, 4).T), q).reshape(K, R, 4, q)
    E0 = np.array([tm.energy_dense(mJ, Pi, x, q) for x in Xr.reshape(K * R, 4)]).reshape(K, R)
    return q, mJ, Pi, Xr, V0, E0


@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_the_vectorised_checker_is_the_checker(R):
    q, mJ, Pi, Xr, V0, E0 = checker_case(R)
    K = len(Xr)
    betas = [1.0, 0.3, 0.6, 0.0][:R]  # (not monotone)
    mask = np.array([1, 0, 1, 1], dtype=np.int8)
    slot0 = np.stack([np.random.default_rng(k).permutation(R) for k in range(K)])
    swapped = 0
    for flags, msk, s0 in ((0, None, None), (sm.GAPS, None, slot0), (sm.GAPS, mask, None)):
        kw = dict(mask=msk, flags=flags, seed=9, stream0=11, swap_every=2, burn=4, stride=6, n_samples=3, slot0=s0)
        n_steps, n_rounds = 22, 11
        thr = np.stack([-np.log(sm.uniforms(9, 11 + g, n_steps)[1]) for g in range(K * R)]).reshape(K, R, n_steps)
        sthr = np.stack([-np.log(tm.swap_uniforms(9, 11, k, R, n_rounds)) for k in range(K)])
        a = tm.emulate_chains(V0, E0, mJ, Xr, q, betas, thr, sthr, **kw)
        b = tm.emulate_chains(V0, E0, mJ, Xr, q, betas, None, None, **kw)
        assert all(np.array_equal(a[n], b[n]) for n in a)
        for k in range(K):
            one = tm.emulate(V0[k], E0[k], mJ, Xr[k], q, betas, thr[k], sthr[k], **dict(kw, stream0=11 + k * R, slot0=None if s0 is None else s0[k]))
            for n in a:
                assert np.array_equal(one[n], a[n][k]), (R, flags, k, n)
            assert one["accepted"].sum() == (one["moves"] >= 0).sum() and sorted(one["slot_out"]) == list(range(R))
            assert np.array_equal(one["slot_path"][-1], one["slot_out"]) and np.all(one["swaps"] <= tm.attempts(R, n_rounds))
            if R == 1:
                Xs, dE_s, acc, moves, V = sm.emulate(V0[k, 0], mJ, Xr[k, 0], q, thr[k, 0], msk, flags, betas[0], 9, 11 + k, 4, 6, 3)
                assert np.array_equal(Xs, one["Xs"]) and np.array_equal(E0[k, 0] + dE_s, one["E_s"]) and acc == one["accepted"][0]
                assert np.array_equal(moves, one["moves"][0]) and np.array_equal(V, one["V"][0])
        swapped += int(a["swaps"].sum())
    assert R == 1 or swapped > 0


def test_equal_betas_accept_every_swap_and_any_swap_every_is_the_same_chain_at_one_replica():
    q, mJ, Pi, Xr, V0, E0 = checker_case(3)
    a = tm.emulate_chains(V0, E0, mJ, Xr, q, [0.7] * 3, flags=sm.GAPS, seed=2, swap_every=3, burn=6, stride=3, n_samples=4)
    assert np.array_equal(a["swaps"], np.repeat(tm.attempts(3, 6)[None], len(Xr), axis=0))
    q, mJ, Pi, Xr, V0, E0 = checker_case(1)
    runs = [tm.emulate_chains(V0, E0, mJ, Xr, q, [1.0], flags=sm.GAPS, seed=2, swap_every=e, burn=10, stride=5, n_samples=4) for e in (1, 5)]
    assert all(np.array_equal(runs[0][n], runs[1][n]) for n in runs[0] if n != "slot_path")


# ---- 3. the barrier toy -----------------------------------------------------------------------------------------------------------------------
def test_tempering_crosses_the_barrier_the_plain_chains_do_not():
    Xs, rates, states, p = tm.toy_chains(tm.TOY_LADDER, TOY_CHAIN_SEED)
    assert len(states) == 81 and int((p * tm.TOY_K >= 5).sum()) >= 15
    pv, x2, df = sm.chi2_p(Xs, states, p, tm.TOY_Q)
    print("ladder %s: chi2 %.1f on %d degrees of freedom, p = %.3g, swap rates %s" % (tm.TOY_LADDER, x2, df, pv, np.round(rates, 3).tolist()))
    assert pv >= P_PASS, pv
    assert np.all((rates >= 0.3) & (rates <= 0.95)), rates
    # the plain chains under the same budget from the same start stay on their side of the barrier
    Xp, _, _, _ = tm.toy_chains((1.0,), TOY_CHAIN_SEED)
    pp, x2p, _ = sm.chi2_p(Xp, states, p, tm.TOY_Q)
    print("plain: chi2 %.1f, p = %.3g" % (x2p, pp))
    assert pp < P_POWER, pp
    # power: the ladder with the wrong target must be seen
    Xw, _, _, _ = tm.toy_chains((1.1,) + tm.TOY_LADDER[1:], TOY_CHAIN_SEED)
    pw, x2w, _ = sm.chi2_p(Xw, states, p, tm.TOY_Q)
    print("target 1.1: chi2 %.1f, p = %.3g" % (x2w, pw))
    assert pw < P_POWER, pw


# ---- 4. exports, bindings, argument checks --------------------------------------------------------------------------------------------------
def test_exports_bindings_and_argument_checks(refdata, tmp_path):
    import gaussdca.jl_amd as g
    from gaussdca.jl_amd import _lib, devops
    from test_cabi_cpu import _header_prototypes

    assert os.path.exists(_lib.LIB_PATH), "libgdca.so not built"
    raw = ctypes.CDLL(_lib.LIB_PATH)
    protos = _header_prototypes()
    for s in NEW_SYMBOLS:
        assert hasattr(raw, s), s
        assert len(_lib.SYMBOLS[s][1]) == len(protos[s][1]), s
    assert len(protos["gdca_sample_tempered_dev"][1]) == 28 and len(protos["gdca_run_sample_tempered"][1]) == 29
    assert protos["gdca_sample_tempered"][1][12:14] == ["uint64_t", "uint64_t"]
    assert _lib.SYMBOLS["gdca_sample_tempered"][1][12:14] == [ctypes.c_uint64] * 2
    assert g.load().gdca_version() == 6
    hdr = open(os.path.join(ROOT, "include", "gdca.h")).read()
    assert "#define GDCA_TEMPER_MAX 64" in hdr and _lib.TEMPER_MAX == 64 and "Replica-exchange chains" in hdr
    assert callable(g.sample_tempered) and callable(g.gDCA_sample_tempered) and callable(devops.sample_tempered_dev)
    for m in ("sample_tempered_dev", "run_sample_tempered_dev", "run_sample_tempered_ptr"):
        assert hasattr(g.Context, m), m
    for f in (g.sample_tempered, g.gDCA_sample_tempered):
        assert "(betas[p] - betas[p + 1]) * (E_b - E_a)" in " ".join(f.__doc__.split()) and "beta * dE <= -log(u)" in f.__doc__
    assert "in sweeps" in g.gDCA_sample_tempered.__doc__.lower()

    fasta = os.path.join(refdata, "small.fasta.gz")  # N = 53
    missing = str(tmp_path / "missing.fasta")
    X = np.ones((53, 4), dtype=np.int8)
    mJ, Pi = np.eye(53 * 20), np.full(53 * 20, 0.05)
    ok = dict(betas=(1.0, 0.5))
    with pytest.raises(g.ArgumentError, match="incompatible sizes"):
        g.sample_tempered(mJ, Pi, X[:-1], 21, **ok)
    with pytest.raises(g.ArgumentError, match="too big"):
        g.sample_tempered(mJ, Pi, X, 32, **ok)
    with pytest.raises(g.ArgumentError, match="no sequence"):
        g.sample_tempered(mJ, Pi, X[:, :0], 21, **ok)
    with pytest.raises(g.ArgumentError, match="replicas"):
        g.sample_tempered(mJ, Pi, np.ones((53, 3, 4), dtype=np.int8), 21, **ok)
    for bad in ((), [1.0] * 65, (1.0, -1e-9), (float("nan"),), (1.0, float("inf")), "x", (1.0, None)):
        with pytest.raises(g.ArgumentError, match="betas"):
            g.sample_tempered(mJ, Pi, X, 21, betas=bad)
    for bad in (0, -1, 2.5, 7):  # (7 does not divide burn = 530 and stride = 53)
        with pytest.raises(g.ArgumentError, match="swap_every"):
            g.sample_tempered(mJ, Pi, X, 21, swap_every=bad, **ok)
    with pytest.raises(g.ArgumentError, match="swap_every"):
        g.sample_tempered(mJ, Pi, X, 21, swap_every=4, burn=8, stride=6, **ok)
    with pytest.raises(g.ArgumentError, match="swap_every"):
        g.sample_tempered(mJ, Pi, X, 21, swap_every=4, burn=6, stride=8, **ok)
    for name, bads in (("burn", (-1, 2.5)), ("stride", (0, -1, 1.5)), ("n_samples", (0, -3, 2.0))):
        for bad in bads:
            with pytest.raises(g.ArgumentError, match=name):
                g.sample_tempered(mJ, Pi, X, 21, **{name: bad}, **ok)
    with pytest.raises(g.ArgumentError, match="2\\^31"):
        g.sample_tempered(mJ, Pi, X, 21, burn=2 ** 31 - 1, stride=1, n_samples=1, swap_every=1, **ok)
    for name in ("seed", "stream0"):
        for bad in (-1, 2 ** 64, 0.5):
            with pytest.raises(g.ArgumentError, match=name):
                g.sample_tempered(mJ, Pi, X, 21, **{name: bad}, **ok)
    for bad in (np.ones(52), np.ones((53, 2)), np.ones(53) * 0.5):
        with pytest.raises(g.ArgumentError, match="mask"):
            g.sample_tempered(mJ, Pi, X, 21, mask=bad, **ok)
    for bad in (np.zeros((4, 2), dtype=int), np.array([[0, 1]] * 3), np.array([[0, 2]] * 4), np.array([[0.0, 1.0]] * 4)):
        with pytest.raises(g.ArgumentError, match="slot0"):
            g.sample_tempered(mJ, Pi, X, 21, slot0=bad, **ok)
    with pytest.raises(g.ArgumentError, match="target symbols"):
        g.sample_tempered(np.eye(53), np.full(53, 0.5), X, 2, **ok)
    with pytest.raises(g.ArgumentError, match="invalid pseudocount"):
        g.gDCA_sample_tempered(missing, X, pseudocount=1.5, **ok)
    with pytest.raises(g.ArgumentError, match="cannot open file"):
        g.gDCA_sample_tempered(missing, X, **ok)
    with pytest.raises(TypeError):
        g.gDCA_sample_tempered(fasta, X, score=":DI", **ok)
    with pytest.raises(g.ArgumentError, match="burn"):
        g.gDCA_sample_tempered(fasta, X, burn=-1, **ok)
    with pytest.raises(g.ArgumentError, match="sites"):
        g.gDCA_sample_tempered(fasta, X[:-1], **ok)
    if g.load().gdca_device_count() <= 0:
        # valid arguments, no device: an error, never a CPU computation (tests/test_cabi_cpu.py::test_no_cpu_fallback)
        with pytest.raises(g.GdcaError):
            g.sample_tempered(mJ, Pi, X, 21, **ok)
        with pytest.raises(g.GdcaError):
            g.gDCA_sample_tempered(fasta, X, **ok)
        with pytest.raises(g.GdcaError):  # the argument errors of the library itself come first, the device second
            g.gDCA_sample_tempered(fasta, X, betas=(1.0, 0.5), swap_every=7)


# ---- 5. the compiler's report on k_temper.hip -----------------------------------------------------------------------------------------------
def test_temper_kernels_do_not_spill_and_hold_no_barrier_on_a_rejected_proposal(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    report = compiler_report(tmp_path, "k_temper.hip", kernels=("k_temper_chainILb1E", "k_temper_chainILb0E", "k_temper_round", "k_temper_init",
                                                                "k_temper_finish", "k_temper_replicate"))
    assert len(report) == 6
    for name, field in report:
        assert field(r"LDS Size \[bytes/block\]") == 0  # (the table and the lists are the launch's dynamic LDS)
    compiler_report(tmp_path, "k_temper.hip", min_loops=12)
    code, hdr = ("\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, f)).read().split("\n")) for f in ("k_temper.hip", "gdca_chain.h"))
    assert "atomic" not in code and "atomic" not in hdr
    # the chain body is csrc/gdca_chain.h's: k_temper_chain runs it and adds no barrier
    kern = code[code.index("void k_temper_chain("):code.index("struct k_temper_init_args")]
    assert "chain_run<TL>(" in kern and len(re.findall(r"__syncthreads\(\)", kern)) == 0
    chain = hdr[hdr.index("int chain_run("):hdr.index("inline chain_args chain_args_of(")]
    # two barriers of the prologue, two of an accepted move -- none on the path of a rejected proposal
    assert len(re.findall(r"__syncthreads\(\)", chain)) == 4
    loop = chain[chain.index("for (int tt = p.t0;"):]
    assert len(re.findall(r"__syncthreads\(\)", loop)) == 2 and len(re.findall(r"__syncthreads\(\)", loop[loop.index("if (acc) {"):])) == 2
    # the update the accepted move calls between its two barriers holds none of its own, nor does anything else of the header
    assert len(re.findall(r"__syncthreads\(\)", hdr[hdr.index("void chain_rows("):hdr.index("struct chain_layout")])) == 0
    assert len(re.findall(r"__syncthreads\(\)", hdr)) == 4
    # the round: one barrier, between the pairs' writes and the reads of the maps
    assert len(re.findall(r"__syncthreads\(\)", code)) == 1
