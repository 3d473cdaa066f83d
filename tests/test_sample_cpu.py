"""The Metropolis chains without a GPU: the generator's known answers, the numpy statement of the rule (tests/sample_model.py)
against the exact Boltzmann distribution of a toy model, the exported symbols and bindings with their argument checks, and the
compiler's report on k_sample.hip."""
import ctypes
import os
import re

import numpy as np
import pytest

import mutation_model as mm
import sample_model as sm
from gdca_testutil import CSRC, HIPCC, ROOT, compiler_report

NEW_SYMBOLS = ("gdca_sample_dev", "gdca_sample", "gdca_run_sample_dev", "gdca_run_sample")

# the statistical test's fixed conditions (the GPU test runs the library under the same ones)
TOY_MODEL_SEED, TOY_K, TOY_BURN = 7, 32768, 400
TOY_START = np.array([1, 2, 3, 1], dtype=np.int8)
TOY_CHAIN_SEED = 1  # with it the checker alone passes both requirements below, in both state spaces (asserted here)
P_PASS, P_POWER = 1e-4, 1e-6


# ---- 1. known answers ---------------------------------------------------------------------------------------------------------------------------
def test_known_answers():
    table = [((0, 0), 0xa706dd2f4d197e6f, [0x238275bc38fcbe91, 0xf89a2566b5822c54, 0x47200e1d9780fa44]),
             ((1, 0), 0x5e41ab087439611e, [0xb18a02f46d8d86c3, 0xf8c5b62c83f707e8]),
             ((1, 5), 0xc63f062c5c30e3d4, [0xfdba48dbc8c4fa9a]),
             ((2 ** 64 - 1, 2 ** 63), 0xf7f1454e6a8a1fa6, [0xe447897adec0a36e])]
    for (seed, stream), k, draws in table:
        assert sm.key(seed, stream) == k, (seed, stream)
        assert [sm.draw(k, c) for c in range(len(draws))] == draws
        assert [int(v) for v in sm.draw(k, np.arange(len(draws)))] == draws  # the vectorised form
    k = sm.key(1, 0)
    m, v, b = sm.proposal(sm.draw(k, 0), 53, 20, 3)
    u = sm.uniform53(sm.draw(k, 1))
    assert (m, v, b) == (36, 8, 9) and sm.proposal(sm.draw(k, 0), 53, 20, 8)[2] == 9 and sm.proposal(sm.draw(k, 0), 53, 20, 9)[2] == 8
    assert u == 0.9717668398552314 and -np.log(u) == 0.02863937998886221
    r0, us = sm.uniforms(1, 0, 3)
    assert int(r0[0]) == sm.draw(k, 0) and us[0] == u and int(r0[2]) == sm.draw(k, 4)
    assert abs(float(sm.thresholds_exact(1, 0, 1)[0]) - 0.02863937998886221) <= np.spacing(0.02863937998886221)
    # a counter constructed for a wanted draw (mix64 is a bijection): what the GPU test reaches the ends of u with
    for value, stream, c in ((2 ** 64 - 1, 0, 1), (0, 3, 1), (0x123456789abcdef0, 2 ** 40, 7)):
        assert sm.unmix64(sm.mix64(value)) == value and sm.draw(sm.key(sm.seed_for_draw(value, stream, c), stream), c) == value
    # the ends of u: every bit of r1 >> 11 set, none set
    assert sm.uniform53(2 ** 64 - 1) == 1.0 and sm.uniform53(0) == 2.0 ** -53 and sm.uniform53(2047) == 2.0 ** -53


# ---- 2. the rule samples the Boltzmann distribution ----------------------------------------------------------------------------------------
def toy_chains(flags, beta, seed, run=None):
    """the sampled states (K, N) of TOY_K chains of TOY_BURN proposals from TOY_START on the toy model, one sample each, by `run`
    (default: sample_model.emulate_chains with thresholds from np.log), and the exact distribution at beta = 1"""
    q = 4
    mJ, Pi = sm.toy_model(TOY_MODEL_SEED)
    X = np.asfortranarray(np.repeat(TOY_START[:, None], TOY_K, axis=1))
    if run is None:
        V0 = np.repeat(mm.potentials_dense(mJ, Pi, TOY_START[:, None], q), TOY_K, axis=0)
        Xs = sm.emulate_chains(V0, mJ, X, q, None, None, flags, beta, seed, 0, TOY_BURN, 1, 1)[0][:, 0]
    else:
        Xs = run(mJ, Pi, X, q, flags, beta, seed)
    states, p = sm.boltzmann(mJ, Pi, q, 1.0, flags, TOY_START)
    return Xs, states, p


@pytest.mark.parametrize("flags", [0, sm.GAPS])
def test_the_rule_samples_the_boltzmann_distribution(flags):
    Xs, states, p = toy_chains(flags, 1.0, TOY_CHAIN_SEED)
    assert len(states) == (256 if flags else 81) and float(p.max() / p.min()) >= 1e3
    pv, x2, df = sm.chi2_p(Xs, states, p, 4)
    print("flags %d: %d states, p_max / p_min %.3g, chi2 %.1f on %d degrees of freedom, p = %.3g" % (flags, len(states), float(p.max() / p.min()), x2, df, pv))
    assert pv >= P_PASS, pv
    # power: the same run at the wrong temperature must be seen
    Xw, _, _ = toy_chains(flags, 1.1, TOY_CHAIN_SEED)
    pw, x2w, _ = sm.chi2_p(Xw, states, p, 4)
    print("flags %d: beta x 1.1: chi2 %.1f, p = %.3g" % (flags, x2w, pw))
    assert pw < P_POWER, pw


def test_the_vectorised_checker_is_the_checker():
    q = 4
    mJ, Pi = sm.toy_model(TOY_MODEL_SEED)
    rng = np.random.default_rng(3)
    X = np.asfortranarray(rng.integers(1, q + 1, size=(4, 6)).astype(np.int8))
    X[:, 5] = q
    V0 = mm.potentials_dense(mJ, Pi, X, q)
    mask = np.array([1, 0, 1, 1], dtype=np.int8)
    for flags, msk, beta in ((0, None, 1.0), (sm.GAPS, None, 0.5), (0, mask, 2.0), (sm.GAPS, mask, 0.0)):
        burn, stride, S = 5, 3, 4
        n_steps = burn + S * stride
        thr = np.stack([-np.log(sm.uniforms(9, 11 + k, n_steps)[1]) for k in range(6)])
        Xs, dE_s, acc, V = sm.emulate_chains(V0, mJ, X, q, thr, msk, flags, beta, 9, 11, burn, stride, S)
        Xn = sm.emulate_chains(V0, mJ, X, q, None, msk, flags, beta, 9, 11, burn, stride, S)
        assert all(np.array_equal(a, b) for a, b in zip((Xs, dE_s, acc, V), Xn))
        for k in range(6):
            one = sm.emulate(V0[k], mJ, X[:, k], q, thr[k], msk, flags, beta, 9, 11 + k, burn, stride, S)
            assert np.array_equal(one[0], Xs[k]) and np.array_equal(one[1], dE_s[k]) and one[2] == acc[k] and np.array_equal(one[4], V[k])
            moves = one[3]
            if len(sm.sites_of(X[:, k], q, msk, flags)) == 0:
                assert np.all(moves == np.iinfo(np.int32).min) and acc[k] == 0 and np.all(Xs[k] == X[:, k])
            else:
                code = np.where(moves >= 0, moves, -1 - moves)
                assert (moves >= 0).sum() == acc[k] and np.all(sm.admissible(X[:, k], q, msk, flags)[code // q].any(axis=1))
                if beta == 0.0:
                    assert acc[k] == n_steps
            if msk is not None:
                assert np.all(Xs[k][:, 1] == X[1, k])
            if not flags:
                assert np.array_equal(Xs[k] == q, np.repeat((X[:, k] == q)[None], S, axis=0))


# ---- 3. exports, bindings, argument checks --------------------------------------------------------------------------------------------------
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
    assert len(protos["gdca_sample_dev"][1]) == 21 and len(protos["gdca_run_sample"][1]) == 23
    assert protos["gdca_sample"][1][10:12] == ["uint64_t", "uint64_t"] and _lib.SYMBOLS["gdca_sample"][1][10:12] == [ctypes.c_uint64] * 2
    assert g.load().gdca_version() == 6
    assert _lib.SAMPLE_GAPS == 1
    hdr = open(os.path.join(ROOT, "include", "gdca.h")).read()
    assert "enum { GDCA_SAMPLE_GAPS = 1 };" in hdr and "SAMPLE_CHUNK" in hdr and "Metropolis chains" in hdr
    assert callable(g.sample) and callable(g.gDCA_sample) and callable(devops.sample_dev)
    for m in ("sample_dev", "run_sample_dev", "run_sample_ptr"):
        assert hasattr(g.Context, m), m
    assert "one sweep is n proposals" in g.gDCA_sample.__doc__.lower() and "beta * dE <= -log(u)" in g.gDCA_sample.__doc__
    assert "Xs.reshape(N, -1" in g.gDCA_sample.__doc__

    fasta = os.path.join(refdata, "small.fasta.gz")  # N = 53
    missing = str(tmp_path / "missing.fasta")
    X = np.ones((53, 4), dtype=np.int8)
    mJ, Pi = np.eye(53 * 20), np.full(53 * 20, 0.05)
    with pytest.raises(g.ArgumentError, match="incompatible sizes"):
        g.sample(mJ, Pi, X[:-1], 21)
    with pytest.raises(g.ArgumentError, match="too big"):
        g.sample(mJ, Pi, X, 32)
    with pytest.raises(g.ArgumentError, match="no sequence"):
        g.sample(mJ, Pi, X[:, :0], 21)
    for bad in (-1e-9, float("nan"), float("inf"), "x"):
        with pytest.raises(g.ArgumentError, match="beta"):
            g.sample(mJ, Pi, X, 21, beta=bad)
    for name, bads in (("burn", (-1, 2.5)), ("stride", (0, -1, 1.5)), ("n_samples", (0, -3, 2.0))):
        for bad in bads:
            with pytest.raises(g.ArgumentError, match=name):
                g.sample(mJ, Pi, X, 21, **{name: bad})
    with pytest.raises(g.ArgumentError, match="2\\^31"):
        g.sample(mJ, Pi, X, 21, burn=2 ** 31 - 1, stride=1, n_samples=1)
    for name in ("seed", "stream0"):
        for bad in (-1, 2 ** 64, 0.5):
            with pytest.raises(g.ArgumentError, match=name):
                g.sample(mJ, Pi, X, 21, **{name: bad})
    for bad in (np.ones(52), np.ones((53, 2)), np.ones(53) * 0.5):
        with pytest.raises(g.ArgumentError, match="mask"):
            g.sample(mJ, Pi, X, 21, mask=bad)
    with pytest.raises(g.ArgumentError, match="target symbols"):
        g.sample(np.eye(53), np.full(53, 0.5), X, 2)
    with pytest.raises(g.ArgumentError, match="invalid pseudocount"):
        g.gDCA_sample(missing, X, pseudocount=1.5)
    with pytest.raises(g.ArgumentError, match="cannot open file"):
        g.gDCA_sample(missing, X)
    with pytest.raises(TypeError):
        g.gDCA_sample(fasta, X, score=":DI")
    with pytest.raises(g.ArgumentError, match="sites"):
        g.gDCA_sample(fasta, X[:-1])
    if g.load().gdca_device_count() <= 0:
        # valid arguments, no device: an error, never a CPU computation (tests/test_cabi_cpu.py::test_no_cpu_fallback)
        with pytest.raises(g.GdcaError):
            g.sample(mJ, Pi, X, 21)
        with pytest.raises(g.GdcaError):
            g.gDCA_sample(fasta, X)


# ---- 4. the compiler's report on k_sample.hip -----------------------------------------------------------------------------------------------
def test_sample_kernels_do_not_spill_and_hold_no_barrier_in_a_divergent_loop(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    report = compiler_report(tmp_path, "k_sample.hip", kernels=("k_sampleILb1E", "k_sampleILb0E"))
    assert len(report) == 2
    for name, field in report:
        assert field(r"LDS Size \[bytes/block\]") == 0  # (the table and the lists are the launch's dynamic LDS)
    # each instance: the proposal loop with the update loop in it, the loops of the prologue (symbols, table, site list) and the epilogue
    compiler_report(tmp_path, "k_sample.hip", min_loops=12)
    code, chain = ("\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, f)).read().split("\n")) for f in ("k_sample.hip", "gdca_chain.h"))
    # the chain body (csrc/gdca_chain.h): two barriers of the prologue, two of an accepted move -- none on the path of a rejected
    # proposal; the kernel adds none
    assert len(re.findall(r"__syncthreads\(\)", chain)) == 4 and "atomic" not in chain
    assert len(re.findall(r"__syncthreads\(\)", code)) == 0 and "atomic" not in code and "chain_run<TL>(" in code
