"""Annealed importance sampling without a GPU: the known answers of the start draws, the numpy statement of the rule
(tests/ais_model.py) against the exact partition function of a toy model, the exported symbols and bindings with their argument checks,
and the compiler's report on k_ais.hip."""
import ctypes
import os
import re

import numpy as np
import pytest

import ais_model as am
import mutation_model as mm
import sample_model as sm
from gdca_testutil import CSRC, HIPCC, ROOT, compiler_report
from test_sample_cpu import P_PASS, P_POWER, TOY_MODEL_SEED

NEW_SYMBOLS = ("gdca_log_partition_dev", "gdca_log_partition")

# the statistical test's fixed conditions (the GPU test runs the library under the same ones)
TOY_K = 32768
TOY_LADDER, TOY_WRONG_LADDER, TOY_SWEEP = np.linspace(0, 1, 17), np.linspace(0, 1.1, 17), 4
TOY_SHORT_LADDER, TOY_SHORT_SWEEP = np.linspace(0, 1, 5), 1
TOY_AIS_SEED = 0  # with it the checker alone passes every requirement below, in both state spaces (asserted here)


# ---- 1. known answers of the start draws -------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_starts():
    ikey = am.start_key(0, 0)
    assert ikey == 0x1c44fab6a246bae2 == sm.mix64(~sm.key(0, 0) & sm.M64)
    table = [(0, 0x3dc548297666b4b4, (0, 0, 4, 5)), (4, 0xace4d333b149e3d1, (2, 2, 13, 14)), (69, 0x8537d76ccb32cd7e, (1, 2, 10, 10))]
    for m, r, symbols in table:
        assert sm.draw(ikey, m) == r, m
        assert tuple(am.start_symbol(r, T) for T in (3, 4, 20, 21)) == symbols, m
    # starts: the template's site list, position by position -- no flag: gaps stay gaps and a masked site keeps its symbol
    q = 21
    x = np.array([3, q, 7, 1, q, 20, 5], dtype=np.int8)
    mask = np.array([1, 1, 0, 1, 1, 1, 1], dtype=np.int8)
    X0 = am.starts(x, q, mask, 0, 0, 0, 2)
    assert X0.shape == (7, 2) and X0.dtype == np.int8
    assert np.array_equal(X0[[1, 2, 4], 0], [q, 7, q]) and np.array_equal(X0[[1, 2, 4], 1], [q, 7, q])
    assert X0[0, 0] == 4 + 1 and X0[6, 0] == am.start_symbol(sm.draw(ikey, 3), 20) + 1  # (sites 0, 3, 5, 6: positions 0 .. 3)
    assert X0[0, 1] == am.start_symbol(sm.draw(am.start_key(0, 1), 0), 20) + 1
    # the flag: every site the mask lets change, the gap a symbol
    Xg = am.starts(x, q, mask, sm.GAPS, 0, 0, 1)
    assert Xg[2, 0] == 7 and Xg[0, 0] == 5 + 1 and Xg[6, 0] == am.start_symbol(sm.draw(ikey, 5), 21) + 1
    # no template: every site is free, more than 64 of them
    Xn = am.starts(None, 5, None, sm.GAPS, 0, 0, 1, N=70)
    assert Xn.shape == (70, 1) and Xn[0, 0] == am.start_symbol(0x3dc548297666b4b4, 5) + 1
    assert Xn[69, 0] == am.start_symbol(0x8537d76ccb32cd7e, 5) + 1 and Xn.min() >= 1 and Xn.max() <= 5
    # an all-gap template without the flag has no site
    assert np.array_equal(am.starts(np.full(4, q, dtype=np.int8), q, None, 0, 3, 9, 2), np.full((4, 2), q))


# ---- 2. the rule estimates Z ------------------------------------------------------------------------------------------------------------------
def toy_ais(flags, betas, sweep, seed, run=None):
    """the log-weights (K,) of TOY_K annealed chains on the toy model over all N = 4 sites, by `run` (default: ais_model.emulate_chains
    with thresholds from np.log) -> (logw, n_sites, T)"""
    q = 4
    mJ, Pi = sm.toy_model(TOY_MODEL_SEED)
    if run is not None:
        return np.asarray(run(mJ, Pi, q, flags, betas, sweep, seed)), 4, sm.targets(q, flags)
    X0 = am.starts(None, q, None, flags, seed, 0, TOY_K, N=4)
    # (the tables and energies of the at most 256 distinct starts, once each)
    code, inv = np.unique(sm.state_index(X0.T, q), return_inverse=True)
    first = np.array([np.nonzero(inv == j)[0][0] for j in range(len(code))])
    V0 = mm.potentials_dense(mJ, Pi, X0[:, first], q)[inv]
    E0 = am.energies_dense(mJ, Pi, X0[:, first], q)[inv]
    return am.emulate_chains(V0, E0, mJ, X0, q, betas, sweep, None, None, flags, seed, 0)[0], 4, sm.targets(q, flags)


def toy_log_z(flags, beta=1.0):
    mJ, Pi = sm.toy_model(TOY_MODEL_SEED)
    return am.log_z_exact(mJ, Pi, 4, beta, flags, None, None, N=4)


def assert_estimates_z(flags, run=None, what="checker"):
    """the two toy cases and the power case under the fixed conditions, by `run`"""
    lz = toy_log_z(flags)
    for tag, betas, sweep in (("17-point ladder, sweep 4", TOY_LADDER, TOY_SWEEP), ("5-point ladder, sweep 1", TOY_SHORT_LADDER, TOY_SHORT_SWEEP)):
        logw, n_sites, T = toy_ais(flags, betas, sweep, TOY_AIS_SEED, run)
        assert logw.shape == (TOY_K,) and T ** n_sites == (256 if flags else 81)
        z, p = am.z_test(logw, lz - n_sites * np.log(np.longdouble(T)))
        lz_hat, ess = (float(v) for v in am.reduce_exact(logw, n_sites, T)[:2])
        print("%s flags %d, %s: log Z %.6f (exact %.6f), ess %.0f of %d, z = %.2f, p = %.3g" % (what, flags, tag, lz_hat, float(lz), ess, TOY_K, z, p))
        assert p >= P_PASS, (tag, z, p)
    # power: the same run on a ladder that ends at the wrong temperature must be seen
    logw, n_sites, T = toy_ais(flags, TOY_WRONG_LADDER, TOY_SWEEP, TOY_AIS_SEED, run)
    z, p = am.z_test(logw, lz - n_sites * np.log(np.longdouble(T)))
    print("%s flags %d, ladder to beta 1.1 against Z(1): log Z %.6f, z = %.1f, p = %.3g" % (what, flags, float(am.reduce_exact(logw, n_sites, T)[0]), z, p))
    assert p < P_POWER, (z, p)


@pytest.mark.parametrize("flags", [0, sm.GAPS])
def test_the_rule_estimates_z(flags):
    assert_estimates_z(flags)


def test_the_vectorised_checker_is_the_checker():
    q = 4
    mJ, Pi = sm.toy_model(TOY_MODEL_SEED)
    rng = np.random.default_rng(5)
    X = np.asfortranarray(rng.integers(1, q + 1, size=(4, 6)).astype(np.int8))
    X[:, 5] = q
    V0 = mm.potentials_dense(mJ, Pi, X, q)
    E0 = am.energies_dense(mJ, Pi, X, q)
    mask = np.array([1, 0, 1, 1], dtype=np.int8)
    for flags, msk, betas, sweep in ((0, None, np.linspace(0, 1, 5), 3), (sm.GAPS, None, np.array([0.0, 0.6, 0.3, 1.0]), 4),
                                     (0, mask, np.array([0.0, 2.0]), 5), (sm.GAPS, mask, np.array([0.0, 0.0, 0.5]), 1)):
        L = len(betas) - 1
        n_steps = L * sweep
        thr = np.stack([-np.log(sm.uniforms(9, 11 + k, n_steps)[1]) for k in range(6)])
        logw, E_end, Xout, acc = am.emulate_chains(V0, E0, mJ, X, q, betas, sweep, thr, msk, flags, 9, 11)
        again = am.emulate_chains(V0, E0, mJ, X, q, betas, sweep, None, msk, flags, 9, 11)
        assert all(np.array_equal(a, b) for a, b in zip((logw, E_end, Xout, acc), again))
        for k in range(6):
            moves, a1, x1, lw1, Ee1 = am.emulate(V0[k], E0[k], mJ, X[:, k], q, betas, sweep, thr[k], msk, flags, 9, 11 + k)
            assert a1 == acc[k] and np.array_equal(x1, Xout[k]) and lw1 == logw[k] and Ee1 == E_end[k], (flags, k)
            if len(sm.sites_of(X[:, k], q, msk, flags)) == 0:
                assert np.all(moves == am.INT_MIN) and a1 == 0 and np.array_equal(x1, X[:, k]) and Ee1 == E0[k]
                want = np.float64(0.0)
                for l in range(1, L + 1):
                    want = want + (betas[l - 1] - betas[l]) * (E0[k] + 0.0)
                assert lw1 == want
            else:
                assert (moves >= 0).sum() == a1
            if L == 1:
                assert lw1 == (0.0 - betas[1]) * E0[k]  # plain importance sampling


def test_the_exact_reduction():
    rng = np.random.default_rng(1)
    logw = rng.normal(size=1000) * 3
    lz, ess, m, lo = am.reduce_exact(logw, 4, 3)
    w = np.exp(logw.astype(np.longdouble))
    assert abs(float(lz - np.log(81 * w.mean()))) < 1e-15 * 10 and abs(float(ess - w.sum() ** 2 / (w * w).sum())) < 1e-9
    assert m == logw.max() and abs(float(lo) - 4 * np.log(3)) < 1e-15
    assert 1.0 <= ess <= 1000.0
    # Z of a model without couplings and fields is |Omega|
    assert abs(float(am.log_z_exact(np.zeros((9, 9)), np.zeros(9), 4, 1.0, sm.GAPS, None, None, N=3)) - 3 * np.log(4)) < 1e-15


# ---- 3. exports, bindings, argument checks --------------------------------------------------------------------------------------------------
def test_exports_bindings_and_argument_checks():
    import gaussdca.jl_amd as g
    from gaussdca.jl_amd import _lib, devops
    from test_cabi_cpu import _header_prototypes

    assert os.path.exists(_lib.LIB_PATH), "libgdca.so not built"
    raw = ctypes.CDLL(_lib.LIB_PATH)
    protos = _header_prototypes()
    for s in NEW_SYMBOLS:
        assert hasattr(raw, s), s
        assert len(_lib.SYMBOLS[s][1]) == len(protos[s][1]) == 22, s
    assert protos["gdca_log_partition"][1][12:14] == ["uint64_t", "uint64_t"] and _lib.SYMBOLS["gdca_log_partition"][1][12:14] == [ctypes.c_uint64] * 2
    assert g.load().gdca_version() == 6
    hdr = open(os.path.join(ROOT, "include", "gdca.h")).read()
    assert "Log partition function (annealed importance sampling)" in hdr and "0x8537d76ccb32cd7e" in hdr
    assert callable(g.log_partition) and callable(g.potts_loglik) and callable(devops.log_partition_dev)
    assert hasattr(g.Context, "log_partition_dev")

    N, q = 6, 4
    n = N * (q - 1)
    mJ, Pi = np.eye(n), np.full(n, 0.1)
    x = np.array([1, 2, 3, 4, 1, 2], dtype=np.int8)
    with pytest.raises(g.ArgumentError, match="incompatible sizes"):
        g.log_partition(mJ, Pi[:-1], q)
    with pytest.raises(g.ArgumentError, match="incompatible sizes"):
        g.log_partition(mJ, np.full(n + 1, 0.1), q)
    with pytest.raises(g.ArgumentError, match="too big"):
        g.log_partition(mJ, Pi, 32)
    for bad in ([0.0], [0.1, 1.0], [0.0, -1.0], [0.0, float("nan")], [0.0, float("inf")], "x"):
        with pytest.raises(g.ArgumentError, match="betas"):
            g.log_partition(mJ, Pi, q, betas=bad)
    for bad in (0, -1, 2.5):
        with pytest.raises(g.ArgumentError, match="n_stages"):
            g.log_partition(mJ, Pi, q, n_stages=bad)
    for bad in (-1e-9, float("nan"), float("inf"), "x"):
        with pytest.raises(g.ArgumentError, match="beta"):
            g.log_partition(mJ, Pi, q, beta=bad)
    for bad in (0, -1, 1.5):
        with pytest.raises(g.ArgumentError, match="sweep"):
            g.log_partition(mJ, Pi, q, sweep=bad)
    with pytest.raises(g.ArgumentError, match="2\\^31"):
        g.log_partition(mJ, Pi, q, n_stages=2 ** 16, sweep=2 ** 15)
    for bad in (0, -1, 2.0):
        with pytest.raises(g.ArgumentError, match="K"):
            g.log_partition(mJ, Pi, q, K=bad)
    for bad in (np.ones(N - 1, dtype=np.int8), np.zeros(N, dtype=np.int8), np.full(N, q + 1), np.ones(N) * 1.5):
        with pytest.raises(g.ArgumentError, match="x must"):
            g.log_partition(mJ, Pi, q, x=bad)
    for bad in (np.ones(N - 1), np.ones((N, 2)), np.ones(N) * 0.5):
        with pytest.raises(g.ArgumentError, match="mask"):
            g.log_partition(mJ, Pi, q, x=x, mask=bad)
    with pytest.raises(g.ArgumentError, match="mask needs a template"):
        g.log_partition(mJ, Pi, q, mask=np.ones(N, dtype=np.int8))
    for name in ("seed", "stream0"):
        for bad in (-1, 2 ** 64, 0.5):
            with pytest.raises(g.ArgumentError, match=name):
                g.log_partition(mJ, Pi, q, **{name: bad})
    with pytest.raises(g.ArgumentError, match="target symbols"):
        g.log_partition(np.eye(N), np.full(N, 0.5), 2)
    # potts_loglik: a sequence outside the state space
    X = np.asfortranarray(np.repeat(x[:, None], 3, axis=1))
    with pytest.raises(g.ArgumentError, match="outside the state space"):
        g.potts_loglik(mJ, Pi, X, q)  # (a gap at site 3, no gaps=True)
    Xd = X.copy()
    Xd[0, 1] = 2
    with pytest.raises(g.ArgumentError, match="outside the state space"):
        g.potts_loglik(mJ, Pi, Xd, q, x=x, mask=np.array([0, 1, 1, 1, 1, 1]), gaps=True)
    with pytest.raises(g.ArgumentError, match="trace"):
        g.potts_loglik(mJ, Pi, X, q, gaps=True, trace=True)
    if g.load().gdca_device_count() <= 0:
        # valid arguments, no device: an error, never a CPU computation (tests/test_cabi_cpu.py::test_no_cpu_fallback)
        with pytest.raises(g.GdcaError):
            g.log_partition(mJ, Pi, q, n_stages=3, K=4)
        with pytest.raises(g.GdcaError):
            g.potts_loglik(mJ, Pi, X, q, gaps=True, n_stages=3, K=4)


# ---- 4. the compiler's report on k_ais.hip --------------------------------------------------------------------------------------------------
def test_ais_kernels_do_not_spill_and_hold_no_barrier_in_a_divergent_loop(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    report = compiler_report(tmp_path, "k_ais.hip", kernels=("k_aisILb1E", "k_aisILb0E", "k_ais_start", "k_ais_reduce"))
    assert len(report) == 4
    for name, field in report:
        assert field("SGPRs Spill") == 0, name
        if "k_aisILb" in name:
            assert field(r"LDS Size \[bytes/block\]") == 0  # (the table and the lists are the launch's dynamic LDS)
    # each chain instance as k_sample's (the proposal loop with the update loop in it, the prologue's and the epilogue's loops), the
    # start's loop and the reduction's two
    compiler_report(tmp_path, "k_ais.hip", min_loops=15)
    code = "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, "k_ais.hip")).read().split("\n"))
    body = re.search(r"void k_ais\(const k_ais_args p\)\n\{\n(.*?)\n\}\n", code, re.S).group(1)
    # the chain kernel's own text adds no barrier to the chain body's four and shares nothing between threads
    assert "chain_run<TL>(" in body and "__syncthreads()" not in body and "atomic" not in body
    chain = open(os.path.join(CSRC, "gdca_chain.h")).read()
    assert len(re.findall(r"__syncthreads\(\)", chain)) == 4 and "beta_at(beta, tt) * dE <= thr" in chain
