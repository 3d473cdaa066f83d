"""Boltzmann-machine refinement without a GPU: tests/bm_model.py against itself (the vectorised loop and a scalar restatement), the
sign of the gradient on exact marginals, the learning run in pure numpy with its control -- the measurement the GPU test's bar comes
from --, the exported symbols and bindings with their argument checks, and the compiler's report on k_bm.hip."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bm_model as bm
import mutation_model as mm
import sample_model as sm
import tally_model as tm
from gdca_testutil import CSRC, FLAGS, HIPCC, ROOT, compiler_report

NEW_SYMBOLS = ("gdca_potts_from_gaussian_dev", "gdca_potts_from_gaussian", "gdca_bm_update_dev", "gdca_bm_update", "gdca_bm_readout_dev",
               "gdca_bm_readout", "gdca_bm_learn_dev", "gdca_bm_learn")

# ---- the learning problem (the GPU test runs the library on the same one) -------------------------------------------------------------------
# target: the exact marginals of sample_model.toy_model(N = 4, q = 3, ratio = 1e6) with the gap a symbol (81 states); start: the
# independent-site model of the target's Pi, whose exact pair frequencies are 0.0371 off at the worst entry.
LEARN = dict(K=1024, n_iter=400, burn=16, stride=1, n_samples=1, eta=1.0, seed=0, x_seed=100)
START_DEVIATION = 0.0371
# MEASURED with bm_model.learn (pure numpy, thresholds -np.log(u)) at exactly these settings, seeds 0 .. 5: the exact pair-frequency
# deviation of the learned model was 0.00621, 0.00856, 0.00277, 0.00336, 0.00352, 0.00665.  The bar is twice the largest: the device's
# thresholds may differ from numpy's by 2 ulp, so its run is another random realisation of the same process, not the same bits.
LEARN_MEASURED = (0.00621, 0.00856, 0.00277, 0.00336, 0.00352, 0.00665)
LEARN_BAR = 2 * 0.008562
assert LEARN_BAR < START_DEVIATION / 2  # the condition: otherwise the test could not tell learning from none


def learn_problem():
    """(N, q, Pi_target, Pij_target, W0, X0 (N, K), the start's exact deviation)"""
    N, q = 4, 3
    mJ, Pi = sm.toy_model(N=N, q=q, ratio=1e6)
    P1, P2, states, _ = bm.exact_marginals(mJ, Pi, q, N)
    assert len(states) == 81
    W0 = bm.potts_independent(P1, N, q)
    X0 = np.asfortranarray(np.random.default_rng(LEARN["x_seed"]).integers(1, q + 1, size=(N, LEARN["K"])).astype(np.int8))
    return N, q, P1, P2, W0, X0, bm.pair_deviation(W0, P2, q, N)


def small_family(seed=3, N=3, q=4, M=40):
    """(rng behind it, Z (N, M)): the alignment of small_problem"""
    rng = np.random.default_rng(seed)
    return rng, rng.integers(1, q + 1, size=(N, M)).astype(np.int8)


def small_problem(seed=3, N=3, q=4, K=6, M=40):
    rng, Z = small_family(seed, N, q, M)
    Pi_d, Pij_d = tm.frequencies(Z, np.ones(M), float(M), q)
    n = N * (q - 1)
    A = rng.normal(size=(n, n)) * 0.3
    W = np.where(bm.multipliers(N, q) == 1.0, A + A.T, 0.0)
    W[np.arange(n), np.arange(n)] = rng.normal(size=n)
    return N, q, W, Pi_d, Pij_d, np.asfortranarray(Z[:, :K])


# ---- 1. the model against itself --------------------------------------------------------------------------------------------------------------
def test_the_vectorised_loop_is_the_scalar_restatement():
    N, q, W, Pi_d, Pij_d, X = small_problem()
    mask = np.array([1, 0, 1], dtype=np.int8)
    for flags, msk, lam in ((bm.GAPS, None, 0.0), (0, None, 0.05), (bm.GAPS, mask, 0.05)):
        kw = dict(flags=flags, seed=5, iter0=2, burn=3, stride=2, n_samples=3, eta=0.7, lam=lam, mask=msk)
        Wv, Xv, tv = bm.learn(W, Pi_d, Pij_d, X, q, 4, **kw)
        Ws, Xs, ts = bm.learn_scalar(W, Pi_d, Pij_d, X, q, 4, **kw)
        assert np.array_equal(Wv, Ws) and np.array_equal(Xv, Xs) and np.array_equal(tv, ts, equal_nan=True)
        assert np.array_equal(Wv, Wv.T) and not np.array_equal(Wv, W)
        m = bm.multipliers(N, q)
        assert np.all(Wv[m == 0.0] == 0.0) and not np.signbit(Wv[m == 0.0]).any()
        # 4 = 1 + 3 through W, X and iter0
        Wa, Xa, ta = bm.learn(W, Pi_d, Pij_d, X, q, 1, **kw)
        Wb, Xb, tb = bm.learn(Wa, Pi_d, Pij_d, Xa, q, 3, **dict(kw, iter0=3))
        assert np.array_equal(Wb, Wv) and np.array_equal(Xb, Xv) and np.array_equal(np.concatenate((ta, tb)), tv, equal_nan=True)
        if msk is not None:
            assert np.array_equal(Xv[1], X[1])


def test_the_container_and_the_readout_of_the_model():
    N, q, W, Pi_d, Pij_d, X = small_problem(seed=4, N=5, q=3, M=60)
    n = N * (q - 1)
    rng = np.random.default_rng(0)
    # potts_from_gaussian: the same energies up to a constant, the same site potentials
    R = rng.normal(size=(n, n))
    mJ = np.linalg.inv(R @ R.T / n + 0.5 * np.eye(n))
    mJ = (mJ + mJ.T) / 2
    Pi = rng.dirichlet(np.ones(q), size=N)[:, :q - 1].ravel()
    g = bm.g_in_device_order(mJ, Pi)
    assert np.allclose(g, mJ @ Pi, rtol=1e-13, atol=1e-15)
    big = rng.normal(size=(150, 150))
    big = big + big.T
    assert np.allclose(bm.g_in_device_order(big, np.arange(150) / 150.0), big @ (np.arange(150) / 150.0), rtol=1e-12, atol=1e-12)
    Wg = bm.potts_from_gaussian(mJ, Pi, q)
    pg = sm.boltzmann(mJ, Pi, q, 1.0, bm.GAPS, np.ones(N, dtype=np.int8))[1]
    pw = sm.boltzmann(Wg, np.zeros(n), q, 1.0, bm.GAPS, np.ones(N, dtype=np.int8))[1]
    assert float(np.abs(pg - pw).max()) < 1e-14
    # the independent-site model has the marginals it was made of, and no correlations
    Wi = bm.potts_independent(Pi_d, N, q)
    P1, P2 = bm.potts_marginals(Wi, q, N)[:2]
    assert np.allclose(P1, Pi_d, atol=1e-14)
    a, b = bm._terms(P1, P2, P1, P2, N, q)
    assert np.abs(a).max() < 1e-15
    # the read-out: a model compared with itself, and its bound
    out, bound = bm.readout(Pi_d, Pij_d, Pi_d, Pij_d, N, q)
    assert out[0] == 0.0 and out[1] == 0.0 and abs(out[2] - 1.0) <= bound < 1e-10
    a, b = bm._terms(Pi_d, Pij_d, P1, Pij_d, N, q)
    want = float(np.corrcoef(a, b)[0, 1])
    out, bound = bm.readout(P1, Pij_d, Pi_d, Pij_d, N, q)
    assert abs(out[2] - want) < 1e-12 and np.isfinite(bound)
    assert np.array_equal(bm.update(W, Pij_d, P2, N, q, 0.3, 0.1), bm.update_scalar(W, Pij_d, P2, N, q, 0.3, 0.1))


def test_fit_is_the_composition_it_states():
    """bm_model.fit on small_problem's alignment against its steps taken one by one: the oracle's weights and add_pseudocount on
    tally_model's true tallies, numpy's inverse, then bm_model.learn from iteration 0 with burn = 10 N and stride = N"""
    from oracle import gdca_oracle as o

    N, q, K, M = 3, 4, 6, 40
    _, Z = small_family()
    Z[0, 0] = q
    wts, Meff, _, _ = o.compute_weights(np.ascontiguousarray(Z.T), 0.7)
    assert Meff < M  # (the weights are not all 1: a fit that dropped them would differ)
    Pi_t, Pij_t = tm.frequencies(Z, wts, Meff, q)
    for pc in (0.0, 0.1, 0.8):  # the pseudocount stated twice: the oracle's loop over the diagonal blocks, and the masks of bm_model
        Pi_o, Pij_o = o.add_pseudocount(Pi_t, Pij_t, pc, q)
        Pi_m, Pij_m = bm.add_pseudocount(Pi_t, Pij_t, pc, q)
        assert np.array_equal(Pi_m, Pi_o) and np.array_equal(Pij_m, Pij_o), pc
    kw = dict(eta=0.7, lam=0.05, n_samples=2, beta=0.9, seed=5)
    out = {}
    for init, tpc in (("gaussian", 0.0), ("gaussian", 0.1), ("independent", 0.1)):
        f = out[init, tpc] = bm.fit(Z, q, 3, wts, Meff, K, pseudocount=0.8, target_pseudocount=tpc, init=init, **kw)
        Pi_d, Pij_d = o.add_pseudocount(Pi_t, Pij_t, tpc, q)
        Pi, Pij = o.add_pseudocount(Pi_t, Pij_t, 0.8, q)
        assert np.array_equal(f["Pi_d"], Pi_d) and np.array_equal(f["Pij_d"], Pij_d) and np.array_equal(f["Pi"], Pi)
        W0 = bm.potts_from_gaussian(np.linalg.inv(o.compute_C(Pi, Pij)), Pi, q) if init == "gaussian" else bm.potts_independent(Pi, N, q)
        assert np.array_equal(f["W0"], W0)
        W, X, trace = bm.learn(W0, Pi_d, Pij_d, np.asfortranarray(Z[:, :K]), q, 3, burn=10 * N, stride=N, **kw)
        assert np.array_equal(f["W"], W) and np.array_equal(f["X"], X) and np.array_equal(f["trace"], trace)
        assert len(f["Ws"]) == 3 and np.array_equal(f["Ws"][-1], W) and not np.array_equal(f["Ws"][0], f["Ws"][1])
        # a shorter fit is a prefix, and the hooks are where the defaults come from
        two = bm.fit(Z, q, 2, wts, Meff, K, pseudocount=0.8, target_pseudocount=tpc, init=init, **kw)
        assert np.array_equal(two["trace"], trace[:2]) and np.array_equal(two["W"], f["Ws"][1])
    n_steps = 10 * N + 2 * N
    hooked = bm.fit(Z, q, 3, wts, Meff, K, pseudocount=0.8, target_pseudocount=0.1, init="gaussian", inverse=np.linalg.inv,
                    thresholds=lambda t: np.stack([-np.log(sm.uniforms(5, t * K + k, n_steps)[1]) for k in range(K)]),
                    tables=lambda W, X: mm.potentials_dense(bm.library_symmetric(W), np.zeros(N * (q - 1)), X, q), **kw)
    assert np.array_equal(hooked["W"], out["gaussian", 0.1]["W"]) and np.array_equal(hooked["trace"], out["gaussian", 0.1]["trace"])
    # what must matter does: the target's pseudocount, the start, and which K sequences the chains start from
    assert not np.array_equal(out["gaussian", 0.0]["W"], out["gaussian", 0.1]["W"])
    assert np.array_equal(out["gaussian", 0.0]["W0"], out["gaussian", 0.1]["W0"])
    assert not np.array_equal(out["independent", 0.1]["W"], out["gaussian", 0.1]["W"])
    assert np.all(out["independent", 0.1]["W0"][~np.eye(N * (q - 1), dtype=bool)] == 0.0)
    assert not np.array_equal(bm.fit(Z, q, 3, wts, Meff, K - 1, target_pseudocount=0.1, **kw)["W"], out["gaussian", 0.1]["W"])


# ---- 2. the sign of the gradient ----------------------------------------------------------------------------------------------------------------
def test_one_exact_step_lowers_the_exact_kl_divergence():
    N, q, P1, P2, W0, _, start = learn_problem()
    assert abs(start - START_DEVIATION) < 5e-5
    mJ, Pi = sm.toy_model(N=N, q=q, ratio=1e6)
    p_target = bm.exact_marginals(mJ, Pi, q, N)[3]
    W, kls = W0, []
    for _ in range(3):
        Pm1, Pm2, _, p_model = bm.potts_marginals(W, q, N)
        kls.append(bm.kl(p_target, p_model))
        W = bm.update(W, P2, Pm2, N, q, 1.0)
    print("KL(target || model) over three exact steps:", kls)
    assert kls[0] > kls[1] > kls[2] > 0
    # the other sign raises it
    Pm2 = bm.potts_marginals(W0, q, N)[1]
    assert bm.kl(p_target, bm.potts_marginals(bm.update(W0, Pm2, P2, N, q, 1.0), q, N)[3]) > kls[0]


# ---- 3. learning in pure numpy, and its control -------------------------------------------------------------------------------------------------
def test_numpy_learning_meets_the_bar_and_the_start_does_not():
    N, q, P1, P2, W0, X0, start = learn_problem()
    L = LEARN
    W, X, trace = bm.learn(W0, P1, P2, X0, q, L["n_iter"], seed=L["seed"], burn=L["burn"], stride=L["stride"], n_samples=L["n_samples"],
                           eta=L["eta"])
    dev = bm.pair_deviation(W, P2, q, N)
    print("exact pair deviation: start %.4f, learned %.5f, bar %.5f" % (start, dev, LEARN_BAR))
    assert abs(dev - LEARN_MEASURED[0]) < 1e-5  # the recorded measurement of seed 0 is this run
    assert dev < LEARN_BAR / 2 and max(LEARN_MEASURED) * 2 <= LEARN_BAR + 1e-12
    assert not start < LEARN_BAR
    assert trace[-50:, 1].mean() < trace[:10, 1].mean()


# ---- 4. exports, bindings, argument checks ---------------------------------------------------------------------------------------------------------
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
    assert len(protos["gdca_bm_learn_dev"][1]) == 21 and len(protos["gdca_bm_update_dev"][1]) == 10 and len(protos["gdca_bm_readout"][1]) == 8
    assert protos["gdca_bm_learn"][1][11:13] == ["uint64_t", "uint64_t"] and _lib.SYMBOLS["gdca_bm_learn"][1][11:13] == [ctypes.c_uint64] * 2
    assert protos["gdca_bm_learn"][1][17:19] == ["double", "double"] and _lib.SYMBOLS["gdca_bm_learn_dev"][1][17:19] == [ctypes.c_double] * 2
    lib = g.load()
    assert lib.gdca_version() == 6 and lib.gdca_stats_bytes() == ctypes.sizeof(_lib.Stats) and lib.gdca_params_bytes() == ctypes.sizeof(_lib.Params)
    hdr = open(os.path.join(ROOT, "include", "gdca.h")).read()
    assert "Boltzmann-machine refinement" in hdr and "THE CONTAINER" in hdr and "W[r, r] = -2 h[r]" in hdr
    for f in ("potts_from_gaussian_dev", "bm_update_dev", "bm_readout_dev", "bm_learn_dev"):
        assert callable(getattr(devops, f)) and hasattr(g.Context, f), f
    assert callable(g.gDCA_bm) and callable(g.bm_learn) and callable(g.potts_from_gaussian)
    assert "one sweep is n proposals" in g.gDCA_bm.__doc__.lower()
    Pi = np.array([0.2, 0.3, 0.1, 0.6])
    assert np.array_equal(g.potts_independent(Pi, 2, 3), bm.potts_independent(Pi, 2, 3))

    fasta = os.path.join(refdata, "small.fasta.gz")
    missing = str(tmp_path / "missing.fasta")
    with pytest.raises(g.ArgumentError, match="cannot open file"):
        g.gDCA_bm(missing, 3)
    with pytest.raises(g.ArgumentError, match="invalid pseudocount"):
        g.gDCA_bm(fasta, 3, pseudocount=1.5)
    with pytest.raises(g.ArgumentError, match="target_pseudocount"):
        g.gDCA_bm(fasta, 3, target_pseudocount=-0.1)
    with pytest.raises(g.ArgumentError, match="init"):
        g.gDCA_bm(fasta, 3, init="random")
    for bad in (0, -1, 2.5):
        with pytest.raises(g.ArgumentError, match="n_iter"):
            g.gDCA_bm(fasta, bad)
    with pytest.raises(g.ArgumentError, match="K"):
        g.gDCA_bm(fasta, 3, K=0)
    with pytest.raises(TypeError):
        g.gDCA_bm(fasta, 3, score=":DI")
    N, q, W, Pi_d, Pij_d, X = small_problem()
    with pytest.raises(g.ArgumentError, match="incompatible sizes"):
        g.bm_learn(W[:-1, :-1], Pi_d, Pij_d, X, 2, q)
    with pytest.raises(g.ArgumentError, match="no sequence"):
        g.bm_learn(W, Pi_d, Pij_d, X[:, :0], 2, q)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(g.ArgumentError, match="eta"):
            g.bm_learn(W, Pi_d, Pij_d, X, 2, q, eta=bad)
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(g.ArgumentError, match="lam"):
            g.bm_learn(W, Pi_d, Pij_d, X, 2, q, lam=bad)
    with pytest.raises(g.ArgumentError, match="n_iter"):
        g.bm_learn(W, Pi_d, Pij_d, X, 0, q)
    with pytest.raises(g.ArgumentError, match="stride"):
        g.bm_learn(W, Pi_d, Pij_d, X, 2, q, stride=0)
    with pytest.raises(g.ArgumentError, match="incompatible sizes"):
        g.potts_from_gaussian(np.eye(6), np.full(5, 0.1), 3)
    if lib.gdca_device_count() <= 0:
        # valid arguments, no device: an error, never a CPU computation
        with pytest.raises(g.GdcaError):
            g.bm_learn(W, Pi_d, Pij_d, X, 2, q)
        with pytest.raises(g.GdcaError):
            g.potts_from_gaussian(np.eye(6), np.full(6, 0.1), 3)


# ---- 5. the compiler's report on k_bm.hip -----------------------------------------------------------------------------------------------------------
def test_bm_kernels_do_not_spill(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    report = compiler_report(tmp_path, "k_bm.hip", kernels=("k_bm_updateILi2E", "k_bm_updateILi1E", "k_bm_from_gaussian", "k_bm_read_cols",
                                                            "k_bm_read_fin", "k_bm_accept", "k_bm_last_sample", "k_bm_fill"))
    assert len(report) == 8
    code = "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, "k_bm.hip")).read().split("\n"))
    assert "atomic" not in code
    # no contraction where the header fixes every operation: the entrywise kernels and the read-out's column pass hold no fused
    # multiply-add (the division and the square roots of the two final kernels are the compiler's own sequences)
    out = tmp_path / "k_bm.s"
    r = subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", os.path.join(CSRC, "k_bm.hip"), "-o", str(out)], capture_output=True,
                       text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = out.read_text()
    for name in ("_Z11k_bm_updateILi2EEv16k_bm_update_args", "_Z11k_bm_updateILi1EEv16k_bm_update_args", "_Z18k_bm_from_gaussianPKdS0_iiPd",
                 "_Z14k_bm_read_colsPKdS0_S0_S0_iiPd"):
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), asm, re.S | re.M)
        assert body, name
        text = body.group(1)
        assert "v_add_f64" in text and ("v_mul_f64" in text or "from_gaussian" in name) and not re.search(r"v_(fma|fmac|mad)\w*_f64", text), name
