"""Energies of sequences under the fitted Gaussian model, the part that needs no GPU: the rule itself (tests/energy_model.py states
it twice; the two statements are pinned against each other on models built by the oracle chain from both golden alignments), the
exported surface, the order of the argument checks, and the compiler's report on k_energy.hip."""
import os
import re
import shutil

import numpy as np
import pytest

import energy_model as em
from gdca_testutil import HIPCC, ROOT, compiler_report

NEW_SYMBOLS = ["gdca_energies_dev", "gdca_energies", "gdca_run_energies_dev", "gdca_run_energies"]


@pytest.mark.parametrize("name", ["small.fasta.gz", "large.fasta.gz"])
@pytest.mark.parametrize("pc", [0.8, 0.2])
def test_the_two_statements_of_the_rule_agree(refdata, name, pc):
    from oracle import gdca_oracle as o

    Zo = o.read_fasta_alignment(os.path.join(refdata, name), 0.9)
    q = int(Zo.max())
    mJ, Pi = em.model_from_Z(Zo, q, pc)
    N = Zo.shape[1]
    rng = np.random.default_rng(2)
    X = np.concatenate([Zo[:24].T, rng.integers(1, q + 1, size=(N, 8)).astype(np.int8), np.full((N, 1), q, dtype=np.int8)], axis=1)
    assert (X == q).any()  # gaps included
    E_dense = em.energies_dense(mJ, Pi, X, q)
    E, B, c0 = em.energies_gather(mJ, Pi, X, q)
    rel = np.abs(E_dense - E) / np.abs(E)
    print("%s pc %g: dense vs gather max rel %.3g; bound / |E| %.3g .. %.3g" %
          (name, pc, rel.max(), (em.order_bound(N, q, B) / np.abs(E)).min(), (em.order_bound(N, q, B) / np.abs(E)).max()))
    # the dense form sums the n^2 products d_i mJ_ij d_j in f64 (two nested n-term sums, each term two roundings from the products and
    # from d = x - Pi): to first order at most (2 n + 3) u times the sum of their absolute values, the factor 2 for the higher orders
    d = np.abs(em.one_hot(X, q) - Pi[None, :])
    B_dense = 0.5 * np.einsum("ki,ki->k", d @ np.abs(mJ), d)
    n = N * (q - 1)
    assert np.all(np.abs(E_dense - E) <= 2 * (2 * n + 3) * em.U * B_dense)
    assert E[-1] == pytest.approx(c0 / 2, rel=1e-15)  # all gaps: x = 0
    assert np.all(B >= np.abs(E))
    # the family fits better than noise
    assert E[:24].mean() < E[24:32].min()


def test_anchor_values_of_the_small_golden(refdata):
    from oracle import gdca_oracle as o

    Zo = o.read_fasta_alignment(os.path.join(refdata, "small.fasta.gz"), 0.9)
    mJ, Pi = em.model_from_Z(Zo, 21, 0.8)
    E, _, _ = em.energies_gather(mJ, Pi, Zo.T, 21)
    assert 127.0 < E.min() < 127.5 and 198.0 < E.max() < 198.5


def test_symbols_are_declared_and_bound():
    import gaussdca.jl_amd as g

    header = open(os.path.join(ROOT, "include", "gdca.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"gdca_status %s\(gdca_ctx \*ctx" % s, header), s
        assert s in g._lib.SYMBOLS, s
    assert callable(g.sequence_energies) and callable(g.gDCA_energies)
    assert hasattr(g.Context, "run_energies_ptr")
    import gaussdca

    assert gaussdca.jl_amd.gDCA_energies is g.gDCA_energies or callable(gaussdca.jl_amd.gDCA_energies)
    if os.path.exists(g._lib.LIB_PATH):
        lib = g.load()
        for s in NEW_SYMBOLS:
            assert hasattr(lib, s)
        assert lib.gdca_version() == 6


def _no_gpu(g):
    return not os.path.exists(g._lib.LIB_PATH) or g.load().gdca_device_count() <= 0


def test_argument_errors_come_first_then_no_cpu_fallback(refdata, tmp_path):
    import gaussdca.jl_amd as g

    fasta = os.path.join(refdata, "small.fasta.gz")
    X = np.ones((53, 4), dtype=np.int8)
    # gDCA's checks, in gDCA's order
    with pytest.raises(g.ArgumentError, match="invalid pseudocount"):
        g.gDCA_energies(str(tmp_path / "missing.fasta"), X, pseudocount=1.5, theta=7)
    with pytest.raises(g.ArgumentError, match="invalid θ"):
        g.gDCA_energies(str(tmp_path / "missing.fasta"), X, theta=7, max_gap_fraction=2)
    with pytest.raises(g.ArgumentError, match="invalid max_gap_fraction"):
        g.gDCA_energies(str(tmp_path / "missing.fasta"), X, max_gap_fraction=2)
    with pytest.raises(g.ArgumentError, match="cannot open file"):
        g.gDCA_energies(str(tmp_path / "missing.fasta"), X)
    with pytest.raises(g.ArgumentError, match="cannot open file"):
        g.gDCA_energies(fasta, str(tmp_path / "missing_too.fasta"))
    with pytest.raises(TypeError):
        g.gDCA_energies(fasta, X, score=":DI")
    assert os.path.exists(g._lib.LIB_PATH), "libgdca.so not built (the FASTA reader is part of it)"
    with pytest.raises(g.ArgumentError, match="sites"):  # wrong N: needs no device either
        g.gDCA_energies(fasta, np.ones((52, 4), dtype=np.int8))
    mJ, Pi = np.eye(53 * 20), np.full(53 * 20, 0.05)
    with pytest.raises(g.ArgumentError, match="incompatible sizes"):
        g.sequence_energies(mJ, Pi, X[:-1], 21)
    with pytest.raises(g.ArgumentError, match="too big"):
        g.sequence_energies(mJ, Pi, X, 32)
    with pytest.raises(g.ArgumentError):
        g.sequence_energies(mJ, Pi, X[:, :0], 21)
    with pytest.raises(g.ArgumentError):
        g.sequence_energies(mJ, Pi, X[0], 21)
    if _no_gpu(g):
        # valid arguments, no device: an error, never a CPU computation
        with pytest.raises(g.GdcaError):
            g.sequence_energies(mJ, Pi, X, 21)
        with pytest.raises(g.GdcaError):
            g.gDCA_energies(fasta)
        with pytest.raises(g.GdcaError):
            g.gDCA_energies(fasta, X)


# ---- the compiler's report on k_energy.hip (tests/test_kernel_resources.py has a fixed list of files) -----------------------------------
def test_energy_kernels_do_not_spill(tmp_path):
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("no hipcc")
    compiler_report(tmp_path, "k_energy.hip", kernels=("k_energy_pack", "k_energy_gtile", "k_energy_gfin", "k_energy_c0", "k_energy_rowsILi20ELi8E",
                                                       "k_energy_rowsILi20ELi2E", "k_energy_rowsILi0ELi8E", "k_energy_rowsILi0ELi2E", "k_energy_final"))


def test_no_barrier_sits_inside_a_divergent_loop_of_the_energy_kernels(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    compiler_report(tmp_path, "k_energy.hip", min_loops=4)  # (the tile walk, the g pass, the reductions)
