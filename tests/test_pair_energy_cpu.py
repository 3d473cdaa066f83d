"""All-pairs partner energies across a split alignment, the part that needs no GPU: the identity
E(a (+) b) = E(a (+) gaps) + E(gaps (+) b) - c0 / 2 + R(a, b) (tests/pair_energy_model.py) against the energy of the explicit
concatenation on models built by the oracle chain from both golden alignments, the exported surface, the order of the argument
checks, the partner-matching check on the numpy model alone, and the compiler's report on k_pair_energy.hip."""
import os
import re

import numpy as np
import pytest

import energy_model as em
import pair_energy_model as pm
from gdca_testutil import HIPCC, ROOT, compiler_report

NEW_SYMBOLS = ["gdca_pair_energies_dev", "gdca_pair_energies", "gdca_run_pair_energies_dev", "gdca_run_pair_energies"]
SPLITS = {"small.fasta.gz": 26, "large.fasta.gz": 20}


@pytest.mark.parametrize("name", ["small.fasta.gz", "large.fasta.gz"])
@pytest.mark.parametrize("pc", [0.8, 0.2])
def test_the_composition_is_the_energy_of_the_concatenation(refdata, name, pc):
    from oracle import gdca_oracle as o

    Zo = o.read_fasta_alignment(os.path.join(refdata, name), 0.9)
    q = int(Zo.max())
    N, split = Zo.shape[1], SPLITS[name]
    mJ, Pi = em.model_from_Z(Zo, q, pc)
    rng = np.random.default_rng(4)
    XA, XB = pm.mixed_halves(rng, Zo, q, split, 6, 5)
    E, bound, c0, EA, EB = pm.pair_energy(mJ, Pi, XA, XB, q)
    cat = pm.concatenations(XA, XB)
    E_cat, B_cat, c0_cat = em.energies_gather(mJ, Pi, cat, q)
    E_cat = E_cat.reshape(5, 6).T  # column a + K_A b -> [a, b]
    err = np.abs(E - E_cat)
    print("%s pc %g: composition vs concatenation max rel %.3g, max err / bound %.3g" %
          (name, pc, float((err / np.abs(E_cat)).max()), float((err / bound).max())))
    assert c0 == c0_cat
    assert np.all(err <= bound)
    # the bound of the composition is that of the concatenation with |c0| added
    assert np.allclose(bound, em.order_bound(N, q, B_cat.reshape(5, 6).T + abs(c0)), rtol=1e-12)

    # the two statements of R: the longdouble double sum against the difference of the four longdouble energies
    R, BR = pm.coupling_gather(mJ, XA, XB, q)
    R_diff = E_cat - EA[:, None] - EB[None, :] + c0 / 2
    # each of the four f64-rounded terms carries u of itself
    slack = em.U * (np.abs(E_cat) + np.abs(EA)[:, None] + np.abs(EB)[None, :] + abs(c0)) * 4
    assert np.all(np.abs(R - R_diff) <= pm.coupling_bound(split, N - split, BR) + slack)
    assert np.all(BR >= np.abs(R))
    # an all-gap a or b: no cross term at all, and the energy is the other half's marginal
    ga, gb = np.all(XA == q, axis=0), np.all(XB == q, axis=0)
    assert ga.any() and gb.any()
    assert np.all(R[ga, :] == 0.0) and np.all(R[:, gb] == 0.0) and np.all(BR[ga, :] == 0.0) and np.all(BR[:, gb] == 0.0)
    assert np.all(np.abs(E[ga][:, ~gb] - EB[None, ~gb]) <= bound[ga][:, ~gb])
    assert np.all(np.abs(E[:, gb][~ga] - EA[~ga, None]) <= bound[:, gb][~ga])


def test_symbols_are_declared_and_bound():
    import gaussdca.jl_amd as g

    header = open(os.path.join(ROOT, "include", "gdca.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"gdca_status %s\(gdca_ctx \*ctx" % s, header), s
        assert s in g._lib.SYMBOLS, s
    assert re.search(r"enum \{ GDCA_PAIR_COUPLING = 0, GDCA_PAIR_ENERGY = 1 \};", header)
    assert (g._lib.PAIR_COUPLING, g._lib.PAIR_ENERGY) == (0, 1)
    assert callable(g.pair_energies) and callable(g.gDCA_pair_energies)
    assert hasattr(g.Context, "run_pair_energies_ptr") and hasattr(g.Context, "pair_energies_dev")
    assert os.path.exists(g._lib.LIB_PATH), "libgdca.so not built"
    lib = g.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)
    assert lib.gdca_version() == 6
    jl = open(os.path.join(ROOT, "julia", "src", "GaussDCAHip.jl")).read()
    assert "ccall((:gdca_pair_energies, libgdca)" in jl and re.search(r"export[^\n]*\n[^\n]*pair_energies", jl)


def _no_gpu(g):
    return not os.path.exists(g._lib.LIB_PATH) or g.load().gdca_device_count() <= 0


def test_argument_errors_come_first_then_no_cpu_fallback(refdata, tmp_path):
    import gaussdca.jl_amd as g

    fasta = os.path.join(refdata, "small.fasta.gz")  # N = 53
    missing = str(tmp_path / "missing.fasta")
    XA, XB = np.ones((26, 4), dtype=np.int8), np.ones((27, 3), dtype=np.int8)
    # gDCA's checks, in gDCA's order; then the split; then the widths
    with pytest.raises(g.ArgumentError, match="invalid pseudocount"):
        g.gDCA_pair_energies(missing, 0, XA[:-1], XB, pseudocount=1.5, theta=7, max_gap_fraction=2)
    with pytest.raises(g.ArgumentError, match="invalid θ"):
        g.gDCA_pair_energies(missing, 0, XA[:-1], XB, theta=7, max_gap_fraction=2)
    with pytest.raises(g.ArgumentError, match="invalid θ"):
        g.gDCA_pair_energies(missing, 0, XA[:-1], XB, θ=7)
    with pytest.raises(g.ArgumentError, match="invalid max_gap_fraction"):
        g.gDCA_pair_energies(missing, 0, XA[:-1], XB, max_gap_fraction=2)
    with pytest.raises(g.ArgumentError, match="cannot open file"):
        g.gDCA_pair_energies(missing, 0, XA[:-1], XB)
    with pytest.raises(g.ArgumentError, match="cannot open file"):
        g.gDCA_pair_energies(fasta, 26, missing, XB)
    with pytest.raises(TypeError):
        g.gDCA_pair_energies(fasta, 26, XA, XB, score=":DI")
    assert os.path.exists(g._lib.LIB_PATH), "libgdca.so not built (the FASTA reader is part of it)"
    for bad in (0, 53, -1, 54):
        with pytest.raises(g.ArgumentError, match="split"):
            g.gDCA_pair_energies(fasta, bad, XA[:-1], XB)  # (the widths are wrong too: the split is reported)
    with pytest.raises(g.ArgumentError, match="sites"):
        g.gDCA_pair_energies(fasta, 26, XA[:-1], XB)
    with pytest.raises(g.ArgumentError, match="sites"):
        g.gDCA_pair_energies(fasta, 26, XA, XB[:-1])
    with pytest.raises(g.ArgumentError, match="sites"):
        g.gDCA_pair_energies(fasta, 27, None, XB)
    with pytest.raises(g.ArgumentError, match="what"):
        g.gDCA_pair_energies(fasta, 26, XA, XB, what="both")
    with pytest.raises(g.ArgumentError):  # a wider integer type is not wrapped into a legal symbol (261 -> 5)
        g.gDCA_pair_energies(fasta, 26, XA.astype(np.int64) + 260, XB)
    # the operator-level wrapper
    mJ, Pi = np.eye(53 * 20), np.full(53 * 20, 0.05)
    with pytest.raises(g.ArgumentError, match="incompatible sizes"):
        g.pair_energies(mJ, Pi, XA[:-1], XB, 21)
    with pytest.raises(g.ArgumentError, match="incompatible sizes"):
        g.pair_energies(mJ, Pi[:-1], XA, XB, 21)
    with pytest.raises(g.ArgumentError, match="incompatible sizes"):
        g.pair_energies(mJ, Pi, XA, XB[:0], 21)
    with pytest.raises(g.ArgumentError, match="too big"):
        g.pair_energies(mJ, Pi, XA, XB, 32)
    with pytest.raises(g.ArgumentError, match="what"):
        g.pair_energies(mJ, Pi, XA, XB, 21, what="both")
    with pytest.raises(g.ArgumentError):
        g.pair_energies(mJ, Pi, XA[:, :0], XB, 21)
    with pytest.raises(g.ArgumentError):
        g.pair_energies(mJ, Pi, XA[0], XB, 21)
    with pytest.raises(g.ArgumentError):
        g.pair_energies(mJ, Pi, XA.astype(np.int64) + 260, XB, 21)
    with pytest.raises(g.ArgumentError):
        g.pair_energies(mJ, Pi, XA.astype(np.float64), XB, 21)
    if _no_gpu(g):
        # valid arguments, no device: an error, never a CPU computation
        with pytest.raises(g.GdcaError):
            g.pair_energies(mJ, Pi, XA, XB, 21)
        with pytest.raises(g.GdcaError):
            g.pair_energies(mJ, None, XA, XB, 21, what="coupling")
        with pytest.raises(g.GdcaError):
            g.gDCA_pair_energies(fasta, 26)
        with pytest.raises(g.GdcaError):
            g.gDCA_pair_energies(fasta, 26, XA, XB)


def test_partner_matching_on_the_numpy_model():
    """The paired family of the GPU test's `meaning` check, with the numpy model alone: the row-wise argmin of the energy matrix of
    64 held-out native pairs finds the native partner more often than a uniform guess (1 / 64)."""
    Zfit, Zheld = pm.paired_family(30, 1000, 64)
    mJ, Pi = em.model_from_Z(Zfit, 21, 0.5)
    XA, XB = np.asfortranarray(Zheld[:, :30].T), np.asfortranarray(Zheld[:, 30:].T)
    E = pm.pair_energy(mJ, Pi, XA, XB, 21)[0]
    rate = float((E.argmin(axis=1) == np.arange(64)).mean())
    print("native partner recovered in %.3f of 64 rows (uniform guess: %.3f)" % (rate, 1 / 64))
    assert rate > 1 / 64


# ---- the compiler's report on k_pair_energy.hip (tests/test_kernel_resources.py has a fixed list of files) -----------------------------
def test_pair_energy_kernels_do_not_spill(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    # (the halves are packed by k_energy_pack: tests/test_energy_cpu.py)
    compiler_report(tmp_path, "k_pair_energy.hip", kernels=("k_pair_pad", "k_pair_foldILi32E", "k_pair_foldILi4E", "k_pair_gatherILi2E", "k_pair_gatherILi1E"))


def test_no_barrier_sits_inside_a_divergent_loop_of_the_pair_energy_kernels(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    compiler_report(tmp_path, "k_pair_energy.hip", min_loops=4)  # (the tile walks and the segment walks of both instances)
