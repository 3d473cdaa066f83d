"""The mutation scan, the part that needs no GPU: the formula dE(x; i, b) = V(x; i, b) - V(x; i, x_i) (tests/mutation_model.py) against
the energies of the explicit mutants for EVERY (k, i, b) of a handful of sequences, the gap conventions, the exported surface and its
argument checks, the sanity property of the GPU test on the numpy model alone, and the compiler's report on k_mutation.hip."""
import os
import re

import numpy as np
import pytest

import energy_model as em
import mutation_model as mm
from gdca_testutil import CSRC, HIPCC, ROOT, compiler_report, mixed_sequences

NEW_SYMBOLS = ["gdca_mutation_scan_dev", "gdca_mutation_scan", "gdca_run_mutation_scan_dev", "gdca_run_mutation_scan"]


def seeded_model(q, N, M, seed):
    from gdca_testutil import random_msa

    Zo = random_msa(np.random.default_rng(seed), M, N, q)
    return (Zo,) + mm.model_from_Z(Zo, q, 0.5)


def handful(Zo, q, seed):
    """(N, 6): two members of the family (one of them with gaps), an all-gap sequence, one without gaps, one uniformly random (gaps
    included), one more member"""
    rng = np.random.default_rng(seed)
    X = mixed_sequences(rng, Zo, q, 5, shift=3)  # member, all gaps, no gaps, random, member
    gappy = Zo[np.argmax((Zo == q).sum(axis=1))]
    return np.asfortranarray(np.concatenate([X, gappy[:, None]], axis=1))


# ---- 1. the model against itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,N,M", [(21, 37, 300), (5, 30, 400)])
def test_delta_is_the_energy_of_the_mutant_minus_that_of_the_wild_type(q, N, M):
    Zo, mJ, Pi = seeded_model(q, N, M, 100 * q + N)
    X = handful(Zo, q, q)
    K = X.shape[1]
    assert np.all(X[:, 1] == q) and (X[:, 5] == q).any() and not (X[:, 2] == q).any()
    V, B, Vl = mm.potentials_exact(mJ, Pi, X, q)
    dE = mm.delta_exact(Vl, X, q)
    tol_d = mm.delta_bound(N, q, B, X, dE)
    mJl, Pil = mJ.astype(np.longdouble), Pi.astype(np.longdouble)
    E_wt = em.energies_dense(mJl, Pil, X, q)
    assert E_wt.dtype == np.longdouble
    _, B_wt, _ = em.energies_gather(mJ, Pi, X, q)
    worst = 0.0
    for k in range(K):
        Xm = mm.single_mutants(X[:, k], q)
        E_mut = em.energies_dense(mJl, Pil, Xm, q)                       # longdouble
        _, B_mut, _ = em.energies_gather(mJ, Pi, Xm, q)
        ref = (E_mut - E_wt[k]).reshape(N, q)
        tol = em.order_bound(N, q, B_mut).reshape(N, q) + em.order_bound(N, q, B_wt[k]) + tol_d[k]
        err = np.abs(dE[k].astype(np.longdouble) - ref).astype(np.float64)
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), (k, float((err / tol).max()))
    print("q %d N %d: max |dE - (E_mut - E_wt)| / tolerance = %.3g" % (q, N, worst))
    # the f64 matrix form agrees with the longdouble sums within the potentials' own bound
    assert np.all(np.abs(mm.potentials_dense(mJ, Pi, X, q) - V) <= mm.bound_V(N, q, B))


# ---- 2. gap conventions ---------------------------------------------------------------------------------------------------------------------
def test_gap_conventions():
    q, N = 5, 30
    Zo, mJ, Pi = seeded_model(q, N, 400, 7)
    X = handful(Zo, q, 3)
    V, B, Vl = mm.potentials_exact(mJ, Pi, X, q)
    dE = mm.delta_exact(Vl, X, q)
    assert np.all(V[:, :, q - 1] == 0.0) and not np.signbit(V[:, :, q - 1]).any() and np.all(B[:, :, q - 1] == 0.0)
    gap = (X.T == q)                                           # (K, N)
    assert gap.any() and np.array_equal(dE[gap], V[gap])       # from a gap site: dE(b) = V(b)
    own = mm.wild_type(dE, X, q)
    assert np.all(own == 0.0) and not np.signbit(own).any()    # b = x_i: exactly +0.0
    # deleting a residue: dE(q) = -V(x_i)
    assert np.array_equal(dE[:, :, q - 1][~gap], -mm.wild_type(V, X, q)[:, :, 0][~gap])
    # an all-gap sequence: no coupling term at all
    g = mJ @ Pi
    assert np.allclose(V[1, :, :q - 1].ravel(), 0.5 * np.diagonal(mJ) - g, rtol=1e-13, atol=0)


# ---- 3. the binding surface -------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_bound():
    import gaussdca.jl_amd as g

    header = open(os.path.join(ROOT, "include", "gdca.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"gdca_status %s\(gdca_ctx \*ctx" % s, header), s
        assert s in g._lib.SYMBOLS, s
    assert re.search(r"enum \{ GDCA_MUT_DELTA = 0, GDCA_MUT_POTENTIAL = 1 \};", header)
    assert (g._lib.MUT_DELTA, g._lib.MUT_POTENTIAL) == (0, 1)
    assert callable(g.mutation_scan) and callable(g.gDCA_mutation_scan)
    from gaussdca.jl_amd import devops

    assert callable(devops.mutation_scan_dev)
    assert hasattr(g.Context, "run_mutation_scan_ptr") and hasattr(g.Context, "mutation_scan_dev")
    assert os.path.exists(g._lib.LIB_PATH), "libgdca.so not built"
    lib = g.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)
    assert lib.gdca_version() == 6
    jl = open(os.path.join(ROOT, "julia", "src", "GaussDCAHip.jl")).read()
    assert "ccall((:gdca_mutation_scan, libgdca)" in jl and "ccall((:gdca_run_mutation_scan, libgdca)" in jl
    assert re.search(r"export[^\n]*\n[^\n]*mutation_scan, gDCA_mutation_scan", jl)


def _no_gpu(g):
    return not os.path.exists(g._lib.LIB_PATH) or g.load().gdca_device_count() <= 0


def test_argument_errors_come_first_then_no_cpu_fallback(refdata, tmp_path):
    import gaussdca.jl_amd as g

    fasta = os.path.join(refdata, "small.fasta.gz")  # N = 53
    missing = str(tmp_path / "missing.fasta")
    X = np.ones((53, 4), dtype=np.int8)
    # gDCA's checks, in gDCA's order; then `what`; then the sequences
    with pytest.raises(g.ArgumentError, match="invalid pseudocount"):
        g.gDCA_mutation_scan(missing, X[:-1], pseudocount=1.5, theta=7, max_gap_fraction=2)
    with pytest.raises(g.ArgumentError, match="invalid θ"):
        g.gDCA_mutation_scan(missing, X[:-1], theta=7, max_gap_fraction=2)
    with pytest.raises(g.ArgumentError, match="invalid θ"):
        g.gDCA_mutation_scan(missing, X[:-1], θ=7)
    with pytest.raises(g.ArgumentError, match="invalid max_gap_fraction"):
        g.gDCA_mutation_scan(missing, X[:-1], max_gap_fraction=2)
    with pytest.raises(g.ArgumentError, match="cannot open file"):
        g.gDCA_mutation_scan(missing, X[:-1])
    with pytest.raises(g.ArgumentError, match="cannot open file"):
        g.gDCA_mutation_scan(fasta, missing)
    with pytest.raises(TypeError):
        g.gDCA_mutation_scan(fasta, X, score=":DI")
    with pytest.raises(g.ArgumentError, match="what"):
        g.gDCA_mutation_scan(fasta, X, what="both")
    with pytest.raises(g.ArgumentError, match="N x K"):
        g.gDCA_mutation_scan(fasta, X[0])
    with pytest.raises(g.ArgumentError, match="integer symbols"):  # a wider integer type is not wrapped into a legal symbol (261 -> 5)
        g.gDCA_mutation_scan(fasta, X.astype(np.int64) + 260)
    with pytest.raises(g.ArgumentError, match="integer symbols"):
        g.gDCA_mutation_scan(fasta, X.astype(np.float64))
    assert os.path.exists(g._lib.LIB_PATH), "libgdca.so not built (the FASTA reader is part of it)"
    with pytest.raises(g.ArgumentError, match="sites"):
        g.gDCA_mutation_scan(fasta, X[:-1])
    with pytest.raises(g.ArgumentError, match="no sequence"):
        g.gDCA_mutation_scan(fasta, X[:, :0])
    # the operator-level wrapper
    mJ, Pi = np.eye(53 * 20), np.full(53 * 20, 0.05)
    with pytest.raises(g.ArgumentError, match="incompatible sizes"):
        g.mutation_scan(mJ, Pi, X[:-1], 21)
    with pytest.raises(g.ArgumentError, match="incompatible sizes"):
        g.mutation_scan(mJ, Pi[:-1], X, 21)
    with pytest.raises(g.ArgumentError, match="too big"):
        g.mutation_scan(mJ, Pi, X, 32)
    with pytest.raises(g.ArgumentError, match="what"):
        g.mutation_scan(mJ, Pi, X, 21, what="energy")
    with pytest.raises(g.ArgumentError, match="no sequence"):
        g.mutation_scan(mJ, Pi, X[:, :0], 21)
    with pytest.raises(g.ArgumentError):
        g.mutation_scan(mJ, Pi, X[0], 21)
    with pytest.raises(g.ArgumentError):
        g.mutation_scan(mJ, Pi, X.astype(np.int64) + 260, 21)
    with pytest.raises(g.ArgumentError):
        g.mutation_scan(mJ, Pi, X.astype(np.float64), 21)
    if _no_gpu(g):
        # valid arguments, no device: an error, never a CPU computation
        with pytest.raises(g.GdcaError):
            g.mutation_scan(mJ, Pi, X, 21)
        with pytest.raises(g.GdcaError):
            g.mutation_scan(mJ, Pi, X, 21, what="potential")
        with pytest.raises(g.GdcaError):
            g.gDCA_mutation_scan(fasta)
        with pytest.raises(g.GdcaError):
            g.gDCA_mutation_scan(fasta, X, what=":potential")


# ---- the sanity property of the GPU test, on the numpy model alone -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small.fasta.gz", "large.fasta.gz"])
def test_native_residues_sit_in_minima_on_the_numpy_model(refdata, name):
    from oracle import gdca_oracle as o

    Zo = o.read_fasta_alignment(os.path.join(refdata, name), 0.9)
    q = int(Zo.max())
    mJ, Pi = mm.model_from_Z(Zo, q, 0.8)
    rng = np.random.default_rng(1)
    Xf = np.asfortranarray(Zo[:32].T)
    Xr = np.asfortranarray(rng.integers(1, q + 1, size=(Zo.shape[1], 32)).astype(np.int8))
    med = []
    for X in (Xf, Xr):
        V = mm.potentials_dense(mJ, Pi, X, q)
        med.append(float(np.median(V - mm.wild_type(V, X, q))))
    print("%s: median dE over all substitutions: family %.4g, random %.4g" % (name, med[0], med[1]))
    assert med[0] > med[1]


# ---- 4. the compiler's report on k_mutation.hip ---------------------------------------------------------------------------------------------
def test_mutation_kernels_do_not_spill_and_two_workgroups_share_a_compute_unit(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    report = compiler_report(tmp_path, "k_mutation.hip",
                             kernels=("k_mut_rowsILi20ELi32E", "k_mut_rowsILi20ELi4E", "k_mut_rowsILi0ELi32E", "k_mut_rowsILi0ELi4E"))
    text = open(os.path.join(CSRC, "k_mutation.hip")).read()
    MT, MLD = (int(re.search(r"#define %s (\d+)" % d, text).group(1)) for d in ("MT", "MLD"))
    for name, field in report:
        occ = field(r"Occupancy \[waves/SIMD\]")
        print("%-50s %d waves / SIMD" % (name, occ))
        if "ILi20E" in name:
            # two workgroups of four waves on a compute unit's four SIMDs = two waves a SIMD, and twice the tile within the 160 KB of LDS
            assert occ >= 2, (name, occ)
            assert field(r"LDS Size \[bytes/block\]") == 0  # (the tile is the launch's dynamic LDS: MT (s + 1) columns of MLD doubles)
            assert 2 * MT * 21 * MLD * 8 <= 160 * 1024
    # the generic form's largest tile (s = 30) too
    assert 2 * MT * 31 * MLD * 8 <= 160 * 1024
