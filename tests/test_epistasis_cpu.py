"""The double-mutant scan, the part that needs no GPU: the identity ddE = dE(i,b) + dE(j,c) + eps (tests/epistasis_model.py) against
the energies of the explicit double mutants in longdouble, the zeros of eps, the transposed-code convention, the exported surface and
its argument checks, and the compiler's report on k_epistasis.hip."""
import os
import re

import numpy as np
import pytest

import energy_model as em
import epistasis_model as ep
import mutation_model as mm
from gdca_testutil import CSRC, HIPCC, ROOT, compiler_report, random_msa

NEW_SYMBOLS = ["gdca_double_mutant_scan_dev", "gdca_double_mutant_scan", "gdca_double_mutants_dev", "gdca_double_mutants",
               "gdca_run_double_mutant_scan_dev", "gdca_run_double_mutant_scan", "gdca_run_double_mutants_dev", "gdca_run_double_mutants"]


def assert_identity(mJ, Pi, x, q, pairs, tag):
    """ddE of the model against E(double mutant) - E(x), both in longdouble, for all q^2 targets of the pairs.  The tolerance is
    longdouble's own: the energies are sums of about (N + 1)^2 + n terms of magnitude sum |term| =: T each, the model's side of
    O(N) terms; 4 (N^2 + n + 8 N) 2^-64 T covers any order of both (u_ld = 2^-64)."""
    N = len(x)
    ddE, eps, dE, bD = ep.ddE_exact(mJ, Pi, x, q)
    assert ddE.dtype == np.longdouble
    mJl, Pil = mJ.astype(np.longdouble), Pi.astype(np.longdouble)
    E_wt = em.energies_dense(mJl, Pil, np.asarray(x)[:, None], q)[0]
    _, B_wt, _ = em.energies_gather(mJ, Pi, np.asarray(x)[:, None], q)
    worst, scale = 0.0, 0.0
    for (i, j) in pairs:
        Xm = ep.explicit_double_mutants(x, i, j, q)
        E_mut = em.energies_dense(mJl, Pil, Xm, q)
        assert E_mut.dtype == np.longdouble
        _, B_mut, _ = em.energies_gather(mJ, Pi, Xm, q)
        ref = E_mut - E_wt
        tol = 4.0 * (N * N + N * (q - 1) + 8 * N) * 2.0 ** -64 * (B_mut + B_wt[0])
        err = np.abs(ep.by_code(ddE, i, j) - ref).astype(np.float64)
        worst = max(worst, float((err / tol).max()))
        scale = max(scale, float(np.abs(E_wt)))
        assert np.all(err <= tol), (tag, i, j, float((err / tol).max()))
        # the same pair named the other way round is the same number
        assert np.array_equal(ddE[j, :, i, :], ddE[i, :, j, :].T)
    print("%s: max |ddE - (E_mut - E_wt)| / longdouble tolerance = %.3g at |E| = %.3g" % (tag, worst, scale))


def test_identity_all_pairs_of_a_small_sequence_with_gaps():
    q, N = 5, 6
    Zo = random_msa(np.random.default_rng(56), 300, N, q)
    mJ, Pi = mm.model_from_Z(Zo, q, 0.5)
    x = np.array([1, q, 3, 4, q, 2], dtype=np.int8)
    assert_identity(mJ, Pi, x, q, [(i, j) for i in range(N) for j in range(i + 1, N)], "q 5 N 6")
    assert_identity(mJ, Pi, np.full(N, q, dtype=np.int8), q, [(0, 1), (2, 5)], "q 5 N 6 all gaps")


def test_identity_three_pairs_of_a_golden_sequence(refdata):
    from oracle import gdca_oracle as o

    Zo = o.read_fasta_alignment(os.path.join(refdata, "small.fasta.gz"), 0.9)
    q = int(Zo.max())
    assert (Zo.shape[1], q) == (53, 21)
    mJ, Pi = mm.model_from_Z(Zo, q, 0.8)
    x = Zo[np.argmax((Zo == q).sum(axis=1) > 0)]
    assert (x == q).any()
    gap_site = int(np.nonzero(x == q)[0][0])
    other = 0 if gap_site != 0 else 1
    pairs = [(0, 1) if gap_site > 1 else (2, 3), (min(gap_site, other), max(gap_site, other)), (17, 52)]
    assert_identity(mJ, Pi, x, q, pairs, "small.fasta.gz")


@pytest.mark.parametrize("q,N", [(5, 6), (21, 4), (2, 2)])
def test_eps_is_exactly_zero_at_the_wild_type_symbols(q, N):
    """b == x_i or c == x_j: the fixed f64 grouping cancels exactly, so ddE_fixed is the single change of the other site bit for bit"""
    rng = np.random.default_rng(q + N)
    Zo = random_msa(rng, 300, N, q)
    mJ, Pi = mm.model_from_Z(Zo, q, 0.5)
    for x in (rng.integers(1, q + 1, size=N).astype(np.int8), np.full(N, q, dtype=np.int8), Zo[0]):
        e = ep.eps_fixed(mJ, x, q)
        a = x.astype(np.int64) - 1
        ii = np.arange(N)
        assert np.all(e[ii, a] == 0.0) and np.all(e[:, :, ii, a] == 0.0)
        V, B, Vl = mm.potentials_exact(mJ, Pi, x[:, None], q)
        dE = mm.delta_exact(Vl, x[:, None], q)[0]
        d = ep.ddE_fixed(mJ, dE, x, q)
        for i in range(N):
            for j in range(N):
                if i != j:
                    assert np.array_equal(d[i, a[i], j, :], dE[j])       # b = x_i: dE[j, c]
                    assert np.array_equal(d[i, :, j, a[j]], dE[i])       # c = x_j: dE[i, b]
                    assert d[i, a[i], j, a[j]] == 0.0
        # ... and within its bound of the exact value everywhere
        ddE, eps, dE2, bD = ep.ddE_exact(mJ, Pi, x, q, pot=(V, B, Vl))
        assert np.array_equal(dE, dE2)
        off = ~np.eye(N, dtype=bool)[:, None, :, None].repeat(q, 1).repeat(q, 3)
        assert np.all(np.abs(d - ddE)[off] <= ep.ddE_bound(mJ, x, q, bD, ddE)[off])
        epi = ep.epi_exact(eps)
        epi_f = np.sqrt((e * e).sum(axis=(1, 3)))
        assert np.all(np.abs(epi_f - epi) <= ep.epi_bound(mJ, x, q, epi))


def test_transposed_code_convention():
    q = 5
    code = np.array([-1, 0, 3, 7, 24, 5 * 2 + 4])
    t = ep.transpose_code(code, q)
    assert t.tolist() == [-1, 0, 15, 11, 24, 4 * 5 + 2]
    assert np.array_equal(ep.transpose_code(t, q), code)
    from gaussdca.jl_amd.dcautils import decode_double_code

    b, c = decode_double_code(code, q)
    assert b.tolist() == [0, 1, 4, 3, 5, 5] and c.tolist() == [0, 1, 1, 2, 5, 3] and b.dtype == c.dtype == np.int8
    bt, ct = decode_double_code(t, q)
    assert np.array_equal(bt, c) and np.array_equal(ct, b)
    # the explicit mutants are laid out by the same code
    x = np.array([1, 2, 3], dtype=np.int8)
    Xm = ep.explicit_double_mutants(x, 0, 2, q)
    assert Xm.shape == (3, 25) and Xm[:, 7].tolist() == [3, 2, 2] and Xm[:, 15].tolist() == [1, 2, 4]
    rec, pairs = ep.all_records(np.asfortranarray(np.stack([x, x], axis=1)), q)
    assert rec.shape == (2 * 3 * 25, 5) and pairs == [(0, 1), (0, 2), (1, 2)]
    assert rec[25 + 7].tolist() == [0, 0, 3, 2, 2] and rec[75 + 50 + 15].tolist() == [1, 1, 1, 2, 4]


def test_symbols_are_declared_and_bound():
    import gaussdca.jl_amd as g
    from gaussdca.jl_amd import devops

    header = open(os.path.join(ROOT, "include", "gdca.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"gdca_status %s\(gdca_ctx \*ctx" % s, header), s
        assert s in g._lib.SYMBOLS, s
    for name in ("double_mutant_scan", "double_mutant_energies", "gDCA_double_mutant_scan", "gDCA_double_mutants"):
        assert callable(getattr(g, name)), name
    assert callable(devops.double_mutant_scan_dev) and callable(devops.double_mutants_dev)
    for m in ("run_double_mutant_scan_ptr", "run_double_mutant_scan_dev", "run_double_mutants_ptr", "run_double_mutants_dev",
              "double_mutant_scan_dev", "double_mutants_dev"):
        assert hasattr(g.Context, m), m
    assert os.path.exists(g._lib.LIB_PATH), "libgdca.so not built"
    lib = g.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)
    assert lib.gdca_version() == 6
    jl = open(os.path.join(ROOT, "julia", "src", "GaussDCAHip.jl")).read()
    for s in ("gdca_double_mutant_scan", "gdca_double_mutants", "gdca_run_double_mutant_scan", "gdca_run_double_mutants"):
        assert "ccall((:%s, libgdca)" % s in jl, s
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "double_mutant_scan" in open(os.path.join(ROOT, doc)).read(), doc


def test_argument_errors_come_first_then_no_cpu_fallback(refdata, tmp_path):
    import gaussdca.jl_amd as g

    fasta = os.path.join(refdata, "small.fasta.gz")  # N = 53
    missing = str(tmp_path / "missing.fasta")
    X = np.ones((53, 4), dtype=np.int8)
    muts = np.array([[0, 1, 2, 3, 4], [3, 52, 21, 0, 1]])
    for fn, extra in ((g.gDCA_double_mutant_scan, ()), (g.gDCA_double_mutants, (muts,))):
        with pytest.raises(g.ArgumentError, match="invalid pseudocount"):
            fn(missing, X, *extra, pseudocount=1.5, theta=7)
        with pytest.raises(g.ArgumentError, match="invalid θ"):
            fn(missing, X, *extra, θ=7)
        with pytest.raises(g.ArgumentError, match="cannot open file"):
            fn(missing, X, *extra)
        with pytest.raises(g.ArgumentError, match="cannot open file"):
            fn(fasta, missing, *extra)
        with pytest.raises(g.ArgumentError, match="needs sequences"):
            fn(fasta, None, *extra)
        with pytest.raises(TypeError):
            fn(fasta, X, *extra, score=":DI")
        with pytest.raises(g.ArgumentError, match="integer symbols"):
            fn(fasta, X.astype(np.float64), *extra)
        with pytest.raises(g.ArgumentError, match="sites"):
            fn(fasta, X[:-1], *extra)
        with pytest.raises(g.ArgumentError, match="no sequence"):
            fn(fasta, X[:, :0], *extra)
    for bad in (muts[:, :4], muts.astype(np.float64), muts[:0], muts[0], muts + 2 ** 40):
        with pytest.raises(g.ArgumentError, match="mutations"):
            g.gDCA_double_mutants(fasta, X, bad)
    mJ, Pi = np.eye(53 * 20), np.full(53 * 20, 0.05)
    for fn, extra in ((g.double_mutant_scan, ()), (g.double_mutant_energies, (muts,))):
        with pytest.raises(g.ArgumentError, match="incompatible sizes"):
            fn(mJ, Pi, X[:-1], *extra, 21)
        with pytest.raises(g.ArgumentError, match="incompatible sizes"):
            fn(mJ, Pi[:-1], X, *extra, 21)
        with pytest.raises(g.ArgumentError, match="too big"):
            fn(mJ, Pi, X, *extra, 32)
        with pytest.raises(g.ArgumentError, match="no sequence"):
            fn(mJ, Pi, X[:, :0], *extra, 21)
        with pytest.raises(g.ArgumentError, match="at least 2"):
            fn(np.eye(20), np.full(20, 0.05), X[:1], *extra, 21)
    with pytest.raises(g.ArgumentError, match="mutations"):
        g.double_mutant_energies(mJ, Pi, X, muts[:, :3], 21)
    if not os.path.exists(g._lib.LIB_PATH) or g.load().gdca_device_count() <= 0:
        # valid arguments, no device: an error, never a CPU computation
        with pytest.raises(g.GdcaError):
            g.double_mutant_scan(mJ, Pi, X, 21)
        with pytest.raises(g.GdcaError):
            g.double_mutant_energies(mJ, Pi, X, muts, 21)
        with pytest.raises(g.GdcaError):
            g.gDCA_double_mutant_scan(fasta, X)
        with pytest.raises(g.GdcaError):
            g.gDCA_double_mutants(fasta, X, muts)


def test_epistasis_kernels_do_not_spill_and_two_workgroups_share_a_compute_unit(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    report = compiler_report(tmp_path, "k_epistasis.hip", kernels=("k_epi_tilesILi20E", "k_epi_tilesILi0E", "k_epi_list"))
    DT = int(re.search(r"#define DT (\d+)", open(os.path.join(CSRC, "k_epistasis.hip")).read()).group(1))
    ESEQ = int(re.search(r"#define ESEQ (\d+)", open(os.path.join(CSRC, "k_epistasis.hip")).read()).group(1))
    lds = lambda q: DT * q * (DT * q + 1) * 8 + DT * DT * ESEQ * 20  # noqa: E731  (the launcher's formula: the tile and the staging)
    for name, field in report:
        occ = field(r"Occupancy \[waves/SIMD\]")
        print("%-50s %d waves / SIMD" % (name, occ))
        assert field(r"LDS Size \[bytes/block\]") == 0  # (the tile is the launch's dynamic LDS)
        if "ILi20E" in name:
            assert occ >= 2 and 2 * lds(21) <= 160 * 1024, (name, occ)
    assert lds(31) <= 160 * 1024
