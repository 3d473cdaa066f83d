"""Partner matching per species without a GPU: the surface (header, exports, bindings), gdca_pair_blocks_length and species_blocks
(host code), the numpy / scipy model of tests/partner_model.py, and the compiler's report on the two new kernels."""
import os
import re

import numpy as np
import pytest

import energy_model as em
import pair_energy_model as pm
import partner_model as pt
from gdca_testutil import HIPCC, ROOT, compiler_report

NEW_SYMBOLS = ["gdca_pair_energies_blocked_dev", "gdca_pair_energies_blocked", "gdca_assign_blocks_dev", "gdca_assign_blocks",
               "gdca_run_partner_match_dev", "gdca_run_partner_match"]


def test_symbols_are_declared_exported_and_bound():
    import gaussdca.jl_amd as g

    header = open(os.path.join(ROOT, "include", "gdca.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"gdca_status %s\(gdca_ctx \*ctx" % s, header), s
        assert s in g._lib.SYMBOLS, s
    assert re.search(r"int64_t gdca_pair_blocks_length\(const int32_t \*offA, const int32_t \*offB, int32_t S\);", header)
    assert "gdca_pair_blocks_length" in g._lib.SYMBOLS
    assert re.search(r"#define GDCA_ASSIGN_MAX 512\b", header)
    assert re.search(r"#define GDCA_VERSION_MINOR\s+6\b", header)
    for name in ("species_blocks", "pair_energies_blocked", "assign_blocks", "gDCA_partner_match"):
        assert callable(getattr(g, name)), name
    for name in ("pair_energies_blocked_dev", "assign_blocks_dev", "run_partner_match_ptr", "run_partner_match_dev"):
        assert hasattr(g.Context, name), name
    from gaussdca.jl_amd import devops

    assert callable(devops.pair_energies_blocked_dev) and callable(devops.assign_blocks_dev)
    assert os.path.exists(g._lib.LIB_PATH), "libgdca.so not built"
    lib = g.load()
    for s in NEW_SYMBOLS + ["gdca_pair_blocks_length"]:
        assert hasattr(lib, s)
    assert lib.gdca_version() == 6
    jl = open(os.path.join(ROOT, "julia", "src", "GaussDCAHip.jl")).read()
    for s in ("gdca_pair_energies_blocked_dev", "gdca_assign_blocks_dev", "gdca_run_partner_match_dev", "gdca_run_partner_match"):
        assert "ccall((:%s, libgdca)" % s in jl, s
    assert re.search(r"export[^\n]*(\n[^\n]+)*gDCA_partner_match", jl)


def test_pair_blocks_length():
    import gaussdca.jl_amd as g

    rng = np.random.default_rng(4)
    for S in (1, 2, 17, 1000):
        offA, offB = pt.offsets(rng.integers(0, 40, size=S)), pt.offsets(rng.integers(0, 40, size=S))
        assert g._lib.pair_blocks_length(offA, offB) == pt.blocks_length(offA, offB)
    assert g._lib.pair_blocks_length([0, 0], [0, 5]) == 0
    # 64-bit: 40000 x 60000 in one species
    assert g._lib.pair_blocks_length([0, 40000], [0, 60000]) == 2400000000
    # non-monotone, on either side
    assert g._lib.pair_blocks_length([0, 3, 2, 5], [0, 1, 2, 3]) == -1
    assert g._lib.pair_blocks_length([0, 1, 2, 3], [0, 3, 2, 5]) == -1
    # a wrong end: the offsets do not start at 0
    assert g._lib.pair_blocks_length([1, 3, 5], [0, 1, 2]) == -1
    assert g._lib.pair_blocks_length([0, 3, 5], [2, 2, 2]) == -1
    # S = 0, and no offsets at all
    lib = g.load()
    zero = np.zeros(1, dtype=np.int32)
    assert lib.gdca_pair_blocks_length(g._lib._p(zero), g._lib._p(zero), 0) == -1
    assert lib.gdca_pair_blocks_length(None, g._lib._p(zero), 1) == -1


def test_species_blocks():
    import gaussdca.jl_amd as g

    la, lb = np.array([7, 3, 7, 9, 3, 7]), np.array([9, 9, 3, 12, 7])
    perm_a, perm_b, offA, offB, labels = g.species_blocks(la, lb)
    assert labels.tolist() == [3, 7, 9, 12]
    # stable: inside a species the caller's order
    assert perm_a.tolist() == [1, 4, 0, 2, 5, 3] and perm_b.tolist() == [2, 4, 0, 1, 3]
    assert offA.dtype == offB.dtype == np.int32
    # a label present on one side only: an empty side (12 has no sequence of A)
    assert offA.tolist() == [0, 2, 5, 6, 6] and offB.tolist() == [0, 1, 2, 4, 5]
    perm_a, perm_b, offA, offB, labels = g.species_blocks([1, 1], [2])
    assert labels.tolist() == [1, 2] and offA.tolist() == [0, 2, 2] and offB.tolist() == [0, 0, 1]
    # unsorted input round-trips: values scattered back through the permutation are the caller's
    rng = np.random.default_rng(0)
    la = rng.integers(-5, 30, size=200)
    lb = rng.integers(-5, 30, size=150)
    perm_a, perm_b, offA, offB, labels = g.species_blocks(la, lb)
    assert np.all(np.diff(la[perm_a]) >= 0) and np.all(np.diff(lb[perm_b]) >= 0)
    for s, lab in enumerate(labels):
        assert np.all(la[perm_a][offA[s]:offA[s + 1]] == lab) and np.all(lb[perm_b][offB[s]:offB[s + 1]] == lab)
        assert np.all(np.diff(perm_a[offA[s]:offA[s + 1]]) > 0)  # stable
    back = np.empty_like(la)
    back[perm_a] = la[perm_a]
    assert np.array_equal(back, la)
    assert offA[-1] == 200 and offB[-1] == 150
    with pytest.raises(g.ArgumentError):
        g.species_blocks([1.5, 2.0], [1])
    with pytest.raises(g.ArgumentError):
        g.species_blocks([[1, 2]], [1])


def test_scipy_equals_brute_force():
    rng = np.random.default_rng(11)
    n = 0
    for kA in range(0, 7):
        for kB in range(0, 7):
            for trial in range(3):
                C = rng.normal(size=(kA, kB)) * 10.0 if trial else rng.integers(-4, 5, size=(kA, kB)).astype(float)  # (ties too)
                match, total = pt.assign_scipy(C)
                assert pt.is_valid_matching(C, match)
                brute = pt.assign_brute(C)
                assert abs(total - brute) <= pt.solver_bar(C) + 1e-300, (kA, kB, total, brute)
                assert total == pt.total_of(C, match) or abs(total - pt.total_of(C, match)) <= pt.solver_bar(C)
                if not trial:
                    assert total == brute  # integers: exact
                n += 1
    assert n == 147
    # the gap: the row's own minimum overridden gives a negative one; one column: +inf; unmatched: 0.0
    C = np.array([[1.0, 2.0], [1.5, 9.0]])
    match, _ = pt.assign_scipy(C)
    assert match.tolist() == [1, 0] and pt.gap_of(C, match).tolist() == [-1.0, 7.5]
    assert pt.gap_of(np.array([[3.0], [1.0]]), np.array([-1, 0])).tolist() == [0.0, np.inf]


@pytest.fixture(scope="module")
def paired_blocks():
    """the held-out pairs of the paired family cut into species, their energy blocks under the numpy model"""
    Zfit, Zheld = pm.paired_family(30, 1000, 64)
    mJ, Pi = em.model_from_Z(Zfit, 21, 0.5)
    XA, XB = np.asfortranarray(Zheld[:, :30].T), np.asfortranarray(Zheld[:, 30:].T)
    E = pm.pair_energy(mJ, Pi, XA, XB, 21)[0]
    off = pt.offsets(pt.SPECIES_CUT)
    return E, pt.cut_blocks(E, off, off)


def test_the_assignment_recovers_more_native_partners_than_the_row_minimum(paired_blocks):
    E, blocks = paired_blocks
    assert sum(pt.SPECIES_CUT) == 64 == E.shape[0]
    by_argmin_all = int(np.sum(E.argmin(axis=1) == np.arange(64)))
    by_argmin = pt.native_recovered([b.argmin(axis=1) for b in blocks])
    by_assignment = pt.native_recovered([pt.assign_scipy(b)[0] for b in blocks])
    print("native partners of 64: row argmin over all %d, row argmin inside the species %d, assignment inside the species %d" %
          (by_argmin_all, by_argmin, by_assignment))
    assert by_assignment > by_argmin >= by_argmin_all
    assert by_assignment >= 50


def test_second_best_assignments_lie_far_above_the_bar(paired_blocks):
    """so that the permutation itself is a fair thing to compare on the GPU"""
    _, blocks = paired_blocks
    for b in blocks:
        margin, bar = pt.second_best_margin(b), pt.solver_bar(b)
        print("species %2d x %2d: second best above the optimum by %.4g, bar %.3g" % (*b.shape, margin, bar))
        assert margin > 1000.0 * bar, (b.shape, margin, bar)


# ---- the compiler's report on the new kernels -----------------------------------------------------------------------------------------
def test_partner_kernels_do_not_spill(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    compiler_report(tmp_path, "k_pair_energy.hip", kernels=("k_pair_gather_blocked",))
    compiler_report(tmp_path, "k_assign.hip", kernels=("k_assign_blocks",))


def test_no_barrier_sits_inside_a_divergent_loop_of_the_partner_kernels(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    compiler_report(tmp_path, "k_pair_energy.hip", min_loops=6)  # (the two full instances' four, the blocked gather's two)
    compiler_report(tmp_path, "k_assign.hip", min_loops=3)      # (the additions, the tree's growth, the column scans)
