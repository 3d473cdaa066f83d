"""The greedy walk without a GPU: the numpy statement of its rule (tests/walk_model.py) against the exact replay within the derived
bounds on the inputs the GPU tests use, a model with exact ties whose path is written down by hand, the exported symbols and
bindings with their argument checks, and the compiler's report on k_walk.hip."""
import ctypes
import os
import re

import numpy as np
import pytest

import mutation_model as mm
import walk_model as wm
from gdca_testutil import CSRC, HIPCC, ROOT, compiler_report, golden_model, mixed_sequences

NEW_SYMBOLS = ("gdca_greedy_walk_dev", "gdca_greedy_walk", "gdca_run_greedy_walk_dev", "gdca_run_greedy_walk")


# ---- 1. the rule against the exact replay, on the inputs of tests/test_gpu_walk.py -----------------------------------------------------------
@pytest.mark.parametrize("pc", [0.8, 0.2])
def test_emulated_walks_hold_the_bounds_and_end_in_local_minima(refdata, pc):
    Zo, q, mJ, Pi = golden_model(refdata, "small.fasta.gz", pc)
    N = Zo.shape[1]
    assert (N, q) == (53, 21)
    X = mixed_sequences(np.random.default_rng(7), Zo, q, 8)
    V0 = mm.potentials_dense(mJ, Pi, X, q)
    T = 4 * N
    lengths, worst = [], 0.0
    for k in range(8):
        xout, steps, path, dE_path, dE_sum, V = wm.emulate(V0[k], mJ, X[:, k], q, None, 0, 0.0, T)
        assert np.array_equal(xout, wm.states_of(X[:, k], path, steps)[:, -1])
        assert np.all(path[steps:] == -1) and np.all(dE_path[steps:] == 0.0)
        _, w = wm.check_walk(mJ, Pi, X[:, k], q, None, 0, 0.0, T, steps, path, dE_path, V, "pc %g k %d" % (pc, k))
        worst = max(worst, w)
        lengths.append(steps)
    print("pc %g: walk lengths %s, largest error / bound %.3g" % (pc, lengths, worst))
    # what the GPU tests rely on
    assert min(lengths) == 0 and max(lengths) >= N and max(lengths) < T
    cut = [wm.emulate(V0[k], mJ, X[:, k], q, None, 0, 0.0, 16)[1] for k in range(8)]
    assert 16 in cut and cut == [min(n, 16) for n in lengths]
    # both flags: the all-gap sequence may move now, and every walk still ends
    both = [wm.emulate(V0[k], mJ, X[:, k], q, None, 3, 0.0, T) for k in range(8)]
    assert all(r[1] < T for r in both)
    for k in (0, 2):
        r = both[k]
        wm.check_walk(mJ, Pi, X[:, k], q, None, 3, 0.0, T, r[1], r[2], r[3], r[5], "flags 3 k %d" % k)


# ---- 2. exact ties: an independent-site model whose every operation is exact ---------------------------------------------------------------
def tie_model():
    """N = 4, q = 3: mJ diagonal with powers of two, Pi multiples of 1/8, so V[i][c] = d (1/2 - Pi) exactly and no step changes another
    site's potentials.  Sites 0 and 1 have identical blocks and equal symbols.  -> (mJ, Pi, x, V)"""
    d = np.array([4.0, 2.0, 4.0, 2.0, 8.0, 1.0, 2.0, 4.0])
    Pi = np.array([1, 3, 1, 3, 5, 1, 2, 4]) / 8.0
    V = np.array([[1.5, 0.25, 0.0], [1.5, 0.25, 0.0], [-1.0, 0.375, 0.0], [0.5, 0.0, 0.0]])
    x = np.array([1, 1, 2, 3], dtype=np.int8)
    return np.diag(d), Pi, x, V


# flags, mask, min_gain -> (path rows (i, b), their dE, the final sequence): by hand, ordered by dE, then by the code 3 i + (b - 1)
TIE_CASES = [
    # residues into residues: site 2 -> 1 (-1.375), then the tie of sites 0 and 1 (-1.25 each), the smaller code first
    (0, None, 0.0, [(2, 1), (0, 2), (1, 2)], [-1.375, -1.25, -1.25], [2, 2, 1, 3]),
    # the gap as a target and gap sites free: deleting at sites 0 and 1 (-1.5 each, codes 2 and 5) beats everything; site 3's best
    # move is worth exactly 0 and is not taken
    (3, None, 0.0, [(0, 3), (1, 3), (2, 1)], [-1.5, -1.5, -1.375], [3, 3, 1, 3]),
    (0, [0, 1, 1, 1], 0.0, [(2, 1), (1, 2)], [-1.375, -1.25], [1, 2, 1, 3]),
    (0, None, 1.3, [(2, 1)], [-1.375], [1, 1, 1, 3]),
    (2, None, 0.0, [(2, 1), (0, 2), (1, 2)], [-1.375, -1.25, -1.25], [2, 2, 1, 3]),  # fill_gaps alone: site 3's fills cost >= 0
]


def test_exact_ties_follow_the_hand_written_path():
    mJ, Pi, x, V = tie_model()
    assert np.array_equal(mm.potentials_dense(mJ, Pi, x[:, None], 3)[0], V)
    for flags, mask, min_gain, moves, dEs, final in TIE_CASES:
        xout, steps, path, dE_path, dE_sum, Vf = wm.emulate(V, mJ, x, 3, mask, flags, min_gain, 8)
        assert steps == len(moves) and [tuple(r) for r in path[:steps]] == moves, (flags, mask, min_gain, path)
        assert list(dE_path[:steps]) == dEs and dE_sum == sum(dEs)
        assert list(xout) == final and np.array_equal(Vf, V)
        assert np.all(path[steps:] == -1) and np.all(dE_path[steps:] == 0.0)


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
    assert len(protos["gdca_greedy_walk_dev"][1]) == 17 and len(protos["gdca_run_greedy_walk"][1]) == 19
    assert g.load().gdca_version() == 6
    assert (_lib.WALK_GAP_TARGET, _lib.WALK_FILL_GAPS, _lib.WALK_MAX_STEPS) == (1, 2, 65535)
    hdr = open(os.path.join(ROOT, "include", "gdca.h")).read()
    assert "enum { GDCA_WALK_GAP_TARGET = 1, GDCA_WALK_FILL_GAPS = 2 };" in hdr and "#define GDCA_WALK_MAX_STEPS 65535" in hdr
    assert "WALK_TABLE" in hdr
    assert callable(g.greedy_walk) and callable(g.gDCA_greedy_walk) and callable(devops.greedy_walk_dev)
    for m in ("greedy_walk_dev", "run_greedy_walk_dev", "run_greedy_walk_ptr"):
        assert hasattr(g.Context, m), m

    fasta = os.path.join(refdata, "small.fasta.gz")  # N = 53
    missing = str(tmp_path / "missing.fasta")
    X = np.ones((53, 4), dtype=np.int8)
    mJ, Pi = np.eye(53 * 20), np.full(53 * 20, 0.05)
    with pytest.raises(g.ArgumentError, match="incompatible sizes"):
        g.greedy_walk(mJ, Pi, X[:-1], 21)
    with pytest.raises(g.ArgumentError, match="too big"):
        g.greedy_walk(mJ, Pi, X, 32)
    with pytest.raises(g.ArgumentError, match="no sequence"):
        g.greedy_walk(mJ, Pi, X[:, :0], 21)
    for bad in (0, -1, 65536, 2.5):
        with pytest.raises(g.ArgumentError, match="max_steps"):
            g.greedy_walk(mJ, Pi, X, 21, max_steps=bad)
    for bad in (-1e-9, float("nan"), "x"):
        with pytest.raises(g.ArgumentError, match="min_gain"):
            g.greedy_walk(mJ, Pi, X, 21, min_gain=bad)
    for bad in (np.ones(52), np.ones((53, 2)), np.ones(53) * 0.5):
        with pytest.raises(g.ArgumentError, match="mask"):
            g.greedy_walk(mJ, Pi, X, 21, mask=bad)
    with pytest.raises(g.ArgumentError, match="invalid pseudocount"):
        g.gDCA_greedy_walk(missing, X, pseudocount=1.5)
    with pytest.raises(g.ArgumentError, match="cannot open file"):
        g.gDCA_greedy_walk(missing, X)
    with pytest.raises(TypeError):
        g.gDCA_greedy_walk(fasta, X, score=":DI")
    with pytest.raises(g.ArgumentError, match="sites"):
        g.gDCA_greedy_walk(fasta, X[:-1])
    if g.load().gdca_device_count() <= 0:
        # valid arguments, no device: an error, never a CPU computation (tests/test_cabi_cpu.py::test_no_cpu_fallback)
        with pytest.raises(g.GdcaError):
            g.greedy_walk(mJ, Pi, X, 21)
        with pytest.raises(g.GdcaError):
            g.gDCA_greedy_walk(fasta, X)


# ---- 4. the compiler's report on k_walk.hip -------------------------------------------------------------------------------------------------
def test_walk_kernels_do_not_spill_and_hold_no_barrier_in_a_divergent_loop(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    report = compiler_report(tmp_path, "k_walk.hip", kernels=("k_walkILb1E", "k_walkILb0E"))
    assert len(report) == 2
    for name, field in report:
        assert field(r"LDS Size \[bytes/block\]") == 0  # (the table is the launch's dynamic LDS)
    # each instance: the step loop with the scan and the update loops in it, the loops of the prologue and the epilogue
    compiler_report(tmp_path, "k_walk.hip", min_loops=16)
    code = "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, "k_walk.hip")).read().split("\n"))
    assert len(re.findall(r"__syncthreads\(\)", code)) == 5 and "atomic" not in code
