"""Shared helpers for the parity tests: the reference test-suite's cases and comparator
(/root/reference/test/runtests.jl:29-50) plus the tie rule of SURVEY.md 4.3."""
import os
import re
import subprocess
from itertools import groupby

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussdca.jl_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-std=c++17", "-Wno-unused-function", "-Wno-pass-failed",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]

# the four golden cases of test/runtests.jl:52-76 (keyword names as in src/GaussDCA.jl:10-15,
# with theta spelled out)
CASES = {
    "small.FNRout.txt": dict(fasta="small.fasta.gz", kw={}),
    "small.DIRout.txt": dict(fasta="small.fasta.gz", kw=dict(pseudocount=0.2, score="DI", remove_dups=True)),
    "small.DIRout2.txt": dict(fasta="small.fasta.gz",
                              kw=dict(pseudocount=0.2, score="DI", theta=0.0, max_gap_fraction=0.8,
                                      min_separation=4)),
    "large.DIRout.txt": dict(fasta="large.fasta.gz", kw=dict(pseudocount=0.2, score="DI", remove_dups=True)),
}


def parse_golden(path):
    """'i j score' lines -> ({(i,j): (float, str)}, [(i,j) in file order])  (runtests.jl:29-39)"""
    d, order = {}, []
    with open(path) as f:
        for line in f:
            sl = line.split()
            if not sl:
                continue
            assert len(sl) == 3
            k = (int(sl[0]), int(sl[1]))
            assert k not in d
            d[k] = (float(sl[2]), sl[2])
            order.append(k)
    return d, order


def _order_mod_ties(pairs_scores):
    """Stable re-sort inside groups of equal 7-digit printed score (SURVEY.md 4.3 tie rule)."""
    out = []
    for _, grp in groupby(pairs_scores, key=lambda t: t[1]):
        out.extend(sorted(k for k, _ in grp))
    return out


def compare_with_golden(R, golden_path):
    d, order = parse_golden(golden_path)
    keys = [(i, j) for i, j, _ in R]
    rep = dict(rows=len(R), keys_equal=(set(keys) == set(d) and len(keys) == len(d)))
    if not rep["keys_equal"]:
        return rep
    max_rel, mism = 0.0, 0
    for i, j, x in R:
        g, gs = d[(i, j)]
        max_rel = max(max_rel, abs(x - g) / abs(g))
        if ("%e" % x) != gs:
            mism += 1
    rep["max_rel"] = max_rel
    rep["string_mismatches"] = mism
    rep["order_equal"] = keys == order
    mine = _order_mod_ties([((i, j), "%e" % x) for i, j, x in R])
    theirs = _order_mod_ties([(k, d[k][1]) for k in order])
    rep["order_equal_mod_ties"] = mine == theirs
    return rep


def score_close(S, S_ref, rtol=1e-6, atol_frac=1e-9, atol_abs=0.0):
    """Elementwise |S - S_ref| <= rtol |S_ref| + atol_frac max|S_ref| + atol_abs on the off-diagonal.

    rtol = 1e-6 is north_star's bar for FN/DI scores; the small absolute term only covers
    APC-corrected scores that cross zero (their relative error is unbounded by construction).
    Returns (ok, max_rel_over_entries_above_1e-3_of_max, max_abs)."""
    N = S.shape[0]
    off = ~np.eye(N, dtype=bool)
    a, b = S[off], S_ref[off]
    # magnitude reference: all entries, diagonal included (the APC-corrected diagonal is -S_i.^2 / Sa, i.e. the
    # size of the raw scores; with few sequences every off-diagonal entry can cancel to rounding noise)
    scale = np.max(np.abs(S_ref))
    ok = bool(np.all(np.abs(a - b) <= rtol * np.abs(b) + atol_frac * scale + atol_abs))
    big = np.abs(b) > 1e-3 * scale
    max_rel = float(np.max(np.abs(a[big] - b[big]) / np.abs(b[big]))) if np.any(big) else 0.0
    return ok, max_rel, float(np.max(np.abs(a - b)))


def random_msa(rng, M, N, q=21, gap_runs=True, clusters=None):
    """Small seeded 'Pfam-like' alignment: cluster centres + per-sequence mutation + gap runs."""
    root = rng.integers(1, q, size=N)
    K = clusters or max(1, M // 25)
    centres = np.tile(root, (K, 1))
    cm = rng.random((K, N)) < 0.25
    centres[cm] = rng.integers(1, q, size=int(cm.sum()))
    Z = centres[rng.integers(0, K, size=M)]
    mu = rng.choice([0.02, 0.05, 0.1, 0.2, 0.3, 0.5], size=M)
    mask = rng.random((M, N)) < mu[:, None]
    Z[mask] = rng.integers(1, q, size=int(mask.sum()))
    if gap_runs:
        for k in range(M):
            for _ in range(rng.integers(0, 4)):
                a = rng.integers(0, N)
                Z[k, a:a + rng.integers(1, max(2, N // 10) + 1)] = q
    return np.ascontiguousarray(Z.astype(np.int8))


def edge_family(M, N, q, seed):
    """(N, M) Fortran int8: a random family plus the columns the tally's skip form treats specially (N >= 5).  For q < 5 the
    symbols of the special columns are clipped to q - 1, so the family stays inside 1..q."""
    c = (lambda x: x) if q >= 5 else (lambda x: min(x, q - 1))
    rng = np.random.default_rng(seed)
    Z = random_msa(rng, M, N, q=q)                      # (M, N)
    Z[:, 0] = c(3)                                      # one symbol everywhere: column 0's kept list is empty
    Z[:, 1] = q                                         # the gap everywhere
    Z[:, 2] = np.where(rng.random(M) < 0.7, q, Z[:, 2])  # the gap is the most frequent symbol
    Z[:, 3] = np.where(np.arange(M) % 2 == 0, c(2), c(5))  # two symbols, equal counts: a tie (with equal weights)
    if M % 2:
        Z[-1, 3] = 1
    Z[:, 4] = np.where(np.arange(M) % 3 == 0, c(4), Z[:, 4])
    return np.asfortranarray(Z.T.astype(np.int8))


# ---- the schedules of the SPD inverse that the tests force through a context's options (test_gpu_parity.py, test_gpu_inverse_exact.py) -------
_SCHEDULES = [{"GDCA_GROUP": "1"}, {"GDCA_GROUP": "2"}, {"GDCA_GROUP": "3"}, {"GDCA_GROUP": "4"},
              {"GDCA_GROUP": "3", "GDCA_MCUS": "1"}, {"GDCA_GROUP": "2", "GDCA_MCUS": "16"},
              {"GDCA_GROUP": "4", "GDCA_MCUS": "3"}, {"GDCA_GROUP": "3", "GDCA_REM_TAIL": "0"},
              {"GDCA_GROUP": "2", "GDCA_REM_TAIL": "7"}, {"GDCA_GROUP": "4", "GDCA_REM_TAIL": "100000"},
              {"GDCA_GROUP": "3", "GDCA_PANEL_HALVES": "1"}, {"GDCA_GROUP": "2", "GDCA_PANEL_HALVES": "0"},
              {"GDCA_GROUP": "1", "GDCA_PANEL_HALVES": "0"}, {"GDCA_GROUP": "3", "GDCA_RAMP": "0"},
              {"GDCA_GROUP": "4", "GDCA_RAMP": "0"}, {"GDCA_GROUP": "2", "GDCA_RAMP": "0", "GDCA_MCUS": "2"},
              {"GDCA_GROUP": "3", "GDCA_RAGGED": "0"}, {"GDCA_GROUP": "4", "GDCA_SWEEP_DEBUG": "1"},
              {"GDCA_GROUP": "1", "GDCA_SWEEP_DEBUG": "1", "GDCA_MCUS": "16"},
              {"GDCA_GROUP": "1", "GDCA_SLAB": "0"}, {"GDCA_GROUP": "1", "GDCA_SLAB": "0", "GDCA_RING": "2"},
              {"GDCA_GROUP": "1", "GDCA_RING": "2"}, {"GDCA_GROUP": "1", "GDCA_RING": "3", "GDCA_MCUS": "2"},
              {"GDCA_GROUP": "1", "GDCA_MCUS": "1"},
              # the merged kernel (k_sweep_merged) carrying this one inverse (SWEEP_DEBUG bit 3), workspaces poisoned (bit 4)
              {"GDCA_SWEEP_DEBUG": "24"}, {"GDCA_SWEEP_DEBUG": "24", "GDCA_SLAB": "0"}, {"GDCA_SWEEP_DEBUG": "25", "GDCA_RING": "2"},
              {"GDCA_SWEEP_DEBUG": "24", "GDCA_MERGE_MCUS": "1"}, {"GDCA_SWEEP_DEBUG": "24", "GDCA_RAGGED": "0", "GDCA_MERGE_MCUS": "16"}]


# ---- the model read-outs (energies, pair energies, mutation scan): what their GPU tests share ---------------------------------------------
@pytest.fixture(scope="module")
def g():
    import gaussdca.jl_amd as g

    assert os.path.exists(g._lib.LIB_PATH), "libgdca.so missing: the GPU tests never fall back to the CPU"
    assert g.load().gdca_device_count() > 0, "no HIP device"
    return g


@pytest.fixture(scope="module")
def ctx(g):
    c = g.Context(0)
    yield c
    c.close()


_models = {}  # one cache for every file: an oracle model is fitted once per run of the suite


def golden_model(refdata, name, pc, theta="auto", dedup=False):
    """(Zo (M, N), q, mJ, Pi) of the oracle chain on a golden alignment"""
    import energy_model as em
    from oracle import gdca_oracle as o

    key = (name, pc, theta, dedup)
    if key not in _models:
        Zo = o.read_fasta_alignment(os.path.join(refdata, name), 0.9)
        if dedup:
            Zo = o.remove_duplicate_sequences(Zo)[0]
        q = int(Zo.max())
        _models[key] = (Zo, q) + em.model_from_Z(Zo, q, pc, theta)
    return _models[key]


def synth_model(q, N, seed=None):
    import energy_model as em
    from gaussdca.jl_amd.synth import synth_family

    key = ("synth", q, N)
    if key not in _models:
        Zo = synth_family(N, 300, q, seed=seed or 1000 * q + N)
        _models[key] = (Zo, q) + em.model_from_Z(Zo, q, 0.5)
    return _models[key]


def mixed_sequences(rng, Zo, q, K, shift=0):
    """(N, K) int8: column j is, by (j + shift) % 4: all gaps, a sequence without gaps, a uniformly random one (gaps included), a
    member of the family Zo (M, N)"""
    M, N = Zo.shape
    X = np.empty((N, K), dtype=np.int8)
    for j in range(K):
        kind = (j + shift) % 4
        if kind == 0:
            X[:, j] = q
        elif kind == 1:
            X[:, j] = rng.integers(1, q, size=N)
        elif kind == 2:
            X[:, j] = rng.integers(1, q + 1, size=N)
        else:
            X[:, j] = Zo[rng.integers(0, M)]
    return np.asfortranarray(X)


def assert_within_order_bound(E, mJ, Pi, X, q, what):
    """energies E of the sequences X against tests/energy_model.py, within its bound of any summation order"""
    import energy_model as em

    E_ref, B, c0 = em.energies_gather(mJ, Pi, X, q)
    bound = em.order_bound(X.shape[0], q, B)
    err = np.abs(E - E_ref)
    print("%s: max |E - E_ref| / bound = %.3g, bound / |E| = %.3g .. %.3g" %
          (what, float((err / bound).max()), float((bound / np.abs(E_ref)).min()), float((bound / np.abs(E_ref)).max())))
    assert np.all(err <= bound), (what, float((err / bound).max()))
    return E_ref, c0, bound


def mutation_reference(mJ, Pi, X, q):
    """tests/mutation_model.py on the sequences X: (V, bound of V, dE, bound of dE), all (K, N, q)"""
    import mutation_model as mm

    N = X.shape[0]
    V, B, Vl = mm.potentials_exact(mJ, Pi, X, q)
    dE = mm.delta_exact(Vl, X, q)
    return V, mm.bound_V(N, q, B), dE, mm.delta_bound(N, q, B, X, dE)


def ratio(D, ref, bound):
    """max |D - ref| / bound over the entries with a bound; where the bound is 0 (the gap target of V, the b = x_i entry of a gap site)
    the entry must be exact"""
    err = np.abs(D - ref)
    z = bound == 0
    assert np.all(err[z] == 0)
    return float((err[~z] / bound[~z]).max()) if (~z).any() else 0.0


def compiler_report(tmp_path, file, kernels=None, min_loops=None):
    """The compiler's report on one kernel file of csrc (tests/test_kernel_resources.py has a fixed list of files).
    ``kernels``: the file is compiled with the resource-usage remarks; every name of ``kernels`` must be among its kernels, and EVERY
    kernel of the file must be free of spills and scratch.  Returns [(kernel name, field)], field(label) = that kernel's number.
    ``min_loops``: the file's assembly must carry at least that many of the compiler's loop annotations, and no barrier may sit inside
    a divergent loop (tools/asm_loops.py)."""
    src = os.path.join(CSRC, file)
    report = []
    if kernels is not None:
        r = subprocess.run([HIPCC, *FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "x.o")],
                           capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stderr[-3000:]
        blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
        names = [b.split()[0] for b in blocks]
        for k in kernels:
            assert any(k in n for n in names), (k, names)
        for b in blocks:
            name = b.split()[0]

            def field(label, b=b, name=name):
                m = re.search(label + r": (\d+)", b)
                assert m, (name, label)
                return int(m.group(1))

            spills, scratch, vgprs = field("VGPRs Spill"), field(r"ScratchSize \[bytes/lane\]"), field("VGPRs")
            print("%-60s VGPRs %3d spilled %3d scratch %3d B" % (name, vgprs, spills, scratch))
            assert spills == 0 and scratch == 0, (name, vgprs, spills, scratch)
            report.append((name, field))
    if min_loops is not None:
        import importlib.util

        spec = importlib.util.spec_from_file_location("asm_loops", os.path.join(ROOT, "tools", "asm_loops.py"))
        al = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(al)
        out = tmp_path / (file + ".s")
        r = subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", src, "-o", str(out)], capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stderr[-3000:]
        bad, seen = al.divergent_barrier_loops(out.read_text())
        assert seen >= min_loops, seen  # (the compiler's loop annotations are there)
        assert not bad, bad
    return report
