"""The rule that picks the cut word of the two-phase Hamming bound (csrc/gdca_hamming_cut.h), on the CPU: the header
is plain C++ shared by k_hamming_decide and this test, which compiles it alone with the host compiler and calls it through ctypes."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussdca.jl_amd", "csrc")
LIST_CAP = 2048   # HAM_LIST_CAP
TILE_PAIRS = 128 * 128
PAIRS = 192 * TILE_PAIRS  # what the probe samples

# alive fraction after w words (tools/hamming_alive.py on the benchmark's families); words the table leaves out are
# alive (1.0)
TABLE = {
    "C": (16, {7: 0.981, 8: 0.79, 9: 0.526, 10: 0.31, 11: 0.155, 12: 5.8e-2, 13: 1.6e-2, 14: 2.6e-3, 15: 4.2e-4, 16: 2.4e-4}),
    "D": (32, {20: 0.313, 21: 0.223, 22: 0.151, 23: 9.7e-2, 24: 5.8e-2, 25: 3.1e-2, 26: 1.4e-2, 27: 5.4e-3, 28: 1.6e-3, 29: 4.3e-4,
               30: 1.5e-4, 31: 1.2e-4, 32: 1.2e-4}),
    "B": (4, {1: 0.913, 2: 2.8e-2, 3: 6.1e-4, 4: 2.9e-4}),
}
# the cut that measured best at each configuration (profiles/hamming_cut_sweep.log)
MEASURED_BEST = {"C": 12, "D": 24, "B": 3}


@pytest.fixture(scope="module")
def pick(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    d = tmp_path_factory.mktemp("cut")
    src = d / "pick.cpp"
    src.write_text('#include "gdca_hamming_cut.h"\n'
                   'extern "C" int pick(const unsigned *alive, double pairs, int NW) { return gdca_hamming_pick_cut(alive, pairs, NW); }\n'
                   'extern "C" int list_cap(void) { return HAM_LIST_CAP; }\n'
                   'extern "C" int alive_slots(void) { return HAM_ALIVE_SLOTS; }\n')
    so = d / "pick.so"
    subprocess.run([cxx, "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.pick.restype = ctypes.c_int
    lib.pick.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_int]
    assert lib.list_cap() == LIST_CAP and lib.alive_slots() == 64

    def call(fractions, NW, pairs=PAIRS):
        """fractions[w - 1] = alive fraction after w words"""
        a = np.zeros(64, dtype=np.uint32)
        n = min(len(fractions), 64)
        a[:n] = np.rint(np.asarray(fractions[:n], dtype=np.float64) * pairs).astype(np.uint32)
        return int(lib.pick(a.ctypes.data, float(pairs), int(NW)))

    return call


def _fractions(NW, known):
    return [known.get(w, 1.0) for w in range(1, NW + 1)]


def test_no_cut_where_every_pair_stays_alive(pick):
    for NW in (3, 4, 10, 16, 32, 64):
        assert pick([1.0] * NW, NW) == NW


def test_no_cut_on_short_alignments_or_without_counts(pick):
    for NW in (1, 2):  # N <= 64
        assert pick([1e-4] * NW, NW) == NW
    assert pick([1e-4] * 64, 65) == 65             # more words than the probe counts
    assert pick([0.0] * 16, 16, pairs=0) == 16     # nothing sampled


@pytest.mark.parametrize("config", sorted(TABLE))
def test_the_benchmark_families_are_cut_in_their_last_chunk(pick, config):
    NW, known = TABLE[config]
    cut = pick(_fractions(NW, known), NW)
    assert (NW - 1) // 8 * 8 <= cut < NW, (config, cut)
    assert known[cut] * TILE_PAIRS <= LIST_CAP / 2
    assert cut == MEASURED_BEST[config]


def test_never_a_cut_whose_expected_list_exceeds_half_the_capacity(pick):
    rng = np.random.default_rng(5)
    picked = 0
    for _ in range(2000):
        NW = int(rng.integers(3, 65))
        # a monotone alive curve that falls off somewhere, at a random rate, to a random floor
        knee, rate, floor = rng.uniform(0, NW), rng.uniform(0.2, 3.0), 10.0 ** rng.uniform(-6, -0.5)
        fr = [float(min(1.0, max(floor, np.exp(-rate * max(0.0, w - knee))))) for w in range(1, NW + 1)]
        cut = pick(fr, NW)
        assert 1 <= cut <= NW
        if cut < NW:
            picked += 1
            assert fr[cut - 1] * TILE_PAIRS <= LIST_CAP / 2 + 1, (NW, cut, fr[cut - 1])
    assert picked > 200  # (the curves do reach the rule's "cut" branch)
