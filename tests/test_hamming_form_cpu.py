"""The rule that picks the form of the all-pairs reweighting (csrc/gdca_hamming_form.h), on the CPU: the header is plain
C++ shared by k_hamming_decide and this test, which compiles it alone with the host compiler and calls it through ctypes.  The
argmin is checked against a restatement of the cost model in Python on a grid of densities and sizes; no density at which a bound
form is chosen fills more than half of the candidate list."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussdca.jl_amd", "csrc")
PAIRS = 192 * 128 * 128  # what the probes sample


def constants():
    """the header's #define lines with a plain number"""
    text = open(os.path.join(CSRC, "gdca_hamming_form.h")).read()
    return {m.group(1): float(m.group(2)) for m in re.finditer(r"^#define (HAM_\w+) (-?[0-9.]+(?:e-?[0-9]+)?)\s", text, re.M)}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    d = tmp_path_factory.mktemp("form")
    src = d / "form.cpp"
    src.write_text('#include "gdca_hamming_form.h"\n'
                   'extern "C" int pick(double c3, double c1, double pairs, int N, int M, int cut) { return gdca_hamming_pick_form(c3, c1, pairs, N, M, cut); }\n'
                   'extern "C" int gate(int N, int M) { return gdca_hamming_consensus_gate(N, M); }\n'
                   'extern "C" int per_tile(void) { return HAM_CAND_PER_TILE; }\n'
                   'extern "C" double max_density(void) { return HAM_FORM_MAX_DENSITY; }\n')
    so = d / "form.so"
    subprocess.run([cxx, "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.pick.restype = ctypes.c_int
    lib.pick.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.gate.restype = ctypes.c_int
    lib.gate.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.per_tile.restype = ctypes.c_int
    lib.max_density.restype = ctypes.c_double
    return lib


def model(c, f3, f1, N, M, cut):
    """the header's rule, restated"""
    NW = (N + 31) // 32
    Mt = (M + 127) // 128
    tiles, pairs = 0.5 * Mt * (Mt + 1), 0.5 * M * M
    other = 1 if f3 < c["HAM_FORM_BOUND3_DENSITY"] else 0
    if f1 is None or f1 > 0.5 * c["HAM_CAND_PER_TILE"] / 16384.0:
        return other
    weff = cut + c["HAM_CUT_TAIL"] * (NW - cut) if 0 < cut < NW else NW
    E = (NW + 7) // 8 * 8
    pair = c["HAM_T_PAIR"] + N * c["HAM_T_REFINE"]
    if other:
        cost_other = tiles * weff * c["HAM_T_DENSE"] + f3 * pairs * pair
    else:
        cost_other = tiles * NW * 1.5 * c["HAM_T_DENSE"]
    cost_cons = tiles * (c["HAM_T_TILE"] + E * c["HAM_T_ENTRY"]) + f1 * pairs * pair + M * E * c["HAM_T_IMAGE"] + c["HAM_T_FIXED"]
    return 2 if cost_cons < cost_other else other


DENSITIES = (0.0, 1e-5, 1.2e-4, 2.4e-4, 5e-4, 9.3e-4, 1.1e-3, 1.5e-3, 1.9e-3, 2.0e-3, 3.1e-3, 8.1e-3, 0.56)
SIZES = ((128, 10000), (129, 69318), (227, 33345), (286, 76423), (360, 39662), (500, 50000), (1000, 100000), (100, 5000), (600, 80000))


def test_the_argmin_is_the_models(lib):
    c = constants()
    assert c["HAM_CAND_PER_TILE"] == lib.per_tile() and abs(lib.max_density() - 0.5 * c["HAM_CAND_PER_TILE"] / 16384.0) < 1e-15
    seen = set()
    for (N, M), f3, f1 in itertools.product(SIZES, DENSITIES, DENSITIES + (None,)):
        NW = (N + 31) // 32
        for cut in (0, max(1, 3 * NW // 4), NW):
            got = lib.pick(f3 * PAIRS, -1.0 if f1 is None else f1 * PAIRS, float(PAIRS), N, M, cut)
            assert got == model(c, f3, f1, N, M, cut), (N, M, f3, f1, cut)
            seen.add(got)
    assert seen == {0, 1, 2}


def test_no_chosen_density_fills_more_than_half_the_list(lib):
    half = 0.5 * lib.per_tile() / 16384.0
    for (N, M), f3, f1 in itertools.product(SIZES, DENSITIES, DENSITIES):
        got = lib.pick(f3 * PAIRS, f1 * PAIRS, float(PAIRS), N, M, 0)
        if got == 2:
            assert f1 <= half, (N, M, f1)
        if got == 1:
            assert f3 <= half, (N, M, f3)


def test_the_benchmark_families(lib):
    """the densities tools/hamming_alive.py --bound consensus measures: configs C and D take the consensus form; a family that was
    not probed for it (config B is below the gate) stays with the three-plane form"""
    assert lib.pick(2.39e-4 * PAIRS, 9.3e-4 * PAIRS, float(PAIRS), 500, 50000, 12) == 2
    assert lib.pick(1.2e-4 * PAIRS, 3.3e-4 * PAIRS, float(PAIRS), 1000, 100000, 24) == 2
    assert not lib.gate(128, 10000) and lib.pick(2.9e-4 * PAIRS, -1.0, float(PAIRS), 128, 10000, 3) == 1
    assert lib.gate(500, 50000) and lib.gate(1000, 100000)
    assert lib.pick(3.4e-4 * PAIRS, 1.5e-3 * PAIRS, float(PAIRS), 360, 39662, 9) == 2    # E family 1: measured 0.69 ms against 1.11
    assert lib.pick(5.8e-4 * PAIRS, 3.1e-3 * PAIRS, float(PAIRS), 227, 33345, 6) == 1    # E family 0: more than half the list
    assert lib.pick(1.4e-3 * PAIRS, 8.1e-3 * PAIRS, float(PAIRS), 129, 69318, 0) == 0    # E family 2: neither bound pays
    assert not lib.gate(64, 1000000)  # two words per plane: the exact form, unprobed
    assert lib.pick(0.0, 0.0, 0.0, 500, 50000, 0) == 0  # nothing sampled
