"""The consensus bound of the reweighting on the fp4 matrix pipe (csrc/k_hamming_fp4.hip): x_k(i) = [Z[k, i] is not the
most frequent symbol of column i], D1 = popcount(x_k xor x_l) <= d(k, l); pairs with D1 < thresh are listed and counted exactly.
Whatever the bound lists, the neighbour counts are the integers of a numpy brute force and of the exact form (HAMMING_MODE=full).

Shapes: M around the 256-row tiles and the walks of tiles (1, 2, 255, 256, 257, 513, 600), N around the 32-position words, the
8-entry chunks of the image and the 512-position strip that stays in LDS (1, 31, 32, 33, 127, 129, 255, 257; 520 and 800 take the
streamed-A form), thresholds 0, 1, N / 3, N / 2, N and N + 1.  The thresholds up to N also go through a fixed theta (compute_weights:
theta in [0, 1], thresh = floor(theta N)); N + 1 only exists as a threshold of the operator gdca_neighbour_counts."""
import os

import numpy as np
import pytest

from gdca_testutil import random_msa

pytestmark = pytest.mark.gpu

MS = (1, 2, 255, 256, 257, 513, 600)
NS = (1, 31, 32, 33, 127, 129, 255, 257)
MODES = ("mfma", "auto")


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
    c.set_options(HAMMING_MODE="auto")
    c.close()


def brute_counts(Zo, thr):
    """1 + #{l != k: d(k, l) < thr}, straight from the definition"""
    Zo = np.ascontiguousarray(Zo)
    M = Zo.shape[0]
    n = np.ones(M, dtype=np.int64)
    if thr <= 0:
        return n.astype(np.int32)
    for k0 in range(0, M, 64):
        d = (Zo[k0:k0 + 64, None, :] != Zo[None, :, :]).sum(axis=2)
        n[k0:k0 + 64] += (d < thr).sum(axis=1) - 1  # (d(k, k) = 0 < thr)
    return n.astype(np.int32)


def thresholds(N):
    return sorted({0, 1, N // 3, N // 2, N, N + 1})


def check(g, ctx, Zo, thrs, what, modes=MODES):
    Z = np.asfortranarray(Zo.T)
    try:
        for thr in thrs:
            want = brute_counts(Zo, thr)
            ctx.set_option("HAMMING_MODE", "full")
            assert np.array_equal(g.neighbour_counts(Z, thr, ctx=ctx), want), (what, "full", thr)
            for mode in modes:
                ctx.set_option("HAMMING_MODE", mode)
                assert np.array_equal(g.neighbour_counts(Z, thr, ctx=ctx), want), (what, mode, thr)
    finally:
        ctx.set_option("HAMMING_MODE", "auto")


def family(N, M, seed):
    from gaussdca.jl_amd import synth

    return synth.synth_family(N, M, 21, seed)


@pytest.mark.parametrize("N", NS)
def test_counts_at_every_edge_of_words_chunks_and_tiles(g, ctx, N):
    for M in MS:
        check(g, ctx, family(N, M, 0xC0 + 7 * N + M), thresholds(N), (N, M))


@pytest.mark.parametrize("N,M", [(520, 300), (800, 257)])
def test_rows_longer_than_the_resident_strip(g, ctx, N, M):
    """more than two LDS chunks per row: the A operand is streamed beside B (three and four chunks)"""
    check(g, ctx, family(N, M, 0x5A + N), (1, N // 3, N // 2, N + 1), (N, M))


@pytest.mark.parametrize("N,M", [(33, 257), (129, 513)])
def test_thresholds_through_a_fixed_theta(g, ctx, N, M):
    from oracle import gdca_oracle as o

    Zo = family(N, M, 0x7E + N)
    Z = np.asfortranarray(Zo.T)
    try:
        for thr in (0, 1, N // 3, N // 2, N):
            theta = min((thr + 0.5) / N, 1.0) if thr else 0.0
            want = 1.0 / brute_counts(Zo, thr)
            for mode in ("full",) + MODES:
                ctx.set_option("HAMMING_MODE", mode)
                W, Meff, th, got_thr = g.compute_weights(Z, 21, theta, ctx=ctx, return_theta=True)
                assert got_thr == thr == o.hamming_threshold(theta, N)
                assert np.array_equal(W, want), (N, M, thr, mode)
    finally:
        ctx.set_option("HAMMING_MODE", "auto")


def test_a_column_with_one_symbol_and_a_column_with_a_tie(g, ctx):
    """column 0 holds one symbol (its plane is +1.0 for every sequence); column 1 holds two symbols exactly half and half (sigma:
    the smaller one -- any choice lists a valid superset); column 2 a three-way tie with a rarer fourth symbol"""
    N, M = 70, 300
    Zo = family(N, M, 0x71E)
    Zo[:, 0] = 5
    Zo[:, 1] = np.where(np.arange(M) % 2 == 0, 9, 3)
    Zo[:, 2] = np.array([4, 17, 11])[np.arange(M) % 3]
    Zo[:6, 2] = 20
    check(g, ctx, Zo, (1, 2, 3, N // 3, N // 2, N), "single symbol, ties")


def test_identical_sequences_overflow_the_list_and_the_exact_form_counts(g, ctx):
    """600 copies of one sequence: all 179 700 pairs are candidates, the list holds a few thousand, nothing is dropped: n_k = M"""
    N, M = 100, 600
    Zo = np.tile(family(N, 1, 0x1D), (M, 1))
    Z = np.asfortranarray(Zo.T)
    try:
        for mode in MODES:
            ctx.set_option("HAMMING_MODE", mode)
            for thr in (1, N // 2):
                assert np.array_equal(g.neighbour_counts(Z, thr, ctx=ctx), np.full(M, M, dtype=np.int32)), (mode, thr)
    finally:
        ctx.set_option("HAMMING_MODE", "auto")


def test_unrelated_random_sequences_against_a_family(g, ctx):
    """uniform random bytes over q = 21 symbols (the consensus is nearly arbitrary, D1 is small: many candidates, few neighbours)
    and a family drawn from synth_family (most sequences share the root's symbol)"""
    rng = np.random.default_rng(31)
    N, M = 160, 520
    check(g, ctx, random_msa(rng, M, N, 21), (N // 3, N // 2, int(0.9 * N), N), "random")
    check(g, ctx, family(N, M, 0xFA3), (N // 3, N // 2, int(0.9 * N), N), "family")


def test_rows_that_are_not_dword_aligned(g, ctx):
    """N not a multiple of four: the image is built byte by byte"""
    for N, M in ((30, 260), (131, 300)):
        check(g, ctx, family(N, M, 0xA1 + N), (1, N // 3, N // 2), (N, M))


def test_the_same_call_twice_lists_the_same_pairs(g, ctx):
    Zo = family(200, 600, 0x2C7)
    Z = np.asfortranarray(Zo.T)
    try:
        ctx.set_option("HAMMING_MODE", "mfma")
        a = g.neighbour_counts(Z, 70, ctx=ctx)
        b = g.neighbour_counts(Z, 70, ctx=ctx)
    finally:
        ctx.set_option("HAMMING_MODE", "auto")
    assert np.array_equal(a, b) and np.array_equal(a, brute_counts(Zo, 70))


def test_phase_batch_of_three_unequal_families_equals_single_runs(g):
    """three families of different N and M batched by phase (one grid per kernel kind carries all three), the consensus form
    forced: the same Meff bits as their single runs, and the same Meff bits and scores as the batch under the exact form"""
    import torch

    sizes = [(100, 700), (170, 300), (260, 520)]
    fams = [family(N, M, 0xBA7 + N) for N, M in sizes]
    Zd = [torch.from_numpy(z).cuda() for z in fams]
    cs = [g.Context(0) for _ in fams]
    try:
        res = {}
        for mode in ("mfma", "full"):
            for c in cs:
                c.set_options(HAMMING_MODE=mode, PHASED_GRIDS=1)
            single = []
            for c, zd, (N, M) in zip(cs, Zd, sizes):
                S = torch.zeros((N, N), dtype=torch.float64, device="cuda")
                st = c.run_dev(zd.data_ptr(), N, M, 21, 0.8, -1.0, 0, S.data_ptr())
                single.append(st["Meff"])
            outs = [torch.zeros((N, N), dtype=torch.float64, device="cuda") for N, _ in sizes]
            g.run_dev_phased(cs, [z.data_ptr() for z in Zd], [N for N, _ in sizes], [M for _, M in sizes], [21] * len(cs), 0.8, -1.0, 0,
                             [x.data_ptr() for x in outs])
            sts = [c.collect() for c in cs]
            assert [st["Meff"] for st in sts] == single, mode
            res[mode] = ([st["Meff"] for st in sts], [x.cpu() for x in outs])
        assert res["mfma"][0] == res["full"][0]
        for a, b in zip(res["mfma"][1], res["full"][1]):
            assert torch.equal(a, b)
    finally:
        for c in cs:
            c.close()
