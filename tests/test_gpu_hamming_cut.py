"""The two-phase form of the three-plane Hamming bound (csrc/k_hamming.hip): dense over the words 0 .. cut - 1, then
the pairs still below the threshold go into lists in LDS and only those are walked to the end.  Whatever the cut -- every word
from 1 to NW + 1, and the automatic choice -- the listed pairs are the same set, so the neighbour counts are the oracle's integers.
Shapes: the smallest at which each piece of the index arithmetic can go wrong (a single chunk, a two-word last chunk, a cut on and
across a chunk boundary, ragged M, padding bits, diagonal tiles alone, lists that overflow, lists that stay empty)."""
import os

import numpy as np
import pytest

from gdca_testutil import random_msa

pytestmark = pytest.mark.gpu


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
    c.set_options(HAM_CUT=0, HAMMING_MODE="auto")
    c.close()


@pytest.fixture(scope="module")
def o():
    from oracle import gdca_oracle as o

    return o


def _check(g, ctx, o, Zo, thr, cuts, what, modes=("bound", "auto"), want=None):
    Z = np.asfortranarray(Zo.T)
    want = o.neighbour_counts(Zo, thr) if want is None else want
    try:
        for mode in modes:
            ctx.set_option("HAMMING_MODE", mode)
            for cut in cuts:
                ctx.set_option("HAM_CUT", cut)
                assert np.array_equal(g.neighbour_counts(Z, thr, ctx=ctx), want), (what, mode, "HAM_CUT", cut)
    finally:
        ctx.set_options(HAM_CUT=0, HAMMING_MODE="auto")
    return want


@pytest.mark.parametrize("N,M,thr", [(128, 300, 25), (130, 257, 30), (300, 1000, 90), (500, 2000, 174), (600, 700, 200)])
def test_every_cut_word_counts_exactly(g, ctx, o, N, M, thr):
    """NW = 4 (one chunk, ragged M, three tile rows), padding bits in the last word, NW = 10 (a two-word last chunk, the cut in
    either chunk), the benchmark's NW = 16, NW = 19 (the sparse phase crosses a chunk boundary): every HAM_CUT from 1 to NW + 1, and 0."""
    from gaussdca.jl_amd import synth

    NW = (N + 31) // 32
    _check(g, ctx, o, synth.synth_family(N, M, 21, 0xC07 + N), thr, list(range(1, NW + 2)) + [0], (N, M, thr))


def _dense_family(rng, n_unrelated=0):
    root = rng.integers(1, 21, size=300).astype(np.int8)
    dense = np.tile(root, (700, 1))
    flip = rng.random(dense.shape) < 0.05
    dense[flip] = rng.integers(1, 22, size=int(flip.sum())).astype(np.int8)
    if n_unrelated:
        dense[:n_unrelated] = random_msa(rng, n_unrelated, 300, 21)
    return dense


def test_lists_that_overflow_fall_back_to_the_dense_form(g, ctx, o):
    """700 near-copies of one root (N = 300, thr = 100): every pair is alive at every cut, every tile's lists overflow and the tile
    is finished dense; and the same family with its first 128 sequences replaced by unrelated ones, so that tiles that overflow and
    tiles that do not meet in one launch.  Nothing is dropped."""
    rng = np.random.default_rng(23)
    for name, Zo in (("dense", _dense_family(rng)), ("dense+unrelated", _dense_family(rng, 128))):
        _check(g, ctx, o, Zo, 100, (1, 5, 9, 0), name)


def test_lists_that_stay_empty_end_the_tile(g, ctx, o):
    """Unrelated sequences under a low threshold (N = 256, M = 600, thr = 20): nearly every tile ends at the switch.  And diagonal
    tiles alone, M = 128 and 129, unrelated and related."""
    from gaussdca.jl_amd import synth

    rng = np.random.default_rng(29)
    _check(g, ctx, o, random_msa(rng, 600, 256, 21), 20, range(0, 10), "unrelated")
    for M in (128, 129):
        _check(g, ctx, o, random_msa(rng, M, 256, 21), 20, range(0, 10), ("unrelated diagonal", M))
        _check(g, ctx, o, synth.synth_family(256, M, 21, 0xD1A6 + M), 90, range(0, 10), ("related diagonal", M))


def test_thresholds_around_the_partial_distances_at_the_cut(g, ctx, o):
    """Strict '<' at the switch and in the sparse phase: one N = 160, M = 400 family, every threshold from the smallest to the
    largest partial three-plane distance seen at the cut word, one below and one above."""
    from gaussdca.jl_amd import synth

    N, M = 160, 400
    Zo = synth.synth_family(N, M, 21, 0x7A2)
    low = (Zo & 7).astype(np.int16)
    for cut in (2, 4):
        part = low[:, : 32 * cut]
        d3 = np.zeros((M, M), dtype=np.int64)
        for k in range(M):
            d3[k] = (part != part[k]).sum(axis=1)
        off = d3[~np.eye(M, dtype=bool)]
        for thr in range(max(int(off.min()) - 1, 1), min(int(off.max()) + 1, N) + 1):
            _check(g, ctx, o, Zo, thr, (cut,), ("cut", cut, "thr", thr), modes=("bound",))


def test_phase_batch_with_a_forced_cut_equals_single_runs(g, ctx, o):
    """The instance that carries up to sixteen members in one grid: four small families of different N batched by phase, the cut
    forced, against their single runs -- the same Meff bits; and the batch's scores are bit for bit those of the batch without a cut."""
    import torch

    from gaussdca.jl_amd import synth

    sizes = [(100, 700), (160, 900), (230, 600), (300, 1000)]
    fams = [synth.synth_family(N, M, 21, 0xBA7 + N) for N, M in sizes]
    Zd = [torch.from_numpy(z).cuda() for z in fams]
    cs = [g.Context(0) for _ in fams]
    try:
        for c in cs:
            c.set_options(HAMMING_MODE="bound", PHASED_GRIDS=1)
        meff = []
        for c, zd, (N, M) in zip(cs, Zd, sizes):
            c.set_option("HAM_CUT", 1 << 20)
            S = torch.zeros((N, N), dtype=torch.float64, device="cuda")
            meff.append(c.run_dev(zd.data_ptr(), N, M, 21, 0.8, -1.0, 0, S.data_ptr())["Meff"])
        got = {}
        for cut in (1 << 20, 2, 3):
            for c in cs:
                c.set_option("HAM_CUT", cut)
            outs = [torch.zeros((N, N), dtype=torch.float64, device="cuda") for N, _ in sizes]
            g.run_dev_phased(cs, [z.data_ptr() for z in Zd], [N for N, _ in sizes], [M for _, M in sizes], [21] * len(cs), 0.8, -1.0, 0,
                             [x.data_ptr() for x in outs])
            sts = [c.collect() for c in cs]
            assert [st["Meff"] for st in sts] == meff, cut
            got[cut] = [x.cpu() for x in outs]
        for cut in (2, 3):
            for k in range(len(cs)):
                assert torch.equal(got[cut][k], got[1 << 20][k]), (cut, k)
    finally:
        for c in cs:
            c.close()


def test_the_same_call_twice_gives_the_same_counts(g, ctx, o):
    from gaussdca.jl_amd import synth

    Zo = synth.synth_family(300, 1500, 21, 0x2C7)
    Z = np.asfortranarray(Zo.T)
    try:
        ctx.set_options(HAMMING_MODE="bound", HAM_CUT=7)
        a = g.neighbour_counts(Z, 100, ctx=ctx)
        b = g.neighbour_counts(Z, 100, ctx=ctx)
    finally:
        ctx.set_options(HAM_CUT=0, HAMMING_MODE="auto")
    assert np.array_equal(a, b) and np.array_equal(a, o.neighbour_counts(Zo, 100))
