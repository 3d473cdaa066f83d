"""The consensus product (csrc/k_hamming_fp4.hip) over more than one walk of tiles: a workgroup walks eight 256 x 256 tiles of one
tile row, a tile's candidates wait in an LDS list for the chunk after it, and the walk's last tile is flushed behind the loop.
tests/test_gpu_hamming_consensus.py stops at M = 600 (three tiles a side, one walk); here M = 2049 and 2305 are 9 and 10 tiles a
side: a full walk of eight and a short second walk of one or two tiles in the first rows, every shorter walk below.  N = 33 is one
chunk a tile, N = 257 the resident strip with all its chunks, N = 520 the streamed-A form.  Thresholds N / 3 and N / 2 list a part
of the pairs (synth_family's clusters of 25: tiles with many candidates beside tiles with none; up to 41 000 in a tile, far more
than a tile's LDS list holds), N + 1 lists every pair, overflows the global list and must end in the exact form's counts.
At these shapes the two partial thresholds overflow the global list as well (16 146 .. 1.6 M listed pairs against 9792 and 12 160),
so those cases test the counting of everything and the fall to the exact form.  What the epilogue LISTS is tested by the cases
with planted copies and small thresholds further down, whose lists hold (asserted on the CPU from the bound's definition): every
form of the kernel, both sizes, a tile beyond its LDS list, candidates in a second walk, and the batched instance.

The neighbour counts under HAMMING_MODE=mfma and auto are the integers of the exact form (HAMMING_MODE=full)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(N, M) for N in (33, 257, 520) for M in (2049, 2305)]


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


def family(N, M, seed):
    from gaussdca.jl_amd import synth

    return synth.synth_family(N, M, 21, seed)


@pytest.mark.parametrize("N,M", SHAPES)
def test_counts_over_two_walks_equal_the_exact_form(g, ctx, N, M):
    Z = np.asfortranarray(family(N, M, 0xF4 + 3 * N + M).T)
    try:
        for thr in (N // 3, N // 2, N + 1):
            ctx.set_option("HAMMING_MODE", "full")
            want = g.neighbour_counts(Z, thr, ctx=ctx)  # (the reference of this threshold: computed once, never written to)
            want.setflags(write=False)
            assert want.shape == (M,) and want.min() >= 1
            if thr == N + 1:
                assert np.array_equal(want, np.full(M, M, dtype=want.dtype))
            for mode in ("mfma", "auto"):
                ctx.set_option("HAMMING_MODE", mode)
                assert np.array_equal(g.neighbour_counts(Z, thr, ctx=ctx), want), (N, M, thr, mode)
    finally:
        ctx.set_option("HAMMING_MODE", "auto")


def listed_by_the_bound(Zo, thr):
    """the pairs k < l the consensus bound lists, from its definition (numpy): D1 = popcount(x_k xor x_l) < thr"""
    zs = Zo & 31
    sigma = np.array([np.bincount(zs[:, i], minlength=32).argmax() for i in range(Zo.shape[1])])
    x = (zs != sigma).astype(np.float32)
    return np.triu(x @ (1 - x).T + (1 - x) @ x.T < thr, 1)


def list_capacity(M):
    t128 = (M + 127) // 128
    return 64 * t128 * (t128 + 1) // 2  # (gdca_hamming_form.h: HAM_CAND_PER_TILE pairs per 128 x 128 tile of the triangle)


LCAP = 1536  # entries of a tile's LDS list (k_hamming_fp4.hip: F4_LCAP)


def counts_equal_the_exact_form(g, ctx, Zo, thr):
    Z = np.asfortranarray(Zo.T)
    try:
        ctx.set_option("HAMMING_MODE", "full")
        want = g.neighbour_counts(Z, thr, ctx=ctx)
        for mode in ("mfma", "auto"):
            ctx.set_option("HAMMING_MODE", mode)
            assert np.array_equal(g.neighbour_counts(Z, thr, ctx=ctx), want), mode
    finally:
        ctx.set_option("HAMMING_MODE", "auto")
    return want


def test_a_tile_beyond_its_lds_list_while_the_global_list_holds(g, ctx):
    """The shapes above list more pairs than the global list holds at both partial thresholds (84 757 .. 1.6 M against 9792 and
    12 160), so their counts are the exact form's in the end.  Here the list holds and is what the counts are made from: 80 copies
    of one sequence inside one tile (3160 pairs of it, with the family's own 3188: beyond the 1536 entries of a tile's LDS list, the
    rest goes straight to the global list) and 71 copies across a tile boundary, 8387 listed pairs of 9792.  Both figures are
    checked here on the CPU from the bound's definition, so that a change of the family cannot silently empty the case."""
    N, M, thr = 257, 2049, 40
    Zo = family(N, M, 0x51DE).copy()
    Zo[300:380] = Zo[300]
    Zo[1000:1071] = Zo[1000]
    listed = listed_by_the_bound(Zo, thr)
    assert listed.sum() <= list_capacity(M)
    assert listed[256:512, 256:512].sum() > LCAP
    want = counts_equal_the_exact_form(g, ctx, Zo, thr)
    assert want[300] >= 80 and want[1000] >= 71


# (N, M, threshold): small thresholds, so that the family's own candidates and the planted copies together stay inside the global list
HELD = [(33, 2049, 3), (33, 2305, 3), (257, 2305, 30), (520, 2049, 60), (520, 2305, 60)]


@pytest.mark.parametrize("N,M,thr", HELD)
def test_held_lists_in_every_form_and_in_the_second_walk(g, ctx, N, M, thr):
    """The list holds (checked on the CPU: 4521 .. 8029 listed pairs against 9792 and 12 160), so the counts are made from what the
    epilogue listed: one chunk a tile (N = 33), the resident strip (257) and streamed A (520), nine and ten tiles a side.  Planted:
    80 copies of one sequence inside tile (1, 1) -- more than its LDS list holds, the rest goes straight to the global list -- and
    copies of another in rows 10 .. 49 and from row 2048 on, whose pairs lie in tile (0, 8): the first tile of row 0's SECOND walk
    (M = 2049: the one row of tile column 8, 40 pairs; M = 2305: 40 x 40 pairs, again beyond an LDS list) and in the one-tile
    walk (8, 8)."""
    Zo = family(N, M, 0x51DE + N).copy()
    Zo[300:380] = Zo[300]
    Zo[10:50] = Zo[10]
    Zo[2048:min(2088, M)] = Zo[10]
    listed = listed_by_the_bound(Zo, thr)
    assert listed.sum() <= list_capacity(M)
    assert listed[256:512, 256:512].sum() > LCAP
    in_second_walk = listed[0:256, 2048:].sum()
    assert in_second_walk >= 40 and (M == 2049 or in_second_walk > LCAP)
    want = counts_equal_the_exact_form(g, ctx, Zo, thr)
    assert want[300] >= 80 and want[10] >= 40 + min(2088, M) - 2048


def test_two_families_in_one_phase_batch_equal_their_single_runs(g):
    """Two different families batched by phase: one launch of the GDCA_MAXB instance carries both products.  theta is fixed at 0.1
    (thresholds 13 and 25) and copies of one sequence are planted at both ends of each family, so that the lists hold (checked on
    the CPU: 3844 of 9792 and 4069 of 12 160 pairs) and one tile of each -- (0, 7) and (0, 8), the latter in a second walk -- lists
    more than an LDS list holds: Meff of the batch is made from what the batched instance listed."""
    import torch

    from oracle import gdca_oracle as o

    theta = 0.1
    sizes = [(130, 2049), (257, 2305)]
    fams = []
    for N, M in sizes:
        Zo = family(N, M, 0xB2 + N).copy()
        Zo[10:50] = Zo[10]
        Zo[M - 40:M] = Zo[10]
        listed = listed_by_the_bound(Zo, o.hamming_threshold(theta, N))
        assert listed.sum() <= list_capacity(M)
        col0 = (M - 40) // 256 * 256  # (the tile column that holds most of the copies at the end)
        assert listed[0:256, col0:col0 + 256].sum() > LCAP
        fams.append(np.ascontiguousarray(Zo))
    Zd = [torch.from_numpy(z).cuda() for z in fams]
    cs = [g.Context(0) for _ in fams]
    try:
        # (a batch's inverses may share a merged sweep launch, whose scores are not the single launch's bits: Meff is compared with
        # the single runs, and the batch's scores with the batch under the exact form)
        res = {}
        for mode in ("mfma", "full"):
            for c in cs:
                c.set_options(HAMMING_MODE=mode, PHASED_GRIDS=1)
            single = []
            for c, zd, (N, M) in zip(cs, Zd, sizes):
                S = torch.zeros((N, N), dtype=torch.float64, device="cuda")
                st = c.run_dev(zd.data_ptr(), N, M, 21, 0.8, theta, 0, S.data_ptr())
                assert st["thresh"] == o.hamming_threshold(theta, N)
                single.append(st["Meff"])
            outs = [torch.zeros((N, N), dtype=torch.float64, device="cuda") for N, _ in sizes]
            g.run_dev_phased(cs, [z.data_ptr() for z in Zd], [N for N, _ in sizes], [M for _, M in sizes], [21] * len(cs), 0.8, theta, 0,
                             [x.data_ptr() for x in outs])
            sts = [c.collect() for c in cs]
            assert [st["Meff"] for st in sts] == single, mode
            res[mode] = (single, [x.cpu() for x in outs])
        assert res["mfma"][0] == res["full"][0]
        for a, b in zip(res["mfma"][1], res["full"][1]):
            assert torch.equal(a, b)
    finally:
        for c in cs:
            c.close()
