"""k_pair_tally's load path and grid (k_tally.hip) against the exact integer model, bit for bit, at the shapes tests/tally_cases.py's
grid does not reach:

  * the kept list's entries are loaded one staging pass ahead of the gathers they address, so a list of three passes and more has
    two entries in flight at the `nk - 1` clamp: lengths 2049, 3072, 3073, spread over the sequences and at their end;
  * in a workgroup's last pass a wave whose 64 sequences start at or behind the list's end adds nothing, and the wave that straddles
    the end stops behind the step of 16 sequences that covers it: lengths 1024 + 63, + 64, + 65, + 80, and the full loop
    (TALLY_SKIP=0) at M = 1087, 1088, 1089;
  * the grid is one line of working workgroups, column block outermost and row fastest, decoded from the linear id: more than eight
    column blocks at q = 21 (N = 129, 130, 145: the last block one, two and one column wide, its first id past a multiple of the
    eight XCDs), 18 blocks at q = 5 (N = 273), and a phase batch whose members' lines lie one behind the other in a flat grid.

Every case asks `tally_model.first_mismatch(...) is None` of Pi_true and of the whole Pij_true, under TALLY_SKIP 0 and 1 and
TALLY_TJ 16 and 32; the model imports neither the library nor the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import tally_cases
import tally_model as tm

pytestmark = pytest.mark.gpu

FROB = 0


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


def _frequencies(ctx, Zf, q, W, Meff):
    N, M = Zf.shape
    n = N * (q - 1)
    Pi = np.full(n, np.nan)
    Pij = np.full((n, n), np.nan, order="F")
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    ctx.check(ctx.lib.gdca_frequencies(ctx.h, ptr(Zf), N, M, q, ptr(W), float(Meff), ptr(Pi), ptr(Pij)))
    return Pi, Pij


def _check(ctx, name, Z, q, W, Meff, settings):
    N, M = Z.shape
    s = q - 1
    shift = tm.fix_shift(M)
    Pifix, H = tm.tallies(Z, tm.wfix(W, shift), q)
    Pi_m, Pij_m = tm.to_frequency(Pifix.reshape(-1), shift, Meff), tm.to_frequency(H, shift, Meff)
    try:
        for skip, tj in settings:
            ctx.set_options(TALLY_SKIP=skip, TALLY_TJ=tj)
            Pi, Pij = _frequencies(ctx, Z, q, W, Meff)
            label = "%s (N=%d M=%d q=%d TALLY_SKIP=%d TALLY_TJ=%d)" % (name, N, M, q, skip, tj or 16)
            msg = tm.first_mismatch(Pi, Pi_m, Pifix.reshape(-1), shift, Meff, s)
            assert msg is None, "%s Pi: %s" % (label, msg)
            msg = tm.first_mismatch(Pij, Pij_m, H, shift, Meff, s)
            assert msg is None, "%s Pij: %s" % (label, msg)
            assert np.array_equal(Pij, Pij.T), label
    finally:
        ctx.set_options(TALLY_SKIP=1, TALLY_TJ=0)


ALL = [(skip, tj) for skip in (0, 1) for tj in (0, 32)]


@pytest.mark.parametrize("where", ["spread", "last"])
@pytest.mark.parametrize("L", [2049, 3072, 3073, 1024 + 63, 1024 + 64, 1024 + 65, 1024 + 80])
def test_kept_lists_across_three_passes_and_at_the_wave_trim(g, ctx, L, where):
    Z, q, W, Meff = tally_cases._kept(L, where)
    assert Z.shape == (8, L + 777)
    length, sigma = tally_cases.kept_length(Z, tm.wfix(W, tm.fix_shift(Z.shape[1])), q, tally_cases.KEPT_COL)
    assert (length, sigma) == (L, tally_cases.SYM), "the family does not hold the kept list it is named for"
    _check(ctx, "kept-%d-%s" % (L, where), Z, q, W, Meff, ALL)


@pytest.mark.parametrize("M", [1087, 1088, 1089])
def test_full_form_at_the_wave_trim(g, ctx, M):
    Z, q, W, Meff = tally_cases._plain(M, 6)()
    _check(ctx, "trim-M%d" % M, Z, q, W, Meff, ALL)


@pytest.mark.parametrize("N,q", [(129, 21), (130, 21), (145, 21), (273, 5)])
def test_more_column_blocks_than_xcds(g, ctx, N, q):
    Z, q, W, Meff = tally_cases._plain(300, N, q=q)()
    _check(ctx, "blocks-N%d-q%d" % (N, q), Z, q, W, Meff, ALL)


def test_batched_grid_members_equal_single_runs(g, ctx):
    """A phase batch of three members of different N: each member's line of workgroups starts where the one before ends, and the
    decode is relative to the member's first block.  The single runs' tallies are the ones the model pins above (N = 130), so the
    members' scores must be theirs bit for bit.  MERGE_GROUP=1 as in test_gpu_tally_exact's phase batch."""
    import torch

    fams = [tally_cases._plain(300, N)()[:2] for N in (40, 130, 75)]
    Zd = [torch.from_numpy(np.ascontiguousarray(Z.T)).cuda() for Z, _ in fams]
    Ns, Ms, qs = [Z.shape[0] for Z, _ in fams], [Z.shape[1] for Z, _ in fams], [q for _, q in fams]
    cs = [g.Context(0) for _ in fams]
    cs[0].set_options(MERGE_GROUP=1, PHASED_GRIDS=1)
    try:
        for skip in (0, 1):
            ctx.set_options(TALLY_SKIP=skip)
            want = [ctx.run(Z, q, 0.8, -1.0, FROB)[0] for Z, q in fams]
            for c in cs:
                c.set_options(TALLY_SKIP=skip)
            outs = [torch.zeros((n, n), dtype=torch.float64, device="cuda") for n in Ns]
            torch.cuda.synchronize()
            g.run_dev_phased(cs, [z.data_ptr() for z in Zd], Ns, Ms, qs, 0.8, -1.0, FROB, [x.data_ptr() for x in outs])
            sts = [c.collect() for c in cs]
            for k in range(len(fams)):
                assert sts[k]["info"] == 0
                assert np.isfinite(want[k]).all()
                assert np.array_equal(outs[k].cpu().numpy(), want[k]), (Ns[k], skip)
    finally:
        ctx.set_options(TALLY_SKIP=1, TALLY_TJ=0)
        for c in cs:
            c.close()
