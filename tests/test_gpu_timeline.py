"""The stage times of gdca_stats (include/gdca.h) as relations between them.  Every ms_* is the device time between two named
boundaries of the run's timeline (DESIGN.md "The timeline of a run"), marked by one of two clocks -- HIP events, or the device
time stamps of a batch issued as batched grids -- and an interval is only ever formed from two ends of one clock.  So intervals
nested in another can never sum to more than it, a stage the run does not have reports exactly 0, and the launch accounting
(update_launches, inverse_batch) adds up -- for single runs, the members of a phase batch in either form, and gdca_run_multi.
(The retried run is in test_gpu_parity.py, which already forces the retry.)

The 1e-3 ms slack: the times are floats of millisecond magnitude below 1e3 (checked), six of them in the longest sum."""
import os
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FROB, DI = 0, 1
SLACK = 1e-3
STAGES = ("ms_theta", "ms_weights", "ms_covariance", "ms_inverse", "ms_inverse_update", "ms_score")


@pytest.fixture(scope="module")
def g():
    import gaussdca.jl_amd as g

    assert os.path.exists(g._lib.LIB_PATH), "libgdca.so missing: the GPU tests never fall back to the CPU"
    assert g.load().gdca_device_count() > 0, "no HIP device"
    return g


@pytest.fixture(scope="module")
def fams():
    from gaussdca.jl_amd import synth

    return {(N, M): synth.synth_family(N, M, 21, 0x71 + N) for N, M in ((40, 500), (64, 64), (130, 2000))}   # (M, N) int8 each


def _check_single(st, score, tally=True):
    print({k: v for k, v in st.items() if k.startswith("ms_")})
    for key in STAGES + ("ms_total",):
        assert 0.0 < st[key] < 1e3, (key, st[key])
    assert st["ms_theta"] + st["ms_weights"] + st["ms_covariance"] + st["ms_inverse"] + st["ms_score"] <= st["ms_total"] + SLACK, st
    assert st["ms_inverse_update"] <= st["ms_inverse"] + SLACK, st
    if score == FROB:
        assert 0.0 < st["ms_fn"] <= st["ms_score"] + SLACK, st
    else:
        assert st["ms_fn"] == 0.0, st
    if tally:
        assert 0.0 < st["ms_pair_tally"] <= st["ms_covariance"] + SLACK, st
    else:
        assert st["ms_pair_tally"] == 0.0, st
    assert st["update_launches"] == 1 and st["inverse_batch"] == 1, st


@pytest.mark.parametrize("N,M", [(40, 500), (130, 2000)])
def test_single_runs(g, fams, N, M):
    Zf = np.asfortranarray(fams[(N, M)].T)
    c = g.Context(0)
    try:
        for score in (FROB, DI, FROB):                       # (... a second and third run on the same context: its events are reused)
            _, st = c.run(Zf, 21, 0.8, -1.0, score)
            _check_single(st, score)
        c.set_options(REFINE=0)                              # no conditioning screen: the pair tally is not the timed first build
        _, st = c.run(Zf, 21, 0.8, -1.0, FROB)
        _check_single(st, FROB, tally=False)
    finally:
        c.close()


@pytest.mark.parametrize("grids", [1, 0])
def test_phase_batch(g, fams, grids):
    import torch

    sizes = [(40, 500), (64, 64), (130, 2000)]
    Zd = [torch.from_numpy(fams[s]).cuda() for s in sizes]
    cs = [g.Context(0) for _ in sizes]
    try:
        cs[0].set_options(PHASED_GRIDS=grids)
        for score in (FROB, DI):
            outs = [torch.zeros((N, N), dtype=torch.float64, device="cuda") for N, _ in sizes]
            g.run_dev_phased(cs, [z.data_ptr() for z in Zd], [N for N, _ in sizes], [M for _, M in sizes], [21] * len(sizes), 0.8, -1.0, score,
                             [x.data_ptr() for x in outs])
            sts = [c.collect() for c in cs]
            for k, st in enumerate(sts):
                print(grids, score, k, {key: v for key, v in st.items() if key.startswith("ms_")}, st["inverse_batch"], st["update_launches"])
                for key in STAGES:
                    assert 0.0 < st[key] < 1e3, (grids, k, key, st[key])
                assert st["ms_inverse_update"] <= st["ms_inverse"] + SLACK, (grids, k, st)
                assert st["ms_fn"] <= st["ms_score"] + SLACK, (grids, k, st)
                assert st["ms_total"] >= st["ms_inverse"], (grids, k, st)
                assert st["info"] == 0
            # a launch is accounted for once: by its only member, or by the first of those that shared it
            launches = sum(Fraction(1, st["inverse_batch"]) for st in sts)
            assert launches.denominator == 1 and sum(st["update_launches"] for st in sts) == launches, [(st["inverse_batch"], st["update_launches"]) for st in sts]
    finally:
        for c in cs:
            c.close()


def test_run_multi(g, fams):
    """The stats rules of gdca_run_multi (gdca.h): the front end ran once, its tallies are not the timed fused build, and a group's
    further member is scored behind the first."""
    Zf = np.asfortranarray(fams[(40, 500)].T)
    c = g.Context(0)
    try:
        res = c.run_multi(Zf, 21, [(0.8, FROB), (0.2, DI), (0.8, DI)], -1.0)
        sts = [st for _, st in res]
        for k, st in enumerate(sts):
            print(k, {key: v for key, v in st.items() if key.startswith("ms_")})
        assert len({(st["ms_theta"], st["ms_weights"]) for st in sts}) == 1 and sts[0]["ms_theta"] > 0.0 and sts[0]["ms_weights"] > 0.0
        assert all(st["ms_pair_tally"] == 0.0 for st in sts)
        first, second = sts[0], sts[2]                       # the group of pseudocount 0.8
        assert second["ms_score"] > 0.0 and second["ms_total"] >= first["ms_total"], (first, second)
        assert first["ms_fn"] > 0.0 and second["ms_fn"] == 0.0 and sts[1]["ms_fn"] == 0.0   # (FROB, DI, DI)
        for st in sts:
            assert st["ms_inverse"] + st["ms_score"] <= st["ms_total"] + SLACK, st
    finally:
        c.close()
