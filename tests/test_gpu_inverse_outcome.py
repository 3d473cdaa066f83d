"""The operator-level inverses walk one recovery ladder (gdca_api.hip: inverse_ladder): a member of
gdca_spd_inverse_batch_dev has the bits of a gdca_spd_inverse_dev call of its own -- the inverse, info, the log det and its source --
with the switches at their defaults, with the Newton-Schulz step forced (REFINE=1) and with the Cholesky fallback forced (CHOLESKY=2).

n = 130 and n = 257 are two and three 128-blocks, the last one ragged: the smallest matrices at which the ladder sees more than one
block and a padded tail.  The batch carries K = 3 members (130, 257 and 130 again) on three contexts; with the default options all
three share one merged launch."""
import ctypes

import numpy as np
import pytest

import logdet_model as lm
from gdca_testutil import g  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SIZES = (130, 257, 130)


def matrix(n):
    return lm.random_spd(n, seed=9000 + n)  # B B' + n I: cond of a few


def contexts(g, k, switch):
    cs = [g.Context(0) for _ in range(k)]
    if switch:
        for c in cs:
            c.set_option(*switch)
    return cs


def on_device(C):
    import torch

    d = torch.from_numpy(np.asfortranarray(C).ravel(order="F").copy()).cuda()
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("switch", [None, ("REFINE", 1), ("CHOLESKY", 2)], ids=["default", "REFINE=1", "CHOLESKY=2"])
def test_batch_members_have_the_bits_of_calls_of_their_own(g, switch):
    single = {}
    for n in sorted(set(SIZES)):
        (c,) = contexts(g, 1, switch)
        try:
            d = on_device(matrix(n))
            info = ctypes.c_int32(-1)
            c.check(c.lib.gdca_spd_inverse_dev(c.h, ctypes.c_void_p(d.data_ptr()), n, ctypes.byref(info)), info.value)
            single[n] = (d.cpu().numpy(), info.value, c.last_logdet(return_source=True))
        finally:
            c.close()
    cs = contexts(g, len(SIZES), switch)
    try:
        bufs = [on_device(matrix(n)) for n in SIZES]
        infos = g.spd_inverse_batch_dev(cs, [b.data_ptr() for b in bufs], list(SIZES))
        for k, n in enumerate(SIZES):
            X, info, (ld, src) = single[n]
            got_ld, got_src = cs[k].last_logdet(return_source=True)
            print("member %d n=%d: info %d, logdet %+.17e (source %d), its own call's %+.17e (source %d)" % (k, n, infos[k], got_ld, got_src, ld, src))
            assert infos[k] == info == 0
            assert np.array_equal(bufs[k].cpu().numpy(), X), (k, n)
            assert (got_ld, got_src) == (ld, src), (k, n)
            assert src == (1 if switch == ("CHOLESKY", 2) else 0) and np.isfinite(ld)
            # (an inverse at all: the matrix is well conditioned)
            assert np.allclose(X.reshape((n, n), order="F") @ matrix(n), np.eye(n), atol=1e-9)
    finally:
        for c in cs:
            c.close()
