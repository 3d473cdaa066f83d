"""The streaming passes over the alignment in front of the big kernels -- the relayout Z -> Zt, Zc (k_relayout), the column symbol
counts of theta = :auto (k_column_hist, k_column_hist_sum) and the single-site sums with the pair tally's keep lists (k_pi_keep) --
through what the library exposes.  Every quantity here is an integer or a function of integers, so every comparison is exact
equality:

  * pair_sum = sum_i sum_a c_ia (c_ia - 1) / 2 from numpy's symbol counts, theta and thresh from it in the kernel's operation order;
  * Pi_true and Pij_true against tests/tally_model.py's integer contract, with TALLY_SKIP 0 and 1: the relayouts feed the pair tally,
    the single-site sums are Pi_true and the recovered rows, and a wrong keep list or sigma cannot give the model's bits.

Shapes: the tiles are 64 x 64 bytes with dword loads where N % 4 == 0 (N = 130, 65, 63, 17, 15, 1 are not; the "aligned" cases are),
the column blocks 16 and 32 columns, a strip of the column counts 256 columns (N = 257, 515: theta only) over chunks of at least 64
sequences (128 per pass of a workgroup), a step of k_pi_keep 8192 sequences (M = 8193 and 16385 are just past one and two)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import tally_model as tm

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
    c.set_options(TALLY_SKIP=1, TALLY_TJ=0)
    c.close()


def family(N, M, q, seed):
    """(N, M) Fortran int8 in 1..q: every column has a favoured symbol of its own weight (conserved, mixed and gapped columns)."""
    rng = np.random.default_rng(seed)
    Z = rng.integers(1, q + 1, size=(N, M))
    fav = rng.integers(1, q + 1, size=N)
    p = rng.random(N)
    hit = rng.random((N, M)) < p[:, None]
    Z = np.where(hit, fav[:, None], Z)
    return np.asfortranarray(Z.astype(np.int8))


class OnDevice:
    """Z in HBM, `offset` bytes into a larger allocation."""

    def __init__(self, g, ctx, Zf, offset=0):
        self.N, self.M = Zf.shape
        self.buf = g._lib.DeviceBuffer(ctx, self.N * self.M + 16)
        self.buf.upload(np.ascontiguousarray(Zf.T), offset=offset)   # (M, N) row-major: sequence k at k * N
        self.ptr = self.buf.ptr + offset


def theta_model(Zf):
    """(pair_sum, theta, thresh) of theta = :auto: the counts of byte & 31 per column, then k_theta_finalize's expression."""
    N, M = Zf.shape
    tot = 0
    for i in range(N):
        c = np.bincount(Zf[i].astype(np.uint8) & 31, minlength=32).astype(object)
        tot += int(sum(int(x) * (int(x) - 1) // 2 for x in c))
    if M < 2:
        theta = 0.0
    else:
        with np.errstate(divide="ignore"):
            phi = np.float64(tot) / (np.float64(N) * (np.float64(0.5) * np.float64(M) * np.float64(M - 1)))
            t = np.float64(0.38 * 0.32) / phi
        theta = float(t) if t < 0.5 else 0.5
    return tot, theta, int(math.floor(theta * N))


def device_theta(ctx, dev):
    from gaussdca.jl_amd import devops

    ps = C.c_uint64()
    ctx.check(ctx.lib.gdca_pair_identity_sum_dev(ctx.h, C.c_void_p(dev.ptr), dev.N, dev.M, C.byref(ps)))
    dW, Meff, theta, thresh = devops.compute_weights_dev(ctx, dev.ptr, dev.N, dev.M, ":auto")
    return int(ps.value), theta, thresh, dW, Meff


def device_frequencies(ctx, dev, q, dW, Meff, skip):
    from gaussdca.jl_amd import devops

    n = dev.N * (q - 1)
    ctx.set_options(TALLY_SKIP=skip)
    dPi, dPij = devops.compute_weighted_frequencies_dev(ctx, dev.ptr, dev.N, dev.M, q, dW, Meff)
    return dPi.download((n,)), dPij.download((n, n))


def assert_frequencies(ctx, dev, Zf, q, dW, W, Meff, label):
    """Pi_true and Pij_true of both tally forms against the integer model (computed once)."""
    N, M = Zf.shape
    shift = tm.fix_shift(M)
    Pifix, H = tm.tallies(Zf, tm.wfix(W, shift), q)
    Pi_m, Pij_m = tm.to_frequency(Pifix.reshape(-1), shift, Meff), tm.to_frequency(H, shift, Meff)
    out = []
    for skip in (0, 1):
        Pi, Pij = device_frequencies(ctx, dev, q, dW, Meff, skip)
        msg = tm.first_mismatch(Pi, Pi_m, Pifix.reshape(-1), shift, Meff, q - 1)
        assert msg is None, "%s TALLY_SKIP=%d Pi: %s" % (label, skip, msg)
        msg = tm.first_mismatch(Pij, Pij_m, H, shift, Meff, q - 1)
        assert msg is None, "%s TALLY_SKIP=%d Pij: %s" % (label, skip, msg)
        out.append((Pi, Pij))
    return out


def check_pipeline(g, ctx, Zf, q, label, offset=0):
    """theta = :auto, the device's own weights, then both tally forms"""
    dev = OnDevice(g, ctx, Zf, offset)
    ps, theta, thresh, dW, Meff = device_theta(ctx, dev)
    assert (ps, theta, thresh) == theta_model(Zf), label
    W = dW.download((dev.M,))
    return (ps, theta, thresh, W, Meff), assert_frequencies(ctx, dev, Zf, q, dW, W, Meff, label)


def check_given_weights(g, ctx, Zf, q, W, label):
    dev = OnDevice(g, ctx, Zf)
    dW = g._lib.DeviceBuffer.from_array(ctx, np.ascontiguousarray(W, dtype=np.float64))
    return assert_frequencies(ctx, dev, Zf, q, dW, W, math.fsum(W), label)


GRID = [(N, M, 21) for N in (1, 15, 17, 63, 65, 130) for M in (1, 2, 63, 257, 4097)] + [(17, 257, 5), (17, 257, 31), (17, 8193, 21), (17, 16385, 21)]


@pytest.mark.parametrize("N,M,q", GRID, ids=["N%d-M%d-q%d" % c for c in GRID])
def test_theta_and_frequencies_on_the_grid(g, ctx, N, M, q):
    check_pipeline(g, ctx, family(N, M, q, 1000 * N + M + q), q, "N=%d M=%d q=%d" % (N, M, q))


@pytest.mark.parametrize("N,M,q", [(64, 64, 21), (64, 4100, 21), (128, 260, 21), (32, 1028, 31)], ids=lambda v: str(v))
def test_theta_and_frequencies_where_the_wide_loads_apply(g, ctx, N, M, q):
    """N % 4 == 0 and M % 4 == 0 on the context's aligned buffers: dword loads of Z, dword stores and loads of Zt."""
    check_pipeline(g, ctx, family(N, M, q, 77 + N + M), q, "N=%d M=%d q=%d" % (N, M, q))


@pytest.mark.parametrize("N,M", [(257, 63), (257, 4097), (515, 257), (516, 4097)], ids=lambda v: str(v))
def test_theta_across_strips_of_256_columns(g, ctx, N, M):
    """The column counts beyond one strip (theta only: Pij of 515 columns would be 850 MB)."""
    Zf = family(N, M, 21, 31 * N + M)
    dev = OnDevice(g, ctx, Zf)
    ps, theta, thresh, _, _ = device_theta(ctx, dev)
    assert (ps, theta, thresh) == theta_model(Zf)


def named_family(N, M, q, seed):
    """column 0: a single symbol (empty keep list, sigma that symbol); 1: all gaps (sigma = q); 2: two symbols that tie at equal
    weights where M is even (sigma the smaller one), 3: three symbols, the two largest tie where M % 5 == 0."""
    Zf = family(N, M, q, seed)
    k = np.arange(M)
    Zf[0] = 7 if q > 7 else 2
    Zf[1] = q
    Zf[2] = np.where(k % 2 == 0, 9, 4) if q > 9 else np.where(k % 2 == 0, 3, 2)
    Zf[3] = np.array([2, 1, 1, 2, 3], dtype=np.int8)[k % 5]
    return Zf


@pytest.mark.parametrize("N,M,q", [(9, 4096, 21), (9, 600, 5), (21, 1000, 31)], ids=lambda v: str(v))
def test_named_columns_with_equal_weights(g, ctx, N, M, q):
    """All weights 1: with M = 4096 the single-symbol column's sum is exactly 2^63 and the skip form's recovery is exact modulo 2^64
    (the model holds the same u64)."""
    Zf = named_family(N, M, q, 5 + M)
    c2 = np.sort(np.bincount(Zf[2], minlength=32))
    assert M % 2 == 0 and c2[-1] == c2[-2] == M // 2, "column 2 is a true tie"
    W = np.ones(M)
    if M == 4096:
        shift = tm.fix_shift(M)
        assert int(tm.tallies(Zf[:1], tm.wfix(W, shift), q)[0].max()) == 1 << 63
    check_given_weights(g, ctx, Zf, q, W, "named N=%d M=%d q=%d" % (N, M, q))
    check_pipeline(g, ctx, Zf, q, "named (device weights) N=%d M=%d q=%d" % (N, M, q))


@pytest.mark.parametrize("N,M", [(130, 257), (17, 4097), (64, 260)], ids=lambda v: str(v))
def test_unaligned_device_pointer_gives_the_aligned_results(g, ctx, N, M):
    """Z_dev 1 and 3 bytes into a larger allocation: no wide load may assume alignment."""
    Zf = family(N, M, 21, 9 * N + M)
    want = check_pipeline(g, ctx, Zf, 21, "aligned")
    for off in (1, 3):
        got = check_pipeline(g, ctx, Zf, 21, "offset %d" % off, offset=off)
        assert got[0][:3] == want[0][:3] and got[0][4] == want[0][4] and np.array_equal(got[0][3], want[0][3]), off
        for (Pi, Pij), (Pi0, Pij0) in zip(got[1], want[1]):
            assert np.array_equal(Pi, Pi0) and np.array_equal(Pij, Pij0), off


# What the parent commit answers for a byte outside the alphabet, recorded here: the weights of the operator path check against the
# largest alphabet (1..31: a byte 22 passes there, 0 and -1 do not), the frequencies and the fused run against 1..q.
@pytest.mark.parametrize("byte,weights_ok", [(0, False), (22, True), (-1, False)], ids=["zero", "q+1", "minus-one"])
@pytest.mark.parametrize("skip", [0, 1])
def test_a_byte_outside_the_alphabet(g, ctx, byte, weights_ok, skip):
    from gaussdca.jl_amd import devops

    N, M, q = 17, 257, 21
    Zf = family(N, M, q, 4242)
    good = OnDevice(g, ctx, Zf)
    dW, Meff, _, _ = devops.compute_weights_dev(ctx, good.ptr, N, M, ":auto")
    Zf[11, 200] = byte
    dev = OnDevice(g, ctx, Zf)
    if weights_ok:
        devops.compute_weights_dev(ctx, dev.ptr, N, M, ":auto")
    else:
        with pytest.raises(g.ArgumentError, match="symbol outside 1..q"):
            devops.compute_weights_dev(ctx, dev.ptr, N, M, ":auto")
    ctx.set_options(TALLY_SKIP=skip)
    try:
        with pytest.raises(g.ArgumentError, match="symbol outside 1..q"):
            devops.compute_weighted_frequencies_dev(ctx, dev.ptr, N, M, q, dW, Meff)
        with pytest.raises(g.ArgumentError, match="symbol outside 1..q"):
            ctx.run(Zf, q, 0.8, -1.0, 0)
        # the context is as good as before: the clean family still gives the model's bits
        Pi, _ = device_frequencies(ctx, good, q, dW, Meff, skip)
        assert np.isfinite(Pi).all()
    finally:
        ctx.set_options(TALLY_SKIP=1)
