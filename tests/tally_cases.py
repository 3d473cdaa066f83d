"""The grid of families the exact-tally tests run (tests/test_tally_model_cpu.py holds the model to its reference on every one of
them without a GPU; tests/test_gpu_tally_exact.py holds the kernels to the model).  Every family sits on a boundary of k_tally.hip:
the 1024-sequence staging pass of k_pair_tally, the 4096-sequence step of k_tally_keep, the 16 / 32-column blocks, k_pi_tally's
128-column blocks, 64-sequence chunk floor and 16-way unroll, the powers of two where the fixed-point shift steps, the alphabet
sizes, and weights at the edges of the fixed-point format.

A case is (Z, q, W, Meff): Z (N, M) Fortran int8 with symbols in 1..q, W in [0, 1], Meff = the correctly rounded sum of W.
Everything is seeded; nothing here needs the library."""
import math

import numpy as np

from gdca_testutil import edge_family, random_msa

SYM = 7          # the symbol a "kept list" column holds wherever it is not kept (legal for q >= 8)
KEPT_COL = 5     # the column whose kept list has a chosen length


def _family(M, N, q, seed, edge=True):
    if edge and N >= 5:
        return edge_family(M, N, q, seed)
    rng = np.random.default_rng(seed)
    return np.asfortranarray(random_msa(rng, M, N, q=q).T)


def _weights(M, seed):
    """In [0, 1), with bits below the fixed-point resolution whatever M is (a plain 53-bit uniform draw is a multiple of 2^-53,
    which rint leaves alone at every shift >= 53, i.e. for all M <= 1024: the rounding would go unexercised)."""
    rng = np.random.default_rng(seed)
    return rng.random(M) / rng.integers(1, 64, size=M)


def _case(Z, q, W):
    W = np.ascontiguousarray(W, dtype=np.float64)
    assert Z.shape[1] == W.shape[0] and int(Z.min()) >= 1 and int(Z.max()) <= q
    return Z, q, W, math.fsum(W)


def _kept(L, where, q=21):
    """A ragged M; column KEPT_COL holds SYM in all but L sequences, whose symbols are the others (the gap included).  SYM carries
    most of the column's weight, so it is the symbol the skip form leaves out and the kept list has length exactly L."""
    M = L + 777
    Z = _family(M, 8, q, 900 + L)
    rng = np.random.default_rng(L)
    other = np.array([a for a in range(1, q + 1) if a != SYM])
    pos = {"spread": np.sort(rng.choice(M, size=L, replace=False)), "last": np.arange(M - L, M)}[where]
    Z[KEPT_COL] = SYM
    Z[KEPT_COL, pos] = other[rng.integers(0, len(other), size=L)]
    W = 0.25 + 0.75 * _weights(M, L + 1)   # bounded below: 777 sequences of SYM outweigh any other symbol's ~L/20
    return _case(Z, q, W)


def _last_step_only(M, N, seed):
    """k_tally_keep walks 4096 sequences per step: column KEPT_COL keeps sequences of the last step only."""
    Z = _family(M, N, 21, seed)
    first = ((M - 1) // 4096) * 4096
    col = Z[KEPT_COL].copy()
    col[col == SYM] = SYM + 1
    col[:first] = SYM
    Z[KEPT_COL] = col
    return _case(Z, 21, 0.25 + 0.75 * _weights(M, seed + 1))


def _ones_power_of_two(M):
    """All weights exactly 1: column 0 (one symbol everywhere) sums to M * 2^shift, which is exactly 2^63 at M = 2^k >= 32."""
    return _case(_family(M, 6, 21, 70 + M), 21, np.ones(M))


def _zero_third():
    M = 300
    Z = _family(M, 8, 21, 81)
    Z[KEPT_COL, 1::4] = SYM
    W = _weights(M, 82)
    W[::3] = 0.0
    W[Z[KEPT_COL] == SYM] = 0.0   # every sequence that carries SYM in this column: a whole histogram row is zero
    return _case(Z, 21, W)


def _sub_resolution():
    """M = 20: shift 58.  In fixed-point units these weights are 1/2, 1/4, 3/2, 1, 5/2, 3/4 and 0: rint gives 0, 0, 2, 1, 2, 1, 0
    (halves go to the even neighbour)."""
    M = 20
    u = np.array([0.5, 0.25, 1.5, 1.0, 2.5, 0.75, 0.0])
    return _case(_family(M, 7, 21, 83), 21, np.ldexp(u[np.arange(M) % len(u)], -58))


def _one_over_n():
    M = 300
    return _case(_family(M, 8, 21, 84), 21, 1.0 / np.random.default_rng(85).integers(1, M + 1, size=M))


def _weighted_tie():
    """Column 3 of the edge family alternates two symbols; with the weights equal in pairs their sums tie exactly."""
    M = 200
    return _case(_family(M, 8, 21, 86), 21, np.repeat(_weights(M // 2, 87), 2))


def _count_vs_weight():
    """Column KEPT_COL: SYM in 60 % of the sequences at weight 1/16, SYM + 2 in the others at weight 1: the largest count and the
    largest weighted sum are different symbols."""
    M = 250
    Z = _family(M, 8, 21, 88)
    many = np.arange(M) % 5 < 3
    Z[KEPT_COL] = np.where(many, SYM, SYM + 2)
    return _case(Z, 21, np.where(many, 1.0 / 16, 1.0))


def _plain(M, N, q=21, seed=None, edge=True):
    seed = 1000 * q + 7 * N + M if seed is None else seed
    return lambda: _case(_family(M, N, q, seed, edge), q, _weights(M, seed + 1))


def _no_gap_q20():
    """q = 20 with symbols 1..19 only: no gap anywhere in Z."""
    M, N = 500, 9
    Z = np.asfortranarray(random_msa(np.random.default_rng(20), M, N, q=20, gap_runs=False).T)
    assert int(Z.max()) <= 19
    return _case(Z, 20, _weights(M, 21))


GRID = {}
for _M in (1023, 1024, 1025, 2047, 2048, 2049, 3072):                # staging passes of 1024 sequences
    GRID["pass-M%d" % _M] = _plain(_M, 6)
for _L in (0, 1, 1023, 1024, 1025, 2048):                            # kept-list length of one column, M ragged
    GRID["kept-%d" % _L] = (lambda L: lambda: _kept(L, "spread"))(_L)
GRID["kept-1025-last"] = lambda: _kept(1025, "last")                # the kept sequences are the last ones: the nk - 1 clamp, high k
for _M in (4095, 4096, 4097, 8191, 8193, 12289):                     # k_tally_keep's 4096-sequence steps
    GRID["step-M%d" % _M] = (lambda M: lambda: _last_step_only(M, 20, 300 + M))(_M)
for _N in (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65):        # column blocks of 16 / 32
    GRID["cols-N%d" % _N] = _plain(300, _N)
for _N in (127, 128, 129):                                           # k_pi_tally's 128-column blocks, k_colblock's 64-column strips
    GRID["cols-q5-N%d" % _N] = _plain(300, _N, q=5)
for _M in (1, 15, 16, 17, 63, 64, 65, 127, 129):                     # k_pi_tally's chunk floor and unroll
    GRID["chunk-M%d" % _M] = _plain(_M, 7)
for _q in (2, 3, 21, 22, 24, 30, 31):                                # alphabet (q = 20 below)
    GRID["q%d" % _q] = _plain(500, 9, q=_q)
GRID["q20-nogap"] = _no_gap_q20
for _M in (32, 33, 64, 65, 1024, 1025):                              # the fixed-point shift's steps; a sum of exactly 2^63
    GRID["ones-M%d" % _M] = (lambda M: lambda: _ones_power_of_two(M))(_M)
GRID["w-zero-third"] = _zero_third
GRID["w-sub-resolution"] = _sub_resolution
GRID["w-one-over-n"] = _one_over_n
GRID["w-tie"] = _weighted_tie
GRID["w-count-vs-weight"] = _count_vs_weight

# eight families for the paths that consume the tally without exposing it: a full staging pass, a kept list that ends one past a
# pass with the clamp in use, two k_tally_keep steps plus one sequence, a column block of 32 plus one, three full blocks of 16,
# 128-column blocks plus one at q = 5, the largest alphabet and the smallest one that has scores (at q = 2 the zero-sum gauge of a
# 1 x 1 coupling block is 0 and the average-product correction divides 0 by 0: every score is NaN by definition)
CONSUMERS = ("pass-M1024", "kept-1025-last", "step-M8193", "cols-N33", "cols-N48", "cols-q5-N129", "q31", "q3")
# families that also go through the device's own weights
PIPELINE = ("pass-M2048", "cols-N17", "q31")


def kept_length(Z, Wfix, q, col):
    """(length, sigma) of the skip form's kept list of a column: the sequences whose symbol is not sigma = the argmax of the
    single-site sums over 1..q, ties to the smallest symbol."""
    sums = [sum(int(w) for w in np.asarray(Wfix)[Z[col] == a]) for a in range(1, q + 1)]
    sigma = 1 + max(range(q), key=lambda a: (sums[a], -a))
    return int(np.count_nonzero(Z[col] != sigma)), sigma
