"""A numpy model of the pair tally's skip-and-recover form (k_tally.hip, TALLY_SKIP; no GPU).  Per column i the sequences whose
symbol is sigma(i) = the argmax of the single-site fixed-point sums (ties to the smallest symbol) are left out, and histogram row
sigma(i) is rebuilt as  Pifix[j][b] - sum_{a != sigma(i)} H[a][b]  in u64 arithmetic.  The rebuilt tallies must equal the direct
ones exactly, for every column pair, the diagonal blocks included."""
import numpy as np
import pytest

U64 = np.uint64


def _fixed_weights(rng, M):
    # 2^shift fixed point with M * 2^shift <= 2^63, as gdca_fix_shift
    shift = 63 - int(np.ceil(np.log2(M)))
    w = rng.random(M)
    return np.array([int(x * 2.0 ** shift) for x in w], dtype=U64)


def _direct(Z, Wfix, q, i, j):
    H = np.zeros((q, q), dtype=U64)
    for a, b, w in zip(Z[:, i], Z[:, j], Wfix):
        H[a - 1, b - 1] += w
    return H


def _pifix(Z, Wfix, q):
    N = Z.shape[1]
    P = np.zeros((N, 32), dtype=U64)
    for i in range(N):
        for a, w in zip(Z[:, i], Wfix):
            P[i, a] += w
    return P


def _sigma(P, q):
    return int(np.argmax(P[:, 1:q + 1] if P.ndim == 2 else P[1:q + 1])) + 1  # argmax keeps the first of equal maxima


def _keep_list(Z, i, sig, q):
    # k_tally_keep: (k << 5) | Z[i,k] for every legal symbol other than sigma, ascending k
    z = Z[:, i].astype(np.int64)
    k = np.nonzero((z >= 1) & (z <= q) & (z != sig))[0]
    return (k << 5) | z[k]


def _skip_and_recover(Z, Wfix, P, q, i, j):
    sig = _sigma(P[i], q)
    H = np.zeros((q, q), dtype=U64)
    for e in _keep_list(Z, i, sig, q):
        k, a = int(e >> 5), int(e & 31)
        H[a - 1, Z[k, j] - 1] += Wfix[k]
    assert not H[sig - 1].any()
    with np.errstate(over="ignore"):
        H[sig - 1] = P[j, 1:q + 1] - (H.sum(axis=0, dtype=U64) - H[sig - 1])
    return H


def _family(rng, M, N, q):
    Z = rng.integers(1, q + 1, size=(M, N))
    Z[:, 0] = q                                                  # the gap everywhere: sigma = gap, nothing kept
    Z[:, 1] = 4                                                  # one symbol everywhere: an empty kept list
    Z[:, 2] = np.where(rng.random(M) < 0.6, q, Z[:, 2])          # the gap most frequent
    Z[:, 3] = np.where(rng.random(M) < 0.5, 2, 3)
    return Z


@pytest.mark.parametrize("M,N,q", [(1037, 19, 21), (3001, 13, 21), (517, 11, 5), (260, 9, 31)])
def test_recovered_tallies_equal_direct(M, N, q):
    rng = np.random.default_rng(M + N)
    Z = _family(rng, M, N, q)
    Wfix = _fixed_weights(rng, M)
    P = _pifix(Z, Wfix, q)
    assert _sigma(P[0], q) == q and len(_keep_list(Z, 0, q, q)) == 0
    assert len(_keep_list(Z, 1, _sigma(P[1], q), q)) == 0
    assert _sigma(P[2], q) == q
    for i in range(N):
        for j in range(i, N):
            assert np.array_equal(_skip_and_recover(Z, Wfix, P, q, i, j), _direct(Z, Wfix, q, i, j)), (i, j)


def test_ties_go_to_the_smallest_symbol():
    # equal weights, equal counts of 2 and 7: sigma = 2 -- and the recovery is exact whichever symbol is skipped
    M, q = 64, 21
    Z = np.stack([np.where(np.arange(M) % 2 == 0, 7, 2), np.arange(M) % q + 1], axis=1)
    Wfix = np.full(M, 1 << 40, dtype=U64)
    P = _pifix(Z, Wfix, q)
    assert _sigma(P[0], q) == 2
    for i in range(2):
        for j in range(i, 2):
            assert np.array_equal(_skip_and_recover(Z, Wfix, P, q, i, j), _direct(Z, Wfix, q, i, j))


def test_share_of_kept_sequences_on_a_synthetic_family():
    # what the skip form saves on a family like the benchmark's (random_msa: cluster centres + mutation + gap runs)
    from gdca_testutil import random_msa

    rng = np.random.default_rng(0)
    Z = random_msa(rng, 2000, 60, q=21).astype(np.int64)
    W = np.ones(Z.shape[0], dtype=U64)
    P = _pifix(Z, W, 21)
    kept = np.mean([len(_keep_list(Z, i, _sigma(P[i], 21), 21)) for i in range(Z.shape[1])]) / Z.shape[0]
    assert 0.0 < kept < 0.8, kept
