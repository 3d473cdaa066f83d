"""The exact tally model (tests/tally_model.py) held to its own definition, without a GPU: the limb/BLAS form against the
Python-integer form, the fixed-point shift at its steps, the column-sum identity the skip form's recovery rests on (with a sum of
exactly 2^63), and -- on every family of the grid the GPU module runs -- the model inside the derived bound against the true sums."""
from fractions import Fraction

import numpy as np
import pytest

import tally_cases
import tally_model as tm


@pytest.mark.parametrize("M,want", [(1, 58), (2, 58), (32, 58), (33, 57), (64, 57), (65, 56), (2 ** 20, 43), (2 ** 20 + 1, 42)])
def test_fix_shift_steps(M, want):
    sh = tm.fix_shift(M)
    assert sh == want
    assert (M << sh) <= (1 << 63) and sh <= 58 and (sh == 58 or (M << (sh + 1)) > (1 << 63))


def test_wfix_rounds_half_to_even():
    u = np.array([0.5, 0.25, 1.5, 1.0, 2.5, 0.75, 0.0, 3.5])
    assert tm.wfix(np.ldexp(u, -58), 58).tolist() == [0, 0, 2, 1, 2, 1, 0, 4]
    assert tm.wfix(np.array([1.0]), 58).tolist() == [1 << 58]
    # a weight with bits below the resolution on both sides of a half
    assert tm.wfix(np.array([np.ldexp(1.5, -58) * (1 + 2.0 ** -52), np.ldexp(1.5, -58) * (1 - 2.0 ** -52)]), 58).tolist() == [2, 1]


@pytest.mark.parametrize("name", ["chunk-M17", "ones-M64", "w-sub-resolution", "w-zero-third", "q3", "q31", "cols-N17"])
def test_fast_form_equals_python_integers(name):
    Z, q, W, Meff = tally_cases.GRID[name]()
    N, M = Z.shape
    s = q - 1
    shift = tm.fix_shift(M)
    Wf = tm.wfix(W, shift)
    Pifix, H = tm.tallies(Z, Wf, q)
    rng = np.random.default_rng(1)
    pairs = {(0, 0), (0, N - 1), (N - 1, N - 1)} | {tuple(int(x) for x in rng.integers(0, N, size=2)) for _ in range(12)}
    for i, j in sorted(pairs):
        D = tm.pair_tally_direct(Z, Wf, q, i, j)
        assert [[int(x) for x in row] for row in H[i * s:(i + 1) * s, j * s:(j + 1) * s]] == D, (i, j)
        assert [[int(x) for x in row] for row in tm.pair_tally(Z, Wf, q, i, j)] == D, (i, j)
        if i == j:
            assert [int(x) for x in Pifix[i]] == [D[a][a] for a in range(s)]
            assert all(D[a][b] == 0 for a in range(s) for b in range(s) if a != b)
    assert np.array_equal(H, H.T)


@pytest.mark.parametrize("name", ["ones-M32", "ones-M64", "ones-M1024", "ones-M33", "w-one-over-n", "q2", "kept-1"])
def test_column_sums_are_the_single_site_sums(name):
    """sum over a in 1..q-1 of H[(i,a),(j,b)], plus the gap's row, is Pifix[j][b]: what the recovery subtracts from.  With all
    weights 1 and M a power of two the single-symbol column's sum is exactly 2^63."""
    Z, q, W, Meff = tally_cases.GRID[name]()
    N, M = Z.shape
    shift = tm.fix_shift(M)
    Wf = tm.wfix(W, shift)
    Pifix, H = tm.tallies(Z, Wf, q)
    Pg, Hg = tm.tallies(Z, Wf, q, with_gap=True)
    s = q - 1
    assert np.array_equal(Pg[:, :s], Pifix)
    Hg4 = Hg.reshape(N, q, N, q)
    assert np.array_equal(Hg4[:, :s, :, :s].reshape(N * s, N * s), H)
    for i in range(N):
        for j in range(N):
            for b in range(s):
                col = sum(int(x) for x in Hg4[i, :s, j, b]) + int(Hg4[i, s, j, b])
                assert col == int(Pifix[j, b]), (i, j, b)
    if name.startswith("ones-M") and M & (M - 1) == 0:
        assert int(Pifix[0, 2]) == 1 << 63      # column 0 holds symbol 3 everywhere
        assert tm.to_frequency(Pifix[0, 2], shift, Meff) == 1.0


def test_kept_list_families_have_the_length_they_name():
    for name, L in [("kept-%d" % L, L) for L in (0, 1, 1023, 1024, 1025, 2048)] + [("kept-1025-last", 1025)]:
        Z, q, W, Meff = tally_cases.GRID[name]()
        n, sigma = tally_cases.kept_length(Z, tm.wfix(W, tm.fix_shift(Z.shape[1])), q, tally_cases.KEPT_COL)
        assert (n, sigma) == (L, tally_cases.SYM), name
    Z, q, W, Meff = tally_cases.GRID["kept-1025-last"]()
    assert np.all(Z[tally_cases.KEPT_COL, :-1025] == tally_cases.SYM) and np.all(Z[tally_cases.KEPT_COL, -1025:] != tally_cases.SYM)
    for name in ("step-M8193", "step-M12289"):
        Z, q, W, Meff = tally_cases.GRID[name]()
        M = Z.shape[1]
        n, sigma = tally_cases.kept_length(Z, tm.wfix(W, tm.fix_shift(M)), q, tally_cases.KEPT_COL)
        first = ((M - 1) // 4096) * 4096
        assert sigma == tally_cases.SYM and n == M - first and np.all(Z[tally_cases.KEPT_COL, first:] != tally_cases.SYM)
    # the symbol with the largest count is not the one with the largest weighted sum
    Z, q, W, Meff = tally_cases.GRID["w-count-vs-weight"]()
    col = Z[tally_cases.KEPT_COL]
    assert np.count_nonzero(col == tally_cases.SYM) > np.count_nonzero(col == tally_cases.SYM + 2)
    assert tally_cases.kept_length(Z, tm.wfix(W, tm.fix_shift(Z.shape[1])), q, tally_cases.KEPT_COL)[1] == tally_cases.SYM + 2
    # two symbols of column 3 tie exactly
    Z, q, W, Meff = tally_cases.GRID["w-tie"]()
    Pifix, _ = tm.tallies(Z, tm.wfix(W, tm.fix_shift(Z.shape[1])), q)
    assert int(Pifix[3, 1]) == int(Pifix[3, 4]) > 0
    Z, q, W, Meff = tally_cases.GRID["w-zero-third"]()
    Pifix, H = tm.tallies(Z, tm.wfix(W, tm.fix_shift(Z.shape[1])), q)
    r = tally_cases.KEPT_COL * (q - 1) + tally_cases.SYM - 1
    assert np.count_nonzero(Z[tally_cases.KEPT_COL] == tally_cases.SYM) > 0 and not H[r].any()


def check_bound(name, Pi, Pij, Z, q, W, Meff):
    """Pi, Pij (f64) against the true sums: inside `bound` everywhere."""
    shift = tm.fix_shift(Z.shape[1])
    Pi_x, Pij_x, cnt_i, cnt_ij = tm.exact_frequencies(Z, W, Meff, q)
    for got, ref, cnt in ((Pi, Pi_x, cnt_i), (Pij, Pij_x, cnt_ij)):
        err = np.abs(got.astype(np.longdouble) - ref)
        lim = tm.bound(cnt, shift, Meff, got)
        over = err > lim
        assert not over.any(), "%s: %d entries outside the bound, worst %.3g x the bound at %s" % (
            name, int(over.sum()), float((err / np.maximum(lim, np.finfo(np.float64).tiny)).max()),
            np.unravel_index(int(np.argmax(err - lim)), err.shape))


@pytest.mark.parametrize("name", list(tally_cases.GRID))
def test_model_is_inside_the_derived_bound(name):
    Z, q, W, Meff = tally_cases.GRID[name]()
    Pi, Pij = tm.frequencies(Z, W, Meff, q)
    assert np.array_equal(Pij, Pij.T)
    check_bound(name, Pi, Pij, Z, q, W, Meff)
    # the long-double reference against the definition in rational arithmetic, on a few cells
    N, M = Z.shape
    s = q - 1
    _, Pij_x, _, _ = tm.exact_frequencies(Z, W, Meff, q)
    rng = np.random.default_rng(len(name))
    for _ in range(4 if M <= 1100 else 1):
        i, j = (int(x) for x in rng.integers(0, N, size=2))
        a, b = (int(x) for x in rng.integers(1, s + 1, size=2))
        want = tm.exact_cell(Z, W, Meff, q, i, a, j, b)
        got = Fraction(float(Pij_x[i * s + a - 1, j * s + b - 1]))   # (the f64 nearest the long double value)
        assert abs(got - want) <= Fraction(1, 2 ** 52) * want, (name, i, a, j, b)


def test_the_bound_sees_a_truncated_weight_conversion():
    """The bound is not slack: floor instead of rint in the weight conversion leaves it (each weight then errs by up to a whole
    unit, in one direction)."""
    Z, q, W, Meff = tally_cases.GRID["w-one-over-n"]()
    shift = tm.fix_shift(Z.shape[1])
    Pifix, H = tm.tallies(Z, np.floor(np.ldexp(W, shift)).astype(np.uint64), q)
    with pytest.raises(AssertionError):
        check_bound("floor", tm.to_frequency(Pifix.reshape(-1), shift, Meff), tm.to_frequency(H, shift, Meff), Z, q, W, Meff)
