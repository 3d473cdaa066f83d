"""tests/inverse_model.py holds what it claims, on the host: the family's inverse is exact for LAPACK itself, the intermediates of a
sweep stay far inside the exactness condition, and dpotrf reports a bad pivot where the model put it."""
import numpy as np
import pytest

import inverse_model as im
from oracle import gdca_oracle as o

SIZES = (129, 300, 1100)


@pytest.mark.parametrize("n", SIZES)
def test_the_family_is_exact_and_lapack_returns_its_inverse_bit_for_bit(n):
    A, X, E, e = im.integer_family(n, 7000 + n)
    assert np.array_equal(np.tril(E, -1), E) and set(np.unique(E)) <= {-1, 0, 1}
    idx = np.arange(n)
    assert not E[idx % 32 < 16, :].any() and not E[:, idx % 32 >= 16].any()
    m = im.sweep_growth(A, X)
    print("n=%d: max|A| %d, max|X| %d, largest intermediate %d, zeros of X %.0f %%, cond %.3g" %
          (n, np.abs(A).max(), np.abs(X).max(), m, 100.0 * np.mean(X == 0), np.linalg.cond(A.astype(np.float64))))
    assert m <= n + 2 and im.exact_condition(m)
    As, Xs, e2 = im.family(n)
    assert np.array_equal(e2, e) and e.min() >= -4 and e.max() <= 4
    assert np.array_equal(As, np.ldexp(A.astype(np.float64), e[:, None] + e[None, :]))
    assert np.array_equal(As, As.T) and np.array_equal(Xs, Xs.T)
    assert np.array_equal(As @ Xs, np.eye(n))
    assert np.array_equal(o.spd_inverse(As), Xs)
    Au, Xu, eu = im.exact_family(n, 7000 + n, scaled=False)
    assert not eu.any() and np.array_equal(Au, A) and np.array_equal(Xu, X)


def test_exact_condition_is_the_stated_inequality():
    assert im.exact_condition(4194303) and not im.exact_condition(4194304)   # 512 m^2 < 2^53  <=>  m < 2^22
    assert im.exact_condition(7702)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["neg", "zero"])
def test_lapack_reports_the_bad_pivot_where_the_model_put_it(n, kind):
    As, _, e = im.family(n)
    pos = im.positions(n)
    nblk = (n + 127) // 128
    ks = [p[0] for p in pos]
    assert ks == sorted(set(ks)) and ks[-1] == n - 1
    for b in range(nblk):
        assert b * 128 in ks and min(b * 128 + 127, n - 1) in ks
        assert n - b * 128 <= 2 or any(b * 128 < k < min(b * 128 + 127, n - 1) for k in ks)
    for k, *_ in pos:
        B = im.bad_pivot(As, e, k, kind)
        assert np.array_equal(B, B.T) and np.count_nonzero(B != As) == 1
        with pytest.raises(o.NotPositiveDefinite) as ei:
            o.spd_inverse(B)
        assert ei.value.info == k + 1, (n, kind, k)


def test_of_two_bad_rows_the_smaller_is_reported():
    As, _, e = im.family(1100)
    for k1, k2, kinds in ((131, 401, ("neg", "zero")), (640, 1099, ("zero", "neg")), (127, 128, ("zero", "zero"))):
        B = im.bad_pivot(im.bad_pivot(As, e, k2, kinds[1]), e, k1, kinds[0])
        with pytest.raises(o.NotPositiveDefinite) as ei:
            o.spd_inverse(B)
        assert ei.value.info == k1 + 1


def test_group_sizes_and_positions_follow_the_plan():
    # 14 blocks: the smallest count at which the ramp of groups of four engages (6 + 8)
    assert im.group_sizes(14, 4) == [1, 2, 3, 4, 4] and im.group_sizes(13, 4) == [4, 4, 4, 1]
    assert im.group_sizes(14, 3) == [1, 2, 2, 3, 3, 3] and im.group_sizes(14, 2) == [1, 1] + [2] * 6
    assert im.group_sizes(14, 4, ramp=False) == [4, 4, 4, 2] and im.group_sizes(14, 1) == [1] * 14
    assert im.group_sizes(3, 2) == [1, 1, 1] and im.group_sizes(3, 4) == [1, 1, 1]     # fewer than 2 g blocks: single blocks
    assert [im.auto_group(b) for b in (44, 45, 52, 53, 60, 61)] == [1, 2, 2, 3, 3, 4]
    assert im.group_sizes(45, 2) == [1, 2] + [2] * 21 and sum(im.group_sizes(53, 3)) == 53 and sum(im.group_sizes(61, 4)) == 61
    pos = im.positions(1752, im.group_sizes(14, 4))
    assert len(pos) == 14 * 3 and pos[-1] == (1751, 13, 4, 3)
    assert (0, 0, 0, 0) in pos and (128, 1, 1, 0) in pos and (383, 2, 1, 1) in pos and (6 * 128, 6, 3, 0) in pos and (9 * 128 + 127, 9, 3, 3) in pos
    # every slot of every group holds a first, an interior and a last row
    for p, sz in enumerate(im.group_sizes(14, 4)):
        for s in range(sz):
            assert sum(1 for q in pos if q[2:] == (p, s)) == 3
