"""An exact integer model of the weighted frequency tallies (k_tally.hip), in numpy and Python integers.
It imports neither the product nor the oracle: the contract is restated here, and the kernels are held to it bit for bit.

The contract.  For an alignment Z (N x M, symbols 1..q, q the gap), weights W in [0, 1] and a positive Meff:

    shift  = fix_shift(M)                                   the largest shift with M * 2^shift <= 2^63, at most 58
    Wfix_k = rint(W_k * 2^shift)                            u64, round half to even
    Pifix[i][a]       = sum_k Wfix_k [Z[i,k] == a]          u64, a in 1..q-1 (at most 2^63: exactly 2^63 is possible)
    H[(i,a),(j,b)]    = sum_k Wfix_k [Z[i,k] == a][Z[j,k] == b]
    Pi_true[i*s+a-1]  = f64(Pifix[i][a]) * 2^-shift / Meff  one rounding in the conversion, one in the division
    Pij_true likewise from H (n x n, n = N*s, s = q-1, symmetric, zero off the diagonal inside a diagonal block)

and against the true sums  sum_k W_k [..] / Meff  the fixed-point form is off by at most `bound` (derived there).

Z is (N, M) everywhere in this file, as the C-ABI takes it."""
import math
from fractions import Fraction

import numpy as np

U64 = np.uint64
LIMB = 21                      # bits per limb: a limb sum over M <= 2^32 sequences stays below 2^53, exact in f64
LIMB_MASK = (1 << LIMB) - 1


def fix_shift(M):
    """The largest shift with M * 2^shift <= 2^63, capped at 58 (a weight <= 1 must fit the tally's 59-bit field)."""
    assert M >= 1
    sh = 0
    while sh < 58 and (M << (sh + 1)) <= (1 << 63):
        sh += 1
    return sh


def wfix(W, shift):
    """rint(ldexp(w, shift)) per weight as u64.  ldexp is exact here (no underflow: shift >= 0, w >= 2^-1022), np.rint rounds half
    to even, and the result is an integer below 2^59, so the conversion to u64 is exact."""
    W = np.asarray(W, dtype=np.float64)
    assert np.all((W >= 0.0) & (W <= 1.0))
    return np.rint(np.ldexp(W, shift)).astype(U64)


def _onehot(Z, states):
    """(M, N*states) f64: X[k, i*states + a-1] = [Z[i,k] == a] for a in 1..states (other symbols give a zero row segment)."""
    Z = np.asarray(Z)
    N, M = Z.shape
    X = np.zeros((M, N * states))
    for i in range(N):
        a = Z[i].astype(np.int64) - 1
        ok = (a >= 0) & (a < states)
        X[np.nonzero(ok)[0], i * states + a[ok]] = 1.0
    return X


def _limbs(ints, nlimbs):
    """u64 array or Python integers -> nlimbs f64 vectors of LIMB-bit digits, least significant first."""
    if isinstance(ints, np.ndarray):
        assert ints.dtype == U64 and int(ints.max(initial=0)) >> (LIMB * nlimbs) == 0
        return [((ints >> U64(LIMB * l)) & U64(LIMB_MASK)).astype(np.float64) for l in range(nlimbs)]
    return [np.array([(int(v) >> (LIMB * l)) & LIMB_MASK for v in ints], dtype=np.float64) for l in range(nlimbs)]


def _limb_products(XA, XB, ints, nlimbs):
    """XA.T @ diag(v) @ XB digit by digit.  XA, XB hold 0/1 and a digit is below 2^21, so every entry of a product is an integer
    below M * 2^21 <= 2^53 whatever the order BLAS sums in: exact.  Returns nlimbs int64 matrices."""
    assert XA.shape[0] <= (1 << 32)
    return [np.rint(XA.T @ (XB * d[:, None])).astype(np.int64) for d in _limbs(ints, nlimbs)]


def _combine_u64(parts):
    """sum_l parts[l] << (21 l) in u64 (the caller knows the total is below 2^64)."""
    tot = np.zeros(parts[0].shape, dtype=U64)
    for l, p in enumerate(parts):
        tot += p.astype(U64) << U64(LIMB * l)
    return tot


def tallies(Z, Wfix, q, with_gap=False):
    """(Pifix, H): the exact u64 sums.  Pifix is (N, s), H is (N*s, N*s) indexed [(i,a), (j,b)] with a, b in 1..s, s = q-1.
    with_gap=True keeps the gap as a state of its own (s = q): what the recovery of the skip form sums over.
    Wfix < 2^59 takes three 21-bit limbs; a sum is at most M * 2^shift <= 2^63."""
    Wfix = np.asarray(Wfix, dtype=U64)
    assert int(Wfix.max(initial=0)) < (1 << 59)
    N, M = np.asarray(Z).shape
    s = q if with_gap else q - 1
    X = _onehot(Z, s)
    H = _combine_u64(_limb_products(X, X, Wfix, 3))
    Pifix = _combine_u64(_limb_products(X, np.ones((M, 1)), Wfix, 3)).reshape(N, s)
    return Pifix, H


def single_site(Z, Wfix, q):
    """Pifix (N, q-1) alone, column by column: for alignments whose n x n tally is too large to hold."""
    Z = np.asarray(Z)
    N, M = Z.shape
    Wfix, ones = np.asarray(Wfix, dtype=U64), np.ones((M, 1))
    return np.concatenate([_combine_u64(_limb_products(_onehot(Z[i:i + 16], q - 1), ones, Wfix, 3)).reshape(-1, q - 1)
                           for i in range(0, N, 16)])


def pair_tally(Z, Wfix, q, i, j):
    """H's s x s block of the column pair (i, j) by the fast form, without the n x n matrix."""
    Z = np.asarray(Z)
    Xi, Xj = _onehot(Z[i:i + 1], q - 1), _onehot(Z[j:j + 1], q - 1)
    return _combine_u64(_limb_products(Xi, Xj, np.asarray(Wfix, dtype=U64), 3))


def pair_tally_direct(Z, Wfix, q, i, j):
    """The statement of what is computed: Python integers, one sequence at a time.  s x s nested lists, [a-1][b-1]."""
    s = q - 1
    H = [[0] * s for _ in range(s)]
    for a, b, w in zip(np.asarray(Z)[i], np.asarray(Z)[j], Wfix):
        a, b = int(a), int(b)
        if 1 <= a <= s and 1 <= b <= s:
            H[a - 1][b - 1] += int(w)
    return H


def to_frequency(T, shift, Meff):
    """u64 tallies -> f64(T) * 2^-shift / Meff.  numpy's u64 -> f64 rounds to nearest even, as the device conversion does."""
    return np.ldexp(np.asarray(T, dtype=U64).astype(np.float64), -shift) / np.float64(Meff)


def frequencies(Z, W, Meff, q):
    """(Pi_true, Pij_true): what the kernels promise bit for bit."""
    N, M = np.asarray(Z).shape
    shift = fix_shift(M)
    Pifix, H = tallies(Z, wfix(W, shift), q)
    return to_frequency(Pifix.reshape(-1), shift, Meff), to_frequency(H, shift, Meff)


# ---- the independent reference: the true sums ---------------------------------------------------------------------------------
def _weight_ints(W):
    """W_k = ints[k] * 2^-E exactly (a double is a dyadic rational)."""
    fr = [float(w).as_integer_ratio() for w in W]
    E = max(d.bit_length() - 1 for _, d in fr)
    return [n << (E - (d.bit_length() - 1)) for n, d in fr], E


def _ld_quotient(parts, E, Meff):
    """sum_l parts[l] 2^(21 l) * 2^-E / Meff in long double (64-bit significand).  The digit sums are first carried into proper
    21-bit digits, so each term of the Horner sum below is exact and the sum rounds at most once per digit that still holds
    bits: with the division, a relative error below 8 * 2^-64 = 2^-61, 1/256 of ONE of the two f64 roundings `bound` allows."""
    assert np.finfo(np.longdouble).nmant >= 63, "needs an 80-bit long double"
    digits, carry = [], np.zeros(parts[0].shape, dtype=np.int64)
    for p in parts:
        t = p + carry
        digits.append(t & LIMB_MASK)
        carry = t >> LIMB
    digits.append(carry)
    acc = np.zeros(parts[0].shape, dtype=np.longdouble)
    for d in reversed(digits):
        acc = acc * np.longdouble(1 << LIMB) + d.astype(np.longdouble)
    return np.ldexp(acc, -E) / np.longdouble(Meff)


def exact_frequencies(Z, W, Meff, q):
    """The true  sum_k W_k [..] / Meff : the sums exact (integers at the weights' common scale 2^-E, by limbs as above), the
    scaling and the one division in long double.  Returns (Pi, Pij, count_i, count_ij): long double values and, per entry, how many
    sequences feed it (what `bound` needs).  `exact_cell` is the same thing as a Fraction, with no rounding at all."""
    N, M = np.asarray(Z).shape
    X = _onehot(Z, q - 1)
    ints, E = _weight_ints(W)
    nl = (E + 1 + LIMB - 1) // LIMB
    ones = np.ones((M, 1))
    Pi = _ld_quotient(_limb_products(X, ones, ints, nl), E, Meff).reshape(-1)
    Pij = _ld_quotient(_limb_products(X, X, ints, nl), E, Meff)
    cnt = np.rint(X.T @ X).astype(np.int64)
    return Pi, Pij, np.diag(cnt).copy(), cnt


def exact_cell(Z, W, Meff, q, i, a, j, b):
    """sum_k W_k [Z[i,k] == a][Z[j,k] == b] / Meff as a Fraction (a, b in 1..q-1): the definition."""
    Z = np.asarray(Z)
    tot = Fraction(0)
    for k in np.nonzero((Z[i] == a) & (Z[j] == b))[0]:
        tot += Fraction(float(W[k]))
    return tot / Fraction(float(Meff))


def bound(count, shift, Meff, value):
    """|fixed-point form - true value| for an entry fed by `count` sequences.  Each Wfix_k is rint of W_k 2^shift, off by at most
    1/2, so the integer tally is off by at most count/2 units of 2^-shift: count * 2^-(shift+1) / Meff after the division.  The
    tally is then converted to f64 (relative 2^-53) and divided (relative 2^-53): 2 * 2^-53 * |value|.  (Second-order terms, 2^-106
    relative, are far below the reference's own 2^-61.)"""
    return (np.asarray(count, dtype=np.longdouble) * np.ldexp(np.longdouble(1), -(shift + 1)) / np.longdouble(Meff)
            + np.ldexp(np.longdouble(2), -53) * np.abs(np.asarray(value, dtype=np.longdouble)))


def first_mismatch(got, want, T, shift, Meff, s):
    """None when got == want bit for bit, else a message naming the first differing cell as (i, a, j, b) (a, b in 1..s), the
    model's integer tally there and the difference in units of one weight of 1.0 (so a lost or doubled sequence reads as about
    -1 or +1 times its weight)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    if got.shape != want.shape:
        return "shape %s, expected %s" % (got.shape, want.shape)
    bad = np.argwhere(got != want)
    r = [int(x) for x in bad[0]]
    t = int(np.asarray(T)[tuple(r)])
    d = (float(got[tuple(r)]) - float(want[tuple(r)])) * float(Meff)
    if len(r) == 1:
        cell = "(i=%d, a=%d)" % (r[0] // s, r[0] % s + 1)
    else:
        cell = "(i=%d, a=%d, j=%d, b=%d)" % (r[0] // s, r[0] % s + 1, r[1] // s, r[1] % s + 1)
    return ("%d of %d entries differ; first at %s: got %r, model %r, model's integer tally %d (shift %d), "
            "difference %+.6g weight units (%+.6g fixed-point units)"
            % (len(bad), got.size, cell, float(got[tuple(r)]), float(want[tuple(r)]), t, shift, d, d * 2.0 ** shift))
