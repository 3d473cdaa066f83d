"""SPD matrices whose inverse is known exactly, and where a non-positive pivot must be reported (the model of
tests/test_inverse_model_cpu.py and tests/test_gpu_inverse_exact.py).  numpy only; the device-side builder imports torch when called.

The family.  Call index i a *column index* if i % 32 < 16, otherwise a *row index*.  E is an integer matrix that is nonzero only where
i is a row index, j is a column index and i > j, with entries from {-1, 0, 1}.  A product E[i, k] E[k, j] needs k to be a column index
and a row index at once, so E @ E = 0: L = I + E is unit lower triangular with inv(L) = I - E, and

    A = L L',    X = (I - E)' (I - E),    A X = I

are integer matrices.  With D = diag(2^e_i), e_i in -4..4, A_s = D A D and X_s = inv(D) X inv(D) are still exact in float64, and the
pivots of symmetric elimination on A_s are 4^e_k: the reciprocal (v_rcp_f64 and two Newton steps), the fallback's sqrt and 1 / a are
exact on them.  Every intermediate of a sweep over a prefix of the indices is an entry of -inv(A11), inv(A11) A12 or the Schur
complement L22 L22', each a sum of at most n products of entries of {-1, 0, 1} matrices times a power of two.  So a correct inverse
returns X_s bit for bit IN ANY SUMMATION ORDER as long as every partial sum of the deepest tile product (K = 512: a group of four pivot
blocks) of two such intermediates is an integer float64 holds:  512 m^2 < 2^53  with m the largest intermediate (exact_condition;
sweep_growth measures m, and m <= n + 2 from the structure).

Where the inverse must fail: A_s[k, k] = -1 makes the pivot of row k negative, A_s[k, k] -= 4^e_k makes it exactly zero, and the
pivots before row k are untouched: LAPACK's dpotrf and the sweep must both report k + 1.
"""
import time

import numpy as np

T = 128  # the sweep's pivot block


# ---- the family ---------------------------------------------------------------------------------------------------------------------
def _draw(n, seed, density):
    """(rows, cols, V, e): the row and column indices, the int8 entries E[rows x cols] before the i > j mask, the exponents of D"""
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    cols, rows = idx[idx % 32 < 16], idx[idx % 32 >= 16]
    sign = (rng.integers(0, 2, size=(rows.size, cols.size), dtype=np.int8) * 2 - 1).astype(np.int8)
    keep = rng.random((rows.size, cols.size), dtype=np.float32) < density
    e = rng.integers(-4, 5, size=n)
    return rows, cols, np.where(keep, sign, np.int8(0)).astype(np.int8), e


def _exact_product(P, Q):
    """P @ Q of integer matrices as int64.  Through the float64 BLAS (numpy's integer product takes a minute at n = 1752), which is
    exact here: every partial sum is an integer below 2^53 (asserted from the operands' magnitudes)."""
    k = P.shape[1]
    assert k * int(np.abs(P).max(initial=0)) * int(np.abs(Q).max(initial=0)) < 2 ** 53
    R = P.astype(np.float64) @ Q.astype(np.float64)
    Ri = R.astype(np.int64)
    assert np.array_equal(Ri, R)
    return Ri


def integer_family(n, seed, density=0.5):
    """(A, X, E, e) as int64: the unscaled pair and its factor, with E @ E == 0 and A @ X == I asserted"""
    rows, cols, V, e = _draw(n, seed, density)
    E = np.zeros((n, n), dtype=np.int64)
    if rows.size:
        E[np.ix_(rows, cols)] = np.where(rows[:, None] > cols[None, :], V, 0)
    I = np.eye(n, dtype=np.int64)
    assert not _exact_product(E, E).any()
    L, Li = I + E, I - E
    A, X = _exact_product(L, L.T), _exact_product(Li.T, Li)
    assert np.array_equal(_exact_product(A, X), I)
    return A, X, E, e


def exact_family(n, seed, density=0.5, scaled=True):
    """(A, X, e) as float64: A = D L L' D and its exact inverse X = inv(D) (I - E)' (I - E) inv(D), D = diag(2^e) (scaled=False: e = 0)"""
    A, X, _, e = integer_family(n, seed, density)
    if not scaled:
        e = np.zeros(n, dtype=e.dtype)
    s = e[:, None] + e[None, :]
    return np.ldexp(A.astype(np.float64), s), np.ldexp(X.astype(np.float64), -s), e


def sweep_growth(A_int, X_int=None):
    """The scalar sweep of every index in turn on the integer matrix, in int64: after the indices of a set S the state is
    [-inv(A_SS), inv(A_SS) A_SR; A_RS inv(A_SS), A_RR - A_RS inv(A_SS) A_SR].  Returns the largest |entry| any state holds (the
    matrix itself and the result included); asserts that every pivot is 1 and, given X_int, that the sweep ends at -X_int."""
    B = np.array(A_int, dtype=np.int64)
    n = B.shape[0]
    m = int(max(B.max(), -B.min()))
    for k in range(n):
        assert B[k, k] == 1, (k, int(B[k, k]))
        c = B[:, k].copy()
        B -= np.multiply.outer(c, c)   # (d = 1: no division anywhere)
        B[:, k] = c
        B[k, :] = c
        B[k, k] = -1
        m = max(m, int(B.max()), int(-B.min()))
    if X_int is not None:
        assert np.array_equal(B, -np.asarray(X_int, dtype=np.int64))
    return m


def exact_condition(m):
    """every partial sum of a K = 512 product of two intermediates of magnitude <= m is an integer float64 holds"""
    return 512 * int(m) * int(m) < 2 ** 53


def bad_diagonal(a_kk, e_k, kind):
    """what A_s[k, k] = a_kk becomes: -1 ("neg": the pivot of row k turns negative) or a_kk - 4^e_k ("zero": it turns exactly zero)"""
    if kind == "neg":
        return -1.0
    if kind == "zero":
        return float(a_kk) - 4.0 ** int(e_k)
    raise ValueError(kind)


def bad_pivot(A, e, k, kind):
    """A copy of the scaled matrix whose pivot of row k is negative ("neg") or exactly zero ("zero"); the pivots before it stay 4^e_i"""
    B = np.array(A, dtype=np.float64, copy=True)
    B[k, k] = bad_diagonal(B[k, k], e[k], kind)
    return B


# ---- the sweep's schedule, as far as the positions need it --------------------------------------------------------------------------
def auto_group(nblk):
    """the group size the sweep picks by itself (plan_sweep, g_rule): 1 up to 44 blocks, 2 from 45, 3 from 53, 4 from 61"""
    return 4 if nblk >= 61 else (3 if nblk >= 53 else (2 if nblk >= 45 else 1))


def group_sizes(nblk, g, ramp=True):
    """The pivot groups of a sweep over nblk blocks in groups of g (plan_sweep): a matrix of fewer than 2 g blocks is swept in single
    blocks; from g (g - 1) / 2 + 2 g blocks on the sweep opens with the ramp 1, 2, .. g - 1, into which the remainder of the block
    count is inserted; otherwise (and with ramp=False) uniform groups with the remainder last."""
    if nblk < 2 * g:
        g = 1
    ramp_sum = g * (g - 1) // 2
    if ramp and g > 1 and nblk >= ramp_sum + 2 * g:
        sizes = list(range(1, g))
        rest = nblk - ramp_sum
        if rest % g:
            sizes = sorted(sizes + [rest % g])   # (std::upper_bound: behind its equals -- the same list)
        return sizes + [g] * (rest // g)
    return [min(g, nblk - b) for b in range(0, nblk, g)]


def positions(n, sizes=None):
    """The rows at which the tests place a bad pivot: for every 128-block its first row, its last (real) row and one interior row
    (another micro-block and another offset in every block), and row n - 1.  Returns [(k, block, group, slot)], k ascending and
    unique: `group` is the index of the pivot group the block belongs to under the group sizes `sizes` (default: single blocks) and
    `slot` the block's place inside its group -- so that a failure names the group and the slot it happened in."""
    nblk = (n + T - 1) // T
    sizes = list(sizes) if sizes is not None else [1] * nblk
    assert sum(sizes) == nblk, (sizes, nblk)
    where = []
    for p, sz in enumerate(sizes):
        where += [(p, s) for s in range(sz)]
    out = {}
    for b in range(nblk):
        first, last = b * T, min(b * T + T - 1, n - 1)
        inner = first + 1 + (37 * b + 52) % max(last - first - 1, 1)
        for k in (first, min(inner, last), last):
            out[k] = (k, b) + where[b]
    out[n - 1] = (n - 1, nblk - 1) + where[nblk - 1]
    return [out[k] for k in sorted(out)]


# ---- one family per size for the whole suite ----------------------------------------------------------------------------------------
_families = {}


def family(n):
    """exact_family(n, seed 7000 + n), computed once per run of the suite: (A_s, X_s, e)"""
    if n not in _families:
        _families[n] = exact_family(n, 7000 + n)
    return _families[n]


# ---- the same family built on the device, for sizes at which the host products take too long ----------------------------------------
def exact_family_dev(n, seed, density=0.5, device="cuda"):
    """(A_s, X_s, e) as float64 torch tensors on `device`, A_s and X_s n x n: E is drawn on the host as int8 (the draw of
    exact_family), the products are torch's float64 products on the device -- exact for the reason every product of this family is
    (asserted: E E == 0, A X == I, max |A| max |X| n < 2^53, and exact_condition at the structural bound m <= n + 2).  Prints what
    the build took."""
    import torch

    t0 = time.perf_counter()
    assert exact_condition(n + 2)
    rows, cols, V, e = _draw(n, seed, density)
    r, c = torch.from_numpy(rows).to(device), torch.from_numpy(cols).to(device)
    Vd = torch.from_numpy(V).to(device).to(torch.float64)
    E = torch.zeros((n, n), dtype=torch.float64, device=device)
    E[r[:, None], c[None, :]] = Vd * (r[:, None] > c[None, :])
    del Vd
    I = torch.eye(n, dtype=torch.float64, device=device)
    assert not bool((E @ E).any())
    L, Li = I + E, I - E
    A, X = L @ L.T, Li.T @ Li
    del L, Li, E
    assert float(A.abs().max()) * float(X.abs().max()) * n < 2.0 ** 53
    assert torch.equal(A @ X, I)
    del I
    s = torch.from_numpy(np.ldexp(1.0, e)).to(device)
    A *= s[:, None]
    A *= s[None, :]
    X /= s[:, None]
    X /= s[None, :]
    if A.is_cuda:
        torch.cuda.synchronize()
    print("exact_family_dev(n=%d): %.2f s" % (n, time.perf_counter() - t0))
    return A, X, e
