"""log det C stated in extended precision, and the bar the device's value is held to (the checker of tests/test_logdet_cpu.py and
tests/test_gpu_logdet.py).

The device sums the logarithms of the pivots d_i of symmetric elimination without pivoting (the block sweep's, or the squares of the
Cholesky fallback's diagonal).  The reference is the same quantity from a Cholesky factorisation in np.longdouble (u_ld = 2^-64; for
n <= 64 also in mpmath at 40 digits, which the longdouble value must reproduce to its own rounding):

    logdet_ref = sum_i log d_i,   d_i = R_ii^2,   C = R R'.

The bar, stated from the backward error of the elimination before anything was measured.  The computed pivots are the exact pivots of
C + dC with |dC| <= gamma_{n+1} |R| |R|' (Higham, Accuracy and Stability, Thm 10.3; R lower triangular here), and
d log det = trace(inv(C) dC), so to first order

    |d logdet| <= gamma_{n+1} S1,      S1 = sum_ij |mJ_ij| (|R| |R|')_ij,    mJ = inv(C),

to which the logarithms and their summation tree add (log2(n) + 2) u S2, S2 = sum_i |log d_i| (one rounding of log to within an ulp
and its argument's, a per-thread chain of n / 1024 and a tree of depth 10: at most log2(n) + 2 roundings a term for the sizes here).

    bar = F gamma_{n+1} S1 + (log2(n) + 2) u S2,       F = 4.

F covers what the blocked sweep does differently from the Cholesky recurrence of the theorem, chosen from the depth of its sums, not
from a measurement:
  * a factor 2 for the form of every update term: the sweep multiplies by p = fl(1 / d) (a reciprocal refined by two Newton steps,
    then g * p, then the product with the other operand inside the MFMA's accumulation: three roundings a term) where the theorem's
    recurrence has a division and a product (two; its gamma_{n+1} counts n - 1 such terms, the subtraction chain and the square root);
  * a factor 2 for the depth of the elimination: a pivot's Schur complement is formed on two levels -- inside its 128-block (or, in a
    multi-block group, on the group's scratch matrix through the explicit inverse of the blocks before it: N = S Pw, S - N S') and by
    the updates of the groups before -- so a term may pass through two eliminations' roundings instead of one.
The order of the sums themselves costs nothing: gamma_n bounds an n-term inner product in ANY order.

S1 needs two n^3 products of non-negative numbers that enter a bound used to two digits: they are taken in float64 from the reference
factor (relative error n u, 1e-13), their n^2-term sum in longdouble -- in longdouble arithmetic they alone would take 20 s at
n = 1300.  The pivots, their logarithms and S2 are longdouble throughout.
"""
import numpy as np

U = 2.0 ** -53
F_BLOCKED = 4.0
LD = np.longdouble


def gamma(k):
    return k * U / (1.0 - k * U)


def cholesky_ld(C):
    """Lower Cholesky factor of C in np.longdouble (left-looking, column by column).  Raises ValueError at a non-positive pivot."""
    A = np.asarray(C).astype(LD)
    n = A.shape[0]
    R = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - R[j:, :j] @ R[j, :j]
        if not v[0] > 0:
            raise ValueError("not positive definite at pivot %d" % (j + 1))
        R[j:, j] = v / np.sqrt(v[0])
    return R


def logdet_mp(C, digits=40):
    """The same sum from an mpmath Cholesky at `digits` digits (small n only), as a float"""
    import mpmath as mp

    with mp.workdps(digits):
        n = C.shape[0]
        R = mp.cholesky(mp.matrix(np.asarray(C, dtype=np.float64).tolist()))
        return float(mp.fsum(2 * mp.log(R[i, i]) for i in range(n)))


class Reference:
    """logdet (float, rounded once from the longdouble sum), the pivots d (longdouble), the bar and its two terms"""

    def __init__(self, C):
        C = np.asarray(C, dtype=np.float64)
        n = C.shape[0]
        R = cholesky_ld(C)
        self.n = n
        self.d = np.diag(R) ** 2
        logs = np.log(self.d)
        self.logdet_ld = logs.sum(dtype=LD)
        self.logdet = float(self.logdet_ld)
        self.S2 = float(np.abs(logs).sum(dtype=LD))
        # S1 = sum_ij |mJ_ij| (|R| |R|')_ij: the two products in float64 from the reference factor (see the module's text)
        R64 = np.abs(R.astype(np.float64))
        from scipy.linalg import solve_triangular

        Rinv = solve_triangular(R.astype(np.float64), np.eye(n), lower=True)
        mJ = np.abs(Rinv.T @ Rinv)
        self.S1 = float((mJ.astype(LD) * (R64 @ R64.T).astype(LD)).sum(dtype=LD))
        self.term_elim = gamma(n + 1) * self.S1
        self.term_log = (np.log2(n) + 2.0) * U * self.S2
        self.bar = F_BLOCKED * self.term_elim + self.term_log

    def fraction(self, value):
        """|value - logdet_ref| / bar (the error against the longdouble sum, in longdouble)"""
        return float(abs(LD(value) - self.logdet_ld) / LD(self.bar))


def logdet_numpy(C):
    """numpy's own f64 value: 2 sum log diag(cholesky(C))"""
    return float(2.0 * np.sum(np.log(np.diag(np.linalg.cholesky(np.asarray(C, dtype=np.float64))))))


# ---- the test matrices: one place, so that the CPU test and the GPU test hold the same ones to the same bar --------------------------------
OPERATOR_SIZES = [1, 15, 16, 17, 127, 128, 129, 257, 640, 1300]


def random_spd(n, seed=None):
    """B B' + n I from a fixed seed"""
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    B = rng.standard_normal((n, n))
    C = B @ B.T + n * np.eye(n)
    return (C + C.T) * 0.5


def pow2_diagonal(n=300, seed=5):
    """diag(2^e_i), e_i in -30..30: exact pivots.  -> (C, e)"""
    e = np.random.default_rng(seed).integers(-30, 31, size=n)
    return np.diag(np.ldexp(1.0, e)), e


_refs = {}


def reference(key, make):
    """The Reference of make(), computed once per run of the suite under `key`"""
    if key not in _refs:
        C = make()
        _refs[key] = (C, Reference(C))
    return _refs[key]


def operator_case(n):
    return reference(("spd", n), lambda: random_spd(n))


FAMILIES = [(7, 200, 2), (53, 500, 5), (30, 1000, 21)]  # (N, M, q) of synth_family
PSEUDOCOUNTS = [0.5, 0.8]


def family(N, M, q):
    """(M, N) int8 of the fused cases (a fixed seed per shape)"""
    from gaussdca.jl_amd.synth import synth_family

    return synth_family(N, M, q, seed=4000 + 100 * q + N)


def family_case(N, M, q, pc):
    """The oracle chain on the family: (C, Reference) with Pi (with pseudocount) kept beside it"""
    from oracle import gdca_oracle as o

    key = ("family", N, M, q, pc)
    if key not in _refs:
        Zo = family(N, M, q)
        Pi_true, Pij_true, _, _ = o.compute_weighted_frequencies(np.ascontiguousarray(Zo), q, "auto")
        Pi, Pij = o.add_pseudocount(Pi_true, Pij_true, float(pc), q)
        C = o.compute_C(Pi, Pij)
        ref = Reference(C)
        ref.Pi = Pi
        _refs[key] = (C, ref)
    return _refs[key]
