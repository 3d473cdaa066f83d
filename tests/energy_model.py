"""The energy rule stated twice in numpy (the checker of tests/test_energy_cpu.py and tests/test_gpu_energy.py):

    E(x) = 1/2 (x - Pi)' mJ (x - Pi)

with the project's one-hot encoding (oracle compute_frequencies: x[i*s + a - 1] = 1 for symbol a in 1..s at 0-based site i; symbol
q, the gap, leaves the site's block zero; s = q - 1), Pi the single-site frequencies with pseudocount (add_pseudocount,
src/GaussDCA.jl:30) and mJ = inv(cholesky(C)) (:34).  Sequences are the COLUMNS of X, shape (N, K), like Z in the package.

  energies_dense   the quadratic form as written, in float64 matrix arithmetic;
  energies_gather  the expanded form a kernel wants, accumulated in np.longdouble:
                       E = 1/2 ( sum_i sum_j mJ[r(i), r(j)] - 2 sum_i g[r(i)] + c0 ),  g = mJ Pi, c0 = Pi' g, r(i) = i s + a_i - 1
                   (sums over the non-gap sites), together with the sum of the terms' absolute values
                       B = 1/2 ( sum |mJ[r(i), r(j)]| + 2 sum |g[r(i)]| + |c0| )
                   which bounds the rounding error of ANY summation order of the T = N^2 + N + 1 terms: (T - 1) u B to first order.
"""
import numpy as np


def model_from_Z(Zo, q, pseudocount, theta="auto"):
    """The oracle chain on an (M, N) alignment: compute_weighted_frequencies -> add_pseudocount -> compute_C -> spd_inverse.
    Returns (mJ, Pi) -- Pi WITH pseudocount."""
    from oracle import gdca_oracle as o

    Pi_true, Pij_true, _, _ = o.compute_weighted_frequencies(np.ascontiguousarray(Zo), q, theta)
    Pi, Pij = o.add_pseudocount(Pi_true, Pij_true, float(pseudocount), q)
    return o.spd_inverse(o.compute_C(Pi, Pij)), Pi


def one_hot(X, q):
    """(N, K) symbols -> (K, n) float64"""
    X = np.asarray(X)
    N, K = X.shape
    s = q - 1
    out = np.zeros((K, N * s))
    ii, kk = np.nonzero((X >= 1) & (X < q))
    out[kk, ii * s + X[ii, kk].astype(np.int64) - 1] = 1.0
    return out


def energies_dense(mJ, Pi, X, q):
    d = one_hot(X, q) - np.asarray(Pi)[None, :]
    return 0.5 * np.einsum("ki,ki->k", d @ np.asarray(mJ), d)


def energies_gather(mJ, Pi, X, q):
    """-> (E float64[K] rounded once from the longdouble sums, B float64[K], c0 float64)"""
    X = np.asarray(X)
    N, K = X.shape
    s = q - 1
    L = np.asarray(mJ).astype(np.longdouble)
    Pl = np.asarray(Pi).astype(np.longdouble)
    g = L @ Pl
    c0 = Pl @ g
    La, ga = np.abs(L), np.abs(g)
    E = np.empty(K)
    B = np.empty(K)
    for k in range(K):
        col = X[:, k].astype(np.int64)
        sites = np.nonzero((col >= 1) & (col < q))[0]
        r = sites * s + col[sites] - 1
        quad = L[np.ix_(r, r)].sum(dtype=np.longdouble) if r.size else np.longdouble(0)
        lin = g[r].sum(dtype=np.longdouble) if r.size else np.longdouble(0)
        E[k] = float((quad - 2 * lin + c0) / 2)
        qa = La[np.ix_(r, r)].sum(dtype=np.longdouble) if r.size else np.longdouble(0)
        la = ga[r].sum(dtype=np.longdouble) if r.size else np.longdouble(0)
        B[k] = float((qa + 2 * la + abs(c0)) / 2)
    return E, B, float(c0)


U = 2.0 ** -53


def order_bound(N, q, B):
    """|E_any_order - E_exact| <= 2 (T + n) u B: T = N^2 + N + 1 terms in any order ((T - 1) u B to first order), g and c0 each
    an n-term sum of their own (n u relative on their terms), the factor 2 for the second-order terms."""
    n = N * (q - 1)
    T = N * N + N + 1
    return 2.0 * (T + n) * U * np.asarray(B)
