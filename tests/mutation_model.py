"""The mutation scan stated in numpy (the checker of tests/test_mutation_cpu.py and tests/test_gpu_mutation.py).  Conventions of
tests/energy_model.py (one-hot x, s = q - 1, r(i, c) = i s + c - 1, the gap q has no row, g = mJ Pi).  With E(x) = 1/2 d' mJ d,
d = x - Pi, and delta = e_b - e_a the change of x when site i goes from symbol a to b (a unit vector less where one of them is the gap):

    E(x + delta) - E(x) = delta' mJ d + 1/2 delta' mJ delta
                        = (mJ x - g)[r(i,b)] - (mJ x - g)[r(i,a)] + 1/2 mJ[bb] + 1/2 mJ[aa] - mJ[ab]

(mJ x)[r(i,c)] contains the site's own term mJ[r(i,c), r(i,a)]; without it the - mJ[ab] is gone and + 1/2 mJ[aa] becomes - 1/2 mJ[aa]:

    V(x; i, c) = sum_{j != i, x_j no gap} mJ[r(i,c), r(j,x_j)] + 1/2 mJ[r(i,c), r(i,c)] - g[r(i,c)],   V(x; i, q) = 0
    dE(x; i, b) = V(x; i, b) - V(x; i, x_i)

  potentials_dense   V from the full symmetric mJ in float64 matrix arithmetic;
  potentials_exact   the same sums in np.longdouble, rounded once, with the bound's ingredient
                         B_V(i,c) = sum_{j != i} |mJ[r(i,c), r(j,x_j)]| + |mJ[r(i,c), r(i,x_i)]| + 1/2 |mJ[r,r]| + Gabs[r],
                         Gabs[r] = sum_c |mJ[r,c]| |Pi[c]| >= |g[r]|.
Sequences are the COLUMNS of X, shape (N, K); results have shape (K, N, q), column q - 1 = the gap target."""
import numpy as np

from energy_model import U, energies_dense, model_from_Z, one_hot  # noqa: F401  (re-exported for the tests)


def potentials_dense(mJ, Pi, X, q):
    X = np.asarray(X)
    N, K = X.shape
    s = q - 1
    mJ = np.asarray(mJ, dtype=np.float64)
    g = mJ @ np.asarray(Pi, dtype=np.float64)
    F = one_hot(X, q) @ mJ  # (K, n): (mJ x)[r], mJ symmetric
    V = np.zeros((K, N, q))
    diag = np.diagonal(mJ).reshape(N, s)
    for k in range(K):
        for i in range(N):
            rows = slice(i * s, (i + 1) * s)
            own = mJ[rows, i * s + int(X[i, k]) - 1] if 1 <= X[i, k] < q else 0.0
            V[k, i, :s] = (F[k, rows] - own) + (0.5 * diag[i] - g[rows])
    return V


def potentials_exact(mJ, Pi, X, q):
    """-> (V float64 (K, N, q) rounded once from the longdouble sums, B_V float64 (K, N, q), the unrounded longdouble V)"""
    X = np.asarray(X)
    N, K = X.shape
    s = q - 1
    n = N * s
    mJ = np.asarray(mJ, dtype=np.float64)
    Pl = np.asarray(Pi).astype(np.longdouble)
    g = np.empty(n, dtype=np.longdouble)
    Gabs = np.empty(n, dtype=np.longdouble)
    hd = np.diagonal(mJ).astype(np.longdouble) / 2
    for a in range(0, n, 512):  # (row chunks: the whole matrix in longdouble is 1 GB at n = 8000)
        Lc = mJ[a:a + 512].astype(np.longdouble)
        g[a:a + 512] = Lc @ Pl
        Gabs[a:a + 512] = np.abs(Lc) @ np.abs(Pl)
    Vl = np.zeros((K, N, q), dtype=np.longdouble)
    B = np.zeros((K, N, q))
    for k in range(K):
        col = X[:, k].astype(np.int64)
        sites = np.nonzero((col >= 1) & (col < q))[0]
        r = sites * s + col[sites] - 1
        Ck = mJ[:, r].astype(np.longdouble)  # (n, non-gap sites): the columns the sequence selects
        Sa = np.abs(Ck).sum(axis=1, dtype=np.longdouble)  # every j, the own site too
        for i in range(N):
            rows = slice(i * s, (i + 1) * s)
            S = Ck[rows][:, sites != i].sum(axis=1, dtype=np.longdouble)
            Vl[k, i, :s] = S + hd[rows] - g[rows]
            B[k, i, :s] = (Sa[rows] + np.abs(hd[rows]) + Gabs[rows]).astype(np.float64)
    return Vl.astype(np.float64), B, Vl


def bound_V(N, q, B):
    """|V_any_order - V_exact| <= 2 (N + 2 + n) u B_V: at most N + 2 outer terms in any order (the site's own coupling may be added
    and taken out again), g[r] an n-term sum of its own whose terms Gabs dominates, the factor 2 for the second order"""
    n = N * (q - 1)
    return 2.0 * (N + 2 + n) * U * np.asarray(B)


def wild_type(A, X, q):
    """A (K, N, q) -> (K, N, 1): the entry of each site's own symbol (column q - 1, the gap's, is 0 for V and B_V)"""
    idx = (np.asarray(X).T.astype(np.int64) - 1)[:, :, None]
    return np.take_along_axis(A, idx, axis=2)


def delta_exact(Vl, X, q):
    """dE from the unrounded potentials, rounded once"""
    return (Vl - wild_type(Vl, X, q)).astype(np.float64)


def delta_bound(N, q, B, X, dE):
    """bound_V(i, b) + bound_V(i, x_i) + 2 u |dE|: the two potentials and the one subtraction"""
    bv = bound_V(N, q, B)
    return bv + wild_type(bv, X, q) + 2.0 * U * np.abs(dE)


def single_mutants(x, q):
    """x (N,) -> (N, N q) int8: column i q + (b - 1) is x with site i set to b"""
    N = x.shape[0]
    Xm = np.repeat(np.asarray(x, dtype=np.int8)[:, None], N * q, axis=1)
    for i in range(N):
        Xm[i, i * q:(i + 1) * q] = np.arange(1, q + 1)
    return np.asfortranarray(Xm)
