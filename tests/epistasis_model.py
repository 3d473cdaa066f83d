"""The double-mutant scan stated in numpy (the checker of tests/test_epistasis_cpu.py and tests/test_gpu_epistasis.py).  Conventions of
tests/mutation_model.py (one-hot x, s = q - 1, r(i, c) = i s + c - 1, the gap q has no row).  With K(i,b; j,c) = mJ[r(i,b), r(j,c)],
0 where b or c is the gap, a = x_i and a' = x_j, setting site i to b AND site j to c changes the energy by

    ddE(x; i, b; j, c) = dE(x; i, b) + dE(x; j, c) + eps(x; i, b; j, c)
    eps(x; i, b; j, c) = K(i,b; j,c) - K(i,a; j,c) - K(i,b; j,a') + K(i,a; j,a')

(delta = delta_i + delta_j in E(x + delta) - E(x) = delta' mJ d + 1/2 delta' mJ delta: the cross term delta_i' mJ delta_j is the four
couplings above; dE(x; j, c) already holds K(j,c; i,a) - K(j,a'; i,a), so does dE(x; i, b) its own two).

Everything for ONE sequence x comes as (N, q, N, q) arrays indexed [i, b - 1, j, c - 1]; the entries with i == j mean nothing.
  eps_exact        eps in np.longdouble (four f64 entries: exact up to the longdouble's own rounding, 2^-64 relative);
  ddE_exact        dE(i,b) + dE(j,c) + eps from the UNROUNDED longdouble potentials of mutation_model.potentials_exact;
  ddE_bound        the bound of the library's fixed f64 expressions (include/gdca.h)
                       eps_f = (B[b,c] - B[a,c]) - (B[b,a'] - B[a,a']),      ddE_f = (dE_f[i,b] + dE_f[j,c]) + eps_f
                   against ddE_exact:  delta_bound(i,b) + delta_bound(j,c) + 2u SB + 2u |ddE|,  SB = |B[b,c]| + |B[a,c]| + |B[b,a']| + |B[a,a']|.
                   Derivation, to first order in u = 2^-53: the two inner differences of eps_f err by u (|B[b,c]| + |B[a,c]|) and
                   u (|B[b,a']| + |B[a,a']|), the outer one by u |eps| <= u SB: 2u SB.  dE_f[i,b] and dE_f[j,c] are within their
                   delta_bounds, which hold 2u |dE| where their one subtraction needs u |dE|: the spare u (|dE[i,b]| + |dE[j,c]|)
                   covers the rounding u |dE[i,b] + dE[j,c]| of the first addition.  The last addition: u |ddE|; the second u |ddE| and
                   the factor-2 slack of bound_V take the second-order terms.
  epi_bound        epi_f = sqrt(sum eps_f^2) (q^2 rounded products, q^2 rounded additions in a fixed order, one rounded sqrt) against
                   ||eps||_2:  ||d||_2 + (q^2 + 4) u ||eps||_2,  d[b,c] = 2u SB[b,c].  Derivation: | ||eps_f|| - ||eps|| | <= ||eps_f - eps||
                   <= ||d|| (triangle inequality); a sum of q^2 non-negative rounded products is within (q^2 + 1) u relative of the
                   exact sum of squares to first order in ANY order, the square root halves that and adds its own u:
                   ((q^2 + 1) / 2 + 1) u relative -- doubled here for the second order.
  eps_fixed / ddE_fixed   the library's expressions evaluated in float64 by numpy with the same grouping: what the device must return BIT
                   FOR BIT given its own dE (every operation is one IEEE rounding, nothing is summed in an order of its own)."""
import numpy as np

import mutation_model as mm
from energy_model import U


def padded_blocks(mJ, N, q, dtype=np.float64):
    """(N, q, N, q): [i, b-1, j, c-1] = mJ[r(i,b), r(j,c)], +0.0 where b or c is the gap"""
    s = q - 1
    Bp = np.zeros((N, q, N, q), dtype=dtype)
    Bp[:, :s, :, :s] = np.asarray(mJ, dtype=np.float64).reshape(N, s, N, s)
    return Bp


def _parts(Bp, x):
    """B[a,c] as [i, 1, j, c], B[b,a'] as [i, b, j, 1], B[a,a'] as [i, 1, j, 1] of the sequence x (N,)"""
    N = Bp.shape[0]
    a = np.asarray(x, dtype=np.int64) - 1
    ii = np.arange(N)
    Bac = Bp[ii, a][:, None, :, :]                       # [i, j, c] -> [i, 1, j, c]
    Bba = Bp[:, :, ii, a][:, :, :, None]                 # [i, b, j] -> [i, b, j, 1]
    Baa = Bp[ii, a][:, ii, a][:, None, :, None]          # [i, j]
    return Bac, Bba, Baa


def eps_exact(mJ, x, q):
    N = len(x)
    Bp = padded_blocks(mJ, N, q, np.longdouble)
    Bac, Bba, Baa = _parts(Bp, x)
    return Bp - Bac - Bba + Baa


def eps_fixed(mJ, x, q):
    """(B[b,c] - B[a,c]) - (B[b,a'] - B[a,a']) in float64, this grouping"""
    N = len(x)
    Bp = padded_blocks(mJ, N, q)
    Bac, Bba, Baa = _parts(Bp, x)
    return (Bp - Bac) - (Bba - Baa)


def ddE_fixed(mJ, dE_k, x, q):
    """(dE[i,b] + dE[j,c]) + eps_fixed in float64 from a (N, q) float64 dE of the sequence (the device's own, for the bit-exact check)"""
    return (dE_k[:, :, None, None] + dE_k[None, None, :, :]) + eps_fixed(mJ, x, q)


def sum_abs_blocks(mJ, x, q):
    """SB[i, b, j, c] = |B[b,c]| + |B[a,c]| + |B[b,a']| + |B[a,a']|"""
    N = len(x)
    Bp = np.abs(padded_blocks(mJ, N, q))
    Bac, Bba, Baa = _parts(Bp, x)
    return Bp + Bac + Bba + Baa


def ddE_exact(mJ, Pi, x, q, pot=None):
    """-> (ddE longdouble (N, q, N, q) unrounded, eps longdouble, dE float64 (N, q) rounded once, delta_bound (N, q)) of ONE sequence
    x (N,); pot: mutation_model.potentials_exact(mJ, Pi, x[:, None], q) where the caller has it already"""
    x = np.asarray(x)
    N = len(x)
    X1 = x[:, None]
    V, B, Vl = pot if pot is not None else mm.potentials_exact(mJ, Pi, X1, q)
    dEl = (Vl - mm.wild_type(Vl, X1, q))[0]              # (N, q) longdouble, unrounded
    dE = dEl.astype(np.float64)
    bD = mm.delta_bound(N, q, B, X1, dE[None])[0]
    eps = eps_exact(mJ, x, q)
    return dEl[:, :, None, None] + dEl[None, None, :, :] + eps, eps, dE, bD


def ddE_bound(mJ, x, q, bD, ddE):
    """delta_bound(i,b) + delta_bound(j,c) + 2u SB + 2u |ddE| (see the module's docstring)"""
    return bD[:, :, None, None] + bD[None, None, :, :] + 2.0 * U * sum_abs_blocks(mJ, x, q) + 2.0 * U * np.abs(ddE).astype(np.float64)


def epi_exact(eps):
    """||eps[i, :, j, :]||_2 -> (N, N) longdouble"""
    return np.sqrt((eps * eps).sum(axis=(1, 3), dtype=np.longdouble))


def epi_bound(mJ, x, q, epi):
    d = 2.0 * U * sum_abs_blocks(mJ, x, q)
    return np.sqrt((d * d).sum(axis=(1, 3))) + (q * q + 4) * U * np.asarray(epi, dtype=np.float64)


def admissible(x, q):
    """(N, q, N, q) bool: b != x_i and c != x_j (a true double substitution; the gap target is in, a gap site takes any residue)"""
    a = np.asarray(x, dtype=np.int64) - 1
    nb = np.arange(q)[None, :] != a[:, None]             # [i, b]
    return nb[:, :, None, None] & nb[None, None, :, :]


def by_code(T, i, j):
    """T[i, :, j, :] (b, c) of a pair i < j laid out by the code (b - 1) + q (c - 1): a vector of q^2 entries"""
    return T[i, :, j, :].T.reshape(-1)


def transpose_code(code, q):
    """(b - 1) + q (c - 1) -> (c - 1) + q (b - 1); negative codes (the diagonal) stay"""
    code = np.asarray(code)
    return np.where(code < 0, code, code // q + q * (code % q))


def explicit_double_mutants(x, i, j, q):
    """x (N,) -> (N, q^2) int8, column-major: column (b - 1) + q (c - 1) is x with site i set to b and site j set to c"""
    assert i != j
    Xm = np.repeat(np.asarray(x, dtype=np.int8)[:, None], q * q, axis=1)
    code = np.arange(q * q)
    Xm[i] = code % q + 1
    Xm[j] = code // q + 1
    return np.asfortranarray(Xm)


def all_records(X, q, pairs=None):
    """(L, 5) int32 records (k, i, b, j, c): every target (b, c) of every pair i < j (or of `pairs`) of every column of X, ordered
    k, pair, code -- so that out.reshape(K, pairs, q, q)[k, p, c - 1, b - 1] is the record's"""
    N, K = X.shape
    if pairs is None:
        pairs = [(i, j) for i in range(N) for j in range(i + 1, N)]
    P = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    code = np.arange(q * q, dtype=np.int32)
    k, p, cd = np.meshgrid(np.arange(K, dtype=np.int32), np.arange(len(P), dtype=np.int32), code, indexing="ij")
    rec = np.stack([k, P[p, 0], cd % q + 1, P[p, 1], cd // q + 1], axis=-1).reshape(-1, 5)
    return np.ascontiguousarray(rec, dtype=np.int32), [tuple(r) for r in P.tolist()]
