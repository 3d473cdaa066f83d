"""Extended-precision model of the score stage (csrc/k_score.hip): compute_FN, compute_DI_gauss and correct_APC restated from
the f64 inputs as given, the per-entry error bars they are held to, and the seeded inputs of tests/test_score_model_cpu.py and
tests/test_gpu_score.py.

FN and APC run in np.longdouble (x87 extended, eps 1.08e-19); DI runs in mpmath at 40 digits.  DI takes seconds to minutes per
case, so its expectations are stored (tests/golden/score_cases.npz, made by tests/golden/make_score_cases.py) together with a
SHA-256 of the inputs: a test rebuilds the inputs from score_cases(), checks the hash, and compares with the stored matrix.

The inputs are built without BLAS / LAPACK: every product, orthogonalisation and Cholesky factor below runs in np.longdouble
through numpy's plain loops and is rounded to f64 once, and the graded spectra are made of divisions and powers of two (_grades), not of
pow or exp: beyond the draws of numpy's Generator nothing in the bytes (and the hashes) goes through BLAS, LAPACK or libm.
"""
import hashlib

import numpy as np

assert np.finfo(np.longdouble).eps < 2e-19, "score_model needs an extended-precision np.longdouble (x87 80-bit or wider)"

LD = np.longdouble
U = 2.0 ** -53  # unit roundoff of f64

# DI bar: |DI - ref| <= DI_C s^2 u B^2 + 4 s u,  B = ||L_i||_2 ||L_j||_2 ||X_ij||_2.  DI_C_MEASURED is the largest error of the
# f64 oracle (oracle.compute_DI_gauss: eigh square roots + eigvalsh) against di_model over every pair of every DI case, beyond the
# log-sum term 4 s u, in units of s^2 u B^2 (tests/golden/make_score_cases.py prints it; tests/golden/README.md records it, and
# beside it the plain ratio err / (s^2 u B^2) over the pairs with B >= 1: 0.27, so c = 8 by either count).
# DI_C = max(8, 8 x measured): the device's route (Cholesky factors, Householder, QL) is backward stable like the oracle's, with
# another constant.
DI_C_MEASURED = 0.0185   # case gradedC_s2; every other case is below 0.007
DI_C = max(8.0, 8.0 * DI_C_MEASURED)


# ---- the three operators ----------------------------------------------------------------------------------------------------
def fn_model(mJ, q):
    """SURVEY rule 9: per site pair, the Frobenius norm of the block minus its row means and column means plus its total mean.
    Returns (FN, scale): N x N np.longdouble, zero diagonal; scale[j, i] = max |block (j, i)| (f64), the unit of fn_bound."""
    s = q - 1
    n = mJ.shape[0]
    N = n // s
    FN = np.zeros((N, N), dtype=LD)
    scale = np.zeros((N, N))
    for i in range(N):  # one column site at a time: the largest case (n = 2900) stays at a few megabytes
        B = np.asarray(mJ[:, i * s:(i + 1) * s], dtype=LD).reshape(N, s, s)  # [j, a, b]
        K = B - B.mean(axis=2, keepdims=True) - B.mean(axis=1, keepdims=True) + B.mean(axis=(1, 2), keepdims=True)
        FN[:, i] = np.sqrt((K * K).sum(axis=(1, 2)))
        scale[:, i] = np.abs(mJ[:, i * s:(i + 1) * s]).reshape(N, s, s).max(axis=(1, 2))
    FN = np.tril(FN, -1)   # the device reads block (j, i), j > i, of the lower triangle
    scale = np.tril(scale, -1)
    return FN + FN.T, scale + scale.T


def fn_bound(s, ref, scale):
    """|FN - ref| <= s (3 s + 4) u max|X_ij| + s^2 u ref: the rounding of the s-term means subtracted from every element, summed
    over s^2 elements; then the sum of squares and the root."""
    return np.asarray(s * (3 * s + 4) * U * scale.astype(LD) + s * s * U * ref, dtype=LD)


def apc_model(S):
    """SURVEY rule 11: S - Sj Si / (sum(S) (1 - 1/N)).  Returns (out, corr, amp) in np.longdouble: corr = Sj Si / Sa and
    amp = sum|S| / |sum S|, the two quantities apc_bound scales with."""
    S = np.asarray(S, dtype=LD)
    N = S.shape[0]
    Si = S.sum(axis=0, keepdims=True)
    Sj = S.sum(axis=1, keepdims=True)
    tot = S.sum()
    Sa = tot * (LD(1) - LD(1) / LD(N))
    corr = (Sj * Si) / Sa
    return S - corr, corr, np.abs(S).sum() / abs(tot)


def apc_bound(S, corr, amp):
    """|out - ref| <= 4 u (|S_ij| + |corr_ij|) + (N + 8) u |corr_ij| amp: the subtraction and the correction's own arithmetic;
    then the rounding of the N-term sums that feed the correction."""
    N = S.shape[0]
    return 4 * U * (np.abs(np.asarray(S, dtype=LD)) + np.abs(corr)) + (N + 8) * U * np.abs(corr) * amp


def di_model(mJ, C, q, pairs=None):
    """SURVEY rule 10 in mpmath at 40 digits: per pair i < j, gamma = eigenvalues of MM MM^T, MM = L_j^T X L_i, X = block (j, i) of
    mJ, L = Cholesky factor of the diagonal block of C; DI = s/2 log 1/2 + 1/2 sum log(1 + sqrt(1 + 4 max(gamma, 0))).
    Returns (DI, B), N x N, rounded to f64, zero diagonal: B[i, j] = ||L_i||_2 ||L_j||_2 ||X_ij||_2, the unit of di_bound
    (||L_i||_2^2 = the largest eigenvalue of the diagonal block).  `pairs` restricts the work to some (i, j); the others stay 0."""
    import mpmath

    s = q - 1
    N = mJ.shape[0] // s
    DI, B = np.zeros((N, N)), np.zeros((N, N))
    with mpmath.workdps(40):
        def block(A, a, b):
            return mpmath.matrix([[mpmath.mpf(float(A[a * s + r, b * s + c])) for c in range(s)] for r in range(s)])

        def top(A):  # largest eigenvalue of a symmetric matrix
            return max(mpmath.eigsy(A, eigvals_only=True))

        L, nl = {}, {}
        if pairs is None:
            pairs = [(i, j) for j in range(N) for i in range(j)]
        for i, j in pairs:
            for k in (i, j):
                if k not in L:
                    Ck = block(C, k, k)
                    L[k] = mpmath.cholesky(Ck)
                    nl[k] = mpmath.sqrt(top(Ck))
            X = block(mJ, j, i)
            MM = L[j].T * X * L[i]
            gam = mpmath.eigsy(MM * MM.T, eigvals_only=True)
            acc = mpmath.mpf(0)
            for t in range(s):
                gm = gam[t] if gam[t] > 0 else mpmath.mpf(0)
                acc += mpmath.log(1 + mpmath.sqrt(1 + 4 * gm))
            DI[i, j] = DI[j, i] = float(mpmath.mpf(s) / 2 * mpmath.log(mpmath.mpf(1) / 2) + acc / 2)
            nx = top(X * X.T)
            B[i, j] = B[j, i] = float(nl[i] * nl[j] * mpmath.sqrt(nx if nx > 0 else 0))
    return DI, B


def di_bound(s, B, c=None):
    """|DI - ref| <= c s^2 u B^2 + 4 s u: the three products, V and a backward-stable eigensolver, times s eigenvalues
    (|d/dgamma log(1 + sqrt(1 + 4 gamma))| <= 1); then the log-sum."""
    return (DI_C if c is None else c) * s * s * U * B * B + 4 * s * U


def di_units(s, B, err):
    """the error beyond the log-sum term, in units of s^2 u B^2 (what DI_C is measured in); 0 where that term covers it"""
    excess = np.maximum(err - 4 * s * U, 0.0)
    unit = s * s * U * B * B
    return np.where(excess > 0, excess / np.where(unit > 0, unit, 1e-300), 0.0)


def input_hash(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


# ---- building blocks of the inputs (np.longdouble, rounded to f64 once) -----------------------------------------------------
def _mm(*ms):
    out = np.asarray(ms[0], dtype=LD)
    for m in ms[1:]:
        out = out @ np.asarray(m, dtype=LD)
    return out


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _sym(a):
    """lower triangle mirrored: bitwise symmetric"""
    a = _f64(a)
    return np.tril(a) + np.tril(a, -1).T


def _orth(rng, s):
    """random orthogonal s x s (np.longdouble): Gram-Schmidt, twice, on a Gaussian matrix"""
    Q = np.asarray(rng.standard_normal((s, s)), dtype=LD)
    for _ in range(2):
        for k in range(s):
            for m in range(k):
                Q[:, k] -= (Q[:, m] * Q[:, k]).sum() * Q[:, m]
            Q[:, k] /= np.sqrt((Q[:, k] * Q[:, k]).sum())
    return Q


def _chol(A):
    """lower Cholesky factor in np.longdouble"""
    A = np.array(A, dtype=LD)
    s = A.shape[0]
    Lo = np.zeros((s, s), dtype=LD)
    for c in range(s):
        Lo[c, c] = np.sqrt(A[c, c] - (Lo[c, :c] * Lo[c, :c]).sum())
        for r in range(c + 1, s):
            Lo[r, c] = (A[r, c] - (Lo[r, :c] * Lo[c, :c]).sum()) / Lo[c, c]
    return Lo


def _spd(rng, s):
    """G G^T / s + I"""
    G = rng.standard_normal((s, s))
    return _sym(_mm(G, G.T) / LD(s) + np.eye(s, dtype=LD))


def _grades(s, e_lo, e_hi):
    """s grades from 2^e_lo to 2^e_hi, nearly geometric: 2^floor(e) (1 + e - floor(e)) at equally spaced e.  One division, one
    floor and one scaling by a power of two per grade, each correctly rounded: no pow, no exp, so no libm in the bytes."""
    e = e_lo + (e_hi - e_lo) * (np.arange(s, dtype=np.float64) / max(s - 1, 1))
    f = np.floor(e)
    return np.ldexp(1.0 + (e - f), f.astype(np.int64))


def _spd_graded(rng, s):
    """Q diag(lambda) Q^T, lambda from 2^-10 to 2^10: condition 2^20 = 1.05e6"""
    Q = _orth(rng, s)
    lam = np.asarray(_grades(s, -10.0, 10.0), dtype=LD)
    return _sym(_mm(Q * lam, Q.T))


def _svd_block(rng, s, sigma):
    """U diag(sigma) W^T with random orthogonal U, W"""
    return _f64(_mm(_orth(rng, s) * np.asarray(sigma, dtype=LD), _orth(rng, s).T))


def _assemble(rng, N, s, Cblocks, X):
    """(mJ, C): C with the given diagonal blocks (the rest random and symmetric: the score stage must not read it); mJ symmetric
    with block (j, i) = X[(i, j)] for i < j, both triangles filled, random symmetric diagonal blocks"""
    n = N * s
    C = _sym(0.01 * rng.standard_normal((n, n)))
    mJ = _sym(rng.standard_normal((n, n)))
    for k in range(N):
        C[k * s:(k + 1) * s, k * s:(k + 1) * s] = Cblocks[k]
    for (i, j), x in X.items():
        assert i < j
        mJ[j * s:(j + 1) * s, i * s:(i + 1) * s] = x
        mJ[i * s:(i + 1) * s, j * s:(j + 1) * s] = x.T
    assert np.array_equal(mJ, mJ.T) and np.array_equal(C, C.T)
    return mJ, C


def _pairs(N):
    return [(i, j) for j in range(N) for i in range(j)]


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


# ---- the cases --------------------------------------------------------------------------------------------------------------
DI_GENERIC_S = (1, 2, 3, 12, 13, 16, 17, 20, 23, 30)
DI_GRADED_DELTA = (3e-9, 1e-9)


def _di_case(name):
    """one DI case by name -> dict(q, N, mJ, C, exact_zero=[(i, j)...])"""
    rng = np.random.default_rng(_seed(name))
    kind, _, arg = name.partition("_s")
    s = int(arg.split("_")[0])
    N = 5
    zero = []
    eye = np.eye(s)
    if kind == "generic":  # dense blocks, G G^T / s + I on the diagonal of C
        Cb = [_spd(rng, s) for _ in range(N)]
        X = {p: rng.standard_normal((s, s)) for p in _pairs(N)}
    elif kind == "gradedC":  # the same with diagonal blocks of condition 1e6
        Cb = [_spd_graded(rng, s) for _ in range(N)]
        X = {p: rng.standard_normal((s, s)) for p in _pairs(N)}
    elif kind == "zero":  # one pair with X = 0 exactly: every reflector inactive, DI = 0
        Cb = [_spd(rng, s) for _ in range(N)]
        X = {p: rng.standard_normal((s, s)) for p in _pairs(N)}
        X[(1, 3)] = np.zeros((s, s))
        zero = [(1, 3)]
    elif kind == "degenerate":  # C = I: gamma = sigma^2 exactly -- rank 1, two clusters, all equal, one zero among distinct ones
        Cb = [eye for _ in range(N)]
        sig = [np.r_[3.0, np.zeros(s - 1)], np.r_[np.full(s // 2, 2.0), np.full(s - s // 2, 0.5)], np.full(s, 1.5),
               np.r_[0.0, np.linspace(0.1, 2.0, s - 1)], np.r_[np.full(s - 1, 1.0), 1.0 + 1e-9]]
        X = {p: _svd_block(rng, s, sig[k % len(sig)]) for k, p in enumerate(_pairs(N))}
    elif kind == "strong":  # sigma from 1e4 2^-20 = 0.0095 up to 1e4
        Cb = [_spd(rng, s) for _ in range(N)]
        X = {p: _svd_block(rng, s, 1e4 * _grades(s, -20.0, 0.0)) for p in _pairs(N)}
    elif kind == "weak":  # all sigma ~ 1e-8: DI ~ sum sigma^2, far below the s/2 log 2 terms that cancel
        Cb = [_spd(rng, s) for _ in range(N)]
        X = {p: _svd_block(rng, s, 1e-8 * rng.uniform(0.5, 1.5, s)) for p in _pairs(N)}
    elif kind == "gradedcol":
        # C = I, X = chol(V) with V = G G^T / s + I, V[0,0] = 3, V[1,0] = 1, V[2:,0] = delta randn: the first Householder column of
        # V = X X^T has a tail 1e-9 of its leading entry.  X in one pair and X^T in another: one of them is the device's
        # orientation whichever way it reads the block.
        Cb = [eye for _ in range(N)]
        X = {p: rng.standard_normal((s, s)) for p in _pairs(N)}
        slots = [((0, 1), (2, 3)), ((0, 4), (1, 2))]
        for delta, (pa, pb) in zip(DI_GRADED_DELTA, slots):
            G = rng.standard_normal((s, s))
            V = np.array(_mm(G, G.T) / LD(s) + np.eye(s, dtype=LD))
            V[0, 0] = 3.0
            V[1, 0] = V[0, 1] = 1.0
            V[2:, 0] = V[0, 2:] = delta * rng.standard_normal(s - 2)
            x = _f64(_chol(V))
            X[pa] = x
            X[pb] = x.T.copy()
    elif kind == "pairs":  # N = 2: one pair, the second half-wave idle; N = 12: 66 pairs, the last QL workgroup partly live
        N = int(name.rsplit("_N", 1)[1])
        Cb = [_spd(rng, s) for _ in range(N)]
        X = {p: rng.standard_normal((s, s)) for p in _pairs(N)}
    else:
        raise KeyError(name)
    mJ, C = _assemble(rng, N, s, Cb, X)
    return dict(q=s + 1, N=N, mJ=mJ, C=C, exact_zero=zero)


DI_CASES = tuple(["generic_s%d" % s for s in DI_GENERIC_S] + ["gradedC_s%d" % s for s in DI_GENERIC_S]
                 + ["zero_s4", "zero_s20", "degenerate_s20", "strong_s20", "weak_s20", "gradedcol_s8", "gradedcol_s20",
                    "pairs_s20_N2", "pairs_s20_N12"])
# the sample test_score_model_cpu regenerates: the smallest s, the largest s, the graded column
DI_SAMPLE = ("generic_s1", "generic_s30", "gradedcol_s8")

FN_GENERIC_S = (1, 2, 19, 20, 21, 23, 29, 30)
FN_GENERIC_N = (2, 5, 6, 7, 13)


def _fn_case(name):
    rng = np.random.default_rng(_seed(name))
    if name.startswith("generic"):
        s, N = (int(x[1:]) for x in name.split("_")[1:])
        mJ = _sym(rng.standard_normal((N * s, N * s)))
    elif name == "persistent_s20_N145":  # n = 2900: the k_fn20 list is longer than its grid
        s, N = 20, 145
        mJ = _sym(rng.standard_normal((N * s, N * s)))
    elif name == "offset_s20_N7":  # cancellation in the centring: 1e6 + randn, and a 1^T + 1 b^T + 1e-6 randn, pair by pair in turn
        s, N = 20, 7
        mJ = _sym(rng.standard_normal((N * s, N * s)))
        for k, (i, j) in enumerate(_pairs(N)):
            if k % 2 == 0:
                x = 1e6 + rng.standard_normal((s, s))
            else:
                a, b = rng.standard_normal((s, 1)), rng.standard_normal((1, s))
                x = (a + b) + 1e-6 * rng.standard_normal((s, s))
            mJ[j * s:(j + 1) * s, i * s:(i + 1) * s] = x
            mJ[i * s:(i + 1) * s, j * s:(j + 1) * s] = x.T
    else:
        raise KeyError(name)
    return dict(q=s + 1, N=N, mJ=mJ)


FN_CASES = tuple(["generic_s%d_N%d" % (s, N) for s in FN_GENERIC_S for N in FN_GENERIC_N] + ["persistent_s20_N145", "offset_s20_N7"])

APC_N = (2, 3, 256, 257, 600)
APC_KINDS = ("positive", "dominant", "signed")


def _apc_case(name):
    rng = np.random.default_rng(_seed(name))
    kind, N = name.split("_N")
    N = int(N)
    if kind == "positive":  # scores as FN leaves them: positive, zero diagonal
        S = np.tril(rng.uniform(0.1, 2.0, (N, N)), -1)
    elif kind == "dominant":  # one column (and row) a thousand times the rest
        S = np.tril(rng.uniform(0.1, 2.0, (N, N)), -1)
        S[N // 2, :] *= 1e3
        S[:, N // 2] *= 1e3
    elif kind == "signed":  # both signs, total far from 0 (sum|S| / |sum S| ~ 2), non-zero diagonal
        S = np.tril(rng.standard_normal((N, N)) + 0.5)
    else:
        raise KeyError(name)
    return dict(N=N, S=_sym(S))


APC_CASES = tuple("%s_N%d" % (k, N) for k in APC_KINDS for N in APC_N)

_cache = {}


def score_cases(op, name):
    """the seeded inputs of case `name` of operator `op` ('di', 'fn', 'apc'); built once per process, never modified"""
    key = (op, name)
    if key not in _cache:
        c = {"di": _di_case, "fn": _fn_case, "apc": _apc_case}[op](name)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = c
    return _cache[key]
