"""Boltzmann-machine refinement stated in numpy (the checker of tests/test_bm_cpu.py and tests/test_gpu_bm.py): the container, the
warm start, the update, the read-out and the loop of include/gdca.h, "Boltzmann-machine refinement".  Conventions of
tests/sample_model.py (s = q - 1, r(i, c) = i s + c - 1, the gap q has no row, the library's triangle of a matrix through sym_column).

THE CONTAINER.  A Potts model is the pair (W, 0) in mJ's layout: off-diagonal blocks the couplings, W[r, r] = -2 h[r], +0.0 elsewhere
in a diagonal block, Pi = n zeros.  Then E(x) = sum_{i<j} W[r_i, r_j] + 1/2 sum_i W[r_i, r_i].

  multipliers        m[r, c]: 2 on the diagonal, 0 elsewhere inside a diagonal block, 1 outside;
  g_in_device_order  g = mJ Pi summed as the header states it (blocks of 64 columns), bit for bit the library's;
  potts_from_gaussian, potts_independent   the two starts;
  update / update_scalar   one step: d = Pij_m - Pij_d; g = m d; m == 1 and lam != 0: g = g - lam W; W = W + eta g;
  readout            out[0], out[1] bit for bit, out[2] from exactly rounded sums (math.fsum) with the bound below;
  learn / learn_scalar     the loop on sample_model.emulate_chains (emulate) and tally_model.frequencies;
  add_pseudocount, fit     devops.bm_fit: tallies, targets and start from the same true tallies, the start model, the loop from iteration 0;
  exact_marginals    (Pi, Pij) of a model by enumeration (sample_model.boltzmann); kl, pair_deviation on them.

THE BOUND OF out[2] (u = 2^-53).  The T terms a_k = c_m, b_k = c_d and their rounded products a_k a_k, a_k b_k, b_k b_k are the
same bits here and on the device (one operation each).  A sum of T terms taken in ANY order is within gamma |x|_1 of the exact sum,
gamma = (T - 1) u / (1 - (T - 1) u) (the standard bound: Higham, Accuracy and Stability of Numerical Algorithms, 4.4).  So the
device's five sums lie in intervals S +- e around the exact ones.  num = T Sab - Sa Sb is two rounded products and one rounded
subtraction of operands from those intervals:
    |num_dev - num| <= T e_ab + |Sa| e_b + |Sb| e_a + e_a e_b + 2 u (T (|Sab| + e_ab) + (|Sa| + e_a)(|Sb| + e_b)),
likewise va = T Saa - Sa Sa and vb.  Where an interval of va or vb reaches zero there is no bound (inf).  Otherwise r = num / (sqrt va
sqrt vb) over the corners of the three intervals gives the largest deviation, and the two square roots, the product and the division
add 5 u |r| (half an ulp each where correctly rounded; an ulp allowed for the square roots)."""
import math

import numpy as np

import mutation_model as mm
import sample_model as sm
import tally_model as tm
from energy_model import U, one_hot

GAPS = sm.GAPS


def library_symmetric(mJ):
    """the full symmetric matrix the library sees in the array mJ handed over as it lies: its element (row, col), row >= col, is
    mJ[col, row] (walk_model.sym_column)"""
    mJ = np.asarray(mJ, dtype=np.float64)
    up = np.triu(mJ)
    return up + np.triu(mJ, 1).T


def multipliers(N, q):
    s = q - 1
    site = np.arange(N * s) // s
    m = (site[:, None] != site[None, :]).astype(np.float64)
    m[np.arange(N * s), np.arange(N * s)] = 2.0
    return m


def g_in_device_order(mJ, Pi):
    """g = mJ Pi in the order of include/gdca.h: per block of 64 columns a partial, the products added one by one with the column
    ascending -- in the row's own block the columns c <= r and the columns c > r apart, then the two added --, the partials added one
    by one with the block ascending"""
    A = library_symmetric(mJ)
    Pi = np.asarray(Pi, dtype=np.float64)
    n = A.shape[0]
    rows = np.arange(n)
    g = np.zeros(n)
    for o in range((n + 63) // 64):
        own = rows // 64 == o
        lo, hi = np.zeros(n), np.zeros(n)
        for c in range(64 * o, min(64 * o + 64, n)):
            term = A[:, c] * Pi[c]
            first = ~own | (c <= rows)
            lo = np.where(first, lo + term, lo)
            hi = np.where(first, hi, hi + term)
        g = g + np.where(own, lo + hi, lo)
    return g


def potts_from_gaussian(mJ, Pi, q, g=None):
    """W of the Gaussian model (mJ, Pi): g None -> g_in_device_order"""
    A = library_symmetric(mJ)
    n = A.shape[0]
    g = g_in_device_order(mJ, Pi) if g is None else np.asarray(g)
    W = np.where(multipliers(n // (q - 1), q) == 1.0, A, 0.0)
    W[np.arange(n), np.arange(n)] = np.diagonal(A) - 2.0 * g
    return W


def potts_independent(Pi, N, q):
    P = np.asarray(Pi, dtype=np.float64).reshape(N, q - 1)
    return np.diag((-2.0 * np.log(P / (1.0 - P.sum(axis=1))[:, None])).ravel())


def update(W, Pij_d, Pij_m, N, q, eta, lam=0.0):
    W = np.asarray(W, dtype=np.float64)
    m = multipliers(N, q)
    d = np.asarray(Pij_m, dtype=np.float64) - np.asarray(Pij_d, dtype=np.float64)
    g = m * d
    if lam != 0.0:
        g = np.where(m == 1.0, g - np.float64(lam) * W, g)
    return W + np.float64(eta) * g


def update_scalar(W, Pij_d, Pij_m, N, q, eta, lam=0.0):
    s = q - 1
    n = N * s
    out = np.empty((n, n))
    eta, lam = np.float64(eta), np.float64(lam)
    for r in range(n):
        for c in range(n):
            m = 2.0 if r == c else (0.0 if r // s == c // s else 1.0)
            g = np.float64(m) * (np.float64(Pij_m[r, c]) - np.float64(Pij_d[r, c]))
            if m == 1.0 and lam != 0.0:
                g = g - lam * np.float64(W[r, c])
            out[r, c] = np.float64(W[r, c]) + eta * g
    return out


def _terms(Pi_d, Pij_d, Pi_m, Pij_m, N, q):
    """(a, b): c_m and c_d of the entries below the diagonal blocks, from the library's triangle"""
    s = q - 1
    n = N * s
    site = np.arange(n) // s
    rr, cc = np.nonzero(site[:, None] > site[None, :])
    Ld, Lm = library_symmetric(Pij_d), library_symmetric(Pij_m)
    a = Lm[rr, cc] - np.asarray(Pi_m)[rr] * np.asarray(Pi_m)[cc]
    b = Ld[rr, cc] - np.asarray(Pi_d)[rr] * np.asarray(Pi_d)[cc]
    return a, b


def readout(Pi_d, Pij_d, Pi_m, Pij_m, N, q):
    """-> (out (3,) float64, bound of out[2]): out[0] and out[1] are what the device must return bit for bit; out[2] is the
    correlation from exactly rounded sums, and the device's is within `bound` of it (the module's docstring)"""
    a, b = _terms(Pi_d, Pij_d, Pi_m, Pij_m, N, q)
    out0 = float(np.abs(np.asarray(Pi_m) - np.asarray(Pi_d)).max())
    T = len(a)
    if T == 0:
        return np.array([out0, 0.0, np.nan]), np.inf
    out1 = float(np.abs(a - b).max())
    L = np.longdouble
    terms = (a, b, a * a, a * b, b * b)
    S = [L(math.fsum(x)) for x in terms]
    gam = L(T - 1) * L(U) / (1 - L(T - 1) * L(U))
    e = [gam * L(math.fsum(np.abs(x))) for x in terms]
    Tl, u = L(T), L(U)

    def form(Sxy, exy, Sx, ex, Sy, ey):
        val = Tl * Sxy - Sx * Sy
        err = Tl * exy + abs(Sx) * ey + abs(Sy) * ex + ex * ey + 2 * u * (Tl * (abs(Sxy) + exy) + (abs(Sx) + ex) * (abs(Sy) + ey))
        return val, err

    num, en = form(S[3], e[3], S[0], e[0], S[1], e[1])
    va, ea = form(S[2], e[2], S[0], e[0], S[0], e[0])
    vb, eb = form(S[4], e[4], S[1], e[1], S[1], e[1])
    if not (va - ea > 0 and vb - eb > 0):
        return np.array([out0, out1, float(num / np.sqrt(va * vb)) if va * vb > 0 else np.nan]), np.inf
    r = num / (np.sqrt(va) * np.sqrt(vb))
    worst = max(abs((num + sn * en) / (np.sqrt(va + sa * ea) * np.sqrt(vb + sb * eb)) - r)
                for sn in (-1, 1) for sa in (-1, 1) for sb in (-1, 1))
    bound = float((worst + 5 * u * abs(r)) * (1 + L(2.0) ** -40))  # (the last factor: this computation's own roundings)
    return np.array([out0, out1, float(r)]), bound


def iteration(W, Pi_d, Pij_d, X, q, t, flags, beta, seed, burn, stride, n_samples, eta, lam, mask=None, thr=None, V0=None, scalar=False,
              with_bound=False):
    """one iteration t of the loop from the chains' states X (N, K) -> (W, X, out (4,), Xs (K, n_samples, N), Pi_m, Pij_m), and with
    with_bound readout's bound of out[2] behind them (the read-out's exact sums are the expensive part: taken once).
    thr (K, n_steps) and V0 (K, N, q): the device's thresholds and start tables, where the comparison is to be bit for bit;
    None: -np.log(u) and mutation_model.potentials_dense"""
    X = np.asarray(X)
    N, K = X.shape
    n = N * (q - 1)
    n_steps = burn + n_samples * stride
    if V0 is None:
        V0 = mm.potentials_dense(library_symmetric(W), np.zeros(n), X, q)
    if scalar:
        th = thr if thr is not None else np.stack([-np.log(sm.uniforms(seed, t * K + k, n_steps)[1]) for k in range(K)])
        runs = [sm.emulate(V0[k], W, X[:, k], q, th[k], mask, flags, beta, seed, t * K + k, burn, stride, n_samples) for k in range(K)]
        Xs, acc = np.stack([r[0] for r in runs]), np.array([r[2] for r in runs], dtype=np.int64)
    else:
        Xs, _, acc, _ = sm.emulate_chains(V0, W, X, q, thr, mask, flags, beta, seed, t * K, burn, stride, n_samples)
    Z = np.ascontiguousarray(Xs.reshape(K * n_samples, N).T)  # (N, K n_samples), chain by chain
    Pi_m, Pij_m = tm.frequencies(Z, np.ones(K * n_samples), float(K * n_samples), q)
    out3, bound = readout(Pi_d, Pij_d, Pi_m, Pij_m, N, q)
    rate = np.float64(int(np.asarray(acc, dtype=np.int64).sum())) / np.float64(K * n_steps)
    Wn = (update_scalar if scalar else update)(W, Pij_d, Pij_m, N, q, eta, lam)
    return (Wn, np.asfortranarray(Xs[:, -1].T.astype(np.int8)), np.append(out3, rate), Xs, Pi_m, Pij_m) + ((bound,) if with_bound else ())


def learn(W, Pi_d, Pij_d, X, q, n_iter, flags=GAPS, beta=1.0, seed=0, iter0=0, burn=0, stride=1, n_samples=1, eta=1.0, lam=0.0, mask=None,
          scalar=False):
    """the loop in pure numpy -> (W, X, trace (n_iter, 4))"""
    trace = np.empty((n_iter, 4))
    for it in range(n_iter):
        W, X, trace[it] = iteration(W, Pi_d, Pij_d, X, q, iter0 + it, flags, beta, seed, burn, stride, n_samples, eta, lam, mask,
                                    scalar=scalar)[:3]
    return W, X, trace


def learn_scalar(*a, **kw):
    return learn(*a, scalar=True, **kw)


# ---- the whole fit: devops.bm_fit stated in numpy ---------------------------------------------------------------------------------------
def add_pseudocount(Pi_true, Pij_true, pc, q):
    """add_pseudocount of src/GaussDCA.jl:30, one f64 operation after the other as the oracle writes them: off the diagonal blocks
    (1 - pc) P + (pc / q) / q, on the diagonal (1 - pc) P + pc / q, elsewhere inside a diagonal block (1 - pc) P; Pi = (1 - pc) P + pc / q"""
    Pi_true, Pij_true = np.asarray(Pi_true, dtype=np.float64), np.asarray(Pij_true, dtype=np.float64)
    pc = np.float64(pc)
    pcq = pc / np.float64(q)
    m = multipliers(Pi_true.shape[0] // (q - 1), q)
    scaled = (1.0 - pc) * Pij_true
    Pij = np.where(m == 1.0, scaled + pcq / np.float64(q), np.where(m == 2.0, scaled + pcq, scaled))
    return (1.0 - pc) * Pi_true + pcq, Pij


def fit(Z, q, n_iter, weights, Meff, K, eta=1.0, lam=0.0, pseudocount=0.8, target_pseudocount=0.0, init="gaussian", burn=None, stride=None,
        n_samples=1, beta=1.0, seed=0, flags=GAPS, inverse=None, thresholds=None, tables=None):
    """devops.bm_fit on the alignment Z (N, M) with the sequence weights and Meff GIVEN (the reweighting has its own model): the true
    tallies (tally_model.frequencies), the targets at target_pseudocount and the start at pseudocount from the SAME true tallies, the
    start model -- init = "gaussian": potts_from_gaussian of the inverse of C = Pij - Pi Pi'; "independent": potts_independent of Pi --,
    the chains from the first K sequences, burn = 10 N and stride = N unless given, then n_iter iterations from iteration 0.
    inverse(C) -> mJ, thresholds(t) -> (K, n_steps) and tables(W, X) -> (K, N, q) let a test hand in the device's own inverse, thresholds
    and start tables where the comparison is to be bit for bit; None: numpy's inverse, -np.log(u), mutation_model.potentials_dense.
    -> dict(W, trace (n_iter, 4), bounds (n_iter,): readout's of trace[:, 2], Ws: W after every iteration, X (N, K), W0, Pi_d, Pij_d, Pi)"""
    Z = np.asarray(Z)
    N, M = Z.shape
    assert 1 <= K <= M and n_iter >= 1 and init in ("gaussian", "independent")
    burn = 10 * N if burn is None else int(burn)
    stride = N if stride is None else int(stride)
    Pi_t, Pij_t = tm.frequencies(Z, weights, Meff, q)
    Pi_d, Pij_d = add_pseudocount(Pi_t, Pij_t, target_pseudocount, q)
    Pi, Pij = add_pseudocount(Pi_t, Pij_t, pseudocount, q)
    if init == "gaussian":
        C = Pij - np.outer(Pi, Pi)
        mJ = np.linalg.inv(C) if inverse is None else inverse(C)
        W0 = potts_from_gaussian(mJ, Pi, q)
    else:
        W0 = potts_independent(Pi, N, q)
    W, X = W0, np.asfortranarray(Z[:, :K].astype(np.int8))
    trace, Ws, bounds = np.empty((n_iter, 4)), [], np.empty(n_iter)
    for t in range(n_iter):
        step = iteration(W, Pi_d, Pij_d, X, q, t, flags, beta, seed, burn, stride, n_samples, eta, lam,
                         thr=None if thresholds is None else thresholds(t), V0=None if tables is None else tables(W, X), with_bound=True)
        W, X, trace[t], bounds[t] = step[0], step[1], step[2], step[6]
        Ws.append(W)
    return dict(W=W, trace=trace, bounds=bounds, Ws=Ws, X=X, W0=W0, Pi_d=Pi_d, Pij_d=Pij_d, Pi=Pi)


# ---- exact marginals of a small model ------------------------------------------------------------------------------------------------
def exact_marginals(mJ, Pi, q, N, flags=GAPS):
    """(Pi, Pij) float64 of exp(-E) / Z, E the library's energy of (mJ, Pi), by enumeration from a gap-free start, and the
    probabilities (states, p) themselves"""
    states, p = sm.boltzmann(mJ, Pi, q, 1.0, flags, np.ones(N, dtype=np.int8))
    OH = one_hot(np.ascontiguousarray(states.T), q).astype(np.longdouble)  # (S, n)
    P1 = p @ OH
    P2 = OH.T @ (OH * p[:, None])
    return P1.astype(np.float64), P2.astype(np.float64), states, p


def potts_marginals(W, q, N, flags=GAPS):
    return exact_marginals(W, np.zeros(W.shape[0]), q, N, flags)


def pair_deviation(W, Pij_target, q, N, flags=GAPS):
    """max |Pij of the model (W, 0), exact - Pij_target|"""
    return float(np.abs(potts_marginals(W, q, N, flags)[1] - Pij_target).max())


def kl(p_target, p_model):
    p, m = np.asarray(p_target, dtype=np.longdouble), np.asarray(p_model, dtype=np.longdouble)
    return float((p * np.log(p / m)).sum())
