"""The pseudo-likelihood fit of the Potts model (W, zeros) restated in numpy (include/gdca.h, "Pseudo-likelihood fit"): the
conditionals, nll, the conditional tallies -- once vectorised in any dtype (np.longdouble: the reference of the bars), once IN THE
DEVICE'S STATED ORDER (f64, to reproduce bits) --, the gradient, the loop, the adaptive rule, and the toy's exact parameters in the
container's gauge.  Sequences are Z (N, M) with symbols 1 .. q, the gap q; p is (M, N, q) with the gap's probability last (the scan's
layout); W is n x n, n = N (q - 1)."""
import numpy as np

import bm_model as bm
import sample_model as sm

LD = np.longdouble
CHUNK_RULE = 512  # GDCA_PLM_CHUNK_RULE
GROW = 1.2        # devops.PLM_GROW


def one_hot(Z, q, dtype=np.float64):
    """(M, n): row k the one-hot code of sequence k, a gap leaving its site's block zero"""
    Z = np.asarray(Z, dtype=np.int64)
    N, M = Z.shape
    s = q - 1
    X = np.zeros((M, N * s), dtype=dtype)
    for i in range(N):
        res = np.nonzero(Z[i] < q)[0]
        X[res, i * s + Z[i, res] - 1] = 1
    return X


def potentials(W, Z, q, dtype=LD):
    """V (M, N, q) of the mutation stage under (W, zeros): V[k, i, c] = sum_{j != i, x_kj no gap} W[r(i,c), r(j,x_kj)] + 1/2 W[r, r],
    the gap's (last) +0.0 -- summed by numpy's matrix product in `dtype`, not in the device's order"""
    N, M = np.asarray(Z).shape
    s = q - 1
    Wd = np.asarray(W).astype(dtype)
    off = np.where(bm.multipliers(N, q) == 1.0, Wd, dtype(0))
    V = one_hot(Z, q, dtype) @ off + np.diagonal(Wd) / 2
    return np.concatenate([V.reshape(M, N, s), np.zeros((M, N, 1), dtype=dtype)], axis=2)


def symbols(Z, q):
    """(M, N) indices 0 .. q - 1 into a site's q entries (the gap q - 1)"""
    return np.asarray(Z, dtype=np.int64).T - 1


def softmax(V, Z, q):
    """(p (M, N, q), l (M, N)) from the potentials, in V's dtype and in the header's operations: m = min V; e = exp(m - V);
    Zs = e_1 + .. + e_q added to +0.0 with c ascending; p = e / Zs; l = (V[x] - m) + log(Zs)"""
    V = np.asarray(V)
    m = V.min(axis=2)
    e = np.exp(m[:, :, None] - V)
    Zs = np.zeros_like(m)
    for c in range(q):
        Zs = Zs + e[:, :, c]
    x = symbols(Z, q)
    vx = np.take_along_axis(V, x[:, :, None], axis=2)[:, :, 0]
    return e / Zs[:, :, None], (vx - m) + np.log(Zs)


def conditionals(W, Z, q, dtype=LD):
    """(p, l, nll_k) in `dtype`; nll_k = the l_ki added to +0.0 with i ascending"""
    p, l = softmax(potentials(W, Z, q, dtype), Z, q)
    nll_k = np.zeros(l.shape[0], dtype=l.dtype)
    for i in range(l.shape[1]):
        nll_k = nll_k + l[:, i]
    return p, l, nll_k


def nll_of(W, Z, w, Meff, q, dtype=LD):
    """nll = (sum_k w_k nll_k) / Meff in `dtype` (numpy's own sum: not the device's order)"""
    return (np.asarray(w).astype(dtype) * conditionals(W, Z, q, dtype)[2]).sum() / dtype(Meff)


def penalty(W, N, q, dtype=np.float64):
    """sum_{i<j} |W_ij|^2: devops.plm_penalty's sum"""
    s = q - 1
    site = np.arange(N * s) // s
    return np.sum(np.where(site[:, None] > site[None, :], np.asarray(W).astype(dtype) ** 2, dtype(0)))


def _finish(Q, S, Meff, N, q):
    m = bm.multipliers(N, q)
    Pi = S / Meff
    Pij = np.where(m == 1.0, (Q + Q.T) / (2 * Meff), 0 * Q)
    n = Q.shape[0]
    Pij[np.arange(n), np.arange(n)] = Pi
    return Pi, Pij


def tallies(p, Z, w, Meff, q):
    """(Pi_c, Pij_c) vectorised in p's dtype: Q[r, c] = sum_k a[k, r] X[k, c], a = w_k p_k[r]"""
    p = np.asarray(p)
    M, N, _ = p.shape
    dtype = p.dtype.type
    a = np.asarray(w).astype(dtype)[:, None] * p[:, :, :q - 1].reshape(M, -1)
    return _finish(a.T @ one_hot(Z, q, dtype), a.sum(axis=0), dtype(Meff), N, q)


def tallies_ordered(p, Z, w, Meff, q, chunk=CHUNK_RULE):
    """(Pi_c, Pij_c) in f64 IN THE DEVICE'S ORDER: a = w_k p_k[r] one rounded product; inside a block of `chunk` sequences an entry's
    terms are added to +0.0 with k ascending (only the sequences that select its column); the blocks' partials are added to +0.0 with
    the block ascending; one addition of Q and its transpose, one division by 2 Meff (Pi_c: by Meff)"""
    p = np.asarray(p, dtype=np.float64)
    M, N, _ = p.shape
    s = q - 1
    n = N * s
    a = np.asarray(w, dtype=np.float64)[:, None] * p[:, :, :s].reshape(M, n)
    x = symbols(Z, q)
    Q, S = np.zeros((n, n)), np.zeros(n)
    for b0 in range(0, M, chunk):
        part, ps = np.zeros((n, n)), np.zeros(n)
        for k in range(b0, min(b0 + chunk, M)):
            sites = np.nonzero(x[k] < s)[0]
            cols = sites * s + x[k, sites]
            part[:, cols] = part[:, cols] + a[k][:, None]
            ps = ps + a[k]
        Q, S = Q + part, S + ps
    return _finish(Q, S, np.float64(Meff), N, q)


def nll_ordered(w, nll_k, Meff):
    """nll in f64 in the device's order: partial t the rounded products w_k nll_k of k = t, t + 256, .. added to +0.0 ascending, the
    256 partials folded by the halving tree, one division"""
    prod = np.asarray(w, dtype=np.float64) * np.asarray(nll_k, dtype=np.float64)
    part = np.zeros(256)
    for k0 in range(0, len(prod), 256):
        blk = prod[k0:k0 + 256]
        part[:len(blk)] = part[:len(blk)] + blk
    h = 128
    while h >= 1:
        part[:h] = part[:h] + part[h:2 * h]
        h //= 2
    return part[0] / np.float64(Meff)


def gradient(W, Z, w, Meff, Pi_d, Pij_d, q, dtype=LD):
    """dF/dW (n, n) in `dtype`: 2 (Pij_c - Pij_d) outside the diagonal blocks (the symmetric pair counted as ONE parameter, the same
    number in both triangles), 1/2 (Pi_c - Pi_d) on the diagonal, 0 elsewhere"""
    N = np.asarray(Z).shape[0]
    Pi_c, Pij_c = tallies(conditionals(W, Z, q, dtype)[0], Z, w, Meff, q)
    m = bm.multipliers(N, q)
    G = np.where(m == 1.0, 2 * (Pij_c - np.asarray(Pij_d).astype(dtype)), dtype(0))
    n = G.shape[0]
    G[np.arange(n), np.arange(n)] = (Pi_c - np.asarray(Pi_d).astype(dtype)) / 2
    return G


def frequencies(Z, w, Meff, q, dtype=LD):
    """(Pi_d, Pij_d): the weighted one- and two-site frequencies of Z in `dtype` (numpy's sums)"""
    X = one_hot(Z, q, dtype)
    wl = np.asarray(w).astype(dtype)
    N = np.asarray(Z).shape[0]
    Pij = X.T @ (X * wl[:, None]) / dtype(Meff)
    Pij = np.where(bm.multipliers(N, q) == 0.0, dtype(0), Pij)
    return wl @ X / dtype(Meff), Pij


def iteration(W, Z, w, Meff, Pi_d, Pij_d, q, eta, lam, chunk=CHUNK_RULE, ordered=True):
    """one iteration in f64 -> (W', (Pi_c, Pij_c), trace row): tallies, bm_model.readout with nll in its fourth place, bm_model.update"""
    N = np.asarray(Z).shape[0]
    p, _, nll_k = conditionals(W, Z, q, np.float64)
    Pi_c, Pij_c = tallies_ordered(p, Z, w, Meff, q, chunk) if ordered else tallies(p, Z, w, Meff, q)
    row = np.append(bm.readout(Pi_d, Pij_d, Pi_c, Pij_c, N, q)[0], nll_ordered(w, nll_k, Meff))
    return bm.update(W, Pij_d, Pij_c, N, q, eta, lam), (Pi_c, Pij_c), row


def learn(W, Z, w, Meff, Pi_d, Pij_d, q, n_iter, eta, lam=0.0, chunk=CHUNK_RULE, ordered=True, keep=False):
    """the loop in f64 -> (W, trace (n_iter, 4)) and, keep, the list of the W every iteration started from"""
    W = np.array(W, dtype=np.float64)
    trace, Ws = np.empty((n_iter, 4)), []
    for t in range(n_iter):
        Ws.append(W)
        W, _, trace[t] = iteration(W, Z, w, Meff, Pi_d, Pij_d, q, eta, lam, chunk, ordered)
    return (W, trace, Ws) if keep else (W, trace)


def learn_adaptive(W, Z, w, Meff, Pi_d, Pij_d, q, n_iter, eta, lam=0.0, state=None, chunk=CHUNK_RULE, ordered=True):
    """devops.plm_learn_adaptive_dev's rule in numpy -> (W, trace, etas, log, state): f = nll + lam penalty(W) at the current W; no
    accepted point yet or f < f_acc: accepted, eta grows by GROW (not at the first point); f == f_acc: accepted, eta stays; then the
    step.  f > f_acc: W restored from the copy, eta halved.  log: per iteration (f, accepted); state: (eta, f_acc, W_save)"""
    N = np.asarray(Z).shape[0]
    W = np.array(W, dtype=np.float64)
    eta, f_acc, W_save = (float(eta), None, W.copy()) if state is None else state
    trace, etas, log = np.empty((n_iter, 4)), np.zeros(n_iter), []
    for t in range(n_iter):
        _, (_, Pij_c), trace[t] = iteration(W, Z, w, Meff, Pi_d, Pij_d, q, eta, lam, chunk, ordered)
        f = float(trace[t, 3]) + (float(lam) * float(penalty(W, N, q)) if lam else 0.0)
        if f_acc is None or f <= f_acc:
            if f_acc is not None and f < f_acc:
                eta *= GROW
            f_acc, W_save = f, W.copy()
            W, etas[t] = bm.update(W, Pij_d, Pij_c, N, q, eta, lam), eta
            log.append((f, True))
        else:
            W, eta = W_save.copy(), eta * 0.5
            log.append((f, False))
    return W, trace, etas, log, (eta, f_acc, W_save)


def parameters(W, N, q):
    """the free parameters of the container as a vector: the diagonal, then the entries below the diagonal blocks"""
    s = q - 1
    site = np.arange(N * s) // s
    low = site[:, None] > site[None, :]
    return np.concatenate([np.diagonal(W), np.asarray(W)[low]])


def from_parameters(theta, N, q):
    s = q - 1
    n = N * s
    site = np.arange(n) // s
    low = site[:, None] > site[None, :]
    W = np.zeros((n, n), dtype=np.asarray(theta).dtype)
    W[low] = theta[n:]
    W = W + W.T
    W[np.arange(n), np.arange(n)] = theta[:n]
    return W


def true_potts_in_gauge(mJ, Pi, q):
    """The exact parameters of the toy (mJ, Pi) -- E(x) = 1/2 (x - Pi)' mJ (x - Pi) over one-hot x -- in the container's gauge (the
    gap's row zero): couplings the off-diagonal blocks of mJ, W[r, r] = mJ[r, r] - 2 (mJ Pi)[r], g summed in np.longdouble.  The entries
    of mJ inside a diagonal block off the diagonal never meet a one-hot x and are dropped."""
    A = bm.library_symmetric(mJ)
    g = (A.astype(LD) @ np.asarray(Pi).astype(LD)).astype(np.float64)
    return bm.potts_from_gaussian(mJ, Pi, q, g=g)


def consistency_toy(N=4, q=3):
    """(mJ, Pi, Z (N, q^N) every state with the gap a symbol, w: the states' exact probabilities (Meff = 1), W_true)"""
    mJ, Pi = sm.toy_model(N=N, q=q)
    states, p = sm.boltzmann(mJ, Pi, q, 1.0, sm.GAPS, np.ones(N, dtype=np.int8))
    return mJ, Pi, np.asfortranarray(states.T.astype(np.int8)), p, true_potts_in_gauge(mJ, Pi, q)


def ulps(got, ref, floor=0.0):
    """|got - ref| in units of the f64 spacing at max(|ref|, floor)"""
    ref = np.asarray(ref, dtype=LD)
    at = np.maximum(np.abs(ref).astype(np.float64), floor)
    return (np.abs(np.asarray(got).astype(LD) - ref) / np.spacing(at).astype(LD)).astype(np.float64)
