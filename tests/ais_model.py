"""Annealed importance sampling stated in numpy (the checker of tests/test_ais_cpu.py and tests/test_gpu_ais.py), on
tests/sample_model.py: its generator, site list, proposal and table update are the Metropolis chains'.  The rule of include/gdca.h,
"Log partition function":

    start of chain k   ikey = mix64(~key(seed, stream0 + k)); the site at list position m of the TEMPLATE's site list takes the 0-based
                       symbol ((draw(ikey, m) >> 32) T) >> 32, every other site keeps the template's symbol
    stage l = 1 .. L   E = E0 + S;  logw = logw + (betas[l-1] - betas[l]) * E;  then the proposals (l-1) sweep .. l sweep - 1 at betas[l]
    reduction          m = max logw;  e = exp(logw - m);  log Z = n_sites log T + m + log(mean e);  ess = (sum e)^2 / sum e^2

  starts           the K uniform starts;
  emulate          one chain in float64, operation for operation, from a GIVEN start table, start energy and GIVEN thresholds;
  emulate_chains   the same, vectorised over many chains of a SMALL model; equal to emulate bit for bit;
  log_z_exact      log Z by enumeration in np.longdouble;
  reduce_exact     the reduction in np.longdouble;
  z_test           the two-sided normal test of mean(w) against Z / |Omega|."""
import math

import numpy as np

import sample_model as sm
from sample_model import GAPS, M64, sym_column  # noqa: F401

INT_MIN = np.iinfo(np.int32).min


def start_key(seed, stream):
    return sm.mix64(~sm.key(seed, stream) & M64)


def start_symbol(r, T):
    """the 0-based symbol of a draw"""
    return ((int(r) >> 32) * T) >> 32


def template_of(x, q, N=None):
    """the template as an array: x, or -- None -- N residues (every site is then free in either state space)"""
    return np.ones(N, dtype=np.int8) if x is None else np.asarray(x, dtype=np.int8)


def starts(x, q, mask, flags, seed, stream0, K, N=None):
    """-> X0 (N, K) int8, Fortran order: the start of chain k in column k.  x None (no mask then): N free sites"""
    assert x is not None or mask is None
    x = template_of(x, q, N)
    sites, T = sm.sites_of(x, q, mask, flags), sm.targets(q, flags)
    X0 = np.asfortranarray(np.repeat(x[:, None], K, axis=1))
    pos = np.arange(len(sites), dtype=np.uint64)
    for k in range(K):
        if len(sites):
            r = sm.draw(start_key(seed, stream0 + k), pos)
            X0[sites, k] = (((r >> np.uint64(32)) * np.uint64(T)) >> np.uint64(32)).astype(np.int8) + 1
    return X0


def emulate(V0, E0, mJ, x0, q, betas, sweep, thr, mask=None, flags=0, seed=0, stream=0):
    """-> (moves (n_steps,) int32, accepted, Xout (N,) int8, logw, E_end): what the library returns for the chain that starts at x0 (N
    symbols 1..q) with the table V0 (N, q) and the energy E0, GIVEN its thresholds thr (n_steps,) -- bit for bit, if the library
    follows the rule"""
    x = np.array(x0, dtype=np.int64)
    N, s = x.shape[0], q - 1
    betas = np.asarray(betas, dtype=np.float64)
    L = len(betas) - 1
    n_steps = L * sweep
    V = np.array(V0, dtype=np.float64)
    thr = np.asarray(thr, dtype=np.float64)
    assert V.shape == (N, q) and thr.shape == (n_steps,) and L >= 1 and betas[0] == 0.0
    sites, T = sm.sites_of(x, q, mask, flags), sm.targets(q, flags)
    k = sm.key(seed, stream)
    moves = np.full(n_steps, INT_MIN, dtype=np.int32)
    zero = np.zeros(N * s)
    E0 = np.float64(E0)
    S, logw, accepted = np.float64(0.0), np.float64(0.0), 0
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(1, L + 1):
            E = E0 + S
            d = betas[l - 1] - betas[l]
            w = d * E
            logw = logw + w
            for t in range((l - 1) * sweep, l * sweep):
                if not len(sites):
                    continue
                m, v, _ = sm.proposal(sm.draw(k, 2 * t), len(sites), T)
                i = int(sites[m])
                a = int(x[i]) - 1
                b = v + (v >= a)
                dE = V[i, b] - V[i, a]
                go = bool(betas[l] * dE <= thr[t])
                code = i * q + b
                moves[t] = code if go else -1 - code
                if go:
                    S = S + dE
                    accepted += 1
                    kb = sym_column(mJ, i * s + b) if b < s else zero
                    ka = sym_column(mJ, i * s + a) if a < s else zero
                    keep = V[i].copy()
                    V[:, :s] = V[:, :s] + (kb - ka).reshape(N, s)
                    V[i] = keep
                    x[i] = b + 1
        E_end = E0 + S
    return moves, accepted, x.astype(np.int8), logw, E_end


def emulate_chains(V0, E0, mJ, X0, q, betas, sweep, thr=None, mask=None, flags=0, seed=0, stream0=0):
    """emulate for the K chains that start at the columns of X0 (N, K) with the tables V0 (K, N, q) and the energies E0 (K,), chain k
    on stream0 + k, vectorised over the chains (a dense symmetric matrix: small models only).  thr (K, n_steps), or None: -np.log(u)
    in float64.  -> (logw (K,), E_end (K,), Xout (K, N) int8, accepted (K,))"""
    X0 = np.asarray(X0)
    N, K = X0.shape
    s = q - 1
    betas = np.asarray(betas, dtype=np.float64)
    L = len(betas) - 1
    sym = np.stack([sym_column(mJ, r) for r in range(N * s)], axis=1)
    cols = np.zeros((N * q, N, s))
    for i in range(N):
        cols[i * q:i * q + s] = sym[:, i * s:(i + 1) * s].T.reshape(s, N, s)
    V = np.array(V0, dtype=np.float64)
    x = X0.T.astype(np.int64) - 1
    T = sm.targets(q, flags)
    lists = [sm.sites_of(X0[:, k], q, mask, flags) for k in range(K)]
    n_sites = np.array([len(li) for li in lists], dtype=np.uint64)
    table = np.zeros((K, max(int(n_sites.max()), 1)), dtype=np.int64)
    for k, li in enumerate(lists):
        table[k, :len(li)] = li
    live = n_sites > 0
    keys = np.array([sm.key(seed, stream0 + k) for k in range(K)], dtype=np.uint64)
    rows = np.arange(K)
    E0 = np.asarray(E0, dtype=np.float64)
    S, logw, accepted = np.zeros(K), np.zeros(K), np.zeros(K, dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(1, L + 1):
            E = E0 + S
            d = betas[l - 1] - betas[l]
            w = d * E
            logw = logw + w
            for t in range((l - 1) * sweep, l * sweep):
                r0 = sm.mix64(keys + np.uint64((2 * t + 1) * sm.G & M64))
                r1 = sm.mix64(keys + np.uint64((2 * t + 2) * sm.G & M64))
                th = -np.log(((r1 >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53) if thr is None else thr[:, t]
                m = (((r0 >> np.uint64(32)) * n_sites) >> np.uint64(32)).astype(np.int64)
                v = (((r0 & np.uint64(0xffffffff)) * np.uint64(T - 1)) >> np.uint64(32)).astype(np.int64)
                i = table[rows, m]
                a = x[rows, i]
                b = v + (v >= a)
                dE = V[rows, i, b] - V[rows, i, a]
                go = live & (betas[l] * dE <= th)
                g = np.nonzero(go)[0]
                if len(g):
                    S[g] = S[g] + dE[g]
                    accepted[g] += 1
                    dk = cols[i[g] * q + b[g]] - cols[i[g] * q + a[g]]
                    keep = V[g, i[g]].copy()
                    V[g, :, :s] = V[g, :, :s] + dk
                    V[g, i[g]] = keep
                    x[g, i[g]] = b[g]
        E_end = E0 + S
    return logw, E_end, (x + 1).astype(np.int8), accepted


def energies_dense(mJ, Pi, X, q):
    """E (K,) = 1/2 (x - Pi)' mJ (x - Pi) of the columns of X (N, K) in float64 (a dense symmetric matrix: small models only)"""
    X = np.asarray(X, dtype=np.int64)
    N, K = X.shape
    s = q - 1
    sym = np.stack([sym_column(mJ, r) for r in range(N * s)], axis=1)
    D = np.repeat(-np.asarray(Pi, dtype=np.float64)[None, :], K, axis=0)
    for k in range(K):
        res = np.nonzero(X[:, k] < q)[0]
        D[k, res * s + X[res, k] - 1] += 1
    return np.einsum("kr,rc,kc->k", D, sym, D) / 2


def enumerate_states(q, flags, x, mask=None, N=None):
    """-> (states (S, N) int8, n_sites, T): the state space of the template x (None: N free sites)"""
    x = template_of(x, q, N).astype(np.int64)
    sites, T = sm.sites_of(x, q, mask, flags), sm.targets(q, flags)
    S = T ** len(sites)
    states = np.repeat(x[None, :], S, axis=0)
    for pos, i in enumerate(sites):
        states[:, i] = (np.arange(S) // T ** pos) % T + 1
    return states.astype(np.int8), len(sites), T


def energies_exact(mJ, Pi, states, q):
    """E (S,) of the rows of states (S, N) in np.longdouble"""
    S, N = states.shape
    s = q - 1
    sym = np.stack([sym_column(mJ, r) for r in range(N * s)], axis=1).astype(np.longdouble)
    Pl = np.asarray(Pi).astype(np.longdouble)
    E = np.empty(S, dtype=np.longdouble)
    for k in range(S):
        d = -Pl.copy()
        res = np.nonzero(states[k] < q)[0]
        d[res * s + states[k, res] - 1] += 1
        E[k] = (d @ (sym @ d)) / 2
    return E


def log_z_exact(mJ, Pi, q, beta, flags, x, mask=None, N=None):
    """log sum_{x in Omega} exp(-beta E(x)) in np.longdouble, by enumeration"""
    states, _, _ = enumerate_states(q, flags, x, mask, N)
    e = -np.longdouble(beta) * energies_exact(mJ, Pi, states, q)
    return e.max() + np.log(np.exp(e - e.max()).sum())


def reduce_exact(logw, n_sites, T):
    """out4 of the log-weights in np.longdouble: (log Z, ess, max logw, log |Omega|)"""
    lw = np.asarray(logw).astype(np.longdouble)
    m = lw.max()
    e = np.exp(lw - m)
    log_omega = np.longdouble(n_sites) * np.log(np.longdouble(T))
    return log_omega + (m + np.log(e.sum() / len(lw))), e.sum() ** 2 / (e * e).sum(), m, log_omega


def z_test(logw, log_z_over_omega):
    """-> (z, p): z = (mean(w) - Z / |Omega|) / (std(w, ddof=1) / sqrt(K)) of w = exp(logw), and the two-sided normal p"""
    w = np.exp(np.asarray(logw, dtype=np.float64))
    z = float((w.mean() - math.exp(float(log_z_over_omega))) / (w.std(ddof=1) / math.sqrt(len(w))))
    return z, math.erfc(abs(z) / math.sqrt(2.0))
