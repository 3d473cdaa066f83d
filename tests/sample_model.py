"""The Metropolis chains stated in numpy (the checker of tests/test_sample_cpu.py and tests/test_gpu_sample.py).  Conventions of
tests/walk_model.py (s = q - 1, r(i, c) = i s + c - 1, the gap q has no row, V(x; i, q) = +0.0, the library's triangle of mJ through
sym_column) and the rule of include/gdca.h, "Metropolis chains":

    mix64(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^ z >> 31      (mod 2^64)
    key(seed, stream) = mix64(mix64(seed + G) + (stream + 1) G),  draw(key, c) = mix64(key + (c + 1) G),  G = 0x9E3779B97F4A7C15
    proposal t: r0 = draw(key, 2 t), r1 = draw(key, 2 t + 1);  m = ((r0 >> 32) n_sites) >> 32, i = sites[m];
                v = ((r0 & 0xffffffff) (T - 1)) >> 32, b = v + (v >= a);  u = ((r1 >> 11) + 1) 2^-53;  thr = -log(u)
    dE = V[i][b] - V[i][a];  accept iff beta * dE <= thr;  then V[j][c] = V[j][c] + (K(j,c; i,b) - K(j,c; i,a)), j != i, c in 1..s

  emulate            the rule in float64, operation for operation, from a GIVEN initial table and GIVEN thresholds, one chain;
  emulate_chains     the same, vectorised over many chains of a SMALL model (the statistical tests); equal to emulate bit for bit;
  thresholds_exact   -log(u) in np.longdouble: what the device's thresholds are held against;
  boltzmann          the exact distribution over the reachable states of a toy model, by enumeration in np.longdouble;
  chi2_p             Pearson's chi-square of observed state counts against it.
The mathematics of an accepted path (the recorded dE, the final table) is the walk's: replay_exact and walk_bounds of walk_model.py
take the accepted moves as a path (accepted_path)."""
import numpy as np

import walk_model as wm
from walk_model import replay_exact, sym_column, walk_bounds  # noqa: F401  (re-exported for the tests)

GAPS = 1
G = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
_C1, _C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def mix64(z):
    """a Python int (mod 2^64), or an array of np.uint64 (wrapping arithmetic)"""
    if isinstance(z, np.ndarray):
        with np.errstate(over="ignore"):
            z = (z ^ (z >> np.uint64(30))) * np.uint64(_C1)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(_C2)
            return z ^ (z >> np.uint64(31))
    z &= M64
    z = ((z ^ (z >> 30)) * _C1) & M64
    z = ((z ^ (z >> 27)) * _C2) & M64
    return z ^ (z >> 31)


def key(seed, stream):
    return mix64(mix64(seed + G) + (stream + 1) * G)


def draw(k, c):
    """draw c of the key k; c an int, or an array of counters (-> np.uint64 array)"""
    if isinstance(c, np.ndarray):
        with np.errstate(over="ignore"):
            return mix64(np.uint64(k) + (c.astype(np.uint64) + np.uint64(1)) * np.uint64(G))
    return mix64(k + (c + 1) * G)


def unmix64(z):
    """the inverse of mix64 (a Python int): mix64 is a bijection of 64-bit words"""
    z ^= z >> 31
    z ^= z >> 62
    z = (z * pow(_C2, -1, 1 << 64)) & M64
    z ^= z >> 27
    z ^= z >> 54
    z = (z * pow(_C1, -1, 1 << 64)) & M64
    z ^= z >> 30
    z ^= z >> 60
    return z


def seed_for_draw(value, stream, c):
    """the seed whose chain `stream` has draw(key, c) == value: a counter constructed for a wanted random number"""
    k = (unmix64(value) - (c + 1) * G) & M64
    return (unmix64((unmix64(k) - (stream + 1) * G) & M64) - G) & M64


def proposal(r0, n_sites, T, a=None):
    """-> (list position m, v, the 0-based target b = v + (v >= a); None without a)"""
    r0 = int(r0)
    m = ((r0 >> 32) * n_sites) >> 32
    v = ((r0 & 0xffffffff) * (T - 1)) >> 32
    return m, v, (None if a is None else v + (v >= a))


def uniform53(r1):
    """u in (0, 1], exact in float64"""
    return float((int(r1) >> 11) + 1) * 2.0 ** -53


def targets(q, flags):
    return q if flags & GAPS else q - 1


def sites_of(x, q, mask, flags):
    """walk_model.admissible restated for the two state spaces: the ascending list of the sites that may change -- the mask lets them,
    and without GAPS they hold a residue.  (With GAPS every symbol but the own is a target, without it every residue but the own.)"""
    x = np.asarray(x)
    ok = np.ones(x.shape[0], dtype=bool) if mask is None else np.asarray(mask) != 0
    if not flags & GAPS:
        ok = ok & (x != q)
    return np.nonzero(ok)[0]


def admissible(x, q, mask, flags):
    """(N, q) bool: the moves (i, b) a proposal can name in state x"""
    N = np.asarray(x).shape[0]
    adm = np.zeros((N, q), dtype=bool)
    adm[sites_of(x, q, mask, flags), :targets(q, flags)] = True
    adm[np.arange(N), np.asarray(x, dtype=np.int64) - 1] = False
    return adm


def uniforms(seed, stream, n_steps):
    """(r0 (n_steps,) np.uint64, u (n_steps,) float64) of the proposals 0 .. n_steps - 1 of one chain"""
    k = key(seed, stream)
    t = np.arange(n_steps, dtype=np.uint64)
    r0, r1 = draw(k, np.uint64(2) * t), draw(k, np.uint64(2) * t + np.uint64(1))
    return r0, ((r1 >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53


def thresholds_exact(seed, stream, n_steps):
    """-log(u) in np.longdouble of the proposals 0 .. n_steps - 1"""
    _, u = uniforms(seed, stream, n_steps)
    return -np.log(u.astype(np.longdouble))


def emulate(V0, mJ, x, q, thr, mask=None, flags=0, beta=1.0, seed=0, stream=0, burn=0, stride=1, n_samples=1):
    """-> (Xs (n_samples, N) int8, dE_s (n_samples,), accepted, moves (n_steps,) int32, V (N, q)): what the library returns for the chain
    that starts at x (N symbols 1..q) with the table V0 (N, q), GIVEN its thresholds thr (n_steps,) -- bit for bit, if the library
    follows the rule"""
    x = np.array(x, dtype=np.int64)
    N, s = x.shape[0], q - 1
    n_steps = burn + n_samples * stride
    V = np.array(V0, dtype=np.float64)
    thr = np.asarray(thr, dtype=np.float64)
    assert V.shape == (N, q) and thr.shape == (n_steps,)
    sites, T = sites_of(x, q, mask, flags), targets(q, flags)
    k = key(seed, stream)
    Xs = np.empty((n_samples, N), dtype=np.int8)
    dE_s = np.empty(n_samples)
    moves = np.full(n_steps, np.iinfo(np.int32).min, dtype=np.int32)
    zero = np.zeros(N * s)  # (+0.0: the gap's column)
    total, accepted = 0.0, 0
    beta = np.float64(beta)
    for t in range(n_steps):
        if len(sites):
            m, v, _ = proposal(draw(k, 2 * t), len(sites), T)
            i = int(sites[m])
            a = int(x[i]) - 1
            b = v + (v >= a)
            dE = V[i, b] - V[i, a]
            with np.errstate(invalid="ignore"):
                go = bool(beta * dE <= thr[t])
            code = i * q + b
            moves[t] = code if go else -1 - code
            if go:
                total = total + dE
                accepted += 1
                kb = sym_column(mJ, i * s + b) if b < s else zero
                ka = sym_column(mJ, i * s + a) if a < s else zero
                keep = V[i].copy()
                V[:, :s] = V[:, :s] + (kb - ka).reshape(N, s)
                V[i] = keep
                x[i] = b + 1
        d, r = divmod(t + 1 - burn, stride)
        if t + 1 > burn and r == 0:
            Xs[d - 1] = x
            dE_s[d - 1] = total
    return Xs, dE_s, accepted, moves, V


def emulate_chains(V0, mJ, X, q, thr=None, mask=None, flags=0, beta=1.0, seed=0, stream0=0, burn=0, stride=1, n_samples=1):
    """emulate for the K chains that start at the columns of X (N, K) with the tables V0 (K, N, q), chain k on stream0 + k, vectorised
    over the chains (a dense symmetric matrix: small models only).  thr (K, n_steps), or None: -np.log(u) in float64.
    -> (Xs (K, n_samples, N) int8, dE_s (K, n_samples), accepted (K,), V (K, N, q))"""
    X = np.asarray(X)
    N, K = X.shape
    s = q - 1
    n_steps = burn + n_samples * stride
    sym = np.stack([sym_column(mJ, r) for r in range(N * s)], axis=1)           # [row, col] from the library's triangle
    cols = np.zeros((N * q, N, s))                                               # [i q + b] = column r(i, b) as (N, s); +0.0 for the gap
    for i in range(N):
        cols[i * q:i * q + s] = sym[:, i * s:(i + 1) * s].T.reshape(s, N, s)
    V = np.array(V0, dtype=np.float64)
    x = X.T.astype(np.int64) - 1                                                 # (K, N), 0-based
    T = targets(q, flags)
    lists = [sites_of(X[:, k], q, mask, flags) for k in range(K)]
    n_sites = np.array([len(li) for li in lists], dtype=np.uint64)
    table = np.zeros((K, max(int(n_sites.max()), 1)), dtype=np.int64)
    for k, li in enumerate(lists):
        table[k, :len(li)] = li
    live = n_sites > 0
    keys = np.array([key(seed, stream0 + k) for k in range(K)], dtype=np.uint64)
    rows = np.arange(K)
    Xs = np.empty((K, n_samples, N), dtype=np.int8)
    dE_s = np.empty((K, n_samples))
    total, accepted = np.zeros(K), np.zeros(K, dtype=np.int32)
    beta = np.float64(beta)
    for t in range(n_steps):
        with np.errstate(over="ignore"):
            r0 = mix64(keys + np.uint64((2 * t + 1) * G & M64))
            r1 = mix64(keys + np.uint64((2 * t + 2) * G & M64))
        if thr is None:
            th = -np.log(((r1 >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53)
        else:
            th = thr[:, t]
        m = (((r0 >> np.uint64(32)) * n_sites) >> np.uint64(32)).astype(np.int64)
        v = (((r0 & np.uint64(0xffffffff)) * np.uint64(T - 1)) >> np.uint64(32)).astype(np.int64)
        i = table[rows, m]
        a = x[rows, i]
        b = v + (v >= a)
        dE = V[rows, i, b] - V[rows, i, a]
        with np.errstate(invalid="ignore"):
            go = live & (beta * dE <= th)
        g = np.nonzero(go)[0]
        if len(g):
            total[g] = total[g] + dE[g]
            accepted[g] += 1
            dk = cols[i[g] * q + b[g]] - cols[i[g] * q + a[g]]                   # (g, N, s)
            keep = V[g, i[g]].copy()
            V[g, :, :s] = V[g, :, :s] + dk
            V[g, i[g]] = keep
            x[g, i[g]] = b[g]
        d, r = divmod(t + 1 - burn, stride)
        if t + 1 > burn and r == 0:
            Xs[:, d - 1] = x + 1
            dE_s[:, d - 1] = total
    return Xs, dE_s, accepted, V


def accepted_path(moves, q):
    """the accepted moves of a chain as a walk's path: (n_accepted, 2) int32 rows (site 0-based, symbol 1..q)"""
    acc = np.asarray(moves)[np.asarray(moves) >= 0].astype(np.int64)
    return np.stack((acc // q, acc % q + 1), axis=1).astype(np.int32).reshape(-1, 2)


def boltzmann(mJ, Pi, q, beta, flags, x0, mask=None):
    """-> (states (S, N) int8, p (S,) np.longdouble): every state a chain from x0 can reach and its probability exp(-beta E) / Z,
    E(x) = 1/2 (x - Pi)' mJ (x - Pi) over the one-hot x, in np.longdouble"""
    x0 = np.asarray(x0, dtype=np.int64)
    N, s = x0.shape[0], q - 1
    sites, T = sites_of(x0, q, mask, flags), targets(q, flags)
    S = T ** len(sites)
    states = np.repeat(x0[None, :], S, axis=0)
    for pos, i in enumerate(sites):
        states[:, i] = (np.arange(S) // T ** pos) % T + 1
    sym = np.stack([sym_column(mJ, r) for r in range(N * s)], axis=1).astype(np.longdouble)
    Pl = np.asarray(Pi).astype(np.longdouble)
    E = np.empty(S, dtype=np.longdouble)
    for k in range(S):
        d = -Pl.copy()
        res = np.nonzero(states[k] < q)[0]
        d[res * s + states[k, res] - 1] += 1
        E[k] = (d @ (sym @ d)) / 2
    w = np.exp(-np.longdouble(beta) * (E - E.min()))
    return states.astype(np.int8), w / w.sum()


def state_index(Xs, q):
    """(K, N) symbols 1..q -> (K,) the states' codes sum_i (x_i - 1) q^i"""
    Xs = np.asarray(Xs, dtype=np.int64)
    return ((Xs - 1) * q ** np.arange(Xs.shape[1])).sum(axis=1)


def chi2_p(samples, states, p, q, min_expected=5.0):
    """Pearson's chi-square of the sampled states (K, N) against the distribution (states, p): the states with an expected count of at
    least min_expected one bin each, the rest together in one -> (p-value, chi2, degrees of freedom).  A sample outside `states` is an
    error."""
    from scipy.stats import chi2

    K = len(samples)
    code = {int(c): k for k, c in enumerate(state_index(states, q))}
    obs = np.zeros(len(states))
    for c, cnt in zip(*np.unique(state_index(samples, q), return_counts=True)):
        assert int(c) in code, "a sample outside the reachable states"
        obs[code[int(c)]] = cnt
    exp = (p * K).astype(np.float64)
    big = exp >= min_expected
    o, e = obs[big], exp[big]
    if (~big).any():
        o, e = np.append(o, obs[~big].sum()), np.append(e, exp[~big].sum())
    x2 = float(((o - e) ** 2 / e).sum())
    return float(chi2.sf(x2, len(e) - 1)), x2, len(e) - 1


def toy_model(seed=7, N=4, q=4, ratio=1e3):
    """(mJ, Pi): a scaled inverse of a random SPD matrix, scaled so that p_max / p_min at beta = 1 is at least `ratio` (1.5 x that on the
    smaller of the two state spaces of a gap-free start), symmetric to the bit"""
    rng = np.random.default_rng(seed)
    n = N * (q - 1)
    R = rng.normal(size=(n, n))
    mJ = np.linalg.inv(R @ R.T / n + 0.5 * np.eye(n))
    mJ = (mJ + mJ.T) / 2
    Pi = rng.dirichlet(np.ones(q), size=N)[:, :q - 1].ravel()
    x0 = np.ones(N, dtype=np.int8)
    span = min(float(np.log(pp.max() / pp.min())) for pp in (boltzmann(mJ, Pi, q, 1.0, f, x0)[1] for f in (0, GAPS)))
    return mJ * (np.log(1.5 * ratio) / span), Pi
