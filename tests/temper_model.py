"""Replica exchange over the Metropolis chains stated in numpy (the checker of tests/test_temper_cpu.py and tests/test_gpu_temper.py), on
top of tests/sample_model.py (the generator, the proposal, the table update) and the rule of include/gdca.h, "Replica-exchange chains":

    replica (k, r) proposes on stream stream0 + k R + r at beta = betas[the slot it holds]
    round e after proposal t whenever (t + 1) % swap_every == 0: the pairs p in 0 .. R - 2 with p % 2 == e % 2;
        a, b = the holders of the slots p, p + 1;  Ea = E0[a] + S[a], Eb = E0[b] + S[b];  d = (betas[p] - betas[p + 1]) * (Eb - Ea)
        skey = mix64(~key(seed, stream0 + k R));  u = ((draw(skey, e R + p) >> 11) + 1) 2^-53;  thr_s = -log(u);  accept iff d <= thr_s
    sample j: the holder of slot 0 after the round at proposal burn + (j + 1) stride - 1

  emulate               the rule in float64, operation for operation, ONE chain of R replicas from GIVEN tables, E0, thr and swap_thr;
  emulate_chains        the same, vectorised over many chains of a SMALL model (the statistical tests); equal to emulate bit for bit;
  swap_uniforms / swap_thresholds_exact   the u of every (round, pair) of a chain, and -log(u) in np.longdouble;
  attempts              how often every pair is attempted in n_rounds rounds;
  barrier_toy           the 4-site 3-symbol ferromagnet whose two ordered states a cold single-substitution chain does not get between."""
import numpy as np

import sample_model as sm
from sample_model import G, M64, draw, key, mix64, sym_column

INT_MIN = np.iinfo(np.int32).min


def skey(seed, stream0, k, R):
    """the key of chain k's swap draws"""
    return mix64(~key(seed, stream0 + k * R) & M64)


def swap_uniforms(seed, stream0, k, R, n_rounds):
    """u (n_rounds, R - 1) float64 of every (round, pair) of chain k -- attempted or not"""
    c = (np.arange(n_rounds, dtype=np.uint64)[:, None] * np.uint64(R) + np.arange(R - 1, dtype=np.uint64)[None, :]).reshape(-1)
    r = draw(skey(seed, stream0, k, R), c) if c.size else np.zeros(0, dtype=np.uint64)
    return (((r >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53).reshape(n_rounds, R - 1)


def swap_thresholds_exact(seed, stream0, k, R, n_rounds):
    """-log(u) in np.longdouble, (n_rounds, R - 1)"""
    return -np.log(swap_uniforms(seed, stream0, k, R, n_rounds).astype(np.longdouble))


def attempted(R, n_rounds):
    """(n_rounds, R - 1) bool: pair p is attempted in round e"""
    return (np.arange(R - 1)[None, :] % 2) == (np.arange(n_rounds)[:, None] % 2)


def attempts(R, n_rounds):
    """(R - 1,) how often every pair is attempted"""
    return attempted(R, n_rounds).sum(axis=0)


def emulate(V0, E0, mJ, Xr, q, betas, thr, swap_thr, mask=None, flags=0, seed=0, stream0=0, swap_every=1, burn=0, stride=1, n_samples=1,
            slot0=None):
    """What the library returns for ONE chain of R replicas that start at the rows of Xr (R, N) with the tables V0 (R, N, q) and the
    energies E0 (R,), replica r on stream stream0 + r, GIVEN its thresholds thr (R, n_steps) and swap_thr (n_rounds, R - 1) -- bit for
    bit, if the library follows the rule.  -> dict: Xs (n_samples, N) int8, E_s (n_samples,), accepted (R,) by slot, swaps (R - 1,),
    Xr_out (R, N) int8, slot_out (R,), moves (R, n_steps) int32, slot_path (n_rounds, R), V (R, N, q)"""
    betas = np.asarray(betas, dtype=np.float64)
    R = len(betas)
    x = np.array(Xr, dtype=np.int64)
    N, s = x.shape[1], q - 1
    n_steps = burn + n_samples * stride
    assert swap_every >= 1 and burn % swap_every == 0 and stride % swap_every == 0 and x.shape == (R, N)
    n_rounds = n_steps // swap_every
    V = np.array(V0, dtype=np.float64)
    E0 = np.asarray(E0, dtype=np.float64)
    thr = np.asarray(thr, dtype=np.float64).reshape(R, n_steps)
    swap_thr = np.asarray(swap_thr, dtype=np.float64).reshape(n_rounds, R - 1)
    slot_of = np.arange(R) if slot0 is None else np.array(slot0, dtype=np.int64)
    assert sorted(slot_of) == list(range(R))
    holder = np.empty(R, dtype=np.int64)
    holder[slot_of] = np.arange(R)
    T = sm.targets(q, flags)
    lists = [sm.sites_of(x[r], q, mask, flags) for r in range(R)]
    keys = [key(seed, stream0 + r) for r in range(R)]
    zero = np.zeros(N * s)
    S = np.zeros(R)
    accepted, swaps = np.zeros(R, dtype=np.int32), np.zeros(max(R - 1, 0), dtype=np.int32)
    moves = np.full((R, n_steps), INT_MIN, dtype=np.int32)
    slot_path = np.empty((n_rounds, R), dtype=np.int32)
    Xs, E_s = np.empty((n_samples, N), dtype=np.int8), np.empty(n_samples)
    for t in range(n_steps):
        for r in range(R):
            sites = lists[r]
            if not len(sites):
                continue
            beta = betas[slot_of[r]]
            m, v, _ = sm.proposal(draw(keys[r], 2 * t), len(sites), T)
            i = int(sites[m])
            a = int(x[r, i]) - 1
            b = v + (v >= a)
            dE = V[r, i, b] - V[r, i, a]
            with np.errstate(invalid="ignore"):
                go = bool(beta * dE <= thr[r, t])
            code = i * q + b
            moves[r, t] = code if go else -1 - code
            if go:
                S[r] = S[r] + dE
                accepted[slot_of[r]] += 1
                kb = sym_column(mJ, i * s + b) if b < s else zero
                ka = sym_column(mJ, i * s + a) if a < s else zero
                keep = V[r, i].copy()
                V[r, :, :s] = V[r, :, :s] + (kb - ka).reshape(N, s)
                V[r, i] = keep
                x[r, i] = b + 1
        if (t + 1) % swap_every == 0:
            e = (t + 1) // swap_every - 1
            for p in range(e % 2, R - 1, 2):
                a, b = holder[p], holder[p + 1]
                Ea, Eb = E0[a] + S[a], E0[b] + S[b]
                with np.errstate(invalid="ignore"):
                    d = (betas[p] - betas[p + 1]) * (Eb - Ea)
                    go = bool(d <= swap_thr[e, p])
                if go:
                    holder[p], holder[p + 1] = b, a
                    slot_of[a], slot_of[b] = p + 1, p
                    swaps[p] += 1
            slot_path[e] = slot_of
            j, rem = divmod(t + 1 - burn, stride)
            if t + 1 > burn and rem == 0:
                h = holder[0]
                Xs[j - 1] = x[h]
                E_s[j - 1] = E0[h] + S[h]
    return dict(Xs=Xs, E_s=E_s, accepted=accepted, swaps=swaps, Xr_out=x.astype(np.int8), slot_out=slot_of.astype(np.int32), moves=moves,
                slot_path=slot_path, V=V)


def emulate_chains(V0, E0, mJ, Xr, q, betas, thr=None, swap_thr=None, mask=None, flags=0, seed=0, stream0=0, swap_every=1, burn=0, stride=1,
                   n_samples=1, slot0=None):
    """emulate for K chains: Xr (K, R, N), V0 (K, R, N, q), E0 (K, R), chain k on the streams stream0 + k R + r, vectorised over all
    K R replicas (a dense symmetric matrix: small models only).  thr (K, R, n_steps) / swap_thr (K, n_rounds, R - 1), or None:
    -np.log(u) in float64.  slot0 (K, R) or None.  -> dict as emulate's with a leading K (no moves)"""
    betas = np.asarray(betas, dtype=np.float64)
    R = len(betas)
    Xr = np.asarray(Xr)
    K, _, N = Xr.shape
    Gn, s = K * R, q - 1
    n_steps = burn + n_samples * stride
    assert swap_every >= 1 and burn % swap_every == 0 and stride % swap_every == 0 and Xr.shape[1] == R
    n_rounds = n_steps // swap_every
    sym = np.stack([sym_column(mJ, r) for r in range(N * s)], axis=1)
    cols = np.zeros((N * q, N, s))
    for i in range(N):
        cols[i * q:i * q + s] = sym[:, i * s:(i + 1) * s].T.reshape(s, N, s)
    V = np.array(V0, dtype=np.float64).reshape(Gn, N, q)
    E0 = np.asarray(E0, dtype=np.float64).reshape(K, R)
    x = Xr.reshape(Gn, N).astype(np.int64) - 1
    T = sm.targets(q, flags)
    lists = [sm.sites_of(x[g] + 1, q, mask, flags) for g in range(Gn)]
    n_sites = np.array([len(li) for li in lists], dtype=np.uint64)
    table = np.zeros((Gn, max(int(n_sites.max()), 1)), dtype=np.int64)
    for g, li in enumerate(lists):
        table[g, :len(li)] = li
    live = n_sites > 0
    keys = np.array([key(seed, stream0 + g) for g in range(Gn)], dtype=np.uint64)
    skeys = np.array([skey(seed, stream0, k, R) for k in range(K)], dtype=np.uint64)
    rows, ks = np.arange(Gn), np.arange(K)
    slot_of = np.repeat(np.arange(R)[None], K, axis=0) if slot0 is None else np.array(slot0, dtype=np.int64).reshape(K, R)
    holder = np.empty((K, R), dtype=np.int64)
    holder[ks[:, None], slot_of] = np.arange(R)[None]
    S = np.zeros((K, R))
    accepted, swaps = np.zeros((K, R), dtype=np.int32), np.zeros((K, max(R - 1, 0)), dtype=np.int32)
    slot_path = np.empty((K, n_rounds, R), dtype=np.int32)
    Xs, E_s = np.empty((K, n_samples, N), dtype=np.int8), np.empty((K, n_samples))
    chain = rows // R
    for t in range(n_steps):
        with np.errstate(over="ignore"):
            r0 = mix64(keys + np.uint64((2 * t + 1) * G & M64))
            r1 = mix64(keys + np.uint64((2 * t + 2) * G & M64))
        if thr is None:
            th = -np.log(((r1 >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53)
        else:
            th = np.asarray(thr).reshape(Gn, n_steps)[:, t]
        beta = betas[slot_of.reshape(Gn)]
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
            Sf = S.reshape(Gn)
            Sf[g] = Sf[g] + dE[g]
            np.add.at(accepted, (chain[g], slot_of.reshape(Gn)[g]), 1)
            dk = cols[i[g] * q + b[g]] - cols[i[g] * q + a[g]]
            keep = V[g, i[g]].copy()
            V[g, :, :s] = V[g, :, :s] + dk
            V[g, i[g]] = keep
            x[g, i[g]] = b[g]
        if (t + 1) % swap_every == 0:
            e = (t + 1) // swap_every - 1
            for p in range(e % 2, R - 1, 2):
                if swap_thr is None:
                    with np.errstate(over="ignore"):
                        r = mix64(skeys + np.uint64((e * R + p + 1) * G & M64))
                    ths = -np.log(((r >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53)
                else:
                    ths = np.asarray(swap_thr).reshape(K, n_rounds, R - 1)[:, e, p]
                ha, hb = holder[:, p].copy(), holder[:, p + 1].copy()
                Ea, Eb = E0[ks, ha] + S[ks, ha], E0[ks, hb] + S[ks, hb]
                with np.errstate(invalid="ignore"):
                    w = np.nonzero((betas[p] - betas[p + 1]) * (Eb - Ea) <= ths)[0]
                holder[w, p], holder[w, p + 1] = hb[w], ha[w]
                slot_of[w, ha[w]], slot_of[w, hb[w]] = p + 1, p
                swaps[w, p] += 1
            slot_path[:, e] = slot_of
            j, rem = divmod(t + 1 - burn, stride)
            if t + 1 > burn and rem == 0:
                h = holder[:, 0]
                Xs[:, j - 1] = x.reshape(K, R, N)[ks, h] + 1
                E_s[:, j - 1] = E0[ks, h] + S[ks, h]
    return dict(Xs=Xs, E_s=E_s, accepted=accepted, swaps=swaps, Xr_out=(x + 1).astype(np.int8).reshape(K, R, N),
                slot_out=slot_of.astype(np.int32), slot_path=slot_path, V=V.reshape(K, R, N, q))


# ---- the barrier toy -----------------------------------------------------------------------------------------------------------------------
TOY_N, TOY_Q, TOY_J = 4, 3, 2.0
TOY_LADDER = (1.0, 0.6, 0.36, 0.2, 0.1)
TOY_SWAP_EVERY, TOY_STEPS, TOY_K = 4, 400, 32768
TOY_START = np.ones(TOY_N, dtype=np.int8)


def barrier_toy(seed=11):
    """(mJ, Pi, q): a 4-site, 3-symbol ferromagnet in the (W, 0) container, the gap a symbol (81 states with GAPS): W[r(i,c), r(j,c)] =
    -J for i != j and the residues c = 1, 2, small random fields on the diagonal.  E(x) = 1/2 x' W x over the one-hot x: two ordered
    states (all 1, all 2) of energy ~ -6 J each, a single substitution away from either costs ~ 3 J -- a barrier a chain at beta = 1
    does not cross in a few hundred proposals"""
    rng = np.random.default_rng(seed)
    s = TOY_Q - 1
    n = TOY_N * s
    W = np.zeros((n, n))
    for i in range(TOY_N):
        for j in range(TOY_N):
            if i != j:
                for c in range(s):
                    W[i * s + c, j * s + c] = -TOY_J
    W[np.arange(n), np.arange(n)] = rng.normal(scale=0.2, size=n)
    return W, np.zeros(n), TOY_Q


def energy_dense(mJ, Pi, x, q):
    """E(x) = 1/2 (x - Pi)' mJ (x - Pi) over the one-hot x, float64, from the library's triangle (the checker's E0 on a toy model)"""
    x = np.asarray(x, dtype=np.int64)
    s = q - 1
    sym = np.stack([sym_column(mJ, r) for r in range(len(Pi))], axis=1)
    d = -np.asarray(Pi, dtype=np.float64)
    res = np.nonzero(x < q)[0]
    d[res * s + x[res] - 1] += 1
    return float(d @ (sym @ d) / 2)


def toy_chains(betas, seed, run=None, K=TOY_K):
    """The sampled states (K, N) of K chains of TOY_STEPS proposals from TOY_START on the barrier toy, one sample each, the ladder
    `betas` swapped every TOY_SWAP_EVERY proposals, by `run(mJ, Pi, X (N, K), q, betas, seed) -> (Xs (K, N), swaps (K, R - 1))`
    (default: emulate_chains with thresholds from np.log) -> (Xs, swap rate of every pair, states, p exact at beta = 1)"""
    import mutation_model as mm

    mJ, Pi, q = barrier_toy()
    R = len(betas)
    X = np.asfortranarray(np.repeat(TOY_START[:, None], K, axis=1))
    if run is None:
        V1 = mm.potentials_dense(mJ, Pi, TOY_START[:, None], q)[0]
        E1 = energy_dense(mJ, Pi, TOY_START, q)
        out = emulate_chains(np.broadcast_to(V1, (K, R, TOY_N, q)), np.full((K, R), E1), mJ, np.broadcast_to(TOY_START, (K, R, TOY_N)), q, betas,
                             flags=sm.GAPS, seed=seed, swap_every=TOY_SWAP_EVERY, burn=TOY_STEPS - TOY_SWAP_EVERY, stride=TOY_SWAP_EVERY,
                             n_samples=1)
        Xs, swaps = out["Xs"][:, 0], out["swaps"]
    else:
        Xs, swaps = run(mJ, Pi, X, q, betas, seed)
    rates = swaps.sum(axis=0) / (K * attempts(R, TOY_STEPS // TOY_SWAP_EVERY)) if R > 1 else np.zeros(0)
    states, p = sm.boltzmann(mJ, Pi, q, 1.0, sm.GAPS, TOY_START)
    return Xs, rates, states, p


# ---- the Boltzmann-machine loop with a ladder ---------------------------------------------------------------------------------------------
def energies_dense(mJ, Pi, X, q):
    """energy_dense of the rows of X (G, N), vectorised"""
    X = np.asarray(X, dtype=np.int64)
    Gn, N = X.shape
    s = q - 1
    sym = np.stack([sym_column(mJ, r) for r in range(N * s)], axis=1)
    d = np.repeat(-np.asarray(Pi, dtype=np.float64)[None], Gn, axis=0)
    g, i = np.nonzero(X < q)
    d[g, i * s + X[g, i] - 1] += 1
    return np.einsum("gr,rc,gc->g", d, sym, d) / 2


def bm_learn(W, Pi_d, Pij_d, X, q, betas, n_iter, seed=0, burn=0, stride=1, n_samples=1, eta=1.0, lam=0.0, swap_every=1, flags=sm.GAPS):
    """devops.bm_learn_tempered_dev in pure numpy (thresholds -np.log(u)): K chains of R replicas from the columns of X (N, K), iteration
    t on the streams t K R .., the replicas and their slots persistent, the samples of slot 0 tallied -> (W, trace (n_iter, 4),
    swap rates (n_iter, R - 1))"""
    import bm_model as bm
    import mutation_model as mm
    import tally_model

    X = np.asarray(X)
    N, K = X.shape
    R, n = len(betas), N * (q - 1)
    T = burn + n_samples * stride
    Xr = np.repeat(X.T[:, None, :], R, axis=1)  # (K, R, N)
    slot = None
    zeros = np.zeros(n)
    trace, rates = np.empty((n_iter, 4)), np.empty((n_iter, R - 1))
    att = attempts(R, T // swap_every)
    for t in range(n_iter):
        flat = Xr.reshape(K * R, N)
        A = bm.library_symmetric(W)
        V0 = mm.potentials_dense(A, zeros, np.asfortranarray(flat.T), q).reshape(K, R, N, q)
        E0 = energies_dense(A, zeros, flat, q).reshape(K, R)
        out = emulate_chains(V0, E0, W, Xr, q, betas, flags=flags, seed=seed, stream0=t * K * R, swap_every=swap_every, burn=burn, stride=stride,
                             n_samples=n_samples, slot0=slot)
        Xr, slot = out["Xr_out"], out["slot_out"]
        Z = np.ascontiguousarray(out["Xs"].reshape(K * n_samples, N).T)
        Pi_m, Pij_m = tally_model.frequencies(Z, np.ones(K * n_samples), float(K * n_samples), q)
        trace[t, :3] = bm.readout(Pi_d, Pij_d, Pi_m, Pij_m, N, q)[0]
        trace[t, 3] = np.float64(int(out["accepted"][:, 0].astype(np.int64).sum())) / np.float64(K * T)
        if R > 1:
            rates[t] = out["swaps"].sum(axis=0) / (K * att)
        W = bm.update(W, Pij_d, Pij_m, N, q, eta, lam)
    return W, trace, rates
