"""numpy model of iterative partner matching (gdca_select_confident*, gdca_concat_pairs*, gdca_run_partner_ipa*), used by
tests/test_ipa_cpu.py and tests/test_gpu_ipa.py.

  rank_key           the 64-bit key of compute_ranking's order (csrc/gdca_internal.h gdca_rank_key, csrc/gdca_host.cpp), written out:
                     ascending keys = descending values under isless, NaN first, then +inf, 0.0 before -0.0
  select             the candidates (match >= 0) by that key, equal keys in ascending a; the first min(n_take, candidates) of them, in
                     ascending a, then -1
  concat             column t = XA[:, selA[t]] over XB[:, selB[t]]
  next_training_set  Z_{r+1} = [Zfix | the selected pairs in ascending a]
  loop               the rounds over a callable "fit and match", with the stop rule of include/gdca.h
  pools              the paired family both suites run on, cut into species

THE BARS OF THE MODEL COMPARISON (test_ipa_cpu.test_model_loop_margins establishes them, test_gpu_ipa relies on them).  The device fits
its own model; every fused comparison of this suite holds its energies to the numpy model at score_close's bar
    ebar = 1e-6 |E| + 1e-9 max|E|                     (tests/gdca_testutil.py; test_gpu_partner.blocks_close),
far above the order bound of pair_energy_model.  Two runs whose blocks agree within ebar entry by entry return
  * the same assignment in a species of k a side if the second-best total lies more than solver_bar + 2 k ebar above the optimum
    (partner_model.solver_bar is the solver's own rounding; k entries of either assignment move by at most ebar each);
  * gaps within 2 ebar of each other, hence the same selection if the last selected and the first rejected confidence differ by more
    than 4 ebar (equal infinities are ordered by a in both and count as an infinite margin);
and then the same next training alignment: by induction the same natives per round."""
import numpy as np

import pair_energy_model as pm
import partner_model as pt

# native pairs per species of the pools (160 in all; five singletons); three more species are appended by pools()
SPECIES = (1, 1, 2, 3, 5, 8, 4, 1, 6, 7, 9, 12, 1, 10, 3, 8, 16, 2, 11, 13, 5, 1, 14, 17)
N_NATIVE, N_FIX, N_INC = 160, 40, 16
IPA_FIELDS = ("M_train", "candidates", "n_sel", "n_changed", "Meff", "theta", "logdet", "cost", "ms_fit", "ms_match", "ms_select", "reserved")


def rank_key(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    u = x.view(np.uint64)
    asc = np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))
    asc = np.where(np.isnan(x), np.uint64(0xFFFFFFFFFFFFFFFF), asc)
    return ~asc


def select(match, gap, n_take):
    """-> (sel int32[KA], n_sel)"""
    match, gap = np.asarray(match), np.asarray(gap, dtype=np.float64)
    cand = np.nonzero(match >= 0)[0]
    order = cand[np.argsort(rank_key(gap[cand]), kind="stable")]
    chosen = np.sort(order[:max(int(n_take), 0)])
    sel = np.full(len(match), -1, dtype=np.int32)
    sel[:len(chosen)] = chosen
    return sel, len(chosen)


def selection_margin(match, gap, n_take):
    """the confidence of the last selected minus that of the first rejected candidate (+inf: nobody is rejected, or both are the same
    infinity and ordered by a)"""
    match, gap = np.asarray(match), np.asarray(gap, dtype=np.float64)
    cand = np.nonzero(match >= 0)[0]
    g = gap[cand][np.argsort(rank_key(gap[cand]), kind="stable")]
    n = max(int(n_take), 0)
    if n == 0 or n >= len(g) or (np.isinf(g[n - 1]) and g[n - 1] == g[n]):
        return np.inf
    return float(g[n - 1] - g[n])


def concat(XA, XB, selA, selB):
    XA, XB = np.asarray(XA), np.asarray(XB)
    selA, selB = np.asarray(selA, dtype=np.int64), np.asarray(selB, dtype=np.int64)
    return np.asfortranarray(np.concatenate([XA[:, selA], XB[:, selB]], axis=0).astype(np.int8))


def next_training_set(Zfix, XA, XB, match, gap, n_take):
    """-> (Z (N, Mfix + n_sel), sel, n_sel)"""
    sel, n = select(match, gap, n_take)
    a = sel[:n]
    tail = concat(XA, XB, a, np.asarray(match)[a])
    Z = tail if Zfix is None or Zfix.shape[1] == 0 else np.concatenate([np.asarray(Zfix), tail], axis=1)
    return np.asfortranarray(Z.astype(np.int8)), sel, n


def seed_alignment(Zfix, XA, XB, seedA, seedB):
    """Z_1: Zfix, then the seed pairs in ascending a"""
    seedA, seedB = np.asarray(seedA, dtype=np.int64), np.asarray(seedB, dtype=np.int64)
    order = np.argsort(seedA, kind="stable")
    tail = concat(XA, XB, seedA[order], seedB[order])
    Z = tail if Zfix is None or Zfix.shape[1] == 0 else np.concatenate([np.asarray(Zfix), tail], axis=1)
    return np.asfortranarray(Z.astype(np.int8))


def loop(fit_and_match, Zfix, XA, XB, seedA, seedB, n_inc, max_rounds):
    """fit_and_match(Z (N, M)) -> (match, gap).  -> one dict a round: Z, match, gap, sel, n_sel, candidates, n_changed"""
    Z = seed_alignment(Zfix, XA, XB, seedA, seedB)
    mfix = 0 if Zfix is None else Zfix.shape[1]
    rounds, before = [], None
    for r in range(1, max_rounds + 1):
        match, gap = fit_and_match(Z)
        match = np.asarray(match)
        cand = int(np.sum(match >= 0))
        Zn, sel, n = next_training_set(Zfix, XA, XB, match, gap, r * n_inc)
        changed = cand if not rounds else int(np.sum(match != rounds[-1]["match"]))
        rounds.append(dict(Z=Z, match=match, gap=np.asarray(gap), sel=sel, n_sel=n, candidates=cand, n_changed=changed))
        if r == max_rounds or (r >= 2 and before[0] == before[1]) or mfix + n < 1:
            break
        before, Z = (n, cand), Zn
    return rounds


# ---- the paired family of both suites -------------------------------------------------------------------------------------------------
def pools(q, N, split, seed=0x9A12):
    """Pools of 160 native pairs (pair_energy_model.paired_family; N odd: its last site dropped) cut into the species of SPECIES, the B
    side permuted inside each species; then a species empty on the A side (0, 3), one empty on the B side (2, 0), and the species of
    five gets two of its b taken away (kA > kB).  Zfix: 40 further pairs.  native[a] = the b that came with a, or -1."""
    Nh = (N + 1) // 2
    extra = 5
    Zfix, Zheld = pm.paired_family(Nh, N_FIX, 3 * (N_NATIVE + extra), q=q, seed=seed)
    Zfix, Zheld = Zfix[:, :N], Zheld[:, :N]   # (M, N): row k = sequence k
    # The family's halves repeat (a half of 30 sites at a mutation rate of 2 % often IS its cluster centre), and two equal sequences of
    # one species are an exact tie no margin can separate: the held-out pairs whose A half and B half have both not been seen before
    # come first, the others behind them (used only where the alphabet and the length leave too few distinct halves: q = 2, N = 7)
    seenA, seenB, first, rest = set(), set(), [], []
    for k, row in enumerate(Zheld):
        ha, hb = row[:split].tobytes(), row[split:].tobytes()
        (rest if ha in seenA or hb in seenB else first).append(k)
        seenA.add(ha)
        seenB.add(hb)
    Zheld = Zheld[(first + rest)[:N_NATIVE + extra]]
    rng = np.random.default_rng(1000 * q + N)
    colsA, colsB, native = [], [], []
    sizesA, sizesB = [], []
    at = 0
    for s, k in enumerate(SPECIES):
        ids = np.arange(at, at + k)
        perm = rng.permutation(k)
        if k == 5 and 5 not in sizesA:        # kA > kB: the b of two sequences a are not in the pool
            perm = perm[perm < 3]
        b0 = len(colsB)
        colsA += ids.tolist()
        colsB += ids[perm].tolist()
        where = {int(i): b0 + t for t, i in enumerate(ids[perm])}
        native += [where.get(int(i), -1) for i in ids]
        sizesA.append(k)
        sizesB.append(len(perm))
        at += k
    # (0, 3): three strangers on the B side; (2, 0): two on the A side
    colsB += [at, at + 1, at + 2]
    sizesA.append(0)
    sizesB.append(3)
    colsA += [at + 3, at + 4]
    native += [-1, -1]
    sizesA.append(2)
    sizesB.append(0)
    XA = np.asfortranarray(Zheld[colsA, :split].T.astype(np.int8))
    XB = np.asfortranarray(Zheld[colsB, split:].T.astype(np.int8))
    offA, offB = pt.offsets(sizesA), pt.offsets(sizesB)
    one = np.nonzero((np.diff(offA) == 1) & (np.diff(offB) == 1))[0]
    return dict(q=q, N=N, split=split, XA=XA, XB=XB, offA=offA, offB=offB, Zfix=np.asfortranarray(Zfix.T.astype(np.int8)),
                native=np.asarray(native), seedA=offA[one].astype(np.int32), seedB=offB[one].astype(np.int32))


VARIANTS = ("seed", "fix", "both")


def variant(P, name):
    """(Zfix or None, seedA, seedB): the singletons with no Zfix; Zfix and an empty seed; both"""
    none = np.empty(0, dtype=np.int32)
    return {"seed": (None, P["seedA"], P["seedB"]), "fix": (P["Zfix"], none, none), "both": (P["Zfix"], P["seedA"], P["seedB"])}[name]


def natives(P, match):
    match = np.asarray(match)
    return int(np.sum((match >= 0) & (match == P["native"])))
