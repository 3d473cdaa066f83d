"""numpy / scipy model of partner matching per species (gdca_pair_energies_blocked*, gdca_assign_blocks*, gdca_run_partner_match*).

Blocked energies: the diagonal blocks cut out of the full K_A x K_B matrix of tests/pair_energy_model.py (pair_energy,
coupling_gather), packed block after block, each column-major -- the layout include/gdca.h describes.

Assignment: scipy.optimize.linear_sum_assignment per block, and for blocks of at most 6 a side brute force over the permutations, so
the model does not rest on scipy alone.  gap[a] = min_{b' != match(a)} C[a, b'] - C[a, match(a)], one subtraction.

THE ROUNDING BAR OF THE SOLVER (solver_bar).  On costs whose sums are exact (integers) the device's total must EQUAL the optimum.  On
energies the shortest-augmenting-path solver works with reduced costs c - u - v and path lengths that are sums of such terms, so it
finds an assignment that is optimal for costs perturbed by some eps per entry; such an assignment is within 2 k eps of the true
optimum (k = max(kA, kB): k entries of the returned assignment each at most eps too cheap, k of the optimal one each at most eps too
dear).  A potential is changed once per augmentation, by a path length: a chain of at most k f64 additions of reduced costs, each
rounded with a relative error u on a magnitude of at most 2 max|c| (potentials stay within the range of the costs), so a potential
gathers at most k * 2 u max|c| of error per augmentation, over at most k augmentations: eps <= 2 k^2 u max|c|, hence

    total_dev - total_opt  <=  2 k eps  =  4 k^3 u max|c|,        u = 2^-53.

(No tighter bound is claimed; the tests print what fraction of it is used.)  scipy's own total is the optimum of the same f64 costs,
summed in f64: its rounding (k additions, <= k u k max|c|) is inside the same bar."""
import itertools

import numpy as np

import energy_model as em

# the 64 held-out pairs of pair_energy_model.paired_family(30, 1000, 64) cut into species (sizes in order of the sequences)
SPECIES_CUT = (1, 2, 3, 5, 8, 13, 7, 9, 16)


def offsets(sizes):
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)


def blocks_length(offA, offB):
    return int(np.sum(np.diff(np.asarray(offA, dtype=np.int64)) * np.diff(np.asarray(offB, dtype=np.int64))))


def cut_blocks(E, offA, offB):
    """the diagonal blocks of a full K_A x K_B matrix"""
    return [E[offA[s]:offA[s + 1], offB[s]:offB[s + 1]] for s in range(len(offA) - 1)]


def pack(blocks):
    """block after block, each column-major: the packed array of include/gdca.h"""
    return np.concatenate([np.asarray(b, dtype=np.float64).ravel(order="F") for b in blocks]) if blocks else np.empty(0)


def unpack(E, offA, offB):
    out, at = [], 0
    for ka, kb in zip(np.diff(offA).tolist(), np.diff(offB).tolist()):
        out.append(E[at:at + ka * kb].reshape((ka, kb), order="F"))
        at += ka * kb
    assert at == E.size
    return out


def assign_scipy(C):
    """(match, total): match[a] = the column matched to row a, -1 if unmatched; min(kA, kB) pairs at minimum total"""
    from scipy.optimize import linear_sum_assignment

    C = np.asarray(C, dtype=np.float64)
    match = np.full(C.shape[0], -1, dtype=np.int64)
    if C.size == 0:
        return match, 0.0
    r, c = linear_sum_assignment(C)
    match[r] = c
    return match, float(C[r, c].sum())


def assign_brute(C):
    """the minimum total over every one-to-one assignment of min(kA, kB) pairs (at most 6 a side)"""
    C = np.asarray(C, dtype=np.float64)
    kA, kB = C.shape
    assert max(kA, kB) <= 6
    if C.size == 0:
        return 0.0
    if kA > kB:
        return assign_brute(C.T)
    rows = np.arange(kA)
    return min(float(C[rows, list(p)].sum()) for p in itertools.permutations(range(kB), kA))


def total_of(C, match):
    C, match = np.asarray(C), np.asarray(match)
    a = np.nonzero(match >= 0)[0]
    return float(C[a, match[a]].sum())


def is_valid_matching(C, match):
    """min(kA, kB) rows matched, to distinct columns inside the block"""
    kA, kB = np.asarray(C).shape
    m = np.asarray(match)
    used = m[m >= 0]
    return m.shape == (kA,) and np.all(m >= -1) and np.all(m < max(kB, 1)) and len(used) == min(kA, kB) and len(set(used.tolist())) == len(used)


def gap_of(C, match):
    C = np.asarray(C, dtype=np.float64)
    g = np.zeros(C.shape[0])
    for a, b in enumerate(np.asarray(match).tolist()):
        if b < 0:
            continue
        others = np.delete(C[a], b)
        g[a] = (others.min() if others.size else np.inf) - C[a, b]
    return g


def solver_bar(C):
    """4 k^3 u max|c| (the module's docstring)"""
    C = np.asarray(C, dtype=np.float64)
    if C.size == 0:
        return 0.0
    k = max(C.shape)
    return 4.0 * k ** 3 * em.U * float(np.abs(C).max())


def second_best_margin(C):
    """total of the best assignment that differs from the optimum, minus the optimum (+inf: there is no other).  A different
    assignment of the shorter side lacks at least one pair of the optimum: the minimum over the optimum's pairs of the optimum with
    that pair forbidden."""
    from scipy.optimize import linear_sum_assignment

    C = np.asarray(C, dtype=np.float64)
    match, best = assign_scipy(C)
    margin = np.inf
    for a in np.nonzero(match >= 0)[0]:
        D = C.copy()
        D[a, match[a]] = np.inf
        try:
            r, c = linear_sum_assignment(D)
        except ValueError:  # (infeasible: the forbidden pair was the only one)
            continue
        margin = min(margin, float(D[r, c].sum()) - best)
    return margin


def species_labels(sizes):
    return np.repeat(np.arange(len(sizes)), sizes)


def native_recovered(blocks_match):
    """native partners found: within a species of the held-out pairs the native partner of row a is column a"""
    return int(sum(int(np.sum(np.asarray(m) == np.arange(len(m)))) for m in blocks_match))
