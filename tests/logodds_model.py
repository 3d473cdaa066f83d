"""The pair log-odds in numpy (the checker of tests/test_logodds_cpu.py and tests/test_gpu_logodds.py; include/gdca.h, "pair log-odds").

    L(a, b) = log p_AB(a (+) b) - log p_A(a) - log p_B(b) = ((EmA[a] + EmB[b]) - E[a, b]) + I
    I       = -1/2 ((log det C - log det C_AA) - log det C_BB)

p_AB = N(Pi, C) of the oracle's fit, p_A = N(Pi_A, C_AA) and p_B = N(Pi_B, C_BB) its TRUE marginals: C_AA and C_BB are the diagonal
blocks of that very C (the same weights, theta, Meff and pseudocount), their precisions inv(C_AA) and inv(C_BB) -- not the diagonal
blocks of inv(C).  n log 2 pi cancels.  Every part comes from a model this directory already has:

    EmA, EmB   energy_model.energies_gather (longdouble) under (inv(C_AA), Pi_A) and (inv(C_BB), Pi_B), with their sums B of absolute terms;
    E          pair_energy_model.pair_energy under (inv(C), Pi);
    log dets   logdet_model.Reference (longdouble Cholesky) of C, C_AA, C_BB.

The bar of an entry is the sum of the bars the project already derives for its parts -- no new constant:

    bar(a, b) = order_bound(split, q, BmA[a]) + order_bound(N - split, q, BmB[b]) + pair_energy's bound[a, b]
              + 0.5 (bar_ld + bar_ldA + bar_ldB) + 4 u (|EmA| + |EmB| + |E| + |I|)

(the last term: the three combining operations and the host's I, one rounding each on a magnitude of at most the sum of the four).

The golden record tests/golden/logodds_family.json is written by

    python tests/logodds_model.py --write-golden
"""
import json
import os
import sys

import numpy as np

import energy_model as em
import logdet_model as lm
import pair_energy_model as pm
import partner_model as ptm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "logodds_family.json")
GOLDEN_COMMAND = "python tests/logodds_model.py --write-golden"


class Model:
    """The three Gaussian models of one oracle fit and what the bar needs of them.  Zo: (M, N) alignment.
    reference_logdets=False (the operator form's shapes, where I is an INPUT and a longdouble factorisation of n = 3630 would take
    minutes): the log dets are numpy's f64 values and the bar carries no log-det term -- a tighter bar, never a wider one."""

    def __init__(self, Zo, q, pseudocount, split, theta="auto", reference_logdets=True):
        from oracle import gdca_oracle as o

        Zo = np.ascontiguousarray(Zo)
        self.q, self.split, self.N = int(q), int(split), Zo.shape[1]
        s = self.q - 1
        self.nA = self.split * s
        Pi_true, Pij_true, self.Meff, _ = o.compute_weighted_frequencies(Zo, self.q, theta)
        self.Pi, Pij = o.add_pseudocount(Pi_true, Pij_true, float(pseudocount), self.q)
        self.C = o.compute_C(self.Pi, Pij)
        nA = self.nA
        self.CA, self.CB = np.ascontiguousarray(self.C[:nA, :nA]), np.ascontiguousarray(self.C[nA:, nA:])
        self.mJ, self.mJA, self.mJB = o.spd_inverse(self.C), o.spd_inverse(self.CA), o.spd_inverse(self.CB)
        self.PiA, self.PiB = self.Pi[:nA], self.Pi[nA:]
        if not reference_logdets:
            self.ld, self.ldA, self.ldB = lm.logdet_numpy(self.C), lm.logdet_numpy(self.CA), lm.logdet_numpy(self.CB)
            self.I, self.bar_I = information_f64(self.ld, self.ldA, self.ldB), 0.0
            return
        self.ref, self.refA, self.refB = lm.Reference(self.C), lm.Reference(self.CA), lm.Reference(self.CB)
        self.ld, self.ldA, self.ldB = self.ref.logdet, self.refA.logdet, self.refB.logdet
        # I from the longdouble sums, rounded once; the device forms it in f64 from its three f64 log dets
        self.I = float(np.longdouble(-0.5) * ((self.ref.logdet_ld - self.refA.logdet_ld) - self.refB.logdet_ld))
        self.bar_I = 0.5 * (self.ref.bar + self.refA.bar + self.refB.bar)

    def parts(self, XA, XB):
        """-> dict: EmA, EmB, E (joint), L, bar, and the bars of the parts"""
        q = self.q
        EmA, BmA, _ = em.energies_gather(self.mJA, self.PiA, XA, q)
        EmB, BmB, _ = em.energies_gather(self.mJB, self.PiB, XB, q)
        E, boundE, _, _, _ = pm.pair_energy(self.mJ, self.Pi, XA, XB, q)
        L = ((EmA[:, None] + EmB[None, :]) - E) + self.I
        barA = em.order_bound(self.split, q, BmA)
        barB = em.order_bound(self.N - self.split, q, BmB)
        mag = np.abs(EmA)[:, None] + np.abs(EmB)[None, :] + np.abs(E) + abs(self.I)
        bar = barA[:, None] + barB[None, :] + boundE + self.bar_I + 4.0 * em.U * mag
        return dict(EmA=EmA, EmB=EmB, E=E, L=L, bar=bar, barA=barA, barB=barB, boundE=boundE, mag=mag)


def information_f64(ld, ldA, ldB):
    """I exactly as the library forms it on the host: plain f64, two subtractions and one multiplication"""
    return float(np.float64(-0.5) * ((np.float64(ld) - np.float64(ldA)) - np.float64(ldB)))


def combine_f64(EmA, EmB, E, I):
    """L exactly as the gather's epilogue forms it: ((EmA[a] + EmB[b]) - E[a, b]) + I in f64"""
    return ((np.asarray(EmA)[:, None] + np.asarray(EmB)[None, :]) - np.asarray(E)) + np.float64(I)


def swapped(Zo, split):
    """the alignment with its halves swapped: B's sites first (split' = N - split)"""
    Zo = np.asarray(Zo)
    return np.ascontiguousarray(np.concatenate([Zo[:, split:], Zo[:, :split]], axis=1))


# ---- the recorded illustration: 640 x 52, q = 21, fit on the first 600 rows, 40 pairs held out ----------------------------------------------
FAMILY = dict(seed=7, M=640, N=52, q=21, fit=600, split=26, pseudocount=0.5)
SPECIES_SIZES = (1, 2, 5, 8, 24)  # the 40 held-out pairs cut into species
# The held-out pairs are dealt to the species in the order of default_rng(SPECIES_SEED).permutation(40).  In their own order (and
# under seeds 1, 5, 6) the species of 24 is NOT decided on the CPU: held-out pairs 32 and 37 have the same A half, so where both fall
# into one species two assignments tie exactly (second-best margin 0.0).  Seed 2 is the first that puts them into different species;
# every species' margin then exceeds twice its bar, which the golden records.
SPECIES_SEED = 2


def family_alignment():
    from gdca_testutil import random_msa

    f = FAMILY
    Z = random_msa(np.random.default_rng(f["seed"]), f["M"], f["N"], q=f["q"])
    return Z[:f["fit"]], Z[f["fit"]:]


_family = {}


def family_model(pseudocount=None):
    """(Model, XA, XB, parts) of the illustration, computed once per run of the suite"""
    pc = FAMILY["pseudocount"] if pseudocount is None else pseudocount
    if pc not in _family:
        Zfit, Zheld = family_alignment()
        split = FAMILY["split"]
        m = Model(Zfit, FAMILY["q"], pc, split)
        Zheld = Zheld[np.random.default_rng(SPECIES_SEED).permutation(Zheld.shape[0])]
        XA, XB = np.asfortranarray(Zheld[:, :split].T), np.asfortranarray(Zheld[:, split:].T)
        _family[pc] = (m, XA, XB, m.parts(XA, XB))
    return _family[pc]


def species_bar(bar_block):
    """what the total of ANY assignment inside a species can differ by between two L matrices that agree within `bar`: every row
    contributes one entry, so at most the sum over the rows of the row's largest bar"""
    return float(np.asarray(bar_block).max(axis=1).sum()) if np.asarray(bar_block).size else 0.0


def family_record():
    """what tests/golden/logodds_family.json holds, computed by the model"""
    m, XA, XB, p = family_model()
    K = XA.shape[1]
    E, L, bar = p["E"], p["L"], p["bar"]
    nat = np.arange(K)
    srt = np.sort(L, axis=1)
    row_margin = srt[:, -1] - srt[:, -2]  # best minus second best of every row
    off = ptm.offsets(SPECIES_SIZES)
    species = []
    for s in range(len(SPECIES_SIZES)):
        blk = slice(off[s], off[s + 1])
        Ls, bs = L[blk, blk], bar[blk, blk]
        match, _ = ptm.assign_scipy(-Ls)
        margin = ptm.second_best_margin(-Ls)
        need = 2.0 * species_bar(bs) + ptm.solver_bar(Ls)
        species.append(dict(size=int(SPECIES_SIZES[s]), natives=int(np.sum(match == np.arange(len(match)))),
                            margin=float(margin) if np.isfinite(margin) else None, twice_bar=need,
                            decided=bool(margin > need)))
    nonnat = ~np.eye(K, dtype=bool)
    return dict(
        command=GOLDEN_COMMAND,
        family=dict(FAMILY, species_sizes=list(SPECIES_SIZES), species_seed=SPECIES_SEED),
        native_fraction_E=float((E.argmin(axis=1) == nat).mean()),
        native_fraction_L=float((L.argmax(axis=1) == nat).mean()),
        information=m.I,
        logdet=[m.ld, m.ldA, m.ldB],
        mean_L_native=float(np.diag(L).mean()),
        mean_L_nonnative=float(L[nonnat].mean()),
        max_bar=float(bar.max()),
        min_row_margin_over_bar=float((row_margin / bar.max(axis=1)).min()),
        species=species,
        natives_by_assignment=int(sum(sp["natives"] for sp in species)),
    )


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1:] == ["--write-golden"]:
        rec = family_record()
        with open(GOLDEN, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(rec, indent=1, sort_keys=True))
    else:
        sys.exit("usage: " + GOLDEN_COMMAND)
