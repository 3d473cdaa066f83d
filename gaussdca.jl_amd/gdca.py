"""gDCA(): host-side mirror of the reference's only entry point
(/root/reference/src/GaussDCA.jl:8-47), same keyword arguments, defaults, validation order and
messages (:49-65).  Everything between compute_weighted_frequencies (:28) and correct_APC (:42)
and compute_ranking (:44) is one call into libgdca.so (gdca_run_ranked): Z goes to the MI355X once,
the sorted ranking comes back; text output stays on the host as in the reference."""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Tuple

import numpy as np

from . import _lib
from ._lib import ArgumentError, default_context
from .dcautils import (FastaAlignment, Ranking, _block_views, _mut_what_arg, _walk_args, _sample_args, _temper_args, _mutations_arg, decode_double_code, _symbols, _theta_arg, _what_arg, read_fasta_alignment,
                       remove_duplicate_sequences, species_blocks)

last_stats = None  # stats of the most recent gDCA call (theta, threshold, Meff, device timings)
last_multi_stats = None  # gDCA_multi: one stats dict per setting of its most recent call, in the order of the settings


def _score_arg(score) -> int:
    s = str(score).lstrip(":")
    if s == "DI":
        return _lib.SCORE_DI
    if s == "frob":
        return _lib.SCORE_FROB
    raise ArgumentError(f"invalid score value: {score} (must be either :DI or :frob)")


def check_arguments(filename, pseudocount, theta, max_gap_fraction, score, min_separation) -> bool:
    """Same checks, same order, same messages as src/GaussDCA.jl:49-65."""
    if not (0 <= pseudocount <= 1):
        raise ArgumentError(f"invalid pseudocount value: {pseudocount} (must be between 0 and 1)")
    _theta_arg(theta)
    if not (0 <= max_gap_fraction <= 1):
        raise ArgumentError(f"invalid max_gap_fraction value: {max_gap_fraction} (must be between 0 and 1)")
    _score_arg(score)
    if not (min_separation >= 1):
        raise ArgumentError(f"invalid min_separation value: {min_separation} (must be >= 1)")
    if not os.path.isfile(filename):
        raise ArgumentError(f"cannot open file {filename}")
    return True


def gDCA(filename: str, pseudocount: float = 0.8, theta=":auto", max_gap_fraction: float = 0.9,
         score=":frob", min_separation: int = 5, remove_dups: bool = False, ctx=None,
         **kw) -> List[Tuple[int, int, float]]:
    """Gaussian DCA contact ranking of a FASTA alignment: [(i, j, score)], best first.

    Keyword ``θ`` is accepted as an alias of ``theta``; ``score`` may be ':frob'/'frob' or
    ':DI'/'DI'; ``theta`` may be ':auto'/'auto' or a number in [0, 1]."""
    global last_stats
    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA() got unexpected keyword arguments {sorted(kw)}")
    check_arguments(filename, pseudocount, theta, max_gap_fraction, score, min_separation)

    ctx = ctx or default_context()
    if remove_dups:
        Z = read_fasta_alignment(filename, max_gap_fraction)
        Z, _ = remove_duplicate_sequences(Z)
        q = int(Z.max())
        if q >= 32:
            raise RuntimeError(f"parameter q={q} is too big (max 31 is allowed)")
        Zf = np.asfortranarray(Z, dtype=np.int8)
        ii, jj, sc, last_stats = ctx.run_ranked_ptr(Zf.ctypes.data, Zf.shape[0], Zf.shape[1], q, float(pseudocount), _theta_arg(theta),
                                                    _score_arg(score), int(min_separation), apc=True)
    else:
        # the parsed matrix goes to gdca_run where the native reader left it (gdca_fasta_data), q = maximum(Z) comes from the
        # reader (gdca_fasta_max_symbol): no copy into an array of the host language, no second pass over Z
        with FastaAlignment(filename, max_gap_fraction) as fa:
            q = fa.q
            if q >= 32:
                raise RuntimeError(f"parameter q={q} is too big (max 31 is allowed)")
            ii, jj, sc, last_stats = ctx.run_ranked_ptr(fa.ptr, fa.N, fa.M, q, float(pseudocount), _theta_arg(theta), _score_arg(score),
                                                        int(min_separation), apc=True)
    if last_stats.get("refined", 0) < 0:
        import warnings

        warnings.warn("gDCA: the covariance is too ill-conditioned for the block sweep even with its refinement step "
                      f"(||inv(C)||_1 = {last_stats['inverse_norm1']:.3g}; pseudocount {pseudocount}): scores are unreliable",
                      RuntimeWarning, stacklevel=2)
    return Ranking(ii, jj, sc)


def _sequences_arg(seqs, name: str, dims: str):
    """The ``sequences`` / ``seqs_a`` / ``seqs_b`` conventions of the fused read-outs: an array of symbols, a string naming a FASTA
    file (read with ``max_gap_fraction = 1.0``: every record is kept) or None (the alignment's own) -> int8 column-major, or None."""
    if seqs is None:
        return None
    if isinstance(seqs, (str, bytes, os.PathLike)):
        if not os.path.isfile(seqs):
            raise ArgumentError(f"cannot open file {seqs}")
        return np.asfortranarray(read_fasta_alignment(os.fspath(seqs) if not isinstance(seqs, bytes) else seqs.decode(), 1.0), dtype=np.int8)
    return _symbols(seqs, name, dims)


def _ptr_count(X):
    """parsed sequences as the context calls take them: (pointer, count); (None, 0): the alignment's own"""
    return (None, 0) if X is None else (X.ctypes.data, X.shape[1])


def _check_whole_sequences(X, N):
    if X is not None and X.shape[0] != N:
        raise ArgumentError(f"sequences have {X.shape[0]} sites, the alignment has {N}")
    if X is not None and X.shape[1] < 1:
        raise ArgumentError("sequences holds no sequence")


def _fit_then_score(filename, pseudocount, max_gap_fraction, remove_dups, ctx, check, run, unreliable):
    """What the fused read-outs of the fitted model share (gDCA_energies, gDCA_pair_energies, gDCA_mutation_scan): the alignment with
    or without deduplication, the stats and the conditioning warning.  ``check(N)`` holds the entry's own arguments against the
    alignment, ``run(c, ptr, N, M, q)`` is the context call, ``unreliable`` names the result in the warning.  Called by the entry
    itself, after check_arguments: the warning points at the entry's caller."""
    global last_stats

    def _run(ptr, N, M, q):
        if q >= 32:
            raise RuntimeError(f"parameter q={q} is too big (max 31 is allowed)")
        check(N)
        return run(ctx or default_context(), ptr, N, M, q)

    if remove_dups:
        Z = read_fasta_alignment(filename, max_gap_fraction)
        Z, _ = remove_duplicate_sequences(Z)
        Zf = np.asfortranarray(Z, dtype=np.int8)
        out, last_stats = _run(Zf.ctypes.data, Zf.shape[0], Zf.shape[1], int(Z.max()))
    else:
        with FastaAlignment(filename, max_gap_fraction) as fa:
            out, last_stats = _run(fa.ptr, fa.N, fa.M, fa.q)
    if last_stats.get("refined", 0) < 0:
        import warnings

        warnings.warn("gDCA: the covariance is too ill-conditioned for the block sweep even with its refinement step "
                      f"(||inv(C)||_1 = {last_stats['inverse_norm1']:.3g}; pseudocount {pseudocount}): {unreliable} are unreliable",
                      RuntimeWarning, stacklevel=3)
    return out


def gDCA_energies(filename: str, sequences=None, pseudocount: float = 0.8, theta=":auto", max_gap_fraction: float = 0.9,
                  remove_dups: bool = False, ctx=None, **kw) -> np.ndarray:
    """Energies of sequences under the Gaussian model gDCA fits to the alignment in ``filename`` (same reading, reweighting,
    pseudocount, covariance and inverse; same validation and messages): E(x) = 1/2 (x - Pi)' mJ (x - Pi), minus the log-likelihood
    up to the model's constant.  Lower = fits the family better.

    ``sequences``: ``None`` scores the alignment's own sequences (after the gap filter and the optional deduplication); an
    ``(N, K)`` int8 array (symbols 1..q like ``Z``) scores its columns; a string names a second FASTA file, read with the same reader
    and ``max_gap_fraction = 1.0`` -- every record is kept, so the energies line up with the records.  Stats go to ``last_stats``."""
    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_energies() got unexpected keyword arguments {sorted(kw)}")
    check_arguments(filename, pseudocount, theta, max_gap_fraction, ":frob", 1)
    X = _sequences_arg(sequences, "sequences", "an N x K")
    return _fit_then_score(filename, pseudocount, max_gap_fraction, remove_dups, ctx, lambda N: _check_whole_sequences(X, N),
                           lambda c, ptr, N, M, q: c.run_energies_ptr(ptr, N, M, q, float(pseudocount), _theta_arg(theta), *_ptr_count(X)),
                           "energies")


def gDCA_loglik(filename: str, sequences=None, pseudocount: float = 0.8, theta=":auto", max_gap_fraction: float = 0.9,
                remove_dups: bool = False, ctx=None, **kw):
    """Log-likelihoods of sequences under the Gaussian model gDCA fits to the alignment in ``filename`` (the fit and the arguments
    are ``gDCA_energies``'): ``(L, logdet)`` with L[k] = log p(x_k) = -E(x_k) - 1/2 (n log 2 pi + log det C), the density of the
    continuous Gaussian N(Pi, C) at the one-hot point, and logdet = log det C from the pivots of the very inverse the model comes
    from.  Unlike the energies these are on one scale for every model: compare families, pseudocounts (a held-out likelihood) or
    the halves of a paired alignment with them.  Higher = fits better.  Stats go to ``last_stats``."""
    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_loglik() got unexpected keyword arguments {sorted(kw)}")
    check_arguments(filename, pseudocount, theta, max_gap_fraction, ":frob", 1)
    X = _sequences_arg(sequences, "sequences", "an N x K")

    def run(c, ptr, N, M, q):
        L, logdet, st = c.run_loglik_ptr(ptr, N, M, q, float(pseudocount), _theta_arg(theta), *_ptr_count(X))
        return (L, logdet), st

    return _fit_then_score(filename, pseudocount, max_gap_fraction, remove_dups, ctx, lambda N: _check_whole_sequences(X, N), run,
                           "log-likelihoods")


def _split_check(split, XA, XB):
    """check(N) of the entries that score pairings across a split: the split and the halves' sizes held against the alignment"""
    def check(N):
        if not isinstance(split, (int, np.integer)) or not 1 <= split <= N - 1:
            raise ArgumentError(f"invalid split value: {split} (must be between 1 and N - 1 = {N - 1})")
        if XA is not None and XA.shape[0] != split:
            raise ArgumentError(f"seqs_a have {XA.shape[0]} sites, protein A has {split}")
        if XB is not None and XB.shape[0] != N - split:
            raise ArgumentError(f"seqs_b have {XB.shape[0]} sites, protein B has {N - split}")
        if (XA is not None and XA.shape[1] < 1) or (XB is not None and XB.shape[1] < 1):
            raise ArgumentError("seqs_a or seqs_b holds no sequence")

    return check


def _species_half(ptr, N, M, X, perm, lo, hi, name):
    """one side's sequences sorted by species (sites lo .. hi - 1 of the alignment at ptr where X is None); None: the alignment's own
    already are"""
    count = M if X is None else X.shape[1]
    if len(perm) != count:
        raise ArgumentError(f"{name} has {len(perm)} labels for {count} sequences")
    if X is not None:
        return np.asfortranarray(X[:, perm])
    if np.array_equal(perm, np.arange(M)):
        return None
    Z = np.ctypeslib.as_array(C.cast(C.c_void_p(ptr), C.POINTER(C.c_int8)), shape=(M, N))  # (row k = sequence k)
    return np.asfortranarray(Z[perm, lo:hi].T)


def gDCA_pair_energies(filename: str, split: int, seqs_a=None, seqs_b=None, what="energy", pseudocount: float = 0.8, theta=":auto",
                       max_gap_fraction: float = 0.9, remove_dups: bool = False, ctx=None, **kw) -> np.ndarray:
    """Energies of every pairing across a split alignment under the Gaussian model gDCA fits to ``filename``, an alignment of
    concatenated pairs A (+) B whose first ``split`` sites are protein A (same reading, reweighting, pseudocount, covariance and
    inverse as gDCA; same validation and messages).  Returns the (K_A, K_B) matrix E[a, b] = the energy ``gDCA_energies`` gives the
    concatenation of sequence a of ``seqs_a`` with sequence b of ``seqs_b`` (``what="coupling"``: only the part R[a, b] that
    depends on the pairing).  Lower = the better pairing; row-wise minima are the matches partner matching starts from.

    ``seqs_a`` / ``seqs_b``: ``None`` takes that half of the alignment's own sequences (after the gap filter and the optional
    deduplication; both None: the diagonal holds the native pairs); a ``(split, K_A)`` / ``(N - split, K_B)`` int8 array (symbols
    1..q); or a string naming a FASTA file of that half alone, read with ``max_gap_fraction = 1.0`` so every record is kept.
    Stats go to ``last_stats``."""
    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_pair_energies() got unexpected keyword arguments {sorted(kw)}")
    check_arguments(filename, pseudocount, theta, max_gap_fraction, ":frob", 1)
    w = _what_arg(what)
    XA, XB = _sequences_arg(seqs_a, "seqs_a", "a sites x K"), _sequences_arg(seqs_b, "seqs_b", "a sites x K")

    check = _split_check(split, XA, XB)

    return _fit_then_score(filename, pseudocount, max_gap_fraction, remove_dups, ctx, check,
                           lambda c, ptr, N, M, q: c.run_pair_energies_ptr(ptr, N, M, q, float(pseudocount), _theta_arg(theta), int(split),
                                                                           *_ptr_count(XA), *_ptr_count(XB), w),
                           "energies")


def gDCA_partner_match(filename: str, split: int, seqs_a=None, seqs_b=None, species_a=None, species_b=None, what="energy",
                       pseudocount: float = 0.8, theta=":auto", max_gap_fraction: float = 0.9, remove_dups: bool = False, ctx=None,
                       return_blocks: bool = False, **kw):
    """Partner matching per species under the Gaussian model gDCA fits to ``filename`` (an alignment of concatenated pairs A (+) B,
    the first ``split`` sites protein A; the fit is ``gDCA_pair_energies``'): inside every species the sequences of A are matched one
    to one with those of B at minimum total energy (``what="coupling"``: total coupling) -- min(kA_s, kB_s) pairs a species, on the
    device, only the within-species pairings are ever computed.

    ``seqs_a`` / ``seqs_b`` as for ``gDCA_pair_energies``; ``species_a`` / ``species_b``: one integer label per sequence of that
    side, in any order.  ``None`` sequences take that half of the alignment's own sequences: the labels then go with the sequences
    the reader keeps (``max_gap_fraction = 1.0`` keeps every record).  Returns ``(match, gap)`` in the caller's order: ``match[a]``
    the index into ``seqs_b`` of a's partner, or -1 (its species has fewer sequences of B); ``gap[a]`` the least other energy of a
    with a sequence of B of its species minus the matched one (+inf: the only candidate; 0.0: unmatched; negative: the assignment
    overrode a's own best).  ``return_blocks=True`` adds the list of per-species energy matrices (``pair_energies_blocked``' form).
    At most 512 sequences a side in one species.  Stats go to ``last_stats``."""
    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_partner_match() got unexpected keyword arguments {sorted(kw)}")
    check_arguments(filename, pseudocount, theta, max_gap_fraction, ":frob", 1)
    w = _what_arg(what)
    XA, XB = _sequences_arg(seqs_a, "seqs_a", "a sites x K"), _sequences_arg(seqs_b, "seqs_b", "a sites x K")
    if species_a is None or species_b is None:
        raise ArgumentError("species_a and species_b are needed: one integer label per sequence")
    perm_a, perm_b, offA, offB, _ = species_blocks(species_a, species_b)

    check = _split_check(split, XA, XB)

    def run(c, ptr, N, M, q):
        XAs = _species_half(ptr, N, M, XA, perm_a, 0, int(split), "species_a")
        XBs = _species_half(ptr, N, M, XB, perm_b, int(split), N, "species_b")
        (E, m, g), st = c.run_partner_match_ptr(ptr, N, M, q, float(pseudocount), _theta_arg(theta), int(split), *_ptr_count(XAs),
                                                *_ptr_count(XBs), offA, offB, w, want_blocks=return_blocks)
        match, gap = np.empty_like(m), np.empty_like(g)
        match[perm_a] = np.where(m >= 0, perm_b[np.maximum(m, 0)], -1)
        gap[perm_a] = g
        return ((match, gap, _block_views(E, offA, offB)) if return_blocks else (match, gap)), st

    return _fit_then_score(filename, pseudocount, max_gap_fraction, remove_dups, ctx, check, run, "matches")


def gDCA_pair_logodds(filename: str, split: int, seqs_a=None, seqs_b=None, pseudocount: float = 0.8, theta=":auto",
                      max_gap_fraction: float = 0.9, remove_dups: bool = False, ctx=None, return_info: bool = False, **kw):
    """Log-odds of every pairing across a split alignment: L[a, b] = log p_AB(a (+) b) - log p_A(a) - log p_B(b), the joint Gaussian
    model gDCA fits to ``filename`` against the two proteins modelled on their own -- the TRUE marginals N(Pi_A, C_AA), N(Pi_B, C_BB)
    of that very fit (same weights, theta and pseudocount; two more inverses).  This is the method's partner score: where the joint
    energy of ``gDCA_pair_energies`` ranks a pairing largely by how typical a and b each are, the log-odds removes exactly that part.
    HIGHER = more likely partners.  Arguments as ``gDCA_pair_energies`` (without ``what``).  Returns the (K_A, K_B) matrix;
    ``return_info=True``: ``(L, info)`` with the three log dets, the mutual information I of the halves (the expected log-odds of a
    native pair), the marginal energies ``EmA`` / ``EmB`` and the marginal fits' ``refined``.  Stats of the joint fit go to
    ``last_stats``."""
    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_pair_logodds() got unexpected keyword arguments {sorted(kw)}")
    check_arguments(filename, pseudocount, theta, max_gap_fraction, ":frob", 1)
    XA, XB = _sequences_arg(seqs_a, "seqs_a", "a sites x K"), _sequences_arg(seqs_b, "seqs_b", "a sites x K")

    def run(c, ptr, N, M, q):
        (L, EmA, EmB, info), st = c.run_pair_logodds_ptr(ptr, N, M, q, float(pseudocount), _theta_arg(theta), int(split), *_ptr_count(XA),
                                                         *_ptr_count(XB))
        return ((L, dict(info, EmA=EmA, EmB=EmB)) if return_info else L), st

    return _fit_then_score(filename, pseudocount, max_gap_fraction, remove_dups, ctx, _split_check(split, XA, XB), run, "log-odds")


def gDCA_partner_logodds(filename: str, split: int, seqs_a=None, seqs_b=None, species_a=None, species_b=None, pseudocount: float = 0.8,
                         theta=":auto", max_gap_fraction: float = 0.9, remove_dups: bool = False, ctx=None, return_blocks: bool = False,
                         return_info: bool = False, **kw):
    """Partner matching per species on the log-odds of ``gDCA_pair_logodds``: inside every species the sequences of A are matched one
    to one with those of B at MAXIMUM total log-odds.  Arguments and the returned ``(match, gap)`` as ``gDCA_partner_match`` (without
    ``what``); ``gap[a]`` is the matched log-odds minus the greatest other one of a with a sequence of B of its species (+inf: the only
    candidate; 0.0: unmatched; negative: the assignment overrode a's own best).  ``return_blocks=True`` adds the per-species log-odds
    matrices, ``return_info=True`` the info dict (after them).  Stats of the joint fit go to ``last_stats``."""
    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_partner_logodds() got unexpected keyword arguments {sorted(kw)}")
    check_arguments(filename, pseudocount, theta, max_gap_fraction, ":frob", 1)
    XA, XB = _sequences_arg(seqs_a, "seqs_a", "a sites x K"), _sequences_arg(seqs_b, "seqs_b", "a sites x K")
    if species_a is None or species_b is None:
        raise ArgumentError("species_a and species_b are needed: one integer label per sequence")
    perm_a, perm_b, offA, offB, _ = species_blocks(species_a, species_b)

    def run(c, ptr, N, M, q):
        XAs = _species_half(ptr, N, M, XA, perm_a, 0, int(split), "species_a")
        XBs = _species_half(ptr, N, M, XB, perm_b, int(split), N, "species_b")
        (L, m, g, info), st = c.run_partner_logodds_ptr(ptr, N, M, q, float(pseudocount), _theta_arg(theta), int(split), *_ptr_count(XAs),
                                                        *_ptr_count(XBs), offA, offB, want_blocks=return_blocks)
        match, gap = np.empty_like(m), np.empty_like(g)
        match[perm_a] = np.where(m >= 0, perm_b[np.maximum(m, 0)], -1)
        gap[perm_a] = g
        out = (match, gap) + ((_block_views(L, offA, offB),) if return_blocks else ()) + ((info,) if return_info else ())
        return out, st

    return _fit_then_score(filename, pseudocount, max_gap_fraction, remove_dups, ctx, _split_check(split, XA, XB), run, "matches")


def gDCA_partner_ipa(seqs_a, seqs_b, species_a, species_b, known_pairs=None, seed="singletons", n_inc: int = 6, max_rounds: int = 50,
                     what="energy", pseudocount: float = 0.8, theta=":auto", max_gap_fraction: float = 0.9, q=None, ctx=None, **kw):
    """Iterative partner matching (progressive paralog matching / the iterative pairing algorithm) for two alignments without a
    trusted alignment of pairs: fit on the pairs trusted so far, match every species (``gDCA_partner_match``'s fit and assignment),
    keep the ``r * n_inc`` most confident matches of round r as the next training set, repeat -- on the device, the pools and the
    growing alignment resident from the first round to the last (``gdca_run_partner_ipa``).

    ``seqs_a`` / ``seqs_b``: the two sides, ``(sites, K)`` int8 arrays (symbols 1..q) or FASTA files (every record kept);
    ``species_a`` / ``species_b``: one integer label per sequence, in any order.  ``seed``: ``"singletons"`` -- the species with
    exactly one sequence on each side -- or a list of ``(a, b)`` index pairs (the caller's indices; a pair lies inside one species);
    it is the first training set and is replaced from round 1 on.  ``known_pairs``: an alignment file of concatenated pairs A (+) B
    (read as gDCA reads its input, ``max_gap_fraction``) that is part of every round's training alignment.  The loop ends after
    ``max_rounds`` rounds, or one round after the training set held every matched sequence.  ``q``: the alphabet (default: the
    largest symbol present).

    Returns ``(match, gap, rounds)``: match / gap of the last round in the caller's order, as ``gDCA_partner_match`` returns them;
    ``rounds``: one dict a round (``M_train, candidates, n_sel, n_changed, Meff, theta, logdet, cost, ms_*``).  The last fit's stats
    go to ``last_stats``."""
    global last_stats
    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_partner_ipa() got unexpected keyword arguments {sorted(kw)}")
    if not (isinstance(pseudocount, (int, float, np.integer, np.floating)) and 0 <= pseudocount <= 1):
        raise ArgumentError(f"invalid pseudocount value: {pseudocount} (must be between 0 and 1)")
    th, w = _theta_arg(theta), _what_arg(what)
    XA, XB = _sequences_arg(seqs_a, "seqs_a", "a sites x K"), _sequences_arg(seqs_b, "seqs_b", "a sites x K")
    if XA is None or XB is None or species_a is None or species_b is None:
        raise ArgumentError("seqs_a, seqs_b, species_a and species_b are all needed")
    if XA.shape[1] < 1 or XB.shape[1] < 1:
        raise ArgumentError("seqs_a or seqs_b holds no sequence")
    for k, name in ((n_inc, "n_inc"), (max_rounds, "max_rounds")):
        if not isinstance(k, (int, np.integer)) or k < 1:
            raise ArgumentError(f"invalid {name} value: {k} (must be an integer >= 1)")
    split, N = XA.shape[0], XA.shape[0] + XB.shape[0]
    perm_a, perm_b, offA, offB, _ = species_blocks(species_a, species_b)
    if len(perm_a) != XA.shape[1] or len(perm_b) != XB.shape[1]:
        raise ArgumentError(f"species_a / species_b have {len(perm_a)} / {len(perm_b)} labels for {XA.shape[1]} / {XB.shape[1]} sequences")
    Zfix = None
    if known_pairs is not None:
        if not os.path.isfile(known_pairs):
            raise ArgumentError(f"cannot open file {known_pairs}")
        Zfix = np.asfortranarray(read_fasta_alignment(os.fspath(known_pairs), max_gap_fraction), dtype=np.int8)
        if Zfix.shape[0] != N:
            raise ArgumentError(f"known_pairs has {Zfix.shape[0]} sites, the two sides have {N}")
    # the seed in the species-sorted order the library works in
    inv_a, inv_b = np.empty_like(perm_a), np.empty_like(perm_b)
    inv_a[perm_a], inv_b[perm_b] = np.arange(len(perm_a)), np.arange(len(perm_b))
    if isinstance(seed, str):
        if seed.lstrip(":") != "singletons":
            raise ArgumentError(f"invalid seed value: {seed} (must be singletons or a list of index pairs)")
        one = np.nonzero((np.diff(offA) == 1) & (np.diff(offB) == 1))[0]
        seedA, seedB = offA[one].astype(np.int32), offB[one].astype(np.int32)
    else:
        pairs = np.asarray(seed if seed is not None else [], dtype=np.int64).reshape(-1, 2)
        if pairs.size and (pairs.min() < 0 or pairs[:, 0].max() >= len(perm_a) or pairs[:, 1].max() >= len(perm_b)):
            raise ArgumentError("a seed index is outside its side")
        seedA, seedB = inv_a[pairs[:, 0]].astype(np.int32), inv_b[pairs[:, 1]].astype(np.int32)
    if len(seedA) + (0 if Zfix is None else Zfix.shape[1]) < 1:
        raise ArgumentError("nothing to fit the first round on: no seed pair and no known_pairs")
    qq = int(q) if q is not None else int(max(XA.max(), XB.max(), 0 if Zfix is None else Zfix.max()))
    if qq >= 32:
        raise RuntimeError(f"parameter q={qq} is too big (max 31 is allowed)")
    XAs, XBs = np.asfortranarray(XA[:, perm_a]), np.asfortranarray(XB[:, perm_b])
    c = ctx or default_context()
    (m, g, _, _), rounds, last_stats = c.run_partner_ipa_ptr(XAs.ctypes.data, XAs.shape[1], XBs.ctypes.data, XBs.shape[1], offA, offB, N, qq, split,
                                                             float(pseudocount), th, None if Zfix is None else Zfix.ctypes.data,
                                                             0 if Zfix is None else Zfix.shape[1], seedA, seedB, int(n_inc), int(max_rounds), w)
    match, gap = np.empty_like(m), np.empty_like(g)
    match[perm_a] = np.where(m >= 0, perm_b[np.maximum(m, 0)], -1)
    gap[perm_a] = g
    return match, gap, rounds


def gDCA_mutation_scan(filename: str, sequences=None, what="delta", pseudocount: float = 0.8, theta=":auto", max_gap_fraction: float = 0.9,
                       remove_dups: bool = False, ctx=None, **kw) -> np.ndarray:
    """The mutational landscape of sequences under the Gaussian model gDCA fits to the alignment in ``filename`` (same reading,
    reweighting, pseudocount, covariance and inverse; same validation and messages): a ``(K, N, q)`` array D with D[k, i, b - 1] the
    energy change, in the sense of ``gDCA_energies``, of setting site i of sequence k to symbol b (``what="delta"``: exactly 0 at the
    sequence's own symbol, b = q deletes the residue; negative = the mutant fits the family better), or the site potentials V the
    changes are differences of (``what="potential"``).

    ``sequences`` as for ``gDCA_energies``: ``None`` scans the alignment's own sequences (after the gap filter and the optional
    deduplication); an ``(N, K)`` int8 array (symbols 1..q like ``Z``) scans its columns; a string names a second FASTA file, read
    with ``max_gap_fraction = 1.0`` so every record is kept.  Stats go to ``last_stats``."""
    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_mutation_scan() got unexpected keyword arguments {sorted(kw)}")
    check_arguments(filename, pseudocount, theta, max_gap_fraction, ":frob", 1)
    w = _mut_what_arg(what)
    X = _sequences_arg(sequences, "sequences", "an N x K")
    return _fit_then_score(filename, pseudocount, max_gap_fraction, remove_dups, ctx, lambda N: _check_whole_sequences(X, N),
                           lambda c, ptr, N, M, q: c.run_mutation_scan_ptr(ptr, N, M, q, float(pseudocount), _theta_arg(theta),
                                                                           *_ptr_count(X), w),
                           "energy changes")


def gDCA_greedy_walk(filename: str, sequences=None, max_steps=None, min_gain: float = 0.0, mask=None, gap_target: bool = False,
                     fill_gaps: bool = False, path: bool = False, table: bool = False, pseudocount: float = 0.8, theta=":auto",
                     max_gap_fraction: float = 0.9, remove_dups: bool = False, ctx=None, **kw):
    """Greedy walks under the Gaussian model gDCA fits to the alignment in ``filename`` (the fit and its arguments are
    ``gDCA_mutation_scan``'s): every sequence takes the single substitution that lowers its energy most, again and again, until none
    lowers it by more than ``min_gain`` or ``max_steps`` (default min(4 N, 65535)) steps are done.  The walk's arguments and what is
    returned -- ``(Xout, steps, dE_sum[, path, dE_path][, V])`` -- are ``dcautils.greedy_walk``'s.

    ``sequences`` as for ``gDCA_energies``: ``None`` walks the alignment's own sequences (after the gap filter and the optional
    deduplication); an ``(N, K)`` int8 array (symbols 1..q like ``Z``) walks its columns; a string names a second FASTA file, read
    with ``max_gap_fraction = 1.0`` so every record is kept.  Stats go to ``last_stats``."""
    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_greedy_walk() got unexpected keyword arguments {sorted(kw)}")
    check_arguments(filename, pseudocount, theta, max_gap_fraction, ":frob", 1)
    X = _sequences_arg(sequences, "sequences", "an N x K")

    def run(c, ptr, N, M, q):
        T, mg, m, flags = _walk_args(N, max_steps, min_gain, mask, gap_target, fill_gaps)
        return c.run_greedy_walk_ptr(ptr, N, M, q, float(pseudocount), _theta_arg(theta), *_ptr_count(X), mask=m, flags=flags, min_gain=mg,
                                     max_steps=T, path=path, table=table)

    return _fit_then_score(filename, pseudocount, max_gap_fraction, remove_dups, ctx, lambda N: _check_whole_sequences(X, N), run,
                           "walks")


def gDCA_sample(filename: str, starts=None, beta: float = 1.0, burn=None, stride=None, n_samples: int = 1, seed: int = 0, stream0: int = 0,
                mask=None, gaps: bool = False, trace: bool = False, pseudocount: float = 0.8, theta=":auto", max_gap_fraction: float = 0.9,
                remove_dups: bool = False, ctx=None, **kw):
    """Sequences drawn from the Gaussian model gDCA fits to the alignment in ``filename`` (the fit and its arguments are
    ``gDCA_mutation_scan``'s): one Metropolis chain starts from each sequence of ``starts`` and samples exp(-beta E(x)) / Z.  A
    proposal picks a site and another symbol for it, both uniformly, and is accepted iff ``beta * dE <= -log(u)`` with dE its energy
    change and u uniform in (0, 1].  ONE SWEEP IS N PROPOSALS: a chain runs ``burn`` proposals (default 10 N), then returns its state
    after every ``stride`` (default N) more, ``n_samples`` times.  ``mask``, ``gaps``, ``seed``, ``stream0`` as ``dcautils.sample``.

    ``starts`` as ``sequences`` for ``gDCA_energies``: ``None`` starts a chain from each of the alignment's own sequences (after the
    gap filter and the optional deduplication); an ``(N, K)`` int8 array (symbols 1..q like ``Z``) from its columns; a string names a
    second FASTA file, read with ``max_gap_fraction = 1.0`` so every record is kept.

    Returns ``(Xs (N, n_samples, K) int8, dE_s (K, n_samples), accepted (K,))``; with ``trace=True`` also ``thr, moves`` (K, n_steps)
    each.  ``Xs.reshape(N, -1, order="F")`` is an alignment (N x n_samples K, chain by chain) that can be handed to ``gDCA_energies`` or
    ``compute_weighted_frequencies`` as it lies; ``dE_s`` is each sample's energy minus its start's.  Stats go to ``last_stats``."""
    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_sample() got unexpected keyword arguments {sorted(kw)}")
    check_arguments(filename, pseudocount, theta, max_gap_fraction, ":frob", 1)
    X = _sequences_arg(starts, "starts", "an N x K")

    def run(c, ptr, N, M, q):
        b, bu, sd, S, sd0, st0, m, flags = _sample_args(N, q, beta, burn, stride, n_samples, seed, stream0, mask, gaps)
        return c.run_sample_ptr(ptr, N, M, q, float(pseudocount), _theta_arg(theta), *_ptr_count(X), mask=m, flags=flags, beta=b, seed=sd0,
                                stream0=st0, burn=bu, stride=sd, n_samples=S, trace=trace)

    return _fit_then_score(filename, pseudocount, max_gap_fraction, remove_dups, ctx, lambda N: _check_whole_sequences(X, N), run,
                           "samples")


def gDCA_sample_tempered(filename: str, starts=None, betas=(1.0,), swap_every=None, burn: int = 10, stride: int = 1, n_samples: int = 1,
                         seed: int = 0, stream0: int = 0, mask=None, gaps: bool = False, pseudocount: float = 0.8, theta=":auto",
                         max_gap_fraction: float = 0.9, remove_dups: bool = False, ctx=None, **kw):
    """Sequences drawn from the Gaussian model gDCA fits to the alignment in ``filename`` by replica-exchange (parallel tempering)
    Metropolis chains (the fit and its arguments are ``gDCA_mutation_scan``'s, ``starts`` is ``gDCA_sample``'s).  Every chain runs
    R = len(betas) replicas from its start sequence; a replica is a chain of ``gDCA_sample`` on a stream of its own at ``betas[slot]``
    of the slot it holds (a proposal is accepted iff ``beta * dE <= -log(u)``), and after every ``swap_every`` proposals (default N) the
    holders a, b of neighbouring slots p, p + 1 (p % 2 == round % 2) exchange slots iff ``(betas[p] - betas[p + 1]) * (E_b - E_a) <=
    -log(u)``; ``betas[0]`` is the target temperature and only its holder is sampled.  ``burn`` and ``stride`` are IN SWEEPS (one
    sweep is N proposals); ``swap_every`` in proposals must divide a sweep's multiples ``burn N`` and ``stride N``.

    Returns ``(Xs (N, n_samples, K) int8, E_s (K, n_samples), accepted (K, R), swaps (K, R - 1))``: the samples, their energies, the
    accepted proposals by slot and the accepted swaps by pair (a pair is attempted every other round).  Stats go to ``last_stats``."""
    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_sample_tempered() got unexpected keyword arguments {sorted(kw)}")
    check_arguments(filename, pseudocount, theta, max_gap_fraction, ":frob", 1)
    X = _sequences_arg(starts, "starts", "an N x K")
    for v, name, lo in ((burn, "burn", 0), (stride, "stride", 1)):
        if not isinstance(v, (int, np.integer)) or v < lo:
            raise ArgumentError(f"invalid {name} value: {v} (must be an integer >= {lo}, in sweeps)")

    def run(c, ptr, N, M, q):
        _, bu, sd, S, sd0, st0, m, flags = _sample_args(N, q, 1.0, int(burn) * N, int(stride) * N, n_samples, seed, stream0, mask, gaps)
        b, every = _temper_args(N, betas, swap_every, bu, sd)
        out, st = c.run_sample_tempered_ptr(ptr, N, M, q, float(pseudocount), _theta_arg(theta), *_ptr_count(X), betas=b, mask=m, flags=flags,
                                            seed=sd0, stream0=st0, swap_every=every, burn=bu, stride=sd, n_samples=S)
        return out[:4], st

    return _fit_then_score(filename, pseudocount, max_gap_fraction, remove_dups, ctx, lambda N: _check_whole_sequences(X, N), run,
                           "samples")


def gDCA_bm(filename: str, n_iter: int, K: int = 1024, eta: float = 1.0, lam: float = 0.0, target_pseudocount: float = 0.0,
            init: str = "gaussian", burn=None, stride=None, n_samples: int = 1, beta: float = 1.0, seed: int = 0, gaps: bool = True,
            scores: bool = False, min_separation: int = 5, pseudocount: float = 0.8, theta=":auto", max_gap_fraction: float = 0.9,
            remove_dups: bool = False, ctx=None, betas=None, swap_every=None, plm_iter: int = 100, plm_lam: float = 0.01, **kw):
    """Boltzmann-machine refinement (bmDCA) of the model gDCA fits to the alignment in ``filename``: the Potts model the Metropolis
    chains of ``gDCA_sample`` draw from is moved until the one- and two-site frequencies of its samples are the family's.  Built from
    the device operators like ``gDCA_stepwise``: weights, frequencies, pseudocount, covariance, inverse -- the Gaussian warm start at
    ``pseudocount`` (``init="gaussian"``; ``"independent"``: the independent-site model, no inverse; ``"plm"``: the independent-site
    model after ``plm_iter`` pseudo-likelihood iterations with the penalty ``plm_lam``, ``gDCA_plm``'s loop) --, then ``n_iter`` iterations of
    sample, tally, update (``devops.bm_learn_dev``: nothing crosses to the host inside the loop) towards the family's frequencies at
    ``target_pseudocount``.  ``K`` persistent chains start from the first K sequences of the alignment (fewer if it has fewer);
    ONE SWEEP IS N PROPOSALS: every iteration runs ``burn`` proposals (default 10 N) and tallies ``n_samples`` states ``stride`` (default
    N) apart; ``eta`` is the step, ``lam`` an L2 penalty on the couplings; ``gaps`` (default True) lets the chains change gaps.

    Returns ``(W, trace)``: W (n, n) is the model as the pair (W, zeros) that ``sequence_energies``, ``mutation_scan``,
    ``greedy_walk``, ``sample``, ``compute_FN`` take in the place of (mJ, Pi); ``trace`` (n_iter, 4) holds max |Pi_m - Pi_d|,
    max |c_m - c_d|, the Pearson correlation of the connected correlations and the acceptance rate per iteration.  With
    ``scores=True`` a third entry: the ranking of APC(FN(W)) at ``min_separation``, the bmDCA contact score.

    ``betas`` (default None: the plain chains at ``beta``): a ladder of inverse temperatures, the target first -- every chain becomes
    R = len(betas) replicas that swap neighbouring temperatures every ``swap_every`` proposals (default N) as in
    ``gDCA_sample_tempered``, the samples of the target temperature are tallied, and the loop is driven from Python over the operator
    forms (``devops.bm_learn_tempered_dev``).  ``trace[:, 3]`` is then the acceptance at the target temperature, and the accepted
    fraction of every pair's swaps per iteration, (n_iter, R - 1), comes back as a third entry (before the ranking)."""
    from . import devops

    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_bm() got unexpected keyword arguments {sorted(kw)}")
    check_arguments(filename, pseudocount, theta, max_gap_fraction, ":frob", min_separation)
    if not (0 <= target_pseudocount <= 1):
        raise ArgumentError(f"invalid target_pseudocount value: {target_pseudocount} (must be between 0 and 1)")
    if init not in ("gaussian", "independent", "plm"):
        raise ArgumentError(f"invalid init value: {init} (must be \"gaussian\", \"independent\" or \"plm\")")
    if not isinstance(n_iter, (int, np.integer)) or n_iter < 1:
        raise ArgumentError(f"invalid n_iter value: {n_iter} (must be an integer >= 1)")
    if not isinstance(K, (int, np.integer)) or K < 1:
        raise ArgumentError(f"invalid K value: {K} (must be an integer >= 1)")
    Z = read_fasta_alignment(filename, max_gap_fraction)
    if remove_dups:
        Z, _ = remove_duplicate_sequences(Z)
    q = int(Z.max())
    if q >= 32:
        raise RuntimeError(f"parameter q={q} is too big (max 31 is allowed)")
    if betas is not None:
        N = Z.shape[0]
        betas, swap_every = _temper_args(N, betas, swap_every, 10 * N if burn is None else int(burn), N if stride is None else int(stride))
    out = devops.bm_fit(Z, q, int(n_iter), K=min(int(K), Z.shape[1]), eta=eta, lam=lam, pseudocount=float(pseudocount),
                        target_pseudocount=float(target_pseudocount), theta=theta, init=init, burn=burn, stride=stride,
                        n_samples=n_samples, beta=beta, seed=seed, gaps=gaps, scores=scores, ctx=ctx, betas=betas, swap_every=swap_every,
                        plm_iter=plm_iter, plm_lam=plm_lam)
    if scores:
        from .dcautils import compute_ranking

        return out[:-1] + (compute_ranking(out[-1], int(min_separation)),)
    return out


def gDCA_plm(filename: str, n_iter: int, lam: float = 0.01, eta=None, init: str = "independent", adapt: bool = False,
             scores: bool = False, target_pseudocount: float = 0.0, min_separation: int = 5, pseudocount: float = 0.8, theta=":auto",
             max_gap_fraction: float = 0.9, remove_dups: bool = False, ctx=None, **kw):
    """Pseudo-likelihood fit (plmDCA) of a Potts model to the alignment in ``filename``: gradient ascent on the reweighted log
    pseudo-likelihood (1 / Meff) sum_k w_k sum_i log P(x_ki | the rest of sequence k) minus ``lam`` times the squared couplings, with
    no sampler -- the conditionals are the softmax of ``mutation_scan``'s site potentials, their tally against the alignment is the
    model's side of the gradient (``devops.plm_learn_dev``: nothing crosses to the host inside the loop).  Built from the device
    operators like ``gDCA_bm``: weights, frequencies, the start at ``pseudocount`` (``init="independent"``: the independent-site
    model; ``"gaussian"``: the Gaussian fit read as a Potts model), then ``n_iter`` iterations towards the family's frequencies at
    ``target_pseudocount`` (0: the true ones, the exact gradient).

    ``eta=None`` selects 1 / (N + 2 lam), the step at which the penalised objective cannot rise in exact arithmetic.
    ``adapt=True`` drives the loop from Python (``devops.plm_learn_adaptive_dev``) with this deterministic rule: every iteration
    evaluates f = nll + lam sum_{i<j} |W_ij|^2 at the current W; where f fell below the last accepted value eta grows by 1.2, where
    it is equal eta stays, and the step is taken; where f rose W is restored from a device copy and eta is halved, so no step size is
    kept after a rise.

    Returns ``(W, trace)``: W (n, n) is the model as the pair (W, zeros) every read-out takes in the place of (mJ, Pi); ``trace``
    (n_iter, 4) holds max |Pi_c - Pi_d|, max |c_c - c_d|, the Pearson correlation of the connected correlations and nll, each at the
    W the iteration started from.  With ``scores=True`` a third entry: the ranking of APC(FN(W)) at ``min_separation``, the plmDCA
    contact score."""
    from . import devops

    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_plm() got unexpected keyword arguments {sorted(kw)}")
    check_arguments(filename, pseudocount, theta, max_gap_fraction, ":frob", min_separation)
    if not (0 <= target_pseudocount <= 1):
        raise ArgumentError(f"invalid target_pseudocount value: {target_pseudocount} (must be between 0 and 1)")
    if init not in ("gaussian", "independent"):
        raise ArgumentError(f"invalid init value: {init} (must be \"gaussian\" or \"independent\")")
    if not isinstance(n_iter, (int, np.integer)) or n_iter < 1:
        raise ArgumentError(f"invalid n_iter value: {n_iter} (must be an integer >= 1)")
    Z = read_fasta_alignment(filename, max_gap_fraction)
    if remove_dups:
        Z, _ = remove_duplicate_sequences(Z)
    q = int(Z.max())
    if q >= 32:
        raise RuntimeError(f"parameter q={q} is too big (max 31 is allowed)")
    out = devops.plm_fit(Z, q, int(n_iter), lam=lam, eta=eta, init=init, adapt=bool(adapt), pseudocount=float(pseudocount),
                         target_pseudocount=float(target_pseudocount), theta=theta, scores=scores, ctx=ctx)
    if scores:
        from .dcautils import compute_ranking

        return out[0], out[1], compute_ranking(out[2], int(min_separation))
    return out


def _required_sequences(sequences, name):
    X = _sequences_arg(sequences, "sequences", "an N x K")
    if X is None:
        raise ArgumentError(f"{name}() needs sequences: the alignment's own are not scanned (N^2 M outputs)")
    return X


def gDCA_double_mutant_scan(filename: str, sequences, pseudocount: float = 0.8, theta=":auto", max_gap_fraction: float = 0.9,
                            remove_dups: bool = False, ctx=None, **kw):
    """The double-mutant landscape of sequences under the Gaussian model gDCA fits to the alignment in ``filename`` (the fit and its
    arguments are ``gDCA_mutation_scan``'s): ``(ddE_min, sub_i, sub_j, epistasis)``, each (K, N, N) and indexed [k, i, j], as
    ``dcautils.double_mutant_scan`` returns them -- the lowest energy change over the true double substitutions of every site pair, the
    two symbols that reach it, and the pair's epistasis strength in that sequence.

    ``sequences``: an ``(N, K)`` int8 array (symbols 1..q like ``Z``) or a string naming a FASTA file (read with
    ``max_gap_fraction = 1.0``); required.  Stats go to ``last_stats``."""
    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_double_mutant_scan() got unexpected keyword arguments {sorted(kw)}")
    check_arguments(filename, pseudocount, theta, max_gap_fraction, ":frob", 1)
    X = _required_sequences(sequences, "gDCA_double_mutant_scan")
    qbox = []

    def run(c, ptr, N, M, q):
        qbox.append(q)
        return c.run_double_mutant_scan_ptr(ptr, N, M, q, float(pseudocount), _theta_arg(theta), *_ptr_count(X))

    Emin, code, epi = _fit_then_score(filename, pseudocount, max_gap_fraction, remove_dups, ctx, lambda N: _check_whole_sequences(X, N), run,
                                      "energy changes")
    sub_i, sub_j = decode_double_code(code.transpose(0, 2, 1), qbox[0])
    return Emin, sub_i, sub_j, epi


def gDCA_double_mutants(filename: str, sequences, mutations, pseudocount: float = 0.8, theta=":auto", max_gap_fraction: float = 0.9,
                        remove_dups: bool = False, ctx=None, **kw) -> np.ndarray:
    """The energy change of listed double mutants under the Gaussian model gDCA fits to the alignment in ``filename``: ``mutations``
    is an (L, 5) integer array of records (k, i, b, j, c) as ``dcautils.double_mutant_energies`` takes them, ``sequences`` as for
    ``gDCA_double_mutant_scan``.  Returns L energy changes -- what one holds against an experimental double-mutant library.  Stats go
    to ``last_stats``."""
    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_double_mutants() got unexpected keyword arguments {sorted(kw)}")
    check_arguments(filename, pseudocount, theta, max_gap_fraction, ":frob", 1)
    X = _required_sequences(sequences, "gDCA_double_mutants")
    m = _mutations_arg(mutations)
    return _fit_then_score(filename, pseudocount, max_gap_fraction, remove_dups, ctx, lambda N: _check_whole_sequences(X, N),
                           lambda c, ptr, N, M, q: c.run_double_mutants_ptr(ptr, N, M, q, float(pseudocount), _theta_arg(theta),
                                                                            *_ptr_count(X), m.ctypes.data, m.shape[0]),
                           "energy changes")


def _setting(s):
    """(pseudocount, score) or {"pseudocount": .., "score": ..} -> (pseudocount, score)"""
    if isinstance(s, dict):
        unknown = set(s) - {"pseudocount", "score"}
        if unknown:
            raise ArgumentError(f"invalid setting keys: {sorted(unknown)} (a setting has a pseudocount and a score)")
        return s.get("pseudocount", 0.8), s.get("score", ":frob")
    try:
        pc, score = s
    except (TypeError, ValueError):
        raise ArgumentError(f"invalid setting: {s!r} (must be a (pseudocount, score) pair)") from None
    return pc, score


def gDCA_multi(filename: str, settings, theta=":auto", max_gap_fraction: float = 0.9, min_separation: int = 5,
               remove_dups: bool = False, ctx=None, **kw) -> List[Ranking]:
    """gDCA of one alignment under several (pseudocount, score) settings in one pass: [Ranking], one per setting, in order.

    ``settings``: a sequence of ``(pseudocount, score)`` pairs or of dicts with those keys, e.g. the reference's two standard
    rankings ``[(0.8, ":frob"), (0.2, ":DI")]`` or a scan of the pseudocount.  Every ranking is the one ``gDCA`` returns for that
    setting with the other arguments given here; the alignment is read, reweighted and tallied once (gdca_run_ranked_multi), and
    settings with the same pseudocount share one inverse.  At most 16 settings a call.  Keyword ``θ`` is an alias of ``theta``.
    Per-setting stats go to ``last_multi_stats``."""
    global last_multi_stats
    if "θ" in kw:
        theta = kw.pop("θ")
    if kw:
        raise TypeError(f"gDCA_multi() got unexpected keyword arguments {sorted(kw)}")
    try:
        settings = [_setting(s) for s in settings]
    except TypeError:
        raise ArgumentError(f"invalid settings: {settings!r} (must be a sequence of (pseudocount, score) pairs)") from None
    if not 1 <= len(settings) <= _lib.MULTI_MAX:
        raise ArgumentError(f"invalid number of settings: {len(settings)} (must be between 1 and {_lib.MULTI_MAX})")
    for pc, score in settings:
        check_arguments(filename, pc, theta, max_gap_fraction, score, min_separation)
    prm = [(float(pc), _score_arg(score)) for pc, score in settings]

    ctx = ctx or default_context()
    if remove_dups:
        Z = read_fasta_alignment(filename, max_gap_fraction)
        Z, _ = remove_duplicate_sequences(Z)
        q = int(Z.max())
        if q >= 32:
            raise RuntimeError(f"parameter q={q} is too big (max 31 is allowed)")
        Zf = np.asfortranarray(Z, dtype=np.int8)
        out = ctx.run_ranked_multi_ptr(Zf.ctypes.data, Zf.shape[0], Zf.shape[1], q, prm, _theta_arg(theta), int(min_separation), apc=True)
    else:
        with FastaAlignment(filename, max_gap_fraction) as fa:
            q = fa.q
            if q >= 32:
                raise RuntimeError(f"parameter q={q} is too big (max 31 is allowed)")
            out = ctx.run_ranked_multi_ptr(fa.ptr, fa.N, fa.M, q, prm, _theta_arg(theta), int(min_separation), apc=True)
    last_multi_stats = [st for _, _, _, st in out]
    for (pc, _), st in zip(settings, last_multi_stats):
        if st.get("refined", 0) < 0:
            import warnings

            warnings.warn("gDCA: the covariance is too ill-conditioned for the block sweep even with its refinement step "
                          f"(||inv(C)||_1 = {st['inverse_norm1']:.3g}; pseudocount {pc}): scores are unreliable",
                          RuntimeWarning, stacklevel=2)
    return [Ranking(ii, jj, sc) for ii, jj, sc, _ in out]
